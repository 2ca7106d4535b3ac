// SPH interpolation at points (grace_interpolate_points_f4 / grace_interpolate_grid_f4): the field
//   A(p) = sum over spheres i containing p of fl(w_i W(|p - x_i|, H_i))
// summed per channel in the class order of the column densities, and the number of spheres that
// contain p.  An extension the reference lacks; the arithmetic is stated in include/grace_hip.h.
//
// One wave owns a PACKET of 64 points: a brick of lattice points (8 x 8 x 1 for a slice, 4 x 4 x 4
// for a volume; positions formed in registers), or 64 consecutive points of a Morton order of the
// caller's points (keys against the tree's root box, read on the device; sorted by the library's
// own sort in the call's workspace) that lie in one Morton cell of ~256 points on average: a packet
// of 64 consecutive sorted points may straddle a jump of the curve and span half the scene, and the
// wave that owns it then tests every sphere in that box against all its lanes (10^6 random points
// in bench.py's scene: 99 ms with such packets, most of it the tail of a few straddling waves).
// Packets start every 64 sorted points and wherever the cell changes (a scan on the device; the
// grid is launched for the upper bound n / 64 + cells, surplus waves exit).
//
// The packet's box is reduced across the wave, and the wave walks the ALBVH against it with
// packet_walk.hpp's stack and cluster sweep: left child first, so leaves (pushed as node indices)
// come in ascending primitive order.  The cull tests each candidate's box against the packet's box
// (conservatively: the boxes are widened by 2^-20 of their bounds, far more than the half ulp by
// which fl(x - H) can move inward); the survivors go into LDS as {x, y, z, H^2}, {1/H, 1/H^3} and
// the walk's <= 4 weights, and every lane then runs the survivor list in ascending order against
// its own point.  A cluster never straddles a granule of 1024 primitives, so a round is one
// summation class: the running sum of the current class stays in VGPRs and is swapped with a
// per-class LDS slot when the class changes -- each class sum is the fp32 sum in ascending index
// order -- and the epilogue adds the 8 class sums pairwise.
//
// Containment d2 < fl(H^2) with d2 formed in fp32 is never true for a point outside the exact box
// [x - H, x + H] of a sphere (|dx| >= H there, and every fp32 step is monotonic), so the widened
// box tests drop no contained sphere: results are a function of the point and the scene only.
//
// Periodic boxes (interpolate_kernel over Periodic<InterpArgs>, grace_interpolate_points_periodic_f4 /
// grace_interpolate_grid_periodic_f4; packet_walk.hpp's WalkPeriod: per axis the period L and
// h = fl(0.5 L), an open axis L = 0 and h = +inf).  The separation is range_walk.hpp's: per component
// d0 = fl(p - x); d0 > h: dw = fl(d0 - L); else d0 < -h: dw = fl(d0 + L); else dw = d0.  A sphere with
// H > h on a periodic axis is off (more than one of its images could contain a point); every other
// sphere is tested once per point, with the wrapped d2.
//   The cull, wrapped.  Let d2 < fl(H H) for an on sphere.  fp32 squaring and the sums are monotonic,
// so |dw| < H on every axis.  Not wrapped: dw = fl(p - x), so the exact |p - x| < H (H is a float)
// and p is inside [x - H, x + H], as in the open walk.  d0 > h: beyond 2 L, fl(d0 - L) >= L >= 2 H,
// impossible; up to 2 L the subtraction is exact (Sterbenz), so d0 is in (L - H, L + H), below 1.5 L,
// and the exact p - x is within 1.5 L 2^-24 (1 + 2^-23) < 2^-23 L of d0: the exact box [x - H, x + H]
// meets [p - L - 2^-23 L, p - L + 2^-23 L].  d0 < -h mirrors this about p + L.  That slack is absolute
// in L and may exceed a small H, so the packet's box is that of its points moved out by
// e = L 2^-22 (exact) and then, like a query box, by 2^-20 of each bound, which covers the rounding
// of plo - e, phi + e; its images at -L and +L are rounded outward once more (axis_images).  A
// candidate's box fl(x -+ H) and the node boxes, which hold them, are moved out by 2^-20 of their
// bounds as in the open walk and must meet, per axis, the box or one of its two images.  So no
// sphere with wrapped d2 < fl(H H) is culled; what passes through an image it does not belong to
// fails the containment test.
//   Two wave-uniform fast paths.  A packet whose shifted boxes miss the root's box (moved out like
// every node box, so it holds every candidate's box) tests against the box itself.  And per axis
// the centres x with bhi - h <= x <= blo + h (both bounds moved inward by 2^-20, far more than their
// rounding) have |p - x| <= h exactly for every p in [blo, bhi], hence |fl(p - x)| <= h and no wrap:
// a cluster whose survivors all lie there on every axis runs the open loop, with the same bits.
// Bricks and Morton cells are narrow against h, so this is the common case.
//
// Gradients (gradient_kernel, grace_interpolate_gradient_points_f4 / _grid_f4 and their periodic forms):
// the same walk (interp_walk<..., GRAD = true>) -- packets, cull, staging, class swap, wrap -- with four
// running sums per channel, {d/dx, d/dy, d/dz, value}: per contained hit one more divide (1 / r), the
// unit vector fl(d_k / r), G = fl(f'(q) H^-4) (kernel_df, 1/H^4 staged beside 1/H and 1/H^3) and three
// selected products per channel; at d2 == 0 the select gives +0.  GRAD_CHANNELS channels per walk
// (DESIGN.md section 4 has the measurement behind the choice).  The value sum is the field kernel's
// operation sequence, so the optional value output is the field call's, bit for bit.
#include "packet_walk.hpp"
#include "sph_kernel_f.hpp"

using namespace grace_hip;

namespace {

constexpr int IP_CHANNELS = 4;     // channels per walk

// points entry point: PacketPoints.  Grid entry point (points == nullptr): p(i, j, k) = org + i u + j v + k w
struct InterpArgs : PacketPoints, PacketScene {
    float org[3], eu[3], ev[3], ew[3];
    int dims[3];
    int brick[3];          // lattice points per packet along i, j, k
    int nb[2];             // packets along i, j
    int n_packets;
    const float* weights;  // this walk's first channel; sphere i's channel c at weights[i w_stride + c]
    int w_stride;
    float* out;            // point p's channel c at out[p out_stride + c]
    int out_stride;
    int* counts;           // or null
    float* grad;           // gradient walks: point p's channel c, component k at grad[(p grad_stride + c) 3 + k]
    int grad_stride;
    unsigned long long* tests;   // measurement hook: survivor tests (lanes x survivors), or null
};

// The packet's point box on one axis of a periodic box, moved out by L 2^-22 and by 2^-20 of its bounds,
// with its images at -L and +L (wave-uniform).
__device__ __forceinline__ AxisImages point_images(const float plo, const float phi, const float L)
{
    float lo, hi, unused;
    query_bounds(plo, L * 0.25f * PW_SLACK, true, lo, unused);
    query_bounds(phi, L * 0.25f * PW_SLACK, true, unused, hi);
    return axis_images(uniform(lo), uniform(hi), L);
}

// [lo, hi] moved out by 2^-20 of each bound meets the box or one of its images.
__device__ __forceinline__ bool meets_widened(const AxisImages& b, const float lo, const float hi)
{
    return b.meets(lo - fabsf(lo) * PW_SLACK, hi + fabsf(hi) * PW_SLACK);
}

// The centres that no point of [blo, bhi] wraps against: [bhi - h, blo + h], moved inward (open axis: all).
struct NoWrap {
    float lo, hi;
    __device__ __forceinline__ bool holds(const float x) const { return x >= lo && x <= hi; }
};
__device__ __forceinline__ NoWrap no_wrap(const AxisImages& b, const float h)
{
    const float l = b.hi - h, u = b.lo + h;
    const bool open = !(h < __int_as_float(0x7f800000));
    return { open ? __int_as_float(0xff800000) : uniform(l + fabsf(l) * PW_SLACK),
             open ? __int_as_float(0x7f800000) : uniform(u - fabsf(u) * PW_SLACK) };
}

// The walk of both kernels below.  NW = channels of this walk (0: counts only).  GRAD: every channel
// carries four running sums {d/dx, d/dy, d/dz, value} (grace_hip.h, "SPH gradients at points") instead
// of the value alone; sum c * NA + k of the lane is acc[c * NA + k].  Args: InterpArgs, or
// Periodic<InterpArgs> for the periodic walk.
template <int KIND, int NW, bool GRAD, typename Args>
__device__ __forceinline__ void interp_walk(const Args& a)
{
    constexpr bool PERIODIC = is_periodic<Args>::value;
    constexpr int NA = GRAD ? 4 : 1;                     // running sums per channel
    constexpr int NS = NW > 0 ? NW * NA : 1;             // running sums per lane
    constexpr int NC = NW > 0 ? NW : 1;
    static_assert(!GRAD || NW > 0, "a gradient walk has channels");
    __shared__ float4 s_rec[PW_WAVES][64];               // survivors: {x, y, z, H^2}
    __shared__ float2 s_inv[PW_WAVES][NW > 0 ? 64 : 1];  // {1/H, 1/H^3}
    __shared__ float s_ih4[PW_WAVES][GRAD ? 64 : 1];     // 1/H^4
    __shared__ float s_w[PW_WAVES][NW > 0 ? 64 : 1][NC]; // weights
    __shared__ float s_cls[PW_WAVES][NW > 0 ? 8 : 1][NS][64];   // class sums, per lane

    const PacketWave w = packet_wave();
    const int lane = w.lane, wv = w.wv, packet = w.packet;
    if (packet >= a.n_packets) return;                   // (wave-uniform)

    // ---- the packet's points ----
    float px, py, pz;
    bool active;
    size_t slot;                                         // output index of this lane's point
    if (a.points) {
        if (packet >= int(*a.n_starts)) return;          // (wave-uniform)
        const PacketPoint pt = load_point(a, packet, lane);
        active = pt.in_range;
        slot = pt.src;
        px = pt.px; py = pt.py; pz = pt.pz;
    } else {
        const int bi = packet % a.nb[0], bj = (packet / a.nb[0]) % a.nb[1], bk = packet / (a.nb[0] * a.nb[1]);
        const int li = lane % a.brick[0], lj = (lane / a.brick[0]) % a.brick[1], lk = lane / (a.brick[0] * a.brick[1]);
        const int i = bi * a.brick[0] + li, j = bj * a.brick[1] + lj, k = bk * a.brick[2] + lk;
        active = i < a.dims[0] && j < a.dims[1] && k < a.dims[2];
        slot = (size_t(k) * a.dims[1] + j) * a.dims[0] + i;
        const float fi = float(i), fj = float(j), fk = float(k);
        px = ((a.org[0] + fi * a.eu[0]) + fj * a.ev[0]) + fk * a.ew[0];
        py = ((a.org[1] + fi * a.eu[1]) + fj * a.ev[1]) + fk * a.ew[1];
        pz = ((a.org[2] + fi * a.eu[2]) + fj * a.ev[2]) + fk * a.ew[2];
    }
    if (!active) px = py = pz = __int_as_float(0x7fc00000);   // NaN: outside every box and sphere
    // (fminf / fmaxf skip NaN points; a packet of NaN points keeps +inf / -inf and culls everything)
    const float plo_x = wave_min(px), phi_x = wave_max(px);
    const float plo_y = wave_min(py), phi_y = wave_max(py);
    const float plo_z = wave_min(pz), phi_z = wave_max(pz);
    // periodic: the box's images, the centres no point wraps against, whether any image meets the root's box
    AxisImages bx = {}, by = {}, bz = {};
    NoWrap nx = {}, ny = {}, nz = {};
    bool images = true, plain = true;
    float hx = 0.0f, hy = 0.0f, hz = 0.0f;
    if constexpr (PERIODIC) {
        hx = a.per.h[0]; hy = a.per.h[1]; hz = a.per.h[2];
        bx = point_images(plo_x, phi_x, a.per.L[0]);
        by = point_images(plo_y, phi_y, a.per.L[1]);
        bz = point_images(plo_z, phi_z, a.per.L[2]);
        nx = no_wrap(bx, hx); ny = no_wrap(by, hy); nz = no_wrap(bz, hz);
        const int rt = *a.root;
        if (rt >= 0 && rt < a.n_nodes) {                  // (the root's box: the union of its children's)
            const float4* np = a.nodes + 4 * size_t(rt);
            const float4 L = np[1], R = np[2], Z = np[3];
            const float dlo_x = fminf(L.x, R.x), dhi_x = fmaxf(L.y, R.y), dlo_y = fminf(L.z, R.z), dhi_y = fmaxf(L.w, R.w);
            const float dlo_z = fminf(Z.x, Z.z), dhi_z = fmaxf(Z.y, Z.w);
            images = overlaps_widened(dlo_x, dhi_x, bx.mlo, bx.mhi) || overlaps_widened(dlo_x, dhi_x, bx.plo, bx.phi)
                || overlaps_widened(dlo_y, dhi_y, by.mlo, by.mhi) || overlaps_widened(dlo_y, dhi_y, by.plo, by.phi)
                || overlaps_widened(dlo_z, dhi_z, bz.mlo, bz.mhi) || overlaps_widened(dlo_z, dhi_z, bz.plo, bz.phi);
            images = __builtin_amdgcn_readfirstlane(int(images)) != 0;
        }
    }

    // ---- class sums ----
    float acc[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) acc[c] = 0.0f;
    if constexpr (NW > 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int c = 0; c < NS; ++c) s_cls[wv][k][c][lane] = 0.0f;
    }
    int cur = 0;                                         // class of acc (wave-uniform)
    int count = 0;
    unsigned long long tests = 0;

    PacketStack stack;
    auto push = [&](const int idx) { stack.push(lane, idx); };
    push(*a.root);

    while (!stack.empty()) {
        const int idx = stack.pop();
        if (idx < a.n_nodes) {
            const float4* np = a.nodes + 4 * size_t(idx);
            const float4 n0 = np[0], L = np[1], R = np[2], Z = np[3];
            bool hit_l, hit_r;
            if constexpr (PERIODIC) {
                if (images) {
                    hit_l = meets_widened(bx, L.x, L.y) && meets_widened(by, L.z, L.w) && meets_widened(bz, Z.x, Z.y);
                    hit_r = meets_widened(bx, R.x, R.y) && meets_widened(by, R.z, R.w) && meets_widened(bz, Z.z, Z.w);
                } else {
                    hit_l = overlaps_widened(L.x, L.y, bx.lo, bx.hi) && overlaps_widened(L.z, L.w, by.lo, by.hi)
                        && overlaps_widened(Z.x, Z.y, bz.lo, bz.hi);
                    hit_r = overlaps_widened(R.x, R.y, bx.lo, bx.hi) && overlaps_widened(R.z, R.w, by.lo, by.hi)
                        && overlaps_widened(Z.z, Z.w, bz.lo, bz.hi);
                }
            } else {
                hit_l = overlaps_widened(L.x, L.y, plo_x, phi_x) && overlaps_widened(L.z, L.w, plo_y, phi_y)
                    && overlaps_widened(Z.x, Z.y, plo_z, phi_z);
                hit_r = overlaps_widened(R.x, R.y, plo_x, phi_x) && overlaps_widened(R.z, R.w, plo_y, phi_y)
                    && overlaps_widened(Z.z, Z.w, plo_z, phi_z);
            }
            if (hit_r) push(__float_as_int(n0.y));
            if (hit_l) push(__float_as_int(n0.x));       // popped first: ascending primitive order
            continue;
        }
        const int4 lf = a.leaves[idx - a.n_nodes];
        sweep_clusters(a.spheres, lf.x, lf.x + lf.y, lane,
            [&](const bool in, const float4& s) {
                if constexpr (PERIODIC) {
                    // a sphere above half a period is off (NaN H: no box test is true)
                    const bool on = in && !(s.w > hx || s.w > hy || s.w > hz);
                    const bool kept = on && (images
                        ? meets_widened(bx, s.x - s.w, s.x + s.w) && meets_widened(by, s.y - s.w, s.y + s.w)
                            && meets_widened(bz, s.z - s.w, s.z + s.w)
                        : overlaps_widened(s.x - s.w, s.x + s.w, bx.lo, bx.hi)
                            && overlaps_widened(s.y - s.w, s.y + s.w, by.lo, by.hi)
                            && overlaps_widened(s.z - s.w, s.z + s.w, bz.lo, bz.hi));
                    const bool wraps = kept && !(nx.holds(s.x) && ny.holds(s.y) && nz.holds(s.z));
                    plain = __builtin_amdgcn_ballot_w64(wraps) == 0ull;
                    return kept;
                } else {
                    return in && overlaps_widened(s.x - s.w, s.x + s.w, plo_x, phi_x)
                        && overlaps_widened(s.y - s.w, s.y + s.w, plo_y, phi_y)
                        && overlaps_widened(s.z - s.w, s.z + s.w, plo_z, phi_z);
                }
            },
            [&](const int pos, const float4& s, const int j) {
                s_rec[wv][pos] = make_float4(s.x, s.y, s.z, s.w * s.w);
                if constexpr (NW > 0) {
                    const float ih = 1.0f / s.w;
                    s_inv[wv][pos] = make_float2(ih, (ih * ih) * ih);
                    if constexpr (GRAD) s_ih4[wv][pos] = (ih * ih) * (ih * ih);
#pragma unroll
                    for (int c = 0; c < NW; ++c) s_w[wv][pos][c] = a.weights[size_t(j) * a.w_stride + c];
                }
            },
            [&](const int cl, const int n_surv) {
                if constexpr (NW > 0) {
                    // the lane's own slots: the swap needs no order against the staging
                    const int cls = (cl >> (GRANULE_SHIFT - 6)) & (SUM_CLASSES - 1);
                    if (cls != cur) {
#pragma unroll
                        for (int c = 0; c < NS; ++c) {
                            s_cls[wv][cur][c][lane] = acc[c];
                            acc[c] = s_cls[wv][cls][c][lane];
                        }
                        cur = cls;
                    }
                }
                tests += uint64_t(n_surv);
                for (int j = 0; j < n_surv; ++j) {
                    const float4 r = s_rec[wv][j];
                    float dx = px - r.x, dy = py - r.y, dz = pz - r.z;
                    if constexpr (PERIODIC) {
                        if (!plain) {                              // (wave-uniform)
                            dx = wrap_sep(dx, a.per.L[0], hx);
                            dy = wrap_sep(dy, a.per.L[1], hy);
                            dz = wrap_sep(dz, a.per.L[2], hz);
                        }
                    }
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < r.w) {
                        ++count;
                        if constexpr (GRAD) {
                            const float2 inv = s_inv[wv][j];
                            const float r = sqrt_rn(d2);
                            const float q = r * inv.x;
                            const float W = kernel_f<KIND>(q) * inv.y;
                            const float G = kernel_df<KIND>(q) * s_ih4[wv][j];
                            const float ir = 1.0f / r;
                            const float ux = dx * ir, uy = dy * ir, uz = dz * ir;
                            const bool off = d2 > 0.0f;              // at the centre: +0, not 0 * inf
#pragma unroll
                            for (int c = 0; c < NW; ++c) {
                                const float wc = s_w[wv][j][c], wG = wc * G;
                                acc[c * NA + 0] = acc[c * NA + 0] + (off ? wG * ux : 0.0f);
                                acc[c * NA + 1] = acc[c * NA + 1] + (off ? wG * uy : 0.0f);
                                acc[c * NA + 2] = acc[c * NA + 2] + (off ? wG * uz : 0.0f);
                                acc[c * NA + 3] = acc[c * NA + 3] + wc * W;
                            }
                        } else if constexpr (NW > 0) {
                            const float2 inv = s_inv[wv][j];
                            const float W = kernel_f<KIND>(sqrt_rn(d2) * inv.x) * inv.y;
#pragma unroll
                            for (int c = 0; c < NW; ++c) acc[c] = acc[c] + s_w[wv][j][c] * W;
                        }
                    }
                }
            });
    }

    stack.report(lane, a.status);
    const unsigned long long n_active = __builtin_popcountll(__builtin_amdgcn_ballot_w64(active));
    if (a.tests && lane == 0) atomicAdd(a.tests, tests * n_active);
    if (!active) return;
    if (a.counts) a.counts[slot] = count;
    if constexpr (NW > 0) {
#pragma unroll
        for (int c = 0; c < NS; ++c) s_cls[wv][cur][c][lane] = acc[c];
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            float t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = s_cls[wv][k][c][lane];
            const float s01 = t[0] + t[1], s23 = t[2] + t[3], s45 = t[4] + t[5], s67 = t[6] + t[7];
            const float sum = (s01 + s23) + (s45 + s67);
            if constexpr (GRAD) {
                if (c % NA < 3) a.grad[(slot * a.grad_stride + c / NA) * 3 + c % NA] = sum;
                else if (a.out) a.out[slot * a.out_stride + c / NA] = sum;
            } else {
                a.out[slot * a.out_stride + c] = sum;
            }
        }
    }
}

template <int KIND, int NW, typename Args>
__global__ __launch_bounds__(PW_BLOCK) void interpolate_kernel(const Args a)
{
    interp_walk<KIND, NW, false>(a);
}

// NG = gradient channels of this walk.
template <int KIND, int NG, typename Args>
__global__ __launch_bounds__(PW_BLOCK) void gradient_kernel(const Args a)
{
    interp_walk<KIND, NG, true>(a);
}

// grace_gradient_div_curl_f32: row p of g[n][3][3] is g_ck = d_k A_c.
__global__ __launch_bounds__(256) void div_curl_kernel(const float* __restrict__ g, const int n,
                                                       float* __restrict__ div, float* __restrict__ curl)
{
    const int p = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (p >= n) return;
    float m[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) m[e] = g[size_t(p) * 9 + e];
    if (div) div[p] = (m[0] + m[4]) + m[8];
    if (curl) {
        curl[size_t(p) * 3 + 0] = m[7] - m[5];           // g_zy - g_yz
        curl[size_t(p) * 3 + 1] = m[2] - m[6];           // g_xz - g_zx
        curl[size_t(p) * 3 + 2] = m[3] - m[1];           // g_yx - g_xy
    }
}

// Process-wide measurement hook (grace_interpolate_enable_stats): a device counter of survivor tests.
unsigned long long* g_tests = nullptr;
bool g_stats = false;

template <typename Args>
grace_status launch_walk(const Args& a, int kind, int nw, hipStream_t stream)
{
    const int blocks = ceil_div(size_t(a.n_packets), PW_WAVES);
    if (nw == 0) {
        interpolate_kernel<GRACE_SPH_KERNEL_CUBIC, 0, Args><<<blocks, PW_BLOCK, 0, stream>>>(a);
    } else {
        with_kernel(kind, nw, [&](auto k, auto n) {
            interpolate_kernel<decltype(k)::value, decltype(n)::value, Args><<<blocks, PW_BLOCK, 0, stream>>>(a);
        });
    }
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

// Gradient channels per walk: GRAD_CHANNELS unless the measurement hook says otherwise
// (grace_interpolate_gradient_channels_per_walk).
constexpr int GRAD_CHANNELS = 2, GRAD_CHANNELS_MAX = 2;
int g_grad_channels = GRAD_CHANNELS;

template <typename Args>
grace_status launch_gradient_walk(const Args& a, int kind, int ng, hipStream_t stream)
{
    const int blocks = ceil_div(size_t(a.n_packets), PW_WAVES);
    with_kernel(kind, ng, [&](auto k, auto n) {
        if constexpr (decltype(n)::value <= GRAD_CHANNELS_MAX)
            gradient_kernel<decltype(k)::value, decltype(n)::value, Args><<<blocks, PW_BLOCK, 0, stream>>>(a);
    });
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

// Checks shared by both entry points, and the scene / output fields of the arguments.  d_grad: the
// gradient calls' (they need it, and weights); null for the field calls.
grace_status interp_common(InterpArgs& a, const float* d_spheres, size_t n_spheres, const int* d_nodes,
                           size_t n_nodes, const int* d_leaves, const int* d_root, const float* d_weights,
                           int n_channels, float* d_out, int* d_counts, TraceState** ts_out,
                           bool gradient = false, float* d_grad = nullptr)
{
    PACKET_SCENE(a, "interpolate", false, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root);
    if (gradient) GRACE_REQUIRE(d_grad, "interpolate_gradient: null gradient output");
    else GRACE_REQUIRE(d_out || d_counts, "interpolate: no output");
    if (d_out || gradient) {
        GRACE_REQUIRE(n_channels >= 1 && n_channels <= 64, "interpolate: channels must be 1..64");
        GRACE_REQUIRE(d_weights, "interpolate: null weights");
    }
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    GRACE_REQUIRE(ts->sph_kernel >= GRACE_SPH_KERNEL_CUBIC && ts->sph_kernel <= GRACE_SPH_KERNEL_WENDLAND_C6,
                  "interpolate: a custom SPH kernel table has no kernel function f(q)");
    a.w_stride = n_channels;
    a.out_stride = n_channels;
    a.grad_stride = n_channels;
    *ts_out = ts;
    return GRACE_OK;
}

// The measurement hook's counter, zeroed for this call.
grace_status interp_hook(InterpArgs& a, hipStream_t stream)
{
    if (g_stats && g_tests) {
        GRACE_TRY_HIP(hipMemsetAsync(g_tests, 0, sizeof(unsigned long long), stream));
        a.tests = g_tests;
    }
    return GRACE_OK;
}

// The walks of one call: channels four at a time, counts with the first walk.  A gradient call
// (d_grad): g_grad_channels at a time, each walk with its channels' values (d_out, or null).
template <typename Args>
grace_status interp_walks(Args a, int kind, const float* d_weights, int n_channels, float* d_out,
                          int* d_counts, hipStream_t stream, float* d_grad = nullptr)
{
    if (d_grad) {
        for (int g = 0; g < n_channels; g += g_grad_channels) {
            a.weights = d_weights + g;
            a.grad = d_grad + 3 * size_t(g);
            a.out = d_out ? d_out + g : nullptr;
            a.counts = g == 0 ? d_counts : nullptr;
            GRACE_TRY(launch_gradient_walk(a, kind, min(g_grad_channels, n_channels - g), stream));
        }
        return GRACE_OK;
    }
    if (!d_out) {
        a.counts = d_counts;
        return launch_walk(a, kind, 0, stream);
    }
    for (int g = 0; g < n_channels; g += IP_CHANNELS) {
        a.weights = d_weights + g;
        a.out = d_out + g;
        a.counts = g == 0 ? d_counts : nullptr;
        GRACE_TRY(launch_walk(a, kind, min(IP_CHANNELS, n_channels - g), stream));
    }
    return GRACE_OK;
}

// grace_interpolate_points_f4, grace_interpolate_gradient_points_f4 (gradient: d_out is its d_value) and
// their periodic forms: `a` is zero but for a period.
template <typename Args>
grace_status interpolate_points(Args a, const float* d_points, size_t n_points, int elems_per_point,
                                const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                size_t n_nodes, const int* d_leaves, const int* d_root,
                                const float* d_weights, int n_channels,
                                float* d_out, int* d_counts, grace_stream stream,
                                bool gradient = false, float* d_grad = nullptr)
{
    GRACE_REQUIRE(elems_per_point >= 3 && elems_per_point <= 16, "interpolate: elements per point must be 3..16");
    GRACE_REQUIRE(n_points < (size_t(1) << 31), "interpolate: too many points");
    if (n_points == 0) return GRACE_OK;   // (before the output checks: a caller's empty arrays may be null)
    GRACE_REQUIRE(d_points, "interpolate: null points");
    TraceState* ts = nullptr;
    GRACE_TRY(interp_common(a, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, d_weights, n_channels,
                            d_out, d_counts, &ts, gradient, d_grad));
    const hipStream_t stream_ = as_stream(stream);
    GRACE_TRY(interp_hook(a, stream_));
    return packet_run(a, *ts, d_points, n_points, elems_per_point, stream_,
                      [&](Args w, size_t max_packets) -> grace_status {
        w.n_packets = int(max_packets);
        return interp_walks(w, ts->sph_kernel, d_weights, n_channels, d_out, d_counts, stream_, d_grad);
    });
}

// grace_interpolate_grid_f4, grace_interpolate_gradient_grid_f4 and their periodic forms.
template <typename Args>
grace_status interpolate_grid(Args a, const float* h_origin3, const float* h_uvw9, const int* h_dims3,
                              const float* d_spheres, size_t n_spheres, const int* d_nodes,
                              size_t n_nodes, const int* d_leaves, const int* d_root,
                              const float* d_weights, int n_channels,
                              float* d_out, int* d_counts, grace_stream stream,
                              bool gradient = false, float* d_grad = nullptr)
{
    GRACE_REQUIRE(h_origin3 && h_uvw9 && h_dims3, "interpolate_grid: null lattice argument");
    GRACE_REQUIRE(h_dims3[0] > 0 && h_dims3[1] > 0 && h_dims3[2] > 0, "interpolate_grid: dimensions must be positive");
    const size_t n = size_t(h_dims3[0]) * size_t(h_dims3[1]) * size_t(h_dims3[2]);
    GRACE_REQUIRE(n < (size_t(1) << 31), "interpolate_grid: too many lattice points");
    TraceState* ts = nullptr;
    GRACE_TRY(interp_common(a, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, d_weights, n_channels,
                            d_out, d_counts, &ts, gradient, d_grad));
    for (int d = 0; d < 3; ++d) {
        a.org[d] = h_origin3[d];
        a.eu[d] = h_uvw9[d]; a.ev[d] = h_uvw9[3 + d]; a.ew[d] = h_uvw9[6 + d];
        a.dims[d] = h_dims3[d];
    }
    const bool slice = h_dims3[2] == 1;
    a.brick[0] = slice ? 8 : 4; a.brick[1] = slice ? 8 : 4; a.brick[2] = slice ? 1 : 4;
    a.nb[0] = ceil_div(size_t(h_dims3[0]), a.brick[0]);
    a.nb[1] = ceil_div(size_t(h_dims3[1]), a.brick[1]);
    const size_t packets = size_t(a.nb[0]) * a.nb[1] * size_t(ceil_div(size_t(h_dims3[2]), a.brick[2]));
    GRACE_REQUIRE(packets < (size_t(1) << 31) / 64, "interpolate_grid: too many lattice points");
    a.n_packets = int(packets);
    const hipStream_t stream_ = as_stream(stream);
    GRACE_TRY(interp_hook(a, stream_));
    return timed_walks(a, *ts, stream_, [&] {  // (a lattice has no packets to make)
        return interp_walks(a, ts->sph_kernel, d_weights, n_channels, d_out, d_counts, stream_, d_grad);
    });
}

} // namespace

extern "C" {

grace_status grace_interpolate_points_f4(const float* d_points, size_t n_points, int elems_per_point,
                                         const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                         size_t n_nodes, const int* d_leaves, const int* d_root,
                                         const float* d_weights, int n_channels,
                                         float* d_out, int* d_counts, grace_stream stream)
{
    return interpolate_points(InterpArgs(), d_points, n_points, elems_per_point, d_spheres, n_spheres, d_nodes, n_nodes,
                              d_leaves, d_root, d_weights, n_channels, d_out, d_counts, stream);
}

grace_status grace_interpolate_grid_f4(const float* h_origin3, const float* h_uvw9, const int* h_dims3,
                                       const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                       size_t n_nodes, const int* d_leaves, const int* d_root,
                                       const float* d_weights, int n_channels,
                                       float* d_out, int* d_counts, grace_stream stream)
{
    return interpolate_grid(InterpArgs(), h_origin3, h_uvw9, h_dims3, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves,
                            d_root, d_weights, n_channels, d_out, d_counts, stream);
}

grace_status grace_interpolate_points_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                  const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                  size_t n_nodes, const int* d_leaves, const int* d_root,
                                                  const float* d_weights, int n_channels,
                                                  float* d_out, int* d_counts, const float* h_period3,
                                                  grace_stream stream)
{
    Periodic<InterpArgs> a = {};
    GRACE_TRY(walk_period(a.per, h_period3, nullptr));
    return interpolate_points(a, d_points, n_points, elems_per_point, d_spheres, n_spheres, d_nodes, n_nodes,
                              d_leaves, d_root, d_weights, n_channels, d_out, d_counts, stream);
}

grace_status grace_interpolate_grid_periodic_f4(const float* h_origin3, const float* h_uvw9, const int* h_dims3,
                                                const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                size_t n_nodes, const int* d_leaves, const int* d_root,
                                                const float* d_weights, int n_channels,
                                                float* d_out, int* d_counts, const float* h_period3,
                                                grace_stream stream)
{
    Periodic<InterpArgs> a = {};
    GRACE_TRY(walk_period(a.per, h_period3, nullptr));
    return interpolate_grid(a, h_origin3, h_uvw9, h_dims3, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves,
                            d_root, d_weights, n_channels, d_out, d_counts, stream);
}

grace_status grace_interpolate_gradient_points_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                  const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                  size_t n_nodes, const int* d_leaves, const int* d_root,
                                                  const float* d_weights, int n_channels, float* d_grad,
                                                  float* d_value, int* d_counts, grace_stream stream)
{
    return interpolate_points(InterpArgs(), d_points, n_points, elems_per_point, d_spheres, n_spheres, d_nodes, n_nodes,
                              d_leaves, d_root, d_weights, n_channels, d_value, d_counts, stream, true, d_grad);
}

grace_status grace_interpolate_gradient_grid_f4(const float* h_origin3, const float* h_uvw9, const int* h_dims3,
                                                const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                size_t n_nodes, const int* d_leaves, const int* d_root,
                                                const float* d_weights, int n_channels, float* d_grad,
                                                float* d_value, int* d_counts, grace_stream stream)
{
    return interpolate_grid(InterpArgs(), h_origin3, h_uvw9, h_dims3, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves,
                            d_root, d_weights, n_channels, d_value, d_counts, stream, true, d_grad);
}

grace_status grace_interpolate_gradient_points_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                           const float* d_spheres, size_t n_spheres,
                                                           const int* d_nodes, size_t n_nodes, const int* d_leaves,
                                                           const int* d_root, const float* d_weights, int n_channels,
                                                           float* d_grad, float* d_value, int* d_counts,
                                                           const float* h_period3, grace_stream stream)
{
    Periodic<InterpArgs> a = {};
    GRACE_TRY(walk_period(a.per, h_period3, nullptr));
    return interpolate_points(a, d_points, n_points, elems_per_point, d_spheres, n_spheres, d_nodes, n_nodes,
                              d_leaves, d_root, d_weights, n_channels, d_value, d_counts, stream, true, d_grad);
}

grace_status grace_interpolate_gradient_grid_periodic_f4(const float* h_origin3, const float* h_uvw9,
                                                         const int* h_dims3, const float* d_spheres, size_t n_spheres,
                                                         const int* d_nodes, size_t n_nodes, const int* d_leaves,
                                                         const int* d_root, const float* d_weights, int n_channels,
                                                         float* d_grad, float* d_value, int* d_counts,
                                                         const float* h_period3, grace_stream stream)
{
    Periodic<InterpArgs> a = {};
    GRACE_TRY(walk_period(a.per, h_period3, nullptr));
    return interpolate_grid(a, h_origin3, h_uvw9, h_dims3, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves,
                            d_root, d_weights, n_channels, d_value, d_counts, stream, true, d_grad);
}

grace_status grace_gradient_div_curl_f32(const float* d_grad, size_t n, float* d_div, float* d_curl,
                                         grace_stream stream)
{
    GRACE_REQUIRE(d_div || d_curl, "gradient_div_curl: no output");
    GRACE_REQUIRE(n < (size_t(1) << 31), "gradient_div_curl: too many rows");
    if (n == 0) return GRACE_OK;
    GRACE_REQUIRE(d_grad, "gradient_div_curl: null gradient");
    div_curl_kernel<<<ceil_div(n, size_t(256)), 256, 0, as_stream(stream)>>>(d_grad, int(n), d_div, d_curl);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

int grace_interpolate_gradient_channels_per_walk(int channels)
{
    if (channels == 0) g_grad_channels = GRAD_CHANNELS;
    else if (channels >= 1 && channels <= GRAD_CHANNELS_MAX) g_grad_channels = channels;
    return g_grad_channels;
}

grace_status grace_interpolate_enable_stats(int enabled)
{
    if (enabled && !g_tests)
        GRACE_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&g_tests), sizeof(unsigned long long)));
    g_stats = enabled != 0;
    return GRACE_OK;
}

grace_status grace_interpolate_last_stats(unsigned long long* h_survivor_tests)
{
    GRACE_REQUIRE(h_survivor_tests, "interpolate_last_stats: null output");
    GRACE_REQUIRE(g_stats && g_tests, "interpolate_last_stats: statistics are not enabled");
    GRACE_TRY_HIP(hipDeviceSynchronize());
    GRACE_TRY_HIP(hipMemcpy(h_survivor_tests, g_tests, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return GRACE_OK;
}

} // extern "C"
