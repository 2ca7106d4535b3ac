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
    unsigned long long* tests;   // measurement hook: survivor tests (lanes x survivors), or null
};

// NW = channels of this walk (0: counts only).
template <int KIND, int NW>
__global__ __launch_bounds__(PW_BLOCK) void interpolate_kernel(const InterpArgs a)
{
    constexpr int NS = NW > 0 ? NW : 1;
    __shared__ float4 s_rec[PW_WAVES][64];               // survivors: {x, y, z, H^2}
    __shared__ float2 s_inv[PW_WAVES][NW > 0 ? 64 : 1];  // {1/H, 1/H^3}
    __shared__ float s_w[PW_WAVES][NW > 0 ? 64 : 1][NS]; // weights
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

    // ---- class sums ----
    float acc[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) acc[c] = 0.0f;
    if constexpr (NW > 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int c = 0; c < NW; ++c) s_cls[wv][k][c][lane] = 0.0f;
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
            const bool hit_l = overlaps_widened(L.x, L.y, plo_x, phi_x) && overlaps_widened(L.z, L.w, plo_y, phi_y)
                && overlaps_widened(Z.x, Z.y, plo_z, phi_z);
            const bool hit_r = overlaps_widened(R.x, R.y, plo_x, phi_x) && overlaps_widened(R.z, R.w, plo_y, phi_y)
                && overlaps_widened(Z.z, Z.w, plo_z, phi_z);
            if (hit_r) push(__float_as_int(n0.y));
            if (hit_l) push(__float_as_int(n0.x));       // popped first: ascending primitive order
            continue;
        }
        const int4 lf = a.leaves[idx - a.n_nodes];
        sweep_clusters(a.spheres, lf.x, lf.x + lf.y, lane,
            [&](const bool in, const float4& s) {
                return in && overlaps_widened(s.x - s.w, s.x + s.w, plo_x, phi_x)
                    && overlaps_widened(s.y - s.w, s.y + s.w, plo_y, phi_y)
                    && overlaps_widened(s.z - s.w, s.z + s.w, plo_z, phi_z);
            },
            [&](const int pos, const float4& s, const int j) {
                s_rec[wv][pos] = make_float4(s.x, s.y, s.z, s.w * s.w);
                if constexpr (NW > 0) {
                    const float ih = 1.0f / s.w;
                    s_inv[wv][pos] = make_float2(ih, (ih * ih) * ih);
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
                        for (int c = 0; c < NW; ++c) {
                            s_cls[wv][cur][c][lane] = acc[c];
                            acc[c] = s_cls[wv][cls][c][lane];
                        }
                        cur = cls;
                    }
                }
                tests += uint64_t(n_surv);
                for (int j = 0; j < n_surv; ++j) {
                    const float4 r = s_rec[wv][j];
                    const float dx = px - r.x, dy = py - r.y, dz = pz - r.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < r.w) {
                        ++count;
                        if constexpr (NW > 0) {
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
        for (int c = 0; c < NW; ++c) s_cls[wv][cur][c][lane] = acc[c];
#pragma unroll
        for (int c = 0; c < NW; ++c) {
            float t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) t[k] = s_cls[wv][k][c][lane];
            const float s01 = t[0] + t[1], s23 = t[2] + t[3], s45 = t[4] + t[5], s67 = t[6] + t[7];
            a.out[slot * a.out_stride + c] = (s01 + s23) + (s45 + s67);
        }
    }
}

// Process-wide measurement hook (grace_interpolate_enable_stats): a device counter of survivor tests.
unsigned long long* g_tests = nullptr;
bool g_stats = false;

grace_status launch_walk(const InterpArgs& a, int kind, int nw, hipStream_t stream)
{
    const int blocks = ceil_div(size_t(a.n_packets), PW_WAVES);
    if (nw == 0) {
        interpolate_kernel<GRACE_SPH_KERNEL_CUBIC, 0><<<blocks, PW_BLOCK, 0, stream>>>(a);
    } else {
        with_kernel(kind, nw, [&](auto k, auto n) {
            interpolate_kernel<decltype(k)::value, decltype(n)::value><<<blocks, PW_BLOCK, 0, stream>>>(a);
        });
    }
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

// Checks shared by both entry points, and the scene / output fields of the arguments.
grace_status interp_common(InterpArgs& a, const float* d_spheres, size_t n_spheres, const int* d_nodes,
                           size_t n_nodes, const int* d_leaves, const int* d_root, const float* d_weights,
                           int n_channels, float* d_out, int* d_counts, TraceState** ts_out)
{
    PACKET_SCENE(a, "interpolate", false, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root);
    GRACE_REQUIRE(d_out || d_counts, "interpolate: no output");
    if (d_out) {
        GRACE_REQUIRE(n_channels >= 1 && n_channels <= 64, "interpolate: channels must be 1..64");
        GRACE_REQUIRE(d_weights, "interpolate: null weights");
    }
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    GRACE_REQUIRE(ts->sph_kernel >= GRACE_SPH_KERNEL_CUBIC && ts->sph_kernel <= GRACE_SPH_KERNEL_WENDLAND_C6,
                  "interpolate: a custom SPH kernel table has no kernel function f(q)");
    a.w_stride = n_channels;
    a.out_stride = n_channels;
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

// The walks of one call: channels four at a time, counts with the first walk.
grace_status interp_walks(InterpArgs a, int kind, const float* d_weights, int n_channels, float* d_out,
                          int* d_counts, hipStream_t stream)
{
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

} // namespace

extern "C" {

grace_status grace_interpolate_points_f4(const float* d_points, size_t n_points, int elems_per_point,
                                         const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                         size_t n_nodes, const int* d_leaves, const int* d_root,
                                         const float* d_weights, int n_channels,
                                         float* d_out, int* d_counts, grace_stream stream)
{
    GRACE_REQUIRE(elems_per_point >= 3 && elems_per_point <= 16, "interpolate: elements per point must be 3..16");
    GRACE_REQUIRE(n_points < (size_t(1) << 31), "interpolate: too many points");
    if (n_points == 0) return GRACE_OK;   // (before the output checks: a caller's empty arrays may be null)
    GRACE_REQUIRE(d_points, "interpolate: null points");
    InterpArgs a = {};
    TraceState* ts = nullptr;
    GRACE_TRY(interp_common(a, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, d_weights, n_channels,
                            d_out, d_counts, &ts));
    const hipStream_t stream_ = as_stream(stream);
    GRACE_TRY(interp_hook(a, stream_));
    return packet_run(a, *ts, d_points, n_points, elems_per_point, stream_,
                      [&](InterpArgs w, size_t max_packets) -> grace_status {
        w.n_packets = int(max_packets);
        return interp_walks(w, ts->sph_kernel, d_weights, n_channels, d_out, d_counts, stream_);
    });
}

grace_status grace_interpolate_grid_f4(const float* h_origin3, const float* h_uvw9, const int* h_dims3,
                                       const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                       size_t n_nodes, const int* d_leaves, const int* d_root,
                                       const float* d_weights, int n_channels,
                                       float* d_out, int* d_counts, grace_stream stream)
{
    GRACE_REQUIRE(h_origin3 && h_uvw9 && h_dims3, "interpolate_grid: null lattice argument");
    GRACE_REQUIRE(h_dims3[0] > 0 && h_dims3[1] > 0 && h_dims3[2] > 0, "interpolate_grid: dimensions must be positive");
    const size_t n = size_t(h_dims3[0]) * size_t(h_dims3[1]) * size_t(h_dims3[2]);
    GRACE_REQUIRE(n < (size_t(1) << 31), "interpolate_grid: too many lattice points");
    InterpArgs a = {};
    TraceState* ts = nullptr;
    GRACE_TRY(interp_common(a, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, d_weights, n_channels,
                            d_out, d_counts, &ts));
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
        return interp_walks(a, ts->sph_kernel, d_weights, n_channels, d_out, d_counts, stream_);
    });
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
