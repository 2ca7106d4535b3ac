// k nearest neighbours of points among the sphere centres (grace_nearest_neighbours_f4), and
// smoothing lengths from the k-th neighbour of every particle (grace_smoothing_lengths_f4).  An
// extension the reference lacks; the ranking is stated exactly in include/grace_hip.h.
//
// The walk is packet_walk.hpp's (packets, stack, cluster sweep, box helpers).  The smoothing-length
// entry sorts the sphere centres too: tree order is a Morton order of the build's bounds, whose grid
// is not the root box's (the root box includes H), so cutting tree order at root-box cell changes
// left packets of ~4 points (lane fill 0.061 measured on bench.py's scene).
//
// Every lane keeps its k best candidates as 64-bit keys (bits(d2) << 32) | j, ascending in K
// registers (K in {8, 16, 32, 64}, k <= K): for d2 >= 0 the float bits order as the floats, so one
// unsigned compare ranks by (d2, j).  The list sits in the top k slots; the K - k slots below hold
// the key 0, which no candidate is ever below, so the current k-th key is always key[K - 1] (a
// compile-time index) and an insertion is an unrolled compare-and-shift over all K slots.  Empty
// slots hold (+inf, 0xffffffff), above every real candidate, also one at d2 = +inf.
//
// The wave walks the ALBVH against the union of its lanes' query boxes [p - r, p + r], r the
// lane's current k-th distance widened, recomputed whenever a lane's list changes.  Nearer child
// first (box distance to the packet centre), so lists fill early and the boxes shrink.  Leaves are
// pushed as node indices; a leaf's primitives go through the cluster sweep, the survivors
// {x, y, z, j}, and every lane ranks them all.
//
// Widening.  packet_walk.hpp's argument with D := the lane's k-th d2: pruning only drops
// candidates whose d2 is strictly above it, so equal d2 with a lower index still gets in, and the
// result does not depend on the visiting order.
//
// Periodic boxes (walk_packet<K, true>, grace_nearest_neighbours_periodic_f4 /
// grace_smoothing_lengths_periodic_f4; packet_walk.hpp's WalkPeriod: per axis the period L and
// h = fl(0.5 L), an open axis L = 0 and h = +inf).  The separation is range_walk.hpp's: per component
// d = fl(p - x); d > h: d = fl(d - L); else d < -h: d = fl(d + L); every centre is ranked once per
// lane, by its wrapped d2, and there is no radius limit: a k-th distance above h is legal.
//   Pruning, wrapped.  Let D be the lane's current k-th d2 and r' = widened_radius(D).  A centre the
// lane may still take has wrapped d2 <= D, so per component |dw| <= rho = sqrt(D) (1 + 2^-22) < r'.
// On a periodic axis where !(r' < h) -- +inf at the start included -- the lane's bounds are
// -inf .. +inf: the axis prunes nothing for the packet until that lane's radius has shrunk.  Where
// r' < h, range_walk.hpp's "Widening, wrapped" holds with r' in place of r (all it needs of the radius
// is rho < h: beyond 2 L the wrapped component is at least L > 2 rho, up to 2 L the wrap is exact):
// not wrapped, x is in [p - r', p + r']; wrapped, x is within rho + 2^-23 L of p -+ L.  So the lane's
// bounds are p -+ r'', r'' = fl(r' + L 2^-22), moved out by 2^-20 of themselves, and per axis a node
// or a centre passes if it meets the union of the lanes' bounds or that union shifted by -L or +L
// (rounded outward in SGPRs, re-derived whenever a list changes).  Pruning therefore only drops
// centres whose wrapped d2 is strictly above the lane's current k-th d2: a centre with equal d2 and
// a lower index, across the seam or not, still reaches the ranking, which decides by (d2, index).
// The k-th key only falls, so what was dropped against an earlier, larger box stays dropped rightly.
//   The two wave-uniform fast paths are range_walk.hpp's, re-evaluated with the box: while the shifted
// boxes miss the root's box (which holds every node box and centre) nodes and centres are tested
// against the box itself, as in the open walk; and where the box is no wider than h on every axis,
// a cluster whose survivors all came through the unshifted box is ranked without the wrap
// (|fl(p - x)| <= h there: the same bits either way).  A root that is a leaf has no box: images.
//   Child order (for ordering only): the gap to the packet centre or to its images at -+L, whichever
// is smallest, so a packet at a face descends towards the nearer image first.
#include "packet_walk.hpp"

#include <cmath>

using namespace grace_hip;

namespace {

constexpr uint64_t NB_EMPTY = (uint64_t(0x7f800000u) << 32) | 0xffffffffu;

struct NbrArgs : PacketPoints, PacketScene {
    int k;
    int* indices;                // point p's slot s at [p k + s], or null
    float* d2;                   // or null
    float* h;                    // smoothing lengths: h[p] = fl(eta sqrt_rn(d2 of slot k - 1)), or null
    float eta;
    unsigned long long* stats;   // measurement hook (grace_neighbours_last_stats), or null
};

// Squared distance from c to the box (gap per axis; for ordering only).
__device__ __forceinline__ float box_dist2(const float xlo, const float xhi, const float ylo, const float yhi,
                                           const float zlo, const float zhi, const float cx, const float cy,
                                           const float cz)
{
    const float gx = fmaxf(fmaxf(xlo - cx, cx - xhi), 0.0f);
    const float gy = fmaxf(fmaxf(ylo - cy, cy - yhi), 0.0f);
    const float gz = fmaxf(fmaxf(zlo - cz, cz - zhi), 0.0f);
    return gx * gx + gy * gy + gz * gz;
}

// The same on a torus: per axis the smallest gap to c or to its images c - L, c + L (an open axis: L = 0).
__device__ __forceinline__ float wrapped_gap(const float lo, const float hi, const float c, const float L)
{
    const float cm = c - L, cp = c + L;
    const float g0 = fmaxf(lo - c, c - hi), g1 = fmaxf(lo - cm, cm - hi), g2 = fmaxf(lo - cp, cp - hi);
    return fmaxf(fminf(g0, fminf(g1, g2)), 0.0f);
}
__device__ __forceinline__ float box_dist2_wrapped(const float xlo, const float xhi, const float ylo, const float yhi,
                                                   const float zlo, const float zhi, const float cx, const float cy,
                                                   const float cz, const WalkPeriod& per)
{
    const float gx = wrapped_gap(xlo, xhi, cx, per.L[0]);
    const float gy = wrapped_gap(ylo, yhi, cy, per.L[1]);
    const float gz = wrapped_gap(zlo, zhi, cz, per.L[2]);
    return gx * gx + gy * gy + gz * gz;
}

// The lane's bounds on one axis of a periodic box: p -+ fl(r + L 2^-22) where r < h, else everything.
__device__ __forceinline__ void periodic_bounds(const float p, const float r, const float L, const float h,
                                                const bool on, float& lo, float& hi)
{
    query_bounds(p, r + L * 0.25f * PW_SLACK, on, lo, hi);
    if (on && !(r < h)) { lo = __int_as_float(0xff800000); hi = __int_as_float(0x7f800000); }
}

// One packet: the walk, then the lanes' rows.  s_rec: the wave's 64 survivor records {x, y, z, j}.
// PERIODIC: the separation wraps by `per`.
template <int K, bool PERIODIC = false>
__device__ __forceinline__ void walk_packet(const NbrArgs& a, const int packet, const int lane, float4* s_rec,
                                            const WalkPeriod& per = WalkPeriod())
{
    // ---- the packet's points ----
    const PacketPoint pt = load_point(a, packet, lane);
    const bool in_range = pt.in_range;
    const uint32_t src = pt.src;
    float px = pt.px, py = pt.py, pz = pt.pz;
    const bool active = in_range && isfinite(px) && isfinite(py) && isfinite(pz);
    if (!active) px = py = pz = __int_as_float(0x7fc00000);   // NaN: d2 is NaN, ranked after every slot
    const float cx = 0.5f * (wave_min(px) + wave_max(px));    // packet centre (NaN points skipped)
    const float cy = 0.5f * (wave_min(py) + wave_max(py));
    const float cz = 0.5f * (wave_min(pz) + wave_max(pz));

    // ---- the lane's list: slots K - k .. K - 1 ----
    uint64_t key[K];
#pragma unroll
    for (int s = 0; s < K; ++s) key[s] = s < K - a.k ? 0ull : NB_EMPTY;

    float ulo_x, uhi_x, ulo_y, uhi_y, ulo_z, uhi_z;      // union of the lanes' query boxes
    // periodic: the box's images, whether it is narrow enough for a cluster to skip the wrap, whether any
    // image meets the root's box (the union of its children's; a root that is a leaf has none: images)
    AxisImages bx = {}, by = {}, bz = {};
    bool narrow = false, images = true, plain = true;
    float dlo_x = 0.0f, dhi_x = 0.0f, dlo_y = 0.0f, dhi_y = 0.0f, dlo_z = 0.0f, dhi_z = 0.0f;
    bool root_box = false;
    if constexpr (PERIODIC) {
        const int rt = *a.root;
        if (rt >= 0 && rt < a.n_nodes) {
            const float4* np = a.nodes + 4 * size_t(rt);
            const float4 L = np[1], R = np[2], Z = np[3];
            dlo_x = uniform(fminf(L.x, R.x)); dhi_x = uniform(fmaxf(L.y, R.y));
            dlo_y = uniform(fminf(L.z, R.z)); dhi_y = uniform(fmaxf(L.w, R.w));
            dlo_z = uniform(fminf(Z.x, Z.z)); dhi_z = uniform(fmaxf(Z.y, Z.w));
            root_box = true;
        }
    }
    auto union_box = [&]() {
        const float D = __uint_as_float(uint32_t(key[K - 1] >> 32));
        const float r = widened_radius(D);
        float lo, hi;
        if constexpr (PERIODIC) {
            periodic_bounds(px, r, per.L[0], per.h[0], active, lo, hi); ulo_x = wave_min(lo); uhi_x = wave_max(hi);
            periodic_bounds(py, r, per.L[1], per.h[1], active, lo, hi); ulo_y = wave_min(lo); uhi_y = wave_max(hi);
            periodic_bounds(pz, r, per.L[2], per.h[2], active, lo, hi); ulo_z = wave_min(lo); uhi_z = wave_max(hi);
            bx = axis_images(ulo_x, uhi_x, per.L[0]);
            by = axis_images(ulo_y, uhi_y, per.L[1]);
            bz = axis_images(ulo_z, uhi_z, per.L[2]);
            narrow = (uhi_x - ulo_x) * (1.0f + PW_SLACK) <= per.h[0] && (uhi_y - ulo_y) * (1.0f + PW_SLACK) <= per.h[1]
                && (uhi_z - ulo_z) * (1.0f + PW_SLACK) <= per.h[2];
            images = !root_box
                || overlaps(dlo_x, dhi_x, bx.mlo, bx.mhi) || overlaps(dlo_x, dhi_x, bx.plo, bx.phi)
                || overlaps(dlo_y, dhi_y, by.mlo, by.mhi) || overlaps(dlo_y, dhi_y, by.plo, by.phi)
                || overlaps(dlo_z, dhi_z, bz.mlo, bz.mhi) || overlaps(dlo_z, dhi_z, bz.plo, bz.phi);
        } else {
            query_bounds(px, r, active, lo, hi); ulo_x = wave_min(lo); uhi_x = wave_max(hi);
            query_bounds(py, r, active, lo, hi); ulo_y = wave_min(lo); uhi_y = wave_max(hi);
            query_bounds(pz, r, active, lo, hi); ulo_z = wave_min(lo); uhi_z = wave_max(hi);
        }
    };
    union_box();
    unsigned long long tests = 0, steps = 0;               // survivors; survivors some lane inserted

    PacketStack stack;
    auto push = [&](const int idx) { stack.push(lane, idx); };
    push(*a.root);

    while (!stack.empty()) {
        const int idx = stack.pop();
        if (idx < a.n_nodes) {
            const float4* np = a.nodes + 4 * size_t(idx);
            const float4 n0 = np[0], L = np[1], R = np[2], Z = np[3];
            bool hit_l, hit_r;
            if (PERIODIC && images) {
                hit_l = bx.meets(L.x, L.y) && by.meets(L.z, L.w) && bz.meets(Z.x, Z.y);
                hit_r = bx.meets(R.x, R.y) && by.meets(R.z, R.w) && bz.meets(Z.z, Z.w);
            } else {
                hit_l = overlaps(L.x, L.y, ulo_x, uhi_x) && overlaps(L.z, L.w, ulo_y, uhi_y)
                    && overlaps(Z.x, Z.y, ulo_z, uhi_z);
                hit_r = overlaps(R.x, R.y, ulo_x, uhi_x) && overlaps(R.z, R.w, ulo_y, uhi_y)
                    && overlaps(Z.z, Z.w, ulo_z, uhi_z);
            }
            const int left = __float_as_int(n0.x), right = __float_as_int(n0.y);
            if (hit_l && hit_r) {
                // a leaf child first, which leaves nothing on the stack (the ALBVH of coincident points is
                // a spine of leaves deeper than the stack); of two inner children the nearer one
                const bool l_leaf = left >= a.n_nodes, r_leaf = right >= a.n_nodes;
                bool left_first;
                if constexpr (PERIODIC)
                    left_first = l_leaf != r_leaf ? l_leaf
                        : box_dist2_wrapped(L.x, L.y, L.z, L.w, Z.x, Z.y, cx, cy, cz, per)
                            <= box_dist2_wrapped(R.x, R.y, R.z, R.w, Z.z, Z.w, cx, cy, cz, per);
                else
                    left_first = l_leaf != r_leaf ? l_leaf
                        : box_dist2(L.x, L.y, L.z, L.w, Z.x, Z.y, cx, cy, cz) <= box_dist2(R.x, R.y, R.z, R.w, Z.z, Z.w, cx, cy, cz);
                push(left_first ? right : left);
                push(left_first ? left : right);          // popped first: the nearer child
            } else if (hit_l) {
                push(left);
            } else if (hit_r) {
                push(right);
            }
            continue;
        }
        const int4 lf = a.leaves[idx - a.n_nodes];
        sweep_clusters(a.spheres, lf.x, lf.x + lf.y, lane,
            [&](const bool in, const float4& c) {
                if (PERIODIC && images) {
                    const bool kept = in && bx.holds(c.x) && by.holds(c.y) && bz.holds(c.z);
                    const bool image = kept && !(bx.direct(c.x) && by.direct(c.y) && bz.direct(c.z));
                    plain = narrow && __builtin_amdgcn_ballot_w64(image) == 0ull;
                    return kept;
                }
                if constexpr (PERIODIC) plain = narrow;
                return in && c.x >= ulo_x && c.x <= uhi_x && c.y >= ulo_y && c.y <= uhi_y
                    && c.z >= ulo_z && c.z <= uhi_z;
            },
            [&](const int pos, const float4& c, const int j) {
                s_rec[pos] = make_float4(c.x, c.y, c.z, __int_as_float(j));
            },
            [&](int, const int n_surv) {
                tests += uint64_t(n_surv);
                bool changed = false;
                for (int j = 0; j < n_surv; ++j) {
                    const float4 r = s_rec[j];
                    float dx = px - r.x, dy = py - r.y, dz = pz - r.z;
                    if constexpr (PERIODIC) {
                        if (!plain) {                              // (wave-uniform)
                            dx = wrap_sep(dx, per.L[0], per.h[0]);
                            dy = wrap_sep(dy, per.L[1], per.h[1]);
                            dz = wrap_sep(dz, per.L[2], per.h[2]);
                        }
                    }
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    const uint64_t c = (uint64_t(__float_as_uint(d2)) << 32) | uint32_t(__float_as_int(r.w));
                    const bool ins = c < key[K - 1];
                    steps += __builtin_amdgcn_ballot_w64(ins) != 0ull;
                    if (ins) {
                        // compare-and-shift: slot s takes slot s - 1 if c ranks below it, else c if c ranks below slot s
                        bool lt_hi = true;                         // c < key[s2]
#pragma unroll
                        for (int s2 = K - 1; s2 > 0; --s2) {
                            const bool lt_lo = c < key[s2 - 1];
                            key[s2] = lt_lo ? key[s2 - 1] : (lt_hi ? c : key[s2]);
                            lt_hi = lt_lo;
                        }
                        key[0] = lt_hi ? c : key[0];
                        changed = true;
                    }
                }
                if (__builtin_amdgcn_ballot_w64(changed)) union_box();
            });
    }

    stack.report(lane, a.status);
    const unsigned long long n_active = __builtin_popcountll(__builtin_amdgcn_ballot_w64(active));   // (all lanes)
    if (a.stats && lane == 0) {
        atomicAdd(a.stats, tests * n_active);
        atomicAdd(a.stats + 1, 1ull);
        atomicAdd(a.stats + 2, steps);
    }
    if (!in_range) return;
    if (a.h) {
        const float D = __uint_as_float(uint32_t(key[K - 1] >> 32));
        a.h[src] = a.eta * sqrt_rn(D);
    }
    const int k = a.k;
#pragma unroll
    for (int s = 0; s < K; ++s) {
        if (s < K - k) continue;
        const uint32_t j = uint32_t(key[s]);
        const size_t o = size_t(src) * k + (s - (K - k));
        if (a.indices) a.indices[o] = j == 0xffffffffu ? -1 : int(j);
        if (a.d2) a.d2[o] = j == 0xffffffffu ? __int_as_float(0x7f800000) : __uint_as_float(uint32_t(key[s] >> 32));
    }
}

// Args: NbrArgs, or Periodic<NbrArgs> for the periodic walk.
template <int K, typename Args>
__global__ __launch_bounds__(PW_BLOCK) void neighbours_kernel(const Args a)
{
    __shared__ float4 s_rec[PW_WAVES][64];
    const PacketWave w = packet_wave();
    if (w.packet < int(*a.n_starts)) {
        if constexpr (is_periodic<Args>::value) walk_packet<K, true>(a, w.packet, w.lane, s_rec[w.wv], a.per);
        else walk_packet<K>(a, w.packet, w.lane, s_rec[w.wv]);
    }
}

// Process-wide measurement hook (grace_neighbours_enable_stats): {candidate tests, packets,
// insertion steps}.
unsigned long long* g_stats_dev = nullptr;
bool g_stats = false;

template <int K, typename Args>
void launch_k(const Args& a, size_t waves, hipStream_t stream)
{
    neighbours_kernel<K, Args><<<ceil_div(waves, PW_WAVES), PW_BLOCK, 0, stream>>>(a);
}

// Keys against the root box, sort, packet starts, then the walk.
template <typename Args>
grace_status nbr_run(Args a, const float* d_points, size_t n_points, int stride, hipStream_t stream)
{
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    if (g_stats && g_stats_dev) {
        GRACE_TRY_HIP(hipMemsetAsync(g_stats_dev, 0, 3 * sizeof(unsigned long long), stream));
        a.stats = g_stats_dev;
    }
    return packet_run(a, *ts, d_points, n_points, stride, stream, [&](const Args& w, size_t waves) -> grace_status {
        if (w.k <= 8) launch_k<8>(w, waves, stream);
        else if (w.k <= 16) launch_k<16>(w, waves, stream);
        else if (w.k <= 32) launch_k<32>(w, waves, stream);
        else launch_k<64>(w, waves, stream);
        GRACE_CHECK_LAUNCH();
        return GRACE_OK;
    });
}

// grace_nearest_neighbours_f4 and its periodic form: `a` is zero but for a period.
template <typename Args>
grace_status nearest_neighbours(Args a, const float* d_points, size_t n_points, int elems_per_point,
                                const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                size_t n_nodes, const int* d_leaves, const int* d_root,
                                int k, int* d_indices, float* d_d2, grace_stream stream)
{
    GRACE_REQUIRE(elems_per_point >= 3 && elems_per_point <= 16, "nearest_neighbours: elements per point must be 3..16");
    GRACE_REQUIRE(k >= 1 && k <= 64, "nearest_neighbours: k must be 1..64");
    GRACE_REQUIRE(n_points < (size_t(1) << 31), "nearest_neighbours: too many points");
    if (n_points == 0) return GRACE_OK;   // (before the output checks: a caller's empty arrays may be null)
    GRACE_REQUIRE(d_points, "nearest_neighbours: null points");
    GRACE_REQUIRE(d_indices || d_d2, "nearest_neighbours: no output");
    PACKET_SCENE(a, "neighbours", true, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root);
    a.k = k;
    a.indices = d_indices;
    a.d2 = d_d2;
    return nbr_run(a, d_points, n_points, elems_per_point, as_stream(stream));
}

// grace_smoothing_lengths_f4 and its periodic form.
template <typename Args>
grace_status smoothing_lengths(Args a, const float* d_spheres, size_t n_spheres, const int* d_nodes,
                               size_t n_nodes, const int* d_leaves, const int* d_root,
                               int k, float eta, float* d_h, grace_stream stream)
{
    GRACE_REQUIRE(k >= 1 && k <= 64, "smoothing_lengths: k must be 1..64");
    GRACE_REQUIRE(std::isfinite(eta) && eta > 0.0f, "smoothing_lengths: eta must be finite and positive");
    GRACE_REQUIRE(d_h, "smoothing_lengths: null output");
    GRACE_REQUIRE(size_t(k) <= n_spheres, "smoothing_lengths: k exceeds the number of spheres");
    PACKET_SCENE(a, "neighbours", true, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root);
    a.k = k;
    a.h = d_h;
    a.eta = eta;
    return nbr_run(a, d_spheres, n_spheres, 4, as_stream(stream));
}

} // namespace

extern "C" {

grace_status grace_nearest_neighbours_f4(const float* d_points, size_t n_points, int elems_per_point,
                                         const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                         size_t n_nodes, const int* d_leaves, const int* d_root,
                                         int k, int* d_indices, float* d_d2, grace_stream stream)
{
    return nearest_neighbours(NbrArgs(), d_points, n_points, elems_per_point, d_spheres, n_spheres, d_nodes, n_nodes,
                              d_leaves, d_root, k, d_indices, d_d2, stream);
}

grace_status grace_smoothing_lengths_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                        size_t n_nodes, const int* d_leaves, const int* d_root,
                                        int k, float eta, float* d_h, grace_stream stream)
{
    return smoothing_lengths(NbrArgs(), d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, k, eta, d_h, stream);
}

grace_status grace_nearest_neighbours_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                  const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                  size_t n_nodes, const int* d_leaves, const int* d_root,
                                                  int k, int* d_indices, float* d_d2, const float* h_period3,
                                                  grace_stream stream)
{
    Periodic<NbrArgs> a = {};
    GRACE_TRY(walk_period(a.per, h_period3, nullptr));
    return nearest_neighbours(a, d_points, n_points, elems_per_point, d_spheres, n_spheres, d_nodes, n_nodes,
                              d_leaves, d_root, k, d_indices, d_d2, stream);
}

grace_status grace_smoothing_lengths_periodic_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                 size_t n_nodes, const int* d_leaves, const int* d_root,
                                                 int k, float eta, float* d_h, const float* h_period3,
                                                 grace_stream stream)
{
    Periodic<NbrArgs> a = {};
    GRACE_TRY(walk_period(a.per, h_period3, nullptr));
    return smoothing_lengths(a, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, k, eta, d_h, stream);
}

grace_status grace_neighbours_enable_stats(int enabled)
{
    if (enabled && !g_stats_dev)
        GRACE_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&g_stats_dev), 3 * sizeof(unsigned long long)));
    g_stats = enabled != 0;
    return GRACE_OK;
}

grace_status grace_neighbours_last_stats(unsigned long long* h_candidate_tests, unsigned long long* h_packets,
                                         unsigned long long* h_insertion_steps)
{
    GRACE_REQUIRE(h_candidate_tests && h_packets && h_insertion_steps, "neighbours_last_stats: null output");
    GRACE_REQUIRE(g_stats && g_stats_dev, "neighbours_last_stats: statistics are not enabled");
    unsigned long long v[3];
    GRACE_TRY_HIP(hipDeviceSynchronize());
    GRACE_TRY_HIP(hipMemcpy(v, g_stats_dev, sizeof(v), hipMemcpyDeviceToHost));
    *h_candidate_tests = v[0];
    *h_packets = v[1];
    *h_insertion_steps = v[2];
    return GRACE_OK;
}

} // extern "C"
