// Range queries of points among the sphere centres: every centre within the query point's own
// radius (grace_range_counts_f4: counts and gather sums, grace_range_neighbours_f4: CSR lists).  An
// extension the reference lacks; membership, order and the sums' arithmetic are stated exactly in
// include/grace_hip.h.
//
// Packets are the interpolation's (point_packets.hpp): one wave owns up to 64 points of one Morton
// cell, keys against the tree's root box, sorted.  The wave walks the ALBVH against the union of its
// lanes' query boxes [p - r', p + r'], r' the lane's radius widened (below).  The radii are known up
// front, so the union is computed once and there is nothing to keep per lane but a counter, the
// running sums or the row's write position; the row itself is never held in registers.
//
// Order.  A node's left child covers the lower index range (albvh.hip: the left child spans leaves
// first .. j, the right one j + 1 .. last), so left child first visits the leaves, and with them
// the primitives, in ascending tree index: the lists and the sums' order fall out of the walk.
//
// Stack.  128 entries, one per lane of two registers (the trace's convention), and a second word
// per entry: an entry is an inner node, or a RANGE of primitives [lo, lo + n) -- a leaf whose box
// met the union box.  A range pushed directly under a range that starts where it ends is merged
// into it.  The ALBVH of coincident points is a spine of leaves deeper than the stack; whichever
// side its leaves hang on, they are popped at once (left) or merged into the waiting range
// (right), so the spine never grows the stack.  Overflow is reported through the status word.
//
// A range is swept in 64-aligned clusters: each lane tests one centre against the union box, a
// ballot compacts the survivors {x, y, z, j} (and the walk's <= 4 weights) into LDS in ascending j,
// and every lane tests them all against its own point: one compare, then a count, an append or the
// kernel and one multiply-add pair per channel.
//
// Widening.  A centre in range has d2 <= D := R2 = fl(r * r), so fl(dx*dx) <= D, since the rounded
// sums of non-negative terms never fall below a term, so the exact |p - x| per component is below
// sqrt(D) (1 + 2^-22).  r' = fl(v_sqrt(D) (1 + 2^-20)) + 2^-60 exceeds that (v_sqrt is within 1 ulp;
// the 2^-60 covers D that underflowed to 0 or a flushed denormal), and the rounded bounds p - r',
// p + r' are then moved out by 2^-20 of themselves, far more than their rounding.  Node boxes built
// with any H >= 0 contain their centres exactly.  So pruning only drops centres whose d2 is
// strictly above the lane's R2: d2 == R2 still gets in, and the result does not depend on the tree's
// H, max_per_leaf or the packets.  Off points (a non-finite coordinate; r negative, NaN or +inf)
// have an empty box and NaN in place of their coordinates and R2: no lane widens for them, and
// no compare is ever true.
#include "point_packets.hpp"
#include "sph_kernel_f.hpp"

#include <cmath>

using namespace grace_hip;

namespace {

constexpr int RG_BLOCK = 256;
constexpr int RG_WAVES = RG_BLOCK / 64;
constexpr int RG_STACK = 128;
constexpr int RG_CHANNELS = 4;     // channels per walk
constexpr float RG_SLACK = 9.5367431640625e-07f;     // 2^-20
constexpr float RG_FLOOR = 8.673617379884035e-19f;   // 2^-60

enum { RG_COUNT = 0, RG_SUMS = 1, RG_FILL = 2 };

struct RangeArgs {
    const float* points;         // n records of `stride` floats, visited in the order `perm`
    int stride;
    const uint32_t* perm;        // sorted position -> point index
    const uint32_t* starts;      // packet p: sorted points [starts[p], starts[p + 1])
    const uint32_t* n_starts;    // number of packets (device)
    const float* radii;          // per point, caller's order, or null: `radius` for all
    float radius;
    const float4* spheres;
    const float4* nodes;
    int n_nodes;
    const int4* leaves;
    const int* root;
    const float* weights;        // this walk's first channel; sphere j's channel c at weights[j w_stride + c]
    int w_stride;
    float* sums;                 // point p's channel c at sums[p w_stride + c]
    int* counts;                 // or null
    const int* offsets;          // fill: row p is [offsets[p], offsets[p + 1])
    int* indices;                // or null
    float* d2;                   // or null
    int* status;
};

// The lane's query box on one axis, widened as stated above (off lanes: empty, +inf / -inf).
__device__ __forceinline__ void query_bounds(const float p, const float r, const bool on, float& lo, float& hi)
{
    const float l = p - r, u = p + r;
    lo = on ? l - fabsf(l) * RG_SLACK : __int_as_float(0x7f800000);
    hi = on ? u + fabsf(u) * RG_SLACK : __int_as_float(0xff800000);
}

__device__ __forceinline__ bool overlaps(const float lo, const float hi, const float ulo, const float uhi)
{
    return lo <= uhi && hi >= ulo;
}

// One packet.  MODE: what a lane does with a centre in range; KIND, NW: the SPH kernel and the
// channels of a RG_SUMS walk.  s_rec / s_w: the wave's 64 survivor records and their weights.
template <int MODE, int KIND, int NW>
__device__ __forceinline__ void walk_packet(const RangeArgs& a, const int packet, const int lane, float4* s_rec,
                                            float (*s_w)[NW > 0 ? NW : 1])
{
    constexpr int NS = NW > 0 ? NW : 1;
    // ---- the packet's points ----
    const uint32_t first = a.starts[packet], end = a.starts[packet + 1];
    const uint32_t spos = first + uint32_t(lane);
    const bool in_range = spos < end;
    const uint32_t src = in_range ? a.perm[spos] : 0u;
    const float* q = a.points + size_t(src) * a.stride;
    float px = q[0], py = q[1], pz = q[2];
    const float r = a.radii ? a.radii[src] : a.radius;
    const bool on = in_range && isfinite(px) && isfinite(py) && isfinite(pz) && r >= 0.0f
        && r < __int_as_float(0x7f800000);
    if (!on) px = py = pz = __int_as_float(0x7fc00000);
    const float R2 = on ? r * r : __int_as_float(0x7fc00000);   // NaN: no d2 <= R2

    // ---- the union of the lanes' query boxes, once ----
    float ulo_x, uhi_x, ulo_y, uhi_y, ulo_z, uhi_z;
    {
        const float rw = __builtin_amdgcn_sqrtf(R2) * (1.0f + RG_SLACK) + RG_FLOOR;   // R2 = +inf: +inf
        float lo, hi;
        query_bounds(px, rw, on, lo, hi); ulo_x = wave_min(lo); uhi_x = wave_max(hi);
        query_bounds(py, rw, on, lo, hi); ulo_y = wave_min(lo); uhi_y = wave_max(hi);
        query_bounds(pz, rw, on, lo, hi); ulo_z = wave_min(lo); uhi_z = wave_max(hi);
    }

    int found = 0;
    float acc[NS];
#pragma unroll
    for (int c = 0; c < NS; ++c) acc[c] = 0.0f;
    float ih = 0.0f, ih3 = 0.0f;
    bool summing = false;                                   // r == 0: the sum is 0 (no 1 / r)
    if constexpr (MODE == RG_SUMS) {
        summing = on && r > 0.0f;
        ih = summing ? 1.0f / r : 0.0f;
        ih3 = (ih * ih) * ih;
    }
    int row = 0, row_end = 0;
    if constexpr (MODE == RG_FILL) {
        if (in_range) { row = a.offsets[src]; row_end = a.offsets[src + 1]; }
    }

    // ---- packet stack: entry e in lane (e & 63) of stk0 / cnt0 (e < 64) or stk1 / cnt1.
    //      cnt == 0: the inner node stk;  cnt > 0: the primitives [stk, stk + cnt) ----
    int stk0 = 0, stk1 = 0, cnt0 = 0, cnt1 = 0, sp = -1;
    bool overflow = false;
    auto top = [&](int& value, int& count) {
        value = sp < 64 ? __builtin_amdgcn_readlane(stk0, sp) : __builtin_amdgcn_readlane(stk1, sp - 64);
        count = sp < 64 ? __builtin_amdgcn_readlane(cnt0, sp) : __builtin_amdgcn_readlane(cnt1, sp - 64);
    };
    auto set_top = [&](const int value, const int count) {
        if (sp < 64) { stk0 = lane == sp ? value : stk0; cnt0 = lane == sp ? count : cnt0; }
        else { stk1 = lane == sp - 64 ? value : stk1; cnt1 = lane == sp - 64 ? count : cnt1; }
    };
    // a child of a node (or the root): an inner node, or a leaf as its range of primitives
    auto push = [&](const int idx) {
        int value = idx, count = 0;
        if (idx >= a.n_nodes) {
            const int4 lf = a.leaves[idx - a.n_nodes];
            if (lf.y <= 0) return;
            value = lf.x; count = lf.y;
            if (sp >= 0) {
                int tv, tc;
                top(tv, tc);
                if (tc > 0 && tv == value + count) { set_top(value, count + tc); return; }   // merge
            }
        }
        if (sp >= RG_STACK - 1) { overflow = true; return; }   // bounds check before every push
        ++sp;
        set_top(value, count);
    };
    push(*a.root);

    while (sp >= 0) {
        int idx, n_prims;
        top(idx, n_prims);
        --sp;
        if (n_prims == 0) {
            const float4* np = a.nodes + 4 * size_t(idx);
            const float4 n0 = np[0], L = np[1], R = np[2], Z = np[3];
            const bool hit_l = overlaps(L.x, L.y, ulo_x, uhi_x) && overlaps(L.z, L.w, ulo_y, uhi_y)
                && overlaps(Z.x, Z.y, ulo_z, uhi_z);
            const bool hit_r = overlaps(R.x, R.y, ulo_x, uhi_x) && overlaps(R.z, R.w, ulo_y, uhi_y)
                && overlaps(Z.z, Z.w, ulo_z, uhi_z);
            if (hit_r) push(__float_as_int(n0.y));
            if (hit_l) push(__float_as_int(n0.x));       // popped first: ascending primitive order
            continue;
        }
        const int r_lo = idx, r_hi = idx + n_prims;
        for (int cl = r_lo >> 6; cl <= (r_hi - 1) >> 6; ++cl) {
            const int pj = (cl << 6) + lane;
            const bool in = pj >= r_lo && pj < r_hi;
            const int pc = min(max(pj, r_lo), r_hi - 1);
            const float4 s = a.spheres[pc];
            const bool keep = in && s.x >= ulo_x && s.x <= uhi_x && s.y >= ulo_y && s.y <= uhi_y
                && s.z >= ulo_z && s.z <= uhi_z;
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
            if (mask == 0ull) continue;
            const int n_surv = __builtin_popcountll(mask);
            if (keep) {
                const int pos = __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0));
                s_rec[pos] = make_float4(s.x, s.y, s.z, __int_as_float(pj));
                if constexpr (MODE == RG_SUMS) {
#pragma unroll
                    for (int c = 0; c < NW; ++c) s_w[pos][c] = a.weights[size_t(pc) * a.w_stride + c];
                }
            }
            wave_sync();
            for (int j = 0; j < n_surv; ++j) {
                const float4 rec = s_rec[j];
                const float dx = px - rec.x, dy = py - rec.y, dz = pz - rec.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 <= R2) {
                    if constexpr (MODE == RG_FILL) {
                        const int o = row + found;
                        if (o < row_end) {               // never outside the row
                            if (a.indices) a.indices[o] = __float_as_int(rec.w);
                            if (a.d2) a.d2[o] = d2;
                        }
                    }
                    ++found;
                    if constexpr (MODE == RG_SUMS) {
                        if (summing) {
                            const float W = kernel_f<KIND>(sqrt_rn(d2) * ih) * ih3;
#pragma unroll
                            for (int c = 0; c < NW; ++c) acc[c] = acc[c] + s_w[j][c] * W;
                        }
                    }
                }
            }
            wave_sync();
        }
    }

    if (overflow && lane == 0) atomicMax(a.status, int(GRACE_STACK_OVERFLOW));
    if (!in_range) return;
    if constexpr (MODE == RG_FILL) {
        if (found != row_end - row) atomicMax(a.status, int(GRACE_INVALID_ARGUMENT));
    } else {
        if (a.counts) a.counts[src] = found;
    }
    if constexpr (MODE == RG_SUMS) {
#pragma unroll
        for (int c = 0; c < NW; ++c) a.sums[size_t(src) * a.w_stride + c] = acc[c];
    }
}

template <int MODE, int KIND, int NW>
__global__ __launch_bounds__(RG_BLOCK) void range_kernel(const RangeArgs a)
{
    __shared__ float4 s_rec[RG_WAVES][64];
    __shared__ float s_w[RG_WAVES][NW > 0 ? 64 : 1][NW > 0 ? NW : 1];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int packet = blockIdx.x * RG_WAVES + wv;      // (surplus waves of the n / 64 + cells bound exit)
    if (packet < int(*a.n_starts)) walk_packet<MODE, KIND, NW>(a, packet, lane, s_rec[wv], s_w[wv]);
}

template <int KIND>
void launch_sums(const RangeArgs& a, int nw, int blocks, hipStream_t stream)
{
    switch (nw) {
    case 1: range_kernel<RG_SUMS, KIND, 1><<<blocks, RG_BLOCK, 0, stream>>>(a); break;
    case 2: range_kernel<RG_SUMS, KIND, 2><<<blocks, RG_BLOCK, 0, stream>>>(a); break;
    case 3: range_kernel<RG_SUMS, KIND, 3><<<blocks, RG_BLOCK, 0, stream>>>(a); break;
    default: range_kernel<RG_SUMS, KIND, 4><<<blocks, RG_BLOCK, 0, stream>>>(a); break;
    }
}

// One walk: mode RG_COUNT / RG_FILL, or RG_SUMS over nw channels with the built-in kernel `kind`.
grace_status launch_walk(const RangeArgs& a, int mode, int kind, int nw, size_t waves, hipStream_t stream)
{
    const int blocks = ceil_div(waves, RG_WAVES);
    if (mode == RG_COUNT) {
        range_kernel<RG_COUNT, GRACE_SPH_KERNEL_CUBIC, 0><<<blocks, RG_BLOCK, 0, stream>>>(a);
    } else if (mode == RG_FILL) {
        range_kernel<RG_FILL, GRACE_SPH_KERNEL_CUBIC, 0><<<blocks, RG_BLOCK, 0, stream>>>(a);
    } else {
        switch (kind) {
        case GRACE_SPH_KERNEL_CUBIC: launch_sums<GRACE_SPH_KERNEL_CUBIC>(a, nw, blocks, stream); break;
        case GRACE_SPH_KERNEL_QUARTIC: launch_sums<GRACE_SPH_KERNEL_QUARTIC>(a, nw, blocks, stream); break;
        case GRACE_SPH_KERNEL_QUINTIC: launch_sums<GRACE_SPH_KERNEL_QUINTIC>(a, nw, blocks, stream); break;
        case GRACE_SPH_KERNEL_WENDLAND_C2: launch_sums<GRACE_SPH_KERNEL_WENDLAND_C2>(a, nw, blocks, stream); break;
        case GRACE_SPH_KERNEL_WENDLAND_C4: launch_sums<GRACE_SPH_KERNEL_WENDLAND_C4>(a, nw, blocks, stream); break;
        default: launch_sums<GRACE_SPH_KERNEL_WENDLAND_C6>(a, nw, blocks, stream); break;
        }
    }
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

// The checks both entry points share (before anything is enqueued), and the scene's fields.
grace_status range_common(RangeArgs& a, const float* d_points, size_t n_points,
                          const float* d_radii, float radius, const float* d_spheres, size_t n_spheres,
                          const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root)
{
    GRACE_REQUIRE(d_points, "range query: null points");
    GRACE_REQUIRE(d_radii || (std::isfinite(radius) && radius >= 0.0f),
                  "range query: the radius must be finite and not negative");
    GRACE_REQUIRE(d_spheres && d_leaves && d_root && (d_nodes || n_nodes == 0), "range query: null scene pointer");
    GRACE_REQUIRE(n_nodes < (size_t(1) << 30), "range query: bad node count");
    GRACE_REQUIRE(n_spheres > 0 && n_spheres < (size_t(1) << 31), "range query: bad sphere count");
    a.radii = d_radii;
    a.radius = radius;
    a.spheres = reinterpret_cast<const float4*>(d_spheres);
    a.nodes = reinterpret_cast<const float4*>(d_nodes);
    a.n_nodes = int(n_nodes);
    a.leaves = reinterpret_cast<const int4*>(d_leaves);
    a.root = d_root;
    return GRACE_OK;
}

// Keys against the root box, sort, packet starts, then the walks of one call (timed together).
template <typename Walks>
grace_status range_run(RangeArgs a, TraceState& ts, const float* d_points, size_t n_points, int stride,
                       hipStream_t stream, Walks walks)
{
    FrameGuard frame;
    PointPackets pk;
    GRACE_TRY(point_packets(frame, d_points, n_points, stride, a.nodes, a.n_nodes, a.root, stream, pk));
    a.points = d_points;
    a.stride = stride;
    a.perm = pk.perm;
    a.starts = pk.starts;
    a.n_starts = pk.n_starts;
    GRACE_TRY(ensure_status(ts, stream));
    a.status = ts.status;
    if (ts.timing) {
        if (!ts.ev0) { GRACE_TRY_HIP(hipEventCreate(&ts.ev0)); GRACE_TRY_HIP(hipEventCreate(&ts.ev1)); }
        GRACE_TRY_HIP(hipEventRecord(ts.ev0, stream));
    }
    GRACE_TRY(walks(a, pk.max_packets));
    if (ts.timing) {
        GRACE_TRY_HIP(hipEventRecord(ts.ev1, stream));
        ts.ev_valid = true;
    }
    return GRACE_OK;
}

} // namespace

extern "C" {

grace_status grace_range_counts_f4(const float* d_points, size_t n_points, int elems_per_point,
                                   const float* d_radii, float radius,
                                   const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                   size_t n_nodes, const int* d_leaves, const int* d_root,
                                   const float* d_weights, int n_channels,
                                   int* d_counts, float* d_sums, grace_stream stream)
{
    GRACE_REQUIRE(elems_per_point >= 3 && elems_per_point <= 16, "range_counts: elements per point must be 3..16");
    GRACE_REQUIRE(n_points < (size_t(1) << 31), "range_counts: too many points");
    if (d_sums) {
        GRACE_REQUIRE(n_channels >= 1 && n_channels <= 64, "range_counts: channels must be 1..64");
        GRACE_REQUIRE(d_weights, "range_counts: sums need weights");
    }
    if (n_points == 0) return GRACE_OK;   // (before the output checks: a caller's empty arrays may be null)
    GRACE_REQUIRE(d_counts || d_sums, "range_counts: no output");
    RangeArgs a = {};
    GRACE_TRY(range_common(a, d_points, n_points, d_radii, radius, d_spheres, n_spheres, d_nodes,
                           n_nodes, d_leaves, d_root));
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    const int kind = ts->sph_kernel;
    if (d_sums)
        GRACE_REQUIRE(kind >= GRACE_SPH_KERNEL_CUBIC && kind <= GRACE_SPH_KERNEL_WENDLAND_C6,
                      "range_counts: a custom SPH kernel table has no kernel function f(q)");
    a.w_stride = n_channels;
    const hipStream_t stream_ = as_stream(stream);
    return range_run(a, *ts, d_points, n_points, elems_per_point, stream_,
                     [&](RangeArgs w, size_t waves) -> grace_status {
        if (!d_sums) {
            w.counts = d_counts;
            return launch_walk(w, RG_COUNT, kind, 0, waves, stream_);
        }
        // channels four at a time, counts with the first walk
        for (int g = 0; g < n_channels; g += RG_CHANNELS) {
            w.weights = d_weights + g;
            w.sums = d_sums + g;
            w.counts = g == 0 ? d_counts : nullptr;
            GRACE_TRY(launch_walk(w, RG_SUMS, kind, min(RG_CHANNELS, n_channels - g), waves, stream_));
        }
        return GRACE_OK;
    });
}

grace_status grace_range_neighbours_f4(const float* d_points, size_t n_points, int elems_per_point,
                                       const float* d_radii, float radius,
                                       const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                       size_t n_nodes, const int* d_leaves, const int* d_root,
                                       const int* d_offsets, int* d_indices, float* d_d2,
                                       grace_stream stream)
{
    GRACE_REQUIRE(elems_per_point >= 3 && elems_per_point <= 16, "range_neighbours: elements per point must be 3..16");
    GRACE_REQUIRE(n_points < (size_t(1) << 31), "range_neighbours: too many points");
    if (n_points == 0) return GRACE_OK;   // (before the output checks: a caller's empty arrays may be null)
    GRACE_REQUIRE(d_offsets, "range_neighbours: null offsets");
    GRACE_REQUIRE(d_indices || d_d2, "range_neighbours: no output");
    RangeArgs a = {};
    GRACE_TRY(range_common(a, d_points, n_points, d_radii, radius, d_spheres, n_spheres,
                           d_nodes, n_nodes, d_leaves, d_root));
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    a.offsets = d_offsets;
    a.indices = d_indices;
    a.d2 = d_d2;
    const hipStream_t stream_ = as_stream(stream);
    return range_run(a, *ts, d_points, n_points, elems_per_point, stream_,
                     [&](RangeArgs w, size_t waves) -> grace_status {
        return launch_walk(w, RG_FILL, GRACE_SPH_KERNEL_CUBIC, 0, waves, stream_);
    });
}

} // extern "C"
