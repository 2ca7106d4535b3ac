// The packet walk under every point query (neighbours.hip, interpolate.hip, and range_walk.hpp
// for range.hip, fof.hip and pairs.hip): one wave owns up to 64 Morton-sorted points of one Morton
// cell (point_packets.hpp) and walks the ALBVH against a box that holds all its lanes' queries.
// Here are the pieces each of them used to carry: the argument blocks, the lane's point, the
// packet stack, the cluster sweep, the box tests, the pieces of the periodic variants, and on the
// host the scene checks and the "packets, then walks" sequence.  What is tested, in which order
// the children go and what a lane does with a survivor is the including file's.  Everything on the
// device is forceinlined and holds no state its caller does not use (internal linkage: a copy per
// including unit).
#pragma once

#include "point_packets.hpp"

#include <cmath>
#include <limits>
#include <type_traits>

namespace {

constexpr int PW_BLOCK = 256;
constexpr int PW_WAVES = PW_BLOCK / 64;
constexpr int PW_STACK = 128;
constexpr float PW_SLACK = 9.5367431640625e-07f;     // 2^-20
constexpr float PW_FLOOR = 8.673617379884035e-19f;   // 2^-60

// What every walk reads: the packets of the query points, and the scene.  A kernel's argument
// struct derives from them.
struct PacketPoints {
    const float* points;         // n records of `stride` floats, visited in the order `perm`
    int stride;
    const uint32_t* perm;        // sorted position -> point index
    const uint32_t* starts;      // packet p: sorted points [starts[p], starts[p + 1])
    const uint32_t* n_starts;    // number of packets (device)
};
struct PacketScene {
    const float4* spheres;
    const float4* nodes;         // 4 x float4 per node
    int n_nodes;
    const int4* leaves;
    const int* root;
    int* status;
};

// A kernel's prologue: the wave's lane, its slot in the block and its packet (the grid is
// launched for the bound n / 64 + cells; surplus waves have packet >= *n_starts and exit).
struct PacketWave {
    int lane, wv, packet;
};
__device__ __forceinline__ PacketWave packet_wave()
{
    const int wv = threadIdx.x >> 6;
    return { int(threadIdx.x & 63), wv, int(blockIdx.x) * PW_WAVES + wv };
}

// The lane's point of its packet: src is its index in the caller's order (0 beyond the packet's
// end, where in_range is false and the coordinates are point 0's).
struct PacketPoint {
    bool in_range;
    uint32_t src;
    float px, py, pz;
};
__device__ __forceinline__ PacketPoint load_point(const PacketPoints& a, const int packet, const int lane)
{
    const uint32_t first = a.starts[packet], end = a.starts[packet + 1];
    const uint32_t spos = first + uint32_t(lane);
    const bool in_range = spos < end;
    const uint32_t src = in_range ? a.perm[spos] : 0u;
    const float* q = a.points + size_t(src) * a.stride;
    return { in_range, src, q[0], q[1], q[2] };
}

// Widening.  A lane that accepts d2 <= D (fp32: its squared radius, or its k-th best d2) has
// fl(dx*dx) <= D, since the rounded sums of non-negative terms never fall below a term, so the
// exact |p - x| per component is below sqrt(D) (1 + 2^-22).  r = widened_radius(D) exceeds that
// (v_sqrt is within 1 ulp; the 2^-60 covers D that underflowed to 0 or a flushed denormal), and the
// rounded bounds p - r, p + r are then moved out by 2^-20 of themselves, far more than their
// rounding.  Node boxes built with any H >= 0 contain their centres exactly.  So pruning against
// the union of these boxes only drops centres whose d2 is strictly above the lane's D.
__device__ __forceinline__ float widened_radius(const float D)
{
    return __builtin_amdgcn_sqrtf(D) * (1.0f + PW_SLACK) + PW_FLOOR;   // D = +inf: +inf
}

// The lane's query box on one axis (off lanes: empty, +inf / -inf).
__device__ __forceinline__ void query_bounds(const float p, const float r, const bool on, float& lo, float& hi)
{
    const float l = p - r, u = p + r;
    lo = on ? l - fabsf(l) * PW_SLACK : __int_as_float(0x7f800000);
    hi = on ? u + fabsf(u) * PW_SLACK : __int_as_float(0xff800000);
}

__device__ __forceinline__ bool overlaps(const float lo, const float hi, const float ulo, const float uhi)
{
    return lo <= uhi && hi >= ulo;
}

// [lo, hi] moved out by 2^-20 of each bound overlaps [plo, phi] (NaN: no).
__device__ __forceinline__ bool overlaps_widened(const float lo, const float hi, const float plo, const float phi)
{
    return overlaps(lo - fabsf(lo) * PW_SLACK, hi + fabsf(hi) * PW_SLACK, plo, phi);
}

// GRACE_STACK_OVERFLOW is the largest status code, so the maximum leaves the word a plain store
// would, in every interleaving with the other writers of the status.
__device__ __forceinline__ void report_overflow(const bool overflow, const int lane, int* status)
{
    if (overflow && lane == 0) atomicMax(status, int(GRACE_STACK_OVERFLOW));
}

// The packet stack: 128 entries, entry e in lane (e & 63) of stk0 (e < 64) or stk1 (the trace's
// convention), popped with a readlane; overflow is reported through the status word.  An entry is
// one word, a node index (inner or leaf).  range_walk.hpp keeps the same convention with a second
// word per entry.
struct PacketStack {
    int stk0 = 0, stk1 = 0, sp = -1;
    bool overflow = false;

    __device__ __forceinline__ bool empty() const { return sp < 0; }
    __device__ __forceinline__ void push(const int lane, const int value)
    {
        if (sp >= PW_STACK - 1) { overflow = true; return; }   // bounds check before every push
        ++sp;
        // (selects, no branch on sp: lane < 64, so at most one of the two compares is true; stores to
        // members under a branch become one dynamically indexed store and put the object in scratch)
        stk0 = lane == sp ? value : stk0;
        stk1 = lane == sp - 64 ? value : stk1;
    }
    __device__ __forceinline__ int pop()
    {
        const int value = sp < 64 ? __builtin_amdgcn_readlane(stk0, sp) : __builtin_amdgcn_readlane(stk1, sp - 64);
        --sp;
        return value;
    }
    __device__ __forceinline__ void report(const int lane, int* status) const { report_overflow(overflow, lane, status); }
};

// The cluster sweep of the primitives [r_lo, r_hi) in 64-aligned clusters: each lane
// loads one candidate; keep(in, s) is the cull (in: the lane's candidate is inside the range; the
// load is clamped into it); a ballot compacts the survivors, in ascending index: stage(pos, s, j)
// puts the lane's candidate j into the wave's LDS as record `pos`; then every lane runs
// body(cl, n_surv) over the records 0 .. n_surv - 1 of cluster cl.  Wave-uniform throughout.
template <typename Keep, typename Stage, typename Body>
__device__ __forceinline__ void sweep_clusters(const float4* spheres, const int r_lo, const int r_hi, const int lane,
                                               Keep keep, Stage stage, Body body)
{
    for (int cl = r_lo >> 6; cl <= (r_hi - 1) >> 6; ++cl) {
        const int pj = (cl << 6) + lane;
        const bool in = pj >= r_lo && pj < r_hi;
        const float4 s = spheres[min(max(pj, r_lo), r_hi - 1)];
        const bool kept = keep(in, s);
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(kept);
        if (mask == 0ull) continue;
        if (kept)
            stage(__builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0)), s, pj);
        wave_sync();
        body(cl, __builtin_popcountll(mask));
        wave_sync();
    }
}

// ---- periodic boxes (range_walk.hpp states the separation and the rounding argument) ----

// A periodic box: per axis the period L (0: open) and h = fl(0.5 L) (open: +inf).
struct WalkPeriod {
    float L[3];
    float h[3];
};

// Args with a period beside them: what the periodic kernels take (the including file picks its walk).
template <typename Base>
struct Periodic : Base {
    WalkPeriod per;
};
template <typename T> struct is_periodic : std::false_type {};
template <typename Base> struct is_periodic<Periodic<Base>> : std::true_type {};

// The union box on one axis and its images shifted by -L and +L, rounded outward (wave-uniform).
struct AxisImages {
    float lo, hi, mlo, mhi, plo, phi;
    __device__ __forceinline__ bool meets(const float blo, const float bhi) const
    {
        return overlaps(blo, bhi, lo, hi) || overlaps(blo, bhi, mlo, mhi) || overlaps(blo, bhi, plo, phi);
    }
    __device__ __forceinline__ bool direct(const float x) const { return x >= lo && x <= hi; }
    __device__ __forceinline__ bool holds(const float x) const
    {
        return direct(x) || (x >= mlo && x <= mhi) || (x >= plo && x <= phi);
    }
};

__device__ __forceinline__ float uniform(const float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

__device__ __forceinline__ AxisImages axis_images(const float ulo, const float uhi, const float L)
{
    const float ml = ulo - L, mh = uhi - L, pl = ulo + L, ph = uhi + L;
    return { ulo, uhi, uniform(ml - fabsf(ml) * PW_SLACK), uniform(mh + fabsf(mh) * PW_SLACK),
             uniform(pl - fabsf(pl) * PW_SLACK), uniform(ph + fabsf(ph) * PW_SLACK) };
}

// One component of the periodic separation: at most one wrap (open axis: h = +inf, none).
__device__ __forceinline__ float wrap_sep(const float d, const float L, const float h)
{
    return d > h ? d - L : (d < -h ? d + L : d);
}

// ---- host ----

// The scene checks every entry point over a walk shares (before anything is enqueued; the
// messages are the including function's, with its file and line), then the scene's fields.
// family: the message prefix, a literal ("neighbours", "range query", "interpolate").
// leaf_root: the walk takes a tree whose root is a leaf (no nodes).
#define PACKET_SCENE(s, family, leaf_root, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root)             \
    do {                                                                                                         \
        GRACE_REQUIRE((d_spheres) && (d_leaves) && (d_root) && ((d_nodes) || ((leaf_root) && (n_nodes) == 0)),   \
                      family ": null scene pointer");                                                            \
        GRACE_REQUIRE(((leaf_root) || (n_nodes) >= 1) && (n_nodes) < (size_t(1) << 30), family ": bad node count"); \
        GRACE_REQUIRE((n_spheres) > 0 && (n_spheres) < (size_t(1) << 31), family ": bad sphere count");          \
        (s).spheres = reinterpret_cast<const float4*>(d_spheres);                                                \
        (s).nodes = reinterpret_cast<const float4*>(d_nodes);                                                    \
        (s).n_nodes = int(n_nodes);                                                                              \
        (s).leaves = reinterpret_cast<const int4*>(d_leaves);                                                    \
        (s).root = d_root;                                                                                       \
    } while (0)

// A caller's period (three host floats) as the walk takes it, checked before anything is enqueued.
// radius: the call's host radius, which must not exceed half a period (NULL: the radii are per point
// and the walk switches such points off, or the walk has no host radius: neighbours, interpolation).
grace_status walk_period(WalkPeriod& per, const float* h_period3, const float* radius)
{
    GRACE_REQUIRE(h_period3, "periodic query: null period");
    for (int d = 0; d < 3; ++d) {
        const float L = h_period3[d];
        GRACE_REQUIRE(std::isfinite(L) && L >= 0.0f, "periodic query: a period must be finite and not negative (0: open)");
        per.L[d] = L > 0.0f ? L : 0.0f;
        per.h[d] = L > 0.0f ? 0.5f * L : std::numeric_limits<float>::infinity();
        GRACE_REQUIRE(!radius || !(*radius > per.h[d]), "periodic query: the radius exceeds half a period");
    }
    return GRACE_OK;
}

// The status word, then the launches of one call inside the timing bracket.
template <typename Args, typename Launches>
grace_status timed_walks(Args& a, grace_hip::TraceState& ts, hipStream_t stream, Launches launches)
{
    GRACE_TRY(grace_hip::ensure_status(ts, stream));
    a.status = ts.status;
    return grace_hip::timed(ts, stream, launches);
}

// Keys against the root box, sort, packet starts, then the walks of one call (timed together).
// Args: derived from PacketPoints and PacketScene; walks(args, max_packets) launches.
template <typename Args, typename Walks>
grace_status packet_run(Args a, grace_hip::TraceState& ts, const float* d_points, size_t n_points, int stride,
                        hipStream_t stream, Walks walks)
{
    grace_hip::FrameGuard frame;
    grace_hip::PointPackets pk;
    GRACE_TRY(grace_hip::point_packets(frame, d_points, n_points, stride, a.nodes, a.n_nodes, a.root, stream, pk));
    a.points = d_points;
    a.stride = stride;
    a.perm = pk.perm;
    a.starts = pk.starts;
    a.n_starts = pk.n_starts;
    return timed_walks(a, ts, stream, [&] { return walks(a, pk.max_packets); });
}

} // namespace
