// Tree gravity (grace_gravity_moments_f4, grace_gravity_points_f4): potentials and accelerations
// at points from the BVH, a Barnes-Hut walk with monopoles of the inner nodes.  An extension the
// reference lacks; the moments, the acceptance test, the pair term and the order of the fp64 sums
// are stated exactly in include/grace_hip.h.
//
// Moments.  One thread per leaf sums its primitives in fp64, then climbs: it stores what it carries
// for the node it stands on, releases at agent scope, and adds one to the parent's arrival
// counter.  The first to arrive leaves; the second acquires at agent scope, reads what its sibling
// stored, combines left + right in that order, writes the parent's record and goes on from there.
// Nobody waits for anybody: there is no loop that polls, and the climb itself is bounded by the
// node count.  The node layout holds no parents, so a kernel before the climb writes them; a
// child index outside the tree is ignored there, and a node that is reached a third time (a
// tree that is none) ends the thread, so nothing is indexed out of bounds whatever the arrays hold.
//
// Walk.  packet_walk.hpp's packets and prologue, and range_walk.hpp's stack -- two words per
// entry, an inner node or a merged range of primitives, left child first, so everything is met in
// ascending primitive index (the words and the push are restated here as they are local to that
// walk).  The wave visits the union of what its lanes need.  Each lane keeps skip_hi, the end of
// the span of the last node it accepted: a lane is live at a node iff it is on and the node's span
// starts at or after skip_hi -- the nodes below an accepted one start before it, everything after
// them does not, and spans are met in ascending order.  Live lanes evaluate acceptance; accepting
// ones add the monopole and move skip_hi; if a live lane rejected, both children are pushed.  A
// range is swept in 64-aligned clusters: every lane stages one {x, y, z, m} in the wave's LDS
// records, and every lane takes record j iff j >= skip_hi.  So each lane adds exactly the terms of
// its own recursion, in its order, into four fp64 accumulators.
//
// Arithmetic.  fp32, every operation rounded (-ffp-contract=off, correctly rounded divide and
// sqrt): 1.0f / sqrtf(s) as written, no reciprocal-square-root instruction, so that a NumPy
// restatement reproduces every bit.  LDS: 64 records of 16 bytes per wave, 4 KiB per block.
//
// Gravity within groups (grace_gravity_group_moments_f4, grace_gravity_group_points_f4): every point
// feels the particles that carry its own label, in one walk of the whole-scene tree.  Both kernels
// are compile-time variants of the ones above.  Moments: a leaf skips its unlabelled primitives
// (label < 0), and the partial record carries the smallest and largest label below beside the sums;
// spans still cover every primitive.  Walk: a lane is live at a node iff, in addition, its label
// lies in the node's label range; a node is a monopole only where that range is one label; the leaf
// sweep stages each candidate's label beside its record (64 more words of LDS per wave) and a lane
// takes record j iff j >= skip_hi and the staged label is its own.  Label ranges nest, so a lane
// a node's range keeps out is kept out of everything below it and needs no skip_hi of its own.
#include "packet_walk.hpp"

#include <cmath>

using namespace grace_hip;

namespace {

constexpr int GM_BLOCK = 256;

// What a thread of the climb carries for the node or leaf it stands on.
struct alignas(16) Partial {
    double M, Sx, Sy, Sz;
    float lo_x, lo_y, lo_z;
    int span_lo;
    float hi_x, hi_y, hi_z;
    int span_hi;
};
static_assert(sizeof(Partial) == 64, "one 64-byte record per node or leaf");

// ... and with labels: the smallest and largest label >= 0 below ({INT32_MAX, -1}: none).
struct alignas(16) GroupPartial : Partial {
    int lab_lo, lab_hi;
};
static_assert(sizeof(GroupPartial) == 80, "the partial record and two ints, padded to 16 bytes");

// parent[child] = node, children indexed as the nodes do: inner nodes first, leaf l at n_nodes + l.
__global__ __launch_bounds__(GM_BLOCK) void gravity_parents_kernel(const float4* __restrict__ nodes, int n_nodes,
                                                                   int* __restrict__ parent)
{
    const int i = blockIdx.x * GM_BLOCK + threadIdx.x;
    if (i >= n_nodes) return;
    const float4 n0 = nodes[4 * size_t(i)];
    const int l = __float_as_int(n0.x), r = __float_as_int(n0.y);
    const int n_all = 2 * n_nodes + 1;
    if (l >= 0 && l < n_all) parent[l] = i;
    if (r >= 0 && r < n_all) parent[r] = i;
}

__device__ __forceinline__ Partial combine(const Partial& l, const Partial& r)
{
    Partial p;
    p.M = l.M + r.M;
    p.Sx = l.Sx + r.Sx;
    p.Sy = l.Sy + r.Sy;
    p.Sz = l.Sz + r.Sz;
    p.lo_x = fminf(l.lo_x, r.lo_x); p.lo_y = fminf(l.lo_y, r.lo_y); p.lo_z = fminf(l.lo_z, r.lo_z);
    p.hi_x = fmaxf(l.hi_x, r.hi_x); p.hi_y = fmaxf(l.hi_y, r.hi_y); p.hi_z = fmaxf(l.hi_z, r.hi_z);
    p.span_lo = min(l.span_lo, r.span_lo);
    p.span_hi = max(l.span_hi, r.span_hi);
    return p;
}

__device__ __forceinline__ GroupPartial combine(const GroupPartial& l, const GroupPartial& r)
{
    GroupPartial p;
    static_cast<Partial&>(p) = combine(static_cast<const Partial&>(l), static_cast<const Partial&>(r));
    p.lab_lo = min(l.lab_lo, r.lab_lo);
    p.lab_hi = max(l.lab_hi, r.lab_hi);
    return p;
}

// P: Partial (labels and label_ranges unused, null) or GroupPartial.
template <typename P>
__global__ __launch_bounds__(GM_BLOCK) void gravity_moments_kernel(const float4* __restrict__ spheres, int n_spheres,
                                                                   const float* __restrict__ masses,
                                                                   const int* __restrict__ labels,
                                                                   const float4* __restrict__ nodes, int n_nodes,
                                                                   const int4* __restrict__ leaves,
                                                                   const int* __restrict__ parent, int* counters,
                                                                   P* partials, float4* __restrict__ moments,
                                                                   int2* __restrict__ label_ranges)
{
    constexpr bool GROUPS = std::is_same<P, GroupPartial>::value;
    const int leaf = blockIdx.x * GM_BLOCK + threadIdx.x;
    if (leaf > n_nodes) return;                                  // n_nodes + 1 leaves
    const int4 lf = leaves[leaf];
    const int first = min(max(lf.x, 0), n_spheres);
    const int end = first + min(max(lf.y, 0), n_spheres - first);   // inside [0, n_spheres] whatever the leaf holds
    P mine;
    mine.M = mine.Sx = mine.Sy = mine.Sz = 0.0;
    mine.lo_x = mine.lo_y = mine.lo_z = __int_as_float(0x7f800000);
    mine.hi_x = mine.hi_y = mine.hi_z = __int_as_float(0xff800000);
    mine.span_lo = first;
    mine.span_hi = end;
    if constexpr (GROUPS) { mine.lab_lo = INT32_MAX; mine.lab_hi = -1; }
    for (int j = first; j < end; ++j) {
        if constexpr (GROUPS) {
            const int lab = labels[j];
            if (lab < 0) continue;                               // in no group: absent, but it keeps its index
            mine.lab_lo = min(mine.lab_lo, lab);
            mine.lab_hi = max(mine.lab_hi, lab);
        }
        const float4 s = spheres[j];
        const double m = double(masses[j]);
        mine.M += m;
        mine.Sx += m * double(s.x);
        mine.Sy += m * double(s.y);
        mine.Sz += m * double(s.z);
        mine.lo_x = fminf(mine.lo_x, s.x); mine.lo_y = fminf(mine.lo_y, s.y); mine.lo_z = fminf(mine.lo_z, s.z);
        mine.hi_x = fmaxf(mine.hi_x, s.x); mine.hi_y = fmaxf(mine.hi_y, s.y); mine.hi_z = fmaxf(mine.hi_z, s.z);
    }
    int at = n_nodes + leaf;
    for (int step = 0; step < n_nodes; ++step) {                 // a path to the root has at most n_nodes nodes
        const int up = parent[at];
        if (up < 0 || up >= n_nodes) return;                     // the root (or a leaf nothing points to)
        partials[at] = mine;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const int before = __hip_atomic_fetch_add(counters + up, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before != 1) return;                                 // first to arrive: the sibling's thread goes on
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const float4 n0 = nodes[4 * size_t(up)];
        const int l = __float_as_int(n0.x), r = __float_as_int(n0.y);
        const int other = l == at ? r : l;
        if (other < 0 || other > 2 * n_nodes || parent[other] != up) return;   // not a tree
        const P theirs = partials[other];
        mine = l == at ? combine(mine, theirs) : combine(theirs, mine);
        float cx = mine.lo_x, cy = mine.lo_y, cz = mine.lo_z;
        if (mine.M != 0.0) {
            cx = float(mine.Sx / mine.M);
            cy = float(mine.Sy / mine.M);
            cz = float(mine.Sz / mine.M);
        }
        float4* rec = moments + 3 * size_t(up);
        rec[0] = make_float4(cx, cy, cz, float(mine.M));
        rec[1] = make_float4(mine.lo_x, mine.lo_y, mine.lo_z, __int_as_float(mine.span_lo));
        rec[2] = make_float4(mine.hi_x, mine.hi_y, mine.hi_z, __int_as_float(mine.span_hi));
        if constexpr (GROUPS) label_ranges[up] = make_int2(mine.lab_lo, mine.lab_hi);
        at = up;
    }
}

struct GravityArgs : PacketPoints, PacketScene {
    int n_spheres;
    const float* masses;
    const float4* moments;       // 3 x float4 per inner node
    float theta2, eps2;
    double* out;                 // {a_x, a_y, a_z, phi} per point, or null
    int* counts;                 // {node terms, particle terms} per point, or null
};

// ... within groups: a label per primitive and per point, a label range per inner node.
struct GroupGravityArgs : GravityArgs {
    const int* labels;           // per primitive, tree order; < 0: in no group
    const int2* label_ranges;    // {lab_lo, lab_hi} per inner node
    const int* point_labels;     // per point, the caller's order
};

// The lane's four running sums and the pair term added to them.
struct GravitySums {
    double ax = 0.0, ay = 0.0, az = 0.0, pot = 0.0;

    __device__ __forceinline__ void add(const float px, const float py, const float pz, const float x, const float y,
                                        const float z, const float m, const float eps2)
    {
        const float dx = x - px, dy = y - py, dz = z - pz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 == 0.0f) return;                                  // the self pair and coincident centres
        const float s = d2 + eps2;
        const float ir = 1.0f / sqrtf(s);
        const float u = m * ir;
        const float f = m * ((ir * ir) * ir);
        ax += double(f * dx);
        ay += double(f * dy);
        az += double(f * dz);
        pot += double(u);
    }
};

// Args: GravityArgs, or GroupGravityArgs for the walk within groups.
template <typename Args>
__global__ __launch_bounds__(PW_BLOCK) void gravity_kernel(const Args a)
{
    constexpr bool GROUPS = std::is_same<Args, GroupGravityArgs>::value;
    __shared__ float4 s_rec_all[PW_WAVES][64];
    __shared__ int s_lab_all[GROUPS ? PW_WAVES : 1][64];         // (the open walk never names it: no LDS there)
    const PacketWave w = packet_wave();
    const int lane = w.lane, packet = w.packet;
    if (packet >= int(*a.n_starts)) return;
    float4* s_rec = s_rec_all[w.wv];

    const PacketPoint pt = load_point(a, packet, lane);
    const float px = pt.px, py = pt.py, pz = pt.pz;
    bool on = pt.in_range && isfinite(px) && isfinite(py) && isfinite(pz);
    // the lane's label, and the range of the labels of the wave's on-lanes ({INT32_MAX, -1}: none is on)
    int my_label = -1, wave_lab_lo = INT32_MAX, wave_lab_hi = -1;
    int* s_lab = nullptr;
    if constexpr (GROUPS) {
        s_lab = s_lab_all[w.wv];
        if (pt.in_range) my_label = a.point_labels[pt.src];
        on = on && my_label >= 0;
        wave_lab_lo = on ? my_label : INT32_MAX;
        wave_lab_hi = on ? my_label : -1;
        for (int off = 32; off > 0; off >>= 1) {
            wave_lab_lo = min(wave_lab_lo, __shfl_xor(wave_lab_lo, off));
            wave_lab_hi = max(wave_lab_hi, __shfl_xor(wave_lab_hi, off));
        }
    }

    GravitySums sum;
    int skip_hi = 0, n_node_terms = 0, n_particle_terms = 0;

    // ---- range_walk.hpp's stack: entry e in lane (e & 63) of stk0 / cnt0 (e < 64) or stk1 / cnt1.
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
    auto push = [&](const int idx) {
        if (idx < 0 || idx > 2 * a.n_nodes) return;              // not an index of this tree
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
        if (sp >= PW_STACK - 1) { overflow = true; return; }     // bounds check before every push
        ++sp;
        set_top(value, count);
    };
    push(*a.root);

    while (sp >= 0) {
        int idx, n_prims;
        top(idx, n_prims);
        --sp;
        if (n_prims == 0) {
            const float4* rec = a.moments + 3 * size_t(idx);
            const float4 cm = rec[0], lo = rec[1], hi = rec[2];
            const int span_lo = __float_as_int(lo.w), span_hi = __float_as_int(hi.w);
            bool live = on && span_lo >= skip_hi;
            bool pure = true;
            if constexpr (GROUPS) {
                const int2 lr = a.label_ranges[idx];
                live = live && lr.x <= my_label && my_label <= lr.y;
                pure = lr.x == lr.y;                             // two or more labels: never a monopole
            }
            if (__builtin_amdgcn_ballot_w64(live) == 0ull) continue;
            const float ex = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.0f);
            const float ey = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.0f);
            const float ez = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.0f);
            const float d2min = (ex * ex + ey * ey) + ez * ez;
            const float size = fmaxf(fmaxf(hi.x - lo.x, hi.y - lo.y), hi.z - lo.z);
            const float size2 = size * size;
            const bool accept = live && pure && size2 < a.theta2 * d2min;
            if (accept) {
                sum.add(px, py, pz, cm.x, cm.y, cm.z, cm.w, a.eps2);
                ++n_node_terms;
                skip_hi = span_hi;
            }
            if (__builtin_amdgcn_ballot_w64(live && !accept) == 0ull) continue;
            const float4 n0 = a.nodes[4 * size_t(idx)];
            push(__float_as_int(n0.y));
            push(__float_as_int(n0.x));                          // popped first: ascending primitive order
            continue;
        }
        const int r_lo = max(idx, 0), r_hi = min(idx + n_prims, a.n_spheres);
        for (int cl = r_lo >> 6; cl <= (r_hi - 1) >> 6; ++cl) {
            const int j_lo = max(cl << 6, r_lo), j_hi = min((cl << 6) + 64, r_hi);
            if (__builtin_amdgcn_ballot_w64(on && j_hi > skip_hi) == 0ull) continue;
            const int pj = (cl << 6) + lane;
            if constexpr (GROUPS) {
                // the candidate's label (-1 outside the range); no on-lane carries a label outside the
                // wave's range, so a cluster without a candidate inside it holds no lane's term
                const int cand = pj >= j_lo && pj < j_hi ? a.labels[pj] : -1;
                if (__builtin_amdgcn_ballot_w64(cand >= wave_lab_lo && cand <= wave_lab_hi) == 0ull) continue;
                s_lab[lane] = cand;
            }
            if (pj >= j_lo && pj < j_hi) {
                const float4 s = a.spheres[pj];
                s_rec[lane] = make_float4(s.x, s.y, s.z, a.masses[pj]);
            }
            wave_sync();
            if (on) {
                if constexpr (GROUPS) {
                    for (int j = max(j_lo, skip_hi); j < j_hi; ++j) {
                        if (s_lab[j & 63] != my_label) continue;
                        const float4 r = s_rec[j & 63];
                        sum.add(px, py, pz, r.x, r.y, r.z, r.w, a.eps2);
                        ++n_particle_terms;
                    }
                } else {
                    for (int j = max(j_lo, skip_hi); j < j_hi; ++j) {
                        const float4 r = s_rec[j & 63];
                        sum.add(px, py, pz, r.x, r.y, r.z, r.w, a.eps2);
                    }
                    n_particle_terms += max(j_hi - max(j_lo, skip_hi), 0);
                }
            }
            wave_sync();
        }
    }

    report_overflow(overflow, lane, a.status);
    if (!pt.in_range) return;
    if (a.out) {
        double* o = a.out + 4 * size_t(pt.src);
        o[0] = sum.ax; o[1] = sum.ay; o[2] = sum.az; o[3] = on ? -sum.pot : 0.0;   // off points: +0 throughout
    }
    if (a.counts) {
        a.counts[2 * size_t(pt.src)] = n_node_terms;
        a.counts[2 * size_t(pt.src) + 1] = n_particle_terms;
    }
}

// The parents, then the climb, in the context workspace (the scene and the pointers are checked by the caller).
template <typename P>
grace_status moments_run(const PacketScene& s, size_t n_spheres, size_t n_nodes, const float* d_masses,
                         const int* d_labels, float* d_moments, int* d_label_ranges, hipStream_t stream_)
{
    const size_t n_all = 2 * n_nodes + 1;
    FrameGuard frame;
    GRACE_TRY(frame.begin(Workspace::aligned(n_all * sizeof(int)) + Workspace::aligned(n_nodes * sizeof(int))
                          + Workspace::aligned(n_all * sizeof(P)), stream_));
    int* parent = Workspace::take<int>(n_all);
    int* counters = Workspace::take<int>(n_nodes);
    P* partials = Workspace::take<P>(n_all);
    GRACE_TRY_HIP(hipMemsetAsync(parent, 0xff, n_all * sizeof(int), stream_));
    GRACE_TRY_HIP(hipMemsetAsync(counters, 0, n_nodes * sizeof(int), stream_));
    gravity_parents_kernel<<<ceil_div(n_nodes, GM_BLOCK), GM_BLOCK, 0, stream_>>>(s.nodes, s.n_nodes, parent);
    GRACE_CHECK_LAUNCH();
    gravity_moments_kernel<P><<<ceil_div(n_nodes + 1, GM_BLOCK), GM_BLOCK, 0, stream_>>>(
        s.spheres, int(n_spheres), d_masses, d_labels, s.nodes, s.n_nodes, s.leaves, parent, counters, partials,
        reinterpret_cast<float4*>(d_moments), reinterpret_cast<int2*>(d_label_ranges));
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

// What both walks check and set, before anything is enqueued.
#define GRAVITY_WALK_ARGS(a)                                                                                      \
    do {                                                                                                          \
        GRACE_REQUIRE(elems_per_point >= 3 && elems_per_point <= 16, "gravity: elements per point must be 3..16"); \
        GRACE_REQUIRE(n_points < (size_t(1) << 31), "gravity: too many points");                                  \
        GRACE_REQUIRE(std::isfinite(theta) && theta >= 0.0f, "gravity: theta must be finite and not negative");    \
        GRACE_REQUIRE(std::isfinite(eps) && eps >= 0.0f, "gravity: eps must be finite and not negative");         \
        if (n_points == 0) return GRACE_OK;                      /* (a caller's empty arrays may be null) */      \
        GRACE_REQUIRE(d_out || d_counts, "gravity: no output");                                                   \
        GRACE_REQUIRE(d_points, "gravity: null points");                                                          \
        PACKET_SCENE(a, "gravity", true, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root);               \
        GRACE_REQUIRE(d_masses, "gravity: null masses");                                                          \
        GRACE_REQUIRE(d_moments || n_nodes == 0, "gravity: null moments");                                        \
        (a).n_spheres = int(n_spheres);                                                                           \
        (a).masses = d_masses;                                                                                    \
        (a).moments = reinterpret_cast<const float4*>(d_moments);                                                 \
        (a).theta2 = theta * theta;                                                                               \
        (a).eps2 = eps * eps;                                                                                     \
        (a).out = d_out;                                                                                          \
        (a).counts = d_counts;                                                                                    \
    } while (0)

template <typename Args>
grace_status walk_run(const Args& a, const float* d_points, size_t n_points, int elems_per_point, hipStream_t stream_)
{
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    return packet_run(a, *ts, d_points, n_points, elems_per_point, stream_,
                      [&](const Args& w, size_t waves) -> grace_status {
        gravity_kernel<Args><<<ceil_div(waves, PW_WAVES), PW_BLOCK, 0, stream_>>>(w);
        GRACE_CHECK_LAUNCH();
        return GRACE_OK;
    });
}

} // namespace

extern "C" {

grace_status grace_gravity_moments_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                      const int* d_leaves, const int* d_root, const float* d_masses,
                                      float* d_moments, grace_stream stream)
{
    PacketScene s = {};
    PACKET_SCENE(s, "gravity", true, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root);
    GRACE_REQUIRE(d_masses, "gravity_moments: null masses");
    if (n_nodes == 0) return GRACE_OK;                           // the root is a leaf: no records
    GRACE_REQUIRE(d_moments, "gravity_moments: null moments");
    return moments_run<Partial>(s, n_spheres, n_nodes, d_masses, nullptr, d_moments, nullptr, as_stream(stream));
}

grace_status grace_gravity_group_moments_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                            size_t n_nodes, const int* d_leaves, const int* d_root,
                                            const float* d_masses, const int* d_labels, float* d_moments,
                                            int* d_label_ranges, grace_stream stream)
{
    PacketScene s = {};
    PACKET_SCENE(s, "gravity", true, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root);
    GRACE_REQUIRE(d_masses, "gravity_group_moments: null masses");
    GRACE_REQUIRE(d_labels, "gravity_group_moments: null labels");
    if (n_nodes == 0) return GRACE_OK;                           // the root is a leaf: no records
    GRACE_REQUIRE(d_moments, "gravity_group_moments: null moments");
    GRACE_REQUIRE(d_label_ranges, "gravity_group_moments: null label ranges");
    return moments_run<GroupPartial>(s, n_spheres, n_nodes, d_masses, d_labels, d_moments, d_label_ranges,
                                     as_stream(stream));
}

grace_status grace_gravity_points_f4(const float* d_points, size_t n_points, int elems_per_point,
                                     const float* d_spheres, size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                     const int* d_leaves, const int* d_root, const float* d_masses,
                                     const float* d_moments, float theta, float eps, double* d_out, int* d_counts,
                                     grace_stream stream)
{
    GravityArgs a = {};
    GRAVITY_WALK_ARGS(a);
    return walk_run(a, d_points, n_points, elems_per_point, as_stream(stream));
}

grace_status grace_gravity_group_points_f4(const float* d_points, size_t n_points, int elems_per_point,
                                           const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                           size_t n_nodes, const int* d_leaves, const int* d_root,
                                           const float* d_masses, const int* d_labels, const float* d_moments,
                                           const int* d_label_ranges, const int* d_point_labels, float theta,
                                           float eps, double* d_out, int* d_counts, grace_stream stream)
{
    GroupGravityArgs a = {};
    GRAVITY_WALK_ARGS(a);
    GRACE_REQUIRE(d_labels, "gravity_groups: null labels");
    GRACE_REQUIRE(d_point_labels, "gravity_groups: null point labels");
    GRACE_REQUIRE(d_label_ranges || n_nodes == 0, "gravity_groups: null label ranges");
    a.labels = d_labels;
    a.label_ranges = reinterpret_cast<const int2*>(d_label_ranges);
    a.point_labels = d_point_labels;
    return walk_run(a, d_points, n_points, elems_per_point, as_stream(stream));
}

} // extern "C"
