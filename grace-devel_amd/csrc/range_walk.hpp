// The fixed-radius packet walk shared by the range queries (range.hip) and the friends-of-friends
// link kernel (fof.hip): one wave owns up to 64 query points of one Morton cell
// (point_packets.hpp) and walks the ALBVH against the union of its lanes' query boxes; what a lane
// does with a centre in range is the including file's Visitor.  Each including translation unit
// gets its own copies (internal linkage).
//
// Order.  A node's left child covers the lower index range (albvh.hip: the left child spans leaves
// first .. j, the right one j + 1 .. last), so left child first visits the leaves, and with them
// the primitives, in ascending tree index: lists and running sums fall out of the walk in order.
//
// Stack.  128 entries, one per lane of two registers (the trace's convention), and a second word
// per entry: an entry is an inner node, or a RANGE of primitives [lo, lo + n) -- a leaf whose box
// met the union box.  A range pushed directly under a range that starts where it ends is merged
// into it.  The ALBVH of coincident points is a spine of leaves deeper than the stack; whichever
// side its leaves hang on, they are popped at once (left) or merged into the waiting range
// (right), so the spine never grows the stack.  Overflow is reported through the status word.
//
// A range is swept in 64-aligned clusters: each lane tests one centre against the union box, a
// ballot compacts the survivors {x, y, z, j} (and whatever the visitor stages beside them) into LDS
// in ascending j, and every lane tests them all against its own point: one compare, then the
// visitor's hit().
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
//
// A Visitor provides
//   void begin(bool in_range, bool on, uint32_t src, float r)   before the walk: the lane's point
//        (src: its index in the caller's order; off lanes and lanes beyond the packet too)
//   bool clip(int& lo, int& hi)      a popped range of primitives [lo, hi): may narrow it; false
//                                    skips it (wave-uniform; hi > lo must hold where it returns true)
//   void stage(int pos, int j)       the lane's centre j survived the cull and is record `pos`
//   void hit(int pos, const float4& rec, float d2)   record `pos` = {x, y, z, bits of j} is in range
//   void finish(uint32_t src)        after the walk, lanes of the packet only
#pragma once

#include "point_packets.hpp"

namespace {

constexpr int RG_BLOCK = 256;
constexpr int RG_WAVES = RG_BLOCK / 64;
constexpr int RG_STACK = 128;
constexpr float RG_SLACK = 9.5367431640625e-07f;     // 2^-20
constexpr float RG_FLOOR = 8.673617379884035e-19f;   // 2^-60

// What the walk itself reads: the packets, the query points with their radii, and the scene.
struct WalkArgs {
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

// One packet.  s_rec: the wave's 64 survivor records.
template <typename Visitor>
__device__ __forceinline__ void walk_packet(const WalkArgs& a, const int packet, const int lane, float4* s_rec,
                                            Visitor& v)
{
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

    v.begin(in_range, on, src, r);

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
        int r_lo = idx, r_hi = idx + n_prims;
        if (!v.clip(r_lo, r_hi)) continue;
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
                v.stage(pos, pc);
            }
            wave_sync();
            for (int j = 0; j < n_surv; ++j) {
                const float4 rec = s_rec[j];
                const float dx = px - rec.x, dy = py - rec.y, dz = pz - rec.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 <= R2) v.hit(j, rec, d2);
            }
            wave_sync();
        }
    }

    if (overflow && lane == 0) atomicMax(a.status, int(GRACE_STACK_OVERFLOW));
    if (!in_range) return;
    v.finish(src);
}

// The checks every entry point over this walk shares (before anything is enqueued), and the
// scene's fields.
grace_status walk_scene(WalkArgs& a, const float* d_radii, float radius, const float* d_spheres, size_t n_spheres,
                        const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root)
{
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
// Args: WalkArgs or a struct derived from it; walks(args, max_packets) launches.
template <typename Args, typename Walks>
grace_status walk_run(Args a, grace_hip::TraceState& ts, const float* d_points, size_t n_points, int stride,
                      hipStream_t stream, Walks walks)
{
    grace_hip::FrameGuard frame;
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
