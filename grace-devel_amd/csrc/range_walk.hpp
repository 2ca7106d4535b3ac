// The fixed-radius packet walk shared by the range queries (range.hip), the friends-of-friends link
// kernel (fof.hip) and the pair counts (pairs.hip): packet_walk.hpp's walk against the union of its
// lanes' query boxes, the radii known up front; what a lane does with a centre in range is the
// including file's Visitor.  Each including translation unit gets its own copies (internal linkage).
//
// Order.  A node's left child covers the lower index range (albvh.hip: the left child spans leaves
// first .. j, the right one j + 1 .. last), so left child first visits the leaves, and with them
// the primitives, in ascending tree index: lists and running sums fall out of the walk in order.
//
// Stack.  packet_walk.hpp's convention (128 entries, one per lane of two registers), kept here as
// local words with a second word per entry: an entry is an inner node, or a RANGE of primitives
// [lo, lo + n) -- a leaf whose box met the union box.  A range pushed directly under a range that
// starts where it ends is merged into it.  The ALBVH of coincident points is a spine of leaves
// deeper than the stack; whichever side its leaves hang on, they are popped at once (left) or
// merged into the waiting range (right), so the spine never grows the stack.  (Two-word entries
// as members of packet_walk.hpp's PacketStack cost this walk 3 to 8 % on the MI355X with the
// same survivor loop, so the words and the sweep below stay local to it.)
//
// A range is swept as packet_walk.hpp's sweep_clusters does, the survivors {x, y, z, j} (and
// whatever the visitor stages beside them) in ascending j, and every lane tests them all against
// its own point: one compare, then the visitor's hit().
//
// Widening.  packet_walk.hpp's argument with D := R2 = fl(r * r): pruning only drops centres whose
// d2 is strictly above the lane's R2, so d2 == R2 still gets in, and the result does not depend on
// the tree's H, max_per_leaf or the packets.  Off points (a non-finite coordinate; r negative, NaN
// or +inf) have an empty box and NaN in place of their coordinates and R2: no lane widens for
// them, and no compare is ever true.
//
// Periodic boxes (walk_packet<Visitor, true>, a WalkPeriod: per axis the period L and h = fl(0.5 L),
// exact; an open axis has L = 0 and h = +inf, which no |d| exceeds and no radius, so it needs no
// case of its own).  The pair test wraps each component once, d = fl(p - x); d > h: d = fl(d - L);
// else d < -h: d = fl(d + L), and a lane whose r exceeds h on some axis is off.  Each centre is
// still tested once per lane: the union box stays one box, and per axis a node or a centre passes
// if it meets the box, the box shifted by -L or the box shifted by +L (both rounded outward, once
// per packet, in SGPRs like the box itself).
//   Widening, wrapped.  Let rho = sqrt(D) (1 + 2^-22) < r' = widened_radius(D); a centre in range has a
// wrapped component |dw| <= rho.  No wrap: dw = fl(p - x) and x is in [p - r', p + r'] as before.
// d0 = fl(p - x) > h: if d0 > 2 L then fl(d0 - L) >= L >= 2 r and the square is above D (an on lane
// has r <= h); else d0 is in [L / 2, 2 L] and d0 - L is exact (Sterbenz), so |d0 - L| <= rho and
// d0 <= L + rho < 1.51 L.  The exact p - x is d0 / (1 + e), |e| <= 2^-24, within 1.51 L 2^-24
// (1 + 2^-23) < 2^-23 L of d0, so |x - (p - L)| <= rho + 2^-23 L.  d0 < -h is the mirror image
// about p + L.  That error is absolute in L and may exceed a small r, so on a periodic axis the
// lane's radius is r'' = fl(r' + L 2^-22) (the product is exact; the sum's rounding is below
// 2^-25 L, so r'' > r' + 2^-23 L), and x lies in [p - r'', p + r''] shifted by -+L.  The lane's
// rounded bounds are moved out by 2^-20 of themselves as before; the union's bounds u -+ L are
// rounded once more (2^-24 of the result) and moved out by 2^-20 of the result.  So pruning still
// only drops centres whose wrapped d2 is strictly above the lane's R2.  Over-inclusion costs tests
// only: a centre that passes through an image it is not in range of fails d2 <= R2.
//   Skipping the wrap.  Every on lane's p is inside the union box.  If on every axis the box is no
// wider than h (fl(fl(uhi - ulo) (1 + 2^-20)) <= h, which bounds the exact width) and a cluster's
// survivors all passed through the unshifted box, then |p - x| <= h exactly, rounding is monotone and
// h is a float, so |fl(p - x)| <= h and neither wrap can fire: that cluster is tested without the
// wrap, a wave-uniform branch with the same bits either way.
//   Skipping the images.  The root's box holds every node box and every centre.  A packet whose
// shifted boxes do not meet it on any axis can pass nothing through an image: it tests nodes and
// centres against the box itself, as the open walk does (wave-uniform; most packets of a box that
// the data fills are away from its faces).
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

#include "packet_walk.hpp"

#include <cmath>

namespace {

// What the walk itself reads: the packets, the query points with their radii, and the scene.
struct WalkArgs : PacketPoints, PacketScene {
    const float* radii;          // per point, caller's order, or null: `radius` for all
    float radius;
};

// One packet.  s_rec: the wave's 64 survivor records.  PERIODIC: the separation wraps by `per`.
template <typename Visitor, bool PERIODIC = false>
__device__ __forceinline__ void walk_packet(const WalkArgs& a, const int packet, const int lane, float4* s_rec,
                                            Visitor& v, const WalkPeriod& per = WalkPeriod())
{
    // ---- the packet's points ----
    const PacketPoint pt = load_point(a, packet, lane);
    const bool in_range = pt.in_range;
    const uint32_t src = pt.src;
    float px = pt.px, py = pt.py, pz = pt.pz;
    const float r = a.radii ? a.radii[src] : a.radius;
    bool on = in_range && isfinite(px) && isfinite(py) && isfinite(pz) && r >= 0.0f
        && r < __int_as_float(0x7f800000);
    if constexpr (PERIODIC) on = on && !(r > per.h[0] || r > per.h[1] || r > per.h[2]);
    if (!on) px = py = pz = __int_as_float(0x7fc00000);
    const float R2 = on ? r * r : __int_as_float(0x7fc00000);   // NaN: no d2 <= R2

    // ---- the union of the lanes' query boxes, once ----
    float ulo_x, uhi_x, ulo_y, uhi_y, ulo_z, uhi_z;
    {
        const float rw = widened_radius(R2);
        float lo, hi;
        if constexpr (PERIODIC) {
            query_bounds(px, rw + per.L[0] * 0.25f * PW_SLACK, on, lo, hi); ulo_x = wave_min(lo); uhi_x = wave_max(hi);
            query_bounds(py, rw + per.L[1] * 0.25f * PW_SLACK, on, lo, hi); ulo_y = wave_min(lo); uhi_y = wave_max(hi);
            query_bounds(pz, rw + per.L[2] * 0.25f * PW_SLACK, on, lo, hi); ulo_z = wave_min(lo); uhi_z = wave_max(hi);
        } else {
            query_bounds(px, rw, on, lo, hi); ulo_x = wave_min(lo); uhi_x = wave_max(hi);
            query_bounds(py, rw, on, lo, hi); ulo_y = wave_min(lo); uhi_y = wave_max(hi);
            query_bounds(pz, rw, on, lo, hi); ulo_z = wave_min(lo); uhi_z = wave_max(hi);
        }
    }
    // periodic: the box's images, and whether it is narrow enough for a cluster to skip the wrap
    AxisImages bx = {}, by = {}, bz = {};
    bool narrow = false, images = true;
    if constexpr (PERIODIC) {
        bx = axis_images(ulo_x, uhi_x, per.L[0]);
        by = axis_images(ulo_y, uhi_y, per.L[1]);
        bz = axis_images(ulo_z, uhi_z, per.L[2]);
        narrow = (uhi_x - ulo_x) * (1.0f + PW_SLACK) <= per.h[0] && (uhi_y - ulo_y) * (1.0f + PW_SLACK) <= per.h[1]
            && (uhi_z - ulo_z) * (1.0f + PW_SLACK) <= per.h[2];
        // the root's box (the union of its children's) holds every node box and centre: a packet none
        // of whose images meets it needs the box itself only (a root that is a leaf has no box: images)
        const int rt = *a.root;
        if (rt >= 0 && rt < a.n_nodes) {
            const float4* np = a.nodes + 4 * size_t(rt);
            const float4 L = np[1], R = np[2], Z = np[3];
            const float dlo_x = fminf(L.x, R.x), dhi_x = fmaxf(L.y, R.y), dlo_y = fminf(L.z, R.z), dhi_y = fmaxf(L.w, R.w);
            const float dlo_z = fminf(Z.x, Z.z), dhi_z = fmaxf(Z.y, Z.w);
            images = overlaps(dlo_x, dhi_x, bx.mlo, bx.mhi) || overlaps(dlo_x, dhi_x, bx.plo, bx.phi)
                || overlaps(dlo_y, dhi_y, by.mlo, by.mhi) || overlaps(dlo_y, dhi_y, by.plo, by.phi)
                || overlaps(dlo_z, dhi_z, bz.mlo, bz.mhi) || overlaps(dlo_z, dhi_z, bz.plo, bz.phi);
        }
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
        if (sp >= PW_STACK - 1) { overflow = true; return; }   // bounds check before every push
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
            bool keep, plain = true;
            if (PERIODIC && images) {
                keep = in && bx.holds(s.x) && by.holds(s.y) && bz.holds(s.z);
                const bool image = keep && !(bx.direct(s.x) && by.direct(s.y) && bz.direct(s.z));
                plain = narrow && __builtin_amdgcn_ballot_w64(image) == 0ull;
            } else {
                keep = in && s.x >= ulo_x && s.x <= uhi_x && s.y >= ulo_y && s.y <= uhi_y
                    && s.z >= ulo_z && s.z <= uhi_z;
                if constexpr (PERIODIC) plain = narrow;
            }
            const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
            if (mask == 0ull) continue;
            const int n_surv = __builtin_popcountll(mask);
            if (keep) {
                const int pos = __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0));
                s_rec[pos] = make_float4(s.x, s.y, s.z, __int_as_float(pj));
                v.stage(pos, pc);
            }
            wave_sync();
            if (!PERIODIC || plain) {
                for (int j = 0; j < n_surv; ++j) {
                    const float4 rec = s_rec[j];
                    const float dx = px - rec.x, dy = py - rec.y, dz = pz - rec.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 <= R2) v.hit(j, rec, d2);
                }
            } else {
                for (int j = 0; j < n_surv; ++j) {
                    const float4 rec = s_rec[j];
                    const float dx = wrap_sep(px - rec.x, per.L[0], per.h[0]);
                    const float dy = wrap_sep(py - rec.y, per.L[1], per.h[1]);
                    const float dz = wrap_sep(pz - rec.z, per.L[2], per.h[2]);
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 <= R2) v.hit(j, rec, d2);
                }
            }
            wave_sync();
        }
    }

    report_overflow(overflow, lane, a.status);
    if (!in_range) return;
    v.finish(src);
}

// The walk the kernel's arguments ask for: Periodic<...> the periodic one, anything else the open one.
template <typename Args, typename Visitor>
__device__ __forceinline__ void walk(const Args& a, const int packet, const int lane, float4* s_rec, Visitor& v)
{
    if constexpr (is_periodic<Args>::value) walk_packet<Visitor, true>(a, packet, lane, s_rec, v, a.per);
    else walk_packet(a, packet, lane, s_rec, v);
}

// The checks every entry point over this walk shares (before anything is enqueued), the radii and
// the scene's fields.
grace_status walk_scene(WalkArgs& a, const float* d_radii, float radius, const float* d_spheres, size_t n_spheres,
                        const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root)
{
    PACKET_SCENE(a, "range query", true, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root);
    a.radii = d_radii;
    a.radius = radius;
    return GRACE_OK;
}

} // namespace
