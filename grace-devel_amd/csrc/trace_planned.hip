// The packet plan of the column-density traces, for gfx950 (see PacketPlan in trace_state.hpp):
// the kernel that records it, its buffers, and the PLANNED instantiations of trace_kernel that
// consume it (a translation unit of their own: they compile beside trace.hip's).
//
// The record kernel is the cull of trace_kernel's axis path on its own -- group boxes, cluster
// boxes, then per culling round the exact beam bound, the lean / fat decisions and the
// origin-lattice cull -- one wave per packet, all eight classes, no survivor loop.  It is not a
// hot path (it runs when a plan is first sized and recorded, and again when a signature goes
// stale), so the axis is a run-time value and nothing is prefetched.  A recorded mask need not
// equal the mask the ordinary kernel would form: any conservative superset of the true hits gives
// the same sums bit for bit (the exact integral tests every survivor; the fast one adds exactly +0
// for a miss), as long as the lean and fat bits are decided on the recorded survivors, which they
// are.  The lattice cull is applied wherever the packet's origins form a lattice, whatever the
// batch-level flag says.
// The recorder also groups each list's consecutive entries (one cluster's survivor mask each) into
// dense rounds and tallies what it formed in PlanCtl::stats.  It stores the cull inverted: the
// survivors' primitive indices, contiguous per list in list order, and one header per dense round
// (plan_header) -- the planned kernel's lane l takes index word `round's first + l`.
// SUB: the sub-tile layout (PLAN_FORMAT_SUBTILE, trace_state.hpp).  The packet set-up also forms the
// origin rectangle of each quadrant (lanes 16 q .. 16 q + 15); every entry's packet-level mask is
// cut into four sub-masks by the same bound against those rectangles, and each quadrant appends its
// survivors to a stream of its own.  Rounds are runs of PLAN_SUB_ROUND_STEPS steps; the streams
// drift apart, so an entry's bits are ANDed into every round its words fall in.
#include "trace_kernel.hpp"

#include <vector>

using namespace grace_hip;

namespace {

struct PlanRef {
    uint32_t* idx;
    uint32_t* hdr;
    const int4* spans;   // null: sizing pass (counts only)
    int4* counts;
    PlanCtl* ctl;
    int force;           // record whatever ctl->record says (the first fill)
};

template <bool FUSED, bool SUB = false>
__global__ __launch_bounds__(TRACE_BLOCK) void plan_record_kernel(const TraceArgs a, const PlanRef pl)
{
    static_assert(!SUB || FUSED, "sub-tile plans: the fast integral only");
    __shared__ float s_lat[TRACE_BLOCK / 64][2][8];   // the packets' origin lattices
    if (pl.spans && !pl.force && pl.ctl->record == 0u) return;   // (workgroup-uniform)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n_packets = (a.n_rays + a.width - 1) / a.width;
    const int packet = blockIdx.x * (TRACE_BLOCK / 64) + wv;
    if (packet >= n_packets) return;
    // the packet's set-up, with trace_kernel's own pieces (trace_packet.hpp)
    const PacketRay ray = load_packet_ray(a, packet * a.width, lane);
    const int axis = packet_axis(ray.dx, ray.dy, ray.dz);
    const float4* const group_boxes = a.C + 2 * ((size_t(a.n_prims) + 63) >> 6) + 1;
    const int covered = min(__float_as_int(group_boxes[-1].y), a.n_prims);
    int cnt = 0;     // lane c < SUM_CLASSES: entries of class c so far (t_surv: its survivors,
                     // t_rounds: its closed rounds)
    // Rounds (the planned kernel runs one survivor loop per round): consecutive entries of a list,
    // at most 64 survivors together, all with the same lean / fat bits.  Lane c holds the open
    // round of class c -- its survivors and its bits -- and the class's tallies for PlanCtl.
    int round_n = 0, round_bits = 0;
    int t_surv = 0, t_rounds = 0, t_full = 0, t_cap = 0, t_flag = 0, t_max = 0;
    // ... and the survivor loop of the fused consumer that the class's closed rounds have opened
    // (planned_fuses; FUSED: the fast integral -- the exact one runs a loop per round)
    int loop_n = 0, loop_bits = 0, t_loops = 0, t_lmax = 0;
    // SUB: lane 4 c + q holds the steps of class c's stream of quadrant q so far; lane c the rounds
    // of class c whose header has been started
    int sub_pos = 0, sub_touched = 0;
    (void)sub_pos; (void)sub_touched;
    auto round_closed = [&](const int n, const int bits) {   // (on the class's own lane)
        if (FUSED && loop_n > 0 && planned_fuses(loop_n, loop_bits, plan_header(n, bits))) {
            loop_n += n;
        } else {
            if (loop_n > 0) { t_loops += 1; t_lmax = max(t_lmax, loop_n); }
            loop_n = n; loop_bits = bits;
        }
    };
    bool failed = axis < 0 || covered < 0;   // not an axis-aligned flat packet: no plan for this batch
    if (!failed) {
        const AxisRay ar = axis_ray(axis, ray);
        float noda_lo, noda_hi, len_lo, da0;
        bool same_sense;
        axis_extremes(ar, ray.len, noda_lo, noda_hi, len_lo, da0, same_sense);
        // the origin rectangle, and the packet's extent along the axis
        const float lo1 = wave_min(ar.o1), hi1 = wave_max(ar.o1), lo2 = wave_min(ar.o2), hi2 = wave_max(ar.o2);
        const float ea = ar.oa + ar.da * ray.len;
        const float alo = wave_min(fminf(ar.oa, ea)), ahi = wave_max(fmaxf(ar.oa, ea));
        const float fat_r2 = fat_radius2(hi1 - lo1, hi2 - lo2);
        bool lat_ok;
        float cell2;
        build_origin_lattice(ar.o1, ar.o2, lane, s_lat, lat_ok, cell2);
        const float lat_r2 = lat_ok ? cell2 : 0.f;
        // SUB: the quadrants' origin rectangles, from their own valid lanes (each row of 16 lanes
        // reduces its own); a quadrant without a valid ray keeps nothing
        float qlo1[4] = {}, qhi1[4] = {}, qlo2[4] = {}, qhi2[4] = {};
        unsigned long long q_lanes[4] = {};
        if constexpr (SUB) {
            float m1 = ray.valid ? ar.o1 : INFINITY, x1 = ray.valid ? ar.o1 : -INFINITY;
            float m2 = ray.valid ? ar.o2 : INFINITY, x2 = ray.valid ? ar.o2 : -INFINITY;
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                m1 = fminf(m1, __shfl_xor(m1, off)); x1 = fmaxf(x1, __shfl_xor(x1, off));
                m2 = fminf(m2, __shfl_xor(m2, off)); x2 = fmaxf(x2, __shfl_xor(x2, off));
            }
            const unsigned long long valid_lanes = __builtin_amdgcn_ballot_w64(ray.valid);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                qlo1[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m1), 16 * q));
                qhi1[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x1), 16 * q));
                qlo2[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, m2), 16 * q));
                qhi2[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x2), 16 * q));
                q_lanes[q] = ((valid_lanes >> (16 * q)) & 0xffffull) != 0ull ? ~0ull : 0ull;
            }
        }

        // a box against the packet's origin rectangle (and, for groups, its extent along the axis)
        auto box_may_hit = [&](const float4 blo, const float4 bhi, const bool along) {
            const float l1 = axis == 0 ? blo.y : blo.x, h1 = axis == 0 ? bhi.y : bhi.x;
            const float l2 = axis == 2 ? blo.y : blo.z, h2 = axis == 2 ? bhi.y : bhi.z;
            const float la = axis == 0 ? blo.x : axis == 1 ? blo.y : blo.z;
            const float ha = axis == 0 ? bhi.x : axis == 1 ? bhi.y : bhi.z;
            // (negated forms: a NaN bound keeps the box)
            return !(l1 > hi1) && !(h1 < lo1) && !(l2 > hi2) && !(h2 < lo2)
                && (!along || (!(la > ahi) && !(ha < alo)));
        };
        const int n_groups = int((size_t(covered) + (size_t(1) << a.group_shift) - 1) >> a.group_shift);
        for (int g0 = 0; g0 < n_groups; g0 += 64) {
            const int gj = min(g0 + lane, n_groups - 1);
            const bool g_may = box_may_hit(group_boxes[2 * size_t(gj)], group_boxes[2 * size_t(gj) + 1], true);
            const int n_g = min(64, n_groups - g0);
            unsigned long long gmask = __builtin_amdgcn_ballot_w64(g_may) & (n_g >= 64 ? ~0ull : ((1ull << n_g) - 1ull));
            while (gmask != 0ull) {
                const int g = g0 + __builtin_ctzll(gmask);
                gmask &= gmask - 1ull;
                const int r_lo = g << a.group_shift;
                const int r_hi = r_lo + min(1 << a.group_shift, covered - r_lo);
                const int c_first = r_lo >> 6, c_last = (r_hi - 1) >> 6;
                for (int cg = c_first; cg <= c_last; cg += 64) {
                    const int cj = min(cg + lane, c_last);
                    const bool c_may = box_may_hit(a.C[2 * size_t(cj)], a.C[2 * size_t(cj) + 1], false);
                    const int n_c = min(64, c_last - cg + 1);
                    unsigned long long cmask = __builtin_amdgcn_ballot_w64(c_may)
                        & (n_c >= 64 ? ~0ull : ((1ull << n_c) - 1ull));
                    while (cmask != 0ull) {
                        const int c = cg + __builtin_ctzll(cmask);
                        cmask &= cmask - 1ull;
                        const int pbase = c << 6;
                        const int pj = min(max(pbase + lane, r_lo), r_hi - 1);
                        const float4 mine = a.A[pj];
                        const int lo_bit = max(r_lo - pbase, 0), hi_bit = min(r_hi - pbase, 64);
                        const unsigned long long m_mask =
                            (hi_bit >= 64 ? ~0ull : ((1ull << hi_bit) - 1ull)) & (~0ull << lo_bit);
                        const float s1 = axis == 0 ? mine.y : mine.x;
                        const float s2 = axis == 2 ? mine.y : mine.z;
                        const float sa = axis == 0 ? mine.x : axis == 1 ? mine.y : mine.z;
                        // axis_beam_may_hit: the exact lower bound of the rays' own b^2 expression
                        const float q1 = s1 - __builtin_amdgcn_fmed3f(s1, lo1, hi1);
                        const float q2 = s2 - __builtin_amdgcn_fmed3f(s2, lo2, hi2);
                        const float b2_lo = FUSED ? __builtin_fmaf(q1, q1, q2 * q2) : q1 * q1 + q2 * q2;
                        bool keep = !(b2_lo >= mine.w);
                        unsigned long long rest = __builtin_amdgcn_ballot_w64(keep) & m_mask;
                        keep = __builtin_amdgcn_inverse_ballot_w64(rest);
                        if (rest != 0ull && __builtin_amdgcn_ballot_w64(keep && mine.w < lat_r2) != 0ull) {
                            float p1 = INFINITY, p2 = INFINITY;
                            for (int k = 0; k < 8; ++k) {
                                p1 = fminf(p1, fabsf(s1 - s_lat[wv][0][k]));
                                p2 = fminf(p2, fabsf(s2 - s_lat[wv][1][k]));
                            }
                            const float nan_if_nan = (s1 + s2) * 0.0f;   // (a NaN centre stays)
                            const float l2 = (FUSED ? __builtin_fmaf(p1, p1, p2 * p2) : p1 * p1 + p2 * p2) + nan_if_nan;
                            keep = keep && !(l2 >= mine.w);
                            rest = __builtin_amdgcn_ballot_w64(keep);
                        }
                        if (rest == 0ull) continue;
                        // lean: every survivor lies inside every ray's [0, length) along the axis
                        const unsigned long long inside =
                            __builtin_amdgcn_ballot_w64(__builtin_fmaf(sa, da0, noda_lo) >= 0.0f)
                            & __builtin_amdgcn_ballot_w64(__builtin_fmaf(sa, da0, noda_hi) < len_lo);
                        const bool lean = same_sense && (rest & ~inside) == 0ull;
                        const bool fat = FUSED && (rest & ~__builtin_amdgcn_ballot_w64(mine.w >= fat_r2)) == 0ull;
                        const int cls = (c >> (GRANULE_SHIFT - 6)) & (SUM_CLASSES - 1);
                        const int n = __builtin_amdgcn_readlane(cnt, cls);
                        const int bits = (lean ? 1 : 0) | (fat ? 2 : 0);
                        // the class's open round takes this entry, or closes before it: (a) past 64
                        // survivors with it, (b) other lean / fat bits
                        const int n_surv = __builtin_popcountll(rest);
                        if constexpr (SUB) {
                            const int4 span = pl.spans ? pl.spans[packet * SUM_CLASSES + cls] : make_int4(0, 0, 0, 0);
                            int touched = __builtin_amdgcn_readlane(sub_touched, cls);
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                // the same bound against the quadrant's rectangle (negated: a NaN
                                // centre or bound stays in every quadrant)
                                const float u1 = s1 - __builtin_amdgcn_fmed3f(s1, qlo1[q], qhi1[q]);
                                const float u2 = s2 - __builtin_amdgcn_fmed3f(s2, qlo2[q], qhi2[q]);
                                const unsigned long long rest_q =
                                    __builtin_amdgcn_ballot_w64(!(__builtin_fmaf(u1, u1, u2 * u2) >= mine.w)) & rest & q_lanes[q];
                                if (rest_q == 0ull) continue;
                                const int n_q = __builtin_popcountll(rest_q);
                                const int at = __builtin_amdgcn_readlane(sub_pos, 4 * cls + q);
                                const int r_first = at / PLAN_SUB_ROUND_STEPS, r_last = (at + n_q - 1) / PLAN_SUB_ROUND_STEPS;
                                if (pl.spans) {
                                    // room for the quadrant's words and for the headers of the rounds they fall in
                                    if (at + n_q <= span.z && r_last < span.w) {
                                        if ((rest_q >> lane) & 1ull)
                                            pl.idx[size_t(span.x) + 4 * size_t(at + int(__builtin_amdgcn_mbcnt_hi(uint32_t(rest_q >> 32),
                                                                                           __builtin_amdgcn_mbcnt_lo(uint32_t(rest_q), 0u)))) + q] =
                                                uint32_t(pbase + lane);
                                        // (headers are read and written by lane 0 alone, in program order;
                                        // counts are set when the list ends)
                                        if (lane == 0) {
                                            for (int r = r_first; r <= r_last; ++r) {
                                                uint32_t* const h = pl.hdr + size_t(span.y) + r;
                                                *h = plan_header(64, r < touched ? bits & plan_header_bits(*h) : bits);
                                            }
                                        }
                                    } else {
                                        failed = true;   // the list has outgrown its room
                                    }
                                }
                                touched = max(touched, r_last + 1);
                                if (lane == 4 * cls + q) sub_pos += n_q;
                            }
                            if (lane == cls) { sub_touched = touched; t_surv += n_surv; cnt += 1; }
                            continue;
                        }
                        const int open_n = __builtin_amdgcn_readlane(round_n, cls);
                        const int open_bits = __builtin_amdgcn_readlane(round_bits, cls);
                        const bool close_cap = n > 0 && open_n + n_surv > 64;
                        const bool close_flag = n > 0 && !close_cap && open_bits != bits;
                        const bool close = close_cap || close_flag;
                        if (pl.spans) {
                            const int4 span = pl.spans[packet * SUM_CLASSES + cls];
                            const int surv_at = __builtin_amdgcn_readlane(t_surv, cls);
                            const int closed = __builtin_amdgcn_readlane(t_rounds, cls);
                            // room for the entry's survivors, and for the header of the round it is
                            // in (round closed + 1 if it closes one: written when that round closes)
                            if (surv_at + n_surv <= span.z && closed + (close ? 1 : 0) < span.w) {
                                if (close && lane == 0) pl.hdr[size_t(span.y) + closed] = plan_header(open_n, open_bits);
                                // the lanes the mask names, at the list's running count + their rank
                                if ((rest >> lane) & 1ull)
                                    pl.idx[size_t(span.x) + surv_at
                                           + int(__builtin_amdgcn_mbcnt_hi(uint32_t(rest >> 32),
                                                                           __builtin_amdgcn_mbcnt_lo(uint32_t(rest), 0u)))] =
                                        uint32_t(pbase + lane);
                            } else {
                                failed = true;   // the list has outgrown its room
                            }
                        }
                        if (lane == cls) {
                            if (close) {
                                t_rounds += 1; t_full += open_n == 64 ? 1 : 0;
                                t_cap += close_cap ? 1 : 0; t_flag += close_flag ? 1 : 0;
                                t_max = max(t_max, open_n);
                                round_closed(open_n, open_bits);
                                round_n = 0;
                            }
                            round_n += n_surv; round_bits = bits;
                            t_surv += n_surv;
                            cnt += 1;
                        }
                    }
                }
            }
        }
    }
    if (failed) {
        cnt = 0;
        if (lane == 0) { pl.ctl->unusable = 1u; pl.ctl->usable = 0u; }
    }
    // SUB: the end of a list pads its shorter streams with the null record up to the longest, sets
    // the round counts (every round PLAN_SUB_ROUND_STEPS steps, the last what is left) and tallies
    // the list's rounds and loops
    int sub_steps = 0, sub_real = 0;   // lane c: class c's steps, and its streams' real words
    if constexpr (SUB) {
        for (int c = 0; c < SUM_CLASSES; ++c) {
            int steps = 0, real = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = failed ? 0 : __builtin_amdgcn_readlane(sub_pos, 4 * c + q);
                steps = max(steps, n); real += n;
            }
            const int rounds = (steps + PLAN_SUB_ROUND_STEPS - 1) / PLAN_SUB_ROUND_STEPS;
            int loops = 0, lmax = 0;
            if (pl.spans && steps > 0) {
                const int4 span = pl.spans[packet * SUM_CLASSES + c];   // (steps <= span.z, rounds <= span.w: the entries' tests)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    for (int t = __builtin_amdgcn_readlane(sub_pos, 4 * c + q) + lane; t < steps; t += 64)
                        pl.idx[size_t(span.x) + 4 * size_t(t) + q] = uint32_t(a.n_prims);
                if (lane == 0) {
                    uint32_t* const h = pl.hdr + size_t(span.y);
                    h[rounds - 1] = plan_header(4 * (steps - (rounds - 1) * PLAN_SUB_ROUND_STEPS), plan_header_bits(h[rounds - 1]));
                    int ln = 0, lb = 0;
                    for (int r = 0; r < rounds; ++r) {
                        const uint32_t next = h[r];
                        if (ln > 0 && planned_fuses(ln, lb, next)) {
                            ln += plan_header_count(next);
                        } else {
                            if (ln > 0) { loops += 1; lmax = max(lmax, ln); }
                            ln = plan_header_count(next); lb = plan_header_bits(next);
                        }
                    }
                    loops += 1; lmax = max(lmax, ln);
                }
                loops = __builtin_amdgcn_readlane(loops, 0); lmax = __builtin_amdgcn_readlane(lmax, 0);
            }
            if (lane == c) {
                t_rounds = rounds; t_full = steps / PLAN_SUB_ROUND_STEPS;
                t_max = min(4 * steps, 4 * PLAN_SUB_ROUND_STEPS);
                t_loops = loops; t_lmax = lmax;
                sub_steps = steps; sub_real = real;
            }
        }
    }
    // (c) the end of a list closes its round (its header had room: see the entries' test)
    if (!SUB && lane < SUM_CLASSES && cnt > 0) {
        if (pl.spans && !failed)
            pl.hdr[size_t(pl.spans[packet * SUM_CLASSES + lane].y) + t_rounds] = plan_header(round_n, round_bits);
        t_rounds += 1; t_full += round_n == 64 ? 1 : 0;
        t_max = max(t_max, round_n);
        round_closed(round_n, round_bits);
        t_loops += 1; t_lmax = max(t_lmax, loop_n);   // ... and its loop
    }
    if (lane < SUM_CLASSES) pl.counts[packet * SUM_CLASSES + lane] = failed ? make_int4(0, 0, 0, 0) : make_int4(t_rounds, t_surv, cnt, sub_steps);
    if (pl.spans && !failed) {
        // the packet's tallies (the recording pass only: not a hot path, and the planned kernel
        // never reads them)
        if (lane >= SUM_CLASSES) cnt = 0;
        int tally[7] = { cnt, t_surv, t_rounds, t_full, t_cap, t_flag, t_loops };
#pragma unroll
        for (int off = 1; off < SUM_CLASSES; off <<= 1) {
#pragma unroll
            for (int k = 0; k < 7; ++k) tally[k] += __shfl_xor(tally[k], off);
            t_max = max(t_max, __shfl_xor(t_max, off));
            t_lmax = max(t_lmax, __shfl_xor(t_lmax, off));
            if constexpr (SUB) { sub_steps += __shfl_xor(sub_steps, off); sub_real += __shfl_xor(sub_real, off); }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (tally[k]) atomicAdd(&pl.ctl->stats[k], (unsigned long long)tally[k]);
            if (tally[6]) atomicAdd(&pl.ctl->loops, (unsigned long long)tally[6]);
            if (SUB && sub_steps) atomicAdd(&pl.ctl->sub_steps, (unsigned long long)sub_steps);
            if (SUB && sub_real) atomicAdd(&pl.ctl->sub_slots, (unsigned long long)sub_real);
            atomicMax(&pl.ctl->largest_round, uint32_t(t_max));
            atomicMax(&pl.ctl->largest_loop, uint32_t(t_lmax));
        }
    }
}

grace_status launch_record(const bool fast, const bool subtiles, const TraceArgs& a, const PlanRef& pl, hipStream_t stream)
{
    const int n_packets = (a.n_rays + a.width - 1) / a.width;
    const int grid = ceil_div(size_t(n_packets), size_t(TRACE_BLOCK / 64));
    if (subtiles) plan_record_kernel<true, true><<<grid, TRACE_BLOCK, 0, stream>>>(a, pl);
    else if (fast) plan_record_kernel<true><<<grid, TRACE_BLOCK, 0, stream>>>(a, pl);
    else plan_record_kernel<false><<<grid, TRACE_BLOCK, 0, stream>>>(a, pl);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

grace_status plan_free_buffers(PacketPlan& pp)
{
    void* bufs[] = { pp.idx, pp.hdr, pp.spans, pp.counts, pp.ctl };
    bool any = false;
    for (void* b : bufs) any = any || b;
    if (any) GRACE_TRY_HIP(hipDeviceSynchronize());
    for (void* b : bufs)
        if (b) GRACE_TRY_HIP(hipFree(b));
    pp.idx = nullptr; pp.hdr = nullptr; pp.spans = nullptr; pp.counts = nullptr; pp.ctl = nullptr;
    pp.valid = false;
    pp.n_lists = pp.n_words = pp.n_hdrs = pp.recorded = 0;
    pp.key.subtiles = false;
    return GRACE_OK;
}

} // namespace

namespace grace_hip {

grace_status plan_release(TraceState& ts)
{
    GRACE_TRY(plan_free_buffers(ts.plan));
    ts.plan = PacketPlan();
    ts.last_plan_ctl = nullptr;
    return GRACE_OK;
}

grace_status plan_fill(TraceState& ts, const PlanKey& key, const int request, const TraceArgs& a, hipStream_t stream)
{
    PacketPlan& pp = ts.plan;
    GRACE_TRY(plan_free_buffers(pp));
    ts.last_plan_ctl = nullptr;
    pp.key = key;
    pp.key.subtiles = false;
    pp.asked = request;
    pp.dead = true;      // until the plan stands
    const int n_packets = (a.n_rays + a.width - 1) / a.width;
    const size_t n_lists = size_t(n_packets) * SUM_CLASSES;
    // (out of memory at any step: no plan, the call goes on without one)
    auto alloc = [&](auto*& ptr, const size_t bytes) {
        if (hipMalloc(reinterpret_cast<void**>(&ptr), bytes) == hipSuccess) return true;
        (void)hipGetLastError();
        ptr = nullptr;
        return false;
    };
    if (n_lists * (sizeof(int4) + sizeof(int4)) > ts.plan_budget) return GRACE_OK;
    if (!alloc(pp.counts, n_lists * sizeof(int4)) || !alloc(pp.spans, n_lists * sizeof(int4))
        || !alloc(pp.ctl, sizeof(PlanCtl)))
        return plan_free_buffers(pp);
    std::vector<int4> counts(n_lists), spans(n_lists);
    // The sub-tile layout first, where the call asks for it (only fast, unweighted calls over full
    // packets do: use_records), then format 3: whichever is sized, fits and -- automatic -- pays.
    for (int sub = request != 0 && key.fast && a.width == 64 ? 1 : 0; sub >= 0; --sub) {
        // 1. sizing pass: rounds, survivors and entries per list (sub-tile layout: and steps), and
        //    whether every packet can be planned at all
        GRACE_TRY_HIP(hipMemsetAsync(pp.ctl, 0, sizeof(PlanCtl), stream));
        GRACE_TRY(launch_record(key.fast, sub != 0, a, PlanRef{ nullptr, nullptr, nullptr, pp.counts, pp.ctl, 1 }, stream));
        PlanCtl seen = {};
        GRACE_TRY_HIP(hipMemcpyAsync(counts.data(), pp.counts, n_lists * sizeof(int4), hipMemcpyDeviceToHost, stream));
        GRACE_TRY_HIP(hipMemcpyAsync(&seen, pp.ctl, sizeof(seen), hipMemcpyDeviceToHost, stream));
        GRACE_TRY_HIP(hipStreamSynchronize(stream));
        if (seen.unusable) return plan_free_buffers(pp);
        // 2. room per list, in survivors and in rounds: what it holds now and an eighth more, so that
        //    a re-record after a small change of the scene or the rays still fits.  The rounds' room is
        //    counted from the ENTRIES (a round holds at least one): a change that only moves lean /
        //    fat bits, or shrinks spheres, splits rounds without adding entries, and must still fit.
        //    Sub-tile layout: room in steps, the longest stream and an eighth more, four words each;
        //    the rounds' room is what those steps can make.
        size_t words = 0, hdrs = 0, used = 0, steps = 0;
        bool fits = true;
        for (size_t l = 0; l < n_lists && fits; ++l) {
            const size_t surv = size_t(counts[l].y), entries = size_t(counts[l].z), len = size_t(counts[l].w);
            const size_t room_s = sub ? len + len / 8 + 2 : surv + surv / 8 + 2;
            const size_t room_r = sub ? (room_s + PLAN_SUB_ROUND_STEPS - 1) / PLAN_SUB_ROUND_STEPS : entries + entries / 8 + 2;
            spans[l] = make_int4(int(words), int(hdrs), int(room_s), int(room_r));
            words += sub ? 4 * room_s : room_s;
            hdrs += room_r;
            used += surv;
            steps += len;
            fits = words < (size_t(1) << 31) - PLAN_IDX_PAD;
        }
        pp.n_lists = n_lists; pp.n_words = words; pp.n_hdrs = hdrs; pp.recorded = used;
        fits = fits && pp.bytes() <= ts.plan_budget;
        if (sub) {
            // the automatic rule: enough packets, and streams that drop enough of the survivors' steps
            const bool pays = n_packets >= PLAN_SUB_MIN_PACKETS && double(steps) < PLAN_SUB_MAX_RATIO * double(used);
            if (!fits || (request < 0 && !pays)) continue;
        }
        if (!fits || !alloc(pp.idx, (words + PLAN_IDX_PAD) * sizeof(uint32_t))
            || !alloc(pp.hdr, (hdrs + PLAN_HDR_PAD) * sizeof(uint32_t))) {
            if (sub) {   // (no memory for this layout: format 3 may still fit)
                if (pp.idx) { GRACE_TRY_HIP(hipFree(pp.idx)); pp.idx = nullptr; }
                continue;
            }
            return plan_free_buffers(pp);
        }
        GRACE_TRY_HIP(hipMemcpy(pp.spans, spans.data(), n_lists * sizeof(int4), hipMemcpyHostToDevice));
        // (the padding the planned kernel may read past the last list)
        GRACE_TRY_HIP(hipMemsetAsync(pp.idx + words, 0, PLAN_IDX_PAD * sizeof(uint32_t), stream));
        GRACE_TRY_HIP(hipMemsetAsync(pp.hdr + hdrs, 0, PLAN_HDR_PAD * sizeof(uint32_t), stream));
        // 3. record
        pp.key.subtiles = sub != 0;
        GRACE_TRY_HIP(hipMemsetAsync(pp.ctl, 0, sizeof(PlanCtl), stream));   // (the sizing pass's tallies)
        GRACE_TRY_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&pp.ctl->usable), 1, 1, stream));
        GRACE_TRY_HIP(hipMemcpyAsync(&pp.ctl->sig[0], ts.scene.ctl->sig, 16, hipMemcpyDeviceToDevice, stream));
        GRACE_TRY_HIP(hipMemcpyAsync(&pp.ctl->sig[2], ts.rays.ctl->sig, 16, hipMemcpyDeviceToDevice, stream));
        GRACE_TRY(launch_record(key.fast, sub != 0, a, PlanRef{ pp.idx, pp.hdr, pp.spans, pp.counts, pp.ctl, 1 }, stream));
        pp.valid = true;
        pp.dead = false;
        return GRACE_OK;
    }
    return GRACE_OK;   // (not reached: the format-3 pass returns)
}

grace_status plan_record(const TraceState& ts, const TraceArgs& a, hipStream_t stream)
{
    const PacketPlan& pp = ts.plan;
    return launch_record(pp.key.fast, pp.key.subtiles, a, PlanRef{ pp.idx, pp.hdr, pp.spans, pp.counts, pp.ctl, 0 }, stream);
}

grace_status launch_planned(const int mode, const bool fast, const bool subtiles, const int grid, const TraceArgs& a, hipStream_t stream)
{
    if (subtiles) {
        if (mode != MODE_CUMULATIVE || !fast)
            return set_error(GRACE_INVALID_ARGUMENT, __FILE__, __LINE__, "no sub-tile planned kernel for this mode");
        trace_kernel<MODE_CUMULATIVE, true, true, false, true, true><<<grid, TRACE_BLOCK, 0, stream>>>(a);
        GRACE_CHECK_LAUNCH();
        return GRACE_OK;
    }
    auto go = [&](auto mode_tag) {
        constexpr int MODE = decltype(mode_tag)::value;
        if (fast) trace_kernel<MODE, true, true, false, true><<<grid, TRACE_BLOCK, 0, stream>>>(a);
        else trace_kernel<MODE, true, false, false, true><<<grid, TRACE_BLOCK, 0, stream>>>(a);
    };
    switch (mode) {
    case MODE_CUMULATIVE: go(std::integral_constant<int, MODE_CUMULATIVE>()); break;
    case MODE_WCUM1: go(std::integral_constant<int, MODE_WCUM1>()); break;
    case MODE_WCUM2: go(std::integral_constant<int, MODE_WCUM2>()); break;
    case MODE_WCUM3: go(std::integral_constant<int, MODE_WCUM3>()); break;
    case MODE_WCUM4: go(std::integral_constant<int, MODE_WCUM4>()); break;
    default: return set_error(GRACE_INVALID_ARGUMENT, __FILE__, __LINE__, "no planned kernel for this mode");
    }
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

} // namespace grace_hip
