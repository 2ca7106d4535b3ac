// Depth-ordered emission-absorption integrals along rays (grace_trace_emission_absorption_f4;
// the contract is in grace_hip.h).  gfx950 only.
//
// The call's host sequence (counting walk, 64-bit offsets, batches under the byte budget, nested
// per-hit walks) and the fused kernel's load + sort with its three tiers are in ordered_core.hpp,
// shared with deposit.hip; this file has the composite that follows the sort, and the process-wide
// budget and stats hook both calls use.
// Composite: fp64.  tau_k is carry + (sums of the waves before) + (exclusive wave scan), the
// carry running over groups of blockDim hits; hit k's factor I phi(a) exp(-tau) replaces its
// distance/integral words; then four channels per pass, hit k on thread k mod blockDim, a
// butterfly over the wave and the waves in order.  Every addition's place is a function of k
// and n alone: results do not depend on packets, batches or neighbours.

#include "ordered_core.hpp"

namespace grace_hip {

size_t g_ordered_budget = ORD_DEFAULT_BUDGET;
bool g_ordered_stats_on = false;
grace_ordered_stats g_ordered_stats = {};

namespace {

// ---- the fused sort + composite -----------------------------------------------------------------
struct OrdArgs : OrdBatch {
    const float* emission; int channels; const float* absorption;
    float* out; float* tau;
};

// TIER 0 / 1: arrays of CAP hits in LDS; TIER 2: in place in global memory.  GROUPED: the ray's hits
// are those of all its segments, ordered segment first (ordered_core.hpp); what follows the sort is
// the same code.
template <int T, int CAP, int TIER, bool GROUPED>
__global__ __launch_bounds__(T) void ordered_composite_kernel(const OrdArgs a)
{
    constexpr int WAVES = T / 64;
    __shared__ uint32_t s_d[CAP ? CAP : 1];
    __shared__ int s_x[CAP ? CAP : 1];
    __shared__ uint32_t s_i[CAP ? CAP : 1];
    __shared__ double s_wave[WAVES];
    __shared__ double s_red[WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *D, *I;
    int* X;
    int n;
    size_t r;
    OrdSpan span;
    if (!ordered_load_sort<T, CAP, TIER, GROUPED>(a, s_d, s_x, s_i, D, X, I, n, r, span)) return;


    // optical depths in front of every hit; the hit's factor replaces its (distance, integral) words
    double carry = 0.0;
    for (int base = 0; base < n; base += T) {
        const int k = base + tid;
        double ak = 0.0, Ik = 0.0;
        if (k < n) {
            Ik = static_cast<double>(__uint_as_float(I[k]));
            ak = static_cast<double>(a.absorption[X[k]]) * Ik;
        }
        double inc = ak;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        double exc = __shfl_up(inc, 1);
        if (lane == 0) exc = 0.0;
        double before = exc, total = __shfl(inc, 63);
        if (WAVES > 1) {
            if (lane == 63) s_wave[wave] = inc;
            __syncthreads();
            double run = 0.0, mine = 0.0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) { if (w == wave) mine = run; run += s_wave[w]; }
            before = mine + exc;
            total = run;
            __syncthreads();
        }
        if (k < n) {
            const double phi = ak != 0.0 ? -expm1(-ak) / ak : 1.0;
            const double f = Ik * phi * exp(-(carry + before));
            const unsigned long long fb = static_cast<unsigned long long>(__double_as_longlong(f));
            D[k] = static_cast<uint32_t>(fb >> 32);
            I[k] = static_cast<uint32_t>(fb);
        }
        carry += total;
    }
    if (tid == 0 && a.tau) a.tau[r] = static_cast<float>(carry);

    // (hit k stays on thread k mod T from here on: no barrier needed after the pass above)
    const int C = a.channels;
    for (int c0 = 0; c0 < C; c0 += 4) {
        const int nc = C - c0 < 4 ? C - c0 : 4;
        double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
        for (int k = tid; k < n; k += T) {
            const double f = __longlong_as_double(
                static_cast<long long>((static_cast<unsigned long long>(D[k]) << 32) | I[k]));
            const float* e = a.emission + size_t(X[k]) * C + c0;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < nc) acc[j] += static_cast<double>(e[j]) * f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_xor(acc[j], o);
        // (GROUPED: through LDS in the wave tier too -- the same values; the open wave tier's select
        // below becomes an indexed read of acc in scratch, 48 bytes a lane, which it keeps)
        if (WAVES > 1 || GROUPED) {
            if (lane == 0)
#pragma unroll
                for (int j = 0; j < 4; ++j) s_red[wave][j] = acc[j];
            __syncthreads();
            if (tid < nc) {
                double s = s_red[0][tid];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) s += s_red[w][tid];
                a.out[r * C + c0 + tid] = static_cast<float>(s);
            }
            __syncthreads();
        } else if (tid < nc) {
            double s = acc[0];
            if (tid == 1) s = acc[1];
            if (tid == 2) s = acc[2];
            if (tid == 3) s = acc[3];
            a.out[r * C + c0 + tid] = static_cast<float>(s);
        }
    }
}

template <bool GROUPED>
grace_status composite_launch(const OrdArgs& a, const int nb, const bool any_block, const bool any_global,
                              const hipStream_t stream)
{
    ordered_composite_kernel<64, ORD_WAVE_MAX, 0, GROUPED><<<nb, 64, 0, stream>>>(a);
    GRACE_CHECK_LAUNCH();
    if (any_block) {
        ordered_composite_kernel<256, ORD_BLOCK_MAX, 1, GROUPED><<<nb, 256, 0, stream>>>(a);
        GRACE_CHECK_LAUNCH();
    }
    if (any_global) {
        ordered_composite_kernel<256, 0, 2, GROUPED><<<nb, 256, 0, stream>>>(a);
        GRACE_CHECK_LAUNCH();
    }
    return GRACE_OK;
}

// The open call (grouped == null) and the periodic one: d_rays are then the segments, the weights
// are indexed by source.
grace_status emission_absorption(const void* d_rays, size_t n_rays, const float* d_spheres, size_t n_spheres,
                                 const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root,
                                 const float* d_emission, int n_channels, const float* d_absorption, float* d_out,
                                 float* d_tau, grace_stream stream_, const OrdGroups* grouped)
{
    GRACE_REQUIRE(n_channels >= 1 && n_channels <= 64, "trace_emission_absorption: channels must be 1..64");
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_emission && d_absorption, "trace_emission_absorption: null weights");
    GRACE_REQUIRE(d_out, "trace_emission_absorption: null output");
    GRACE_REQUIRE(d_rays && d_spheres && d_nodes && d_leaves && d_root, "trace_emission_absorption: null pointer");
    GRACE_REQUIRE(n_rays < (size_t(1) << 31), "trace_emission_absorption: bad ray count");
    GRACE_REQUIRE(n_nodes >= 1 && n_nodes < (size_t(1) << 30), "trace_emission_absorption: bad node count");
    GRACE_REQUIRE(n_spheres > 0 && n_spheres < (size_t(1) << 31), "trace_emission_absorption: bad primitive count");
    const hipStream_t stream = as_stream(stream_);
    OrdArgs a;
    a.emission = d_emission; a.channels = n_channels; a.absorption = d_absorption;
    a.out = d_out; a.tau = d_tau;
    FrameGuard frame;
    return ordered_run(
        frame, d_rays, n_rays, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, 0, stream,
        [](char*) -> grace_status { return GRACE_OK; },
        [&](const OrdBatch& batch, const int nb, const bool any_block, const bool any_global) -> grace_status {
            static_cast<OrdBatch&>(a) = batch;
            return grouped ? composite_launch<true>(a, nb, any_block, any_global, stream)
                           : composite_launch<false>(a, nb, any_block, any_global, stream);
        },
        grouped);
}

} // namespace
} // namespace grace_hip

using namespace grace_hip;

extern "C" {

grace_status grace_trace_emission_absorption_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                                size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                                const int* d_leaves, const int* d_root,
                                                const float* d_emission, int n_channels,
                                                const float* d_absorption, float* d_out, float* d_tau,
                                                grace_stream stream_)
{
    return emission_absorption(d_rays, n_rays, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, d_emission,
                               n_channels, d_absorption, d_out, d_tau, stream_, nullptr);
}

grace_status grace_trace_emission_absorption_periodic_f4(const void* d_segments, size_t n_segments,
                                                         const float* d_images, size_t n_images, const int* d_nodes,
                                                         size_t n_nodes, const int* d_leaves, const int* d_root,
                                                         const int* d_segment_offsets, size_t n_rays,
                                                         const int* d_source, size_t n_sources,
                                                         const float* d_emission, int n_channels,
                                                         const float* d_absorption, float* d_out, float* d_tau,
                                                         grace_stream stream_)
{
    if (n_rays == 0) return GRACE_OK;
    OrdGroups g;
    GRACE_TRY(ordered_groups(g, d_segments, n_segments, d_segment_offsets, n_rays, d_source, n_sources, nullptr));
    return emission_absorption(d_segments, n_segments, d_images, n_images, d_nodes, n_nodes, d_leaves, d_root,
                               d_emission, n_channels, d_absorption, d_out, d_tau, stream_, &g);
}

grace_status grace_trace_set_ordered_budget(size_t bytes)
{
    g_ordered_budget = bytes ? bytes : ORD_DEFAULT_BUDGET;
    return GRACE_OK;
}

grace_status grace_trace_ordered_limits(int* wave_max_hits, int* block_max_hits)
{
    GRACE_REQUIRE(wave_max_hits && block_max_hits, "trace_ordered_limits: null output");
    *wave_max_hits = ORD_WAVE_MAX;
    *block_max_hits = ORD_BLOCK_MAX;
    return GRACE_OK;
}

grace_status grace_trace_ordered_enable_stats(int enabled)
{
    g_ordered_stats_on = enabled != 0;
    if (!g_ordered_stats_on) g_ordered_stats = grace_ordered_stats();
    return GRACE_OK;
}

grace_status grace_trace_ordered_last_stats(grace_ordered_stats* h_stats)
{
    GRACE_REQUIRE(h_stats, "trace_ordered_last_stats: null output");
    GRACE_REQUIRE(g_ordered_stats_on, "trace_ordered_last_stats: statistics are not enabled");
    *h_stats = g_ordered_stats;
    return GRACE_OK;
}

} // extern "C"
