// Depth-ordered emission-absorption integrals along rays (grace_trace_emission_absorption_f4;
// the contract is in grace_hip.h).  gfx950 only.
//
// The call, on the caller's stream and inside ONE workspace frame:
//   1. hit counts of all rays (the counting walk, nested in this frame), their 64-bit exclusive
//      scan, and the batch ends: rays are cut, in array order, into batches whose hits fit the
//      budget (a ray with more hits than that is a batch of its own).  One single-workgroup
//      kernel does scan and cuts; the host reads back the cut table -- O(batches) values, one
//      synchronisation -- and never the per-ray counts.
//   2. per batch: offsets rebased to the batch, the per-hit walk on the ray sub-range (nested:
//      it carves from this frame and leaves the automatic ray cache alone), then the fused
//      kernel below, once per tier.
//
// The fused kernel orders a ray's hits by (distance, sphere index) and composites them, one
// workgroup per ray.  All three tiers run the same code on three arrays of 32-bit words (the
// order-preserving bits of the distance, the sphere index, the integral's bits); they differ in
// where the arrays live and in the workgroup's size:
//   wave   n <= ORD_WAVE_MAX    64 threads,  arrays in LDS ( 6 KiB)
//   block  n <= ORD_BLOCK_MAX   256 threads, arrays in LDS (72 KiB: two workgroups per CU)
//   global longer rays          256 threads, in place in the batch's per-hit arrays
// Sort: a bitonic network whose comparators all point the same way (the first step of every
// merge compares i with its mirror image in the block, the others are half-cleaners), so a ray
// of any length n sorts as if padded to a power of two with +inf keys that are never stored:
// a comparator whose upper end is >= n is skipped.  Keys are distinct (a ray hits a sphere
// once), so the result is the contract's total order whatever the traversal wrote.
// Composite: fp64.  tau_k is carry + (sums of the waves before) + (exclusive wave scan), the
// carry running over groups of blockDim hits; hit k's factor I phi(a) exp(-tau) replaces its
// distance/integral words; then four channels per pass, hit k on thread k mod blockDim, a
// butterfly over the wave and the waves in order.  Every addition's place is a function of k
// and n alone: results do not depend on packets, batches or neighbours.

#include "common.hpp"

#include <vector>

namespace grace_hip {
namespace {

constexpr int ORD_WAVE_MAX = 512, ORD_BLOCK_MAX = 6144;
constexpr int ORD_TABLE_HEAD = 8;          // batches, hits, rays per tier (wave, block, global), spare
constexpr size_t ORD_TABLE_FIRST = 4096;   // table words read back with the first (usually only) copy
constexpr size_t ORD_DEFAULT_BUDGET = size_t(1) << 30;
constexpr size_t ORD_HIT_BYTES = 12;       // index, integral, distance

size_t g_budget = ORD_DEFAULT_BUDGET;
bool g_stats_on = false;
grace_ordered_stats g_stats = {};

// ---- counts -> 64-bit offsets, tier census, batch ends -----------------------------------------
__global__ __launch_bounds__(1024) void ordered_scan_cut_kernel(const int* __restrict__ counts, const int n,
                                                               const long long cap, long long* __restrict__ offs,
                                                               long long* __restrict__ table)
{
    __shared__ long long s_sum[1024];
    __shared__ unsigned long long s_tier[3];
    const int tid = threadIdx.x;
    if (tid < 3) s_tier[tid] = 0;
    const long long per = (static_cast<long long>(n) + 1023) / 1024;
    const long long b = per * tid < n ? per * tid : n, e = b + per < n ? b + per : n;
    long long sum = 0;
    unsigned long long tier[3] = { 0, 0, 0 };
    for (long long i = b; i < e; ++i) {
        const int c = counts[i];
        sum += c;
        ++tier[c <= ORD_WAVE_MAX ? 0 : c <= ORD_BLOCK_MAX ? 1 : 2];
    }
    s_sum[tid] = sum;
    __syncthreads();
    for (int t = 0; t < 3; ++t) if (tier[t]) atomicAdd(&s_tier[t], tier[t]);
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < 1024; ++t) { const long long v = s_sum[t]; s_sum[t] = run; run += v; }
        offs[n] = run;
        table[1] = run;
    }
    __syncthreads();
    long long run = s_sum[tid];
    for (long long i = b; i < e; ++i) { offs[i] = run; run += counts[i]; }
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        long long nb = 0;
        while (s < n) {
            const long long limit = offs[s] + cap;
            int lo = s + 1, hi = n;          // the last end whose hits fit; s + 1 if none does
            while (lo < hi) {
                const int mid = lo + (hi - lo + 1) / 2;
                if (offs[mid] <= limit) lo = mid; else hi = mid - 1;
            }
            table[ORD_TABLE_HEAD + nb++] = lo;
            s = lo;
        }
        table[0] = nb;
        table[2] = s_tier[0]; table[3] = s_tier[1]; table[4] = s_tier[2];
    }
}

__global__ void ordered_rebase_kernel(const long long* __restrict__ offs, const int n, int* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = static_cast<int>(offs[i] - offs[0]);
}

// ---- the fused sort + composite -----------------------------------------------------------------
struct OrdArgs {
    const long long* offs;     // [n_rays + 1], of the whole call
    int ray0;                  // the batch's first ray: its per-hit arrays start at offs[ray0]
    int* hit_idx; float* hit_integral; float* hit_dist;   // the batch's per-hit arrays
    const float* emission; int channels; const float* absorption;
    float* out; float* tau;
};

// fp32 order (with -0 == +0) as unsigned order
__device__ __forceinline__ uint32_t dist_key(const float d)
{
    const uint32_t u = __float_as_uint(d + 0.0f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

template <int T>
__device__ __forceinline__ void ordered_sort(uint32_t* D, int* X, uint32_t* I, const int n, const int tid)
{
    int N = 1;
    while (N < n) N <<= 1;
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const bool mirror = j == (k >> 1);
            for (int t = tid; t < (N >> 1); t += T) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = mirror ? (i ^ (k - 1)) : (i + j);
                if (l < n) {
                    const uint32_t di = D[i], dl = D[l];
                    const int xi = X[i], xl = X[l];
                    if (di > dl || (di == dl && xi > xl)) {
                        D[i] = dl; D[l] = di; X[i] = xl; X[l] = xi;
                        const uint32_t ii = I[i]; I[i] = I[l]; I[l] = ii;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// TIER 0 / 1: arrays of CAP hits in LDS; TIER 2: in place in global memory.
template <int T, int CAP, int TIER>
__global__ __launch_bounds__(T) void ordered_composite_kernel(const OrdArgs a)
{
    constexpr int WAVES = T / 64;
    __shared__ uint32_t s_d[CAP ? CAP : 1];
    __shared__ int s_x[CAP ? CAP : 1];
    __shared__ uint32_t s_i[CAP ? CAP : 1];
    __shared__ double s_wave[WAVES];
    __shared__ double s_red[WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r = size_t(a.ray0) + blockIdx.x;
    const long long o0 = a.offs[r];
    const long long n64 = a.offs[r + 1] - o0;
    if (TIER == 0 ? n64 > ORD_WAVE_MAX
                  : TIER == 1 ? (n64 <= ORD_WAVE_MAX || n64 > ORD_BLOCK_MAX) : n64 <= ORD_BLOCK_MAX) return;
    const int n = static_cast<int>(n64);
    const size_t h0 = size_t(o0 - a.offs[a.ray0]);
    uint32_t *D, *I;
    int* X;
    if (CAP) {
        D = s_d; X = s_x; I = s_i;
        for (int k = tid; k < n; k += T) {
            D[k] = dist_key(a.hit_dist[h0 + k]);
            X[k] = a.hit_idx[h0 + k];
            I[k] = __float_as_uint(a.hit_integral[h0 + k]);
        }
    } else {
        D = reinterpret_cast<uint32_t*>(a.hit_dist) + h0;
        X = a.hit_idx + h0;
        I = reinterpret_cast<uint32_t*>(a.hit_integral) + h0;
        for (int k = tid; k < n; k += T) D[k] = dist_key(__uint_as_float(D[k]));
    }
    __syncthreads();
    ordered_sort<T>(D, X, I, n, tid);

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
        if (WAVES > 1) {
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

struct Events {     // per-phase timing for the stats hook
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    grace_status mark(hipStream_t stream)
    {
        hipEvent_t e = nullptr;
        GRACE_TRY_HIP(hipEventCreate(&e));
        ev.push_back(e);
        GRACE_TRY_HIP(hipEventRecord(e, stream));
        return GRACE_OK;
    }
};

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
    GRACE_REQUIRE(n_channels >= 1 && n_channels <= 64, "trace_emission_absorption: channels must be 1..64");
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_emission && d_absorption, "trace_emission_absorption: null weights");
    GRACE_REQUIRE(d_out, "trace_emission_absorption: null output");
    GRACE_REQUIRE(d_rays && d_spheres && d_nodes && d_leaves && d_root, "trace_emission_absorption: null pointer");
    GRACE_REQUIRE(n_rays < (size_t(1) << 31), "trace_emission_absorption: bad ray count");
    GRACE_REQUIRE(n_nodes >= 1 && n_nodes < (size_t(1) << 30), "trace_emission_absorption: bad node count");
    GRACE_REQUIRE(n_spheres > 0 && n_spheres < (size_t(1) << 31), "trace_emission_absorption: bad primitive count");
    const hipStream_t stream = as_stream(stream_);
    const bool stats = g_stats_on;
    const char* rays = static_cast<const char*>(d_rays);
    const size_t ray_bytes = 28;

    // ---- 1. counts, offsets, batch ends ---------------------------------------------------------
    size_t nested_all = 0;
    GRACE_TRY(trace_nested_bytes(n_rays, n_spheres, n_nodes, &nested_all));
    const size_t table_words = ORD_TABLE_HEAD + n_rays;
    const size_t off_counts = 0, off_offs = off_counts + Workspace::aligned(n_rays * sizeof(int)),
                 off_table = off_offs + Workspace::aligned((n_rays + 1) * sizeof(long long)),
                 own = off_table + Workspace::aligned(table_words * sizeof(long long));
    FrameGuard frame;
    GRACE_TRY(frame.begin(own + nested_all, stream));
    (void)Workspace::take<char>(own);
    const size_t mark = Workspace::mark();
    int* counts = reinterpret_cast<int*>(Workspace::base() + off_counts);
    long long* offs = reinterpret_cast<long long*>(Workspace::base() + off_offs);
    long long* table = reinterpret_cast<long long*>(Workspace::base() + off_table);
    Events ev;
    if (stats) GRACE_TRY(ev.mark(stream));
    GRACE_TRY(trace_hitcounts_nested(d_rays, n_rays, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root,
                                     counts, stream));
    Workspace::rewind(mark);
    size_t cap = g_budget / ORD_HIT_BYTES;
    if (cap > size_t(INT32_MAX)) cap = size_t(INT32_MAX);     // a batch's offsets are 32-bit
    if (cap < 1) cap = 1;
    ordered_scan_cut_kernel<<<1, 1024, 0, stream>>>(counts, int(n_rays), static_cast<long long>(cap), offs, table);
    GRACE_CHECK_LAUNCH();
    if (stats) GRACE_TRY(ev.mark(stream));
    std::vector<long long> h_table(table_words < ORD_TABLE_FIRST ? table_words : ORD_TABLE_FIRST);
    GRACE_TRY_HIP(hipMemcpyAsync(h_table.data(), table, h_table.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    GRACE_TRY_HIP(hipStreamSynchronize(stream));
    const size_t n_batches = size_t(h_table[0]);
    GRACE_REQUIRE(n_batches >= 1 && n_batches <= n_rays, "trace_emission_absorption: bad batch table");
    if (ORD_TABLE_HEAD + n_batches > h_table.size()) {       // (more batches than the first copy holds)
        const size_t have = h_table.size();
        h_table.resize(ORD_TABLE_HEAD + n_batches);
        GRACE_TRY_HIP(hipMemcpyAsync(h_table.data() + have, table + have, (h_table.size() - have) * sizeof(long long),
                                     hipMemcpyDeviceToHost, stream));
        GRACE_TRY_HIP(hipStreamSynchronize(stream));
    }
    const bool any_block = h_table[3] != 0, any_global = h_table[4] != 0;

    // ---- 2. the batches -----------------------------------------------------------------------
    // The frame holds, behind this call's arrays, the largest batch's offsets and per-hit arrays
    // and the nested walk's own buffers.  Per-batch hit totals are not read back: a batch of more
    // than one ray holds at most `cap` hits, a batch of one ray at most n_spheres.
    size_t max_rays = 0, nested_max = 0, last_size = 0;
    bool single = false;
    for (size_t b = 0, s = 0; b < n_batches; ++b) {
        const size_t e = size_t(h_table[ORD_TABLE_HEAD + b]), nb = e - s;
        GRACE_REQUIRE(e > s && e <= n_rays, "trace_emission_absorption: bad batch table");
        if (nb > max_rays) max_rays = nb;
        if (nb == 1) single = true;
        if (nb != last_size) {
            size_t need = 0;
            GRACE_TRY(trace_nested_bytes(nb, n_spheres, n_nodes, &need));
            if (need > nested_max) nested_max = need;
            last_size = nb;
        }
        s = e;
    }
    size_t max_hits = max_rays > 1 ? cap : 0;
    if (single && n_spheres > max_hits) max_hits = n_spheres;
    if (size_t(h_table[1]) < max_hits) max_hits = size_t(h_table[1]);
    const size_t hits_stride = Workspace::aligned(max_hits * sizeof(int));
    const size_t per_batch = Workspace::aligned(max_rays * sizeof(int)) + 3 * hits_stride;
    GRACE_TRY(Workspace::grow_frame(mark + per_batch + nested_max, stream));
    offs = reinterpret_cast<long long*>(Workspace::base() + off_offs);
    int* off32 = Workspace::take<int>(max_rays);
    int* hit_idx = reinterpret_cast<int*>(Workspace::take<char>(hits_stride));
    float* hit_integral = reinterpret_cast<float*>(Workspace::take<char>(hits_stride));
    float* hit_dist = reinterpret_cast<float*>(Workspace::take<char>(hits_stride));
    const size_t batch_mark = Workspace::mark();

    for (size_t b = 0, s = 0; b < n_batches; ++b) {
        const size_t e = size_t(h_table[ORD_TABLE_HEAD + b]), nb = e - s;
        Workspace::rewind(batch_mark);
        ordered_rebase_kernel<<<ceil_div(nb, 256), 256, 0, stream>>>(offs + s, int(nb), off32);
        GRACE_CHECK_LAUNCH();
        if (stats) GRACE_TRY(ev.mark(stream));
        if (h_table[1] != 0)
            GRACE_TRY(trace_hits_nested(rays + s * ray_bytes, nb, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves,
                                        d_root, off32, hit_idx, hit_integral, hit_dist, stream));
        if (stats) GRACE_TRY(ev.mark(stream));
        OrdArgs a;
        a.offs = offs; a.ray0 = int(s);
        a.hit_idx = hit_idx; a.hit_integral = hit_integral; a.hit_dist = hit_dist;
        a.emission = d_emission; a.channels = n_channels; a.absorption = d_absorption;
        a.out = d_out; a.tau = d_tau;
        ordered_composite_kernel<64, ORD_WAVE_MAX, 0><<<int(nb), 64, 0, stream>>>(a);
        GRACE_CHECK_LAUNCH();
        if (any_block) {
            ordered_composite_kernel<256, ORD_BLOCK_MAX, 1><<<int(nb), 256, 0, stream>>>(a);
            GRACE_CHECK_LAUNCH();
        }
        if (any_global) {
            ordered_composite_kernel<256, 0, 2><<<int(nb), 256, 0, stream>>>(a);
            GRACE_CHECK_LAUNCH();
        }
        if (stats) GRACE_TRY(ev.mark(stream));
        s = e;
    }
    if (stats) {
        GRACE_TRY_HIP(hipStreamSynchronize(stream));
        grace_ordered_stats st = {};
        st.batches = n_batches; st.total_hits = static_cast<unsigned long long>(h_table[1]);
        st.rays_wave = static_cast<unsigned long long>(h_table[2]);
        st.rays_block = static_cast<unsigned long long>(h_table[3]);
        st.rays_global = static_cast<unsigned long long>(h_table[4]);
        st.budget_bytes = g_budget; st.frame_bytes = mark + per_batch + nested_max;
        float ms = 0.f;
        GRACE_TRY_HIP(hipEventElapsedTime(&ms, ev.ev[0], ev.ev[1]));
        st.ms_count = ms;
        for (size_t b = 0; b < n_batches; ++b) {
            GRACE_TRY_HIP(hipEventElapsedTime(&ms, ev.ev[2 + 3 * b], ev.ev[3 + 3 * b]));
            st.ms_trace += ms;
            GRACE_TRY_HIP(hipEventElapsedTime(&ms, ev.ev[3 + 3 * b], ev.ev[4 + 3 * b]));
            st.ms_composite += ms;
        }
        g_stats = st;
    }
    return GRACE_OK;
}

grace_status grace_trace_set_ordered_budget(size_t bytes)
{
    g_budget = bytes ? bytes : ORD_DEFAULT_BUDGET;
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
    g_stats_on = enabled != 0;
    if (!g_stats_on) g_stats = grace_ordered_stats();
    return GRACE_OK;
}

grace_status grace_trace_ordered_last_stats(grace_ordered_stats* h_stats)
{
    GRACE_REQUIRE(h_stats, "trace_ordered_last_stats: null output");
    GRACE_REQUIRE(g_stats_on, "trace_ordered_last_stats: statistics are not enabled");
    *h_stats = g_stats;
    return GRACE_OK;
}

} // extern "C"
