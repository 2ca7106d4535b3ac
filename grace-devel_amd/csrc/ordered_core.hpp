// Pieces shared by the depth-ordered traces (ordered.hip, deposit.hip, spectra.hip): the tier limits, counts ->
// 64-bit offsets and batch ends, the load + sort of one ray's hits, and the host sequence that
// counts, cuts and walks the batches.  The kernels and device functions have internal linkage:
// each including translation unit gets its own copies.  The budget and the stats hook are
// process-wide and defined once, in ordered.hip.  gfx950 only.
//
// The sequence, on the caller's stream and inside ONE workspace frame:
//   1. hit counts of all rays (the counting walk, nested in this frame), their 64-bit exclusive
//      scan, and the batch ends: rays are cut, in array order, into batches whose hits fit the
//      budget (a ray with more hits than that is a batch of its own).  One single-workgroup
//      kernel does scan and cuts; the host reads back the cut table -- O(batches) values, one
//      synchronisation -- and never the per-ray counts.
//   2. per batch: offsets rebased to the batch, the per-hit walk on the ray sub-range (nested:
//      it carves from this frame and leaves the automatic ray cache alone), then the caller's
//      fused kernel, once per tier.
//
// A fused kernel orders a ray's hits by (distance, sphere index), one workgroup per ray.  The
// tiers run the same code on three arrays of 32-bit words (the order-preserving bits of the
// distance, the sphere index, the integral's bits); they differ in where the arrays live and in
// the workgroup's size:
//   wave   n <= ORD_WAVE_MAX    64 threads,  arrays in LDS ( 6 KiB)
//   block  n <= ORD_BLOCK_MAX   256 threads, arrays in LDS (72 KiB: two workgroups per CU)
//   global longer rays          256 threads, in place in the batch's per-hit arrays
// Sort: a bitonic network whose comparators all point the same way (the first step of every
// merge compares i with its mirror image in the block, the others are half-cleaners), so a ray
// of any length n sorts as if padded to a power of two with +inf keys that are never stored:
// a comparator whose upper end is >= n is skipped.  Keys are distinct (a ray hits a sphere
// once), so the result is the contract's total order whatever the traversal wrote.
#pragma once

#include "common.hpp"

#include <vector>

namespace grace_hip {

extern size_t g_ordered_budget;
extern bool g_ordered_stats_on;
extern grace_ordered_stats g_ordered_stats;

namespace {

constexpr int ORD_WAVE_MAX = 512, ORD_BLOCK_MAX = 6144;
constexpr int ORD_TABLE_HEAD = 8;          // batches, hits, rays per tier (wave, block, global), spare
constexpr size_t ORD_TABLE_FIRST = 4096;   // table words read back with the first (usually only) copy
constexpr size_t ORD_DEFAULT_BUDGET = size_t(1) << 30;
constexpr size_t ORD_HIT_BYTES = 12;       // index, integral, distance

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

// ---- one ray's hits, loaded and sorted ------------------------------------------------------------
struct OrdBatch {              // what every fused kernel's argument block starts with
    const long long* offs;     // [n_rays + 1], of the whole call
    int ray0;                  // the batch's first ray: its per-hit arrays start at offs[ray0]
    int* hit_idx; float* hit_integral; float* hit_dist;   // the batch's per-hit arrays
};

// fp32 order (with -0 == +0) as unsigned order
__device__ __forceinline__ uint32_t dist_key(const float d)
{
    const uint32_t u = __float_as_uint(d + 0.0f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
// ... and back: the distance a key was made from (a zero comes back as +0)
__device__ __forceinline__ float dist_from_key(const uint32_t k)
{
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
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

// Workgroup blockIdx.x of a fused kernel <T, CAP, TIER>: its ray r, the ray's n hits in D / X / I
// (distance keys, sphere indices, integral bits), sorted.  TIER 0 / 1: the arrays are the CAP-word
// LDS arrays s_d / s_x / s_i; TIER 2: in place in global memory.  False if the ray belongs to
// another tier (uniform over the workgroup: return at once).
template <int T, int CAP, int TIER>
__device__ __forceinline__ bool ordered_load_sort(const OrdBatch& a, uint32_t* s_d, int* s_x, uint32_t* s_i,
                                                  uint32_t*& D, int*& X, uint32_t*& I, int& n, size_t& r)
{
    const int tid = threadIdx.x;
    r = size_t(a.ray0) + blockIdx.x;
    const long long o0 = a.offs[r];
    const long long n64 = a.offs[r + 1] - o0;
    if (TIER == 0 ? n64 > ORD_WAVE_MAX
                  : TIER == 1 ? (n64 <= ORD_WAVE_MAX || n64 > ORD_BLOCK_MAX) : n64 <= ORD_BLOCK_MAX) return false;
    n = static_cast<int>(n64);
    const size_t h0 = size_t(o0 - a.offs[a.ray0]);
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
    return true;
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

// ---- the host sequence ----------------------------------------------------------------------------
// frame: the caller's, not yet open; it stays open when the sequence returns, so the caller may
// still launch on what the front region holds.  front_bytes: room the caller wants in the frame in front of the per-batch region, where it
// survives all batches.  front(p) is called once with its address, after the frame has reached its
// final place and before the first batch; launch(batch, n_batch_rays, any_block, any_global) runs
// the caller's fused kernels on one batch (any_*: the census found rays in that tier).
template <typename Front, typename Launch>
grace_status ordered_run(FrameGuard& frame, const void* d_rays, const size_t n_rays, const float* d_spheres, const size_t n_spheres,
                         const int* d_nodes, const size_t n_nodes, const int* d_leaves, const int* d_root,
                         const size_t front_bytes, const hipStream_t stream, Front front, Launch launch)
{
    const bool stats = g_ordered_stats_on;
    const char* rays = static_cast<const char*>(d_rays);
    const size_t ray_bytes = 28;

    // ---- 1. counts, offsets, batch ends ---------------------------------------------------------
    size_t nested_all = 0;
    GRACE_TRY(trace_nested_bytes(n_rays, n_spheres, n_nodes, &nested_all));
    const size_t table_words = ORD_TABLE_HEAD + n_rays;
    const size_t off_counts = 0, off_offs = off_counts + Workspace::aligned(n_rays * sizeof(int)),
                 off_table = off_offs + Workspace::aligned((n_rays + 1) * sizeof(long long)),
                 off_front = off_table + Workspace::aligned(table_words * sizeof(long long)),
                 own = off_front + Workspace::aligned(front_bytes);
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
    size_t cap = g_ordered_budget / ORD_HIT_BYTES;
    if (cap > size_t(INT32_MAX)) cap = size_t(INT32_MAX);     // a batch's offsets are 32-bit
    if (cap < 1) cap = 1;
    ordered_scan_cut_kernel<<<1, 1024, 0, stream>>>(counts, int(n_rays), static_cast<long long>(cap), offs, table);
    GRACE_CHECK_LAUNCH();
    if (stats) GRACE_TRY(ev.mark(stream));
    std::vector<long long> h_table(table_words < ORD_TABLE_FIRST ? table_words : ORD_TABLE_FIRST);
    GRACE_TRY_HIP(hipMemcpyAsync(h_table.data(), table, h_table.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    GRACE_TRY_HIP(hipStreamSynchronize(stream));
    const size_t n_batches = size_t(h_table[0]);
    GRACE_REQUIRE(n_batches >= 1 && n_batches <= n_rays, "ordered trace: bad batch table");
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
        GRACE_REQUIRE(e > s && e <= n_rays, "ordered trace: bad batch table");
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
    GRACE_TRY(front(Workspace::base() + off_front));

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
        OrdBatch batch;
        batch.offs = offs; batch.ray0 = int(s);
        batch.hit_idx = hit_idx; batch.hit_integral = hit_integral; batch.hit_dist = hit_dist;
        GRACE_TRY(launch(batch, int(nb), any_block, any_global));
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
        st.budget_bytes = g_ordered_budget; st.frame_bytes = mark + per_batch + nested_max;
        float ms = 0.f;
        GRACE_TRY_HIP(hipEventElapsedTime(&ms, ev.ev[0], ev.ev[1]));
        st.ms_count = ms;
        for (size_t b = 0; b < n_batches; ++b) {
            GRACE_TRY_HIP(hipEventElapsedTime(&ms, ev.ev[2 + 3 * b], ev.ev[3 + 3 * b]));
            st.ms_trace += ms;
            GRACE_TRY_HIP(hipEventElapsedTime(&ms, ev.ev[3 + 3 * b], ev.ev[4 + 3 * b]));
            st.ms_composite += ms;
        }
        g_ordered_stats = st;
    }
    return GRACE_OK;
}

} // namespace
} // namespace grace_hip
