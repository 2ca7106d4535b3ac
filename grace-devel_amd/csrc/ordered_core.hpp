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
//
// The GROUPED variant (the periodic traces; grace_hip.h, "Periodic boxes for traces", "Ordered
// traces"): the traced rays are the SEGMENTS of the caller's rays, groups[r] .. groups[r + 1] ray
// r's.  The counting walk and offs stay per segment; the scan kernel checks groups, takes the
// census per ray and cuts the batches at ray boundaries ({ray end, segment end, hits} per batch);
// a batch's per-hit walk runs on its segments, the fused kernels get one workgroup per ray.  A
// ray's hits are contiguous and already grouped by segment, so the order (segment, distance,
// image index) is each segment's slice sorted in turn; then every hit's image index becomes its
// source, the caller's particle, and the composites run unchanged.  A compile-time variant: the
// GROUPED = false instantiations are the open calls'.
#pragma once

#include "common.hpp"
#include "trace_state.hpp"

#include <vector>

namespace grace_hip {

extern size_t g_ordered_budget;
extern bool g_ordered_stats_on;
extern grace_ordered_stats g_ordered_stats;

namespace {

constexpr int ORD_WAVE_MAX = 512, ORD_BLOCK_MAX = 6144;
constexpr int ORD_TABLE_HEAD = 8;          // batches, hits, rays per tier (wave, block, global), the grouped form's two flags, spare
constexpr int ORD_TABLE_BAD_GROUPS = 5, ORD_TABLE_LONG_RAY = 6;
constexpr int ORD_MAX_SEGMENTS = 65536;    // per ray of a grouped call (periodic_trace.hip's MAX_SEGMENTS)
constexpr size_t ORD_TABLE_FIRST = 4096;   // table words read back with the first (usually only) copy
constexpr size_t ORD_DEFAULT_BUDGET = size_t(1) << 30;
constexpr size_t ORD_HIT_BYTES = 12;       // index, integral, distance

// ---- counts -> 64-bit offsets, tier census, batch ends -----------------------------------------
// GROUPED (the periodic traces): the n counted items are ray SEGMENTS, ray r's are
// groups[r] .. groups[r + 1]; a ray's hits are those of all its segments, the census and the cuts
// are per ray, and the table holds three words per batch {ray end, segment end, hits}.  groups is a
// caller array: it is checked here, before anything is indexed with it; a bad one (or a ray whose
// hits do not fit a batch's 32-bit offsets) leaves no batch, a flag in the table and the status word.
template <bool GROUPED>
__global__ __launch_bounds__(1024) void ordered_scan_cut_kernel(const int* __restrict__ counts, const int n,
                                                               const long long cap, long long* __restrict__ offs,
                                                               long long* __restrict__ table,
                                                               const int* __restrict__ groups, const int n_rays,
                                                               int* __restrict__ status)
{
    __shared__ long long s_sum[1024];
    __shared__ unsigned long long s_tier[3];
    __shared__ int s_bad[2];
    const int tid = threadIdx.x;
    if (tid < 3) s_tier[tid] = 0;
    const long long rper = (static_cast<long long>(n_rays) + 1023) / 1024;      // (GROUPED: this thread's rays)
    const long long rb = rper * tid < n_rays ? rper * tid : n_rays, re = rb + rper < n_rays ? rb + rper : n_rays;
    if constexpr (GROUPED) {
        if (tid < 2) s_bad[tid] = 0;
        __syncthreads();
        bool bad = tid == 0 && (groups[0] != 0 || groups[n_rays] != n);
        for (long long i = rb; i < re; ++i) {
            const int g0 = groups[i], g1 = groups[i + 1];
            bad = bad || g0 < 0 || g1 < g0 || g1 > n || g1 - g0 > ORD_MAX_SEGMENTS;
        }
        if (bad) s_bad[0] = 1;
        __syncthreads();
        if (s_bad[0]) {
            if (tid == 0) {
                table[0] = 0; table[ORD_TABLE_BAD_GROUPS] = 1; table[ORD_TABLE_LONG_RAY] = 0;
                atomicMax(status, int(GRACE_INVALID_ARGUMENT));
            }
            return;
        }
    }
    const long long per = (static_cast<long long>(n) + 1023) / 1024;
    const long long b = per * tid < n ? per * tid : n, e = b + per < n ? b + per : n;
    long long sum = 0;
    unsigned long long tier[3] = { 0, 0, 0 };
    for (long long i = b; i < e; ++i) {
        const int c = counts[i];
        sum += c;
        if constexpr (!GROUPED) ++tier[c <= ORD_WAVE_MAX ? 0 : c <= ORD_BLOCK_MAX ? 1 : 2];
    }
    s_sum[tid] = sum;
    __syncthreads();
    if constexpr (!GROUPED)
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
    if constexpr (GROUPED) {
        bool too_long = false;
        for (long long i = rb; i < re; ++i) {
            const long long c = offs[groups[i + 1]] - offs[groups[i]];
            too_long = too_long || c > static_cast<long long>(INT32_MAX);
            ++tier[c <= ORD_WAVE_MAX ? 0 : c <= ORD_BLOCK_MAX ? 1 : 2];
        }
        for (int t = 0; t < 3; ++t) if (tier[t]) atomicAdd(&s_tier[t], tier[t]);
        if (too_long) s_bad[1] = 1;
        __syncthreads();
        if (tid == 0) {
            table[ORD_TABLE_BAD_GROUPS] = 0; table[ORD_TABLE_LONG_RAY] = s_bad[1];
            int s = 0;
            long long nb = 0;
            if (s_bad[1]) { s = n_rays; atomicMax(status, int(GRACE_INVALID_ARGUMENT)); }      // no batch
            while (s < n_rays) {
                const long long first = offs[groups[s]], limit = first + cap;
                int lo = s + 1, hi = n_rays;     // the last ray end whose hits fit; s + 1 if none does
                while (lo < hi) {
                    const int mid = lo + (hi - lo + 1) / 2;
                    if (offs[groups[mid]] <= limit) lo = mid; else hi = mid - 1;
                }
                long long* row = table + ORD_TABLE_HEAD + 3 * nb++;
                row[0] = lo; row[1] = groups[lo]; row[2] = offs[groups[lo]] - first;
                s = lo;
            }
            table[0] = nb;
            table[2] = s_tier[0]; table[3] = s_tier[1]; table[4] = s_tier[2];
        }
        return;
    }
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
    // What the GROUPED variant reads (null / 0 in an open call).  offs is then per SEGMENT,
    // [n_segments + 1], ray0 still the batch's first ray: its arrays start at offs[groups[ray0]].
    const int* groups;         // ray -> first segment, [n_rays + 1]
    const int* source;         // image -> the caller's particle, [n_images]
    int n_sources, n_segments;
    const double* seg_t0;      // segment -> its starting parameter along its ray (spectra only)
    int* status;               // the context's status word
};

// A ray's segments and where its hits start in offs (GROUPED; in an open call the ray itself).
struct OrdSpan { int g0, g1; long long o0; };

// groups[i] as the kernels use it: within [0, n_segments] whatever the array holds.
__device__ __forceinline__ int ordered_group(const OrdBatch& a, const size_t i)
{
    const int g = a.groups[i];
    return g < 0 ? 0 : g > a.n_segments ? a.n_segments : g;
}

// The segment of ray `span` that holds the ray's hit k (k < the ray's total): the last s in
// [g0, g1) with offs[s] - o0 <= k.
__device__ __forceinline__ int ordered_segment_of(const OrdBatch& a, const OrdSpan& span, const int k)
{
    int lo = span.g0, hi = span.g1 - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (a.offs[mid] - span.o0 <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

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
//
// GROUPED: the ray's hits are those of its segments groups[r] .. groups[r + 1], contiguous in offs
// and already grouped by segment; the tier goes by their total.  The order is (segment, distance
// within the segment, image index): each segment's slice is sorted in turn (the slices' bounds are
// uniform over the workgroup, so every thread meets the same barriers; a slice of fewer than two
// hits has none), then X[k] = source[X[k]], and the composites run as in an open call.  An image
// whose source is outside [0, n_sources) keeps its place with a zero integral -- it contributes
// nothing -- and sets the status word.  span: the ray's segments, for the caller's own look-ups.
template <int T, int CAP, int TIER, bool GROUPED>
__device__ __forceinline__ bool ordered_load_sort(const OrdBatch& a, uint32_t* s_d, int* s_x, uint32_t* s_i,
                                                  uint32_t*& D, int*& X, uint32_t*& I, int& n, size_t& r,
                                                  OrdSpan& span)
{
    const int tid = threadIdx.x;
    r = size_t(a.ray0) + blockIdx.x;
    size_t first = r, batch_first = size_t(a.ray0);      // in offs: the ray's and the batch's first entries
    size_t last = r + 1;
    if constexpr (GROUPED) {
        first = size_t(ordered_group(a, r));
        last = size_t(ordered_group(a, r + 1));
        if (last < first) last = first;
        if (last - first > size_t(ORD_MAX_SEGMENTS)) last = first + size_t(ORD_MAX_SEGMENTS);
        batch_first = size_t(ordered_group(a, size_t(a.ray0)));
    }
    const long long o0 = a.offs[first];
    const long long n64 = a.offs[last] - o0;
    span.g0 = int(first); span.g1 = int(last); span.o0 = o0;
    if (TIER == 0 ? n64 > ORD_WAVE_MAX
                  : TIER == 1 ? (n64 <= ORD_WAVE_MAX || n64 > ORD_BLOCK_MAX) : n64 <= ORD_BLOCK_MAX) return false;
    n = static_cast<int>(n64);
    const size_t h0 = size_t(o0 - a.offs[batch_first]);
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
    if constexpr (GROUPED) {
        for (size_t s = first; s < last; ++s) {
            const int b = static_cast<int>(a.offs[s] - o0), m = static_cast<int>(a.offs[s + 1] - a.offs[s]);
            if (m >= 2) ordered_sort<T>(D + b, X + b, I + b, m, tid);
        }
        bool bad = false;
        for (int k = tid; k < n; k += T) {
            int i = a.source[X[k]];
            if (i < 0 || i >= a.n_sources) { bad = true; i = 0; I[k] = 0u; }
            X[k] = i;
        }
        if (bad) atomicMax(a.status, int(GRACE_INVALID_ARGUMENT));
        __syncthreads();
    } else {
        ordered_sort<T>(D, X, I, n, tid);
    }
    return true;
}

template <int T, int CAP, int TIER>
__device__ __forceinline__ bool ordered_load_sort(const OrdBatch& a, uint32_t* s_d, int* s_x, uint32_t* s_i,
                                                  uint32_t*& D, int*& X, uint32_t*& I, int& n, size_t& r)
{
    OrdSpan span;
    return ordered_load_sort<T, CAP, TIER, false>(a, s_d, s_x, s_i, D, X, I, n, r, span);
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
// What a grouped call (the periodic traces) adds: the traced rays are SEGMENTS, ray r's are
// groups[r] .. groups[r + 1]; batches are cut at ray boundaries, the per-hit walk runs on a batch's
// segments, and the fused kernels get one workgroup per RAY of the batch.
struct OrdGroups {
    const int* groups; size_t n_rays;
    const int* source; size_t n_sources;
    const double* seg_t0;
};

// The host-side checks every periodic entry point makes on the arrays a grouped call adds (what they
// HOLD is checked on the device, in the scan kernel and the fused kernels).
inline grace_status ordered_groups(OrdGroups& g, const void* d_segments, const size_t n_segments,
                                   const int* d_segment_offsets, const size_t n_rays, const int* d_source,
                                   const size_t n_sources, const double* d_segment_t0)
{
    GRACE_REQUIRE(n_rays < (size_t(1) << 31), "periodic ordered trace: bad ray count");
    GRACE_REQUIRE(d_segments && n_segments >= 1 && n_segments < (size_t(1) << 31),
                  "periodic ordered trace: no segments, or more than INT32_MAX");
    GRACE_REQUIRE(d_segment_offsets && d_source, "periodic ordered trace: null segment offsets or sources");
    GRACE_REQUIRE(n_sources >= 1 && n_sources < (size_t(1) << 31), "periodic ordered trace: bad source count");
    g.groups = d_segment_offsets; g.n_rays = n_rays;
    g.source = d_source; g.n_sources = n_sources;
    g.seg_t0 = d_segment_t0;
    return GRACE_OK;
}

// frame: the caller's, not yet open; it stays open when the sequence returns, so the caller may
// still launch on what the front region holds.  front_bytes: room the caller wants in the frame in front of the per-batch region, where it
// survives all batches.  front(p) is called once with its address, after the frame has reached its
// final place and before the first batch; launch(batch, n_batch_rays, any_block, any_global) runs
// the caller's fused kernels on one batch (any_*: the census found rays in that tier).
// grouped (or null: an open call): n_rays then counts the segments in d_rays, the table has three
// words per batch, and a bad groups array or a ray whose hits exceed a batch's 32-bit offsets is
// GRACE_INVALID_ARGUMENT before any batch is traced.
template <typename Front, typename Launch>
grace_status ordered_run(FrameGuard& frame, const void* d_rays, const size_t n_rays, const float* d_spheres, const size_t n_spheres,
                         const int* d_nodes, const size_t n_nodes, const int* d_leaves, const int* d_root,
                         const size_t front_bytes, const hipStream_t stream, Front front, Launch launch,
                         const OrdGroups* grouped = nullptr)
{
    const bool stats = g_ordered_stats_on;
    const char* rays = static_cast<const char*>(d_rays);
    const size_t ray_bytes = 28;
    const size_t n_cut = grouped ? grouped->n_rays : n_rays;      // what the batches are cut from
    const size_t row_words = grouped ? 3 : 1;                     // per batch: {ray end[, segment end, hits]}
    int* status = nullptr;
    if (grouped) {
        TraceState* ts = nullptr;
        GRACE_TRY(trace_state(&ts));
        GRACE_TRY(ensure_status(*ts, stream));
        status = ts->status;
    }

    // ---- 1. counts, offsets, batch ends ---------------------------------------------------------
    size_t nested_all = 0;
    GRACE_TRY(trace_nested_bytes(n_rays, n_spheres, n_nodes, &nested_all));
    const size_t table_words = ORD_TABLE_HEAD + row_words * n_cut;
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
    if (grouped)
        ordered_scan_cut_kernel<true><<<1, 1024, 0, stream>>>(counts, int(n_rays), static_cast<long long>(cap), offs,
                                                              table, grouped->groups, int(n_cut), status);
    else
        ordered_scan_cut_kernel<false><<<1, 1024, 0, stream>>>(counts, int(n_rays), static_cast<long long>(cap), offs,
                                                               table, nullptr, 0, nullptr);
    GRACE_CHECK_LAUNCH();
    if (stats) GRACE_TRY(ev.mark(stream));
    std::vector<long long> h_table(table_words < ORD_TABLE_FIRST ? table_words : ORD_TABLE_FIRST);
    GRACE_TRY_HIP(hipMemcpyAsync(h_table.data(), table, h_table.size() * sizeof(long long), hipMemcpyDeviceToHost, stream));
    GRACE_TRY_HIP(hipStreamSynchronize(stream));
    if (grouped) {
        GRACE_REQUIRE(h_table[ORD_TABLE_BAD_GROUPS] == 0,
                      "periodic ordered trace: the segment offsets must start at 0, not decrease, end at n_segments "
                      "and give a ray at most 65536 segments");
        GRACE_REQUIRE(h_table[ORD_TABLE_LONG_RAY] == 0,
                      "periodic ordered trace: one ray's hits over all its segments exceed INT32_MAX");
    }
    const size_t n_batches = size_t(h_table[0]);
    GRACE_REQUIRE(n_batches >= 1 && n_batches <= n_cut, "ordered trace: bad batch table");
    if (ORD_TABLE_HEAD + row_words * n_batches > h_table.size()) {       // (more batches than the first copy holds)
        const size_t have = h_table.size();
        h_table.resize(ORD_TABLE_HEAD + row_words * n_batches);
        GRACE_TRY_HIP(hipMemcpyAsync(h_table.data() + have, table + have, (h_table.size() - have) * sizeof(long long),
                                     hipMemcpyDeviceToHost, stream));
        GRACE_TRY_HIP(hipStreamSynchronize(stream));
    }
    const bool any_block = h_table[3] != 0, any_global = h_table[4] != 0;
    const long long* rows = h_table.data() + ORD_TABLE_HEAD;
    // the end of batch b in d_rays (an open call: its ray end; a grouped one: its segment end)
    const auto traced_end = [&](const size_t b) { return size_t(rows[row_words * b + (grouped ? 1 : 0)]); };

    // ---- 2. the batches -----------------------------------------------------------------------
    // The frame holds, behind this call's arrays, the largest batch's offsets and per-hit arrays
    // and the nested walk's own buffers.  An open call's per-batch hit totals are not read back: a
    // batch of more than one ray holds at most `cap` hits, a batch of one ray at most n_spheres.
    // A grouped call's ray hits up to n_spheres per segment: its table has the totals.
    size_t max_rays = 0, nested_max = 0, last_size = 0, max_hits = 0;
    bool single = false;
    for (size_t b = 0, s = 0, c = 0; b < n_batches; ++b) {
        const size_t e = traced_end(b), nb = e - s, ce = size_t(rows[row_words * b]);
        GRACE_REQUIRE(ce > c && ce <= n_cut && e >= s && e <= n_rays && (grouped || e > s), "ordered trace: bad batch table");
        if (nb > max_rays) max_rays = nb;
        if (nb == 1) single = true;
        if (nb != last_size && nb != 0) {
            size_t need = 0;
            GRACE_TRY(trace_nested_bytes(nb, n_spheres, n_nodes, &need));
            if (need > nested_max) nested_max = need;
            last_size = nb;
        }
        if (grouped) {
            GRACE_REQUIRE(rows[3 * b + 2] >= 0 && rows[3 * b + 2] <= h_table[1], "ordered trace: bad batch table");
            if (size_t(rows[3 * b + 2]) > max_hits) max_hits = size_t(rows[3 * b + 2]);
        }
        s = e; c = ce;
    }
    if (!grouped) {
        max_hits = max_rays > 1 ? cap : 0;
        if (single && n_spheres > max_hits) max_hits = n_spheres;
        if (size_t(h_table[1]) < max_hits) max_hits = size_t(h_table[1]);
    }
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

    for (size_t b = 0, s = 0, c = 0; b < n_batches; ++b) {
        const size_t e = traced_end(b), nb = e - s, ce = size_t(rows[row_words * b]);
        Workspace::rewind(batch_mark);
        if (nb) {
            ordered_rebase_kernel<<<ceil_div(nb, 256), 256, 0, stream>>>(offs + s, int(nb), off32);
            GRACE_CHECK_LAUNCH();
        }
        if (stats) GRACE_TRY(ev.mark(stream));
        if (h_table[1] != 0 && nb)
            GRACE_TRY(trace_hits_nested(rays + s * ray_bytes, nb, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves,
                                        d_root, off32, hit_idx, hit_integral, hit_dist, stream));
        if (stats) GRACE_TRY(ev.mark(stream));
        OrdBatch batch;
        batch.offs = offs; batch.ray0 = int(c);
        batch.hit_idx = hit_idx; batch.hit_integral = hit_integral; batch.hit_dist = hit_dist;
        batch.groups = grouped ? grouped->groups : nullptr;
        batch.source = grouped ? grouped->source : nullptr;
        batch.n_sources = grouped ? int(grouped->n_sources) : 0;
        batch.n_segments = grouped ? int(n_rays) : 0;
        batch.seg_t0 = grouped ? grouped->seg_t0 : nullptr;
        batch.status = status;
        GRACE_TRY(launch(batch, int(ce - c), any_block, any_global));
        if (stats) GRACE_TRY(ev.mark(stream));
        s = e; c = ce;
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
