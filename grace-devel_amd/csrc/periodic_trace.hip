// Periodic boxes for traces (an extension the reference lacks): the kernels that turn a periodic
// trace into an open one.  The periodic trace is DEFINED as the open trace of a stated set of ray
// segments over a stated set of sphere images (include/grace_hip.h, "Periodic boxes for traces");
// this file makes the two sets and folds the per-segment results back per ray.  The traversal, its
// caches and its kernels are not touched: the front ends call the open traces in between.  (The
// depth-ordered traces are no fold; their periodic form is in ordered_core.hpp.)
//
//   images    one thread per sphere: the crossing code (which faces the sphere sticks out of), then
//             2^popcount(code) copies, every subset of the crossing axes shifted by one period;
//   segments  one thread per ray: the ray cut where it crosses a face of the lattice of boxes, every
//             piece moved back into the box.  fp64 from the widened fp32 members, nothing fused;
//   starts    one thread per ray: every segment's starting parameter along its ray, from the same walk
//             (the periodic ordered traces' spectra need a hit's distance from the ray's origin);
//   fold      per ray and channel, the running sum of its segments' results in segment order;
//   gather    an image's weight row is its source's.
//
// Count, the caller's exclusive scan (scan.hip, grace_scan_exclusive_i32), then fill: the outputs
// are the caller's, sized from the scan's total.  The fills never write outside a row of the
// offsets they are given.  No loop here has a trip count above MAX_SEGMENTS whatever the inputs
// hold: the count per axis is a closed form corrected against the stated predicate, and a ray that
// would need more segments is emitted as itself and reported through the status word.
#include "common.hpp"
#include "trace_state.hpp"

#include <cmath>

#pragma clang fp contract(off)

using namespace grace_hip;

namespace {

constexpr int PT_BLOCK = 256;
constexpr int MAX_SEGMENTS = 65536;      // per ray
constexpr int RAY_FLOATS = 7;            // {dx, dy, dz, ox, oy, oz, length}: include/grace/ray.h:5-10

struct Box {
    float lo[3];
    float period[3];     // 0: the axis is open
};

// ---- images --------------------------------------------------------------------------------------

// The crossing code of a sphere: bit k set iff it sticks out of a face of periodic axis k; bit 3 set
// iff the sphere is refused (centre outside the box or H above half a period): emitted once.
__device__ __forceinline__ int crossing_code(const float4 s, const Box& b)
{
    if (!(isfinite(s.x) && isfinite(s.y) && isfinite(s.z) && isfinite(s.w))) return 0;
    const float x[3] = { s.x, s.y, s.z };
    int code = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float L = b.period[k];
        if (!(L > 0.0f)) continue;
        const float top = b.lo[k] + L;
        if (x[k] < b.lo[k] || x[k] > top || s.w > 0.5f * L) return 8;
        if (x[k] - s.w < b.lo[k] || x[k] + s.w > top) code |= 1 << k;
    }
    return code;
}

__global__ __launch_bounds__(PT_BLOCK) void image_counts_kernel(const float4* __restrict__ spheres, const int n,
                                                                const Box b, int* __restrict__ counts,
                                                                int* __restrict__ status)
{
    const int i = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int code = crossing_code(spheres[i], b);
    if (code & 8) atomicMax(status, int(GRACE_INVALID_ARGUMENT));
    counts[i] = (code & 8) ? 1 : 1 << __popc(code);
}

__global__ __launch_bounds__(PT_BLOCK) void images_kernel(const float4* __restrict__ spheres, const int n, const Box b,
                                                          const int* __restrict__ offsets,
                                                          float4* __restrict__ images, int* __restrict__ source,
                                                          int* __restrict__ status)
{
    const int i = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 s = spheres[i];
    int code = crossing_code(s, b);
    if (code & 8) { atomicMax(status, int(GRACE_INVALID_ARGUMENT)); code = 0; }
    const float x[3] = { s.x, s.y, s.z };
    float moved[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)      // (the lower face first, as the code's test)
        moved[k] = (code >> k & 1) ? (x[k] - s.w < b.lo[k] ? x[k] + b.period[k] : x[k] - b.period[k]) : x[k];
    int row = offsets[i];
    const int row_end = offsets[i + 1];
    if (row_end - row != 1 << __popc(code)) atomicMax(status, int(GRACE_INVALID_ARGUMENT));
#pragma unroll
    for (int subset = 0; subset < 8; ++subset) {
        if ((subset & ~code) != 0) continue;
        if (row >= 0 && row < row_end) {                       // never outside the row
            images[row] = make_float4(subset & 1 ? moved[0] : s.x, subset & 2 ? moved[1] : s.y,
                                      subset & 4 ? moved[2] : s.z, s.w);
            source[row] = i;
        }
        ++row;
    }
}

// ---- segments ------------------------------------------------------------------------------------

// What both segment kernels derive from a ray: its widened members, the starting cell, the cuts per
// axis and whether it is emitted as itself.
struct SegmentPlan {
    double d[3], o[3], len;
    double lo[3], L[3];
    double cell[3];
    int cuts[3];
    bool finite;        // no member is NaN or infinite
    bool refused;       // more than MAX_SEGMENTS segments
    int total;          // segments to emit
};

// t of the n-th cut (n = 1, 2, ...) of axis k: plane m = c + n for d > 0, m = c - (n - 1) for d < 0.
// Evaluated from m, never accumulated.
__device__ __forceinline__ double cut_t(const SegmentPlan& p, const int k, const int n)
{
    const double m = p.d[k] > 0.0 ? p.cell[k] + double(n) : p.cell[k] - double(n - 1);
    return (p.lo[k] + m * p.L[k] - p.o[k]) / p.d[k];
}

// The number of cuts of axis k, n with t(1..n) in (0, len) and t(n + 1) not: t(n) does not decrease
// with n, so the estimate n ~ (len - t(1)) |d| / L + 1 is corrected by at most two steps either way
// against the predicate itself.  Never more than MAX_SEGMENTS + 2.
__device__ __forceinline__ int axis_cuts(const SegmentPlan& p, const int k)
{
    if (!(p.L[k] > 0.0) || p.d[k] == 0.0) return 0;
    const double t1 = cut_t(p, k, 1);
    if (!(t1 > 0.0 && t1 < p.len)) return 0;
    double e = floor((p.len - t1) * fabs(p.d[k]) / p.L[k]) + 1.0;
    e = e >= 1.0 ? e : 1.0;                                   // (NaN: 1)
    int n = e < double(MAX_SEGMENTS) ? int(e) : MAX_SEGMENTS;
#pragma unroll
    for (int step = 0; step < 2; ++step)
        if (n > 1 && !(cut_t(p, k, n) < p.len)) --n;
#pragma unroll
    for (int step = 0; step < 2; ++step)
        if (cut_t(p, k, n + 1) < p.len) ++n;
    return n;
}

__device__ __forceinline__ SegmentPlan segment_plan(const float* __restrict__ ray, const Box& b)
{
    SegmentPlan p;
    p.finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p.d[k] = double(ray[k]);
        p.o[k] = double(ray[3 + k]);
        p.lo[k] = double(b.lo[k]);
        p.L[k] = double(b.period[k]);
        p.finite = p.finite && isfinite(ray[k]) && isfinite(ray[3 + k]);
    }
    p.len = double(ray[6]);
    p.finite = p.finite && isfinite(ray[6]);
    p.refused = false;
    p.total = 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) { p.cell[k] = 0.0; p.cuts[k] = 0; }
    if (!p.finite) return p;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!(p.L[k] > 0.0)) continue;
        const double u = (p.o[k] - p.lo[k]) / p.L[k];
        p.cell[k] = p.d[k] >= 0.0 ? floor(u) : ceil(u) - 1.0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p.cuts[k] = axis_cuts(p, k);
        p.total += p.cuts[k];
    }
    if (p.total > MAX_SEGMENTS) { p.refused = true; p.total = 1; }
    return p;
}

__global__ __launch_bounds__(PT_BLOCK) void segment_counts_kernel(const float* __restrict__ rays, const int n_rays,
                                                                  const Box b, int* __restrict__ counts,
                                                                  int* __restrict__ status)
{
    const int r = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (r >= n_rays) return;
    const SegmentPlan p = segment_plan(rays + size_t(r) * RAY_FLOATS, b);
    if (p.refused) atomicMax(status, int(GRACE_INVALID_ARGUMENT));
    counts[r] = p.total;
}

// A three-axis DDA over the cuts, ordered by (t, axis), of a ray that is not emitted as itself:
// emit(j, t, t_next, cell) for segment j = 0 .. n - 1, [t, t_next) in the running cell.  Both fills
// walk through here, so a segment and its starting parameter come from the same arithmetic.
template <typename Emit>
__device__ __forceinline__ void walk_segments(const SegmentPlan& p, const int n, Emit emit)
{
    const double inf = double(INFINITY);
    int used[3] = { 0, 0, 0 };
    double next[3], cell[3];                                   // the running cell; p.cell stays the starting one
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        next[k] = p.cuts[k] > 0 ? cut_t(p, k, 1) : inf;
        cell[k] = p.cell[k];
    }
    double t = 0.0;
    for (int j = 0; j < n; ++j) {
        int axis = -1;
        double t_next = p.len;
        if (j + 1 < p.total) {                                 // the smallest (t, axis) of the cuts left
            axis = 0;
            if (next[1] < next[axis]) axis = 1;
            if (next[2] < next[axis]) axis = 2;
            t_next = next[axis];
        }
        emit(j, t, t_next, cell);
        if (axis >= 0) {
            // (no dynamic indexing of the small arrays: they stay in registers)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k != axis) continue;
                cell[k] += p.d[k] > 0.0 ? 1.0 : -1.0;
                ++used[k];
                next[k] = used[k] < p.cuts[k] ? cut_t(p, k, used[k] + 1) : inf;
            }
            t = t_next;
        }
    }
}

// A ray emitted as itself, bit for bit: one with a non-finite member, a refused one, or one without
// cuts in cell 0.
__device__ __forceinline__ bool emitted_as_itself(const SegmentPlan& p)
{
    return !p.finite || p.refused || (p.total == 1 && p.cell[0] == 0.0 && p.cell[1] == 0.0 && p.cell[2] == 0.0);
}

// It stops at the row's end.
__global__ __launch_bounds__(PT_BLOCK) void segments_kernel(const float* __restrict__ rays, const int n_rays,
                                                            const Box b, const int* __restrict__ offsets,
                                                            float* __restrict__ segments, int* __restrict__ status)
{
    const int r = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (r >= n_rays) return;
    const float* ray = rays + size_t(r) * RAY_FLOATS;
    const SegmentPlan p = segment_plan(ray, b);
    const int row = offsets[r], row_end = offsets[r + 1];
    if (p.refused || row_end - row != p.total) atomicMax(status, int(GRACE_INVALID_ARGUMENT));
    if (row < 0 || row >= row_end) return;
    if (emitted_as_itself(p)) {
        float* out = segments + size_t(row) * RAY_FLOATS;
#pragma unroll
        for (int c = 0; c < RAY_FLOATS; ++c) out[c] = ray[c];
        return;
    }
    const int n = min(p.total, row_end - row);                 // never outside the row; <= MAX_SEGMENTS
    walk_segments(p, n, [&](const int j, const double t, const double t_next, const double (&cell)[3]) {
        float* out = segments + size_t(row + j) * RAY_FLOATS;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out[k] = ray[k];
            out[3 + k] = float(p.o[k] + t * p.d[k] - cell[k] * p.L[k]);
        }
        out[6] = float(t_next - t);
    });
}

// t0[s] of every segment: the t at which segments_kernel starts it; 0 for a ray emitted as itself.
__global__ __launch_bounds__(PT_BLOCK) void segment_starts_kernel(const float* __restrict__ rays, const int n_rays,
                                                                  const Box b, const int* __restrict__ offsets,
                                                                  double* __restrict__ t0, int* __restrict__ status)
{
    const int r = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (r >= n_rays) return;
    const SegmentPlan p = segment_plan(rays + size_t(r) * RAY_FLOATS, b);
    const int row = offsets[r], row_end = offsets[r + 1];
    if (p.refused || row_end - row != p.total) atomicMax(status, int(GRACE_INVALID_ARGUMENT));
    if (row < 0 || row >= row_end) return;
    if (emitted_as_itself(p)) { t0[row] = 0.0; return; }
    const int n = min(p.total, row_end - row);                 // never outside the row; <= MAX_SEGMENTS
    walk_segments(p, n, [&](const int j, const double t, const double, const double (&)[3]) { t0[row + j] = t; });
}

// ---- results -------------------------------------------------------------------------------------

// out[r, c] = the running sum, from 0, of values[s, c] over ray r's segments s in ascending order.
template <typename T>
__global__ __launch_bounds__(PT_BLOCK) void fold_kernel(const T* __restrict__ values, const int* __restrict__ offsets,
                                                        const size_t n_out, const int n_channels,
                                                        T* __restrict__ out)
{
    const size_t i = size_t(blockIdx.x) * PT_BLOCK + threadIdx.x;
    if (i >= n_out) return;
    const size_t r = i / size_t(n_channels);
    const int c = int(i - r * size_t(n_channels));
    const int begin = offsets[r];
    const int n = min(max(offsets[r + 1] - begin, 0), MAX_SEGMENTS);    // a ray never has more
    T sum = T(0);
    if (begin >= 0)
        for (int s = 0; s < n; ++s) sum = sum + values[size_t(begin + s) * n_channels + c];
    out[i] = sum;
}

__global__ __launch_bounds__(PT_BLOCK) void gather_rows_kernel(const float* __restrict__ rows,
                                                               const int* __restrict__ source, const size_t n_out,
                                                               const int n_channels, float* __restrict__ out)
{
    const size_t i = size_t(blockIdx.x) * PT_BLOCK + threadIdx.x;
    if (i >= n_out) return;
    const size_t j = i / size_t(n_channels);
    const int c = int(i - j * size_t(n_channels));
    const int src = source[j];
    out[i] = src >= 0 ? rows[size_t(src) * n_channels + c] : 0.0f;
}

// ---- host ----------------------------------------------------------------------------------------

// lo and period of a box from the caller's host arrays; a period of 0 leaves its axis open.
grace_status make_box(Box& b, const float* h_lo3, const float* h_period3)
{
    GRACE_REQUIRE(h_lo3 && h_period3, "periodic trace: null box origin or period");
    for (int k = 0; k < 3; ++k) {
        GRACE_REQUIRE(std::isfinite(h_period3[k]) && h_period3[k] >= 0.0f,
                      "periodic trace: a period must be finite and not negative (0 leaves the axis open)");
        GRACE_REQUIRE(std::isfinite(h_lo3[k]), "periodic trace: the box origin must be finite");
        b.lo[k] = h_lo3[k];
        b.period[k] = h_period3[k];
    }
    return GRACE_OK;
}

grace_status status_word(int** status, hipStream_t stream)
{
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    GRACE_TRY(ensure_status(*ts, stream));
    *status = ts->status;
    return GRACE_OK;
}

template <typename T>
grace_status fold(const T* d_values, const int* d_offsets, size_t n_rays, int n_channels, T* d_out,
                  grace_stream stream)
{
    GRACE_REQUIRE(n_channels >= 1 && n_channels <= 64, "periodic_fold: channels must be 1..64");
    GRACE_REQUIRE(n_rays < (size_t(1) << 31), "periodic_fold: too many rays");
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_values && d_offsets && d_out, "periodic_fold: null pointer");
    const size_t n_out = n_rays * size_t(n_channels);
    fold_kernel<T><<<ceil_div(n_out, PT_BLOCK), PT_BLOCK, 0, as_stream(stream)>>>(d_values, d_offsets, n_out,
                                                                                  n_channels, d_out);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

} // namespace

extern "C" {

grace_status grace_periodic_image_counts_f4(const float* d_spheres, size_t n, const float* h_lo3,
                                            const float* h_period3, int* d_counts, grace_stream stream)
{
    Box b;
    GRACE_TRY(make_box(b, h_lo3, h_period3));
    GRACE_REQUIRE(n < (size_t(1) << 31), "periodic_image_counts: more than INT32_MAX spheres");
    if (n == 0) return GRACE_OK;
    GRACE_REQUIRE(d_spheres && d_counts, "periodic_image_counts: null pointer");
    const hipStream_t st = as_stream(stream);
    int* status = nullptr;
    GRACE_TRY(status_word(&status, st));
    image_counts_kernel<<<ceil_div(n, PT_BLOCK), PT_BLOCK, 0, st>>>(reinterpret_cast<const float4*>(d_spheres),
                                                                    int(n), b, d_counts, status);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

grace_status grace_periodic_images_f4(const float* d_spheres, size_t n, const float* h_lo3,
                                      const float* h_period3, const int* d_offsets, float* d_images,
                                      int* d_source, grace_stream stream)
{
    Box b;
    GRACE_TRY(make_box(b, h_lo3, h_period3));
    GRACE_REQUIRE(n < (size_t(1) << 31), "periodic_images: more than INT32_MAX spheres");
    if (n == 0) return GRACE_OK;
    GRACE_REQUIRE(d_spheres && d_offsets && d_images && d_source, "periodic_images: null pointer");
    GRACE_TRY(scene_invalidate_if_written(d_images));
    const hipStream_t st = as_stream(stream);
    int* status = nullptr;
    GRACE_TRY(status_word(&status, st));
    images_kernel<<<ceil_div(n, PT_BLOCK), PT_BLOCK, 0, st>>>(reinterpret_cast<const float4*>(d_spheres), int(n), b,
                                                              d_offsets, reinterpret_cast<float4*>(d_images),
                                                              d_source, status);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

grace_status grace_periodic_segment_counts(const void* d_rays, size_t n_rays, const float* h_lo3,
                                           const float* h_period3, int* d_counts, grace_stream stream)
{
    Box b;
    GRACE_TRY(make_box(b, h_lo3, h_period3));
    GRACE_REQUIRE(n_rays < (size_t(1) << 31), "periodic_segment_counts: more than INT32_MAX rays");
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_rays && d_counts, "periodic_segment_counts: null pointer");
    const hipStream_t st = as_stream(stream);
    int* status = nullptr;
    GRACE_TRY(status_word(&status, st));
    segment_counts_kernel<<<ceil_div(n_rays, PT_BLOCK), PT_BLOCK, 0, st>>>(static_cast<const float*>(d_rays),
                                                                           int(n_rays), b, d_counts, status);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

grace_status grace_periodic_segments(const void* d_rays, size_t n_rays, const float* h_lo3,
                                     const float* h_period3, const int* d_offsets, void* d_segments,
                                     grace_stream stream)
{
    Box b;
    GRACE_TRY(make_box(b, h_lo3, h_period3));
    GRACE_REQUIRE(n_rays < (size_t(1) << 31), "periodic_segments: more than INT32_MAX rays");
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_rays && d_offsets && d_segments, "periodic_segments: null pointer");
    GRACE_TRY(rays_invalidate_if_written(d_segments));
    const hipStream_t st = as_stream(stream);
    int* status = nullptr;
    GRACE_TRY(status_word(&status, st));
    segments_kernel<<<ceil_div(n_rays, PT_BLOCK), PT_BLOCK, 0, st>>>(static_cast<const float*>(d_rays), int(n_rays), b,
                                                                     d_offsets, static_cast<float*>(d_segments),
                                                                     status);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

grace_status grace_periodic_segment_starts(const void* d_rays, size_t n_rays, const float* h_lo3,
                                           const float* h_period3, const int* d_offsets, double* d_t0,
                                           grace_stream stream)
{
    Box b;
    GRACE_TRY(make_box(b, h_lo3, h_period3));
    GRACE_REQUIRE(n_rays < (size_t(1) << 31), "periodic_segment_starts: more than INT32_MAX rays");
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_rays && d_offsets && d_t0, "periodic_segment_starts: null pointer");
    const hipStream_t st = as_stream(stream);
    int* status = nullptr;
    GRACE_TRY(status_word(&status, st));
    segment_starts_kernel<<<ceil_div(n_rays, PT_BLOCK), PT_BLOCK, 0, st>>>(static_cast<const float*>(d_rays),
                                                                           int(n_rays), b, d_offsets, d_t0, status);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

grace_status grace_periodic_fold_f32(const float* d_values, const int* d_offsets, size_t n_rays, int n_channels,
                                     float* d_out, grace_stream stream)
{
    return fold(d_values, d_offsets, n_rays, n_channels, d_out, stream);
}

grace_status grace_periodic_fold_i32(const int* d_values, const int* d_offsets, size_t n_rays, int n_channels,
                                     int* d_out, grace_stream stream)
{
    return fold(d_values, d_offsets, n_rays, n_channels, d_out, stream);
}

grace_status grace_periodic_gather_rows_f32(const float* d_rows, const int* d_source, size_t n_images,
                                            int n_channels, float* d_out, grace_stream stream)
{
    GRACE_REQUIRE(n_channels >= 1 && n_channels <= 64, "periodic_gather_rows: channels must be 1..64");
    GRACE_REQUIRE(n_images < (size_t(1) << 31), "periodic_gather_rows: more than INT32_MAX images");
    if (n_images == 0) return GRACE_OK;
    GRACE_REQUIRE(d_rows && d_source && d_out, "periodic_gather_rows: null pointer");
    const size_t n_out = n_images * size_t(n_channels);
    gather_rows_kernel<<<ceil_div(n_out, PT_BLOCK), PT_BLOCK, 0, as_stream(stream)>>>(d_rows, d_source, n_out,
                                                                                      n_channels, d_out);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

} // extern "C"
