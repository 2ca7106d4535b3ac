// Range queries of points among the sphere centres: every centre within the query point's own
// radius (grace_range_counts_f4: counts and gather sums, grace_range_neighbours_f4: CSR lists).  An
// extension the reference lacks; membership, order and the sums' arithmetic are stated exactly in
// include/grace_hip.h.
//
// Packets are the interpolation's (point_packets.hpp): one wave owns up to 64 points of one Morton
// cell, keys against the tree's root box, sorted.  The wave walks the ALBVH against the union of its
// lanes' query boxes [p - r', p + r'], r' the lane's radius widened (below).  The radii are known up
// front, so the union is computed once and there is nothing to keep per lane but a counter, the
// running sums or the row's write position; the row itself is never held in registers.
//
// The walk itself -- its order, stack, cluster sweep and the widening argument that makes pruning
// exact -- is range_walk.hpp's, shared with the friends-of-friends link kernel (fof.hip); this file
// holds what a lane does with a centre in range: one compare, then a count, an append or the kernel
// and one multiply-add pair per channel.  The survivors' <= 4 weights of a sums walk are staged in
// LDS beside their records.
//
// The periodic entry points run the same visitors over the walk's periodic variant: the kernels are
// instantiated a second time with Periodic<RangeArgs> arguments.
#include "range_walk.hpp"
#include "sph_kernel_f.hpp"

#include <cmath>

using namespace grace_hip;

namespace {

constexpr int RG_CHANNELS = 4;     // channels per walk

enum { RG_COUNT = 0, RG_SUMS = 1, RG_FILL = 2 };

struct RangeArgs : WalkArgs {
    const float* weights;        // this walk's first channel; sphere j's channel c at weights[j w_stride + c]
    int w_stride;
    float* sums;                 // point p's channel c at sums[p w_stride + c]
    int* counts;                 // or null
    const int* offsets;          // fill: row p is [offsets[p], offsets[p + 1])
    int* indices;                // or null
    float* d2;                   // or null
};

// What a lane does with a centre in range (range_walk.hpp's Visitor).  MODE: a count, a row entry or
// a term of the sums; KIND, NW: the SPH kernel and the channels of a RG_SUMS walk.  s_w: the
// weights of the wave's 64 survivor records.
template <int MODE, int KIND, int NW>
struct RangeVisitor {
    static constexpr int NS = NW > 0 ? NW : 1;
    const RangeArgs& a;
    float (*s_w)[NS];
    int found = 0;
    float acc[NS];
    float ih = 0.0f, ih3 = 0.0f;
    bool summing = false;                                   // r == 0: the sum is 0 (no 1 / r)
    int row = 0, row_end = 0;

    __device__ __forceinline__ RangeVisitor(const RangeArgs& args, float (*weights)[NS]) : a(args), s_w(weights) {}

    __device__ __forceinline__ void begin(const bool in_range, const bool on, const uint32_t src, const float r)
    {
#pragma unroll
        for (int c = 0; c < NS; ++c) acc[c] = 0.0f;
        if constexpr (MODE == RG_SUMS) {
            summing = on && r > 0.0f;
            ih = summing ? 1.0f / r : 0.0f;
            ih3 = (ih * ih) * ih;
        }
        if constexpr (MODE == RG_FILL) {
            if (in_range) { row = a.offsets[src]; row_end = a.offsets[src + 1]; }
        }
    }
    __device__ __forceinline__ bool clip(int&, int&) const { return true; }
    __device__ __forceinline__ void stage(const int pos, const int j)
    {
        if constexpr (MODE == RG_SUMS) {
#pragma unroll
            for (int c = 0; c < NW; ++c) s_w[pos][c] = a.weights[size_t(j) * a.w_stride + c];
        }
    }
    __device__ __forceinline__ void hit(const int pos, const float4& rec, const float d2)
    {
        if constexpr (MODE == RG_FILL) {
            const int o = row + found;
            if (o < row_end) {               // never outside the row
                if (a.indices) a.indices[o] = __float_as_int(rec.w);
                if (a.d2) a.d2[o] = d2;
            }
        }
        ++found;
        if constexpr (MODE == RG_SUMS) {
            if (summing) {
                const float W = kernel_f<KIND>(sqrt_rn(d2) * ih) * ih3;
#pragma unroll
                for (int c = 0; c < NW; ++c) acc[c] = acc[c] + s_w[pos][c] * W;
            }
        }
    }
    __device__ __forceinline__ void finish(const uint32_t src)
    {
        if constexpr (MODE == RG_FILL) {
            if (found != row_end - row) atomicMax(a.status, int(GRACE_INVALID_ARGUMENT));
        } else {
            if (a.counts) a.counts[src] = found;
        }
        if constexpr (MODE == RG_SUMS) {
#pragma unroll
            for (int c = 0; c < NW; ++c) a.sums[size_t(src) * a.w_stride + c] = acc[c];
        }
    }
};

template <int MODE, int KIND, int NW, typename Args>
__global__ __launch_bounds__(PW_BLOCK) void range_kernel(const Args a)
{
    __shared__ float4 s_rec[PW_WAVES][64];
    __shared__ float s_w[PW_WAVES][NW > 0 ? 64 : 1][NW > 0 ? NW : 1];
    const PacketWave w = packet_wave();
    if (w.packet < int(*a.n_starts)) {
        RangeVisitor<MODE, KIND, NW> v(a, s_w[w.wv]);
        walk(a, w.packet, w.lane, s_rec[w.wv], v);
    }
}

// One walk: mode RG_COUNT / RG_FILL, or RG_SUMS over nw channels with the built-in kernel `kind`.
template <typename Args>
grace_status launch_walk(const Args& a, int mode, int kind, int nw, size_t waves, hipStream_t stream)
{
    const int blocks = ceil_div(waves, PW_WAVES);
    if (mode == RG_COUNT) {
        range_kernel<RG_COUNT, GRACE_SPH_KERNEL_CUBIC, 0><<<blocks, PW_BLOCK, 0, stream>>>(a);
    } else if (mode == RG_FILL) {
        range_kernel<RG_FILL, GRACE_SPH_KERNEL_CUBIC, 0><<<blocks, PW_BLOCK, 0, stream>>>(a);
    } else {
        with_kernel(kind, nw, [&](auto k, auto n) {
            range_kernel<RG_SUMS, decltype(k)::value, decltype(n)::value><<<blocks, PW_BLOCK, 0, stream>>>(a);
        });
    }
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

// The checks both entry points share (before anything is enqueued), and the scene's fields.
grace_status range_common(RangeArgs& a, const float* d_points, size_t n_points,
                          const float* d_radii, float radius, const float* d_spheres, size_t n_spheres,
                          const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root)
{
    GRACE_REQUIRE(d_points, "range query: null points");
    GRACE_REQUIRE(d_radii || (std::isfinite(radius) && radius >= 0.0f),
                  "range query: the radius must be finite and not negative");
    return walk_scene(a, d_radii, radius, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root);
}

// grace_range_counts_f4 and its periodic form: `a` is zero but for a period.
template <typename Args>
grace_status range_counts(Args a, const float* d_points, size_t n_points, int elems_per_point,
                          const float* d_radii, float radius, const float* d_spheres, size_t n_spheres,
                          const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root,
                          const float* d_weights, int n_channels, int* d_counts, float* d_sums, grace_stream stream)
{
    GRACE_REQUIRE(elems_per_point >= 3 && elems_per_point <= 16, "range_counts: elements per point must be 3..16");
    GRACE_REQUIRE(n_points < (size_t(1) << 31), "range_counts: too many points");
    if (d_sums) {
        GRACE_REQUIRE(n_channels >= 1 && n_channels <= 64, "range_counts: channels must be 1..64");
        GRACE_REQUIRE(d_weights, "range_counts: sums need weights");
    }
    if (n_points == 0) return GRACE_OK;   // (before the output checks: a caller's empty arrays may be null)
    GRACE_REQUIRE(d_counts || d_sums, "range_counts: no output");
    GRACE_TRY(range_common(a, d_points, n_points, d_radii, radius, d_spheres, n_spheres, d_nodes,
                           n_nodes, d_leaves, d_root));
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    const int kind = ts->sph_kernel;
    if (d_sums)
        GRACE_REQUIRE(kind >= GRACE_SPH_KERNEL_CUBIC && kind <= GRACE_SPH_KERNEL_WENDLAND_C6,
                      "range_counts: a custom SPH kernel table has no kernel function f(q)");
    a.w_stride = n_channels;
    const hipStream_t stream_ = as_stream(stream);
    return packet_run(a, *ts, d_points, n_points, elems_per_point, stream_,
                      [&](Args w, size_t waves) -> grace_status {
        if (!d_sums) {
            w.counts = d_counts;
            return launch_walk(w, RG_COUNT, kind, 0, waves, stream_);
        }
        // channels four at a time, counts with the first walk
        for (int g = 0; g < n_channels; g += RG_CHANNELS) {
            w.weights = d_weights + g;
            w.sums = d_sums + g;
            w.counts = g == 0 ? d_counts : nullptr;
            GRACE_TRY(launch_walk(w, RG_SUMS, kind, min(RG_CHANNELS, n_channels - g), waves, stream_));
        }
        return GRACE_OK;
    });
}

// grace_range_neighbours_f4 and its periodic form.
template <typename Args>
grace_status range_neighbours(Args a, const float* d_points, size_t n_points, int elems_per_point,
                              const float* d_radii, float radius, const float* d_spheres, size_t n_spheres,
                              const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root,
                              const int* d_offsets, int* d_indices, float* d_d2, grace_stream stream)
{
    GRACE_REQUIRE(elems_per_point >= 3 && elems_per_point <= 16, "range_neighbours: elements per point must be 3..16");
    GRACE_REQUIRE(n_points < (size_t(1) << 31), "range_neighbours: too many points");
    if (n_points == 0) return GRACE_OK;   // (before the output checks: a caller's empty arrays may be null)
    GRACE_REQUIRE(d_offsets, "range_neighbours: null offsets");
    GRACE_REQUIRE(d_indices || d_d2, "range_neighbours: no output");
    GRACE_TRY(range_common(a, d_points, n_points, d_radii, radius, d_spheres, n_spheres,
                           d_nodes, n_nodes, d_leaves, d_root));
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    a.offsets = d_offsets;
    a.indices = d_indices;
    a.d2 = d_d2;
    const hipStream_t stream_ = as_stream(stream);
    return packet_run(a, *ts, d_points, n_points, elems_per_point, stream_,
                      [&](const Args& w, size_t waves) -> grace_status {
        return launch_walk(w, RG_FILL, GRACE_SPH_KERNEL_CUBIC, 0, waves, stream_);
    });
}

} // namespace

extern "C" {

grace_status grace_range_counts_f4(const float* d_points, size_t n_points, int elems_per_point,
                                   const float* d_radii, float radius,
                                   const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                   size_t n_nodes, const int* d_leaves, const int* d_root,
                                   const float* d_weights, int n_channels,
                                   int* d_counts, float* d_sums, grace_stream stream)
{
    return range_counts(RangeArgs(), d_points, n_points, elems_per_point, d_radii, radius, d_spheres, n_spheres,
                        d_nodes, n_nodes, d_leaves, d_root, d_weights, n_channels, d_counts, d_sums, stream);
}

grace_status grace_range_neighbours_f4(const float* d_points, size_t n_points, int elems_per_point,
                                       const float* d_radii, float radius,
                                       const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                       size_t n_nodes, const int* d_leaves, const int* d_root,
                                       const int* d_offsets, int* d_indices, float* d_d2,
                                       grace_stream stream)
{
    return range_neighbours(RangeArgs(), d_points, n_points, elems_per_point, d_radii, radius, d_spheres, n_spheres,
                            d_nodes, n_nodes, d_leaves, d_root, d_offsets, d_indices, d_d2, stream);
}

grace_status grace_range_counts_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                            const float* d_radii, float radius,
                                            const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                            size_t n_nodes, const int* d_leaves, const int* d_root,
                                            const float* d_weights, int n_channels,
                                            int* d_counts, float* d_sums, const float* h_period3,
                                            grace_stream stream)
{
    Periodic<RangeArgs> a = {};
    GRACE_TRY(walk_period(a.per, h_period3, d_radii ? nullptr : &radius));
    return range_counts(a, d_points, n_points, elems_per_point, d_radii, radius, d_spheres, n_spheres,
                        d_nodes, n_nodes, d_leaves, d_root, d_weights, n_channels, d_counts, d_sums, stream);
}

grace_status grace_range_neighbours_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                const float* d_radii, float radius,
                                                const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                size_t n_nodes, const int* d_leaves, const int* d_root,
                                                const int* d_offsets, int* d_indices, float* d_d2,
                                                const float* h_period3, grace_stream stream)
{
    Periodic<RangeArgs> a = {};
    GRACE_TRY(walk_period(a.per, h_period3, d_radii ? nullptr : &radius));
    return range_neighbours(a, d_points, n_points, elems_per_point, d_radii, radius, d_spheres, n_spheres,
                            d_nodes, n_nodes, d_leaves, d_root, d_offsets, d_indices, d_d2, stream);
}

} // extern "C"
