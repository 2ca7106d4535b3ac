// grace/detail/pairs_sph.h -- the one definition of the pair counts and radial profiles, an
// extension the reference lacks, shared by the drop-in grace/cuda/pairs_sph.cuh and the HIP-free
// mirror grace/grace.h (grace/detail/front_end.h): how many sphere centres lie in each shell of
// separation around each query point, as totals over all points (the DD(r) of a two-point
// correlation function), per-point histograms and per-point sums of weights per shell --
// grace_pair_counts_f4 (grace_hip.h states the fp32 distance, the bins d2 <= fl(e_k e_k), the
// ordered pairs of the totals and the sums' order).  Spheres in tree order; their w is ignored.
// edges are host floats, 1..64 of them, finite, not negative, strictly ascending.  d_weights holds
// n_channels (1..4, n_edges * n_channels <= 64) weights per sphere, sphere-major, in the order of
// d_spheres; d_counts[p * n_edges + k]; d_sums[(p * n_edges + k) * n_channels + c].  float4 spheres
// only; points are 3..16 floats, x y z first.  Size mismatches throw std::invalid_argument; a stack
// overflow is reported as by the traces.  Every function has an overload with a trailing
// grace::PeriodicBox (grace/detail/periodic_box.h): the separation wraps once per component and each
// pair is still counted once -- the DD(r) on the torus that an analytic RR goes with
// (grace_pair_counts_periodic_f4); a last edge above half a period is refused.  Not provided:
// double4 spheres, weighted totals, halving the work for auto-pairs, estimators (Landy-Szalay,
// xi(r)), per-point edge lists.
#pragma once

#include "grace/detail/periodic_box.h"
#include "grace/detail/trace_sph.h"

#include <stdexcept>
#include <vector>

namespace grace {

namespace detail {

// The one call of grace_pair_counts_f4 (box NULL) or grace_pair_counts_periodic_f4; any of totals /
// counts / sums may be NULL.
template <typename PointType, typename Real4>
inline void pair_counts_call(const dvec<PointType>& d_points, const std::vector<float>& edges,
                             const dvec<Real4>& d_spheres, const Tree& d_tree, const float* weights,
                             const int n_channels, unsigned long long* totals, int* counts, float* sums,
                             const PeriodicBox* box = NULL)
{
    static_assert(std::is_same<Real4, float4>::value, "pair counts: float4 spheres only (float edges, distances and sums)");
    static_assert(sizeof(PointType) % sizeof(float) == 0 && sizeof(PointType) >= 3 * sizeof(float)
                      && sizeof(PointType) <= 16 * sizeof(float),
                  "pair counts: points are 3..16 floats, x y z first");
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    if (box) {
        const float period[3] = { box->lx, box->ly, box->lz };
        GRACE_STATUS_CHECK(grace_pair_counts_periodic_f4(
            reinterpret_cast<const float*>(raw(d_points)), d_points.size(), int(sizeof(PointType) / sizeof(float)),
            edges.empty() ? NULL : &edges[0], int(edges.size()), GRACE_SCENE(a), weights, n_channels, totals, counts,
            sums, period, NULL));
    } else {
        GRACE_STATUS_CHECK(grace_pair_counts_f4(
            reinterpret_cast<const float*>(raw(d_points)), d_points.size(), int(sizeof(PointType) / sizeof(float)),
            edges.empty() ? NULL : &edges[0], int(edges.size()), GRACE_SCENE(a), weights, n_channels, totals, counts,
            sums, NULL));
    }
    check_trace_status();
}

} // namespace detail

// d_totals[k] = the number of (point, sphere) pairs whose d2 falls in bin k, over all points; resized
// to the number of edges.  Ordered pairs: with the sphere centres as points, every unordered pair
// twice and every self pair once (bin 0).
template <typename PointType, typename Real4>
GRACE_HOST void pair_counts_sph(const detail::dvec<PointType>& d_points, const std::vector<float>& edges,
                                const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                detail::dvec<unsigned long long>& d_totals)
{
    d_totals.resize(edges.size());
    detail::pair_counts_call(d_points, edges, d_spheres, d_tree, (const float*)NULL, 0, detail::raw(d_totals),
                             (int*)NULL, (float*)NULL);
}

// d_counts[p * n_edges + k] = the number of sphere centres in bin k of d_points[p]; resized.
template <typename PointType, typename Real4>
GRACE_HOST void radial_profiles_sph(const detail::dvec<PointType>& d_points, const std::vector<float>& edges,
                                    const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                    detail::dvec<int>& d_counts)
{
    d_counts.resize(d_points.size() * edges.size());
    detail::pair_counts_call(d_points, edges, d_spheres, d_tree, (const float*)NULL, 0, (unsigned long long*)NULL,
                             detail::raw(d_counts), (float*)NULL);
}

// ... and d_sums[(p * n_edges + k) * n_channels + c] = the sum of d_weights[j * n_channels + c] over
// the spheres j in bin k of point p, ascending j, a plain fp32 running sum; resized.
template <typename PointType, typename Real4>
GRACE_HOST void radial_profiles_sph(const detail::dvec<PointType>& d_points, const std::vector<float>& edges,
                                    const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                    detail::dvec<int>& d_counts, const detail::dvec<float>& d_weights,
                                    const int n_channels, detail::dvec<float>& d_sums)
{
    if (n_channels < 1 || n_channels > 4 || edges.size() * size_t(n_channels) > 64)
        throw std::invalid_argument("radial_profiles_sph: n_channels must be 1..4 and n_edges * n_channels <= 64");
    if (d_weights.size() != d_spheres.size() * size_t(n_channels))
        throw std::invalid_argument("radial_profiles_sph: d_weights must hold n_channels per sphere");
    d_counts.resize(d_points.size() * edges.size());
    d_sums.resize(d_points.size() * edges.size() * size_t(n_channels));
    detail::pair_counts_call(d_points, edges, d_spheres, d_tree, detail::raw(d_weights), n_channels,
                             (unsigned long long*)NULL, detail::raw(d_counts), detail::raw(d_sums));
}

// ---- the same in a periodic box: the separation wraps once per component ----
template <typename PointType, typename Real4>
GRACE_HOST void pair_counts_sph(const detail::dvec<PointType>& d_points, const std::vector<float>& edges,
                                const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                detail::dvec<unsigned long long>& d_totals, const PeriodicBox& box)
{
    d_totals.resize(edges.size());
    detail::pair_counts_call(d_points, edges, d_spheres, d_tree, (const float*)NULL, 0, detail::raw(d_totals),
                             (int*)NULL, (float*)NULL, &box);
}

template <typename PointType, typename Real4>
GRACE_HOST void radial_profiles_sph(const detail::dvec<PointType>& d_points, const std::vector<float>& edges,
                                    const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                    detail::dvec<int>& d_counts, const PeriodicBox& box)
{
    d_counts.resize(d_points.size() * edges.size());
    detail::pair_counts_call(d_points, edges, d_spheres, d_tree, (const float*)NULL, 0, (unsigned long long*)NULL,
                             detail::raw(d_counts), (float*)NULL, &box);
}

template <typename PointType, typename Real4>
GRACE_HOST void radial_profiles_sph(const detail::dvec<PointType>& d_points, const std::vector<float>& edges,
                                    const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                    detail::dvec<int>& d_counts, const detail::dvec<float>& d_weights,
                                    const int n_channels, detail::dvec<float>& d_sums, const PeriodicBox& box)
{
    if (n_channels < 1 || n_channels > 4 || edges.size() * size_t(n_channels) > 64)
        throw std::invalid_argument("radial_profiles_sph: n_channels must be 1..4 and n_edges * n_channels <= 64");
    if (d_weights.size() != d_spheres.size() * size_t(n_channels))
        throw std::invalid_argument("radial_profiles_sph: d_weights must hold n_channels per sphere");
    d_counts.resize(d_points.size() * edges.size());
    d_sums.resize(d_points.size() * edges.size() * size_t(n_channels));
    detail::pair_counts_call(d_points, edges, d_spheres, d_tree, detail::raw(d_weights), n_channels,
                             (unsigned long long*)NULL, detail::raw(d_counts), detail::raw(d_sums), &box);
}

} // namespace grace
