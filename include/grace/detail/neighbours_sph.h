// grace/detail/neighbours_sph.h -- the one definition of k nearest neighbours and smoothing lengths,
// an extension the reference lacks, shared by the drop-in grace/cuda/neighbours_sph.cuh and the
// HIP-free mirror grace/grace.h (grace/detail/front_end.h): grace_nearest_neighbours_f4 /
// grace_smoothing_lengths_f4 (grace_hip.h states the fp32 distance and the exact (d2, index)
// ranking).  Spheres in tree order; their w is ignored.  float4 spheres only.  Size mismatches throw
// std::invalid_argument; a stack overflow is reported as by the traces.  Both functions have an
// overload with a trailing grace::PeriodicBox (grace/detail/periodic_box.h): the separation wraps
// once per component and the ranking uses the wrapped d2, without a radius limit
// (grace_nearest_neighbours_periodic_f4 / grace_smoothing_lengths_periodic_f4).
#pragma once

#include "grace/detail/periodic_box.h"
#include "grace/detail/trace_sph.h"

namespace grace {

namespace detail {

// What both nearest_neighbours_sph overloads do: grace_nearest_neighbours_f4 (box NULL) or its periodic form.
template <typename PointType, typename Real4>
inline void nearest_neighbours(const dvec<PointType>& d_points, const dvec<Real4>& d_spheres, const Tree& d_tree,
                               const int k, dvec<int>& d_indices, dvec<float>& d_d2, const PeriodicBox* box)
{
    static_assert(std::is_same<Real4, float4>::value, "nearest_neighbours_sph: float4 spheres only");
    static_assert(sizeof(PointType) % sizeof(float) == 0 && sizeof(PointType) >= 3 * sizeof(float)
                      && sizeof(PointType) <= 16 * sizeof(float),
                  "nearest_neighbours_sph: points are 3..16 floats, x y z first");
    if (k < 1 || k > 64)
        throw std::invalid_argument("nearest_neighbours_sph: k must be 1..64");
    if (d_indices.size() != d_points.size() * size_t(k) || d_d2.size() != d_points.size() * size_t(k))
        throw std::invalid_argument("nearest_neighbours_sph: d_indices and d_d2 must hold k entries per point");
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    const float* points = reinterpret_cast<const float*>(raw(d_points));
    const int elems = int(sizeof(PointType) / sizeof(float));
    if (box) {
        const float period[3] = { box->lx, box->ly, box->lz };
        GRACE_STATUS_CHECK(grace_nearest_neighbours_periodic_f4(points, d_points.size(), elems, GRACE_SCENE(a), k,
                                                                raw(d_indices), raw(d_d2), period, NULL));
    } else {
        GRACE_STATUS_CHECK(grace_nearest_neighbours_f4(points, d_points.size(), elems, GRACE_SCENE(a), k,
                                                       raw(d_indices), raw(d_d2), NULL));
    }
    check_trace_status();
}

// What both smoothing_lengths_sph overloads do.
template <typename Real4>
inline void smoothing_lengths(const dvec<Real4>& d_spheres, const Tree& d_tree, const int k, const float eta,
                              dvec<float>& d_h, const PeriodicBox* box)
{
    static_assert(std::is_same<Real4, float4>::value, "smoothing_lengths_sph: float4 spheres only");
    if (d_h.size() != d_spheres.size())
        throw std::invalid_argument("smoothing_lengths_sph: d_h must hold one value per sphere");
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    if (box) {
        const float period[3] = { box->lx, box->ly, box->lz };
        GRACE_STATUS_CHECK(grace_smoothing_lengths_periodic_f4(GRACE_SCENE(a), k, eta, raw(d_h), period, NULL));
    } else {
        GRACE_STATUS_CHECK(grace_smoothing_lengths_f4(GRACE_SCENE(a), k, eta, raw(d_h), NULL));
    }
    check_trace_status();
}

} // namespace detail

// d_indices[p * k + s] / d_d2[p * k + s]: the s-th nearest sphere centre of d_points[p] and its d2
// (-1 / +inf past the number of spheres or for a non-finite point).  Points are 3..16 floats.
template <typename PointType, typename Real4>
GRACE_HOST void nearest_neighbours_sph(const detail::dvec<PointType>& d_points,
                                       const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                       const int k, detail::dvec<int>& d_indices,
                                       detail::dvec<float>& d_d2)
{
    detail::nearest_neighbours(d_points, d_spheres, d_tree, k, d_indices, d_d2, (const PeriodicBox*)NULL);
}

// d_h[i] = fl(eta * sqrt(d2 of the k-th nearest centre of sphere i's own centre)), tree order.
template <typename Real4>
GRACE_HOST void smoothing_lengths_sph(const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                      const int k, const float eta, detail::dvec<float>& d_h)
{
    detail::smoothing_lengths(d_spheres, d_tree, k, eta, d_h, (const PeriodicBox*)NULL);
}

// ---- the same in a periodic box: the separation wraps once per component ----
template <typename PointType, typename Real4>
GRACE_HOST void nearest_neighbours_sph(const detail::dvec<PointType>& d_points,
                                       const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                       const int k, detail::dvec<int>& d_indices,
                                       detail::dvec<float>& d_d2, const PeriodicBox& box)
{
    detail::nearest_neighbours(d_points, d_spheres, d_tree, k, d_indices, d_d2, &box);
}

template <typename Real4>
GRACE_HOST void smoothing_lengths_sph(const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                      const int k, const float eta, detail::dvec<float>& d_h,
                                      const PeriodicBox& box)
{
    detail::smoothing_lengths(d_spheres, d_tree, k, eta, d_h, &box);
}

} // namespace grace
