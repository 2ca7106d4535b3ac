// grace/detail/range_sph.h -- the one definition of the range queries, an extension the reference
// lacks, shared by the drop-in grace/cuda/range_sph.cuh and the HIP-free mirror grace/grace.h
// (grace/detail/front_end.h): every sphere centre within the query point's own radius, as counts,
// gather sums of the SPH kernel and CSR neighbour lists -- grace_range_counts_f4 /
// grace_range_neighbours_f4 (grace_hip.h states the fp32 distance, the inclusive test d2 <= fl(r r),
// the ascending order and the sums' arithmetic).  Spheres in tree order; their w is ignored.
// d_weights holds n_channels weights per sphere, sphere-major, in the order of d_spheres;
// d_sums[p * n_channels + c].  float4 spheres only; points are 3..16 floats, x y z first; radii are
// one float per point, or one float for all.  Size mismatches throw std::invalid_argument; a stack
// overflow is reported as by the traces.  Every function has an overload with a trailing
// grace::PeriodicBox (grace/detail/periodic_box.h): the separation wraps once per component, a point
// whose radius exceeds half a period is off, one radius for all that does is refused
// (grace_range_counts_periodic_f4 / grace_range_neighbours_periodic_f4).  Not provided: symmetric
// max(h_p, H_j) criteria, double4 spheres, 64-bit offsets.
#pragma once

#include "grace/detail/periodic_box.h"
#include "grace/detail/trace_sph.h"

#include <limits>
#include <stdexcept>

namespace grace {

namespace detail {

template <typename PointType, typename Real4>
inline int range_point_elems()
{
    static_assert(std::is_same<Real4, float4>::value, "range queries: float4 spheres only (float radii, distances and sums)");
    static_assert(sizeof(PointType) % sizeof(float) == 0 && sizeof(PointType) >= 3 * sizeof(float)
                      && sizeof(PointType) <= 16 * sizeof(float),
                  "range queries: points are 3..16 floats, x y z first");
    return int(sizeof(PointType) / sizeof(float));
}

// The one call of grace_range_counts_f4 (box NULL) or grace_range_counts_periodic_f4.  d_radii
// NULL: `radius` for every point; weights / sums NULL: counts only.
template <typename PointType, typename Real4>
inline void range_counts_call(const dvec<PointType>& d_points, const dvec<float>* d_radii, const float radius,
                              const dvec<Real4>& d_spheres, const Tree& d_tree, const float* weights,
                              const int n_channels, int* counts, float* sums, const PeriodicBox* box = NULL)
{
    const int elems = range_point_elems<PointType, Real4>();
    if (d_radii && d_radii->size() != d_points.size())
        throw std::invalid_argument("range queries: d_radii must hold one radius per point");
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    if (box) {
        const float period[3] = { box->lx, box->ly, box->lz };
        GRACE_STATUS_CHECK(grace_range_counts_periodic_f4(
            reinterpret_cast<const float*>(raw(d_points)), d_points.size(), elems, d_radii ? raw(*d_radii) : NULL,
            radius, GRACE_SCENE(a), weights, n_channels, counts, sums, period, NULL));
    } else {
        GRACE_STATUS_CHECK(grace_range_counts_f4(
            reinterpret_cast<const float*>(raw(d_points)), d_points.size(), elems, d_radii ? raw(*d_radii) : NULL,
            radius, GRACE_SCENE(a), weights, n_channels, counts, sums, NULL));
    }
    check_trace_status();
}

// What every range_counts_sph overload does.
template <typename PointType, typename Real4>
inline void range_counts(const dvec<PointType>& d_points, const dvec<float>* d_radii, const float radius,
                         const dvec<Real4>& d_spheres, const Tree& d_tree, const dvec<float>* d_weights,
                         const int n_channels, dvec<int>& d_counts, dvec<float>* d_sums,
                         const PeriodicBox* box = NULL)
{
    if (d_counts.size() != d_points.size())
        throw std::invalid_argument("range_counts_sph: d_counts must hold one count per point");
    if (d_sums) {
        if (n_channels < 1 || n_channels > 64)
            throw std::invalid_argument("range_counts_sph: n_channels must be 1..64");
        if (d_weights->size() != d_spheres.size() * size_t(n_channels))
            throw std::invalid_argument("range_counts_sph: d_weights must hold n_channels per sphere");
        if (d_sums->size() != d_points.size() * size_t(n_channels))
            throw std::invalid_argument("range_counts_sph: d_sums must hold n_channels per point");
    }
    range_counts_call(d_points, d_radii, radius, d_spheres, d_tree, d_sums ? raw(*d_weights) : NULL, n_channels,
                      raw(d_counts), d_sums ? raw(*d_sums) : NULL, box);
}

// What both range_neighbours_sph overloads do.
template <typename PointType, typename Real4>
inline void range_neighbours(const dvec<PointType>& d_points, const dvec<float>* d_radii, const float radius,
                             const dvec<Real4>& d_spheres, const Tree& d_tree, dvec<int>& d_offsets,
                             dvec<int>& d_indices, dvec<float>& d_d2, const PeriodicBox* box = NULL)
{
    const int elems = range_point_elems<PointType, Real4>();
    const size_t n = d_points.size();
    // counts into the first n of n + 1 entries, the last one 0: their exclusive scan ends in the total
    d_offsets.assign(n + 1, 0);
    range_counts_call(d_points, d_radii, radius, d_spheres, d_tree, (const float*)NULL, 0, raw(d_offsets),
                      (float*)NULL, box);
    long long total = 0;
    GRACE_STATUS_CHECK(grace_scan_exclusive_i32(raw(d_offsets), n + 1, raw(d_offsets), &total, NULL));
    if (total > (long long)std::numeric_limits<int>::max())
        throw std::length_error("range_neighbours_sph: more than INT32_MAX list entries; the int offsets cannot "
                                "address them. Split the points into several calls.");
    d_indices.resize(size_t(total));
    d_d2.resize(size_t(total));
    if (total == 0) return;   // every row is empty
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    if (box) {
        const float period[3] = { box->lx, box->ly, box->lz };
        GRACE_STATUS_CHECK(grace_range_neighbours_periodic_f4(
            reinterpret_cast<const float*>(raw(d_points)), n, elems, d_radii ? raw(*d_radii) : NULL, radius,
            GRACE_SCENE(a), raw(d_offsets), raw(d_indices), raw(d_d2), period, NULL));
    } else {
        GRACE_STATUS_CHECK(grace_range_neighbours_f4(
            reinterpret_cast<const float*>(raw(d_points)), n, elems, d_radii ? raw(*d_radii) : NULL, radius,
            GRACE_SCENE(a), raw(d_offsets), raw(d_indices), raw(d_d2), NULL));
    }
    check_trace_status();
}

} // namespace detail

// d_counts[p] = the number of sphere centres within d_radii[p] of d_points[p] (d2 <= fl(r r)).
template <typename PointType, typename Real4>
GRACE_HOST void range_counts_sph(const detail::dvec<PointType>& d_points, const detail::dvec<float>& d_radii,
                                 const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                 detail::dvec<int>& d_counts)
{
    detail::range_counts(d_points, &d_radii, 0.0f, d_spheres, d_tree, (const detail::dvec<float>*)NULL, 0, d_counts,
                         (detail::dvec<float>*)NULL);
}

// ... within one radius for every point.
template <typename PointType, typename Real4>
GRACE_HOST void range_counts_sph(const detail::dvec<PointType>& d_points, const float radius,
                                 const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                 detail::dvec<int>& d_counts)
{
    detail::range_counts(d_points, (const detail::dvec<float>*)NULL, radius, d_spheres, d_tree,
                         (const detail::dvec<float>*)NULL, 0, d_counts, (detail::dvec<float>*)NULL);
}

// ... and the gather sums d_sums[p * n_channels + c] = sum over in-range j, ascending, of
// fl(d_weights[j * n_channels + c] W(|x_p - x_j|, r_p)) with the context's SPH kernel.
template <typename PointType, typename Real4>
GRACE_HOST void range_counts_sph(const detail::dvec<PointType>& d_points, const detail::dvec<float>& d_radii,
                                 const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                 const detail::dvec<float>& d_weights, const int n_channels,
                                 detail::dvec<int>& d_counts, detail::dvec<float>& d_sums)
{
    detail::range_counts(d_points, &d_radii, 0.0f, d_spheres, d_tree, &d_weights, n_channels, d_counts, &d_sums);
}

template <typename PointType, typename Real4>
GRACE_HOST void range_counts_sph(const detail::dvec<PointType>& d_points, const float radius,
                                 const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                 const detail::dvec<float>& d_weights, const int n_channels,
                                 detail::dvec<int>& d_counts, detail::dvec<float>& d_sums)
{
    detail::range_counts(d_points, (const detail::dvec<float>*)NULL, radius, d_spheres, d_tree, &d_weights,
                         n_channels, d_counts, &d_sums);
}

// The lists in CSR form: row p is [d_offsets[p], d_offsets[p + 1]) of d_indices (tree indices,
// ascending) and d_d2.  Counts, the library's scan, then the fill; the three outputs are resized
// (d_offsets to n + 1).  std::length_error for more than INT32_MAX list entries: split the points.
template <typename PointType, typename Real4>
GRACE_HOST void range_neighbours_sph(const detail::dvec<PointType>& d_points, const detail::dvec<float>& d_radii,
                                     const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                     detail::dvec<int>& d_offsets, detail::dvec<int>& d_indices,
                                     detail::dvec<float>& d_d2)
{
    detail::range_neighbours(d_points, &d_radii, 0.0f, d_spheres, d_tree, d_offsets, d_indices, d_d2);
}

template <typename PointType, typename Real4>
GRACE_HOST void range_neighbours_sph(const detail::dvec<PointType>& d_points, const float radius,
                                     const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                     detail::dvec<int>& d_offsets, detail::dvec<int>& d_indices,
                                     detail::dvec<float>& d_d2)
{
    detail::range_neighbours(d_points, (const detail::dvec<float>*)NULL, radius, d_spheres, d_tree, d_offsets,
                             d_indices, d_d2);
}

// ---- the same in a periodic box: the separation wraps once per component ----
template <typename PointType, typename Real4>
GRACE_HOST void range_counts_sph(const detail::dvec<PointType>& d_points, const detail::dvec<float>& d_radii,
                                 const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                 detail::dvec<int>& d_counts, const PeriodicBox& box)
{
    detail::range_counts(d_points, &d_radii, 0.0f, d_spheres, d_tree, (const detail::dvec<float>*)NULL, 0, d_counts,
                         (detail::dvec<float>*)NULL, &box);
}

template <typename PointType, typename Real4>
GRACE_HOST void range_counts_sph(const detail::dvec<PointType>& d_points, const float radius,
                                 const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                 detail::dvec<int>& d_counts, const PeriodicBox& box)
{
    detail::range_counts(d_points, (const detail::dvec<float>*)NULL, radius, d_spheres, d_tree,
                         (const detail::dvec<float>*)NULL, 0, d_counts, (detail::dvec<float>*)NULL, &box);
}

template <typename PointType, typename Real4>
GRACE_HOST void range_counts_sph(const detail::dvec<PointType>& d_points, const detail::dvec<float>& d_radii,
                                 const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                 const detail::dvec<float>& d_weights, const int n_channels,
                                 detail::dvec<int>& d_counts, detail::dvec<float>& d_sums, const PeriodicBox& box)
{
    detail::range_counts(d_points, &d_radii, 0.0f, d_spheres, d_tree, &d_weights, n_channels, d_counts, &d_sums,
                         &box);
}

template <typename PointType, typename Real4>
GRACE_HOST void range_counts_sph(const detail::dvec<PointType>& d_points, const float radius,
                                 const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                 const detail::dvec<float>& d_weights, const int n_channels,
                                 detail::dvec<int>& d_counts, detail::dvec<float>& d_sums, const PeriodicBox& box)
{
    detail::range_counts(d_points, (const detail::dvec<float>*)NULL, radius, d_spheres, d_tree, &d_weights,
                         n_channels, d_counts, &d_sums, &box);
}

template <typename PointType, typename Real4>
GRACE_HOST void range_neighbours_sph(const detail::dvec<PointType>& d_points, const detail::dvec<float>& d_radii,
                                     const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                     detail::dvec<int>& d_offsets, detail::dvec<int>& d_indices,
                                     detail::dvec<float>& d_d2, const PeriodicBox& box)
{
    detail::range_neighbours(d_points, &d_radii, 0.0f, d_spheres, d_tree, d_offsets, d_indices, d_d2, &box);
}

template <typename PointType, typename Real4>
GRACE_HOST void range_neighbours_sph(const detail::dvec<PointType>& d_points, const float radius,
                                     const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                     detail::dvec<int>& d_offsets, detail::dvec<int>& d_indices,
                                     detail::dvec<float>& d_d2, const PeriodicBox& box)
{
    detail::range_neighbours(d_points, (const detail::dvec<float>*)NULL, radius, d_spheres, d_tree, d_offsets,
                             d_indices, d_d2, &box);
}

} // namespace grace
