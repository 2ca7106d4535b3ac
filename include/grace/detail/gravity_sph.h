// grace/detail/gravity_sph.h -- the one definition of the tree gravity, an extension the reference
// lacks, shared by the drop-in grace/cuda/gravity_sph.cuh and the HIP-free mirror grace/grace.h
// (grace/detail/front_end.h): potentials and accelerations at points from the BVH, the Barnes-Hut
// walk with monopoles of the inner nodes, G = 1 -- grace_gravity_moments_f4 and
// grace_gravity_points_f4 (grace_hip.h states the moments, the acceptance test
// size2 < fl(theta^2 d2min), the fp32 pair term and the order of the fp64 sums).  Spheres and
// d_masses in tree order; the spheres' w is ignored.  gravity_moments_sph once per tree and set of
// masses, then any number of gravity_sph calls.  d_moments holds 12 floats per inner node;
// d_out[p * 4 + ..] = {a_x, a_y, a_z, phi}; d_counts[p * 2 + ..] = {node terms, particle terms}.
// theta = 0 is the direct sum in ascending tree index; eps is a Plummer softening length, 0 is
// Newtonian.  float4 spheres only; points are 3..16 floats, x y z first.  Size mismatches throw
// std::invalid_argument; a stack overflow is reported as by the traces.  Not provided: periodic
// boxes (they need Ewald sums), quadrupoles, spline or per-particle softening, leaf monopoles,
// double4 spheres, G.
#pragma once

#include "grace/detail/trace_sph.h"

#include <stdexcept>

namespace grace {

namespace detail {

// The one call of grace_gravity_points_f4; out or counts may be NULL.
template <typename PointType, typename Real4>
inline void gravity_call(const dvec<PointType>& d_points, const dvec<Real4>& d_spheres, const dvec<float>& d_masses,
                         const Tree& d_tree, const dvec<float>& d_moments, const float theta, const float eps,
                         double* out, int* counts)
{
    static_assert(std::is_same<Real4, float4>::value, "gravity: float4 spheres only (float distances, double sums)");
    static_assert(sizeof(PointType) % sizeof(float) == 0 && sizeof(PointType) >= 3 * sizeof(float)
                      && sizeof(PointType) <= 16 * sizeof(float),
                  "gravity: points are 3..16 floats, x y z first");
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    if (d_masses.size() != d_spheres.size())
        throw std::invalid_argument("gravity_sph: d_masses must hold one mass per sphere");
    if (d_moments.size() != a.n_nodes * 12)
        throw std::invalid_argument("gravity_sph: d_moments must hold 12 floats per node (gravity_moments_sph)");
    GRACE_STATUS_CHECK(grace_gravity_points_f4(
        reinterpret_cast<const float*>(raw(d_points)), d_points.size(), int(sizeof(PointType) / sizeof(float)),
        GRACE_SCENE(a), raw(d_masses), a.n_nodes ? raw(d_moments) : NULL, theta, eps, out, counts, NULL));
    check_trace_status();
}

} // namespace detail

// d_moments[i * 12 + ..] = node i's {c_x, c_y, c_z, M32}, {lo_x, lo_y, lo_z, bits(span_lo)},
// {hi_x, hi_y, hi_z, bits(span_hi)}; resized to 12 floats per inner node.
template <typename Real4>
GRACE_HOST void gravity_moments_sph(const detail::dvec<Real4>& d_spheres, const detail::dvec<float>& d_masses,
                                    const Tree& d_tree, detail::dvec<float>& d_moments)
{
    static_assert(std::is_same<Real4, float4>::value, "gravity: float4 spheres only (float distances, double sums)");
    const detail::SceneArgs<Real4> a = detail::scene_args(d_spheres, d_tree);
    if (d_masses.size() != d_spheres.size())
        throw std::invalid_argument("gravity_moments_sph: d_masses must hold one mass per sphere");
    d_moments.resize(a.n_nodes * 12);
    GRACE_STATUS_CHECK(grace_gravity_moments_f4(GRACE_SCENE(a), detail::raw(d_masses),
                                                a.n_nodes ? detail::raw(d_moments) : NULL, NULL));
}

// d_out[p * 4 + ..] = {a_x, a_y, a_z, phi} at d_points[p]; resized.
template <typename PointType, typename Real4>
GRACE_HOST void gravity_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                            const detail::dvec<float>& d_masses, const Tree& d_tree,
                            const detail::dvec<float>& d_moments, const float theta, const float eps,
                            detail::dvec<double>& d_out)
{
    d_out.resize(d_points.size() * 4);
    detail::gravity_call(d_points, d_spheres, d_masses, d_tree, d_moments, theta, eps, detail::raw(d_out), (int*)NULL);
}

// ... and d_counts[p * 2 + ..] = {node terms, particle terms} of the point's walk; resized.
template <typename PointType, typename Real4>
GRACE_HOST void gravity_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                            const detail::dvec<float>& d_masses, const Tree& d_tree,
                            const detail::dvec<float>& d_moments, const float theta, const float eps,
                            detail::dvec<double>& d_out, detail::dvec<int>& d_counts)
{
    d_out.resize(d_points.size() * 4);
    d_counts.resize(d_points.size() * 2);
    detail::gravity_call(d_points, d_spheres, d_masses, d_tree, d_moments, theta, eps, detail::raw(d_out),
                         detail::raw(d_counts));
}

// ---- Gravity within groups (grace_gravity_group_moments_f4, grace_gravity_group_points_f4): every
// point feels the particles that carry its own label.  d_labels: one int per sphere in tree order
// (fof_labels_sph's labels, fof_groups_sph's group_of), < 0: in no group, attracts nobody;
// d_point_labels: one int per point.  gravity_group_moments_sph once per tree, masses and labels,
// then any number of gravity_groups_sph calls; an unbinding pass sets labels to -1 and calls both
// again.  Not provided: a theta or eps per group, particles in more than one group, the unbinding
// loop itself, periodic boxes, and everything gravity_sph leaves out.

namespace detail {

// The one call of grace_gravity_group_points_f4; out or counts may be NULL.
template <typename PointType, typename Real4>
inline void gravity_groups_call(const dvec<PointType>& d_points, const dvec<int>& d_point_labels,
                                const dvec<Real4>& d_spheres, const dvec<float>& d_masses, const dvec<int>& d_labels,
                                const Tree& d_tree, const dvec<float>& d_moments, const dvec<int>& d_label_ranges,
                                const float theta, const float eps, double* out, int* counts)
{
    static_assert(std::is_same<Real4, float4>::value, "gravity: float4 spheres only (float distances, double sums)");
    static_assert(sizeof(PointType) % sizeof(float) == 0 && sizeof(PointType) >= 3 * sizeof(float)
                      && sizeof(PointType) <= 16 * sizeof(float),
                  "gravity: points are 3..16 floats, x y z first");
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    if (d_masses.size() != d_spheres.size())
        throw std::invalid_argument("gravity_groups_sph: d_masses must hold one mass per sphere");
    if (d_labels.size() != d_spheres.size())
        throw std::invalid_argument("gravity_groups_sph: d_labels must hold one label per sphere");
    if (d_point_labels.size() != d_points.size())
        throw std::invalid_argument("gravity_groups_sph: d_point_labels must hold one label per point");
    if (d_moments.size() != a.n_nodes * 12)
        throw std::invalid_argument("gravity_groups_sph: d_moments must hold 12 floats per node (gravity_group_moments_sph)");
    if (d_label_ranges.size() != a.n_nodes * 2)
        throw std::invalid_argument("gravity_groups_sph: d_label_ranges must hold 2 ints per node (gravity_group_moments_sph)");
    GRACE_STATUS_CHECK(grace_gravity_group_points_f4(
        reinterpret_cast<const float*>(raw(d_points)), d_points.size(), int(sizeof(PointType) / sizeof(float)),
        GRACE_SCENE(a), raw(d_masses), raw(d_labels), a.n_nodes ? raw(d_moments) : NULL,
        a.n_nodes ? raw(d_label_ranges) : NULL, raw(d_point_labels), theta, eps, out, counts, NULL));
    check_trace_status();
}

} // namespace detail

// d_moments as gravity_moments_sph's, over the labelled spheres only; d_label_ranges[i * 2 + ..] =
// {smallest, largest label >= 0 below node i} ({INT32_MAX, -1}: none).  Both resized.
template <typename Real4>
GRACE_HOST void gravity_group_moments_sph(const detail::dvec<Real4>& d_spheres, const detail::dvec<float>& d_masses,
                                          const detail::dvec<int>& d_labels, const Tree& d_tree,
                                          detail::dvec<float>& d_moments, detail::dvec<int>& d_label_ranges)
{
    static_assert(std::is_same<Real4, float4>::value, "gravity: float4 spheres only (float distances, double sums)");
    const detail::SceneArgs<Real4> a = detail::scene_args(d_spheres, d_tree);
    if (d_masses.size() != d_spheres.size())
        throw std::invalid_argument("gravity_group_moments_sph: d_masses must hold one mass per sphere");
    if (d_labels.size() != d_spheres.size())
        throw std::invalid_argument("gravity_group_moments_sph: d_labels must hold one label per sphere");
    d_moments.resize(a.n_nodes * 12);
    d_label_ranges.resize(a.n_nodes * 2);
    GRACE_STATUS_CHECK(grace_gravity_group_moments_f4(GRACE_SCENE(a), detail::raw(d_masses), detail::raw(d_labels),
                                                      a.n_nodes ? detail::raw(d_moments) : NULL,
                                                      a.n_nodes ? detail::raw(d_label_ranges) : NULL, NULL));
}

// d_out[p * 4 + ..] = {a_x, a_y, a_z, phi} at d_points[p] due to the spheres labelled d_point_labels[p]; resized.
template <typename PointType, typename Real4>
GRACE_HOST void gravity_groups_sph(const detail::dvec<PointType>& d_points, const detail::dvec<int>& d_point_labels,
                                   const detail::dvec<Real4>& d_spheres, const detail::dvec<float>& d_masses,
                                   const detail::dvec<int>& d_labels, const Tree& d_tree,
                                   const detail::dvec<float>& d_moments, const detail::dvec<int>& d_label_ranges,
                                   const float theta, const float eps, detail::dvec<double>& d_out)
{
    d_out.resize(d_points.size() * 4);
    detail::gravity_groups_call(d_points, d_point_labels, d_spheres, d_masses, d_labels, d_tree, d_moments,
                                d_label_ranges, theta, eps, detail::raw(d_out), (int*)NULL);
}

// ... and d_counts[p * 2 + ..] = {node terms, particle terms} of the point's walk; resized.
template <typename PointType, typename Real4>
GRACE_HOST void gravity_groups_sph(const detail::dvec<PointType>& d_points, const detail::dvec<int>& d_point_labels,
                                   const detail::dvec<Real4>& d_spheres, const detail::dvec<float>& d_masses,
                                   const detail::dvec<int>& d_labels, const Tree& d_tree,
                                   const detail::dvec<float>& d_moments, const detail::dvec<int>& d_label_ranges,
                                   const float theta, const float eps, detail::dvec<double>& d_out,
                                   detail::dvec<int>& d_counts)
{
    d_out.resize(d_points.size() * 4);
    d_counts.resize(d_points.size() * 2);
    detail::gravity_groups_call(d_points, d_point_labels, d_spheres, d_masses, d_labels, d_tree, d_moments,
                                d_label_ranges, theta, eps, detail::raw(d_out), detail::raw(d_counts));
}

} // namespace grace
