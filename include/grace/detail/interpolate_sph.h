// grace/detail/interpolate_sph.h -- the one definition of SPH interpolation at points, an extension
// the reference lacks, shared by the drop-in grace/cuda/interpolate_sph.cuh and the HIP-free mirror
// grace/grace.h (grace/detail/front_end.h): the field A(p) = sum_i fl(w_i W(|p - x_i|, H_i)) of the
// spheres (tree order, w = support radius H) with the context's SPH kernel (set_sph_kernel; a custom
// table is refused), and the number of spheres containing each point -- grace_interpolate_points_f4 /
// grace_interpolate_grid_f4 (grace_hip.h states the arithmetic and the summation order).  d_weights
// holds n_channels weights per sphere, sphere-major, in the order of d_spheres; d_out[p * n_channels
// + c].  float4 spheres only; points are 3..16 floats, x y z first.  Size mismatches throw
// std::invalid_argument; a stack overflow is reported as by the traces.  Every function has an overload
// with a trailing grace::PeriodicBox (grace/detail/periodic_box.h): the separation wraps once per
// component, and a sphere whose H exceeds half a period contributes nothing
// (grace_interpolate_points_periodic_f4 / grace_interpolate_grid_periodic_f4).
#pragma once

#include "grace/detail/periodic_box.h"
#include "grace/detail/trace_sph.h"

namespace grace {

namespace detail {

template <typename PointType>
inline int interp_point_elems()
{
    static_assert(sizeof(PointType) % sizeof(float) == 0 && sizeof(PointType) >= 3 * sizeof(float)
                      && sizeof(PointType) <= 16 * sizeof(float),
                  "interpolate_sph: points are 3..16 floats, x y z first");
    return int(sizeof(PointType) / sizeof(float));
}

// Without weights (an empty d_weights) the C ABI decides: counts alone are allowed, d_out is not.
template <typename Real4>
inline void interp_check(const dvec<Real4>& d_spheres, const float* weights, size_t n_weights,
                         int n_channels, size_t n_points, size_t n_out)
{
    static_assert(std::is_same<Real4, float4>::value, "interpolate_sph: float4 spheres only (float weights and outputs)");
    if (weights) {
        if (n_channels < 1 || n_channels > 64)
            throw std::invalid_argument("interpolate_sph: n_channels must be 1..64");
        if (n_weights != d_spheres.size() * size_t(n_channels))
            throw std::invalid_argument("interpolate_sph: d_weights must hold n_channels per sphere");
        if (n_out != n_points * size_t(n_channels))
            throw std::invalid_argument("interpolate_sph: d_out must hold n_channels per point");
    }
}

// What every interpolate_sph overload does: grace_interpolate_points_f4 (box NULL) or its periodic form.
template <typename PointType, typename Real4>
inline void interpolate_points(const dvec<PointType>& d_points, const dvec<Real4>& d_spheres, const Tree& d_tree,
                               const dvec<float>& d_weights, const int n_channels, dvec<float>& d_out,
                               dvec<int>* d_counts, const PeriodicBox* box)
{
    const int elems = interp_point_elems<PointType>();
    interp_check(d_spheres, raw(d_weights), d_weights.size(), n_channels, d_points.size(), d_out.size());
    if (d_counts && d_counts->size() != d_points.size())
        throw std::invalid_argument("interpolate_sph: d_counts must hold one count per point");
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    const float* points = reinterpret_cast<const float*>(raw(d_points));
    int* counts = d_counts ? raw(*d_counts) : NULL;
    if (box) {
        const float period[3] = { box->lx, box->ly, box->lz };
        GRACE_STATUS_CHECK(grace_interpolate_points_periodic_f4(points, d_points.size(), elems, GRACE_SCENE(a),
                                                                raw(d_weights), n_channels, raw(d_out), counts,
                                                                period, NULL));
    } else {
        GRACE_STATUS_CHECK(grace_interpolate_points_f4(points, d_points.size(), elems, GRACE_SCENE(a), raw(d_weights),
                                                       n_channels, raw(d_out), counts, NULL));
    }
    check_trace_status();
}

// What every interpolate_grid_sph overload does.
template <typename Real4>
inline void interpolate_grid(const float3 origin, const float3 u, const float3 v, const float3 w,
                             const int nx, const int ny, const int nz, const dvec<Real4>& d_spheres,
                             const Tree& d_tree, const dvec<float>& d_weights, const int n_channels,
                             dvec<float>& d_out, const PeriodicBox* box)
{
    if (nx <= 0 || ny <= 0 || nz <= 0)
        throw std::invalid_argument("interpolate_grid_sph: dimensions must be positive");
    const size_t n = size_t(nx) * size_t(ny) * size_t(nz);
    interp_check(d_spheres, raw(d_weights), d_weights.size(), n_channels, n, d_out.size());
    const float o3[3] = { origin.x, origin.y, origin.z };
    const float uvw[9] = { u.x, u.y, u.z, v.x, v.y, v.z, w.x, w.y, w.z };
    const int d3[3] = { nx, ny, nz };
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    if (box) {
        const float period[3] = { box->lx, box->ly, box->lz };
        GRACE_STATUS_CHECK(grace_interpolate_grid_periodic_f4(o3, uvw, d3, GRACE_SCENE(a), raw(d_weights), n_channels,
                                                              raw(d_out), NULL, period, NULL));
    } else {
        GRACE_STATUS_CHECK(grace_interpolate_grid_f4(o3, uvw, d3, GRACE_SCENE(a), raw(d_weights), n_channels,
                                                     raw(d_out), NULL, NULL));
    }
    check_trace_status();
}

} // namespace detail

// d_out[p * n_channels + c] = sum over spheres i containing d_points[p] of fl(d_weights[i * n_channels + c] W_ip),
// and d_counts[p] (if given) = the number of spheres containing d_points[p].
template <typename PointType, typename Real4>
GRACE_HOST void interpolate_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                                const Tree& d_tree, const detail::dvec<float>& d_weights, const int n_channels,
                                detail::dvec<float>& d_out, detail::dvec<int>* d_counts = NULL)
{
    detail::interpolate_points(d_points, d_spheres, d_tree, d_weights, n_channels, d_out, d_counts,
                               (const PeriodicBox*)NULL);
}

// The same with the counts by reference.
template <typename PointType, typename Real4>
GRACE_HOST void interpolate_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                                const Tree& d_tree, const detail::dvec<float>& d_weights, const int n_channels,
                                detail::dvec<float>& d_out, detail::dvec<int>& d_counts)
{
    interpolate_sph(d_points, d_spheres, d_tree, d_weights, n_channels, d_out, &d_counts);
}

// The lattice p(i, j, k) = origin + i u + j v + k w, 0 <= i < nx ...; outputs row-major (k slowest,
// i fastest), d_out[p * n_channels + c].  nz == 1 is a slice.
template <typename Real4>
GRACE_HOST void interpolate_grid_sph(const float3 origin, const float3 u, const float3 v, const float3 w,
                                     const int nx, const int ny, const int nz,
                                     const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                     const detail::dvec<float>& d_weights, const int n_channels,
                                     detail::dvec<float>& d_out)
{
    detail::interpolate_grid(origin, u, v, w, nx, ny, nz, d_spheres, d_tree, d_weights, n_channels, d_out,
                             (const PeriodicBox*)NULL);
}

// The same with the dimensions as one int3.
template <typename Real4>
GRACE_HOST void interpolate_grid_sph(const float3 origin, const float3 u, const float3 v, const float3 w,
                                     const int3 dims, const detail::dvec<Real4>& d_spheres,
                                     const Tree& d_tree, const detail::dvec<float>& d_weights,
                                     const int n_channels, detail::dvec<float>& d_out)
{
    interpolate_grid_sph(origin, u, v, w, dims.x, dims.y, dims.z, d_spheres, d_tree, d_weights, n_channels, d_out);
}

// ---- the same in a periodic box: the separation wraps once per component; a sphere whose H exceeds
//      half a period is off ----
template <typename PointType, typename Real4>
GRACE_HOST void interpolate_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                                const Tree& d_tree, const detail::dvec<float>& d_weights, const int n_channels,
                                detail::dvec<float>& d_out, const PeriodicBox& box)
{
    detail::interpolate_points(d_points, d_spheres, d_tree, d_weights, n_channels, d_out, (detail::dvec<int>*)NULL, &box);
}

template <typename PointType, typename Real4>
GRACE_HOST void interpolate_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                                const Tree& d_tree, const detail::dvec<float>& d_weights, const int n_channels,
                                detail::dvec<float>& d_out, detail::dvec<int>& d_counts, const PeriodicBox& box)
{
    detail::interpolate_points(d_points, d_spheres, d_tree, d_weights, n_channels, d_out, &d_counts, &box);
}

template <typename Real4>
GRACE_HOST void interpolate_grid_sph(const float3 origin, const float3 u, const float3 v, const float3 w,
                                     const int nx, const int ny, const int nz,
                                     const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                     const detail::dvec<float>& d_weights, const int n_channels,
                                     detail::dvec<float>& d_out, const PeriodicBox& box)
{
    detail::interpolate_grid(origin, u, v, w, nx, ny, nz, d_spheres, d_tree, d_weights, n_channels, d_out, &box);
}

template <typename Real4>
GRACE_HOST void interpolate_grid_sph(const float3 origin, const float3 u, const float3 v, const float3 w,
                                     const int3 dims, const detail::dvec<Real4>& d_spheres,
                                     const Tree& d_tree, const detail::dvec<float>& d_weights,
                                     const int n_channels, detail::dvec<float>& d_out, const PeriodicBox& box)
{
    detail::interpolate_grid(origin, u, v, w, dims.x, dims.y, dims.z, d_spheres, d_tree, d_weights, n_channels, d_out,
                             &box);
}

} // namespace grace
