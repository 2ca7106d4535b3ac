// grace/detail/interpolate_sph.h -- the one definition of SPH interpolation at points, an extension
// the reference lacks, shared by the drop-in grace/cuda/interpolate_sph.cuh and the HIP-free mirror
// grace/grace.h (grace/detail/front_end.h): the field A(p) = sum_i fl(w_i W(|p - x_i|, H_i)) of the
// spheres (tree order, w = support radius H) with the context's SPH kernel (set_sph_kernel; a custom
// table is refused), and the number of spheres containing each point -- grace_interpolate_points_f4 /
// grace_interpolate_grid_f4 (grace_hip.h states the arithmetic and the summation order).  d_weights
// holds n_channels weights per sphere, sphere-major, in the order of d_spheres; d_out[p * n_channels
// + c].  float4 spheres only; points are 3..16 floats, x y z first.  Size mismatches throw
// std::invalid_argument; a stack overflow is reported as by the traces.
#pragma once

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

} // namespace detail

// d_out[p * n_channels + c] = sum over spheres i containing d_points[p] of fl(d_weights[i * n_channels + c] W_ip),
// and d_counts[p] (if given) = the number of spheres containing d_points[p].
template <typename PointType, typename Real4>
GRACE_HOST void interpolate_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                                const Tree& d_tree, const detail::dvec<float>& d_weights, const int n_channels,
                                detail::dvec<float>& d_out, detail::dvec<int>* d_counts = NULL)
{
    const int elems = detail::interp_point_elems<PointType>();
    detail::interp_check(d_spheres, detail::raw(d_weights), d_weights.size(), n_channels, d_points.size(), d_out.size());
    if (d_counts && d_counts->size() != d_points.size())
        throw std::invalid_argument("interpolate_sph: d_counts must hold one count per point");
    const detail::SceneArgs<Real4> a = detail::scene_args(d_spheres, d_tree);
    GRACE_STATUS_CHECK(grace_interpolate_points_f4(
        reinterpret_cast<const float*>(detail::raw(d_points)), d_points.size(), elems, GRACE_SCENE(a),
        detail::raw(d_weights), n_channels, detail::raw(d_out), d_counts ? detail::raw(*d_counts) : NULL, NULL));
    detail::check_trace_status();
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
    if (nx <= 0 || ny <= 0 || nz <= 0)
        throw std::invalid_argument("interpolate_grid_sph: dimensions must be positive");
    const size_t n = size_t(nx) * size_t(ny) * size_t(nz);
    detail::interp_check(d_spheres, detail::raw(d_weights), d_weights.size(), n_channels, n, d_out.size());
    const float o3[3] = { origin.x, origin.y, origin.z };
    const float uvw[9] = { u.x, u.y, u.z, v.x, v.y, v.z, w.x, w.y, w.z };
    const int d3[3] = { nx, ny, nz };
    const detail::SceneArgs<Real4> a = detail::scene_args(d_spheres, d_tree);
    GRACE_STATUS_CHECK(grace_interpolate_grid_f4(o3, uvw, d3, GRACE_SCENE(a), detail::raw(d_weights), n_channels,
                                                 detail::raw(d_out), NULL, NULL));
    detail::check_trace_status();
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

} // namespace grace
