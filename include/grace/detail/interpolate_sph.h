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
//   Gradients of the same field (grace_interpolate_gradient_points_f4 / _grid_f4 and their periodic
// forms): interpolate_gradient_sph and interpolate_gradient_grid_sph write d_grad[(p * n_channels + c) * 3
// + k] = d_k A_c and, if given, the field's value and counts from the same walk; divergence_curl_sph turns
// the gradient of a 3-channel vector field into its divergence and curl (grace_gradient_div_curl_f32).
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

// d_grad holds 3 floats per point and channel; the optional outputs are sized like interpolate_sph's.
template <typename Real4>
inline void gradient_check(const dvec<Real4>& d_spheres, const dvec<float>& d_weights, int n_channels,
                           size_t n_points, const dvec<float>& d_grad, const dvec<float>* d_value,
                           const dvec<int>* d_counts)
{
    static_assert(std::is_same<Real4, float4>::value, "interpolate_gradient_sph: float4 spheres only (float weights and outputs)");
    if (n_channels < 1 || n_channels > 64)
        throw std::invalid_argument("interpolate_gradient_sph: n_channels must be 1..64");
    if (d_weights.size() != d_spheres.size() * size_t(n_channels))
        throw std::invalid_argument("interpolate_gradient_sph: d_weights must hold n_channels per sphere");
    if (d_grad.size() != n_points * size_t(n_channels) * 3)
        throw std::invalid_argument("interpolate_gradient_sph: d_grad must hold 3 n_channels per point");
    if (d_value && d_value->size() != n_points * size_t(n_channels))
        throw std::invalid_argument("interpolate_gradient_sph: d_value must hold n_channels per point");
    if (d_counts && d_counts->size() != n_points)
        throw std::invalid_argument("interpolate_gradient_sph: d_counts must hold one count per point");
}

// What every interpolate_gradient_sph overload does: grace_interpolate_gradient_points_f4 (box NULL) or
// its periodic form.
template <typename PointType, typename Real4>
inline void gradient_points(const dvec<PointType>& d_points, const dvec<Real4>& d_spheres, const Tree& d_tree,
                            const dvec<float>& d_weights, const int n_channels, dvec<float>& d_grad,
                            dvec<float>* d_value, dvec<int>* d_counts, const PeriodicBox* box)
{
    const int elems = interp_point_elems<PointType>();
    gradient_check(d_spheres, d_weights, n_channels, d_points.size(), d_grad, d_value, d_counts);
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    const float* points = reinterpret_cast<const float*>(raw(d_points));
    float* value = d_value ? raw(*d_value) : NULL;
    int* counts = d_counts ? raw(*d_counts) : NULL;
    if (box) {
        const float period[3] = { box->lx, box->ly, box->lz };
        GRACE_STATUS_CHECK(grace_interpolate_gradient_points_periodic_f4(points, d_points.size(), elems,
                                                                         GRACE_SCENE(a), raw(d_weights), n_channels,
                                                                         raw(d_grad), value, counts, period, NULL));
    } else {
        GRACE_STATUS_CHECK(grace_interpolate_gradient_points_f4(points, d_points.size(), elems, GRACE_SCENE(a),
                                                                raw(d_weights), n_channels, raw(d_grad), value,
                                                                counts, NULL));
    }
    check_trace_status();
}

// What every interpolate_gradient_grid_sph overload does.
template <typename Real4>
inline void gradient_grid(const float3 origin, const float3 u, const float3 v, const float3 w,
                          const int nx, const int ny, const int nz, const dvec<Real4>& d_spheres,
                          const Tree& d_tree, const dvec<float>& d_weights, const int n_channels,
                          dvec<float>& d_grad, dvec<float>* d_value, const PeriodicBox* box)
{
    if (nx <= 0 || ny <= 0 || nz <= 0)
        throw std::invalid_argument("interpolate_gradient_grid_sph: dimensions must be positive");
    const size_t n = size_t(nx) * size_t(ny) * size_t(nz);
    gradient_check(d_spheres, d_weights, n_channels, n, d_grad, d_value, (const dvec<int>*)NULL);
    const float o3[3] = { origin.x, origin.y, origin.z };
    const float uvw[9] = { u.x, u.y, u.z, v.x, v.y, v.z, w.x, w.y, w.z };
    const int d3[3] = { nx, ny, nz };
    const SceneArgs<Real4> a = scene_args(d_spheres, d_tree);
    float* value = d_value ? raw(*d_value) : NULL;
    if (box) {
        const float period[3] = { box->lx, box->ly, box->lz };
        GRACE_STATUS_CHECK(grace_interpolate_gradient_grid_periodic_f4(o3, uvw, d3, GRACE_SCENE(a), raw(d_weights),
                                                                       n_channels, raw(d_grad), value, NULL, period,
                                                                       NULL));
    } else {
        GRACE_STATUS_CHECK(grace_interpolate_gradient_grid_f4(o3, uvw, d3, GRACE_SCENE(a), raw(d_weights), n_channels,
                                                              raw(d_grad), value, NULL, NULL));
    }
    check_trace_status();
}

// What both divergence_curl_sph overloads do: the gradient of the three channels, then
// grace_gradient_div_curl_f32.
template <typename PointType, typename Real4>
inline void divergence_curl(const dvec<PointType>& d_points, const dvec<Real4>& d_spheres, const Tree& d_tree,
                            const dvec<float>& d_vectors, dvec<float>& d_div, dvec<float>& d_curl,
                            const PeriodicBox* box)
{
    if (d_div.size() != d_points.size() || d_curl.size() != d_points.size() * 3)
        throw std::invalid_argument("divergence_curl_sph: d_div must hold 1 and d_curl 3 floats per point");
    dvec<float> d_grad(d_points.size() * 9);
    gradient_points(d_points, d_spheres, d_tree, d_vectors, 3, d_grad, (dvec<float>*)NULL, (dvec<int>*)NULL, box);
    GRACE_STATUS_CHECK(grace_gradient_div_curl_f32(raw(d_grad), d_points.size(), raw(d_div), raw(d_curl), NULL));
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

// ---- SPH gradients at points (grace_interpolate_gradient_points_f4 / _grid_f4; grace_hip.h states the
//      arithmetic): d_grad[(p * n_channels + c) * 3 + k] = sum over spheres i containing d_points[p] of
//      fl(fl(w_ic H^-4 f'(q)) n_k), n the unit vector from the centre to the point.  d_value and d_counts
//      (if given) receive exactly interpolate_sph's d_out and d_counts. ----
template <typename PointType, typename Real4>
GRACE_HOST void interpolate_gradient_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                                         const Tree& d_tree, const detail::dvec<float>& d_weights,
                                         const int n_channels, detail::dvec<float>& d_grad,
                                         detail::dvec<float>* d_value = NULL, detail::dvec<int>* d_counts = NULL)
{
    detail::gradient_points(d_points, d_spheres, d_tree, d_weights, n_channels, d_grad, d_value, d_counts,
                            (const PeriodicBox*)NULL);
}

template <typename PointType, typename Real4>
GRACE_HOST void interpolate_gradient_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                                         const Tree& d_tree, const detail::dvec<float>& d_weights,
                                         const int n_channels, detail::dvec<float>& d_grad,
                                         detail::dvec<float>* d_value, detail::dvec<int>* d_counts,
                                         const PeriodicBox& box)
{
    detail::gradient_points(d_points, d_spheres, d_tree, d_weights, n_channels, d_grad, d_value, d_counts, &box);
}

// The lattice of interpolate_grid_sph; d_grad row-major like its d_out, 3 floats per point and channel.
template <typename Real4>
GRACE_HOST void interpolate_gradient_grid_sph(const float3 origin, const float3 u, const float3 v, const float3 w,
                                              const int nx, const int ny, const int nz,
                                              const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                              const detail::dvec<float>& d_weights, const int n_channels,
                                              detail::dvec<float>& d_grad, detail::dvec<float>* d_value = NULL)
{
    detail::gradient_grid(origin, u, v, w, nx, ny, nz, d_spheres, d_tree, d_weights, n_channels, d_grad, d_value,
                          (const PeriodicBox*)NULL);
}

template <typename Real4>
GRACE_HOST void interpolate_gradient_grid_sph(const float3 origin, const float3 u, const float3 v, const float3 w,
                                              const int nx, const int ny, const int nz,
                                              const detail::dvec<Real4>& d_spheres, const Tree& d_tree,
                                              const detail::dvec<float>& d_weights, const int n_channels,
                                              detail::dvec<float>& d_grad, detail::dvec<float>* d_value,
                                              const PeriodicBox& box)
{
    detail::gradient_grid(origin, u, v, w, nx, ny, nz, d_spheres, d_tree, d_weights, n_channels, d_grad, d_value, &box);
}

// Divergence and curl at points of the vector field with the weights d_vectors (3 per sphere, e.g.
// m / rho * v): d_div[p] = fl(fl(g_xx + g_yy) + g_zz), d_curl[p * 3 + 0..2] = (g_zy - g_yz, g_xz - g_zx,
// g_yx - g_xy) of the 3-channel gradient g_ck = d_k A_c (grace_gradient_div_curl_f32).
template <typename PointType, typename Real4>
GRACE_HOST void divergence_curl_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                                    const Tree& d_tree, const detail::dvec<float>& d_vectors,
                                    detail::dvec<float>& d_div, detail::dvec<float>& d_curl)
{
    detail::divergence_curl(d_points, d_spheres, d_tree, d_vectors, d_div, d_curl, (const PeriodicBox*)NULL);
}

template <typename PointType, typename Real4>
GRACE_HOST void divergence_curl_sph(const detail::dvec<PointType>& d_points, const detail::dvec<Real4>& d_spheres,
                                    const Tree& d_tree, const detail::dvec<float>& d_vectors,
                                    detail::dvec<float>& d_div, detail::dvec<float>& d_curl, const PeriodicBox& box)
{
    detail::divergence_curl(d_points, d_spheres, d_tree, d_vectors, d_div, d_curl, &box);
}

} // namespace grace
