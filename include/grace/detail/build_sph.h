// grace/detail/build_sph.h -- the one definition of the SPH build API (reference
// include/grace/cuda/build_sph.cuh:16-124), shared by the drop-in grace/cuda/build_sph.cuh and the
// HIP-free mirror grace/grace.h; every body a type dispatch onto libgrace_hip.so.  The including
// front end has defined detail::dvec, detail::raw, GRACE_STATUS_CHECK, Tree and the vector types
// beforehand (grace/detail/front_end.h lists them).
//
//   morton_keys_sph            -> grace_morton_keys{30,63}_f4[_d3] / _points[_d3]   (csrc/morton.hip)
//   morton_keys{30,63}_sort_sph-> the same + grace_sort_pairs_u32/u64               (csrc/sort.hip;
//                                 the reference calls thrust::sort_by_key: stable, in place)
//   euclidean / surface_area / XOR _deltas_sph -> grace_deltas_*                    (csrc/deltas.hip)
//   ALBVH_sph                  -> grace_albvh_build_*                               (csrc/albvh.hip)
//
// Real4 is float4 or double4, KeyType / XOR DeltaType uinteger32 or uinteger64, Real the scalar
// type of Real4 (as the reference requires, build_sph.cuh:84-86) or float for double4 (the delta
// functors return float whatever Real is, generic/functors/albvh.h:44-74).
#pragma once

#include "grace/detail/front_end.h"

namespace grace {

namespace detail {

// ---- Morton keys: (Real4, bounds precision, key type) -> entry point -----------------------
inline void keys_dispatch(const float4* s, size_t n, const float* b, const float* t, uinteger32* k)
{ GRACE_STATUS_CHECK(grace_morton_keys30_f4(reinterpret_cast<const float*>(s), n, b, t, k, NULL)); }
inline void keys_dispatch(const float4* s, size_t n, const float* b, const float* t, uinteger64* k)
{ GRACE_STATUS_CHECK(grace_morton_keys63_f4(reinterpret_cast<const float*>(s), n, b, t, k, NULL)); }
inline void keys_dispatch(const float4* s, size_t n, const double* b, const double* t, uinteger32* k)
{ GRACE_STATUS_CHECK(grace_morton_keys30_f4_d3(reinterpret_cast<const float*>(s), n, b, t, k, NULL)); }
inline void keys_dispatch(const float4* s, size_t n, const double* b, const double* t, uinteger64* k)
{ GRACE_STATUS_CHECK(grace_morton_keys63_f4_d3(reinterpret_cast<const float*>(s), n, b, t, k, NULL)); }
// double4: keys from the co-ordinates narrowed to float (CentroidSphere)
inline void keys_dispatch(const double4* s, size_t n, const float* b, const float* t, uinteger32* k)
{ GRACE_STATUS_CHECK(grace_morton_keys30_points(s, n, 1, 4, b, t, k, NULL)); }
inline void keys_dispatch(const double4* s, size_t n, const float* b, const float* t, uinteger64* k)
{ GRACE_STATUS_CHECK(grace_morton_keys63_points(s, n, 1, 4, b, t, k, NULL)); }
inline void keys_dispatch(const double4* s, size_t n, const double* b, const double* t, uinteger32* k)
{ GRACE_STATUS_CHECK(grace_morton_keys30_points_d3(s, n, 1, 4, b, t, k, NULL)); }
inline void keys_dispatch(const double4* s, size_t n, const double* b, const double* t, uinteger64* k)
{ GRACE_STATUS_CHECK(grace_morton_keys63_points_d3(s, n, 1, 4, b, t, k, NULL)); }
// float3 points (the centroids of the generic morton_keys forms, kernels/morton.cuh)
inline void keys_dispatch(const float3* c, size_t n, const float* b, const float* t, uinteger32* k)
{ GRACE_STATUS_CHECK(grace_morton_keys30_points(c, n, 0, 3, b, t, k, NULL)); }
inline void keys_dispatch(const float3* c, size_t n, const float* b, const float* t, uinteger64* k)
{ GRACE_STATUS_CHECK(grace_morton_keys63_points(c, n, 0, 3, b, t, k, NULL)); }
inline void keys_dispatch(const float3* c, size_t n, const double* b, const double* t, uinteger32* k)
{ GRACE_STATUS_CHECK(grace_morton_keys30_points_d3(c, n, 0, 3, b, t, k, NULL)); }
inline void keys_dispatch(const float3* c, size_t n, const double* b, const double* t, uinteger64* k)
{ GRACE_STATUS_CHECK(grace_morton_keys63_points_d3(c, n, 0, 3, b, t, k, NULL)); }

// Centroid bounds of the spheres (the bounds-free overloads: compute_centroids + min/max,
// kernels/morton.cuh:139-174); centroids are float3 for either Real4.
inline void centroid_bounds(const float4* s, size_t n, float* b, float* t)
{ GRACE_STATUS_CHECK(grace_centroid_bounds_f4(reinterpret_cast<const float*>(s), n, b, t, NULL)); }
inline void centroid_bounds(const double4* s, size_t n, float* b, float* t)
{ GRACE_STATUS_CHECK(grace_centroid_bounds_points(s, n, 1, 4, b, t, NULL)); }

// ---- stable sort of the spheres by key, in place --------------------------------------------
template <typename Real4>
inline void sort_spheres(dvec<uinteger32>& k, dvec<Real4>& s, int bits)
{ GRACE_STATUS_CHECK(grace_sort_pairs_u32(raw(k), raw(s), s.size(), int(sizeof(Real4)), 0, bits, NULL, NULL)); }
template <typename Real4>
inline void sort_spheres(dvec<uinteger64>& k, dvec<Real4>& s, int bits)
{ GRACE_STATUS_CHECK(grace_sort_pairs_u64(raw(k), raw(s), s.size(), int(sizeof(Real4)), 0, bits, NULL, NULL)); }

// ---- deltas ------------------------------------------------------------------------------------
inline void euclid_dispatch(const float4* s, size_t n, float* d)
{ GRACE_STATUS_CHECK(grace_deltas_euclid_f4(reinterpret_cast<const float*>(s), n, d, NULL)); }
inline void euclid_dispatch(const double4* s, size_t n, double* d)
{ GRACE_STATUS_CHECK(grace_deltas_euclid_d4_f64(reinterpret_cast<const double*>(s), n, d, NULL)); }
inline void euclid_dispatch(const double4* s, size_t n, float* d)
{ GRACE_STATUS_CHECK(grace_deltas_euclid_d4(reinterpret_cast<const double*>(s), n, d, NULL)); }
inline void area_dispatch(const float4* s, size_t n, float* d)
{ GRACE_STATUS_CHECK(grace_deltas_area_f4(reinterpret_cast<const float*>(s), n, d, NULL)); }
inline void area_dispatch(const double4* s, size_t n, double* d)
{ GRACE_STATUS_CHECK(grace_deltas_area_d4_f64(reinterpret_cast<const double*>(s), n, d, NULL)); }
inline void area_dispatch(const double4* s, size_t n, float* d)
{ GRACE_STATUS_CHECK(grace_deltas_area_d4(reinterpret_cast<const double*>(s), n, d, NULL)); }
inline void xor_dispatch(const uinteger32* k, size_t n, uinteger32* d)
{ GRACE_STATUS_CHECK(grace_deltas_xor_u32(k, n, d, NULL)); }
inline void xor_dispatch(const uinteger64* k, size_t n, uinteger64* d)
{ GRACE_STATUS_CHECK(grace_deltas_xor_u64(k, n, d, NULL)); }

// ---- ALBVH: (Real4, DeltaType) -> entry point ------------------------------------------------
#define GRACE_ALBVH_DISPATCH(PRIM_T, CAST_T, DELTA_T, FN)                                        \
    inline void albvh_dispatch(const PRIM_T* s, size_t n, const DELTA_T* d, int mpl, int* nodes, \
                               int* leaves, int* root, size_t* n_leaves)                         \
    { GRACE_STATUS_CHECK(FN(reinterpret_cast<const CAST_T*>(s), n, d, mpl, nodes, leaves, root,  \
                            n_leaves, NULL)); }
GRACE_ALBVH_DISPATCH(float4, float, float, grace_albvh_build_f4)
GRACE_ALBVH_DISPATCH(float4, float, double, grace_albvh_build_f4_f64)
GRACE_ALBVH_DISPATCH(float4, float, uinteger32, grace_albvh_build_f4_u32)
GRACE_ALBVH_DISPATCH(float4, float, uinteger64, grace_albvh_build_f4_u64)
GRACE_ALBVH_DISPATCH(double4, double, float, grace_albvh_build_d4)
GRACE_ALBVH_DISPATCH(double4, double, double, grace_albvh_build_d4_f64)
GRACE_ALBVH_DISPATCH(double4, double, uinteger32, grace_albvh_build_d4_u32)
GRACE_ALBVH_DISPATCH(double4, double, uinteger64, grace_albvh_build_d4_u64)
#undef GRACE_ALBVH_DISPATCH

// Bounds arrive as any type with .x/.y/.z; the arithmetic precision is that of Real3's
// components (kernels/morton.cuh:104-113).
template <typename Real3> struct bounds_scalar { typedef float type; };
template <> struct bounds_scalar<double3> { typedef double type; };
template <> struct bounds_scalar<double4> { typedef double type; };

} // namespace detail

// build_sph.cuh:19-25: bounds from the centroids.
// Real4 should be float4 or double4.
// KeyType should be grace::uinteger{32,64}.
template <typename Real4, typename KeyType>
GRACE_HOST void morton_keys_sph(
    const detail::dvec<Real4>& d_spheres,
    detail::dvec<KeyType>& d_keys)
{
    float bot[3], top[3];
    detail::centroid_bounds(detail::raw(d_spheres), d_spheres.size(), bot, top);
    detail::keys_dispatch(detail::raw(d_spheres), d_spheres.size(), bot, top, detail::raw(d_keys));
}

// build_sph.cuh:27-35
template <typename Real3, typename Real4, typename KeyType>
GRACE_HOST void morton_keys_sph(
    const detail::dvec<Real4>& d_spheres,
    const Real3 bot,
    const Real3 top,
    detail::dvec<KeyType>& d_keys)
{
    typedef typename detail::bounds_scalar<Real3>::type B;
    B b[3], t[3];
    detail::xyz(bot, b);
    detail::xyz(top, t);
    detail::keys_dispatch(detail::raw(d_spheres), d_spheres.size(), b, t, detail::raw(d_keys));
}

// build_sph.cuh:41-47.  Generates 30-bit Morton keys and sorts the spheres by them (stable; in
// place).  Requires O(N) on-device temporary storage.
template <typename Real4>
GRACE_HOST void morton_keys30_sort_sph(
    detail::dvec<Real4>& d_spheres)
{
    detail::dvec<grace::uinteger32> d_keys;
    d_keys.resize(d_spheres.size());
    morton_keys_sph(d_spheres, d_keys);
    detail::sort_spheres(d_keys, d_spheres, 30);
}

// build_sph.cuh:50-58
template <typename Real3, typename Real4>
GRACE_HOST void morton_keys30_sort_sph(
    detail::dvec<Real4>& d_spheres,
    const Real3 bot,
    const Real3 top)
{
    detail::dvec<grace::uinteger32> d_keys;
    d_keys.resize(d_spheres.size());
    morton_keys_sph(d_spheres, bot, top, d_keys);
    detail::sort_spheres(d_keys, d_spheres, 30);
}

// build_sph.cuh:65-71.  Generates 63-bit Morton keys and sorts the spheres by them.
template <typename Real4>
GRACE_HOST void morton_keys63_sort_sph(
    detail::dvec<Real4>& d_spheres)
{
    detail::dvec<grace::uinteger64> d_keys;
    d_keys.resize(d_spheres.size());
    morton_keys_sph(d_spheres, d_keys);
    detail::sort_spheres(d_keys, d_spheres, 63);
}

// build_sph.cuh:74-82
template <typename Real3, typename Real4>
GRACE_HOST void morton_keys63_sort_sph(
    detail::dvec<Real4>& d_spheres,
    const Real3 bot,
    const Real3 top)
{
    detail::dvec<grace::uinteger64> d_keys;
    d_keys.resize(d_spheres.size());
    morton_keys_sph(d_spheres, bot, top, d_keys);
    detail::sort_spheres(d_keys, d_spheres, 63);
}

// build_sph.cuh:87-94
template <typename Real4, typename Real>
GRACE_HOST void euclidean_deltas_sph(
    const detail::dvec<Real4>& d_spheres,
    detail::dvec<Real>& d_deltas)
{
    GRACE_ASSERT(d_spheres.size() + 1 == d_deltas.size());
    detail::euclid_dispatch(detail::raw(d_spheres), d_spheres.size(), detail::raw(d_deltas));
}

// build_sph.cuh:98-105
template <typename Real4, typename Real>
GRACE_HOST void surface_area_deltas_sph(
    const detail::dvec<Real4>& d_spheres,
    detail::dvec<Real>& d_deltas)
{
    GRACE_ASSERT(d_spheres.size() + 1 == d_deltas.size());
    detail::area_dispatch(detail::raw(d_spheres), d_spheres.size(), detail::raw(d_deltas));
}

// build_sph.cuh:109-114.  KeyType should be grace::uinteger{32,64}; DeltaType the same type.
template <typename KeyType, typename DeltaType>
GRACE_HOST void XOR_deltas_sph(
    const detail::dvec<KeyType>& d_morton_keys,
    detail::dvec<DeltaType>& d_deltas)
{
    GRACE_ASSERT(d_morton_keys.size() + 1 == d_deltas.size());
    detail::xor_dispatch(detail::raw(d_morton_keys), d_morton_keys.size(), detail::raw(d_deltas));
}

// build_sph.cuh:118-124 -> build_ALBVH (kernels/albvh.cuh:986-1021).  Real4 should be float4 or
// double4.  Throws std::invalid_argument if the number of spheres does not exceed
// d_tree.max_per_leaf (albvh.cuh:795-799).  Resizes d_tree.nodes / leaves to the tree that was
// built (albvh.cuh:842-845), after growing them to the capacity the build writes into.
template <typename Real4, typename DeltaType>
GRACE_HOST void ALBVH_sph(
    const detail::dvec<Real4>& d_spheres,
    const detail::dvec<DeltaType>& d_deltas,
    Tree& d_tree)
{
    const size_t n = d_spheres.size();
    GRACE_ASSERT(n + 1 == d_deltas.size());
    if (d_tree.leaves.size() < n) d_tree.leaves.resize(n);
    if (n && d_tree.nodes.size() < 4 * (n - 1)) d_tree.nodes.resize(4 * (n - 1));
    size_t n_leaves = 0;
    detail::albvh_dispatch(detail::raw(d_spheres), n, detail::raw(d_deltas), d_tree.max_per_leaf,
                           reinterpret_cast<int*>(detail::raw(d_tree.nodes)),
                           reinterpret_cast<int*>(detail::raw(d_tree.leaves)),
                           d_tree.root_index_ptr, &n_leaves);
    d_tree.leaves.resize(n_leaves);
    d_tree.nodes.resize(4 * (n_leaves - 1));
}

} // namespace grace
