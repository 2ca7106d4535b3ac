// grace/detail/trace_sph.h -- the one definition of the SPH trace API (reference
// include/grace/cuda/trace_sph.cuh:22-241, plus this library's extensions), shared by the drop-in
// grace/cuda/trace_sph.cuh and the HIP-free mirror grace/grace.h, written against the names
// grace/detail/front_end.h lists.
//
// (Real4, Real) is (float4, float), (double4, double) or (float4, double) -- float spheres under the
// fp64 test with double sums and per-hit outputs, the reference's promotions for that pair --;
// (double4, float) is refused at compile time.  IndexType is a 32-bit integer.  Per-ray
// results equal the brute-force loop over all spheres (the reference's own criterion,
// tests/tree_traversal); column densities are the class-ordered fp32 sum documented in
// grace_hip.h (within 1e-6 of the reference's single running sum).  As in the reference the
// number of rays must be a multiple of 32 (bintree_trace.cuh:231-238: std::invalid_argument).
#pragma once

#include "grace/detail/front_end.h"

#include <array>
#include <limits>
#include <stdexcept>
#include <type_traits>
#include <vector>

namespace grace {

// include/grace/cuda/trace_sph.cuh:22-50: the normalised cubic-spline column kernel,
// F(b / h) at 51 equidistant impact parameters; libgrace_hip.so holds the same table.
const int N_table = 51;

template <typename Real>
struct KernelIntegrals
{
    const static Real table[N_table];
};

template <typename Real>
const Real KernelIntegrals<Real>::table[N_table] = {
    Real(1.90986019771937), Real(1.90563449910964), Real(1.89304415940934), Real(1.87230928086763),
    Real(1.84374947679902), Real(1.80776276033034), Real(1.76481079856299), Real(1.71540816859939),
    Real(1.66011373131439), Real(1.59952322363667), Real(1.53426266082279), Real(1.46498233888091),
    Real(1.39235130929287), Real(1.31705223652377), Real(1.23977618317103), Real(1.16121278415369),
    Real(1.08201943664419), Real(1.00288866679720), Real(0.924475767210246), Real(0.847415371038733),
    Real(0.772316688105931), Real(0.699736940377312), Real(0.630211918937167), Real(0.564194562399538),
    Real(0.502076205853037), Real(0.444144023534733), Real(0.390518196140658), Real(0.341148855945766),
    Real(0.295941946237307), Real(0.254782896476983), Real(0.217538645099225), Real(0.184059547649710),
    Real(0.154181189781890), Real(0.127726122453554), Real(0.104505535066266),
    Real(8.432088120445191E-002), Real(6.696547102921641E-002), Real(5.222604427168923E-002),
    Real(3.988433820097490E-002), Real(2.971866601747601E-002), Real(2.150552303075515E-002),
    Real(1.502124104014533E-002), Real(1.004371608622562E-002), Real(6.354242122978656E-003),
    Real(3.739494884706115E-003), Real(1.993729589156428E-003), Real(9.212900163813992E-004),
    Real(3.395908945333921E-004), Real(8.287326418242995E-005), Real(7.387919939044624E-006),
    Real(0.000000000000000E+000)
};

namespace detail {

inline void check_ray_count(size_t n_rays)
{
    // bintree_trace.cuh:231-238
    if (n_rays % 32 != 0)
        throw std::invalid_argument("Number of rays must be a multiple of the warp size (32).");
}

// What every tree-using entry point of the C ABI takes: rays (none for the point queries), spheres
// as their scalars, and the tree.  Formed here and nowhere else; spelled out in a call by
// GRACE_SCENE / GRACE_RAYS_SCENE.
template <typename Real4> struct sphere_scalar;
template <> struct sphere_scalar<float4> { typedef float type; };
template <> struct sphere_scalar<double4> { typedef double type; };

template <typename Real4>
struct SceneArgs
{
    const Ray* rays; size_t n_rays;
    const typename sphere_scalar<Real4>::type* spheres; size_t n_spheres;
    const int* nodes; size_t n_nodes; const int* leaves; const int* root;
};

template <typename Real4>
inline SceneArgs<Real4> scene_args(const dvec<Real4>& d_spheres, const Tree& t)
{
    SceneArgs<Real4> a = { NULL, 0,
                           reinterpret_cast<const typename sphere_scalar<Real4>::type*>(raw(d_spheres)),
                           d_spheres.size(), reinterpret_cast<const int*>(raw(t.nodes)),
                           t.leaves.size() - 1, reinterpret_cast<const int*>(raw(t.leaves)),
                           t.root_index_ptr };
    return a;
}

template <typename Real4>
inline SceneArgs<Real4> scene_args(const dvec<Ray>& d_rays, const dvec<Real4>& d_spheres, const Tree& t)
{
    SceneArgs<Real4> a = scene_args(d_spheres, t);
    a.rays = raw(d_rays);
    a.n_rays = d_rays.size();
    return a;
}

#define GRACE_SCENE(a) (a).spheres, (a).n_spheres, (a).nodes, (a).n_nodes, (a).leaves, (a).root
#define GRACE_RAYS_SCENE(a) (a).rays, (a).n_rays, GRACE_SCENE(a)

inline void hitcounts_dispatch(const SceneArgs<float4>& a, int* out)
{ GRACE_STATUS_CHECK(grace_trace_hitcounts_f4(GRACE_RAYS_SCENE(a), out, NULL)); }
inline void hitcounts_dispatch(const SceneArgs<double4>& a, int* out)
{ GRACE_STATUS_CHECK(grace_trace_hitcounts_d4(GRACE_RAYS_SCENE(a), out, NULL)); }

// The hit-count pass of trace_sph: the library keeps what the per-hit pass can reuse.
// The last argument names Real: the counts must come from the test the per-hit pass applies.
inline void hitcounts_keep_dispatch(const SceneArgs<float4>& a, int* out, const float*)
{ GRACE_STATUS_CHECK(grace_trace_hitcounts_keep_f4(GRACE_RAYS_SCENE(a), out, NULL)); }
inline void hitcounts_keep_dispatch(const SceneArgs<double4>& a, int* out, const double*)
{ hitcounts_dispatch(a, out); }
// (float4, double): the fp64 test in both passes, so offsets and written hits always agree (the
// reference sizes with the float test here)
inline void hitcounts_keep_dispatch(const SceneArgs<float4>& a, int* out, const double*)
{ GRACE_STATUS_CHECK(grace_trace_hitcounts_f4_f64(GRACE_RAYS_SCENE(a), out, NULL)); }

inline void cumulative_dispatch(const SceneArgs<float4>& a, float* out)
{ GRACE_STATUS_CHECK(grace_trace_cumulative_f4(GRACE_RAYS_SCENE(a), out, NULL)); }
inline void cumulative_dispatch(const SceneArgs<double4>& a, double* out)
{ GRACE_STATUS_CHECK(grace_trace_cumulative_d4(GRACE_RAYS_SCENE(a), out, NULL)); }
inline void cumulative_dispatch(const SceneArgs<float4>& a, double* out)
{ GRACE_STATUS_CHECK(grace_trace_cumulative_f4_f64(GRACE_RAYS_SCENE(a), out, NULL)); }

inline void hits_dispatch(const SceneArgs<float4>& a, const int* off, int* idx, float* integrals, float* dists)
{ GRACE_STATUS_CHECK(grace_trace_hits_f4(GRACE_RAYS_SCENE(a), off, idx, integrals, dists, NULL)); }
inline void hits_dispatch(const SceneArgs<double4>& a, const int* off, int* idx, double* integrals, double* dists)
{ GRACE_STATUS_CHECK(grace_trace_hits_d4(GRACE_RAYS_SCENE(a), off, idx, integrals, dists, NULL)); }
inline void hits_dispatch(const SceneArgs<float4>& a, const int* off, int* idx, double* integrals, double* dists)
{ GRACE_STATUS_CHECK(grace_trace_hits_f4_f64(GRACE_RAYS_SCENE(a), off, idx, integrals, dists, NULL)); }

// double4 spheres with float outputs: the reference compiles them (fp64 test, fp32 sums); this
// library does not provide that pairing -- a clear refusal instead of an overload-resolution error.
template <typename Real4, typename Real>
struct sph_precision_check
{
    static_assert(!(std::is_same<Real4, double4>::value && std::is_same<Real, float>::value),
                  "grace: double4 spheres with float outputs are not supported; use double outputs "
                  "(or float4 spheres with float or double outputs)");
    static const bool ok = true;
};

// The traversal's status word (one word for every precision): the reference asserts on stack
// exhaustion in GRACE_DEBUG builds (bintree_trace.cuh:164); here it is an error in every build.
inline void check_trace_status() { GRACE_STATUS_CHECK(grace_trace_status(NULL)); }

// Hit counts -> exclusive offsets; returns the total (trace_sph.cuh:126-137), refusing totals
// that int offsets cannot address.  sentinel_slots: one more slot per ray, or none.
inline size_t counts_to_offsets(dvec<int>& d_ray_offsets, size_t sentinel_slots)
{
    long long total = 0;
    GRACE_STATUS_CHECK(grace_scan_exclusive_i32(raw(d_ray_offsets), d_ray_offsets.size(),
                                                raw(d_ray_offsets), &total, NULL));
    if (total + (long long)sentinel_slots > (long long)std::numeric_limits<int>::max())
        too_many_hits(sentinel_slots != 0);
    return size_t(total);
}

template <typename T>
inline void fill_bits(dvec<T>& v, T value)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "32- or 64-bit elements");
    if (sizeof(T) == 4) {
        uint32_t bits;
        __builtin_memcpy(&bits, &value, 4);
        GRACE_STATUS_CHECK(grace_fill_u32(raw(v), v.size(), bits, NULL));
    } else {
        // 64-bit sentinels (double): the container's own fill (container behaviour, not an
        // algorithm on the hot path).
        v.assign(v.size(), value);
    }
}

} // namespace detail

// trace_sph.cuh:58-80
template <typename Real4>
GRACE_HOST void trace_hitcounts_sph(
    const detail::dvec<Ray>& d_rays,
    const detail::dvec<Real4>& d_spheres,
    const Tree& d_tree,
    detail::dvec<int>& d_hit_counts)
{
    detail::check_ray_count(d_rays.size());
    detail::hitcounts_dispatch(detail::scene_args(d_rays, d_spheres, d_tree), detail::raw(d_hit_counts));
    detail::check_trace_status();
}

// trace_sph.cuh:82-110
template <typename Real4, typename Real>
GRACE_HOST void trace_cumulative_sph(
    const detail::dvec<Ray>& d_rays,
    const detail::dvec<Real4>& d_spheres,
    const Tree& d_tree,
    detail::dvec<Real>& d_cumulated)
{
    static_assert(detail::sph_precision_check<Real4, Real>::ok, "");
    detail::check_ray_count(d_rays.size());
    detail::cumulative_dispatch(detail::scene_args(d_rays, d_spheres, d_tree), detail::raw(d_cumulated));
    detail::check_trace_status();
}

// Extension (the reference has no such call): weighted, multi-channel column densities in one
// traversal -- grace_trace_cumulative_weighted_f4 (grace_hip.h).  d_weights holds n_channels
// weights per sphere, sphere-major and in the order of d_spheres (the tree's sorted order);
// d_cumulated[r * n_channels + c] is ray r's sum of fl(w[i][c] I_ri), I_ri being the term
// trace_cumulative_sph adds.  Channels are traced four at a time, each group a walk of its own.
template <typename Real4>
GRACE_HOST void trace_cumulative_weighted_sph(
    const detail::dvec<Ray>& d_rays,
    const detail::dvec<Real4>& d_spheres,
    const Tree& d_tree,
    const detail::dvec<float>& d_weights,
    const int n_channels,
    detail::dvec<float>& d_cumulated)
{
    static_assert(std::is_same<Real4, float4>::value,
                  "trace_cumulative_weighted_sph: float4 spheres only (float weights and sums)");
    detail::check_ray_count(d_rays.size());
    if (n_channels < 1 || n_channels > 64)
        throw std::invalid_argument("trace_cumulative_weighted_sph: n_channels must be 1..64");
    if (d_weights.size() != d_spheres.size() * size_t(n_channels))
        throw std::invalid_argument("trace_cumulative_weighted_sph: d_weights must hold n_channels per sphere");
    if (d_cumulated.size() != d_rays.size() * size_t(n_channels))
        throw std::invalid_argument("trace_cumulative_weighted_sph: d_cumulated must hold n_channels per ray");
    const detail::SceneArgs<Real4> a = detail::scene_args(d_rays, d_spheres, d_tree);
    GRACE_STATUS_CHECK(grace_trace_cumulative_weighted_f4(GRACE_RAYS_SCENE(a), detail::raw(d_weights), n_channels,
                                                          detail::raw(d_cumulated), NULL));
    detail::check_trace_status();
}

// Extension (the reference has no such call): depth-ordered emission-absorption integrals --
// grace_trace_emission_absorption_f4 (grace_hip.h has the contract).  d_emission holds n_channels
// values per sphere, sphere-major, d_absorption one, both in the order of d_spheres (the tree's
// sorted order).  Every ray's hits are ordered by (distance, sphere index); d_out[r * n_channels +
// c] is the fp64 sum of emission I phi(a) exp(-tau) over them, d_tau[r] (if given) the ray's
// optical depth.  The rays are traced in batches that fit set_ordered_budget's bytes.
template <typename Real4>
GRACE_HOST void trace_emission_absorption_sph(
    const detail::dvec<Ray>& d_rays,
    const detail::dvec<Real4>& d_spheres,
    const Tree& d_tree,
    const detail::dvec<float>& d_emission,
    const int n_channels,
    const detail::dvec<float>& d_absorption,
    detail::dvec<float>& d_out,
    detail::dvec<float>* d_tau = NULL)
{
    static_assert(std::is_same<Real4, float4>::value,
                  "trace_emission_absorption_sph: float4 spheres only (float coefficients and outputs)");
    detail::check_ray_count(d_rays.size());
    if (n_channels < 1 || n_channels > 64)
        throw std::invalid_argument("trace_emission_absorption_sph: n_channels must be 1..64");
    if (d_emission.size() != d_spheres.size() * size_t(n_channels))
        throw std::invalid_argument("trace_emission_absorption_sph: d_emission must hold n_channels per sphere");
    if (d_absorption.size() != d_spheres.size())
        throw std::invalid_argument("trace_emission_absorption_sph: d_absorption must hold one value per sphere");
    if (d_out.size() != d_rays.size() * size_t(n_channels))
        throw std::invalid_argument("trace_emission_absorption_sph: d_out must hold n_channels per ray");
    if (d_tau && d_tau->size() != d_rays.size())
        throw std::invalid_argument("trace_emission_absorption_sph: d_tau must hold one value per ray");
    const detail::SceneArgs<Real4> a = detail::scene_args(d_rays, d_spheres, d_tree);
    GRACE_STATUS_CHECK(grace_trace_emission_absorption_f4(
        GRACE_RAYS_SCENE(a), detail::raw(d_emission), n_channels, detail::raw(d_absorption), detail::raw(d_out),
        d_tau ? detail::raw(*d_tau) : NULL, NULL));
    detail::check_trace_status();
}

// Extension (the reference has no such call): absorbed radiation deposited on the particles --
// grace_trace_absorption_deposit_f4 (grace_hip.h has the contract).  d_luminosity holds n_channels
// values per ray, d_absorption n_channels per sphere in the order of d_spheres (the tree's sorted
// order).  d_deposit[i * n_channels + c] is what sphere i absorbs of all rays in channel c (fp64,
// overwritten; summed in 64-bit fixed point, so bit-identical for any order of the rays),
// d_transmitted (if given) what every ray has left, d_quantum (if given) the channels' quanta.
template <typename Real4>
GRACE_HOST void trace_absorption_deposit_sph(
    const detail::dvec<Ray>& d_rays,
    const detail::dvec<Real4>& d_spheres,
    const Tree& d_tree,
    const detail::dvec<float>& d_luminosity,
    const int n_channels,
    const detail::dvec<float>& d_absorption,
    detail::dvec<double>& d_deposit,
    detail::dvec<float>* d_transmitted = NULL,
    detail::dvec<double>* d_quantum = NULL)
{
    static_assert(std::is_same<Real4, float4>::value,
                  "trace_absorption_deposit_sph: float4 spheres only (float coefficients)");
    detail::check_ray_count(d_rays.size());
    if (n_channels < 1 || n_channels > 64)
        throw std::invalid_argument("trace_absorption_deposit_sph: n_channels must be 1..64");
    if (d_luminosity.size() != d_rays.size() * size_t(n_channels))
        throw std::invalid_argument("trace_absorption_deposit_sph: d_luminosity must hold n_channels per ray");
    if (d_absorption.size() != d_spheres.size() * size_t(n_channels))
        throw std::invalid_argument("trace_absorption_deposit_sph: d_absorption must hold n_channels per sphere");
    if (d_deposit.size() != d_spheres.size() * size_t(n_channels))
        throw std::invalid_argument("trace_absorption_deposit_sph: d_deposit must hold n_channels per sphere");
    if (d_transmitted && d_transmitted->size() != d_rays.size() * size_t(n_channels))
        throw std::invalid_argument("trace_absorption_deposit_sph: d_transmitted must hold n_channels per ray");
    if (d_quantum && d_quantum->size() != size_t(n_channels))
        throw std::invalid_argument("trace_absorption_deposit_sph: d_quantum must hold n_channels values");
    const detail::SceneArgs<Real4> a = detail::scene_args(d_rays, d_spheres, d_tree);
    GRACE_STATUS_CHECK(grace_trace_absorption_deposit_f4(
        GRACE_RAYS_SCENE(a), detail::raw(d_luminosity), detail::raw(d_absorption), n_channels,
        detail::raw(d_deposit), d_transmitted ? detail::raw(*d_transmitted) : NULL,
        d_quantum ? detail::raw(*d_quantum) : NULL, NULL));
    detail::check_trace_status();
}

// Extension (the reference has no such call): velocity-space absorption spectra along rays --
// grace_trace_spectra_f4 (grace_hip.h has the contract).  d_amount and d_width hold n_channels
// values per sphere, d_velocity three, in the order of d_spheres (the tree's sorted order).
// d_tau[(r * n_channels + c) * grid.n_bins + j] is the optical depth of ray r in channel c and
// velocity bin j (every hit a Gaussian of Doppler parameter d_width about its line-of-sight
// velocity, integrated over the bins, in fp64 and in a fixed order); d_column (if given) the
// rays' columns per channel.  SpectrumGrid is the C struct: v0, dv, n_bins, periodic, hubble.
typedef grace_spectrum_grid SpectrumGrid;

template <typename Real4>
GRACE_HOST void trace_spectra_sph(
    const detail::dvec<Ray>& d_rays,
    const detail::dvec<Real4>& d_spheres,
    const Tree& d_tree,
    const detail::dvec<float>& d_amount,
    const detail::dvec<float>& d_width,
    const detail::dvec<float>& d_velocity,
    const int n_channels,
    const SpectrumGrid& grid,
    detail::dvec<float>& d_tau,
    detail::dvec<float>* d_column = NULL)
{
    static_assert(std::is_same<Real4, float4>::value,
                  "trace_spectra_sph: float4 spheres only (float coefficients)");
    detail::check_ray_count(d_rays.size());
    if (n_channels < 1 || n_channels > 16)
        throw std::invalid_argument("trace_spectra_sph: n_channels must be 1..16");
    if (grid.n_bins < 1 || grid.n_bins > 4096)
        throw std::invalid_argument("trace_spectra_sph: grid.n_bins must be 1..4096");
    if (d_amount.size() != d_spheres.size() * size_t(n_channels))
        throw std::invalid_argument("trace_spectra_sph: d_amount must hold n_channels per sphere");
    if (d_width.size() != d_spheres.size() * size_t(n_channels))
        throw std::invalid_argument("trace_spectra_sph: d_width must hold n_channels per sphere");
    if (d_velocity.size() != d_spheres.size() * 3)
        throw std::invalid_argument("trace_spectra_sph: d_velocity must hold three values per sphere");
    if (d_tau.size() != d_rays.size() * size_t(n_channels) * size_t(grid.n_bins))
        throw std::invalid_argument("trace_spectra_sph: d_tau must hold n_channels * n_bins per ray");
    if (d_column && d_column->size() != d_rays.size() * size_t(n_channels))
        throw std::invalid_argument("trace_spectra_sph: d_column must hold n_channels per ray");
    const detail::SceneArgs<Real4> a = detail::scene_args(d_rays, d_spheres, d_tree);
    GRACE_STATUS_CHECK(grace_trace_spectra_f4(
        GRACE_RAYS_SCENE(a), detail::raw(d_amount), detail::raw(d_width), detail::raw(d_velocity), n_channels,
        &grid, detail::raw(d_tau), d_column ? detail::raw(*d_column) : NULL, NULL));
    detail::check_trace_status();
}

GRACE_HOST void set_ordered_budget(const size_t bytes)
{
    GRACE_STATUS_CHECK(grace_trace_set_ordered_budget(bytes));
}

// Extension (the reference has no such choice): the SPH kernel of every integrating trace --
// column densities, weighted sums, the per-hit integrals of trace_sph / trace_with_sentinels_sph
// (grace_trace_set_sph_kernel*, grace_hip.h).  A sphere's w is the kernel's support radius H.  A
// per-context knob: the reference-signature calls above and below keep their signatures and use
// the kernel selected when they run.  Default SphKernel::cubic, the reference's table (N_table
// values above).  set_sph_kernel_table takes 51 values (finite, >= 0, the last one 0), else
// std::invalid_argument with the active kernel unchanged; it synchronises the device before it
// overwrites the context's table buffer.  sph_kernel_table gives a built-in kernel's values, for
// instance for an OnHit_sphere_cumulate-style functor of the generic trace.
enum class SphKernel {
    cubic = GRACE_SPH_KERNEL_CUBIC,
    quartic = GRACE_SPH_KERNEL_QUARTIC,
    quintic = GRACE_SPH_KERNEL_QUINTIC,
    wendland_c2 = GRACE_SPH_KERNEL_WENDLAND_C2,
    wendland_c4 = GRACE_SPH_KERNEL_WENDLAND_C4,
    wendland_c6 = GRACE_SPH_KERNEL_WENDLAND_C6
};

GRACE_HOST void set_sph_kernel(const SphKernel kernel)
{
    GRACE_STATUS_CHECK(grace_trace_set_sph_kernel(static_cast<int>(kernel)));
}

GRACE_HOST void set_sph_kernel_table(const std::vector<double>& table)
{
    if (table.size() != size_t(N_table))
        throw std::invalid_argument("set_sph_kernel_table: the table must hold 51 values");
    GRACE_STATUS_CHECK(grace_trace_set_sph_kernel_table(table.data(), int(table.size())));
}

GRACE_HOST std::array<double, N_table> sph_kernel_table(const SphKernel kernel)
{
    std::array<double, N_table> t;
    GRACE_STATUS_CHECK(grace_sph_kernel_table(static_cast<int>(kernel), t.data()));
    return t;
}

// trace_sph.cuh:112-168
template <typename Real4, typename IndexType, typename Real>
GRACE_HOST void trace_sph(
    const detail::dvec<Ray>& d_rays,
    const detail::dvec<Real4>& d_spheres,
    const Tree& d_tree,
    // The segmented scans and sorts require ray offsets to be int.
    detail::dvec<int>& d_ray_offsets,
    detail::dvec<IndexType>& d_hit_indices,
    detail::dvec<Real>& d_hit_integrals,
    detail::dvec<Real>& d_hit_distances)
{
    static_assert(sizeof(IndexType) == sizeof(int), "IndexType must be a 32-bit integer");
    static_assert(detail::sph_precision_check<Real4, Real>::ok, "");
    // Initially, d_ray_offsets is actually per-ray *hit counts*.
    detail::check_ray_count(d_rays.size());
    const detail::SceneArgs<Real4> a = detail::scene_args(d_rays, d_spheres, d_tree);
    detail::hitcounts_keep_dispatch(a, detail::raw(d_ray_offsets), static_cast<const Real*>(NULL));
    const size_t total_hits = detail::counts_to_offsets(d_ray_offsets, 0);

    d_hit_integrals.resize(total_hits);
    d_hit_indices.resize(total_hits);
    d_hit_distances.resize(total_hits);
    if (total_hits == 0) return;   // no ray hits anything: empty vectors

    detail::hits_dispatch(a, detail::raw(d_ray_offsets), reinterpret_cast<int*>(detail::raw(d_hit_indices)),
                          detail::raw(d_hit_integrals), detail::raw(d_hit_distances));
    detail::check_trace_status();
}

// trace_sph.cuh:171-241
template <typename Real4, typename IndexType, typename Real>
GRACE_HOST void trace_with_sentinels_sph(
    const detail::dvec<Ray>& d_rays,
    const detail::dvec<Real4>& d_spheres,
    const Tree& d_tree,
    detail::dvec<int>& d_ray_offsets,
    detail::dvec<IndexType>& d_hit_indices,
    const int index_sentinel,
    detail::dvec<Real>& d_hit_integrals,
    const Real integral_sentinel,
    detail::dvec<Real>& d_hit_distances,
    const Real distance_sentinel)
{
    static_assert(sizeof(IndexType) == sizeof(int), "IndexType must be a 32-bit integer");
    static_assert(detail::sph_precision_check<Real4, Real>::ok, "");
    const size_t n_rays = d_rays.size();
    detail::check_ray_count(n_rays);
    const detail::SceneArgs<Real4> a = detail::scene_args(d_rays, d_spheres, d_tree);
    detail::hitcounts_keep_dispatch(a, detail::raw(d_ray_offsets), static_cast<const Real*>(NULL));
    // Each ray segment in the output arrays ends with a sentinel value marking the end of the
    // ray; increase offsets accordingly (trace_sph.cuh:199-208).
    const size_t allocate_size = detail::counts_to_offsets(d_ray_offsets, n_rays) + n_rays;
    GRACE_STATUS_CHECK(grace_add_iota_i32(detail::raw(d_ray_offsets), n_rays, NULL));

    // Outputs start out as their sentinel values: these slots are not touched by the trace.
    d_hit_indices.resize(allocate_size);
    d_hit_integrals.resize(allocate_size);
    d_hit_distances.resize(allocate_size);
    detail::fill_bits(d_hit_indices, IndexType(index_sentinel));
    detail::fill_bits(d_hit_integrals, integral_sentinel);
    detail::fill_bits(d_hit_distances, distance_sentinel);

    detail::hits_dispatch(a, detail::raw(d_ray_offsets), reinterpret_cast<int*>(detail::raw(d_hit_indices)),
                          detail::raw(d_hit_integrals), detail::raw(d_hit_distances));
    detail::check_trace_status();
}

// ---- extensions (not in the reference) ------------------------------------------------------
// What every trace call derives from its arguments alone -- the scene's pre-pass records, the ray
// coherence order -- is cached by the library for arrays that are traced repeatedly (from the second
// consecutive call on; see "Cached trace records" in grace_hip.h).  prepare_trace_sph /
// prepare_trace_rays fill that cache NOW and pin it for as long as the returned handle lives.
// Cached records are validated against the arrays' current contents before every use, so modifying
// or reallocating d_spheres / d_tree / d_rays while a handle is alive is safe (it costs a
// re-derivation); only grace_trace_set_cache_validation(0) turns that into the caller's promise.
// Results never depend on any of this.
class PreparedTrace
{
public:
    PreparedTrace() : scene_(false), rays_(false) {}
    PreparedTrace(PreparedTrace&& o) : scene_(o.scene_), rays_(o.rays_) { o.scene_ = o.rays_ = false; }
    PreparedTrace& operator=(PreparedTrace&& o)
    {
        if (this != &o) { release(); scene_ = o.scene_; rays_ = o.rays_; o.scene_ = o.rays_ = false; }
        return *this;
    }
    ~PreparedTrace() { release(); }
    // Unpins and frees what this handle pinned (a later prepare_* may already have replaced it).
    void release()
    {
        if (scene_) GRACE_STATUS_CHECK(grace_trace_release());
        if (rays_) GRACE_STATUS_CHECK(grace_trace_release_rays());
        scene_ = rays_ = false;
    }

private:
    PreparedTrace(const PreparedTrace&);
    PreparedTrace& operator=(const PreparedTrace&);
    bool scene_, rays_;
    friend PreparedTrace prepare_trace_sph(const detail::dvec<float4>&, const Tree&);
    friend PreparedTrace prepare_trace_rays(const detail::dvec<Ray>&);
};

__attribute__((warn_unused_result))
GRACE_HOST PreparedTrace prepare_trace_sph(const detail::dvec<float4>& d_spheres, const Tree& d_tree)
{
    const detail::SceneArgs<float4> a = detail::scene_args(d_spheres, d_tree);
    GRACE_STATUS_CHECK(grace_trace_prepare_f4(a.spheres, a.n_spheres, a.nodes, a.n_nodes, a.leaves, NULL));
    PreparedTrace h;
    h.scene_ = true;
    return h;
}

__attribute__((warn_unused_result))
GRACE_HOST PreparedTrace prepare_trace_rays(const detail::dvec<Ray>& d_rays)
{
    GRACE_STATUS_CHECK(grace_trace_prepare_rays(detail::raw(d_rays), d_rays.size(), NULL));
    PreparedTrace h;
    h.rays_ = true;
    return h;
}

// Drops whatever the calling thread's context has cached or pinned.
GRACE_HOST void release_prepared_trace()
{
    GRACE_STATUS_CHECK(grace_trace_release());
    GRACE_STATUS_CHECK(grace_trace_release_rays());
}

} // namespace grace
