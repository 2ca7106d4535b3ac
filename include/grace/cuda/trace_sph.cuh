// grace/cuda/trace_sph.cuh -- the SPH trace API of the reference
// (include/grace/cuda/trace_sph.cuh:22-241) with its template signatures over
// thrust::device_vector; every body dispatches on Real4 / Real to the traversal kernel of
// libgrace_hip.so (csrc/trace.hip), which stands in for trace_texref<RayData>(... functors ...)
// with the functors the reference passes here:
//
//   trace_hitcounts_sph      Intersect_sphere_bool    + OnHit_increment          -> grace_trace_hitcounts_*
//   trace_cumulative_sph     Intersect_sphere_b2dist  + OnHit_sphere_cumulate    -> grace_trace_cumulative_*
//   trace_sph                hit counts, exclusive scan, resize, then
//                            RayEntry_from_array + OnHit_sphere_individual       -> grace_trace_hits_*
//   trace_with_sentinels_sph the same with one sentinel slot per ray
//
// (Real4, Real) is (float4, float), (double4, double) or (float4, double) -- float spheres under the
// fp64 test with double sums and per-hit outputs, the reference's promotions for that pair --;
// (double4, float) is refused at compile time.  IndexType is a 32-bit integer.  Per-ray
// results equal the brute-force loop over all spheres (the reference's own criterion,
// tests/tree_traversal); column densities are the class-ordered fp32 sum documented in
// grace_hip.h (within 1e-6 of the reference's single running sum).  As in the reference the
// number of rays must be a multiple of 32 (bintree_trace.cuh:231-238: std::invalid_argument).
#pragma once

#include "grace/cuda/nodes.h"
#include "grace/detail/raw.h"
#include "grace/ray.h"

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

struct TreeArgs { const int* nodes; size_t n_nodes; const int* leaves; const int* root; };
inline TreeArgs tree_args(const Tree& t)
{
    TreeArgs a = { reinterpret_cast<const int*>(raw(t.nodes)), t.leaves.size() - 1,
                   reinterpret_cast<const int*>(raw(t.leaves)), t.root_index_ptr };
    return a;
}

inline void hitcounts_dispatch(const Ray* r, size_t nr, const float4* s, size_t n, const TreeArgs& t, int* out)
{ GRACE_STATUS_CHECK(grace_trace_hitcounts_f4(r, nr, reinterpret_cast<const float*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, out, NULL)); }
inline void hitcounts_dispatch(const Ray* r, size_t nr, const double4* s, size_t n, const TreeArgs& t, int* out)
{ GRACE_STATUS_CHECK(grace_trace_hitcounts_d4(r, nr, reinterpret_cast<const double*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, out, NULL)); }

// The hit-count pass of trace_sph: the library keeps what the per-hit pass can reuse.
// The last argument names Real: the counts must come from the test the per-hit pass applies.
inline void hitcounts_keep_dispatch(const Ray* r, size_t nr, const float4* s, size_t n, const TreeArgs& t, int* out,
                                    const float*)
{ GRACE_STATUS_CHECK(grace_trace_hitcounts_keep_f4(r, nr, reinterpret_cast<const float*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, out, NULL)); }
inline void hitcounts_keep_dispatch(const Ray* r, size_t nr, const double4* s, size_t n, const TreeArgs& t, int* out,
                                    const double*)
{ hitcounts_dispatch(r, nr, s, n, t, out); }
// (float4, double): the fp64 test in both passes, so offsets and written hits always agree (the
// reference sizes with the float test here)
inline void hitcounts_keep_dispatch(const Ray* r, size_t nr, const float4* s, size_t n, const TreeArgs& t, int* out,
                                    const double*)
{ GRACE_STATUS_CHECK(grace_trace_hitcounts_f4_f64(r, nr, reinterpret_cast<const float*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, out, NULL)); }

inline void cumulative_dispatch(const Ray* r, size_t nr, const float4* s, size_t n, const TreeArgs& t, float* out)
{ GRACE_STATUS_CHECK(grace_trace_cumulative_f4(r, nr, reinterpret_cast<const float*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, out, NULL)); }
inline void cumulative_dispatch(const Ray* r, size_t nr, const double4* s, size_t n, const TreeArgs& t, double* out)
{ GRACE_STATUS_CHECK(grace_trace_cumulative_d4(r, nr, reinterpret_cast<const double*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, out, NULL)); }
inline void cumulative_dispatch(const Ray* r, size_t nr, const float4* s, size_t n, const TreeArgs& t, double* out)
{ GRACE_STATUS_CHECK(grace_trace_cumulative_f4_f64(r, nr, reinterpret_cast<const float*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, out, NULL)); }

inline void hits_dispatch(const Ray* r, size_t nr, const float4* s, size_t n, const TreeArgs& t,
                          const int* off, int* idx, float* integrals, float* dists)
{ GRACE_STATUS_CHECK(grace_trace_hits_f4(r, nr, reinterpret_cast<const float*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, off, idx, integrals, dists, NULL)); }
inline void hits_dispatch(const Ray* r, size_t nr, const double4* s, size_t n, const TreeArgs& t,
                          const int* off, int* idx, double* integrals, double* dists)
{ GRACE_STATUS_CHECK(grace_trace_hits_d4(r, nr, reinterpret_cast<const double*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, off, idx, integrals, dists, NULL)); }
inline void hits_dispatch(const Ray* r, size_t nr, const float4* s, size_t n, const TreeArgs& t,
                          const int* off, int* idx, double* integrals, double* dists)
{ GRACE_STATUS_CHECK(grace_trace_hits_f4_f64(r, nr, reinterpret_cast<const float*>(s), n, t.nodes, t.n_nodes, t.leaves, t.root, off, idx, integrals, dists, NULL)); }

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

// The traversal's status word: the reference asserts on stack exhaustion in GRACE_DEBUG builds
// (bintree_trace.cuh:164); here it is an error in every build.
inline void check_trace_status() { GRACE_STATUS_CHECK(grace_trace_status(NULL)); }

// Hit counts -> exclusive offsets; returns the total (trace_sph.cuh:126-137), refusing totals
// that int offsets cannot address.
inline size_t counts_to_offsets(thrust::device_vector<int>& d_ray_offsets, size_t extra)
{
    long long total = 0;
    GRACE_STATUS_CHECK(grace_scan_exclusive_i32(raw(d_ray_offsets), d_ray_offsets.size(),
                                                raw(d_ray_offsets), &total, NULL));
    if (total + (long long)extra > (long long)std::numeric_limits<int>::max())
        throw std::invalid_argument("trace_sph: more than INT_MAX hits; the int ray offsets cannot "
                                    "address the per-hit arrays. Trace fewer rays per call.");
    return size_t(total);
}

template <typename T>
inline void fill_bits(thrust::device_vector<T>& v, T value)
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

template <typename Real4>
GRACE_HOST void trace_hitcounts_sph(
    const thrust::device_vector<Ray>& d_rays,
    const thrust::device_vector<Real4>& d_spheres,
    const Tree& d_tree,
    thrust::device_vector<int>& d_hit_counts)
{
    detail::check_ray_count(d_rays.size());
    detail::hitcounts_dispatch(detail::raw(d_rays), d_rays.size(), detail::raw(d_spheres),
                               d_spheres.size(), detail::tree_args(d_tree), detail::raw(d_hit_counts));
    detail::check_trace_status();
}

template <typename Real4, typename Real>
GRACE_HOST void trace_cumulative_sph(
    const thrust::device_vector<Ray>& d_rays,
    const thrust::device_vector<Real4>& d_spheres,
    const Tree& d_tree,
    thrust::device_vector<Real>& d_cumulated)
{
    static_assert(detail::sph_precision_check<Real4, Real>::ok, "");
    detail::check_ray_count(d_rays.size());
    detail::cumulative_dispatch(detail::raw(d_rays), d_rays.size(), detail::raw(d_spheres),
                                d_spheres.size(), detail::tree_args(d_tree), detail::raw(d_cumulated));
    detail::check_trace_status();
}

// Extension (the reference has no such call): weighted, multi-channel column densities in one
// traversal -- grace_trace_cumulative_weighted_f4 (grace_hip.h).  d_weights holds n_channels
// weights per sphere, sphere-major and in the order of d_spheres (the tree's sorted order);
// d_cumulated[r * n_channels + c] is ray r's sum of fl(w[i][c] I_ri), I_ri being the term
// trace_cumulative_sph adds.  Channels are traced four at a time, each group a walk of its own.
template <typename Real4>
GRACE_HOST void trace_cumulative_weighted_sph(
    const thrust::device_vector<Ray>& d_rays,
    const thrust::device_vector<Real4>& d_spheres,
    const Tree& d_tree,
    const thrust::device_vector<float>& d_weights,
    const int n_channels,
    thrust::device_vector<float>& d_cumulated)
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
    const detail::TreeArgs t = detail::tree_args(d_tree);
    GRACE_STATUS_CHECK(grace_trace_cumulative_weighted_f4(
        detail::raw(d_rays), d_rays.size(), reinterpret_cast<const float*>(detail::raw(d_spheres)),
        d_spheres.size(), t.nodes, t.n_nodes, t.leaves, t.root, detail::raw(d_weights), n_channels,
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
    const thrust::device_vector<Ray>& d_rays,
    const thrust::device_vector<Real4>& d_spheres,
    const Tree& d_tree,
    const thrust::device_vector<float>& d_emission,
    const int n_channels,
    const thrust::device_vector<float>& d_absorption,
    thrust::device_vector<float>& d_out,
    thrust::device_vector<float>* d_tau = NULL)
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
    const detail::TreeArgs t = detail::tree_args(d_tree);
    GRACE_STATUS_CHECK(grace_trace_emission_absorption_f4(
        detail::raw(d_rays), d_rays.size(), reinterpret_cast<const float*>(detail::raw(d_spheres)),
        d_spheres.size(), t.nodes, t.n_nodes, t.leaves, t.root, detail::raw(d_emission), n_channels,
        detail::raw(d_absorption), detail::raw(d_out), d_tau ? detail::raw(*d_tau) : NULL, NULL));
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
    const thrust::device_vector<Ray>& d_rays,
    const thrust::device_vector<Real4>& d_spheres,
    const Tree& d_tree,
    const thrust::device_vector<float>& d_luminosity,
    const int n_channels,
    const thrust::device_vector<float>& d_absorption,
    thrust::device_vector<double>& d_deposit,
    thrust::device_vector<float>* d_transmitted = NULL,
    thrust::device_vector<double>* d_quantum = NULL)
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
    const detail::TreeArgs t = detail::tree_args(d_tree);
    GRACE_STATUS_CHECK(grace_trace_absorption_deposit_f4(
        detail::raw(d_rays), d_rays.size(), reinterpret_cast<const float*>(detail::raw(d_spheres)),
        d_spheres.size(), t.nodes, t.n_nodes, t.leaves, t.root, detail::raw(d_luminosity),
        detail::raw(d_absorption), n_channels, detail::raw(d_deposit),
        d_transmitted ? detail::raw(*d_transmitted) : NULL, d_quantum ? detail::raw(*d_quantum) : NULL, NULL));
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
    const thrust::device_vector<Ray>& d_rays,
    const thrust::device_vector<Real4>& d_spheres,
    const Tree& d_tree,
    const thrust::device_vector<float>& d_amount,
    const thrust::device_vector<float>& d_width,
    const thrust::device_vector<float>& d_velocity,
    const int n_channels,
    const SpectrumGrid& grid,
    thrust::device_vector<float>& d_tau,
    thrust::device_vector<float>* d_column = NULL)
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
    const detail::TreeArgs t = detail::tree_args(d_tree);
    GRACE_STATUS_CHECK(grace_trace_spectra_f4(
        detail::raw(d_rays), d_rays.size(), reinterpret_cast<const float*>(detail::raw(d_spheres)),
        d_spheres.size(), t.nodes, t.n_nodes, t.leaves, t.root, detail::raw(d_amount),
        detail::raw(d_width), detail::raw(d_velocity), n_channels, &grid, detail::raw(d_tau),
        d_column ? detail::raw(*d_column) : NULL, NULL));
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

template <typename Real4, typename IndexType, typename Real>
GRACE_HOST void trace_sph(
    const thrust::device_vector<Ray>& d_rays,
    const thrust::device_vector<Real4>& d_spheres,
    const Tree& d_tree,
    // The segmented scans and sorts require ray offsets to be int.
    thrust::device_vector<int>& d_ray_offsets,
    thrust::device_vector<IndexType>& d_hit_indices,
    thrust::device_vector<Real>& d_hit_integrals,
    thrust::device_vector<Real>& d_hit_distances)
{
    static_assert(sizeof(IndexType) == sizeof(int), "IndexType must be a 32-bit integer");
    static_assert(detail::sph_precision_check<Real4, Real>::ok, "");
    // Initially, d_ray_offsets is actually per-ray *hit counts*.
    detail::check_ray_count(d_rays.size());
    detail::hitcounts_keep_dispatch(detail::raw(d_rays), d_rays.size(), detail::raw(d_spheres),
                                    d_spheres.size(), detail::tree_args(d_tree), detail::raw(d_ray_offsets),
                                    static_cast<const Real*>(NULL));
    const size_t total_hits = detail::counts_to_offsets(d_ray_offsets, 0);

    d_hit_integrals.resize(total_hits);
    d_hit_indices.resize(total_hits);
    d_hit_distances.resize(total_hits);
    if (total_hits == 0) return;

    detail::hits_dispatch(detail::raw(d_rays), d_rays.size(), detail::raw(d_spheres),
                          d_spheres.size(), detail::tree_args(d_tree), detail::raw(d_ray_offsets),
                          reinterpret_cast<int*>(detail::raw(d_hit_indices)),
                          detail::raw(d_hit_integrals), detail::raw(d_hit_distances));
    detail::check_trace_status();
}

template <typename Real4, typename IndexType, typename Real>
GRACE_HOST void trace_with_sentinels_sph(
    const thrust::device_vector<Ray>& d_rays,
    const thrust::device_vector<Real4>& d_spheres,
    const Tree& d_tree,
    thrust::device_vector<int>& d_ray_offsets,
    thrust::device_vector<IndexType>& d_hit_indices,
    const int index_sentinel,
    thrust::device_vector<Real>& d_hit_integrals,
    const Real integral_sentinel,
    thrust::device_vector<Real>& d_hit_distances,
    const Real distance_sentinel)
{
    static_assert(sizeof(IndexType) == sizeof(int), "IndexType must be a 32-bit integer");
    static_assert(detail::sph_precision_check<Real4, Real>::ok, "");
    const size_t n_rays = d_rays.size();
    detail::check_ray_count(n_rays);
    detail::hitcounts_keep_dispatch(detail::raw(d_rays), n_rays, detail::raw(d_spheres),
                                    d_spheres.size(), detail::tree_args(d_tree), detail::raw(d_ray_offsets),
                                    static_cast<const Real*>(NULL));
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

    detail::hits_dispatch(detail::raw(d_rays), n_rays, detail::raw(d_spheres), d_spheres.size(),
                          detail::tree_args(d_tree), detail::raw(d_ray_offsets),
                          reinterpret_cast<int*>(detail::raw(d_hit_indices)),
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
    friend PreparedTrace prepare_trace_sph(const thrust::device_vector<float4>&, const Tree&);
    friend PreparedTrace prepare_trace_rays(const thrust::device_vector<Ray>&);
};

__attribute__((warn_unused_result))
GRACE_HOST PreparedTrace prepare_trace_sph(const thrust::device_vector<float4>& d_spheres, const Tree& d_tree)
{
    const detail::TreeArgs t = detail::tree_args(d_tree);
    GRACE_STATUS_CHECK(grace_trace_prepare_f4(reinterpret_cast<const float*>(detail::raw(d_spheres)),
                                              d_spheres.size(), t.nodes, t.n_nodes, t.leaves, NULL));
    PreparedTrace h;
    h.scene_ = true;
    return h;
}

__attribute__((warn_unused_result))
GRACE_HOST PreparedTrace prepare_trace_rays(const thrust::device_vector<Ray>& d_rays)
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
