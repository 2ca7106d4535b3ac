// grace/detail/periodic_trace.h -- the one definition of the periodic traces, an extension the
// reference lacks, shared by the drop-in grace/cuda/periodic_trace.cuh and the HIP-free mirror
// grace/grace.h (grace/detail/front_end.h).  The periodic trace is DEFINED as the open trace of the
// rays' segments over the spheres' images, folded back per ray (grace_hip.h, "Periodic boxes for
// traces", states both sets and the fold); everything here composes the grace_periodic_* entry points
// with the unchanged open traces.
//
//   PeriodicScene scene;
//   periodic_scene_sph(d_spheres, domain, max_per_leaf, scene);   // images, their sources, their tree
//   trace_hitcounts_sph(d_rays, scene, d_hit_counts);             // any number of rays
//   trace_cumulative_sph(d_rays, scene, d_cumulated);
//   trace_cumulative_weighted_sph(d_rays, scene, d_weights, n_channels, d_cumulated);
//   trace_emission_absorption_sph(d_rays, scene, d_emission, n_channels, d_absorption, d_out, &d_tau);
//   trace_absorption_deposit_sph(d_rays, scene, d_luminosity, n_channels, d_absorption, d_deposit);
//   trace_spectra_sph(d_rays, scene, d_amount, d_width, d_velocity, n_channels, grid, d_tau);
//
// d_spheres is the caller's array and is not modified; d_weights holds n_channels per CALLER sphere, in
// the order of d_spheres as passed (an image carries the weight row of its source).  float4 spheres
// only.  A sphere outside the box or with H above half a period, and a ray of more than 65536
// segments, throw std::invalid_argument (the status word); more than INT32_MAX images or segments
// std::length_error, before any fill.
// The three ordered traces are no fold of per-segment results: they are the open call's composite
// applied per ray to the hits of ALL the ray's segments, ordered by (segment along the ray, fp32
// distance within the segment, image index), every hit standing for its source (grace_hip.h, "Ordered
// traces").  Their per-particle arrays -- and the deposit -- hold one row per CALLER sphere
// (scene.n_sources), in the order of d_spheres as passed.
// Not provided: per-hit outputs, double4 spheres, H > L / 2.
#pragma once

#include "grace/detail/build_sph.h"
#include "grace/detail/periodic_box.h"
#include "grace/detail/trace_sph.h"

#include <limits>
#include <memory>
#include <stdexcept>

namespace grace {

struct PeriodicScene
{
    detail::dvec<float4> spheres;    // the images, in tree order
    detail::dvec<int> source;        // per image: the index of its sphere in the caller's array
    std::unique_ptr<Tree> tree;      // over `spheres`
    PeriodicDomain domain;
    size_t n_sources = 0;            // spheres in the caller's array
};

namespace detail {

struct DomainArrays
{
    float lo[3], period[3];
    explicit DomainArrays(const PeriodicDomain& d)
    {
        lo[0] = d.ox; lo[1] = d.oy; lo[2] = d.oz;
        period[0] = d.period.lx; period[1] = d.period.ly; period[2] = d.period.lz;
    }
};

// Counts in the first n of n + 1 entries -> offsets; returns the total.
inline size_t periodic_offsets(dvec<int>& d_offsets, const char* too_many)
{
    long long total = 0;
    GRACE_STATUS_CHECK(grace_scan_exclusive_i32(raw(d_offsets), d_offsets.size(), raw(d_offsets), &total, NULL));
    if (total > (long long)std::numeric_limits<int>::max()) throw std::length_error(too_many);
    return size_t(total);
}

// The rays' segments (grace_periodic_segment_counts, the library's scan, grace_periodic_segments):
// the C ABI, which takes any number of rays.
inline void periodic_segments(const dvec<Ray>& d_rays, const PeriodicDomain& domain, dvec<Ray>& d_segments,
                              dvec<int>& d_offsets)
{
    const DomainArrays box(domain);
    const size_t n = d_rays.size();
    d_offsets.assign(n + 1, 0);
    GRACE_STATUS_CHECK(grace_periodic_segment_counts(raw(d_rays), n, box.lo, box.period, raw(d_offsets), NULL));
    const size_t total = n ? periodic_offsets(d_offsets, "periodic trace: more than INT32_MAX ray segments; "
                                                         "trace fewer rays per call.") : 0;
    d_segments.resize(total);
    if (total)
        GRACE_STATUS_CHECK(grace_periodic_segments(raw(d_rays), n, box.lo, box.period, raw(d_offsets),
                                                   raw(d_segments), NULL));
}

// ... and their starting parameters along their rays (grace_periodic_segment_starts).
inline void periodic_segment_starts(const dvec<Ray>& d_rays, const PeriodicDomain& domain, const dvec<int>& d_offsets,
                                    const size_t n_segments, dvec<double>& d_t0)
{
    const DomainArrays box(domain);
    d_t0.resize(n_segments);
    if (n_segments)
        GRACE_STATUS_CHECK(grace_periodic_segment_starts(raw(d_rays), d_rays.size(), box.lo, box.period, raw(d_offsets),
                                                         raw(d_t0), NULL));
}

// What every periodic ordered entry point takes between the scene and the open call's own arguments.
#define GRACE_PERIODIC_GROUPS(d_offsets, n_rays, scene) \
    detail::raw(d_offsets), (n_rays), detail::raw((scene).source), (scene).n_sources

inline const SceneArgs<float4> periodic_scene_args(const dvec<Ray>& d_segments, const PeriodicScene& scene)
{
    if (!scene.tree) throw std::invalid_argument("periodic trace: the scene is empty (periodic_scene_sph first)");
    return scene_args(d_segments, scene.spheres, *scene.tree);
}

} // namespace detail

// The images of d_spheres in the box, their source indices and their tree (the steps of the tests'
// build_tree: 30-bit keys inside the images' own bounds, a stable sort -- the sources follow as a
// payload of their own under a copy of the keys --, Euclidean deltas, ALBVH).
GRACE_HOST void periodic_scene_sph(const detail::dvec<float4>& d_spheres, const PeriodicDomain& domain,
                                   const int max_per_leaf, PeriodicScene& scene)
{
    const detail::DomainArrays box(domain);
    const size_t n = d_spheres.size();
    if (n == 0) throw std::invalid_argument("periodic_scene_sph: no spheres");
    detail::dvec<int> d_offsets;
    d_offsets.assign(n + 1, 0);
    GRACE_STATUS_CHECK(grace_periodic_image_counts_f4(reinterpret_cast<const float*>(detail::raw(d_spheres)), n, box.lo,
                                                      box.period, detail::raw(d_offsets), NULL));
    const size_t total = detail::periodic_offsets(d_offsets, "periodic_scene_sph: more than INT32_MAX sphere images");
    scene.domain = domain;
    scene.n_sources = n;
    scene.spheres.resize(total);
    scene.source.resize(total);
    GRACE_STATUS_CHECK(grace_periodic_images_f4(reinterpret_cast<const float*>(detail::raw(d_spheres)), n, box.lo,
                                                box.period, detail::raw(d_offsets),
                                                reinterpret_cast<float*>(detail::raw(scene.spheres)),
                                                detail::raw(scene.source), NULL));
    detail::check_trace_status();
    detail::dvec<uinteger32> d_keys, d_source_keys;
    d_keys.resize(total);
    d_source_keys.resize(total);
    morton_keys_sph(scene.spheres, d_keys);
    GRACE_STATUS_CHECK(grace_memcpy_dtod(detail::raw(d_source_keys), detail::raw(d_keys), total * sizeof(uinteger32), NULL));
    GRACE_STATUS_CHECK(grace_sort_pairs_u32(detail::raw(d_source_keys), detail::raw(scene.source), total,
                                            int(sizeof(int)), 0, 30, NULL, NULL));
    detail::sort_spheres(d_keys, scene.spheres, 30);
    detail::dvec<float> d_deltas;
    d_deltas.resize(total + 1);
    scene.tree.reset(new Tree(total, max_per_leaf));
    euclidean_deltas_sph(scene.spheres, d_deltas);
    ALBVH_sph(scene.spheres, d_deltas, *scene.tree);
}

// d_hit_counts[r] = the number of lattice images of the scene's spheres that ray r hits: the sum of
// the open hit counts of its segments.  Any number of rays.
GRACE_HOST void trace_hitcounts_sph(const detail::dvec<Ray>& d_rays, const PeriodicScene& scene,
                                    detail::dvec<int>& d_hit_counts)
{
    if (d_hit_counts.size() != d_rays.size())
        throw std::invalid_argument("trace_hitcounts_sph (periodic): d_hit_counts must hold one count per ray");
    if (d_rays.size() == 0) return;
    detail::dvec<Ray> d_segments;
    detail::dvec<int> d_offsets, d_per_segment;
    detail::periodic_segments(d_rays, scene.domain, d_segments, d_offsets);
    d_per_segment.resize(d_segments.size());
    detail::hitcounts_dispatch(detail::periodic_scene_args(d_segments, scene), detail::raw(d_per_segment));
    GRACE_STATUS_CHECK(grace_periodic_fold_i32(detail::raw(d_per_segment), detail::raw(d_offsets), d_rays.size(), 1,
                                               detail::raw(d_hit_counts), NULL));
    detail::check_trace_status();
}

// d_cumulated[r] = the fp32 running sum, from 0 and in order along the ray, of the open column
// densities of ray r's segments.
GRACE_HOST void trace_cumulative_sph(const detail::dvec<Ray>& d_rays, const PeriodicScene& scene,
                                     detail::dvec<float>& d_cumulated)
{
    if (d_cumulated.size() != d_rays.size())
        throw std::invalid_argument("trace_cumulative_sph (periodic): d_cumulated must hold one value per ray");
    if (d_rays.size() == 0) return;
    detail::dvec<Ray> d_segments;
    detail::dvec<int> d_offsets;
    detail::dvec<float> d_per_segment;
    detail::periodic_segments(d_rays, scene.domain, d_segments, d_offsets);
    d_per_segment.resize(d_segments.size());
    detail::cumulative_dispatch(detail::periodic_scene_args(d_segments, scene), detail::raw(d_per_segment));
    GRACE_STATUS_CHECK(grace_periodic_fold_f32(detail::raw(d_per_segment), detail::raw(d_offsets), d_rays.size(), 1,
                                               detail::raw(d_cumulated), NULL));
    detail::check_trace_status();
}

// ... weighted: d_weights holds n_channels per caller sphere, d_cumulated n_channels per ray.
GRACE_HOST void trace_cumulative_weighted_sph(const detail::dvec<Ray>& d_rays, const PeriodicScene& scene,
                                              const detail::dvec<float>& d_weights, const int n_channels,
                                              detail::dvec<float>& d_cumulated)
{
    if (n_channels < 1 || n_channels > 64)
        throw std::invalid_argument("trace_cumulative_weighted_sph (periodic): n_channels must be 1..64");
    if (d_weights.size() % size_t(n_channels) != 0 || d_weights.size() == 0)
        throw std::invalid_argument("trace_cumulative_weighted_sph (periodic): d_weights must hold n_channels per sphere");
    if (d_cumulated.size() != d_rays.size() * size_t(n_channels))
        throw std::invalid_argument("trace_cumulative_weighted_sph (periodic): d_cumulated must hold n_channels per ray");
    if (d_rays.size() == 0) return;
    detail::dvec<Ray> d_segments;
    detail::dvec<int> d_offsets;
    detail::dvec<float> d_per_segment, d_image_weights;
    detail::periodic_segments(d_rays, scene.domain, d_segments, d_offsets);
    const detail::SceneArgs<float4> a = detail::periodic_scene_args(d_segments, scene);
    d_image_weights.resize(scene.spheres.size() * size_t(n_channels));
    GRACE_STATUS_CHECK(grace_periodic_gather_rows_f32(detail::raw(d_weights), detail::raw(scene.source),
                                                      scene.spheres.size(), n_channels,
                                                      detail::raw(d_image_weights), NULL));
    d_per_segment.resize(d_segments.size() * size_t(n_channels));
    GRACE_STATUS_CHECK(grace_trace_cumulative_weighted_f4(GRACE_RAYS_SCENE(a), detail::raw(d_image_weights), n_channels,
                                                          detail::raw(d_per_segment), NULL));
    GRACE_STATUS_CHECK(grace_periodic_fold_f32(detail::raw(d_per_segment), detail::raw(d_offsets), d_rays.size(),
                                               n_channels, detail::raw(d_cumulated), NULL));
    detail::check_trace_status();
}

// trace_emission_absorption_sph in a periodic box.  d_emission holds n_channels per CALLER sphere,
// d_absorption one value; d_out n_channels per ray, d_tau (if given) one.  Any number of rays.
GRACE_HOST void trace_emission_absorption_sph(const detail::dvec<Ray>& d_rays, const PeriodicScene& scene,
                                              const detail::dvec<float>& d_emission, const int n_channels,
                                              const detail::dvec<float>& d_absorption, detail::dvec<float>& d_out,
                                              detail::dvec<float>* d_tau = NULL)
{
    if (n_channels < 1 || n_channels > 64)
        throw std::invalid_argument("trace_emission_absorption_sph (periodic): n_channels must be 1..64");
    if (d_emission.size() != scene.n_sources * size_t(n_channels) || d_absorption.size() != scene.n_sources)
        throw std::invalid_argument("trace_emission_absorption_sph (periodic): d_emission must hold n_channels, "
                                    "d_absorption one value per sphere given to periodic_scene_sph");
    if (d_out.size() != d_rays.size() * size_t(n_channels) || (d_tau && d_tau->size() != d_rays.size()))
        throw std::invalid_argument("trace_emission_absorption_sph (periodic): d_out must hold n_channels, d_tau one "
                                    "value per ray");
    if (d_rays.size() == 0) return;
    detail::dvec<Ray> d_segments;
    detail::dvec<int> d_offsets;
    detail::periodic_segments(d_rays, scene.domain, d_segments, d_offsets);
    const detail::SceneArgs<float4> a = detail::periodic_scene_args(d_segments, scene);
    GRACE_STATUS_CHECK(grace_trace_emission_absorption_periodic_f4(
        GRACE_RAYS_SCENE(a), GRACE_PERIODIC_GROUPS(d_offsets, d_rays.size(), scene), detail::raw(d_emission),
        n_channels, detail::raw(d_absorption), detail::raw(d_out), d_tau ? detail::raw(*d_tau) : NULL, NULL));
    detail::check_trace_status();
}

// trace_absorption_deposit_sph in a periodic box.  d_luminosity holds n_channels per ray; d_absorption and
// d_deposit n_channels per CALLER sphere: a particle receives what all its images absorb in its one row.
GRACE_HOST void trace_absorption_deposit_sph(const detail::dvec<Ray>& d_rays, const PeriodicScene& scene,
                                             const detail::dvec<float>& d_luminosity, const int n_channels,
                                             const detail::dvec<float>& d_absorption, detail::dvec<double>& d_deposit,
                                             detail::dvec<float>* d_transmitted = NULL,
                                             detail::dvec<double>* d_quantum = NULL)
{
    if (n_channels < 1 || n_channels > 64)
        throw std::invalid_argument("trace_absorption_deposit_sph (periodic): n_channels must be 1..64");
    if (d_luminosity.size() != d_rays.size() * size_t(n_channels)
        || (d_transmitted && d_transmitted->size() != d_rays.size() * size_t(n_channels)))
        throw std::invalid_argument("trace_absorption_deposit_sph (periodic): d_luminosity and d_transmitted must "
                                    "hold n_channels per ray");
    if (d_absorption.size() != scene.n_sources * size_t(n_channels) || d_deposit.size() != d_absorption.size())
        throw std::invalid_argument("trace_absorption_deposit_sph (periodic): d_absorption and d_deposit must hold "
                                    "n_channels per sphere given to periodic_scene_sph");
    if (d_quantum && d_quantum->size() != size_t(n_channels))
        throw std::invalid_argument("trace_absorption_deposit_sph (periodic): d_quantum must hold n_channels values");
    detail::dvec<Ray> d_segments;
    detail::dvec<int> d_offsets;
    if (d_rays.size()) detail::periodic_segments(d_rays, scene.domain, d_segments, d_offsets);
    const detail::SceneArgs<float4> a = detail::periodic_scene_args(d_segments, scene);
    GRACE_STATUS_CHECK(grace_trace_absorption_deposit_periodic_f4(
        GRACE_RAYS_SCENE(a), GRACE_PERIODIC_GROUPS(d_offsets, d_rays.size(), scene), detail::raw(d_luminosity),
        detail::raw(d_absorption), n_channels, detail::raw(d_deposit),
        d_transmitted ? detail::raw(*d_transmitted) : NULL, d_quantum ? detail::raw(*d_quantum) : NULL, NULL));
    detail::check_trace_status();
}

// trace_spectra_sph in a periodic box: a sightline may start anywhere and be as long as wanted; a hit's
// distance from the ray's origin is its segment's starting parameter plus its distance within the
// segment, in fp64.  d_amount and d_width hold n_channels per CALLER sphere, d_velocity three.
GRACE_HOST void trace_spectra_sph(const detail::dvec<Ray>& d_rays, const PeriodicScene& scene,
                                  const detail::dvec<float>& d_amount, const detail::dvec<float>& d_width,
                                  const detail::dvec<float>& d_velocity, const int n_channels,
                                  const SpectrumGrid& grid, detail::dvec<float>& d_tau,
                                  detail::dvec<float>* d_column = NULL)
{
    if (n_channels < 1 || n_channels > 16)
        throw std::invalid_argument("trace_spectra_sph (periodic): n_channels must be 1..16");
    if (grid.n_bins < 1 || grid.n_bins > 4096)
        throw std::invalid_argument("trace_spectra_sph (periodic): grid.n_bins must be 1..4096");
    if (d_amount.size() != scene.n_sources * size_t(n_channels) || d_width.size() != d_amount.size()
        || d_velocity.size() != scene.n_sources * 3)
        throw std::invalid_argument("trace_spectra_sph (periodic): d_amount and d_width must hold n_channels, "
                                    "d_velocity three values per sphere given to periodic_scene_sph");
    if (d_tau.size() != d_rays.size() * size_t(n_channels) * size_t(grid.n_bins)
        || (d_column && d_column->size() != d_rays.size() * size_t(n_channels)))
        throw std::invalid_argument("trace_spectra_sph (periodic): d_tau must hold n_channels * n_bins, d_column "
                                    "n_channels per ray");
    if (d_rays.size() == 0) return;
    detail::dvec<Ray> d_segments;
    detail::dvec<int> d_offsets;
    detail::dvec<double> d_t0;
    detail::periodic_segments(d_rays, scene.domain, d_segments, d_offsets);
    detail::periodic_segment_starts(d_rays, scene.domain, d_offsets, d_segments.size(), d_t0);
    const detail::SceneArgs<float4> a = detail::periodic_scene_args(d_segments, scene);
    GRACE_STATUS_CHECK(grace_trace_spectra_periodic_f4(
        GRACE_RAYS_SCENE(a), GRACE_PERIODIC_GROUPS(d_offsets, d_rays.size(), scene), detail::raw(d_t0),
        detail::raw(d_amount), detail::raw(d_width), detail::raw(d_velocity), n_channels, &grid, detail::raw(d_tau),
        d_column ? detail::raw(*d_column) : NULL, NULL));
    detail::check_trace_status();
}

} // namespace grace
