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
//
// d_spheres is the caller's array and is not modified; d_weights holds n_channels per CALLER sphere, in
// the order of d_spheres as passed (an image carries the weight row of its source).  float4 spheres
// only.  A sphere outside the box or with H above half a period, and a ray of more than 65536
// segments, throw std::invalid_argument (the status word); more than INT32_MAX images or segments
// std::length_error, before any fill.  Not provided: the ordered traces (emission-absorption,
// deposits, spectra), per-hit outputs, double4 spheres, H > L / 2.
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

} // namespace grace
