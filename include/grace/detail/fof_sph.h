// grace/detail/fof_sph.h -- the one definition of the friends-of-friends front end, an extension the
// reference lacks, shared by the drop-in grace/cuda/fof_sph.cuh and the HIP-free mirror
// grace/grace.h (grace/detail/front_end.h): the connected components of the graph that links sphere
// centres within one linking length, as labels (the smallest tree index of each group), and the
// catalogue built from them -- grace_fof_labels_f4 / grace_fof_groups / grace_fof_members
// (grace_hip.h states the fp32 distance, the inclusive test d2 <= fl(b b), the labels and the
// catalogue's order).  Spheres in tree order; their w is ignored.  float4 spheres only.  A stack
// overflow is reported as by the traces.  fof_labels_sph has an overload with a trailing
// grace::PeriodicBox (grace/detail/periodic_box.h): the separation wraps once per component, so a
// group that straddles a face of the box is one group (grace_fof_labels_periodic_f4); a linking
// length above half a period is refused.  Not provided: per-particle linking lengths, double4
// spheres, more than INT32_MAX spheres, unbinding or sub-halo finding, groups ordered by size (one
// argsort of d_sizes by the caller).
#pragma once

#include "grace/detail/periodic_box.h"
#include "grace/detail/trace_sph.h"

namespace grace {

// d_labels[i] = the smallest tree index in sphere i's group, for the linking length b; d_labels is
// resized to the number of spheres.
template <typename Real4>
GRACE_HOST void fof_labels_sph(const detail::dvec<Real4>& d_spheres, const Tree& d_tree, const float linking_length,
                               detail::dvec<int>& d_labels)
{
    static_assert(std::is_same<Real4, float4>::value, "friends-of-friends: float4 spheres only (float distances)");
    d_labels.resize(d_spheres.size());
    const detail::SceneArgs<Real4> a = detail::scene_args(d_spheres, d_tree);
    GRACE_STATUS_CHECK(grace_fof_labels_f4(GRACE_SCENE(a), linking_length, detail::raw(d_labels), NULL));
    detail::check_trace_status();
}

// ... in a periodic box.
template <typename Real4>
GRACE_HOST void fof_labels_sph(const detail::dvec<Real4>& d_spheres, const Tree& d_tree, const float linking_length,
                               detail::dvec<int>& d_labels, const PeriodicBox& box)
{
    static_assert(std::is_same<Real4, float4>::value, "friends-of-friends: float4 spheres only (float distances)");
    d_labels.resize(d_spheres.size());
    const detail::SceneArgs<Real4> a = detail::scene_args(d_spheres, d_tree);
    const float period[3] = { box.lx, box.ly, box.lz };
    GRACE_STATUS_CHECK(grace_fof_labels_periodic_f4(GRACE_SCENE(a), linking_length, detail::raw(d_labels), period,
                                                    NULL));
    detail::check_trace_status();
}

// The catalogue of d_labels: groups of at least min_members members, numbered in ascending label.
// d_group_of[i]: sphere i's group or -1; d_sizes[g]: its member count; row g of the CSR lists
// [d_offsets[g], d_offsets[g + 1]) of d_members: its members in ascending tree index.  The four
// outputs are resized (d_sizes to the number of groups, d_offsets to one more).  Synchronises once,
// to read the number of groups.
GRACE_HOST void fof_groups_sph(const detail::dvec<int>& d_labels, const int min_members,
                               detail::dvec<int>& d_group_of, detail::dvec<int>& d_sizes,
                               detail::dvec<int>& d_offsets, detail::dvec<int>& d_members)
{
    const size_t n = d_labels.size();
    d_group_of.resize(n);
    d_sizes.resize(n);
    detail::dvec<int> d_counts;
    d_counts.assign(2, 0);
    GRACE_STATUS_CHECK(grace_fof_groups(detail::raw(d_labels), n, min_members, detail::raw(d_group_of),
                                        detail::raw(d_sizes), detail::raw(d_counts), NULL));
    int counts[2] = { 0, 0 };                  // {groups, members of kept groups}
    GRACE_STATUS_CHECK(grace_memcpy_dtoh(counts, detail::raw(d_counts), sizeof(counts), NULL));
    GRACE_STATUS_CHECK(grace_stream_synchronize(NULL));
    d_sizes.resize(size_t(counts[0]));
    d_offsets.assign(size_t(counts[0]) + 1, 0);
    d_members.resize(size_t(counts[1]));
    GRACE_STATUS_CHECK(grace_fof_members(detail::raw(d_group_of), n, detail::raw(d_sizes), size_t(counts[0]),
                                         detail::raw(d_offsets), detail::raw(d_members), NULL));
}

} // namespace grace
