// grace/detail/front_end.h -- what the shared API bodies under grace/detail/ (build_sph.h,
// trace_sph.h, scan.h, sort.h, gen_rays.h, interpolate_sph.h, neighbours_sph.h, range_sph.h, fof_sph.h, pairs_sph.h,
// periodic_trace.h) are written
// against.
// The library has two C++ front ends over the C ABI of grace_hip.h: the drop-in set
// grace/cuda/*.cuh (thrust::device_vector, hipcc) and the HIP-free mirror grace/grace.h
// (grace::device_vector, any host compiler).  Every grace:: function that forwards to the C ABI is
// defined once, in one of the shared headers, and each front end includes them AFTER it has
// defined, in namespace grace:
//
//   detail::dvec<T>            alias template of its device container; the bodies use size(),
//                              resize(n) and assign(n, value) of it
//   detail::raw(v)             the container's raw device pointer, const and non-const
//   GRACE_STATUS_CHECK(s)      its policy for a grace_status: both throw std::invalid_argument for
//                              GRACE_INVALID_ARGUMENT and print and exit on any other failure
//   detail::too_many_hits(b)   throws its std::invalid_argument for more than INT_MAX per-hit slots
//                              (b: with one sentinel slot per ray)
//   Tree                       nodes, leaves, root_index_ptr, max_per_leaf
//   float3, float4, int3, double3, double4, Octants, RaySortType
//
// The drop-in set defines them in grace/detail/raw.h, grace/cuda/nodes.h, grace/error.h and
// grace/types.h, the mirror at the top of grace/grace.h.  Inside namespace grace the unqualified
// vector types resolve to HIP's in the drop-in set and to grace::float4 ... in the mirror.  No shared
// header includes a HIP or container-library header, so none can be included on its own.
#pragma once

#include "grace/detail/config.h"
#include "grace/ray.h"
#include "grace_hip.h"

#include <stddef.h>

namespace grace {
namespace detail {

// x y z of float3 / double3 / float4 / ... as an array of the component type.
template <typename Real, typename Vec3>
inline void xyz(const Vec3& v, Real* out) { out[0] = Real(v.x); out[1] = Real(v.y); out[2] = Real(v.z); }

} // namespace detail
} // namespace grace
