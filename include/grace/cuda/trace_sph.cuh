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

#include <stdexcept>

namespace grace {
namespace detail {

// More hits than the int ray offsets address (trace_sph, trace_with_sentinels_sph alike).
inline void too_many_hits(bool)
{
    throw std::invalid_argument("trace_sph: more than INT_MAX hits; the int ray offsets cannot "
                                "address the per-hit arrays. Trace fewer rays per call.");
}

} // namespace detail
} // namespace grace

// N_table, KernelIntegrals, trace_hitcounts_sph, trace_cumulative_sph, trace_sph,
// trace_with_sentinels_sph and the extensions (weighted, emission-absorption, deposit, spectra,
// SphKernel, PreparedTrace)
#include "grace/detail/trace_sph.h"
