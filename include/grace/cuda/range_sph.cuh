// grace/cuda/range_sph.cuh -- range queries, an extension the reference lacks: every sphere centre
// within the query point's own radius, as counts, gather sums of the SPH kernel and CSR neighbour
// lists -- grace_range_counts_f4 / grace_range_neighbours_f4 (grace_hip.h states the fp32 distance,
// the inclusive test, the order and the sums' arithmetic).  Spheres in tree order; their w is ignored.
// float4 spheres only.  Size mismatches throw std::invalid_argument, more than INT32_MAX list entries
// std::length_error; a stack overflow is reported as by the traces.
#pragma once

#include "grace/cuda/trace_sph.cuh"

#include "grace/detail/range_sph.h"   // range_counts_sph, range_neighbours_sph
