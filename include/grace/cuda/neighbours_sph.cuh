// grace/cuda/neighbours_sph.cuh -- k nearest neighbours and smoothing lengths, an extension the
// reference lacks: grace_nearest_neighbours_f4 / grace_smoothing_lengths_f4 (grace_hip.h states
// the fp32 distance and the exact (d2, index) ranking).  Spheres in tree order; their w is ignored.
// float4 spheres only.  Size mismatches throw std::invalid_argument; a stack overflow is reported
// as by the traces.
#pragma once

#include "grace/cuda/trace_sph.cuh"

#include "grace/detail/neighbours_sph.h"   // nearest_neighbours_sph, smoothing_lengths_sph
