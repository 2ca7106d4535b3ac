// grace/cuda/pairs_sph.cuh -- pair counts in separation bins and radial profiles, an extension the
// reference lacks: how many sphere centres lie in each shell of separation around each query point,
// as totals over all points, per-point histograms and per-point sums of weights per shell --
// grace_pair_counts_f4 (grace_hip.h states the fp32 distance, the bins, the ordered pairs of the
// totals and the sums' order).  Spheres in tree order; their w is ignored.  float4 spheres only.
// Size mismatches throw std::invalid_argument; a stack overflow is reported as by the traces.
#pragma once

#include "grace/cuda/trace_sph.cuh"

#include "grace/detail/pairs_sph.h"   // pair_counts_sph, radial_profiles_sph
