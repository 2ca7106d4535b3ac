// grace/cuda/gravity_sph.cuh -- tree gravity, an extension the reference lacks: potentials and
// accelerations at points from the BVH, the Barnes-Hut walk with monopoles of the inner nodes,
// G = 1 -- grace_gravity_moments_f4 and grace_gravity_points_f4 (grace_hip.h states the moments,
// the acceptance test, the fp32 pair term and the order of the fp64 sums).  Spheres and masses in
// tree order; the spheres' w is ignored.  float4 spheres only.  Size mismatches throw
// std::invalid_argument; a stack overflow is reported as by the traces.
#pragma once

#include "grace/cuda/trace_sph.cuh"

#include "grace/detail/gravity_sph.h"   // gravity_moments_sph, gravity_sph, gravity_group_moments_sph, gravity_groups_sph
