// grace/cuda/gen_rays.cuh -- the ray generators of the reference
// (include/grace/cuda/gen_rays.cuh:25-399) with their signatures, dispatching to the
// deterministic generators of libgrace_hip.so (csrc/rays.hip).  The reference draws from
// cuRAND, whose streams are device-specific by its own account (kernels/gen_rays.cuh:21-24):
// only the distributions and the ordering contracts are kept, never the random stream.
// Positions, directions and lengths are computed in float (Real = float arithmetic); a double
// Real or Real3 argument is narrowed.
#pragma once

#include "grace/detail/raw.h"
#include "grace/ray.h"

// uniform_random_rays[_single_octant], one_to_many_rays, plane_parallel_random_rays,
// orthographic_projection_rays, pinhole_camera_rays: pointer and vector overloads
#include "grace/detail/gen_rays.h"
