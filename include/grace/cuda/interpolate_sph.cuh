// grace/cuda/interpolate_sph.cuh -- SPH interpolation at points, an extension the reference lacks:
// the field A(p) = sum_i fl(w_i W(|p - x_i|, H_i)) of the spheres (tree order, w = support radius H)
// with the context's SPH kernel (set_sph_kernel; a custom table is refused), and the number of
// spheres containing each point -- grace_interpolate_points_f4 / grace_interpolate_grid_f4
// (grace_hip.h states the arithmetic and the summation order).  d_weights holds n_channels weights
// per sphere, sphere-major, in the order of d_spheres; d_out[p * n_channels + c].  float4 spheres
// only.  Size mismatches throw std::invalid_argument; a stack overflow is reported as by the traces.
// Gradients of the same field: grace::interpolate_gradient_sph, interpolate_gradient_grid_sph and
// divergence_curl_sph (grace_interpolate_gradient_points_f4 / _grid_f4, grace_gradient_div_curl_f32).
#pragma once

#include "grace/cuda/trace_sph.cuh"

#include "grace/detail/interpolate_sph.h"   // interpolate_sph, interpolate_grid_sph, interpolate_gradient_sph, ...
