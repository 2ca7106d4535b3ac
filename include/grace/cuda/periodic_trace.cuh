// grace/cuda/periodic_trace.cuh -- periodic boxes for traces, an extension the reference lacks: the
// images of the spheres that stick out of a face (grace::periodic_scene_sph) and the
// grace::PeriodicScene overloads of trace_hitcounts_sph, trace_cumulative_sph and
// trace_cumulative_weighted_sph, which cut every ray at the faces it crosses, trace the pieces with the
// open traces and fold the results back (grace_hip.h, "Periodic boxes for traces", has the definition).
// float4 spheres only; any number of rays.
#pragma once

#include "grace/cuda/build_sph.cuh"
#include "grace/cuda/trace_sph.cuh"

#include "grace/detail/periodic_trace.h"   // PeriodicScene, periodic_scene_sph, the trace overloads
