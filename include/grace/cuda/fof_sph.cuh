// grace/cuda/fof_sph.cuh -- friends-of-friends groups, an extension the reference lacks: the
// connected components of the graph that links sphere centres within one linking length, as labels
// and as a catalogue (group numbers, sizes, CSR member lists) -- grace_fof_labels_f4 /
// grace_fof_groups / grace_fof_members (grace_hip.h states the fp32 distance, the inclusive test,
// the labels and the catalogue's order).  Spheres in tree order; their w is ignored.  float4
// spheres only.  A stack overflow is reported as by the traces.
#pragma once

#include "grace/cuda/trace_sph.cuh"

#include "grace/detail/fof_sph.h"   // fof_labels_sph, fof_groups_sph
