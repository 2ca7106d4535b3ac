// grace/cuda/build_sph.cuh -- the SPH build API of the reference
// (include/grace/cuda/build_sph.cuh:16-124) with its template signatures over
// thrust::device_vector, every body a type dispatch onto libgrace_hip.so:
//
//   morton_keys_sph            -> grace_morton_keys{30,63}_f4[_d3] / _points[_d3]   (csrc/morton.hip)
//   morton_keys{30,63}_sort_sph-> the same + grace_sort_pairs_u32/u64               (csrc/sort.hip;
//                                 the reference calls thrust::sort_by_key: stable, in place)
//   euclidean / surface_area / XOR _deltas_sph -> grace_deltas_*                    (csrc/deltas.hip)
//   ALBVH_sph                  -> grace_albvh_build_*                               (csrc/albvh.hip)
//
// Real4 is float4 or double4, KeyType / XOR DeltaType uinteger32 or uinteger64, Real the scalar
// type of Real4 (as the reference requires, build_sph.cuh:84-86).  rocThrust is the container
// only: no Thrust algorithm runs on this path.
#pragma once

#include "grace/cuda/nodes.h"
#include "grace/detail/raw.h"
#include "grace/generic/meta.h"

// morton_keys_sph, morton_keys{30,63}_sort_sph, euclidean / surface_area / XOR _deltas_sph, ALBVH_sph
#include "grace/detail/build_sph.h"
