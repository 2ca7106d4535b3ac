// grace/cuda/sort.cuh -- per-ray sort of hits by distance (reference
// include/grace/cuda/sort.cuh:97-131, there sgpu SegSortPairsFromIndices + thrust::gather; here
// the one-wavefront-per-ray radix sort of libgrace_hip.so, csrc/segsort.hip): within each ray's
// segment the distances become non-decreasing, equal distances keep their order, and the hit
// indices and hit data are permuted by the same map.
#pragma once

#include "grace/detail/raw.h"

#include "grace/detail/sort.h"   // sort_by_distance
