// grace/cuda/scan.cuh -- per-ray exclusive prefix sums over hit lists (reference
// include/grace/cuda/scan.cuh:15-58, there through the vendored sgpu SegScanCsr; here the
// wave64 segmented scan of libgrace_hip.so, csrc/scan.hip).  Segment s covers
// [offsets[s], offsets[s + 1]) (the last one up to the end of the data); empty segments are
// allowed.
#pragma once

#include "grace/detail/raw.h"

#include "grace/detail/scan.h"   // exclusive_segmented_scan, weighted_exclusive_segmented_scan
