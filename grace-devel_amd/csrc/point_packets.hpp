// Pieces shared by the point-packet walks (packet_walk.hpp): the packets of the caller's points
// (point_packets.hip: Morton keys against the tree's root box, packet starts cut at Morton-cell
// changes), and the device helpers every walk uses -- wave reductions, the wave-level LDS
// ordering and the correctly rounded fp32 sqrt (internal linkage: a copy per including unit).
#pragma once

#include "common.hpp"
#include "trace_state.hpp"

namespace {

// Correctly rounded sqrt for x = 0 or x >= 2^-96 (finite): v_sqrt_f32 is within 1 ulp, the two FMA
// residuals pick the neighbour if it is closer (the trace's sqrt_rn_normal).
__device__ __forceinline__ float sqrt_rn_normal(const float x)
{
    const float y = __builtin_amdgcn_sqrtf(x);
    const float ym = __int_as_float(__float_as_int(y) - 1);
    const float yp = __int_as_float(__float_as_int(y) + 1);
    const float rm = __builtin_fmaf(-ym, y, x);
    const float rp = __builtin_fmaf(-yp, y, x);
    float r = (0.0f >= rm) ? ym : y;
    r = (0.0f < rp) ? yp : r;
    return r;
}

__device__ __forceinline__ float sqrt_rn(const float x)
{
    const bool tiny = x < 1.2621774e-29f && x > 0.0f;   // 2^-96: the general expansion (practically never)
    return __builtin_amdgcn_ballot_w64(tiny) ? __builtin_sqrtf(x) : sqrt_rn_normal(x);
}

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// Orders LDS stores of some lanes before loads of others within the wave.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

} // namespace

namespace grace_hip {

// The caller's points in packets: 30-bit keys against the root box, the library's sort, packet
// starts at every 64th sorted point and at every change of the Morton cell.  Cells hold ~256 points
// of a uniform set: 8^L cells, L the largest level with 8^L <= n / 256.  Opens `frame`, which must
// stay open until the walk reading perm and starts has been launched.
struct PointPackets {
    const uint32_t* perm;        // sorted position -> point index
    const uint32_t* starts;      // packet p: sorted points [starts[p], starts[p + 1])
    const uint32_t* n_starts;    // number of packets (device)
    size_t max_packets;          // upper bound of *n_starts: n / 64 + cells
};

// (point_packets.hip)
grace_status point_packets(FrameGuard& frame, const float* pts, size_t n, int stride, const float4* nodes,
                           int n_nodes, const int* root, hipStream_t stream, PointPackets& out);

} // namespace grace_hip
