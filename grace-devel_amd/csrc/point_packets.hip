// The point-query front end (point_packets.hpp): Morton keys of the caller's points against the
// tree's root box, packet starts cut at every 64th sorted point and at Morton-cell changes, and the
// host sequence that runs them.
#include "point_packets.hpp"

#include "grace/generic/morton.h"

namespace grace_hip {

namespace {

// 30-bit Morton keys of the points against the tree's root box (read here: no host round trip);
// points are clamped into the box (NaN: to its lower corner).
__global__ __launch_bounds__(256) void packet_keys_kernel(const float* __restrict__ pts, size_t n, int stride,
                                                          const float4* __restrict__ nodes, int n_nodes,
                                                          const int* __restrict__ root, uint32_t* __restrict__ keys)
{
    const int r = *root;
    float lo[3] = { 0.f, 0.f, 0.f }, hi[3] = { 0.f, 0.f, 0.f };
    if (r >= 0 && r < n_nodes) {
        const float4 L = nodes[4 * size_t(r) + 1], R = nodes[4 * size_t(r) + 2], Z = nodes[4 * size_t(r) + 3];
        lo[0] = fminf(L.x, R.x); hi[0] = fmaxf(L.y, R.y);
        lo[1] = fminf(L.z, R.z); hi[1] = fmaxf(L.w, R.w);
        lo[2] = fminf(Z.x, Z.z); hi[2] = fmaxf(Z.y, Z.w);
    }
    for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
        uint32_t c[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const float v = fminf(fmaxf(pts[i * size_t(stride) + d], lo[d]), hi[d]);
            const float ext = hi[d] - lo[d];
            const float t = ext > 0.0f ? (v - lo[d]) / ext : 0.0f;
            c[d] = min(uint32_t(fmaxf(t, 0.0f) * 1023.0f), 1023u);
        }
        keys[i] = grace::morton_key(c[0], c[1], c[2]);
    }
}

// Packet starts of the sorted points: every 64th point and every change of the Morton cell
// (key >> shift).  flags -> (scan) -> positions; the last thread also writes the end sentinel.
__global__ __launch_bounds__(256) void packet_flags_kernel(const uint32_t* __restrict__ keys, size_t n, int shift,
                                                           uint32_t* __restrict__ flags)
{
    for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x)
        flags[i] = (i % 64 == 0 || (keys[i] >> shift) != (keys[i - 1] >> shift)) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void packet_starts_kernel(const uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ pos, size_t n,
                                                            uint32_t* __restrict__ starts)
{
    for (size_t i = blockIdx.x * size_t(blockDim.x) + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
        if (flags[i]) starts[pos[i]] = uint32_t(i);
        if (i == n - 1) starts[pos[i] + flags[i]] = uint32_t(n);
    }
}

} // namespace

grace_status point_packets(FrameGuard& frame, const float* pts, size_t n, int stride,
                           const float4* nodes, int n_nodes, const int* root, hipStream_t stream, PointPackets& out)
{
    int level = 0;
    while (level < 10 && (size_t(1) << (3 * (level + 1))) * 256 <= n) ++level;
    const int shift = 30 - 3 * level;
    const size_t max_packets = (n + 63) / 64 + (size_t(1) << (3 * level));
    GRACE_TRY(frame.begin(4 * Workspace::aligned(n * 4) + Workspace::aligned((max_packets + 1) * 4)
                          + Workspace::aligned(scan_ws_count(n) * 4) + Workspace::aligned(4)
                          + sort_ws_bytes(n, 4, 0), stream));
    uint32_t* keys = Workspace::take<uint32_t>(n);
    uint32_t* perm = Workspace::take<uint32_t>(n);
    uint32_t* flags = Workspace::take<uint32_t>(n);
    uint32_t* pos = Workspace::take<uint32_t>(n);
    uint32_t* starts = Workspace::take<uint32_t>(max_packets + 1);
    uint32_t* scan_ws = Workspace::take<uint32_t>(scan_ws_count(n));
    uint32_t* n_starts = Workspace::take<uint32_t>(1);
    const int grid = stream_grid(n, 256);
    packet_keys_kernel<<<grid, 256, 0, stream>>>(pts, n, stride, nodes, n_nodes, root, keys);
    GRACE_CHECK_LAUNCH();
    GRACE_TRY(sort_pairs_u32_nested(keys, nullptr, n, 0, 0, 30, perm, stream));
    packet_flags_kernel<<<grid, 256, 0, stream>>>(keys, n, shift, flags);
    GRACE_CHECK_LAUNCH();
    GRACE_TRY(exclusive_scan_u32(flags, pos, n, scan_ws, n_starts, stream));
    packet_starts_kernel<<<grid, 256, 0, stream>>>(flags, pos, n, starts);
    GRACE_CHECK_LAUNCH();
    out.perm = perm;
    out.starts = starts;
    out.n_starts = n_starts;
    out.max_packets = max_packets;
    return GRACE_OK;
}

} // namespace grace_hip
