// Friends-of-friends groups of the sphere centres (grace_fof_labels_f4) and the catalogue built
// from their labels (grace_fof_groups, grace_fof_members).  An extension the reference lacks; the
// link, the labels and the catalogue's order are stated exactly in include/grace_hip.h.
//
// Link kernel.  The query points are the spheres themselves, packed by point_packets(); one wave
// owns a packet and walks the ALBVH with range_walk.hpp's fixed-radius walk (every lane has the
// same radius, the linking length b).  A lane p only unites with survivors j < p: the fp32 d2 is
// symmetric, so each undirected link is seen from its upper end, once.  A popped range of
// primitives is therefore cut at the packet's largest index (and skipped if nothing is left); both
// are exact.  The pair list is never formed: each link is consumed by a concurrent union-find whose
// parent array is the label output itself, labels[i] = i to start.
//
// Union-find rules (what makes it correct on this chip).
//  * Forest.  parent[i] <= i always; a root has parent[i] == i.  parent[i] only ever changes to a
//    node that is, at that moment, an ancestor of i (or becomes one by that very change), so every
//    value parent[i] has ever held is i itself or an ancestor of i in every later forest: a member of
//    i's group, not above i.
//  * Hooking.  A hook is atomicCAS(&parent[hi], hi, lo) with lo < hi, both believed to be roots.
//    It succeeds only if hi IS a root at the coherence point.  A failed CAS returns hi's true
//    parent and the find resumes from there.  Every edge points to a smaller index, so there are no
//    cycles, every loop strictly decreases an index and ends, and the surviving root of a group is
//    its minimum.  No loop anywhere waits for another wave.
//  * Compression.  atomicMin(&parent[i], g) with g an ancestor of i, applied to non-roots only
//    (halving along a find; the two ends of a link after their union).  A root's parent is never
//    touched by it, so only a CAS can end a root.
//  * Loads of parent are relaxed agent-scope atomic loads.  The per-XCD L2s are not coherent and a
//    CU's L1 is never refreshed by other CUs' stores, so a plain load may return a value of any age;
//    these loads bypass L1, and whatever age their value has, by the forest rule it is a member
//    of the same group, not above i.  A stale "parent[i] == i" only ends a find early, at a node
//    that is no root any more: the CAS that follows fails and says so.  "Same root, skip" is a
//    monotone fact: two nodes that shared an ancestor once are in one group for good.  Every
//    decision that changes the forest is a CAS (or an atomicMin) at the coherence point.  So no
//    fence is needed, and none is used.
//  * Early-out.  The lane keeps its current root in a register.  A survivor's parent is staged in
//    LDS beside its record when the cluster is compacted (one coalesced load per cluster); if that,
//    or one fresh load of parent[j], equals the lane's root, the link is already known.  Inside a
//    dense core that is the common case after the first few links; after a union both ends are
//    pointed at the new root so that it stays the common case.
//  The result does not depend on which wave wins which race: a link (p, j) is dropped only when p
//  and j are already in one group, and is otherwise retried until one hook succeeds, so the final
//  forest's trees are exactly the connected components, and each one's root is its minimum.
//
// The flatten kernel runs after the link kernel -- the kernel boundary makes the forest visible --
// and sets labels[i] = root(i).  It writes what it reads: a parent that has been flattened already
// is the root, an ancestor like any other.
//
// Catalogue.  Sizes are an integer atomicAdd histogram on the root's slot (integer adds commute:
// deterministic); kept roots (size >= min_members) are marked and scanned into group numbers, in
// ascending label; members are the stable sort of the indices keyed on group_of over the bits
// n_groups needs, so rows come out in ascending index with no atomic append.  All scratch is the
// workspace frame's: no allocation and no synchronisation in any launch function.
#include "range_walk.hpp"

#include <cmath>

using namespace grace_hip;

namespace {

struct FofArgs : WalkArgs {
    int* parent;                 // the labels
};

__device__ __forceinline__ int load_parent(const int* parent, const int i)
{
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of i's tree as far as this lane can see (see the header: it may be a root no more),
// halving the path behind it.  p: a value of parent[i].
__device__ __forceinline__ int find_root(int* parent, int i, int p)
{
    while (p != i) {                                     // i is no root: p < i
        const int g = load_parent(parent, p);
        if (g != p) atomicMin(parent + i, g);            // g < p: i's grandparent, an ancestor
        i = p;
        p = g;
    }
    return i;
}

// Unites the groups of u (the lane's root, or an ancestor-to-be of it) and of j, whose parent was
// just read as pj.  Returns the root of the united group.
__device__ __forceinline__ int unite(int* parent, int u, const int j, const int pj)
{
    u = find_root(parent, u, load_parent(parent, u));
    int v = find_root(parent, j, pj);
    while (u != v) {
        const int hi = max(u, v), lo = min(u, v);
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;                        // hooked: hi was a root
        const int r = find_root(parent, old, load_parent(parent, old));   // old < hi: hi's true parent
        if (u == hi) u = r; else v = r;
    }
    return u;
}

__device__ __forceinline__ int wave_max_int(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
    return __builtin_amdgcn_readfirstlane(v);
}

// range_walk.hpp's Visitor: a lane links its own sphere p to every centre j < p in range.
struct LinkVisitor {
    int* parent;
    int* s_par;                  // parents of the wave's 64 survivor records, as staged
    int p = -1, p_max = -1, root = -1;

    __device__ __forceinline__ LinkVisitor(int* labels, int* staged) : parent(labels), s_par(staged) {}

    __device__ __forceinline__ void begin(const bool in_range, const bool on, const uint32_t src, const float)
    {
        p = on ? int(src) : -1;                          // off lanes link nothing: no j < -1
        p_max = wave_max_int(p);
        root = p;                                        // (its own root until the first union)
    }
    // only j < p_max can be below some lane's p
    __device__ __forceinline__ bool clip(const int& lo, int& hi) const
    {
        hi = min(hi, p_max);
        return hi > lo;
    }
    __device__ __forceinline__ void stage(const int pos, const int j) { s_par[pos] = load_parent(parent, j); }
    __device__ __forceinline__ void hit(const int pos, const float4& rec, const float)
    {
        const int j = __float_as_int(rec.w);
        if (j >= p || s_par[pos] == root) return;
        const int pj = load_parent(parent, j);
        if (pj == root) return;
        root = unite(parent, root, j, pj);
        // both ends straight under the root (non-roots only: a node that is not the root of its
        // group is no root)
        if (j != root) atomicMin(parent + j, root);
        if (p != root) atomicMin(parent + p, root);
    }
    __device__ __forceinline__ void finish(const uint32_t) const {}
};

template <typename Args>
__global__ __launch_bounds__(PW_BLOCK) void fof_link_kernel(const Args a)
{
    __shared__ float4 s_rec[PW_WAVES][64];
    __shared__ int s_par[PW_WAVES][64];
    const PacketWave w = packet_wave();
    if (w.packet < int(*a.n_starts)) {
        LinkVisitor v(a.parent, s_par[w.wv]);
        walk(a, w.packet, w.lane, s_rec[w.wv], v);
    }
}

__global__ __launch_bounds__(256) void fof_init_kernel(int* __restrict__ labels, const int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) labels[i] = i;
}

__global__ __launch_bounds__(256) void fof_flatten_kernel(int* labels, const int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int r = i, p = load_parent(labels, i);
        while (p != r) { r = p; p = load_parent(labels, r); }
        __hip_atomic_store(labels + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- catalogue ----
// A label outside [0, n) (not one of grace_fof_labels_f4's) counts for no group: group_of = -1.
__global__ __launch_bounds__(256) void fof_hist_kernel(const int* __restrict__ labels, const int n,
                                                       int* __restrict__ hist)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int l = labels[i];
        if (l >= 0 && l < n) atomicAdd(hist + l, 1);
    }
}

__global__ __launch_bounds__(256) void fof_mark_kernel(const int* __restrict__ labels, const int* __restrict__ hist,
                                                       const int n, const int min_members,
                                                       uint32_t* __restrict__ marks)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        marks[i] = (labels[i] == i && hist[i] >= min_members) ? 1u : 0u;
}

// counts: {n_groups (written by the scan), members of kept groups (zeroed before)}
__global__ __launch_bounds__(256) void fof_compact_kernel(const int* __restrict__ labels, const int* __restrict__ hist,
                                                          const uint32_t* __restrict__ marks,
                                                          const uint32_t* __restrict__ pos, const int n,
                                                          int* __restrict__ group_of, int* __restrict__ sizes,
                                                          int* __restrict__ counts)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int l = labels[i];
        const bool kept = l >= 0 && l < n && marks[l] != 0u;
        if (marks[i]) {
            sizes[pos[i]] = hist[i];                     // pos[i] < n_groups <= n
            atomicAdd(counts + 1, hist[i]);              // (one integer add per kept group)
        }
        group_of[i] = kept ? int(pos[l]) : -1;
    }
}

__global__ __launch_bounds__(256) void fof_keys_kernel(const int* __restrict__ group_of, const int n,
                                                       const int n_groups, uint32_t* __restrict__ keys)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int g = group_of[i];
        keys[i] = (g >= 0 && g < n_groups) ? uint32_t(g) : uint32_t(n_groups);   // not kept: after every row
    }
}

// members = the first offsets[n_groups] sorted indices (never more than n)
__global__ __launch_bounds__(256) void fof_members_kernel(const uint32_t* __restrict__ perm, const int n,
                                                          const int* __restrict__ total, int* __restrict__ members)
{
    const int m = min(max(*total, 0), n);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) members[i] = int(perm[i]);
}

// grace_fof_labels_f4 and its periodic form (Periodic<FofArgs>: the link kernel over the walk's
// periodic variant; the visitor, the union-find and the flatten are the same): `a` is zero but for
// a period.
template <typename Args>
grace_status fof_labels(Args a, const float* d_spheres, size_t n_spheres, const int* d_nodes, size_t n_nodes,
                        const int* d_leaves, const int* d_root, float linking_length, int* d_labels,
                        grace_stream stream)
{
    GRACE_REQUIRE(std::isfinite(linking_length) && linking_length >= 0.0f,
                  "fof_labels: the linking length must be finite and not negative");
    GRACE_REQUIRE(n_spheres < (size_t(1) << 31), "fof_labels: more than INT32_MAX spheres");
    if (n_spheres == 0) return GRACE_OK;   // (before the pointer checks: a caller's empty arrays may be null)
    GRACE_REQUIRE(d_labels, "fof_labels: null labels");
    GRACE_TRY(walk_scene(a, nullptr, linking_length, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root));
    a.parent = d_labels;
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    const hipStream_t stream_ = as_stream(stream);
    const int n = int(n_spheres);
    fof_init_kernel<<<stream_grid(n_spheres, 256), 256, 0, stream_>>>(d_labels, n);
    GRACE_CHECK_LAUNCH();
    return packet_run(a, *ts, d_spheres, n_spheres, 4, stream_, [&](const Args& w, size_t waves) -> grace_status {
        fof_link_kernel<<<ceil_div(waves, PW_WAVES), PW_BLOCK, 0, stream_>>>(w);
        GRACE_CHECK_LAUNCH();
        fof_flatten_kernel<<<stream_grid(n_spheres, 256), 256, 0, stream_>>>(w.parent, n);
        GRACE_CHECK_LAUNCH();
        return GRACE_OK;
    });
}

} // namespace

extern "C" {

grace_status grace_fof_labels_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                 const int* d_leaves, const int* d_root, float linking_length, int* d_labels,
                                 grace_stream stream)
{
    return fof_labels(FofArgs(), d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, linking_length, d_labels,
                      stream);
}

grace_status grace_fof_labels_periodic_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                          size_t n_nodes, const int* d_leaves, const int* d_root,
                                          float linking_length, int* d_labels, const float* h_period3,
                                          grace_stream stream)
{
    Periodic<FofArgs> a = {};
    GRACE_TRY(walk_period(a.per, h_period3, &linking_length));
    return fof_labels(a, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, d_root, linking_length, d_labels, stream);
}

grace_status grace_fof_groups(const int* d_labels, size_t n, int min_members, int* d_group_of, int* d_sizes,
                              int* d_n_groups, grace_stream stream)
{
    GRACE_REQUIRE(min_members >= 1, "fof_groups: min_members must be at least 1");
    GRACE_REQUIRE(n < (size_t(1) << 31), "fof_groups: more than INT32_MAX labels");
    if (n == 0) return GRACE_OK;
    GRACE_REQUIRE(d_labels && d_group_of && d_sizes && d_n_groups, "fof_groups: null pointer");
    const hipStream_t st = as_stream(stream);
    FrameGuard frame;
    GRACE_TRY(frame.begin(3 * Workspace::aligned(n * 4) + Workspace::aligned(scan_ws_count(n) * 4), st));
    int* hist = Workspace::take<int>(n);
    uint32_t* marks = Workspace::take<uint32_t>(n);
    uint32_t* pos = Workspace::take<uint32_t>(n);
    uint32_t* scan_ws = Workspace::take<uint32_t>(scan_ws_count(n));
    const int grid = stream_grid(n, 256);
    GRACE_TRY_HIP(hipMemsetAsync(hist, 0, n * 4, st));
    GRACE_TRY_HIP(hipMemsetAsync(d_n_groups, 0, 8, st));
    fof_hist_kernel<<<grid, 256, 0, st>>>(d_labels, int(n), hist);
    GRACE_CHECK_LAUNCH();
    fof_mark_kernel<<<grid, 256, 0, st>>>(d_labels, hist, int(n), min_members, marks);
    GRACE_CHECK_LAUNCH();
    GRACE_TRY(exclusive_scan_u32(marks, pos, n, scan_ws, reinterpret_cast<uint32_t*>(d_n_groups), st));
    fof_compact_kernel<<<grid, 256, 0, st>>>(d_labels, hist, marks, pos, int(n), d_group_of, d_sizes, d_n_groups);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

grace_status grace_fof_members(const int* d_group_of, size_t n, const int* d_sizes, size_t n_groups,
                               int* d_offsets, int* d_members, grace_stream stream)
{
    GRACE_REQUIRE(n < (size_t(1) << 31), "fof_members: more than INT32_MAX spheres");
    GRACE_REQUIRE(n_groups <= n, "fof_members: more groups than spheres");
    if (n == 0) return GRACE_OK;
    GRACE_REQUIRE(d_group_of && d_offsets, "fof_members: null pointer");
    GRACE_REQUIRE(n_groups == 0 || (d_sizes && d_members), "fof_members: null pointer");
    const hipStream_t st = as_stream(stream);
    FrameGuard frame;
    GRACE_TRY(frame.begin(2 * Workspace::aligned(n * 4) + Workspace::aligned(scan_ws_count(n_groups) * 4)
                          + sort_ws_bytes(n, 4, 0), st));
    uint32_t* keys = Workspace::take<uint32_t>(n);
    uint32_t* perm = Workspace::take<uint32_t>(n);
    uint32_t* scan_ws = Workspace::take<uint32_t>(scan_ws_count(n_groups));
    // offsets[0 .. n_groups) = the exclusive scan of the sizes, offsets[n_groups] = their total
    GRACE_TRY(exclusive_scan_u32(reinterpret_cast<const uint32_t*>(d_sizes), reinterpret_cast<uint32_t*>(d_offsets),
                                 n_groups, scan_ws, reinterpret_cast<uint32_t*>(d_offsets) + n_groups, st));
    if (n_groups == 0) return GRACE_OK;
    int bits = 1;                                        // keys 0 .. n_groups
    while ((n_groups >> bits) != 0) ++bits;
    const int grid = stream_grid(n, 256);
    fof_keys_kernel<<<grid, 256, 0, st>>>(d_group_of, int(n), int(n_groups), keys);
    GRACE_CHECK_LAUNCH();
    GRACE_TRY(sort_pairs_u32_nested(keys, nullptr, n, 0, 0, bits, perm, st));
    fof_members_kernel<<<grid, 256, 0, st>>>(perm, int(n), d_offsets + n_groups, d_members);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

} // extern "C"
