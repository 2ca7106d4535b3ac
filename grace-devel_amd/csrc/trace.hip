// BVH traversal with ray-sphere tests and SPH-kernel line integrals, for gfx950.
//
// Replaces trace_kernel (reference include/grace/cuda/kernels/bintree_trace.cuh:52-197) as
// instantiated by trace_hitcounts_sph / trace_cumulative_sph / trace_sph
// (include/grace/cuda/trace_sph.cuh:58-168) with the functors of
// include/grace/cuda/functors/trace.cuh, AABBs_hit (include/grace/cuda/device/intersect.cuh:
// 10-40) and sphere_hit (include/grace/generic/intersect.h:10-55).
//
// Same traversal semantics: a packet of rays shares one stack; a child is pushed if ANY
// ray of the packet hits its box (right first, so the left subtree is walked first and
// every ray meets its hits in ascending primitive index); every ray of the packet is
// tested against every sphere of every leaf the packet enters.  Results per ray therefore
// equal the brute-force loop over all spheres (the reference's own criterion,
// tests/tree_traversal/tree_traversal.cu:65-100).
//
// CDNA4 design (not the reference's; measurements in DESIGN.md section 4/6):
//   * packet = one 64-lane wavefront (the reference: a 32-thread warp); for the per-hit and
//     triangle walks of small batches, 32 or 16 rays per wave;
//   * the packet's stack lives in TWO VGPRs indexed by lane (pop = v_readlane, push =
//     lane-select, with a scalar stack pointer): 128 entries, no LDS traffic;
//   * node records are wave-uniform: child indices / primitive spans are consumed as scalars,
//     the per-ray slab test keeps the reference's arithmetic (~100 node tests per packet);
//   * no FMA contraction (-ffp-contract=off), IEEE 1/x and sqrt in everything that decides a
//     hit or feeds a bit-exact output: the reference's CPU/GPU equality test is built with
//     -fmad=false (tests/tree_traversal/Makefile:5-8).  Explicit FMAs appear only where they
//     provably return the unfused bits (axis dot product), in culls, and in the fast integral;
//   * a streaming pre-pass hoists per-sphere work out of the (ray x sphere) loop:
//     A[i] = {x, y, z, h*h}, B[i] = {1/h or 50/h, (1/h)^2};
//   * ray coherence order: 64 consecutive rays of a space-filling order of the ray
//     co-ordinates that vary form a packet (15-bit round-to-nearest keys; a Hilbert curve for
//     two varying co-ordinates and, over the octahedral map of the direction, for batches from
//     one origin -- its runs never join distant patches; Z-order for power-of-two pixel grids,
//     whose tiles are the same and whose tile order suits the dispatcher better, and for
//     general batches); results do not depend on it; a batch traced repeatedly can have its
//     order prepared once (grace_trace_prepare_rays);
//   * hit counts and column densities do not walk the tree: primitives are Morton-sorted, so
//     groups of 4096 consecutive ones are compact cells; a packet tests all group boxes up
//     front, 64 per lane-parallel pass (boxes behind the cluster records, masks kept in LDS),
//     and sweeps the surviving groups in ascending order (trace_kernel.hpp);
//   * the per-hit traces, triangles and the stats walk descend the tree to subtrees of <= T
//     primitives (contiguous indices; T = 8192, 512 for triangles) and sweep those;
//   * a sweep (of a group or a subtree) has a cluster level: one box per 64 consecutive
//     primitives (a pre-pass) is tested first, lane j for cluster j, and only the surviving
//     clusters go through culling rounds of 64;
//   * scenes with spheres smaller than the ray spacing (dense cores of clustered SPH data) run
//     a separate instantiation (LAT), selected by a device flag: an exact cull against the
//     packet's origin lattice, and four waves per packet for big batches (their packets are
//     very unequal);
//   * beam culling per round, lane j deciding for candidate j whether ANY ray of the packet
//     can hit it: exact lower bound of b^2 for axis-aligned packets (rounding is monotone),
//     cone + four side planes for packets from one origin, interval arithmetic otherwise;
//   * survivors of a round are written compacted (slot = v_mbcnt) to the wave's LDS tile as
//     three 8-byte planes and read back two survivors ahead into three rotating register sets
//     (unconditional reads pinned by sched_barrier; immediates address the slots);
//   * axis-aligned packets (orthographic projections): sphere_hit collapses exactly under IEEE
//     rules to dot = fma(s_k, d_k, -o_k d_k), b2 = q1^2 + q2^2; rounds whose candidates are
//     provably inside every ray's [0, length) skip the range tests (6 instructions per test);
//   * kernel integral of the column-density trace: hardware sqrt + fp32 lerp of an fp32
//     (y, dy) table in LDS (7 instructions, tolerance parity) by default; the reference's
//     arithmetic bit for bit (correctly rounded sqrt, fp64 lerp) on request and always for
//     the per-hit outputs;
//   * class-ordered sums and packet splitting: primitives are dealt to 8 CLASSES in granules
//     of 1024 consecutive indices (class = (index >> 10) & 7).  A ray's column density is
//     defined as the balanced pairwise (binary-tree) fp32 sum of its 8 class sums, each class
//     summed in ascending primitive order.  The value is a function of the ray and the scene
//     only -- not of how rays are batched, ordered or sharded -- and differs from the
//     reference's single running sum only in the last bits (both within 1e-6 of the exact
//     sum; tolerance 1e-5).  What it buys: a packet can be walked by K = 1, 2, 4 or 8
//     waves, wave k owning the 8/K classes [k 8/K, (k+1) 8/K) -- a subtree of the summation
//     tree, and, because classes interleave along the Morton order, an even share of the
//     work for any beam -- with NO change of the result: each wave reduces its classes, a
//     tiny kernel finishes the tree.  K is the smallest power of two that puts >= 16384 waves
//     in flight; for batches of one direction (light packets) a device-side choice lowers it
//     (choose_split).  A wave keeps its class accumulators in LDS (2 KiB) and switches at
//     granule boundaries, once per culling round at most.  Hit counts split the same way
//     (integers);
//   * packet plan: once the scene records and the ray order both come out of their validated
//     caches, the cull of every axis-aligned packet -- per class the list of its survivors'
//     indices, with a {count, lean / fat bits} header per dense round -- is recorded beside them
//     (trace_planned.hip) and the column-density calls that follow run the PLANNED instantiation:
//     one gather per round and the survivor loops, headers by scalar loads; re-recorded on the
//     device when a signature has moved;
//   * per-hit outputs (ordered per ray): large batches stage hits per lane in LDS and drain
//     them eight entries per ray; small batches split a packet over K waves by contiguous
//     chunk ranges with per-(ray, chunk) output offsets from a counting walk (hits_plan_kernel);
//   * packets are dealt to workgroups so that the workgroups sharing an XCD (blockIdx % 8)
//     walk a contiguous range of packets: neighbouring packets touch the same subtree and
//     each XCD's 4 MiB L2 keeps it.
//
// Roofline: divergent tree walk, integer/fp32 scalar-operand work -- no MFMA.  Algorithmic
// bytes per ray: 28 + 64 * nodes + 16 * leaves + 16 * spheres tested + 4,
// counted per ray by the `stats` instantiation below.
#include "kernel_tables.hpp"
#include "trace_kernel.hpp"
#include "trace_plan.hpp"

#include <cmath>

using namespace grace_hip;

namespace grace_hip {

// The built-in SPH kernels' line-integral tables (kernel_tables.hpp, GRACE_SPH_KERNEL_* order): one
// device array, whose rows a context's trace calls point to, and its host copy.
static_assert(GRACE_SPH_KERNEL_TABLE_ROWS == GRACE_SPH_KERNEL_WENDLAND_C6 + 1, "one table per built-in kernel");
__device__ double g_sph_kernel_tables[GRACE_SPH_KERNEL_TABLE_ROWS][N_TABLE] = GRACE_SPH_KERNEL_TABLES_INIT;
static const double k_sph_kernel_tables[GRACE_SPH_KERNEL_TABLE_ROWS][N_TABLE] = GRACE_SPH_KERNEL_TABLES_INIT;

static grace_status trace_state_destroy(Context& c)
{
    if (!c.trace) return GRACE_OK;
    TraceState& ts = *c.trace;
    GRACE_TRY(plan_release(ts));
    GRACE_TRY(scene_release(ts));
    GRACE_TRY(rays_release(ts));
    if (ts.hits.chunk_counts) GRACE_TRY_HIP(hipFree(ts.hits.chunk_counts));
    if (ts.custom_table) GRACE_TRY_HIP(hipFree(ts.custom_table));
    if (ts.status) GRACE_TRY_HIP(hipFree(ts.status));
    if (ts.ev0) GRACE_TRY_HIP(hipEventDestroy(ts.ev0));
    if (ts.ev1) GRACE_TRY_HIP(hipEventDestroy(ts.ev1));
    delete c.trace;
    c.trace = nullptr;
    return GRACE_OK;
}

grace_status trace_state(TraceState** out)
{
    Context* c = nullptr;
    GRACE_TRY(current_context(&c));
    if (!c->trace) {
        void* tables = nullptr;     // on the context's device, which is the current one
        GRACE_TRY_HIP(hipGetSymbolAddress(&tables, HIP_SYMBOL(g_sph_kernel_tables)));
        c->trace = new TraceState();
        c->trace->builtin_tables = static_cast<const double*>(tables);
        c->trace->kernel_table = c->trace->builtin_tables + GRACE_SPH_KERNEL_CUBIC * N_TABLE;
        g_trace_state_destroy = trace_state_destroy;
    }
    *out = c->trace;
    return GRACE_OK;
}

} // namespace grace_hip

namespace {

struct LaunchPlan {   // how a call is launched: everything that follows from the sizes and the knobs alone
    int width = 64, n_packets = 0;   // rays per packet, packets
    int split = 1;                   // waves launched per packet ...
    bool dev_split = false;          // ... of which the device picks the working ones
    // split per-hit trace of small batches (see TraceArgs / hits_plan_kernel); packets of 64 rays
    int hit_chunk_shift = GRANULE_SHIFT, hit_chunks = 0, hit_split = 1;
    size_t hit_packets = 0;
    bool hits_split = false;         // this per-hit trace splits its packets by chunk ranges
    bool keep_chunks = false;        // this hit-count call keeps its chunk counts for that per-hit trace
    bool reorder = false;            // rays walk in coherence order
    bool lattice = false;            // the device flag picks the LAT instantiation (TraceArgs::lat_dev) ...
    int lat_split = 0;               // ... over this many waves per packet where one wave is planned (0: not)
    bool fast_b = false;             // column densities by the fast integral: records B50, the ALT kernels
    int treelet = 0, treelet_axis = 0;
};

template <int MODE>
LaunchPlan plan_launch(const TraceState& ts, const bool keep_requested, const size_t n_rays, const size_t n_prims)
{
    LaunchPlan p;
    // Split per-hit trace for small batches (see TraceArgs / hits_plan_kernel): chunk size =
    // a power of two >= one granule giving at most MAX_HIT_CHUNKS chunks.
    while ((((n_prims - 1) >> p.hit_chunk_shift) + 1) > size_t(MAX_HIT_CHUNKS)) ++p.hit_chunk_shift;
    p.hit_chunks = int(((n_prims - 1) >> p.hit_chunk_shift) + 1);
    p.hit_packets = ceil_div(n_rays, size_t(64));
    // Does a per-hit trace of this batch split?  (also asked by the hit-count call that keeps chunk counts)
    const bool split_hits = ts.width <= 0 && p.hit_packets < 4096 && p.hit_chunks >= 8 && ts.split != 1;
    p.hits_split = MODE == MODE_HITS && split_hits;
    p.keep_chunks = MODE == MODE_COUNT && keep_requested && split_hits;
    if (p.hits_split) {     // (2 to 8 waves per packet)
        if (ts.split > 0) p.hit_split = ts.split;
        else while (p.hit_split < 8 && p.hit_packets * p.hit_split < 16384) p.hit_split *= 2;
    }
    // Per-hit and triangle traces cannot split a packet among waves (their outputs are ordered
    // / reduced per ray inside one wave); with few rays they use narrower packets instead:
    // 2-4x the waves, each with a tighter beam, on a chip that would otherwise sit idle.
    if (ts.width > 0) p.width = ts.width;
    else if (ordered(MODE) && !p.hits_split)
        while (p.width > 16 && ceil_div(n_rays, size_t(p.width)) < 4096) p.width /= 2;
    // Hit counts and column densities split packets eight ways at most; a batch too small to fill
    // the chip even then (< 512 packets) also gets narrower packets (10^7 particles, 12288 HEALPix
    // rays: 3.5 -> 2.0 ms at 16 rays per packet; from 49152 rays on it loses: config 3 0.87 -> 0.95 ms).
    else if (class_split(MODE) && ts.split <= 0)
        while (p.width > 16 && ceil_div(n_rays, size_t(p.width)) * SUM_CLASSES < 4096) p.width /= 2;
    p.n_packets = ceil_div(n_rays, size_t(p.width));
    p.reorder = ts.ray_reorder && n_rays > 64;
    // Waves per packet: two resident sets of waves (2 x 8192) for small ray batches.
    if (class_split(MODE)) {
        // (column densities: a batch of exactly 16384 packets -- the 1024^2 frame -- still gets a
        // second wave per packet, 32768 waves; see choose_split.  Larger batches run one.)
        const size_t wave_budget = f4_sums(MODE) ? 16385 : 16384;
        if (ts.split > 0) p.split = ts.split;
        else {
            while (p.split < SUM_CLASSES && size_t(p.n_packets) * p.split < wave_budget) p.split *= 2;
            // (the device picks the working waves per packet: scenes with spheres smaller than the ray
            // spacing want four -- see lat_split below --, one-direction batches two, others one)
            if (f4_sums(MODE) && p.split > 1 && p.split < ts.lat_split && p.reorder && p.width == 64)
                p.split = ts.lat_split;
        }
    }
    if (p.hits_split) p.split = p.hit_split;
    // (the working waves per packet are chosen on the device, by ray_keys_kernel)
    p.dev_split = f4_class_split(MODE) && p.split > 1 && ts.split <= 0;
    p.lattice = has_lattice(MODE) && p.reorder;
    // A batch of >= 16384 packets runs one wave per packet -- unless the device flag says the scene
    // holds spheres smaller than the ray spacing (clustered SPH data: dense cores).  Such scenes
    // have packets dozens of times heavier than the median (10^7 particles, 90 % of them in 50
    // clumps: with the lattice cull the heaviest of 16384 waves still lived 14x the mean and set
    // the kernel time), so the lattice instantiation of these batches is the class-split kernel
    // with four waves per packet: the heaviest packets' work is spread over four SIMDs (measured
    // on two clustered scenes: K = 2 / 4 / 8 -> 3.62 / 3.47 / 4.24 ms and 4.24 / 3.42 / 3.71 ms;
    // one wave: 4.66 and 6.78 ms).  Same class sums, same bits.
    if (f4_class_split(MODE) && p.split == 1 && p.lattice && p.width == 64
        && ts.lat_split > 0 && ts.split <= 0)   // (an explicit grace_trace_set_packet_split is obeyed)
        p.lat_split = ts.lat_split;
    p.fast_b = f4_sums(MODE) && !ts.exact_integrals;
    // Subtrees of up to this many primitives are swept -- cluster tests, then culling rounds
    // over the surviving clusters -- rather than descended.
    // Axis-aligned packets test a cluster's box against their origin rectangle (sharp: large
    // subtrees pay; 16384 measured best in round 2); pencil packets test it
    // against the bundle's side planes, general packets its circumscribed sphere.
    // (re-measured after the pencil cluster test became a box-against-side-planes test: sphere
    // scenes now prefer 8192 there too -- config 2 column densities 1.74 -> 1.46 ms, hit counts
    // 1.54 -> 1.19, config 3 0.94 -> 0.87 --; triangles, culled through bounding spheres, keep 512:
    // 5.3 / 4.6 / 2.8 ms for the three cameras against 6.9 / 5.8 / 3.0 at 8192)
    // (round 3, after the test-free 16-byte survivor rounds made the sweeps cheaper relative to
    // the walk: axis-aligned packets prefer 32768 -- 1024^2 frame 2.82 -> 2.78 ms, its 1/2, 1/4,
    // 1/8 shards 1.53 -> 1.46, 0.84 -> 0.80, 0.51 -> 0.47 ms (their split waves each repeat the
    // walk); 65536 the same, 131072 worse; clustered scenes +3 %.  Pencil / general packets stay
    // at 8192: config 2 1.47 / 1.50 / 1.50 ms at 8192 / 16384 / 32768, config 3 0.87 / 0.83 / 0.86.)
    const int auto_treelet = (MODE == MODE_TRI) ? 512 : 8192, auto_treelet_axis = 32768;
#ifdef GRACE_PACKET_STATS
    p.treelet = ts.treelet < 0 ? auto_treelet : ts.treelet;
    p.treelet_axis = ts.treelet < 0 ? auto_treelet_axis : ts.treelet;
#else
    p.treelet = (MODE == MODE_STATS) ? 0 : (ts.treelet < 0 ? auto_treelet : ts.treelet);
    p.treelet_axis = (MODE == MODE_STATS) ? 0 : (ts.treelet < 0 ? auto_treelet_axis : ts.treelet);
#endif
    return p;
}

// A trace made inside another entry point's open workspace frame (the ordered integrals trace
// their rays batch by batch): it carves from that frame instead of opening one, and leaves the
// automatic ray cache alone.  measure: only report the frame bytes such a call needs at most.
struct Nested { bool on = false; size_t* measure = nullptr; };

struct TraceBuffers {   // a call's buffers in its workspace frame (null: not needed)
    unsigned long long* sig = nullptr;   // signature partials (launch_signatures)
    // scene records derived per call (not cached)
    float4* A = nullptr; float2* B = nullptr; double* T64 = nullptr; int2* node_prims = nullptr; float4* C = nullptr;
    float* partial = nullptr; double* partial_d = nullptr;   // class sums of split packets
    int *chunk_counts = nullptr, *chunk_off = nullptr, *scratch_counts = nullptr;   // split per-hit trace
    int4* wave_map = nullptr; int *n_wave_map = nullptr, *pk_first = nullptr, *pk_parts = nullptr;
    uint32_t *pk_prefix = nullptr, *pk_total = nullptr;
    // ray order; ext: 12 extents + [12] the device-side split + [13] the lattice flag (per call)
    // + [14], [15] the grid flag and the longest ray + [16] the planned kernel's split (per call)
    uint32_t* ext = nullptr; uint32_t* keys = nullptr; uint32_t* perm = nullptr;
    // Packet plan (set by use_records): this call may use one -- both caches serve it --, under this key
    bool plan_eligible = false;
    PlanKey plan_key;
    int plan_request = 0;   // what the call asks of the plan's layout: 0 format 3; -1 / 1 sub-tiles, automatic / forced
};

// Opens the call's frame and points `a` at its scene records and ray order, cached or derived here.
// Side effects in this order: the caches' `seen` keys, a cache allocated on FILL, the frame, the
// signatures, the scene pre-pass, the ray order (or, for a cached order, the device-side choices).
template <int MODE>
grace_status use_records(TraceState& ts, TraceArgs& a, TraceBuffers& b, FrameGuard& frame, const LaunchPlan& p,
                         const size_t n_rays, const size_t n_prims, const size_t n_nodes, hipStream_t stream,
                         const Nested nested = Nested())
{
    // ---- which cached records does this call use?  (see trace_state.hpp) -------------------
    // NONE: derive into the workspace (a scene / batch seen for the first time);  FILL: the
    // same arrays as the previous call -- derive into the cache;  CHECK: cached -- validate by
    // signature on the device, the gated pre-pass recomputes if stale;  TRUST: cached, and the
    // caller has switched validation off.
    enum CacheUse { USE_NONE, USE_FILL, USE_CHECK, USE_TRUST };
    auto decide = [&](const bool have, const bool pinned, const bool repeat) {
        if (have) return ts.cache_validation ? USE_CHECK : USE_TRUST;
        return (ts.cache_auto && repeat && !pinned) ? USE_FILL : USE_NONE;
    };
    CacheUse scene_use = USE_NONE, rays_use = USE_NONE;
    const SceneKey skey{primitive(MODE), a.spheres, a.nodes, a.leaves, n_prims, n_nodes};
    // The fp64 modes' records (inflated for the fp64 test) are derived per call: the scene cache
    // is neither read nor filled nor counted as seen by them, so float calls on the same arrays
    // cache exactly as they would without them.
    if (!fp64(MODE) && MODE != MODE_STATS && !nested.measure) {
        scene_use = decide(ts.scene.valid && ts.scene.key == skey, ts.scene.valid && ts.scene.pinned,
                           ts.scene.seen == skey);
        ts.scene.seen = skey;
        if (scene_use == USE_FILL && scene_cache_alloc(ts, skey) != GRACE_OK) scene_use = USE_NONE;   // (no memory: no cache)
    }
    const RayKey rkey{a.rays, n_rays};
    // (a nested call traces a sub-range of its caller's rays: the ray cache, which validates by
    // content and reallocates when the range changes, neither sees nor serves it)
    if (p.reorder && !nested.on) {
        rays_use = decide(ts.rays.valid && ts.rays.key == rkey, ts.rays.valid && ts.rays.pinned,
                          ts.rays.seen == rkey);
        ts.rays.seen = rkey;
        if (rays_use == USE_FILL && rays_cache_alloc(ts, rkey) != GRACE_OK) rays_use = USE_NONE;
    }
    const bool scene_cached = scene_use != USE_NONE, rays_cached = rays_use != USE_NONE;
    // A packet plan is recorded from, and used with, records and an order that both come out of
    // their caches (each seen repeated, or prepared).  Batches that run the lattice kernel split
    // (lat_split) keep it: their heaviest packets need its four waves.
    auto held = [](const CacheUse u) { return u == USE_CHECK || u == USE_TRUST; };
    b.plan_eligible = ts.plan_on && f4_sums(MODE) && held(scene_use) && held(rays_use) && p.lat_split == 0;
    if (b.plan_eligible) {
        b.plan_key = PlanKey{ PLAN_FORMAT, false, p.fast_b, group_shift(n_prims), p.width, p.reorder, n_rays, n_prims, ts.scene.gen, ts.rays.gen };
        // The sub-tile layout serves the unweighted fast kernel over full packets only; every other
        // call asks for format 3.  A format-3 plan (or none) that this very request has already
        // been answered with stands; otherwise the call asks for the sub-tile layout.
        b.plan_request = !weighted(MODE) && p.fast_b && p.width == 64 ? ts.plan_subtiles : 0;
        if (b.plan_request != 0) {
            const PacketPlan& pp = ts.plan;
            const bool answered = (pp.valid || pp.dead) && pp.key == b.plan_key && pp.asked == b.plan_request;
            b.plan_key.subtiles = !answered;
        }
    }
    // (a recorded plan of this key: the device-side gate decides whether this call re-records it)
    PlanGate gate;
    const bool plan_steady = b.plan_eligible && ts.plan.valid && ts.plan.key == b.plan_key;
    if (plan_steady) {
        gate.ctl = ts.plan.ctl; gate.scene = ts.scene.ctl; gate.rays = ts.rays.ctl;
    }
    const bool scene_sig = scene_use == USE_FILL || scene_use == USE_CHECK;
    const bool rays_sig = rays_use == USE_FILL || rays_use == USE_CHECK, sig = scene_sig || rays_sig;
    // The frame's layout: carve(base) takes the buffers from `base` and returns the bytes taken; over
    // base == nullptr it only counts, so the frame is sized by the same code that carves it.
    auto carve = [&](char* const base) {
        size_t used = 0;
        auto take = [&](auto*& ptr, const size_t count) {
            using T = std::remove_reference_t<decltype(*ptr)>;
            ptr = base ? reinterpret_cast<T*>(base + used) : nullptr;
            used += Workspace::aligned(count * sizeof(T));
        };
        if (sig) take(b.sig, sig_partial_words());
        if (!scene_cached) {
            take(b.A, n_prims + 4);
            if (f4_integrals(MODE)) take(b.B, n_prims + 4);
            if (MODE == MODE_TRI) take(b.T64, 9 * (n_prims + 4));
            take(b.node_prims, n_nodes); take(b.C, cluster_record_count(n_prims));
        }
        if (f4_sums(MODE)) take(b.partial, n_rays * SUM_CLASSES * channels(MODE));
        if (double_sums(MODE)) take(b.partial_d, n_rays * SUM_CLASSES);
        if (p.hits_split) {
            take(b.chunk_counts, n_rays * size_t(p.hit_chunks)); take(b.chunk_off, n_rays * size_t(p.hit_chunks));
            take(b.scratch_counts, n_rays); take(b.wave_map, p.hit_packets * p.hit_split); take(b.n_wave_map, 16);
            take(b.pk_prefix, p.hit_packets * size_t(p.hit_chunks));
            take(b.pk_total, p.hit_packets + 16); take(b.pk_first, p.hit_packets + 16); take(b.pk_parts, p.hit_packets + 16);
        }
        if (p.reorder) { take(b.ext, 20); take(b.keys, n_rays); take(b.perm, n_rays); }
        return used;
    };
    const size_t own = carve(nullptr);
    // (ray_order's sort carves its temporaries after these)
    const size_t need = own + (p.reorder ? sort_ws_bytes(n_rays, 4, 0) : 0);
    if (nested.measure) {   // (no cache assumed, room for the signatures a cached call adds)
        *nested.measure = need + Workspace::aligned(sig_partial_words() * sizeof(*b.sig));
        return GRACE_OK;
    }
    if (nested.on) GRACE_REQUIRE(Workspace::room() >= need, "trace: the caller's frame is too small for a nested trace");
    else GRACE_TRY(frame.begin(need, stream));
    carve(Workspace::take<char>(own));
    if (sig) {
        SigRequest rq;
        if (scene_sig) {
            rq.prims = a.spheres; rq.prims_bytes = n_prims * (MODE == MODE_TRI ? 36 : 16);
            rq.nodes = a.nodes; rq.nodes_bytes = n_nodes * 64;
            rq.leaves = a.leaves; rq.leaves_bytes = (n_nodes + 1) * 16;
            rq.scene_ctl = ts.scene.ctl; rq.scene_force = scene_use == USE_FILL;
        }
        if (rays_sig) {
            rq.rays = a.rays; rq.rays_bytes = n_rays * 28;
            rq.rays_ctl = ts.rays.ctl; rq.rays_force = rays_use == USE_FILL; rq.rays_ext = ts.rays.ext;
        }
        GRACE_TRY(launch_signatures(rq, b.sig, stream));
    }
    if (scene_cached) {
        Scene& sc = ts.scene;
        if (scene_use != USE_TRUST) {
            // (gated by the cache's stale flag: a first fill is forced stale)
            GRACE_TRY(scene_fill(skey.kind, a.spheres, n_prims, a.nodes, n_nodes, a.leaves, sc.A, sc.B1, sc.B50,
                                 sc.T64, sc.node_prims, sc.C, stream, &sc.ctl->stale));
            sc.valid = true;
        }
        a.A = sc.A; a.T64 = sc.T64; a.node_prims = sc.node_prims; a.C = sc.C;
        a.B = f4_integrals(MODE) ? (p.fast_b ? sc.B50 : sc.B1) : nullptr;
    } else {
        GRACE_TRY(scene_fill(skey.kind, primitive(MODE) == PRIM_D4 ? static_cast<const void*>(a.spheres_d) : a.spheres,
                             n_prims, a.nodes, n_nodes, a.leaves, b.A, p.fast_b ? nullptr : b.B, p.fast_b ? b.B : nullptr,
                             b.T64, b.node_prims, b.C, stream));
        a.A = b.A; a.B = b.B; a.T64 = b.T64; a.node_prims = b.node_prims; a.C = b.C;
    }
    if (p.reorder) {
        const float4* scene_min = a.C + 2 * ((n_prims + 63) / 64);
        uint32_t* lat_flag = p.lattice ? b.ext + 13 : nullptr;
        int* split_dev = p.dev_split ? reinterpret_cast<int*>(b.ext + 12) : nullptr;
        const int split_flags = f4_sums(MODE) ? SPLIT_WIDE_BUDGET : 0;
        if (rays_cached) {
            RayOrder& ro = ts.rays;
            if (rays_use != USE_TRUST) {
                // (gated by the cache's stale flag; the order lands in the cache's own buffers)
                GRACE_TRY(ray_order(a.rays, n_rays, ro.ext, b.keys, ro.perm, nullptr, nullptr, 0, 0, nullptr,
                                    stream, &ro.ctl->stale));
                ro.valid = true;
            }
            // cached order: only this call's device-side choices remain
            // (an unweighted call that may run from a plan, where the device chooses the split at all,
            // also gets the planned kernel's own: see planned_split.  Weighted calls keep one K: their
            // planned kernels run 3 to 8 waves per SIMD on LDS accumulators, and with four channels
            // the extra waves cost 6-13 % instead of saving time -- measured, see planned_split)
            int* plan_split_dev = b.plan_eligible && split_dev && !weighted(MODE)
                ? reinterpret_cast<int*>(b.ext + 16) : nullptr;
            if (lat_flag || split_dev || plan_steady)
                GRACE_TRY(launch_choose_variants(ro.ext, int(n_rays), scene_min, lat_flag, p.n_packets,
                                                 p.split | split_flags, split_dev, stream, plan_steady ? &gate : nullptr,
                                                 plan_split_dev));
            a.perm = ro.perm; a.plan_split_dev = plan_split_dev;
        } else {
            GRACE_TRY(ray_order(a.rays, n_rays, b.ext, b.keys, b.perm, scene_min, lat_flag, p.n_packets,
                                p.split | split_flags, split_dev, stream));
            a.perm = b.perm;
        }
        a.lat_dev = reinterpret_cast<const int*>(lat_flag); a.split_dev = split_dev;
    }
    return GRACE_OK;
}

// Both variants of a kernel with a lattice instantiation (the device flag lets one run).
template <int MODE, bool SPLIT, bool ALT = false>
void launch_walk(const int grid, const TraceArgs& args, hipStream_t stream)
{
    trace_kernel<MODE, SPLIT, ALT, false><<<grid, TRACE_BLOCK, 0, stream>>>(args);
    if constexpr (has_lattice(MODE))
        if (args.lat_dev) trace_kernel<MODE, SPLIT, ALT, true><<<grid, TRACE_BLOCK, 0, stream>>>(args);
}

// The walk of a planned call and the kernels around it.  kept: the chunk counts a hit-count call
// has kept for this per-hit trace (null: count them here).
template <int MODE>
grace_status dispatch(const TraceState& ts, const TraceArgs& a, const TraceBuffers& b, const LaunchPlan& p,
                      const int* kept, const size_t n_rays, hipStream_t stream)
{
    const int grid = ceil_div(size_t(p.n_packets) * p.split, TRACE_BLOCK / 64);
    // Upper levels of the class sum tree: k partial sums per ray (k_dev: the device's k, if set;
    // run_if: the kernel returns at once if *run_if == 0).  Counts are summed by atomics.
    // (a planned kernel with a split of its own: the pass takes that K if the plan's flag says it ran)
    const int* const plan_k_dev = a.plan_usable ? a.plan_split_dev : nullptr;
    auto combine = [&](const int k, const int* k_dev, const int* run_if) -> grace_status {
        const int g = ceil_div(n_rays * channels(MODE), 256);   // (one thread per ray and channel)
        if constexpr (double_sums(MODE))
            combine_classes_kernel<double><<<g, 256, 0, stream>>>(a.partial_d, int(n_rays), k, k_dev, a.out_sums_d, run_if);
        else if constexpr (weighted(MODE))
            combine_channel_classes_kernel<<<g, 256, 0, stream>>>(a.partial, int(n_rays), channels(MODE), k, k_dev,
                                                                  a.out_sums, a.out_stride, run_if,
                                                                  a.plan_usable, plan_k_dev);
        else if constexpr (f4_sums(MODE))
            combine_classes_kernel<float><<<g, 256, 0, stream>>>(a.partial, int(n_rays), k, k_dev, a.out_sums, run_if,
                                                                 a.plan_usable, plan_k_dev);
        else return GRACE_OK;
        GRACE_CHECK_LAUNCH();
        return GRACE_OK;
    };
    if constexpr (class_split(MODE)) {
        auto walk = [&](auto alt_tag) -> grace_status {
            constexpr bool ALT = decltype(alt_tag)::value;
            if constexpr (has_lattice(MODE)) if (p.lat_split) {   // one wave, or the LAT kernel split (see plan_launch)
                if (output(MODE) == OUT_COUNTS)
                    GRACE_TRY_HIP(hipMemsetAsync(a.out_counts, 0, n_rays * sizeof(int), stream));
                trace_kernel<MODE, false, ALT, false><<<grid, TRACE_BLOCK, 0, stream>>>(a);
                GRACE_CHECK_LAUNCH();
                TraceArgs a_lat = a;
                a_lat.split = p.lat_split; a_lat.split_dev = nullptr;
                trace_kernel<MODE, true, ALT, true><<<ceil_div(size_t(p.n_packets) * p.lat_split, TRACE_BLOCK / 64),
                                                      TRACE_BLOCK, 0, stream>>>(a_lat);
                GRACE_CHECK_LAUNCH();
                return combine(p.lat_split, nullptr, a.lat_dev);
            }
            if constexpr (f4_sums(MODE)) if (a.plan_usable) {
                // A call with a packet plan: the gated re-record, the planned kernel (always the
                // class-split one: with one wave per packet it leaves one partial sum per ray), then
                // the ordinary kernels; the plan's device flag lets one side run.
                GRACE_TRY(plan_record(ts, a, stream));
                // (its own grid where it has its own waves per packet.  The kernel takes its K from the
                // word choose_variants_kernel wrote, planned_split(p.n_packets) as well: the grid covers
                // every working wave only because host and device call the same function with the same
                // packet count -- a rule that looks at anything else must size this grid for its largest K)
                const int grid_planned = a.plan_split_dev
                    ? ceil_div(size_t(p.n_packets) * planned_split(p.n_packets), TRACE_BLOCK / 64) : grid;
                GRACE_TRY(launch_planned(MODE, ALT, ts.plan.key.subtiles, grid_planned, a, stream));
                if (p.split == 1) GRACE_TRY(combine(1, nullptr, reinterpret_cast<const int*>(a.plan_usable)));
            }
            if (p.split > 1) launch_walk<MODE, true, ALT>(grid, a, stream);
            else launch_walk<MODE, false, ALT>(grid, a, stream);
            return GRACE_OK;
        };
        if constexpr (f4_sums(MODE)) GRACE_TRY(p.fast_b ? walk(std::true_type()) : walk(std::false_type()));
        else GRACE_TRY(walk(std::false_type()));
    } else if constexpr (MODE == MODE_HITS) {
        if (p.hits_split) {
            // 1. hits per (ray, chunk): the counting walk, split by summation class -- unless the
            //    hit-count call made for this trace_sph has kept them (grace_trace_hitcounts_keep_f4)
            const int* counts = kept;
            if (!kept) {
                TraceArgs c = a;
                c.chunk_counts = b.chunk_counts; c.out_counts = b.scratch_counts;
                GRACE_TRY_HIP(hipMemsetAsync(b.chunk_counts, 0, n_rays * size_t(p.hit_chunks) * 4, stream));
                GRACE_TRY_HIP(hipMemsetAsync(b.scratch_counts, 0, n_rays * 4, stream));
                launch_walk<MODE_COUNT, true>(grid, c, stream);
                GRACE_CHECK_LAUNCH();
                counts = b.chunk_counts;
            }
            // 2. output offsets per (ray, chunk); the launched waves dealt to the packets by hit
            //    totals; each packet's chunks cut into its waves' ranges
            hits_offsets_kernel<<<ceil_div(n_rays, 4), 256, 0, stream>>>(counts, a.offsets, int(n_rays),
                                                                         p.hit_chunks, b.chunk_off);
            GRACE_CHECK_LAUNCH();
            hits_plan_kernel<<<p.n_packets, MAX_HIT_CHUNKS, 0, stream>>>(counts, a.perm, int(n_rays),
                                                                         p.hit_chunks, b.pk_prefix, b.pk_total);
            GRACE_CHECK_LAUNCH();
            hits_assign_kernel<<<1, 1024, 0, stream>>>(b.pk_total, p.n_packets, p.n_packets * p.split, p.hit_chunks,
                                                       b.pk_first, b.pk_parts, b.n_wave_map,
                                                       ts.hits_stage_split ? 200000ull : 0ull);
            GRACE_CHECK_LAUNCH();
            hits_bounds_kernel<<<p.n_packets, 64, 0, stream>>>(b.pk_prefix, b.pk_total, b.pk_first, b.pk_parts,
                                                               p.hit_chunks, b.wave_map);
            GRACE_CHECK_LAUNCH();
            // 3. the per-hit walk, wave w owning wave_map[w]'s range of chunks
            //    Heavy packets (output-bandwidth-bound: 10^5 isotropic rays through 10^6 large spheres,
            //    410 k hits per packet: 18.0 -> 11.0 ms) stage their hits in LDS and store them eight
            //    per ray at a time; light ones (61 M hits over 768 packets: 3.6 ms direct, 4.5 staged)
            //    store directly.  The hit total is known on the device only: BOTH variants are
            //    launched and the plan's flag (hits_assign_kernel) lets one of them run -- no read-back,
            //    no host synchronisation inside the call.
            TraceArgs staged = a, direct = a;
            staged.stage_dev = direct.stage_dev = b.n_wave_map + 4;
            staged.stage_want = 1; direct.stage_want = 0;
            launch_walk<MODE, true, true>(grid, staged, stream);
            GRACE_CHECK_LAUNCH();
            launch_walk<MODE, true, false>(grid, direct, stream);
        } else if (p.n_packets >= 4096) {
            launch_walk<MODE, false, true>(grid, a, stream);
        } else {
            launch_walk<MODE, false, false>(grid, a, stream);
        }
    } else {
        launch_walk<MODE, false>(grid, a, stream);
    }
    GRACE_CHECK_LAUNCH();
    GRACE_TRY(stamps_report(MODE));
    if (p.split > 1) GRACE_TRY(combine(p.split, a.split_dev, nullptr));
    return GRACE_OK;
}

template <int MODE>
grace_status launch_trace(TraceArgs a, size_t n_rays, size_t n_spheres, size_t n_nodes,
                          hipStream_t stream, const Nested nested = Nested())
{
    GRACE_REQUIRE(a.rays && a.spheres && a.nodes && a.leaves && a.root, "trace: null pointer");
    GRACE_REQUIRE(n_rays < (size_t(1) << 31), "trace: bad ray count");
    GRACE_REQUIRE(n_nodes >= 1 && n_nodes < (size_t(1) << 30), "trace: bad node count");
    GRACE_REQUIRE(n_spheres > 0 && n_spheres < (size_t(1) << 31), "trace: bad primitive count");
    TraceState* ts_ptr = nullptr;
    GRACE_TRY(trace_state(&ts_ptr));
    TraceState& ts = *ts_ptr;
    GRACE_TRY(ensure_status(ts, stream));
    a.kernel_table = ts.kernel_table;     // this call's table, whatever the context selects later
    const LaunchPlan p = plan_launch<MODE>(ts, a.keep_chunks, n_rays, n_spheres);
    const bool reuse_chunks = p.hits_split && ts.hits.valid && ts.hits.rays == a.rays
        && ts.hits.n_rays == n_rays && ts.hits.prims == static_cast<const void*>(a.spheres)
        && ts.hits.n_prims == n_spheres && ts.hits.n_chunks == p.hit_chunks;
    if (chunked(MODE)) ts.hits.valid = false;   // consumed, or stale from here on
    const size_t need = n_rays * size_t(p.hit_chunks);
    if (p.keep_chunks && ts.hits.capacity < need) {
        if (ts.hits.chunk_counts) { GRACE_TRY_HIP(hipDeviceSynchronize()); GRACE_TRY_HIP(hipFree(ts.hits.chunk_counts)); }
        ts.hits.chunk_counts = nullptr; ts.hits.capacity = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&ts.hits.chunk_counts), need * sizeof(int));
        if (e != hipSuccess) return set_error(GRACE_OUT_OF_MEMORY, __FILE__, __LINE__, hipGetErrorString(e));
        ts.hits.capacity = need;
    }
    FrameGuard frame;
    TraceBuffers b;
    GRACE_TRY(use_records<MODE>(ts, a, b, frame, p, n_rays, n_spheres, n_nodes, stream, nested));
    if (nested.measure) return GRACE_OK;
    a.width = p.width; a.split = p.split; a.treelet = p.treelet; a.treelet_axis = p.treelet_axis;
    a.n_rays = int(n_rays); a.n_nodes = int(n_nodes); a.n_prims = int(n_spheres); a.status = ts.status;
    a.group_shift = group_shift(n_spheres); a.chunk_shift = p.hit_chunk_shift; a.n_chunks = p.hit_chunks;
    a.partial = b.partial; a.partial_d = b.partial_d;
    a.chunk_off = b.chunk_off; a.wave_map = b.wave_map; a.n_wave_map = b.n_wave_map;
    if (p.split > 1 && output(MODE) == OUT_COUNTS)
        GRACE_TRY_HIP(hipMemsetAsync(a.out_counts, 0, n_rays * sizeof(int), stream));
    if (p.keep_chunks && p.split > 1) {
        a.chunk_counts = ts.hits.chunk_counts;
        GRACE_TRY_HIP(hipMemsetAsync(ts.hits.chunk_counts, 0, n_rays * size_t(p.hit_chunks) * 4, stream));
        ts.hits.valid = true; ts.hits.rays = a.rays; ts.hits.n_rays = n_rays;
        ts.hits.prims = a.spheres; ts.hits.n_prims = n_spheres; ts.hits.n_chunks = p.hit_chunks;
    }
    ts.last_lat_dev = a.lat_dev; ts.last_lat_stream = stream;
    if constexpr (f4_sums(MODE)) {
        // The packet plan: sized and recorded by the first call that both caches serve (one stream
        // synchronisation, where the caches' own fills have theirs), used from then on.
        PacketPlan& pp = ts.plan;
        if (b.plan_eligible && !(pp.key == b.plan_key && (pp.valid || pp.dead)))
            GRACE_TRY(plan_fill(ts, b.plan_key, b.plan_request, a, stream));
        // (a request for sub-tiles that the rule or the budget declined was answered with format 3)
        if (b.plan_eligible && (pp.valid || pp.dead) && pp.asked == b.plan_request) b.plan_key.subtiles = pp.key.subtiles;
        ts.last_plan_ctl = nullptr;
        if (b.plan_eligible && pp.valid && pp.key == b.plan_key) {
            a.plan_idx = pp.idx; a.plan_hdr = pp.hdr; a.plan_spans = pp.spans; a.plan_counts = pp.counts;
            a.plan_usable = &pp.ctl->usable;
            ts.last_plan_ctl = pp.ctl; ts.last_plan_stream = stream;
            ts.last_plan_fuses = !weighted(MODE) && p.fast_b;   // (the kernel that fuses: trace_kernel.hpp, FUSE)
        }
    }
    return timed(ts, stream, [&] {
        return dispatch<MODE>(ts, a, b, p, reuse_chunks ? ts.hits.chunk_counts : nullptr, n_rays, stream);
    });
}

// What every trace entry point passes the same way (a double4 trace also sets spheres_d; its
// `spheres` is checked for null only).
TraceArgs trace_args(const void* d_rays, const void* d_prims, const int* d_nodes, const int* d_leaves,
                     const int* d_root)
{
    TraceArgs a = {};
    a.rays = static_cast<const float*>(d_rays);
    a.spheres = static_cast<const float4*>(d_prims);
    a.nodes = reinterpret_cast<const float4*>(d_nodes);
    a.leaves = reinterpret_cast<const int4*>(d_leaves);
    a.root = d_root;
    return a;
}

} // namespace

namespace grace_hip {
// Called by this library's entry points that WRITE caller arrays (sort payloads, tree builds):
// a prepared scene over that array is stale from here on.
grace_status rays_invalidate_if_written(const void* d_written)
{
    Context* c = nullptr;
    GRACE_TRY(current_context(&c));
    if (!c->trace) return GRACE_OK;
    TraceState& ts = *c->trace;
    if (ts.cache_validation) return GRACE_OK;     // validated before every use: nothing to drop eagerly
    if (ts.rays.valid && d_written && d_written == static_cast<const void*>(ts.rays.key.rays)) return rays_release(ts);
    return GRACE_OK;
}

grace_status scene_invalidate_if_written(const void* d_written)
{
    Context* c = nullptr;
    GRACE_TRY(current_context(&c));
    if (!c->trace) return GRACE_OK;
    TraceState& ts = *c->trace;
    if (ts.cache_validation) return GRACE_OK;
    if (ts.scene.valid && d_written
        && (d_written == ts.scene.key.prims || d_written == ts.scene.key.nodes || d_written == ts.scene.key.leaves))
        return scene_release(ts);
    return GRACE_OK;
}

// Hit counts / per-hit outputs of a ray range inside the caller's open frame (see Nested).
grace_status trace_nested_bytes(size_t n_rays, size_t n_spheres, size_t n_nodes, size_t* bytes)
{
    // (never dereferenced: measuring returns before any launch)
    TraceArgs a = trace_args(bytes, bytes, reinterpret_cast<const int*>(bytes), reinterpret_cast<const int*>(bytes),
                             reinterpret_cast<const int*>(bytes));
    size_t counts = 0, hits = 0;
    GRACE_TRY(launch_trace<MODE_COUNT>(a, n_rays, n_spheres, n_nodes, nullptr, Nested{true, &counts}));
    GRACE_TRY(launch_trace<MODE_HITS>(a, n_rays, n_spheres, n_nodes, nullptr, Nested{true, &hits}));
    *bytes = counts > hits ? counts : hits;
    return GRACE_OK;
}

grace_status trace_hitcounts_nested(const void* d_rays, size_t n_rays, const float* d_spheres, size_t n_spheres,
                                    const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root,
                                    int* d_hit_counts, hipStream_t stream)
{
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.out_counts = d_hit_counts;
    return launch_trace<MODE_COUNT>(a, n_rays, n_spheres, n_nodes, stream, Nested{true, nullptr});
}

grace_status trace_hits_nested(const void* d_rays, size_t n_rays, const float* d_spheres, size_t n_spheres,
                               const int* d_nodes, size_t n_nodes, const int* d_leaves, const int* d_root,
                               const int* d_ray_offsets, int* d_hit_indices, float* d_hit_integrals,
                               float* d_hit_distances, hipStream_t stream)
{
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.offsets = d_ray_offsets;
    a.hit_idx = d_hit_indices;
    a.hit_integral = d_hit_integrals;
    a.hit_dist = d_hit_distances;
    return launch_trace<MODE_HITS>(a, n_rays, n_spheres, n_nodes, stream, Nested{true, nullptr});
}
} // namespace grace_hip

extern "C" {

grace_status grace_trace_hitcounts_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                      size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                      const int* d_leaves, const int* d_root,
                                      int* d_hit_counts, grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_hit_counts, "trace_hitcounts: null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.out_counts = d_hit_counts;
    return launch_trace<MODE_COUNT>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_trace_hitcounts_keep_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                           size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                           const int* d_leaves, const int* d_root,
                                           int* d_hit_counts, grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_hit_counts, "trace_hitcounts: null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.out_counts = d_hit_counts;
    a.keep_chunks = true;
    return launch_trace<MODE_COUNT>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_trace_cumulative_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                       size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                       const int* d_leaves, const int* d_root,
                                       float* d_cumulated, grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_cumulated, "trace_cumulative: null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.out_sums = d_cumulated;
    return launch_trace<MODE_CUMULATIVE>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

// Weighted column densities (an extension): channels in groups of up to MAX_LAUNCH_CHANNELS, one
// walk per group.
grace_status grace_trace_cumulative_weighted_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                                size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                                const int* d_leaves, const int* d_root,
                                                const float* d_weights, int n_channels, float* d_out,
                                                grace_stream stream)
{
    GRACE_REQUIRE(n_channels >= 1 && n_channels <= 64, "trace_cumulative_weighted: channels must be 1..64");
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_weights || n_spheres == 0, "trace_cumulative_weighted: null weights");
    GRACE_REQUIRE(d_out, "trace_cumulative_weighted: null output");
    GRACE_REQUIRE(n_rays * size_t(n_channels) < (size_t(1) << 31), "trace_cumulative_weighted: too many outputs");
    for (int g = 0; g < n_channels; g += MAX_LAUNCH_CHANNELS) {
        TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
        a.weights = d_weights + g;
        a.w_stride = n_channels;
        a.out_sums = d_out + g;
        a.out_stride = n_channels;
        const hipStream_t s = as_stream(stream);
        switch (n_channels - g < MAX_LAUNCH_CHANNELS ? n_channels - g : MAX_LAUNCH_CHANNELS) {
        case 1: GRACE_TRY(launch_trace<MODE_WCUM1>(a, n_rays, n_spheres, n_nodes, s)); break;
        case 2: GRACE_TRY(launch_trace<MODE_WCUM2>(a, n_rays, n_spheres, n_nodes, s)); break;
        case 3: GRACE_TRY(launch_trace<MODE_WCUM3>(a, n_rays, n_spheres, n_nodes, s)); break;
        default: GRACE_TRY(launch_trace<MODE_WCUM4>(a, n_rays, n_spheres, n_nodes, s)); break;
        }
    }
    return GRACE_OK;
}

grace_status grace_trace_hits_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                 size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                 const int* d_leaves, const int* d_root,
                                 const int* d_ray_offsets, int* d_hit_indices,
                                 float* d_hit_integrals, float* d_hit_distances,
                                 grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_ray_offsets && d_hit_indices && d_hit_integrals && d_hit_distances,
                  "trace_hits: null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.offsets = d_ray_offsets;
    a.hit_idx = d_hit_indices;
    a.hit_integral = d_hit_integrals;
    a.hit_dist = d_hit_distances;
    return launch_trace<MODE_HITS>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_trace_closest_tri(const void* d_rays, size_t n_rays, const float* d_tris,
                                     size_t n_tris, const int* d_nodes, size_t n_nodes,
                                     const int* d_leaves, const int* d_root, int* d_closest,
                                     grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_closest, "trace_closest_tri: null output");
    TraceArgs a = trace_args(d_rays, d_tris, d_nodes, d_leaves, d_root);   // (9 floats per triangle)
    a.out_counts = d_closest;
    return launch_trace<MODE_TRI>(a, n_rays, n_tris, n_nodes, as_stream(stream));
}

// ---- double4 spheres (Real4 = double4, Real = double) ----------------------------------------
grace_status grace_trace_hitcounts_d4(const void* d_rays, size_t n_rays, const double* d_spheres,
                                      size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                      const int* d_leaves, const int* d_root, int* d_hit_counts,
                                      grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_hit_counts, "trace_hitcounts (double4): null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.spheres_d = d_spheres;
    a.out_counts = d_hit_counts;
    return launch_trace<MODE_COUNT_D4>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_trace_cumulative_d4(const void* d_rays, size_t n_rays, const double* d_spheres,
                                       size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                       const int* d_leaves, const int* d_root, double* d_sums,
                                       grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_sums, "trace_cumulative (double4): null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.spheres_d = d_spheres;
    a.out_sums_d = d_sums;
    return launch_trace<MODE_CUM_D4>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_trace_hits_d4(const void* d_rays, size_t n_rays, const double* d_spheres,
                                 size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                 const int* d_leaves, const int* d_root, const int* d_ray_offsets,
                                 int* d_hit_indices, double* d_hit_integrals,
                                 double* d_hit_distances, grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_ray_offsets && d_hit_indices && d_hit_integrals && d_hit_distances,
                  "trace_hits (double4): null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.spheres_d = d_spheres;
    a.offsets = d_ray_offsets;
    a.hit_idx = d_hit_indices;
    a.hit_integral_d = d_hit_integrals;
    a.hit_dist_d = d_hit_distances;
    return launch_trace<MODE_HITS_D4>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_trace_status_d4(grace_stream stream) { return grace_trace_status(stream); }

// ---- float4 spheres, double outputs (Real4 = float4, Real = double) ---------------------------
grace_status grace_trace_hitcounts_f4_f64(const void* d_rays, size_t n_rays, const float* d_spheres,
                                          size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                          const int* d_leaves, const int* d_root, int* d_hit_counts,
                                          grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_hit_counts, "trace_hitcounts (float4, double): null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.out_counts = d_hit_counts;
    return launch_trace<MODE_COUNT_F4D>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_trace_cumulative_f4_f64(const void* d_rays, size_t n_rays, const float* d_spheres,
                                           size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                           const int* d_leaves, const int* d_root, double* d_sums,
                                           grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_sums, "trace_cumulative (float4, double): null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.out_sums_d = d_sums;
    return launch_trace<MODE_CUM_F4D>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_trace_hits_f4_f64(const void* d_rays, size_t n_rays, const float* d_spheres,
                                     size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                     const int* d_leaves, const int* d_root, const int* d_ray_offsets,
                                     int* d_hit_indices, double* d_hit_integrals,
                                     double* d_hit_distances, grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;
    GRACE_REQUIRE(d_ray_offsets && d_hit_indices && d_hit_integrals && d_hit_distances,
                  "trace_hits (float4, double): null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.offsets = d_ray_offsets;
    a.hit_idx = d_hit_indices;
    a.hit_integral_d = d_hit_integrals;
    a.hit_dist_d = d_hit_distances;
    return launch_trace<MODE_HITS_F4D>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_trace_stats_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                  size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                  const int* d_leaves, const int* d_root,
                                  uint32_t* d_stats4, grace_stream stream)
{
    if (n_rays == 0) return GRACE_OK;   // an empty shard of a sharded batch: nothing to trace
    GRACE_REQUIRE(d_stats4, "trace_stats: null output");
    TraceArgs a = trace_args(d_rays, d_spheres, d_nodes, d_leaves, d_root);
    a.stats = d_stats4;
    return launch_trace<MODE_STATS>(a, n_rays, n_spheres, n_nodes, as_stream(stream));
}

grace_status grace_hit_integrals_f32(const float* d_b2, const float* d_h, size_t n, float* d_out,
                                     grace_stream stream)
{
    GRACE_REQUIRE(n == 0 || (d_b2 && d_h && d_out), "hit_integrals: null pointer");
    if (n == 0) return GRACE_OK;
    TraceState* ts = nullptr;
    GRACE_TRY(trace_state(&ts));
    hit_integrals_kernel<<<stream_grid(n, 256), 256, 0, as_stream(stream)>>>(d_b2, d_h, n, d_out,
                                                                             ts->kernel_table);
    GRACE_CHECK_LAUNCH();
    return GRACE_OK;
}

grace_status grace_sph_kernel_table(int kind, double* h_out51)
{
    GRACE_REQUIRE(kind >= GRACE_SPH_KERNEL_CUBIC && kind <= GRACE_SPH_KERNEL_WENDLAND_C6,
                  "sph_kernel_table: kind must be a built-in GRACE_SPH_KERNEL_* (0..5)");
    GRACE_REQUIRE(h_out51, "sph_kernel_table: null output");
    for (int i = 0; i < N_TABLE; ++i) h_out51[i] = k_sph_kernel_tables[kind][i];
    return GRACE_OK;
}

// The calling thread's TraceState as `ts` (entry-point boilerplate).
#define GRACE_TRACE_STATE()                                                                      \
    TraceState* ts_ptr_ = nullptr;                                                               \
    GRACE_TRY(trace_state(&ts_ptr_));                                                            \
    TraceState& ts = *ts_ptr_

grace_status grace_trace_prepare_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                    size_t n_nodes, const int* d_leaves, grace_stream stream)
{
    GRACE_TRACE_STATE();
    return scene_prepare(ts, PRIM_F4, d_spheres, n_spheres, d_nodes, n_nodes, d_leaves, as_stream(stream));
}

grace_status grace_trace_prepare_tri(const float* d_tris, size_t n_tris, const int* d_nodes,
                                     size_t n_nodes, const int* d_leaves, grace_stream stream)
{
    GRACE_TRACE_STATE();
    return scene_prepare(ts, PRIM_TRI, d_tris, n_tris, d_nodes, n_nodes, d_leaves, as_stream(stream));
}

grace_status grace_trace_prepare_rays(const void* d_rays, size_t n_rays, grace_stream stream)
{
    GRACE_TRACE_STATE();
    return rays_prepare(ts, static_cast<const float*>(d_rays), n_rays, as_stream(stream));
}

grace_status grace_trace_release_rays(void)
{
    GRACE_TRACE_STATE();
    GRACE_TRY(plan_release(ts));
    return rays_release(ts);
}

grace_status grace_trace_release(void)
{
    GRACE_TRACE_STATE();
    if (ts.hits.chunk_counts) {
        GRACE_TRY_HIP(hipDeviceSynchronize());
        GRACE_TRY_HIP(hipFree(ts.hits.chunk_counts));
    }
    ts.hits = HitsCache();
    GRACE_TRY(plan_release(ts));
    return scene_release(ts);
}

grace_status grace_trace_enable_timing(int enabled)
{
    GRACE_TRACE_STATE();
    ts.timing = enabled != 0;
    ts.ev_valid = false;
    return GRACE_OK;
}

grace_status grace_trace_last_kernel_ms(float* h_ms)
{
    GRACE_REQUIRE(h_ms, "null output");
    GRACE_TRACE_STATE();
    GRACE_REQUIRE(ts.timing && ts.ev_valid, "no timed traversal launch recorded");
    GRACE_TRY_HIP(hipEventSynchronize(ts.ev1));
    GRACE_TRY_HIP(hipEventElapsedTime(h_ms, ts.ev0, ts.ev1));
    return GRACE_OK;
}

grace_status grace_trace_last_lattice(int* h_lattice)
{
    GRACE_REQUIRE(h_lattice, "null output");
    *h_lattice = 0;
    GRACE_TRACE_STATE();
    if (ts.last_lat_dev) {
        GRACE_TRY_HIP(hipStreamSynchronize(ts.last_lat_stream));
        GRACE_TRY_HIP(hipMemcpy(h_lattice, ts.last_lat_dev, sizeof(int), hipMemcpyDeviceToHost));
    }
    return GRACE_OK;
}

grace_status grace_trace_last_plan_used(int* h_used)
{
    GRACE_REQUIRE(h_used, "null output");
    *h_used = 0;
    GRACE_TRACE_STATE();
    if (ts.last_plan_ctl) {
        PlanCtl h = {};
        GRACE_TRY_HIP(hipStreamSynchronize(ts.last_plan_stream));
        GRACE_TRY_HIP(hipMemcpy(&h, ts.last_plan_ctl, sizeof(h), hipMemcpyDeviceToHost));
        *h_used = h.usable != 0u ? 1 : 0;
    }
    return GRACE_OK;
}

grace_status grace_trace_plan_stats(unsigned long long* h_stats)
{
    GRACE_REQUIRE(h_stats, "null output");
    for (int k = 0; k < 7; ++k) h_stats[k] = 0;
    GRACE_TRACE_STATE();
    if (ts.last_plan_ctl) {
        PlanCtl h = {};
        GRACE_TRY_HIP(hipStreamSynchronize(ts.last_plan_stream));
        GRACE_TRY_HIP(hipMemcpy(&h, ts.last_plan_ctl, sizeof(h), hipMemcpyDeviceToHost));
        if (h.usable != 0u) {
            for (int k = 0; k < 6; ++k) h_stats[k] = h.stats[k];
            h_stats[6] = h.largest_round;
        }
    }
    return GRACE_OK;
}

grace_status grace_trace_plan_loops(unsigned long long* h_loops)
{
    GRACE_REQUIRE(h_loops, "null output");
    h_loops[0] = h_loops[1] = 0;
    GRACE_TRACE_STATE();
    if (ts.last_plan_ctl) {
        PlanCtl h = {};
        GRACE_TRY_HIP(hipStreamSynchronize(ts.last_plan_stream));
        GRACE_TRY_HIP(hipMemcpy(&h, ts.last_plan_ctl, sizeof(h), hipMemcpyDeviceToHost));
        if (h.usable != 0u) {
            // (a kernel that does not fuse runs one loop per dense round)
            h_loops[0] = ts.last_plan_fuses ? h.loops : h.stats[2];
            h_loops[1] = ts.last_plan_fuses ? h.largest_loop : h.largest_round;
        }
    }
    return GRACE_OK;
}

grace_status grace_trace_set_plan(int on)
{
    GRACE_TRACE_STATE();
    ts.plan_on = on != 0;
    if (!ts.plan_on) GRACE_TRY(plan_release(ts));
    return GRACE_OK;
}

grace_status grace_trace_set_plan_budget(size_t bytes)
{
    GRACE_TRACE_STATE();
    ts.plan_budget = bytes;
    GRACE_TRY(plan_release(ts));    // (sized again, under the new budget, by the next call it can serve)
    return GRACE_OK;
}

grace_status grace_trace_set_plan_subtiles(int mode)
{
    GRACE_REQUIRE(mode >= -1 && mode <= 1, "plan sub-tiles: -1 (automatic), 0 (never) or 1 (whenever eligible)");
    GRACE_TRACE_STATE();
    if (ts.plan_subtiles != mode) GRACE_TRY(plan_release(ts));   // (sized again, in the layout the next call asks for)
    ts.plan_subtiles = mode;
    return GRACE_OK;
}

grace_status grace_trace_plan_subtiles(int* h_used, unsigned long long* h_steps, unsigned long long* h_slots)
{
    GRACE_REQUIRE(h_used && h_steps && h_slots, "null output");
    *h_used = 0; *h_steps = 0; *h_slots = 0;
    GRACE_TRACE_STATE();
    if (ts.last_plan_ctl && ts.plan.valid && ts.plan.key.subtiles) {
        PlanCtl h = {};
        GRACE_TRY_HIP(hipStreamSynchronize(ts.last_plan_stream));
        GRACE_TRY_HIP(hipMemcpy(&h, ts.last_plan_ctl, sizeof(h), hipMemcpyDeviceToHost));
        if (h.usable != 0u) { *h_used = 1; *h_steps = h.sub_steps; *h_slots = h.sub_slots; }
    }
    return GRACE_OK;
}

grace_status grace_trace_plan_bytes(size_t* h_bytes)
{
    GRACE_REQUIRE(h_bytes, "null output");
    GRACE_TRACE_STATE();
    const PacketPlan& pp = ts.plan;
    *h_bytes = pp.valid ? pp.bytes() : 0;
    return GRACE_OK;
}

grace_status grace_trace_set_packet_split(int waves_per_packet)
{
    GRACE_REQUIRE(waves_per_packet == -1 || waves_per_packet == 1 || waves_per_packet == 2
                      || waves_per_packet == 4 || waves_per_packet == 8,
                  "packet split must be 1, 2, 4, 8 or -1 (automatic)");
    GRACE_TRACE_STATE();
    ts.split = waves_per_packet;
    return GRACE_OK;
}

grace_status grace_trace_set_packet_width(int rays_per_packet)
{
    GRACE_REQUIRE(rays_per_packet == -1 || rays_per_packet == 16 || rays_per_packet == 32
                      || rays_per_packet == 64,
                  "packet width must be 16, 32, 64 or -1 (automatic)");
    GRACE_TRACE_STATE();
    ts.width = rays_per_packet;
    return GRACE_OK;
}

grace_status grace_trace_set_exact_integrals(int enabled)
{
    GRACE_TRACE_STATE();
    ts.exact_integrals = enabled != 0;
    return GRACE_OK;
}

grace_status grace_trace_set_sph_kernel(int kind)
{
    GRACE_REQUIRE(kind >= GRACE_SPH_KERNEL_CUBIC && kind <= GRACE_SPH_KERNEL_WENDLAND_C6,
                  "set_sph_kernel: kind must be a built-in GRACE_SPH_KERNEL_* (0..5); a custom table is "
                  "set with grace_trace_set_sph_kernel_table");
    GRACE_TRACE_STATE();
    ts.sph_kernel = kind;
    ts.kernel_table = ts.builtin_tables + kind * N_TABLE;
    return GRACE_OK;
}

grace_status grace_trace_set_sph_kernel_table(const double* h_table, int n)
{
    GRACE_REQUIRE(h_table && n == N_TABLE, "set_sph_kernel_table: the table must hold 51 values");
    for (int i = 0; i < N_TABLE; ++i)
        GRACE_REQUIRE(std::isfinite(h_table[i]) && h_table[i] >= 0.0,
                      "set_sph_kernel_table: every value must be finite and >= 0");
    GRACE_REQUIRE(h_table[N_TABLE - 1] == 0.0, "set_sph_kernel_table: the last value (b = H) must be 0");
    GRACE_TRACE_STATE();
    // Calls already queued may read the buffer: let them finish before it is overwritten.
    GRACE_TRY_HIP(hipDeviceSynchronize());
    if (!ts.custom_table)
        GRACE_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&ts.custom_table), N_TABLE * sizeof(double)));
    GRACE_TRY_HIP(hipMemcpy(ts.custom_table, h_table, N_TABLE * sizeof(double), hipMemcpyHostToDevice));
    for (int i = 0; i < N_TABLE; ++i) ts.custom_host[i] = h_table[i];
    ts.sph_kernel = GRACE_SPH_KERNEL_CUSTOM;
    ts.kernel_table = ts.custom_table;
    return GRACE_OK;
}

grace_status grace_trace_get_sph_kernel(int* h_kind, double* h_table51)
{
    GRACE_TRACE_STATE();
    if (h_kind) *h_kind = ts.sph_kernel;
    if (h_table51) {
        const double* t = ts.sph_kernel == GRACE_SPH_KERNEL_CUSTOM ? ts.custom_host
                                                                   : k_sph_kernel_tables[ts.sph_kernel];
        for (int i = 0; i < N_TABLE; ++i) h_table51[i] = t[i];
    }
    return GRACE_OK;
}

grace_status grace_trace_set_treelet_size(int max_primitives)
{
    GRACE_REQUIRE(max_primitives >= -1, "treelet size must be >= 0 (or -1 for automatic)");
    GRACE_TRACE_STATE();
    ts.treelet = max_primitives;
    return GRACE_OK;
}

grace_status grace_trace_set_ray_reorder(int enabled)
{
    GRACE_TRACE_STATE();
    ts.ray_reorder = enabled != 0;
    return GRACE_OK;
}

grace_status grace_trace_set_cache_validation(int enabled)
{
    GRACE_TRACE_STATE();
    ts.cache_validation = enabled != 0;
    return GRACE_OK;
}

grace_status grace_trace_set_cache_auto(int enabled)
{
    GRACE_TRACE_STATE();
    ts.cache_auto = enabled != 0;
    if (!ts.cache_auto) {     // what was cached automatically goes; pinned (prepared) records stay
        if ((ts.scene.valid && !ts.scene.pinned) || (ts.rays.valid && !ts.rays.pinned)) GRACE_TRY(plan_release(ts));
        if (ts.scene.valid && !ts.scene.pinned) GRACE_TRY(scene_release(ts));
        if (ts.rays.valid && !ts.rays.pinned) GRACE_TRY(rays_release(ts));
        ts.scene.seen = SceneKey();
        ts.rays.seen = RayKey();
    }
    return GRACE_OK;
}

grace_status grace_trace_set_lattice_split(int waves_per_packet)
{
    GRACE_REQUIRE(waves_per_packet == 0 || waves_per_packet == 2 || waves_per_packet == 4
                      || waves_per_packet == 8,
                  "lattice split must be 0 (one wave per packet), 2, 4 or 8");
    GRACE_TRACE_STATE();
    ts.lat_split = waves_per_packet;
    return GRACE_OK;
}

grace_status grace_trace_set_hits_staging(int enabled)
{
    GRACE_TRACE_STATE();
    ts.hits_stage_split = enabled != 0;
    return GRACE_OK;
}

grace_status grace_trace_status(grace_stream stream)
{
    GRACE_TRACE_STATE();
    if (!ts.status) return GRACE_OK;
    int h = 0;
    GRACE_TRY_HIP(hipMemcpyAsync(&h, ts.status, sizeof(int), hipMemcpyDeviceToHost,
                                 as_stream(stream)));
    GRACE_TRY_HIP(hipStreamSynchronize(as_stream(stream)));
    if (h != 0) {
        GRACE_TRY_HIP(hipMemsetAsync(ts.status, 0, sizeof(int), as_stream(stream)));
        if (h == GRACE_INVALID_ARGUMENT)
            return set_error(GRACE_INVALID_ARGUMENT, __FILE__, __LINE__,
                             "range_neighbours: a row of d_offsets does not have the length of its list");
        return set_error(GRACE_STACK_OVERFLOW, __FILE__, __LINE__,
                         "trace: packet stack (128 entries) exhausted");
    }
    return GRACE_OK;
}

} // extern "C"
