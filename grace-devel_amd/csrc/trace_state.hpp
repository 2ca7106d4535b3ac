// Shared declarations of the traversal's translation units -- trace.hip (the kernel's
// instantiations, launch logic, entry points), trace_prepass.hip (scene-constant records) and
// trace_coherence.hip (ray coherence order): modes, the kernel's argument block, and the state a
// Context keeps between trace calls (status word, knobs, timing events, cached scene records and
// ray order).
#pragma once

#include "common.hpp"

namespace grace_hip {

constexpr int TRACE_BLOCK = 256;
constexpr int N_TABLE = 51;
// Flag on the `launched` argument of the device-side split choice: column densities let a second
// wave per packet work up to 32768 waves (hit counts: 16384).
constexpr int SPLIT_WIDE_BUDGET = 0x100;

// Cluster records C of a scene of n primitives (float4 units): {lo, hi} per cluster of 64
// consecutive primitives, one tail record (the scene's smallest r^2 and the node_prims flag), then
// {lo, hi} per GROUP of 2^group_shift(n) consecutive primitives -- the union of its clusters'
// boxes; at most 4096 groups, of 4096 primitives each up to 16.7 M primitives.  Axis-aligned
// packets of the hit-count / column-density traces test the groups' boxes, 64 per lane-parallel
// pass, instead of walking the tree down to subtrees of that size (trace_kernel.hpp).
inline int group_shift(size_t n_prims)
{
    int s = 12;
    while (((n_prims + (size_t(1) << s) - 1) >> s) > 4096) ++s;
    return s;
}
inline size_t group_count(size_t n_prims)
{
    const int s = group_shift(n_prims);
    return (n_prims + (size_t(1) << s) - 1) >> s;
}
inline size_t cluster_record_count(size_t n_prims)
{
    return 2 * ((n_prims + 63) / 64) + 1 + 2 * group_count(n_prims);
}
constexpr int MAX_HIT_CHUNKS = 256; // chunk ranges of the split per-hit trace
constexpr int SUM_CLASSES = 8;   // summation classes (leaves of the pairwise sum tree)
constexpr int GRANULE_SHIFT = 10; // 1024 consecutive primitives share a class


enum { MODE_COUNT = 0, MODE_CUMULATIVE = 1, MODE_HITS = 2, MODE_STATS = 3, MODE_TRI = 4,
       // Real4 = double4, Real = double (trace_sph.cuh:57-241 instantiated in double): the walk and
       // every cull run on float records that CONTAIN the double spheres; each survivor is then
       // tested and integrated in double against the caller's double4 record.
       MODE_COUNT_D4 = 5, MODE_CUM_D4 = 6, MODE_HITS_D4 = 7,
       // Real4 = float4, Real = double (mixed precision): the same walk on float records that
       // contain every sphere the fp64 test can accept (trace_prepass_f4d_kernel); each survivor is
       // tested in double from the caller's float4 record, its per-hit terms follow the reference's
       // promotions for that pair, and column densities are the class-ordered double sum.
       MODE_COUNT_F4D = 8, MODE_CUM_F4D = 9, MODE_HITS_F4D = 10,
       // Weighted column densities (an extension the reference lacks): float4 spheres, 1 to 4
       // channels per launch, channel c of a ray = the class-ordered fp32 sum of fl(w[i][c] I_i).
       MODE_WCUM1 = 11, MODE_WCUM2 = 12, MODE_WCUM3 = 13, MODE_WCUM4 = 14 };

// What a mode does is its primitive and its output; every choice that depends on the mode is made
// from these two (or the properties below), never from a list of modes.
// The primitive is also the kind of scene records the pre-pass derives (SceneKey, scene_fill).
enum Primitive { PRIM_F4 = 0,    // float4 spheres
                 PRIM_TRI = 1,   // triangles, 9 floats each
                 PRIM_D4 = 2,    // double4 spheres
                 PRIM_F4D = 3 }; // float4 spheres, double results
enum Output { OUT_COUNTS, OUT_SUMS, OUT_HITS, OUT_STATS, OUT_CLOSEST,
              OUT_WSUMS };   // per-channel sums of weighted terms (TraceArgs::weights)

struct ModeParts { Primitive prim; Output out; int channels = 1; };
constexpr ModeParts mode_parts(const int mode)
{
    switch (mode) {
    case MODE_COUNT:      return { PRIM_F4, OUT_COUNTS };
    case MODE_CUMULATIVE: return { PRIM_F4, OUT_SUMS };
    case MODE_HITS:       return { PRIM_F4, OUT_HITS };
    case MODE_STATS:      return { PRIM_F4, OUT_STATS };
    case MODE_TRI:        return { PRIM_TRI, OUT_CLOSEST };
    case MODE_COUNT_D4:   return { PRIM_D4, OUT_COUNTS };
    case MODE_CUM_D4:     return { PRIM_D4, OUT_SUMS };
    case MODE_HITS_D4:    return { PRIM_D4, OUT_HITS };
    case MODE_COUNT_F4D:  return { PRIM_F4D, OUT_COUNTS };
    case MODE_CUM_F4D:    return { PRIM_F4D, OUT_SUMS };
    case MODE_HITS_F4D:   return { PRIM_F4D, OUT_HITS };
    case MODE_WCUM1:      return { PRIM_F4, OUT_WSUMS, 1 };
    case MODE_WCUM2:      return { PRIM_F4, OUT_WSUMS, 2 };
    case MODE_WCUM3:      return { PRIM_F4, OUT_WSUMS, 3 };
    case MODE_WCUM4:      return { PRIM_F4, OUT_WSUMS, 4 };
    }
    __builtin_unreachable();   // (a mode missing above is no constant expression: trace_kernel fails to compile)
}
constexpr Primitive primitive(const int mode) { return mode_parts(mode).prim; }
constexpr Output output(const int mode) { return mode_parts(mode).out; }
// Output channels of a launch (weighted sums: 1 to 4; every other output: 1).
constexpr int channels(const int mode) { return mode_parts(mode).channels; }
constexpr int MAX_LAUNCH_CHANNELS = 4;
constexpr bool weighted(const int mode) { return output(mode) == OUT_WSUMS; }

// Each survivor is tested, and its results formed, in double from the caller's record (the walk
// and every cull run on float records that contain those spheres).
constexpr bool fp64(const int mode) { return primitive(mode) == PRIM_D4 || primitive(mode) == PRIM_F4D; }
// Hit counts and column densities: summed by class, so a packet splits among waves by class.
constexpr bool class_split(const int mode)
{
    return output(mode) == OUT_COUNTS || output(mode) == OUT_SUMS || output(mode) == OUT_WSUMS;
}
// ... of float4 spheres: compacted survivor tiles, and the device-side choice of the working waves.
constexpr bool f4_class_split(const int mode) { return class_split(mode) && primitive(mode) == PRIM_F4; }
// Column densities (weighted or not) of float4 spheres: fp32 class sums (the fast integral, split
// partials in float).
constexpr bool f4_sums(const int mode)
{
    return primitive(mode) == PRIM_F4 && (output(mode) == OUT_SUMS || output(mode) == OUT_WSUMS);
}
// Column densities whose class sums are kept in double.
constexpr bool double_sums(const int mode) { return output(mode) == OUT_SUMS && fp64(mode); }
// A ray's result depends on the order its hits are met in (per-hit lists, closest hit): the packet
// walks the tree in one wave.
constexpr bool ordered(const int mode) { return output(mode) == OUT_HITS || output(mode) == OUT_CLOSEST; }
// Kernel line integrals (the kernel table).
constexpr bool integrates(const int mode)
{
    return output(mode) == OUT_SUMS || output(mode) == OUT_WSUMS || output(mode) == OUT_HITS;
}
// ... in fp32: the 1/h records B, and the alternative (ALT) instantiations.
constexpr bool f4_integrals(const int mode) { return integrates(mode) && primitive(mode) == PRIM_F4; }
// Modes with an origin-lattice (LAT) instantiation.
constexpr bool has_lattice(const int mode) { return primitive(mode) == PRIM_F4 && output(mode) != OUT_STATS; }
// Per-(ray, chunk) hit bookkeeping of the split per-hit trace: its own walk, and the hit-count walk
// that counts for it (HitsCache).
constexpr bool chunked(const int mode)
{
    return primitive(mode) == PRIM_F4 && (output(mode) == OUT_COUNTS || output(mode) == OUT_HITS);
}

struct TraceArgs {
    const float* rays;      // 7 floats per ray
    const uint32_t* perm;   // packet slot -> ray index (coherence order), or null
    int n_rays;
    const float4* spheres;
    const int2* node_prims; // pre-pass: per node {first primitive, primitive count}
    int treelet;            // nodes with <= treelet primitives are swept as one leaf (0: off)
    int treelet_axis;       // the same for axis-aligned packets (whose cluster test is much sharper)
    const float4* A;        // pre-pass: {x, y, z, h*h}, padded by 4 entries
    const float2* B;        // pre-pass: {1/h, (1/h)^2}, padded by 4 entries
    int group_shift;        // primitives per group box = 2^group_shift (see cluster_record_count)
    const float4* C;        // pre-pass: per CLUSTER (64 consecutive primitives) {lo.xyz, -}, {hi.xyz, -}:
                            // the box of the member spheres, slightly inflated (cluster_boxes_kernel)
    const double* T64;      // PRIM_TRI pre-pass: {v, e1, e2} widened to fp64, 9 per triangle
    const double* spheres_d; // PRIM_D4: the caller's double4 spheres
    double* out_sums_d;      // double_sums
    double* hit_integral_d;  // OUT_HITS, fp64
    double* hit_dist_d;
    int split;              // waves per packet (1, 2, 4, 8); each owns SUM_CLASSES / split classes
    int n_prims;
    float* partial;         // split > 1, cumulative: [n_rays][split] subtree sums
    double* partial_d;      // ... of double_sums
    // Class split only: the number of waves per packet that actually work (a power of two <=
    // split, chosen on the device from the batch's coherence); waves beyond it exit at once.
    const int* split_dev;
    const int* lat_dev;     // which of the LAT = false / true instantiations runs (null: false)
    // Split per-hit walk: which of the direct (0) / LDS-staged (1) instantiations runs -- both are
    // launched, the device-side plan (hits_assign_kernel) has set *stage_dev (null: no gate).
    const int* stage_dev;
    int stage_want;
    // Split per-hit trace (small batches): primitives are cut into n_chunks ranges of
    // 2^chunk_shift consecutive indices.  The counting pass fills chunk_counts[ray][chunk];
    // the per-hit pass lets wave w own chunks [wave_map[w].y, wave_map[w].z) of packet
    // wave_map[w].x -- heavier packets get more waves (hits_assign_kernel) -- and writes a ray's
    // hits of a chunk from chunk_off[ray][chunk] on.
    int* chunk_counts;
    const int* chunk_off;
    const int4* wave_map;
    const int* n_wave_map;
    bool keep_chunks;       // host only: a hit-count trace whose chunk counts the per-hit trace will reuse
    int chunk_shift, n_chunks;
    int width;              // rays per packet: 64, or 32 / 16 for small batches (lanes >= width
                            // re-trace the packet's last ray)
    const float4* nodes;    // 4 x float4 per node
    int n_nodes;
    const int4* leaves;
    const int* root;
    int* out_counts;        // OUT_COUNTS; OUT_CLOSEST: the closest triangle's index (-1: none)
    float* out_sums;        // OUT_SUMS, PRIM_F4
    const int* offsets;     // OUT_HITS
    int* hit_idx;
    float* hit_integral;    // OUT_HITS, PRIM_F4
    float* hit_dist;
    uint32_t* stats;        // OUT_STATS, 4 per ray
    int* status;            // set to GRACE_STACK_OVERFLOW on stack exhaustion
    // OUT_WSUMS (appended: the fields above keep their offsets): the launch's first weight
    // column and first output column; candidate i's weight of channel c is weights[i w_stride + c],
    // ray r's sum of channel c goes to out_sums[r out_stride + c] (partial: [n_rays][channels][split]).
    const float* weights;
    int w_stride;
    int out_stride;
    // Integrating outputs (appended as well): the SPH kernel's 51-entry line-integral table, device
    // memory (a row of the built-in tables, or the context's custom table).  Captured when the call
    // is enqueued; the prologue copies it into LDS (s_lut / s_lutf) and nothing else reads it.
    const double* kernel_table;
    // Packet plan (appended; see PacketPlan below; all null: no plan for this call).  List
    // packet * SUM_CLASSES + class holds plan_counts[list].x dense rounds (.y survivors, .z entries): their headers from
    // plan_hdr[plan_spans[list].y] on, their survivors' indices from plan_idx[plan_spans[list].x] on.
    // *plan_usable != 0: the planned kernel runs and the others return at once; 0: the reverse.
    const uint32_t* plan_idx;
    const int4* plan_spans;
    const int4* plan_counts;
    const uint32_t* plan_usable;
    // The planned kernel's own waves per packet (planned_split; the word next to *split_dev in the
    // call's frame; null: it takes split_dev / split like the ordinary kernels).  The combine pass
    // reads the one whose kernel ran.
    const int* plan_split_dev;
    const uint32_t* plan_hdr;   // (appended: the fields above keep their offsets)
};


// ---- cached records and their validation (trace_cache.hip) -----------------------------------
// A trace call is stateless for its caller -- trace(rays, spheres, tree) like the reference's --
// but most callers trace the same scene, or the same rays, again and again (frames of a camera
// path over one snapshot; one ray batch over an evolving simulation).  The records a call derives
// from its inputs alone are therefore kept per context: when the arrays of a call are those of
// the previous one (same pointers and sizes), the call after that finds their records cached.
// A cached record is NEVER trusted on pointer equality: every use first re-reads the inputs
// through a 128-bit signature kernel (one streaming pass, HBM-bound, ~1/5 of the cost of
// re-deriving the records) and compares it ON THE DEVICE with the signature the records were
// derived from; if they differ the (flag-gated) pre-pass kernels recompute the records in place.
// No host round trip either way.  grace_trace_set_cache_validation(0) lets a caller who promises
// not to modify cached arrays skip the signature pass.
struct CacheCtl {                 // device memory, one per cache
    unsigned long long sig[2];    // signature of the inputs the cached records were derived from
    uint32_t stale;               // set by the check kernel of the current call: recompute
    uint32_t pad;
};

struct SceneKey {
    Primitive kind = PRIM_F4;     // PRIM_F4 or PRIM_TRI (the fp64 modes' records are never cached)
    const void* prims = nullptr; const void* nodes = nullptr; const void* leaves = nullptr;
    size_t n_prims = 0, n_nodes = 0;
    bool operator==(const SceneKey& o) const
    {
        return kind == o.kind && prims == o.prims && nodes == o.nodes && leaves == o.leaves
            && n_prims == o.n_prims && n_nodes == o.n_nodes;
    }
};

// Scene-constant pre-pass data (trace_prepass.hip): A, B, the nodes' primitive spans and the
// cluster boxes depend on the primitives and the tree only.
struct Scene {
    bool valid = false;           // the buffers hold the records of `key`
    SceneKey key;
    SceneKey seen;                // the previous call's scene (a repeat is what gets cached)
    float4* A = nullptr; float2* B1 = nullptr; float2* B50 = nullptr; double* T64 = nullptr;
    int2* node_prims = nullptr; float4* C = nullptr;
    CacheCtl* ctl = nullptr;
    bool pinned = false;          // filled by grace_trace_prepare_*: kept until released / replaced
    unsigned long long gen = 0;   // which fill of the cache this is (TraceState::cache_gen; see PacketPlan)
};

struct RayKey {
    const float* rays = nullptr;
    size_t n = 0;
    bool operator==(const RayKey& o) const { return rays == o.rays && n == o.n; }
};

// Ray coherence order (trace_coherence.hip).
struct RayOrder {
    bool valid = false;
    RayKey key, seen;
    uint32_t* perm = nullptr;     // n
    uint32_t* ext = nullptr;      // 16 words: 12 extents (order-preserving uints: minima then maxima
                                  // of d, o), [14] not-a-grid flag, [15] longest ray
    CacheCtl* ctl = nullptr;
    bool pinned = false;
    unsigned long long gen = 0;
};

// Packet plan (trace_planned.hip): the cull of an axis-aligned batch -- which groups, clusters and
// candidates survive for each packet -- is a function of the ray order and the scene records alone,
// the two things the caches above hold and validate.  Once both caches serve a call, the cull is
// recorded: for every packet and summation class, the survivors of its non-empty culling rounds
// (entries: one cluster's survivor mask with its lean / fat bits), in list order.  Consecutive
// entries of a list form a dense round: at most 64 survivors together, all with the same lean /
// fat bits.  What is stored (format 3) is the cull already inverted: per list one contiguous run
// of the survivors' primitive indices, 4 bytes each, and per dense round one 4-byte header
// (plan_header: the round's survivor count and its bits) -- lane l of the planned kernel takes
// index word `round's first + l`.  The planned
// kernel (trace_kernel<.., PLANNED>) walks the lists of its classes, one coalesced index load and
// one gather per dense round, and runs
// the survivor loops; it makes no group pass, cluster test or cull.  The lists are per class
// because a class is summed in ascending primitive order and nothing depends on the order between
// classes: one plan serves every packet split K.
// The plan is tied to the fills of the two caches it was recorded from (gen) and remembers their
// signatures: when either cache's signature has moved on -- its records were re-derived, by this
// call or by a call of another kind in between -- the plan is re-recorded in place on that call
// (PlanCtl::record, set on the device).  A batch with a
// packet that is not axis-aligned, a list that outgrows its room on a re-record, or a plan beyond
// the byte budget is unusable: the call runs the ordinary kernels.
struct PlanCtl {                  // device memory
    uint32_t record;              // this call re-records (set by the gate in choose_variants_kernel)
    uint32_t unusable;            // set by the record kernel
    uint32_t usable;              // its complement (a run_if for the kernels that follow)
    uint32_t largest_round;       // survivors of the largest dense round (tallied with stats)
    unsigned long long sig[4];    // the scene cache's and the ray cache's signatures it was recorded under
    // Tallies of the last recording (grace_trace_plan_stats; never read by a trace): entries,
    // survivors, dense rounds, rounds of exactly 64 survivors, rounds closed because the next entry
    // would have passed 64, rounds closed because the next entry's lean / fat bits differed.
    unsigned long long stats[6];
    // Survivor loops the fused consumer runs (planned_fuses) and the survivors of the largest
    // (grace_trace_plan_loops; tallied with stats)
    unsigned long long loops;
    uint32_t largest_loop, pad;
    // Sub-tile layout only (grace_trace_plan_subtiles; tallied with stats): the lists' steps, and the
    // index words of their four streams that name a survivor (the rest name the null record)
    unsigned long long sub_steps, sub_slots;
};
constexpr int PLAN_FORMAT = 3;            // 1: one round per entry; 2: dense rounds; 3: index lists
// Format 4, the SUB-TILE layout of format 3 (unweighted fast kernel only; PlanKey::subtiles): a
// packet's 64 lanes are four quadrants of 16, q = lane >> 4, and each quadrant has a survivor
// stream of its own per list -- the list's survivors that can reach the quadrant's own origin
// rectangle, in the list's (ascending) order.  A list stores STEPS: step t is four index words,
// quadrant q's at `list base + 4 t + q`; a stream shorter than the list's longest is padded at its
// end with the index of the scene's NULL RECORD, n_prims (A = (0, 0, 0, +inf), B50 = (0, 0): its
// term is fma(t, 0, sum) = sum, at table position 0).  Headers, dense rounds and planned_fuses work
// on SLOTS (4 per step): a dense round is PLAN_SUB_ROUND_STEPS consecutive steps (the list's last:
// what is left), its bits the AND over every real survivor in its slots.  The consumer gathers
// and stages exactly as in format 3 -- lane l takes index word l, record l goes to tile slot l --
// and its survivor loops read slot 4 k + q at step k.
constexpr int PLAN_FORMAT_SUBTILE = 4;
constexpr int PLAN_SUB_ROUND_STEPS = 16;
// Below this many packets the automatic rule keeps format 3 (plan_fill; never under 1024) ...
constexpr int PLAN_SUB_MIN_PACKETS = 1024;
// ... and so it does when the steps are more than this fraction of the survivors.
constexpr double PLAN_SUB_MAX_RATIO = 0.82;
// A dense round's header: its survivors (1 .. 64) and its bits (1: lean, 2: fat).
__host__ __device__ inline uint32_t plan_header(const int n_surv, const int bits)
{
    return uint32_t(n_surv) | (uint32_t(bits) << 8);
}
// (the count is clamped to the wave's 64 lanes whatever the word holds: the consumer's own guard)
__host__ __device__ inline int plan_header_count(const uint32_t h) { return int(h & 0xffu) < 64 ? int(h & 0xffu) : 64; }
__host__ __device__ inline int plan_header_bits(const uint32_t h) { return int((h >> 8) & 3u); }
// What the planned kernel may read past the end of a list: 64 index words with every gather (and
// as many again for the gather issued ahead), the headers fetched ahead.
constexpr size_t PLAN_IDX_PAD = 128, PLAN_HDR_PAD = 8;

struct PlanKey {
    int format = PLAN_FORMAT;     // what the entries mean: a plan of another format is never consumed
    bool subtiles = false;        // the sub-tile layout (PLAN_FORMAT_SUBTILE)
    bool fast = false;            // axis_beam_may_hit<AX, FUSED> bounds the b^2 the survivors compute
    int group_shift = 0, width = 0;
    bool reorder = false;
    size_t n_rays = 0, n_prims = 0;
    unsigned long long scene_gen = 0, rays_gen = 0;
    bool operator==(const PlanKey& o) const
    {
        return format == o.format && subtiles == o.subtiles && fast == o.fast && group_shift == o.group_shift && width == o.width && reorder == o.reorder
            && n_rays == o.n_rays && n_prims == o.n_prims && scene_gen == o.scene_gen && rays_gen == o.rays_gen;
    }
};

struct PacketPlan {
    bool valid = false;           // the buffers hold a plan recorded under `key`
    bool dead = false;            // `key`'s batch cannot be planned (known on the host): nothing is launched for it
    PlanKey key;
    // What the call that sized it asked of the layout (plan_subtile_request): a format-3 plan sized
    // under the same request is what that request gets (the rule, or the budget, declined the
    // sub-tile layout), and serves every call that asks for none.
    int asked = 0;
    uint32_t* idx = nullptr;      // n_words + PLAN_IDX_PAD: the lists' survivor indices
    uint32_t* hdr = nullptr;      // n_hdrs + PLAN_HDR_PAD: the lists' round headers
    int4* spans = nullptr;        // per list {first index word, first header, room in survivors, room in rounds}
                                  // (sub-tile layout: room in steps)
    int4* counts = nullptr;       // per list {dense rounds, survivors, entries, sub-tile layout: steps}
    PlanCtl* ctl = nullptr;
    size_t n_lists = 0, n_words = 0, n_hdrs = 0;
    size_t recorded = 0;          // survivors in use when the plan was sized
    size_t bytes() const          // the device memory it takes (grace_trace_plan_bytes)
    {
        return (n_words + PLAN_IDX_PAD + n_hdrs + PLAN_HDR_PAD) * sizeof(uint32_t)
            + n_lists * (sizeof(int4) + sizeof(int4)) + sizeof(PlanCtl);
    }
};

// What the device-side gate of a call with a recorded plan needs (launch_choose_variants).
struct PlanGate {
    const CacheCtl* scene = nullptr;   // the caches the plan was recorded from
    const CacheCtl* rays = nullptr;
    PlanCtl* ctl = nullptr;
};

// Waves per packet of the planned kernel, a function of the packet count alone.  Its extra waves
// repeat nothing -- no walk, no cluster test, no cull: each takes its classes' lists -- so the
// ordinary kernels' rule (choose_split: as few waves as fill the chip) does not apply; what an
// extra wave costs is its prologue (the rays, the table) and a partial sum per ray.  Thresholds
// from the sweep over the 1024^2 frame's shards (profiles/trace_quad_reads_mi355x.txt, section 3):
// of the unweighted kernel with the fast integral; the exact integral's sweep agrees (K = 8 is
// best or tied at every size).  The weighted planned kernels do NOT take it (use_records, trace.hip):
// with four channels K = 2 or 4 is best and this rule would cost them 6-13 %; one to three
// channels were not swept.  They keep the ordinary kernels' K.
// The host sizes the planned launch with it, the device writes it to TraceArgs::plan_split_dev.
__host__ __device__ inline int planned_split(const int n_packets)
{
    return n_packets <= 8192 ? SUM_CLASSES : SUM_CLASSES / 2;
}

// Survivor loops of the unweighted planned kernel with the fast integral: consecutive dense rounds
// of a list run as ONE loop while they are test-free (lean), carry the same bits and hold at most
// PLAN_LOOP_MAX survivors together -- a list's index words are contiguous, so the loop's second 64
// are simply the next 64 words.  planned_fuses: does the round with header `next` join the open
// loop of loop_n survivors and loop_bits?  The kernel forms its loops with it and the recorder
// tallies them with it (PlanCtl::loops).  The weighted planned kernels (their occupancy is set by
// LDS, and the longer tile would cost MODE_WCUM1 a wave per SIMD) and the exact integral (no
// test-free loop) run one loop per dense round.
constexpr int PLAN_LOOP_MAX = 128;
__host__ __device__ inline bool planned_fuses(const int loop_n, const int loop_bits, const uint32_t next)
{
    return (loop_bits & 1) != 0 && plan_header_bits(next) == loop_bits
        && loop_n + plan_header_count(next) <= PLAN_LOOP_MAX;
}

// trace_sph walks twice -- hit counts (for the offsets), then the per-hit pass -- and the split
// per-hit pass of small batches needs hits per (ray, chunk), a third walk.  The hit-count call
// made on behalf of trace_sph (grace_trace_hitcounts_keep_f4) records them into this buffer of
// its own (the workspace is reset by the scan in between); the per-hit call that follows on the
// same rays and spheres consumes them.
struct HitsCache {
    int* chunk_counts = nullptr;
    size_t capacity = 0;      // ints
    bool valid = false;
    const void* rays = nullptr; const void* prims = nullptr;
    size_t n_rays = 0, n_prims = 0;
    int n_chunks = 0;
};

struct TraceState {
    int* status = nullptr;                 // one device int, allocated on first use
    // Measurement hook (grace_trace_last_lattice): the device flag of the last trace launch (lives
    // in the call's workspace frame: valid until the next library call on the context).
    const int* last_lat_dev = nullptr;
    hipStream_t last_lat_stream = nullptr;
    bool timing = false;                   // record HIP events around the traversal kernel itself
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ev_valid = false;
    // knobs (grace_trace_set_*)
    bool ray_reorder = true;
    int treelet = -1;                      // -1: chosen per call
    int split = -1;                        // waves per packet; -1: automatic
    int lat_split = 4;                     // waves per packet of big batches in scenes with sub-spacing spheres (0: one)
    int width = -1;                        // rays per packet of the per-hit / triangle traces; -1: automatic
    bool exact_integrals = false;          // column-density trace: bit-reproducible per-hit arithmetic
    bool hits_stage_split = true;          // split per-hit walk: stage heavy packets' hits in LDS
    bool cache_validation = true;          // validate cached records by signature before every use
    bool cache_auto = true;                // cache the records of a scene / ray batch seen twice in a row
    // SPH kernel (grace_trace_set_sph_kernel*): GRACE_SPH_KERNEL_* (-1: custom) and its device table,
    // a row of the built-in tables (set when the state is created) or custom_table.  Only ever
    // copied into TraceArgs::kernel_table: no cached record depends on it.
    int sph_kernel = 0;
    const double* builtin_tables = nullptr;  // device address of the built-in tables, [6][N_TABLE]
    const double* kernel_table = nullptr;
    double* custom_table = nullptr;          // N_TABLE doubles, allocated by the first custom table
    double custom_host[N_TABLE] = {};        // its host copy (grace_trace_get_sph_kernel)
    bool plan_on = true;                   // record and use packet plans (grace_trace_set_plan)
    // bytes a plan may take (grace_trace_set_plan_budget): the 1024^2 frame over 10^7 particles takes
    // 1.475 GB in the sub-tile layout (530 MB in format 3)
    size_t plan_budget = size_t(2) << 30;
    int plan_subtiles = -1;                // sub-tile layout: -1 automatic, 0 never, 1 whenever eligible (grace_trace_set_plan_subtiles)
    Scene scene;
    RayOrder rays;
    HitsCache hits;
    unsigned long long cache_gen = 0;      // fills of the scene / ray caches so far
    PacketPlan plan;
    // Measurement hook (grace_trace_last_plan_used): the last class-sum launch's plan flags
    const PlanCtl* last_plan_ctl = nullptr;
    hipStream_t last_plan_stream = nullptr;
    bool last_plan_fuses = false;          // ... and whether its planned kernel fuses rounds (planned_fuses)
};

// The TraceState of the calling thread's context (created on first use).
grace_status trace_state(TraceState** out);

// The context's status word, allocated and zeroed on first use.
inline grace_status ensure_status(TraceState& ts, hipStream_t stream)
{
    if (!ts.status) {
        GRACE_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&ts.status), sizeof(int)));
        GRACE_TRY_HIP(hipMemsetAsync(ts.status, 0, sizeof(int), stream));
    }
    return GRACE_OK;
}

// The ts.timing bracket around the launches of one call (what grace_trace_last_kernel_ms reports):
// the events are created on first use.
template <typename Launches>
grace_status timed(TraceState& ts, hipStream_t stream, Launches launches)
{
    if (ts.timing) {
        if (!ts.ev0) { GRACE_TRY_HIP(hipEventCreate(&ts.ev0)); GRACE_TRY_HIP(hipEventCreate(&ts.ev1)); }
        GRACE_TRY_HIP(hipEventRecord(ts.ev0, stream));
    }
    GRACE_TRY(launches());
    if (ts.timing) {
        GRACE_TRY_HIP(hipEventRecord(ts.ev1, stream));
        ts.ev_valid = true;
    }
    return GRACE_OK;
}

// trace_cache.hip: signatures of the inputs behind cached records.
// One launch reads up to four arrays -- the scene's primitives, nodes and leaves (group 0) and the
// rays (group 1); a null array is skipped -- and leaves per-workgroup partial sums in `partial`
// (sig_partial_words() 64-bit words of scratch); a second, single-workgroup launch folds them,
// compares each requested group with its cache's stored signature, stores the new one and sets the
// cache's stale flag (force: set it regardless -- a first fill).  A stale ray cache also gets its
// extents re-initialised.
size_t sig_partial_words();
struct SigRequest {
    const void* prims = nullptr; size_t prims_bytes = 0;
    const void* nodes = nullptr; size_t nodes_bytes = 0;
    const void* leaves = nullptr; size_t leaves_bytes = 0;
    CacheCtl* scene_ctl = nullptr; bool scene_force = false;
    const void* rays = nullptr; size_t rays_bytes = 0;
    CacheCtl* rays_ctl = nullptr; bool rays_force = false;
    uint32_t* rays_ext = nullptr;
};
grace_status launch_signatures(const SigRequest& rq, unsigned long long* partial, hipStream_t stream);

// trace_prepass.hip
grace_status scene_release(TraceState& ts);
// Buffers of the scene cache for `key` (replaces whatever is cached).
grace_status scene_cache_alloc(TraceState& ts, const SceneKey& key);
// Fills the scene-constant arrays (any of B1 / B50 / T64 may be null) for primitives of `kind`:
// the double4 and mixed-precision records are float boxes that contain every sphere the fp64 test
// can accept.  run_if (device, optional): every kernel returns at once if *run_if == 0.
grace_status scene_fill(Primitive kind, const void* prims, size_t n_prims, const float4* nodes,
                        size_t n_nodes, const int4* leaves, float4* A, float2* B1, float2* B50,
                        double* T64, int2* node_prims, float4* C, hipStream_t stream,
                        const uint32_t* run_if = nullptr);
grace_status scene_prepare(TraceState& ts, Primitive kind, const void* prims, size_t n_prims,
                           const int* d_nodes, size_t n_nodes, const int* d_leaves, hipStream_t stream);

// trace_coherence.hip
grace_status rays_release(TraceState& ts);
grace_status rays_cache_alloc(TraceState& ts, const RayKey& key);
// extents -> keys -> partial sort; keys: n words of scratch (the caller's workspace frame must
// include sort_ws_bytes(n_rays, 4, 0)).  run_if (device, optional): gates every kernel; the
// extents must then have been initialised already (launch_signatures does it for a stale cache).
grace_status ray_order(const float* d_rays, size_t n_rays, uint32_t* ext, uint32_t* keys, uint32_t* perm,
                       const float4* scene_min, uint32_t* lat_flag, int n_packets, int split, int* split_dev,
                       hipStream_t stream, const uint32_t* run_if = nullptr);
grace_status rays_prepare(TraceState& ts, const float* d_rays, size_t n_rays, hipStream_t stream);
// The device-side choices of a trace launch for a batch whose order is cached.
// gate (optional): also decides whether this call re-records its packet plan.
// plan_split_dev (optional): receives the planned kernel's waves per packet (planned_split).
grace_status launch_choose_variants(const uint32_t* ext12, int n, const float4* scene_min, uint32_t* lat_flag,
                                    int split_packets, int split_launched, int* split_dev, hipStream_t stream,
                                    const PlanGate* gate = nullptr, int* plan_split_dev = nullptr);

// trace_planned.hip: the packet plan, its record kernel and the planned class-sum kernels.
grace_status plan_release(TraceState& ts);
// Sizes, allocates and records the plan of `key` for the batch `a` describes (its records and ray
// order already queued on `stream`); synchronises the stream once.  On return ts.plan is valid, or dead.
// request (plan_subtile_request): 0 records format 3; otherwise the sub-tile layout is recorded if
// it fits the budget and, request < 0, the automatic rule takes it -- else format 3 as for 0.
// ts.plan.key.subtiles says which it was.
grace_status plan_fill(TraceState& ts, const PlanKey& key, int request, const TraceArgs& a, hipStream_t stream);
// The gated re-record of a call with a valid plan.
grace_status plan_record(const TraceState& ts, const TraceArgs& a, hipStream_t stream);
// trace_kernel<mode, SPLIT, fast, false, PLANNED> over `grid` workgroups (mode: f4_sums).
// subtiles: the plan is of the sub-tile layout (unweighted, fast only): the SUBTILE instantiation.
grace_status launch_planned(int mode, bool fast, bool subtiles, int grid, const TraceArgs& a, hipStream_t stream);

} // namespace grace_hip
