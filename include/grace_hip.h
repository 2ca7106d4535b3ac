/*
 * grace_hip.h -- C ABI of libgrace_hip.so: the MI355X (gfx950) implementation of the
 * GRACE BVH-build + SPH ray-traversal hot path.
 *
 * The reference (spthm/grace-devel) has no FFI layer: its boundary is the header-template
 * API of namespace grace, compiled by nvcc into the caller.  Each entry point below is one
 * concrete instantiation of that API over raw device pointers; the reference interface it
 * replaces is cited as file:line (paths relative to the reference root).  The C++ header
 * mirror (include/grace/grace.h) forwards to these and restores the reference's error
 * behaviour (throw std::invalid_argument / print + exit).
 *
 * Conventions
 *  - All pointers named d_* are device pointers on the current HIP device; h_* are host.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *    asynchronous on that stream unless they return a value to the host (documented).
 *  - Every function returns a grace_status; grace_last_error() describes the last failure
 *    of the calling thread.
 *  - Temporaries come from a grow-only device workspace owned by the library (the
 *    reference allocates and frees thrust temporaries inside every call).  Workspace, status
 *    word, cached trace scene / ray order, timing events and tuning knobs belong to a CONTEXT.
 *    Every device has a default context, used by threads that never ask for another: with one
 *    process per GPU, or one process that sets a device current and calls, nothing needs to be
 *    done.  A context serves one call at a time; host threads may call concurrently iff each has
 *    made a context of its own current (grace_context_create / grace_context_set_current) -- one
 *    thread per GPU of a node, or several threads sharing one GPU.  Calls may use any stream;
 *    consecutive calls of a context on different streams are ordered by the library (their
 *    temporaries share memory), and a stream may be destroyed as soon as the caller has
 *    synchronised with it.
 *  - float4 / int4 / Ray arrays are passed as float* / int* / void* with the reference's
 *    memory layout: sphere = {x, y, z, h}; Ray = {dx,dy,dz,ox,oy,oz,length} (28 B,
 *    include/grace/ray.h:5-10); node = 4 x 16 B, leaf = int4 (include/grace/cuda/nodes.h:22-42).
 */
#ifndef GRACE_HIP_H
#define GRACE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum grace_status {
    GRACE_OK = 0,
    GRACE_INVALID_ARGUMENT = 1, /* the reference throws std::invalid_argument          */
    GRACE_HIP_ERROR = 2,        /* the reference prints and exit()s (error.h:40-56)     */
    GRACE_OUT_OF_MEMORY = 3,
    GRACE_STACK_OVERFLOW = 4    /* traversal stack exhausted (reference: GRACE_ASSERT)  */
} grace_status;

typedef void* grace_stream;

int grace_version(void);
const char* grace_last_error(void);

/* ---- device memory helpers: let HIP-free host code (include/grace) own device vectors,
 *      the role thrust::device_vector plays in the reference ---------------------------- */
grace_status grace_device_malloc(void** d_ptr, size_t bytes);
grace_status grace_device_free(void* d_ptr);
grace_status grace_memcpy_htod(void* d_dst, const void* h_src, size_t bytes, grace_stream stream);
grace_status grace_memcpy_dtoh(void* h_dst, const void* d_src, size_t bytes, grace_stream stream);
grace_status grace_memcpy_dtod(void* d_dst, const void* d_src, size_t bytes, grace_stream stream);
grace_status grace_memset(void* d_dst, int byte, size_t bytes, grace_stream stream);
grace_status grace_stream_synchronize(grace_stream stream);
/* Pre-size / drop the workspace of the calling thread's context (optional). */
grace_status grace_workspace_reserve(size_t bytes);
grace_status grace_workspace_release(void);

/* ---- contexts: everything the library keeps between calls (see Conventions).  The reference has
 *      one set of globals per process (texture references, bintree_trace.cuh:37-38) and drives
 *      several GPUs from one process only through ncclCommInitAll-style code of the caller's
 *      (SURVEY.md section 8e); a context per (thread, device) is what makes that form work here.
 *      grace_context_create: a fresh context on the CURRENT device.  grace_context_set_current:
 *      the calling thread's context from now on (NULL: back to the current device's default
 *      context).  grace_context_destroy frees the context's device memory and events (its device
 *      is made current for the duration); default contexts are never destroyed.
 *      grace_context_get_current returns the context the next call of this thread would use. */
typedef struct grace_context_s* grace_context;
grace_status grace_context_create(grace_context* ctx);
grace_status grace_context_destroy(grace_context ctx);
grace_status grace_context_set_current(grace_context ctx);
grace_status grace_context_get_current(grace_context* ctx);

/* ---- Morton keys ------------------------------------------------------------------- */
/* AABB of sphere centroids: compute_centroids + min_vec3/max_vec3
 * (include/grace/cuda/kernels/morton.cuh:153-164), fused into one pass.  Synchronises;
 * results in host arrays h_bot[3], h_top[3]. */
grace_status grace_centroid_bounds_f4(const float* d_spheres, size_t n,
                                      float* h_bot, float* h_top, grace_stream stream);
/* min_vec4 / max_vec4 over x,y,z,w (include/grace/cuda/util/extrema.cuh, as used by
 * tests/project_gadget/project_gadget.cu:66-68).  Synchronises. */
grace_status grace_minmax_f4(const float* d_v4, size_t n, float* h_mins4, float* h_maxs4,
                             grace_stream stream);
/* The rest of include/grace/cuda/util/extrema.cuh:190-772 (min_max_x/y/z/w, min/max_vec2/3/4 over
 * any vector type): component-wise minima and maxima of n records of n_comp (1..4) leading
 * components of elem_type, stride_bytes apart.  h_mins / h_maxs: host arrays of n_comp elements
 * of the same type.  Synchronises. */
enum { GRACE_ELEM_F32 = 0, GRACE_ELEM_F64 = 1, GRACE_ELEM_I32 = 2, GRACE_ELEM_U32 = 3 };
grace_status grace_minmax_components(const void* d_data, size_t n, int elem_type, int n_comp,
                                     size_t stride_bytes, void* h_mins, void* h_maxs,
                                     grace_stream stream);
/* grace::morton_keys(prims, N, bot, top, keys, CentroidSphere) with uinteger32 keys and
 * Real3 = float3 (include/grace/cuda/kernels/morton.cuh:97-119,30-55; build_sph.cuh:27-35).
 * Per axis the cell is KeyType(scale * (centre - bot)), scale = span / (top - bot) rounded once
 * on the host, span = 2^10 - 1 (2^21 - 1 for 63-bit keys).  In the unit box a centre at `top`
 * falls in cell `span` exactly, so the key of the point at `top` on all three axes is all ones
 * (in other boxes the rounded scale may leave it in cell span - 1).  An axis with top == bot (a
 * planar scene through the bounds-free overloads) has scale 0, so every primitive gets cell 0 on
 * it.  Centres outside [bot, top] are unspecified, as in the reference.  This holds for every
 * grace_morton_keys* entry point below. */
grace_status grace_morton_keys30_f4(const float* d_spheres, size_t n, const float* h_bot,
                                    const float* h_top, uint32_t* d_keys, grace_stream stream);
/* Same with uinteger64 keys (63 bits); float3 and double3 bounds. */
grace_status grace_morton_keys63_f4(const float* d_spheres, size_t n, const float* h_bot,
                                    const float* h_top, uint64_t* d_keys, grace_stream stream);
grace_status grace_morton_keys63_f4_d3(const float* d_spheres, size_t n, const double* h_bot,
                                       const double* h_top, uint64_t* d_keys,
                                       grace_stream stream);

/* morton_keys_sph / morton_keys over other point types (build_sph.cuh:16-33, Real4 = double4;
 * kernels/gen_rays.cuh:603-604, PointType = float3/float4): n records of elems_per_point
 * floats (is_double = 0) or doubles (1), x y z first.  Co-ordinates are narrowed to float
 * before the key arithmetic (CentroidSphere, generic/functors/centroid.h:33-40 --
 * tests/morton_key_kernel/63bit_keys.cu:52-58).  bot/top: host float[3]. */
grace_status grace_morton_keys30_points(const void* d_points, size_t n, int is_double,
                                        int elems_per_point, const float* h_bot,
                                        const float* h_top, uint32_t* d_keys, grace_stream stream);
grace_status grace_morton_keys63_points(const void* d_points, size_t n, int is_double,
                                        int elems_per_point, const float* h_bot,
                                        const float* h_top, uint64_t* d_keys, grace_stream stream);

/* The remaining (point type, bounds type, key type) instantiations of grace::morton_keys
 * (kernels/morton.cuh:97-189): float4 spheres with double3 bounds and 30-bit keys; generic
 * points with double3 bounds (scale and key arithmetic in double on the float-narrowed
 * co-ordinates); and the centroid bounds of generic points (the bounds-free overloads for
 * Real4 = double4: compute_centroids + min/max of the float3 centroids, morton.cuh:139-174).
 * grace_centroid_bounds_points synchronises. */
grace_status grace_morton_keys30_f4_d3(const float* d_spheres, size_t n, const double* h_bot,
                                       const double* h_top, uint32_t* d_keys,
                                       grace_stream stream);
grace_status grace_centroid_bounds_points(const void* d_points, size_t n, int is_double,
                                          int elems_per_point, float* h_bot, float* h_top,
                                          grace_stream stream);
grace_status grace_morton_keys30_points_d3(const void* d_points, size_t n, int is_double,
                                           int elems_per_point, const double* h_bot,
                                           const double* h_top, uint32_t* d_keys,
                                           grace_stream stream);
grace_status grace_morton_keys63_points_d3(const void* d_points, size_t n, int is_double,
                                           int elems_per_point, const double* h_bot,
                                           const double* h_top, uint64_t* d_keys,
                                           grace_stream stream);

/* ---- stable radix sort: the thrust::sort_by_key(keys, values) call sites
 *      (include/grace/cuda/build_sph.cuh:46,57,70,81; kernels/gen_rays.cuh:483,520,577,615).
 *      Keys ascending, equal keys keep their input order; values (value_bytes per element,
 *      a multiple of 4: 4/16/28/32/36 are the reference's payloads) are permuted in place.
 *      d_values may be NULL (keys only).  d_perm (optional, n uint32) receives the source
 *      index of every output element.  Asynchronous on `stream`, no host round trip; inputs
 *      of 2^18 elements or more also use the context's internal side stream, forked from
 *      and joined to `stream` by events (bucket sort with a device-gated fallback, see
 *      csrc/sort.hip). ---------------------------------------------------------------- */
grace_status grace_sort_pairs_u32(uint32_t* d_keys, void* d_values, size_t n, int value_bytes,
                                  int begin_bit, int end_bit, uint32_t* d_perm,
                                  grace_stream stream);
grace_status grace_sort_pairs_u64(uint64_t* d_keys, void* d_values, size_t n, int value_bytes,
                                  int begin_bit, int end_bit, uint32_t* d_perm,
                                  grace_stream stream);
/* Large sorts try the bucket sort first and fall back to the index sort on the device when a bucket
 * overflows (clustered keys).  The library remembers per context whether the last large sort
 * overflowed -- a word of pinned host memory written by the sort's own kernel, never waited for --
 * and then goes straight to the index sort, looking again every 8th time.  0 switches the memory
 * off (every large sort tries the buckets); the choice is between two paths with identical results. */
grace_status grace_sort_set_overflow_hint(int enabled);
/* Which sort the last grace_sort_pairs_* call of the calling thread's context took (the sorts made
 * inside other entry points, e.g. the composite-key sort of grace_sort_by_distance_f32, record
 * too).  Recorded on the host when the call is made: no launch, no synchronisation. */
typedef struct grace_sort_stats {
    int msd_bits;       /* bits of the bucket digit the call planned; 0: the index sort */
    int tile;           /* records per bucket tile / bucket capacity for the key and payload: 4096 or 8192 */
    int hint_skipped;   /* 1: a bucket plan was made but the overflow hint sent the call to the index sort */
    int overflowed;     /* the word the bucket sort's flag kernel writes: 1 if a bucket was above the capacity
                           (the gated index sort did the work), 0 if the bucket kernels did; valid once the
                           call's stream is synchronised.  -1: no bucket sort was enqueued by that call, or the
                           pinned word could not be allocated */
} grace_sort_stats;
grace_status grace_sort_last_stats(grace_sort_stats* h_stats);

/* ---- deltas: grace::compute_deltas (include/grace/cuda/kernels/albvh.cuh:33-47,949-978)
 *      with DeltaEuclidean / DeltaSurfaceArea / DeltaXOR
 *      (include/grace/generic/functors/albvh.h:17-126).  d_deltas has n + 1 entries,
 *      d_deltas[i] = delta(i - 1); sentinels +inf / all-ones. --------------------------- */
grace_status grace_deltas_euclid_f4(const float* d_spheres, size_t n, float* d_deltas,
                                    grace_stream stream);
grace_status grace_deltas_area_f4(const float* d_spheres, size_t n, float* d_deltas,
                                  grace_stream stream);
grace_status grace_deltas_xor_u32(const uint32_t* d_keys, size_t n, uint32_t* d_deltas,
                                  grace_stream stream);
grace_status grace_deltas_xor_u64(const uint64_t* d_keys, size_t n, uint64_t* d_deltas,
                                  grace_stream stream);

/* ---- ALBVH: grace::build_ALBVH (include/grace/cuda/kernels/albvh.cuh:986-1072) with
 *      DeltaComp = less and AABBSphere.  d_nodes: capacity 16 * (n - 1) ints; d_leaves:
 *      capacity 4 * n ints; d_root: one device int.  *h_n_leaves receives the leaf count
 *      (the reference resizes tree.nodes/leaves from it, albvh.cuh:842-845): synchronises.
 *      GRACE_INVALID_ARGUMENT if n <= max_per_leaf (albvh.cuh:795-799). ---------------- */
grace_status grace_albvh_build_f4(const float* d_spheres, size_t n, const float* d_deltas,
                                  int max_per_leaf, int* d_nodes, int* d_leaves, int* d_root,
                                  size_t* h_n_leaves, grace_stream stream);
/* XOR (uint32) deltas variant. */
grace_status grace_albvh_build_f4_u32(const float* d_spheres, size_t n, const uint32_t* d_deltas,
                                      int max_per_leaf, int* d_nodes, int* d_leaves,
                                      int* d_root, size_t* h_n_leaves, grace_stream stream);

/* ---- triangle primitives: the alternate-primitive instantiation of the same templates
 *      (tests/profile_trace_triangle).  Triangle = {v, e1, e2}, 9 floats, 36 B
 *      (triangle.cuh:11-25). ------------------------------------------------------------- */
/* compute_centroids + min/max with TriangleCentroid (triangle.cuh:92-102;
 * include/grace/cuda/kernels/morton.cuh:139-174).  Synchronises. */
grace_status grace_centroid_bounds_tri(const float* d_tris, size_t n, float* h_bot, float* h_top,
                                       grace_stream stream);
/* grace::morton_keys(d_tris, ..., TriangleCentroid()) with 30-bit keys (tris_tree.cuh:27). */
grace_status grace_morton_keys30_tri(const float* d_tris, size_t n, const float* h_bot,
                                     const float* h_top, uint32_t* d_keys, grace_stream stream);
/* grace::build_ALBVH(d_tree, d_tris, d_deltas, TriangleAABB()) with XOR deltas
 * (tris_tree.cuh:28-29; TriangleAABB triangle.cu:3-35). */
grace_status grace_albvh_build_tri_u32(const float* d_tris, size_t n, const uint32_t* d_deltas,
                                       int max_per_leaf, int* d_nodes, int* d_leaves, int* d_root,
                                       size_t* h_n_leaves, grace_stream stream);

/* ---- the generic forms of grace/cuda/kernels/albvh.cuh:986-1072 in one entry: any primitive kind
 *      (float4 / double4 spheres with AABBSphere, the shipped triangles, or GRACE_PRIM_BOX: the
 *      caller's own AABBFunc already evaluated per primitive -- 6 floats {bot xyz, top xyz} each,
 *      written by the header kernel of include/grace/cuda/kernels/albvh.cuh, which runs the functor
 *      in the caller's translation unit), any delta type, and DeltaComp = thrust::less or
 *      thrust::greater (albvh.cuh:1029-1045; the comparator is only ever applied as
 *      delta_comp(delta_L, delta_R), albvh.cuh:129,194,465,607). -------------------------------- */
enum { GRACE_PRIM_SPHERE_F4 = 0, GRACE_PRIM_TRIANGLE = 1, GRACE_PRIM_SPHERE_D4 = 2, GRACE_PRIM_BOX = 3 };
enum { GRACE_DELTA_F32 = 0, GRACE_DELTA_F64 = 1, GRACE_DELTA_U32 = 2, GRACE_DELTA_U64 = 3 };
enum { GRACE_COMP_LESS = 0, GRACE_COMP_GREATER = 1 };
grace_status grace_albvh_build_ex(int prim_kind, const void* d_prims, size_t n, int delta_type,
                                  const void* d_deltas, int delta_comp, int max_per_leaf,
                                  int* d_nodes, int* d_leaves, int* d_root, size_t* h_n_leaves,
                                  grace_stream stream);

/* Measurement hook for profile_tree-style harnesses (tests/profile_tree/profile_tree.cu prints
 * one line per build phase): when enabled, HIP events are recorded on the build's stream around
 * its leaf stage (leaf heads + scan + leaf records AND their deltas: the reference's
 * build_leaves, remove_empty_leaves and copy_leaf_deltas, fused here) and its node stage
 * (leaf boxes, pyramids, nodes: build_nodes). */
grace_status grace_albvh_enable_timing(int enabled);
grace_status grace_albvh_last_phase_ms(float* h_leaves_ms, float* h_nodes_ms);
/* trace_closest_tri (tris_trace.cu:43-62): RayEntry_tri / RayIntersect_tri / OnHit_tri
 * (tris_trace.cuh:11-73) over Moeller-Trumbore with back-face culling (triangle.cuh:54-88);
 * d_closest[ray] = index of the nearest triangle hit, or -1. */
grace_status grace_trace_closest_tri(const void* d_rays, size_t n_rays, const float* d_tris,
                                     size_t n_tris, const int* d_nodes, size_t n_nodes,
                                     const int* d_leaves, const int* d_root, int* d_closest,
                                     grace_stream stream);

/* ---- traversal: grace::trace_hitcounts_sph / trace_cumulative_sph / trace_sph pass 2
 *      (include/grace/cuda/trace_sph.cuh:58-168) over trace_kernel
 *      (include/grace/cuda/kernels/bintree_trace.cuh:52-197).  n_nodes = n_leaves - 1.
 *      Any n_rays is accepted here (0: nothing to do, e.g. the empty shard of a sharded
 *      batch); the header mirror enforces the reference's n_rays % 32 == 0
 *      (bintree_trace.cuh:231-238). ----------------------------------------------------- */
grace_status grace_trace_hitcounts_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                      size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                      const int* d_leaves, const int* d_root,
                                      int* d_hit_counts, grace_stream stream);
/* grace_trace_hitcounts_f4 for a caller that goes on to the per-hit pass (trace_sph,
 * trace_with_sentinels_sph: trace_sph.cuh:121-141): same output; for small batches it also keeps
 * the hits per (ray, primitive chunk) in a buffer of the library's, which the next
 * grace_trace_hits_f4 call on the same rays and spheres consumes instead of walking the tree a
 * third time.  Any trace call in between drops them. */
grace_status grace_trace_hitcounts_keep_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                           size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                           const int* d_leaves, const int* d_root,
                                           int* d_hit_counts, grace_stream stream);
grace_status grace_trace_cumulative_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                       size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                       const int* d_leaves, const int* d_root,
                                       float* d_cumulated, grace_stream stream);
/* Weighted, multi-channel column densities -- an extension the reference lacks: the terms of
 * OnHit_sphere_cumulate (functors/trace.cuh:164-186) scaled as multiply_by_weights scales per-hit
 * integrals (kernels/weights.cuh:12-50), summed per ray without writing any hit:
 *   d_out[r * n_channels + c] = sum over hits i of ray r of fl32(d_weights[i * n_channels + c] * I_ri)
 * where I_ri is the term grace_trace_cumulative_f4 adds for that (ray, sphere) pair and i indexes
 * d_spheres as passed (the tree's sorted order).  Each channel is summed in the same class-ordered
 * fp32 order as grace_trace_cumulative_f4.  Exact mode (grace_trace_set_exact_integrals(1)): I_ri is
 * the reference's per-hit integral and the result is that sum bit for bit.  Default mode: within
 * 1e-5 of sum |w| I of the fp64 sum (the weight is folded into the term's 1/h^2 factor).  Weights of
 * 1.0f give grace_trace_cumulative_f4's bits in both modes.  1 <= n_channels <= 64; channels are
 * traced four at a time, each group of four a walk of its own.  Weights are read on every call
 * (never cached).  GRACE_INVALID_ARGUMENT for n_channels outside 1..64 or null weights; zero rays:
 * GRACE_OK, nothing written. */
grace_status grace_trace_cumulative_weighted_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                                size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                                const int* d_leaves, const int* d_root,
                                                const float* d_weights, int n_channels, float* d_out,
                                                grace_stream stream);
/* Depth-ordered emission-absorption integrals along rays -- an extension the reference lacks: light
 * emitted by the spheres along the ray and absorbed by what lies in front of it, in one call and
 * without ever holding more than a batch of hits.
 * Inputs: rays, float4 spheres and the tree as for the other traces; d_emission [n_spheres *
 * n_channels] fp32, 1 <= n_channels <= 64; d_absorption [n_spheres] fp32; both in tree order, read on
 * every call.  Outputs: d_out [n_rays * n_channels] fp32; d_tau [n_rays] fp32, or null to skip it.
 * For ray r, its hits are exactly those of grace_trace_hits_f4 on that ray: the same hit test, the
 * same per-hit integral I (the reference's arithmetic, with the context's SPH kernel) and the same
 * distance d, both bit for bit.  The hits are ordered ascending by (d, sphere index): d compared
 * as fp32 (-0 == +0), ties broken by the lower index -- a total order, so the sequence does not
 * depend on the traversal.  Then, in fp64, over the ordered hits k = 0, 1, ... with sphere i_k:
 *   a_k      = (double)d_absorption[i_k] * (double)I_k         optical depth of hit k
 *   tau_k    = sum over m < k of a_m                           what lies in front of it
 *   phi(a)   = -expm1(-a) / a  for a != 0,  1 for a == 0       self-absorption of a uniform slab
 *   d_out[r * n_channels + c] = fl32( sum_k (double)d_emission[i_k * n_channels + c] * (double)I_k * phi(a_k) * exp(-tau_k) )
 *   d_tau[r]                  = fl32( sum_k a_k )
 * (the formal solution of the transfer equation with each sphere a slab of constant source
 * function).  Zero absorption gives the weighted column density; one sphere gives S (1 - e^-a)
 * with S = emission / absorption.  Negative absorption is the caller's business: the formulas are
 * applied as written.  A ray without hits gets zeros.  The order of the fp64 additions is a function
 * of the ray's ordered hit list alone: results are bit-identical from run to run and do not depend
 * on the packet width, the budget below, the other rays of the call or the ray's place among them.
 * Against an evaluation of the formulas in another order, with another libm:
 *   |out - ref| <= ulp32(ref) / 2 + 8 (n_r + 8) 2^-53 max(1, tau_r) sum_k |term_k|     (n_r hits).
 * The call counts every ray's hits, cuts the rays, in array order, into batches whose per-hit
 * arrays (12 bytes a hit) fit a byte budget, and per batch runs the per-hit walk into the context's
 * workspace and one fused sort-and-composite kernel; it synchronises the stream once, to read the
 * batch ends (not the per-ray counts).  The total number of hits is not limited to INT32_MAX.
 * GRACE_INVALID_ARGUMENT for n_channels outside 1..64, null emission / absorption or null d_out
 * (checked before any launch); zero rays: GRACE_OK, nothing written.
 * Periodic boxes: grace_trace_emission_absorption_periodic_f4 below. */
grace_status grace_trace_emission_absorption_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                                size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                                const int* d_leaves, const int* d_root,
                                                const float* d_emission, int n_channels,
                                                const float* d_absorption, float* d_out, float* d_tau,
                                                grace_stream stream);
/* Absorbed radiation deposited on the particles -- the transpose of the integral above, an extension
 * the reference lacks (its trace_sph + sort_by_distance + weighted_exclusive_segmented_scan chain
 * stops at the optical depth in front of every hit): rays leave a source carrying photons, and the
 * call returns how much of every ray every particle absorbs, summed over the rays, and how much
 * escapes.
 * Inputs: rays, float4 spheres and the tree as for the other traces; d_luminosity [n_rays *
 * n_channels] fp32, what ray r carries in channel c; d_absorption [n_spheres * n_channels] fp32, in
 * tree order, per channel; 1 <= n_channels <= 64.  Outputs: d_deposit [n_spheres * n_channels] fp64,
 * overwritten (not added to); d_transmitted [n_rays * n_channels] fp32, or null; d_quantum
 * [n_channels] fp64, or null.
 * For ray r its hits, their integrals I and distances d, and their order (ascending by d as fp32 with
 * -0 == +0, then by sphere index) are those of grace_trace_emission_absorption_f4.  Then, in fp64, per
 * channel c, over the ordered hits k with sphere i_k (C = n_channels, L = d_luminosity):
 *   a_kc   = (double)d_absorption[i_k * C + c] * (double)I_k
 *   tau_kc = sum over m < k of a_mc
 *   dep_kc = (double)L[r * C + c] * exp(-tau_kc) * (-expm1(-a_kc))               absorbed by hit k
 *   d_transmitted[r * C + c] = fl32( (double)L[r * C + c] * exp(-sum_k a_kc) )
 * and d_deposit[i * C + c] is the sum of dep_kc over every (ray, hit) with i_k == i.  By construction
 * sum_i deposit[i, c] + sum_r transmitted[r, c] = sum_r L[r, c] up to rounding, whatever the optical
 * depths: the scheme conserves photons.  Rays without hits transmit L unchanged; spheres nobody hits
 * get +0.0.
 * The sum over rays is made in 64-bit fixed point, so it does not depend on arrival order.  Per
 * channel, with M_c = max_r |L[r, c]|, e_c the integer with 2^(e_c - 1) <= M_c < 2^(e_c) and
 * b = ceil(log2(n_rays)):
 *   q_c  = 2^(e_c + b - 62)                        (d_quantum[c]; 0.0 when M_c == 0)
 *   u_kc = round-half-even( dep_kc / q_c )         (exact scaling; a signed 64-bit integer)
 *   d_deposit[i * C + c] = (double)( sum of u_kc ) * q_c
 * For absorption >= 0 and finite L, |dep_kc| <= |L_rc| < 2^(e_c) and a sphere is hit by at most
 * n_rays <= 2^b rays, so the integer sum stays below 2^62 plus at most 2^31 units of rounding: it
 * cannot overflow.  The price: a hit that absorbs less than q_c / 2 deposits nothing, i.e. less than
 * 2^(b - 62) of the brightest ray (2^-42 for 2^20 rays).  Integer addition is associative, so
 * d_deposit is bit-identical from run to run, across budgets, packet widths, contexts, streams and
 * any permutation of the rays (with L permuted alike); d_transmitted[r] depends on ray r alone.  A
 * caller that sums deposits across devices and needs the same property sums the exact integers
 * deposit / q_c (with one q_c for all ranks).
 * Against an evaluation of the formulas in another order with another libm, m_i the number of rays
 * that hit sphere i and n_r, tau_rc the hits and optical depth of ray r:
 *   |deposit[i,c] - ref| <= m_i q_c + sum over the hits on i of 8 (n_r + 8) 2^-53 max(1, tau_rc) |dep_kc|
 *   |transmitted - ref|  <= ulp32(ref) / 2 + 8 (n_r + 8) 2^-53 max(1, tau_rc) |ref|
 * Outside the stated domain (negative absorption, non-finite L or absorption) the values of the
 * affected channels are unspecified, but nothing faults: dep / q is clamped to [-2^62, 2^62], NaN
 * to 0, before it becomes an integer.
 * Batches, the byte budget (grace_trace_set_ordered_budget), the tiers and the stats hook are those
 * of grace_trace_emission_absorption_f4; the int64 accumulators (8 bytes per sphere and channel) live
 * in the workspace for the length of the call.  GRACE_INVALID_ARGUMENT for n_channels outside 1..64,
 * null d_luminosity / d_absorption / d_deposit and counts out of range, checked before any launch;
 * zero rays: GRACE_OK, d_deposit and d_quantum zeroed (d_luminosity may then be null).
 * Periodic boxes: grace_trace_absorption_deposit_periodic_f4 below. */
grace_status grace_trace_absorption_deposit_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                               size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                               const int* d_leaves, const int* d_root,
                                               const float* d_luminosity, const float* d_absorption,
                                               int n_channels, double* d_deposit, float* d_transmitted,
                                               double* d_quantum, grace_stream stream);
/* Velocity-space absorption spectra along rays -- an extension the reference lacks: the optical depth
 * of an absorption line (Lyman-alpha forest, metal lines, 21 cm) as a function of velocity along each
 * ray, every hit a thermally broadened Gaussian integrated over the velocity bins it reaches.
 * Inputs: rays, float4 spheres and the tree as for the other traces; d_amount [n_spheres * C] fp32,
 * what a unit of the line integral I contributes to the column of channel c (species / line);
 * d_width [n_spheres * C] fp32, the Doppler parameter b; d_velocity [n_spheres * 3] fp32; all in tree
 * order, read on every call; 1 <= C = n_channels <= 16.  grid: a host pointer, read before the call
 * returns.  Outputs: d_tau [n_rays * C * n_bins] fp32, every element written; d_column [n_rays * C]
 * fp32, or null.
 * For ray r its hits, their integrals I and distances d (the projection of the centre on the ray), and
 * their order (ascending by d as fp32 with -0 == +0, then by sphere index) are those of
 * grace_trace_emission_absorption_f4.  Then, in fp64, over the ordered hits k with sphere i_k and the
 * ray's direction (dx, dy, dz) as stored in the ray:
 *   N_kc    = (double)d_amount[i_k * C + c] * (double)I_k                  column of hit k in channel c
 *   v_k     = hubble * (double)d_k + (((double)vx * dx + (double)vy * dy) + (double)vz * dz)
 *   b_kc    = (double)d_width[i_k * C + c]
 *   e_u     = v0 + u * dv                                                   edge u, u any integer
 *   P_kc(u) = 0.5 * ( erf((e_{u+1} - v_k) / b_kc) - erf((e_u - v_k) / b_kc) )   the Gaussian over bin u
 *   window of hit k in channel c: u_lo = floor((v_k - 6 b_kc - v0) / dv) .. u_hi = floor((v_k + 6 b_kc - v0) / dv)
 *   periodic == 0:  d_tau[(r * C + c) * n_bins + j] = fl32( (1 / dv) * sum_k [u_lo <= j <= u_hi] N_kc P_kc(j) )
 *   periodic != 0:  d_tau[(r * C + c) * n_bins + j] = fl32( (1 / dv) * sum_k sum_{u in window, u mod n_bins == j} N_kc P_kc(u) )
 *   d_column[r * C + c] = fl32( sum_k N_kc )
 * for 0 <= j < n_bins.  The profile is integrated over the bin, not sampled at its centre: a line
 * narrower than a bin is not lost, and dv * sum_j tau[r, c, j] equals column[r, c] up to erfc(6) =
 * 2.2e-17 per hit and rounding -- always in periodic mode, and in window mode when no window leaves
 * [0, n_bins).  Flux is exp(-tau), left to the caller.
 * Per bin the terms are added hit by hit in depth order and, within one hit, in ascending u.  A ray's
 * spectrum is therefore a function of its ordered hit list alone: bit-identical from run to run, for
 * any budget, packet width, context and stream, and whatever the other rays of the call or the ray's
 * place among them.
 * A hit whose width is <= 0, NaN or infinite adds nothing to d_tau in that channel (it still counts
 * in d_column); a hit with a non-finite v_k adds nothing to d_tau.  In periodic mode a window is
 * clipped to n_bins bins either side of v_k's bin, so no input makes the work per hit exceed
 * 2 n_bins + 1 bins; a width above a quarter of the period n_bins * dv is outside the domain (values
 * unspecified), and so is |v_k - v0| / dv >= 2^52 (the hit adds nothing).  Rays without hits get zeros.
 * Against an evaluation of the formulas in another order with another libm, with eps = 2^-53, n_r
 * the ray's hits and V_k = |v0| + n_bins dv + |hubble d_k| + |vx dx| + |vy dy| + |vz dz|:
 *   |tau - ref| <= ulp32(ref) / 2 + eps sum_k (|N_kc| / dv) 16 (1 + V_k / b_kc) + 8 (n_r + 8) eps sum_k |term_k|
 * plus |N_kc| / dv * erfc(6) for every hit whose window's edge falls in another bin on the other
 * side; d_column is within ulp32(ref) / 2 + 8 (n_r + 8) eps sum_k |N_kc|.
 * Batches, the byte budget (grace_trace_set_ordered_budget), the tiers and the stats hook are those
 * of grace_trace_emission_absorption_f4; the call needs no workspace of its own beyond theirs.
 * GRACE_INVALID_ARGUMENT, before any launch, for n_channels outside 1..16, n_bins outside 1..4096, dv
 * not a positive finite number, non-finite v0 or hubble, null grid / d_amount / d_width / d_velocity /
 * d_tau and counts out of range; zero rays: GRACE_OK, nothing written.
 * Not here: Voigt (damped) profiles, double4 spheres, fp64 outputs.
 * Periodic boxes (of the SCENE; `periodic` below is the velocity grid's): grace_trace_spectra_periodic_f4 below. */
typedef struct grace_spectrum_grid {
    double v0;        /* lower edge of bin 0 */
    double dv;        /* bin width, > 0 */
    int    n_bins;    /* 1 .. 4096 */
    int    periodic;  /* 0: the bins are a window; 1: velocity wraps with period n_bins * dv */
    double hubble;    /* velocity per unit length along the ray; 0 for none */
} grace_spectrum_grid;
grace_status grace_trace_spectra_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                    size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                    const int* d_leaves, const int* d_root,
                                    const float* d_amount, const float* d_width, const float* d_velocity,
                                    int n_channels, const grace_spectrum_grid* grid, float* d_tau,
                                    float* d_column, grace_stream stream);
/* The byte budget of a batch's per-hit arrays (process-wide; 0 restores the default, 1 GiB).  A
 * target, never an error: a ray with more hits than the budget holds is a batch of its own.  The
 * workspace grows to about the budget plus 12 bytes a ray plus the per-hit walk's own buffers. */
grace_status grace_trace_set_ordered_budget(size_t bytes);
/* The fused kernel's tiers: rays of up to *wave_max_hits hits are ordered by one wave in LDS, of up
 * to *block_max_hits by a 256-thread workgroup in LDS, longer ones in global memory. */
grace_status grace_trace_ordered_limits(int* wave_max_hits, int* block_max_hits);
/* Measurement hook (process-wide): when enabled, every grace_trace_emission_absorption_f4 and
 * grace_trace_absorption_deposit_f4 and grace_trace_spectra_f4 call times its phases with events,
 * synchronises the stream before it returns and records what it did (ms_composite: the call's own fused kernels);
 * grace_trace_ordered_last_stats returns the last call's record. */
typedef struct grace_ordered_stats {
    unsigned long long batches;       /* batches the rays were cut into */
    unsigned long long total_hits;    /* hits of all rays */
    unsigned long long rays_wave, rays_block, rays_global;   /* rays per tier (no hits: wave) */
    unsigned long long budget_bytes, frame_bytes;            /* the budget used; workspace bytes of the call */
    float ms_count, ms_trace, ms_composite;   /* counting walk + scan; per-hit walks; fused kernels */
} grace_ordered_stats;
grace_status grace_trace_ordered_enable_stats(int enabled);
grace_status grace_trace_ordered_last_stats(grace_ordered_stats* h_stats);
/* Per-hit outputs written from d_ray_offsets[ray] (RayEntry_from_array +
 * OnHit_sphere_individual, include/grace/cuda/functors/trace.cuh:44-60,196-235). */
grace_status grace_trace_hits_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                 size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                 const int* d_leaves, const int* d_root,
                                 const int* d_ray_offsets, int* d_hit_indices,
                                 float* d_hit_integrals, float* d_hit_distances,
                                 grace_stream stream);
/* Instrumented walk: per ray {nodes visited, leaves visited, spheres tested, hits} for that
 * ray alone (4 x uint32 per ray) -- the counts SURVEY.md section 8d's algorithmic-bytes
 * formula is built from.  Not part of the reference API. */
grace_status grace_trace_stats_f4(const void* d_rays, size_t n_rays, const float* d_spheres,
                                  size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                  const int* d_leaves, const int* d_root,
                                  uint32_t* d_stats4, grace_stream stream);

/* The per-hit kernel integral of OnHit_sphere_cumulate / OnHit_sphere_individual
 * (include/grace/cuda/functors/trace.cuh:181-186, 221-224) evaluated on arrays:
 * out[i] = lerp(50 * sqrt(b2[i]) / h[i], table) / h[i]^2, bit-for-bit the traversal's value, with
 * the context's SPH kernel table (grace_trace_set_sph_kernel). */
grace_status grace_hit_integrals_f32(const float* d_b2, const float* d_h, size_t n, float* d_out,
                                     grace_stream stream);

/* Packets are formed from 64 consecutive rays of a coherence order computed inside every
 * trace call (Morton code over the varying ray coordinates + stable sort); results per ray
 * do not depend on it.  0 disables it: packets then follow the caller's ray order, as in
 * the reference.  Default 1.  Not part of the reference API. */
grace_status grace_trace_set_ray_reorder(int enabled);

/* Measurement hook: when enabled, HIP events are recorded on the call's stream directly
 * around the traversal kernel of every trace call (not around its pre-passes);
 * grace_trace_last_kernel_ms waits for the last one and returns its duration. */
grace_status grace_trace_enable_timing(int enabled);
grace_status grace_trace_last_kernel_ms(float* h_ms);

/* Measurement hook: 1 if the last hit-count / cumulative / per-hit trace ran the kernel
 * instantiation with the origin-lattice cull (chosen on the device: all rays share one
 * axis-aligned direction and the scene holds spheres smaller than the mean ray cell), else 0.
 * Valid until the next library call on the device.  Results never depend on the choice. */
grace_status grace_trace_last_lattice(int* h_lattice);

/* Waves per 64-ray packet for the hit-count and cumulative traces: 1, 2, 4 or 8 (each wave
 * owns 8/K of the 8 interleaved primitive classes over which the column density is summed), or
 * -1 (default) = as many as it takes to put >= 16384 waves on the chip (>= 4096 if all rays of
 * the batch share one direction: decided on the device from the ray extents; an unweighted
 * column-density call that runs from a packet plan takes 8 up to 8192 packets and 4 up to 16384,
 * whatever the directions: its waves repeat nothing).  An explicit value holds for every kernel of the call.
 * The results do not depend on it (see csrc/trace.hip, "class-ordered sums and packet splitting"). */
grace_status grace_trace_set_packet_split(int waves_per_packet);

/* Rays per packet of the per-hit and triangle traces (which cannot split a packet among waves):
 * 64, 32 or 16, or -1 (default) = halve while the call has fewer than 4096 packets.  Results do
 * not depend on it. */
grace_status grace_trace_set_packet_width(int rays_per_packet);

/* Column-density trace (grace_trace_cumulative_f4) only.  0 (default): each hit's kernel
 * integral is evaluated with the hardware sqrt (1 ulp) and an fp32 table lerp -- within a few
 * ulp of the reference arithmetic per term, column densities within 1e-6 of the fp64 sum
 * (stated tolerance 1e-5).  1: the reference's arithmetic bit for bit (correctly rounded
 * sqrt, fp64 lerp of the fp64 table; functors/trace.cuh:181-186, interpolate.h:11-39) --
 * the result is then bit-identical to the CPU oracle's class-ordered sum, ~20 % slower.
 * The per-hit outputs (grace_trace_hits_f4, grace_hit_integrals_f32) always use the latter. */
grace_status grace_trace_set_exact_integrals(int enabled);

/* ---- SPH kernel of the integrating traces (not part of the reference API) -----------------------
 * A sphere's w is the kernel's support radius H: W(r, H) = H^-3 f(r / H), zero for r >= H, with
 * 4 pi int_0^1 f(q) q^2 dq = 1.  Every integrating trace -- the column densities of
 * grace_trace_cumulative_f4 / _d4 / _f4_f64 and _weighted_f4, the per-hit integrals of
 * grace_trace_hits_f4 / _d4 / _f4_f64, and grace_hit_integrals_f32 -- adds, per hit,
 * lerp(F, 50 sqrt(b^2) / H) / H^2 with the same operations in every mode; F is the kernel's table of
 * 51 line integrals F_i = int f(sqrt((i/50)^2 + z^2)) dz over the whole chord, F_50 = 0.  Hit
 * counts, stats and closest-triangle traces do not use it.  The kernel is a per-context knob; a
 * trace call uses the table selected when it is enqueued.  Default: GRACE_SPH_KERNEL_CUBIC, the
 * reference's cubic spline (M4) table bit for bit.  The other built-in tables are the exact
 * integrals of their kernels (INTEGRATION.md lists them and their lerp's volume bias). */
#define GRACE_SPH_KERNEL_CUSTOM      (-1)
#define GRACE_SPH_KERNEL_CUBIC       0
#define GRACE_SPH_KERNEL_QUARTIC     1   /* M5 */
#define GRACE_SPH_KERNEL_QUINTIC     2   /* M6 */
#define GRACE_SPH_KERNEL_WENDLAND_C2 3
#define GRACE_SPH_KERNEL_WENDLAND_C4 4
#define GRACE_SPH_KERNEL_WENDLAND_C6 5
/* Selects a built-in kernel (0..5): only switches a pointer, no synchronisation.
 * GRACE_INVALID_ARGUMENT for anything else (GRACE_SPH_KERNEL_CUSTOM included). */
grace_status grace_trace_set_sph_kernel(int kind);
/* Selects a caller's table of n == 51 host doubles, every one finite and >= 0, the last one 0.
 * The table is copied to a device buffer of the context; the call SYNCHRONISES THE DEVICE first
 * (hipDeviceSynchronize), because trace calls still queued may read the buffer it overwrites.
 * Anything else: GRACE_INVALID_ARGUMENT, and the active kernel stays unchanged. */
grace_status grace_trace_set_sph_kernel_table(const double* h_table, int n);
/* The active kernel: its GRACE_SPH_KERNEL_* (GRACE_SPH_KERNEL_CUSTOM for a caller's table) and its
 * 51 values.  Either pointer may be NULL. */
grace_status grace_trace_get_sph_kernel(int* h_kind, double* h_table51);
/* A built-in kernel's 51 values (0..5, else GRACE_INVALID_ARGUMENT).  Host only: needs no context
 * and no device. */
grace_status grace_sph_kernel_table(int kind, double* h_out51);

/* Subtrees with at most this many primitives are swept -- one test per cluster of 64 consecutive
 * primitives, then culling rounds over the surviving clusters -- instead of being descended
 * (results per ray unchanged).  0 disables; -1 (default) = 16384 for axis-aligned packets (whose
 * cluster test is a sharp box-rectangle overlap), 512 for the others. */
grace_status grace_trace_set_treelet_size(int max_primitives);

/* Measurement switches (results never depend on them).  Lattice split: waves per packet that a
 * batch of >= 16384 packets gets when the device finds spheres smaller than the ray spacing in the
 * scene (clustered SPH data): 0 = one wave per packet, 2, 4 (default) or 8.  Hits staging: 0 = the
 * split per-hit walk of small batches always stores hits directly (default 1: heavy packets stage
 * them in LDS). */
grace_status grace_trace_set_lattice_split(int waves_per_packet);
grace_status grace_trace_set_hits_staging(int enabled);

/* Cached trace records.  Every trace call derives, from the primitives and the tree alone,
 * per-sphere records ({x, y, z, h^2}, {1/h, 1/h^2}), every node's primitive span and one box per
 * cluster of 64 consecutive primitives; and from the rays alone the coherence order in which
 * packets are formed (see csrc/trace.hip).  The reference's traces are stateless
 * (trace_sph.cuh:58-241 rebuild even the 51-entry table per call) and so is every call here for its
 * caller -- but a context KEEPS the records of the scene and of the ray batch it was last given:
 * when a call names the same arrays (pointers and sizes) as the call before it, the records are
 * derived into buffers of the context's own, and later calls on those arrays reuse them.
 *
 * A cached record is never trusted on pointer equality.  Before every use, one streaming pass
 * reduces the arrays the call was given to a 128-bit signature and compares it -- on the device,
 * no host round trip -- with the signature the cached records were derived from; if the caller
 * (or an allocator that handed out the same address again) changed the contents, the records are
 * recomputed in place by the same call.  Results are therefore always those of a fresh derivation;
 * the signature pass costs about a fifth of one (0.06 ms against 0.35 ms at 10^7 particles and
 * 10^6 rays).
 *
 * grace_trace_prepare_f4 / _tri / _rays fill the cache NOW instead of at the second call, and pin
 * it: it is kept until released or replaced by another prepare.  One scene and one ray batch per
 * context.  grace_trace_set_cache_validation(0) switches the signature pass off for a caller who
 * promises not to modify cached arrays until grace_trace_release() / _release_rays() (this
 * library's own sort, build and ray-generator entry points then drop the cache themselves when they
 * write to one of its arrays); default 1.  grace_trace_set_cache_auto(0): cache on
 * grace_trace_prepare_* only; default 1.  Not part of the reference API. */
grace_status grace_trace_prepare_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                    size_t n_nodes, const int* d_leaves, grace_stream stream);
grace_status grace_trace_prepare_tri(const float* d_tris, size_t n_tris, const int* d_nodes,
                                     size_t n_nodes, const int* d_leaves, grace_stream stream);
grace_status grace_trace_release(void);
grace_status grace_trace_prepare_rays(const void* d_rays, size_t n_rays, grace_stream stream);
grace_status grace_trace_release_rays(void);
grace_status grace_trace_set_cache_validation(int enabled);
grace_status grace_trace_set_cache_auto(int enabled);

/* Packet plan of the column-density traces (grace_trace_cumulative_f4, _weighted_f4).  Which groups,
 * clusters and candidates a packet of axis-aligned rays has to look at depends on the rays, their
 * coherence order and the scene records only: once BOTH caches above serve a call (each has seen
 * its arrays repeated, or was prepared), that call records the cull -- per packet and summation
 * class the primitive indices of its survivors, 4 bytes each, with a 4-byte header per dense
 * round -- and later calls on the same
 * arrays (the next frame field, the next group of weight channels, another SPH kernel, any packet
 * split) run the survivor loops from the plan without repeating it.  The plan lives and dies with
 * the two caches; when a signature shows that the scene or the rays have changed, the same call
 * re-records it in place on the device.  The call that first records a plan synchronises its
 * stream once (it sizes the plan on the host).  A batch with a packet that is not axis-aligned, or
 * whose plan would exceed the byte budget, has no plan and runs as before.  Results are bit for bit
 * those without a plan.
 * grace_trace_set_plan(0 / 1): off / on (default: see DESIGN.md section 6).
 * grace_trace_set_plan_budget(bytes): the device memory a plan may take (default 2 GiB; the
 * 1024^2 frame over 10^7 particles takes 1.475 GB in the sub-tile layout and 530.5 MB in the
 * ordinary one).
 * grace_trace_plan_bytes: the device memory of the current plan (0: none).
 * grace_trace_last_plan_used (measurement hook, in the manner of grace_trace_last_lattice): 1 if
 * the last column-density trace ran the planned kernel, else 0.  Synchronises.
 * grace_trace_plan_stats (diagnostic): seven figures of the plan the last column-density trace ran
 * from, as its last recording tallied them (zeros if it ran from none): h_stats[0] entries,
 * [1] survivors, [2] dense rounds (runs of consecutive entries of a list that the planned kernel
 * works off in one survivor loop: at most 64 survivors, one lean / fat class), [3] rounds of exactly
 * 64 survivors, [4] rounds closed because the next entry would have taken them past 64, [5] rounds
 * closed because the next entry's lean / fat bits differed, [6] the largest round's survivors.
 * Synchronises; a steady-state call pays nothing for it.
 * grace_trace_plan_loops (diagnostic): the survivor loops the last column-density trace's planned
 * kernel runs over that plan -- h_loops[0] their number, [1] the survivors of the largest (zeros if
 * it ran from none).  The unweighted kernel with the fast integral runs consecutive test-free
 * rounds of equal bits as one loop of up to 128 survivors; every other planned kernel runs one
 * loop per dense round (at most 64).  Synchronises.  With the sub-tile layout both figures are in
 * slots (four per step).
 * grace_trace_set_plan_subtiles(-1 / 0 / 1): the plan's sub-tile layout -- one survivor stream per
 * quadrant of 16 rays instead of one per packet, for the unweighted column-density trace with the
 * fast integral over packets of 64 rays; it takes about three times the memory of the ordinary
 * layout.  -1 (default): taken when the batch has enough packets and the streams drop enough of
 * the survivors' steps; 0: never; 1: whenever the call is eligible and the
 * plan fits the budget.  A change releases the current plan.  Results are bit for bit the same.
 * grace_trace_plan_subtiles (diagnostic): *h_used 1 if the last column-density trace ran from a
 * plan of the sub-tile layout, with *h_steps the steps of its lists and *h_slots the index words
 * of their streams that name a survivor (of 4 x steps; the rest name the null record); zeros
 * otherwise.  Synchronises.
 * Not part of the reference API. */
grace_status grace_trace_set_plan(int on);
grace_status grace_trace_set_plan_budget(size_t bytes);
grace_status grace_trace_plan_bytes(size_t* h_bytes);
grace_status grace_trace_last_plan_used(int* h_used);
grace_status grace_trace_plan_stats(unsigned long long* h_stats /* [7] */);
grace_status grace_trace_plan_loops(unsigned long long* h_loops /* [2] */);
grace_status grace_trace_set_plan_subtiles(int mode);
grace_status grace_trace_plan_subtiles(int* h_used, unsigned long long* h_steps, unsigned long long* h_slots);

/* Reads (and clears) the traversal status word: GRACE_STACK_OVERFLOW if any packet ran out
 * of its 128-entry stack since the last check (the reference only asserts this in
 * GRACE_DEBUG builds, bintree_trace.cuh:164); GRACE_INVALID_ARGUMENT if grace_range_neighbours_f4
 * met a row of another length than its list.  Synchronises. */
grace_status grace_trace_status(grace_stream stream);

/* ---- scans ---------------------------------------------------------------------------
 * thrust::exclusive_scan of hit counts (include/grace/cuda/trace_sph.cuh:135-137).
 * In place allowed.  *h_total (optional) receives the grand total, computed in 64 bits:
 * synchronises if given.  The offsets themselves wrap modulo 2^32 like the reference's int scan;
 * a caller that turns them into array positions (trace_sph, trace_with_sentinels_sph) must
 * refuse a total above INT32_MAX -- the host-side mirrors do, with std::invalid_argument /
 * ValueError. */
grace_status grace_scan_exclusive_i32(const int* d_in, size_t n, int* d_out, long long* h_total,
                                      grace_stream stream);
/* grace::exclusive_segmented_scan (include/grace/cuda/scan.cuh:15-37): per-segment
 * exclusive prefix sums; segment s covers [offsets[s], offsets[s+1]) (last: to n); empty
 * segments allowed.  d_data and d_results may alias. */
grace_status grace_segscan_exclusive_f32(const int* d_segment_offsets, size_t n_segments,
                                         const float* d_data, size_t n, float* d_results,
                                         grace_stream stream);
grace_status grace_segscan_exclusive_f64(const int* d_segment_offsets, size_t n_segments,
                                         const double* d_data, size_t n, double* d_results,
                                         grace_stream stream);
/* Pieces of trace_with_sentinels_sph (include/grace/cuda/trace_sph.cuh:171-241):
 * offsets[i] += i (thrust::transform with a counting iterator, :205-208) and the sentinel
 * fill of the per-hit arrays (:212-214; 32-bit pattern, so int and float sentinels alike). */
grace_status grace_add_iota_i32(int* d_values, size_t n, grace_stream stream);
grace_status grace_fill_u32(void* d_values, size_t n, uint32_t bits, grace_stream stream);
/* detail::multiply_by_weights (include/grace/cuda/kernels/weights.cuh:13-27). */
grace_status grace_multiply_by_weights_f32(const float* d_unweighted, size_t n,
                                           const float* d_weights, const uint32_t* d_weight_map,
                                           float* d_weighted, grace_stream stream);
/* ... with Real = double (scan.cuh:43-58 is a template on Real). */
grace_status grace_multiply_by_weights_f64(const double* d_unweighted, size_t n,
                                           const double* d_weights, const uint32_t* d_weight_map,
                                           double* d_weighted, grace_stream stream);

/* ---- per-ray sort of hits by distance: grace::sort_by_distance
 *      (include/grace/cuda/sort.cuh:100-131): within each ray's segment distances become
 *      non-decreasing (equal distances keep their order); hit_indices and hit_data (either
 *      may be NULL) are permuted by the same map. ---------------------------------------- */
grace_status grace_sort_by_distance_f32(float* d_distances, const int* d_ray_offsets,
                                        size_t n_rays, size_t n_hits, int* d_hit_indices,
                                        float* d_hit_data, grace_stream stream);

/* sort_by_distance<double, int, double>: the double outputs of grace_trace_hits_d4. */
grace_status grace_sort_by_distance_f64(double* d_distances, const int* d_ray_offsets,
                                        size_t n_rays, size_t n_hits, int* d_hit_indices,
                                        double* d_hit_data, grace_stream stream);

/* ---- ray inputs (deterministic generators; the reference's cuRAND streams are
 *      device-specific by its own account, include/grace/cuda/kernels/gen_rays.cuh:21-24) */
/* orthographic_projection_rays specialised as orthogonal_rays_z
 * (tests/helper/rays.cuh:55-79; kernels/gen_rays.cuh:319-360,667-725). mins4/maxs4 host. */
grace_status grace_rays_orthogonal_z(int n_side, const float* h_mins4, const float* h_maxs4,
                                     void* d_rays, float* h_area, grace_stream stream);
/* pinhole_camera_rays (kernels/gen_rays.cuh:362-395,727-789), Real = float; fovy in radians.
 * res_x * res_y must be below 2^31, as for orthogonal_z and plane_parallel_random: more is
 * GRACE_INVALID_ARGUMENT and d_rays is not written. */
grace_status grace_rays_pinhole(int res_x, int res_y, const float* h_camera, const float* h_look_at,
                                const float* h_view_up, float fovy, float length, void* d_rays,
                                grace_stream stream);
/* One source, HEALPix nested pixel centres (RayVectorGeneration/src/generateRays.c:57-59). */
grace_status grace_rays_healpix(int nside, float ox, float oy, float oz, float length,
                                void* d_rays, grace_stream stream);
/* Isotropic rays from one origin, sorted by ray_dir_morton_key
 * (kernels/gen_rays.cuh:38-43,104-170 uniform_random_rays); own counter-based generator. */
grace_status grace_rays_isotropic(size_t n_rays, float ox, float oy, float oz, float length,
                                  uint64_t seed, void* d_rays, grace_stream stream);

/* uniform_random_rays_single_octant (gen_rays.cuh:62-97; kernels/gen_rays.cuh:161-204,484-517):
 * octant 0 (MMM) .. 7 (PPP), bit 2 = x, bit 1 = y, bit 0 = z, set = positive component. */
grace_status grace_rays_isotropic_octant(size_t n_rays, float ox, float oy, float oz, float length,
                                         int octant, uint64_t seed, void* d_rays,
                                         grace_stream stream);
/* one_to_many_rays (gen_rays.cuh:99-208; kernels/gen_rays.cuh:206-243,519-611): ray i goes from
 * the origin to point i (direction normalised, length = distance).  Points: elems_per_point
 * floats/doubles each, x y z first.  sort_type: 0 NoSort, 1 DirectionSort (ray_dir_morton_key),
 * 2 EndPointSort (30-bit Morton key of the end point within h_bot/h_top; the reference's
 * bounds-free overload passes AABB_bot twice, gen_rays.cuh:121-122 -- not reproduced: pass the
 * real bounds).  Anything else: GRACE_INVALID_ARGUMENT (std::invalid_argument there). */
grace_status grace_rays_one_to_many(size_t n_rays, float ox, float oy, float oz,
                                    const void* d_points, int is_double, int elems_per_point,
                                    int sort_type, const float* h_bot, const float* h_top,
                                    void* d_rays, grace_stream stream);
/* plane_parallel_random_rays (gen_rays.cuh:210-262; kernels/gen_rays.cuh:245-317,613-665): a
 * width x height grid of cells spanned by w and h from base, one ray per cell from a random
 * point of the cell, direction normalize(cross(w, h)).  base, w, h: host float[3]. */
grace_status grace_rays_plane_parallel_random(int width, int height, const float* h_base,
                                              const float* h_w, const float* h_h, float length,
                                              uint64_t seed, void* d_rays, grace_stream stream);
/* orthographic_projection_rays (gen_rays.cuh:264-329; kernels/gen_rays.cuh:319-360,667-725),
 * Real = float: ray 0 is the top-left pixel, x fastest. */
grace_status grace_rays_orthographic_projection(int res_x, int res_y, const float* h_camera,
                                                const float* h_look_at, const float* h_view_up,
                                                float vertical_extent, float length,
                                                void* d_rays, grace_stream stream);

/* ---- double4 spheres: the reference's templates with Real4 = double4, Real = double
 *      (build_sph.cuh:84-126, trace_sph.cuh:57-110).  Keys: grace_morton_keys{30,63}_points;
 *      sort: grace_sort_pairs_u32/u64 with 32-byte records. -------------------------------- */
/* euclidean_deltas_sph<double4>: DeltaEuclidean forms the squared distance in double and returns
 * it as float (generic/functors/albvh.h:44-74); deltas[n + 1] floats, +inf at both ends. */
grace_status grace_deltas_euclid_d4(const double* d_spheres, size_t n, float* d_deltas,
                                    grace_stream stream);
/* The same with a device_vector<double> of deltas (build_tree<double4> declares
 * device_vector<Real> deltas, tests/helper/tree.cuh:20-24: the functor's float widened), and
 * surface_area_deltas_sph<double4> (build_sph.cuh:97-105; generic/functors/albvh.h:84-126 with
 * AABBSphere narrowing centre -+ radius to float3, generic/functors/aabb.h:9-26). */
grace_status grace_deltas_euclid_d4_f64(const double* d_spheres, size_t n, double* d_deltas,
                                        grace_stream stream);
grace_status grace_deltas_area_d4(const double* d_spheres, size_t n, float* d_deltas,
                                  grace_stream stream);
grace_status grace_deltas_area_d4_f64(const double* d_spheres, size_t n, double* d_deltas,
                                      grace_stream stream);
/* ALBVH_sph<Real4, DeltaType> (build_sph.cuh:118-124) for the remaining delta types: 64-bit XOR
 * deltas (morton_keys63_sort_sph -> XOR_deltas_sph -> ALBVH_sph), double deltas, and double4
 * spheres with XOR deltas.  DeltaComp is thrust::less in all of them (albvh.cuh:1045-1072); a
 * caller-defined comparator functor cannot cross a C ABI. */
grace_status grace_albvh_build_f4_u64(const float* d_spheres, size_t n, const uint64_t* d_deltas,
                                      int max_per_leaf, int* d_nodes, int* d_leaves, int* d_root,
                                      size_t* h_n_leaves, grace_stream stream);
grace_status grace_albvh_build_f4_f64(const float* d_spheres, size_t n, const double* d_deltas,
                                      int max_per_leaf, int* d_nodes, int* d_leaves, int* d_root,
                                      size_t* h_n_leaves, grace_stream stream);
grace_status grace_albvh_build_d4_f64(const double* d_spheres, size_t n, const double* d_deltas,
                                      int max_per_leaf, int* d_nodes, int* d_leaves, int* d_root,
                                      size_t* h_n_leaves, grace_stream stream);
grace_status grace_albvh_build_d4_u32(const double* d_spheres, size_t n, const uint32_t* d_deltas,
                                      int max_per_leaf, int* d_nodes, int* d_leaves, int* d_root,
                                      size_t* h_n_leaves, grace_stream stream);
grace_status grace_albvh_build_d4_u64(const double* d_spheres, size_t n, const uint64_t* d_deltas,
                                      int max_per_leaf, int* d_nodes, int* d_leaves, int* d_root,
                                      size_t* h_n_leaves, grace_stream stream);
/* ALBVH_sph<double4>: same tree builder; leaf / node boxes are AABBSphere's float3 corners of the
 * double centre -+ radius (generic/functors/aabb.h:9-26).  Same output layout as _f4. */
grace_status grace_albvh_build_d4(const double* d_spheres, size_t n, const float* d_deltas,
                                  int max_per_leaf, int* d_nodes, int* d_leaves, int* d_root,
                                  size_t* h_n_leaves, grace_stream stream);
/* trace_hitcounts_sph / trace_cumulative_sph / trace_sph pass 2 <double4, (int,) double>
 * (trace_sph.cuh:57-168): sphere_hit and the kernel integral in double (ray members are float,
 * generic/intersect.h:9-55), one running double sum per ray in ascending primitive index; per-hit
 * integrals and distances are double.  Same kernel as the float path (ray coherence order,
 * cluster tests, culling rounds) walking float records that contain the double spheres; every
 * surviving candidate is then tested against the caller's double4 record. */
grace_status grace_trace_hitcounts_d4(const void* d_rays, size_t n_rays, const double* d_spheres,
                                      size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                      const int* d_leaves, const int* d_root, int* d_hit_counts,
                                      grace_stream stream);
grace_status grace_trace_cumulative_d4(const void* d_rays, size_t n_rays, const double* d_spheres,
                                       size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                       const int* d_leaves, const int* d_root, double* d_sums,
                                       grace_stream stream);
grace_status grace_trace_hits_d4(const void* d_rays, size_t n_rays, const double* d_spheres,
                                 size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                 const int* d_leaves, const int* d_root, const int* d_ray_offsets,
                                 int* d_hit_indices, double* d_hit_integrals,
                                 double* d_hit_distances, grace_stream stream);
/* Same status word as grace_trace_status (kept for callers of the round-1 interface). */
grace_status grace_trace_status_d4(grace_stream stream);

/* trace_hitcounts_sph / trace_cumulative_sph / trace_sph pass 2 <float4, (int,) double>, mixed
 * precision (trace_sph.cuh:81-241 with RayData_sphere<double, double>): sphere_hit<float4, double>
 * (generic/intersect.h:9-55) -- p = s - o subtracted in float then widened, dot_p and b2 in double,
 * tested against the float product w * w --; per-hit terms as OnHit_sphere_cumulate /
 * OnHit_sphere_individual<int, double> promote them (functors/trace.cuh:164-235,
 * generic/interpolate.h:11-39): column-density terms are floats (ir, b, the lerp's result and
 * the ir * ir scaling in float) added into the class-ordered double sum of
 * grace_trace_cumulative_d4; per-hit integrals and distances are double, from ir = 1.f / w.
 * grace_trace_hitcounts_f4_f64 counts with THIS test -- it is the hit-count pass of the mixed
 * trace_sph (the reference sizes that pass with the float test, trace_sph.cuh:121-141;
 * INTEGRATION.md) -- and grace_trace_hitcounts_f4 keeps the float test.  The walk runs on float
 * records of their own, inflated so that every cull keeps what the fp64 test can accept; they
 * are derived per call and never enter the scene cache.  grace_trace_set_exact_integrals does
 * not apply.  Status word: grace_trace_status. */
grace_status grace_trace_hitcounts_f4_f64(const void* d_rays, size_t n_rays, const float* d_spheres,
                                          size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                          const int* d_leaves, const int* d_root, int* d_hit_counts,
                                          grace_stream stream);
grace_status grace_trace_cumulative_f4_f64(const void* d_rays, size_t n_rays, const float* d_spheres,
                                           size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                           const int* d_leaves, const int* d_root, double* d_sums,
                                           grace_stream stream);
grace_status grace_trace_hits_f4_f64(const void* d_rays, size_t n_rays, const float* d_spheres,
                                     size_t n_spheres, const int* d_nodes, size_t n_nodes,
                                     const int* d_leaves, const int* d_root, const int* d_ray_offsets,
                                     int* d_hit_indices, double* d_hit_integrals,
                                     double* d_hit_distances, grace_stream stream);

/* ---- SPH interpolation at points (an extension the reference lacks) -----------------------------
 * The SPH field of the spheres (tree order, as traced) at points, with the context's SPH kernel
 * (grace_trace_set_sph_kernel; a sphere's w is the support radius H, W(r, H) = H^-3 f(r / H)):
 *   d_out[p * n_channels + c] = sum over spheres i containing point p of fl32(d_weights[i * n_channels + c] * W_ip)
 *   d_counts[p]               = number of spheres i containing point p
 * Weights in tree order as for grace_trace_cumulative_weighted_f4 (weights = m gives the density,
 * m / rho * A the field A); read on every call, never cached.  Containment is d2 < fl(H * H),
 * strict: a point on a sphere's surface is not contained; NaN points and points outside every
 * sphere get 0 and a count of 0.
 *
 * Arithmetic (fp32, every operation rounded, none fused), per point p and sphere {x, H}:
 *   d = p - x per component;  d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz));
 *   ih = fl(1 / H);  q = fl(sqrt_rn(d2) * ih);  u = max(fl(1 - q), 0);
 *   K = f(q), below;  W = fl(K * fl(fl(ih * ih) * ih));  term_c = fl(w_c * W).
 * f(q) with p4(t) = fl(fl(t*t) * fl(t*t)), constants rounded to fp32, the normalisation last:
 *   cubic (M4, support H):  q < 0.5 ? fl(fl(fl(fl(6q) - 6) * fl(q*q)) + 1) : fl(2 * fl(fl(u*u) * u)),  times 8/pi
 *   quartic:  t2 = max(fl(u - 0.4), 0), t3 = max(fl(u - 0.8), 0);
 *             fl(fl(p4(u) - fl(5 p4(t2))) + fl(10 p4(t3))),  times 25 2.5^4 / (32 pi)
 *   quintic:  t2 = max(fl(u - 1/3), 0), t3 = max(fl(u - 2/3), 0), p5(t) = fl(p4(t) * t);
 *             fl(fl(p5(u) - fl(6 p5(t2))) + fl(15 p5(t3))),  times 9 3^5 / (40 pi)
 *   Wendland C2:  fl(p4(u) * fl(fl(4q) + 1)),  times 21 / (2 pi)
 *   Wendland C4:  fl(fl(p4(u) * fl(u*u)) * fl(fl(q * fl(fl(q * 35/3) + 6)) + 1)),  times 495 / (32 pi)
 *   Wendland C6:  fl(fl(p4(u) * p4(u)) * fl(fl(q * fl(fl(q * fl(fl(32q) + 25)) + 8)) + 1)),  times 1365 / (64 pi)
 * (the functions of tools/gen_kernel_tables.py, written in u = 1 - q).  Each channel is summed in
 * the class order of the column densities: class (i >> 10) & 7, fp32 sums in ascending index within
 * each class, the 8 class sums added pairwise ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)).  The result is a
 * function of the point and the scene only: not of the point order, elems_per_point, the entry
 * point, the trace's cache knobs.
 *
 * Points: n_points records of elems_per_point (3..16) floats, x y z first (the layout of
 * grace_morton_keys30_points); outputs in the caller's order (the call orders points internally by
 * Morton keys against the tree's root box, computed and sorted on the device).
 * Grid: the lattice p(i, j, k) = origin + i u + j v + k w, per component
 * fl(fl(fl(o + fl(i*u)) + fl(j*v)) + fl(k*w)), 0 <= i < dims[0] ..., outputs row-major (k slowest,
 * i fastest); dims[2] == 1 is a slice (oblique slices allowed).  h_uvw9 = {u, v, w}.
 *
 * Either output may be NULL, not both; d_out needs non-NULL weights and 1 <= n_channels <= 64
 * (channels are walked four at a time).  GRACE_INVALID_ARGUMENT, nothing written: bad
 * elems_per_point, channel count, dimension or scene, or a custom SPH kernel table (there is no
 * f(q)).  Zero points: GRACE_OK, nothing written.  A packet that exhausts its 128-entry stack sets
 * the status word of grace_trace_status (GRACE_STACK_OVERFLOW); nothing is written out of bounds.
 * Stream-ordered, no host synchronisation, no allocation (the context workspace): capturable.
 * Periodic boxes: grace_interpolate_points_periodic_f4 / grace_interpolate_grid_periodic_f4 below. */
grace_status grace_interpolate_points_f4(const float* d_points, size_t n_points, int elems_per_point,
                                         const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                         size_t n_nodes, const int* d_leaves, const int* d_root,
                                         const float* d_weights, int n_channels,
                                         float* d_out, int* d_counts, grace_stream stream);
grace_status grace_interpolate_grid_f4(const float* h_origin3, const float* h_uvw9, const int* h_dims3,
                                       const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                       size_t n_nodes, const int* d_leaves, const int* d_root,
                                       const float* d_weights, int n_channels,
                                       float* d_out, int* d_counts, grace_stream stream);
/* Measurement hook (process-wide, results never depend on it): when enabled, every interpolation
 * call counts its survivor tests (active lanes x survivors of each culling round, all walks);
 * grace_interpolate_last_stats synchronises the device and returns the last call's count.
 * grace_trace_enable_timing / grace_trace_last_kernel_ms also time the interpolation walks. */
grace_status grace_interpolate_enable_stats(int enabled);
grace_status grace_interpolate_last_stats(unsigned long long* h_survivor_tests);

/* ---- SPH gradients at points (an extension the reference lacks) ---------------------------------
 * The gradient of the field of "SPH interpolation at points" above, differentiated term by term:
 * for point p, sphere i = {x, H} in tree order, channel c and component k in x, y, z
 *   d_grad[(p * n_channels + c) * 3 + k] = sum over spheres i containing point p of term_ick
 *   d_value[p * n_channels + c]          = exactly what grace_interpolate_points_f4 writes to d_out  (or NULL)
 *   d_counts[p]                          = exactly what it writes to d_counts                        (or NULL)
 * Containment, d, d2, ih and q are the interpolation's, bit for bit: d2 < fl(H * H), strict, and in
 * a periodic box d wrapped once per component ("Periodic boxes" below).  NaN points and points
 * outside every sphere get 0.
 *
 * New arithmetic (fp32, every operation rounded, none fused, IEEE divide and sqrt):
 *   r = sqrt_rn(d2);  q = fl(r * ih);  E = f'(q), below;
 *   G = fl(E * fl(fl(ih * ih) * fl(ih * ih)));                  H^-4 f'(q)
 *   n_k = fl(d_k * fl(1 / r));                                  the unit vector, formed first
 *   term_ick = fl(fl(w_ic * G) * n_k)        d2 > 0
 *   term_ick = +0 for every k                d2 == 0 (a select, not 0 * inf): a point at a sphere's
 *                                            centre gets no gradient from it; the sphere is counted.
 * f'(q) with u = max(fl(1 - q), 0), p3(t) = fl(fl(t*t) * t), p4 as above, p5(t) = fl(p4(t) * t),
 * p7(t) = fl(fl(p4(t) * fl(t*t)) * t), constants rounded to fp32, the normalisation of f last:
 *   cubic:        q < 0.5 ? fl(fl(fl(18q) - 12) * q) : fl(-6 * fl(u*u))
 *   quartic:      t2, t3 as in f;  fl(fl(fl(20 p3(t2)) - fl(4 p3(u))) - fl(40 p3(t3)))
 *   quintic:      t2, t3 as in f;  fl(fl(fl(30 p4(t2)) - fl(5 p4(u))) - fl(75 p4(t3)))
 *   Wendland C2:  fl(fl(-20 q) * p3(u))
 *   Wendland C4:  fl(fl(fl(-56/3 q) * fl(fl(5q) + 1)) * p5(u))
 *   Wendland C6:  fl(fl(fl(-22 q) * fl(fl(q * fl(fl(16q) + 7)) + 1)) * p7(u))
 * (the fp32 f'(0) of the quartic and the quintic is a few 1e-6 of max |f'|, not 0: hence the select.)
 * Every (c, k) is summed like a field channel: class (i >> 10) & 7, fp32 sums in ascending index
 * within a class (a +0 term is added like any other), the 8 class sums added pairwise
 * ((s0+s1)+(s2+s3))+((s4+s5)+(s6+s7)).  The result is a function of the point and the scene only:
 * not of the point order, elems_per_point, the entry point, the number of channels in the call or
 * in a walk, the trace's cache knobs.
 *
 * weights = m gives the density gradient; the difference forms (grad A - A grad 1) combine a
 * channel of m / rho * A with a channel of m / rho.  Points and the grid as for
 * the interpolation.  The call needs weights, 1 <= n_channels <= 64 and a non-NULL d_grad.
 * GRACE_INVALID_ARGUMENT, nothing written: as for the interpolation, a custom SPH kernel table
 * included (there is no f'(q)).  Zero points: GRACE_OK.  Stack overflow, stream order, workspace and
 * capture as for the interpolation. */
grace_status grace_interpolate_gradient_points_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                  const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                  size_t n_nodes, const int* d_leaves, const int* d_root,
                                                  const float* d_weights, int n_channels, float* d_grad,
                                                  float* d_value, int* d_counts, grace_stream stream);
grace_status grace_interpolate_gradient_grid_f4(const float* h_origin3, const float* h_uvw9, const int* h_dims3,
                                                const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                size_t n_nodes, const int* d_leaves, const int* d_root,
                                                const float* d_weights, int n_channels, float* d_grad,
                                                float* d_value, int* d_counts, grace_stream stream);
/* Divergence and curl of a vector field from the gradient of its three channels, element-wise:
 * d_grad[(p * 3 + c) * 3 + k] = g_ck = d_k A_c (a 3-channel gradient call's output), n rows;
 *   d_div[p]  = fl(fl(g_xx + g_yy) + g_zz)
 *   d_curl[p * 3 + 0..2] = fl(g_zy - g_yz), fl(g_xz - g_zx), fl(g_yx - g_xy)
 * Either output may be NULL, not both.  Stream-ordered, no allocation. */
grace_status grace_gradient_div_curl_f32(const float* d_grad, size_t n, float* d_div, float* d_curl,
                                         grace_stream stream);
/* Measurement hook (process-wide, results never depend on it): gradient channels per walk, 1 or 2
 * (DESIGN.md gives the default and why); 0 restores the default.  Returns the value in effect. */
int grace_interpolate_gradient_channels_per_walk(int channels);

/* ---- Nearest neighbours and smoothing lengths (an extension the reference lacks) ---------------
 * The k nearest sphere centres of each point, and smoothing lengths from the k-th neighbour of
 * every particle (for particles without H: dark matter, stars).
 *
 * Distance (fp32, every operation rounded, none fused), per point p and sphere j (centre x_j; its w
 * is ignored):  d = p - x per component;  d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz))
 * (the interpolation's sequence).
 * Order: spheres are ranked by the pair (d2, j), smallest d2 first, the lower tree index first on
 * equal d2.  Row p holds the first k of that ranking: d_indices[p * k + s] is the tree index and
 * d_d2[p * k + s] its d2, s = 0 .. k-1.  The result is defined exactly, ties included, and is a
 * function of the point and the scene only: not of the point order, elems_per_point, the spheres'
 * w or the H the tree was built with (any H >= 0), max_per_leaf, the SPH kernel or the trace's
 * cache knobs.
 * Padding: slots s >= n_spheres get index -1 and d2 = +inf.  A point with a non-finite coordinate
 * gets -1 and +inf in every slot.
 * Points: n_points records of elems_per_point (3..16) floats, x y z first, as for
 * grace_interpolate_points_f4; outputs in the caller's order.
 *
 * Smoothing lengths: the query points are the sphere centres themselves, so each particle is its
 * own neighbour at d2 = 0; d_h[i] = fl(eta * sqrt_rn(D_i)), D_i the d2 of slot k-1 of particle i's
 * row, written in tree order to a separate array (d_spheres is only read).  k > n_spheres is
 * refused.  More than k-1 other particles at a particle's position give h = 0.
 *
 * Arguments: 1 <= k <= 64; eta finite and positive; either of d_indices and d_d2 may be NULL, not
 * both.  GRACE_INVALID_ARGUMENT, nothing written: a bad argument or scene, including
 * n_spheres == 0 (there is no tree over zero spheres).  Zero points: GRACE_OK, nothing written
 * (k, elems_per_point and n_points are checked first, the rest after).  The tree's leaves must
 * cover exactly [0, n_spheres), as build_tree and build_ALBVH give; node boxes built with any H >= 0 contain the centres.  A packet that exhausts
 * its 128-entry stack sets the status word of grace_trace_status (GRACE_STACK_OVERFLOW); nothing is
 * written out of bounds.  Stream-ordered, no host synchronisation, no allocation (the context
 * workspace): capturable.  grace_trace_enable_timing / grace_trace_last_kernel_ms time the walk.
 * Periodic boxes: grace_nearest_neighbours_periodic_f4 / grace_smoothing_lengths_periodic_f4 below. */
grace_status grace_nearest_neighbours_f4(const float* d_points, size_t n_points, int elems_per_point,
                                         const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                         size_t n_nodes, const int* d_leaves, const int* d_root,
                                         int k, int* d_indices, float* d_d2, grace_stream stream);
grace_status grace_smoothing_lengths_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                        size_t n_nodes, const int* d_leaves, const int* d_root,
                                        int k, float eta, float* d_h, grace_stream stream);
/* Measurement hook (process-wide, results never depend on it): when enabled, every call of the two
 * above counts its candidate tests (active lanes x survivors of each culling round, summed over
 * packets), its packets, and its insertion steps (survivors for which at least one lane of the
 * packet inserted into its list, summed over packets); grace_neighbours_last_stats synchronises
 * the device and returns the last call's. */
grace_status grace_neighbours_enable_stats(int enabled);
grace_status grace_neighbours_last_stats(unsigned long long* h_candidate_tests, unsigned long long* h_packets,
                                         unsigned long long* h_insertion_steps);

/* ---- Range queries (an extension the reference lacks) ------------------------------------------
 * Every sphere centre within a radius that belongs to the QUERY POINT: counts, CSR neighbour lists
 * (any length) and the gather form of the SPH sum, rho_p = sum_j m_j W(|x_p - x_j|, h_p).
 * (grace_interpolate_points_f4 is the scatter form: the spheres whose own H contains the point.)
 *
 * Distance (fp32, every operation rounded, none fused), per point p and sphere j (centre x_j; its w
 * is ignored):  d = p - x per component;  d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz))
 * (the neighbours' sequence).
 * Radius: r_p = d_radii[p], in the caller's point order, or `radius` for every point if d_radii is
 * NULL;  R2_p = fl(r_p * r_p).  Sphere j is in range of point p iff d2 <= R2_p -- inclusive, so
 * r = 0 finds coincident centres, and a query point that is a sphere centre finds itself.
 * Off points: a point with a non-finite coordinate, or whose r_p is negative, NaN or +inf, is off:
 * count 0, sums 0, an empty row.
 * The result is a function of point, radius and scene only: not of the point order,
 * elems_per_point, the spheres' w or the H the tree was built with (any H >= 0), max_per_leaf, the
 * trace's knobs or caches; counts and lists do not depend on the SPH kernel either.
 * Points: n_points records of elems_per_point (3..16) floats, x y z first, as for
 * grace_interpolate_points_f4; outputs in the caller's order.
 *
 * grace_range_counts_f4:  d_counts[p] = the number of spheres in range (or NULL), and, if d_sums is
 * given (needs d_weights and 1 <= n_channels <= 64; weights in tree order, read on every call),
 *   d_sums[p * n_channels + c] = sum over the spheres j in range, ascending j, of
 *                                fl32(d_weights[j * n_channels + c] * W_pj),
 * a plain fp32 running sum from 0 (no summation classes), with W_pj the arithmetic of "SPH
 * interpolation at points" above with H := r_p:  ih = fl(1 / r_p);  q = fl(sqrt_rn(d2) * ih);
 * K = f(q) in the fp32 forms of the context's SPH kernel;  W = fl(K * fl(fl(ih * ih) * ih));
 * term_c = fl(w_c * W).  The sums are 0 where r_p == 0.  A custom SPH kernel table is refused when
 * sums are requested (there is no f(q)).  Channels are walked four at a time.
 *
 * grace_range_neighbours_f4:  row p occupies [d_offsets[p], d_offsets[p + 1]); d_offsets has
 * n_points + 1 int entries, the exclusive scan of the counts (grace_scan_exclusive_i32 over
 * n_points + 1 entries whose last is 0).  The row holds the spheres in range in ascending tree
 * index in d_indices, their d2 in d_d2; either may be NULL, not both.  The fill never writes
 * outside its row: a row whose length differs from the number of spheres found sets the status word
 * of grace_trace_status, which then returns GRACE_INVALID_ARGUMENT (too short: the row is
 * truncated; too long: its tail is left untouched).
 *
 * GRACE_INVALID_ARGUMENT, nothing written: elems_per_point outside 3..16, a bad channel count,
 * sums without weights, no output at all, a bad scene (including n_spheres == 0), a scalar radius
 * that is negative or non-finite when d_radii is NULL, a custom kernel table with sums.  Zero
 * points: GRACE_OK, nothing written (elems_per_point, the channel arguments and n_points are
 * checked first, the rest after).  The tree's leaves must cover exactly [0, n_spheres), as
 * build_tree and build_ALBVH give; node boxes built with any H >= 0 contain the centres.  A packet
 * that exhausts its 128-entry stack sets the status word of grace_trace_status
 * (GRACE_STACK_OVERFLOW); nothing is written out of bounds.  Stream-ordered, no host
 * synchronisation, no allocation (the context workspace): capturable.  grace_trace_enable_timing /
 * grace_trace_last_kernel_ms time the walks of the last call.
 * Periodic boxes: grace_range_counts_periodic_f4 / grace_range_neighbours_periodic_f4 below.
 * Not provided: symmetric criteria (max(h_p, H_j)), double4 spheres, 64-bit offsets (split the
 * points when the lists exceed INT32_MAX entries). */
grace_status grace_range_counts_f4(const float* d_points, size_t n_points, int elems_per_point,
                                   const float* d_radii, float radius,
                                   const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                   size_t n_nodes, const int* d_leaves, const int* d_root,
                                   const float* d_weights, int n_channels,
                                   int* d_counts, float* d_sums, grace_stream stream);
grace_status grace_range_neighbours_f4(const float* d_points, size_t n_points, int elems_per_point,
                                       const float* d_radii, float radius,
                                       const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                       size_t n_nodes, const int* d_leaves, const int* d_root,
                                       const int* d_offsets, int* d_indices, float* d_d2,
                                       grace_stream stream);

/* ---- Friends-of-friends groups (an extension the reference lacks) ------------------------------
 * Which spheres form a clump: the connected components of the graph that links every two sphere
 * centres within one linking length, as a label per sphere, and a catalogue (group numbers, sizes,
 * member lists) built from the labels.  The pair list is never formed: each link is consumed by a
 * concurrent union-find as the walk of the range queries finds it (4 n bytes in all: the labels).
 *
 * Link: spheres i and j, in tree order (centres x; their w is ignored), are linked iff d2(i, j) <= B2,
 * B2 = fl(b * b), b = linking_length, with the range queries' fp32 distance
 * d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), d = x_i - x_j per component -- inclusive, so b = 0
 * links coincident centres.  d2 is symmetric: fp32 subtraction is exactly antisymmetric and the rest
 * is the same operations on equal squares, so the link graph is undirected.  A sphere with a
 * non-finite coordinate links to nothing and is a group of one.
 * Groups are the connected components of that graph.
 *
 * grace_fof_labels_f4 (the reference has no counterpart):  d_labels[i] = the smallest tree index in
 * i's group (n_spheres ints), so labels[i] <= i and labels[labels[i]] == labels[i].  The labelling
 * is a function of the positions and b alone: not of the H the tree was built with (any H >= 0), of
 * max_per_leaf, of the packets or of which wave won which race of the union-find; every output of
 * these three functions is bit-identical from run to run.
 * GRACE_INVALID_ARGUMENT, nothing written: a negative, NaN or infinite linking_length, more than
 * INT32_MAX spheres, null d_labels or a bad scene (checked in this order, before any launch).
 * n_spheres == 0: GRACE_OK, nothing written (checked after the linking length).  The tree's leaves
 * must cover exactly [0, n_spheres), as build_tree and build_ALBVH give.  A packet that exhausts
 * its 128-entry stack sets the status word of grace_trace_status (GRACE_STACK_OVERFLOW).
 * grace_trace_enable_timing / grace_trace_last_kernel_ms time the link and flatten kernels.
 *
 * grace_fof_groups (the reference has no counterpart):  the catalogue of labels as above (n ints;
 * a label outside [0, n) belongs to no group).  Kept groups are those with at least min_members
 * members (min_members >= 1), numbered 0 .. n_groups - 1 in ascending label.
 *   d_group_of[i] = the number of i's group, or -1 in a group that was not kept (n ints);
 *   d_sizes[g]    = the member count of group g (capacity n; entries from n_groups on are untouched);
 *   d_n_groups    = two device ints: {n_groups, the number of spheres in kept groups}.
 * GRACE_INVALID_ARGUMENT, nothing written: min_members < 1, n > INT32_MAX, a null pointer.
 * n == 0: GRACE_OK, nothing written.
 *
 * grace_fof_members (the reference has no counterpart):  the member lists in CSR form from
 * d_group_of and the first n_groups entries of d_sizes (the host's copy of the count):
 *   d_offsets[0 .. n_groups] = the exclusive scan of the sizes and their total;
 *   d_members: row g is [d_offsets[g], d_offsets[g + 1]), the tree indices of group g's members in
 *   ascending order; it needs d_offsets[n_groups] entries, the second word of d_n_groups (n always
 *   suffices).  The stable grace_sort_pairs_u32 order of the indices keyed on group_of, over the
 *   bits n_groups needs.
 * GRACE_INVALID_ARGUMENT, nothing written: n > INT32_MAX, n_groups > n, a null pointer (d_sizes and
 * d_members may be null when n_groups == 0, which writes d_offsets[0] = 0 only).  n == 0: GRACE_OK,
 * nothing written.
 *
 * All three are stream-ordered, without host synchronisation or allocation (the context
 * workspace): capturable.
 * Periodic boxes: grace_fof_labels_periodic_f4 below; the catalogue is the same.
 * Not provided: per-particle linking lengths, double4 spheres, more than INT32_MAX spheres,
 * unbinding or sub-halo finding, groups ordered by size (one argsort of d_sizes by the caller). */
grace_status grace_fof_labels_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                 size_t n_nodes, const int* d_leaves, const int* d_root,
                                 float linking_length, int* d_labels, grace_stream stream);
grace_status grace_fof_groups(const int* d_labels, size_t n, int min_members, int* d_group_of,
                              int* d_sizes, int* d_n_groups, grace_stream stream);
grace_status grace_fof_members(const int* d_group_of, size_t n, const int* d_sizes, size_t n_groups,
                               int* d_offsets, int* d_members, grace_stream stream);

/* ---- Pair counts in separation bins and radial profiles (an extension the reference lacks) -----
 * How many sphere centres lie in each shell of separation around each query point: the totals over
 * all points (the pair counts DD(r) behind a two-point correlation function), the per-point
 * histograms, and the per-point sums of weights per shell (counts and mass in shells around chosen
 * centres, such as those of the groups grace_fof_groups has found).  One walk of the range queries
 * at the outermost edge; each pair is binned where the walk finds it, no list is formed.
 *
 * Distance: the range queries' fp32 sequence d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)),
 * d = p - x per component, every operation rounded, none fused; the spheres' w is ignored.
 * Points: n_points records of elems_per_point (3..16) floats, x y z first, as for
 * grace_range_counts_f4; outputs in the caller's point order.
 * Edges: h_edges is a HOST array of n_edges floats, 1 <= n_edges <= 64, every edge finite and >= 0,
 * strictly ascending.  It is read at call time and travels in the kernel arguments: no device copy,
 * no host synchronisation.  E2_k = fl(e_k * e_k).
 * Bin: the bin of a pair is the smallest k with d2 <= E2_k; a pair with d2 > E2_{n_edges-1}, or a
 * NaN d2, is in no bin.  So bin 0 holds d2 <= E2_0 -- with e_0 = 0 exactly the coincident and self
 * pairs -- and bin k >= 1 holds E2_{k-1} < d2 <= E2_k.  The sum over bins 0..k is the count of
 * grace_range_counts_f4 at radius e_k, by construction.  Where E2_{k-1} == E2_k (small edges whose
 * squares underflow) bin k is empty.
 * Off points: a point with a non-finite coordinate is in no pair; its rows are 0.
 *
 * Outputs, each may be NULL, not all of them:
 *   d_totals[k]  (n_edges 64-bit unsigned): the number of (point, sphere) pairs in bin k over all
 *     points.  Overwritten by the call; accumulated with 64-bit integer atomics only, so exact and
 *     independent of order.  Pairs are ORDERED pairs: when the points are the sphere centres
 *     themselves every unordered pair is counted twice and every self pair once (d2 = 0: bin 0), so
 *     DD_k = (d_totals[k] - (k == 0 ? n : 0)) / 2.
 *   d_counts[p * n_edges + k]  (int): point p's histogram.
 *   d_sums[(p * n_edges + k) * n_channels + c]  (float): the sum of d_weights[j * n_channels + c] over
 *     the spheres j of point p in bin k, in ascending tree index j, a plain fp32 running sum from 0
 *     (no SPH kernel in it): the mass in each shell; the cumulative profile is the caller's prefix
 *     sum.  Needs d_weights (tree order, read on every call), 1 <= n_channels <= 4 and
 *     n_edges * n_channels <= 64.
 * The result is a function of the points, the edges, the centres and the weights only: not of the
 * point order, elems_per_point, the H the tree was built with (any H >= 0), max_per_leaf, the SPH
 * kernel or the trace's knobs; every output is bit-identical from run to run.
 *
 * GRACE_INVALID_ARGUMENT, nothing written: elems_per_point outside 3..16, n_edges outside 1..64, a
 * null h_edges, an edge that is negative, non-finite or not above the one before it, sums with a
 * channel count outside 1..4, with n_edges * n_channels > 64 or without weights, no output at all,
 * a bad scene (including n_spheres == 0).  Zero points: GRACE_OK, and d_totals, if given, is zeroed
 * (elems_per_point, n_points, the edges and the channel arguments are checked first, the rest
 * after).  The tree's leaves must cover exactly [0, n_spheres), as build_tree and build_ALBVH give.
 * A packet that exhausts its 128-entry stack sets the status word of grace_trace_status
 * (GRACE_STACK_OVERFLOW); nothing is written out of bounds.  Stream-ordered, no host
 * synchronisation, no allocation (the context workspace): capturable.  grace_trace_enable_timing /
 * grace_trace_last_kernel_ms time the walk of the last call.
 * Periodic boxes: grace_pair_counts_periodic_f4 below.
 * Not provided: double4 spheres, weighted totals (sum d_sums in fp64), halving the work for
 * auto-pairs (points that are the centres are walked from both ends), estimators (Landy-Szalay,
 * xi(r)), per-point edge lists. */
grace_status grace_pair_counts_f4(const float* d_points, size_t n_points, int elems_per_point,
                                  const float* h_edges, int n_edges,
                                  const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                  size_t n_nodes, const int* d_leaves, const int* d_root,
                                  const float* d_weights, int n_channels,
                                  unsigned long long* d_totals, int* d_counts, float* d_sums,
                                  grace_stream stream);

/* ---- Tree gravity: potentials and accelerations at points (an extension the reference lacks) ----
 * The Barnes-Hut walk over the BVH with monopoles of the inner nodes, G = 1: whether a
 * friends-of-friends group is bound, which member is the most bound, the acceleration on a tracer.
 * Two calls: the node moments once per tree and set of masses, then any number of walks.  The
 * contract is exact, no tolerance; two results depend on the tree (its max_per_leaf and H) by design:
 * the node records, and the walk's outputs when theta > 0.
 *
 * grace_gravity_moments_f4.  d_masses: float[n_spheres] in tree order (as weights elsewhere); the
 * spheres' w is ignored.  d_moments: 12 floats per inner node, n_nodes records.
 *   Per leaf, over its primitives j in ascending index, sequentially in fp64: M = sum double(m_j);
 *   S_k = sum double(m_j) * double(x_jk) (each product is exact, the running sum is not: hence the
 *   order); the box lo_k = min x_jk, hi_k = max x_jk over the centres, fp32 -- tight, H plays no
 *   part; the span [first, first + count).  Leaf values are intermediate (context workspace) and are
 *   never written to d_moments.
 *   Per inner node: M = M_left + M_right, S_k = S_left,k + S_right,k (one fp64 add each, the left
 *   operand first); the box and the span are the unions of the children's.
 *   Record i = {c_x, c_y, c_z, M32}, {lo_x, lo_y, lo_z, bits(span_lo)}, {hi_x, hi_y, hi_z,
 *   bits(span_hi)}: c_k = float(S_k / M) (an fp64 divide, rounded once to fp32), M32 = float(M); where
 *   M == 0, c = lo.  The spans are ints stored by their bit patterns.
 *   Negative or non-finite masses are the caller's responsibility.  n_nodes == 0 (the root is a
 *   leaf): GRACE_OK, nothing written, d_moments may be NULL.  GRACE_INVALID_ARGUMENT, nothing written:
 *   a bad scene (including n_spheres == 0), null d_masses, null d_moments with n_nodes > 0.  The tree
 *   must be one (every node but the root the child of exactly one node; leaves inside [0, n_spheres));
 *   on arrays that are no tree some records stay unwritten, nothing is indexed out of bounds and
 *   nothing waits.  Stream-ordered, no host synchronisation, no allocation (the context workspace):
 *   capturable.  Bit-identical from run to run.
 *
 * grace_gravity_points_f4.  Points: n_points records of elems_per_point (3..16) floats, x y z first,
 * as for every point query; outputs in the caller's point order.  theta (opening angle) and eps
 * (Plummer softening length, one for all particles; 0: Newtonian) are host floats.
 *   d_out[p * 4 + ..] (double) = {a_x, a_y, a_z, phi};  d_counts[p * 2 + ..] (int) = {node terms,
 *   particle terms}.  Either may be NULL, not both.
 * Per point p the recursion visit(root), theta2 = fl(theta * theta), eps2 = fl(eps * eps):
 *   visit(inner node), from its record: e_k = max(max(fl(lo_k - p_k), fl(p_k - hi_k)), 0);
 *     d2min = fl(fl(fl(e_x e_x) + fl(e_y e_y)) + fl(e_z e_z)); size = max_k fl(hi_k - lo_k);
 *     size2 = fl(size * size).  The node is accepted iff size2 < fl(theta2 * d2min): then one term for
 *     {c, M32} and one node term counted; otherwise visit(left child), then visit(right child).  A
 *     point inside or on the box has d2min == 0 and never accepts it; with theta == 0 nothing is
 *     accepted.
 *   visit(leaf): one term per primitive {x_j, m_j} of the leaf, ascending j, a particle term counted
 *     for each.  A leaf is never taken as a monopole.
 *   Term for {x, m}, fp32, every operation rounded, none fused: d = fl(x - p) per component;
 *     d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)).  A term with d2 == 0 contributes nothing, for
 *     any eps (it is still counted): the self pair and coincident centres.  Otherwise
 *     s = fl(d2 + eps2); ir = fl(1 / sqrt_rn(s)) (a correctly rounded square root, then a correctly
 *     rounded divide); u = fl(m * ir); f = fl(m * fl(fl(ir * ir) * ir));
 *     A_k += double(fl(f * d_k)); P += double(u): fp64 running sums from 0 in the order of the
 *     recursion, which is ascending span start.
 *   Output: a = A, phi = -P (so -0 for a point none of whose terms contributed).
 * So with theta == 0 the result is the direct sum over all spheres in ascending tree index: a
 * function of the point, the centres, the masses and eps only, not of the tree's shape, H or
 * max_per_leaf.  For any theta the result does not depend on the point order, elems_per_point, the
 * packets, the SPH kernel or the trace's knobs, and is bit-identical from run to run.
 * Off points: a point with a non-finite coordinate gets zeros (+0, all four) and zero counts.
 * GRACE_INVALID_ARGUMENT, nothing written: theta or eps negative or non-finite, elems_per_point
 * outside 3..16, no output, null d_masses, null d_moments with n_nodes > 0, a bad scene.  Zero points:
 * GRACE_OK (elems_per_point, n_points, theta and eps are checked first, the rest after).  The tree's
 * leaves must cover exactly [0, n_spheres), and d_moments must be grace_gravity_moments_f4's records
 * for this tree.  A packet that exhausts its 128-entry stack sets the status word of
 * grace_trace_status (GRACE_STACK_OVERFLOW); nothing is written out of bounds.  Leaves are pushed as
 * merged ranges as in the range queries, so a spine of coincident centres does not grow the stack.
 * Stream-ordered, no host synchronisation, no allocation (the context workspace): capturable.
 * grace_trace_enable_timing / grace_trace_last_kernel_ms time the walk of the last call.
 * Not provided: periodic boxes (they need Ewald sums), quadrupoles, spline softening or per-particle
 * softening, leaf monopoles, double4 spheres, G (multiply the outputs). */
grace_status grace_gravity_moments_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                      size_t n_nodes, const int* d_leaves, const int* d_root,
                                      const float* d_masses, float* d_moments, grace_stream stream);
grace_status grace_gravity_points_f4(const float* d_points, size_t n_points, int elems_per_point,
                                     const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                     size_t n_nodes, const int* d_leaves, const int* d_root,
                                     const float* d_masses, const float* d_moments, float theta, float eps,
                                     double* d_out, int* d_counts, grace_stream stream);

/* ---- Gravity within groups: every point feels the particles of its own label (an extension the
 * reference lacks)
 * The potential of every member of every friends-of-friends group due to its own group alone, in
 * one walk of the whole-scene tree: which haloes of a catalogue are bound, without a tree, a gather
 * and a launch per group.  The two calls are grace_gravity_moments_f4 and grace_gravity_points_f4 in
 * everything this block does not restate: arguments, layouts, rounding, the order of the sums,
 * status word, stream ordering, timing, capturability.  The contract is exact, no tolerance.
 *
 * Labels.  d_labels: int[n_spheres] in tree order.  A label >= 0 names a group; a label < 0 means
 * "in no group": such a particle attracts nobody -- it is as if it were absent, except that it keeps
 * its index.  d_point_labels: int[n_points] in the caller's point order.  Label values matter only
 * through equality and order.
 *
 * grace_gravity_group_moments_f4.  d_moments: 12 floats per inner node in the layout of
 * grace_gravity_moments_f4; d_label_ranges: 2 ints per inner node.
 *   M, S, lo and hi are taken over the labelled primitives (label >= 0) below the node only: the
 *   fp64 sums per leaf in ascending tree index, skipping unlabelled primitives, and per node as
 *   left + right; lo / hi the tight box of the labelled centres, +inf / -inf where there are none.
 *   span_lo / span_hi are unchanged: they cover every primitive, because the walk skips by spans.
 *   c = float(S / M), or lo where M == 0 (so +inf under a node without a labelled primitive, which the
 *   walk never reads).  d_label_ranges[i * 2 + ..] = {lab_lo, lab_hi}: the smallest and largest label
 *   >= 0 below node i, {INT32_MAX, -1} where there is none.
 *   When no label is negative, the 12-float records equal grace_gravity_moments_f4's bit for bit.
 *   n_nodes == 0: GRACE_OK, nothing written.  GRACE_INVALID_ARGUMENT, nothing written: as
 *   grace_gravity_moments_f4, and null d_labels, null d_label_ranges with n_nodes > 0.
 *
 * grace_gravity_group_points_f4.  For a point p with finite coordinates and label L >= 0 the
 * recursion visit(root):
 *   visit(inner node i):
 *     lab_lo[i] > L or lab_hi[i] < L: nothing, no term and no count;
 *     lab_lo[i] == lab_hi[i] and size2 < fl(theta2 * d2min) (the fp32 test of
 *       grace_gravity_points_f4 on the record's box): one term {c, M32}, one node term counted;
 *     otherwise visit(left child), then visit(right child).
 *     A node that holds two or more labels is never a monopole.
 *   visit(leaf): one term per primitive j with labels[j] == L, in ascending index, a particle term
 *     counted for each.
 *   Terms, rounding, the d2 == 0 rule, the fp64 running sums in the order of the recursion,
 *   out = {a, phi = -P} and counts = {node terms, particle terms} are exactly those of
 *   grace_gravity_points_f4.
 * A point with a negative label or a non-finite coordinate gets +0 throughout and zero counts.  A
 * point whose label no particle carries gets no term (phi = -0).
 * So: theta == 0 is the direct sum over the label's members in ascending tree index, independent of
 * the tree.  With all labels and point labels equal to one value >= 0, out and counts equal
 * grace_gravity_points_f4's bit for bit.  For theta > 0 the result depends on the tree and on which
 * particles carry which labels, and on nothing else: not on the point order, the packets,
 * elems_per_point, the knobs or the stream; it is bit-identical from run to run.
 * GRACE_INVALID_ARGUMENT, nothing written: as grace_gravity_points_f4, and null d_labels, null
 * d_point_labels, null d_label_ranges with n_nodes > 0.  d_moments and d_label_ranges must be
 * grace_gravity_group_moments_f4's for this tree, these masses and these labels.  The walk pushes
 * both children of every node it opens, as the open walk does, so the stack bound is the same; an
 * overflow is reported through the status word.
 * An unbinding pass is: set the labels of the unbound members to -1, the moments again, the walk again.
 * Not provided: a theta or eps per group, particles in more than one group, the unbinding loop itself
 * (INTEGRATION.md shows it), periodic boxes, and everything grace_gravity_points_f4 leaves out. */
grace_status grace_gravity_group_moments_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                            size_t n_nodes, const int* d_leaves, const int* d_root,
                                            const float* d_masses, const int* d_labels, float* d_moments,
                                            int* d_label_ranges, grace_stream stream);
grace_status grace_gravity_group_points_f4(const float* d_points, size_t n_points, int elems_per_point,
                                           const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                           size_t n_nodes, const int* d_leaves, const int* d_root,
                                           const float* d_masses, const int* d_labels, const float* d_moments,
                                           const int* d_label_ranges, const int* d_point_labels, float theta,
                                           float eps, double* d_out, int* d_counts, grace_stream stream);

/* ---- Periodic boxes for the point queries: range queries, friends-of-friends, pair counts, nearest
 * neighbours, smoothing lengths and interpolation (an extension the reference lacks)
 * The five families above on a torus: a cosmological snapshot is a periodic box, and a halo that
 * straddles a face, the pairs across it and the neighbours beyond it belong to the answer.  Each
 * function below takes the arguments of its open counterpart plus h_period3 before the stream, and
 * is that counterpart in everything this block does not restate: arguments, outputs, order, off
 * points, status word, stream ordering, timing.
 *
 * Period: h_period3 is a HOST array of three floats L = (Lx, Ly, Lz), read at call time (it travels in
 * the kernel arguments: no device copy, no host synchronisation).  L_a == 0: the axis is open, no
 * wrapping on it.  Any L_a that is negative, NaN or infinite: GRACE_INVALID_ARGUMENT before
 * anything is enqueued.  No box origin is needed: the arithmetic below is defined for any
 * coordinates.
 *
 * Separation (fp32, every operation rounded, none fused, each component on its own):
 * d = fl(p - x);  h = fl(0.5 * L_a) (exact).  If d > h: d = fl(d - L_a); otherwise, if d < -h:
 * d = fl(d + L_a).  At most one wrap; an open axis gets none.  Then
 * d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), as above.  Everything downstream uses this d2
 * unchanged: membership d2 <= fl(r r), the d2 returned in lists, the bin of a pair (the smallest k
 * with d2 <= fl(e_k e_k)), W(sqrt(d2), r_p) in the gather sums, the link d2 <= fl(b b).  The
 * separation is antisymmetric bit for bit -- fl(p - x) = -fl(x - p), the two wraps mirror each other
 * and fl(d - L) = -fl(-d + L) -- so d2 is symmetric and a link is still seen once, from its upper
 * index.
 * Each centre is tested once per point, not once per image: a pair appears at most once in a list,
 * a count or a bin, pairs at exactly half a period included (d == h and d == -h are not wrapped).
 *
 * Radius: a query point is additionally OFF if r_p > fl(0.5 * L_a) on any periodic axis: an empty
 * row, count 0, sums 0, no bins -- the treatment r = +inf gets above.  Where the radius is a host
 * scalar (`radius` with d_radii NULL, the linking length, the last edge), a value above
 * fl(0.5 * L_a) on a periodic axis is GRACE_INVALID_ARGUMENT, nothing written.
 *
 * Nearest neighbours and smoothing lengths (grace_nearest_neighbours_periodic_f4 /
 * grace_smoothing_lengths_periodic_f4, extending grace_nearest_neighbours_f4 /
 * grace_smoothing_lengths_f4): there is no radius, so no limit.  Every centre is ranked once, by
 * the pair (wrapped d2, tree index); a k-th distance above half a period is legal and is the
 * one-wrap d2 above (beyond half a period it is no longer the distance to the nearest image).
 * d_h[i] = fl(eta * sqrt_rn(D_i)) with D_i the wrapped d2 of slot k-1; k, eta, off points, padding
 * with -1 / +inf and the outputs are the open call's.
 *
 * Interpolation (grace_interpolate_points_periodic_f4 / grace_interpolate_grid_periodic_f4,
 * extending grace_interpolate_points_f4 / grace_interpolate_grid_f4): the radius belongs to the
 * sphere, so the rule above applies to it: a sphere whose H exceeds fl(0.5 * L_a) on a periodic axis
 * is OFF -- it contributes to no point and to no count (more than one of its images could contain a
 * point); H == fl(0.5 * L_a) is on.  Every other sphere is tested once per point, never per image:
 * containment is wrapped d2 < fl(H * H), W = fl(K(fl(sqrt_rn(d2) * ih)) * fl(fl(ih * ih) * ih)) with
 * that d2, and the class order of the sums, the lattice's positions and the outputs are the open
 * call's.
 *
 * Identities, bit for bit: L = (0, 0, 0) gives the open function's output; so does any finite L larger
 * than twice the extent of points and centres together on every axis (no |d| exceeds h; for the
 * interpolation, where no H exceeds half of it either).  Lists and running sums are in ascending
 * tree index, as above.  The result is a function of the points, the radii (edges, linking length,
 * k and eta; for the interpolation the spheres' own H), the centres, the weights and L only: not of
 * the H the tree was built with (any H >= 0; the interpolation's tree is built with the spheres'
 * H), of max_per_leaf, of the packets, of the order of the points or of the stream.
 *
 * GRACE_INVALID_ARGUMENT, nothing written: a NULL h_period3, a bad period, a host radius above half
 * a period, and whatever the open counterpart refuses.  (The period is checked first by the range
 * queries, friends-of-friends, the neighbours and the interpolation, after the edges by the pair
 * counts.)  Zero points or spheres: as the open counterpart, after the period's check.
 * Periodic ray traces: the next block.  Not provided: a box origin (none is needed); radii above half a period
 * (more than one image of a centre in range, or of a sphere around a point). */
grace_status grace_range_counts_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                            const float* d_radii, float radius,
                                            const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                            size_t n_nodes, const int* d_leaves, const int* d_root,
                                            const float* d_weights, int n_channels,
                                            int* d_counts, float* d_sums, const float* h_period3,
                                            grace_stream stream);
grace_status grace_range_neighbours_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                const float* d_radii, float radius,
                                                const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                size_t n_nodes, const int* d_leaves, const int* d_root,
                                                const int* d_offsets, int* d_indices, float* d_d2,
                                                const float* h_period3, grace_stream stream);
grace_status grace_fof_labels_periodic_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                          size_t n_nodes, const int* d_leaves, const int* d_root,
                                          float linking_length, int* d_labels, const float* h_period3,
                                          grace_stream stream);
grace_status grace_pair_counts_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                           const float* h_edges, int n_edges,
                                           const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                           size_t n_nodes, const int* d_leaves, const int* d_root,
                                           const float* d_weights, int n_channels,
                                           unsigned long long* d_totals, int* d_counts, float* d_sums,
                                           const float* h_period3, grace_stream stream);
/* grace_nearest_neighbours_f4 / grace_smoothing_lengths_f4 in a periodic box ("Nearest neighbours and
 * smoothing lengths" above). */
grace_status grace_nearest_neighbours_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                  const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                  size_t n_nodes, const int* d_leaves, const int* d_root,
                                                  int k, int* d_indices, float* d_d2, const float* h_period3,
                                                  grace_stream stream);
grace_status grace_smoothing_lengths_periodic_f4(const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                 size_t n_nodes, const int* d_leaves, const int* d_root,
                                                 int k, float eta, float* d_h, const float* h_period3,
                                                 grace_stream stream);
/* grace_interpolate_points_f4 / grace_interpolate_grid_f4 in a periodic box ("Interpolation" above). */
grace_status grace_interpolate_points_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                  const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                  size_t n_nodes, const int* d_leaves, const int* d_root,
                                                  const float* d_weights, int n_channels,
                                                  float* d_out, int* d_counts, const float* h_period3,
                                                  grace_stream stream);
grace_status grace_interpolate_grid_periodic_f4(const float* h_origin3, const float* h_uvw9, const int* h_dims3,
                                                const float* d_spheres, size_t n_spheres, const int* d_nodes,
                                                size_t n_nodes, const int* d_leaves, const int* d_root,
                                                const float* d_weights, int n_channels,
                                                float* d_out, int* d_counts, const float* h_period3,
                                                grace_stream stream);
/* grace_interpolate_gradient_points_f4 / grace_interpolate_gradient_grid_f4 in a periodic box: the
 * interpolation's wrapped d ("Interpolation" above) is the d of d2 and of the unit vector; a sphere
 * whose H exceeds half a period contributes nothing. */
grace_status grace_interpolate_gradient_points_periodic_f4(const float* d_points, size_t n_points, int elems_per_point,
                                                           const float* d_spheres, size_t n_spheres,
                                                           const int* d_nodes, size_t n_nodes, const int* d_leaves,
                                                           const int* d_root, const float* d_weights, int n_channels,
                                                           float* d_grad, float* d_value, int* d_counts,
                                                           const float* h_period3, grace_stream stream);
grace_status grace_interpolate_gradient_grid_periodic_f4(const float* h_origin3, const float* h_uvw9,
                                                         const int* h_dims3, const float* d_spheres, size_t n_spheres,
                                                         const int* d_nodes, size_t n_nodes, const int* d_leaves,
                                                         const int* d_root, const float* d_weights, int n_channels,
                                                         float* d_grad, float* d_value, int* d_counts,
                                                         const float* h_period3, grace_stream stream);

/* ---- Periodic boxes for traces: sphere images, ray segments, folded results (an extension the
 * reference lacks)
 * The periodic trace is DEFINED as the open trace (grace_trace_hitcounts_f4, grace_trace_cumulative_f4,
 * grace_trace_cumulative_weighted_f4: trace_sph.cuh:58-110, unchanged) of a stated set of ray SEGMENTS
 * over a stated set of sphere IMAGES, folded back per ray.  The functions below make the two sets and
 * fold; the front ends (grace::periodic_scene_sph, Python periodic_scene) call the open traces in
 * between.  The definition is exact because sphere_hit (generic/intersect.h) owns a hit by the point
 * of closest approach -- a pair hits iff b2 < w^2 and 0 <= dot < length -- so segments that tile
 * [0, length) count every lattice image of a sphere exactly once, also one that straddles a cut.
 *
 * Box: h_lo3 and h_period3 are HOST arrays of three floats, the box origin lo and the periods L, read
 * at call time.  L_k == 0 leaves axis k open.  A negative or non-finite period, a non-finite origin or
 * a NULL array: GRACE_INVALID_ARGUMENT, nothing enqueued.  Unlike the point queries, traces need lo.
 *
 * Images (fp32, every operation rounded, none fused).  Sphere i = {x, H} gets, per periodic axis k,
 * bit k of its crossing code if fl(x_k - H) < lo_k -- its image is at fl(x_k + L_k) -- or otherwise if
 * fl(x_k + H) > fl(lo_k + L_k) -- its image is at fl(x_k - L_k).  It is emitted 2^popcount(code) times:
 * every subset of the crossing axes shifted, in ascending subset code, subset 0 being the sphere
 * itself bit for bit; w is copied; output order is ascending (i, subset); d_source[j] = i.
 * A centre outside [lo_k, fl(lo_k + L_k)] or H > fl(0.5 L_k) on a periodic axis sets the status word
 * (GRACE_INVALID_ARGUMENT from grace_trace_status) and the sphere is emitted once, unshifted; so is,
 * without the status word, a sphere with a non-finite member.  All axes open: images == spheres,
 * source == identity.
 * grace_periodic_image_counts_f4 writes d_counts[i], i < n; the caller scans them (n + 1 entries,
 * the last one 0: grace_scan_exclusive_i32) and passes the offsets and arrays of offsets[n] float4 /
 * int to grace_periodic_images_f4.  A row whose length is not the sphere's count sets the status
 * word; nothing is written outside a row.  d_source is an int per image: the payload of
 * grace_sort_pairs_u32 beside the images' keys, so that it follows the images into tree order.
 *
 * Segments (fp64 from the widened fp32 members, every operation rounded, none fused).  Ray {d, o, l}.
 * Per periodic axis u = (o_k - lo_k) / L_k; the starting cell is c_k = floor(u) if d_k >= 0,
 * ceil(u) - 1 if d_k < 0; open axes c_k = 0.  Cuts of axis k: for d_k > 0 the planes m = c_k + 1,
 * c_k + 2, ...; for d_k < 0 the planes m = c_k, c_k - 1, ...; none for d_k == +-0;
 * t = ((lo_k + m L_k) - o_k) / d_k, evaluated for each m, never accumulated; a cut is kept while t > 0
 * and t < l (the first plane that fails ends the axis).  All cuts of the three axes are ordered by
 * (t, axis); equal t on two axes gives two cuts and a zero-length segment, which can hit nothing.  The
 * segments are [0, t_1), [t_1, t_2), ..., [t_n, l); segment j is the Ray with the ray's direction bit
 * for bit, origin fl32((o_k + t_j d_k) - cell_k L_k) -- cell the running cell: c, plus sign(d_k) per
 * cut on k passed -- and length fl32(t_{j+1} - t_j) (t_0 = 0, t_{n+1} = l).  A ray without cuts in
 * cell 0 is its own single segment bit for bit.  A ray with a non-finite member, or with more than
 * 65536 segments, is emitted as itself, once; the second case also sets the status word.
 * grace_periodic_segment_counts / grace_periodic_segments: counts, the caller's scan, fill, as for the
 * images; d_segments holds offsets[n_rays] Rays.  The count is O(1) per axis (a closed form corrected
 * against the predicate above: exact while |o - lo| / L stays below 2^40), the fill a three-axis walk
 * that stops at the row's end; no loop runs more than 65536 times whatever the inputs hold.
 *
 * Results.  With s over a ray's segments (ascending) and the open traces run on (segments, images):
 * hit_counts_periodic[r] = sum of the segments' hit counts (grace_periodic_fold_i32);
 * cumulated_periodic[r, c] = the fp32 running sum, from 0, of the segments' (weighted) column
 * densities (grace_periodic_fold_f32: d_values [n_segments * n_channels], d_out [n_rays * n_channels],
 * rows of d_offsets longer than 65536 are cut there).  An image carries the weight row of its source:
 * grace_periodic_gather_rows_f32 writes d_out[j * n_channels + c] = d_rows[d_source[j] * n_channels + c]
 * (1 <= n_channels <= 64).  Open boxes, or a box much larger than the scene and the rays (no sphere
 * crosses a face, every ray stays in cell 0), give the open outputs bit for bit.
 *
 * Ordered traces (grace_trace_emission_absorption_periodic_f4, grace_trace_absorption_deposit_periodic_f4,
 * grace_trace_spectra_periodic_f4, extending grace_trace_emission_absorption_f4,
 * grace_trace_absorption_deposit_f4 and grace_trace_spectra_f4 above).  A fold of per-segment results
 * does not define them -- a deposit's segment needs the luminosity its predecessor left, a spectrum's
 * hit its distance from the ray's origin -- so they are the open call's composite applied PER RAY to
 * this hit list:
 * 1. Segments: those of grace_periodic_segments, unchanged.  Segment s has the starting parameter
 *    t0_s (fp64): the t above at which it starts, 0 for a ray emitted as itself;
 *    grace_periodic_segment_starts writes d_t0[offsets[n_rays]] with the arithmetic of
 *    grace_periodic_segments (one walk serves both).
 * 2. Hits: those of the open per-hit trace (grace_trace_hits_f4) of segment s over the images: image
 *    index j, integral I, local distance d with 0 <= d < length_s.
 * 3. Order: by (segment ordinal along the ray, fp32 d, image index j).  Within a segment a ray hits an
 *    image once, so the keys are distinct.  A ray may hit the same SOURCE several times, once per
 *    lattice image.  The segment comes first because two lattice images of one particle can have
 *    closest approaches arbitrarily close in t when H is near L / 2: absolute distance and particle
 *    index are no total order.
 * 4. Composite: hit k's particle is i = d_source[j], the caller's index.  Every per-particle input
 *    (emission, absorption, amount, width, velocity) and output (deposit) is indexed by i, in the
 *    caller's order, n_sources rows; nothing is gathered per image.  The arithmetic is the open
 *    call's, every addition placed as a function of k and n with n the ray's total over all segments.
 *    Spectra: d_k = t0_s + (double)d in fp64, v_k = hubble d_k + ...  Deposit: the quantum's n_rays
 *    is the number of rays, not of segments.
 * Arguments: d_segments [n_segments] and d_segment_offsets [n_rays + 1] as grace_periodic_segments made
 * them; d_images, the tree over them and d_source [n_images] (in tree order) as the front ends'
 * periodic scene holds them; d_segment_t0 [n_segments] (spectra); then the open call's own arguments,
 * per-ray arrays holding n_rays rows.  Any number of rays.  With every axis open, or a box so large that
 * no ray is cut and no sphere imaged, the hit list is the open one, d_source the identity and all
 * outputs equal the open calls' bit for bit.  Batches are cut at ray boundaries; one ray's hits over all
 * its segments must fit a batch's 32-bit offsets: if not, GRACE_INVALID_ARGUMENT before any batch is
 * traced (found on the device, reported with the batch table).  d_segment_offsets is checked on the
 * device first -- it must start at 0, not decrease, end at n_segments and give a ray at most 65536
 * segments: otherwise GRACE_INVALID_ARGUMENT and the status word, nothing traced.  An image whose
 * d_source is outside [0, n_sources) contributes nothing and sets the status word.  n_rays == 0 returns
 * at once (the deposit: zeroed, as the open call's).
 * Not provided: per-hit outputs, double4 spheres, H > L / 2. */
grace_status grace_periodic_image_counts_f4(const float* d_spheres, size_t n, const float* h_lo3,
                                            const float* h_period3, int* d_counts, grace_stream stream);
grace_status grace_periodic_images_f4(const float* d_spheres, size_t n, const float* h_lo3,
                                      const float* h_period3, const int* d_offsets, float* d_images,
                                      int* d_source, grace_stream stream);
grace_status grace_periodic_segment_counts(const void* d_rays, size_t n_rays, const float* h_lo3,
                                           const float* h_period3, int* d_counts, grace_stream stream);
grace_status grace_periodic_segments(const void* d_rays, size_t n_rays, const float* h_lo3,
                                     const float* h_period3, const int* d_offsets, void* d_segments,
                                     grace_stream stream);
grace_status grace_periodic_segment_starts(const void* d_rays, size_t n_rays, const float* h_lo3,
                                           const float* h_period3, const int* d_offsets, double* d_t0,
                                           grace_stream stream);
grace_status grace_periodic_fold_f32(const float* d_values, const int* d_offsets, size_t n_rays, int n_channels,
                                     float* d_out, grace_stream stream);
grace_status grace_periodic_fold_i32(const int* d_values, const int* d_offsets, size_t n_rays, int n_channels,
                                     int* d_out, grace_stream stream);
grace_status grace_periodic_gather_rows_f32(const float* d_rows, const int* d_source, size_t n_images,
                                            int n_channels, float* d_out, grace_stream stream);
/* grace_trace_emission_absorption_f4 in a periodic box ("Ordered traces" above). */
grace_status grace_trace_emission_absorption_periodic_f4(const void* d_segments, size_t n_segments,
                                                         const float* d_images, size_t n_images, const int* d_nodes,
                                                         size_t n_nodes, const int* d_leaves, const int* d_root,
                                                         const int* d_segment_offsets, size_t n_rays,
                                                         const int* d_source, size_t n_sources,
                                                         const float* d_emission, int n_channels,
                                                         const float* d_absorption, float* d_out, float* d_tau,
                                                         grace_stream stream);
/* grace_trace_absorption_deposit_f4 in a periodic box: d_absorption and d_deposit hold n_sources rows. */
grace_status grace_trace_absorption_deposit_periodic_f4(const void* d_segments, size_t n_segments,
                                                        const float* d_images, size_t n_images, const int* d_nodes,
                                                        size_t n_nodes, const int* d_leaves, const int* d_root,
                                                        const int* d_segment_offsets, size_t n_rays,
                                                        const int* d_source, size_t n_sources,
                                                        const float* d_luminosity, const float* d_absorption,
                                                        int n_channels, double* d_deposit, float* d_transmitted,
                                                        double* d_quantum, grace_stream stream);
/* grace_trace_spectra_f4 in a periodic box: d_segment_t0 from grace_periodic_segment_starts. */
grace_status grace_trace_spectra_periodic_f4(const void* d_segments, size_t n_segments, const float* d_images,
                                             size_t n_images, const int* d_nodes, size_t n_nodes,
                                             const int* d_leaves, const int* d_root, const int* d_segment_offsets,
                                             size_t n_rays, const int* d_source, size_t n_sources,
                                             const double* d_segment_t0, const float* d_amount, const float* d_width,
                                             const float* d_velocity, int n_channels,
                                             const grace_spectrum_grid* grid, float* d_tau, float* d_column,
                                             grace_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* GRACE_HIP_H */
