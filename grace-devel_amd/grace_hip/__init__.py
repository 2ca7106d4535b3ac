"""Python host-side mirror of the grace:: SPH API over libgrace_hip.so (C ABI, ctypes).

Names, argument meaning and error behaviour follow the reference's user-facing functions
(include/grace/cuda/build_sph.cuh, trace_sph.cuh, scan.cuh, tests/helper/tree.cuh,
tests/helper/rays.cuh); torch tensors play the role of thrust::device_vector (device
memory + streams only -- every computation is a hand-written HIP kernel behind the C ABI).
There is NO CPU fallback: importing this module without the built library raises.
"""
import collections
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libgrace_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libgrace_hip.so is not built (%s). Run __graft_entry__.build() or "
        "`make -C grace-devel_amd`. There is no CPU fallback." % LIB_PATH)

_lib = C.CDLL(LIB_PATH)
_lib.grace_last_error.restype = C.c_char_p
_lib.grace_version.restype = C.c_int

GRACE_OK = 0
GRACE_INVALID_ARGUMENT = 1
GRACE_HIP_ERROR = 2
GRACE_OUT_OF_MEMORY = 3
GRACE_STACK_OVERFLOW = 4

RAY_FLOATS = 7  # include/grace/ray.h:5-10
N_TABLE = 51    # include/grace/cuda/trace_sph.cuh:22


class GraceError(RuntimeError):
    """A GPU API failure; the reference prints the error and exit()s (error.h:40-56)."""


def _check(status):
    if status == GRACE_OK:
        return
    msg = _lib.grace_last_error().decode()
    if status == GRACE_INVALID_ARGUMENT:
        raise ValueError(msg)  # std::invalid_argument in the reference
    if status == GRACE_OUT_OF_MEMORY:
        raise MemoryError(msg)
    raise GraceError("status %d: %s" % (status, msg))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    if t is None:
        return C.c_void_p(0)
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensor required"
    return C.c_void_p(t.data_ptr())


def _spheres(t):
    assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 4
    return t


def _rays(t):
    assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == RAY_FLOATS
    return t


def version():
    return _lib.grace_version()


def exported_symbols():
    """Every entry point include/grace_hip.h declares (checked by the CPU tests)."""
    return _lib


# ---------------------------------------------------------------------------------------
# Tree container -- include/grace/cuda/nodes.h:14-58
# ---------------------------------------------------------------------------------------
class Tree:
    """nodes: int32 [n_nodes, 16] (4 x int4/float4 per node), leaves: int32 [n_leaves, 4],
    root_index: device int32[1]; allocated for N leaves then shrunk by the build
    (nodes.h:48-52, albvh.cuh:842-845)."""

    def __init__(self, n_leaves, max_per_leaf=1, device="cuda"):
        self.max_per_leaf = int(max_per_leaf)
        self.nodes = torch.zeros((max(int(n_leaves) - 1, 1), 16), dtype=torch.int32, device=device)
        self.leaves = torch.zeros((int(n_leaves), 4), dtype=torch.int32, device=device)
        self.root_index = torch.zeros(1, dtype=torch.int32, device=device)

    @property
    def n_leaves(self):
        return self.leaves.shape[0]

    @property
    def n_nodes(self):
        return self.leaves.shape[0] - 1


# ---------------------------------------------------------------------------------------
# Build -- include/grace/cuda/build_sph.cuh
# ---------------------------------------------------------------------------------------
def centroid_bounds(spheres):
    bot = (C.c_float * 3)(); top = (C.c_float * 3)()
    _check(_lib.grace_centroid_bounds_f4(_ptr(_spheres(spheres)), C.c_size_t(len(spheres)),
                                         bot, top, _stream()))
    return np.array(bot, np.float32), np.array(top, np.float32)


def min_max_vec4(v):
    """grace::min_vec4 / max_vec4 (util/extrema.cuh) in one pass."""
    lo = (C.c_float * 4)(); hi = (C.c_float * 4)()
    _check(_lib.grace_minmax_f4(_ptr(_spheres(v)), C.c_size_t(len(v)), lo, hi, _stream()))
    return np.array(lo, np.float32), np.array(hi, np.float32)


def morton_keys_sph(spheres, keys, bot=None, top=None, double_bounds=False):
    """build_sph.cuh:19-35.  keys.dtype selects 30-bit (int32 storage of uint32) or 63-bit
    (int64 storage of uint64) keys."""
    _spheres(spheres)
    if bot is None:
        bot, top = centroid_bounds(spheres)
    n = C.c_size_t(len(spheres))
    if keys.dtype == torch.int32:
        b = (C.c_float * 3)(*[float(x) for x in bot]); t = (C.c_float * 3)(*[float(x) for x in top])
        _check(_lib.grace_morton_keys30_f4(_ptr(spheres), n, b, t, _ptr(keys), _stream()))
    elif keys.dtype == torch.int64:
        if double_bounds:
            b = (C.c_double * 3)(*[float(x) for x in bot]); t = (C.c_double * 3)(*[float(x) for x in top])
            _check(_lib.grace_morton_keys63_f4_d3(_ptr(spheres), n, b, t, _ptr(keys), _stream()))
        else:
            b = (C.c_float * 3)(*[float(x) for x in bot]); t = (C.c_float * 3)(*[float(x) for x in top])
            _check(_lib.grace_morton_keys63_f4(_ptr(spheres), n, b, t, _ptr(keys), _stream()))
    else:
        raise ValueError("keys must be int32 (30-bit) or int64 (63-bit) storage")
    return keys


def sort_by_key(keys, values=None, begin_bit=0, end_bit=None, want_perm=False):
    """thrust::sort_by_key contract: stable, ascending, keys and values permuted in place."""
    n = len(keys)
    perm = torch.empty(n, dtype=torch.int32, device=keys.device) if want_perm else None
    vb = 0
    if values is not None:
        assert values.is_contiguous() and len(values) == n
        vb = values.element_size() * (values.numel() // max(n, 1))
    if keys.dtype == torch.int32:
        fn, bits = _lib.grace_sort_pairs_u32, 32
    elif keys.dtype == torch.int64:
        fn, bits = _lib.grace_sort_pairs_u64, 64
    else:
        raise ValueError("keys must be int32/int64 storage of unsigned keys")
    _check(fn(_ptr(keys), _ptr(values), C.c_size_t(n), C.c_int(vb), C.c_int(begin_bit),
              C.c_int(bits if end_bit is None else end_bit), _ptr(perm), _stream()))
    return perm


def set_sort_overflow_hint(enabled):
    """grace_sort_set_overflow_hint: remember per context that the last large sort overflowed."""
    _check(_lib.grace_sort_set_overflow_hint(C.c_int(1 if enabled else 0)))


class _SortStats(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("msd_bits", "tile", "hint_skipped", "overflowed")]


def sort_last_stats():
    """grace_sort_last_stats: what the last sort of the calling thread's context planned, as a dict:
    msd_bits (0: index sort), tile, hint_skipped, overflowed (valid after a synchronise; -1: no
    bucket sort was enqueued or its flag word is unavailable)."""
    st = _SortStats()
    _check(_lib.grace_sort_last_stats(C.byref(st)))
    return {k: getattr(st, k) for k, _ in _SortStats._fields_}


def morton_keys30_sort_sph(spheres, bot=None, top=None):
    """build_sph.cuh:41-58: keys + stable sort of the spheres by key, in place."""
    keys = torch.empty(len(spheres), dtype=torch.int32, device=spheres.device)
    morton_keys_sph(spheres, keys, bot, top)
    sort_by_key(keys, spheres, 0, 30)
    return keys


def morton_keys63_sort_sph(spheres, bot=None, top=None):
    """build_sph.cuh:65-82."""
    keys = torch.empty(len(spheres), dtype=torch.int64, device=spheres.device)
    morton_keys_sph(spheres, keys, bot, top)
    sort_by_key(keys, spheres, 0, 63)
    return keys


def euclidean_deltas_sph(spheres, deltas):
    """build_sph.cuh:87-94; deltas has len(spheres) + 1 entries."""
    assert len(deltas) == len(spheres) + 1 and deltas.dtype == torch.float32
    _check(_lib.grace_deltas_euclid_f4(_ptr(_spheres(spheres)), C.c_size_t(len(spheres)),
                                       _ptr(deltas), _stream()))
    return deltas


def surface_area_deltas_sph(spheres, deltas):
    """build_sph.cuh:98-105."""
    assert len(deltas) == len(spheres) + 1 and deltas.dtype == torch.float32
    _check(_lib.grace_deltas_area_f4(_ptr(_spheres(spheres)), C.c_size_t(len(spheres)),
                                     _ptr(deltas), _stream()))
    return deltas


def XOR_deltas_sph(keys, deltas):
    """build_sph.cuh:109-114."""
    assert len(deltas) == len(keys) + 1 and deltas.dtype == keys.dtype
    fn = _lib.grace_deltas_xor_u32 if keys.dtype == torch.int32 else _lib.grace_deltas_xor_u64
    _check(fn(_ptr(keys), C.c_size_t(len(keys)), _ptr(deltas), _stream()))
    return deltas


def ALBVH_sph(spheres, deltas, tree):
    """build_sph.cuh:118-124 -> build_ALBVH (albvh.cuh:986-1021); shrinks tree.nodes/leaves."""
    n = len(spheres)
    assert tree.leaves.shape[0] >= n and len(deltas) == n + 1
    n_leaves = C.c_size_t(0)
    fn = {torch.float32: _lib.grace_albvh_build_f4, torch.float64: _lib.grace_albvh_build_f4_f64,
          torch.int32: _lib.grace_albvh_build_f4_u32,
          torch.int64: _lib.grace_albvh_build_f4_u64}.get(deltas.dtype)
    if fn is None:
        raise ValueError("deltas must be float32/float64 or 32/64-bit XOR deltas")
    _check(fn(_ptr(_spheres(spheres)), C.c_size_t(n), _ptr(deltas), C.c_int(tree.max_per_leaf),
              _ptr(tree.nodes), _ptr(tree.leaves), _ptr(tree.root_index), C.byref(n_leaves),
              _stream()))
    tree.leaves = tree.leaves[: n_leaves.value]
    tree.nodes = tree.nodes[: n_leaves.value - 1]
    return tree


PRIM_SPHERE_F4, PRIM_TRIANGLE, PRIM_SPHERE_D4, PRIM_BOX = 0, 1, 2, 3
COMP_LESS, COMP_GREATER = 0, 1
_DELTA_CODES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int64: 3}


def build_ALBVH(tree, prims, deltas, prim_kind=PRIM_SPHERE_F4, delta_comp=COMP_LESS):
    """The generic grace::build_ALBVH forms (kernels/albvh.cuh:986-1072) through
    grace_albvh_build_ex: prims are float4 / double4 spheres, triangles [n, 9], or -- PRIM_BOX --
    the caller's AABB functor already evaluated, [n, 6] floats {bot xyz, top xyz}; DeltaComp is
    thrust::less (default) or thrust::greater."""
    n = len(prims)
    assert tree.leaves.shape[0] >= n and len(deltas) == n + 1
    if deltas.dtype not in _DELTA_CODES:
        raise ValueError("deltas must be float32/float64 or 32/64-bit XOR deltas")
    n_leaves = C.c_size_t(0)
    _check(_lib.grace_albvh_build_ex(C.c_int(prim_kind), _ptr(prims), C.c_size_t(n),
                                     C.c_int(_DELTA_CODES[deltas.dtype]), _ptr(deltas), C.c_int(delta_comp),
                                     C.c_int(tree.max_per_leaf), _ptr(tree.nodes), _ptr(tree.leaves),
                                     _ptr(tree.root_index), C.byref(n_leaves), _stream()))
    tree.leaves = tree.leaves[: n_leaves.value]
    tree.nodes = tree.nodes[: n_leaves.value - 1]
    return tree


def min_max_components(data, n_comp, first=0):
    """grace::min_max_x/y/z/w, min/max_vec2/3/4 (util/extrema.cuh:190-772): minima and maxima of
    components first .. first + n_comp - 1 of the rows of a 2-D float32 / float64 / int32 tensor."""
    code = {torch.float32: 0, torch.float64: 1, torch.int32: 2}[data.dtype]
    assert data.dim() == 2 and data.is_contiguous() and first + n_comp <= data.shape[1]
    npdt = {0: np.float32, 1: np.float64, 2: np.int32}[code]
    lo = np.zeros(n_comp, npdt); hi = np.zeros(n_comp, npdt)
    elem = data.element_size()
    _check(_lib.grace_minmax_components(C.c_void_p(data.data_ptr() + first * elem), C.c_size_t(len(data)),
                                        C.c_int(code), C.c_int(n_comp), C.c_size_t(data.shape[1] * elem),
                                        lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p), _stream()))
    return lo, hi


def build_tree(spheres, tree, low=None, high=None, want_perm=False):
    """tests/helper/tree.cuh:15-43: 30-bit keys, Euclidean deltas, sorts spheres in place.
    want_perm=True returns (tree, perm) instead: perm[j] is the caller's index of the sphere now
    at position j (int32, from the same sort), so per-particle data in the caller's order is
    brought into tree order by data[perm]."""
    deltas = torch.empty(len(spheres) + 1, dtype=torch.float32, device=spheres.device)
    keys = torch.empty(len(spheres), dtype=torch.int32, device=spheres.device)
    morton_keys_sph(spheres, keys, low, high)
    perm = sort_by_key(keys, spheres, 0, 30, want_perm=want_perm)
    euclidean_deltas_sph(spheres, deltas)
    ALBVH_sph(spheres, deltas, tree)
    return (tree, perm) if want_perm else tree


# ---------------------------------------------------------------------------------------
# Trace -- include/grace/cuda/trace_sph.cuh
# ---------------------------------------------------------------------------------------
def _check_rays(rays):
    _rays(rays)
    if len(rays) % 32 != 0:
        # include/grace/cuda/kernels/bintree_trace.cuh:231-238
        raise ValueError("Number of rays must be a multiple of the warp size (32).")


def _trace_args(rays, spheres, tree):
    return (_ptr(rays), C.c_size_t(len(rays)), _ptr(_spheres(spheres)), C.c_size_t(len(spheres)),
            _ptr(tree.nodes), C.c_size_t(tree.n_nodes), _ptr(tree.leaves), _ptr(tree.root_index))


def hit_integrals(b2, h):
    """functors/trace.cuh:181-186 on arrays (device tensors), the traversal's own arithmetic."""
    out = torch.empty_like(b2)
    _check(_lib.grace_hit_integrals_f32(_ptr(b2), _ptr(h), C.c_size_t(len(b2)), _ptr(out), _stream()))
    return out


def enable_kernel_timing(enabled=True):
    _check(_lib.grace_trace_enable_timing(C.c_int(1 if enabled else 0)))


def last_kernel_ms():
    """Duration of the last traversal kernel alone (HIP events on its stream)."""
    ms = C.c_float(0)
    _check(_lib.grace_trace_last_kernel_ms(C.byref(ms)))
    return ms.value


def last_lattice():
    """1 if the last trace ran the origin-lattice instantiation (measurement hook)."""
    v = C.c_int(0)
    _check(_lib.grace_trace_last_lattice(C.byref(v)))
    return v.value


def set_packet_split(k):
    _check(_lib.grace_trace_set_packet_split(C.c_int(int(k))))


def set_packet_width(w):
    _check(_lib.grace_trace_set_packet_width(C.c_int(int(w))))


def set_exact_integrals(enabled):
    """Column-density trace: True = the reference's per-hit arithmetic bit for bit (slower);
    False (default) = hardware sqrt + fp32 table lerp (within the stated 1e-5 tolerance)."""
    _check(_lib.grace_trace_set_exact_integrals(C.c_int(1 if enabled else 0)))


# SPH kernels of the integrating traces (include/grace_hip.h, GRACE_SPH_KERNEL_*); the sphere's w is
# the kernel's support radius H.
SPH_KERNELS = ("cubic", "quartic", "quintic", "wendland_c2", "wendland_c4", "wendland_c6")
SPH_KERNEL_CUSTOM = -1


def _kernel_kind(name):
    if name not in SPH_KERNELS:
        raise ValueError("unknown SPH kernel %r (one of %s)" % (name, ", ".join(SPH_KERNELS)))
    return SPH_KERNELS.index(name)


def sph_kernel_table(name):
    """A built-in kernel's 51 line integrals F_i = int f(sqrt((i/50)^2 + z^2)) dz (support radius 1),
    float64.  Host only: needs no device."""
    out = (C.c_double * N_TABLE)()
    _check(_lib.grace_sph_kernel_table(C.c_int(_kernel_kind(name)), out))
    return np.array(out, np.float64)


def set_sph_kernel(kernel):
    """The current context's SPH kernel for every integrating trace (column densities, weighted sums,
    per-hit integrals, hit_integrals): a name of SPH_KERNELS, or a table of 51 float64 values (finite,
    >= 0, the last one 0).  Selecting a name switches a pointer; a table is copied to the device
    after a device synchronisation (queued traces may still read the previous one).  ValueError
    for anything else; the active kernel is then left as it was.  Calls already enqueued keep
    the kernel they were enqueued with."""
    if isinstance(kernel, str):
        _check(_lib.grace_trace_set_sph_kernel(C.c_int(_kernel_kind(kernel))))
        return
    t = np.asarray(kernel)
    if t.dtype.kind not in "fiu" or t.ndim != 1:
        raise ValueError("an SPH kernel table must be a 1-D array of 51 numbers")
    t = np.ascontiguousarray(t, dtype=np.float64)
    _check(_lib.grace_trace_set_sph_kernel_table(t.ctypes.data_as(C.POINTER(C.c_double)), C.c_int(len(t))))


def sph_kernel():
    """(name, float64 table) of the current context's SPH kernel; name is "custom" for a caller's table."""
    kind = C.c_int(0)
    out = (C.c_double * N_TABLE)()
    _check(_lib.grace_trace_get_sph_kernel(C.byref(kind), out))
    name = "custom" if kind.value == SPH_KERNEL_CUSTOM else SPH_KERNELS[kind.value]
    return name, np.array(out, np.float64)


def set_cache_validation(enabled):
    """1 (default): cached scene / ray records are validated by signature before every use."""
    _check(_lib.grace_trace_set_cache_validation(C.c_int(1 if enabled else 0)))


def set_cache_auto(enabled):
    """1 (default): the records of a scene / ray batch given twice in a row are cached."""
    _check(_lib.grace_trace_set_cache_auto(C.c_int(1 if enabled else 0)))


def set_plan(enabled):
    """Record and use packet plans for column-density traces served by both caches."""
    _check(_lib.grace_trace_set_plan(C.c_int(1 if enabled else 0)))


def set_plan_budget(n_bytes):
    """Device memory a packet plan may take (a plan beyond it is not kept)."""
    _check(_lib.grace_trace_set_plan_budget(C.c_size_t(int(n_bytes))))


def plan_bytes():
    """Device memory of the context's current packet plan (0: none)."""
    v = C.c_size_t(0)
    _check(_lib.grace_trace_plan_bytes(C.byref(v)))
    return v.value


def last_plan_used():
    """1 if the last column-density trace ran the planned kernel (measurement hook)."""
    v = C.c_int(0)
    _check(_lib.grace_trace_last_plan_used(C.byref(v)))
    return v.value


PlanStats = collections.namedtuple(
    "PlanStats", "entries survivors rounds full_rounds closed_by_capacity closed_by_flags largest_round")


def plan_stats():
    """Tallies of the plan the last column-density trace ran from (zeros: it ran from none): its
    entries, survivors and dense rounds, the rounds of exactly 64 survivors, the rounds closed by
    the 64-survivor capacity and by a change of the lean / fat bits, and the largest round."""
    v = (C.c_ulonglong * 7)()
    _check(_lib.grace_trace_plan_stats(v))
    return PlanStats(*[int(x) for x in v])


def plan_loops():
    """(loops, largest): the survivor loops the last column-density trace's planned kernel runs over
    its plan and the survivors of the largest (zeros: it ran from none)."""
    v = (C.c_ulonglong * 2)()
    _check(_lib.grace_trace_plan_loops(v))
    return int(v[0]), int(v[1])


def set_plan_subtiles(mode):
    """The plan's sub-tile layout (a survivor stream per quadrant of 16 rays): -1 automatic
    (default), 0 never, 1 whenever the call is eligible and the plan fits the budget."""
    _check(_lib.grace_trace_set_plan_subtiles(C.c_int(int(mode))))


def plan_subtiles():
    """(used, steps, slots): whether the last column-density trace ran from a plan of the sub-tile
    layout, the steps of its lists and the index words of their streams that name a survivor."""
    used, steps, slots = C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
    _check(_lib.grace_trace_plan_subtiles(C.byref(used), C.byref(steps), C.byref(slots)))
    return used.value, int(steps.value), int(slots.value)


def set_lattice_split(k):
    _check(_lib.grace_trace_set_lattice_split(C.c_int(k)))


def set_hits_staging(enabled):
    _check(_lib.grace_trace_set_hits_staging(C.c_int(1 if enabled else 0)))


class Context:
    """A library context (include/grace_hip.h, "contexts"): workspace, cached scene / ray order,
    knobs and status word of its own, on the device that is current at creation.  Use as
    `with Context(): ...` in the thread that should run on it."""

    def __init__(self):
        self._h = C.c_void_p(0)
        _check(_lib.grace_context_create(C.byref(self._h)))

    def make_current(self):
        _check(_lib.grace_context_set_current(self._h))

    @staticmethod
    def reset_current():
        _check(_lib.grace_context_set_current(C.c_void_p(0)))

    def destroy(self):
        if self._h:
            _check(_lib.grace_context_destroy(self._h))
            self._h = C.c_void_p(0)

    def __enter__(self):
        self.make_current()
        return self

    def __exit__(self, *exc):
        Context.reset_current()
        self.destroy()
        return False


def set_treelet_size(n):
    _check(_lib.grace_trace_set_treelet_size(C.c_int(int(n))))


def set_ray_reorder(enabled):
    _check(_lib.grace_trace_set_ray_reorder(C.c_int(1 if enabled else 0)))


def trace_status():
    _check(_lib.grace_trace_status(_stream()))


_prepared = {}   # tensors behind the prepared scene / ray batch (kept alive: see trace_prepare)


def trace_prepare(spheres, tree):
    """Computes the scene-constant trace data (per-sphere records, node spans, cluster boxes)
    once; later trace calls over the same spheres / tree reuse it until trace_release().  The
    caller must not modify spheres or tree in between (this library's own sort / build calls
    drop it themselves).  Not part of the reference API (its traces are stateless)."""
    _check(_lib.grace_trace_prepare_f4(_ptr(_spheres(spheres)), C.c_size_t(len(spheres)),
                                       _ptr(tree.nodes), C.c_size_t(tree.n_nodes),
                                       _ptr(tree.leaves), _stream()))
    # The cache is keyed on device pointers: keep the tensors alive while it is, so that the
    # allocator cannot hand their addresses to other data.
    _prepared["scene"] = (spheres, tree.nodes, tree.leaves)


def trace_prepare_tri(tris, tree):
    _check(_lib.grace_trace_prepare_tri(_ptr(_tris(tris)), C.c_size_t(len(tris)),
                                        _ptr(tree.nodes), C.c_size_t(tree.n_nodes),
                                        _ptr(tree.leaves), _stream()))
    _prepared["scene"] = (tris, tree.nodes, tree.leaves)


def trace_prepare_rays(rays):
    """Compute the coherence order of this ray batch once; later traces of the same tensor reuse it."""
    _check(_lib.grace_trace_prepare_rays(_ptr(_rays(rays)), C.c_size_t(len(rays)), _stream()))
    _prepared["rays"] = rays       # (see trace_prepare)


def trace_release_rays():
    _check(_lib.grace_trace_release_rays())
    _prepared.pop("rays", None)


def trace_release():
    _check(_lib.grace_trace_release())
    _prepared.pop("scene", None)


def _trace_hitcounts_keep(rays, spheres, tree, hit_counts, real=torch.float32):
    """The hit-count pass of trace_sph / trace_with_sentinels_sph: for small batches the library
    keeps the hits per (ray, primitive chunk) for the per-hit pass that follows.  real=float64:
    the mixed-precision pass, counted with the fp64 test its per-hit pass applies."""
    _check_rays(rays)
    fn = _lib.grace_trace_hitcounts_f4_f64 if real == torch.float64 else _lib.grace_trace_hitcounts_keep_f4
    _check(fn(*_trace_args(rays, spheres, tree), _ptr(hit_counts), _stream()))
    return hit_counts


def _real_of(real):
    assert real in (torch.float32, torch.float64), "real: torch.float32 or torch.float64"
    return real


def trace_hitcounts_f4_f64(rays, spheres, tree, hit_counts, check=False):
    """Hit counts under sphere_hit<float4, double> (the fp64 test on float spheres): the counts
    of the mixed-precision trace_sph.  trace_hitcounts_sph keeps the float test."""
    _check_rays(rays)
    assert hit_counts.dtype == torch.int32 and len(hit_counts) == len(rays)
    _check(_lib.grace_trace_hitcounts_f4_f64(*_trace_args(rays, spheres, tree), _ptr(hit_counts), _stream()))
    if check:
        trace_status()
    return hit_counts


def trace_hitcounts_sph(rays, spheres, tree, hit_counts, check=False):
    """trace_sph.cuh:58-80.  check=True also reads the traversal's status word (a
    synchronisation): packet-stack exhaustion then raises instead of waiting for the next
    trace_status() call."""
    _check_rays(rays)
    assert hit_counts.dtype == torch.int32 and len(hit_counts) == len(rays)
    _check(_lib.grace_trace_hitcounts_f4(*_trace_args(rays, spheres, tree), _ptr(hit_counts),
                                         _stream()))
    if check:
        trace_status()
    return hit_counts


def trace_cumulative_sph(rays, spheres, tree, cumulated, check=False):
    """trace_sph.cuh:82-110.  Asynchronous by default (the bench's timed loop relies on it);
    check=True reads the status word after the launch, as the C++ mirrors do.  cumulated.dtype
    picks Real: float32 (Real4 = float4, Real = float) or float64 (the mixed-precision
    trace_cumulative_sph<float4, double>: fp64 sphere test, double class-ordered sums)."""
    _check_rays(rays)
    assert cumulated.dtype in (torch.float32, torch.float64) and len(cumulated) == len(rays)
    fn = _lib.grace_trace_cumulative_f4_f64 if cumulated.dtype == torch.float64 else _lib.grace_trace_cumulative_f4
    _check(fn(*_trace_args(rays, spheres, tree), _ptr(cumulated), _stream()))
    if check:
        trace_status()
    return cumulated


def trace_cumulative_weighted_sph(rays, spheres, tree, weights, out=None, check=False):
    """Weighted, multi-channel column densities in one traversal (an extension the reference
    lacks): out[r, c] = sum over ray r's hits i of fl32(weights[i, c] * I_ri), I_ri being the term
    trace_cumulative_sph adds, summed per channel in its class order.  weights: float32 [n] or
    [n, C] (1 <= C <= 64), in the order of `spheres` (tree order: see build_tree(want_perm=True));
    out: float32 [n_rays] or [n_rays, C] to match (allocated if None).  Channels are traced four
    at a time, each group a walk of its own."""
    _check_rays(rays)
    if weights.dtype != torch.float32:
        raise ValueError("weights must be float32")
    if weights.dim() not in (1, 2) or weights.shape[0] != len(spheres):
        raise ValueError("weights must have shape [n_spheres] or [n_spheres, C]")
    n_ch = 1 if weights.dim() == 1 else weights.shape[1]
    if not 1 <= n_ch <= 64:
        raise ValueError("weights must have 1..64 channels")
    shape = (len(rays),) if weights.dim() == 1 else (len(rays), n_ch)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=rays.device)
    if out.dtype != torch.float32 or tuple(out.shape) != shape:
        raise ValueError("out must be float32 of shape %s" % (shape,))
    _check(_lib.grace_trace_cumulative_weighted_f4(*_trace_args(rays, spheres, tree), _ptr(weights),
                                                   C.c_int(n_ch), _ptr(out), _stream()))
    if check:
        trace_status()
    return out


def trace_emission_absorption_sph(rays, spheres, tree, emission, absorption, out=None, tau=None,
                                  check=False):
    """Depth-ordered emission-absorption integrals (an extension the reference lacks; the contract
    is in grace_hip.h): every ray's hits ordered by (distance, sphere index), then in fp64
    out[r, c] = sum_k emission[i_k, c] I_k phi(a_k) exp(-tau_k) with a_k = absorption[i_k] I_k,
    tau_k the sum of the a in front of hit k and phi(a) = -expm1(-a) / a; tau[r] = sum_k a_k.
    emission: float32 [n] or [n, C] (1 <= C <= 64), absorption: float32 [n], both in the order of
    `spheres` (tree order); out: float32 [n_rays] or [n_rays, C] to match (allocated if None);
    tau: float32 [n_rays], or None to skip it.  Returns out.  The rays are traced in batches
    whose per-hit arrays fit set_ordered_budget's bytes, so the total number of hits is not
    limited; the call synchronises the stream once."""
    _check_rays(rays)
    if emission.dtype != torch.float32 or absorption.dtype != torch.float32:
        raise ValueError("emission and absorption must be float32")
    if emission.dim() not in (1, 2) or emission.shape[0] != len(spheres):
        raise ValueError("emission must have shape [n_spheres] or [n_spheres, C]")
    if tuple(absorption.shape) != (len(spheres),):
        raise ValueError("absorption must have shape [n_spheres]")
    n_ch = 1 if emission.dim() == 1 else emission.shape[1]
    if not 1 <= n_ch <= 64:
        raise ValueError("emission must have 1..64 channels")
    shape = (len(rays),) if emission.dim() == 1 else (len(rays), n_ch)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=rays.device)
    if out.dtype != torch.float32 or tuple(out.shape) != shape:
        raise ValueError("out must be float32 of shape %s" % (shape,))
    if tau is not None and (tau.dtype != torch.float32 or tuple(tau.shape) != (len(rays),)):
        raise ValueError("tau must be float32 of shape [%d]" % len(rays))
    _check(_lib.grace_trace_emission_absorption_f4(*_trace_args(rays, spheres, tree), _ptr(emission),
                                                   C.c_int(n_ch), _ptr(absorption), _ptr(out), _ptr(tau),
                                                   _stream()))
    if check:
        trace_status()
    return out


def trace_absorption_deposit_sph(rays, spheres, tree, luminosity, absorption, deposit=None,
                                 transmitted=None, quantum=None, check=False):
    """Absorbed radiation deposited on the particles (an extension the reference lacks; the
    contract is in grace_hip.h): ray r carries luminosity[r, c]; its hits, ordered by (distance,
    sphere index), absorb dep = L exp(-tau_k) (1 - exp(-a_k)) each with a_k = absorption[i_k, c] I_k
    and tau_k the sum of the a in front of hit k, in fp64; deposit[i, c] is the sum over all rays
    and transmitted[r, c] = L exp(-sum_k a_k) what escapes.  The sum over rays is made in 64-bit
    fixed point with the quantum q_c = 2^(e_c + ceil(log2 n_rays) - 62), 2^(e_c - 1) <= max_r |L| <
    2^e_c, so deposit is bit-identical for any order of the rays.
    luminosity: float32 [n_rays] or [n_rays, C] (1 <= C <= 64); absorption: float32 [n] or [n, C]
    to match, in the order of `spheres` (tree order); deposit: float64 [n] or [n, C], overwritten
    (allocated if None); transmitted: float32 like luminosity, or None to skip it; quantum:
    float64 [C], or None.  Returns deposit.  Batches and budget as trace_emission_absorption_sph."""
    _check_rays(rays)
    if luminosity.dtype != torch.float32 or absorption.dtype != torch.float32:
        raise ValueError("luminosity and absorption must be float32")
    if luminosity.dim() not in (1, 2) or luminosity.shape[0] != len(rays):
        raise ValueError("luminosity must have shape [n_rays] or [n_rays, C]")
    n_ch = 1 if luminosity.dim() == 1 else luminosity.shape[1]
    if not 1 <= n_ch <= 64:
        raise ValueError("luminosity must have 1..64 channels")
    shape = (len(spheres),) if luminosity.dim() == 1 else (len(spheres), n_ch)
    if tuple(absorption.shape) != shape:
        raise ValueError("absorption must be float32 of shape %s" % (shape,))
    if deposit is None:
        deposit = torch.empty(shape, dtype=torch.float64, device=rays.device)
    if deposit.dtype != torch.float64 or tuple(deposit.shape) != shape:
        raise ValueError("deposit must be float64 of shape %s" % (shape,))
    if transmitted is not None and (transmitted.dtype != torch.float32
                                    or tuple(transmitted.shape) != tuple(luminosity.shape)):
        raise ValueError("transmitted must be float32 of shape %s" % (tuple(luminosity.shape),))
    if quantum is not None and (quantum.dtype != torch.float64 or tuple(quantum.shape) != (n_ch,)):
        raise ValueError("quantum must be float64 of shape [%d]" % n_ch)
    _check(_lib.grace_trace_absorption_deposit_f4(*_trace_args(rays, spheres, tree), _ptr(luminosity),
                                                  _ptr(absorption), C.c_int(n_ch), _ptr(deposit),
                                                  _ptr(transmitted), _ptr(quantum), _stream()))
    if check:
        trace_status()
    return deposit


class _SpectrumGrid(C.Structure):
    _fields_ = [("v0", C.c_double), ("dv", C.c_double), ("n_bins", C.c_int), ("periodic", C.c_int),
                ("hubble", C.c_double)]


def trace_spectra_sph(rays, spheres, tree, amount, width, velocity, v0, dv, n_bins, periodic=False,
                      hubble=0.0, tau=None, column=None, check=False):
    """Velocity-space absorption spectra along rays (an extension the reference lacks; the
    contract is in grace_hip.h): every ray's hits ordered by (distance, sphere index); hit k has the
    column N = amount[i_k, c] I_k, the velocity v = hubble d_k + velocity[i_k] . direction and the
    Doppler parameter b = width[i_k, c], and adds N times the Gaussian of width b about v,
    integrated over each bin [v0 + j dv, v0 + (j + 1) dv) within v -+ 6 b, to tau[r, c, j] / dv, in
    fp64 and in a fixed order.  periodic: velocity wraps with period n_bins dv; otherwise the bins
    are a window.  dv sum_j tau[r, c, j] = column[r, c] = sum_k N when nothing leaves the window.
    amount, width: float32 [n] or [n, C] (1 <= C <= 16), velocity: float32 [n, 3], all in the order
    of `spheres` (tree order); tau: float32 [n_rays, C, n_bins] (allocated if None); column: float32
    [n_rays, C], or None to skip it.  Returns tau.  Batches and budget as
    trace_emission_absorption_sph."""
    _check_rays(rays)
    if amount.dtype != torch.float32 or width.dtype != torch.float32 or velocity.dtype != torch.float32:
        raise ValueError("amount, width and velocity must be float32")
    if amount.dim() not in (1, 2) or amount.shape[0] != len(spheres):
        raise ValueError("amount must have shape [n_spheres] or [n_spheres, C]")
    n_ch = 1 if amount.dim() == 1 else amount.shape[1]
    if not 1 <= n_ch <= 16:
        raise ValueError("amount must have 1..16 channels")
    if tuple(width.shape) != tuple(amount.shape):
        raise ValueError("width must be float32 of shape %s" % (tuple(amount.shape),))
    if tuple(velocity.shape) != (len(spheres), 3):
        raise ValueError("velocity must be float32 of shape [n_spheres, 3]")
    n_bins = int(n_bins)
    if not 1 <= n_bins <= 4096:
        raise ValueError("n_bins must be 1..4096")
    if tau is None:
        tau = torch.empty((len(rays), n_ch, n_bins), dtype=torch.float32, device=rays.device)
    if tau.dtype != torch.float32 or tuple(tau.shape) != (len(rays), n_ch, n_bins):
        raise ValueError("tau must be float32 of shape %s" % ((len(rays), n_ch, n_bins),))
    if column is not None and (column.dtype != torch.float32 or tuple(column.shape) != (len(rays), n_ch)):
        raise ValueError("column must be float32 of shape %s" % ((len(rays), n_ch),))
    grid = _SpectrumGrid(float(v0), float(dv), n_bins, 1 if periodic else 0, float(hubble))
    _check(_lib.grace_trace_spectra_f4(*_trace_args(rays, spheres, tree), _ptr(amount), _ptr(width),
                                       _ptr(velocity), C.c_int(n_ch), C.byref(grid), _ptr(tau),
                                       _ptr(column), _stream()))
    if check:
        trace_status()
    return tau


def set_ordered_budget(n_bytes):
    """Bytes of per-hit arrays (12 a hit) one batch of trace_emission_absorption_sph,
    trace_absorption_deposit_sph or trace_spectra_sph may hold (process-wide; 0 restores the default).  A ray with
    more hits is a batch of its own."""
    _check(_lib.grace_trace_set_ordered_budget(C.c_size_t(int(n_bytes))))


def ordered_limits():
    """(wave_max_hits, block_max_hits): the hit counts up to which a ray is ordered by one wave /
    by one workgroup in LDS; longer rays are ordered in global memory."""
    w, b = C.c_int(0), C.c_int(0)
    _check(_lib.grace_trace_ordered_limits(C.byref(w), C.byref(b)))
    return w.value, b.value


class _OrderedStats(C.Structure):
    _fields_ = [(k, C.c_ulonglong) for k in ("batches", "total_hits", "rays_wave", "rays_block",
                                              "rays_global", "budget_bytes", "frame_bytes")] \
        + [(k, C.c_float) for k in ("ms_count", "ms_trace", "ms_composite")]


def ordered_enable_stats(enabled=True):
    """Measurement hook (process-wide): trace_emission_absorption_sph,
    trace_absorption_deposit_sph and trace_spectra_sph time their phases,
    synchronise before they return and record what they did."""
    _check(_lib.grace_trace_ordered_enable_stats(C.c_int(1 if enabled else 0)))


def ordered_last_stats():
    """The last trace_emission_absorption_sph / trace_absorption_deposit_sph / trace_spectra_sph call's record as a dict: batches, total_hits,
    rays_wave / rays_block / rays_global, budget_bytes, frame_bytes, ms_count / ms_trace /
    ms_composite."""
    st = _OrderedStats()
    _check(_lib.grace_trace_ordered_last_stats(C.byref(st)))
    return {k: getattr(st, k) for k, _ in _OrderedStats._fields_}


def _interp_outputs(n_points, n_spheres, weights, out, counts, device):
    """Checks weights / out / counts of an interpolation call and allocates what is missing."""
    if weights is None:
        if out is not None:
            raise ValueError("out needs weights")
        if counts is None:
            counts = torch.empty(n_points, dtype=torch.int32, device=device)
        n_ch, shape = 0, None
    else:
        if weights.dtype != torch.float32:
            raise ValueError("weights must be float32")
        if weights.dim() not in (1, 2) or weights.shape[0] != n_spheres:
            raise ValueError("weights must have shape [n_spheres] or [n_spheres, C]")
        n_ch = 1 if weights.dim() == 1 else weights.shape[1]
        if not 1 <= n_ch <= 64:
            raise ValueError("weights must have 1..64 channels")
        shape = (n_points,) if weights.dim() == 1 else (n_points, n_ch)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=device)
        if out.dtype != torch.float32 or tuple(out.shape) != shape:
            raise ValueError("out must be float32 of shape %s" % (shape,))
    if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (n_points,)):
        raise ValueError("counts must be int32 of shape [%d]" % n_points)
    return n_ch, out, counts


def _interp_scene(spheres, tree):
    return (_ptr(_spheres(spheres)), C.c_size_t(len(spheres)), _ptr(tree.nodes), C.c_size_t(tree.n_nodes),
            _ptr(tree.leaves), _ptr(tree.root_index))


def interpolate_sph(points, spheres, tree, weights=None, out=None, counts=None, check=False, period=None):
    """The SPH field at points (an extension the reference lacks):
    out[p, c] = sum over spheres i containing point p of fl32(weights[i, c] * W(|p - x_i|, H_i)), with
    the context's SPH kernel (set_sph_kernel; a custom table is refused), summed per channel in the
    class order of the column densities; counts[p] = the number of spheres containing p.
    points: float32 [n, 3..16] (x y z first); weights: float32 [n_spheres] or [n_spheres, C]
    (1 <= C <= 64) in the order of `spheres` (tree order: build_tree(want_perm=True)), or None for
    counts only.  period: None, or (Lx, Ly, Lz) for a periodic box (0 leaves an axis open): every
    component of p - x is wrapped once into [-L/2, L/2] before it is squared, and a sphere whose H exceeds
    half a period contributes nothing (include/grace_hip.h, "Periodic boxes").  Returns out (None without
    weights) and counts (allocated when weights is None or counts is given)."""
    if points.dtype != torch.float32 or points.dim() != 2 or not 3 <= points.shape[1] <= 16:
        raise ValueError("points must be float32 of shape [n, 3..16]")
    points = points.contiguous()
    n_ch, out, counts = _interp_outputs(len(points), len(spheres), weights, out, counts, points.device)
    args = (_ptr(points), C.c_size_t(len(points)), C.c_int(points.shape[1]), *_interp_scene(spheres, tree),
            _ptr(weights), C.c_int(n_ch), _ptr(out), _ptr(counts))
    if period is None:
        _check(_lib.grace_interpolate_points_f4(*args, _stream()))
    else:
        period = _period(period)
        _check(_lib.grace_interpolate_points_periodic_f4(*args, *_period_tail(period)))
    if check:
        trace_status()
    return out, counts


def interpolate_grid_sph(origin, u, v, w, dims, spheres, tree, weights=None, out=None, counts=None,
                         check=False, period=None):
    """interpolate_sph over the lattice p(i, j, k) = origin + i u + j v + k w (fp32, per component
    fl(fl(fl(o + fl(i u)) + fl(j v)) + fl(k w))), dims = (nx, ny, nz); nz = 1 is a slice (oblique
    ones too).  out: float32 [nz, ny, nx] or [nz, ny, nx, C]; counts: int32 [nz, ny, nx].  period: as for
    interpolate_sph (a mesh over a periodic box keeps the mass of the spheres that stick out of a face)."""
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) <= 0:
        raise ValueError("grid dimensions must be positive")
    n = nx * ny * nz
    dev = spheres.device
    flat_out = None if out is None else out.view(n, *out.shape[3:])
    flat_counts = None if counts is None else counts.view(n)
    n_ch, flat_out, flat_counts = _interp_outputs(n, len(spheres), weights, flat_out, flat_counts, dev)
    o3 = (C.c_float * 3)(*[float(x) for x in origin])
    uvw = (C.c_float * 9)(*[float(x) for x in (*u, *v, *w)])
    d3 = (C.c_int * 3)(nx, ny, nz)
    args = (o3, uvw, d3, *_interp_scene(spheres, tree), _ptr(weights), C.c_int(n_ch), _ptr(flat_out),
            _ptr(flat_counts))
    if period is None:
        _check(_lib.grace_interpolate_grid_f4(*args, _stream()))
    else:
        period = _period(period)
        _check(_lib.grace_interpolate_grid_periodic_f4(*args, *_period_tail(period)))
    if check:
        trace_status()
    grid = lambda t: None if t is None else t.view(nz, ny, nx, *t.shape[1:])
    return grid(flat_out), grid(flat_counts)


def interpolate_enable_stats(enabled=True):
    """Measurement hook: count survivor tests of every interpolation call (process-wide)."""
    _check(_lib.grace_interpolate_enable_stats(C.c_int(1 if enabled else 0)))


def interpolate_last_stats():
    """Survivor tests (active lanes x survivors) of the last interpolation call; synchronises."""
    v = C.c_ulonglong(0)
    _check(_lib.grace_interpolate_last_stats(C.byref(v)))
    return v.value


def _gradient_outputs(n_points, n_spheres, weights, grad, value, counts, device):
    """Checks weights / grad / value / counts of a gradient call and allocates grad when it is missing."""
    if weights is None:
        raise ValueError("a gradient needs weights")
    if weights.dtype != torch.float32 or weights.dim() not in (1, 2) or weights.shape[0] != n_spheres:
        raise ValueError("weights must be float32 of shape [n_spheres] or [n_spheres, C]")
    n_ch = 1 if weights.dim() == 1 else weights.shape[1]
    if not 1 <= n_ch <= 64:
        raise ValueError("weights must have 1..64 channels")
    if value is not None:                                  # (checked like interpolate_sph's out; never allocated)
        _, value, counts = _interp_outputs(n_points, n_spheres, weights, value, counts, device)
    elif counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (n_points,)):
        raise ValueError("counts must be int32 of shape [%d]" % n_points)
    shape = (n_points, 3) if weights.dim() == 1 else (n_points, n_ch, 3)
    if grad is None:
        grad = torch.empty(shape, dtype=torch.float32, device=device)
    if grad.dtype != torch.float32 or tuple(grad.shape) != shape:
        raise ValueError("grad must be float32 of shape %s" % (shape,))
    return n_ch, grad, value, counts


def interpolate_gradient_sph(points, spheres, tree, weights, grad=None, value=None, counts=None, check=False,
                             period=None):
    """The gradient of the SPH field of interpolate_sph at points (an extension the reference lacks):
    grad[p, c, k] = sum over spheres i containing point p of fl32(fl32(weights[i, c] * G) * n_k), with
    G = H^-4 f'(q) of the context's SPH kernel and n the unit vector from the sphere's centre to the
    point (at the centre itself the term is +0); containment, the wrap of a periodic box and the class
    order of the sums are interpolate_sph's (include/grace_hip.h, "SPH gradients at points").
    points, weights, period: as for interpolate_sph, but weights are required.  grad: float32 [n, 3] for
    weights [n_spheres], [n, C, 3] for [n_spheres, C].  value (float32 [n] or [n, C]) and counts
    (int32 [n]), when given, receive exactly interpolate_sph's out and counts from the same walk.
    weights = m gives the density gradient; grad A - A grad 1 comes from a channel of m / rho * A and a
    channel of m / rho.  Returns (grad, value, counts)."""
    if points.dtype != torch.float32 or points.dim() != 2 or not 3 <= points.shape[1] <= 16:
        raise ValueError("points must be float32 of shape [n, 3..16]")
    points = points.contiguous()
    n_ch, grad, value, counts = _gradient_outputs(len(points), len(spheres), weights, grad, value, counts,
                                                  points.device)
    args = (_ptr(points), C.c_size_t(len(points)), C.c_int(points.shape[1]), *_interp_scene(spheres, tree),
            _ptr(weights), C.c_int(n_ch), _ptr(grad), _ptr(value), _ptr(counts))
    if period is None:
        _check(_lib.grace_interpolate_gradient_points_f4(*args, _stream()))
    else:
        period = _period(period)
        _check(_lib.grace_interpolate_gradient_points_periodic_f4(*args, *_period_tail(period)))
    if check:
        trace_status()
    return grad, value, counts


def interpolate_gradient_grid_sph(origin, u, v, w, dims, spheres, tree, weights, grad=None, value=None,
                                  counts=None, check=False, period=None):
    """interpolate_gradient_sph over the lattice of interpolate_grid_sph.  grad: float32 [nz, ny, nx, 3]
    or [nz, ny, nx, C, 3]; value: [nz, ny, nx] or [nz, ny, nx, C]; counts: int32 [nz, ny, nx]."""
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) <= 0:
        raise ValueError("grid dimensions must be positive")
    n = nx * ny * nz
    flat = lambda t: None if t is None else t.view(n, *t.shape[3:])
    n_ch, fgrad, fvalue, fcounts = _gradient_outputs(n, len(spheres), weights, flat(grad), flat(value),
                                                     flat(counts), spheres.device)
    o3 = (C.c_float * 3)(*[float(x) for x in origin])
    uvw = (C.c_float * 9)(*[float(x) for x in (*u, *v, *w)])
    d3 = (C.c_int * 3)(nx, ny, nz)
    args = (o3, uvw, d3, *_interp_scene(spheres, tree), _ptr(weights), C.c_int(n_ch), _ptr(fgrad), _ptr(fvalue),
            _ptr(fcounts))
    if period is None:
        _check(_lib.grace_interpolate_gradient_grid_f4(*args, _stream()))
    else:
        period = _period(period)
        _check(_lib.grace_interpolate_gradient_grid_periodic_f4(*args, *_period_tail(period)))
    if check:
        trace_status()
    grid = lambda t: None if t is None else t.view(nz, ny, nx, *t.shape[1:])
    return grid(fgrad), grid(fvalue), grid(fcounts)


def gradient_div_curl(grad, div=None, curl=None):
    """Divergence and curl of a vector field from the gradient of its three channels, element-wise
    (grace_gradient_div_curl_f32): grad float32 [n, 3, 3] with grad[p, c, k] = d_k A_c;
    div[p] = fl(fl(g_xx + g_yy) + g_zz), curl[p] = (g_zy - g_yz, g_xz - g_zx, g_yx - g_xy).
    Returns (div [n], curl [n, 3]), allocated when missing."""
    if grad.dtype != torch.float32 or grad.dim() != 3 or tuple(grad.shape[1:]) != (3, 3):
        raise ValueError("grad must be float32 of shape [n, 3, 3]")
    grad = grad.contiguous()
    n = len(grad)
    if div is None:
        div = torch.empty(n, dtype=torch.float32, device=grad.device)
    if curl is None:
        curl = torch.empty((n, 3), dtype=torch.float32, device=grad.device)
    if div.dtype != torch.float32 or tuple(div.shape) != (n,) or curl.dtype != torch.float32 \
            or tuple(curl.shape) != (n, 3):
        raise ValueError("div must be float32 [n] and curl float32 [n, 3]")
    if n == 0:                                             # (empty tensors have null pointers: "no output" to the library)
        return div, curl
    _check(_lib.grace_gradient_div_curl_f32(_ptr(grad), C.c_size_t(n), _ptr(div), _ptr(curl), _stream()))
    return div, curl


def divergence_curl_sph(points, spheres, tree, vectors, period=None):
    """Divergence and curl at points of the SPH vector field with the weights `vectors` (float32
    [n_spheres, 3], e.g. m / rho * v): interpolate_gradient_sph of the three channels, then
    gradient_div_curl.  Returns (div [n], curl [n, 3])."""
    if vectors.dim() != 2 or vectors.shape[1] != 3:
        raise ValueError("vectors must have shape [n_spheres, 3]")
    grad = interpolate_gradient_sph(points, spheres, tree, vectors, period=period)[0]
    return gradient_div_curl(grad)


def interpolate_gradient_channels_per_walk(channels=0):
    """Measurement hook (process-wide, results never depend on it): gradient channels per walk, 1 or 2;
    0 restores the default.  Returns the value in effect."""
    return int(_lib.grace_interpolate_gradient_channels_per_walk(C.c_int(channels)))


def nearest_neighbours_sph(points, spheres, tree, k, indices=None, d2=None, check=False, period=None):
    """The k nearest sphere centres of each point (an extension the reference lacks): spheres are
    ranked by (d2, tree index), d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)) in fp32; row p holds
    the first k.  Slots beyond the number of spheres, and every slot of a point with a non-finite
    coordinate, are -1 / +inf.  points: float32 [n, 3..16] (x y z first); 1 <= k <= 64.  period: None, or
    (Lx, Ly, Lz) for a periodic box (0 leaves an axis open): every component of p - x is wrapped once
    into [-L/2, L/2] before it is squared (include/grace_hip.h, "Periodic boxes"); there is no radius limit.
    Returns (indices int32 [n, k], d2 float32 [n, k])."""
    if points.dtype != torch.float32 or points.dim() != 2 or not 3 <= points.shape[1] <= 16:
        raise ValueError("points must be float32 of shape [n, 3..16]")
    k = int(k)
    if not 1 <= k <= 64:
        raise ValueError("k must be 1..64")
    points = points.contiguous()
    shape = (len(points), k)
    if indices is None:
        indices = torch.empty(shape, dtype=torch.int32, device=points.device)
    if d2 is None:
        d2 = torch.empty(shape, dtype=torch.float32, device=points.device)
    if indices.dtype != torch.int32 or tuple(indices.shape) != shape:
        raise ValueError("indices must be int32 of shape %s" % (shape,))
    if d2.dtype != torch.float32 or tuple(d2.shape) != shape:
        raise ValueError("d2 must be float32 of shape %s" % (shape,))
    args = (_ptr(points), C.c_size_t(len(points)), C.c_int(points.shape[1]), *_interp_scene(spheres, tree),
            C.c_int(k), _ptr(indices), _ptr(d2))
    if period is None:
        _check(_lib.grace_nearest_neighbours_f4(*args, _stream()))
    else:
        period = _period(period)
        _check(_lib.grace_nearest_neighbours_periodic_f4(*args, *_period_tail(period)))
    if check:
        trace_status()
    return indices, d2


def smoothing_lengths_sph(spheres, tree, k, eta=1.0, out=None, check=False, period=None):
    """Smoothing lengths from the k-th nearest neighbour: h[i] = fl(eta * sqrt(D_i)), D_i the d2 of
    slot k-1 of nearest_neighbours_sph at sphere i's own centre (it is its own first neighbour).
    Returns h float32 [n] in tree order (the order of `spheres`, which is only read); to use it as
    H, write it into spheres[:, 3] and build the tree again.  1 <= k <= min(64, n); eta > 0.  period: as for
    nearest_neighbours_sph (a snapshot's BoxSize: particles near a face count their neighbours beyond it)."""
    n = len(spheres)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=spheres.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (n,):
        raise ValueError("out must be float32 of shape [%d]" % n)
    args = (*_interp_scene(spheres, tree), C.c_int(int(k)), C.c_float(float(eta)), _ptr(out))
    if period is None:
        _check(_lib.grace_smoothing_lengths_f4(*args, _stream()))
    else:
        period = _period(period)
        _check(_lib.grace_smoothing_lengths_periodic_f4(*args, *_period_tail(period)))
    if check:
        trace_status()
    return out


def neighbours_enable_stats(enabled=True):
    """Measurement hook: count candidate tests and packets of every neighbour call (process-wide)."""
    _check(_lib.grace_neighbours_enable_stats(C.c_int(1 if enabled else 0)))


def neighbours_last_stats():
    """(candidate tests (active lanes x survivors), packets, insertion steps (survivors for which some
    lane of the packet inserted)) of the last neighbour call; synchronises."""
    t = C.c_ulonglong(0); p = C.c_ulonglong(0); s = C.c_ulonglong(0)
    _check(_lib.grace_neighbours_last_stats(C.byref(t), C.byref(p), C.byref(s)))
    return t.value, p.value, s.value


INT32_MAX = 2 ** 31 - 1


def _range_args(points, radii):
    """points and radii of a range query -> (points, radii tensor or None, scalar radius)."""
    if points.dtype != torch.float32 or points.dim() != 2 or not 3 <= points.shape[1] <= 16:
        raise ValueError("points must be float32 of shape [n, 3..16]")
    points = points.contiguous()
    if torch.is_tensor(radii):
        if radii.dtype != torch.float32 or tuple(radii.shape) != (len(points),):
            raise ValueError("radii must be a float or float32 of shape [%d]" % len(points))
        return points, radii.contiguous(), 0.0
    return points, None, float(radii)


def _period(period):
    """A period of a periodic query -> three host floats (the library checks their values)."""
    if torch.is_tensor(period):
        period = period.detach().cpu().numpy()
    period = np.ascontiguousarray(np.asarray(period, dtype=np.float32).reshape(-1))
    if len(period) != 3:
        raise ValueError("period must hold three values (Lx, Ly, Lz); 0 leaves an axis open")
    return period


def _period_tail(period):
    """The arguments that follow the outputs: (period,) stream."""
    return (period.ctypes.data_as(C.c_void_p), _stream())


def range_counts_sph(points, radii, spheres, tree, weights=None, counts=None, out=None, check=False, period=None):
    """Every sphere centre within the query point's own radius (an extension the reference lacks):
    sphere j is in range of point p iff d2 <= fl(r_p * r_p), d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz))
    in fp32 -- inclusive; the spheres' w is ignored.  counts[p] = the number of spheres in range, and
    with weights the gather form of the SPH sum,
    sums[p, c] = sum over in-range j, ascending, of fl32(weights[j, c] * W(|x_p - x_j|, r_p)),
    a plain fp32 running sum with the context's SPH kernel (set_sph_kernel; a custom table is refused),
    0 where r_p == 0.  weights = m gives the density at the smoothing length r_p.
    points: float32 [n, 3..16] (x y z first); radii: a float, or float32 [n] in the order of points;
    weights: float32 [n_spheres] or [n_spheres, C] (1 <= C <= 64) in the order of `spheres` (tree order:
    build_tree(want_perm=True)).  A point with a non-finite coordinate or a negative, NaN or infinite
    radius gets 0.  period: None, or (Lx, Ly, Lz) for a periodic box (0 leaves an axis open): every
    component of p - x is wrapped once into [-L/2, L/2] before it is squared (include/grace_hip.h states
    the arithmetic), a point whose radius exceeds half a period gets 0, and a scalar radius that does is
    refused.  Returns (counts int32 [n], sums float32 [n] / [n, C] or None without weights)."""
    points, rt, rs = _range_args(points, radii)
    n = len(points)
    if counts is None:
        counts = torch.empty(n, dtype=torch.int32, device=points.device)
    n_ch, out, counts = _interp_outputs(n, len(spheres), weights, out, counts, points.device)
    if weights is not None:
        weights = weights.contiguous()
    args = (_ptr(points), C.c_size_t(n), C.c_int(points.shape[1]), _ptr(rt), C.c_float(rs),
            *_interp_scene(spheres, tree), _ptr(weights), C.c_int(n_ch), _ptr(counts), _ptr(out))
    if period is None:
        _check(_lib.grace_range_counts_f4(*args, _stream()))
    else:
        period = _period(period)
        _check(_lib.grace_range_counts_periodic_f4(*args, *_period_tail(period)))
    if check:
        trace_status()
    return counts, out


def range_neighbours_sph(points, radii, spheres, tree, want_d2=True, check=False, period=None):
    """The neighbour lists of range_counts_sph in CSR form: row p is [offsets[p], offsets[p + 1]) of
    indices (tree indices, ascending) and d2 (their fp32 squared distances).  Counts, the library's
    scan, then the fill; synchronises to read the total.  ValueError if the lists hold more than
    INT32_MAX entries (split the points).  period: as for range_counts_sph; d2 is the wrapped one.
    Returns (offsets int32 [n + 1], indices int32 [total], d2 float32 [total] or None)."""
    points, rt, rs = _range_args(points, radii)
    n = len(points)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=points.device)
    args = (_ptr(points), C.c_size_t(n), C.c_int(points.shape[1]), _ptr(rt), C.c_float(rs),
            *_interp_scene(spheres, tree))
    if period is None:
        count_fn, fill_fn, tail = _lib.grace_range_counts_f4, _lib.grace_range_neighbours_f4, (_stream(),)
    else:
        period = _period(period)
        count_fn, fill_fn = _lib.grace_range_counts_periodic_f4, _lib.grace_range_neighbours_periodic_f4
        tail = _period_tail(period)
    _check(count_fn(*args, _ptr(None), C.c_int(0), _ptr(offsets), _ptr(None), *tail))
    total = exclusive_scan(offsets, offsets)
    if total > INT32_MAX:
        raise ValueError("range_neighbours_sph: %d list entries exceed INT32_MAX; the int offsets cannot "
                         "address them. Split the points into several calls." % total)
    indices = torch.empty(total, dtype=torch.int32, device=points.device)
    d2 = torch.empty(total, dtype=torch.float32, device=points.device) if want_d2 else None
    if total:                  # (no list entries: every row is empty, nothing to fill)
        _check(fill_fn(*args, _ptr(offsets), _ptr(indices), _ptr(d2), *tail))
    if check:
        trace_status()
    return offsets, indices, d2


def fof_labels_sph(spheres, tree, linking_length, labels=None, check=False, period=None):
    """Friends-of-friends groups (an extension the reference lacks): spheres i and j (tree order; their
    w is ignored) are linked iff d2 <= fl(b * b), b the linking length,
    d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)) in fp32 -- inclusive, so b = 0 links coincident
    centres; groups are the connected components.  labels[i] = the smallest tree index in i's group:
    a function of the positions and b alone, bit-identical from run to run.  A sphere with a
    non-finite coordinate is a group of one.  period: None, or (Lx, Ly, Lz) for a periodic box (0 leaves
    an axis open): d is wrapped once per component as for range_counts_sph, so a group that straddles
    a face is one group; a linking length above half a period is refused.  Returns labels int32 [n]
    (tree order: map them to the caller's particles with the permutation of build_tree(want_perm=True))."""
    n = len(_spheres(spheres))
    if labels is None:
        labels = torch.empty(n, dtype=torch.int32, device=spheres.device)
    if labels.dtype != torch.int32 or tuple(labels.shape) != (n,):
        raise ValueError("labels must be int32 of shape [%d]" % n)
    args = (*_interp_scene(spheres, tree), C.c_float(float(linking_length)), _ptr(labels))
    if period is None:
        _check(_lib.grace_fof_labels_f4(*args, _stream()))
    else:
        period = _period(period)
        _check(_lib.grace_fof_labels_periodic_f4(*args, *_period_tail(period)))
    if check:
        trace_status()
    return labels


def fof_groups_sph(labels, min_members=1, want_members=True):
    """The catalogue of fof_labels_sph's labels: groups of at least min_members members, numbered in
    ascending label.  group_of[i] = sphere i's group or -1; sizes[g] = its member count; with
    want_members the CSR lists: row g is [offsets[g], offsets[g + 1]) of members, tree indices in
    ascending order.  Ordering by size is one argsort of sizes.  Synchronises once, to read the
    number of groups.  Returns (group_of int32 [n], sizes int32 [n_groups], offsets int32
    [n_groups + 1], members int32 [members of kept groups]); offsets and members are None without
    want_members."""
    if labels.dtype != torch.int32 or labels.dim() != 1:
        raise ValueError("labels must be int32 of shape [n]")
    labels = labels.contiguous()
    n = len(labels)
    dev = labels.device
    group_of = torch.empty(n, dtype=torch.int32, device=dev)
    sizes = torch.empty(n, dtype=torch.int32, device=dev)
    n_groups = torch.zeros(2, dtype=torch.int32, device=dev)     # {groups, members of kept groups}
    _check(_lib.grace_fof_groups(_ptr(labels), C.c_size_t(n), C.c_int(int(min_members)), _ptr(group_of),
                                 _ptr(sizes), _ptr(n_groups), _stream()))
    ng, nm = (int(v) for v in n_groups.tolist())
    sizes = sizes[:ng]
    if not want_members:
        return group_of, sizes, None, None
    offsets = torch.zeros(ng + 1, dtype=torch.int32, device=dev)
    members = torch.empty(nm, dtype=torch.int32, device=dev)
    _check(_lib.grace_fof_members(_ptr(group_of), C.c_size_t(n), _ptr(sizes), C.c_size_t(ng), _ptr(offsets),
                                  _ptr(members), _stream()))
    return group_of, sizes, offsets, members


def _pair_edges(edges):
    """The edges of a pair count -> a host float32 array (the library checks their values)."""
    if torch.is_tensor(edges):
        edges = edges.detach().cpu().numpy()
    edges = np.ascontiguousarray(np.asarray(edges, dtype=np.float32).reshape(-1))
    if not 1 <= len(edges) <= 64:
        raise ValueError("edges must hold 1..64 values")
    return edges


def _pair_call(points, edges, spheres, tree, weights, n_ch, totals, counts, sums, check, period=None):
    args = (_ptr(points), C.c_size_t(len(points)), C.c_int(points.shape[1]),
            edges.ctypes.data_as(C.c_void_p), C.c_int(len(edges)),
            *_interp_scene(spheres, tree), _ptr(weights), C.c_int(n_ch),
            _ptr(totals), _ptr(counts), _ptr(sums))
    if period is None:
        _check(_lib.grace_pair_counts_f4(*args, _stream()))
    else:
        period = _period(period)
        _check(_lib.grace_pair_counts_periodic_f4(*args, *_period_tail(period)))
    if check:
        trace_status()


def pair_counts_sph(points, edges, spheres, tree, check=False, period=None):
    """Pair counts in separation bins (an extension the reference lacks): totals[k] = the number of
    (point, sphere) pairs whose d2 = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)) (fp32) falls in bin k,
    the smallest k with d2 <= fl(e_k * e_k) -- bin 0 holds d2 <= fl(e_0 e_0) (with e_0 = 0 the
    coincident and self pairs), bin k >= 1 holds fl(e_{k-1} e_{k-1}) < d2 <= fl(e_k e_k), pairs beyond
    the last edge are in no bin; the spheres' w is ignored.  One walk at the last edge, exact 64-bit
    integer totals.  Pairs are ordered: with the sphere centres as points every unordered pair is
    counted twice and every self pair once, so DD = (totals - [n, 0, 0, ...]) // 2.
    points: float32 [n, 3..16] (x y z first); edges: 1..64 floats (a sequence, array or tensor; read on
    the host), finite, not negative, strictly ascending.  A point with a non-finite coordinate is in
    no pair.  period: None, or (Lx, Ly, Lz) for a periodic box (0 leaves an axis open): d is wrapped
    once per component as for range_counts_sph, each pair is still counted once, and a last edge above
    half a period is refused -- the DD(r) on the torus that an analytic RR goes with.
    Returns totals uint64 [n_edges]."""
    if points.dtype != torch.float32 or points.dim() != 2 or not 3 <= points.shape[1] <= 16:
        raise ValueError("points must be float32 of shape [n, 3..16]")
    points = points.contiguous()
    edges = _pair_edges(edges)
    totals = torch.empty(len(edges), dtype=torch.uint64, device=points.device)
    _pair_call(points, edges, spheres, tree, None, 0, totals, None, None, check, period)
    return totals


def radial_profiles_sph(points, edges, spheres, tree, weights=None, check=False, period=None):
    """The per-point form of pair_counts_sph: counts[p, k] = the number of sphere centres in bin k of
    point p, and with weights sums[p, k, c] = the sum of weights[j, c] over those spheres in ascending
    tree index j, a plain fp32 running sum (no SPH kernel): counts and mass in shells around each point;
    the cumulative profile is a cumsum over k.  counts.cumsum(1)[:, k] is range_counts_sph at radius
    e_k.  weights: float32 [n_spheres] or [n_spheres, C], 1 <= C <= 4 and n_edges * C <= 64, in the
    order of `spheres` (tree order: build_tree(want_perm=True)).  A point with a non-finite coordinate
    gets zeros.  period: as for pair_counts_sph.  Returns (counts int32 [n, n_edges], sums float32
    [n, n_edges] / [n, n_edges, C] or None without weights)."""
    if points.dtype != torch.float32 or points.dim() != 2 or not 3 <= points.shape[1] <= 16:
        raise ValueError("points must be float32 of shape [n, 3..16]")
    points = points.contiguous()
    edges = _pair_edges(edges)
    n, ne = len(points), len(edges)
    counts = torch.empty((n, ne), dtype=torch.int32, device=points.device)
    n_ch, sums = 0, None
    if weights is not None:
        if weights.dtype != torch.float32 or weights.dim() not in (1, 2) or len(weights) != len(spheres):
            raise ValueError("weights must be float32 of shape [n_spheres] or [n_spheres, C]")
        n_ch = 1 if weights.dim() == 1 else int(weights.shape[1])
        if not 1 <= n_ch <= 4 or ne * n_ch > 64:
            raise ValueError("weights must hold 1..4 channels and n_edges * channels must not exceed 64")
        weights = weights.contiguous()
        sums = torch.empty((n, ne) if weights.dim() == 1 else (n, ne, n_ch), dtype=torch.float32,
                           device=points.device)
    _pair_call(points, edges, spheres, tree, weights, n_ch, None, counts, sums, check, period)
    return counts, sums


def _gravity_masses(masses, spheres):
    if masses.dtype != torch.float32 or tuple(masses.shape) != (len(_spheres(spheres)),):
        raise ValueError("masses must be float32 of shape [n_spheres]")
    return masses.contiguous()


def gravity_moments_sph(spheres, masses, tree, moments=None):
    """The node moments of the tree gravity (an extension the reference lacks): per inner node the
    monopole {c, M32}, the tight box of the centres below it and the span of primitives it covers,
    moments[i] = {c_x, c_y, c_z, M32, lo_x, lo_y, lo_z, bits(span_lo), hi_x, hi_y, hi_z, bits(span_hi)}.
    Masses and first moments are fp64 sums, per leaf over ascending tree index, per node left + right;
    c = float(S / M), M32 = float(M), c = lo where M == 0 (include/grace_hip.h states every step).
    masses: float32 [n_spheres] in the order of `spheres` (tree order: build_tree(want_perm=True)); the
    spheres' w is ignored.  Computed once per tree and set of masses, then read by any number of
    gravity_sph calls.  Returns moments float32 [n_nodes, 12] (no rows where the root is a leaf)."""
    masses = _gravity_masses(masses, spheres)
    n_nodes = tree.n_nodes
    if moments is None:
        moments = torch.empty((n_nodes, 12), dtype=torch.float32, device=spheres.device)
    if moments.dtype != torch.float32 or tuple(moments.shape) != (n_nodes, 12):
        raise ValueError("moments must be float32 of shape [%d, 12]" % n_nodes)
    _check(_lib.grace_gravity_moments_f4(*_interp_scene(spheres, tree), _ptr(masses),
                                         _ptr(moments) if n_nodes else C.c_void_p(0), _stream()))
    return moments


def gravity_sph(points, spheres, masses, tree, moments, theta=0.5, eps=0.0, out=None, counts=None, check=False):
    """Potentials and accelerations at points from the BVH (an extension the reference lacks): the
    Barnes-Hut walk with monopoles of the inner nodes, G = 1.  Per point the recursion from the root: an
    inner node whose box has size2 < fl(theta^2 * d2min) -- size its longest edge, d2min the squared
    distance from the point to the box, fp32 -- contributes one term {c, M32}; any other node is opened,
    left child first; a leaf contributes one term per primitive.  A term is, in fp32, d = x - p,
    d2 = |d|^2, nothing if d2 == 0 (the self pair), else ir = 1 / sqrt(d2 + eps^2), m ir^3 d into the
    acceleration and m ir into the potential, both fp64 running sums in the order of the recursion
    (include/grace_hip.h states every rounding).  theta = 0 is the direct sum over all spheres in
    ascending tree index and does not depend on the tree; eps is a Plummer softening length for all
    particles, 0 is Newtonian.
    points: float32 [n, 3..16] (x y z first); masses: float32 [n_spheres] in tree order; moments:
    gravity_moments_sph(spheres, masses, tree).  A point with a non-finite coordinate gets zeros.
    Returns (out float64 [n, 4] = {a_x, a_y, a_z, phi}, counts int32 [n, 2] = {node terms, particle
    terms} if counts is True or a tensor to fill, else None)."""
    if points.dtype != torch.float32 or points.dim() != 2 or not 3 <= points.shape[1] <= 16:
        raise ValueError("points must be float32 of shape [n, 3..16]")
    points = points.contiguous()
    masses = _gravity_masses(masses, spheres)
    n, n_nodes = len(points), tree.n_nodes
    if n_nodes and (moments is None or moments.dtype != torch.float32 or tuple(moments.shape) != (n_nodes, 12)):
        raise ValueError("moments must be float32 of shape [%d, 12]" % n_nodes)
    if out is None:
        out = torch.empty((n, 4), dtype=torch.float64, device=points.device)
    if out.dtype != torch.float64 or tuple(out.shape) != (n, 4):
        raise ValueError("out must be float64 of shape [%d, 4]" % n)
    if counts is True:
        counts = torch.empty((n, 2), dtype=torch.int32, device=points.device)
    if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (n, 2)):
        raise ValueError("counts must be True or int32 of shape [%d, 2]" % n)
    _check(_lib.grace_gravity_points_f4(_ptr(points), C.c_size_t(n), C.c_int(points.shape[1]),
                                        *_interp_scene(spheres, tree), _ptr(masses),
                                        _ptr(moments) if n_nodes else C.c_void_p(0),
                                        C.c_float(float(theta)), C.c_float(float(eps)), _ptr(out), _ptr(counts),
                                        _stream()))
    if check:
        trace_status()
    return out, counts


def _gravity_labels(labels, n, what, of):
    if labels.dtype != torch.int32 or tuple(labels.shape) != (n,):
        raise ValueError("%s must be int32 of shape [%s]" % (what, of))
    return labels.contiguous()


def gravity_group_moments_sph(spheres, masses, labels, tree, moments=None, label_ranges=None):
    """The node moments of the gravity within groups (an extension the reference lacks): gravity_moments_sph's
    records taken over the labelled spheres only, and per inner node the range of the labels below it.
    labels: int32 [n_spheres] in the order of `spheres` (tree order), such as fof_labels_sph's labels or
    fof_groups_sph's group_of; a label >= 0 names a group, a label < 0 means "in no group": such a particle
    attracts nobody, as if it were absent, but keeps its index.  M, S and the tight box lo / hi are over
    the labelled spheres below the node (fp64 sums per leaf in ascending tree index, per node left +
    right; +inf / -inf where there are none); the spans cover every sphere; c = float(S / M), lo where
    M == 0.  label_ranges[i] = {smallest, largest label >= 0 below node i}, {INT32_MAX, -1} where there
    is none.  Where no label is negative the moments equal gravity_moments_sph's bit for bit.
    Returns (moments float32 [n_nodes, 12], label_ranges int32 [n_nodes, 2])."""
    masses = _gravity_masses(masses, spheres)
    labels = _gravity_labels(labels, len(masses), "labels", "n_spheres")
    n_nodes = tree.n_nodes
    if moments is None:
        moments = torch.empty((n_nodes, 12), dtype=torch.float32, device=spheres.device)
    if moments.dtype != torch.float32 or tuple(moments.shape) != (n_nodes, 12):
        raise ValueError("moments must be float32 of shape [%d, 12]" % n_nodes)
    if label_ranges is None:
        label_ranges = torch.empty((n_nodes, 2), dtype=torch.int32, device=spheres.device)
    if label_ranges.dtype != torch.int32 or tuple(label_ranges.shape) != (n_nodes, 2):
        raise ValueError("label_ranges must be int32 of shape [%d, 2]" % n_nodes)
    _check(_lib.grace_gravity_group_moments_f4(*_interp_scene(spheres, tree), _ptr(masses), _ptr(labels),
                                               _ptr(moments) if n_nodes else C.c_void_p(0),
                                               _ptr(label_ranges) if n_nodes else C.c_void_p(0), _stream()))
    return moments, label_ranges


def gravity_groups_sph(points, point_labels, spheres, masses, labels, tree, moments, label_ranges, theta=0.5,
                       eps=0.0, out=None, counts=None, check=False):
    """Gravity within groups (an extension the reference lacks): at every point the potential and the
    acceleration due to the spheres that carry the point's own label, in one walk of the whole-scene
    tree -- the binding energy of every member of every friends-of-friends group in one call.  The
    recursion of gravity_sph with labels: a point of label L >= 0 passes by an inner node whose label
    range does not hold L (no term, no count); a node whose range is the one label L and whose box has
    size2 < fl(theta^2 * d2min) contributes one term {c, M32}; any other node is opened, left child
    first -- a node that holds two or more labels is never a monopole; a leaf contributes one term per
    sphere j with labels[j] == L, ascending j.  Terms, rounding, the fp64 sums and their order are
    gravity_sph's (include/grace_hip.h states every step).  theta = 0 is the direct sum over the
    label's members in ascending tree index and does not depend on the tree; with one label >= 0 on
    every sphere and point the result equals gravity_sph's bit for bit.
    points: float32 [n, 3..16]; point_labels: int32 [n]; masses: float32 [n_spheres] and labels: int32
    [n_spheres] in tree order; moments, label_ranges: gravity_group_moments_sph(spheres, masses, labels,
    tree).  A point with a negative label or a non-finite coordinate gets zeros; a point whose label no
    sphere carries gets no term.  An unbinding pass: labels[unbound] = -1, the moments again, this call
    again.
    Returns (out float64 [n, 4] = {a_x, a_y, a_z, phi}, counts int32 [n, 2] = {node terms, particle
    terms} if counts is True or a tensor to fill, else None)."""
    if points.dtype != torch.float32 or points.dim() != 2 or not 3 <= points.shape[1] <= 16:
        raise ValueError("points must be float32 of shape [n, 3..16]")
    points = points.contiguous()
    masses = _gravity_masses(masses, spheres)
    n, n_nodes = len(points), tree.n_nodes
    labels = _gravity_labels(labels, len(masses), "labels", "n_spheres")
    point_labels = _gravity_labels(point_labels, n, "point_labels", "n_points")
    if n_nodes and (moments is None or moments.dtype != torch.float32 or tuple(moments.shape) != (n_nodes, 12)):
        raise ValueError("moments must be float32 of shape [%d, 12]" % n_nodes)
    if n_nodes and (label_ranges is None or label_ranges.dtype != torch.int32
                    or tuple(label_ranges.shape) != (n_nodes, 2)):
        raise ValueError("label_ranges must be int32 of shape [%d, 2]" % n_nodes)
    if out is None:
        out = torch.empty((n, 4), dtype=torch.float64, device=points.device)
    if out.dtype != torch.float64 or tuple(out.shape) != (n, 4):
        raise ValueError("out must be float64 of shape [%d, 4]" % n)
    if counts is True:
        counts = torch.empty((n, 2), dtype=torch.int32, device=points.device)
    if counts is not None and (counts.dtype != torch.int32 or tuple(counts.shape) != (n, 2)):
        raise ValueError("counts must be True or int32 of shape [%d, 2]" % n)
    _check(_lib.grace_gravity_group_points_f4(_ptr(points), C.c_size_t(n), C.c_int(points.shape[1]),
                                              *_interp_scene(spheres, tree), _ptr(masses), _ptr(labels),
                                              _ptr(moments) if n_nodes else C.c_void_p(0),
                                              _ptr(label_ranges) if n_nodes else C.c_void_p(0), _ptr(point_labels),
                                              C.c_float(float(theta)), C.c_float(float(eps)), _ptr(out),
                                              _ptr(counts), _stream()))
    if check:
        trace_status()
    return out, counts


def _offsets_from_counts(offsets, extra=0):
    """Hit counts -> exclusive offsets in place; returns the total (64-bit).  int offsets cannot
    address more than INT32_MAX per-hit slots: ValueError (std::invalid_argument in the C++
    mirrors) instead of the reference's silent wrap-around."""
    total = exclusive_scan(offsets, offsets)
    if total + extra > INT32_MAX:
        raise ValueError("trace_sph: %d hits (+ %d sentinels) exceed INT32_MAX; the int ray offsets "
                         "cannot address the per-hit arrays. Trace fewer rays per call." % (total, extra))
    return total


def trace_sph(rays, spheres, tree, real=torch.float32):
    """trace_sph.cuh:112-168: returns (ray_offsets, hit_indices, hit_integrals,
    hit_distances); the reference resizes the three per-hit vectors to the total.  real is the
    Real of the integrals and distances: float32, or float64 for trace_sph<float4, int, double>."""
    _check_rays(rays)
    real = _real_of(real)
    n = len(rays)
    offsets = torch.empty(n, dtype=torch.int32, device=rays.device)
    _trace_hitcounts_keep(rays, spheres, tree, offsets, real)
    total = _offsets_from_counts(offsets)
    idx = torch.empty(total, dtype=torch.int32, device=rays.device)
    integrals = torch.empty(total, dtype=real, device=rays.device)
    dists = torch.empty(total, dtype=real, device=rays.device)
    if total == 0:             # no ray hits anything: empty outputs, like the reference's resize(0)
        return offsets, idx, integrals, dists
    fn = _lib.grace_trace_hits_f4_f64 if real == torch.float64 else _lib.grace_trace_hits_f4
    _check(fn(*_trace_args(rays, spheres, tree), _ptr(offsets), _ptr(idx), _ptr(integrals), _ptr(dists),
              _stream()))
    trace_status()
    return offsets, idx, integrals, dists


def trace_with_sentinels_sph(rays, spheres, tree, index_sentinel, integral_sentinel,
                             distance_sentinel, real=torch.float32):
    """trace_sph.cuh:171-241: like trace_sph, but every ray's segment ends with one sentinel
    slot; returns (ray_offsets, hit_indices, hit_integrals, hit_distances).  real as for
    trace_sph."""
    _check_rays(rays)
    real = _real_of(real)
    n = len(rays)
    offsets = torch.empty(n, dtype=torch.int32, device=rays.device)
    _trace_hitcounts_keep(rays, spheres, tree, offsets, real)
    total = _offsets_from_counts(offsets, extra=n) + n
    _check(_lib.grace_add_iota_i32(_ptr(offsets), C.c_size_t(n), _stream()))
    idx = torch.empty(total, dtype=torch.int32, device=rays.device)
    _check(_lib.grace_fill_u32(_ptr(idx), C.c_size_t(total), C.c_uint32(index_sentinel & 0xFFFFFFFF), _stream()))
    if real == torch.float64:
        # (64-bit sentinels: a tensor fill)
        integrals = torch.full((total,), float(integral_sentinel), dtype=real, device=rays.device)
        dists = torch.full((total,), float(distance_sentinel), dtype=real, device=rays.device)
        fn = _lib.grace_trace_hits_f4_f64
    else:
        integrals = torch.empty(total, dtype=torch.float32, device=rays.device)
        dists = torch.empty(total, dtype=torch.float32, device=rays.device)
        bits = lambda f: int(np.float32(f).view(np.uint32))
        _check(_lib.grace_fill_u32(_ptr(integrals), C.c_size_t(total), C.c_uint32(bits(integral_sentinel)), _stream()))
        _check(_lib.grace_fill_u32(_ptr(dists), C.c_size_t(total), C.c_uint32(bits(distance_sentinel)), _stream()))
        fn = _lib.grace_trace_hits_f4
    _check(fn(*_trace_args(rays, spheres, tree), _ptr(offsets), _ptr(idx), _ptr(integrals), _ptr(dists),
              _stream()))
    trace_status()
    return offsets, idx, integrals, dists


def trace_stats(rays, spheres, tree):
    """Per ray {nodes, leaves, spheres tested, hits} for that ray alone."""
    stats = torch.empty((len(rays), 4), dtype=torch.int32, device=rays.device)
    _check(_lib.grace_trace_stats_f4(*_trace_args(rays, spheres, tree), _ptr(stats), _stream()))
    return stats


# ---------------------------------------------------------------------------------------
# Triangles -- tests/profile_trace_triangle/{tris_tree.cuh,tris_trace.cu}
# ---------------------------------------------------------------------------------------
def _tris(t):
    assert t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == 9 and t.is_contiguous()
    return t


def build_tree_tris(tris, tree):
    """tris_tree.cuh:17-30: centroid bounds, 30-bit keys, stable sort of the triangles, XOR
    deltas, ALBVH with TriangleAABB.  Sorts tris in place; returns (bots, tops)."""
    n = len(_tris(tris))
    bot = (C.c_float * 3)(); top = (C.c_float * 3)()
    _check(_lib.grace_centroid_bounds_tri(_ptr(tris), C.c_size_t(n), bot, top, _stream()))
    keys = torch.empty(n, dtype=torch.int32, device=tris.device)
    _check(_lib.grace_morton_keys30_tri(_ptr(tris), C.c_size_t(n), bot, top, _ptr(keys), _stream()))
    sort_by_key(keys, tris, 0, 30)
    deltas = torch.empty(n + 1, dtype=torch.int32, device=tris.device)
    XOR_deltas_sph(keys, deltas)
    n_leaves = C.c_size_t(0)
    _check(_lib.grace_albvh_build_tri_u32(_ptr(tris), C.c_size_t(n), _ptr(deltas),
                                          C.c_int(tree.max_per_leaf), _ptr(tree.nodes),
                                          _ptr(tree.leaves), _ptr(tree.root_index),
                                          C.byref(n_leaves), _stream()))
    tree.leaves = tree.leaves[: n_leaves.value]
    tree.nodes = tree.nodes[: n_leaves.value - 1]
    return np.array(bot, np.float32), np.array(top, np.float32)


def trace_closest_tri(rays, tris, tree, closest):
    """tris_trace.cu:43-62."""
    _check_rays(rays)
    assert closest.dtype == torch.int32 and len(closest) == len(rays)
    _check(_lib.grace_trace_closest_tri(_ptr(rays), C.c_size_t(len(rays)), _ptr(_tris(tris)),
                                        C.c_size_t(len(tris)), _ptr(tree.nodes),
                                        C.c_size_t(tree.n_nodes), _ptr(tree.leaves),
                                        _ptr(tree.root_index), _ptr(closest), _stream()))
    trace_status()
    return closest


def pinhole_camera_rays(res_x, res_y, camera, look_at, view_up, fovy, length, device="cuda"):
    rays = torch.empty((res_x * res_y, RAY_FLOATS), dtype=torch.float32, device=device)
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    _check(_lib.grace_rays_pinhole(C.c_int(res_x), C.c_int(res_y), f3(camera), f3(look_at),
                                   f3(view_up), C.c_float(fovy), C.c_float(length), _ptr(rays),
                                   _stream()))
    return rays


# ---------------------------------------------------------------------------------------
# Scans -- include/grace/cuda/scan.cuh
# ---------------------------------------------------------------------------------------
def exclusive_scan(inp, out):
    total = C.c_longlong(0)
    _check(_lib.grace_scan_exclusive_i32(_ptr(inp), C.c_size_t(len(inp)), _ptr(out),
                                         C.byref(total), _stream()))
    return total.value


def exclusive_segmented_scan(segment_offsets, data, results):
    """scan.cuh:15-37; data and results may be the same tensor."""
    assert segment_offsets.dtype == torch.int32 and data.dtype == results.dtype
    fn = {torch.float32: _lib.grace_segscan_exclusive_f32,
          torch.float64: _lib.grace_segscan_exclusive_f64}[data.dtype]
    _check(fn(_ptr(segment_offsets), C.c_size_t(len(segment_offsets)), _ptr(data),
              C.c_size_t(len(data)), _ptr(results), _stream()))
    return results


def sort_by_distance(hit_distances, ray_offsets, hit_indices, hit_data):
    """sort.cuh:100-131: per-ray sort by distance; indices and data follow."""
    fn = _lib.grace_sort_by_distance_f64 if hit_distances.dtype == torch.float64 \
        else _lib.grace_sort_by_distance_f32
    assert hit_data is None or hit_data.dtype == hit_distances.dtype
    _check(fn(_ptr(hit_distances), _ptr(ray_offsets), C.c_size_t(len(ray_offsets)),
              C.c_size_t(len(hit_distances)), _ptr(hit_indices), _ptr(hit_data), _stream()))


def weighted_exclusive_segmented_scan(to_sum, weights, weight_map, segment_offsets, out):
    """scan.cuh:43-58."""
    weighted = torch.empty_like(to_sum)
    fn = _lib.grace_multiply_by_weights_f64 if to_sum.dtype == torch.float64 else _lib.grace_multiply_by_weights_f32
    _check(fn(_ptr(to_sum), C.c_size_t(len(to_sum)),
              _ptr(weights), _ptr(weight_map), _ptr(weighted), _stream()))
    return exclusive_segmented_scan(segment_offsets, weighted, out)


# ---------------------------------------------------------------------------------------
# Rays -- tests/helper/rays.cuh, include/grace/cuda/gen_rays.cuh
# ---------------------------------------------------------------------------------------
def orthogonal_rays_z(n_side, mins4, maxs4, device="cuda"):
    """tests/helper/rays.cuh:55-79; returns (rays [n_side^2, 7], area per ray)."""
    rays = torch.empty((n_side * n_side, RAY_FLOATS), dtype=torch.float32, device=device)
    lo = (C.c_float * 4)(*[float(x) for x in mins4]); hi = (C.c_float * 4)(*[float(x) for x in maxs4])
    area = C.c_float(0)
    _check(_lib.grace_rays_orthogonal_z(C.c_int(n_side), lo, hi, _ptr(rays), C.byref(area),
                                        _stream()))
    return rays, area.value


def healpix_rays(nside, origin, length, device="cuda"):
    rays = torch.empty((12 * nside * nside, RAY_FLOATS), dtype=torch.float32, device=device)
    _check(_lib.grace_rays_healpix(C.c_int(nside), C.c_float(origin[0]), C.c_float(origin[1]),
                                   C.c_float(origin[2]), C.c_float(length), _ptr(rays), _stream()))
    return rays


def uniform_random_rays(n_rays, origin, length, seed=1234, device="cuda"):
    """gen_rays.cuh uniform_random_rays: isotropic directions, direction-Morton sorted."""
    rays = torch.empty((n_rays, RAY_FLOATS), dtype=torch.float32, device=device)
    _check(_lib.grace_rays_isotropic(C.c_size_t(n_rays), C.c_float(origin[0]),
                                     C.c_float(origin[1]), C.c_float(origin[2]),
                                     C.c_float(length), C.c_uint64(seed), _ptr(rays), _stream()))
    return rays


# enum Octants / enum RaySortType, grace/types.h:36-51
PPP, PPM, PMP, PMM, MPP, MPM, MMP, MMM = 7, 6, 5, 4, 3, 2, 1, 0
NoSort, DirectionSort, EndPointSort = 0, 1, 2


def uniform_random_rays_single_octant(n_rays, origin, length, octant=PPP, seed=1234, device="cuda"):
    """gen_rays.cuh:62-97: isotropic directions confined to one octant, direction-sorted."""
    rays = torch.empty((n_rays, RAY_FLOATS), dtype=torch.float32, device=device)
    _check(_lib.grace_rays_isotropic_octant(C.c_size_t(n_rays), C.c_float(origin[0]),
                                            C.c_float(origin[1]), C.c_float(origin[2]),
                                            C.c_float(length), C.c_int(int(octant)),
                                            C.c_uint64(seed), _ptr(rays), _stream()))
    return rays


def _points(points):
    assert points.is_contiguous() and points.dim() == 2 and 3 <= points.shape[1] <= 16
    assert points.dtype in (torch.float32, torch.float64)
    return C.c_int(1 if points.dtype == torch.float64 else 0), C.c_int(points.shape[1])


def one_to_many_rays(origin, points, sort_type=DirectionSort, bot=None, top=None):
    """gen_rays.cuh:99-208: one ray from `origin` to each point ([n, 3..] float32/float64).
    EndPointSort needs the points' bounds (computed here when not given -- the reference's
    bounds-free overload passes AABB_bot twice, which is not reproduced)."""
    isd, k = _points(points)
    rays = torch.empty((len(points), RAY_FLOATS), dtype=torch.float32, device=points.device)
    b = t = None
    if sort_type == EndPointSort:
        if bot is None:
            bot = points[:, :3].min(dim=0).values.float().tolist()
            top = points[:, :3].max(dim=0).values.float().tolist()
        b = (C.c_float * 3)(*[float(x) for x in bot]); t = (C.c_float * 3)(*[float(x) for x in top])
    _check(_lib.grace_rays_one_to_many(C.c_size_t(len(points)), C.c_float(origin[0]),
                                       C.c_float(origin[1]), C.c_float(origin[2]), _ptr(points),
                                       isd, k, C.c_int(int(sort_type)), b, t, _ptr(rays), _stream()))
    return rays


def plane_parallel_random_rays(width, height, base, w, h, length, seed=1234, device="cuda"):
    """gen_rays.cuh:210-262: one ray per cell of the width x height grid spanned by w, h."""
    rays = torch.empty((width * height, RAY_FLOATS), dtype=torch.float32, device=device)
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    _check(_lib.grace_rays_plane_parallel_random(C.c_int(width), C.c_int(height), f3(base), f3(w),
                                                 f3(h), C.c_float(length), C.c_uint64(seed),
                                                 _ptr(rays), _stream()))
    return rays


def orthographic_projection_rays(res_x, res_y, camera, look_at, view_up, vertical_extent, length,
                                 device="cuda"):
    """gen_rays.cuh:264-329."""
    rays = torch.empty((res_x * res_y, RAY_FLOATS), dtype=torch.float32, device=device)
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])
    _check(_lib.grace_rays_orthographic_projection(C.c_int(res_x), C.c_int(res_y), f3(camera),
                                                   f3(look_at), f3(view_up),
                                                   C.c_float(vertical_extent), C.c_float(length),
                                                   _ptr(rays), _stream()))
    return rays


def morton_keys_points(points, keys, bot, top):
    """morton_keys over float3/float4/double3/double4 points (build_sph.cuh:16-33 with
    Real4 = double4; tests/morton_key_kernel/63bit_keys.cu): co-ordinates narrowed to float
    first.  keys.dtype int32 -> 30-bit, int64 -> 63-bit."""
    isd, k = _points(points)
    b = (C.c_float * 3)(*[float(x) for x in bot]); t = (C.c_float * 3)(*[float(x) for x in top])
    fn = _lib.grace_morton_keys30_points if keys.dtype == torch.int32 else _lib.grace_morton_keys63_points
    _check(fn(_ptr(points), C.c_size_t(len(points)), isd, k, b, t, _ptr(keys), _stream()))
    return keys


# ---------------------------------------------------------------------------------------
# double4 spheres (Real4 = double4, Real = double)
# ---------------------------------------------------------------------------------------
def _spheres_d4(s):
    assert s.is_cuda and s.is_contiguous() and s.dtype == torch.float64 and s.dim() == 2 and s.shape[1] == 4


def build_tree_d4(spheres, tree, bot, top):
    """tests/helper/tree.cuh build_tree with double4 spheres: 30-bit keys of the float-narrowed
    centres, sort of the 32-byte records, Euclidean deltas (formed in double, stored as float),
    ALBVH.  Sorts `spheres` in place."""
    _spheres_d4(spheres)
    n = len(spheres)
    keys = torch.empty(n, dtype=torch.int32, device=spheres.device)
    morton_keys_points(spheres, keys, bot, top)
    sort_by_key(keys, spheres, 0, 30)
    deltas = torch.empty(n + 1, dtype=torch.float32, device=spheres.device)
    _check(_lib.grace_deltas_euclid_d4(_ptr(spheres), C.c_size_t(n), _ptr(deltas), _stream()))
    n_leaves = C.c_size_t(0)
    _check(_lib.grace_albvh_build_d4(_ptr(spheres), C.c_size_t(n), _ptr(deltas),
                                     C.c_int(tree.max_per_leaf), _ptr(tree.nodes), _ptr(tree.leaves),
                                     _ptr(tree.root_index), C.byref(n_leaves), _stream()))
    tree.leaves = tree.leaves[: n_leaves.value]
    tree.nodes = tree.nodes[: n_leaves.value - 1]
    return deltas


def _trace_args_d4(rays, spheres, tree):
    _check_rays(rays); _spheres_d4(spheres)
    return (_ptr(rays), C.c_size_t(len(rays)), _ptr(spheres), C.c_size_t(len(spheres)),
            _ptr(tree.nodes), C.c_size_t(tree.n_leaves - 1), _ptr(tree.leaves), _ptr(tree.root_index))


def trace_hitcounts_d4(rays, spheres, tree, counts):
    _check(_lib.grace_trace_hitcounts_d4(*_trace_args_d4(rays, spheres, tree), _ptr(counts), _stream()))
    _check(_lib.grace_trace_status_d4(_stream()))
    return counts


def trace_cumulative_d4(rays, spheres, tree, sums):
    assert sums.dtype == torch.float64
    _check(_lib.grace_trace_cumulative_d4(*_trace_args_d4(rays, spheres, tree), _ptr(sums), _stream()))
    _check(_lib.grace_trace_status_d4(_stream()))
    return sums


def surface_area_deltas_d4(spheres, deltas):
    """surface_area_deltas_sph<double4> (build_sph.cuh:97-105); deltas float32 or float64."""
    _spheres_d4(spheres)
    fn = _lib.grace_deltas_area_d4_f64 if deltas.dtype == torch.float64 else _lib.grace_deltas_area_d4
    _check(fn(_ptr(spheres), C.c_size_t(len(spheres)), _ptr(deltas), _stream()))
    return deltas


def euclidean_deltas_d4(spheres, deltas):
    _spheres_d4(spheres)
    fn = _lib.grace_deltas_euclid_d4_f64 if deltas.dtype == torch.float64 else _lib.grace_deltas_euclid_d4
    _check(fn(_ptr(spheres), C.c_size_t(len(spheres)), _ptr(deltas), _stream()))
    return deltas


def ALBVH_d4(spheres, deltas, tree):
    """ALBVH_sph<double4, DeltaType> for float / double / 32- / 64-bit XOR deltas."""
    _spheres_d4(spheres)
    fn = {torch.float32: _lib.grace_albvh_build_d4, torch.float64: _lib.grace_albvh_build_d4_f64,
          torch.int32: _lib.grace_albvh_build_d4_u32, torch.int64: _lib.grace_albvh_build_d4_u64}[deltas.dtype]
    n_leaves = C.c_size_t(0)
    _check(fn(_ptr(spheres), C.c_size_t(len(spheres)), _ptr(deltas), C.c_int(tree.max_per_leaf),
              _ptr(tree.nodes), _ptr(tree.leaves), _ptr(tree.root_index), C.byref(n_leaves), _stream()))
    tree.leaves = tree.leaves[: n_leaves.value]
    tree.nodes = tree.nodes[: n_leaves.value - 1]
    return tree


def trace_sph_d4(rays, spheres, tree):
    """trace_sph<double4, int, double> (trace_sph.cuh:112-168): (ray_offsets, hit_indices,
    hit_integrals float64, hit_distances float64)."""
    n = len(rays)
    offsets = torch.empty(n, dtype=torch.int32, device=rays.device)
    trace_hitcounts_d4(rays, spheres, tree, offsets)
    total = _offsets_from_counts(offsets)
    idx = torch.empty(total, dtype=torch.int32, device=rays.device)
    integrals = torch.empty(total, dtype=torch.float64, device=rays.device)
    dists = torch.empty(total, dtype=torch.float64, device=rays.device)
    if total:
        _check(_lib.grace_trace_hits_d4(*_trace_args_d4(rays, spheres, tree), _ptr(offsets), _ptr(idx),
                                        _ptr(integrals), _ptr(dists), _stream()))
        trace_status()
    return offsets, idx, integrals, dists


# ---------------------------------------------------------------------------------------
# Periodic boxes for traces (an extension the reference lacks): include/grace_hip.h,
# "Periodic boxes for traces", has the definition.  The periodic trace IS the open trace of the
# rays' segments over the spheres' images, folded back per ray.
# ---------------------------------------------------------------------------------------
def _box(lo, period):
    """(lo, period) of a periodic box -> two arrays of three host floats (the library checks them)."""
    period = _period(period)
    if torch.is_tensor(lo):
        lo = lo.detach().cpu().numpy()
    lo = np.ascontiguousarray(np.asarray(lo, dtype=np.float32).reshape(-1))
    if len(lo) != 3:
        raise ValueError("lo must hold three values, the box origin")
    return lo, period


def _box_args(lo, period):
    return lo.ctypes.data_as(C.c_void_p), period.ctypes.data_as(C.c_void_p)


def _checked_total(offsets, what):
    total = exclusive_scan(offsets, offsets)
    if total > INT32_MAX:
        raise ValueError("%s: %d entries exceed INT32_MAX; the int offsets cannot address them. "
                         "Split the input into several calls." % (what, total))
    return total


def periodic_sphere_images(spheres, lo, period):
    """The images of float4 spheres in a periodic box: a sphere that sticks out of a face of a periodic
    axis is emitted again one period further on, for every subset of the faces it crosses (1, 2, 4 or 8
    copies, the sphere itself first).  Counts, the library's scan, then the fill; synchronises to read
    the total (ValueError above INT32_MAX, before any fill).  A centre outside the box or H above half a
    period sets the status word (trace_status() raises ValueError) and the sphere is emitted once.
    Returns (images float32 [total, 4], source int32 [total], offsets int32 [n + 1]); spheres is not
    modified."""
    _spheres(spheres)
    lo, period = _box(lo, period)
    n = len(spheres)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=spheres.device)
    _check(_lib.grace_periodic_image_counts_f4(_ptr(spheres), C.c_size_t(n), *_box_args(lo, period),
                                               _ptr(offsets), _stream()))
    total = _checked_total(offsets, "periodic_sphere_images") if n else 0
    images = torch.empty((total, 4), dtype=torch.float32, device=spheres.device)
    source = torch.empty(total, dtype=torch.int32, device=spheres.device)
    if total:
        _check(_lib.grace_periodic_images_f4(_ptr(spheres), C.c_size_t(n), *_box_args(lo, period),
                                             _ptr(offsets), _ptr(images), _ptr(source), _stream()))
    return images, source, offsets


def periodic_ray_segments(rays, lo, period, want_t0=False):
    """The segments of rays in a periodic box: every ray cut where it crosses a face of the lattice of
    boxes, every piece moved back into the box (fp64 arithmetic as stated in include/grace_hip.h).  Any
    number of rays.  A ray with more than 65536 segments sets the status word and is emitted as itself.
    Returns (segments float32 [total, 7], offsets int32 [n_rays + 1]): ray r's segments are rows
    [offsets[r], offsets[r + 1]), in order along the ray.  want_t0: a third value, float64 [total], every
    segment's starting parameter along its ray (0 for a ray emitted as itself), from the same walk as the
    segments.  Synchronises to read the total (ValueError above INT32_MAX, before any fill)."""
    _rays(rays)
    lo, period = _box(lo, period)
    n = len(rays)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=rays.device)
    _check(_lib.grace_periodic_segment_counts(_ptr(rays), C.c_size_t(n), *_box_args(lo, period),
                                              _ptr(offsets), _stream()))
    total = _checked_total(offsets, "periodic_ray_segments") if n else 0
    segments = torch.empty((total, RAY_FLOATS), dtype=torch.float32, device=rays.device)
    if total:
        _check(_lib.grace_periodic_segments(_ptr(rays), C.c_size_t(n), *_box_args(lo, period),
                                            _ptr(offsets), _ptr(segments), _stream()))
    if not want_t0:
        return segments, offsets
    t0 = torch.empty(total, dtype=torch.float64, device=rays.device)
    if total:
        _check(_lib.grace_periodic_segment_starts(_ptr(rays), C.c_size_t(n), *_box_args(lo, period),
                                                  _ptr(offsets), _ptr(t0), _stream()))
    return segments, offsets, t0


class PeriodicScene:
    """What periodic_scene returns: spheres (the images, in tree order), source (int32 per image: the
    index of its sphere in the caller's array as passed), tree, lo and period (host float32 [3]), and
    n_sources, the number of spheres in the caller's array."""

    def __init__(self, spheres, source, tree, lo, period, n_sources=None):
        self.spheres, self.source, self.tree, self.lo, self.period = spheres, source, tree, lo, period
        self.n_sources = n_sources


def periodic_scene(spheres, lo, period, max_per_leaf=32, check=True):
    """The scene of the periodic traces: the images of `spheres` (periodic_sphere_images) and their tree
    (build_tree's steps: 30-bit keys, Euclidean deltas, ALBVH), the images' source indices carried
    through the same stable sort as a payload of their own.  spheres is not modified.  check=True reads
    the status word (a sphere outside the box or with H above half a period: ValueError)."""
    images, source, _ = periodic_sphere_images(spheres, lo, period)
    if check:
        trace_status()
    lo, period = _box(lo, period)
    tree = Tree(len(images), max_per_leaf, device=images.device)
    if len(images):
        keys = torch.empty(len(images), dtype=torch.int32, device=images.device)
        morton_keys_sph(images, keys)
        source_keys = keys.clone()
        sort_by_key(source_keys, source, 0, 30)
        sort_by_key(keys, images, 0, 30)
        deltas = torch.empty(len(images) + 1, dtype=torch.float32, device=images.device)
        euclidean_deltas_sph(images, deltas)
        ALBVH_sph(images, deltas, tree)
    return PeriodicScene(images, source, tree, lo, period, len(spheres))


def _periodic_trace(rays, scene, n_ch, dtype, out, shape, trace):
    """Segments, the open trace `trace(args, per-segment output)`, then the fold into out."""
    _rays(rays)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=rays.device)
    if out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("out must be contiguous %s of shape %s" % (dtype, shape))
    if len(rays) == 0:
        return out
    segments, offsets = periodic_ray_segments(rays, scene.lo, scene.period)
    per_segment = torch.empty((len(segments), n_ch), dtype=dtype, device=rays.device)
    trace(_trace_args(segments, scene.spheres, scene.tree), per_segment)
    fold = _lib.grace_periodic_fold_i32 if dtype == torch.int32 else _lib.grace_periodic_fold_f32
    _check(fold(_ptr(per_segment), _ptr(offsets), C.c_size_t(len(rays)), C.c_int(n_ch), _ptr(out), _stream()))
    return out


def trace_hitcounts_periodic_sph(rays, scene, out=None, check=False):
    """trace_hitcounts_sph in a periodic box: out[r] = the number of lattice images of the scene's
    spheres that ray r hits = the sum of the open hit counts of its segments over scene.spheres.  Any
    number of rays.  scene: periodic_scene(...)."""
    out = _periodic_trace(rays, scene, 1, torch.int32, out, (len(rays),), lambda a, o: _check(
        _lib.grace_trace_hitcounts_f4(*a, _ptr(o), _stream())))
    if check:
        trace_status()
    return out


def trace_cumulative_periodic_sph(rays, scene, out=None, check=False):
    """trace_cumulative_sph in a periodic box: out[r] = the fp32 running sum, from 0 and in order along
    the ray, of the open column densities of ray r's segments over scene.spheres."""
    out = _periodic_trace(rays, scene, 1, torch.float32, out, (len(rays),), lambda a, o: _check(
        _lib.grace_trace_cumulative_f4(*a, _ptr(o), _stream())))
    if check:
        trace_status()
    return out


def trace_cumulative_weighted_periodic_sph(rays, scene, weights, out=None, check=False):
    """trace_cumulative_weighted_sph in a periodic box.  weights: float32 [n] or [n, C] (1 <= C <= 64) per
    CALLER particle, in the order of the array given to periodic_scene: an image carries the weight row
    of its source.  out: float32 [n_rays] or [n_rays, C]."""
    if weights.dtype != torch.float32 or weights.dim() not in (1, 2):
        raise ValueError("weights must be float32 of shape [n] or [n, C]")
    n_ch = 1 if weights.dim() == 1 else weights.shape[1]
    if not 1 <= n_ch <= 64:
        raise ValueError("weights must have 1..64 channels")
    n_img = len(scene.spheres)
    if n_img and (len(weights) == 0 or int(scene.source.max()) >= len(weights)):
        raise ValueError("weights must hold one row per sphere given to periodic_scene")
    weights = weights.contiguous()
    image_weights = torch.empty((n_img, n_ch), dtype=torch.float32, device=weights.device)
    _check(_lib.grace_periodic_gather_rows_f32(_ptr(weights), _ptr(scene.source), C.c_size_t(n_img),
                                               C.c_int(n_ch), _ptr(image_weights), _stream()))
    shape = (len(rays),) if weights.dim() == 1 else (len(rays), n_ch)
    out = _periodic_trace(rays, scene, n_ch, torch.float32, out, shape, lambda a, o: _check(
        _lib.grace_trace_cumulative_weighted_f4(*a, _ptr(image_weights), C.c_int(n_ch), _ptr(o), _stream())))
    if check:
        trace_status()
    return out


# The depth-ordered traces in a periodic box (include/grace_hip.h, "Periodic boxes for traces", "Ordered
# traces").  No fold defines them: they are the open call's composite applied per ray to the hits of all
# the ray's segments over the scene's images, ordered by (segment along the ray, fp32 distance within the
# segment, image index), every hit standing for its source -- the caller's particle.
def _periodic_ordered_args(rays, scene, want_t0=False):
    """The arguments every periodic ordered entry point starts with; the tensors they point into."""
    _rays(rays)
    n_sources = scene.n_sources
    if n_sources is None:
        raise ValueError("the scene must come from periodic_scene (it carries n_sources)")
    keep = periodic_ray_segments(rays, scene.lo, scene.period, want_t0)
    segments, offsets = keep[0], keep[1]
    args = _trace_args(segments, scene.spheres, scene.tree) + (
        _ptr(offsets), C.c_size_t(len(rays)), _ptr(scene.source), C.c_size_t(n_sources))
    if want_t0:
        args += (_ptr(keep[2]),)
    return args, keep


def _per_ray_out(out, shape, dtype, device, what):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError("%s must be contiguous %s of shape %s" % (what, dtype, tuple(shape)))
    return out


def trace_emission_absorption_periodic_sph(rays, scene, emission, absorption, out=None, tau=None, check=False):
    """trace_emission_absorption_sph in a periodic box.  A ray's hit list is that of all its segments
    (periodic_ray_segments) over scene.spheres, ordered by (segment along the ray, fp32 distance within
    the segment, image index); hit k stands for the particle i_k = scene.source[image]; then, in fp64 and
    as in the open call, out[r, c] = sum_k emission[i_k, c] I_k phi(a_k) exp(-tau_k), a_k =
    absorption[i_k] I_k, tau[r] = sum_k a_k, over the ray's whole list.  A ray longer than a period
    meets a particle once per lattice image.  emission: float32 [n] or [n, C] (1 <= C <= 64),
    absorption: float32 [n], per CALLER particle in the order of the array given to periodic_scene.
    Any number of rays.  With open axes, or a box nothing crosses, the open call bit for bit."""
    if emission.dtype != torch.float32 or absorption.dtype != torch.float32:
        raise ValueError("emission and absorption must be float32")
    n = scene.n_sources
    if emission.dim() not in (1, 2) or emission.shape[0] != n:
        raise ValueError("emission must have shape [n] or [n, C], one row per sphere given to periodic_scene")
    if tuple(absorption.shape) != (n,):
        raise ValueError("absorption must have shape [n], one value per sphere given to periodic_scene")
    n_ch = 1 if emission.dim() == 1 else emission.shape[1]
    if not 1 <= n_ch <= 64:
        raise ValueError("emission must have 1..64 channels")
    shape = (len(rays),) if emission.dim() == 1 else (len(rays), n_ch)
    out = _per_ray_out(out, shape, torch.float32, rays.device, "out")
    if tau is not None:
        _per_ray_out(tau, (len(rays),), torch.float32, rays.device, "tau")
    if len(rays) == 0:
        return out
    emission, absorption = emission.contiguous(), absorption.contiguous()
    args, keep = _periodic_ordered_args(rays, scene)
    _check(_lib.grace_trace_emission_absorption_periodic_f4(*args, _ptr(emission), C.c_int(n_ch), _ptr(absorption),
                                                            _ptr(out), _ptr(tau), _stream()))
    if check:
        trace_status()
    return out


def trace_absorption_deposit_periodic_sph(rays, scene, luminosity, absorption, deposit=None, transmitted=None,
                                          quantum=None, check=False):
    """trace_absorption_deposit_sph in a periodic box: the hit list and its order as in
    trace_emission_absorption_periodic_sph; ray r's luminosity[r, c] is absorbed hit by hit along ALL its
    segments (a segment starts with what its predecessor left), deposit[i, c] sums what particle i
    absorbs through any of its images, from all rays, and transmitted[r, c] is what is left at the ray's
    end.  The quantum's n_rays is the number of rays, not of segments, so deposit stays bit-identical for
    any order of the rays.  luminosity: float32 [n_rays] or [n_rays, C]; absorption: float32 [n] or
    [n, C] and deposit: float64 [n] or [n, C], per CALLER particle in the order of the array given to
    periodic_scene.  Any number of rays."""
    _rays(rays)
    if luminosity.dtype != torch.float32 or absorption.dtype != torch.float32:
        raise ValueError("luminosity and absorption must be float32")
    if luminosity.dim() not in (1, 2) or luminosity.shape[0] != len(rays):
        raise ValueError("luminosity must have shape [n_rays] or [n_rays, C]")
    n_ch = 1 if luminosity.dim() == 1 else luminosity.shape[1]
    if not 1 <= n_ch <= 64:
        raise ValueError("luminosity must have 1..64 channels")
    n = scene.n_sources
    shape = (n,) if luminosity.dim() == 1 else (n, n_ch)
    if tuple(absorption.shape) != shape:
        raise ValueError("absorption must be float32 of shape %s, one row per sphere given to periodic_scene" % (shape,))
    deposit = _per_ray_out(deposit, shape, torch.float64, rays.device, "deposit")
    if transmitted is not None:
        _per_ray_out(transmitted, tuple(luminosity.shape), torch.float32, rays.device, "transmitted")
    if quantum is not None:
        _per_ray_out(quantum, (n_ch,), torch.float64, rays.device, "quantum")
    luminosity, absorption = luminosity.contiguous(), absorption.contiguous()
    if len(rays) == 0:
        deposit.zero_()
        if quantum is not None:
            quantum.zero_()
        return deposit
    args, keep = _periodic_ordered_args(rays, scene)
    _check(_lib.grace_trace_absorption_deposit_periodic_f4(*args, _ptr(luminosity), _ptr(absorption), C.c_int(n_ch),
                                                           _ptr(deposit), _ptr(transmitted), _ptr(quantum),
                                                           _stream()))
    if check:
        trace_status()
    return deposit


def trace_spectra_periodic_sph(rays, scene, amount, width, velocity, v0, dv, n_bins, periodic=False, hubble=0.0,
                               tau=None, column=None, check=False):
    """trace_spectra_sph in a periodic box (a sightline through a cosmological snapshot, starting
    anywhere and as long as wanted): the hit list and its order as in
    trace_emission_absorption_periodic_sph; hit k's distance from the RAY's origin is d_k = t0 + d in
    fp64 -- t0 its segment's starting parameter (periodic_ray_segments(..., want_t0=True)), d its fp32
    distance within the segment -- and v_k = hubble d_k + velocity[i_k] . direction; the rest is the open
    call's.  amount, width: float32 [n] or [n, C] (1 <= C <= 16), velocity: float32 [n, 3], per CALLER
    particle in the order of the array given to periodic_scene.  `periodic` is the VELOCITY grid's, as
    in the open call.  Any number of rays.  Returns tau, float32 [n_rays, C, n_bins]."""
    if amount.dtype != torch.float32 or width.dtype != torch.float32 or velocity.dtype != torch.float32:
        raise ValueError("amount, width and velocity must be float32")
    n = scene.n_sources
    if amount.dim() not in (1, 2) or amount.shape[0] != n:
        raise ValueError("amount must have shape [n] or [n, C], one row per sphere given to periodic_scene")
    n_ch = 1 if amount.dim() == 1 else amount.shape[1]
    if not 1 <= n_ch <= 16:
        raise ValueError("amount must have 1..16 channels")
    if tuple(width.shape) != tuple(amount.shape):
        raise ValueError("width must be float32 of shape %s" % (tuple(amount.shape),))
    if tuple(velocity.shape) != (n, 3):
        raise ValueError("velocity must be float32 of shape [n, 3], one row per sphere given to periodic_scene")
    n_bins = int(n_bins)
    if not 1 <= n_bins <= 4096:
        raise ValueError("n_bins must be 1..4096")
    tau = _per_ray_out(tau, (len(rays), n_ch, n_bins), torch.float32, rays.device, "tau")
    if column is not None:
        _per_ray_out(column, (len(rays), n_ch), torch.float32, rays.device, "column")
    if len(rays) == 0:
        return tau
    amount, width, velocity = amount.contiguous(), width.contiguous(), velocity.contiguous()
    grid = _SpectrumGrid(float(v0), float(dv), n_bins, 1 if periodic else 0, float(hubble))
    args, keep = _periodic_ordered_args(rays, scene, want_t0=True)
    _check(_lib.grace_trace_spectra_periodic_f4(*args, _ptr(amount), _ptr(width), _ptr(velocity), C.c_int(n_ch),
                                                C.byref(grid), _ptr(tau), _ptr(column), _stream()))
    if check:
        trace_status()
    return tau


def _project_periodic_sph(spheres, n_side, max_per_leaf, period, lo):
    lo, period = _box(lo if lo is not None else (0.0, 0.0, 0.0), period)
    if not (period[0] > 0 and period[0] == period[1]):
        raise ValueError("project_sph: a periodic map needs Lx == Ly > 0 (square pixels over the box face); "
                         "for other boxes make the rays yourself and use periodic_scene")
    scene = periodic_scene(spheres, lo, period, max_per_leaf)
    top = (lo + period).astype(np.float32)
    if period[2] > 0:
        z_top, length = top[2], period[2]
    else:                                  # z open: the spheres' own extent
        smin, smax = min_max_vec4(spheres)
        z_top = np.float32(smax[2] + smax[3])
        length = np.float32(z_top - (smin[2] - smax[3]))
    camera = (np.float32((lo[0] + top[0]) / 2.), np.float32((lo[1] + top[1]) / 2.), z_top)
    rays = orthographic_projection_rays(n_side, n_side, camera, (camera[0], camera[1], z_top - length),
                                        (0.0, 1.0, 0.0), period[1], length, device=spheres.device)
    out = trace_cumulative_periodic_sph(rays, scene)
    return out.view(n_side, n_side), scene, rays


def project_sph(spheres, n_side, max_per_leaf=32, period=None, lo=None):
    """The projection of tests/project_gadget/project_gadget.cu:58-81: bounds with
    w = 0, build_tree, orthogonal_rays_z, trace_cumulative_sph.  Sorts spheres in place.
    Returns (image [n_side, n_side] float32, tree, rays).
    period=(Lx, Ly, Lz) (lo: the box origin, default 0): the map of a periodic box instead -- the
    frame is the box's z face [lo, lo + L] in x and y (Lx == Ly), the rays look down -z from the top
    face and span one period (Lz == 0: the spheres' extent), and what sticks in through the four
    side faces is included (periodic_scene, trace_cumulative_periodic_sph).  spheres is NOT modified;
    returns (image, scene, rays)."""
    if period is not None:
        return _project_periodic_sph(spheres, n_side, max_per_leaf, period, lo)
    lo, hi = min_max_vec4(spheres)
    lo[3] = 0.0; hi[3] = 0.0
    tree = Tree(len(spheres), max_per_leaf, device=spheres.device)
    build_tree(spheres, tree, lo[:3], hi[:3])
    rays, _ = orthogonal_rays_z(n_side, lo, hi, device=spheres.device)
    out = torch.empty(len(rays), dtype=torch.float32, device=spheres.device)
    trace_cumulative_sph(rays, spheres, tree, out)
    return out.view(n_side, n_side), tree, rays
