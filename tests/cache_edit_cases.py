"""Scenes, ray batches and one-word edits for the tests of the cached trace records.

A context caches the scene records (A, B1 / B50, T64, node_prims, the cluster and group boxes C)
and the ray order (perm, the 16-word extents) of the arrays it was last given, and validates them
before every use by a 128-bit signature of the caller's arrays (include/grace_hip.h, "Cached trace
records": results are always those of a fresh derivation).  The edits here change ONE OR TWO 32-bit
words of one array, in place, at the positions where the signature pass takes another path: the
last chunk of a grid-stride iteration and the first of the next, the last (partial) chunk, the third
array of the scene group, an array whose base is not 16-byte aligned.

A plain helper module (no GPU, no torch): tests/test_cache_edits.py makes the edits on the device,
tests/test_cache_edit_cases.py checks on the CPU that every edit sits in the chunk it is said to sit
in, keeps the tree valid and changes the answer of enough rays to be seen.

Every edit leaves the BVH valid without a rebuild: it shrinks a radius, collapses a triangle into
its own box, cuts the last primitive from the tree's coverage, or touches a ray.  Edits to `nodes`
alone are left out on purpose: the kernels read the node boxes from the caller's array on every
call (nothing of them is cached), and no one-word edit of the child ranges is valid under the
contract without an edit of `leaves` as well.  Out of scope likewise: the fp64 and mixed modes
(their records are never cached), the periodic traces (their arrays are the library's own) and
the point queries (no cache).

Restated from the sources, in one place; every index below follows from these by arithmetic.
"""
import functools

import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32

# csrc/trace_cache.hip:21-22 (SIG_BLOCK, SIG_GRID) and :46 (the grid-stride loop's stride)
SIG_BLOCK, SIG_GRID = 256, 1024
SIG_THREADS = SIG_GRID * SIG_BLOCK            # 262144 chunks per grid-stride iteration
# csrc/trace_cache.hip:48 (n_chunks = (words + 3) / 4) and :53-59 (uint4, or word by word)
CHUNK_WORDS, CHUNK_BYTES = 4, 16
# include/grace/ray.h:5-10; float4 spheres; tris_tree.cuh (vertex, two edges); nodes.h (4 x int4 a
# node, one int4 a leaf); csrc/trace.hip:361-363 (the bytes the signature is taken over)
RAY_WORDS, SPHERE_WORDS, TRI_WORDS, NODE_WORDS, LEAF_WORDS = 7, 4, 9, 16, 4
DX, DY, DZ, OX, OY, OZ, LEN = range(7)


def sort_passes(n_rays):
    """csrc/trace_coherence.hip:417-422 (ray_order): log2(packets of 64) + 2 key bits, in whole
    8-bit passes of the gated radix sort."""
    packets64 = -(-n_rays // 64)
    want_bits = 2
    while (1 << (want_bits - 2)) < packets64 and want_bits < 30:
        want_bits += 1
    return (want_bits + 7) // 8


def chunk_of(word):
    return word // CHUNK_WORDS


def iteration_of(chunk):
    """The grid-stride iteration of the signature kernel that reads chunk `chunk` of an array."""
    return chunk // SIG_THREADS


# The first ray whose words reach into the second grid-stride iteration, and its word that is word 0
# of chunk SIG_THREADS: ray 149796, word 4 (oy).
STRADDLE_RAY = (SIG_THREADS * CHUNK_WORDS) // RAY_WORDS
STRADDLE_WORD = SIG_THREADS * CHUNK_WORDS - STRADDLE_RAY * RAY_WORDS
# The smallest grid of rays that holds it: 388 x 388 = 150544 (16 * 97^2, padded to a multiple of 32)
STRADDLE_SIDE = 388
N_WIDE = SIG_THREADS + 64
THREE_PASS_RAYS = (1 << 20) + 64

PROBE_R = 0.04           # over a 1/64 grid: about 20 rays; a quarter of it: at most one
FINE_PROBE_R = 0.02      # the probes of the 388^2 and 1024^2 batches (rays 0.0015 / 0.0006 apart)
SHRINK = F32(0.25)
TILT = (F32(0.6), F32(0.0), F32(0.8))
TILT_T = 0.45            # the tilted ray crosses its probe this far along
OUTSIDE = 0.25
# ray grids: the whole scene and a margin (scene edits), and a rectangle that stops short of it (ray edits)
FULL = (-0.05, 1.1)
INSET = (0.1, 0.6)
RAY_START, RAY_LEN = -0.1, 1.2


class Edit:
    """words: flat 32-bit word indices into `array` ("spheres", "leaves", "rays" or "tris", from
    the base the library is given); new / old: their bits after / before."""

    def __init__(self, array, words, new, old):
        self.array = array
        self.words = [int(w) for w in words]
        self.new = [int(v) for v in new]
        self.old = [int(v) for v in old]
        assert 1 <= len(self.words) <= 2 and self.new != self.old

    def inverse(self):
        return Edit(self.array, self.words, self.old, self.new)

    def apply(self, a):
        """In place on a NumPy array (C-contiguous, 4-byte elements)."""
        flat = a.reshape(-1).view(U32)
        for w, v, o in zip(self.words, self.new, self.old):
            assert flat[w] == o, "the edit was made for another array"
            flat[w] = v
        return a

    @property
    def chunks(self):
        return [chunk_of(w) for w in self.words]


def _bits(x):
    return int(np.asarray(x, F32).reshape(1).view(U32)[0])


# ---- ray batches -----------------------------------------------------------------------------------
def grid_rays(side, axis, rect, n_total):
    """side x side rays along +e_axis, row-major over the two transverse co-ordinates (the first
    varies fastest), padded with copies of the first ray to n_total."""
    lo, span = rect
    t0, t1 = [k for k in range(3) if k != axis]
    m = side * side
    assert n_total >= m
    k = np.arange(m)
    r = np.zeros((n_total, RAY_WORDS), F32)
    r[:m, axis] = 1
    r[:m, 3 + t0] = (lo + (k % side + 0.5) * span / side).astype(F32)
    r[:m, 3 + t1] = (lo + (k // side + 0.5) * span / side).astype(F32)
    r[:m, 3 + axis] = RAY_START
    r[:m, LEN] = RAY_LEN
    r[m:] = r[0]
    return r


# name: (side, axis, rectangle, rays)
BATCHES = {
    "full4096": (64, 2, FULL, 4096),
    "z4096": (64, 2, INSET, 4096),                                   # one gated sort pass
    "z4128": (64, 2, INSET, 4096 + 32),                              # two
    "z388": (STRADDLE_SIDE, 2, INSET, -(-STRADDLE_SIDE ** 2 // 32) * 32),   # the signature's second iteration
    "z1024": (1024, 2, INSET, THREE_PASS_RAYS),                      # three gated passes
    "x4097": (64, 0, INSET, 4097),                                   # 7 n % 4 == 3 (C entry point only)
    "x4098": (64, 0, INSET, 4098),                                   # 7 n % 4 == 2
    "y4096": (64, 1, FULL, 4096),                                    # the triangles' batch
}


@functools.lru_cache(maxsize=None)
def batch(name):
    side, axis, rect, n = BATCHES[name]
    r = grid_rays(side, axis, rect, n)
    r.setflags(write=False)
    return r


def batch_axis(name):
    return BATCHES[name][1]


def view_offset_bytes(k, row_words):
    """Byte offset of pool[k:] from its (16-byte aligned) pool."""
    return k * row_words * 4


# ---- ray edits ---------------------------------------------------------------------------------------
def move_ray_inside(name, i, coord):
    """Ray i's transverse origin co-ordinate `coord` (OX, OY or OZ) moves to the far side of the
    batch's rectangle: the extents stay as they are."""
    r = batch(name)
    v = r[:, coord]
    assert coord - 3 != batch_axis(name)
    far = v.max() if r[i, coord] < 0.5 * (F64(v.min()) + F64(v.max())) else v.min()
    return Edit("rays", [RAY_WORDS * i + coord], [_bits(far)], [_bits(r[i, coord])])


def move_ray_outside(name, i, coord):
    """Ray i's transverse origin co-ordinate `coord` moves OUTSIDE beyond the rectangle's far edge."""
    r = batch(name)
    assert coord - 3 != batch_axis(name)
    new = F32(F64(r[:, coord].max()) + OUTSIDE)
    return Edit("rays", [RAY_WORDS * i + coord], [_bits(new)], [_bits(r[i, coord])])


def tilt_ray(name, i):
    """Ray i of a +z batch gets the direction (0.6, 0, 0.8): two words (dy stays 0)."""
    r = batch(name)
    assert batch_axis(name) == 2
    return Edit("rays", [RAY_WORDS * i + DX, RAY_WORDS * i + DZ], [_bits(TILT[0]), _bits(TILT[2])],
                [_bits(r[i, DX]), _bits(r[i, DZ])])


RAY_EDITS = {"inside": move_ray_inside, "outside": move_ray_outside, "tilt": lambda name, i, coord: tilt_ray(name, i)}

# (batch, edit, ray, co-ordinate): every ray edit of the tests; -1 stands for the last ray
MOVED_BATCHES = ("z4096", "z4128")
# (the last ray of "z4096" is the grid's far corner and moves along y; the padded batch's is a copy of
# its first ray)
MOVED_RAYS = {"z4096": ((0, OX), (-1, OY)), "z4128": ((0, OX), (-1, OX))}
RAY_CASES = [(b, e, i, c) for b in MOVED_BATCHES for e in ("inside", "outside", "tilt") for i, c in MOVED_RAYS[b]] + [
    ("z388", "inside", STRADDLE_RAY, STRADDLE_WORD), ("z388", "inside", -1, OX),
    ("z1024", "inside", THREE_PASS_RAYS // 2 + 7, OX), ("z1024", "inside", 0, OX),
    ("x4097", "inside", -1, OY), ("x4098", "inside", -1, OZ),
    ("x4097", "outside", -1, OY), ("x4098", "outside", -1, OZ),
]


def ray_index(name, i):
    return i % len(batch(name))


def ray_edit(name, kind, i, coord):
    return RAY_EDITS[kind](name, ray_index(name, i), coord)


def edited_rays(name, edit):
    r = batch(name).copy()
    return edit.apply(r)


def _probe_for(name, kind, i, coord):
    """The probe sphere the edited ray must cross: [x, y, z, r]."""
    i = ray_index(name, i)
    new = edited_rays(name, ray_edit(name, kind, i, coord))[i].astype(F64)
    t = TILT_T if kind == "tilt" else 0.5 - RAY_START
    c = new[3:6] + t * new[0:3]
    return np.array([c[0], c[1], c[2], PROBE_R if BATCHES[name][0] == 64 else FINE_PROBE_R])


# ---- sphere scenes -----------------------------------------------------------------------------------
class Scene:
    """spheres: float32 [n, 4] ALREADY in tree order (30-bit Morton keys over the unit box, stable):
    the build's sort leaves them where they are, so an index here is a sorted index.  probes: name
    -> sorted index.  mpl: max_per_leaf."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _tree_order(s):
    import oracle as O
    keys = O.morton_keys30(s, *UNIT)
    order = np.argsort(keys, kind="stable")
    return order, keys[order]


@functools.lru_cache(maxsize=None)
def small():
    """About 3000 spheres, radii 0.012 .. 0.03, one of 0.004 (below the ray spacing of a 64 x 64
    batch: the lattice rule r2_min < 2 e1 e2 / n of choose_variants holds), the probes "first",
    "mid" and "last" at sorted indices 0, somewhere in the middle and n - 1, and one probe per ray
    edit of RAY_CASES; the columns above the edited rays' ORIGINAL positions are empty."""
    import oracle as O
    rng = np.random.default_rng(2024)
    n_bg = 3000
    bg = np.empty((n_bg, 4), F32)
    bg[:, :3] = (0.002 + 0.996 * rng.random((n_bg, 3))).astype(F32)
    bg[:, 3] = rng.uniform(0.012, 0.03, n_bg).astype(F32)
    named = {"first": [0.03, 0.03, 0.03, PROBE_R], "mid": [0.4, 0.6, 0.45, PROBE_R], "last": [0.97, 0.97, 0.97, PROBE_R],
             "tiny": [0.31, 0.77, 0.52, 0.004]}
    ray_probes = []
    for case in RAY_CASES:
        p = _probe_for(*case)
        if not any(np.abs(p - q).max() < 1e-3 for q in ray_probes):
            ray_probes.append(p)
    probes = np.array(list(named.values()) + ray_probes, F32)
    # nothing above the edited rays where they stand before their edit
    old = np.array([batch(b)[ray_index(b, i)] for b, _, i, _ in RAY_CASES])
    keep = np.array([O.brute_hitcounts(old, bg[k:k + 1]).sum() == 0 for k in range(n_bg)])
    bg = bg[keep]
    # "first" / "last": nothing sorts before / after them
    kb = O.morton_keys30(bg, *UNIT)
    kp = O.morton_keys30(probes, *UNIT)
    bg = bg[(kb > kp[0]) & (kb < kp[2])]
    s = np.concatenate([bg, probes])
    order, _ = _tree_order(s)
    pos = np.empty(len(s), np.int64); pos[order] = np.arange(len(s))
    s = np.ascontiguousarray(s[order])
    where = {name: int(pos[len(bg) + k]) for k, name in enumerate(named)}
    where.update({"ray%d" % k: int(pos[len(bg) + len(named) + k]) for k in range(len(ray_probes))})
    s.setflags(write=False)
    return Scene(spheres=s, probes=where, mpl=16, name="small")


@functools.lru_cache(maxsize=None)
def wide():
    """SIG_THREADS + 64 spheres, radii 0.002 .. 0.004 (about seven hits a ray); the spheres at the
    sorted indices 0, SIG_THREADS - 1, SIG_THREADS and n - 1 -- the last chunk of the signature's
    first grid-stride iteration, the first of its second, and both ends -- are probes.  (A radius
    does not enter a Morton key: a sphere made a probe stays where it sorted.)"""
    rng = np.random.default_rng(77)
    n = N_WIDE
    s = np.empty((n, 4), F32)
    s[:, :3] = (0.002 + 0.996 * rng.random((n, 3))).astype(F32)
    s[:, 3] = rng.uniform(0.002, 0.004, n).astype(F32)
    order, _ = _tree_order(s)
    s = np.ascontiguousarray(s[order])
    where = {"first": 0, "stride_end": SIG_THREADS - 1, "stride_begin": SIG_THREADS, "last": n - 1}
    for j in where.values():
        s[j, 3] = F32(0.05)
    s.setflags(write=False)
    return Scene(spheres=s, probes=where, mpl=16, name="wide")


SCENES = {"small": small, "wide": wide}


def shrink(scene, j):
    """spheres[j].w *= 0.25, j a sorted index."""
    w = scene.spheres[j, 3]
    return Edit("spheres", [SPHERE_WORDS * j + 3], [_bits(F32(w * SHRINK))], [_bits(w)])


def cut_last_leaf(leaves):
    """leaves[n_nodes].y -= 1 (leaves: int32 [n_nodes + 1, 4] as built): the tree then covers
    spheres[:n - 1]."""
    last = len(leaves) - 1
    y = int(leaves[last, 1])
    assert y > 1, "the last leaf holds one sphere: cutting it would leave an empty leaf"
    return Edit("leaves", [LEAF_WORDS * last + 1], [y - 1], [y])


def scene_chunk(scene_n, n_nodes, edit):
    """The edit's chunk indices within the scene group, as the signature numbers them: the
    primitives' chunks, then the nodes', then the leaves' (trace_cache.hip: chunk0)."""
    base = {"spheres": 0, "leaves": chunk_of(SPHERE_WORDS * scene_n + 3) + chunk_of(NODE_WORDS * n_nodes + 3)}[edit.array]
    return [base + c for c in edit.chunks]


# ---- what an edit changes ------------------------------------------------------------------------------
def _sample(n_rays, extra, seed=5):
    rnd = np.random.default_rng(seed).choice(n_rays, min(256, n_rays), replace=False)
    return np.unique(np.concatenate([np.asarray(extra, np.int64).reshape(-1), rnd]))


class Case:
    """rays: the batch BEFORE the edit; edit; affected: the rays whose brute-force hit count (closest
    triangle) differs between the arrays before and after the edit; sub: the affected rays, the
    edited ray and 256 seeded random ones -- the rays checked against brute force."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _row_edit(edit, j):
    """The edit for sphere j's row alone (its radius at word 3, not 4 j + 3)."""
    return Edit(edit.array, [w - SPHERE_WORDS * j for w in edit.words], edit.new, edit.old)


@functools.lru_cache(maxsize=None)
def sphere_case(scene_name, batch_name, probe):
    """shrink of a probe, or (probe == "cut") the cut of the last leaf, whose Edit is made from the
    leaves on the spot: the case then carries edit = None and the sphere that leaves."""
    import oracle as O
    sc, rays = SCENES[scene_name](), batch(batch_name)
    if probe == "cut":
        j, edit = len(sc.spheres) - 1, None
        before = O.brute_hitcounts(rays, sc.spheres[j:j + 1])
        after = np.zeros_like(before)
    else:
        j = sc.probes[probe]
        edit = shrink(sc, j)
        row = _row_edit(edit, j).apply(sc.spheres[j:j + 1].copy())
        before = O.brute_hitcounts(rays, sc.spheres[j:j + 1])
        after = O.brute_hitcounts(rays, row)
    affected = np.nonzero(before != after)[0]
    return Case(scene=sc, batch=batch_name, rays=rays, edit=edit, j=j, affected=affected,
                sub=_sample(len(rays), affected), ray=None)


@functools.lru_cache(maxsize=None)
def ray_case(scene_name, batch_name, kind, i, coord):
    import oracle as O
    sc = SCENES[scene_name]()
    rays = batch(batch_name)
    i = ray_index(batch_name, i)
    edit = ray_edit(batch_name, kind, i, coord)
    new = edited_rays(batch_name, edit)
    before = O.brute_hitcounts(rays[i:i + 1], sc.spheres)
    after = O.brute_hitcounts(new[i:i + 1], sc.spheres)
    affected = np.array([i], np.int64) if before[0] != after[0] else np.zeros(0, np.int64)
    return Case(scene=sc, batch=batch_name, rays=rays, edit=edit, affected=affected, ray=i,
                counts=(int(before[0]), int(after[0])), sub=_sample(len(rays), [i]))


# ---- triangles -------------------------------------------------------------------------------------------
N_TRIS = 2001                      # 9 n % 4 == 1: the last chunk holds one word


@functools.lru_cache(maxsize=None)
def tris():
    """N_TRIS triangles (vertex, two edge vectors) in tree order: small background triangles and
    two probes in planes y = const that face the +y rays, with edges (a, 0, -c) and (a, 0, c) --
    setting the edges' last words to 0 makes them parallel: zero area, no hit, and the collapsed
    triangle lies inside the box of the original.  "last" is the last triangle of the sorted array,
    "mid" one in the middle; every background triangle that a probe's own ray (Scene.rays_of) hits,
    in front of the probe or behind it, is taken out: that ray finds nothing once its probe is
    collapsed."""
    import oracle as O
    rng = np.random.default_rng(9)
    rays = batch("y4096")
    n_bg = N_TRIS - 2
    bg = np.empty((n_bg + 400, 9), F32)
    bg[:, 0:3] = rng.uniform(0.02, 0.85, (len(bg), 3))
    bg[:, 3:9] = rng.uniform(-0.015, 0.015, (len(bg), 6))
    probes = np.array([[0.40, 0.45, 0.50, 0.1, 0, -0.08, 0.1, 0, 0.08],
                       [0.88, 0.97, 0.93, 0.1, 0, -0.08, 0.1, 0, 0.08]], F32)
    own = []
    for p in probes:                                     # the ray nearest the probe's centroid
        c = p[0:3] + (p[3:6] + p[6:9]) / 3
        own.append(int(np.argmin((rays[:, OX] - c[0]) ** 2 + (rays[:, OZ] - c[2]) ** 2)))
    own = np.array(own)
    for _ in range(64):                                  # clear what those rays hit first
        hit = O.brute_closest_tri(rays[own], bg)[0]
        if (hit < 0).all():
            break
        bg = np.delete(bg, hit[hit >= 0], axis=0)
    bg = bg[:n_bg]
    t = np.concatenate([bg, probes])
    bot, top = O.tri_centroid_bounds(t)
    order = np.argsort(O.morton_keys30_tri(t, bot, top), kind="stable")
    pos = np.empty(len(t), np.int64); pos[order] = np.arange(len(t))
    t = np.ascontiguousarray(t[order])
    t.setflags(write=False)
    return Scene(tris=t, probes={"mid": int(pos[n_bg]), "last": int(pos[n_bg + 1])},
                 rays_of={"mid": int(own[0]), "last": int(own[1])}, mpl=8, name="tris")


def collapse(scene, j):
    """The last words of triangle j's two edge vectors become 0."""
    t = scene.tris[j]
    return Edit("tris", [TRI_WORDS * j + 5, TRI_WORDS * j + 8], [0, 0], [_bits(t[5]), _bits(t[8])])


def fold(scene, j):
    """The last word of triangle j's second edge becomes that of its first: the edges coincide.  One
    word; for the last triangle, the last word of the array."""
    t = scene.tris[j]
    return Edit("tris", [TRI_WORDS * j + 8], [_bits(t[5])], [_bits(t[8])])


@functools.lru_cache(maxsize=None)
def tri_case(probe, kind="collapse"):
    import oracle as O
    sc, rays = tris(), batch("y4096")
    j = sc.probes[probe]
    edit = {"collapse": collapse, "fold": fold}[kind](sc, j)
    before = O.brute_closest_tri(rays, sc.tris)[0]
    after = O.brute_closest_tri(rays, edit.apply(sc.tris.copy()))[0]
    affected = np.nonzero(before != after)[0]
    return Case(scene=sc, batch="y4096", rays=rays, edit=edit, j=j, affected=affected, before=before, after=after,
                sub=_sample(len(rays), np.append(affected, sc.rays_of[probe])), ray=sc.rays_of[probe])
