"""Delta patterns, scenes and an independent tree checker for the ALBVH builder's boundaries.

A plain helper module (numpy only; no GPU, no torch, no oracle): tests/test_albvh_boundaries.py
builds its cases on the GPU, tests/test_albvh_boundary_cases.py checks on the CPU that the oracle's
trees pass the checker, that the checker rejects broken trees, and that the cases reach the code
paths they are named after.

Delta arrays have n + 1 entries and keep the reference's +1 shift: deltas[k + 1] = delta(k), the
distance between primitives k and k + 1; deltas[0] and deltas[n] hold the sentinel this library's
delta functions write for the type (deltas.hip, grace_oracle.c: +inf for floats, all ones for
unsigned).  The oracle's restatement reads the sentinels, the HIP build does not, so every inner
delta is strictly below the sentinel (asserted by `finish`).

A pattern is a tuple: ("random",), ("equal",), ("ascending",), ("descending",), ("few",),
("sawtooth", p, s), ("plateau", L, s), and for the node stage ("spike_first",) and ("spike_last",):
ascending deltas after a largest first one, descending deltas before a largest last one, so that every
node's nearest greater neighbour is the first or the last node of the array -- the searches climb to
the top of the pyramid and descend into its first or its ragged last block.  Every pattern is first
an integer array below 2^24, which float32 and uint32 both hold exactly: the f32 and the u32 form of a
pattern have the same order and so the same tree.
"""
import numpy as np

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64

SHIFTS = (0, 1, 63, 255)
SAWTOOTH_PERIODS = (32, 64, 257)
PLATEAU_LENGTHS = (63, 64, 65, 127, 257)
SIMPLE = (("random",), ("equal",), ("ascending",), ("descending",), ("few",))
SHIFTED = tuple(("sawtooth", p, s) for p in SAWTOOTH_PERIODS for s in SHIFTS) \
    + tuple(("plateau", L, s) for L in PLATEAU_LENGTHS for s in SHIFTS)
ALL_PATTERNS = SIMPLE + SHIFTED

LEAF_MPLS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 255, 256, 257, 300)
LEAF_NS = (257, 600, 1025)
NODE_NS = (2, 3, 33, 34, 35, 1025, 1026, 1027, 32769, 32770, 32771)
NODE_PATTERNS = SIMPLE + (("sawtooth", 32, 0),) + (("spike_first",), ("spike_last",))
HUGE_N = (1 << 20) + 2
TYPE_MPLS = (1, 32, 65, 257)
TYPE_PATTERNS = (("equal",), ("ascending",), ("few",), ("plateau", 65, 0))

PYR = 32                        # albvh.hip: the pyramids are 32-ary
LEAF_FAST_MARGIN = 64           # albvh.hip: the reach of the sparse-table searches (mpl <= 64)


def pattern_id(p):
    return "-".join(str(x) for x in p)


def leaf_mpls(n):
    """The max_per_leaf values of the leaf-stage cases at n primitives (n - 1 added)."""
    return tuple(sorted(set(LEAF_MPLS + (n - 1,))))


def sentinel(dtype):
    dtype = np.dtype(dtype)
    return dtype.type(np.inf) if dtype.kind == "f" else dtype.type(np.iinfo(dtype).max)


def finish(inner, dtype):
    """inner: the n - 1 inner deltas.  Returns the shifted array with both sentinels."""
    inner = np.asarray(inner)
    s = sentinel(dtype)
    out = np.empty(len(inner) + 2, dtype)
    out[0] = out[-1] = s
    out[1:-1] = inner
    assert np.array_equal(out[1:-1].astype(inner.dtype), inner), "pattern not exact in dtype"
    assert np.all(out[1:-1] < s), "an inner delta is not strictly below the sentinel"
    return out


def levels(pattern, n, seed=0):
    """The pattern as n - 1 integers in [0, 2^24)."""
    m = n - 1
    k = np.arange(m, dtype=np.int64)
    kind = pattern[0]
    if kind == "random":
        v = np.random.default_rng(1000 + seed).integers(0, 1 << 24, m)
    elif kind == "equal":
        v = np.full(m, 7, np.int64)
    elif kind == "ascending":
        v = k
    elif kind == "descending":
        v = m - 1 - k
    elif kind == "few":
        v = np.random.default_rng(2000 + seed).integers(0, 3, m)
    elif kind == "spike_first":
        v = k.copy()
        v[:1] = m
    elif kind == "spike_last":
        v = m - 1 - k
        v[-1:] = m
    elif kind == "sawtooth":
        _, p, s = pattern
        v = (k + s) % p
    elif kind == "plateau":
        _, L, s = pattern
        v = np.where((k + s) % L == L - 1, 9, 5)
    else:
        raise ValueError(pattern)
    v = np.asarray(v, np.int64)
    assert m == 0 or (v.min() >= 0 and v.max() < (1 << 24))
    return v


def deltas(pattern, n, dtype, seed=0, offset=0):
    """The pattern as a shifted delta array of float32 or uint32.  offset is added to every inner
    value (the comparator cases need unsigned values >= 1, so that their bitwise NOT stays below the
    sentinel)."""
    return finish(levels(pattern, n, seed) + offset, dtype)


def flip(d):
    """Order reversal of the inner deltas: negation for floats, bitwise NOT for unsigned.
    COMP_GREATER on d must give the tree of COMP_LESS on flip(d).  The ends stay the sentinel."""
    d = np.asarray(d)
    inner = -d[1:-1] if d.dtype.kind == "f" else ~d[1:-1]
    return finish(inner, d.dtype)


def ranks(d):
    """Dense ranks of the inner deltas (equal values get equal ranks, order is preserved) as a
    uint64 delta array: the same tree in another type."""
    d = np.asarray(d)
    _, inv = np.unique(d[1:-1], return_inverse=True)
    return finish(inv.astype(U64), U64)


def f64_from_ranks(r):
    """Inner values 1 + rank * 2^-40: distinct in double, all 1.0f once narrowed to float."""
    inner = 1.0 + r[1:-1].astype(F64) * 2.0 ** -40
    assert len(inner) == 0 or np.all(inner.astype(F32) == F32(1.0))
    assert np.array_equal(np.unique(inner, return_inverse=True)[1], r[1:-1].astype(np.int64))
    return finish(inner, F64)


U64_HIGH_WORD = U64(0x5A5A1234) << U64(32)


def u64_high_from_ranks(r):
    """The ranks in the high word only: a compare of the low words sees all-equal deltas."""
    assert np.all(r[1:-1] < U64(1 << 31))
    return finish(r[1:-1] << U64(32), U64)


def u64_low_from_ranks(r):
    """The ranks in the low word under a constant high word."""
    assert np.all(r[1:-1] < U64(1 << 31))
    return finish(r[1:-1] | U64_HIGH_WORD, U64)


def run_lengths(d):
    """Per inner node j, the unbounded run lengths of the leaf stage's two scans (albvh.hip): to
    the left while delta(k) < delta(j), to the right while !(delta(j) < delta(k))."""
    x = np.asarray(d)[1:-1]
    m = len(x)
    out = np.empty(m, np.int64)
    for j in range(m):
        stop_l = np.flatnonzero(~(x[:j] < x[j]))
        stop_r = np.flatnonzero(x[j] < x[j + 1:])
        left = j - (stop_l[-1] + 1) if len(stop_l) else j
        right = stop_r[0] if len(stop_r) else m - 1 - j
        out[j] = left + right
    return out


def pyramid_levels(n_entries):
    """Levels of a 32-ary pyramid over n_entries (albvh.hip: a level is added while the last one
    has more than PYR entries)."""
    lv, size = 1, n_entries
    while size > PYR:
        size = (size + PYR - 1) // PYR
        lv += 1
    return lv


# ---- primitives ----------------------------------------------------------------------------------
def spheres(n, seed=0):
    """Random float4 spheres with positive co-ordinates (no signed zeros in the boxes), unsorted:
    any deltas give a valid tree over any primitive order."""
    rng = np.random.default_rng(3000 + seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.uniform(0.1, 1.0, (n, 3))
    s[:, 3] = rng.uniform(0.002, 0.03, n)
    return s


def sphere_boxes(s):
    """AABBSphere: centre -+ radius, in the primitives' precision, narrowed to float."""
    s = np.asarray(s)
    return np.concatenate([s[:, :3] - s[:, 3:4], s[:, :3] + s[:, 3:4]], 1).astype(F32)


def triangles(n, seed=0):
    rng = np.random.default_rng(4000 + seed)
    t = np.empty((n, 9), F32)
    t[:, :3] = rng.uniform(0.1, 1.0, (n, 3))
    t[:, 3:] = rng.uniform(-0.05, 0.05, (n, 6))
    return t


def triangle_boxes(t):
    """TriangleAABB: min / max over v, v + e1, v + e2 in float (no flat triangles here)."""
    t = np.asarray(t, F32)
    c = np.stack([t[:, :3], t[:, :3] + t[:, 3:6], t[:, :3] + t[:, 6:9]])
    lo, hi = c.min(0), c.max(0)
    assert np.all(lo < hi)
    return np.concatenate([lo, hi], 1).astype(F32)


def spheres_d4(n, seed=0):
    rng = np.random.default_rng(5000 + seed)
    s = np.empty((n, 4), F64)
    s[:, :3] = rng.uniform(0.1, 1.0, (n, 3))
    s[:, 3] = rng.uniform(0.002, 0.03, n)
    return s


# ---- geometry-driven ties (whole pipeline) ---------------------------------------------------------
def tie_scene(name):
    """Unsorted float4 spheres in the unit box whose Euclidean deltas tie."""
    rng = np.random.default_rng(6000)
    if name == "lattice":
        g = (np.arange(16, dtype=F32) + F32(0.5)) / F32(16)
        c = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        r = np.full(len(c), 0.01, F32)
    elif name == "coincident":
        c = rng.uniform(0.05, 0.95, (5000, 3)).astype(F32)
        c[1000:4000] = F32(0.4375)
        r = rng.uniform(0.002, 0.03, 5000).astype(F32)
    elif name == "collinear":
        q = 1.004 ** np.arange(2000)
        x = (0.01 + 0.98 * (q - 1.0) / (q[-1] - 1.0)).astype(F32)
        c = np.stack([x, x, x], 1)
        r = np.full(2000, 1e-4, F32)
    elif name == "two-points":
        c = np.empty((2000, 3), F32)
        c[0::2] = (0.25, 0.5, 0.75)
        c[1::2] = (0.75, 0.25, 0.5)
        r = rng.uniform(0.002, 0.03, 2000).astype(F32)
    else:
        raise ValueError(name)
    s = np.concatenate([c, r[:, None]], 1).astype(F32)
    return np.ascontiguousarray(s[rng.permutation(len(s))])


TIE_SCENES = ("lattice", "coincident", "collinear", "two-points")


# ---- spheres on a line, for traces of deep trees -------------------------------------------------
LINE_DIR = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
LINE_PERP = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
LINE_STEP, LINE_RADIUS = 0.01, 0.003


def line_scene(n):
    """n small spheres on a diagonal line, and 64 rays: 32 along the line (different origins within
    a third of a radius of it: no pencil, not axis-aligned) that hit every sphere, and 32 across it
    that hit one sphere each."""
    rng = np.random.default_rng(7000 + n)
    p0 = np.array([0.1, 0.2, 0.3])
    k = np.arange(n)
    s = np.empty((n, 4), F32)
    s[:, :3] = p0 + (k * LINE_STEP)[:, None] * LINE_DIR
    s[:, 3] = LINE_RADIUS
    rays = np.empty((64, 7), F32)
    other = np.cross(LINE_DIR, LINE_PERP)
    jit = rng.uniform(-1, 1, (32, 2)) * (LINE_RADIUS / 3 / np.sqrt(2))
    rays[:32, 0:3] = LINE_DIR
    rays[:32, 3:6] = p0 - 2 * LINE_STEP * LINE_DIR + jit[:, :1] * LINE_PERP + jit[:, 1:] * other
    rays[:32, 6] = (n + 4) * LINE_STEP
    target = np.linspace(0, n - 1, 32).round().astype(int)
    rays[32:, 0:3] = LINE_PERP
    rays[32:, 3:6] = s[target, :3].astype(F64) - 0.5 * LINE_PERP + jit[:, :1] * other
    rays[32:, 6] = 1.0
    return s, rays


# ---- the checker -----------------------------------------------------------------------------------
class TreeError(AssertionError):
    """The tree violates a property of the build's contract."""


def _req(cond, *what):
    if not cond:
        raise TreeError(*what)


def child_box(nodes, j, right):
    """Node j's child box {bot xyz, top xyz} as uint32 bits (include/grace/cuda/nodes.h:
    nodes[4j+1] = left {bx, tx, by, ty}, [4j+2] = right, [4j+3] = {left bz, tz, right bz, tz})."""
    w = np.asarray(nodes).view(U32).reshape(-1, 16)
    a, z = (8, 14) if right else (4, 12)
    return np.stack([w[j, a], w[j, a + 2], w[j, z], w[j, a + 1], w[j, a + 3], w[j, z + 1]], -1)


def set_child_box(nodes, j, right, box_bits):
    w = nodes.view(U32).reshape(-1, 16)
    a, z = (8, 14) if right else (4, 12)
    for src, dst in enumerate((a, a + 2, z, a + 1, a + 3, z + 1)):
        w[j, dst] = box_bits[src]


def _range_boxes(lb, a, b):
    """Unions of the leaf boxes a[i] .. b[i] (inclusive), exactly (min / max only), through a table
    of unions over 2^k leaves."""
    lo, hi = [lb[:, :3]], [lb[:, 3:]]
    while 2 << (len(lo) - 1) <= len(lb):
        h = 1 << (len(lo) - 1)
        lo.append(np.minimum(lo[-1][:-h], lo[-1][h:]))
        hi.append(np.maximum(hi[-1][:-h], hi[-1][h:]))
    k = np.floor(np.log2(b - a + 1)).astype(np.int64)
    out = np.empty((len(a), 6), F32)
    for lv in np.unique(k):
        m = k == lv
        e = b[m] - (1 << lv) + 1
        out[m, :3] = np.minimum(lo[lv][a[m]], lo[lv][e])
        out[m, 3:] = np.maximum(hi[lv][a[m]], hi[lv][e])
    return out


def check_tree(deltas, mpl, boxes, leaves, nodes, root, thorough=True):
    """Asserts (TreeError) that (leaves, nodes, root) is the tree build_ALBVH must give for these
    shifted deltas, max_per_leaf and primitive boxes [n, 6] {bot xyz, top xyz}:
      * the leaves cover [0, n) in order with 1 .. mpl primitives each, and each is a whole subtree
        of the hierarchy over the primitives;
      * every internal node spans more than mpl primitives (the leaves are maximal);
      * the child slots and the root list 0 .. n_nodes + n_leaves - 1 exactly once;
      * node j's left child covers leaves first .. j, its right child j + 1 .. last, down to the
        leaves, and the root covers every leaf (checked slot by slot and by an iterative walk);
      * node j's range is bounded by its nearest greater neighbours in the order (delta, -index):
        first - 1 = the nearest i < j with !(d(i) < d(j)), last = the nearest i > j with
        d(j) < d(i) (albvh.hip's header), d = the deltas between leaves;
      * both child boxes of every node are, bit for bit, the union of the primitive boxes below.
    thorough=False (trees too large for a Python loop over every node): no walk, the nearest-greater
    searches and the boxes on a sample of nodes only; the other properties on every node, with the
    heap order of every (parent, child) pair standing in for the searches.
    Returns {"depth": ...} (None without the walk)."""
    d = np.asarray(deltas)
    n = len(d) - 1
    leaves = np.asarray(leaves)
    nodes = np.ascontiguousarray(nodes).view(np.int32)
    boxes = np.ascontiguousarray(boxes, F32)
    L = len(leaves)
    N = L - 1
    _req(L >= 2 and leaves.ndim == 2 and leaves.shape[1] == 4, "leaf array shape")
    _req(nodes.shape == (N, 16), "node array shape", nodes.shape, N)
    _req(boxes.shape == (n, 6), "primitive boxes shape")
    start, cnt = leaves[:, 0].astype(np.int64), leaves[:, 1].astype(np.int64)

    # leaves partition the primitives
    _req(start[0] == 0, "first leaf does not start at 0")
    _req(np.all(cnt >= 1) and np.all(cnt <= mpl), "leaf size outside 1 .. mpl")
    _req(np.array_equal(start[1:], start[:-1] + cnt[:-1]), "leaves are not contiguous")
    _req(start[-1] + cnt[-1] == n, "leaves do not end at n")
    _req(np.all(leaves[:, 2:] == 0), "leaf padding not zero")
    # each leaf of several primitives is a whole subtree: its inner deltas stay below the delta on
    # its right, and the delta on its left is not below them (ties merge right first)
    x = d[1:]                                         # x[k] = delta(k), x[n - 1] the sentinel
    for k in np.flatnonzero(cnt > 1):
        a, b = start[k], start[k] + cnt[k] - 1        # primitives a .. b
        top = x[a:b].max()
        _req(b == n - 1 or top < x[b], "leaf is not a subtree (right)", k)
        _req(a == 0 or not (x[a - 1] < top), "leaf is not a subtree (left)", k)
    ld = x[start[:-1] + cnt[:-1] - 1]                 # ld[j] = d(j), the delta between leaves j, j+1

    j = np.arange(N, dtype=np.int64)
    left, right = nodes[:, 0].astype(np.int64), nodes[:, 1].astype(np.int64)
    first, last = nodes[:, 2].astype(np.int64), nodes[:, 3].astype(np.int64)
    _req(np.all((0 <= first) & (first <= j) & (j < last) & (last <= L - 1)), "node range does not hold its split")
    # maximal leaves
    span = start[last] + cnt[last] - start[first]
    _req(np.all(span > mpl), "an internal node holds <= mpl primitives", np.flatnonzero(span <= mpl)[:5])
    # child slots + root: a permutation
    slots = np.concatenate([left, right, [int(root)]])
    _req(np.array_equal(np.sort(slots), np.arange(N + L)), "child slots and root are not a permutation")
    _req(0 <= root < N and first[root] == 0 and last[root] == L - 1, "root does not cover every leaf")
    # ranges nest
    for child, lo, hi, side in ((left, first, j, "left"), (right, j + 1, last, "right")):
        isn = child < N
        c = child[isn]
        _req(np.all(first[c] == lo[isn]) and np.all(last[c] == hi[isn]), side + " child node's range")
        _req(np.all(child[~isn] - N == lo[~isn]) and np.all(lo[~isn] == hi[~isn]), side + " child leaf's range")
    # heap order of every (parent, child) pair under (delta, -index)
    parent = np.full(N + L, -1, np.int64)
    parent[left] = j
    parent[right] = j
    pj = parent[:N]
    has = pj >= 0
    _req(has.sum() == N - 1 and not has[root], "parents")
    dp, dc = ld[pj[has]], ld[j[has]]
    _req(np.all((dc < dp) | (~(dp < dc) & (pj[has] < j[has]))), "a node is not below its parent in (delta, -index)")

    depth = None
    if thorough:
        # the walk, iteratively (a chain is n_leaves deep)
        nl, nr = left.tolist(), right.tolist()
        nf, nt = first.tolist(), last.tolist()
        stack = [(int(root), 0, L - 1, 1)]
        seen, depth = 0, 0
        while stack:
            idx, lo, hi, dep = stack.pop()
            seen += 1
            if dep > depth:
                depth = dep
            if idx < N:
                _req(nf[idx] == lo and nt[idx] == hi, "walk: node range", idx)
                stack.append((nr[idx], idx + 1, hi, dep + 1))
                stack.append((nl[idx], lo, idx, dep + 1))
            else:
                _req(idx - N == lo == hi, "walk: leaf", idx - N)
            _req(seen <= N + L, "walk: cycle")
        _req(seen == N + L, "walk: not every node and leaf is reached")

    if thorough and N <= 4096:
        sample = j
    else:
        rng = np.random.default_rng(N)
        edges = np.concatenate([np.arange(-3, 3) + e for e in range(0, N + 1, 32768)])
        sample = np.unique(np.clip(np.concatenate([edges, rng.integers(0, N, 256)]), 0, N - 1))
    # the merge rule from its definition
    for t in sample:
        stop_l = np.flatnonzero(~(ld[:t] < ld[t]))
        stop_r = np.flatnonzero(ld[t] < ld[t + 1:])
        f = stop_l[-1] + 1 if len(stop_l) else 0
        la = t + 1 + stop_r[0] if len(stop_r) else L - 1
        _req(first[t] == f and last[t] == la, "merge rule", int(t), (first[t], last[t]), (f, la))
    # child boxes: exact unions of the primitive boxes below
    lb = np.concatenate([np.minimum.reduceat(boxes[:, :3], start), np.maximum.reduceat(boxes[:, 3:], start)], 1)
    if L <= (1 << 17):
        for rgt, a, b in ((False, first, j), (True, j + 1, last)):
            want = _range_boxes(lb, a, b).view(U32)
            got = child_box(nodes, j, rgt)
            bad = np.flatnonzero((want != got).any(1))
            _req(len(bad) == 0, "child box is not the exact union", "right" if rgt else "left", bad[:5])
    else:
        for t in sample:
            for rgt, a, b in ((False, first[t], t), (True, t + 1, last[t])):
                want = np.concatenate([lb[a:b + 1, :3].min(0), lb[a:b + 1, 3:].max(0)]).view(U32)
                _req(np.array_equal(want, child_box(nodes, t, rgt)), "child box is not the exact union", int(t))
    return {"depth": depth}
