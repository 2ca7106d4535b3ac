"""CPU checks of tests/albvh_boundary_cases.py: the oracle's trees pass the independent checker on
every pattern the GPU tests build, the checker rejects every broken tree it is shown, and the cases
reach the builder paths they are named after (pyramid levels, runs past the 64-entry margin, chains
deeper than the trace's stack)."""
import numpy as np
import pytest

import albvh_boundary_cases as A

F32, U32, U64 = np.float32, np.uint32, np.uint64
N_LEAF = 600


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- the generator -----------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", A.ALL_PATTERNS, ids=A.pattern_id)
def test_patterns_hold_their_sentinels_and_maps(oracle, pattern):
    n = 300
    s = A.spheres(n)
    f = A.deltas(pattern, n, F32)
    u = A.deltas(pattern, n, U32)
    assert f.dtype == F32 and u.dtype == U32 and len(f) == len(u) == n + 1
    assert np.isposinf(f[0]) and np.isposinf(f[-1]) and u[0] == u[-1] == 0xFFFFFFFF
    # (the oracle's own delta functions write the same sentinels)
    assert np.isposinf(oracle.deltas_euclid(s)[[0, -1]]).all()
    assert (oracle.deltas_xor(np.arange(n, dtype=U32))[[0, -1]] == 0xFFFFFFFF).all()
    assert (oracle.deltas_xor(np.arange(n, dtype=U64))[[0, -1]] == U64(2 ** 64 - 1)).all()
    assert np.array_equal(f[1:-1].astype(np.int64), u[1:-1].astype(np.int64))
    r = A.ranks(f)
    assert r.dtype == U64 and r[0] == r[-1] == U64(2 ** 64 - 1)
    assert np.array_equal(A.ranks(u), r)
    order = np.argsort(f[1:-1], kind="stable")
    assert np.all(np.diff(r[1:-1][order].astype(np.int64)) >= 0)
    assert np.array_equal(np.diff(r[1:-1][order].astype(np.int64)) == 0, np.diff(f[1:-1][order]) == 0)
    # flip reverses the order and is its own inverse
    ff = A.flip(f)
    assert np.array_equal(A.flip(ff), f)
    assert np.array_equal(A.ranks(ff)[1:-1], r[1:-1].max() - r[1:-1])
    u1 = A.deltas(pattern, n, U32, offset=1)
    assert np.array_equal(A.ranks(A.flip(u1)), A.ranks(ff)) and np.array_equal(A.flip(A.flip(u1)), u1)
    # the wide types carry the same order where a narrowed compare cannot see it
    d64 = A.f64_from_ranks(r)
    hi, lo = A.u64_high_from_ranks(r), A.u64_low_from_ranks(r)
    for w in (d64, hi, lo):
        assert np.array_equal(A.ranks(w), r)
    assert np.all(hi[1:-1] & U64(0xFFFFFFFF) == 0) and np.all(lo[1:-1] >> U64(32) == lo[1] >> U64(32))
    for mpl in (1, 32):
        ref = oracle.albvh(s, f, mpl)
        assert _same(ref, oracle.albvh(s, u, mpl)) and _same(ref, oracle.albvh(s, r, mpl))
        assert _same(ref, oracle.albvh(s, hi, mpl)) and _same(ref, oracle.albvh(s, lo, mpl))


def test_an_unsigned_zero_cannot_be_flipped():
    with pytest.raises(AssertionError):
        A.flip(A.deltas(("few",), 50, U32))


# ---- the oracle against the checker ------------------------------------------------------------
@pytest.mark.parametrize("pattern", A.ALL_PATTERNS, ids=A.pattern_id)
def test_oracle_tree_passes_checker(oracle, pattern):
    n = N_LEAF
    s = A.spheres(n)
    boxes = A.sphere_boxes(s)
    f, u = A.deltas(pattern, n, F32), A.deltas(pattern, n, U32)
    for mpl in A.leaf_mpls(n):
        ref = oracle.albvh(s, f, mpl)
        assert _same(ref, oracle.albvh(s, u, mpl))
        A.check_tree(f, mpl, boxes, ref[1], ref[0], ref[2])
    with pytest.raises(ValueError):
        oracle.albvh(s, f, n)


CHAINS = (("equal",), ("ascending",), ("descending",))


@pytest.mark.parametrize("n", [33, 34, 1026, 32770])
@pytest.mark.parametrize("pattern", A.NODE_PATTERNS, ids=A.pattern_id)
def test_oracle_tree_passes_checker_one_primitive_per_leaf(oracle, pattern, n):
    s = A.spheres(n)
    f = A.deltas(pattern, n, F32)
    nodes, leaves, root, _ = oracle.albvh(s, f, 1)
    assert len(leaves) == n
    stats = A.check_tree(f, 1, A.sphere_boxes(s), leaves, nodes, root)
    if pattern in CHAINS or pattern[0].startswith("spike"):
        assert stats["depth"] == n            # a chain: recursion would not survive it
    elif pattern == ("random",):
        assert stats["depth"] < min(n, 64)
    if pattern[0].startswith("spike"):        # every other node is bounded by the spike, far away
        far = nodes[:, 2] == 1 if pattern == ("spike_first",) else nodes[:, 3] == n - 2
        assert far.sum() == n - 2


def test_other_primitive_kinds_pass_checker(oracle):
    n, mpl = 300, 5
    f = A.deltas(("few",), n, F32)
    t, d4 = A.triangles(n), A.spheres_d4(n)
    for prims, boxes, kind in ((t, A.triangle_boxes(t), 1), (d4, A.sphere_boxes(d4), 2)):
        nodes, leaves, root, _ = oracle.albvh(prims, f, mpl, prim_kind=kind)
        A.check_tree(f, mpl, boxes, leaves, nodes, root)


# ---- path coverage -----------------------------------------------------------------------------
MAX_LEVELS = {2: 1, 3: 1, 33: 1, 34: 2, 35: 2, 1025: 2, 1026: 3, 1027: 3, 32769: 3, 32770: 4, 32771: 4,
              A.HUGE_N: 5}
BOX_LEVELS = {2: 1, 3: 1, 33: 2, 34: 2, 35: 2, 1025: 3, 1026: 3, 1027: 3, 32769: 4, 32770: 4, 32771: 4,
              A.HUGE_N: 5}


@pytest.mark.parametrize("n", A.NODE_NS + (A.HUGE_N,))
def test_node_stage_sizes_reach_every_pyramid_depth(oracle, n):
    """mpl = 1: n leaves, n - 1 nodes.  The maxima pyramid (over the nodes) and the box pyramid
    (over the leaves) gain a level when their base passes 32, 1024, 32768, 2^20."""
    _, leaves, _, _ = oracle.albvh(A.spheres(n), A.deltas(("random",), n, F32), 1)
    assert len(leaves) == n
    assert A.pyramid_levels(len(leaves) - 1) == MAX_LEVELS[n]
    assert A.pyramid_levels(len(leaves)) == BOX_LEVELS[n]
    assert set(MAX_LEVELS.values()) == set(BOX_LEVELS.values()) == {1, 2, 3, 4, 5}
    assert [A.pyramid_levels(x) for x in (32, 33, 1024, 1025, 32768, 32769, 1 << 20, (1 << 20) + 1)] \
        == [1, 2, 2, 3, 3, 4, 4, 5]


@pytest.mark.parametrize("n", A.LEAF_NS)
@pytest.mark.parametrize("pattern", [p for p in A.SHIFTED if p[0] == "plateau"], ids=A.pattern_id)
def test_plateau_runs_pass_the_fast_path_margin(pattern, n):
    """The sparse-table searches of the mpl <= 64 path reach 63 entries; every plateau pattern
    holds runs that go on beyond that, so the search has to saturate, not end."""
    runs = A.run_lengths(A.deltas(pattern, n, F32))
    assert runs.max() > A.LEAF_FAST_MARGIN
    assert (runs > A.LEAF_FAST_MARGIN).sum() >= n // pattern[1] - 1


def test_shifts_move_runs_across_words_and_blocks():
    """The shifts put the spikes of plateau(L, s) at different lanes of the 64-lane ballot words
    (for L = 64: the last, the one before it and the first lane of a word)."""
    for L in A.PLATEAU_LENGTHS:
        lanes = set()
        for s in A.SHIFTS:
            spikes = np.flatnonzero(A.levels(("plateau", L, s), 1025) == 9)
            lanes |= set((spikes[:2] % 64).tolist())
        assert len(lanes) >= 3


def test_line_scene_rays_and_chains(oracle):
    for n in (100, 300):
        s, rays = A.line_scene(n)
        counts = oracle.brute_hitcounts(rays, s)
        assert np.all(counts[:32] == n) and np.all(counts[32:] == 1)
        boxes = A.sphere_boxes(s)
        for pattern in CHAINS:
            f = A.deltas(pattern, n, F32)
            nodes, leaves, root, _ = oracle.albvh(s, f, 1)
            assert A.check_tree(f, 1, boxes, leaves, nodes, root)["depth"] == n
            left_deep = nodes[root, 0] < n - 1
            assert left_deep == (pattern == ("ascending",))   # pending right leaves pile up on a stack


@pytest.mark.parametrize("name", A.TIE_SCENES)
def test_tie_scenes_tie(oracle, name):
    s = A.tie_scene(name)
    keys = oracle.morton_keys30(s, (0, 0, 0), (1, 1, 1))
    _, ss, _ = oracle.sort_by_key(keys, s)
    d = oracle.deltas_euclid(ss)[1:-1]
    ties = len(d) - len(np.unique(d))
    assert ties >= {"lattice": 4000, "coincident": 2998, "collinear": 0, "two-points": 1997}[name]
    if name == "collinear":
        # where the spacing exceeds a key cell (2^-10) the deltas ascend: a left-deep chain; below
        # it, spheres share keys and keep the order they came in
        assert np.all(np.diff(d[-300:]) > 0) and not np.all(np.diff(d[:300]) > 0)


# ---- the checker must be able to fail ----------------------------------------------------------
def _valid(oracle, pattern=("random",), n=N_LEAF, mpl=5):
    s = A.spheres(n)
    f = A.deltas(pattern, n, F32)
    nodes, leaves, root, ld = oracle.albvh(s, f, mpl)
    boxes = A.sphere_boxes(s)
    A.check_tree(f, mpl, boxes, leaves, nodes, root)
    return f, mpl, boxes, leaves.copy(), nodes.copy(), root, ld


def _rejected(f, mpl, boxes, leaves, nodes, root):
    with pytest.raises(A.TreeError):
        A.check_tree(f, mpl, boxes, leaves, nodes, root)


def test_checker_rejects_swapped_children(oracle):
    f, mpl, boxes, leaves, nodes, root, _ = _valid(oracle)
    for j in (0, len(nodes) // 2, root):
        m = nodes.copy()
        m[j, [0, 1]] = m[j, [1, 0]]
        _rejected(f, mpl, boxes, leaves, m, root)


def test_checker_rejects_moved_leaf_boundary(oracle):
    f, mpl, boxes, leaves, nodes, root, _ = _valid(oracle)
    grow = np.flatnonzero((leaves[:-1, 1] < mpl) & (leaves[1:, 1] > 1))
    shrink = np.flatnonzero((leaves[:-1, 1] > 1) & (leaves[1:, 1] < mpl))
    assert len(grow) and len(shrink)
    for k, step in [(k, 1) for k in grow[:20]] + [(k, -1) for k in shrink[:20]]:
        m = leaves.copy()
        m[k, 1] += step; m[k + 1, 0] += step; m[k + 1, 1] -= step
        _rejected(f, mpl, boxes, m, nodes, root)


def test_checker_rejects_merged_leaves(oracle):
    """Two sibling leaves merged into one, their node removed and every index renumbered: a
    well-formed tree whose only fault is a leaf that is too large."""
    f, mpl, boxes, leaves, nodes, root, _ = _valid(oracle)
    N = len(nodes)
    k = int(np.flatnonzero((nodes[:, 0] == N + np.arange(N)) & (nodes[:, 1] == N + np.arange(N) + 1))[0])
    assert k != root
    ml = np.delete(leaves, k + 1, 0)
    ml[k, 1] = leaves[k, 1] + leaves[k + 1, 1]
    mn = np.delete(nodes, k, 0)
    ch = mn[:, :2].astype(np.int64)

    def renumber(c):   # node indices above k and leaf indices above k drop by one; N drops by one
        isleaf = c >= N
        leaf = c - N
        return np.where(isleaf, (N - 1) + leaf - (leaf > k), c - (c > k))
    was_k = ch == k
    ch = renumber(ch)
    ch[was_k] = (N - 1) + k
    mn[:, :2] = ch
    mn[:, 2] -= mn[:, 2] > k
    mn[:, 3] -= mn[:, 3] > k
    mroot = root - (root > k)
    with pytest.raises(A.TreeError, match="leaf size"):
        A.check_tree(f, mpl, boxes, ml, mn, mroot)
    # the plain form: a leaf record dropped, the nodes kept
    _rejected(f, mpl, boxes, ml, nodes, root)


def test_checker_rejects_box_one_ulp_inwards(oracle):
    f, mpl, boxes, leaves, nodes, root, _ = _valid(oracle)
    fl = nodes.view(F32)
    for j, col in ((0, 4), (len(nodes) // 3, 9), (root, 12), (len(nodes) - 1, 15), (7, 10), (9, 5)):
        m = nodes.copy()
        is_top = col in (5, 7, 9, 11, 13, 15)        # {bx, tx, by, ty} x 2, {bz, tz} x 2
        m.view(F32)[j, col] = np.nextafter(fl[j, col], F32(-np.inf if is_top else np.inf))
        assert m.view(U32)[j, col] != nodes.view(U32)[j, col]
        _rejected(f, mpl, boxes, leaves, m, root)


def test_checker_rejects_shared_child(oracle):
    f, mpl, boxes, leaves, nodes, root, _ = _valid(oracle)
    m = nodes.copy()
    m[3, 0] = m[10, 1]
    _rejected(f, mpl, boxes, leaves, m, root)


def test_checker_rejects_other_root(oracle):
    f, mpl, boxes, leaves, nodes, root, _ = _valid(oracle)
    for r in (root + 1, root - 1, 0 if root else 1, -1, len(nodes)):
        _rejected(f, mpl, boxes, leaves, nodes, r)


def _rotate_left(nodes, root, p):
    """Node p's right child j takes p's place and p becomes j's left child, boxes and ranges kept
    right: the tree the build would give if, of two equal deltas, the right one won."""
    m = nodes.copy()
    j = int(m[p, 1])
    new_right = A.child_box(nodes, j, False)                 # j's left subtree goes under p
    m[p, 1] = nodes[j, 0]; m[p, 3] = j
    A.set_child_box(m, p, True, new_right)
    lo = np.minimum(A.child_box(nodes, p, False)[:3].view(F32), new_right[:3].view(F32))
    hi = np.maximum(A.child_box(nodes, p, False)[3:].view(F32), new_right[3:].view(F32))
    m[j, 0] = p; m[j, 2] = nodes[p, 2]
    A.set_child_box(m, j, False, np.concatenate([lo, hi]).view(U32))
    if p == root:
        return m, j
    slot = np.argwhere(nodes[:, :2] == p)[0]
    m[slot[0], slot[1]] = j
    return m, root


@pytest.mark.parametrize("pattern", [("few",), ("equal",), ("plateau", 65, 0)], ids=A.pattern_id)
def test_checker_rejects_the_other_side_of_a_tie(oracle, pattern):
    f, mpl, boxes, leaves, nodes, root, ld = _valid(oracle, pattern, mpl=1)
    N = len(nodes)
    d = ld[1:]
    p_all = np.flatnonzero(nodes[:, 1] < N)
    tied = [int(p) for p in p_all if d[p] == d[nodes[p, 1]]]
    assert tied
    for p in tied[:10] + tied[-3:]:
        m, r = _rotate_left(nodes, root, p)
        with pytest.raises(A.TreeError, match="parent in|merge rule"):
            A.check_tree(f, mpl, boxes, leaves, m, r)


def test_the_rotation_is_the_tree_of_a_larger_right_delta(oracle):
    """All deltas equal: node 0 is the root and node 1 its right child.  With node 1's delta one
    float larger, the rotated tree is the right one: the rotation is well formed, and what the
    checker rejects above is the tie rule alone."""
    f, mpl, boxes, leaves, nodes, root, _ = _valid(oracle, ("equal",), mpl=1)
    assert root == 0 and nodes[0, 1] == 1
    m, r = _rotate_left(nodes, root, 0)
    g = f.copy()
    g[2] = np.nextafter(g[2], F32(np.inf))
    rn, rl, rr, _ = oracle.albvh(A.spheres(N_LEAF), g, 1)
    assert r == rr == 1 and np.array_equal(m, rn) and np.array_equal(leaves, rl)
    A.check_tree(g, mpl, boxes, leaves, m, r)
