"""The ALBVH build at its path thresholds and on adversarial deltas, and the trace on the deep trees
such deltas give.

The builder (csrc/albvh.hip) is a reformulation of the reference's algorithm -- run lengths over a
sparse table or a tile of the deltas, ballot words, 32-ary pyramids, nearest-greater searches -- that
must give the reference's tree bit for bit.  The delta patterns of albvh_boundary_cases.py are built
here with hand-given deltas over unsorted random primitives (any deltas give a valid tree over any
primitive order) across every max_per_leaf at which the leaf stage changes kernel or table depth and
every leaf count at which a pyramid gains a level, in every delta type, with both comparators and
every primitive kind.  Every tree is compared bit for bit with the oracle's literal restatement; the
n = 600 trees and one tree per pyramid depth also pass the independent checker."""
import time

import numpy as np
import pytest
import torch

import albvh_boundary_cases as A
from conftest import check_column_densities

pytestmark = pytest.mark.gpu

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64


def _dev(a, cuda):
    a = np.ascontiguousarray(a)
    if a.dtype == U32:
        a = a.view(np.int32)          # torch stores the unsigned deltas as signed words
    elif a.dtype == U64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(cuda)


def _host(tree):
    return tree.nodes.cpu().numpy(), tree.leaves.cpu().numpy(), int(tree.root_index.item())


def _assert_tree(tree, ref, what):
    nodes, leaves, root = _host(tree)
    assert np.array_equal(leaves, ref[1]), ("leaves", what)
    assert root == ref[2], ("root", what)
    assert np.array_equal(nodes, ref[0]), ("nodes", what, np.argwhere(nodes != ref[0])[:4])
    return nodes, leaves, root


# ---- leaf stage ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", A.ALL_PATTERNS, ids=A.pattern_id)
def test_leaf_stage_across_its_paths(gh, oracle, cuda, pattern):
    """max_per_leaf on both sides of 64 / 65 (sparse table -> tiled scans) and 256 / 257 (tiled ->
    untiled), at every change of the table's depth (2/3, 4/5, 8/9, 16/17, 32/33) and at n - 1, over
    one block and a ragged last one (257), three (600) and five (1025), from f32 and u32 deltas."""
    for n in A.LEAF_NS:
        s = A.spheres(n, seed=n)
        ds = _dev(s, cuda)
        boxes = A.sphere_boxes(s)
        both = [A.deltas(pattern, n, t, seed=n) for t in (F32, U32)]
        dev = [_dev(x, cuda) for x in both]
        for mpl in A.leaf_mpls(n) + (n,):
            for x, dx in zip(both, dev):
                tree = gh.Tree(n, mpl, device=cuda)
                if mpl >= n:
                    with pytest.raises(ValueError):
                        gh.ALBVH_sph(ds, dx, tree)
                    continue
                gh.ALBVH_sph(ds, dx, tree)
                got = _assert_tree(tree, oracle.albvh(s, x, mpl), (n, mpl, x.dtype))
                if n == 600 and x.dtype == F32:
                    A.check_tree(x, mpl, boxes, got[1], got[0], got[2])


# ---- node stage ------------------------------------------------------------------------------------
CHECKED_NS = (3, 33, 34, 1026, 32770)       # pyramids of 1, 1 (box: 2), 2, 3 and 4 levels


@pytest.mark.parametrize("pattern", A.NODE_PATTERNS, ids=A.pattern_id)
def test_node_stage_across_pyramid_depths(gh, oracle, cuda, pattern):
    """One primitive per leaf, leaf counts on both sides of 32, 1024 and 32768 nodes: the ascent and
    descent of the nearest-greater searches and of the box unions at the first and last element of
    a block and in ragged last blocks, on balanced trees (random), chains (equal, ascending,
    descending), ties, and -- spike_first, spike_last -- with every node's nearest greater neighbour
    at the far end of the array, so that each search climbs to the top level and comes down in the
    first block or the ragged last one (a top level cut short at 32768 nodes is seen by these at
    32770 leaves; the other patterns need 2^20 for that)."""
    for n in A.NODE_NS:
        s = A.spheres(n, seed=n)
        ds = _dev(s, cuda)
        for t in (F32, U32) if n <= 1027 else (F32,):
            x = A.deltas(pattern, n, t, seed=n)
            tree = gh.Tree(n, 1, device=cuda)
            gh.ALBVH_sph(ds, _dev(x, cuda), tree)
            got = _assert_tree(tree, oracle.albvh(s, x, 1), (n, t))
            if n in CHECKED_NS and t == F32:
                A.check_tree(x, 1, A.sphere_boxes(s), got[1], got[0], got[2])


@pytest.mark.parametrize("pattern", [("random",), ("ascending",)], ids=A.pattern_id)
def test_node_stage_five_pyramid_levels(gh, oracle, cuda, pattern):
    """2^20 + 2 leaves: 2^20 + 1 nodes, five levels.  (Measured on MI355X, build + oracle + copies
    + comparison: see the timings this test prints.)  The checker runs without its per-node Python
    loops here (thorough=False), on the balanced tree only."""
    n = A.HUGE_N
    t0 = time.perf_counter()
    s = A.spheres(n)
    x = A.deltas(pattern, n, F32)
    t1 = time.perf_counter()
    tree = gh.Tree(n, 1, device=cuda)
    gh.ALBVH_sph(_dev(s, cuda), _dev(x, cuda), tree)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    ref = oracle.albvh(s, x, 1)
    t3 = time.perf_counter()
    got = _assert_tree(tree, ref, (n,))
    t4 = time.perf_counter()
    assert A.pyramid_levels(len(got[1]) - 1) == 5
    if pattern == ("random",):
        A.check_tree(x, 1, A.sphere_boxes(s), got[1], got[0], got[2], thorough=False)
    t5 = time.perf_counter()
    print("five levels, %s: inputs %.2f s, upload + build %.2f s, oracle %.2f s, download + compare "
          "%.2f s, checker %.2f s" % (A.pattern_id(pattern), t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4))


# ---- delta types, comparator, primitive kinds ------------------------------------------------------
@pytest.mark.parametrize("pattern", A.TYPE_PATTERNS, ids=A.pattern_id)
def test_delta_types_compare_their_whole_width(gh, oracle, cuda, pattern):
    """f64 deltas that differ from 2^-40 on (a float compare sees them all equal) and u64 deltas
    that differ in the high word only or in the low word only give the tree of their ranks."""
    n = 600
    s = A.spheres(n)
    ds = _dev(s, cuda)
    r = A.ranks(A.deltas(pattern, n, F32))
    wide = [A.f64_from_ranks(r), A.u64_high_from_ranks(r), A.u64_low_from_ranks(r), r]
    for mpl in A.TYPE_MPLS:
        ref = oracle.albvh(s, r, mpl)
        for x in wide:
            dx = _dev(x, cuda)
            t1 = gh.Tree(n, mpl, device=cuda); gh.build_ALBVH(t1, ds, dx)
            t2 = gh.Tree(n, mpl, device=cuda); gh.ALBVH_sph(ds, dx, t2)
            for t in (t1, t2):
                _assert_tree(t, ref, (mpl, x.dtype, x[1]))


@pytest.mark.parametrize("pattern", A.TYPE_PATTERNS, ids=A.pattern_id)
def test_greater_is_less_on_flipped_deltas(gh, oracle, cuda, pattern):
    """COMP_GREATER on d gives the tree of COMP_LESS on flip(d) (negation / bitwise NOT), in all
    four delta types; the reference is the oracle's tree of the ranks of flip(d).  The unsigned
    forms carry the pattern + 1: NOT(0) would be the sentinel."""
    n = 600
    s = A.spheres(n)
    ds = _dev(s, cuda)
    f = A.deltas(pattern, n, F32)
    r1 = A.ranks(f)[1:-1] + U64(1)
    forms = [f, A.f64_from_ranks(A.ranks(f)), A.deltas(pattern, n, U32, offset=1),
             A.finish(r1 << U64(32), U64), A.finish(r1, U64)]
    for mpl in A.TYPE_MPLS:
        for x in forms:
            fx = A.flip(x)
            ref = oracle.albvh(s, A.ranks(fx), mpl)
            tg = gh.Tree(n, mpl, device=cuda)
            gh.build_ALBVH(tg, ds, _dev(x, cuda), delta_comp=gh.COMP_GREATER)
            tl = gh.Tree(n, mpl, device=cuda)
            gh.build_ALBVH(tl, ds, _dev(fx, cuda), delta_comp=gh.COMP_LESS)
            for t in (tg, tl):
                _assert_tree(t, ref, (mpl, x.dtype))
    # the two orders are different trees (the comparator is not ignored)
    if pattern != ("equal",):
        assert not np.array_equal(oracle.albvh(s, A.ranks(A.flip(f)), 1)[0], oracle.albvh(s, f, 1)[0])


@pytest.mark.parametrize("pattern", A.TYPE_PATTERNS, ids=A.pattern_id)
def test_primitive_kinds(gh, oracle, cuda, pattern):
    """double4 spheres, triangles and caller-evaluated boxes under the fast and the tiled leaf
    stage, against the oracle with the matching primitive kind (boxes: the sphere tree, as in
    test_build_from_caller_boxes_equals_sphere_build) and the checker with that kind's boxes."""
    n = 600
    f = A.deltas(pattern, n, F32)
    df = _dev(f, cuda)
    s, tri, d4 = A.spheres(n), A.triangles(n), A.spheres_d4(n)
    cases = [(gh.PRIM_SPHERE_D4, d4, d4, 2, A.sphere_boxes(d4)),
             (gh.PRIM_TRIANGLE, tri, tri, 1, A.triangle_boxes(tri)),
             (gh.PRIM_BOX, A.sphere_boxes(s), s, 0, A.sphere_boxes(s))]
    for mpl in (32, 65):
        for kind, prims, oracle_prims, oracle_kind, boxes in cases:
            tree = gh.Tree(n, mpl, device=cuda)
            gh.build_ALBVH(tree, _dev(prims, cuda), df, kind)
            got = _assert_tree(tree, oracle.albvh(oracle_prims, f, mpl, prim_kind=oracle_kind), (mpl, kind))
            A.check_tree(f, mpl, boxes, got[1], got[0], got[2])


# ---- geometry-driven ties through the whole pipeline -----------------------------------------------
@pytest.mark.parametrize("name", A.TIE_SCENES)
def test_build_tree_on_tied_geometry(gh, oracle, cuda, name):
    """Keys, stable sort, Euclidean deltas and build on a lattice, on coincident spheres, on
    collinear centres with growing spacing and on two positions: sorted spheres, leaves, nodes and
    root are the oracle pipeline's."""
    s = A.tie_scene(name)
    n = len(s)
    keys = oracle.morton_keys30(s, (0, 0, 0), (1, 1, 1))
    _, ss, _ = oracle.sort_by_key(keys, s)
    ss = np.ascontiguousarray(ss)
    deltas = oracle.deltas_euclid(ss)
    for mpl in (1, 32, 65):
        d = _dev(s, cuda)
        tree = gh.Tree(n, mpl, device=cuda)
        gh.build_tree(d, tree, (0, 0, 0), (1, 1, 1))
        assert np.array_equal(d.cpu().numpy().view(U32), ss.view(U32)), ("sorted spheres", mpl)
        _assert_tree(tree, oracle.albvh(ss, deltas, mpl), (name, mpl))


# ---- traces of deep trees --------------------------------------------------------------------------
CHAINS = (("ascending",), ("descending",), ("equal",))


def _is_overflow(gh, err):
    return str(err).startswith("status %d:" % gh.GRACE_STACK_OVERFLOW)


class _Line:
    def __init__(self, gh, oracle, cuda, n, pattern):
        self.s, self.rays_h = A.line_scene(n)
        self.d, self.rays = _dev(self.s, cuda), _dev(self.rays_h, cuda)
        self.tree = gh.Tree(n, 1, device=cuda)
        gh.ALBVH_sph(self.d, _dev(A.deltas(pattern, n, F32), cuda), self.tree)
        self.counts = oracle.brute_hitcounts(self.rays_h, self.s)
        self.c32, self.c64 = oracle.brute_cumulative(self.rays_h, self.s)
        self.max_term = 1.91 / float(self.s[:, 3].min()) ** 2
        assert np.all(self.counts[:32] == n) and np.all(self.counts[32:] == 1)


def _trace_line(gh, cuda, line, mode, may_overflow):
    """Both traces with check=True.  Each returns exactly the brute-force result or (may_overflow
    only) raises GRACE_STACK_OVERFLOW; returns the number of calls that raised."""
    raised = 0
    for which in ("counts", "cumulative"):
        try:
            if which == "counts":
                out = torch.full((64,), -7, dtype=torch.int32, device=cuda)
                gh.trace_hitcounts_sph(line.rays, line.d, line.tree, out, check=True)
                assert np.array_equal(out.cpu().numpy(), line.counts)
            else:
                out = torch.full((64,), -7.0, dtype=torch.float32, device=cuda)
                gh.trace_cumulative_sph(line.rays, line.d, line.tree, out, check=True)
                check_column_densities(out.cpu().numpy(), line.c32, line.c64, mode, line.max_term)
        except gh.GraceError as err:
            assert may_overflow and _is_overflow(gh, err), err
            raised += 1
    return raised


@pytest.mark.parametrize("pattern", CHAINS, ids=A.pattern_id)
def test_trace_on_chains(gh, oracle, cuda, integral_mode, pattern):
    """Spheres on a line under a chain of a tree (one sphere per leaf), 32 rays along the line and
    32 across it in one general packet, hit counts and column densities with check=True, with and
    without ray reordering and a prepared scene, with the automatic treelet size (a subtree of up to
    8192 spheres is swept, not walked: these trees never touch the stack) and with treelets off (the
    walk alone).

    100 spheres: the chain fits the 128-entry packet stack; exact, no error.
    300 spheres, right-deep chains (descending, equal deltas): the walk pops the chain's next node
    right after pushing it; exact, no error.
    300 spheres, left-deep chain (ascending deltas): the pending right leaves pile up.  Each call
    either returns exactly the brute-force result or raises GRACE_STACK_OVERFLOW, never other
    numbers.  The current code returns exact results with automatic treelets and raises with
    treelets off (asserted below, so that a change of either is seen).  After a raised overflow the
    same calls on the 100-sphere tree are exact: the status word is cleared, nothing prepared is
    poisoned."""
    small = _Line(gh, oracle, cuda, 100, pattern)
    big = _Line(gh, oracle, cuda, 300, pattern)
    left_deep = pattern == ("ascending",)
    try:
        for treelet in (-1, 0):
            for reorder in (True, False):
                for prepare in (False, True):
                    gh.set_treelet_size(treelet)
                    gh.set_ray_reorder(reorder)
                    for line in (small, big):
                        if prepare:
                            gh.trace_prepare(line.d, line.tree)
                        raised = _trace_line(gh, cuda, line, integral_mode, left_deep and line is big)
                        if raised:
                            # at once, the overflowed scene still prepared: the small tree is exact
                            assert _trace_line(gh, cuda, small, integral_mode, False) == 0
                        if left_deep and line is big:
                            assert raised == (2 if treelet == 0 else 0), (treelet, reorder, prepare, raised)
                        if prepare:
                            gh.trace_release()
                    assert _trace_line(gh, cuda, small, integral_mode, False) == 0
        gh.trace_status()                     # nothing left behind in the status word
    finally:
        gh.set_treelet_size(-1)
        gh.set_ray_reorder(True)
        gh.trace_release()
