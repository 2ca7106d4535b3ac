"""The restatement of the tree gravity (gravity_cases.py) against itself, and every scene of test_gravity.py
against the preconditions it is used for.  Trees come from the CPU oracle's ALBVH.  No GPU.

Accuracy is not tested: the errors against an fp64 direct sum are measured by
profiles/recipes/gravity_points.py and recorded in DESIGN.md."""
import numpy as np
import pytest

import gravity_cases as G

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _scene(name, mpl, oracle):
    s, nodes, leaves, root = G.cpu_tree(G.SCENES[name](), mpl)
    m = G.masses_for(len(s))
    return s, nodes, leaves, root, m, G.moments(nodes, leaves, root, s, m)


@pytest.mark.parametrize("mpl", G.LEAF_SIZES)
def test_theta_zero_is_the_direct_sum_bit_for_bit(oracle, mpl):
    s, nodes, leaves, root, m, rec = _scene("random", mpl, oracle)
    pts = G.query_points(s, n_random=150, n_centres=80)
    for eps in G.SOFTENINGS:
        out, cnt = G.walk(nodes, leaves, root, s, m, rec, pts, 0.0, eps)
        ref, ref_cnt = G.direct_sum(pts, s, m, eps)
        assert _same(out, ref) and np.array_equal(cnt, ref_cnt), (mpl, eps)
        off = ~np.all(np.isfinite(pts), axis=1)
        assert off.sum() == 4 and np.all(_bits(out[off]) == 0) and np.all(cnt[off] == 0)
        assert np.all(cnt[~off, 0] == 0) and np.all(cnt[~off, 1] == len(s))
    assert np.all(np.isfinite(out))


@pytest.mark.parametrize("name,mpl", [("random", 8), ("clustered", 1), ("lattice", 32)])
def test_the_vectorised_walk_is_the_scalar_recursion(oracle, name, mpl):
    s, nodes, leaves, root, m, rec = _scene(name, mpl, oracle)
    pts = G.query_points(s)
    pts = pts[np.all(np.isfinite(pts), axis=1)][:12]
    for theta, eps in ((0.3, 0.0), (0.7, 0.01), (1000.0, 0.0)):
        out, cnt = G.walk(nodes, leaves, root, s, m, rec, pts, theta, eps)
        for i, p in enumerate(pts):
            o1, c1 = G.walk_point_scalar(nodes, leaves, root, s, m, rec, p, theta, eps)
            assert _same(o1, out[i]) and np.array_equal(c1, cnt[i]), (name, theta, i)
        assert theta < 0.5 or cnt[:, 0].max() > 1


def test_a_hand_written_three_node_tree():
    #            leaf 0        leaf 1        leaf 2        leaf 3
    s = np.array([[0, 0, 0, 9], [1, 0, 0, 9], [4, 2, 0, 9], [5, 0, 0, 9]], F32)
    m = np.array([1, 3, 2, 2], F32)
    nodes = np.zeros((3, 16), np.int32)
    nodes[0, :2] = (1, 2)                                   # the root: nodes 1 and 2
    nodes[1, :2] = (3, 4)                                   # leaves 0 and 1
    nodes[2, :2] = (5, 6)                                   # leaves 2 and 3
    leaves = np.array([[0, 1, 0, 0], [1, 1, 0, 0], [2, 1, 0, 0], [3, 1, 0, 0]], np.int32)
    rec = G.moments(nodes, leaves, 0, s, m)
    c, M32, lo, hi, s0, s1 = G.record_fields(rec)
    assert c.tolist() == [[2.625, 0.5, 0], [0.75, 0, 0], [4.5, 1, 0]] and M32.tolist() == [8, 4, 4]
    assert lo.tolist() == [[0, 0, 0], [0, 0, 0], [4, 0, 0]] and hi.tolist() == [[5, 2, 0], [1, 0, 0], [5, 2, 0]]
    assert s0.tolist() == [0, 0, 2] and s1.tolist() == [4, 2, 4]

    def run(p, theta, eps=0.0):
        return G.walk(nodes, leaves, 0, s, m, rec, np.array([p], F32), theta, eps)

    # from (9, 0, 0): the root has d2min 16, size2 25; node 1 d2min 64, size2 1; node 2 d2min 16, size2 4
    out, cnt = run([9, 0, 0], 1.0)
    assert cnt.tolist() == [[2, 0]]
    assert out[0, 3] == pytest.approx(-(4 / 8.25 + 4 / np.sqrt(21.25)), rel=1e-6)
    assert out[0, 0] == pytest.approx(-(4 / 8.25 ** 2 + 4 * 4.5 / 21.25 ** 1.5), rel=1e-6)
    assert out[0, 1] == pytest.approx(4 * 1.0 / 21.25 ** 1.5, rel=1e-6) and out[0, 2] == 0
    out, cnt = run([9, 0, 0], 0.5)                          # theta2 = 0.25: 4 < 0.25 * 16 is false (strict)
    assert cnt.tolist() == [[1, 2]]
    assert out[0, 3] == pytest.approx(-(4 / 8.25 + 2 / np.sqrt(29) + 2 / 4), rel=1e-6)
    assert run([9, 0, 0], 1.25)[1].tolist() == [[2, 0]]     # 25 < 1.5625 * 16 = 25 is false too
    assert run([9, 0, 0], 1.2500001)[1].tolist() == [[1, 0]]
    assert run([30, 0, 0], 1.0)[1].tolist() == [[1, 0]]     # the root itself
    assert run([5, 1, 0], 1000.0)[1].tolist() == [[1, 2]]   # on the faces of the root's and node 2's boxes
    assert run([5, 1, 0], 0.0)[1].tolist() == [[0, 4]]
    out, cnt = run([1, 0, 0], 0.0, eps=0.5)                 # the self pair contributes nothing, softened or not
    assert cnt.tolist() == [[0, 4]]
    assert out[0, 3] == pytest.approx(-(1 / np.sqrt(1.25) + 2 / np.sqrt(13.25) + 2 / np.sqrt(16.25)), rel=1e-6)
    # the sequential fp64 sum is not a pairwise one: 2^53 + 1 + 1 stays 2^53 term by term
    assert G._running_sums(np.array([[2.0 ** 53, 1.0, 1.0]]))[0] == 2.0 ** 53
    # a massless node: c = lo
    rec0 = G.moments(nodes, leaves, 0, s, np.array([1, 3, 0, 0], F32))
    c0, M0, lo0, _, _, _ = G.record_fields(rec0)
    assert M0.tolist() == [4, 4, 0] and c0[2].tolist() == lo0[2].tolist() == [4, 0, 0]
    assert G.max_stack_entries(nodes, leaves, 0) == 2


def test_mixed_scene_has_one_packet_with_differing_decisions(oracle):
    for name in G.SCENES:
        s, nodes, leaves, root, m, rec = _scene(name, 8, oracle)
        pts, node = G.mixed_points(rec)
        assert node == root and len(pts) == 64                # 64 points in one call are one packet
        acc = G.accepts(*(G.record_fields(rec)[k][node] for k in (2, 3)), pts, 0.7)
        assert 8 < acc.sum() < 56                              # some lanes take the root's monopole, others descend
        _, cnt = G.walk(nodes, leaves, root, s, m, rec, pts, 0.7, 0.0)
        assert np.all(cnt[acc] == (1, 0)) and np.all(cnt[~acc, 0] > 1) and len(np.unique(cnt[:, 0])) > 1


def test_face_scene_has_points_on_faces_and_one_ulp_outside(oracle):
    s, nodes, leaves, root, m, rec = _scene("random", 8, oracle)
    on, outside, which = G.face_points(rec)
    assert len(on) == 48 and root in which
    _, _, lo, hi, _, _ = G.record_fields(rec)
    for p, q, i in zip(on, outside, which):
        d_on, size2 = G.d2min_size2(lo[i], hi[i], p[None, :])
        d_out, _ = G.d2min_size2(lo[i], hi[i], q[None, :])
        assert d_on[0] == 0 and not G.accepts(lo[i], hi[i], p[None, :], G.FACE_THETA)[0]
        assert 0 < d_out[0] < 1e-13 and size2 > 1e-4 and G.accepts(lo[i], hi[i], q[None, :], G.FACE_THETA)[0]
        assert not G.accepts(lo[i], hi[i], q[None, :], 1000.0)[0]
    _, c_on = G.walk(nodes, leaves, root, s, m, rec, on, G.FACE_THETA, 0.0)
    _, c_out = G.walk(nodes, leaves, root, s, m, rec, outside, G.FACE_THETA, 0.0)
    at_root = which == root
    assert np.all(c_out[at_root] == (1, 0)) and np.all(c_on[at_root, 0] > 1)


def _depth(nodes, leaves, root):
    n_nodes, deepest, stack = len(nodes), 0, [(int(root), 1)]
    while stack:
        i, d = stack.pop()
        deepest = max(deepest, d)
        if i < n_nodes:
            stack += [(int(nodes[i, 0]), d + 1), (int(nodes[i, 1]), d + 1)]
    return deepest


def test_deep_scenes_fit_the_stack_under_the_push_rule(oracle):
    s, nodes, leaves, root = G.cpu_tree(G.spine_scene(), 1)
    assert _depth(nodes, leaves, root) > 128 and len(leaves) == 350
    assert G.max_stack_entries(nodes, leaves, root) < 128
    rec = G.moments(nodes, leaves, root, s, G.masses_for(len(s)))
    _, _, lo, hi, s0, s1 = G.record_fields(rec)
    assert np.sum(np.all(lo == hi, axis=1) & (s1 - s0 > 64)) > 0     # size-0 nodes over more than a cluster
    at = np.nonzero(np.all(s[:, :3] == G.SPINE_AT, axis=1))[0]
    assert len(at) == 300 and at.max() - at.min() == 299 and (at.min() >> 6) != (at.max() >> 6)
    for name in G.SCENES:
        for mpl in G.LEAF_SIZES:
            _, nodes, leaves, root = G.cpu_tree(G.SCENES[name](), mpl)
            assert G.max_stack_entries(nodes, leaves, root) < 128, (name, mpl)
    _, nodes, leaves, root = G.cpu_tree(G.clustered_scene(200000, 5), 1)
    assert G.max_stack_entries(nodes, leaves, root) < 128


def test_remaining_scenes_meet_their_preconditions(oracle):
    # packets: 63, 64 and 65 points in three octants, enough points for cells of the first Morton level
    pts = G.packet_points()
    assert len(pts) >= 2048
    octant = (pts[:, 0] > 0.5) * 1 + (pts[:, 1] > 0.5) * 2 + (pts[:, 2] > 0.5) * 4
    assert np.bincount(octant, minlength=8).tolist() == [63, 64, 65, 0, 0, 0, 0, len(pts) - 192]
    assert np.all(np.abs(pts - 0.5) > 0.05)
    # cluster boundaries: leaves of a 200-particle tree that straddle a multiple of 64
    s, nodes, leaves, root = G.cpu_tree(G.random_scene(200, 4), 32)
    first, end = leaves[:, 0], leaves[:, 0] + leaves[:, 1]
    assert np.sum((first >> 6) != ((end - 1) >> 6)) >= 1 and end.max() == 200
    # masses: zeros among them, one leaf without mass, one inner node without mass (c = lo)
    for mpl in G.LEAF_SIZES:
        s, nodes, leaves, root = G.cpu_tree(G.random_scene(), mpl)
        m = G.masses_for(len(s))
        assert np.sum(m == 0) > 20
        rec = G.moments(nodes, leaves, root, s, m)
        m0, node = G.zero_mass_node(G.zero_mass_leaf(m, leaves, len(leaves) // 2), rec)
        c, M32, lo, _, s0, s1 = G.record_fields(G.moments(nodes, leaves, root, s, m0))
        assert M32[node] == 0 and s1[node] - s0[node] >= 2 and np.array_equal(c[node], lo[node])
        assert np.sum(M32 == 0) >= 1 and np.all(np.isfinite(c))
    # the query points: self pairs, far points that accept the root at every theta > 0, four off points
    s, nodes, leaves, root, m, rec = _scene("clustered", 8, oracle)
    pts = G.query_points(s)
    assert 900 < len(pts) < 1100 and np.sum(~np.all(np.isfinite(pts), axis=1)) == 4
    _, cnt = G.walk(nodes, leaves, root, s, m, rec, pts, 0.3, 0.0)
    assert np.sum(np.all(cnt == (1, 0), axis=1)) >= 4
    assert np.sum((pts[:, None, :] == s[None, :, :3]).all(axis=2).any(axis=1)) >= 300
