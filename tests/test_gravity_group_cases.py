"""The restatement of the gravity within groups (gravity_group_cases.py) against itself and against
gravity_cases.py, and the scenes and labellings of test_gravity_groups.py against the preconditions that give
its GPU tests their meaning.  Trees come from the CPU oracle's ALBVH.  No GPU."""
import numpy as np
import pytest

import gravity_cases as G
import gravity_group_cases as GG

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


_cache = {}


def _case(scene, labelling, mpl, oracle):
    """A scene on the oracle's tree under a labelling: everything the walk takes, the query points, and the
    events of one walk at theta 0.7 (computed once)."""
    key = (scene, labelling, mpl)
    if key not in _cache:
        s, nodes, leaves, root = G.cpu_tree(G.SCENES[scene](), mpl)
        m = G.masses_for(len(s))
        lab = GG.LABELLINGS[labelling](s)
        rec, ranges = GG.group_moments(nodes, leaves, root, s, m, lab)
        pts = G.query_points(s)
        pl = GG.point_labels(labelling, pts)
        stats = {}
        out, cnt = GG.group_walk(nodes, leaves, root, s, m, lab, rec, ranges, pts, pl, 0.7, 0.0, stats=stats)
        _cache[key] = dict(s=s, nodes=nodes, leaves=leaves, root=root, m=m, lab=lab, rec=rec, ranges=ranges, pts=pts,
                           pl=pl, stats=stats, out=out, cnt=cnt, tree=(nodes, leaves, root, s, m, lab, rec, ranges))
    return _cache[key]


# ---- the restatement against itself -------------------------------------------------------------------
@pytest.mark.parametrize("scene,labelling,mpl", [("clustered", "lonely", 8), ("random", "scatter", 1),
                                                 ("lattice", "slabs", 32)])
def test_the_vectorised_walk_is_the_scalar_recursion(oracle, scene, labelling, mpl):
    c = _case(scene, labelling, mpl, oracle)
    ok = np.nonzero(np.all(np.isfinite(c["pts"]), axis=1) & (c["pl"] >= 0))[0][:12]
    pts, pl = c["pts"][ok], c["pl"][ok]
    for theta, eps in ((0.3, 0.0), (0.7, 0.01), (1000.0, 0.0)):
        out, cnt = GG.group_walk(*c["tree"], pts, pl, theta, eps)
        for i in range(len(pts)):
            o1, c1 = GG.group_walk_point_scalar(*c["tree"], pts[i], pl[i], theta, eps)
            assert _same(o1, out[i]) and np.array_equal(c1, cnt[i]), (scene, theta, i)


@pytest.mark.parametrize("scene,mpl", [("random", 8), ("clustered", 1), ("lattice", 32)])
def test_one_label_everywhere_is_the_open_contract(oracle, scene, mpl):
    c = _case(scene, "single", mpl, oracle)
    ref_rec = G.moments(c["nodes"], c["leaves"], c["root"], c["s"], c["m"])
    assert _same(c["rec"], ref_rec)
    assert np.all(c["ranges"] == 0) and c["ranges"].dtype == np.int32
    for theta, eps in ((0.0, 0.01), (0.7, 0.0)):
        got = GG.group_walk(*c["tree"], c["pts"], c["pl"], theta, eps)
        ref = G.walk(c["nodes"], c["leaves"], c["root"], c["s"], c["m"], ref_rec, c["pts"], theta, eps)
        assert _same(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (scene, theta)
    # any other value >= 0 does as well: label values matter only through equality and order
    lab5 = np.full(len(c["s"]), 5, np.int32)
    rec5, ranges5 = GG.group_moments(c["nodes"], c["leaves"], c["root"], c["s"], c["m"], lab5)
    assert _same(rec5, ref_rec) and np.all(ranges5 == 5)


@pytest.mark.parametrize("scene,labelling,mpl", [("clustered", "lonely", 1), ("random", "scatter", 8),
                                                 ("clustered", "blobs", 32), ("lattice", "slabs", 8)])
def test_theta_zero_is_the_masked_direct_sum_per_label(oracle, scene, labelling, mpl):
    c = _case(scene, labelling, mpl, oracle)
    pts, pl = c["pts"][:300], c["pl"][:300]
    for eps in G.SOFTENINGS:
        out, cnt = GG.group_walk(*c["tree"], pts, pl, 0.0, eps)
        ref, ref_cnt = GG.masked_direct_sum(pts, pl, c["s"], c["m"], c["lab"], eps)
        assert _same(out, ref) and np.array_equal(cnt, ref_cnt), (scene, labelling, eps)
        members = np.array([np.sum(c["lab"] == L) if L >= 0 else 0 for L in pl])
        on = np.all(np.isfinite(pts), axis=1) & (pl >= 0)
        assert np.all(cnt[on, 0] == 0) and np.array_equal(cnt[on, 1], members[on])
        assert np.all(_bits(out[~on]) == 0) and np.all(cnt[~on] == 0)


def test_a_hand_written_three_node_tree_with_labels():
    #            leaf 0        leaf 1        leaf 2        leaf 3
    s = np.array([[0, 0, 0, 9], [1, 0, 0, 9], [4, 2, 0, 9], [5, 0, 0, 9]], F32)
    m = np.array([1, 3, 2, 2], F32)
    nodes = np.zeros((3, 16), np.int32)
    nodes[0, :2] = (1, 2)
    nodes[1, :2] = (3, 4)
    nodes[2, :2] = (5, 6)
    leaves = np.array([[0, 1, 0, 0], [1, 1, 0, 0], [2, 1, 0, 0], [3, 1, 0, 0]], np.int32)
    lab = np.array([4, 4, -1, 6], np.int32)
    rec, ranges = GG.group_moments(nodes, leaves, 0, s, m, lab)
    c, M32, lo, hi, s0, s1 = G.record_fields(rec)
    assert ranges.tolist() == [[4, 6], [4, 4], [6, 6]]
    assert M32.tolist() == [6, 4, 2] and c.tolist() == [[float(F32(13 / 6)), 0, 0], [0.75, 0, 0], [5, 0, 0]]   # no sphere 2
    assert lo.tolist() == [[0, 0, 0], [0, 0, 0], [5, 0, 0]] and hi.tolist() == [[5, 0, 0], [1, 0, 0], [5, 0, 0]]
    assert s0.tolist() == [0, 0, 2] and s1.tolist() == [4, 2, 4]                    # ... but keeps its index

    def run(p, L, theta, eps=0.0):
        return GG.group_walk(nodes, leaves, 0, s, m, lab, rec, ranges, np.array([p], F32), np.array([L]), theta, eps)

    out, cnt = run([30, 0, 0], 4, 1.0)                     # the root is far enough but holds two labels: opened;
    assert cnt.tolist() == [[1, 0]]                        # node 1 is pure 4: one term; node 2 is passed by
    assert out[0, 3] == pytest.approx(-4 / 29.25, rel=1e-6)
    out, cnt = run([30, 0, 0], 6, 1.0)                     # node 2 has size 0 (one labelled sphere): accepted
    assert cnt.tolist() == [[1, 0]] and out[0, 3] == pytest.approx(-2 / 25, rel=1e-6)
    assert run([30, 0, 0], 5, 1.0)[1].tolist() == [[0, 0]]  # inside the root's range only: no term at all
    out, cnt = run([30, 0, 0], 5, 1.0)
    assert _bits(out).tolist() == [[0, 0, 0, 1 << 63]]     # phi = -0
    assert run([30, 0, 0], 7, 1.0)[1].tolist() == [[0, 0]] and run([30, 0, 0], 3, 1.0)[1].tolist() == [[0, 0]]
    out, cnt = run([30, 0, 0], -1, 1.0)                    # a negative point label: +0 throughout
    assert cnt.tolist() == [[0, 0]] and np.all(_bits(out) == 0)
    out, cnt = run([0.5, 0, 0], 4, 0.0)                    # theta 0: the label's members
    assert cnt.tolist() == [[0, 2]] and out[0, 3] == pytest.approx(-(1 / 0.5 + 3 / 0.5), rel=1e-6)
    # an unbinding pass: sphere 1 leaves
    lab2 = np.array([4, -1, -1, 6], np.int32)
    rec2, ranges2 = GG.group_moments(nodes, leaves, 0, s, m, lab2)
    assert ranges2.tolist() == [[4, 6], [4, 4], [6, 6]] and G.record_fields(rec2)[1].tolist() == [3, 1, 2]
    # nobody labelled below node 2
    rec3, ranges3 = GG.group_moments(nodes, leaves, 0, s, m, np.array([4, 4, -1, -1], np.int32))
    c3, M3, lo3, hi3, _, _ = G.record_fields(rec3)
    assert ranges3.tolist() == [[4, 4], [4, 4], [GG.INT_MAX, -1]] and M3.tolist() == [4, 4, 0]
    assert np.all(lo3[2] == np.inf) and np.all(hi3[2] == -np.inf) and np.all(c3[2] == np.inf)


# ---- the preconditions of the GPU tests ---------------------------------------------------------------
def test_an_inner_node_without_a_labelled_primitive(oracle):
    c = _case("clustered", "blobs", 1, oracle)
    empty = c["ranges"][:, 1] < 0
    assert empty.sum() > 10 and np.all(c["ranges"][empty, 0] == GG.INT_MAX)
    _, M32, lo, hi, s0, s1 = G.record_fields(c["rec"])
    assert np.all(M32[empty] == 0) and np.all(lo[empty] == np.inf) and np.all(hi[empty] == -np.inf)
    assert np.all(s1[empty] - s0[empty] >= 2)              # the spans still cover every primitive
    assert len(c["stats"]["empty"]) > 0                    # and some point's descent reaches one
    assert np.sum(c["lab"] < 0) > 100 and np.sum(c["lab"] >= 0) > 1500
    # the whole tree without a label: the random scene lies outside every blob
    c = _case("random", "blobs", 8, oracle)
    assert np.all(c["lab"] == -1) and np.all(c["ranges"] == (GG.INT_MAX, -1)) and np.all(c["cnt"] == 0)


def test_pure_nodes_are_accepted_and_pure_nodes_of_other_labels_are_met(oracle):
    for scene, labelling, mpl in (("clustered", "blobs", 8), ("random", "slabs", 1), ("lattice", "scatter", 1)):
        c = _case(scene, labelling, mpl, oracle)
        assert len(c["stats"]["pure_accepted"]) > 0 and c["cnt"][:, 0].sum() > 0, (scene, labelling)
        assert len(c["stats"]["pure_other"]) > 0, (scene, labelling)
    # mixed nodes are never monopoles: no pure node, no node term, however far the point
    c = _case("clustered", "scatter", 32, oracle)
    assert np.all(c["ranges"][:, 0] != c["ranges"][:, 1]) and np.all(c["cnt"][:, 0] == 0)
    out, cnt = GG.group_walk(*c["tree"], c["pts"], c["pl"], 1000.0, 0.0)
    assert np.all(cnt[:, 0] == 0) and cnt[:, 1].sum() > 0


def test_a_mixed_node_that_only_its_range_lets_a_point_into(oracle):
    for scene, labelling, mpl in (("random", "scatter", 1), ("clustered", "scatter", 8), ("clustered", "lonely", 32)):
        c = _case(scene, labelling, mpl, oracle)
        assert len(c["stats"]["range_only"]) > 0, (scene, labelling, mpl)
        node = c["stats"]["range_only"][0][0]
        assert c["ranges"][node, 0] < c["ranges"][node, 1]


def test_leaf_ranges_with_two_labels_across_a_cluster_boundary(oracle):
    for scene, labelling in (("random", "slabs"), ("random", "scatter"), ("clustered", "scatter")):
        hits = 0
        c = _case(scene, labelling, 32, oracle)
        first, end = c["leaves"][:, 0], c["leaves"][:, 0] + c["leaves"][:, 1]
        for l in np.nonzero((first >> 6) != ((end - 1) >> 6))[0]:
            inside = c["lab"][first[l]:end[l]]
            hits += len(np.unique(inside[inside >= 0])) >= 2
        assert hits > 0, (scene, labelling)
    # the merged ranges of the spine: 300 coincident centres, one leaf each, two labels interleaved
    s, nodes, leaves, root = G.cpu_tree(G.spine_scene(), 1)
    lab = GG.spine_labels(s)
    at = np.nonzero(np.all(s[:, :3] == G.SPINE_AT, axis=1))[0]
    assert len(at) == 300 and at.max() - at.min() == 299 and (at.min() >> 6) != (at.max() >> 6)
    run = lab[at.min():at.max() + 1]
    assert 100 < run.sum() < 200 and np.sum(run[1:] != run[:-1]) > 100
    assert G.max_stack_entries(nodes, leaves, root) < 128  # the labelled walk pushes as the open one does


def test_one_packet_with_three_labels_and_differing_decisions_at_one_node(oracle):
    for scene, labelling, mpl in (("clustered", "blobs", 8), ("random", "slabs", 8), ("clustered", "lonely", 1)):
        c = _case(scene, labelling, mpl, oracle)
        pts, pl, node = GG.mixed_label_packet(c["rec"], c["ranges"])
        assert len(pts) == 64 and len(np.unique(pl)) == 3     # 64 points in one call are one packet
        A = int(c["ranges"][node, 0])
        assert A == c["ranges"][node, 1] and A >= 0
        _, _, lo, hi, s0, s1 = G.record_fields(c["rec"])
        acc = G.accepts(lo[node], hi[node], pts, 0.7)
        mine = pl == A
        assert 2 < np.sum(acc & mine) < mine.sum() - 2, (scene, labelling)   # lanes that accept, lanes that open,
        assert np.sum(~mine) > 40                                               # and lanes that pass by
        st = {}
        out, cnt = GG.group_walk(*c["tree"], pts, pl, 0.7, 0.0, stats=st)
        took = dict(st["pure_accepted"]).get(node, 0)
        assert took == np.sum(acc & mine)                     # the packet reaches the node itself
        assert len(np.unique(cnt[mine], axis=0)) > 1


def test_point_labels_cover_negative_absent_and_lonely(oracle):
    c = _case("clustered", "lonely", 8, oracle)
    assert np.sum(c["lab"] == GG.LONELY) == 1 and np.sum(c["lab"] == GG.ABSENT) == 0
    lonely, absent = c["pl"] == GG.LONELY, c["pl"] == GG.ABSENT
    finite = np.all(np.isfinite(c["pts"]), axis=1)
    assert lonely.sum() >= 15 and absent.sum() >= 15
    out, cnt = GG.group_walk(*c["tree"], c["pts"], c["pl"], 0.0, 0.0)
    assert np.all(cnt[lonely & finite] == (0, 1)) and np.all(cnt[absent] == 0)
    assert np.all(_bits(out[absent & finite]) == np.array([0, 0, 0, 1 << 63], np.uint64))   # no term: phi = -0
    c = _case("random", "scatter", 8, oracle)
    assert np.sum(c["pl"] < 0) > 100 and np.all(c["cnt"][c["pl"] < 0] == 0) and np.all(_bits(c["out"][c["pl"] < 0]) == 0)
