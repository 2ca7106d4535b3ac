"""The periodic point queries across the point counts at which the front end changes behaviour, on a
clustered scene that fills the periodic cell and straddles its seam.

Which path a packet of a periodic walk takes -- the box and its two images per axis or the box alone
(`images`), the survivor loop with wrap_sep or without (`narrow` / `plain`, the interpolation's NoWrap
interval), a neighbour lane that has become "everything" (periodic_bounds) -- depends on how the points are
cut into packets and on how wide a packet's box is against h = fl(L / 2).  The matrix of
periodic_packet_scenes.py varies exactly that: the open module's point sets (both layouts, both sides of
the cell-level steps at 2048 and 16384 points, 131073 pooled points) on the root box of torus_scene, in a
cube and in an anisotropic slab with an open axis, once far from the origin.  test_periodic_packet_scenes.py
proves on the CPU which classes of packet each case holds.

Every output slot of every family is compared bit for bit with the NumPy restatement of the contract
(include/grace_hip.h, "Periodic boxes": periodic_query_scenes.py, periodic_point_scenes.py), computed on the
records and expanded by the point sets' index maps; output buffers are pre-filled with values the contract
cannot produce (-7, a NaN with a payload).  There is no tolerance anywhere."""
import numpy as np
import pytest

import periodic_packet_scenes as T
import periodic_point_scenes as PS
import periodic_query_scenes as S
from test_fof import restate_catalogue
from test_periodic_queries import _build
from test_point_query_packets import (EDGES, K_LARGE, K_SMALL, R_SHARED, _dev, _eq, _f32, _i32, expand_lists,
                                      in_own_context, inputs, run_counts, run_field, run_knn, run_lists, run_pairs,
                                      weights)
from test_range_queries import restate_sums
from test_sph_interpolation import lattice as grid_points
from test_sph_interpolation import restate as restate_field

F32 = np.float32
CUBE = S.BOXES["cube"]
FAMILIES = ("counts", "lists", "knn", "field", "pairs")
SELF_CASES = [("cube", n) for n in (2047, 2048, 2049, 16383, 16384, 16385)] + [("slab", 2049), ("slab", 16385)]
CONTEXT_CASE = ("cube", 2049, "spread", 0.0)
MPL1_CASE = ("cube", 16385, "clumped", 0.0)


# ---- references, computed once per (case, family) ------------------------------------------------------
_ref_cache = {}


def reference(case, sh, what):
    """The restatement of family `what` on the records of the case's point set against the spheres sh (tree
    order), on the torus of the case's box."""
    key = (case, what)
    if key in _ref_cache:
        return _ref_cache[key]
    ps, period = T.case_points(case), S.BOXES[case[0]]
    P, r = ps.rec_points, ps.rec_radii
    with np.errstate(all="ignore"):
        if what == "lists":
            res = S.restate(P, r, sh, period)
        elif what == "shared":
            res = S.restate(P, np.full(len(P), R_SHARED, F32), sh, period)[0]
        elif what.startswith("sums:"):
            res = restate_sums(P, r, sh, weights(len(sh), 5), what[5:], reference(case, sh, "lists"))
        elif what == "knn":                                          # k = 64; every smaller k is its rows' head
            res = PS.knn(P, sh, K_LARGE, period)
        elif what == "field":
            res = restate_field(len(P), PS.pairs(P, sh, period), sh, weights(len(sh), 2), "cubic")[:2]
        elif what == "pairs":
            res = S.restate_bins(P, EDGES, sh, period, weights(len(sh), 2))
        else:
            raise KeyError(what)
    _ref_cache[key] = res
    return res


def check_counts(case, sh, got, kernel="cubic", shared=False):
    ps = T.case_points(case)
    if shared:
        _eq(got[0], reference(case, sh, "shared")[ps.index], (case, "shared radius"))
        return
    _eq(got[0], reference(case, sh, "lists")[0][ps.index], (case, "counts"))
    _eq(got[1], reference(case, sh, "sums:" + kernel)[ps.index], (case, "sums", kernel))


def total_of(case, sh):
    return int(reference(case, sh, "lists")[0][T.case_points(case).index].astype(np.int64).sum())


def check_lists(case, sh, got):
    ref = expand_lists(reference(case, sh, "lists"), T.case_points(case).index)
    _eq(got[0], ref[0], (case, "lists", "counts"))
    assert got[1] is not None and np.array_equal(got[1].astype(np.int64), ref[1]), (case, "offsets")
    _eq(got[2], ref[2], (case, "lists", "indices"))
    _eq(got[3], ref[3], (case, "lists", "d2"))


def check_knn(case, sh, got, k):
    ps = T.case_points(case)
    ref_i, ref_d = reference(case, sh, "knn")
    _eq(got[0], np.ascontiguousarray(ref_i[ps.index, :k]), (case, "knn indices", k))
    _eq(got[1], np.ascontiguousarray(ref_d[ps.index, :k]), (case, "knn d2", k))
    off = ps.off_at[::6]                                            # the padding rows of a non-finite point
    assert np.all(got[0][off] == -1) and np.all(np.isposinf(got[1][off]))


def check_field(case, sh, got):
    ps = T.case_points(case)
    out, counts = reference(case, sh, "field")
    _eq(got[1], counts[ps.index], (case, "field counts"))
    _eq(got[0], out[ps.index], (case, "field"))


def check_pairs(case, sh, got):
    ps = T.case_points(case)
    _, counts, sums = reference(case, sh, "pairs")
    tot, cnt, sm = got
    ref_tot = counts[ps.index].sum(axis=0, dtype=np.int64).astype(np.uint64)
    assert tot.dtype == np.uint64 and np.array_equal(tot, ref_tot), (case, "totals", tot, ref_tot)
    _eq(cnt, counts[ps.index], (case, "pair counts"))
    _eq(sm, sums[ps.index], (case, "pair sums"))


def differs(a, b):
    """The number of 32-bit slots in which two results differ."""
    return int(np.sum(np.asarray(a).reshape(-1).view(np.uint32) != np.asarray(b).reshape(-1).view(np.uint32)))


def wraps_in_reach(case, sh, what):
    """Whether the restatement of `what` ("field": containment; "pairs": within the last edge) holds a pair whose
    separation wraps -- that is, whether the periodic result can differ from the open call's at all (a point
    set that stays away from the faces, such as the clumped layout below 16384 points, sees no image of a
    sphere of H <= 0.04 Lmin).  The periodic pair set holds the open one (a pair the open call has lies within
    H or the last edge, below half a period: it does not wrap), so it is larger exactly when some pair wraps;
    only the records within reach of a face (of the centres' range moved by a period) need the open count."""
    key = (case, "wraps:" + what)
    if key in _ref_cache:
        return _ref_cache[key]
    from test_range_queries import restate as open_lists
    from test_sph_interpolation import pairs as open_pairs
    ps, period = T.case_points(case), S.BOXES[case[0]]
    P = ps.rec_points
    reach = float(sh[:, 3].max() if what == "field" else EDGES[-1])
    near = np.zeros(len(P), bool)
    with np.errstate(invalid="ignore"):
        for a, L in enumerate(period):
            if L > 0:
                slack = reach + 1e-5 * L
                near |= (P[:, a] <= sh[:, a].max() - L + slack) | (P[:, a] >= sh[:, a].min() + L - slack)
    near &= np.all(np.isfinite(P), axis=1)
    if not near.any():
        _ref_cache[key] = False
        return False
    if what == "field":
        torus = reference(case, sh, "field")[1][near].astype(np.int64).sum()
        plain = len(open_pairs(P[near], sh)[0])
    else:
        torus = reference(case, sh, "pairs")[1][near].astype(np.int64).sum()
        plain = open_lists(P[near], np.full(int(near.sum()), EDGES[-1], F32), sh)[0].astype(np.int64).sum()
    assert torus >= plain
    _ref_cache[key] = bool(torus > plain)
    return _ref_cache[key]


def run_family(gh, family, case, inp, d, tree, sh, cuda, period):
    """One family's call(s) on the current context and stream, checked against the restatement."""
    if family == "counts":
        check_counts(case, sh, run_counts(gh, inp, d, tree, cuda, shared=True, period=period), shared=True)
        check_counts(case, sh, run_counts(gh, inp, d, tree, cuda, period=period))
    elif family == "lists":
        check_lists(case, sh, run_lists(gh, inp, d, tree, cuda, total_of(case, sh), period=period))
    elif family == "knn":
        check_knn(case, sh, run_knn(gh, inp, d, tree, cuda, K_SMALL, period=period), K_SMALL)
    elif family == "field":
        check_field(case, sh, run_field(gh, inp, d, tree, cuda, period=period))
    elif family == "pairs":
        check_pairs(case, sh, run_pairs(gh, inp, d, tree, cuda, period=period))
    else:
        raise KeyError(family)


# ---- GPU --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(gh, cuda):
    """case, max_per_leaf -> (spheres in tree order, tree, the spheres on the host, period); each scene is built
    once, at max_per_leaf 8 and 1, with the same tree order."""
    built = {}

    def get(case, mpl=8):
        key = (case[0], case[3])
        if key not in built:
            s, _, _ = T.case_scene(*key)
            trees = {k: _build(gh, s, cuda, k) for k in (8, 1)}
            assert np.array_equal(trees[1][2], trees[8][2])
            built[key] = trees
        d, tree, sh = built[key][mpl]
        return d, tree, sh, S.BOXES[case[0]]
    return get


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


@pytest.mark.gpu
@pytest.mark.parametrize("key", [("cube", 0.0), ("slab", 0.0), ("cube", 100.0)])
def test_the_restated_root_box_is_the_trees(gh, scenes, key, cuda):
    """A condition on the census, not on a result: the box packet_keys_kernel reads from the root node is the
    restated one to within 4 ulp of its largest coordinate -- far inside the margins of the point sets and of
    the census's band."""
    s, lo, hi = T.case_scene(*key)
    ulp = np.spacing(F32(max(np.abs(lo).max(), np.abs(hi).max())))
    for mpl in (8, 1):
        d, tree, sh, _ = scenes((key[0], 0, "", key[1]), mpl)
        root = int(tree.root_index.cpu()[0])
        node = tree.nodes[root].cpu().numpy().view(F32).reshape(4, 4)
        L, R, Z = node[1], node[2], node[3]
        t_lo = np.array([min(L[0], R[0]), min(L[2], R[2]), min(Z[0], Z[2])], F32)
        t_hi = np.array([max(L[1], R[1]), max(L[3], R[3]), max(Z[1], Z[3])], F32)
        assert np.all(np.abs(t_lo - lo) <= 4 * ulp) and np.all(np.abs(t_hi - hi) <= 4 * ulp), (t_lo, lo, t_hi, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_range_counts_and_gather_sums(gh, scenes, case, cuda, kernel_reset):
    d, tree, sh, period = scenes(case)
    ps = T.case_points(case)
    inp = inputs(ps, sh, cuda)
    check_counts(case, sh, run_counts(gh, inp, d, tree, cuda, shared=True, period=period), shared=True)
    got = run_counts(gh, inp, d, tree, cuda, period=period)
    check_counts(case, sh, got)
    if case[1] == 16385:
        gh.set_sph_kernel("wendland_c2")
        check_counts(case, sh, run_counts(gh, inp, d, tree, cuda, period=period), kernel="wendland_c2")
        gh.set_sph_kernel("cubic")
    counts = reference(case, sh, "lists")[0][ps.index]
    assert counts.min() == 0 and counts.max() > 64                 # rows from empty to beyond a wave of entries
    special = reference(case, sh, "lists")[0][ps.special]
    assert special[0] > 50 and special[1] == 0                     # r = h is on, its successor off
    plain = run_counts(gh, inp, d, tree, cuda)                      # the period reached the kernel
    assert differs(got[0], plain[0]) >= 1 and differs(got[1], plain[1]) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_range_lists(gh, scenes, case, cuda):
    d, tree, sh, period = scenes(case)
    inp = inputs(T.case_points(case), sh, cuda)
    total = total_of(case, sh)
    assert total < 2 * 10 ** 7
    got = run_lists(gh, inp, d, tree, cuda, total, period=period)
    check_lists(case, sh, got)
    plain = run_lists(gh, inp, d, tree, cuda, total)                # (stops after the counts: another total)
    assert differs(got[0], plain[0]) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_nearest_neighbours(gh, scenes, case, cuda):
    d, tree, sh, period = scenes(case)
    inp = inputs(T.case_points(case), sh, cuda)
    for k in (K_SMALL, K_LARGE) if case[1] <= 16385 else (K_SMALL,):
        got = run_knn(gh, inp, d, tree, cuda, k, period=period)
        check_knn(case, sh, got, k)
    plain = run_knn(gh, inp, d, tree, cuda, k)
    assert differs(got[0], plain[0]) >= 1 and differs(got[1], plain[1]) >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_interpolation_at_points(gh, scenes, case, cuda):
    d, tree, sh, period = scenes(case)
    inp = inputs(T.case_points(case), sh, cuda)
    got = run_field(gh, inp, d, tree, cuda, period=period)
    check_field(case, sh, got)
    counts = reference(case, sh, "field")[1]
    assert counts.min() == 0 and counts.max() > 64
    plain = run_field(gh, inp, d, tree, cuda)                       # the period reached the kernel, where it matters
    wraps = wraps_in_reach(case, sh, "field")
    assert (differs(got[0], plain[0]) >= 1) == wraps and (differs(got[1], plain[1]) >= 1) == wraps


@pytest.mark.gpu
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_pair_counts_and_profiles(gh, scenes, case, cuda):
    d, tree, sh, period = scenes(case)
    inp = inputs(T.case_points(case), sh, cuda)
    got = run_pairs(gh, inp, d, tree, cuda, period=period)
    check_pairs(case, sh, got)
    assert np.all(reference(case, sh, "pairs")[1].sum(axis=0)[1:] > 0)   # every bin above the first holds pairs
    plain = run_pairs(gh, inp, d, tree, cuda)                       # the period reached the kernel, where it matters
    wraps = wraps_in_reach(case, sh, "pairs")
    assert (differs(got[1], plain[1]) >= 1) == wraps and (differs(got[2], plain[2]) >= 1) == wraps
    assert bool(np.any(got[0] != plain[0])) == wraps


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_max_per_leaf_1(gh, scenes, family, cuda):
    """The same spheres as a tree of single-sphere leaves: the coincident 100 on the x face are a spine."""
    d, tree, sh, period = scenes(MPL1_CASE, 1)
    inp = inputs(T.case_points(MPL1_CASE), sh, cuda)
    run_family(gh, family, MPL1_CASE, inp, d, tree, sh, cuda, period)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_a_context_with_its_own_stream_gives_the_same_bits(gh, scenes, family, cuda):
    d, tree, sh, period = scenes(CONTEXT_CASE)
    inp = inputs(T.case_points(CONTEXT_CASE), sh, cuda)
    in_own_context(gh, lambda: run_family(gh, family, CONTEXT_CASE, inp, d, tree, sh, cuda, period))


# ---- self queries: the points are the particles ----------------------------------------------------------
def fof_b(n, period):
    return F32(0.4 * n ** (-1.0 / 3.0) * T.lmin_of(period))


@pytest.fixture(scope="module")
def self_scenes(gh, cuda):
    built = {}

    def get(box, n):
        if (box, n) not in built:
            built[(box, n)] = _build(gh, T.torus_scene(S.BOXES[box], n, seed=n), cuda, 8)
        return built[(box, n)]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("box,n", SELF_CASES)
def test_friends_of_friends_across_the_thresholds(gh, self_scenes, box, n, cuda):
    period = S.BOXES[box]
    d, tree, sh = self_scenes(box, n)
    for b in (F32(0.0), fof_b(n, period)):
        ref = T.labels_cells(sh, b, period)
        labels = _i32((n,), cuda)
        gh.fof_labels_sph(d, tree, float(b), labels=labels, check=True, period=period)
        _eq(labels.cpu().numpy(), ref, (box, n, b, "labels"))
        got = tuple(t.cpu().numpy() for t in gh.fof_groups_sph(labels, 2))
        for name, g, r in zip(("group_of", "sizes", "offsets", "members"), got, restate_catalogue(ref, 2)):
            _eq(g, r, (box, n, b, name))
        plain = gh.fof_labels_sph(d, tree, float(b), check=True).cpu().numpy()
        assert b == 0 or differs(plain, ref) >= 1                   # (coincident centres link the same either way)
    assert np.bincount(T.labels_cells(sh, F32(0.0), period)).max() == T.N_CO


@pytest.mark.gpu
@pytest.mark.parametrize("box,n", SELF_CASES)
def test_smoothing_lengths_across_the_thresholds(gh, self_scenes, box, n, cuda):
    period = S.BOXES[box]
    d, tree, sh = self_scenes(box, n)
    k, eta = 32, 1.2
    h = _f32((n,), cuda)
    gh.smoothing_lengths_sph(d, tree, k, eta, out=h, check=True, period=period)
    h = h.cpu().numpy()
    # the contract's identity on every slot: the GPU's own periodic neighbours at the centres
    idx, d2 = _i32((n, k), cuda), _f32((n, k), cuda)
    gh.nearest_neighbours_sph(d, d, tree, k, indices=idx, d2=d2, check=True, period=period)
    _eq(h, (F32(eta) * np.sqrt(d2.cpu().numpy()[:, k - 1])).astype(F32), (box, n, "h of the GPU's own neighbours"))
    # the restatement: every row, or the 1000 centres nearest a face and 2000 drawn at random
    if n <= 2049:
        rows = np.arange(n)
    else:
        gap = np.full(n, np.inf)
        for a, L in enumerate(period):
            if L > 0:
                gap = np.minimum(gap, np.minimum(sh[:, a].astype(np.float64), L - sh[:, a].astype(np.float64)))
        rows = np.unique(np.concatenate([np.argsort(gap, kind="stable")[:1000],
                                         np.random.default_rng(n).choice(n, 2000, replace=False)]))
    _eq(h[rows], PS.lengths(sh, k, eta, period, rows=rows), (box, n, "h"))
    plain = gh.smoothing_lengths_sph(d, tree, k, eta, check=True).cpu().numpy()
    assert differs(h, plain) >= 1


# ---- sparse neighbours: the k-th distance beyond half a period ---------------------------------------------
@pytest.mark.gpu
def test_sparse_neighbours_reach_beyond_half_a_period(gh, cuda):
    """300 spheres and k up to 64: for the queries in the void the k-th distance exceeds h, periodic_bounds
    turns the lane into "everything" and the union box is recomputed as D shrinks; with the first 40 spheres
    alone every lane is "everything" from the start and the rows are padded."""
    s = T.sparse_scene()
    d, tree, sh = _build(gh, s, cuda, 8)
    q = T.sparse_queries(s)
    qd = _dev(q, cuda)
    ref = PS.knn(q, sh, K_LARGE, CUBE)
    for k in (1, 33, 64):
        idx, d2 = _i32((len(q), k), cuda), _f32((len(q), k), cuda)
        gh.nearest_neighbours_sph(qd, d, tree, k, indices=idx, d2=d2, check=True, period=CUBE)
        _eq(idx.cpu().numpy(), np.ascontiguousarray(ref[0][:, :k]), ("sparse indices", k))
        _eq(d2.cpu().numpy(), np.ascontiguousarray(ref[1][:, :k]), ("sparse d2", k))
    rk = np.sqrt(ref[1][:, 63].astype(np.float64))
    assert np.sum(rk >= 0.5) >= 50 and np.sum(rk < 0.25) >= 50
    d40, tree40, sh40 = _build(gh, s[:40], cuda, 8)
    ref = PS.knn(q, sh40, K_LARGE, CUBE)
    idx, d2 = _i32((len(q), K_LARGE), cuda), _f32((len(q), K_LARGE), cuda)
    gh.nearest_neighbours_sph(qd, d40, tree40, K_LARGE, indices=idx, d2=d2, check=True, period=CUBE)
    _eq(idx.cpu().numpy(), ref[0], "40 spheres: indices")
    _eq(d2.cpu().numpy(), ref[1], "40 spheres: d2")
    assert np.all(ref[0][:, 40:] == -1) and np.all(ref[0][:, :40] >= 0)


# ---- grids ------------------------------------------------------------------------------------------
def _axes(dx):
    return (dx, 0.0, 0.0), (0.0, dx, 0.0), (0.0, 0.0, dx)


GRIDS = {
    # name: (dims, origin, (u, v, w), period, scene)
    "G1": ((16, 16, 16), (0.0, 0.0, 0.0), _axes(1.0 / 16), CUBE, "torus"),
    # a 4-point brick spans 3 dx: below, at and above h = 0.75 (every value dyadic at 0.25)
    "G2-0.24": ((6, 6, 6), (0.0, 0.0, 0.0), _axes(0.24), (1.5, 1.5, 1.5), "wide15"),
    "G2-0.25": ((6, 6, 6), (0.0, 0.0, 0.0), _axes(0.25), (1.5, 1.5, 1.5), "wide15"),
    "G2-0.26": ((6, 6, 6), (0.0, 0.0, 0.0), _axes(0.26), (1.5, 1.5, 1.5), "wide15"),
    # partial bricks, a sheared basis, points outside the cell on both sides
    "G3": ((13, 7, 5), (-0.3, -0.2, 0.9), ((0.09, 0.02, 0.0), (-0.03, 0.11, 0.01), (0.01, 0.0, 0.17)), CUBE, "torus"),
    # the 8 x 8 x 1 slice bricks, and 4 x 4 x 4 bricks with one live column
    "G4-17x9x1": ((17, 9, 1), (0.0, 0.0, 0.0), _axes(1.0 / 16), CUBE, "torus"),
    "G4-64x1x1": ((64, 1, 1), (0.0, 0.0, 0.0), _axes(1.0 / 16), CUBE, "torus"),
    "G4-1x1x9": ((1, 1, 9), (0.0, 0.0, 0.0), _axes(1.0 / 16), CUBE, "torus"),
    "G4-1x1x1": ((1, 1, 1), (0.0, 0.0, 0.0), _axes(1.0 / 16), CUBE, "torus"),
    # two periods along x: the single-wrap contract for points more than a period from the spheres
    "G5": ((32, 4, 4), (-0.5, -0.5, -0.5), _axes(1.0 / 16), CUBE, "wide"),
}


def grid_scene(name):
    if name == "torus":
        return T.case_scene("cube")[0]
    return T.torus_scene_wide_H("cube", scale=1.5 if name == "wide15" else 1.0)


@pytest.fixture(scope="module")
def grid_scenes(gh, cuda):
    built = {}

    def get(name):
        if name not in built:
            built[name] = _build(gh, grid_scene(name), cuda, 8)
        return built[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("grid", list(GRIDS))
def test_grids(gh, grid_scenes, grid, cuda):
    dims, origin, (u, v, w), period, scene = GRIDS[grid]
    d, tree, sh = grid_scenes(scene)
    nx, ny, nz = dims
    pts = grid_points(origin, u, v, w, dims)
    pr = PS.pairs(pts, sh, period)
    pd = _dev(pts, cuda)
    for n_ch in (1, 5):
        wt = weights(len(sh), n_ch)
        ref_out, ref_cnt = restate_field(len(pts), pr, sh, wt, "cubic")[:2]
        wd = _dev(wt[:, 0] if n_ch == 1 else wt, cuda)
        out = _f32((nz, ny, nx) if n_ch == 1 else (nz, ny, nx, n_ch), cuda)
        cnt = _i32((nz, ny, nx), cuda)
        gh.interpolate_grid_sph(origin, u, v, w, dims, d, tree, weights=wd, out=out, counts=cnt, check=True, period=period)
        _eq(cnt.cpu().numpy().reshape(-1), ref_cnt, (grid, n_ch, "counts"))
        _eq(out.cpu().numpy().reshape(len(pts), n_ch), ref_out, (grid, n_ch, "out"))
        p_out = _f32((len(pts),) if n_ch == 1 else (len(pts), n_ch), cuda)
        p_cnt = _i32((len(pts),), cuda)
        gh.interpolate_sph(pd, d, tree, weights=wd, out=p_out, counts=p_cnt, check=True, period=period)
        _eq(p_cnt.cpu().numpy(), ref_cnt, (grid, n_ch, "counts at the points"))
        _eq(p_out.cpu().numpy().reshape(len(pts), n_ch), ref_out, (grid, n_ch, "out at the points"))
    cnt_only = _i32((nz, ny, nx), cuda)
    gh.interpolate_grid_sph(origin, u, v, w, dims, d, tree, counts=cnt_only, check=True, period=period)
    _eq(cnt_only.cpu().numpy().reshape(-1), ref_cnt, (grid, "counts alone"))
    if len(pts) > 1:                                                # the period reached the kernel
        plain = gh.interpolate_grid_sph(origin, u, v, w, dims, d, tree, check=True)[1]
        assert differs(plain.cpu().numpy(), cnt_only.cpu().numpy()) >= 1
    if scene != "torus":                                            # H = h is on, its successor is off
        hit = np.bincount(pr[1], minlength=len(sh))
        h = S.half(period[0])
        assert np.all(hit[sh[:, 3] == h] > 0) and np.all(hit[sh[:, 3] == np.nextafter(h, PS.INF)] == 0)
        assert np.sum(sh[:, 3] == h) >= 1 and np.sum(sh[:, 3] == np.nextafter(h, PS.INF)) >= 1
