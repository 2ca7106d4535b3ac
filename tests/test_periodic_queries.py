"""The periodic point queries on the GPU (grace_range_counts_periodic_f4, grace_range_neighbours_periodic_f4,
grace_fof_labels_periodic_f4, grace_pair_counts_periodic_f4 through the `period` argument of
range_counts_sph, range_neighbours_sph, fof_labels_sph, pair_counts_sph and radial_profiles_sph).

Every comparison is bitwise against the NumPy restatement of periodic_query_scenes.py, on its scenes;
test_periodic_query_scenes.py checks the restatement itself.  check=True everywhere: the status word stays
clean on every scene."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import periodic_query_scenes as S
from test_pair_counts import log_edges
from test_periodic_query_scenes import compile_dropin
from test_point_query_packets import in_own_context
from test_range_queries import digest, restate_sums

F32 = np.float32
OPEN = (0.0, 0.0, 0.0)
CUBE = S.BOXES["cube"]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _build(gh, s, cuda, mpl=32):
    """The tree over the data's own bounds (the scenes sit at offsets); returns (spheres, tree, tree order)."""
    d = _dev(np.asarray(s, F32), cuda)
    tree = gh.Tree(len(s), mpl, device=cuda)
    gh.build_tree(d, tree)                                          # sorts d
    return d, tree, d.cpu().numpy()


def _radii(r, cuda):
    return float(r) if np.ndim(r) == 0 else _dev(np.asarray(r, F32), cuda)


def _counts(gh, pts, r, d, tree, cuda, period, weights=None):
    cnt, sums = gh.range_counts_sph(_dev(np.asarray(pts, F32), cuda), _radii(r, cuda), d, tree, weights=weights,
                                    check=True, period=period)
    return cnt.cpu().numpy(), None if sums is None else sums.cpu().numpy()


def _lists(gh, pts, r, d, tree, cuda, period):
    off, idx, d2 = gh.range_neighbours_sph(_dev(np.asarray(pts, F32), cuda), _radii(r, cuda), d, tree, check=True,
                                           period=period)
    return off.cpu().numpy(), idx.cpu().numpy(), d2.cpu().numpy()


def _check_range(gh, pts, r, d, tree, sh, cuda, period, what):
    """Counts, lists and the returned d2 against the restatement; returns the restatement."""
    rr = np.broadcast_to(np.asarray(r, F32), (len(pts),))
    ref = S.restate(pts, rr, sh, period)
    cnt, _ = _counts(gh, pts, r, d, tree, cuda, period)
    bad = np.nonzero(cnt != ref[0])[0]
    assert len(bad) == 0, (what, bad[:5], cnt[bad[:5]], ref[0][bad[:5]], rr[bad[:5]], pts[bad[:5]])
    off, idx, d2 = _lists(gh, pts, r, d, tree, cuda, period)
    assert np.array_equal(off, ref[1]) and np.array_equal(idx, ref[2]), what
    assert _same(d2, ref[3]), what
    return ref


def _check_bins(gh, pts, edges, d, tree, sh, cuda, period, what, w=None, lists=None):
    """Totals, histograms and weighted shells against the restatement."""
    edges = np.asarray(edges, F32)
    totals, counts, sums = S.restate_bins(pts, edges, sh, period, w, lists)
    pd = _dev(np.asarray(pts, F32), cuda)
    got = gh.pair_counts_sph(pd, edges, d, tree, check=True, period=period).cpu().numpy()
    assert np.array_equal(got.astype(np.uint64), totals), (what, got, totals)
    wd = None if w is None else _dev(w[:, 0] if w.shape[1] == 1 else w, cuda)
    g_counts, g_sums = gh.radial_profiles_sph(pd, edges, d, tree, weights=wd, check=True, period=period)
    assert np.array_equal(g_counts.cpu().numpy(), counts), what
    if w is not None:
        assert _same(g_sums.cpu().numpy().reshape(sums.shape), sums), what
    return totals


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


# ---- lattice --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", S.OFFSETS)
def test_lattice_counts_are_translation_invariant(gh, cuda, offset):
    d, tree, sh = _build(gh, S.lattice(offset), cuda)
    pts = sh[:, :3].copy()
    for r, n_torus in zip(S.LATTICE_RADII, S.LATTICE_COUNTS):
        cnt, _ = _counts(gh, pts, float(r), d, tree, cuda, CUBE)
        assert np.all(cnt == n_torus), (offset, r, cnt.min(), cnt.max())
        open_cnt, _ = _counts(gh, pts, float(r), d, tree, cuda, None)
        assert open_cnt.min() < n_torus and open_cnt.max() == n_torus
    r = S.LATTICE_RADII[np.arange(len(pts)) % 3]                    # the three exact radii, per point
    ref = _check_range(gh, pts, r, d, tree, sh, cuda, CUBE, ("lattice", offset))
    assert np.any(ref[3] == F32(1.0 / 256.0))                       # d2 == R2 across the seam too
    a, b = F32(1.0 / 16.0), F32(1.0 / 8.0)
    ties = np.array([np.nextafter(a, F32(0)), a, np.nextafter(b, F32(0)), b], F32)
    totals = _check_bins(gh, pts, ties, d, tree, sh, cuda, CUBE, ("lattice ties", offset))
    assert totals.tolist() == [4096, 6 * 4096, 20 * 4096, 6 * 4096]


# ---- uniform points in an isotropic and an anisotropic box ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", S.OFFSETS)
@pytest.mark.parametrize("box", list(S.BOXES))
def test_uniform_scene_is_the_restatement_bit_for_bit(gh, cuda, box, offset, kernel_reset):
    period = S.BOXES[box]
    d, tree, sh = _build(gh, S.uniform(3000, box, offset, 11), cuda)
    pts, r = S.uniform_queries(sh, box, offset, 11)
    ref = _check_range(gh, pts, r, d, tree, sh, cuda, period, (box, offset))
    open_counts = S.restate(pts, r, sh, OPEN)[0]
    assert np.sum(ref[0] > open_counts) > 100 and ref[0].max() > 256
    k = len(S.special_radii(box))
    assert np.all(ref[0][6:k:2] == 0)                               # the successor of half a period: off
    # gather sums, 1 and 4 channels, two SPH kernels
    rng = np.random.default_rng(4)
    for kernel in ("cubic", "wendland_c2"):
        gh.set_sph_kernel(kernel)
        for n_ch in (1, 4):
            w = (0.5 + rng.random((len(sh), n_ch))).astype(F32)
            cnt, sums = _counts(gh, pts, r, d, tree, cuda, period, weights=_dev(w[:, 0] if n_ch == 1 else w, cuda))
            assert np.array_equal(cnt, ref[0])
            assert _same(sums.reshape(len(pts), n_ch), restate_sums(pts, r, sh, w, kernel, ref)), (box, offset, kernel, n_ch)
    # pair totals, histograms and weighted shells: 1, 8 and 64 edges (4 channels: up to 16 edges, 64 cells)
    e_max = 0.2 * min(L for L in period if L > 0)
    lists = S.restate(pts, F32(e_max), sh, period)
    for edges, n_ch in ((np.array([e_max], F32), 1), (np.array([e_max], F32), 4), (log_edges(e_max / 50, e_max, 8), 1),
                        (log_edges(e_max / 50, e_max, 8), 4), (log_edges(e_max / 50, e_max, 16), 4),
                        (np.concatenate([[F32(0)], log_edges(e_max / 100, e_max, 63)]), 1)):
        w = (0.5 + rng.random((len(sh), n_ch))).astype(F32)
        _check_bins(gh, pts, edges, d, tree, sh, cuda, period, (box, offset, len(edges), n_ch), w,
                    lists if edges[-1] == F32(e_max) else None)
    # the last edge at exactly half the smallest period
    e_half = S.half(min(L for L in period if L > 0))
    _check_bins(gh, pts[:300], [e_half / 4, e_half], d, tree, sh, cuda, period, (box, offset, "half"))


@pytest.mark.gpu
def test_pair_counts_on_the_torus_exceed_the_open_ones(gh, cuda):
    d, tree, sh = _build(gh, S.spheres_of(np.random.default_rng(1).random((3000, 3)).astype(F32)), cuda)
    torus = gh.pair_counts_sph(d, [0.05], d, tree, check=True, period=CUBE).cpu().numpy()
    plain = gh.pair_counts_sph(d, [0.05], d, tree, check=True).cpu().numpy()
    assert int(torus[0]) == 7812 and int(plain[0]) == 7582


# ---- the seam -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", (0.0, 100.0))
def test_seam_within_ulps_of_the_faces(gh, cuda, offset):
    s, q, r = S.seam(offset)
    for mpl in (32, 1):
        d, tree, sh = _build(gh, s, cuda, mpl)
        ref = _check_range(gh, q, r, d, tree, sh, cuda, CUBE, ("seam", offset, mpl))
        assert np.all(ref[0][len(q) - 80:][r[len(q) - 80:] == 0] >= 80)   # > 64 coincident queries in the corner cell
    _check_bins(gh, q, [0.0, 1e-7, 1e-6, 1e-3, 0.05], d, tree, sh, cuda, CUBE, ("seam bins", offset))
    # a centre at o and one at o + L, queried at o with r = 0: both
    two = s[:2]
    d2, t2, sh2 = _build(gh, two, cuda, 1)
    cnt, _ = _counts(gh, q[:1], 0.0, d2, t2, cuda, CUBE)
    assert cnt.tolist() == [2]
    assert _counts(gh, q[:1], 0.0, d2, t2, cuda, None)[0].tolist() == [1]
    off, idx, dd = _lists(gh, q[:1], 0.0, d2, t2, cuda, CUBE)
    assert idx.tolist() == [0, 1] and dd.tolist() == [0.0, 0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("offset", (0.0, 100.0))
def test_coincident_spine_at_a_corner(gh, cuda, offset):
    """max_per_leaf 1: the 200 coincident centres are a spine of leaves deeper than the 128-entry stack, in the
    corner of the box, where a query wraps on three axes; check=True raises if a packet exhausts the stack."""
    d, tree, sh = _build(gh, S.corner_spine(offset), cuda, 1)
    rng = np.random.default_rng(17)
    pts = np.concatenate([sh[:300, :3], sh[rng.choice(len(sh), 200, replace=False), :3],
                          (F32(offset) + rng.random((300, 3), dtype=F32)).astype(F32)])
    r = np.exp(rng.uniform(np.log(1e-6), np.log(0.3), len(pts))).astype(F32)
    ref = _check_range(gh, pts, r, d, tree, sh, cuda, CUBE, ("spine", offset))
    assert ref[0].max() >= 200
    labels = gh.fof_labels_sph(d, tree, 2.0 ** -19, check=True, period=CUBE).cpu().numpy()
    assert np.array_equal(labels, S.restate_labels(sh, 2.0 ** -19, CUBE))


@pytest.mark.gpu
def test_one_sphere(gh, cuda):
    """A tree of one sphere: the root is a leaf, n_nodes == 0."""
    import torch
    one = torch.tensor([[0.25, 0.5, 0.9375, 0.0]], dtype=torch.float32, device=cuda)
    t1 = gh.Tree(1, 1, device=cuda)
    t1.leaves[0] = torch.tensor([0, 1, 0, 0], dtype=torch.int32)
    t1.root_index.zero_()
    sh = one.cpu().numpy()
    pts = np.array([[0.25, 0.5, 0.9375], [0.25, 0.5, 0.0625], [0.25, 0.5, -0.0625], [1.25, 1.5, 1.9375], [0.75, 0.5, 0.9375]], F32)
    r = np.array([0.0, 0.125, 0.0, 0.0, 0.5], F32)
    ref = _check_range(gh, pts, r, one, t1, sh, cuda, CUBE, "one sphere")
    assert ref[0].tolist() == [1, 1, 1, 1, 1]
    assert _counts(gh, pts, r, one, t1, cuda, None)[0].tolist() == [1, 0, 0, 0, 1]
    _check_bins(gh, pts, [0.0, 0.125, 0.5], one, t1, sh, cuda, CUBE, "one sphere")
    assert gh.fof_labels_sph(one, t1, 0.1, check=True, period=CUBE).cpu().numpy().tolist() == [0]


# ---- identities with the open entry points ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("period", [OPEN, (8.0, 300.0, 2.5), (2.5, 0.0, 1e30)])
def test_without_wraps_the_output_is_the_open_entry_points(gh, cuda, period, kernel_reset):
    d, tree, sh = _build(gh, S.uniform(3000, "cube", 0.0, 21), cuda)
    pts, r = S.uniform_queries(sh, "cube", 0.0, 21)
    r[:8] = np.array([0.0, -1.0, np.nan, np.inf, 0.3, 0.6, 1.0, 1.2], F32)
    w = (0.5 + np.random.default_rng(6).random((len(sh), 4))).astype(F32)
    wd = _dev(w, cuda)
    gh.set_sph_kernel("quintic")
    for rad in (r, 0.07):
        c0, s0 = _counts(gh, pts, rad, d, tree, cuda, None, weights=wd)
        c1, s1 = _counts(gh, pts, rad, d, tree, cuda, period, weights=wd)
        assert np.array_equal(c0, c1) and _same(s0, s1)
        assert all(_same(a, b) for a, b in zip(_lists(gh, pts, rad, d, tree, cuda, None), _lists(gh, pts, rad, d, tree, cuda, period)))
    pd = _dev(pts, cuda)
    edges = np.concatenate([[F32(0)], log_edges(0.002, 0.2, 15)])
    assert np.array_equal(gh.pair_counts_sph(pd, edges, d, tree, check=True).cpu().numpy(),
                          gh.pair_counts_sph(pd, edges, d, tree, check=True, period=period).cpu().numpy())
    p0 = gh.radial_profiles_sph(pd, edges, d, tree, weights=wd, check=True)
    p1 = gh.radial_profiles_sph(pd, edges, d, tree, weights=wd, check=True, period=period)
    assert np.array_equal(p0[0].cpu().numpy(), p1[0].cpu().numpy()) and _same(p0[1].cpu().numpy(), p1[1].cpu().numpy())
    for b in (0.03, 0.06):
        assert np.array_equal(gh.fof_labels_sph(d, tree, b, check=True).cpu().numpy(),
                              gh.fof_labels_sph(d, tree, b, check=True, period=period).cpu().numpy())


# ---- friends-of-friends ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", S.OFFSETS)
def test_fof_groups_across_the_seam(gh, cuda, offset):
    # a clump that straddles a face: one group with the period, two without
    s = S.straddling_clump(offset)
    dd = _dev(s, cuda)
    tree = gh.Tree(len(s), 32, device=cuda)
    tree, perm = gh.build_tree(dd, tree, want_perm=True)
    sh, perm = dd.cpu().numpy(), perm.cpu().numpy()
    b = 0.012
    lab = gh.fof_labels_sph(dd, tree, b, check=True, period=CUBE).cpu().numpy()
    assert np.array_equal(lab, S.restate_labels(sh, b, CUBE))
    assert np.array_equal(lab, S.components(len(sh), *S.links(sh, b, CUBE)))
    lab_open = gh.fof_labels_sph(dd, tree, b, check=True).cpu().numpy()
    assert np.array_equal(lab_open, S.restate_labels(sh, b, OPEN))
    clump = perm < 400                                              # the clump's members, in tree order
    assert np.sum(lab[clump] == np.bincount(lab[clump]).argmax()) > 380
    halves = np.sort(np.bincount(lab_open[clump]))[::-1]
    assert halves[0] < 300 and halves[1] > 100
    # the catalogue is the open one's, fed with these labels
    group_of, sizes, offsets, members = gh.fof_groups_sph(_dev(lab, cuda), min_members=20)
    assert sizes.cpu().numpy().max() > 380
    # a chain that closes around the torus
    c, ctree, csh = _build(gh, S.torus_chain(offset), cuda, 1)
    b = 1.0 / 64.0
    assert len(np.unique(gh.fof_labels_sph(c, ctree, b, check=True, period=CUBE).cpu().numpy())) == 1
    assert len(np.unique(gh.fof_labels_sph(c, ctree, b, check=True).cpu().numpy())) == 2
    assert len(np.unique(gh.fof_labels_sph(c, ctree, b, check=True, period=(0.0, 1.0, 1.0)).cpu().numpy())) == 2
    # uniform points, isotropic and anisotropic, linking lengths around the mean separation's scale
    for box in S.BOXES:
        u, utree, ush = _build(gh, S.uniform(3000, box, offset, 31), cuda)
        for b in (0.03, 0.05, S.half(0.5)):
            got = gh.fof_labels_sph(u, utree, float(b), check=True, period=S.BOXES[box]).cpu().numpy()
            assert np.array_equal(got, S.restate_labels(ush, b, S.BOXES[box])), (box, offset, b)


# ---- what the result must not depend on -----------------------------------------------------------------
@pytest.mark.gpu
def test_results_do_not_depend_on_leaf_size_H_stream_or_context(gh, cuda):
    import torch
    base = S.uniform(4000, "cube", 100.0, 41)
    base[:150, :3] = base[0, :3]                                    # a coincident group: a spine at max_per_leaf 1
    base[150:300, :3] = np.array([100.0, 100.0 + 2.0 ** -17, 101.0 - 2.0 ** -17], F32)   # and one on an edge
    pts, r = S.uniform_queries(base, "cube", 100.0, 41, 900)
    w = (0.5 + np.random.default_rng(2).random((len(base), 2))).astype(F32)
    edges = log_edges(0.004, 0.2, 9)
    b = 0.04

    def run(d, tree, wd):
        cnt, sums = _counts(gh, pts, r, d, tree, cuda, CUBE, weights=wd)
        pd = _dev(pts, cuda)
        totals = gh.pair_counts_sph(pd, edges, d, tree, check=True, period=CUBE).cpu().numpy()
        shells = gh.radial_profiles_sph(pd, edges, d, tree, weights=wd, check=True, period=CUBE)
        labels = gh.fof_labels_sph(d, tree, b, check=True, period=CUBE).cpu().numpy()
        return (cnt, sums, *_lists(gh, pts, r, d, tree, cuda, CUBE), totals.view(np.uint32), shells[0].cpu().numpy(),
                shells[1].cpu().numpy(), labels)

    runs = []
    for hscale, mpl in ((1.0, 32), (0.0, 32), (3.0, 8), (1.0, 1)):
        s = base.copy()
        s[:, 3] *= F32(hscale)
        d = _dev(s, cuda)
        tree = gh.Tree(len(s), mpl, device=cuda)
        tree, perm = gh.build_tree(d, tree, want_perm=True)
        wd = _dev(w, cuda)[perm.long()].contiguous()
        runs.append((d[:, :3].cpu().numpy(), run(d, tree, wd), d, tree, wd))
    x0, out0 = runs[0][:2]
    assert np.array_equal(out0[0], S.restate(pts, r, x0, CUBE)[0]) and out0[0].max() > 64
    for x, out, *_ in runs[1:]:
        assert np.array_equal(x, x0)                                # the same tree order
        assert all(_same(a, b_) for a, b_ in zip(out, out0))
    _, _, d, tree, wd = runs[0]
    got = in_own_context(gh, lambda: run(d, tree, wd))              # a context and a stream of its own
    assert all(_same(a, b_) for a, b_ in zip(got, out0))
    torch.cuda.synchronize()


# ---- rejections -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_periods_and_radii_write_nothing(gh, cuda):
    import torch
    d, tree, sh = _build(gh, S.uniform(2000, "cube", 0.0, 51), cuda)
    n = 100
    pts = torch.rand((n, 3), dtype=torch.float32, device=cuda)
    rad = torch.full((n,), 0.05, dtype=torch.float32, device=cuda)
    cnt = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    off = torch.zeros(n + 1, dtype=torch.int32, device=cuda)
    idx = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    lab = torch.full((len(sh),), 7, dtype=torch.int32, device=cuda)
    tot = torch.full((2,), 7, dtype=torch.int64, device=cuda)
    scene = gh._interp_scene(d, tree)
    lib = gh._lib
    edges = np.array([0.1, 0.2], F32)

    def per(v):
        return None if v is None else np.array(v, F32)

    def counts(period, rp=rad, radius=0.0):
        p = per(period)
        return lib.grace_range_counts_periodic_f4(gh._ptr(pts), C.c_size_t(n), C.c_int(3), gh._ptr(rp), C.c_float(radius),
                                                  *scene, gh._ptr(None), C.c_int(0), gh._ptr(cnt), gh._ptr(None),
                                                  None if p is None else p.ctypes.data_as(C.c_void_p), gh._stream())

    def lists(period, rp=rad, radius=0.0):
        p = per(period)
        return lib.grace_range_neighbours_periodic_f4(gh._ptr(pts), C.c_size_t(n), C.c_int(3), gh._ptr(rp),
                                                      C.c_float(radius), *scene, gh._ptr(off), gh._ptr(idx), gh._ptr(None),
                                                      None if p is None else p.ctypes.data_as(C.c_void_p), gh._stream())

    def fof(period, b=0.05):
        p = per(period)
        return lib.grace_fof_labels_periodic_f4(*scene, C.c_float(b), gh._ptr(lab),
                                                None if p is None else p.ctypes.data_as(C.c_void_p), gh._stream())

    def pairs(period, e=edges):
        p = per(period)
        return lib.grace_pair_counts_periodic_f4(gh._ptr(pts), C.c_size_t(n), C.c_int(3), e.ctypes.data_as(C.c_void_p),
                                                 C.c_int(len(e)), *scene, gh._ptr(None), C.c_int(0), gh._ptr(tot),
                                                 gh._ptr(None), gh._ptr(None),
                                                 None if p is None else p.ctypes.data_as(C.c_void_p), gh._stream())

    bad = (None, (-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf")), (1.0, -float("inf"), 1.0))
    for p in bad:
        for fn in (counts, lists, fof, pairs):
            assert fn(p) == gh.GRACE_INVALID_ARGUMENT, (fn.__name__, p)
    # a host radius above half a period on a periodic axis: the uniform radius, the linking length, the last edge
    above = float(np.nextafter(F32(0.25), F32(1)))
    for p in ((1.0, 0.5, 0.0), (0.5, 1.0, 1.0)):
        assert counts(p, rp=None, radius=above) == gh.GRACE_INVALID_ARGUMENT
        assert lists(p, rp=None, radius=above) == gh.GRACE_INVALID_ARGUMENT
        assert fof(p, b=above) == gh.GRACE_INVALID_ARGUMENT
        assert pairs(p, e=np.array([0.1, above], F32)) == gh.GRACE_INVALID_ARGUMENT
    # what the open entry points refuse
    assert counts(CUBE, rp=None, radius=-1.0) == gh.GRACE_INVALID_ARGUMENT
    assert fof(CUBE, b=float("nan")) == gh.GRACE_INVALID_ARGUMENT
    assert pairs(CUBE, e=np.array([0.2, 0.1], F32)) == gh.GRACE_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.all(cnt == 7) and torch.all(idx == 7) and torch.all(lab == 7) and torch.all(tot == 7)
    for fn, kw in ((gh.range_counts_sph, {}), (gh.range_neighbours_sph, {})):
        with pytest.raises(ValueError):
            fn(pts, above, d, tree, period=(1.0, 0.5, 0.0), **kw)
        with pytest.raises(ValueError):
            fn(pts, 0.1, d, tree, period=(1.0, 0.5))
    with pytest.raises(ValueError):
        gh.fof_labels_sph(d, tree, 0.05, period=(-1.0, 1.0, 1.0))
    # accepted: exactly half a period (scalar and open z: any radius fits that axis), -0 as an open axis
    assert counts((1.0, 0.5, 0.0), rp=None, radius=0.25) == gh.GRACE_OK
    assert fof((0.5, 1.0, -0.0), b=0.25) == gh.GRACE_OK
    assert pairs((0.0, 0.0, 0.4), e=np.array([0.1, 0.2], F32)) == gh.GRACE_OK
    gh.trace_status()
    assert int(cnt.min()) > 50


# ---- the drop-in program ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_periodic_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    from test_neighbours import _build as build_unit, _random_scene
    d, tree = build_unit(gh, _random_scene(6000, 43), cuda)
    s = d.cpu().numpy()                                            # tree order
    rng = np.random.default_rng(3)
    pts = rng.random((777, 4), dtype=F32)
    r = np.exp(rng.uniform(np.log(1e-3), np.log(0.25), len(pts))).astype(F32)
    n_ch, radius, b, period = 3, 0.0625, 0.03, (1.0, 0.5, 0.0)
    w = (0.5 + rng.random((len(s), n_ch))).astype(F32)
    edges = log_edges(0.005, 0.2, 9)
    for name, a in (("s", s), ("p", pts), ("r", r), ("w", w), ("e", edges)):
        a.tofile(str(tmp_path / (name + ".f32")))
    exe = str(tmp_path / "dropin_periodic")
    compile_dropin(exe)
    f = lambda x: str(tmp_path / (x + ".f32"))
    res = subprocess.run([exe, f("s"), f("p"), f("r"), f("w"), str(n_ch), str(radius), str(b), f("e"),
                          *(str(L) for L in period)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    wd = _dev(w, cuda)
    cnt, sums = _counts(gh, pts, r, d, tree, cuda, period, weights=wd)
    one, _ = _counts(gh, pts, radius, d, tree, cuda, period)
    off, idx, d2 = _lists(gh, pts, r, d, tree, cuda, period)
    pd = _dev(pts, cuda)
    shells, shell_sums = gh.radial_profiles_sph(pd, edges, d, tree, weights=wd, check=True, period=period)
    exp = {"counts": cnt, "sums": sums, "counts_one": one, "offsets": off, "indices": idx, "d2": d2,
           "labels": gh.fof_labels_sph(d, tree, b, check=True, period=period).cpu().numpy(),
           "totals": gh.pair_counts_sph(pd, edges, d, tree, check=True, period=period).cpu().numpy().view(np.uint32),
           "shells_only": shells.cpu().numpy(), "shells": shells.cpu().numpy(), "shell_sums": shell_sums.cpu().numpy()}
    got = {t[0]: (int(t[1]), int(t[2])) for t in (ln.split() for ln in res.stdout.splitlines())
           if len(t) == 3 and t[0] in exp}
    assert set(got) == set(exp)
    for name, a in exp.items():
        assert got[name] == digest(a), name
    assert np.array_equal(cnt, S.restate(pts, r, s, period)[0])
    assert np.sum(cnt > _counts(gh, pts, r, d, tree, cuda, None)[0]) > 50
