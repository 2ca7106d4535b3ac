"""The periodic nearest neighbours, smoothing lengths and interpolation on the GPU
(grace_nearest_neighbours_periodic_f4, grace_smoothing_lengths_periodic_f4,
grace_interpolate_points_periodic_f4, grace_interpolate_grid_periodic_f4 through the `period` argument of
nearest_neighbours_sph, smoothing_lengths_sph, interpolate_sph and interpolate_grid_sph).

Every comparison is bitwise against the NumPy restatement of periodic_point_scenes.py, on its scenes;
test_periodic_point_scenes.py checks the restatement itself.  check=True everywhere: the status word stays
clean on every scene."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import periodic_point_scenes as PS
import periodic_query_scenes as S
from test_periodic_point_scenes import compile_dropin
from test_periodic_queries import _build, _dev, _same
from test_point_query_packets import in_own_context
from test_range_queries import digest
from test_sph_interpolation import lattice as grid_points, restate as restate_field

F32 = np.float32
OPEN = (0.0, 0.0, 0.0)
CUBE = S.BOXES["cube"]
K_SWITCH = (1, 8, 9, 16, 17, 32, 33, 64)                           # both sides of every K the kernels are built for


def _knn(gh, pts, d, tree, k, cuda, period):
    idx, d2 = gh.nearest_neighbours_sph(_dev(np.asarray(pts, F32), cuda), d, tree, k, check=True, period=period)
    return idx.cpu().numpy(), d2.cpu().numpy()


def _lengths(gh, d, tree, k, eta, period):
    return gh.smoothing_lengths_sph(d, tree, k, eta, check=True, period=period).cpu().numpy()


def _field(gh, pts, d, tree, w, cuda, period):
    """(out float32 [m, C] or None, counts int32 [m]); w: float32 [n, C] in tree order, or None."""
    import torch
    cnt = torch.full((len(pts),), -7, dtype=torch.int32, device=cuda)
    wd = None if w is None else _dev(w[:, 0] if w.shape[1] == 1 else w, cuda)
    out, cnt = gh.interpolate_sph(_dev(np.asarray(pts, F32), cuda), d, tree, weights=wd, counts=cnt, check=True,
                                  period=period)
    return None if out is None else out.cpu().numpy().reshape(len(pts), -1), cnt.cpu().numpy()


def _check_knn(gh, pts, d, tree, ref, k, cuda, period, what):
    """Rows of k against the first k of the restatement's rows (ref: PS.knn at some k' >= k <= n)."""
    idx, d2 = _knn(gh, pts, d, tree, k, cuda, period)
    bad = np.nonzero(np.any(idx != ref[0][:, :k], axis=1))[0]
    assert len(bad) == 0, (what, k, bad[:5], idx[bad[:1]], ref[0][bad[:1], :k])
    assert _same(d2, ref[1][:, :k]), (what, k)
    return idx, d2


def _check_field(gh, pts, d, tree, sh, w, kernel, cuda, period, what, pr=None):
    pr = PS.pairs(pts, sh, period) if pr is None else pr
    ref_out, ref_cnt = restate_field(len(pts), pr, sh, w, kernel)[:2]
    out, cnt = _field(gh, pts, d, tree, w, cuda, period)
    bad = np.nonzero(cnt != ref_cnt)[0]
    assert len(bad) == 0, (what, bad[:5], cnt[bad[:5]], ref_cnt[bad[:5]], pts[bad[:5]])
    assert _same(out, ref_out), (what, kernel, w.shape)
    return out, cnt


def _weights(n, n_ch, seed):
    return (0.5 + np.random.default_rng(seed).random((n, n_ch))).astype(F32)


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


# ---- lattice --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", S.OFFSETS)
def test_lattice_is_translation_invariant(gh, cuda, offset):
    d, tree, sh = _build(gh, PS.lattice_H(offset), cuda)
    pts = sh[:, :3].copy()
    ref = PS.knn(pts, sh, 7, CUBE)
    idx, d2 = _check_knn(gh, pts, d, tree, ref, 7, cuda, CUBE, ("lattice", offset))
    assert np.all(d2[:, 0] == 0) and np.all(d2[:, 1:] == F32(1.0 / 256.0))
    _check_knn(gh, pts, d, tree, ref, 4, cuda, CUBE, ("lattice, inside the tie", offset))   # the indices decide
    open_idx, open_d2 = _knn(gh, pts, d, tree, 7, cuda, None)
    assert np.sum(np.any(open_idx != idx, axis=1)) > 1000 and open_d2.max() > F32(1.0 / 256.0)
    eta = 1.2
    h = _lengths(gh, d, tree, 7, eta, CUBE)
    assert np.all(h == F32(eta) * F32(1.0 / 16.0))
    assert _lengths(gh, d, tree, 7, eta, None).max() > h[0]
    _, cnt = _field(gh, pts, d, tree, None, cuda, CUBE)
    assert np.all(cnt == 19), (offset, cnt.min(), cnt.max())
    _, open_cnt = _field(gh, pts, d, tree, None, cuda, None)
    assert open_cnt.min() == 7 and open_cnt.max() == 19


# ---- uniform points in an isotropic and an anisotropic box ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", S.OFFSETS)
@pytest.mark.parametrize("box", list(S.BOXES))
def test_uniform_scene_is_the_restatement_bit_for_bit(gh, cuda, box, offset, kernel_reset):
    period = S.BOXES[box]
    d, tree, sh = _build(gh, PS.interp_scene(box, offset, 11), cuda)
    pts = S.uniform_queries(sh, box, offset, 11)[0]
    what = (box, offset)
    # neighbours: one restatement at k = 64, every smaller k is its rows' head
    ref = PS.knn(pts, sh, 64, period)
    for k in K_SWITCH:
        _check_knn(gh, pts, d, tree, ref, k, cuda, period, what)
    open_idx, _ = _knn(gh, pts, d, tree, 8, cuda, None)
    assert np.sum(np.any(open_idx != ref[0][:, :8], axis=1)) > 100
    h = _lengths(gh, d, tree, 32, 1.2, period)
    assert _same(h, PS.lengths(sh, 32, 1.2, period))
    assert np.sum(h != _lengths(gh, d, tree, 32, 1.2, None)) > 100
    # fields: two SPH kernels; 1, 4 and 5 channels (5: two walks); the counts with them
    pr = PS.pairs(pts, sh, period)
    for kernel in ("cubic", "wendland_c2"):
        gh.set_sph_kernel(kernel)
        for n_ch in (1, 4, 5):
            out, cnt = _check_field(gh, pts, d, tree, sh, _weights(len(sh), n_ch, n_ch), kernel, cuda, period, what, pr)
    _, cnt_only = _field(gh, pts, d, tree, None, cuda, period)
    assert np.array_equal(cnt_only, cnt)
    _, open_cnt = _field(gh, pts, d, tree, None, cuda, None)
    on = PS.sphere_on(sh, period)
    open_on = np.bincount(PS.pairs(pts, sh[on], OPEN)[0], minlength=len(pts))   # the same spheres, open
    assert np.sum(cnt > open_on) > 100 and np.sum(cnt != open_cnt) > 100
    # the off spheres contain nothing, the sphere at exactly half the smallest period is on
    hit = np.bincount(pr[1], minlength=len(sh))
    lmin = min(L for L in period if L > 0)
    assert np.sum(~on) >= 1 and np.all(hit[~on] == 0) and np.all(hit[sh[:, 3] == S.half(lmin)] > 50)


# ---- the seam -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("offset", (0.0, 100.0))
def test_seam_within_ulps_of_the_faces(gh, cuda, offset):
    s, q, _ = S.seam(offset)
    radii = np.array([1e-7, 3e-7, 1e-6, 1e-5, 1e-3, 0.05, 0.5], F32)    # H down to a few ulp of the box, up to half of it
    s[:, 3] = radii[np.arange(len(s)) % len(radii)]
    for mpl in (32, 1):
        d, tree, sh = _build(gh, s, cuda, mpl)
        ref = PS.knn(q, sh, 64, CUBE)
        for k in (1, 9, 64):
            _check_knn(gh, q, d, tree, ref, k, cuda, CUBE, ("seam", offset, mpl))
        assert np.all(ref[1][len(q) - 80:, :64] == 0)               # > 64 coincident queries in the corner cell
        assert _same(_lengths(gh, d, tree, 17, 1.0, CUBE), PS.lengths(sh, 17, 1.0, CUBE))
        _check_field(gh, q, d, tree, sh, _weights(len(sh), 2, 3), "cubic", cuda, CUBE, ("seam", offset, mpl))
    small = sh[:, 3] <= F32(1e-5)
    cnt_small = np.bincount(PS.pairs(q, sh[small], CUBE)[0], minlength=len(q))
    open_small = np.bincount(PS.pairs(q, sh[small], OPEN)[0], minlength=len(q))
    assert np.sum(cnt_small > open_small) > 20                      # wraps decided within a few ulp of the faces


@pytest.mark.gpu
@pytest.mark.parametrize("mpl", (1, 32))
def test_coincident_spine_at_a_corner(gh, cuda, mpl):
    """max_per_leaf 1: the 200 coincident centres are a spine of leaves deeper than the 128-entry stack, in the
    corner of the box, where a query wraps on three axes; check=True raises if a packet exhausts the stack."""
    s = S.corner_spine(0.0)
    rng = np.random.default_rng(17)
    s[:, 3] = np.exp(rng.uniform(np.log(1e-6), np.log(0.3), len(s))).astype(F32)
    d, tree, sh = _build(gh, s, cuda, mpl)
    pts = np.concatenate([sh[:300, :3], sh[rng.choice(len(sh), 200, replace=False), :3],
                          rng.random((300, 3), dtype=F32)])
    ref = PS.knn(pts, sh, 33, CUBE)
    _check_knn(gh, pts, d, tree, ref, 33, cuda, CUBE, ("spine", mpl))
    h = _lengths(gh, d, tree, 33, 1.0, CUBE)
    assert _same(h, PS.lengths(sh, 33, 1.0, CUBE)) and np.sum(h == 0) >= 300
    _check_field(gh, pts, d, tree, sh, _weights(len(sh), 1, 5), "cubic", cuda, CUBE, ("spine", mpl))


@pytest.mark.gpu
def test_one_and_two_spheres(gh, cuda):
    """A tree of one sphere (the root is a leaf, n_nodes == 0) for the neighbours; two spheres for the
    interpolation, which needs a node."""
    import torch
    one = torch.tensor([[0.25, 0.5, 0.9375, 0.0]], dtype=torch.float32, device=cuda)
    t1 = gh.Tree(1, 1, device=cuda)
    t1.leaves[0] = torch.tensor([0, 1, 0, 0], dtype=torch.int32)
    t1.root_index.zero_()
    sh = one.cpu().numpy()
    pts = np.array([[0.25, 0.5, 0.9375], [0.25, 0.5, 0.0625], [0.25, 0.5, -0.0625], [1.25, 1.5, 1.9375],
                    [0.75, 0.5, 0.9375], [np.nan, 0.5, 0.5]], F32)
    ref = PS.knn(pts, sh, 3, CUBE)
    idx, d2 = _check_knn(gh, pts, one, t1, ref, 3, cuda, CUBE, "one sphere")
    assert idx[:, 0].tolist() == [0, 0, 0, 0, 0, -1] and np.all(idx[:, 1:] == -1)
    assert d2[:5, 0].tolist() == [0.0, 0.015625, 0.0, 0.0, 0.25]
    assert _knn(gh, pts, one, t1, 1, cuda, None)[1][1:4, 0].tolist() == [0.765625, 1.0, 3.0]
    assert _lengths(gh, one, t1, 1, 2.0, CUBE).tolist() == [0.0]
    two = np.array([[0.25, 0.5, 0.9375, 0.125], [0.96875, 0.03125, 0.5, 0.0625]], F32)
    d, tree, sh = _build(gh, two, cuda, 1)
    pts = np.array([[0.25, 0.5, 0.9375], [0.25, 0.5, 0.03125], [0.25, 0.5, -0.03125], [1.25, 1.5, 1.9375],
                    [0.75, 0.5, 0.9375], [np.nan, 0.5, 0.5], [0.0, 0.0, 0.5], [0.0, 1.0, 0.5], [1.0, 0.0625, 0.5],
                    [0.03125, 0.96875, 0.5]], F32)
    out, cnt = _check_field(gh, pts, d, tree, sh, _weights(2, 1, 7), "cubic", cuda, CUBE, "two spheres")
    assert cnt.tolist() == [1, 1, 1, 1, 0, 0, 1, 1, 1, 0] and np.all(out[5] == 0)
    assert _field(gh, pts, d, tree, None, cuda, None)[1].tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 1, 0]


# ---- translation ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_sphere_on_a_grid_translates_with_the_box(gh, cuda):
    """A 32^3 grid over the box and a sphere of H = 0.25 at the corner or at the centre: the same field values,
    2103 of them, in another order.  The second sphere has weight 0."""
    import torch
    m, dx = 32, 1.0 / 32.0
    origin, u, v, w = (0.0, 0.0, 0.0), (dx, 0.0, 0.0), (0.0, dx, 0.0), (0.0, 0.0, dx)
    pts = grid_points(origin, u, v, w, (m, m, m))
    fields = []
    for centre in (0.0, 0.5):
        d, tree, sh = _build(gh, np.array([[centre, centre, centre, 0.25], [0.3, 0.3, 0.3, 0.01]], F32), cuda, 1)
        wt = (sh[:, 3] == F32(0.25)).astype(F32).reshape(-1, 1) * F32(1.75)
        out, cnt = gh.interpolate_grid_sph(origin, u, v, w, (m, m, m), d, tree, weights=_dev(wt[:, 0], cuda),
                                           counts=torch.empty((m, m, m), dtype=torch.int32, device=cuda),
                                           check=True, period=CUBE)
        out, cnt = out.cpu().numpy().reshape(-1), cnt.cpu().numpy().reshape(-1)
        ref_out, ref_cnt = restate_field(len(pts), PS.pairs(pts, sh, CUBE), sh, wt, "cubic")[:2]
        assert _same(out, ref_out[:, 0]) and np.array_equal(cnt, ref_cnt)
        assert np.count_nonzero(out) == 2103
        p_out, p_cnt = _field(gh, pts, d, tree, wt, cuda, CUBE)      # the point entry, the same lattice points
        assert _same(p_out[:, 0], out) and np.array_equal(p_cnt, cnt)
        fields.append(np.sort(out))
    assert _same(fields[0], fields[1])
    open_out, _ = gh.interpolate_grid_sph(origin, u, v, w, (m, m, m), d, tree, weights=_dev(wt[:, 0], cuda), check=True)
    assert np.count_nonzero(open_out.cpu().numpy()) == 2103           # (the centre: nothing sticks out)


# ---- identities with the open entry points, and what the result must not depend on -----------------------
@pytest.mark.gpu
def test_identities_and_independence(gh, cuda, kernel_reset):
    import torch
    base = PS.interp_scene("cube", 0.0, 21)
    base[:, 3] = np.minimum(base[:, 3], F32(0.2))
    base[:150, :3] = base[200, :3]                                  # a coincident group: a spine at max_per_leaf 1
    pts = S.uniform_queries(base, "cube", 0.0, 21, 900)[0]
    w = _weights(len(base), 5, 6)
    origin, u, v, ww, dims = (0.0, 0.0, 0.0), (0.125, 0.0, 0.0), (0.0, 0.125, 0.0), (0.0, 0.0, 0.125), (8, 8, 8)

    def run(d, tree, wd, period, p=pts):
        gh.set_sph_kernel("quintic")                                # (the kernel belongs to the context)
        g_out, g_cnt = gh.interpolate_grid_sph(origin, u, v, ww, dims, d, tree, weights=wd,
                                               counts=torch.empty(dims, dtype=torch.int32, device=cuda), check=True,
                                               period=period)
        out, cnt = gh.interpolate_sph(_dev(p, cuda), d, tree, weights=wd,
                                      counts=torch.empty(len(p), dtype=torch.int32, device=cuda), check=True, period=period)
        return (*_knn(gh, p, d, tree, 9, cuda, period), _lengths(gh, d, tree, 32, 1.2, period), out.cpu().numpy(),
                cnt.cpu().numpy(), g_out.cpu().numpy(), g_cnt.cpu().numpy())

    def build(s, mpl):
        d = _dev(s, cuda)
        tree = gh.Tree(len(s), mpl, device=cuda)
        tree, perm = gh.build_tree(d, tree, want_perm=True)
        return d, tree, _dev(w, cuda)[perm.long()].contiguous()

    d, tree, wd = build(base, 32)
    # no wrap: L = 0 and L far above twice the extent are the open entry points, bit for bit
    plain = run(d, tree, wd, None)
    for period in (OPEN, (1e6, 1e6, 1e6)):
        assert all(_same(a, b) for a, b in zip(run(d, tree, wd, period), plain)), period
    torus = run(d, tree, wd, CUBE)
    assert np.sum(np.any(torus[0] != plain[0], axis=1)) > 100 and np.sum(torus[4] != plain[4]) > 100
    # the order of the points
    perm = np.random.default_rng(8).permutation(len(pts))
    shuffled = run(d, tree, wd, CUBE, pts[perm])
    assert all(_same(shuffled[i], torus[i][perm]) for i in (0, 1, 3, 4))
    # max_per_leaf, a context and a stream of its own
    d1, tree1, wd1 = build(base, 1)
    assert torch.equal(d1, d)                                       # the same tree order
    assert all(_same(a, b) for a, b in zip(run(d1, tree1, wd1, CUBE), torus))
    assert all(_same(a, b) for a, b in zip(in_own_context(gh, lambda: run(d, tree, wd, CUBE)), torus))
    # the neighbours do not depend on the H the tree was built with
    for hscale in (0.0, 3.0):
        s = base.copy()
        s[:, 3] *= F32(hscale)
        dh, treeh, _ = build(s, 8)
        assert torch.equal(dh[:, :3], d[:, :3])
        assert all(_same(a, b) for a, b in zip(_knn(gh, pts, dh, treeh, 9, cuda, CUBE), torus[:2]))
        assert _same(_lengths(gh, dh, treeh, 32, 1.2, CUBE), torus[2])
    torch.cuda.synchronize()


# ---- rejections -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_arguments_write_nothing(gh, cuda):
    import torch
    d, tree, sh = _build(gh, PS.interp_scene("cube", 0.0, 51, 2000), cuda)
    n, n_s = 100, len(sh)
    pts = torch.rand((n, 3), dtype=torch.float32, device=cuda)
    pts[:2] = torch.tensor([[float("nan"), 0.5, 0.5], [0.5, float("inf"), 0.5]])
    idx = torch.full((n, 8), 7, dtype=torch.int32, device=cuda)
    dd = torch.full((n, 8), 7.0, dtype=torch.float32, device=cuda)
    h = torch.full((n_s,), 7.0, dtype=torch.float32, device=cuda)
    out = torch.full((n,), 7.0, dtype=torch.float32, device=cuda)
    cnt = torch.full((n,), 7, dtype=torch.int32, device=cuda)
    g_out = torch.full((64,), 7.0, dtype=torch.float32, device=cuda)
    wd = torch.ones(n_s, dtype=torch.float32, device=cuda)
    scene = gh._interp_scene(d, tree)
    lib = gh._lib
    o3 = (C.c_float * 3)(0.0, 0.0, 0.0)
    uvw = (C.c_float * 9)(0.25, 0, 0, 0, 0.25, 0, 0, 0, 0.25)

    def per(v):
        return None if v is None else np.array(v, F32).ctypes.data_as(C.c_void_p)

    def knn(period, k=8, elems=3):
        return lib.grace_nearest_neighbours_periodic_f4(gh._ptr(pts), C.c_size_t(n), C.c_int(elems), *scene, C.c_int(k),
                                                        gh._ptr(idx), gh._ptr(dd), per(period), gh._stream())

    def sml(period, k=8, eta=1.0):
        return lib.grace_smoothing_lengths_periodic_f4(*scene, C.c_int(k), C.c_float(eta), gh._ptr(h), per(period),
                                                       gh._stream())

    def points(period, n_ch=1, weights=wd):
        return lib.grace_interpolate_points_periodic_f4(gh._ptr(pts), C.c_size_t(n), C.c_int(3), *scene, gh._ptr(weights),
                                                        C.c_int(n_ch), gh._ptr(out), gh._ptr(cnt), per(period),
                                                        gh._stream())

    def grid(period, dims=(4, 4, 4)):
        return lib.grace_interpolate_grid_periodic_f4(o3, uvw, (C.c_int * 3)(*dims), *scene, gh._ptr(wd), C.c_int(1),
                                                      gh._ptr(g_out), gh._ptr(None), per(period), gh._stream())

    bad = (None, (-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf")), (1.0, -float("inf"), 1.0))
    for p in bad:
        for fn in (knn, sml, points, grid):
            assert fn(p) == gh.GRACE_INVALID_ARGUMENT, (fn.__name__, p)
    # what the open entry points refuse
    for kw in (dict(k=0), dict(k=65), dict(elems=2), dict(elems=17)):
        assert knn(CUBE, **kw) == gh.GRACE_INVALID_ARGUMENT, kw
    for kw in (dict(k=0), dict(k=65), dict(eta=0.0), dict(eta=float("nan"))):
        assert sml(CUBE, **kw) == gh.GRACE_INVALID_ARGUMENT, kw
    for kw in (dict(n_ch=0), dict(n_ch=65), dict(weights=None)):
        assert points(CUBE, **kw) == gh.GRACE_INVALID_ARGUMENT, kw
    assert grid(CUBE, dims=(4, 0, 4)) == gh.GRACE_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.all(idx == 7) and torch.all(dd == 7.0) and torch.all(h == 7.0) and torch.all(out == 7.0)
    assert torch.all(cnt == 7) and torch.all(g_out == 7.0)
    for fn, args in ((gh.nearest_neighbours_sph, (pts, d, tree, 8)), (gh.smoothing_lengths_sph, (d, tree, 8)),
                     (gh.interpolate_sph, (pts, d, tree, wd)),
                     (gh.interpolate_grid_sph, ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (4, 4, 4), d, tree, wd))):
        with pytest.raises(ValueError):
            fn(*args, period=(-1.0, 1.0, 1.0))
        with pytest.raises(ValueError):
            fn(*args, period=(1.0, 0.5))
    # accepted: -0 as an open axis; non-finite points get -1 / +inf rows and zero fields
    assert knn((1.0, 0.5, -0.0)) == gh.GRACE_OK and sml(CUBE) == gh.GRACE_OK
    assert points(CUBE) == gh.GRACE_OK and grid((0.0, 0.0, 1.0)) == gh.GRACE_OK
    gh.trace_status()
    assert torch.all(idx[:2] == -1) and torch.all(torch.isinf(dd[:2])) and torch.all(idx[2:] >= 0)
    assert torch.all(out[:2] == 0) and torch.all(cnt[:2] == 0) and int(cnt[2:].max()) > 0
    assert not torch.any(h == 7.0) and not torch.any(g_out == 7.0)


# ---- the drop-in program ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mirror", [False, True])
def test_periodic_points_dropin_program_matches_ctypes(gh, cuda, tmp_path, mirror):
    from test_neighbours import _build as build_unit, _random_scene
    d, tree = build_unit(gh, _random_scene(6000, 43), cuda)
    s = d.cpu().numpy()                                            # tree order
    rng = np.random.default_rng(3)
    pts = rng.random((777, 4), dtype=F32)
    n_ch, k, eta, n_grid, period = 3, 19, 1.5, 12, (1.0, 0.5, 0.0)
    w = _weights(len(s), n_ch, 4)
    for name, a in (("s", s), ("p", pts), ("w", w)):
        a.tofile(str(tmp_path / (name + ".f32")))
    exe = str(tmp_path / "dropin_periodic_points")
    compile_dropin(exe, mirror)
    f = lambda x: str(tmp_path / (x + ".f32"))
    res = subprocess.run([exe, f("s"), f("p"), f("w"), str(n_ch), str(k), str(eta), str(n_grid),
                          *(str(L) for L in period)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    idx, d2 = _knn(gh, pts, d, tree, k, cuda, period)
    out, cnt = _field(gh, pts, d, tree, w, cuda, period)
    dx = F32(1.0) / F32(n_grid)
    grid, _ = gh.interpolate_grid_sph((0, 0, 0), (dx, 0, 0), (0, dx, 0), (0, 0, dx), (n_grid,) * 3, d, tree,
                                      weights=_dev(w, cuda), check=True, period=period)
    exp = {"indices": idx, "d2": d2, "h": _lengths(gh, d, tree, k, eta, period), "out": out, "out_only": out,
           "counts": cnt, "grid": grid.cpu().numpy()}
    got = {t[0]: (int(t[1]), int(t[2])) for t in (ln.split() for ln in res.stdout.splitlines())
           if len(t) == 3 and t[0] in exp}
    assert set(got) == set(exp)
    for name, a in exp.items():
        assert got[name] == digest(a), name
    assert np.sum(np.any(idx != _knn(gh, pts, d, tree, k, cuda, None)[0], axis=1)) > 50
