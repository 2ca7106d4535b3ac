"""The depth-ordered traces in a periodic box (grace_trace_emission_absorption_periodic_f4,
grace_trace_absorption_deposit_periodic_f4, grace_trace_spectra_periodic_f4 and their Python front
ends) against the restatement of tests/periodic_ordered_scenes.py: the open composites of
test_emission_absorption.py, test_absorption_deposit.py and test_spectra.py applied per ray to the hits
of all the ray's segments over the scene's images, ordered by (segment, fp32 distance, image index).

The hit lists are bit-equal inputs on both sides (the oracle's per-hit outputs on the restated segments
and the scene's own images), so every tolerance is the open tests' derived bound with n the ray's total;
none is invented here."""
import ctypes as C
import types

import numpy as np
import pytest

import periodic_ordered_scenes as S
import periodic_trace_scenes as P
import test_absorption_deposit as AD
import test_emission_absorption as EA
import test_spectra as SP
from test_periodic_ordered_scenes import compile_dropin
from test_range_queries import digest

F32, F64 = np.float32, np.float64
BOXES = sorted(P.BOXES)
SCENES = BOXES + ["tiers"]
SPAN = 1000.0
GRIDS = [(1, 64, True, 100.0), (2, 300, False, 0.0)]      # channels, bins, periodic velocity grid, hubble


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(cuda)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def coefficients(sh, n_rays, C, seed):
    """Per caller particle: emission of both signs [n, C], absorption [n] and [n, C] ~ 5e-3 h^2 (with
    I ~ 1 / h^2 a ray of 6000 hits reaches an optical depth of a few tens, one of 100 hits a few
    tenths); per ray: luminosities of both signs over three decades."""
    rng = np.random.default_rng(seed)
    e = (rng.random((len(sh), C)) * 4.0 - 2.0).astype(F32)
    k1 = (5e-3 * sh[:, 3].astype(F64) ** 2 * (0.2 + 1.6 * rng.random(len(sh)))).astype(F32)
    kc = (k1[:, None].astype(F64) * (0.75 + 0.5 * rng.random((1, C)))).astype(F32)
    L = (10.0 ** (3.0 * rng.random((n_rays, C))) * np.where(rng.random((n_rays, C)) < 0.5, -1.0, 1.0)).astype(F32)
    return e, k1, L, kc


def grid(n_bins, periodic, hubble):
    if periodic:
        return -SPAN / 3.0, SPAN / n_bins
    return -0.1 * SPAN, 0.2 * SPAN / n_bins


# ---- the three calls, NumPy in and out ------------------------------------------------------------
def run_ea(gh, rays, scene, e, k, want_tau=True):
    import torch
    tau = torch.empty(len(rays), dtype=torch.float32, device=rays.device) if want_tau else None
    out = gh.trace_emission_absorption_periodic_sph(rays, scene, _dev(e, rays.device), _dev(k, rays.device), tau=tau)
    return out.cpu().numpy().reshape(len(rays), np.asarray(e).reshape(len(e), -1).shape[1]), (tau.cpu().numpy() if want_tau else None)


def run_dep(gh, rays, scene, L, k):
    import torch
    dev = rays.device
    tr = torch.empty(L.shape, dtype=torch.float32, device=dev)
    q = torch.empty(L.shape[1], dtype=torch.float64, device=dev)
    dep = gh.trace_absorption_deposit_periodic_sph(rays, scene, _dev(L, dev), _dev(k, dev), transmitted=tr, quantum=q)
    assert tuple(dep.shape) == (scene.n_sources, L.shape[1])
    return dep.cpu().numpy(), tr.cpu().numpy(), q.cpu().numpy()


def run_sp(gh, rays, scene, fields, cfg):
    import torch
    n_ch, n_bins, periodic, hubble = cfg
    v0, dv = grid(n_bins, periodic, hubble)
    col = torch.empty((len(rays), n_ch), dtype=torch.float32, device=rays.device)
    tau = gh.trace_spectra_periodic_sph(rays, scene, *[_dev(f, rays.device) for f in fields], v0, dv, n_bins,
                                        periodic=periodic, hubble=hubble, column=col)
    return tau.cpu().numpy(), col.cpu().numpy()


def check_all(gh, w, rays_sel, what, grids=GRIDS):
    """The three calls on the rays `rays_sel` of world entry w (in that order) against the restatement."""
    import torch
    rays_sel = np.asarray(rays_sel, np.int64)
    rays_h = w.rays[rays_sel]
    rays = w.rays_d[torch.from_numpy(rays_sel).to(w.rays_d.device)].contiguous()
    H = S.sub_list(w.H, rays_sel)
    n = len(rays_sel)
    for C_ in (1, 3):
        e, k1, L, kc = coefficients(w.sph, n, C_, 40 + C_)
        got, got_tau = run_ea(gh, rays, w.scene, e, k1)
        EA.check(got, got_tau, *S.emission_absorption(H, n, e, k1), what="%s ea C%d" % (what, C_))
        R = S.absorption_deposit(H, n, len(w.sph), L, kc)
        AD.check(run_dep(gh, rays, w.scene, L, kc), R, what="%s deposit C%d" % (what, C_))
    for cfg in grids:
        fields = SP._fields(w.sph, cfg[0], 100 + cfg[0], SPAN, signed=True)
        v0, dv = grid(*cfg[1:])
        ref = S.spectra(H, rays_h, *fields, v0, dv, cfg[1], cfg[2], cfg[3])
        SP.check(*run_sp(gh, rays, w.scene, fields, cfg), *ref, what="%s spectra %s" % (what, cfg))
    gh.trace_status()


@pytest.fixture(scope="module")
def world(gh, oracle, cuda):
    """scene name -> the caller's spheres and rays (host), the PeriodicScene, and the restated hit list of
    all the rays over the scene's own images (tree order: the image index breaks ties)."""
    out = {}
    for name in SCENES:
        if name == "tiers":
            sph, rays, targets = S.tiers(oracle, gh.ordered_limits())
            lo, period = P.BOXES["cube"]
        else:
            (sph, rays), targets = S.seam(name), None
            lo, period = P.BOXES[name]
        scene = gh.periodic_scene(_dev(sph, cuda), lo, period)
        assert scene.n_sources == len(sph)
        images, source = scene.spheres.cpu().numpy(), scene.source.cpu().numpy()
        H = S.hit_list(oracle, rays, images, source, lo, period)
        out[name] = types.SimpleNamespace(sph=sph, rays=rays, rays_d=_dev(rays, cuda), scene=scene, H=H, lo=lo,
                                          period=period, targets=targets, images=images, source=source)
    w = out["tiers"]
    assert list(w.H.totals()[:6]) == w.targets
    for r in range(6):          # spread over at least 3 segments, one of them empty, one with one hit
        per_seg = w.H.seg_hits[w.H.seg_off[r]:w.H.seg_off[r + 1]]
        assert len(per_seg) >= 3 and 0 in per_seg and 1 in per_seg
    return out


@pytest.fixture(autouse=True)
def _budget_reset(request):
    yield
    if "gh" in request.fixturenames:
        gh = request.getfixturevalue("gh")
        gh.set_ordered_budget(0)
        gh.ordered_enable_stats(False)


# ---- 1. the three calls against the restatement ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_the_three_calls_match_the_restatement(gh, world, name):
    w = world[name]
    check_all(gh, w, np.arange(len(w.rays)), name)
    tot = w.H.totals()
    print(name, "rays", len(w.rays), "hits", int(tot.sum()), "longest", int(tot.max()), "segments",
          int(np.diff(w.H.seg_off).max()))
    if name != "tiers":
        per_source = np.bincount(w.source, minlength=len(w.sph))
        assert tot.sum() > 1000 and np.diff(w.H.seg_off).max() >= 4
        # some ray meets one particle through several lattice images
        key = w.H.ray.astype(np.int64) * len(w.sph) + w.H.source
        assert np.unique(key).size < key.size and per_source.max() >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("n", S.SIZES[:-1])
def test_ray_counts_around_the_wave_and_the_workgroup(gh, world, box, n):
    check_all(gh, world[box], np.arange(n), "%s n=%d" % (box, n), grids=GRIDS[:1])


# ---- 2. the open limit, bit for bit ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("how", ["open_axes", "huge_box"])
def test_open_axes_and_a_huge_box_give_the_open_calls_bit_for_bit(gh, cuda, world, box, how):
    import torch
    w = world[box]
    lo, period = (w.lo, np.zeros(3, F32)) if how == "open_axes" else (np.full(3, -100.0, F32), np.full(3, 1000.0, F32))
    scene = gh.periodic_scene(_dev(w.sph, cuda), lo, period)
    src = scene.source.cpu().numpy().astype(np.int64)
    assert len(scene.spheres) == len(w.sph) and np.array_equal(np.sort(src), np.arange(len(w.sph)))
    rays = w.rays_d[:256].contiguous()
    n = len(rays)
    for C_ in (1, 3):
        e, k1, L, kc = coefficients(w.sph, n, C_, 7)
        got, got_tau = run_ea(gh, rays, scene, e, k1)
        tau = torch.empty(n, dtype=torch.float32, device=cuda)
        ref = gh.trace_emission_absorption_sph(rays, scene.spheres, scene.tree, _dev(e[src], cuda), _dev(k1[src], cuda),
                                               tau=tau).cpu().numpy().reshape(n, -1)
        assert _same(got, ref) and _same(got_tau, tau.cpu().numpy())
        assert np.count_nonzero(got) > 100
        dep, tr, q = run_dep(gh, rays, scene, L, kc)
        tr_o = torch.empty((n, C_), dtype=torch.float32, device=cuda)
        q_o = torch.empty(C_, dtype=torch.float64, device=cuda)
        dep_o = gh.trace_absorption_deposit_sph(rays, scene.spheres, scene.tree, _dev(L, cuda), _dev(kc[src], cuda),
                                                transmitted=tr_o, quantum=q_o).cpu().numpy()
        assert _same(dep[src], dep_o) and _same(tr, tr_o.cpu().numpy()) and _same(q, q_o.cpu().numpy())
    for cfg in GRIDS:
        fields = SP._fields(w.sph, cfg[0], 3, SPAN, signed=True)
        tau_p, col_p = run_sp(gh, rays, scene, fields, cfg)
        v0, dv = grid(*cfg[1:])
        col_o = torch.empty((n, cfg[0]), dtype=torch.float32, device=cuda)
        tau_o = gh.trace_spectra_sph(rays, scene.spheres, scene.tree, *[_dev(f[src], cuda) for f in fields], v0, dv,
                                     cfg[1], periodic=cfg[2], hubble=cfg[3], column=col_o).cpu().numpy()
        assert _same(tau_p, tau_o) and _same(col_p, col_o.cpu().numpy())
        assert np.count_nonzero(tau_p) > 100
    gh.trace_status()


# ---- 3. budget independence -----------------------------------------------------------------------
def _everything(gh, w, rays):
    n = len(rays)
    e, k1, L, kc = coefficients(w.sph, n, 3, 11)
    fields = SP._fields(w.sph, 1, 5, SPAN, signed=True)
    return run_ea(gh, rays, w.scene, e, k1) + run_dep(gh, rays, w.scene, L, kc) + run_sp(gh, rays, w.scene, fields, GRIDS[0])


@pytest.mark.gpu
def test_results_do_not_depend_on_the_budget(gh, world):
    w = world["tiers"]
    tot = w.H.totals()
    W, B = gh.ordered_limits()
    census = (int((tot <= W).sum()), int(((tot > W) & (tot <= B)).sum()), int((tot > B).sum()))
    assert min(census) >= 1
    e, k1, _, _ = coefficients(w.sph, len(w.rays), 3, 11)
    results, batches = [], []
    gh.ordered_enable_stats(True)
    try:
        for budget in (0, 12 * (int(tot.max()) - 100), 12):     # default; the longest rays alone; one ray per batch
            gh.set_ordered_budget(budget)
            results.append(_everything(gh, w, w.rays_d))
            run_ea(gh, w.rays_d, w.scene, e, k1)
            st = gh.ordered_last_stats()
            batches.append(st["batches"])
            assert (st["rays_wave"], st["rays_block"], st["rays_global"]) == census and st["total_hits"] == tot.sum()
    finally:
        gh.set_ordered_budget(0)
        gh.ordered_enable_stats(False)
    print("batches", batches, "census", census)
    assert batches[0] == 1 and batches[2] == len(w.rays) and batches[0] < batches[1] < batches[2]
    for other in results[1:]:
        assert all(_same(a, b) for a, b in zip(results[0], other))


# ---- 4. tier edges --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", range(6))
def test_tier_edges_first_last_and_alone(gh, world, which):
    w = world["tiers"]
    fill = list(range(6, 11))
    for place, sel in (("first", [which] + fill), ("last", fill + [which]), ("alone", [which])):
        check_all(gh, w, sel, "total %d %s" % (w.targets[which], place), grids=GRIDS[:1])


# ---- 5. neighbours and order ----------------------------------------------------------------------
@pytest.mark.gpu
def test_a_ray_does_not_depend_on_its_neighbours(gh, world):
    import torch
    w = world["cube"]
    rays = w.rays_d[:48].contiguous()
    n = len(rays)
    e, k1, L, kc = coefficients(w.sph, n, 3, 21)
    fields = SP._fields(w.sph, 1, 5, SPAN, signed=True)
    out, tau = run_ea(gh, rays, w.scene, e, k1)
    dep, tr, q = run_dep(gh, rays, w.scene, L, kc)
    sp, col = run_sp(gh, rays, w.scene, fields, GRIDS[0])
    for r in range(n):
        one = rays[r:r + 1].contiguous()
        o1, t1 = run_ea(gh, one, w.scene, e, k1)
        assert _same(o1[0], out[r]) and _same(t1, tau[r:r + 1])
        s1, c1 = run_sp(gh, one, w.scene, fields, GRIDS[0])
        assert _same(s1[0], sp[r]) and _same(c1[0], col[r])
    # transmitted is per ray; deposits under a permutation of the rays
    perm = np.random.default_rng(2).permutation(n)
    dep_p, tr_p, q_p = run_dep(gh, rays[torch.from_numpy(perm).to(rays.device)].contiguous(), w.scene, L[perm], kc)
    assert _same(dep_p, dep) and _same(tr_p, tr[perm]) and _same(q_p, q)
    gh.trace_status()


@pytest.mark.gpu
@pytest.mark.parametrize("box", ["cube", "slab"])
def test_deposits_land_on_the_callers_particles_and_photons_are_conserved(gh, world, box):
    w = world[box]
    n = len(w.rays)
    rng = np.random.default_rng(9)
    L = (10.0 ** (2.0 * rng.random((n, 2)))).astype(F32)
    kc = coefficients(w.sph, n, 2, 13)[3]
    dep, tr, q = run_dep(gh, w.rays_d, w.scene, L, kc)
    R = S.absorption_deposit(w.H, n, len(w.sph), L, kc)
    AD.check((dep, tr, q), R, what=box)
    # a particle with 8 images, hit through more than one of them: the whole deposit in its one row
    per_source = np.bincount(w.source, minlength=len(w.sph))
    images_hit = np.zeros(len(w.sph), np.int64)
    pairs = np.unique(np.stack([w.H.source.astype(np.int64), w.H.image.astype(np.int64)]), axis=1)
    np.add.at(images_hit, pairs[0], 1)
    many = np.nonzero((per_source == 8) & (images_hit >= 2))[0]
    assert len(many) >= 1, "no 8-image particle is hit through two images"
    assert dep.shape == (len(w.sph), 2) and np.all(dep[many] > 0)
    # conservation, within the open deposit test's bounds summed (plus the fp64 additions made here)
    total = dep.sum(0) + tr.astype(F64).sum(0)
    want = L.astype(F64).sum(0)
    tol = AD.deposit_bound(R).sum(0) + AD.transmitted_bound(R).sum(0) + (n + len(w.sph)) * 2.0 ** -52 * want
    print(box, "conservation err / tol", np.abs(total - want) / tol)
    assert np.all(np.abs(total - want) <= tol)


# ---- 6. twice round the torus ---------------------------------------------------------------------
@pytest.mark.gpu
def test_twice_round_the_torus_doubles_column_and_optical_depth(gh, oracle, world, cuda):
    w = world["cube"]
    rays = np.zeros((2, 7), F32)
    rays[:, 0] = 1.0
    rays[:, 3:6] = (0.0, 0.37, 0.61)            # from the face x = 0, along +x
    rays[:, 6] = (1.0, 2.0)
    H = S.hit_list(oracle, rays, w.images, w.source, w.lo, w.period)
    t = H.totals()
    assert t[0] >= 10 and t[1] == 2 * t[0] and list(np.diff(H.seg_off)) == [1, 2]
    cfg = (1, 64, True, 0.0)
    fields = SP._fields(w.sph, 1, 5, SPAN)
    tau_v, col = run_sp(gh, _dev(rays, cuda), w.scene, fields, cfg)
    v0, dv = grid(*cfg[1:])
    _, _, col_ref, tol_col = S.spectra(H, rays, *fields, v0, dv, 64, True, 0.0)
    twice = 2.0 * col_ref[0]
    print("column", col[:, 0], "2 x fp64 column of one lap", twice, "tol", tol_col[1])
    assert np.all(np.abs(col[1].astype(F64) - twice) <= tol_col[1])
    e, k1, _, _ = coefficients(w.sph, 2, 1, 3)
    out, tau = run_ea(gh, _dev(rays, cuda), w.scene, e, k1)
    ref_out, ref_tau, S_, n_r = S.emission_absorption(H, 2, e, k1)
    tol = EA.bound(ref_tau, np.abs(ref_tau), n_r, ref_tau)
    assert abs(float(tau[1]) - 2.0 * ref_tau[0]) <= tol[1]


# ---- 7. segment starts ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES)
def test_segment_starts_are_the_restatement_bit_for_bit(gh, world, box):
    w = world[box]
    for n in S.SIZES:
        rays = w.rays_d[:n].contiguous()
        segs, off, t0 = gh.periodic_ray_segments(rays, w.lo, w.period, want_t0=True)
        segs2, off2 = gh.periodic_ray_segments(rays, w.lo, w.period)
        ref = P.segments(w.rays[:n], w.lo, w.period)
        assert _same(segs.cpu().numpy(), segs2.cpu().numpy()) and np.array_equal(off.cpu().numpy(), off2.cpu().numpy())
        assert _same(segs.cpu().numpy(), ref[0]) and np.array_equal(off.cpu().numpy(), ref[1])
        assert t0.dtype.itemsize == 8 and _same(t0.cpu().numpy(), ref[4])
    assert np.count_nonzero(ref[4]) > 100
    gh.trace_status()


# ---- 8. refusals ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_ray_of_too_many_segments_is_traced_as_itself(gh, oracle, world, cuda):
    w = world["cube"]
    rays = P.refusals("cube")[1]                     # ray 3: 70 000 periods
    H = S.hit_list(oracle, rays, w.images, w.source, w.lo, w.period)
    assert list(np.nonzero(H.refused)[0]) == [3] and list(np.diff(H.seg_off))[3] == 1
    e, k1, L, kc = coefficients(w.sph, len(rays), 2, 3)
    gh.trace_status()
    got, got_tau = run_ea(gh, _dev(rays, cuda), w.scene, e, k1)
    with pytest.raises(ValueError):
        gh.trace_status()
    EA.check(got, got_tau, *S.emission_absorption(H, len(rays), e, k1), what="refused ray")
    keep = [0, 1, 2, 4, 5, 6, 7]
    others, others_tau = run_ea(gh, _dev(rays[keep], cuda), w.scene, e, k1)
    gh.trace_status()
    assert _same(others, got[keep]) and _same(others_tau, got_tau[keep])


@pytest.mark.gpu
def test_wrong_lengths_raise_and_no_rays_return_at_once(gh, world, cuda):
    import torch
    w = world["cube"]
    rays = w.rays_d[:8].contiguous()
    n = len(w.sph)
    e, k1, L, kc = coefficients(w.sph, 8, 2, 3)
    n_img = len(w.images)
    assert n_img != n
    for bad in (n + 1, n - 1, n_img):
        eb, kb = np.zeros((bad, 2), F32), np.zeros(bad, F32)
        with pytest.raises(ValueError):
            run_ea(gh, rays, w.scene, eb, k1)
        with pytest.raises(ValueError):
            run_ea(gh, rays, w.scene, e, kb)
        with pytest.raises(ValueError):
            run_dep(gh, rays, w.scene, L, np.zeros((bad, 2), F32))
        with pytest.raises(ValueError):
            run_sp(gh, rays, w.scene, (np.zeros((bad, 1), F32), np.ones((bad, 1), F32), np.zeros((n, 3), F32)), GRIDS[0])
        with pytest.raises(ValueError):
            run_sp(gh, rays, w.scene, (np.zeros((n, 1), F32), np.ones((n, 1), F32), np.zeros((bad, 3), F32)), GRIDS[0])
    with pytest.raises(ValueError):
        run_dep(gh, rays, w.scene, L[:7], kc)
    none = rays[:0].contiguous()
    out, tau = run_ea(gh, none, w.scene, e, k1)
    assert out.shape == (0, 2) and tau.shape == (0,)
    dep, tr, q = run_dep(gh, none, w.scene, L[:0], kc)
    assert dep.shape == (n, 2) and not dep.any() and not q.any()
    sp, col = run_sp(gh, none, w.scene, SP._fields(w.sph, 1, 5, SPAN), GRIDS[0])
    assert sp.shape == (0, 1, 64)
    gh.trace_status()


@pytest.mark.gpu
@pytest.mark.parametrize("damage", ["decreasing", "wrong_last", "too_many_segments"])
def test_damaged_segment_offsets_are_refused_and_nothing_else_is_written(gh, world, cuda, damage):
    import torch
    w = world["cube"]
    rays = w.rays_d[:16].contiguous()
    n_rays, n, PAD, SENT = len(rays), len(w.sph), 64, -7.5
    segs, off = gh.periodic_ray_segments(rays, w.lo, w.period)
    off_h = off.cpu().numpy().copy()
    if damage == "decreasing":
        off_h[5], off_h[6] = off_h[6], off_h[5]
        assert off_h[5] > off_h[6]
    elif damage == "wrong_last":
        off_h[-1] += 1
    else:
        off_h[1:] = off_h[-1]                       # legal so far: ray 0 has them all
        segs = segs[:1].repeat(70000, 1).contiguous()
        off_h[1:] = 70000
    bad = _dev(off_h, cuda)
    e, k1, L, kc = coefficients(w.sph, n_rays, 1, 3)
    out = torch.full((n_rays + 2 * PAD,), SENT, dtype=torch.float32, device=cuda)
    tau = torch.full((n_rays + 2 * PAD,), SENT, dtype=torch.float32, device=cuda)
    dep = torch.full((n + 2 * PAD,), SENT, dtype=torch.float64, device=cuda)
    args = gh._trace_args(segs, w.scene.spheres, w.scene.tree) + (
        gh._ptr(bad), C.c_size_t(n_rays), gh._ptr(w.scene.source), C.c_size_t(n))
    gh.trace_status()
    status = gh._lib.grace_trace_emission_absorption_periodic_f4(
        *args, gh._ptr(_dev(e, cuda)), C.c_int(1), gh._ptr(_dev(k1, cuda)), gh._ptr(out[PAD:]), gh._ptr(tau[PAD:]),
        gh._stream())
    assert status == gh.GRACE_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        gh.trace_status()
    status = gh._lib.grace_trace_absorption_deposit_periodic_f4(
        *args, gh._ptr(_dev(L, cuda)), gh._ptr(_dev(kc, cuda)), C.c_int(1), gh._ptr(dep[PAD:]), None, None, gh._stream())
    assert status == gh.GRACE_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        gh.trace_status()
    torch.cuda.synchronize()
    for t, m in ((out, n_rays), (tau, n_rays), (dep, n)):
        h = t.cpu().numpy()
        assert np.all(h[:PAD] == SENT) and np.all(h[PAD + m:] == SENT)
    # the library is as before: the undamaged call runs
    got, got_tau = run_ea(gh, rays, w.scene, e, k1)
    EA.check(got, got_tau, *S.emission_absorption(S.sub_list(w.H, np.arange(n_rays)), n_rays, e, k1), what="after")
    gh.trace_status()


# ---- 9. the C++ front end -------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mirror", [False, True])
def test_dropin_program_prints_the_digests_of_the_python_path(gh, cuda, world, tmp_path, mirror):
    """tests/cpp/dropin_periodic_ordered.hip through the grace:: overloads (both header sets) against the
    ctypes path, bit for bit (digests of the outputs' words)."""
    import subprocess
    import torch
    w = world["slab"]
    rays = w.rays_d[:201].contiguous()
    n, m = len(w.sph), len(rays)
    e, k1, L, kc = coefficients(w.sph, m, 2, 17)
    amount, width, vel = SP._fields(w.sph, 1, 5, SPAN)
    fields = np.concatenate([e, k1[:, None], kc, amount, width, vel], axis=1).astype(F32)
    assert fields.shape == (n, 10)
    for name, a in (("s", w.sph), ("r", rays.cpu().numpy()), ("f", fields), ("l", L)):
        np.ascontiguousarray(a).tofile(str(tmp_path / (name + ".f32")))
    exe = str(tmp_path / "dropin_periodic_ordered")
    compile_dropin(exe, mirror)
    f = lambda x: str(tmp_path / (x + ".f32"))
    res = subprocess.run([exe, f("s"), f("r"), f("f"), f("l"), *(repr(float(v)) for v in w.lo),
                          *(repr(float(v)) for v in w.period)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    out, tau = run_ea(gh, rays, w.scene, e, k1)
    dep, tr, q = run_dep(gh, rays, w.scene, L, kc)
    col = torch.empty((m, 1), dtype=torch.float32, device=cuda)
    sp = gh.trace_spectra_periodic_sph(rays, w.scene, _dev(amount, cuda), _dev(width, cuda), _dev(vel, cuda), -200.0, 10.0,
                                       64, periodic=True, hubble=50.0, column=col, check=True).cpu().numpy()
    exp = {"emission_absorption": out, "tau": tau, "deposit": dep, "transmitted": tr, "quantum": q, "spectra": sp,
           "column": col.cpu().numpy()}
    assert np.count_nonzero(out) > 100 and np.count_nonzero(dep) > 100 and np.count_nonzero(sp) > 100
    got = {t[0]: (int(t[1]), int(t[2])) for t in (ln.split() for ln in res.stdout.splitlines())
           if len(t) == 3 and t[0] in exp}
    assert set(got) == set(exp)
    for name, a in exp.items():
        assert got[name] == digest(a), name
