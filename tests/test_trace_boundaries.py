"""Every trace path against brute force at the hit test's edges.

The scenes (trace_boundary_scenes.py) hold, besides a random background, RADIUS twins (one
sphere whose squared radius is the first representable value above the pair's b2, its twin one
radius below) and RANGE twins (centres at adjacent floats on either side of dot_p = 0 or dot_p =
length), placed against the extreme rays of packets -- corners and edges of axis-aligned origin
rectangles, the edge rays of pencils, the rays with extreme origins of general packets, the
shortest and the latest-starting ray -- so that a cull one ulp too tight drops a real hit.  Four
scales: the unit box, the unit box near 1e3, co-ordinates near 1e5 with |s| / h from 1e4 to 1e6,
and a box of 1e-3.  Knobs are covered pairwise with fixed seeds (not their full product)."""
import numpy as np
import pytest
import torch

import trace_boundary_scenes as B
from conftest import check_column_densities

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _reset(gh):
    gh.set_ray_reorder(True); gh.set_packet_split(-1); gh.set_treelet_size(-1)
    gh.set_packet_width(-1); gh.set_exact_integrals(False); gh.set_lattice_split(4)
    gh.set_hits_staging(True); gh.set_cache_auto(True); gh.set_cache_validation(True)
    gh.trace_release(); gh.trace_release_rays()


def _knobs(gh, k):
    gh.set_ray_reorder(k.get("reorder", True))
    gh.set_packet_width(k.get("width", -1))
    gh.set_packet_split(k.get("split", -1))
    gh.set_lattice_split(k.get("lat", 4))
    gh.set_treelet_size(k.get("treelet", -1))
    gh.set_hits_staging(k.get("staging", True))


def _assert_twins(sc):
    h, m = B.twin_outcomes(sc)
    assert len(sc.hit) > 0 and len(sc.miss) > 0, "the scene has no twins"
    assert h.all() and m.all(), "a twin is not on its side of the boundary"


def _build(gh, cuda, sc, mpl=8, want_perm=False):
    """want_perm (float spheres): also the caller's index of every sorted sphere."""
    s = sc.spheres
    if sc.prec == "d4":
        d = torch.from_numpy(np.ascontiguousarray(s)).to(cuda)
        tree = gh.Tree(len(s), mpl, device=cuda)
        gh.build_tree_d4(d, tree, s[:, :3].min(axis=0).astype(F32), s[:, :3].max(axis=0).astype(F32))
    else:
        d = torch.from_numpy(np.ascontiguousarray(s)).to(cuda)
        tree = gh.Tree(len(s), mpl, device=cuda)
        if want_perm:
            tree, perm = gh.build_tree(d, tree, tuple(s[:, :3].min(axis=0)), tuple(s[:, :3].max(axis=0)), want_perm=True)
            return d, tree, perm.cpu().numpy().astype(np.int64)
        gh.build_tree(d, tree, tuple(s[:, :3].min(axis=0)), tuple(s[:, :3].max(axis=0)))
    return d, tree


def _cached(gh, cache, d, tree, run):
    """Runs `run()` under a caching regime; every result must be the same."""
    if cache == "none":
        gh.set_cache_auto(False)
        try:
            return [run()]
        finally:
            gh.set_cache_auto(True)
    if cache == "prepare":
        gh.trace_prepare(d, tree)
        try:
            return [run(), run()]
        finally:
            gh.trace_release()
    return [run(), run(), run()]     # the second call fills the cache, the third is validated


def _check_hits(got, ref, sub, real):
    offs, idx, w, dist = (t.cpu().numpy() for t in got)
    ro, ri, rw, rd = ref
    counts = np.diff(np.append(offs, len(idx)))
    vt = np.uint64 if real == F64 else np.uint32
    for k, r in enumerate(sub):
        a, b = offs[r], offs[r] + counts[r]
        ra, rb = ro[k], (ro[k + 1] if k + 1 < len(sub) else len(ri))
        assert b - a == rb - ra, ("count", r)
        assert np.array_equal(idx[a:b], ri[ra:rb]), ("idx", r)
        assert np.array_equal(dist[a:b].view(vt), rd[ra:rb].astype(real).view(vt)), ("dist", r)
        if rw is not None:
            assert np.array_equal(w[a:b].view(vt), rw[ra:rb].astype(real).view(vt)), ("integral", r)


def _run_f32(gh, O, cuda, sc, k, modes):
    rays = torch.from_numpy(sc.rays).to(cuda)
    d, tree, perm = _build(gh, cuda, sc, k.get("mpl", 8), want_perm=True)
    ss = d.cpu().numpy()                                    # sorted by the build
    rr = sc.rays[sc.sub]
    R = len(rays)
    ref_c = O.brute_hitcounts(rr, ss)
    assert ref_c.sum() > 0
    _knobs(gh, k)
    cache = k.get("cache", "fill")
    if "counts" in modes:
        def counts():
            out = torch.empty(R, dtype=torch.int32, device=cuda)
            gh.trace_hitcounts_sph(rays, d, tree, out, check=True)
            return out.cpu().numpy()
        for got in _cached(gh, cache, d, tree, counts):
            assert np.array_equal(got[sc.sub], ref_c), np.nonzero(got[sc.sub] != ref_c)[0][:5]
    if "hits" in modes:
        ref = O.brute_hits(rr, ss)
        _check_hits(gh.trace_sph(rays, d, tree), ref, sc.sub, F32)
    if "cum" in modes:
        c32, c64 = O.brute_cumulative(rr, ss)
        max_term = 1.91 / float(ss[:, 3].min()) ** 2
        for exact in (True, False):
            gh.set_exact_integrals(exact)

            def cum():
                out = torch.empty(R, dtype=torch.float32, device=cuda)
                gh.trace_cumulative_sph(rays, d, tree, out, check=True)
                return out.cpu().numpy()
            for got in _cached(gh, cache, d, tree, cum):
                check_column_densities(got[sc.sub], c32, c64, "exact" if exact else "fast", max_term)
        gh.set_exact_integrals(False)
    if "weighted" in modes:
        from test_weighted_column_density import restate
        # spotlight weights: channels 1 and 2 are 0 on everything but the radius and the range twins,
        # whose grazing terms (<= 5.64e-11 / h^2) no other sum can see; brought into tree order
        w = B.spotlight_weights(sc, 4, seed=7)[perm]
        ro, ri, rw, _ = O.brute_hits(rr, ss)
        ref32, _, _ = restate(len(rr), ro, ri, rw, w)
        gh.set_exact_integrals(True)
        try:
            out = gh.trace_cumulative_weighted_sph(rays, d, tree, torch.from_numpy(w).to(cuda), check=True)
        finally:
            gh.set_exact_integrals(False)
        assert np.array_equal(out.cpu().numpy()[sc.sub].view(np.uint32), ref32.view(np.uint32))
    return d, tree


def _run_f4d(gh, O, cuda, sc, k):
    from test_mixed_precision import term_individual
    rays = torch.from_numpy(sc.rays).to(cuda)
    d, tree = _build(gh, cuda, sc, k.get("mpl", 8))
    ss = d.cpu().numpy()
    rr = sc.rays[sc.sub]
    _knobs(gh, k)
    got = torch.empty(len(rays), dtype=torch.int32, device=cuda)
    gh.trace_hitcounts_f4_f64(rays, d, tree, got, check=True)
    ref_c = O.brute_hitcounts_f4d(rr, ss)
    assert np.array_equal(got.cpu().numpy()[sc.sub], ref_c)
    ro, ri, rb2, rd = O.brute_hits_f4d(rr, ss)
    rw = np.array([term_individual(b2, ss[j, 3]) for b2, j in zip(rb2, ri)], F64)
    _check_hits(gh.trace_sph(rays, d, tree, real=torch.float64), (ro, ri, rw, rd), sc.sub, F64)


def _run_d4(gh, O, cuda, sc, k):
    rays = torch.from_numpy(sc.rays).to(cuda)
    d, tree = _build(gh, cuda, sc, k.get("mpl", 8))
    ss = d.cpu().numpy()
    rr = sc.rays[sc.sub]
    _knobs(gh, k)
    got = torch.empty(len(rays), dtype=torch.int32, device=cuda)
    gh.trace_hitcounts_d4(rays, d, tree, got)
    assert np.array_equal(got.cpu().numpy()[sc.sub], O.brute_hitcounts_d4(rr, ss))
    cum = torch.empty(len(rays), dtype=torch.float64, device=cuda)
    gh.trace_cumulative_d4(rays, d, tree, cum)
    assert np.array_equal(cum.cpu().numpy()[sc.sub].view(np.uint64), O.brute_cumulative_d4(rr, ss).view(np.uint64))
    _check_hits(gh.trace_sph_d4(rays, d, tree), O.brute_hits_d4(rr, ss), sc.sub, F64)


# (kind, scale, precision, scene options, knobs, modes): packet kinds x scales x knobs, pairwise
ALL = ("counts", "hits", "cum", "weighted")
CASES = [
    # axis-aligned packets along +-x, +-y, +-z
    ("axis", "unit", "f32", dict(axis=0, sense=1), dict(reorder=False, width=64, split=1, treelet=-1, cache="none"), ALL),
    ("axis", "1e3", "f32", dict(axis=0, sense=-1, neg_zero=True), dict(reorder=True, width=32, split=2, treelet=0, cache="fill"), ALL),
    ("axis", "1e5", "f32", dict(axis=1, sense=1, ragged=True), dict(reorder=False, width=16, split=8, treelet=64, cache="prepare"), ALL),
    ("axis", "1e-3", "f32", dict(axis=1, sense=-1, ragged=True), dict(reorder=True, width=-1, split=-1, treelet=512, cache="fill"), ALL),
    ("axis", "1e5", "f32", dict(axis=2, sense=1, neg_zero=True), dict(reorder=False, width=32, split=-1, treelet=512, cache="none", mpl=1), ALL),
    ("axis", "unit", "f32", dict(axis=2, sense=-1, ragged=True), dict(reorder=False, width=-1, split=2, treelet=64, cache="fill", mpl=32), ALL),
    ("axis", "1e3", "f32", dict(axis=2, sense=1, ragged=True), dict(reorder=True, width=16, split=1, treelet=0, cache="prepare"), ("counts", "cum")),
    # pencils: pinhole, isotropic from one point, HEALPix
    ("pinhole", "unit", "f32", {}, dict(reorder=False, width=64, split=-1, treelet=0, cache="fill"), ALL),
    ("pinhole", "1e5", "f32", {}, dict(reorder=True, width=16, split=8, treelet=-1, cache="none"), ALL),
    ("iso", "1e3", "f32", {}, dict(reorder=False, width=32, split=1, treelet=512, cache="prepare"), ALL),
    ("iso", "1e-3", "f32", {}, dict(reorder=True, width=-1, split=2, treelet=64, cache="fill"), ALL),
    ("healpix", "unit", "f32", {}, dict(reorder=False, width=16, split=2, treelet=-1, cache="prepare"), ALL),
    ("healpix", "1e5", "f32", {}, dict(reorder=True, width=64, split=8, treelet=0, cache="fill"), ALL),
    # general packets
    ("general", "unit", "f32", {}, dict(reorder=False, width=64, split=8, treelet=64, cache="fill"), ALL),
    ("general", "1e5", "f32", {}, dict(reorder=False, width=16, split=-1, treelet=0, cache="prepare"), ALL),
    ("general", "1e-3", "f32", {}, dict(reorder=True, width=32, split=1, treelet=-1, cache="none"), ("counts", "cum")),
    # mixed precision (float4 spheres, fp64 test)
    ("axis", "unit", "f4d", dict(axis=2, sense=1), dict(reorder=False, width=64), None),
    ("axis", "1e5", "f4d", dict(axis=0, sense=-1, ragged=True), dict(reorder=True, treelet=64), None),
    ("pinhole", "1e5", "f4d", {}, dict(reorder=False, width=32), None),
    ("healpix", "unit", "f4d", {}, dict(reorder=True), None),
    ("general", "unit", "f4d", {}, dict(reorder=False, width=64), None),
    # double4 spheres
    ("axis", "1e5", "d4", dict(axis=1, sense=-1), dict(reorder=False, width=64), None),
    ("axis", "unit", "d4", dict(axis=2, sense=1, ragged=True), dict(reorder=True, treelet=0), None),
    ("iso", "1e5", "d4", {}, dict(reorder=False, width=16), None),
    ("general", "1e5", "d4", {}, dict(reorder=False, width=64, treelet=512), None),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_boundary_scene_equals_brute_force(gh, oracle, cuda, case):
    kind, scale, prec, opts, knobs, modes = CASES[case]
    sc = B.boundary_scene(kind, scale, prec, seed=100 + case, width=max(16, knobs.get("width", 64)),
                          **opts)
    _assert_twins(sc)
    try:
        if prec == "f32":
            _run_f32(gh, oracle, cuda, sc, knobs, modes)
        elif prec == "f4d":
            _run_f4d(gh, oracle, cuda, sc, knobs)
        else:
            _run_d4(gh, oracle, cuda, sc, knobs)
    finally:
        _reset(gh)


def _lattice_run(gh, oracle, cuda, sc, per_hit):
    rays = torch.from_numpy(sc.rays).to(cuda)
    d, tree = _build(gh, cuda, sc, 8)
    ss = d.cpu().numpy()
    rr = sc.rays[sc.sub]
    hc = torch.empty(len(rays), dtype=torch.int32, device=cuda)
    gh.trace_hitcounts_sph(rays, d, tree, hc, check=True)
    assert gh.last_lattice() == 1
    assert np.array_equal(hc.cpu().numpy()[sc.sub], oracle.brute_hitcounts(rr, ss))
    c32, c64 = oracle.brute_cumulative(rr, ss)
    for exact in (True, False):
        gh.set_exact_integrals(exact)
        cu = torch.empty(len(rays), dtype=torch.float32, device=cuda)
        gh.trace_cumulative_sph(rays, d, tree, cu, check=True)
        assert gh.last_lattice() == 1
        check_column_densities(cu.cpu().numpy()[sc.sub], c32, c64, "exact" if exact else "fast",
                               1.91 / float(ss[:, 3].min()) ** 2)
    gh.set_exact_integrals(False)
    if per_hit:
        _check_hits(gh.trace_sph(rays, d, tree), oracle.brute_hits(rr, ss), sc.sub, F32)


@pytest.mark.parametrize("scale", ["unit", "1e5", "1e-3", "1e3"])
def test_lattice_scene_equals_brute_force(gh, oracle, cuda, scale):
    """Sub-pixel twins against the first and the 8th column and row of 8 x 8 tiles: the
    origin-lattice instantiation runs (and is checked to).  4096 rays: the class-split kernels
    already run eight waves per packet, so set_lattice_split has no effect at this size (see the
    next test)."""
    sc = B.lattice_scene(scale, seed=len(scale))
    _assert_twins(sc)
    assert set(sc.lattice_cols.tolist()) >= {0, B.TILE - 1} and set(sc.lattice_rows.tolist()) >= {0, B.TILE - 1}
    try:
        _lattice_run(gh, oracle, cuda, sc, per_hit=True)
    finally:
        _reset(gh)


@pytest.mark.parametrize("lat", [0, 2, 4, 8])
def test_lattice_split_on_a_full_frame(gh, oracle, cuda, lat):
    """A 1024 x 1024 grid (16384 packets of 64, reordering on) with sub-pixel twins: the hit-count
    trace runs one wave per packet, so with the lattice flag set it takes the split-lattice
    instantiation with set_lattice_split waves per packet (0: the one-wave kernel); the column
    densities run max(2, lat) waves per packet.  Brute force on the twins' rays and a sample."""
    sc = B.lattice_scene("unit", seed=40 + lat, side=1024, max_places=500)
    _assert_twins(sc)
    try:
        gh.set_lattice_split(lat)
        _lattice_run(gh, oracle, cuda, sc, per_hit=False)
    finally:
        _reset(gh)


def test_per_hit_outputs_at_4096_packets(gh, oracle, cuda):
    """65536 axis-aligned rays in packets of 16: 4096 packets, the per-hit trace's one-wave
    variant that stages its outputs in LDS."""
    sc = B.boundary_scene("axis", "unit", "f32", seed=77, side=256, width=16, axis=2, sense=1, max_twins=800)
    _assert_twins(sc)
    try:
        rays = torch.from_numpy(sc.rays).to(cuda)
        d, tree = _build(gh, cuda, sc, 8)
        ss = d.cpu().numpy()
        ref = oracle.brute_hits(sc.rays[sc.sub], ss)
        gh.set_ray_reorder(False); gh.set_packet_width(16)
        _check_hits(gh.trace_sph(rays, d, tree), ref, sc.sub, F32)
    finally:
        _reset(gh)


@pytest.mark.parametrize("staging", [True, False])
def test_split_per_hit_walk_with_heavy_packets(gh, oracle, cuda, staging):
    """The split per-hit walk (fewer than 4096 packets) stages a packet's hits in LDS when the
    batch averages at least 200 000 hits per packet of 64 rays and hit staging is on (the
    default); off, the same walk stores directly.  100 000 spheres with h ~ 0.12 give ~4500 hits
    per ray; both settings == brute force on a sample of rays."""
    rng = np.random.default_rng(8)
    n = 100_000
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = rng.uniform(0.1, 0.14, n).astype(F32)
    side = 32                                                # 1024 rays: 16 packets of 64
    g = (0.35 + 0.3 * (np.arange(side) + 0.5) / side)
    rays = np.zeros((side * side, 7), F32)
    rays[:, 2] = 1
    rays[:, 3] = np.repeat(g, side).astype(F32); rays[:, 4] = np.tile(g, side).astype(F32)
    rays[:, 5] = -0.1; rays[:, 6] = 1.2
    try:
        d = torch.from_numpy(s).to(cuda)
        tree = gh.Tree(n, 32, device=cuda)
        gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        ss = d.cpu().numpy()
        sub = np.sort(rng.choice(len(rays), 40, replace=False))
        gh.set_hits_staging(staging)
        got = gh.trace_sph(torch.from_numpy(rays).to(cuda), d, tree)
        assert len(got[1]) / (len(rays) / 64) >= 200_000, "below the staging threshold"
        _check_hits(got, oracle.brute_hits(rays[sub], ss), sub, F32)
    finally:
        _reset(gh)


def test_wide_pencil_falls_back_to_the_walk(gh, oracle, cuda):
    """Pencils with 64 rays per origin spread over every direction, through more than 256 x 4096
    spheres: more than 256 groups survive a packet's group test and it walks the tree after all.
    Radius twins against each packet's rays; brute force on a few hundred rays."""
    rng = np.random.default_rng(5)
    n_bg = 1_100_000
    s = np.empty((n_bg, 4), F32)
    s[:, :3] = rng.random((n_bg, 3), dtype=F32)
    s[:, 3] = rng.uniform(0.001, 0.004, n_bg).astype(F32)
    n_pk = 32
    k = np.arange(64) + 0.5                                   # a Fibonacci sphere of 64 directions
    z = 1 - 2 * k / 64; phi = np.pi * (1 + 5 ** 0.5) * k
    fib = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    rays = np.zeros((64 * n_pk, 7), F32)
    for p in range(n_pk):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        rays[64 * p:64 * (p + 1), :3] = B._normalise32(fib @ q)
        rays[64 * p:64 * (p + 1), 3:6] = rng.uniform(0.3, 0.7, 3).astype(F32)
        rays[64 * p:64 * (p + 1), 6] = F32(0.45)
    places = [(int(r), B._perp_unit(rays[r, :3].astype(F64), rng.normal(size=3)), 0.02)
              for r in rng.choice(len(rays), 200, replace=False)]
    c, w_hit, w_miss, tgt = B._place_radius_twins(rays, places, "f32", rng, (0.3, 0.9), True)
    assert len(c) > 100
    assert B.hit_f32(rays[tgt], np.concatenate([c, w_hit[:, None]], axis=1))[0].all()
    assert not B.hit_f32(rays[tgt], np.concatenate([c, w_miss[:, None]], axis=1))[0].any()
    allsph = np.concatenate([s, np.concatenate([c, w_hit[:, None]], axis=1),
                             np.concatenate([c, w_miss[:, None]], axis=1)]).astype(F32)
    sub = np.unique(np.concatenate([tgt, rng.choice(len(rays), 64, replace=False)]))
    try:
        gh.set_ray_reorder(False)
        d = torch.from_numpy(allsph).to(cuda)
        tree = gh.Tree(len(allsph), 32, device=cuda)
        gh.build_tree(d, tree, tuple(allsph[:, :3].min(axis=0)), tuple(allsph[:, :3].max(axis=0)))
        ss = d.cpu().numpy()
        r = torch.from_numpy(rays).to(cuda)
        hc = torch.empty(len(rays), dtype=torch.int32, device=cuda)
        gh.trace_hitcounts_sph(r, d, tree, hc, check=True)
        assert np.array_equal(hc.cpu().numpy()[sub], oracle.brute_hitcounts(rays[sub], ss))
        gh.set_exact_integrals(True)
        cu = torch.empty(len(rays), dtype=torch.float32, device=cuda)
        gh.trace_cumulative_sph(r, d, tree, cu, check=True)
        c32, _ = oracle.brute_cumulative(rays[sub], ss)
        assert np.array_equal(cu.cpu().numpy()[sub].view(np.uint32), c32.view(np.uint32))
    finally:
        _reset(gh)


# ---- a tree over a prefix of the primitive array -------------------------------------------------
def _prefix_rays(gh, cuda, kind):
    if kind == "axis":
        return gh.orthogonal_rays_z(64, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    if kind == "pinhole":
        return gh.pinhole_camera_rays(64, 64, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0, device=cuda)
    if kind == "iso":
        return gh.uniform_random_rays(4096, (0.5, 0.5, 0.5), 1.0, device=cuda)
    if kind == "healpix":
        return gh.healpix_rays(16, (0.5, 0.45, 0.55), 1.0, device=cuda)
    r = B.general_rays(64, np.array([0.5, 0.5, 0.5]), 1.0, np.random.default_rng(3))
    return torch.from_numpy(r).to(cuda)


@pytest.mark.parametrize("kind", ["axis", "pinhole", "iso", "healpix", "general"])
def test_tree_over_a_prefix_sees_only_that_prefix(gh, oracle, cuda, kind):
    """A tree built over spheres[:m], traced with the whole array: every packet kind sees the
    primitives the leaves cover and nothing else -- the walk's (and the reference's) semantics --,
    including the axis-aligned and pencil packets' flat group passes; float, mixed and double4
    spheres; hit counts, column densities and per-hit outputs."""
    n, m = 60000, 37000
    s = oracle.random_real4(n, (0, 0, 0, 0.004), (1, 1, 1, 0.02), first=11)
    d = torch.from_numpy(s).to(cuda)
    pre = d[:m]
    tree = gh.Tree(m, 16, device=cuda)
    gh.build_tree(pre, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))   # sorts d[:m] in place
    ss = d.cpu().numpy()
    rays = _prefix_rays(gh, cuda, kind)
    rr = rays.cpu().numpy()
    sub = np.unique(np.random.default_rng(1).integers(0, len(rr), 512))
    ref_c = oracle.brute_hitcounts(rr[sub], ss[:m])
    assert not np.array_equal(ref_c, oracle.brute_hitcounts(rr[sub], ss)), "the suffix is never hit"
    c32, _ = oracle.brute_cumulative(rr[sub], ss[:m])
    ref_hits = oracle.brute_hits(rr[sub], ss[:m])
    # the same spheres as double4, a tree over their prefix (the flat passes of hit counts and
    # column densities take the same bound)
    d64 = torch.from_numpy(s.astype(np.float64)).to(cuda)
    tree64 = gh.Tree(m, 16, device=cuda)
    gh.build_tree_d4(d64[:m], tree64, np.zeros(3, F32), np.ones(3, F32))
    ss64 = d64.cpu().numpy()
    ref_c64 = oracle.brute_hitcounts_d4(rr[sub], ss64[:m])
    ref_cum64 = oracle.brute_cumulative_d4(rr[sub], ss64[:m])
    ref_hits64 = oracle.brute_hits_d4(rr[sub], ss64[:m])
    try:
        for reorder in (True, False):
            gh.set_ray_reorder(reorder)
            for cache in ("none", "fill"):
                hc = torch.empty(len(rays), dtype=torch.int32, device=cuda)
                runs = _cached(gh, cache, d, tree, lambda: gh.trace_hitcounts_sph(rays, d, tree, hc, check=True).cpu().numpy())
                for got in runs:
                    assert np.array_equal(got[sub], ref_c), (reorder, cache)
            gh.set_exact_integrals(True)
            cu = torch.empty(len(rays), dtype=torch.float32, device=cuda)
            gh.trace_cumulative_sph(rays, d, tree, cu, check=True)
            assert np.array_equal(cu.cpu().numpy()[sub].view(np.uint32), c32.view(np.uint32)), reorder
            gh.set_exact_integrals(False)
            _check_hits(gh.trace_sph(rays, d, tree), ref_hits, sub, F32)
            mixed = torch.empty(len(rays), dtype=torch.int32, device=cuda)
            gh.trace_hitcounts_f4_f64(rays, d, tree, mixed, check=True)
            assert np.array_equal(mixed.cpu().numpy()[sub], oracle.brute_hitcounts_f4d(rr[sub], ss[:m])), reorder
            c64 = torch.empty(len(rays), dtype=torch.int32, device=cuda)
            gh.trace_hitcounts_d4(rays, d64, tree64, c64)
            assert np.array_equal(c64.cpu().numpy()[sub], ref_c64), reorder
            cum64 = torch.empty(len(rays), dtype=torch.float64, device=cuda)
            gh.trace_cumulative_d4(rays, d64, tree64, cum64)
            assert np.array_equal(cum64.cpu().numpy()[sub].view(np.uint64), ref_cum64.view(np.uint64)), reorder
            _check_hits(gh.trace_sph_d4(rays, d64, tree64), ref_hits64, sub, F64)
    finally:
        _reset(gh)


# ---- regression scenes: hits the reference's own walk drops --------------------------------------
def _walk_knobs(gh):
    gh.set_ray_reorder(False); gh.set_packet_width(64); gh.set_treelet_size(0)


def test_ray_in_the_plane_of_a_node_box_face(gh, oracle, cuda):
    """A +z ray whose x equals the rounded face fl(c_x + h) of a tangent sphere's box: the slab
    test's 0 * inf = NaN made the walk (and the reference's, which the oracle restates) reject the
    box although the brute-force test hits the sphere.  The per-hit trace walks; treelet 0 makes
    every node a slab test."""
    rng = np.random.default_rng(12)
    side = 8
    rays = np.zeros((side * side, 7), F32)
    rays[:, 2] = 1
    g = (np.arange(side) + 0.5) / side
    rays[:, 3] = np.repeat(g, side).astype(F32); rays[:, 4] = np.tile(g, side).astype(F32)
    rays[:, 5] = -0.5; rays[:, 6] = 2
    twins = []
    for r in range(len(rays)):
        o = rays[r, 3]
        for _ in range(200):
            q = F32(rng.uniform(0.003, 0.03))
            c = F32(o - q)
            qq = F32(c - o)
            w, _, _ = B.radius_twins(np.array([qq * qq], F32), "f32")
            if F32(c + w[0]) == o:
                twins.append([c, rays[r, 4], rng.uniform(0.1, 0.9), w[0]])
                break
    twins = np.array(twins, F32)
    assert len(twins) > 32
    bg = oracle.random_real4(3000, (0, 0, 0, 0.002), (1, 1, 1, 0.01), first=5)
    s = np.concatenate([bg, twins]).astype(F32)
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(len(s), 1, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    ss = d.cpu().numpy()
    ref = oracle.brute_hits(rays, ss)
    nodes, leaves, root = tree.nodes.cpu().numpy(), tree.leaves.cpu().numpy(), int(tree.root_index.item())
    walk = oracle.trace(rays, ss, nodes.view(F32), leaves, root, width=1)
    assert (walk < oracle.brute_hitcounts(rays, ss)).any(), "the scene no longer trips the reference's walk"
    try:
        _walk_knobs(gh)
        _check_hits(gh.trace_sph(torch.from_numpy(rays).to(cuda), d, tree), ref, np.arange(len(rays)), F32)
    finally:
        _reset(gh)


def test_double4_tangent_hit_outside_the_narrowed_node_box(gh, oracle, cuda):
    """Found by the 1e5 double4 scene (|s| / h ~ 1.4e7): float(c -+ h) moves the box corners inward
    by up to half a float ulp (3.9e-3 here, h = 7.1e-3); the ray's slab test rejected the box of a
    sphere the double test hits.  The walk now widens node boxes by 2^-21 (|lo| + |hi|) in the
    fp64 modes."""
    ray = np.array([0.0513593815267086, 0.13627156615257263, 0.989339292049408,
                    99982.953125, 99937.4453125, 100012.34375, 160.0], F32)
    sph = np.array([99987.39465228793, 99949.22277891377, 100097.90119504783, 0.007146359783243693])
    assert B.hit_d4(ray, sph)[0]
    rng = np.random.default_rng(3)
    rays = np.repeat(ray[None], 64, axis=0)
    rays[1:, 3:6] += rng.uniform(-0.5, 0.5, (63, 3)).astype(F32)
    bg = np.empty((4000, 4))
    bg[:, :3] = sph[:3] + rng.uniform(-20, 20, (4000, 3)); bg[:, 3] = rng.uniform(0.005, 0.5, 4000)
    s = np.concatenate([bg, sph[None]])
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(len(s), 1, device=cuda)
    gh.build_tree_d4(d, tree, s[:, :3].min(axis=0).astype(F32), s[:, :3].max(axis=0).astype(F32))
    ss = d.cpu().numpy()
    r = torch.from_numpy(rays).to(cuda)
    try:
        _walk_knobs(gh)
        got = torch.empty(64, dtype=torch.int32, device=cuda)
        gh.trace_hitcounts_d4(r, d, tree, got)
        assert np.array_equal(got.cpu().numpy(), oracle.brute_hitcounts_d4(rays, ss))
        _check_hits(gh.trace_sph_d4(r, d, tree), oracle.brute_hits_d4(rays, ss), np.arange(64), F64)
    finally:
        _reset(gh)
