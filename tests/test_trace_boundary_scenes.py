"""CPU checks of the boundary-scene generator (trace_boundary_scenes.py): its restatements of
sphere_hit agree with the oracle's on many pairs, near-tangent and boundary pairs included, and
every twin sits exactly on its side of the boundary according to the oracle."""
import numpy as np
import pytest

import trace_boundary_scenes as B

F32, F64 = np.float32, np.float64
KIND = {"f32": 0, "f4d": 1, "d4": 2}


def _pairs(sc):
    """Every twin with its target ray, plus random (ray, sphere) pairs of the scene."""
    rng = np.random.default_rng(0)
    ids = np.concatenate([sc.hit, sc.miss])
    tgt = np.concatenate([sc.target_hit, sc.target_miss])
    ri = rng.integers(0, len(sc.rays), 4000)
    si = rng.integers(0, len(sc.spheres), 4000)
    return (np.ascontiguousarray(sc.rays[np.concatenate([tgt, ri])]),
            np.ascontiguousarray(sc.spheres[np.concatenate([ids, si])]))


def _agree(oracle, rays, s, prec):
    hit, b2, dot = B.RESTATE[prec](rays, s)
    o_hit, o_b2, o_dot = oracle.sphere_hit_pairs(rays, s, KIND[prec])
    assert np.array_equal(hit, o_hit)
    assert np.array_equal(b2.astype(F64).view(np.uint64), o_b2.view(np.uint64))
    assert np.array_equal(dot.astype(F64).view(np.uint64), o_dot.view(np.uint64))


@pytest.mark.parametrize("prec", ["f32", "f4d", "d4"])
@pytest.mark.parametrize("kind,scale", [("axis", "unit"), ("axis", "1e5"), ("pinhole", "1e3"),
                                        ("iso", "1e-3"), ("healpix", "1e5"), ("general", "unit"),
                                        ("general", "1e5")])
def test_restatements_equal_the_oracle(oracle, prec, kind, scale):
    sc = B.boundary_scene(kind, scale, prec, seed=3, n_background=3000, neg_zero=kind == "axis",
                          ragged=scale == "1e5")
    rays, s = _pairs(sc)
    _agree(oracle, rays, s, prec)


def test_restatements_equal_the_oracle_on_random_pairs(oracle):
    rng = np.random.default_rng(1)
    n = 20000
    rays = np.zeros((n, 7), F32)
    rays[:, :3] = B._normalise32(rng.normal(size=(n, 3)))
    rays[:, 3:6] = rng.uniform(-2, 2, (n, 3)).astype(F32)
    rays[:, 6] = rng.uniform(0.1, 4, n).astype(F32)
    s = np.empty((n, 4), F32)
    s[:, :3] = (rays[:, 3:6] + rays[:, :3] * rng.uniform(-0.5, 4.5, (n, 1)) + rng.normal(0, 0.05, (n, 3))).astype(F32)
    s[:, 3] = rng.uniform(0.001, 0.1, n).astype(F32)
    for prec in ("f32", "f4d"):
        _agree(oracle, rays, s, prec)
    _agree(oracle, rays, s.astype(F64) * (1 + 1e-9), "d4")


def test_mixed_restatement_equals_test_mixed_precision(oracle):
    """hit_f4d against the mixed-precision suite's own restatement (test_mixed_precision.mixed_test)."""
    from test_mixed_precision import mixed_test
    sc = B.boundary_scene("axis", "unit", "f4d", seed=4, n_background=2000)
    rays = sc.rays[:64]
    hit, b2, dot = mixed_test(rays, sc.spheres)
    h2, b22, dot2 = B.hit_f4d(rays[:, None, :], sc.spheres[None, :, :])
    assert np.array_equal(hit, h2) and np.array_equal(b2, b22) and np.array_equal(dot, dot2)


@pytest.mark.parametrize("prec", ["f32", "f4d", "d4"])
@pytest.mark.parametrize("kind,scale", [("axis", "unit"), ("axis", "1e3"), ("axis", "1e5"), ("axis", "1e-3"),
                                        ("pinhole", "unit"), ("iso", "1e5"), ("healpix", "1e-3"),
                                        ("general", "1e3"), ("general", "1e5")])
def test_twins_sit_on_the_boundary(oracle, prec, kind, scale):
    """Per the oracle: every hit twin is hit by its ray and every miss twin missed; radius twins
    are one radius apart and (mostly) exact -- the hit twin's square is the first value above b2;
    range twins are adjacent co-ordinates with dot_p on either side of 0 or the ray's length."""
    sc = B.boundary_scene(kind, scale, prec, seed=5, n_background=2000, ragged=kind == "axis")
    k = KIND[prec]
    rh, rm = sc.rays[sc.target_hit], sc.rays[sc.target_miss]
    hit_h, b2_h, dot_h = oracle.sphere_hit_pairs(rh, sc.spheres[sc.hit], k)
    hit_m, b2_m, dot_m = oracle.sphere_hit_pairs(rm, sc.spheres[sc.miss], k)
    assert len(sc.hit) > 20 and hit_h.all() and not hit_m.any()
    nr = sc.n_radius
    assert nr > 10 and len(sc.hit) > nr, "radius and range twins"
    # radius twins: same centre, adjacent radii
    wt = F64 if prec == "d4" else F32
    ch, cm = sc.spheres[sc.hit[:nr]], sc.spheres[sc.miss[:nr]]
    assert np.array_equal(ch[:, :3], cm[:, :3])
    assert np.array_equal(np.nextafter(ch[:, 3].astype(wt), wt(0)), cm[:, 3].astype(wt))
    assert np.array_equal(b2_h[:nr], b2_m[:nr])
    w2 = B._sq(ch[:, 3].astype(wt), prec)
    assert np.all(w2 > b2_h[:nr])
    _, _, exact = B.radius_twins(b2_h[:nr].astype(F32 if prec == "f32" else F64), prec)
    assert exact.mean() > 0.8
    # range twins: same radius, centres adjacent in one co-ordinate, dot_p on either side
    rh_, rm_ = sc.spheres[sc.hit[nr:]], sc.spheres[sc.miss[nr:]]
    assert np.array_equal(rh_[:, 3], rm_[:, 3])
    diff = (rh_[:, :3] != rm_[:, :3]).sum(axis=1)
    assert np.all(diff == 1)
    L = sc.rays[sc.target_hit[nr:], 6].astype(F64)
    at_start = dot_m[nr:] < 0
    at_end = dot_m[nr:] >= L
    assert np.all(at_start | at_end) and at_start.any() and at_end.any()
    assert np.all(dot_h[nr:][at_start] >= 0) and np.all(dot_h[nr:][at_end] < L[at_end])


def test_axis_range_twins_are_exact():
    """Axis-aligned rays: the range twins' dot_p is exactly +0 (and the first value below it), or
    straddles the length (mostly: exactly the length and the first value below it)."""
    sc = B.boundary_scene("axis", "unit", "f32", seed=6, n_background=1000, ragged=True)
    nr = sc.n_radius
    _, _, dh = B.hit_f32(sc.rays[sc.target_hit[nr:]], sc.spheres[sc.hit[nr:]])
    _, _, dm = B.hit_f32(sc.rays[sc.target_miss[nr:]], sc.spheres[sc.miss[nr:]])
    L = sc.rays[sc.target_hit[nr:], 6]
    start = dm < 0
    assert start.any() and (~start).any()
    assert np.all(dh[start] == 0) and not np.signbit(dh[start]).any()
    assert np.all(dm[~start] >= L[~start]) and np.all(dh[~start] < L[~start])
    # (dot_p = fl(c - o) reaches the length itself where the spacing of c allows it)
    assert np.mean(dm[~start] == L[~start]) > 0.5


def test_generator_scenes_are_sharp():
    """Most hit twins are hit by their own ray alone within its packet (axis-aligned: all)."""
    assert B.sharpness(B.boundary_scene("axis", "1e5", "f32", seed=7, n_background=1000)) == 1.0
    assert B.sharpness(B.boundary_scene("general", "unit", "f32", seed=7, n_background=1000)) > 0.9
    assert B.sharpness(B.boundary_scene("pinhole", "unit", "f32", seed=7, n_background=1000)) > 0.5
    sc = B.lattice_scene("unit", seed=1, n_background=1000)
    assert B.sharpness(sc) == 1.0
    assert set(sc.lattice_cols.tolist()) >= {0, 7} and set(sc.lattice_rows.tolist()) >= {0, 7}


# ---- the scenes of test_trace_plan_boundaries.py ---------------------------------------------------
def _digest(sc):
    import hashlib
    h = hashlib.sha256()
    for a in (sc.rays, sc.spheres, sc.hit.astype(np.int64), sc.miss.astype(np.int64)):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_existing_scenes_are_unchanged():
    """Digests (rays, spheres, hit and miss twins) taken before `ragged="one"`, `drop_last` and the
    `width` argument of axis_rays were added: calls that do not use them draw the same numbers."""
    assert _digest(B.boundary_scene("axis", "unit", "f32", seed=0)) == \
        "de7b1cc53887d05b782263e8272e3a1e56b03f7c762ce223461dac85401ef929"
    assert _digest(B.lattice_scene("unit", seed=0)) == \
        "2f7c927df993e1461e487dccde4db591aed82cdab02fe2e99bca587f33016917"


def test_one_ragged_pair_per_packet_and_a_partial_last_packet():
    """ragged="one": per packet one ray ends and one other starts in the middle half of the box,
    every other ray crosses it; the range twins against those two rays lie in that middle half;
    every twin sits on its side.  drop_last=32: 4064 rays, and the partial last packet has twins
    against its own rays."""
    for axis, sense, scale in ((2, 1, "1e3"), (0, -1, "1e5")):
        sc = B.boundary_scene("axis", scale, "f32", seed=9, axis=axis, sense=sense, ragged="one", n_background=1000)
        h, m = B.twin_outcomes(sc)
        assert h.all() and m.all()
        lo, size, _ = B.SCALES[scale]
        depth0 = (sc.rays[:, 3 + axis] - lo[axis]) / size if sense > 0 else (lo[axis] + size - sc.rays[:, 3 + axis]) / size
        depth1 = depth0 + sc.rays[:, 6] / size
        for pk in B._packets(len(sc.rays), 64):
            short = pk[depth1[pk] < 1.0]; late = pk[depth0[pk] > 0.0]
            assert len(short) == 1 and len(late) == 1 and short[0] != late[0]
            assert 0.25 <= depth1[short[0]] <= 0.75 and 0.25 <= depth0[late[0]] <= 0.75
            assert pk[np.argmin(sc.rays[pk, 6])] == short[0]
        nr = sc.n_radius
        along = (sc.spheres[sc.hit[nr:], axis] - lo[axis]) / size
        # one at an end and one at a start per packet (the third, random, ray may be the late one again)
        assert 2 * 64 <= np.sum((along > 0.24) & (along < 0.76)) <= 2 * 64 + 8
        assert B.sharpness(sc) == 1.0
    sc = B.boundary_scene("axis", "unit", "f32", seed=9, drop_last=32, n_background=1000)
    h, m = B.twin_outcomes(sc)
    assert len(sc.rays) == 4064 and h.all() and m.all()
    last = sc.target_hit >= 4032
    assert last[:sc.n_radius].sum() >= 3 and last[sc.n_radius:].sum() >= 2
    assert sc.target_hit.max() < 4064 and sc.sub.max() < 4064


def _plan_scenes():
    return [("case %d" % c, lambda c=c: B.plan_case_scene(c)) for c in range(len(B.PLAN_CASES))] + \
        [("lattice " + s, lambda s=s: B.plan_lattice_scene(s)) for s in B.PLAN_LATTICE_SCALES]


def test_plan_scenes_have_visible_radius_twins_and_full_range_twins(oracle):
    """What keeps test_trace_plan_boundaries.py from being blind: a grazing radius twin's term is at
    most 5.64e-11 / h^2 and often exactly 0 (the table position rounds onto the table's end), so a
    scene must have enough hit twins whose term is nonzero: at least 100 in every scene that file
    traces.  Every range twin on the inner side (c_in) contributes a full, nonzero term.  Every
    twin on its side."""
    for name, make in _plan_scenes():
        sc = make()
        h, m = B.twin_outcomes(sc)
        assert h.all() and m.all(), name
        terms = B.twin_terms(sc, oracle)
        vis = B.visible_twins(sc, oracle)
        assert len(vis) == sc.n_radius and vis.sum() >= 100, (name, int(vis.sum()))
        assert np.array_equal(vis, terms[:sc.n_radius] != 0)
        hh = sc.spheres[sc.hit[:sc.n_radius], 3].astype(F64)
        assert (terms[:sc.n_radius] * hh * hh).max() < 6e-11, name       # no radius twin is more than grazing
        assert np.all(terms[sc.n_radius:] != 0), name
        if not name.startswith("lattice"):
            assert len(sc.hit) - sc.n_radius >= 100, name


def test_spotlight_weights():
    sc = B.boundary_scene("axis", "unit", "f32", seed=2, n_background=500)
    nr, n = sc.n_radius, len(sc.spheres)
    w = B.spotlight_weights(sc, 5, seed=7)
    assert w.shape == (n, 5) and w.dtype == F32
    assert np.all(w[:, 0] == 1)
    radius = np.zeros(n, bool); radius[sc.hit[:nr]] = True; radius[sc.miss[:nr]] = True
    rng_ = np.zeros(n, bool); rng_[sc.hit[nr:]] = True; rng_[sc.miss[nr:]] = True
    assert np.array_equal(w[:, 1], radius.astype(F32)) and np.array_equal(w[:, 2], rng_.astype(F32))
    assert radius.sum() == 2 * nr and rng_.sum() == 2 * (len(sc.hit) - nr) and not (radius & rng_).any()
    assert w[:, 3].min() >= -2 and w[:, 3].max() <= 2 and len(np.unique(w[:, 3])) > n // 2
    assert np.array_equal(w[:, 4], w[:, 1] * F32(0.5))
    for c in (2, 3, 4):
        assert np.array_equal(B.spotlight_weights(sc, c, seed=7), w[:, :c])
    assert np.array_equal(B.spotlight_weights(sc, 1, seed=7), w[:, 1:2])
    assert not np.array_equal(B.spotlight_weights(sc, 4, seed=8)[:, 3], w[:, 3])
