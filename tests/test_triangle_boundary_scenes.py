"""CPU checks of tests/triangle_boundary_scenes.py with the oracle alone: every designed case sits
where the generator says it sits, so that the GPU tests that trace these scenes test what they
claim to test."""
import functools

import numpy as np
import pytest

import triangle_boundary_scenes as T

F32 = np.float32
KINDS = ("axis", "pinhole", "iso", "general")
SCALES = tuple(T.TWIN_SCALES)


@functools.lru_cache(maxsize=None)
def twin_scene(kind, scale):
    return T.edge_twin_scene(kind, scale, seed=1)


@functools.lru_cache(maxsize=None)
def twin_answers(kind, scale):
    import oracle as O
    sc = twin_scene(kind, scale)
    return O.brute_closest_tri(sc.rays, sc.tris)[0]


@pytest.mark.parametrize("axis,sense", [(2, -1), (2, 1), (0, 1), (0, -1), (1, 1), (1, -1)])
@pytest.mark.parametrize("scale", list(T.TIE_SCALES))
def test_tie_scenes_tie(oracle, scale, axis, sense):
    """All 4225 rays hit at t = 0.75 s exactly; 4095 of them tie (96.9 %, at least 90 % asked):
    brute force in ascending and in descending index order names different triangles, exactly for
    the rays the generator marks."""
    sc = T.tie_scene(scale, False, axis, sense)
    assert len(sc.tris) == 2048 and len(sc.rays) == 4225
    up, t = oracle.brute_closest_tri(sc.rays, sc.tris)
    down, t2 = T.brute_descending(sc.rays, sc.tris)
    assert np.all(up >= 0) and np.all(down >= 0)
    assert np.all(t == sc.t) and np.all(t2 == sc.t)
    assert np.array_equal(up != down, sc.tie)
    assert sc.tie.sum() == 4095 and sc.tie.mean() >= 0.9
    assert np.all(up >= down)                                   # the last candidate wins a tie


@pytest.mark.parametrize("scale", list(T.TIE_SCALES))
def test_coplanar_sheets_tie_everywhere(oracle, scale):
    sc = T.tie_scene(scale, True)
    assert len(sc.tris) == 2048 + 32
    up, t = oracle.brute_closest_tri(sc.rays, sc.tris)
    down, _ = T.brute_descending(sc.rays, sc.tris)
    assert np.all(t == sc.t) and np.all(up != down) and sc.tie.all()
    # ties between triangles far apart in index: the two sheets are shuffled into one array
    assert np.median(up - down) > 100


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("kind", KINDS)
def test_twins_sit_on_their_side(oracle, kind, scale):
    """Every accepting twin (and every other designed winner) is the brute-force answer of its
    target ray; no rejecting twin (or designed loser) is the answer of its ray."""
    sc, ref = twin_scene(kind, scale), twin_answers(kind, scale)
    assert np.array_equal(ref[sc.win_ray], sc.win_tri)
    assert not np.any(ref[sc.lose_ray] == sc.lose_tri)
    # pair by pair, with the oracle's own values
    w, l = sc.pair_win, sc.pair_lose
    edge = np.isin(sc.win_sort[w], T.EDGE_SORTS)
    aw, _, _, _, tw = T.accepts(sc.rays[sc.win_ray[w]], sc.tris[sc.win_tri[w]])
    al, _, u, v, tl = T.accepts(sc.rays[sc.lose_ray[l]], sc.tris[sc.lose_tri[l]])
    assert aw.all() and not al[edge].any()
    for i in np.nonzero(edge)[0]:
        assert T._rejected_as(sc.win_sort[w][i], u[i:i + 1], v[i:i + 1])[0]
    # length twins: the triangle is accepted by both copies' geometry; only the length decides
    ln = ~edge
    assert al[ln].all() and np.array_equal(tw[ln], tl[ln])
    Lw, Ll = sc.rays[sc.win_ray[w][ln], 6], sc.rays[sc.lose_ray[l][ln], 6]
    assert np.all(tw[ln] <= Lw * T.LEN_FACTOR) and not np.any(tl[ln] <= Ll * T.LEN_FACTOR)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("kind", KINDS)
def test_twins_differ_by_one_float(kind, scale):
    sc = twin_scene(kind, scale)
    w, l = sc.pair_win, sc.pair_lose
    assert np.array_equal(sc.win_sort[w], sc.lose_sort[l])
    for a, b, sort in zip(w, l, sc.win_sort[w]):
        if sort == "len":
            assert sc.win_tri[a] == sc.lose_tri[b] and sc.win_ray[a] ^ 1 == sc.lose_ray[b]
            ra, rb = sc.rays[sc.win_ray[a]], sc.rays[sc.lose_ray[b]]
            assert np.array_equal(ra[:6].view(np.uint32), rb[:6].view(np.uint32))
            assert np.nextafter(ra[6], F32(0)) == rb[6]
        else:
            assert sc.win_ray[a] == sc.lose_ray[b]
            ta, tb = sc.tris[sc.win_tri[a]], sc.tris[sc.lose_tri[b]]
            diff = np.nonzero(ta.view(np.uint32) != tb.view(np.uint32))[0]
            assert len(diff) == 1 and diff[0] < 3
            k = diff[0]
            assert np.nextafter(ta[k], tb[k]) == tb[k]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_scene_has_twenty_twins_of_each_sort(kind, scale):
    sc = twin_scene(kind, scale)
    sorts = sc.win_sort[sc.pair_win]
    for s in T.TWIN_SORTS:
        assert (sorts == s).sum() >= 20, (s, (sorts == s).sum())
    # the other designed cases are there as well
    for s in ("near0", "nearb", "edgeon", "back"):
        assert (sc.lose_sort == s).sum() >= 4, s
    assert (sc.win_sort == "nearf").sum() >= (0 if kind in ("pinhole", "iso") else 4)


@pytest.mark.parametrize("scale", ["1e3", "1e5"])
def test_exact_and_ragged_vertex_sums(scale):
    """At 1e3 and 1e5 one variant's v + e1, v + e2 are floats, the other's are not."""
    for name, want in ((scale, True), (scale + "r", False)):
        t = twin_scene("axis", name).tris.astype(np.float64)
        s1, s2 = t[:, :3] + t[:, 3:6], t[:, :3] + t[:, 6:9]
        exact = np.all(s1 == s1.astype(F32), axis=1) & np.all(s2 == s2.astype(F32), axis=1)
        assert (exact.mean() > 0.99) if want else (exact.mean() < 0.2), (name, exact.mean())


def test_near_end_and_face_cases(oracle):
    sc = twin_scene("general", "unit")
    for sort, where in (("near0", "lose"), ("nearb", "lose"), ("nearf", "win"), ("edgeon", "lose"), ("back", "lose")):
        tri = getattr(sc, where + "_tri")[getattr(sc, where + "_sort") == sort]
        ray = getattr(sc, where + "_ray")[getattr(sc, where + "_sort") == sort]
        hit, det, u, v, t = oracle.tri_intersect_pairs(sc.rays[ray], sc.tris[tri])
        if sort == "near0":
            assert hit.all() and np.all(t == 0)            # in the plane: only t >= 1e-14 rejects it
        elif sort == "nearb":
            assert hit.all() and np.all(t < 0)
        elif sort == "nearf":
            assert hit.all() and np.all(t > 0) and np.all(t < 1e-3)
        elif sort == "edgeon":
            assert np.all(det == 0) and not hit.any()
        else:
            assert np.all(det < 0) and not hit.any()


@pytest.mark.parametrize("kind,n", [("icosphere", 513), ("icosphere", 70001), ("soup", 9), ("soup", 4097),
                                    ("sheets", 512), ("sheets", 4097), ("repeated", 511)])
def test_mesh_scenes_hit_and_miss(oracle, kind, n):
    sc = T.mesh_scene(kind, n)
    assert len(sc.tris) == n and len(sc.rays) == 4133 and len(sc.rays) % 64 != 0
    ref, _ = oracle.brute_closest_tri(sc.rays, sc.tris)
    assert (ref >= 0).sum() >= 20 and (ref < 0).sum() >= 20
    assert not np.isin(ref, sc.invalid).any()
    bad = T.invalid_triangles(30, np.random.default_rng(3))
    assert np.all(oracle.brute_closest_tri(sc.rays[:256], bad)[0] == -1)
    if kind == "repeated":
        assert set(ref.tolist()) == {-1, n - 1}               # an n-fold tie: the last one wins


def test_icosphere_is_closed_with_front_and_back_faces(oracle):
    V, Fc = T._icosphere(3)
    e = np.sort(np.concatenate([Fc[:, [0, 1]], Fc[:, [1, 2]], Fc[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert len(Fc) == 1280 and np.all(counts == 2)             # every edge shared by two faces
    sc = T.mesh_scene("icosphere", 1280 + 1)
    _, det, _, _, _ = oracle.tri_intersect_pairs(np.repeat(sc.rays[1024 + 528][None], len(sc.tris), 0), sc.tris)
    assert (det > 0).sum() > 300 and (det < 0).sum() > 300


@pytest.mark.parametrize("n", [4097, 70001])
def test_stacked_sheets_are_crossed_many_times(oracle, n):
    """At least a quarter of the rays cross three or more of the eight sheets."""
    sc = T.mesh_scene("sheets", n)
    crossed = np.zeros(len(sc.rays), int)
    for k in range(8):
        crossed += oracle.brute_closest_tri(sc.rays, sc.tris[sc.sheet == k])[0] >= 0
    assert (crossed >= 3).mean() >= 0.25, (crossed >= 3).mean()


def test_soup_spans_three_decades_with_needles():
    t = T.mesh_scene("soup", 4097).tris.astype(np.float64)
    t = t[np.isfinite(t).all(axis=1)]
    l1, l2 = np.linalg.norm(t[:, 3:6], axis=1), np.linalg.norm(t[:, 6:9], axis=1)
    ok = (l1 > 0) & (l2 > 0)
    assert l1[ok].max() / l1[ok].min() > 500
    assert ((l1[ok] / l2[ok]) > 500).sum() > 100                  # needles
    assert (np.minimum(l1, l2) > 0.9).sum() >= 3                   # as large as the box
