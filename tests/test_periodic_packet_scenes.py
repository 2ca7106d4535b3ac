"""CPU checks of periodic_packet_scenes.py: the cell-list link finder against the brute-force one, and that
the inputs of test_periodic_point_query_packets.py are sharp -- that their packets reach both sides of
every wave-uniform decision of the periodic walks, and that their pairs wrap.  No GPU."""
import numpy as np
import pytest

import periodic_packet_scenes as T
import periodic_point_scenes as PS
import periodic_query_scenes as S

F32 = np.float32
OPEN = (0.0, 0.0, 0.0)


def fof_b(n, period):
    return F32(0.4 * n ** (-1.0 / 3.0) * T.lmin_of(period))


# ---- the cell list ----------------------------------------------------------------------------------
@pytest.mark.parametrize("box", list(S.BOXES))
def test_cell_list_finds_the_brute_force_links(box):
    """Sorted edge sets of links_cells and S.links on torus_scene at n = 2049: b = 0 (coincident centres),
    the friends-of-friends length of the GPU module, a b of a third of the cell (three cells per axis: every
    cell is every other's neighbour, through the seam too) and b = half the smallest period (one or two
    cells per periodic axis)."""
    period = S.BOXES[box]
    n = 2049
    x = T.torus_scene(period, n, seed=n)
    lmin = T.lmin_of(period)
    for b in (F32(0.0), fof_b(n, period), F32(0.3 * lmin), S.half(lmin)):
        i, j = S.links(x, b, period)
        order = np.lexsort((j, i))
        ci, cj = T.links_cells(x, b, period)
        assert len(ci) == len(i) and np.array_equal(ci, i[order]) and np.array_equal(cj, j[order]), (box, b)
        assert len(i) >= 100 * 99 // 2                              # (the coincident group at least)
    # away from the origin, and with centres that link to nothing
    y = T.torus_scene(period, 600, seed=5, offset=100.0)
    y[7, 0] = np.nan; y[9, 2] = np.inf
    b = fof_b(600, period)
    i, j = S.links(y, b, period)
    order = np.lexsort((j, i))
    ci, cj = T.links_cells(y, b, period)
    assert np.array_equal(ci, i[order]) and np.array_equal(cj, j[order]) and not np.any(np.isin([7, 9], ci))
    assert np.array_equal(T.labels_cells(y, b, period), S.restate_labels(y, b, period))


# ---- the census's own arithmetic --------------------------------------------------------------------------
def test_census_classifies_hand_made_packets():
    """Four packets of 64, 64, 64 and 8 points at cell level 0 with boxes known by construction."""
    lo, hi = np.zeros(3, F32), np.ones(3, F32)
    rng = np.random.default_rng(1)
    # groups in Morton order: a and b in the octants 0 and 1, c and d in octant 4 with c's z below d's
    def group(k, x0, z0):
        return np.column_stack([x0 + 0.15 * rng.random(k), 0.3 + 0.15 * rng.random(k), z0 + 0.01 * rng.random(k)])
    pts = np.concatenate([group(64, 0.3, 0.05), group(64, 0.55, 0.35), group(64, 0.3, 0.60), group(8, 0.3, 0.97)]).astype(F32)
    r = np.full(len(pts), 0.01, F32)
    r[64] = 0.3                                                     # one lane makes b's box 0.6 wide
    perm = rng.permutation(len(pts))
    cen = T.packet_census(pts[perm], r[perm], lo, hi, len(pts), (1.0, 1.0, 1.0))
    assert cen["n_packets"] == 4 and cen["classified"].all()
    assert np.all(cen["box_lo"][0] > [0.28, 0.28, 0.03]) and np.all(cen["box_hi"][0] < [0.47, 0.47, 0.08])
    assert cen["is_wide"].tolist() == [False, True, False, False]
    assert cen["is_images"].tolist() == [False, False, False, False]
    # radii that reach over the faces: a through z = 0 (its image at +1 meets the root box), d through z = 1
    r[r == F32(0.01)] = 0.06
    cen = T.packet_census(pts[perm], r[perm], lo, hi, len(pts), (1.0, 1.0, 1.0))
    assert cen["is_images"].tolist() == [True, False, False, True]
    assert cen["is_wide"].tolist() == [False, True, False, False]
    # z open: nothing meets an image; x with period 1.5: b is still 0.6 wide in y, whose period is 1
    cen = T.packet_census(pts[perm], r[perm], lo, hi, len(pts), (1.5, 1.0, 0.0))
    assert cen["is_images"].tolist() == [False] * 4 and cen["is_wide"].tolist() == [False, True, False, False]
    assert cen["is_wide"].tolist() != T.packet_census(pts, r, lo, hi, len(pts), (1.5, 1.5, 0.0))["is_wide"].tolist()
    # an off point (r above half a period) does not widen its packet; a packet of off points alone is unclassified
    r[3] = 0.6
    r2 = r.copy(); r2[-8:] = np.inf
    cen = T.packet_census(pts, r2, lo, hi, len(pts), (1.0, 1.0, 1.0))
    assert cen["classified"].tolist() == [True, True, True, False] and cen["narrow"] == 2 and cen["wide"] == 1
    # wraps: one point at the corner, spheres in the far octants
    p = np.array([[0.01, 0.01, 0.01]], F32)
    x = np.array([[0.02, 0.02, 0.02, 0], [0.99, 0.02, 0.02, 0], [0.99, 0.99, 0.02, 0], [0.99, 0.99, 0.99, 0],
                  [0.02, 0.99, 0.99, 0], [0.5, 0.5, 0.5, 0]], F32)
    assert T.wrapped_pairs(p, np.array([0.05], F32), x, (1.0, 1.0, 1.0)) == (1, 2, 1)
    assert T.wrapped_pairs(p, np.array([0.05], F32), x, (1.0, 1.0, 0.0)) == (1, 1, 0)


# ---- sharpness of the matrix ---------------------------------------------------------------------------
_census = {}


def census(case):
    if case not in _census:
        _census[case] = T.case_census(case)
    return _census[case]


def test_scenes_fill_the_cell_and_straddle_the_seam():
    for box, period in S.BOXES.items():
        for offset in (0.0, 100.0):
            s = T.torus_scene(period, offset=offset)
            lo, hi = T.root_box(s)
            lmin = T.lmin_of(period)
            for a, L in enumerate(period):
                if L == 0:
                    continue
                x = s[:, a]
                assert x.min() >= F32(offset) and x.max() < F32(offset + L)           # wrapped into [0, L)
                assert x.min() < offset + 0.001 * L and x.max() > offset + 0.999 * L   # and up to both faces
                # the root box stays within about 0.04 Lmin of the cell
                assert offset - 0.045 * lmin < lo[a] <= offset and offset + L <= hi[a] < offset + L + 0.045 * lmin
            assert np.all(s[:, 3] >= F32(0.999e-3 * lmin)) and np.all(s[:, 3] <= F32(0.04 * lmin))
            # the coincident group: 100 centres one ulp inside the x face (at an offset the cast puts them on it)
            uniq, cnt = np.unique(s[:, :3], axis=0, return_counts=True)
            assert cnt.max() == T.N_CO
            co = uniq[cnt.argmax()]
            if offset == 0.0:
                assert co[0] == np.nextafter(F32(period[0]), F32(0)) and co[1] == 0


def test_matrix_holds_every_case():
    ids = [T.case_id(c) for c in T.CASES]
    assert len(ids) == len(set(ids)) == 19
    assert sum(c[0] == "cube" and c[3] == 0.0 for c in T.CASES) == 2 * len(T.SIZES_P)
    assert sorted(c[1:3] for c in T.CASES if c[0] == "slab") == sorted((m, l) for m in (2049, 16385) for l in T.LAYOUTS)
    assert ("cube", 2049, "spread", 100.0) in T.CASES
    for case in T.CASES:
        ps = T.case_points(case)
        h = S.half(T.lmin_of(S.BOXES[case[0]]))
        assert ps.rec_radii[ps.special].tolist() == [h, np.nextafter(h, F32(np.inf)), 0.0]
        assert ps.n_rec <= 16384 or ps.m < 131071
        assert np.all(np.isin(ps.special, ps.index))                 # each special record is some point's


def test_packets_reach_both_sides_of_every_decision():
    """The census of the matrix (fp64 boxes of the on lanes; packets within 1e-4 of a threshold and packets of
    off points alone left out; wraps: in-range pairs of the 2000-point sample wrapping on exactly 1 / 2 / 3 axes):

      case                   packets  wide narrow images  none  narrow&images  wraps
      cube-2047-spread            32    32      0     32     0       0         5300 / 2386 / 378
      cube-2047-clumped           32    20     12     22    10       6         1014 /  379 /  72
      cube-2048-spread            38    32      6     36     2       4         3550 / 2882 / 404
      cube-2048-clumped           36     5     30     27     8      22          744 /  457 /  90
      cube-2049-spread            38    30      8     37     1       7         3444 / 1993 / 538
      cube-2049-clumped           38     6     32     31     7      25          487 /  117 /   5
      cube-16383-spread          260    70    190    236    24     171         4005 / 3040 / 412
      cube-16383-clumped         260     7    253    168    92     161          457 /  161 /   0
      cube-16384-spread          289    49    240    246    43     204         3349 / 2298 / 462
      cube-16384-clumped         288     1    287    267    21     266         2708 / 1142 / 148
      cube-16385-spread          286    47    238    246    39     202         3874 / 1577 / 310
      cube-16385-clumped         291     1    289    261    29     260         1824 / 1091 / 236
      cube-131073-spread        2308     1   2307   1652   656    1651         4892 / 2843 / 415
      cube-131073-clumped       2321     1   2316    319  1998     318          769 /  423 /  82
      slab-2049-spread            38    34      4     35     3       2         3988 / 1077 /   0
      slab-2049-clumped           38     6     31     29     8      23          298 /  131 /   0
      slab-16385-spread          286   266     20    241    45      11         4724 /  479 /   0
      slab-16385-clumped         291     1    289    267    23     266          186 /   18 /   0
      cube-2049-spread-at100      38    30      8     37     1       7         3147 / 2091 / 539

    narrow: the survivor loops may skip the wrap (`narrow` / `plain`; the NoWrap interval in the interpolation);
    wide: they may not.  images: nodes and centres are tested against the box and its two images per axis;
    none: against the box itself (`images == false`).  At cell level 0 (2047 points) the spread layout has no
    narrow packet: only the level steps bring `plain` within reach, the clumped layout's sparse tail aside."""
    rows = {case: census(case) for case in T.CASES}
    for box in S.BOXES:
        mine = [c for case, c in rows.items() if case[0] == box]
        for name in ("wide", "narrow", "images", "none"):
            assert sum(c[name] >= 5 for c in mine) >= 2, (box, name, [c[name] for c in mine])
        assert any(c["narrow_images"] >= 5 for c in mine), box
    for case, c in rows.items():
        if case[1] == 2047 and case[2] == "spread":
            assert c["narrow"] == 0 and np.all(c["is_wide"][c["classified"]]), case
        assert np.sum(c["classified"]) >= c["n_packets"] - 6, case   # the band leaves out next to nothing
        assert sum(c["wraps"]) >= 30, (case, c["wraps"])
    cube = [c for case, c in rows.items() if case[0] == "cube"]
    assert 2 * sum(c["wraps"][1] >= 100 and c["wraps"][2] >= 100 for c in cube) >= len(cube), [c["wraps"] for c in cube]


def test_table_in_the_docstring_is_the_census():
    doc = test_packets_reach_both_sides_of_every_decision.__doc__
    table = {}
    for line in doc.splitlines():
        t = line.replace("/", " ").split()
        if len(t) == 10 and (t[0].startswith("cube-") or t[0].startswith("slab-")):
            table[t[0]] = [int(v) for v in t[1:]]
    assert len(table) == len(T.CASES)
    for case in T.CASES:
        c = census(case)
        assert table[T.case_id(case)] == [c["n_packets"], c["wide"], c["narrow"], c["images"], c["none"],
                                          c["narrow_images"], *c["wraps"]], case


def test_every_point_set_has_points_inside_more_than_a_wave_of_spheres():
    """The interpolation's counts pass 64 in every case: the point sets' off points with finite coordinates (a
    bad radius only: on for the interpolation) sit in the middle of the scene's first blob, whatever m and the
    layout.  Smallest figure over the matrix: 102 (slab), 106 (cube)."""
    for case in T.CASES:
        s = T.case_scene(case[0], case[3])[0]
        ps = T.case_points(case)
        off = ps.rec_points[-T.N_OFF:]
        off = off[np.all(np.isfinite(off), axis=1)]
        assert len(off) == 6
        assert PS.counts(off, s, S.BOXES[case[0]]).max() > 64, case


def test_sparse_scene_has_neighbours_beyond_and_well_inside_half_a_period():
    """k = 64 on 300 spheres: the k-th distance reaches h = 0.5 for queries in the void (periodic_bounds turns
    the lane into "everything") and stays below h / 2 for queries in the blob.  Figures: see the assertion."""
    s = T.sparse_scene()
    q = T.sparse_queries(s)
    assert len(s) == 300 and len(q) == 800
    _, d2 = PS.knn(q, s, 64, S.BOXES["cube"])
    rk = np.sqrt(d2[:, 63].astype(np.float64))
    far, near = int(np.sum(rk >= 0.5)), int(np.sum(rk < 0.25))
    print("sparse scene, k = 64: %d rows with the k-th distance >= h, %d below h / 2, of %d" % (far, near, len(q)))
    assert far >= 50 and near >= 50, (far, near)
    # its first 40 spheres alone: every row of k = 64 is padded
    _, d2 = PS.knn(q[:50], s[:40], 64, S.BOXES["cube"])
    assert np.all(np.isfinite(d2[:, :40])) and np.all(np.isposinf(d2[:, 40:]))


@pytest.mark.parametrize("box,n", [("cube", n) for n in (2047, 2048, 2049, 16383, 16384, 16385)]
                         + [("slab", 2049), ("slab", 16385)])
def test_fof_scenes_link_across_the_seam(box, n):
    """At b = 0.4 n^(-1/3) Lmin the periodic components are not the open ones, and the coincident 100 sit in a
    component with members on both sides of the x face."""
    period = S.BOXES[box]
    x = T.torus_scene(period, n, seed=n)
    b = fof_b(n, period)
    torus, plain = T.labels_cells(x, b, period), T.labels_cells(x, b, OPEN)
    assert np.sum(torus != plain) > 100 and len(np.unique(torus)) < len(np.unique(plain))
    uniq, inv, cnt = np.unique(x[:, :3], axis=0, return_inverse=True, return_counts=True)
    group = np.nonzero(inv.reshape(-1) == cnt.argmax())[0]
    assert len(group) == T.N_CO and len(np.unique(torus[group])) == 1
    members = x[torus == torus[group[0]], 0]
    L = period[0]
    assert len(members) > T.N_CO and members.min() < 0.25 * L and members.max() > 0.75 * L
    assert np.bincount(T.labels_cells(x, F32(0), period)).max() == T.N_CO
