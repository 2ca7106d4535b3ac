"""The cases of point_arithmetic_cases.py are what they claim to be (CPU): properties of the inputs and of
their restated values, so that the GPU tests of test_point_arithmetic_edges.py cannot pass vacuously."""
import math

import numpy as np
import pytest

import point_arithmetic_cases as PC
import test_sph_gradients as G
from point_arithmetic_cases import F32, F64, KERNELS, MIN_NORMAL, TINY

CHUNK = 1500                                                       # pairs per sqrt scene: 3000 spheres


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def sqrt_chunks():
    cases = PC.sqrt_cases()
    return [cases[i:i + CHUNK] for i in range(0, len(cases), CHUNK)]


# ---- square roots -----------------------------------------------------------------------------------
def test_sqrt_cases_are_exact_and_hard():
    cases = PC.sqrt_cases()
    n, a, b, c = cases.T
    assert np.all(a * a + b * b + c * c == n) and np.all(np.diff(n) > 0)
    assert n.min() >= 1 << 22 and n.max() < 1 << 24 and cases[:, 1:].max() < 4096 and cases[:, 1:].min() >= 0
    assert np.any(n < 1 << 23) and np.any(n >= 1 << 23)           # both exponent parities
    x = (cases[:, 1:] * 2.0 ** -12).astype(F32)
    assert np.array_equal(x.astype(F64) * 4096.0, cases[:, 1:])
    d2 = ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]).astype(F32) + x[:, 2] * x[:, 2]).astype(F32)
    assert np.array_equal(_bits(d2), _bits(np.ldexp(n.astype(F64), -24).astype(F32)))
    assert np.array_equal(d2.astype(F64) * 2.0 ** 24, n)
    dist = np.array([PC.midpoint_distance(v) for v in n])
    assert np.sum(dist < 1e-3) >= 256, np.sum(dist < 1e-3)
    squares = np.array([math.isqrt(v) ** 2 == v for v in n])
    assert squares.sum() == 2048                                   # every m^2, m = 2048 .. 4095
    have = set(int(v) for v in n)
    assert all(m * m + 1 in have for m in range(2048, 4096))       # m^2 + 1 = m^2 + 1 + 0 always decomposes
    assert sum(m * m - 1 in have for m in range(2049, 4096)) > 1000


def test_sqrt_cases_tell_a_one_ulp_root_from_the_rounded_one():
    n = PC.sqrt_cases()[:, 0]
    R = np.array([PC.exact_root(v) for v in n], np.int64)
    for v, r in zip(n, R):                                         # r 2^-24 is the float nearest sqrt(v 2^-24)
        N = int(v) << 24
        r = int(r)
        assert (2 * r - 1) ** 2 < 4 * N < (2 * r + 1) ** 2
        w = PC.wrong_root(v)
        if math.isqrt(int(v)) ** 2 == v:
            assert w is None and r * r == N
        else:                                                      # the exact root lies strictly between r and w
            assert abs(w - r) == 1 and (r * r - N) * (w * w - N) < 0
    # NumPy's float32 square root is the correctly rounded one: the restatements may keep using it
    d2 = np.ldexp(n.astype(F64), -24).astype(F32)
    assert np.array_equal(_bits(np.sqrt(d2)), _bits(np.ldexp(R.astype(F64), -24).astype(F32)))


@pytest.mark.parametrize("scale_exp", PC.SCALE_EXPS)
def test_sqrt_scene_pairs_are_second_neighbours(scale_exp):
    for chunk in sqrt_chunks():
        sc = PC.sqrt_scene(chunk, scale_exp)
        s = sc["spheres"]
        assert len(s) <= 3000
        idx, d2 = PC.brute_knn(s, s, 2)
        assert np.array_equal(idx[:, 0], np.arange(len(s))) and np.all(d2[:, 0] == 0)
        assert np.array_equal(idx[:, 1], sc["partner"])
        assert np.array_equal(_bits(d2[:, 1]), _bits(sc["D"]))
        assert np.array_equal(_bits(np.sqrt(sc["D"])), _bits(sc["root"]))
        assert np.array_equal(_bits(PC.brute_h(s, 2, 1.0)), _bits(sc["root"]))
        squares = sc["wrong"] == sc["root"]
        assert np.array_equal(squares, np.repeat([math.isqrt(v) ** 2 == v for v in chunk[:, 0]], 2))
        assert np.all(np.abs(_bits(sc["wrong"]).astype(np.int64) - _bits(sc["root"])) == ~squares)
        if scale_exp == -50:
            assert np.all((sc["D"] < TINY) & (sc["D"] >= MIN_NORMAL))
        if scale_exp == -47:
            assert np.all(sc["D"] >= TINY) and sc["D"].min() < F32(4) * TINY


# ---- kernel knots -------------------------------------------------------------------------------------
def _knot_q_values(kernel):
    """Every restated q of the kernel's knot scenes: the field's pairs and the gather form's."""
    out = []
    for H in PC.KNOT_H:
        for qs in PC.knot_chunks(kernel):
            sc = PC.knot_scene(qs, H)
            s, pts = sc["spheres"], sc["points"]
            assert len(pts) <= 64
            pi, si, d2 = PC.pairs(pts, s)
            ih = (F32(1) / s[si, 3]).astype(F32)
            q = (np.sqrt(d2) * ih).astype(F32)
            # sphere A's points: contained, at the intended q
            own = np.nonzero(sc["owner"] == 0)[0]
            for p in own:
                m = (pi == p) & (si == 0)
                assert m.sum() == 1 and _bits(q[m])[0] == _bits(sc["q"][p:p + 1])[0], (kernel, H, p)
            a = np.abs(pts[own]).max(axis=1)
            kept = (a * a).astype(F32) > 0
            assert np.array_equal(np.sqrt((a * a).astype(F32))[kept], a[kept])
            # sphere B's points: d2 exactly the targets; the last is on the surface, in range only
            pb = np.nonzero(sc["owner"] == 1)[0]
            d = (pts[pb] - s[1, :3]).astype(F32)
            assert np.array_equal(_bits(PC._d2(d[:, 0], d[:, 1], d[:, 2])), _bits(sc["targets"]))
            H2 = F32(s[1, 3] * s[1, 3])
            assert np.array_equal(sc["targets"], [PC.ulps(H2, -1), PC.ulps(H2, -3), H2])
            assert [int(((pi == p) & (si == 1)).sum()) for p in pb] == [1, 1, 0]
            counts, offsets, gi, g2 = PC.restate_range(pts, sc["radii"], s)
            rows = np.repeat(np.arange(len(pts)), counts)
            assert all(np.any((rows == p) & (gi == 1)) for p in pb)
            gq = (np.sqrt(g2) * (F32(1) / sc["radii"][rows]).astype(F32)).astype(F32)
            assert np.all(gq <= 1) and np.all(q <= 1)              # no q > 1, in either form
            out.append((q, gq))
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_knot_scenes_take_both_branches_of_every_select(kernel):
    want = PC.knot_q(kernel)
    assert all(v in want for v in (F32(0), PC.two(-149), PC.two(-126), PC.two(-64), PC.two(-24)))
    assert all(F32(1.0 - k * 2.0 ** -24) in want for k in PC.EDGE_K)
    res = _knot_q_values(kernel)
    field = np.concatenate([q for q, _ in res])
    both = np.concatenate([np.concatenate(r) for r in res])
    # every q that does not flush is hit exactly at H = 1 (2^-149 and 2^-126 flush: d2 == 0 off the centre)
    hit = set(_bits(field).tolist())
    for v in want:
        assert (int(_bits(v)[0]) in hit) == (v == 0 or F32(v * v) > 0), (kernel, v)
    assert np.any(field == 1) and np.any(both == 1)                # contained with u == 0
    if kernel == "cubic":
        assert np.any(both < F32(0.5)) and np.any(both == F32(0.5)) and np.any(both > F32(0.5))
        assert F32(np.nextafter(F32(0.5), F32(0))) in field
    for c in PC.KNOT_CONSTANTS[kernel]:
        t = PC.clamp_arg(field, c)
        assert np.any(t > 0) and np.any(t <= 0), (kernel, c)         # t2 / t3 non-zero and clamped to zero
        kn = PC.sign_change(c)
        assert PC.clamp_arg(kn, c) <= 0 < PC.clamp_arg(np.nextafter(kn, F32(0)), c)
        assert all(F32(PC.ulps(kn, j)) in field for j in (-2, -1, 0, 1, 2))
    if kernel in ("wendland_c4", "wendland_c6"):
        u = np.maximum(F32(1) - field, F32(0))
        powers = np.concatenate(list(PC.power_forms(kernel, u).values()))
        assert np.any((powers > 0) & (powers < MIN_NORMAL)) and np.any(powers == 0), kernel
        assert len(PC.underflow_k(kernel)) >= 2
    if kernel == "wendland_c6":                                    # u^8 and p7 each pass through the subnormals to 0
        u = (np.array(PC.underflow_k(kernel)) * 2.0 ** -24).astype(F32)
        for v in PC.power_forms(kernel, u).values():
            assert np.any((v > 0) & (v < MIN_NORMAL)) and np.any(v == 0) and np.any(v >= MIN_NORMAL)


# ---- the centre ---------------------------------------------------------------------------------------
def test_centre_scene_covers_every_range_of_d2_in_one_packet():
    sc = PC.centre_scene()
    s, pts = sc["spheres"], sc["points"]
    assert len(pts) <= 64 and len(s) == 6
    pr = PC.pairs(pts, s)
    pi, si, d2 = pr
    d = G.separations(pts, s, pr)
    off_centre = (d[0] != 0) | (d[1] != 0) | (d[2] != 0)
    ranges = {"normal": d2 >= TINY, "tiny": (d2 < TINY) & (d2 >= MIN_NORMAL), "subnormal": (d2 > 0) & (d2 < MIN_NORMAL),
              "flushed": (d2 == 0) & off_centre, "centre": (d2 == 0) & ~off_centre}
    assert all(m.sum() >= 2 for m in ranges.values()), {k: int(m.sum()) for k, m in ranges.items()}
    # the lanes disagree about sqrt_rn's switch: against one sphere, some d2 are tiny and some are not
    for i in range(len(s)):
        m = si == i
        tiny = (d2[m] > 0) & (d2[m] < TINY)
        assert tiny.any() and (~tiny).any(), i
    keep = PC.never_tiny(sc)
    assert 8 <= keep.sum() < len(pts)
    w = PC.centre_weights(len(s))
    for kernel in ("cubic", "wendland_c6"):
        g32, _, _ = PC.restate_gradient(pts, pr, s, w, kernel)
        assert np.all(np.isfinite(g32)) and np.abs(g32).max() > 0
        f32, counts, _, _ = PC.restate(len(pts), pr, s, w, kernel)
        assert np.all(np.isfinite(f32)) and counts.min() >= 2 and counts.max() == 6
        for i in range(len(s)):                                    # sphere by sphere: +0 exactly where d2 == 0
            one = PC.pairs(pts, s[i:i + 1])
            g1, _, _ = PC.restate_gradient(pts, one, s[i:i + 1], w[i:i + 1], kernel)
            zero = one[0][one[2] == 0]
            assert np.all(_bits(g1[zero]) == 0)
    # the gather form meets the same ranges
    counts, _, _, g2 = PC.restate_range(pts, sc["radii"], s)
    assert counts.max() == 6 and np.sum(counts == 6) > 40 and np.any((g2 > 0) & (g2 < MIN_NORMAL)) and np.any((g2 >= MIN_NORMAL) & (g2 < TINY))


def test_overflow_scene_restates_to_infinities_and_nans():
    sc = PC.overflow_scene()
    s, pts = sc["spheres"], sc["points"]
    ih = (F32(1) / s[:, 3]).astype(F32)
    with np.errstate(over="ignore"):
        ih2 = (ih * ih).astype(F32)
        assert np.isinf((ih2 * ih2).astype(F32)).sum() == 4 and np.isinf((ih2 * ih).astype(F32)).sum() == 2
    pr = PC.pairs(pts, s)
    w = PC.centre_weights(len(s))
    w[:, 1] *= np.where(np.arange(len(s)) % 2, F32(-1), F32(1))
    with np.errstate(over="ignore", invalid="ignore"):
        g32, _, _ = PC.restate_gradient(pts, pr, s, w, "cubic")
        f32, _, _, _ = PC.restate(len(pts), pr, s, w, "cubic")
    assert np.isinf(f32).any() and np.isnan(f32).any() and np.isnan(g32).any() and np.isfinite(g32).any()


# ---- scaled scenes, the seam --------------------------------------------------------------------------
@pytest.mark.parametrize("k", PC.SCALES)
def test_scaling_by_a_power_of_two_changes_no_pair(k):
    a, b = PC.scaled_scene(0), PC.scaled_scene(k)
    sc = 2.0 ** k
    for name in ("spheres", "points", "radii"):
        assert np.array_equal(a[name].astype(F64) * sc, b[name].astype(F64), equal_nan=True)
    assert np.array_equal(a["weights"], b["weights"]) and b["high"] == (sc,) * 3
    assert len(a["spheres"]) == 3000 and len(a["points"]) == 400
    pa, pb = PC.pairs(a["points"], a["spheres"]), PC.pairs(b["points"], b["spheres"])
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]) and len(pa[0]) > 300
    assert np.array_equal(pa[2].astype(F64) * sc * sc, pb[2].astype(F64))
    ra = PC.restate_range(a["points"], a["radii"], a["spheres"])
    rb = PC.restate_range(b["points"], b["radii"], b["spheres"])
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[2], rb[2]) and ra[0].max() > 3
    ia, da = PC.brute_knn(a["points"], a["spheres"], 8)
    ib, db = PC.brute_knn(b["points"], b["spheres"], 8)
    assert np.array_equal(ia, ib) and np.array_equal(da.astype(F64) * sc * sc, db.astype(F64))
    finite = ia[:, 0] >= 0
    assert np.all(np.diff(da[finite], axis=1) > 0)                 # no ties: the ranking does not depend on the order


def test_seam_case_wraps_to_an_exact_zero_off_the_centre():
    case = PC.seam_case()
    s, pts = case["spheres"], case["points"]
    pi, si, d2 = PC.seam_pairs(case)
    for p, i in zip(case["named"], case["owner"]):
        m = pi == p
        assert m.sum() == 1 and si[m][0] == i and d2[m][0] == 0    # one sphere, at d2 == 0 exactly
        assert not np.array_equal(pts[p], s[i, :3])                # and the point is not its centre
    # the issue's (1 - 2^-24, 0.5, 0.5) and (pred(1), fl(0.5 + 2^-30), 0.5): one float32 point, d2 = 2^-48
    assert np.array_equal(pts[2], pts[3]) and pts[2, 0] == np.nextafter(F32(1), F32(0))
    for p in (2, 3):
        assert d2[(pi == p) & (si == 0)].tolist() == [2.0 ** -48]
    assert len(pts) == 34 and np.all(np.bincount(pi, minlength=len(pts))[2:] == 1)
    assert np.any((d2 > 0) & (d2 < TINY)) and np.any(d2 == 0)
