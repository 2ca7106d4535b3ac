"""Case builders for the fp32 arithmetic of the point walks at its rounding edges (NumPy only, deterministic):
the correctly rounded square root and its switch at 2^-96, the knots and clamps of the SPH kernel forms, the
support edge where powers of u underflow, separations next to a sphere's centre, inverse powers of H that
overflow, scenes scaled by powers of two and a wrapped separation that rounds to zero.

The restatements are the existing ones (test_sph_interpolation, test_sph_gradients, test_range_queries,
test_neighbours, periodic_point_scenes); this file only chooses inputs.  test_point_arithmetic_cases.py checks
on the CPU that the inputs are what they claim to be, test_point_arithmetic_edges.py runs them on the GPU."""
import functools
import math

import numpy as np

import periodic_point_scenes as PS
import test_sph_gradients as G
import test_sph_interpolation as T
from test_neighbours import brute_h, brute_knn  # noqa: F401  (re-exported for the two test modules)
from test_range_queries import restate as restate_range, restate_sums  # noqa: F401
from test_sph_gradients import df32_kernel, restate_gradient  # noqa: F401
from test_sph_interpolation import f32_kernel, lattice, pairs, restate  # noqa: F401

F32, F64 = np.float32, np.float64
KERNELS = T.KERNELS
TINY = F32(2.0 ** -96)                       # sqrt_rn's switch: 0 < d2 < TINY takes the general square root
MIN_NORMAL = F32(2.0 ** -126)
SCALE_EXPS = (0, -47, -50, 40)
SCALES = (-24, -12, 12, 24)


def two(e):
    """2^e as a float32 (e >= -149)."""
    return F32(2.0 ** e)


def ulps(x, j):
    """The float32 j steps from x > 0 (array or scalar)."""
    return (np.asarray(x, F32).view(np.int32) + np.int32(j)).view(F32)


# ---- square roots -----------------------------------------------------------------------------------
N_LO, N_HI = 1 << 22, 1 << 24
N_HARD, N_RANDOM = 512, 256


def exact_root(n):
    """R with fl(sqrt(n 2^-24)) = R 2^-24, in integers: the root lies in [2^-1, 1), where floats are 2^-24
    apart, so R = round(sqrt(n 2^24)); the midpoint k + 1/2 is no root of an integer, so there are no ties."""
    N = int(n) << 24
    k = math.isqrt(N)
    return k + (N > k * k + k)                                     # sqrt(N) > k + 1/2  <=>  N > k^2 + k + 1/4


def wrong_root(n):
    """The float on the other side of the exact root (the answer of a 1-ulp square root that rounded the
    wrong way), as an integer like exact_root; None for a perfect square."""
    N, R = int(n) << 24, exact_root(n)
    if R * R == N:
        return None
    return R - 1 if R * R > N else R + 1


def midpoint_distance(n):
    """|sqrt(n 2^24) - (k + 1/2)| in ulp of the root, k = isqrt(n 2^24): from the exact integer
    4 N - (2k + 1)^2, divided by 4 (sqrt(N) + k + 1/2)."""
    N = int(n) << 24
    k = math.isqrt(N)
    return abs(4 * N - (2 * k + 1) ** 2) / (4.0 * (math.sqrt(N) + k + 0.5))


def _decomposable(n):
    """Legendre: n is a sum of three squares unless n = 4^j (8 m + 7)."""
    m = np.array(n, np.int64, copy=True)
    for _ in range(12):
        m = np.where((m & 3) == 0, m >> 2, m)
    return (m & 7) != 7


def _decompose(n):
    """(a, b, c) with a^2 + b^2 + c^2 = n, the largest a first."""
    a = math.isqrt(n)
    while a >= 0:
        rem = n - a * a
        b = np.arange(math.isqrt(rem) + 1, dtype=np.int64)
        c2 = rem - b * b
        c = np.floor(np.sqrt(c2.astype(F64))).astype(np.int64)     # exact below 2^53
        hit = np.nonzero(c * c == c2)[0]
        if len(hit):
            return a, int(b[hit[0]]), int(c[hit[0]])
        a -= 1
    raise ValueError(n)


@functools.lru_cache(maxsize=None)
def sqrt_cases():
    """int64 [m, 4] rows (n, a, b, c), n ascending and distinct: n in [2^22, 2^24) with n = a^2 + b^2 + c^2.
    With separations a 2^-12, b 2^-12, c 2^-12 every square and partial sum of d2 is an integer below 2^24
    times 2^-24, so d2 = n 2^-24 exactly, in [2^-2, 1): both exponent parities.
    Contents: every perfect square and its two neighbours where they decompose; the N_HARD decomposable n of
    the whole range (about 10^7 of them) whose root lies nearest the midpoint of two floats; N_RANDOM random."""
    ns = set()
    for m in range(2048, 4096):
        for n in (m * m - 1, m * m, m * m + 1):
            if N_LO <= n < N_HI and _decomposable(n):
                ns.add(n)
    best_n, best_d, enumerated = [], [], 0
    for lo in range(N_LO, N_HI, 1 << 20):
        n = np.arange(lo, lo + (1 << 20), dtype=np.int64)
        n = n[_decomposable(n)]
        enumerated += len(n)
        x = np.sqrt(n.astype(F64)) * 4096.0                        # the root in ulp, to 2^-28
        dist = np.abs((x - np.floor(x)) - 0.5)
        keep = np.argsort(dist, kind="stable")[:N_HARD]
        best_n.append(n[keep]); best_d.append(dist[keep])
    assert enumerated >= 10 ** 6
    best_n, best_d = np.concatenate(best_n), np.concatenate(best_d)
    ns.update(int(v) for v in best_n[np.argsort(best_d, kind="stable")[:N_HARD]])
    rng = np.random.default_rng(96)
    r = rng.integers(N_LO, N_HI, 4 * N_RANDOM)
    ns.update(int(v) for v in r[_decomposable(r)][:N_RANDOM])
    rows = []
    for i, n in enumerate(sorted(ns)):
        abc = _decompose(n)
        rows.append((n, *(abc[(i + j) % 3] for j in range(3))))    # the long component on every axis in turn
    return np.array(rows, np.int64)


def sqrt_scene(cases, scale_exp):
    """One pair of spheres per case: c_t on an integer lattice of spacing 4 and c_t + (a, b, c) 2^-12, all times
    2^scale_exp.  Every coordinate is exact in 24 bits, a pair's separation is below 1 and every other centre
    at least 3 away on some axis, so each sphere's second neighbour is its partner at D = n 2^(2 scale_exp - 24).
    Returns spheres [2m, 4] (sphere 2t and 2t + 1 are pair t), partner [2m], D [2m], root [2m] (the correctly
    rounded sqrt(D) from exact_root), wrong [2m] (wrong_root; the root itself for perfect squares)."""
    cases = np.asarray(cases, np.int64)
    m = len(cases)
    side = max(1, int(math.ceil(m ** (1.0 / 3.0) - 1e-9)))
    t = np.arange(m)
    ct = 4.0 * np.stack([t % side, (t // side) % side, t // (side * side)], axis=1).astype(F64)
    assert side ** 3 >= m and ct.max(initial=0.0) + 1.0 < 4096.0
    x = np.empty((2 * m, 4), F64)
    x[0::2, :3] = ct
    x[1::2, :3] = ct + cases[:, 1:4] / 4096.0
    x[:, 3] = 1.0
    x = np.ldexp(x, scale_exp)
    s = x.astype(F32)
    assert np.array_equal(s.astype(F64), x)                        # exact in float32
    R = np.array([exact_root(n) for n in cases[:, 0]], np.int64)
    Rw = np.array([wrong_root(n) or exact_root(n) for n in cases[:, 0]], np.int64)
    to32 = lambda v, e: np.repeat(np.ldexp(v.astype(F64), e), 2).astype(F32)
    return {"spheres": s, "partner": np.arange(2 * m) ^ 1, "D": to32(cases[:, 0], 2 * scale_exp - 24),
            "root": to32(R, scale_exp - 24), "wrong": to32(Rw, scale_exp - 24)}


# ---- kernel knots -------------------------------------------------------------------------------------
KNOT_CONSTANTS = {"cubic": (), "quartic": (0.4, 0.8), "quintic": (1.0 / 3.0, 2.0 / 3.0), "wendland_c2": (),
                  "wendland_c4": (), "wendland_c6": ()}
EDGE_K = (1, 2, 3, 4, 8, 16, 32, 64, 128, 256)


def clamp_arg(q, c):
    """fl(fl(1 - q) - c): the argument of the quartic's and quintic's max(., 0)."""
    q = np.asarray(q, F32)
    return ((F32(1) - q).astype(F32) - F32(c)).astype(F32)


def sign_change(c):
    """The smallest float32 q with fl(fl(1 - q) - c) <= 0 (its predecessor has a positive argument)."""
    q = F32(F32(1) - F32(c))
    while clamp_arg(q, c) <= 0:
        q = np.nextafter(q, F32(0))
    while clamp_arg(q, c) > 0:
        q = np.nextafter(q, F32(1))
    return F32(q)


def power_forms(kernel, u):
    """The powers of u that the Wendland C4 and C6 forms of f and f' take, in their fp32 operation order."""
    u = np.asarray(u, F32)
    u2 = (u * u).astype(F32)
    p4 = (u2 * u2).astype(F32)
    if kernel == "wendland_c6":
        return {"u8": (p4 * p4).astype(F32), "p7": ((p4 * u2).astype(F32) * u).astype(F32)}
    if kernel == "wendland_c4":
        return {"u6": (p4 * u2).astype(F32), "p5": (p4 * u).astype(F32)}
    return {}


def underflow_k(kernel):
    """The k of u = k 2^-24 (the u of q = 1 - k 2^-24, the only u below 2^-12 that fl(1 - q) can give) at
    which each power first becomes subnormal and first becomes 0 on the way to the edge, each with the k
    just outside, found by evaluating the fp32 forms at k = 1 .. 4096.  (p5(2^-24) = 2^-120 is still normal,
    and u^6 never reaches 0: the C4 powers vanish only at u == 0.)"""
    k = np.arange(1, 4097)
    out = set()
    for v in power_forms(kernel, (k * 2.0 ** -24).astype(F32)).values():
        for mask in ((v > 0) & (v < MIN_NORMAL), v == 0):
            if mask.any():
                top = int(k[mask].max())
                out.update((top, top + 1))
    return sorted(out)


def knot_q(kernel):
    """The float32 q to hit, ascending: 0 and tiny values, every knot of the kernel's selects and clamps with
    its neighbours at 0, +-1, +-2 ulp, the last floats below 1, and the u where powers underflow."""
    q = [F32(0), two(-149), two(-126), two(-64), two(-24)]
    knots = [F32(0.5)] if kernel == "cubic" else [sign_change(c) for c in KNOT_CONSTANTS[kernel]]
    for kn in knots:
        q += [F32(ulps(kn, j)) for j in (-2, -1, 0, 1, 2)]
    q += [F32(1.0 - k * 2.0 ** -24) for k in EDGE_K]
    q += [F32(1.0 - k * 2.0 ** -24) for k in underflow_k(kernel)]
    return np.unique(np.array(q, F32))


def _d2(dx, dy, dz):
    return ((dx * dx + dy * dy).astype(F32) + dz * dz).astype(F32)


@functools.lru_cache(maxsize=None)
def edge_sphere(scale):
    """(HB, offsets [3, 3], targets [3]): a radius that is no power of two, near 0.3 `scale`, with
    fl(sqrt(pred(fl(HB HB))) * fl(1 / HB)) == 1, and offsets (0, dy, dz) found by search whose d2 is exactly
    pred(fl(HB HB)), that d2 two ulp further in, and fl(HB HB) itself."""
    rng = np.random.default_rng(5)
    for j in range(64):
        HB = F32(F32(0.3 * (1.0 + j / 64.0)) * F32(scale))
        H2 = F32(HB * HB)
        ih = F32(F32(1) / HB)
        if F32(np.sqrt(ulps(H2, -1)) * ih) == F32(1):
            break
    else:
        raise ValueError("no radius with q == 1 inside")
    targets = np.array([ulps(H2, -1), ulps(H2, -3), H2], F32)
    offs = []
    for i, T_ in enumerate(targets):
        while True:
            dy = F32(np.sqrt(F64(T_)) * rng.uniform(0.3, 0.9))
            z0 = F32(np.sqrt(max(F64(T_) - F64(dy) ** 2, 0.0)))
            dz = ulps(z0, np.arange(-32, 33))
            hit = np.nonzero(_d2(F32(0), dy, dz) == T_)[0]
            if len(hit):
                sy, sz = (1, -1) if i % 2 else (-1, 1)
                offs.append((F32(0), F32(sy) * dy, F32(sz) * dz[hit[0]]))
                break
    return HB, np.array(offs, F32), targets


KNOT_DIRS = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, -1)], F32)
KNOT_CHUNK = 15                                                    # 4 * 15 + 3 points: one packet


def knot_scene(qs, H):
    """Sphere A at the origin with H a power of two (ih exact) and points (q H) e along four axis directions:
    sqrt(fl(a^2)) == |a| wherever a^2 does not underflow, so q is hit exactly; where fl(a^2) is 0 (q H below
    2^-75) the point is off the centre at d2 == 0 and the q it hits is 0.  Sphere B at (8 H, 0, 0) with
    edge_sphere's radius and its three points.  A far sphere, and a sphere of radius 0 (it contains nothing)
    at every point, so that in the gather form (range sums at these points with the radii below) the same
    d2 and q arise against A and B.
    Returns spheres [n, 4] (A, B, far, then one per point), points [m, 3], owner [m] (0: A, 1: B),
    q [m] (the q intended against the owner; NaN for B's points), radii [m] (the owner's H),
    targets [3] (the d2 of B's points)."""
    qs = np.asarray(qs, F32)
    H = F32(H)
    assert len(qs) <= KNOT_CHUNK and np.log2(float(H)) % 1.0 == 0.0
    a = (qs * H).astype(F32)
    assert np.all((a.astype(F64) == qs.astype(F64) * float(H)) | (a == 0))
    flushed = (a * a).astype(F32) == 0
    pa = (a[:, None, None] * KNOT_DIRS[None, :, :]).reshape(-1, 3).astype(F32)
    HB, offs, targets = edge_sphere(float(H))
    cb = np.array([F32(8) * H, 0, 0], F32)
    pb = (cb[None, :] + offs).astype(F32)
    assert np.array_equal((pb - cb[None, :]).astype(F32), offs)
    points = np.concatenate([pa, pb]).astype(F32)
    main = np.array([[0, 0, 0, H], [cb[0], 0, 0, HB], [F32(64) * H, F32(64) * H, F32(64) * H, H]], F32)
    helpers = np.concatenate([points, np.zeros((len(points), 1), F32)], axis=1)
    owner = np.concatenate([np.zeros(len(pa), np.int64), np.ones(len(pb), np.int64)])
    q = np.concatenate([np.repeat(np.where(flushed, F32(0), qs), 4), np.full(3, np.nan, F32)]).astype(F32)
    return {"spheres": np.concatenate([main, helpers]).astype(F32), "points": points, "owner": owner, "q": q,
            "radii": np.where(owner == 0, H, HB).astype(F32), "targets": targets}


def knot_chunks(kernel):
    q = knot_q(kernel)
    return [q[i:i + KNOT_CHUNK] for i in range(0, len(q), KNOT_CHUNK)]


KNOT_H = (1.0, 2.0 ** -20)


# ---- the centre ---------------------------------------------------------------------------------------
CENTRE_RADII = (2.0 ** -10, 2.0 ** -20, 2.0 ** -31)
OVERFLOW_RADII = (2.0 ** -10, 2.0 ** -33, 2.0 ** -43)             # fl(ih^4) = +inf; fl(ih^3) = +inf as well
CENTRES = np.array([(0.0, 0.0, 0.0), (2.0 ** -50, -2.0 ** -50, 2.0 ** -51)], F32)
CENTRE_LENGTHS = tuple(F32(2.0 ** e) for e in (-21, -40, -47.5, -48, -49, -55, -63, -64, -70, -74, -75, -76)) + (F32(0),)
GATHER_RADIUS = F32(2.0 ** -20)


def _representable(c, off):
    """c + off is a float32 in every component and fl((c + off) - c) == off."""
    p = c.astype(F64) + off.astype(F64)
    p32 = p.astype(F32)
    return np.array_equal(p32.astype(F64), p) and np.array_equal((p32 - c).astype(F32), off)


def centre_scene(radii=CENTRE_RADII):
    """Spheres of the given radii at 0 and at (2^-50, -2^-50, 2^-51), and at most 64 points at offsets from the
    two centres: along an axis at the lengths 2^-21 .. 2^-76 and 0, and along a diagonal with every component of
    that length, with the axis and the signs chosen per centre so that the offset is exactly representable
    there (next to 2^-50 nothing is 2^-76 away, and 2^-75 only below 2^-51); three more at ordinary q.  Every
    point lies in the spheres of both centres, so its d2 runs through ordinary, tiny, subnormal and flushed
    values within one packet, and the lanes of the wave disagree about sqrt_rn's switch.
    Returns spheres [6, 4], points [m, 3], centre [m] (the centre an offset was taken from), offsets [m, 3],
    radii [m] (for the gather form: 2^-20)."""
    spheres = np.array([(*c, F32(h)) for c in CENTRES for h in radii], F32)
    axes = [np.array(v, F32) for v in ((1, 0, 0), (-1, 0, 0), (0, 0, -1), (0, 1, 0), (0, -1, 0), (0, 0, 1))]
    diagonals = [np.array((sx, sy, sz), F32) for sx in (1, -1) for sy in (-1, 1) for sz in (1, -1)]
    pts, centre, offsets = [], [], []
    for ci, c in enumerate(CENTRES):
        for L in CENTRE_LENGTHS:
            for dirs in (axes, diagonals):
                if L == 0 and dirs is diagonals:
                    continue
                off = next((d * L for d in dirs if _representable(c, (d * L).astype(F32))), None)
                if off is None:
                    continue
                off = (off + F32(0)).astype(F32)                   # -0 -> +0
                pts.append((c + off).astype(F32)); centre.append(ci); offsets.append(off)
    for off in ((0.3, 0.2, -0.4), (-0.05, 0.6, 0.1), (0.0, 0.0, 0.9)):
        off = (np.array(off, F32) * F32(radii[0])).astype(F32)
        pts.append(off); centre.append(0); offsets.append(off)
    points, offsets = np.array(pts, F32), np.array(offsets, F32)
    centre = np.array(centre)
    assert len(points) <= 64
    for p, ci, off in zip(points, centre, offsets):                # every offset is exact at its centre
        assert np.array_equal(p.astype(F64) - CENTRES[ci].astype(F64), off.astype(F64))
        assert np.array_equal((p - CENTRES[ci]).astype(F32), off)
    return {"spheres": spheres, "points": points, "centre": centre, "offsets": offsets,
            "radii": np.full(len(points), GATHER_RADIUS, F32)}


def never_tiny(scene):
    """The points none of whose pairs, contained (field, gradient) or in range (gather), has 0 < d2 < 2^-96: a
    wave of these alone never takes sqrt_rn's general path."""
    pi, _, d2 = pairs(scene["points"], scene["spheres"])
    counts, _, _, g2 = restate_range(scene["points"], scene["radii"], scene["spheres"])
    gi = np.repeat(np.arange(len(counts)), counts)
    ok = np.ones(len(scene["points"]), bool)
    ok[pi[(d2 > 0) & (d2 < TINY)]] = False
    ok[gi[(g2 > 0) & (g2 < TINY)]] = False
    return ok


def overflow_scene():
    """centre_scene with H = 2^-33 (fl(ih^4) = +inf) and H = 2^-43 (fl(ih^3) = +inf too): the restatement
    yields +-inf and NaN by IEEE rules."""
    return centre_scene(OVERFLOW_RADII)


def centre_weights(n, n_ch=2, seed=8):
    return (0.5 + np.random.default_rng(seed).random((n, n_ch))).astype(F32)


# ---- scaled scenes ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unit_scene():
    s = T._random_scene(3000, 29, 0.03, 0.08)
    s[50] = G.SURFACE
    pts = G._base_points(s, 17)
    r = np.exp(np.random.default_rng(31).uniform(np.log(0.01), np.log(0.08), len(pts))).astype(F32)
    return s, pts, r, T._weights(len(s), 3, 37)


def scaled_scene(k):
    """3000 random spheres in the unit box with H in [0.03, 0.08], test_sph_gradients' 400 base points (a
    centre, a surface point and a NaN point among them) and a radius per point for the gather form, all
    times 2^k (exact); the weights are left alone.  Returns spheres [3000, 4] in the generator's order,
    points [400, 3], radii [400], weights [3000, 3], low / high (the scaled unit box)."""
    s, pts, r, w = _unit_scene()
    sc = F32(2.0 ** k)
    return {"spheres": (s * sc).astype(F32), "points": (pts * sc).astype(F32), "radii": (r * sc).astype(F32),
            "weights": w, "low": (0.0, 0.0, 0.0), "high": (float(sc),) * 3}


# ---- the seam -----------------------------------------------------------------------------------------
SEAM_PERIOD = (1.0, 1.0, 0.0)


def seam_case():
    """Period (1, 1, 0); sphere 0 at (2^-60, 0.5, 0.5), sphere 1 at (0.25, 2^-60, 0.25), both with H = 2^-3.
    Named points (the first two): (1, 0.5, 0.5) and (0.25, 1, 0.25) -- fl(1 - 2^-60) = 1 = L, so the wrapped
    separation is exactly 0 for a point that is not at the centre (on the torus it is 2^-60 away).
    Then the points (1 - 2^-24, 0.5, 0.5) and (pred(1), fl(0.5 + 2^-30), 0.5) (one float32 point, twice: their
    separation rounds to pred(L), the wrapped d2 is 2^-48) and 30 more a few ulp on either side of both x faces:
    at x = 0 these are subnormals and the neighbours of the centre's 2^-60, at x = 1 the floats around 1.
    Returns spheres [2, 4], points [34, 3], named (indices of the named points), owner (their spheres)."""
    c = two(-60)
    spheres = np.array([(c, 0.5, 0.5, 0.125), (0.25, c, 0.25, 0.125)], F32)
    one = F32(1)
    xs = [one - two(-24), np.nextafter(one, F32(0))]
    xs += [F32(ulps(one, j)) for j in (-4, -3, -2, 1, 2, 3, 4)]                            # 7 around x = 1
    lo = [two(-149), F32(3) * two(-149), two(-126), two(-61), F32(ulps(c, -1)), c, F32(ulps(c, 1)), two(-59),
          two(-30), two(-24)]
    xs += [F32(0)] + lo + [-v for v in lo] + [-one, F32(ulps(one, -1)) - one]               # 23 around x = 0
    pts = [(1.0, 0.5, 0.5), (0.25, 1.0, 0.25)]
    pts += [(x, F32(0.5 + 2.0 ** -30) if i == 1 else 0.5, 0.5) for i, x in enumerate(xs)]
    points = np.array(pts, F32)
    assert len(points) == 34
    return {"spheres": spheres, "points": points, "named": np.array([0, 1]), "owner": np.array([0, 1]),
            "period": SEAM_PERIOD}


def seam_pairs(case):
    return PS.pairs(case["points"], case["spheres"], case["period"])
