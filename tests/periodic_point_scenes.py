"""Scenes and the NumPy restatement for the periodic nearest neighbours, smoothing lengths and SPH
interpolation (grace_nearest_neighbours_periodic_f4, grace_smoothing_lengths_periodic_f4,
grace_interpolate_points_periodic_f4, grace_interpolate_grid_periodic_f4).

The restatement is the contract of include/grace_hip.h, "Periodic boxes": the wrapped fp32 d2 of
periodic_query_scenes.d2_rows (at most one wrap per component), and everything downstream the open
functions' own -- the ranking (d2, tree index) of test_neighbours.brute_knn, h = fl(eta sqrt(D)),
containment d2 < fl(H H) and the class-ordered sums of test_sph_interpolation.restate, which takes the
pairs of this file unchanged.  A sphere whose H exceeds fl(0.5 L) on a periodic axis is off: it
contains no point.

The scenes build on periodic_query_scenes: its full 16^3 lattice (every site is every other's
translate), its uniform boxes and query points, its seam and corner spine; here the spheres get radii
of their own, with the contract's edge values first."""
import numpy as np

import periodic_query_scenes as S

F32 = np.float32
INF = F32(np.inf)


# ---- the restatement ----------------------------------------------------------------------------
def knn(points, spheres, k, period):
    """(indices int32 [m, k], d2 float32 [m, k]): test_neighbours.brute_knn with the wrapped d2."""
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    n = len(X)
    idx = np.full((len(P), k), -1, np.int32)
    dd = np.full((len(P), k), INF, F32)
    finite = np.all(np.isfinite(P), axis=1)
    kk = min(k, n)
    chunk = max(1, min(64, (1 << 22) // max(n, 1)))
    for a in range(0, len(P), chunk):
        d2 = S.d2_rows(P[a:a + chunk], X, period)
        with np.errstate(invalid="ignore"):
            kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
            for r in range(len(d2)):
                if not finite[a + r]:
                    continue
                cand = np.nonzero(d2[r] <= kth[r])[0]       # every candidate that ties the k-th too
                order = np.lexsort((cand, d2[r, cand]))[:kk]
                idx[a + r, :kk] = cand[order]
                dd[a + r, :kk] = d2[r, cand[order]]
    return idx, dd


def lengths(spheres, k, eta, period, rows=None):
    """h = fl(eta sqrt(d2 of slot k - 1)) of the spheres' own centres (rows: a subset)."""
    rows = np.arange(len(spheres)) if rows is None else rows
    _, d2 = knn(spheres[rows], spheres, k, period)
    return (F32(eta) * np.sqrt(d2[:, k - 1])).astype(F32)


def sphere_on(s, period):
    """A sphere is off if its H exceeds half a period on a periodic axis."""
    on = np.ones(len(s), bool)
    with np.errstate(invalid="ignore"):
        for L in period:
            if F32(L) > 0:
                on &= ~(s[:, 3] > S.half(L))
    return on


def pairs(points, s, period, chunk=256):
    """(point index, sphere index, d2) of every containment d2 < fl(H H) with the wrapped d2, spheres that
    are off left out: test_sph_interpolation.pairs on the torus; feeds its restate() unchanged."""
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(s[:, :3], F32)
    H2 = (s[:, 3] * s[:, 3]).astype(F32)
    on = sphere_on(s, period)
    out_p, out_s, out_d2 = [], [], []
    for a in range(0, len(P), chunk):
        d2 = S.d2_rows(P[a:a + chunk], X, period)
        with np.errstate(invalid="ignore"):
            pi, si = np.nonzero((d2 < H2[None, :]) & on[None, :])
        out_p.append(pi + a); out_s.append(si); out_d2.append(d2[pi, si])
    return np.concatenate(out_p), np.concatenate(out_s), np.concatenate(out_d2).astype(F32)


def counts(points, s, period):
    return np.bincount(pairs(points, s, period)[0], minlength=len(points)).astype(np.int32)


# ---- scenes ---------------------------------------------------------------------------------------
def special_H(box):
    """Radii at the contract's edges: half of each period (on where no other period is smaller), its
    successor (off), and 0."""
    out = []
    for L in S.BOXES[box]:
        if L > 0:
            out += [S.half(L), np.nextafter(S.half(L), INF)]
    return np.array(out + [0.0], F32)


def interp_scene(box, offset, seed, n=3000):
    """S.uniform centres with H log-uniform from 1e-3 to 0.5 of the smallest period, the special radii at
    the first spheres."""
    s = S.uniform(n, box, offset, seed)
    lmin = min(L for L in S.BOXES[box] if L > 0)
    rng = np.random.default_rng(seed + 2000)
    s[:, 3] = np.exp(rng.uniform(np.log(1e-3 * lmin), np.log(0.5 * lmin), n)).astype(F32)
    sp = special_H(box)
    s[:len(sp), 3] = sp
    return s


def lattice_H(offset, H=1.5 / 16.0):
    """The full 16^3 lattice with one support radius: on the torus every site lies in equally many spheres."""
    s = S.lattice(offset)
    s[:, 3] = F32(H)
    return s


def one_sphere_grid(centre, m=32, H=0.25):
    """(points [m^3, 3] of the lattice k / m over the period-1 box, sphere [1, 4] at `centre`)."""
    pts = S.lattice(0.0, m)[:, :3].copy()
    return pts, np.array([[centre, centre, centre, H]], F32)


def image_min_d2(p, x, period):
    """The fp64 minimum of |p - (x + n L)|^2 over the 27 explicit images n in {-1, 0, 1}^3: a second method
    for scenes whose fp32 arithmetic is exact."""
    p, x = np.asarray(p, np.float64), np.asarray(x, np.float64)
    best = np.full((len(p), len(x)), np.inf)
    for nx in (-1.0, 0.0, 1.0):
        for ny in (-1.0, 0.0, 1.0):
            for nz in (-1.0, 0.0, 1.0):
                img = x + np.array([nx * period[0], ny * period[1], nz * period[2]])
                d = p[:, None, :] - img[None, :, :]
                best = np.minimum(best, (d * d).sum(axis=2))
    return best
