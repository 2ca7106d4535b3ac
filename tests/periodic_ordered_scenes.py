"""Scenes and the NumPy restatement for the periodic ORDERED traces (include/grace_hip.h, "Periodic boxes
for traces", "Ordered traces"): the open call's composite applied per ray to the hits of all the ray's
segments over the images, ordered by (segment along the ray, fp32 distance within the segment, image
index), every hit standing for its source.

A plain helper module (no GPU, no torch).  The hit list is built from periodic_trace_scenes' segments
and images and the oracle's brute_hits on (segments, images) -- integrals and distances are then bit-equal
with the device's per-hit outputs -- and handed, already in order, to the NumPy composites of
test_emission_absorption.py, test_absorption_deposit.py and test_spectra.py (imported, not copied).
Those sort by (ray, distance, index): they get a hit's rank in the list as its distance, so the order
stays the list's.

  hit_list(oracle, rays, images, source, lo, period)  -> Hits
  emission_absorption / absorption_deposit / spectra  -> the open tests' expected values and bounds
  lattice_hits(rays, spheres, lo, period)             -> fp64, unsegmented rays, every replica in reach
  seam(box) / tiers()                                 -> (spheres, rays[, names])
"""
import functools

import numpy as np

import periodic_trace_scenes as P
import test_absorption_deposit as AD
import test_emission_absorption as EA
import test_spectra as SP
from trace_boundary_scenes import _normalise32, hit_d4

F32, F64 = np.float32, np.float64
SIZES = P.SIZES
TIER_FILL = 58                                   # ordinary rays beside the six threshold rays of tiers()


class Hits:
    """A call's ordered hit list.  Per hit, in order: ray, segment (global), image, source, integral
    (fp32), d (fp32, within the segment), t0 (fp64, the segment's).  off: int64 [n_rays + 1], ray r's hits
    are [off[r], off[r + 1]).  Per segment: segments, seg_off (int32 [n_rays + 1]), seg_t0, cells,
    seg_hits (hits per segment)."""

    def totals(self):
        return np.diff(self.off)

    def open_form(self):
        """(offsets [n_rays], index, integral, rank): what the open tests' restate() take, the rank in
        the list standing in for the distance."""
        return self.off[:-1].astype(np.int32), self.source, self.integral, np.arange(len(self.source), dtype=F64)


def hit_list(oracle, rays, images, source, lo, period):
    """The definition's hit list of `rays` over `images` (in the order given: the image index breaks
    ties) with `source` per image."""
    H = Hits()
    rays = np.ascontiguousarray(rays, F32).reshape(-1, 7)
    H.segments, H.seg_off, H.refused, H.cells, H.seg_t0 = P.segments(rays, lo, period)
    off, idx, integ, dist = oracle.brute_hits(H.segments, np.ascontiguousarray(images, F32))
    H.seg_hits = np.diff(np.append(off, len(idx))).astype(np.int64)
    seg = np.repeat(np.arange(len(H.segments)), H.seg_hits)
    order = np.lexsort((idx, dist, seg))                   # segment ordinal, fp32 distance, image index
    H.segment, H.image = seg[order], idx[order]
    H.integral, H.d = integ[order], dist[order]
    H.source = np.asarray(source, np.int32)[H.image]
    H.t0 = H.seg_t0[H.segment]
    ray_of_segment = np.repeat(np.arange(len(rays)), np.diff(H.seg_off))
    H.ray = ray_of_segment[H.segment]
    H.off = np.concatenate([[0], np.cumsum(np.bincount(H.ray, minlength=len(rays)))]).astype(np.int64)
    return H


def sub_list(H, rays_sel):
    """The hit list of the rays `rays_sel` (indices, in the order wanted) taken out of H."""
    S = Hits()
    rays_sel = np.asarray(rays_sel, np.int64)
    pick = np.concatenate([np.arange(H.off[r], H.off[r + 1]) for r in rays_sel] + [np.zeros(0, np.int64)]).astype(np.int64)
    for name in ("image", "integral", "d", "source", "t0"):
        setattr(S, name, getattr(H, name)[pick])
    counts = H.totals()[rays_sel]
    S.ray = np.repeat(np.arange(len(rays_sel)), counts)
    S.off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return S


def emission_absorption(H, n_rays, emission, absorption):
    """test_emission_absorption.restate on the list: (out, tau, S, n_r)."""
    return EA.restate(n_rays, *H.open_form(), np.asarray(emission, F32).reshape(len(emission), -1),
                      np.asarray(absorption, F32))


def absorption_deposit(H, n_rays, n_sources, luminosity, absorption):
    """test_absorption_deposit.restate on the list: its Ref (deposit per SOURCE; n_rays in the quantum is
    the number of rays)."""
    return AD.restate(n_rays, n_sources, *H.open_form(), np.asarray(luminosity, F32).reshape(n_rays, -1),
                      np.asarray(absorption, F32).reshape(n_sources, -1))


def spectra(H, rays, amount, width, velocity, v0, dv, n_bins, periodic, hubble):
    """test_spectra.restate on the list with d_k = t0 + d in fp64: (tau, tol, column, tol_column)."""
    rays = np.asarray(rays, F32).reshape(-1, 7)
    d = H.t0 + H.d.astype(F64)
    n = len(amount)
    return SP.restate(rays, (H.off[:-1].astype(np.int32), H.source, H.integral, d),
                      np.asarray(amount, F32).reshape(n, -1), np.asarray(width, F32).reshape(n, -1),
                      np.asarray(velocity, F32), v0, dv, n_bins, periodic, hubble)


# ---- fp64 brute force over the infinite lattice ---------------------------------------------------
def lattice_hits(rays, spheres, lo, period):
    """Unsegmented rays against every replica x + m L of every sphere (m over every cell a ray's box,
    widened by the largest H, can touch -- as periodic_trace_scenes.lattice_hitcounts), in fp64.
    Returns (ray, source, m [*, 3] int64, dot, b2, H) of every PAIR whose sphere the ray's line comes within
    1.001 H of and whose dot lies within [-0.001 l, 1.001 l] (hits and near misses: `hit` tells which)
    and hit (bool)."""
    r = np.asarray(rays, F32).reshape(-1, 7); s = np.asarray(spheres, F32).reshape(-1, 4).astype(F64)
    lo64 = np.asarray(lo, F32).astype(F64); L = np.asarray(period, F32).astype(F64)
    o = r[:, 3:6].astype(F64); e = o + r[:, 6:7].astype(F64) * r[:, 0:3].astype(F64)
    hmax = s[:, 3].max()
    rmin, rmax = np.minimum(o, e) - hmax, np.maximum(o, e) + hmax
    ranges = []
    for k in range(3):
        if L[k] > 0:
            ranges.append(range(int(np.floor((rmin[:, k].min() - lo64[k]) / L[k])) - 1,
                                int(np.floor((rmax[:, k].max() - lo64[k]) / L[k])) + 2))
        else:
            ranges.append(range(0, 1))
    out = [[] for _ in range(7)]
    ell = r[:, 6].astype(F64)
    for mx in ranges[0]:
        for my in ranges[1]:
            for mz in ranges[2]:
                m = np.array([mx, my, mz], F64)
                cmin, cmax = lo64 + m * L, lo64 + (m + 1) * L
                near = np.ones(len(r), bool)
                for k in range(3):
                    if L[k] > 0:
                        near &= (rmax[:, k] >= cmin[k]) & (rmin[:, k] <= cmax[k])
                idx = np.nonzero(near)[0]
                if len(idx) == 0:
                    continue
                rep = s.copy(); rep[:, :3] += m * L
                hit, b2, dot = hit_d4(r[idx, None, :], rep[None, :, :])
                h2 = rep[None, :, 3] ** 2
                close = (b2 < 1.002 * h2) & (dot > -0.001 * ell[idx, None] - 1e-6) & (dot < 1.001 * ell[idx, None] + 1e-6)
                a, b = np.nonzero(close)
                out[0].append(idx[a]); out[1].append(b)
                out[2].append(np.broadcast_to(np.array([mx, my, mz], np.int64), (len(a), 3)))
                out[3].append(dot[a, b]); out[4].append(b2[a, b]); out[5].append(rep[b, 3]); out[6].append(hit[a, b])
    cat = [np.concatenate(x) if x else np.zeros(0) for x in out]
    return (cat[0].astype(np.int64), cat[1].astype(np.int64), cat[2].reshape(-1, 3).astype(np.int64), cat[3], cat[4],
            cat[5], cat[6].astype(bool))


def replicas(H, spheres, images, source, period):
    """The lattice replica m [hits, 3] of every hit of H: its segment's cell plus its image's shift."""
    L = np.asarray(period, F32).astype(F64)
    shift = np.zeros((len(images), 3), np.int64)
    for k in range(3):
        if L[k] > 0:
            shift[:, k] = np.rint((images[:, k].astype(F64) - spheres[source, k].astype(F64)) / L[k]).astype(np.int64)
    return np.rint(H.cells[H.segment]).astype(np.int64) + shift[H.image]


# ---- scenes ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam(box, seed=17):
    """(spheres, rays): periodic_trace_scenes' spheres of the box and 257 rays -- rays that start mid-box
    and wrap, rays from a face, axis rays from a face of 2.25 periods (every sphere in reach is hit at least
    twice), oblique rays through the corner region (where spheres have 8 images) and along an edge, and
    short rays inside."""
    lo, period = P.BOXES[box]
    r = P.rays(box)
    rng = np.random.default_rng(seed)
    per = [k for k in range(3) if period[k] > 0]
    long_rays = np.zeros((3 * len(per), 7), F32)
    for m in range(len(long_rays)):
        k = per[m % len(per)]
        long_rays[m, 3:6] = P._inside(rng, 1, lo, period)[0]
        long_rays[m, k] = 1.0
        long_rays[m, 3 + k] = lo[k]
        long_rays[m, 6] = F32(2.25) * period[k]
    # towards a corner of the box (of its periodic axes) and past it at a few hundredths of a period:
    # not through it, where every hit would sit on a tied cut
    Le = np.where(period > 0, period, F32(1.0)).astype(F64)
    loe = np.where(period > 0, lo, F32(-0.5)).astype(F64)
    corner = np.zeros((4, 7), F32)
    for m in range(4):
        sign = 1.0 if m < 2 else -1.0
        frac = np.array([0.8, 0.85, 0.9]) if sign > 0 else np.array([0.2, 0.15, 0.1])
        corner[m, 3:6] = (loe + (frac + 0.01 * m) * Le).astype(F32)
        corner[m, :3] = sign * np.array([1.0, 0.9, 0.8]) * Le * np.where(period > 0, 1.0, 0.1)
        corner[m, 6] = F32(1.2) * P._l_min(period)
    corner[:, :3] = _normalise32(corner[:, :3])
    parts = [long_rays, corner, r["edge"], r["from_face"], r["axis"], r["oblique"][:96]]
    n = sum(len(p) for p in parts)
    parts.append(r["inside"][:257 - n])
    rays = np.concatenate(parts).astype(F32)
    assert len(rays) == 257
    rays.setflags(write=False)
    return P.spheres(box), rays


def _count(oracle, ray, images, lo, period):
    """The restated total of one ray."""
    segs = P.segments(ray[None, :], lo, period)[0]
    return len(oracle.brute_hits(segs, images)[1])


_TIERS = {}


def tiers(oracle, limits=(512, 6144), n=3000, H=0.2, seed=29):
    """(spheres, rays, targets): a dense unit cube ("cube" box) of n spheres of radius H -- one axis
    crossing gives a few hundred hits -- and rays whose TOTALS over all segments are exactly W - 1, W,
    W + 1, B - 1, B, B + 1 (rays 0..5; targets holds the six numbers), then TIER_FILL ordinary rays.  The six share
    origin and direction: nearly along +x, starting just inside the top y and z faces so that the first
    segment (up to the y cut) has no hit and the second (up to the z cut) exactly one; only their
    lengths differ, found by bisection on the restated hit count.  Asserted here, on the CPU."""
    key = (tuple(limits), n, H, seed)
    if key in _TIERS:
        return _TIERS[key]
    lo, period = P.BOXES["cube"]
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = P._inside(rng, n, lo, period)
    s[:, 3] = F32(H)
    images = P.images(s, lo, period)[0]
    d = _normalise32(np.array([[1.0, 0.013, 0.007]], F32))[0]
    base = np.zeros(7, F32)
    base[:3] = d
    first = None
    for a in range(1, 400):                                 # the y cut at t ~ 1e-4, the z cut 1e-4 a later
        t_y, t_z = 1.0e-4, 1.0e-4 * (1 + a)
        base[3:6] = (0.31, 1.0 - t_y * d[1], 1.0 - t_z * d[2])
        base[6] = 1.5
        segs, off = P.segments(base[None, :], lo, period)[:2]
        o, idx, _, _ = oracle.brute_hits(segs, images)
        per_seg = np.diff(np.append(o, len(idx)))
        if len(segs) >= 3 and per_seg[0] == 0 and per_seg[1] == 1:
            first = base.copy()
            break
    assert first is not None, "no start with an empty first and a one-hit second segment: change the seed"
    W, B = limits
    targets = [W - 1, W, W + 1, B - 1, B, B + 1]
    rays = []
    def shortest(want):                                      # the shortest fp32 length with >= want hits
        lo_len, hi_len = F32(0.01), F32(64.0)
        ray = first.copy()
        while True:
            mid = F32(0.5) * (lo_len + hi_len)
            if mid == lo_len or mid == hi_len:
                return hi_len
            ray[6] = mid
            if _count(oracle, ray, images, lo, period) >= want:
                hi_len = mid
            else:
                lo_len = mid

    for want in targets:                                     # midway between where hit `want` and the next come in
        ray = first.copy()
        ray[6] = F32(0.5) * (shortest(want) + shortest(want + 1))
        got = _count(oracle, ray, images, lo, period)
        assert got == want, ("no length gives this total: change the seed", want, got)
        rays.append(ray.copy())
    fill = P.rays("cube")["oblique"][:TIER_FILL].copy()
    fill[:, 6] *= F32(0.2)
    rays = np.concatenate([np.array(rays, F32), fill]).astype(F32)
    s.setflags(write=False); rays.setflags(write=False)
    _TIERS[key] = (s, rays, targets)
    return _TIERS[key]
