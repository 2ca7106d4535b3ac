"""Scenes and the NumPy restatement for the periodic traces (include/grace_hip.h, "Periodic boxes for
traces"): the periodic trace is DEFINED as the open trace of the rays' segments over the spheres'
images, folded back per ray.

A plain helper module (no GPU, no torch): tests/test_periodic_trace.py compares the library with it
bit for bit, tests/test_periodic_trace_scenes.py checks the restatement itself on the CPU -- against an
fp64 brute force over the infinite lattice of unsegmented rays -- and the scenes.

  images(spheres, lo, period)    -> (images, source, offsets, refused)       fp32, as defined
  segments(rays, lo, period)     -> (segments, offsets, refused, cells, t0)  fp64 from widened fp32
  fold(values, offsets)          -> the fp32 running sum from 0 per row, in order
  hits(segments, images)         -> hit_f32 on segments x images (trace_boundary_scenes.py)
  lattice_hitcounts(...)         -> fp64, unsegmented rays, every replica a ray can reach
"""
import functools

import numpy as np

from trace_boundary_scenes import _morton_tile_order, _normalise32, hit_d4, hit_f32

F32, F64 = np.float32, np.float64
MAX_SEGMENTS = 65536
SIZES = (1, 63, 64, 65, 255, 256, 257)           # both sides of the new kernels' 64-lane waves and 256-thread blocks

# name: (lo, period); a period of 0 leaves the axis open
BOXES = {
    "cube": (np.array([0.0, 0.0, 0.0], F32), np.array([1.0, 1.0, 1.0], F32)),
    "slab": (np.array([0.25, -0.5, 3.0], F32), np.array([1.0, 1.5, 0.75], F32)),
    "mixed": (np.array([-0.5, 0.0, 1.0], F32), np.array([1.0, 0.0, 2.0], F32)),
}
OPEN_EXTENT = (-1.0, 1.0)                        # where centres and origins lie on an open axis


# ---- restatement: images --------------------------------------------------------------------------
def images(spheres, lo, period):
    """(images float32 [m, 4], source int32 [m], offsets int32 [n + 1], refused bool [n])."""
    s = np.asarray(spheres, F32).reshape(-1, 4)
    lo = np.asarray(lo, F32); L = np.asarray(period, F32)
    n = len(s)
    finite = np.all(np.isfinite(s), axis=1)
    code = np.zeros(n, np.int64)
    refused = np.zeros(n, bool)
    moved = s[:, :3].copy()
    with np.errstate(all="ignore"):
        for k in range(3):
            if not L[k] > 0:
                continue
            top = F32(lo[k] + L[k])
            x, h = s[:, k], s[:, 3]
            refused |= finite & ((x < lo[k]) | (x > top) | (h > F32(0.5) * L[k]))
            low = (x - h).astype(F32) < lo[k]
            high = ~low & ((x + h).astype(F32) > top)
            code |= (low | high).astype(np.int64) << k
            moved[:, k] = np.where(low, (x + L[k]).astype(F32), np.where(high, (x - L[k]).astype(F32), x))
    code[refused | ~finite] = 0
    out, src = [], []
    for i in range(n):
        for subset in range(8):
            if subset & ~code[i]:
                continue
            row = s[i].copy()
            for k in range(3):
                if subset >> k & 1:
                    row[k] = moved[i, k]
            out.append(row); src.append(i)
    counts = np.array([1 << bin(int(c)).count("1") for c in code], np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return (np.array(out, F32).reshape(-1, 4), np.array(src, np.int32), offsets, refused)


# ---- restatement: segments ------------------------------------------------------------------------
def _cut_t(lo, L, o, d, c, n):
    """t of cuts n (1-based, array) of one axis: planes c + n for d > 0, c - (n - 1) for d < 0."""
    m = c + n.astype(F64) if d > 0 else c - (n.astype(F64) - 1.0)
    with np.errstate(all="ignore"):
        return ((lo + m * L) - o) / d


def _axis_cuts(lo, L, o, d, length, c):
    """The kept cuts' t, ascending: stepped through, in blocks, up to MAX_SEGMENTS + 1 of them."""
    if not L > 0 or d == 0:
        return np.zeros(0, F64)
    kept, start, block = [], 1, 64
    while start <= MAX_SEGMENTS + 1:
        n = np.arange(start, min(start + block, MAX_SEGMENTS + 2))
        t = _cut_t(lo, L, o, d, c, n)
        ok = (t > 0) & (t < length)
        stop = len(ok) if ok.all() else int(np.argmin(ok))
        kept.append(t[:stop])
        if stop < len(ok):
            break
        start += len(n); block *= 8
    return np.concatenate(kept)


def segments(rays, lo, period):
    """(segments float32 [m, 7], offsets int32 [n + 1], refused bool [n], cells float64 [m, 3],
    t0 float64 [m]): cells and t0 are each segment's cell and starting t (0 for a ray emitted as itself)."""
    r = np.asarray(rays, F32).reshape(-1, 7)
    lo64 = np.asarray(lo, F32).astype(F64); L64 = np.asarray(period, F32).astype(F64)
    segs, cells, t0s, counts = [], [], [], []
    refused = np.zeros(len(r), bool)
    for i, ray in enumerate(r):
        if not np.all(np.isfinite(ray)):
            segs.append(ray.copy()); cells.append(np.zeros(3)); t0s.append(0.0); counts.append(1)
            continue
        d = ray[0:3].astype(F64); o = ray[3:6].astype(F64); length = F64(ray[6])
        c = np.zeros(3, F64)
        cuts = []
        for k in range(3):
            if L64[k] > 0:
                u = (o[k] - lo64[k]) / L64[k]
                c[k] = np.floor(u) if d[k] >= 0 else np.ceil(u) - 1.0
        for k in range(3):
            cuts += [(t, k) for t in _axis_cuts(lo64[k], L64[k], o[k], d[k], length, c[k])]
        if 1 + len(cuts) > MAX_SEGMENTS:
            refused[i] = True
            segs.append(ray.copy()); cells.append(np.zeros(3)); t0s.append(0.0); counts.append(1)
            continue
        if not cuts and not np.any(c != 0):
            segs.append(ray.copy()); cells.append(c.copy()); t0s.append(0.0); counts.append(1)
            continue
        cuts.sort()
        ts = [F64(0.0)] + [t for t, _ in cuts] + [length]
        cell = c.copy()
        for j in range(len(cuts) + 1):
            seg = ray.copy()
            seg[3:6] = ((o + ts[j] * d) - cell * L64).astype(F32)
            seg[6] = F32(ts[j + 1] - ts[j])
            segs.append(seg); cells.append(cell.copy()); t0s.append(float(ts[j]))
            if j < len(cuts):
                k = cuts[j][1]
                cell[k] += 1.0 if d[k] > 0 else -1.0
        counts.append(len(cuts) + 1)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return (np.array(segs, F32).reshape(-1, 7), offsets, refused, np.array(cells, F64).reshape(-1, 3),
            np.array(t0s, F64))


# ---- restatement: results -------------------------------------------------------------------------
def fold(values, offsets):
    """The running sum from 0, in row order, of values [m] or [m, C] in their own dtype (fp32 / int32)."""
    v = np.asarray(values)
    v2 = v.reshape(len(v), -1)
    out = np.zeros((len(offsets) - 1, v2.shape[1]), v.dtype)
    longest = int(np.max(np.diff(offsets))) if len(offsets) > 1 else 0
    for j in range(longest):                                     # step j of every row that has one
        rows = np.nonzero(np.diff(offsets) > j)[0]
        out[rows] = out[rows] + v2[offsets[rows] + j]
    return out.reshape((len(offsets) - 1,) + v.shape[1:])


def hits(segs, imgs, chunk=512):
    """hit_f32 on segments x images: (segment index, image index, b2 float32) of every hit."""
    si, ii, b2s = [], [], []
    for a in range(0, len(segs), chunk):
        hit, b2, _ = hit_f32(segs[a:a + chunk, None, :], imgs[None, :, :])
        s, i = np.nonzero(hit)
        si.append(s + a); ii.append(i); b2s.append(b2[s, i])
    return np.concatenate(si), np.concatenate(ii), np.concatenate(b2s).astype(F32)


def hitcounts(rays, spheres, lo, period):
    """Per-ray periodic hit counts as defined: hit_f32 summed over restated segments x images."""
    segs, offsets = segments(rays, lo, period)[:2]
    imgs = images(spheres, lo, period)[0]
    s, _, _ = hits(segs, imgs)
    per_seg = np.bincount(s, minlength=len(segs)).astype(np.int32)
    return fold(per_seg, offsets)


def lattice_hitcounts(rays, spheres, lo, period):
    """fp64 brute force over the infinite lattice: unsegmented rays against every replica x + m L of
    every sphere, m over every cell a ray's box, widened by the largest H, can touch."""
    r = np.asarray(rays, F32).reshape(-1, 7); s = np.asarray(spheres, F32).reshape(-1, 4).astype(F64)
    lo64 = np.asarray(lo, F32).astype(F64); L = np.asarray(period, F32).astype(F64)
    o = r[:, 3:6].astype(F64); e = o + r[:, 6:7].astype(F64) * r[:, 0:3].astype(F64)
    hmax = s[:, 3].max()
    rmin, rmax = np.minimum(o, e) - hmax, np.maximum(o, e) + hmax
    ranges = []
    for k in range(3):
        if L[k] > 0:   # a replica m holds centres in [lo + m L, lo + (m + 1) L]
            ranges.append(range(int(np.floor((rmin[:, k].min() - lo64[k]) / L[k])) - 1,
                                int(np.floor((rmax[:, k].max() - lo64[k]) / L[k])) + 2))
        else:
            ranges.append(range(0, 1))
    counts = np.zeros(len(r), np.int64)
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
                hit = hit_d4(r[idx, None, :], rep[None, :, :])[0]
                counts[idx] += hit.sum(axis=1)
    return counts


# ---- scenes ---------------------------------------------------------------------------------------
def _l_min(period):
    return F32(min(float(p) for p in period if p > 0))


def _inside(rng, n, lo, period):
    """n points in the box, fp32, never outside [lo, fl(lo + L)] on a periodic axis."""
    p = np.empty((n, 3), F32)
    for k in range(3):
        if period[k] > 0:
            top = F32(lo[k] + period[k])
            p[:, k] = np.clip((lo[k] + rng.random(n) * period[k]).astype(F32), lo[k], top)
        else:
            p[:, k] = (OPEN_EXTENT[0] + rng.random(n) * (OPEN_EXTENT[1] - OPEN_EXTENT[0])).astype(F32)
    return p


@functools.lru_cache(maxsize=None)
def spheres(box, n=600, seed=11):
    """n spheres in the box: H mostly small, 24 of them up to exactly L_min / 2 (4 exactly that), and
    centres on a face, an edge and a corner (8 copies of each kind), on the low and the high side."""
    lo, period = BOXES[box]
    rng = np.random.default_rng(seed)
    lmin = _l_min(period)
    s = np.empty((n, 4), F32)
    s[:, :3] = _inside(rng, n, lo, period)
    s[:, 3] = (lmin * (0.01 + 0.14 * rng.random(n))).astype(F32)
    s[:24, 3] = (lmin * (0.25 + 0.25 * rng.random(24))).astype(F32)
    s[:4, 3] = F32(0.5) * lmin
    per = [k for k in range(3) if period[k] > 0]
    top = (lo + period).astype(F32)
    for j in range(24):                                          # 8 on faces, 8 on edges, 8 on corners
        n_axes = min(1 + j // 8, len(per))
        for a in range(n_axes):
            k = per[(j + a) % len(per)]
            s[24 + j, k] = lo[k] if (j >> a) & 1 else top[k]
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def rays(box, seed=5):
    """The rays of a box, by kind (a dict of float32 [m, 7]) -- see the module's tests for what each is for."""
    lo, period = BOXES[box]
    rng = np.random.default_rng(seed)
    lmin = _l_min(period)
    top = (lo + period).astype(F32)
    span = [(lo[k], period[k]) if period[k] > 0 else (F32(OPEN_EXTENT[0]), F32(OPEN_EXTENT[1] - OPEN_EXTENT[0]))
            for k in range(3)]
    out = {}
    # an 8 x 8-tiled 64 x 64 grid along +z from the face z = lo_z, spanning exactly one period
    i, j = _morton_tile_order(64)
    g = np.zeros((64 * 64, 7), F32)
    g[:, 2] = 1.0
    g[:, 3] = (span[0][0] + (i + 0.5) / 64 * span[0][1]).astype(F32)
    g[:, 4] = (span[1][0] + (j + 0.5) / 64 * span[1][1]).astype(F32)
    g[:, 5] = lo[2]
    g[:, 6] = period[2]
    out["grid"] = g

    def batch(n, max_len):
        b = np.empty((n, 7), F32)
        b[:, :3] = _normalise32(rng.normal(size=(n, 3)))
        b[:, 3:6] = _inside(rng, n, lo, period)
        b[:, 6] = (max_len * rng.random(n)).astype(F32)
        return b
    out["inside"] = batch(192, 0.3 * lmin)
    out["oblique"] = batch(192, 3.7 * lmin)
    k0 = [k for k in range(3) if period[k] > 0][0]               # a periodic axis
    plane = batch(16, 2.0 * lmin)                                 # in a face plane: d_k0 = +-0, o_k0 on the face
    plane[:, k0] = 0.0
    plane[:, :3] = _normalise32(plane[:, :3])
    plane[:, k0] = np.where(np.arange(16) % 2 == 0, F32(0.0), F32(-0.0))
    plane[:, 3 + k0] = np.where(np.arange(16) % 4 < 2, lo[k0], top[k0])
    out["plane"] = plane
    neg = batch(16, 2.5 * lmin)                                   # from a face, going out of the box
    neg[:, k0] = -np.abs(neg[:, k0]); neg[:8, :3] = 0.0; neg[:8, k0] = -1.0
    neg[:, 3 + k0] = lo[k0]
    out["from_face"] = neg
    axis = batch(24, 2.2 * lmin)                                  # axis-aligned, the other components +0 / -0
    for m in range(24):
        k = m % 3
        axis[m, :3] = F32(-0.0) if (m // 6) % 2 else F32(0.0)
        axis[m, k] = 1.0 if (m // 3) % 2 == 0 else -1.0
    out["axis"] = axis
    zero = batch(8, 1.0); zero[:, 6] = 0.0
    out["zero_length"] = zero
    corner = np.zeros((4, 7), F32)                                # through a corner of the box: tied cuts
    diag = np.where(period > 0, period, F32(0.0)).astype(F64)
    corner[:, :3] = _normalise32(np.array([diag, diag, -diag, -diag], F32))
    corner[:, 3:6] = (lo + F32(0.5) * period).astype(F32)
    corner[2:, 3:6] = (lo + F32(0.25) * period).astype(F32)
    corner[:, 6] = F32(2.0) * np.sqrt(np.sum(diag * diag)).astype(F32)
    out["corner"] = corner
    # through an edge of the box, away from its corners: two tied (or one rounding step apart) cuts.
    # Unlike a ray through a corner -- which runs through the centre of every replica of a corner sphere,
    # whose closest approach then falls ON a cut, where fp32 rounding decides -- these can be compared
    # with the lattice brute force.
    k1 = [k for k in range(3) if period[k] > 0][1]
    k2 = 3 - k0 - k1
    edge = np.zeros((8, 7), F32)
    for m in range(8):
        v = np.zeros(3, F64)
        v[k0] = period[k0] * (1 if m & 1 else -1); v[k1] = period[k1] * (1 if m & 2 else -1)
        v[k2] = 0.37 * lmin * (1 if m & 4 else -1)
        edge[m, :3] = v
        edge[m, 3:6] = (lo + F32(0.5) * period).astype(F32)
    edge[:, :3] = _normalise32(edge[:, :3])
    edge[:, 6] = F32(2.5) * lmin
    out["edge"] = edge
    for v in out.values():
        v.setflags(write=False)
    return out


def all_rays(box):
    return np.concatenate(list(rays(box).values()))


def refusals(box):
    """(spheres, rays) that the definition refuses: a centre outside the box, H just above L / 2 and a
    ray of 70 000 periods, each beside ordinary entries."""
    lo, period = BOXES[box]
    k0 = [k for k in range(3) if period[k] > 0][0]
    s = spheres(box)[:8].copy()
    s[2, k0] = np.nextafter(lo[k0], F32(-np.inf))
    s[5, 3] = np.nextafter(F32(0.5) * period[k0], F32(np.inf))
    r = rays(box)["oblique"][:8].copy()
    r[3, :3] = 0.0; r[3, k0] = 1.0
    r[3, 6] = F32(70000.0) * period[k0]
    return s, r


def dyadic(box, n=400, seed=3, n_rays=256):
    """Coordinates, H and ray origins on the 2^-10 grid, axis-aligned rays: shifting the centres (wrapped)
    and the origins by a multiple of 2^-10 is exact, so no hit count may change."""
    lo, period = BOXES[box]
    rng = np.random.default_rng(seed)
    q = 1024.0
    s = np.empty((n, 4), F32)
    for k in range(3):
        ext = period[k] if period[k] > 0 else F32(2.0)
        base = lo[k] if period[k] > 0 else F32(-1.0)
        s[:, k] = base + rng.integers(0, int(ext * q), n) / q
    s[:, 3] = rng.integers(8, int(_l_min(period) * q / 2) + 1, n) / q
    r = np.zeros((n_rays, 7), F32)
    for m in range(n_rays):
        k = m % 3
        r[m, k] = 1.0 if (m // 3) % 2 == 0 else -1.0
        for a in range(3):
            ext = period[a] if period[a] > 0 else F32(2.0)
            base = lo[a] if period[a] > 0 else F32(-1.0)
            r[m, 3 + a] = base + (rng.integers(0, int(ext * q)) + 0.5) / q     # (half a step off every centre)
        r[m, 6] = rng.integers(1, int(3 * q)) / q
    return s, r


def dyadic_shift(s, r, lo, period, shift):
    """The scene shifted by `shift` (multiples of 2^-10): centres wrapped into [lo, lo + L), origins not."""
    s2, r2 = s.copy(), r.copy()
    for k in range(3):
        if period[k] > 0:
            x = s[:, k].astype(F64) + shift[k]
            x = lo[k] + np.mod(x - lo[k], F64(period[k]))
            s2[:, k] = x.astype(F32)
            r2[:, 3 + k] = (r[:, 3 + k].astype(F64) + shift[k]).astype(F32)
    return s2, r2
