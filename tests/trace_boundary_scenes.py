"""Boundary scenes for the trace tests: spheres that sit one rounding step inside or outside the
hit test of one ray, placed against a packet's extreme ray so that a cull which is one ulp too
tight drops a real hit.

A plain helper module (no GPU, no torch): tests/test_trace_boundaries.py traces its scenes,
tests/test_trace_boundary_scenes.py checks on the CPU that every twin sits exactly where it is
said to sit according to the oracle.

Restatements of sphere_hit (generic/intersect.h, grace_oracle.c sphere_hit*): vectorised, every
operation rounded in its own precision, no FMA --
  * hit_f32: <float4, float>;
  * hit_f4d: <float4, double> (differences in float, widened; w * w in float);
  * hit_d4:  <double4, double> (ray members float, widened).

Twins.  A RADIUS twin pair shares a centre: the hit twin's w is the smallest radius whose square
(in the test's precision) exceeds the pair's b2, the miss twin's the radius just below it.  A RANGE
twin pair shares a radius: the centres are adjacent floats (doubles) of one co-ordinate on either
side of dot_p = 0 or dot_p = length.

Packets.  Sharpness (only the twin's own ray can hit it) rests on which rays share a packet:
with set_ray_reorder(False) a packet is a run of consecutive caller rays (16, 32 or 64); the ray
grids here are therefore laid out in 8 x 8 tiles, Morton order inside a tile, so that every
aligned run of 16, 32 or 64 rays is a rectangle of the grid.  With reordering on, a power-of-two
pixel grid of axis-aligned rays is cut into the same aligned 8 x 8 tiles.  No correctness
assertion depends on this; only how sharp a scene is does.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
TILE = 8


# ---- restatements ------------------------------------------------------------------------------
def hit_f32(rays, s):
    """sphere_hit<float4, float> on broadcast (ray, sphere) pairs: (hit, b2, dot), float32."""
    rays = np.asarray(rays, F32); s = np.asarray(s, F32)
    px = s[..., 0] - rays[..., 3]
    py = s[..., 1] - rays[..., 4]
    pz = s[..., 2] - rays[..., 5]
    rx, ry, rz = rays[..., 0], rays[..., 1], rays[..., 2]
    dot = px * rx + py * ry + pz * rz
    bx = px - dot * rx
    by = py - dot * ry
    bz = pz - dot * rz
    b2 = bx * bx + by * by + bz * bz
    hit = ~(b2 >= s[..., 3] * s[..., 3]) & ~(dot < F32(0)) & ~(dot >= rays[..., 6])
    return hit, b2, dot


def hit_f4d(rays, s):
    """sphere_hit<float4, double>: differences in float, then double; w * w in float."""
    rays = np.asarray(rays, F32); s = np.asarray(s, F32)
    p = [(s[..., k] - rays[..., 3 + k]).astype(F64) for k in range(3)]
    r = [rays[..., k].astype(F64) for k in range(3)]
    dot = p[0] * r[0] + p[1] * r[1] + p[2] * r[2]
    b = [p[k] - dot * r[k] for k in range(3)]
    b2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2]
    w2 = (s[..., 3] * s[..., 3]).astype(F64)
    hit = ~(b2 >= w2) & ~(dot < 0.0) & ~(dot >= rays[..., 6].astype(F64))
    return hit, b2, dot


def hit_d4(rays, s):
    """sphere_hit<double4, double>: ray members are float, widened; everything else double."""
    rays = np.asarray(rays, F32); s = np.asarray(s, F64)
    p = [s[..., k] - rays[..., 3 + k].astype(F64) for k in range(3)]
    r = [rays[..., k].astype(F64) for k in range(3)]
    dot = p[0] * r[0] + p[1] * r[1] + p[2] * r[2]
    b = [p[k] - dot * r[k] for k in range(3)]
    b2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2]
    hit = ~(b2 >= s[..., 3] * s[..., 3]) & ~(dot < 0.0) & ~(dot >= rays[..., 6].astype(F64))
    return hit, b2, dot


RESTATE = {"f32": hit_f32, "f4d": hit_f4d, "d4": hit_d4}


# ---- twins -------------------------------------------------------------------------------------
def _sq(w, prec):
    """The radius test's right-hand side: fl32(w w) (widened for f4d) or fl64(w w)."""
    if prec == "d4":
        return w * w
    return (w * w).astype(F32).astype(F64) if prec == "f4d" else w * w


def radius_twins(b2, prec):
    """Per pair: (w_hit, w_miss, exact).  w_hit is the smallest radius of the precision's radius
    type with sq(w_hit) > b2, w_miss the next radius below it (sq(w_miss) <= b2); exact: sq(w_hit)
    is the smallest value of the comparison's type above b2 (fl32 for f32, f4d's product; fl64
    for d4)."""
    wt = F64 if prec == "d4" else F32
    b2 = np.asarray(b2, F32 if prec == "f32" else F64)
    w = np.sqrt(b2.astype(F64)).astype(wt)
    for _ in range(3):
        w = np.nextafter(w, wt(0))
    for _ in range(8):
        low = ~(_sq(w, prec) > b2)
        w = np.where(low, np.nextafter(w, wt(np.inf)), w)
    assert np.all(_sq(w, prec) > b2)
    w_miss = np.nextafter(w, wt(0))
    assert np.all(~(_sq(w_miss, prec) > b2))
    if prec == "f32":
        nxt = np.nextafter(b2, F32(np.inf))
    elif prec == "f4d":
        nxt = np.nextafter(b2.astype(F32), F32(np.inf)).astype(F64)   # next float above the double b2
        nxt = np.where(nxt.astype(F64) > b2, nxt, np.nextafter(nxt.astype(F32), F32(np.inf)).astype(F64))
    else:
        nxt = np.nextafter(b2, np.inf)
    exact = _sq(w, prec) == nxt
    return w, w_miss, exact


def _morton_tile_order(side):
    """Grid cells (i, j), i = column, j = row, in 8 x 8 tiles (row-major over tiles), Morton order
    inside a tile: every aligned run of 16, 32 or 64 entries is a rectangle."""
    assert side % TILE == 0
    k = np.arange(TILE * TILE)
    li = sum(((k >> (2 * b)) & 1) << b for b in range(3))
    lj = sum(((k >> (2 * b + 1)) & 1) << b for b in range(3))
    t = side // TILE
    ti, tj = np.meshgrid(np.arange(t), np.arange(t))
    i = (ti.ravel()[:, None] * TILE + li[None, :]).ravel()
    j = (tj.ravel()[:, None] * TILE + lj[None, :]).ravel()
    return i, j


def _normalise32(v):
    v = np.asarray(v, F32)
    n = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F32)
    return (v / n[:, None]).astype(F32)


# Scales: (low corner, edge length of the box holding the scene, smoothing lengths relative to it)
SCALES = {
    "unit": (np.array([0.0, 0.0, 0.0]), 1.0, (0.004, 0.02)),
    "1e3": (np.array([1000.0, 1000.5, 999.25]), 1.0, (0.004, 0.02)),
    # |s| / h from 1e4 (h = 10) to 1e6 (h = 0.1)
    "1e5": (np.array([1.0e5, 1.0e5 - 64.0, 1.0e5 + 32.0]), 64.0, (0.1 / 64, 10.0 / 64)),
    "1e-3": (np.array([0.0, 0.0, 0.0]), 1.0e-3, (0.004, 0.02)),
}


class Scene:
    """rays [R, 7] float32 (caller order); spheres [n, 4] float32 or float64 (caller order, before
    the build sorts them); hit / miss: caller indices of the hit twins and the miss twins; target:
    the ray each twin of `hit` / `miss` was placed against; sub: rays worth a brute-force check
    (every target plus a sample of the rest); box: (low, high) of the background's centres."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def axis_rays(side, axis, sense, lo, size, rng, neg_zero=False, ragged=False, width=64):
    """side x side rays along sense * e_axis over the face of the box [lo, lo + size]^3, in tiles;
    ragged: per-ray starts and lengths (the lean test's len_lo / noda bounds then differ per ray);
    ragged="one": every ray crosses the whole box, except that in each packet (run of `width`
    rays) one ray ends inside the box and one other starts inside it, both at depths drawn per
    packet in the middle half of the box -- the packet's len_lo and its latest start then lie
    inside dense background, and only the rounds around them need a range test."""
    i, j = _morton_tile_order(side)
    perp = [k for k in range(3) if k != axis]
    sp = size / side
    r = np.zeros((side * side, 7), F32)
    if neg_zero:
        r[:, perp[0]] = -0.0; r[:, perp[1]] = -0.0
    r[:, axis] = sense
    r[:, 3 + perp[0]] = (lo[perp[0]] + (i + 0.5) * sp).astype(F32)
    r[:, 3 + perp[1]] = (lo[perp[1]] + (j + 0.5) * sp).astype(F32)
    if isinstance(ragged, str):
        assert ragged == "one"
        start = np.full(len(r), -0.1 * size)
        r[:, 6] = F32(1.2 * size)
        for pk in _packets(len(r), width):
            short, late = pk[rng.choice(len(pk), 2, replace=False)]
            r[short, 6] = F32((0.1 + rng.uniform(0.25, 0.75)) * size)     # ends at that depth
            start[late] = rng.uniform(0.25, 0.75) * size                  # starts at this one
    elif ragged:
        start = rng.uniform(-0.1, 0.4, len(r)) * size
        r[:, 6] = (rng.uniform(0.3, 1.2, len(r)) * size).astype(F32)
    else:
        start = np.full(len(r), -0.1 * size)
        r[:, 6] = F32(1.2 * size)
    r[:, 3 + axis] = (lo[axis] + start if sense > 0 else lo[axis] + size - start).astype(F32)
    return r, sp


def pencil_rays(kind, side, lo, size, rng, nside=16):
    """One-origin rays: "pinhole" (a camera grid), "iso" (the six faces of a cube of directions),
    "healpix" (HEALPix nested directions: consecutive pixels are compact).  Directions normalised
    here in float32."""
    centre = lo + 0.5 * size
    if kind == "pinhole":
        i, j = _morton_tile_order(side)
        o = centre + np.array([0.1, -0.2, -1.6]) * size
        u = (i + 0.5) / side - 0.5; v = (j + 0.5) / side - 0.5
        v3 = np.stack([0.7 * u - 0.06, 0.7 * v + 0.12, np.ones_like(u)], axis=1)
    elif kind == "iso":
        s2 = side // 2
        i, j = _morton_tile_order(s2)
        u = 2 * (i + 0.5) / s2 - 1; v = 2 * (j + 0.5) / s2 - 1
        faces = []
        for ax in range(3):
            for sg in (1, -1):
                f = np.zeros((len(u), 3)); f[:, ax] = sg
                f[:, (ax + 1) % 3] = u; f[:, (ax + 2) % 3] = v
                faces.append(f)
        v3 = np.concatenate(faces)[: side * side]
        o = centre + np.array([0.013, -0.021, 0.007]) * size
    else:
        import oracle as O
        v3 = O.healpix_dirs(nside)
        o = centre + np.array([-0.011, 0.017, 0.023]) * size
    d = _normalise32(v3)
    r = np.zeros((len(d), 7), F32)
    r[:, :3] = d
    r[:, 3:6] = o.astype(F32)
    r[:, 6] = F32(3.0 * size)
    return r


def general_rays(n_packets, lo, size, rng, width=64):
    """Packets of `width` consecutive rays with distinct origins and directions: origins in a small
    box, directions within a narrow cone (every origin differs: neither axis-aligned nor a pencil);
    half of the packets share one direction (oblique parallel rays)."""
    r = np.zeros((n_packets * width, 7), F32)
    for p in range(n_packets):
        sl = slice(p * width, (p + 1) * width)
        c = lo + rng.uniform(-0.3, 0.3, 3) * size
        o = c + rng.uniform(-0.02, 0.02, (width, 3)) * size
        a = rng.normal(size=3); a = np.abs(a) / np.linalg.norm(a)
        a = np.where(rng.random(3) < 0.2, -a, a) if p % 3 else np.abs(a)
        if p % 2:
            dirs = np.repeat(a[None], width, axis=0)
        else:
            dirs = a[None] + rng.uniform(-0.03, 0.03, (width, 3))
        r[sl, :3] = _normalise32(dirs)
        r[sl, 3:6] = o.astype(F32)
        r[sl, 6] = F32(2.5 * size)
    return r


def _perp_unit(d, u):
    """u made perpendicular to d and normalised (float64)."""
    u = u - (u * d).sum(-1, keepdims=True) * d
    return u / np.linalg.norm(u, axis=-1, keepdims=True)


def _packets(n_rays, width):
    return [np.arange(p, min(p + width, n_rays)) for p in range(0, n_rays, width)]


def extreme_placements(rays, kind, width, rng, spacing):
    """(ray index, outward unit vector perpendicular to the ray, offset scale) per extreme ray of
    every packet of `width` consecutive rays."""
    out = []
    d_all = rays[:, :3].astype(F64)
    o_all = rays[:, 3:6].astype(F64)
    for pk in _packets(len(rays), width):
        d, o = d_all[pk], o_all[pk]
        if kind == "axis":
            ax = int(np.argmax(np.abs(d[0])))
            perp = [k for k in range(3) if k != ax]
            a, b = o[:, perp[0]], o[:, perp[1]]
            for sa in (-1, 1):
                for sb in (-1, 1):
                    # corner: outward diagonal; edges: outward along one co-ordinate
                    ia = a == (a.max() if sa > 0 else a.min()); ib = b == (b.max() if sb > 0 else b.min())
                    corner = np.nonzero(ia & ib)[0]
                    if len(corner):
                        u = np.zeros(3); u[perp[0]] = sa; u[perp[1]] = sb
                        out.append((pk[corner[0]], u / math.sqrt(2), spacing))
                edge_a = np.nonzero(ia)[0]
                if len(edge_a):
                    k = edge_a[rng.integers(len(edge_a))]
                    u = np.zeros(3); u[perp[0]] = sa
                    out.append((pk[k], u, spacing))
            for sb in (-1, 1):
                ib = b == (b.max() if sb > 0 else b.min())
                e = np.nonzero(ib)[0]
                k = e[rng.integers(len(e))]
                u = np.zeros(3); u[perp[1]] = sb
                out.append((pk[k], u, spacing))
        elif kind == "pencil":
            a = d.mean(axis=0); a /= np.linalg.norm(a)
            cosang = d @ a
            for k in np.argsort(cosang)[:3]:          # the three rays furthest from the axis
                u = _perp_unit(d[k], d[k] - a)
                # angular spacing: to the nearest other ray of the packet
                others = np.delete(np.arange(len(pk)), k)
                ang = np.arccos(np.clip(d[others] @ d[k], -1, 1)).min() if len(others) else 1e-3
                out.append((pk[k], u, ang))
        else:
            for ax in range(3):
                for sg in (-1, 1):
                    k = int(np.argmax(sg * o[:, ax]))
                    u0 = np.zeros(3); u0[ax] = sg
                    if abs(d[k] @ u0) > 0.95:
                        continue
                    u = _perp_unit(d[k], u0)
                    others = np.delete(np.arange(len(pk)), k)
                    dist = np.linalg.norm(np.cross(o[others] - o[k], d[k]), axis=1)
                    out.append((pk[k], u, max(dist.min(), 1e-12)))
    return out


def _place_radius_twins(rays, places, prec, rng, t_range, pencil, max_tries=6):
    """Centres c = o + t d + delta u; radius twins for the exact restatement of `prec`.
    Returns (centres [m, 3], w_hit [m], w_miss [m], ray index [m])."""
    cs, wh, wm, ri = [], [], [], []
    ct = F64 if prec == "d4" else F32
    fn = RESTATE[prec]
    for (r, u, scale) in places:
        d = rays[r, :3].astype(F64); o = rays[r, 3:6].astype(F64); L = float(rays[r, 6])
        for _ in range(max_tries):
            t = rng.uniform(*t_range) * L
            # pencils: an angular offset (|c - o| / h large); others: a fraction of the spacing
            delta = (rng.uniform(0.1, 0.4) * scale * t) if pencil else rng.uniform(0.1, 0.45) * scale
            c = (o + t * d + delta * u).astype(ct)
            s = np.array([c[0], c[1], c[2], 0.0], ct)
            _, b2, dot = fn(rays[r], s)
            if not (0 < dot < L) or not b2 > 0:
                continue
            w_hit, w_miss, exact = radius_twins(np.array([b2]), prec)
            if exact[0] or _ == max_tries - 1:
                cs.append(c); wh.append(w_hit[0]); wm.append(w_miss[0]); ri.append(r)
                break
    return (np.array(cs, ct).reshape(-1, 3), np.array(wh, ct), np.array(wm, ct), np.array(ri, np.int64))


def range_twins(ray, t0, w, prec):
    """Centres on `ray` at either side of dot_p = t0 (0 or the ray's length), adjacent in the
    co-ordinate the ray advances fastest in: (c_in, c_out) -- c_in's dot_p is t0 (if t0 = 0) or just
    below it, c_out's just past it -- or None.  Both with radius w (b2 << w^2)."""
    ct = F64 if prec == "d4" else F32
    fn = RESTATE[prec]
    d = ray[:3].astype(F64); o = ray[3:6].astype(F64)
    k = int(np.argmax(np.abs(d)))
    c = (o + (t0 / (d @ d)) * d).astype(ct)       # (float directions are unit to a few ulp only)
    inside = lambda dot: (dot >= 0) if t0 == 0 else (dot < ray[6])
    # step towards the outside (decreasing dot_p for t0 = 0, increasing for the length)
    out_dir = -np.sign(d[k]) if t0 == 0 else np.sign(d[k])
    toward_out = ct(np.inf * out_dir)
    toward_in = ct(-np.inf * out_dir)

    def dot_of(cc):
        s = np.array([cc[0], cc[1], cc[2], w], ct)
        return fn(ray, s)[2]
    for _ in range(400):
        if inside(dot_of(c)):
            break
        c = c.copy(); c[k] = np.nextafter(c[k], toward_in)
    else:
        return None
    for _ in range(400):
        nxt = c.copy(); nxt[k] = np.nextafter(c[k], toward_out)
        if not inside(dot_of(nxt)):
            return c, nxt
        c = nxt
    return None


def boundary_scene(kind, scale, prec="f32", seed=0, side=64, axis=2, sense=1, width=64,
                   n_background=60000, neg_zero=False, ragged=False, rim=True, max_twins=600, drop_last=0):
    """A scene of `n_background` random spheres in the scale's box plus radius and range twins
    against the extreme rays of every packet (kind: "axis", "pinhole", "iso", "healpix",
    "general").  prec: the hit test the twins are exact for ("f32", "f4d", "d4").  drop_last: that
    many rays (a multiple of 32, as ray counts are) are removed from the end before the twins are
    placed: the last packet is then partial and gets twins against its own extreme rays."""
    rng = np.random.default_rng(seed)
    lo, size, (hlo, hhi) = SCALES[scale]
    ct = F64 if prec == "d4" else F32
    pencil = kind in ("pinhole", "iso", "healpix")
    if kind == "axis":
        rays, sp = axis_rays(side, axis, sense, lo, size, rng, neg_zero=neg_zero, ragged=ragged, width=width)
        if drop_last:
            assert drop_last % 32 == 0 and 0 < drop_last < len(rays)
            rays = np.ascontiguousarray(rays[:len(rays) - drop_last])
        places = extreme_placements(rays, "axis", width, rng, sp)
        t_range = (0.15, 0.85)
    elif pencil:
        rays = pencil_rays(kind, side, lo, size, rng)
        places = extreme_placements(rays, "pencil", width, rng, None)
        t_range = (0.35, 0.6)
    else:
        rays = general_rays(side * side // 64, lo, size, rng)
        places = extreme_placements(rays, "general", width, rng, None)
        t_range = (0.2, 0.8)
    rng.shuffle(places)
    places = places[:max_twins]
    c, w_hit, w_miss, tgt = _place_radius_twins(rays, places, prec, rng, t_range, pencil)
    twins_c = [c, c]
    twins_w = [w_hit, w_miss]
    hit_tgt, miss_tgt = [tgt], [tgt]
    n_radius = len(c)
    # range twins: the shortest ray of a packet at its end, the ray starting furthest along at
    # its start (the lean test's len_lo, noda_lo / noda_hi), and a few others
    rc_in, rc_out, rw, rt = [], [], [], []
    pk_list = _packets(len(rays), width)
    for pk in pk_list[:: max(1, len(pk_list) // 48)]:
        d = rays[pk, :3].astype(F64); o = rays[pk, 3:6].astype(F64)
        noda = (o * d).sum(axis=1)
        for r, t0 in ((pk[int(np.argmin(rays[pk, 6]))], "len"), (pk[int(np.argmax(noda))], 0),
                      (pk[int(rng.integers(len(pk)))], 0)):
            ray = rays[r]
            w = ct(0.2 * hlo * size)           # a fifth of the smallest background radius
            res = range_twins(ray, float(ray[6]) if t0 == "len" else 0, w, prec)
            if res is None:
                continue
            rc_in.append(res[0]); rc_out.append(res[1]); rw.append(w); rt.append(r)
    if rc_in:
        twins_c += [np.array(rc_in, ct), np.array(rc_out, ct)]
        twins_w += [np.array(rw, ct), np.array(rw, ct)]
        hit_tgt.append(np.array(rt)); miss_tgt.append(np.array(rt))
    # background: uniform in the box, smoothing lengths from the scale's range
    bg = np.empty((n_background, 4), F64)
    bg[:, :3] = lo + rng.random((n_background, 3)) * size
    bg[:, 3] = rng.uniform(hlo, hhi, n_background) * size
    # rim: a twentieth of the background pressed against the faces of the box, so that cluster
    # and group boxes have faces there (the twins themselves are not placed on the rim)
    if rim:
        m = n_background // 20
        ax = rng.integers(0, 3, m)
        bg[np.arange(m), ax] = lo[ax] + np.where(rng.random(m) < 0.5, 0.0, size)
    hit_s = np.concatenate([np.concatenate([twins_c[0], twins_w[0][:, None]], axis=1)] +
                           ([np.concatenate([twins_c[2], twins_w[2][:, None]], axis=1)] if rc_in else []))
    miss_s = np.concatenate([np.concatenate([twins_c[1], twins_w[1][:, None]], axis=1)] +
                            ([np.concatenate([twins_c[3], twins_w[3][:, None]], axis=1)] if rc_in else []))
    spheres = np.concatenate([bg.astype(ct), hit_s.astype(ct), miss_s.astype(ct)])
    n_h, n_m = len(hit_s), len(miss_s)
    hit_ids = n_background + np.arange(n_h)
    miss_ids = n_background + n_h + np.arange(n_m)
    target_hit = np.concatenate(hit_tgt); target_miss = np.concatenate(miss_tgt)
    perm = rng.permutation(len(spheres))                      # the caller's order is arbitrary
    inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
    spheres = np.ascontiguousarray(spheres[perm])
    hit_ids, miss_ids = inv[hit_ids], inv[miss_ids]
    extra = rng.choice(len(rays), min(len(rays), 256), replace=False)
    sub = np.unique(np.concatenate([target_hit, extra]))
    return Scene(rays=rays, spheres=spheres, hit=hit_ids, miss=miss_ids, target_hit=target_hit,
                 target_miss=target_miss, n_radius=n_radius, sub=sub, prec=prec, kind=kind,
                 scale=scale, box=(lo, lo + size), width=width)


def twin_outcomes(sc):
    """(hit twins hit by their ray, miss twins missed by their ray) under the scene's restatement."""
    fn = RESTATE[sc.prec]
    h = fn(sc.rays[sc.target_hit], sc.spheres[sc.hit])[0]
    m = fn(sc.rays[sc.target_miss], sc.spheres[sc.miss])[0]
    return h, ~m


def spotlight_weights(sc, n_channels, seed):
    """float32 [n, C] weights in the scene's caller order that make single twins visible in a
    weighted column density: channel 0 is 1 everywhere (the unweighted trace), channel 1 is 1 on
    the radius twins (hit and miss) and 0 elsewhere, channel 2 the same for the range twins (in and
    out), channel 3 uniform in [-2, 2], channel 4 half of channel 1.  Fewer channels: a prefix,
    except that one channel is channel 1 alone.  With 0 on everything else, channel 1 of a ray is
    exactly the fp32 sum of its twins' terms: a dropped hit twin turns a nonzero value into 0 (or
    changes its bits), a counted miss twin adds a term the reference does not have."""
    assert 1 <= n_channels <= 5
    n, nr = len(sc.spheres), sc.n_radius
    w = np.zeros((n, 5), F32)
    w[:, 0] = 1
    w[sc.hit[:nr], 1] = 1; w[sc.miss[:nr], 1] = 1
    w[sc.hit[nr:], 2] = 1; w[sc.miss[nr:], 2] = 1
    w[:, 3] = np.random.default_rng(seed).uniform(-2, 2, n).astype(F32)
    w[:, 4] = w[:, 1] * F32(0.5)
    return np.ascontiguousarray(w[:, 1:2] if n_channels == 1 else w[:, :n_channels])


def twin_terms(sc, oracle):
    """Per hit twin, the oracle's per-hit integral of the twin traced alone by its target ray
    (float32; 0 where the oracle counts no hit)."""
    out = np.zeros(len(sc.hit), F32)
    for k, (sid, r) in enumerate(zip(sc.hit, sc.target_hit)):
        _, idx, integ, _ = oracle.brute_hits(sc.rays[r:r + 1], sc.spheres[sid:sid + 1].astype(F32))
        if len(idx):
            out[k] = integ[0]
    return out


def visible_twins(sc, oracle):
    """Mask over the radius hit twins (sc.hit[:sc.n_radius]): those whose per-hit integral
    against their target ray is nonzero according to the oracle.  (A grazing twin's table position
    is within a few ulp of the table's end, where the line integral is 0: many terms are exactly 0
    and such a twin cannot be seen in any sum.)"""
    return twin_terms(sc, oracle)[:sc.n_radius] != 0


def sharpness(sc):
    """Fraction of hit twins that no other ray of their packet (runs of sc.width) hits."""
    fn = RESTATE[sc.prec]
    ok = 0
    for sid, r in zip(sc.hit, sc.target_hit):
        p0 = (r // sc.width) * sc.width
        rr = sc.rays[p0:p0 + sc.width]
        hits = fn(rr, np.repeat(sc.spheres[sid][None], len(rr), axis=0))[0]
        ok += int(hits.sum() == 1 and hits[r - p0])
    return ok / max(1, len(sc.hit))


def lattice_scene(scale="unit", seed=0, side=64, n_background=20000, max_places=900):
    """Axis-aligned +z rays on a power-of-two grid and sub-pixel twins (h below the ray spacing)
    against tile-edge rays -- the first and the 8th column and row of 8 x 8 tiles --, so that the
    origin-lattice instantiation runs.  At most `max_places` twin pairs (tile-edge rays drawn at
    random): a 1024 x 1024 grid keeps its brute-force subset small."""
    rng = np.random.default_rng(seed)
    lo, size, _ = SCALES[scale]
    rays, sp = axis_rays(side, 2, 1, lo, size, rng)
    i, j = _morton_tile_order(side)
    li, lj = i % TILE, j % TILE
    # outward (the rectangle's own edge) and, for the 8th column / row, also inward: a sphere
    # between columns 6 and 7 is kept only through the lattice's 8th value
    cand = []
    for k, l in ((0, li), (1, lj)):
        for r in np.nonzero(l == 0)[0]:
            cand.append((r, k, -1.0))
        for r in np.nonzero(l == TILE - 1)[0]:
            cand.append((r, k, 1.0)); cand.append((r, k, -1.0))
    pick = rng.choice(len(cand), min(max_places, len(cand)), replace=False)
    places = []
    for n in pick:
        r, k, sg = cand[n]
        u = np.zeros(3); u[k] = sg
        places.append((int(r), u, sp))
    c, w_hit, w_miss, tgt = _place_radius_twins(rays, places, "f32", rng, (0.15, 0.85), False)
    bg = np.empty((n_background, 4), F64)
    bg[:, :3] = lo + rng.random((n_background, 3)) * size
    bg[:, 3] = rng.uniform(0.05, 0.3, n_background) * sp          # sub-spacing background too
    hit_s = np.concatenate([c, w_hit[:, None]], axis=1)
    miss_s = np.concatenate([c, w_miss[:, None]], axis=1)
    spheres = np.concatenate([bg.astype(F32), hit_s, miss_s]).astype(F32)
    n = n_background
    hit_ids = n + np.arange(len(c)); miss_ids = n + len(c) + np.arange(len(c))
    extra = rng.choice(len(rays), 256, replace=False)
    return Scene(rays=rays, spheres=spheres, hit=hit_ids, miss=miss_ids, target_hit=tgt, target_miss=tgt,
                 n_radius=len(c), sub=np.unique(np.concatenate([tgt, extra])), prec="f32", kind="axis",
                 scale=scale, box=(lo, lo + size), width=64, lattice_cols=i[tgt] % TILE, lattice_rows=j[tgt] % TILE)


# ---- the scenes of tests/test_trace_plan_boundaries.py -------------------------------------------
# (scale, axis, sense, scene options, knobs, weight channels -- each case also runs the unweighted
# trace); the knobs are covered pairwise, not as their full product.  The seeds are chosen so that
# every scene has at least 100 visible radius hit twins (tests/test_trace_boundary_scenes.py).
PLAN_CASES = [
    ("unit", 0, 1, dict(), dict(width=64, reorder=False, split=-1, mpl=8), 4),
    ("1e3", 0, -1, dict(neg_zero=True), dict(width=32, reorder=True, split=2, mpl=8), 1),
    ("1e5", 1, 1, dict(ragged=True), dict(width=16, reorder=False, split=8, mpl=8), 5),
    ("1e-3", 1, -1, dict(ragged=True), dict(width=-1, reorder=True, split=-1, mpl=8), 2),
    ("1e5", 2, 1, dict(neg_zero=True), dict(width=32, reorder=False, split=-1, mpl=1), 3),
    ("unit", 2, -1, dict(ragged=True), dict(width=-1, reorder=False, split=2, mpl=32), 4),
    ("1e3", 2, 1, dict(ragged="one"), dict(width=64, reorder=True, split=-1, mpl=8), 4),
    ("1e5", 0, -1, dict(ragged="one"), dict(width=64, reorder=False, split=4, mpl=8), 1),
    ("unit", 2, 1, dict(drop_last=32), dict(width=64, reorder=False, split=-1, mpl=8), 4),
]
PLAN_BACKGROUND = 20000
PLAN_LATTICE_SCALES = ("unit", "1e3", "1e5", "1e-3")


def plan_case_width(case):
    """The packet width the library runs row `case` at, which the twins are placed against: the
    knob's where it is set; with the automatic width, a column-density batch of 4096 rays runs
    packets of 16 rays (fewer than 512 packets of any wider kind) unless the split is set by hand,
    which keeps 64 (row 6)."""
    knobs = PLAN_CASES[case][4]
    if knobs["width"] > 0:
        return knobs["width"]
    return 64 if knobs["split"] > 0 else 16


def plan_case_scene(case, n_background=PLAN_BACKGROUND):
    """The scene of row `case` of PLAN_CASES.  (The twins are placed before the background is
    drawn: they do not depend on n_background.)"""
    scale, axis, sense, opts, knobs, _ = PLAN_CASES[case]
    return boundary_scene("axis", scale, "f32", seed=300 + case, axis=axis, sense=sense,
                          width=plan_case_width(case), n_background=n_background, max_twins=600, **opts)


def plan_lattice_scene(scale, n_background=PLAN_BACKGROUND):
    return lattice_scene(scale, seed=320 + PLAN_LATTICE_SCALES.index(scale), n_background=n_background)
