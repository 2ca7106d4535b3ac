"""Scenes, a packet census and a cell-list link finder for the periodic point queries at the packet
thresholds (test_periodic_point_query_packets.py; test_periodic_packet_scenes.py checks this file).

Which path a packet of a periodic walk takes (csrc/range_walk.hpp, neighbours.hip, interpolate.hip) is
decided by its union box alone: no wider than h = fl(L / 2) on every axis (`narrow`: a cluster whose
survivors all came through the box itself skips the wrap) or not, and whether a box shifted by -+L meets
the tree's root box on some axis (`images`) or not (the walk tests the box itself only).  packet_census()
restates the packets of a point set (the keys, the stable sort and the cuts of csrc/point_packets.hip)
and classifies them, so that the CPU test can state which classes each input of the GPU matrix reaches.

torus_scene() is the clustered scene those inputs are queried against: it fills the periodic cell, its
blobs sit on a corner, a face and an edge of it, and a coincident group lies one ulp inside the x face."""
import numpy as np

import periodic_point_scenes as PS
import periodic_query_scenes as S
from test_point_query_packets import LAYOUTS, N_OFF, PointSet, cell_level, restate_keys, root_box

F32 = np.float32
F64 = np.float64
BLOBS = np.array([[0.746, 0.746, 0.746], [0.0, 0.0, 0.0], [0.0, 0.35, 0.4], [0.5, 0.0, 0.0]])   # cell fractions
CLUMP_AT = 0.766                                                     # the first blob: this fraction of the root box
N_CO = 100                                                           # the coincident group
N_BRIDGE = 8
EDGE_BAND = 1e-4                                                     # census: relative distance to a threshold left unclassified


def extent(period):
    """The cell: the period on a periodic axis, 1 on an open one."""
    return np.array([L if L > 0 else 1.0 for L in period], F64)


def lmin_of(period):
    return min(float(L) for L in period if L > 0)


# ---- scenes ---------------------------------------------------------------------------------------
def _torus(period, n, rng, offset):
    """float32 [n, 4], not yet permuted: blobs, background (the bridge first), coincident group."""
    ext, lmin = extent(period), lmin_of(period)
    n_bg = n // 4
    n_blob = n - n_bg - N_CO
    which = rng.integers(0, len(BLOBS), n_blob)
    noise = rng.normal(0.0, 0.03 * lmin, (n_blob, 3))
    bg = rng.random((n_bg, 3)) * ext
    co = np.array([float(np.nextafter(F32(ext[0]), F32(0))), 0.0, 0.5 * ext[2]])
    # a bridge from the coincident group's image across the x face into the cell (it takes the place of the
    # first background spheres): the group's friends-of-friends component has members on both sides
    bg[:N_BRIDGE] = co
    bg[:N_BRIDGE, 0] = 0.01 * lmin * np.arange(1, N_BRIDGE + 1)
    X = np.concatenate([BLOBS[which] * ext + noise, bg, np.tile(co, (N_CO, 1))])
    H = np.exp(rng.uniform(np.log(1e-3 * lmin), np.log(0.04 * lmin), n))
    first = np.zeros(n, bool)
    first[:n_blob] = which == 0
    H[first] = rng.uniform(0.02 * lmin, 0.04 * lmin, int(first.sum()))
    for a, L in enumerate(period):
        if L > 0:
            X[:, a] = np.mod(X[:, a], float(L))                      # into [0, L) in fp64
    # the first blob goes to the fraction CLUMP_AT of the root box, which the other spheres decide: the middle
    # of the point sets' off points, inside the clumped layout's cell at every level
    lo = (X[~first] - H[~first, None]).min(axis=0)
    hi = (X[~first] + H[~first, None]).max(axis=0)
    X[first] = lo + CLUMP_AT * (hi - lo) + noise[which == 0]
    s = np.empty((n, 4), F32)
    s[:, :3] = (X + offset).astype(F32)
    s[:, 3] = H.astype(F32)
    for a, L in enumerate(period):
        if L > 0:                                                    # a cast that lands on L goes to 0
            s[s[:, a] >= F32(offset + float(L)), a] = F32(offset)
    return s


def torus_scene(period, n=3000, seed=2, offset=0.0):
    """float32 [n, 4]: four Gaussian blobs (sigma 0.03 Lmin) -- one where the clumped layout puts its clump,
    three at the cell fractions BLOBS[1:]: a corner, a face and an edge -- n / 4 uniform background spheres, a
    coincident group of 100 one ulp inside the x face with a short bridge across it; H log-uniform in
    [1e-3, 0.04] Lmin, so that the root box stays within 0.04 Lmin of the cell; rows permuted.
    Two choices are there so that every point set of the matrix has points inside more than a wave of spheres
    (counts.max() > 64 in the interpolation): the first blob is centred on the fraction CLUMP_AT of the root
    box on every axis (the cell fraction BLOBS[0], kept for reference, is about 0.73 of the root box: outside
    the clump's cell from 16384 points up, and two sigma from the point sets' off points, which are the only
    points every case has in one place), and its members' H is uniform in [0.02, 0.04] Lmin."""
    rng = np.random.default_rng(seed)
    s = _torus(period, n, rng, offset)
    return s[rng.permutation(n)]


def torus_scene_wide_H(box, n=3000, seed=2, offset=0.0, scale=1.0):
    """torus_scene of S.BOXES[box] for the interpolation: 5 % of H log-uniform from 0.04 to 0.5 of the smallest
    period and the contract's edge radii (PS.special_H: half a period, its successor, 0) at the first spheres;
    `scale` multiplies everything (a power of two or 1.5: the edge radii are those of the scaled period)."""
    period = S.BOXES[box]
    rng = np.random.default_rng(seed)
    lmin = lmin_of(period)
    s = _torus(period, n, rng, offset)
    s = s[rng.permutation(n)]
    big = rng.random(n) < 0.05
    s[big, 3] = np.exp(rng.uniform(np.log(0.04 * lmin), np.log(0.5 * lmin), int(big.sum()))).astype(F32)
    s = (s * F32(scale)).astype(F32)
    sp = []
    for L in period:
        if L > 0:
            h = S.half(F32(L) * F32(scale))
            sp += [h, np.nextafter(h, PS.INF)]
    sp = np.array(sp + [0.0], F32)
    s[:len(sp), 3] = sp
    return s


def sparse_scene(seed=9):
    """300 spheres in the unit cube: 200 in a blob of sigma 0.02 and 100 uniform.  With k = 64 a query in the
    blob finds its k-th neighbour well inside h / 2, one in the void beyond h = 0.5."""
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.array([0.3, 0.6, 0.45]) + rng.normal(0.0, 0.02, (200, 3)), rng.random((100, 3))])
    s = S.spheres_of(x.astype(F32))
    return s[rng.permutation(len(s))]


def sparse_queries(s, seed=10):
    """500 uniform points of the unit cube, then the centres."""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.random((500, 3), dtype=F32), s[:, :3]]).astype(F32)


# ---- the matrix of the GPU module: (box, m, layout, offset) ----------------------------------------------
SIZES_P = (2047, 2048, 2049, 16383, 16384, 16385, 131073)           # (131073: pooled to <= 16384 records)
CASES = ([("cube", m, layout, 0.0) for m in SIZES_P for layout in LAYOUTS]
         + [("slab", m, layout, 0.0) for m in (2049, 16385) for layout in LAYOUTS]
         + [("cube", 2049, "spread", 100.0)])
N_SAMPLE = 2000

_scene_cache, _set_cache = {}, {}


def case_id(case):
    box, m, layout, offset = case
    return "%s-%d-%s%s" % (box, m, layout, "" if offset == 0 else "-at%g" % offset)


def case_scene(box, offset=0.0):
    """(torus_scene of the box, the restated root box of its tree: lo, hi)."""
    if (box, offset) not in _scene_cache:
        s = torus_scene(S.BOXES[box], offset=offset)
        _scene_cache[(box, offset)] = (s, *root_box(s))
    return _scene_cache[(box, offset)]


def case_points(case):
    """The open module's PointSet on the root box of the case's scene, its radii kept; the last three of its
    normal records get half the smallest period, its successor (off) and 0."""
    if case not in _set_cache:
        box, m, layout, offset = case
        _, lo, hi = case_scene(box, offset)
        ps = PointSet(m, layout, lo, hi)
        n_norm = ps.n_rec - N_OFF
        h = S.half(lmin_of(S.BOXES[box]))
        ps.special = np.arange(n_norm - 3, n_norm)
        ps.rec_radii[ps.special] = np.array([h, np.nextafter(h, PS.INF), 0.0], F32)
        _set_cache[case] = ps
    return _set_cache[case]


def case_sample(ps):
    """N_SAMPLE point indices for the wrap counts: a draw, and with it the first point of each of the three
    special records (the one point in m with r = h holds most of the pairs that wrap on two and three axes;
    the figures should not depend on whether the draw caught it)."""
    rng = np.random.default_rng(ps.m)
    first = np.array([np.nonzero(ps.index == rec)[0][0] for rec in ps.special])
    draw = rng.choice(ps.m, min(N_SAMPLE, ps.m), replace=False)
    return np.concatenate([first, draw[~np.isin(draw, first)]])[:min(N_SAMPLE, ps.m)]


def case_census(case):
    box, m, layout, offset = case
    s, lo, hi = case_scene(box, offset)
    ps = case_points(case)
    return packet_census(ps.points, ps.radii, lo, hi, m, S.BOXES[box], s, case_sample(ps))


# ---- the packets, restated --------------------------------------------------------------------------
def packet_census(points, radii, lo, hi, m, period, spheres=None, sample=None):
    """The packets of `points` (keys against the root box [lo, hi], a stable sort by key, a cut at every change
    of the Morton cell of cell_level(m) and at every 64th point of a cell) with the range walk's boxes:
    per packet the fp64 union of [p - r, p + r] over its on lanes (S.is_on), and
      wide    some periodic axis of the box is wider than h = L / 2 (narrow otherwise);
      images  the box shifted by -L or +L meets the root box on some periodic axis.
    A packet within EDGE_BAND (relative) of either threshold, and one without an on lane, is left out of
    the four counts.  With `spheres` and `sample` (point indices) also the in-range pairs (wrapped d2 <=
    fl(r r)) of the sampled points whose separation wraps on exactly 1, 2 and 3 axes.
    Returns a dict: n_packets, wide, narrow, images, none, narrow_images, box_lo / box_hi [n_packets, 3],
    is_wide / is_images / classified [n_packets], wraps (n1, n2, n3)."""
    P = np.asarray(points, F32)[:, :3]
    r = np.asarray(radii, F32)
    level = cell_level(m)
    keys = restate_keys(P, lo, hi)
    order = np.argsort(keys, kind="stable")
    cells = (keys >> np.uint32(30 - 3 * level))[order]
    first = np.ones(len(P), bool)
    first[1:] = cells[1:] != cells[:-1]
    start_of_cell = np.maximum.accumulate(np.where(first, np.arange(len(P)), 0))
    cut = first | ((np.arange(len(P)) - start_of_cell) % 64 == 0)
    packet = np.cumsum(cut) - 1
    n_packets = int(packet[-1]) + 1
    on = S.is_on(P, r, period)[order]
    p64, r64 = P[order].astype(F64), r[order].astype(F64)
    blo = np.full((n_packets, 3), np.inf)
    bhi = np.full((n_packets, 3), -np.inf)
    np.minimum.at(blo, packet[on], p64[on] - r64[on, None])
    np.maximum.at(bhi, packet[on], p64[on] + r64[on, None])
    live = np.isfinite(blo[:, 0])
    rlo, rhi = np.asarray(lo, F64), np.asarray(hi, F64)
    is_wide = np.zeros(n_packets, bool)
    is_images = np.zeros(n_packets, bool)
    sharp = live.copy()
    with np.errstate(invalid="ignore"):
        for a, L in enumerate(period):
            L = float(F32(L))
            if L == 0:
                continue
            h = 0.5 * L
            width = bhi[:, a] - blo[:, a]
            is_wide |= width > h
            sharp &= ~(np.abs(width - h) <= EDGE_BAND * h)
            # the box moved by -L meets the root box: bhi - L >= rlo (blo - L <= rhi holds anyway); by +L: blo + L <= rhi
            gap_m, gap_p = (bhi[:, a] - L) - rlo[a], rhi[a] - (blo[:, a] + L)
            is_images |= (gap_m >= 0) & (blo[:, a] - L <= rhi[a])
            is_images |= (gap_p >= 0) & (bhi[:, a] + L >= rlo[a])
            sharp &= ~(np.abs(gap_m) <= EDGE_BAND * L) & ~(np.abs(gap_p) <= EDGE_BAND * L)
    out = {"n_packets": n_packets, "box_lo": blo, "box_hi": bhi, "is_wide": is_wide, "is_images": is_images,
           "classified": sharp,
           "wide": int(np.sum(sharp & is_wide)), "narrow": int(np.sum(sharp & ~is_wide)),
           "images": int(np.sum(sharp & is_images)), "none": int(np.sum(sharp & ~is_images)),
           "narrow_images": int(np.sum(sharp & ~is_wide & is_images)), "wraps": None}
    if spheres is not None and sample is not None:
        out["wraps"] = wrapped_pairs(P[sample], r[sample], spheres, period)
    return out


def wrapped_pairs(points, radii, spheres, period):
    """(n1, n2, n3): the in-range pairs (wrapped d2 <= fl(r r), on points) whose separation wraps on exactly
    1, 2 and 3 axes."""
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    r = np.asarray(radii, F32)
    on = S.is_on(P, r, period)
    with np.errstate(over="ignore", invalid="ignore"):
        R2 = (r * r).astype(F32)
        hit = (S.d2_rows(P, X, period) <= R2[:, None]) & on[:, None]
        n_wrapped = np.zeros(hit.shape, np.int8)
        for a, L in enumerate(period):
            if F32(L) > 0:
                d = (P[:, None, a] - X[None, :, a]).astype(F32)
                n_wrapped += np.abs(d) > S.half(L)
    return tuple(int(np.sum(hit & (n_wrapped == k))) for k in (1, 2, 3))


# ---- friends-of-friends links from a cell list ------------------------------------------------------------
def links_cells(x, b, period):
    """The edges (i, j), j < i, of S.links(x, b, period) -- the decision is still S.d2_rows in fp32 -- found from
    a cell list: cells of side >= max(b, a 16th of the extent) (times 1 + 1e-5: two centres within b of each
    other in fp32 are in neighbouring cells), an integer number of them per period on a periodic axis, and the
    27 neighbours of each cell, through the seam where the axis is periodic.  Centres with a non-finite
    coordinate link to nothing.  Sorted by (i, j)."""
    x = np.ascontiguousarray(x[:, :3], F32)
    n = len(x)
    b2 = F32(b) * F32(b)
    ok = np.all(np.isfinite(x), axis=1)
    x64 = x.astype(F64)
    side = float(b) * (1.0 + 1e-5)
    cell = np.zeros((n, 3), np.int64)
    n_cells = np.ones(3, np.int64)
    for a, L in enumerate(period):
        L = float(F32(L))
        xa = x64[ok, a]
        if L > 0:
            n_cells[a] = max(1, min(16, int(np.floor(L / side)) if side > 0 else 16))
            t = np.mod(xa, L) / L                                     # any coordinates: no box origin is needed
            cell[ok, a] = np.minimum((t * n_cells[a]).astype(np.int64), n_cells[a] - 1)
        else:
            x0, width = (xa.min(), xa.max() - xa.min()) if len(xa) else (0.0, 0.0)
            n_cells[a] = max(1, min(16, int(np.floor(width / side)) if side > 0 and width > 0 else (16 if width > 0 else 1)))
            w = width / n_cells[a] if width > 0 else 1.0
            cell[ok, a] = np.minimum(((xa - x0) / w).astype(np.int64), n_cells[a] - 1)
    flat = (cell[:, 2] * n_cells[1] + cell[:, 1]) * n_cells[0] + cell[:, 0]
    idx = np.nonzero(ok)[0]
    idx = idx[np.argsort(flat[idx], kind="stable")]
    sorted_flat = flat[idx]
    n_flat = int(np.prod(n_cells))
    starts = np.searchsorted(sorted_flat, np.arange(n_flat + 1))
    ii, jj = [], []
    for c in range(n_flat):
        mine = idx[starts[c]:starts[c + 1]]
        if len(mine) == 0:
            continue
        cx, cy, cz = c % n_cells[0], (c // n_cells[0]) % n_cells[1], c // (n_cells[0] * n_cells[1])
        near = set()
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q = [cx + dx, cy + dy, cz + dz]
                    for a in range(3):
                        if F32(period[a]) > 0:
                            q[a] %= n_cells[a]
                    if all(0 <= q[a] < n_cells[a] for a in range(3)):
                        near.add(int((q[2] * n_cells[1] + q[1]) * n_cells[0] + q[0]))
        others = np.concatenate([idx[starts[q]:starts[q + 1]] for q in sorted(near)])
        for a0 in range(0, len(mine), 2048):
            part = mine[a0:a0 + 2048]
            d2 = S.d2_rows(x[part], x[others], period)
            with np.errstate(invalid="ignore"):
                i, j = np.nonzero(d2 <= b2)
            gi, gj = part[i], others[j]
            keep = gj < gi
            ii.append(gi[keep]); jj.append(gj[keep])
    i = np.concatenate(ii) if ii else np.zeros(0, np.int64)
    j = np.concatenate(jj) if jj else np.zeros(0, np.int64)
    order = np.lexsort((j, i))
    return i[order], j[order]


def labels_cells(x, b, period):
    """S.restate_labels with the links of links_cells."""
    from test_fof import unite
    i, j = links_cells(x, b, period)
    parent = np.arange(len(x), dtype=np.int64)
    unite(parent, i, j)
    unite(parent, np.zeros(1, np.int64), np.zeros(1, np.int64))      # compress
    return parent.astype(np.int32)
