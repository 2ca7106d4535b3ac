"""Scenes and the NumPy restatement for the periodic point queries (grace_range_counts_periodic_f4,
grace_range_neighbours_periodic_f4, grace_fof_labels_periodic_f4, grace_pair_counts_periodic_f4).

The restatement is the contract of include/grace_hip.h, "Periodic boxes": per component, in float32,
d = fl(p - x); h = fl(0.5 L) (exact); d > h: d = fl(d - L); else d < -h: d = fl(d + L) -- at most one
wrap, none on an open axis (L == 0) -- then d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) as for the
open queries (d2_rows of test_neighbours.py, whose operation order this keeps).  Everything downstream
is the open queries' own: membership d2 <= fl(r r), rows in ascending tree index, the bin of a pair
the smallest k with d2 <= fl(e_k e_k), the gather sums (restate_sums of test_range_queries.py, fed
with these lists), the union-find of test_fof.py over the links d2 <= fl(b b).  A point is
additionally off if its radius exceeds fl(0.5 L) on a periodic axis.

The scenes are the smallest that reach every branch of the periodic walk: a 16^3 lattice that fills the
box (every wrap is exact, d2 == R2 across the seam, one, two and three axes wrapped at the corners),
uniform points in an isotropic and in an anisotropic box with an open axis, centres within a few ulp
of both ends of the box with radii down to 1e-7 L, more than 64 coincident queries in a corner cell,
a coincident spine at a corner, one sphere -- each at offsets that put the seam at 0, inside the data's
coordinates' sign change (-0.5) and far from the origin (+100), where fl(p - x) and the shifted bounds
round in units of 2^-17."""
import numpy as np

from test_fof import unite
from test_neighbours import _coincident_scene
from test_range_queries import is_on as open_is_on

F32 = np.float32
OFFSETS = (0.0, -0.5, 100.0)
BOXES = {"cube": (1.0, 1.0, 1.0), "slab": (1.0, 0.5, 0.0)}          # slab: anisotropic, z open
LATTICE_RADII = np.array([1.0 / 16.0, 2.0 / 16.0, np.sqrt(2.0) / 16.0]).astype(F32)
LATTICE_COUNTS = (7, 33, 7)                                          # per point, on the torus


# ---- the restatement ----------------------------------------------------------------------------
def half(L):
    return F32(0.5) * F32(L)


def wrap(d, L):
    """One component of the separation, wrapped at most once (d: float32 array; L: one period)."""
    L = F32(L)
    if L == 0:
        return d
    h = half(L)
    with np.errstate(invalid="ignore"):
        up = d > h
        down = ~up & (d < -h)
    out = d.copy()
    out[up] = (d[up] - L).astype(F32)
    out[down] = (d[down] + L).astype(F32)
    return out


def d2_rows(p, x, period):
    """fp32 wrapped d2 of points p [m, 3] to centres x [n, 3]: test_neighbours.d2_rows with the wrap."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = wrap((p[:, None, 0] - x[None, :, 0]).astype(F32), period[0])
        dy = wrap((p[:, None, 1] - x[None, :, 1]).astype(F32), period[1])
        dz = wrap((p[:, None, 2] - x[None, :, 2]).astype(F32), period[2])
        return ((dx * dx + dy * dy) + dz * dz).astype(F32)


def is_on(points, radii, period):
    on = open_is_on(points, radii)
    with np.errstate(invalid="ignore"):
        for L in period:
            if F32(L) > 0:
                on &= ~(radii > half(L))
    return on


def restate(points, radii, spheres, period):
    """(counts int32 [m], offsets int32 [m + 1], indices int32 [total], d2 float32 [total]): the layout of
    test_range_queries.restate."""
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    r = np.broadcast_to(np.asarray(radii, F32), (len(P),)).copy()
    on = is_on(P, r, period)
    with np.errstate(over="ignore", invalid="ignore"):
        R2 = (r * r).astype(F32)
    chunk = max(1, (1 << 21) // max(len(X), 1))
    rows, cols, vals = [], [], []
    for a in range(0, len(P), chunk):
        d2 = d2_rows(P[a:a + chunk], X, period)
        with np.errstate(invalid="ignore"):
            hit = (d2 <= R2[a:a + chunk, None]) & on[a:a + chunk, None]
        pi, si = np.nonzero(hit)                       # row-major: ascending sphere index within a point
        rows.append(pi + a); cols.append(si); vals.append(d2[pi, si])
    pi = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    si = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    dd = np.concatenate(vals).astype(F32) if vals else np.zeros(0, F32)
    counts = np.bincount(pi, minlength=len(P)).astype(np.int32)
    offsets = np.zeros(len(P) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return counts, offsets.astype(np.int32), si.astype(np.int32), dd


def restate_bins(points, edges, spheres, period, weights=None, lists=None):
    """(totals uint64 [E], counts int32 [m, E], sums float32 [m, E, C] or None): the pairs within the last
    edge, each in the smallest bin k with d2 <= fl(e_k e_k); the sums run in ascending tree index."""
    e = np.asarray(edges, F32)
    E2 = (e * e).astype(F32)
    m, ne = len(points), len(e)
    counts, offsets, si, d2 = lists if lists is not None else restate(points, e[-1], spheres, period)
    pi = np.repeat(np.arange(m), counts)
    k = np.searchsorted(E2, d2, side="left")
    assert np.all(k < ne)
    hist = np.bincount(pi * ne + k, minlength=m * ne).reshape(m, ne)
    sums = None
    if weights is not None:
        sums = np.zeros((m * ne, weights.shape[1]), F32)
        for c in range(weights.shape[1]):
            np.add.at(sums[:, c], pi * ne + k, weights[si, c])       # unbuffered: one fp32 add per pair, in order
        sums = sums.reshape(m, ne, weights.shape[1])
    return hist.sum(axis=0).astype(np.uint64), hist.astype(np.int32), sums


def links(x, b, period):
    """The link graph's edges (i, j), j < i, of centres x [n, 3] at linking length b."""
    x = np.ascontiguousarray(x[:, :3], F32)
    b2 = F32(b) * F32(b)
    ii, jj = [], []
    rows = max(1, (1 << 21) // max(len(x), 1))
    for a in range(0, len(x), rows):
        e = min(a + rows, len(x))
        d2 = d2_rows(x[a:e], x[:e], period)
        with np.errstate(invalid="ignore"):
            i, j = np.nonzero(d2 <= b2)
        keep = j < i + a
        ii.append(i[keep] + a); jj.append(j[keep])
    return np.concatenate(ii), np.concatenate(jj)


def restate_labels(x, b, period):
    """labels int32 [n]: the smallest index of each connected component of the link graph."""
    i, j = links(x, b, period)
    parent = np.arange(len(x), dtype=np.int64)
    unite(parent, i, j)
    unite(parent, np.zeros(1, np.int64), np.zeros(1, np.int64))    # compress
    return parent.astype(np.int32)


# ---- scenes ---------------------------------------------------------------------------------------
def spheres_of(x, h=0.01):
    s = np.empty((len(x), 4), F32)
    s[:, :3] = x
    s[:, 3] = F32(h)
    return s


def lattice(offset, m=16):
    """m^3 sites at offset + k / m: they fill the period-1 box, every site is every other's translate."""
    g = (F32(offset) + np.arange(m, dtype=F32) / F32(m)).astype(F32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return spheres_of(np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1), 1.0 / m)


def uniform(n, box, offset, seed):
    """n uniform centres in [offset, offset + L) per periodic axis (an open axis: [offset, offset + 1))."""
    rng = np.random.default_rng(seed)
    ext = np.array([L if L > 0 else 1.0 for L in BOXES[box]], F32)
    return spheres_of((F32(offset) + rng.random((n, 3), dtype=F32) * ext).astype(F32))


def special_radii(box):
    """Radii at the contract's edges: exactly half of each period (on), its successor (off), 0, -0, negative,
    NaN, +inf."""
    out = [0.0, -0.0, -0.125, np.nan, np.inf]
    for L in BOXES[box]:
        if L > 0:
            out += [half(L), np.nextafter(half(L), F32(np.inf))]
    return np.array(out, F32)


def uniform_queries(s, box, offset, seed, m=1200):
    """(points [m, 3], radii [m]): centres and points in and just outside the box, radii log-uniform up to
    half the smallest period, the special radii at the first points (which are centres)."""
    rng = np.random.default_rng(seed + 1000)
    lmin = min(L for L in BOXES[box] if L > 0)
    ext = np.array([L if L > 0 else 1.0 for L in BOXES[box]], F32)
    inside = (F32(offset) + (rng.random((m // 2, 3), dtype=F32) * F32(1.1) - F32(0.05)) * ext).astype(F32)
    pts = np.concatenate([s[rng.choice(len(s), m - m // 2, replace=False), :3], inside]).astype(F32)
    r = np.exp(rng.uniform(np.log(1e-4 * lmin), np.log(0.5 * lmin), m)).astype(F32)
    sp = special_radii(box)
    r[:len(sp)] = sp
    r[len(sp):len(sp) + 20] = half(lmin)                              # long rows at the largest radius
    return pts, r


def seam(offset, L=1.0):
    """Centres within a few ulp of both ends of the period-L box on every axis combination, a pair exactly one
    period apart, 80 coincident centres in the low corner and a sprinkle inside.  Returns (spheres, points,
    radii): the queries are the centres near the faces, each at radii from 1e-7 L up."""
    o, e = F32(offset), F32(offset) + F32(L)
    rng = np.random.default_rng(77)

    def steps(v, k):                                                 # v moved by k ulp
        for _ in range(abs(k)):
            v = np.nextafter(v, F32(np.inf) if k > 0 else F32(-np.inf))
        return v
    lo = [steps(o, k) for k in (0, 1, 2, 5)]
    hi = [steps(e, -k) for k in (1, 2, 3, 7)] + [e]                  # e itself: one period from o
    ends = np.array(lo + hi, F32)
    x = ends[rng.integers(0, len(ends), (300, 3))]                   # corners, edges
    face = (o + rng.random((300, 3), dtype=F32) * F32(L)).astype(F32)
    axis = rng.integers(0, 3, 300)
    face[np.arange(300), axis] = ends[rng.integers(0, len(ends), 300)]   # faces
    corner = np.tile(np.array([[lo[1], lo[0], lo[2]]], F32), (80, 1))
    inside = (o + rng.random((400, 3), dtype=F32) * F32(L)).astype(F32)
    pair = np.array([[o, o, o], [e, o, o], [e, e, e]], F32)
    s = spheres_of(np.concatenate([pair, x, face, corner, inside]))
    q = np.concatenate([pair, x, face[:200], corner])                 # > 64 coincident queries in the corner cell
    radii = np.array([0.0, 1e-7, 3e-7, 1e-6, 1e-5, 1e-3, 0.05, 0.5], F32) * F32(L)
    r = radii[np.arange(len(q)) % len(radii)]
    r[:3] = 0.0
    return s, q.astype(F32), r.astype(F32)


def corner_spine(offset):
    """test_neighbours' coincident scene with its 200 coincident centres moved into the low corner of the
    box and its 100 onto the opposite faces: at max_per_leaf 1 a spine of leaves deeper than the stack whose
    queries wrap on three axes."""
    s = _coincident_scene()
    s[:100, :3] = np.array([1.0 - 2.0 ** -20, 0.5, 1.0 - 2.0 ** -22], F32)
    s[100:300, :3] = np.array([2.0 ** -21, 2.0 ** -20, 0.0], F32)
    s[:, :3] = (s[:, :3] + F32(offset)).astype(F32)
    return s


def straddling_clump(offset, n=400, seed=5):
    """A clump centred on the x = offset face of the period-1 box (half of it wrapped to the far side) and a
    thin uniform background: one group at b with the period, two without."""
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 0.01, (n, 3)) + np.array([0.0, 0.5, 0.5])
    c[:, 0] = np.mod(c[:, 0], 1.0)
    bg = rng.random((600, 3))
    return spheres_of((np.concatenate([c, bg]) + offset).astype(F32))


def torus_chain(offset, gap=29):
    """64 points on a line along x at spacing 1/64 (exact), one of them missing: a chain that is one group
    only through the seam; y and z constant."""
    k = np.arange(64)
    k = k[k != gap]
    x = np.full((len(k), 3), 0.25, F32)
    x[:, 0] = k.astype(F32) / F32(64)
    return spheres_of((x + F32(offset)).astype(F32))


def components(n, i, j):
    """Connected components by plain label propagation: a second method beside unite()."""
    lab = np.arange(n)
    while True:
        new = lab.copy()
        np.minimum.at(new, i, lab[j])
        np.minimum.at(new, j, lab[i])
        if np.array_equal(new, lab):
            return lab.astype(np.int32)
        lab = new
