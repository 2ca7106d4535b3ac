"""Inputs and plain restatements for the front end's boundaries: Morton keys, deltas, ray generators.

A plain helper module (numpy and fractions only; no GPU, no torch device, no oracle):
tests/test_front_end_boundaries.py runs its cases on the GPU, tests/test_front_end_cases.py checks
on the CPU that each builder hits what it claims and that these restatements agree with the C
oracle and with each other.

Sizes.  stream_grid() caps a launch at 4096 blocks of 256 threads = 2^20 threads and every Morton
kernel and ray generator is a grid-stride loop, so 2^20 + 1 elements is the smallest input that
makes a thread take a second iteration.  Inputs of that size index a pool of POOL distinct records:
POOL is prime and 2^20 mod POOL != 0, so element i and element i + 2^20 differ.
"""
from fractions import Fraction

import numpy as np

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64

GRID = 1 << 20                    # stream_grid: 4096 blocks x 256 threads
SIZES = (1, 255, 256, 257, GRID - 1, GRID, GRID + 1, GRID + 257)
POOL = 4099
NAN_BITS = 0x7FC0BEEF             # float32 pre-fill: a NaN no arithmetic produces
NAN64_BITS = 0x7FF80000DEADBEEF   # float64 pre-fill
KEY32_FILL = 0xDEADBEEF           # above 2^30: no 30-bit key
KEY64_FILL = 0xDEADBEEFDEADBEEF   # above 2^63: no 63-bit key

assert GRID % POOL != 0


def pool_index(n):
    return np.arange(n, dtype=np.int64) % POOL


# ---------------------------------------------------------------------------------------------
# Morton keys
# ---------------------------------------------------------------------------------------------
SPAN = {30: (1 << 10) - 1, 63: (1 << 21) - 1}
CELL_KS = {30: (0, 1, 2, 511, 512, 1022, 1023),
           63: (0, 1, (1 << 20) - 1, 1 << 20, (1 << 21) - 2, (1 << 21) - 1)}
# Every corner is a float32 value, so the same box serves float and double bounds and every float
# co-ordinate between the corners is inside the box for both.
BOXES = {
    "unit": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "offset": ((-3.0, 2.0, 10.0), (5.0, 9.0, 11.0)),
    "negative": ((-9.0, -7.5, -2.0), (-1.0, -0.5, -1.25)),
    "aniso": ((0.0, 0.0, 0.0), (float(F32(1e-3)), 1.0, float(F32(1e3)))),
}


def box(name, real=F32):
    lo, hi = BOXES[name]
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    assert np.array_equal(lo.astype(F64), np.asarray(BOXES[name][0])), "corner is not a float32"
    return lo.astype(real), hi.astype(real)


def pool_points(name, seed=0, cols=4, dtype=F32):
    """POOL distinct records in the box: x y z uniform, then (cols - 3) filler columns that a kernel
    reading the wrong element of a record would pick up as a co-ordinate far outside the box."""
    lo, hi = box(name, F64)
    rng = np.random.default_rng(seed)
    p = np.empty((POOL, cols), F64)
    p[:, :3] = lo + rng.random((POOL, 3)) * (hi - lo)
    p[:, 3:] = 1e6 + rng.random((POOL, cols - 3))
    p = p.astype(dtype)
    # narrowed to float the co-ordinates must still lie inside the box
    c = np.clip(p[:, :3].astype(F32), lo.astype(F32), hi.astype(F32))
    if dtype == F32:
        p[:, :3] = c
    else:
        out = p[:, :3].astype(F32) != c
        p[:, :3][out] = c[out]
    assert len(np.unique(p[:, :3], axis=0)) == POOL
    return np.ascontiguousarray(p)


def pool_triangles(name, seed=0):
    """POOL triangles {v, e1, e2} whose fp32 centroids v + fl(1/3) * (e1 + e2) lie inside the box
    (checked by the CPU test through the oracle's centroid bounds)."""
    lo, hi = box(name, F64)
    rng = np.random.default_rng(seed + 17)
    ext = hi - lo
    c = lo + (0.05 + 0.9 * rng.random((POOL, 3))) * ext
    e1 = (rng.random((POOL, 3)) - 0.5) * 0.02 * ext
    e2 = (rng.random((POOL, 3)) - 0.5) * 0.02 * ext
    t = np.concatenate([c - (e1 + e2) / 3.0, e1, e2], axis=1).astype(F32)
    return np.ascontiguousarray(t)


def scaled_exact(c, lo, hi, span):
    """span * (c - lo) / (hi - lo) of the binary values of c, lo, hi, as a Fraction."""
    c, lo, hi = (Fraction(float(v)) for v in (c, lo, hi))
    return span * (c - lo) / (hi - lo)


def rounding_bound(v, real):
    """How far the device's scaled value fl(fl(span / fl(hi - lo)) * fl(c - lo)) can lie from the
    exact v = span (c - lo) / (hi - lo), from its roundings in `real` alone (u = 2^-24 or 2^-53):

        d = (hi - lo)(1 + e1)     s = span / d (1 + e2)     m = (c - lo)(1 + e3)     p = s m (1 + e4)

    with |e_k| <= u, so p = v (1 + e2)(1 + e3)(1 + e4) / (1 + e1) and |p - v| <= v ((1 + u)^3 / (1 - u)
    - 1).  The three roundings of the key arithmetic proper are e2..e4; e1 is the width of the box,
    exact in the unit box.  The conversion to an integer truncates and adds nothing (p >= 0)."""
    u = Fraction(1, 1 << (24 if np.dtype(real) == np.dtype(F32) else 53))
    return Fraction(v) * ((1 + u) ** 3 / (1 - u) - 1)


def exact_cells(coords, lo, hi, bits, real):
    """For float32 co-ordinates of one axis: (floor of the exact scaled value, True where the exact
    value is farther from an integer than rounding_bound, so that the device's cell must equal it)."""
    span = SPAN[bits]
    cells = np.empty(len(coords), np.int64)
    firm = np.empty(len(coords), bool)
    for i, c in enumerate(coords):
        v = scaled_exact(F32(c), lo, hi, span)
        fl = v.numerator // v.denominator
        e = rounding_bound(v, real)
        cells[i] = fl
        firm[i] = (v - fl > e) and (fl + 1 - v > e)
    return cells, firm


def compact(keys, axis, bits):
    """The cell of `axis` (0 = x, the least significant of each bit triple) out of Morton keys."""
    keys = np.asarray(keys).astype(U64)
    out = np.zeros(len(keys), np.int64)
    for b in range(10 if bits == 30 else 21):
        out |= ((keys >> U64(3 * b + axis)) & U64(1)).astype(np.int64) << b
    return out


def _at_or_above(k, lo, hi, span):
    """The smallest float32 c with span (c - lo) / (hi - lo) >= k, exactly."""
    pre = Fraction(float(lo)) + Fraction(k) * (Fraction(float(hi)) - Fraction(float(lo))) / span
    c = F32(float(pre))
    while scaled_exact(c, lo, hi, span) < k:
        c = np.nextafter(c, F32(np.inf))
    while scaled_exact(np.nextafter(c, F32(-np.inf)), lo, hi, span) >= k:
        c = np.nextafter(c, F32(-np.inf))
    return c


def boundary_points(name, bits):
    """Spheres on the cell boundaries of a box.  For each axis and each k of CELL_KS[bits]: the
    smallest float32 whose exact scaled value is >= k ("at"), its float32 predecessor ("below":
    scaled value < k) and successor ("above"), built with nextafter around the exact pre-image
    bot + k (top - bot) / span; the other two axes sit at a fixed interior point.  A neighbour that
    leaves [bot, top] is left out (k = 0 has no "below", k = span no "above": unspecified inputs).
    Last two records: the corners bot and top on all three axes at once.
    Returns (spheres [m, 4] float32, meta) with meta[i] = (axis, k, "below" | "at" | "above")
    or (-1, 0 | span, "bot" | "top")."""
    lo, hi = box(name, F32)
    span = SPAN[bits]
    inner = (lo.astype(F64) + np.array([0.37, 0.61, 0.43]) * (hi.astype(F64) - lo.astype(F64))).astype(F32)
    pts, meta = [], []
    for axis in range(3):
        for k in CELL_KS[bits]:
            at = _at_or_above(k, lo[axis], hi[axis], span)
            for label, c in (("below", np.nextafter(at, F32(-np.inf))), ("at", at),
                             ("above", np.nextafter(at, F32(np.inf)))):
                if c < lo[axis] or c > hi[axis]:
                    continue
                p = inner.copy()
                p[axis] = c
                pts.append(p)
                meta.append((axis, k, label))
    pts.append(lo.copy()); meta.append((-1, 0, "bot"))
    pts.append(hi.copy()); meta.append((-1, span, "top"))
    s = np.zeros((len(pts), 4), F32)
    s[:, :3] = np.array(pts, F32)
    s[:, 3] = 0.01
    return s, meta


def one_hot_points(bits):
    """Unit-box spheres whose cells are a single set bit on one axis and zero on the others:
    co-ordinate (2^b + 1/2) / span, half a cell inside cell 2^b.  Returns (spheres, expected keys):
    bit b of axis a lands on key bit 3 b + a (x least significant; tests/golden/kat.json)."""
    span = SPAN[bits]
    nb = 10 if bits == 30 else 21
    s = np.zeros((3 * nb, 4), F32)
    keys = np.zeros(3 * nb, U64)
    for a in range(3):
        for b in range(nb):
            s[a * nb + b, a] = F32(((1 << b) + 0.5) / span)
            keys[a * nb + b] = 1 << (3 * b + a)
    s[:, 3] = 0.01
    return s, keys.astype(U32 if bits == 30 else U64)


def planar_scene(n=600, seed=3, z=0.375):
    """Spheres with all centres on the plane z = const: the centroid bounds have top == bot there."""
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :2] = rng.random((n, 2))
    s[:, 2] = z
    s[:, 3] = 0.02 + 0.03 * rng.random(n)
    return s


# ---------------------------------------------------------------------------------------------
# Deltas
# ---------------------------------------------------------------------------------------------
DELTA_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, (1 << 16) + 1)
DELTA_BASE = (1 << 16) + 1
EDGES = (62, 63, 64, 255, 256, 257)     # the wave's last lanes and the block's last threads


def euclid_chain(a, b, fma):
    """The Euclidean delta of float4 a, b: the plain fp32 chain ((dx dx + dy dy) + dz dz), or what a
    compiler contracting it to fma(dz, dz, fma(dy, dy, dx dx)) would give (products exact in
    float64, each sum rounded to float32 once)."""
    d = (a[:, :3] - b[:, :3]).astype(F32)
    if not fma:
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    D = d.astype(F64)
    t = (D[:, 1] * D[:, 1] + (d[:, 0] * d[:, 0]).astype(F64)).astype(F32)
    return (D[:, 2] * D[:, 2] + t.astype(F64)).astype(F32)


def area_chain(a, b, fma):
    """The surface-area delta (Lx Ly + Lx Lz) + Ly Lz, plain or contracted to
    fma(Ly, Lz, fma(Lx, Lz, Lx Ly))."""
    r = a[:, 3:4], b[:, 3:4]
    L = (np.maximum(a[:, :3] + r[0], b[:, :3] + r[1]) - np.minimum(a[:, :3] - r[0], b[:, :3] - r[1])).astype(F32)
    if not fma:
        return (L[:, 0] * L[:, 1] + L[:, 0] * L[:, 2]) + L[:, 1] * L[:, 2]
    D = L.astype(F64)
    t = (D[:, 0] * D[:, 2] + (L[:, 0] * L[:, 1]).astype(F64)).astype(F32)
    return (D[:, 1] * D[:, 2] + t.astype(F64)).astype(F32)


def fma_sensitive_pairs(count=8, seed=11):
    """2 * count pairs (a, b) of float4 spheres: for the first `count` a fused multiply-add changes
    the Euclidean delta, for the rest the area delta.  Found by comparing the two chains above on
    random candidates.  Returns records a0, b0, a1, b1, ... [4 * count, 4]."""
    rng = np.random.default_rng(seed)
    a = rng.random((400, 4)).astype(F32)
    b = rng.random((400, 4)).astype(F32)
    a[:, 3] *= 0.1; b[:, 3] *= 0.1
    e = np.nonzero(euclid_chain(a, b, False) != euclid_chain(a, b, True))[0][:count]
    s = np.nonzero(area_chain(a, b, False) != area_chain(a, b, True))[0][:count]
    assert len(e) == count and len(s) == count
    idx = np.concatenate([e, s])
    out = np.empty((2 * len(idx), 4), F32)
    out[0::2] = a[idx]; out[1::2] = b[idx]
    return out


def delta_specials():
    """Records whose neighbouring pairs are the value cases: (0, 1) coincident; (2, 3) differences
    whose squares and extents' products are subnormal; (4, 5) co-ordinates near 1e19 whose squares
    overflow; then the FMA-sensitive pairs."""
    head = np.array([[0.25, 0.5, 0.75, 0.125], [0.25, 0.5, 0.75, 0.125],
                     [1e-20, 2e-20, 0.0, 1e-21], [2e-20, 0.0, 1e-20, 2e-21],
                     [1e19, -1e19, 0.5, 1.0], [-1e19, 1e19, -0.5, 1.0]], F32)
    return np.concatenate([head, fma_sensitive_pairs()])


def delta_base():
    """DELTA_BASE float4 spheres: the specials, then distinct random records (so that the elements
    at the wave and block edges, EDGES, differ from each other and from their neighbours).
    delta_input(n) is its first n records."""
    sp = delta_specials()
    rng = np.random.default_rng(29)
    s = rng.random((DELTA_BASE, 4)).astype(F32)
    s[:, 3] *= 0.05
    s[:len(sp)] = sp
    assert len(sp) < EDGES[0] - 1
    return s


def delta_base_d4():
    """The same records as double4 with a double-only part added to the random ones: differences
    formed after narrowing to float would differ."""
    s = delta_base().astype(F64)
    n0 = len(delta_specials())
    rng = np.random.default_rng(31)
    s[n0:] += rng.random((DELTA_BASE - n0, 4)) * 1e-9
    return s


def delta_keys(dtype):
    rng = np.random.default_rng(37)
    hi = (1 << 30) if dtype == U32 else (1 << 63)
    k = rng.integers(0, hi, DELTA_BASE, dtype=np.uint64).astype(dtype)
    k[1] = k[0]                                  # equal neighbours: delta 0
    return k


# ---------------------------------------------------------------------------------------------
# HEALPix
# ---------------------------------------------------------------------------------------------
HEALPIX_NSIDES = (1, 2, 4, 8, 64, 512)
HEALPIX_FIXTURES = (1, 2, 8, 16)
HEALPIX_ATOL = 1.2e-7


def healpix_ring_z(nside):
    """The z of every pixel centre by rings, ascending: 4 i pixels on cap ring i = 1 .. nside - 1 at
    |z| = 1 - i^2 / (3 nside^2), 4 nside pixels on each of the 2 nside + 1 belt rings at
    z = 2 (2 nside - r) / (3 nside), r = nside .. 3 nside."""
    i = np.arange(1, nside, dtype=F64)
    cap = np.repeat(1.0 - i * i / (3.0 * nside * nside), 4 * np.arange(1, nside))
    r = np.arange(nside, 3 * nside + 1, dtype=F64)
    belt = np.repeat(2.0 * (2 * nside - r) / (3.0 * nside), 4 * nside)
    z = np.sort(np.concatenate([cap, belt, -cap]))
    assert len(z) == 12 * nside * nside
    return z


def healpix_pixel_radius(nside):
    """The radius of the disc with a pixel's area 4 pi / (12 nside^2): the children's mean direction
    must fall within it of the parent's centre (a HEALPix pixel reaches about twice as far)."""
    return 2.0 * np.arcsin(np.sqrt(1.0 / (12.0 * nside * nside)))


def children_mean_angle(parent_dirs, child_dirs):
    """Angle between pixel p at nside and the normalised mean of pixels 4p .. 4p+3 at 2 nside."""
    m = np.asarray(child_dirs, F64).reshape(-1, 4, 3).mean(axis=1)
    m /= np.linalg.norm(m, axis=1)[:, None]
    p = np.asarray(parent_dirs, F64)
    p = p / np.linalg.norm(p, axis=1)[:, None]
    return 2.0 * np.arcsin(np.minimum(np.linalg.norm(m - p, axis=1) / 2.0, 1.0))


# ---------------------------------------------------------------------------------------------
# Grid generators
# ---------------------------------------------------------------------------------------------
GRID_RES = ((1, 1), (1, 257), (257, 1), (255, 3), (1031, 1033))
ORTHO_Z_SIDES = (1, 3, 255, 257, 1031)
assert 1031 * 1033 > GRID and 1031 * 1031 > GRID
U = 2.0 ** -24
# Cameras: (camera, look_at, view_up) at two scales, oblique to every axis; view_up is at least 45
# degrees off the view direction.  All values are rounded to float32 before use.
CAMERAS = {
    "1e5": ((1.5e5, -2.25e5, 0.75e5), (-0.5e5, 0.5e5, 0.25e5), (0.1, 0.3, 1.0), 1.5e5),
    "1e-3": ((1.5e-3, -2.25e-3, 0.75e-3), (-0.5e-3, 0.5e-3, 0.25e-3), (0.1, 0.3, 1.0), 1.5e-3),
}
# From the inputs to an output component the generators perform: the view difference (1 rounding
# per component), two cross products (3 each), three normalisations (a float norm^2 of 5
# roundings, halved by the square root, and 1 narrowing each), the scaling by the extent (2), the
# image-plane co-ordinate (4) and x v + y u (+ n) + camera (5): under 32 roundings, each of
# relative size u of a quantity no larger than the scene scale.  The cross products with view_up
# lose at most a factor 1 / sin(45 deg) < 2 to cancellation.  Hence 64 u, relative to the scale.
GRID_TOL_ROUNDINGS = 64


def camera(name):
    cam, look, up, extent = CAMERAS[name]
    f = lambda v: np.asarray(v, F32)
    return f(cam), f(look), f(up), float(F32(extent))


def _unit(v):
    return v / np.linalg.norm(v)


def _plane_xy(res_x, res_y):
    t = np.arange(res_x * res_y, dtype=np.int64)
    i, j = t % res_x, t // res_x
    return 2.0 * (i + 0.5) / res_x - 1.0, 1.0 - 2.0 * (j + 0.5) / res_y


def orthographic_f64(res_x, res_y, cam, look, up, vertical_extent):
    """orthographic_projection_rays in float64: (direction [3], origins [n, 3])."""
    cam, look, up = (np.asarray(v, F64) for v in (cam, look, up))
    d = _unit(look - cam)
    v = _unit(np.cross(d, up))
    u = _unit(np.cross(v, d))
    v = v * (vertical_extent * (res_x / res_y) / 2.0)
    u = u * (vertical_extent / 2.0)
    x, y = _plane_xy(res_x, res_y)
    return d, cam + x[:, None] * v + y[:, None] * u


def pinhole_f64(res_x, res_y, cam, look, up, fovy):
    """pinhole_camera_rays in float64: directions [n, 3]."""
    cam, look, up = (np.asarray(v, F64) for v in (cam, look, up))
    vd = look - cam
    v = _unit(np.cross(vd, up))
    u = _unit(np.cross(v, vd))
    n = _unit(vd) / np.tan(fovy / 2.0)
    x, y = _plane_xy(res_x, res_y)
    g = (x * (res_x / res_y))[:, None] * v + y[:, None] * u + n
    return g / np.linalg.norm(g, axis=1)[:, None]


ORTHO_Z_BOXES = {
    "wide_x": ((-2.0, 0.25, 1.0, 0.0), (6.0, 1.25, 3.0, 0.0)),
    "wide_y": ((0.5, -40.0, -1.0, 0.0), (1.5, 24.0, 5.0, 0.0)),
    "radius": ((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 0.125)),
}


def orthogonal_z_f64(n_side, mins4, maxs4):
    """orthogonal_rays_z in float64: (origins [n, 3], length, area per ray)."""
    lo, hi = np.asarray(mins4, F32).astype(F64), np.asarray(maxs4, F32).astype(F64)
    span = hi[:3] - lo[:3] + 2.0 * hi[3]
    side = max(span[0], span[1])
    x, y = _plane_xy(n_side, n_side)
    o = np.empty((n_side * n_side, 3), F64)
    o[:, 0] = (lo[0] + hi[0]) / 2.0 + x * side / 2.0
    o[:, 1] = (lo[1] + hi[1]) / 2.0 + y * side / 2.0
    o[:, 2] = span[2]
    return o, 2.0 * span[2], (side / n_side) ** 2


# ---------------------------------------------------------------------------------------------
# Random generators: the map (seed, index) -> ray
# ---------------------------------------------------------------------------------------------
ISO_SEEDS = (1234, 11, 9, 0)
ISO_OCTANTS = (7, 5, 2, 0)
ISO_N = 4096
ISO_SIZES = (1, 2, 255, 256, 257, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, GRID + 257)
TWO_PI_F = F32(6.283185307179586)


def splitmix64(x):
    x = np.asarray(x, U64)
    with np.errstate(over="ignore"):
        x = x + U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
    return x ^ (x >> U64(31))


def u01(bits32, real=F64):
    """(0, 1]: (float(bits >> 8) + 1) / 2^24, exact in float32."""
    return ((np.asarray(bits32, U64) >> U64(8)).astype(real) + real(1)) * real(1.0 / 16777216.0)


def _lo_hi(a):
    return a & U64(0xFFFFFFFF), a >> U64(32)


def isotropic_dirs(seed, n, octant=-1, real=F64):
    """Ray t of the isotropic generators, before the sort: a = splitmix64(seed ^ splitmix64(2 t)),
    b = splitmix64(seed ^ splitmix64(2 t + 1)); radii sqrt(-2 log u01(low word)), angles
    2 pi u01(high word) (2 pi the float32 constant); (r_a cos t_a, r_a sin t_a, r_b cos t_b); the
    octant's signs on the absolute values (bit 2 = x, 1 = y, 0 = z, set = positive); normalised.
    real = float64: the map itself; float32: the same chain in NumPy's float32."""
    t = np.arange(n, dtype=U64)
    a = splitmix64(U64(seed) ^ splitmix64(U64(2) * t))
    b = splitmix64(U64(seed) ^ splitmix64(U64(2) * t + U64(1)))
    (alo, ahi), (blo, bhi) = _lo_hi(a), _lo_hi(b)
    r1 = np.sqrt(real(-2.0) * np.log(u01(alo, real)))
    r2 = np.sqrt(real(-2.0) * np.log(u01(blo, real)))
    t1 = real(TWO_PI_F) * u01(ahi, real)
    t2 = real(TWO_PI_F) * u01(bhi, real)
    g = np.stack([r1 * np.cos(t1), r1 * np.sin(t1), r2 * np.cos(t2)], axis=1)
    assert g.dtype == real
    if octant >= 0:
        sign = np.array([1 if octant & 4 else -1, 1 if octant & 2 else -1, 1 if octant & 1 else -1], real)
        g = np.abs(g) * sign
    n2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
    return g * (real(1.0) / np.sqrt(n2))[:, None]


def isotropic_tolerance(seed, octant=-1):
    """T for one seed: 4 x the largest componentwise deviation of the float32 NumPy chain from the
    float64 one at ISO_N rays.  The factor covers a device logf / cosf / sinf that is allowed an ulp
    more than NumPy's.  Returns (T, deviation).  Measured deviations: 1.2e-6 (seed 1234), 1.2e-6 (11),
    1.1e-6 (9), 2.5e-6 (0), whole sphere and octants alike; a few rays with a small first radius and a
    second angle near a zero of the cosine carry them.  Per seed, because the closest pair of
    directions (7.4e-5 rad, seed 9 folded into an octant) and the largest deviation (seed 0) belong
    to different seeds: T stays under a tenth of the seed's own smallest separation everywhere."""
    dev = float(np.abs(isotropic_dirs(seed, ISO_N, octant, F32).astype(F64)
                       - isotropic_dirs(seed, ISO_N, octant, F64)).max())
    return 4.0 * dev, dev


def row_hashes(rays):
    """One uint64 per row of float32 words (28-byte ray records, or their 3 directions): equal rows give
    equal hashes; distinct rows collide with probability ~ n^2 / 2^64."""
    rays = np.ascontiguousarray(rays, F32)
    w = rays.view(U32).reshape(len(rays), -1).astype(U64)
    mult = splitmix64(np.arange(1, w.shape[1] + 1, dtype=U64)) | U64(1)
    with np.errstate(over="ignore"):
        return splitmix64((w * mult).sum(axis=1, dtype=U64))


PLANE_RES = ((1, 1), (1, 257), (257, 1), (1031, 1033))
# An oblique plane whose cross product is exact in float32 (small dyadic components), so that the
# direction is normalize(cross(w, h)) rounded once: (-15, 9, -21) / sqrt(747).
PLANE = dict(base=(0.5, -1.25, 2.0), w=(4.0, 2.0, -2.0), h=(-1.5, 4.5, 3.0))
# Float operations from the inputs to an origin component: w / W (1), i dw and (i + 1) dw (1 each),
# their difference (1), r times it (1), plus i dw (1): 6 roundings of quantities <= |w|; the same
# for h; two additions to the base.  Under 16 roundings, relative to |base| + |w| + |h|.
PLANE_TOL_ROUNDINGS = 16


def plane_parallel_f64(width, height, base, w, h, seed):
    """plane_parallel_random_rays in float64: base + (i + rw) w / W + (j + rh) h / H with
    (rw, rh) = u01 of the (low, high) word of splitmix64(seed ^ splitmix64(t)), t = j W + i."""
    base, w, h = (np.asarray(v, F32).astype(F64) for v in (base, w, h))
    t = np.arange(width * height, dtype=U64)
    lo, hi = _lo_hi(splitmix64(U64(seed) ^ splitmix64(t)))
    i, j = (t % U64(width)).astype(F64), (t // U64(width)).astype(F64)
    o = base + ((i + u01(lo))[:, None] * w / width) + ((j + u01(hi))[:, None] * h / height)
    return o, _unit(np.cross(w, h))


# ---------------------------------------------------------------------------------------------
# one_to_many_rays
# ---------------------------------------------------------------------------------------------
POINT_LAYOUTS = ((F32, 3), (F32, 4), (F64, 3), (F64, 4), (F32, 7), (F64, 7), (F32, 16))
OTM_LAYOUTS = ((F32, 3), (F32, 4), (F64, 3), (F64, 4), (F32, 7))
OTM_ORIGIN = (0.25, -0.5, 1.0)
OTM_SIZES = tuple(sorted(set(SIZES + ISO_SIZES)))    # block and grid edges, and the nested sort's switch


def otm_pool(dtype, cols, seed=5):
    """POOL end points in (-2, 3)^3.  Records 0..63 of a double pool sit at origin + 1e-7 u, |u| = 1:
    the float nearest such a point is the origin's neighbour, so a kernel that narrowed the point
    before subtracting the origin would turn all of them into a handful of directions.  Records
    64..127 are 8 groups of 8 points within one 30-bit Morton cell of the box (-2, 3)^3: the
    end-point sort's stability decides their order."""
    rng = np.random.default_rng(seed)
    p = np.empty((POOL, cols), F64)
    p[:, :3] = rng.uniform(-2, 3, (POOL, 3))
    p[:, 3:] = 1e6 + rng.random((POOL, cols - 3))
    if dtype == F64:
        u = rng.standard_normal((64, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        p[:64, :3] = np.asarray(OTM_ORIGIN, F32).astype(F64) + 1e-7 * u
    cell = 5.0 / 1023
    centres = -2.0 + (rng.integers(100, 900, (8, 3)) + 0.5) * cell
    p[64:128, :3] = np.repeat(centres, 8, axis=0) + rng.uniform(-0.2, 0.2, (64, 3)) * cell
    return np.ascontiguousarray(p.astype(dtype))


OTM_BOX = (np.full(3, -2.0, F32), np.full(3, 3.0, F32))
