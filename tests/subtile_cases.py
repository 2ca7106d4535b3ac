"""Scenes, ray batches and a NumPy restatement of the sub-tile packet plan's streams
(PLAN_FORMAT_SUBTILE, csrc/trace_state.hpp; the recorder is plan_record_kernel<true, true>,
csrc/trace_planned.hip), for tests/test_trace_subtiles.py.

The restatement covers batches that are power-of-two pixel grids along one axis (8 x 16, 64 x 64,
256 x 256 rays ...): those get Z-order keys (ray_lattice_kernel / ray_keys_kernel,
csrc/trace_coherence.hip), sorted down to the two bits below the packet's, so that packet p is the
8 x 8 tile (iu >> 3, iv >> 3) of the grid and lanes 16 q .. 16 q + 15 are one of its 4 x 4
quadrants, ((iu >> 2) & 1, (iv >> 2) & 1).  Which quadrant gets which q does not matter: a list's
steps are its longest stream, its slots the sum of the four.

A sphere survives for a packet if the packet-level bound keeps it -- fl32 fma(q1, q1, q2 q2) of
the distances to the packet's origin rectangle, NOT >= fl32(h h) -- and the origin-lattice cull,
which runs over a whole cluster of 64 consecutive spheres once one kept member is smaller than the
lattice's cell diagonal, does not drop it; it joins quadrant q's stream if the same bound against
q's rectangle keeps it.  The box culls ahead of the bound (groups, clusters) are supersets of it
for rays that cross the whole scene, which is all this restatement is used for.
Classes: 1024 consecutive spheres share one, eight classes in rotation."""
import numpy as np

F32 = np.float32
BOX = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
PIXEL = F32(0.1 / 8)
CORNER = F32(0.4)
ROUND_STEPS = 16        # PLAN_SUB_ROUND_STEPS
LOOP_MAX = 128          # PLAN_LOOP_MAX, in slots


def perp(axis):
    """The two perpendicular co-ordinates of an axis, in the kernel's order (s1, s2)."""
    return {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]


def pixel(k):
    """Perpendicular co-ordinate of pixel k of the hand-made patches (float32, as the rays hold it)."""
    return F32(CORNER + (F32(k) + F32(0.5)) * PIXEL)


def patch_rays(axis=2, sense=1, nu=8, nv=16, length=2.0, keep=None, jitter=None):
    """nu x nv rays on the pixels of the hand-made patch (8 x 16: two packets side by side), from
    outside the box; keep: only the first `keep` rays; jitter: a Generator that moves every origin
    by up to 0.3 pixel."""
    u = np.array([pixel(k) for k in range(nu)], F32)
    v = np.array([pixel(k) for k in range(nv)], F32)
    a, b = [t.ravel() for t in np.meshgrid(u, v, indexing="ij")]
    if jitter is not None:
        a = (a + F32(0.3) * PIXEL * (jitter.random(len(a), dtype=F32) * F32(2) - F32(1))).astype(F32)
        b = (b + F32(0.3) * PIXEL * (jitter.random(len(b), dtype=F32) * F32(2) - F32(1))).astype(F32)
    r = np.zeros((len(a), 7), F32)
    p1, p2 = perp(axis)
    r[:, 3 + p1], r[:, 3 + p2] = a, b
    r[:, 3 + axis] = -0.5 if sense > 0 else 1.5
    r[:, axis] = sense
    r[:, 6] = length
    return r[:keep] if keep is not None else r


def grid_rays(side, depth=-0.1, length=1.3, axis=2):
    """side^2 rays along +axis over the unit square."""
    u = (np.arange(side, dtype=F32) + F32(0.5)) / F32(side)
    a, b = [t.ravel() for t in np.meshgrid(u, u, indexing="ij")]
    r = np.zeros((side * side, 7), F32)
    p1, p2 = perp(axis)
    r[:, axis] = 1.0
    r[:, 3 + p1], r[:, 3 + p2], r[:, 3 + axis], r[:, 6] = a, b, depth, length
    return r


def spheres_at(placed, axis=2, n_fill=40, seed=5, fill_h=0.02):
    """Spheres placed by hand, [(u, v, h)] in the perpendicular co-ordinates, spread along the axis
    in the order given, with n_fill small spheres near the box's low corner, under no ray (a tree
    wants more primitives than a leaf holds)."""
    rng = np.random.default_rng(seed)
    s = np.empty((n_fill + len(placed), 4), F32)
    s[:n_fill, :3] = F32(0.01) + F32(0.04) * rng.random((n_fill, 3), dtype=F32)
    s[:n_fill, 3] = fill_h
    p1, p2 = perp(axis)
    for k, (u, v, h) in enumerate(placed):
        row = s[n_fill + k]
        row[p1], row[p2], row[3] = u, v, h
        row[axis] = F32(0.1) + F32(0.8) * F32(k + 0.5) / F32(len(placed))
    return s


def fma32(a, b, c):
    """fl32(a b + c) for float32 arrays (the product is exact in double)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _bound_keeps(s1, s2, h2, lo1, hi1, lo2, hi2):
    with np.errstate(invalid="ignore"):
        q1 = (s1 - np.clip(s1, lo1, hi1)).astype(F32)
        q2 = (s2 - np.clip(s2, lo2, hi2)).astype(F32)
        return ~(fma32(q1, q1, (q2 * q2).astype(F32)) >= h2)


def grid_cells(rays, axis):
    """(packet id, quadrant id) of every ray of a power-of-two pixel grid."""
    p1, p2 = perp(axis)
    iu = np.unique(rays[:, 3 + p1], return_inverse=True)[1]
    iv = np.unique(rays[:, 3 + p2], return_inverse=True)[1]
    n_v = int(iv.max()) + 1
    packet = (iu >> 3) * ((n_v + 7) >> 3) + (iv >> 3)
    quadrant = ((iu >> 2) & 1) * 2 + ((iv >> 2) & 1)
    assert np.all(np.bincount(packet) == 64), "not a grid of whole 8 x 8 tiles"
    return packet, quadrant


def streams(spheres, rays, axis=2):
    """The recorder's streams over the SORTED spheres for a power-of-two pixel grid of rays that
    cross the scene: {"lens": [packet][class][quadrant] stream lengths, "survivors": packet-level
    survivors, "steps", "slots"}."""
    p1, p2 = perp(axis)
    s1, s2 = spheres[:, p1].astype(F32), spheres[:, p2].astype(F32)
    h2 = (spheres[:, 3] * spheres[:, 3]).astype(F32)
    cls = (np.arange(len(spheres)) >> 10) & 7
    cluster = np.arange(len(spheres)) >> 6
    packet, quadrant = grid_cells(rays, axis)
    n_packets = int(packet.max()) + 1
    lens = np.zeros((n_packets, 8, 4), np.int64)
    survivors = 0
    for p in range(n_packets):
        mine = packet == p
        o1, o2 = rays[mine, 3 + p1], rays[mine, 3 + p2]
        keep = _bound_keeps(s1, s2, h2, o1.min(), o1.max(), o2.min(), o2.max())
        # the origin-lattice cull: the packet's (at most 8) distinct origins per co-ordinate
        l1, l2 = np.unique(o1), np.unique(o2)
        gap1 = F32(l1[-1] - l1[0]) / F32(len(l1) - 1)
        gap2 = F32(l2[-1] - l2[0]) / F32(len(l2) - 1)
        cell2 = F32(F32(gap1 * gap1) + F32(gap2 * gap2))
        small = keep & (h2 < cell2)
        if small.any():
            run = np.isin(cluster, np.unique(cluster[small]))
            with np.errstate(invalid="ignore"):
                d1 = np.abs(s1[:, None] - l1[None, :]).astype(F32).min(axis=1)
                d2 = np.abs(s2[:, None] - l2[None, :]).astype(F32).min(axis=1)
                nan_if_nan = ((s1 + s2).astype(F32) * F32(0.0)).astype(F32)
                lat = (fma32(d1, d1, (d2 * d2).astype(F32)) + nan_if_nan).astype(F32)
                keep &= ~(run & (lat >= h2))
        survivors += int(keep.sum())
        for q in range(4):
            sub = mine & (quadrant == q)
            oq1, oq2 = rays[sub, 3 + p1], rays[sub, 3 + p2]
            keep_q = keep & _bound_keeps(s1, s2, h2, oq1.min(), oq1.max(), oq2.min(), oq2.max())
            lens[p, :, q] = np.bincount(cls[keep_q], minlength=8)
    return {"lens": lens, "survivors": survivors,
            "steps": int(lens.max(axis=2).sum()), "slots": int(lens.sum())}


def round_headers(steps):
    """The slot counts of a list of `steps` steps: rounds of ROUND_STEPS steps, the last what is left."""
    out = []
    while steps > 0:
        out.append(4 * min(steps, ROUND_STEPS))
        steps -= ROUND_STEPS
    return out


def expected_loops(lens, bits=None):
    """(loops, largest loop in slots) of the fused consumer over lists of equal bits: consecutive
    rounds join while the loop stays within LOOP_MAX slots (planned_fuses)."""
    loops = []
    for steps in lens.max(axis=2).ravel():
        open_n = 0
        for n in round_headers(int(steps)):
            if open_n and open_n + n <= LOOP_MAX:
                open_n += n
            else:
                if open_n:
                    loops.append(open_n)
                open_n = n
        if open_n:
            loops.append(open_n)
    return (len(loops), max(loops)) if loops else (0, 0)


# ---- the hand-made cases: spheres placed over packet 0 of the 8 x 16 patch ----------------------------
# (h = 0.02: wider than the lattice's cell diagonal 0.0177, so the lattice cull never runs; narrower
# than the 0.0375 between pixel 1 and pixel 4, so a sphere over pixel 1 or 6 stays in its quadrant)
H = F32(0.02)


def case_one_quadrant():
    return [(pixel(1), pixel(1), H)]


def case_on_the_seam():
    """Between pixel columns 3 and 4 in u, over pixel 1 in v: both u-quadrants of the lower v half."""
    return [(F32((pixel(3) + pixel(4)) * F32(0.5)), pixel(1), H)]


def case_at_distance_h(ulps=0):
    """Right of the patch in u, level with pixel 5 in v (q2 = 0 exactly): the distance to the
    nearest quadrant's rectangle, fl32(s1 - pixel 7), IS h (ulps = 0: b^2 = fl32(h h), and the
    negated b^2 >= h^2 drops it, as the rays' own hit test does) or one ulp less than h (kept)."""
    s1 = F32(pixel(7) + F32(0.03))
    h = F32(s1 - pixel(7))
    for _ in range(ulps):
        h = np.nextafter(h, F32(1.0))
    return [(s1, pixel(5), h)]


def case_unequal(lens=(0, 1, 33, 130)):
    """lens[q] spheres over quadrant q alone, q = (u half) * 2 + (v half), interleaved along the axis."""
    centre = {0: (pixel(1), pixel(1)), 1: (pixel(1), pixel(6)), 2: (pixel(6), pixel(1)), 3: (pixel(6), pixel(6))}
    placed = []
    for k in range(max(lens)):
        for q in range(4):
            if k < lens[q]:
                placed.append(centre[q] + (H,))
    return placed
