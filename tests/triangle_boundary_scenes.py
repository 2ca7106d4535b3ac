"""Boundary scenes for the closest-hit triangle trace: exact ties in t, triangles one float inside or
outside Moeller-Trumbore's accept tests for one ray, rays one float longer or shorter than the hit
they reach, hits at t = 0, edge-on and back faces, and meshes that are closed, self-overlapping,
stacked, repeated, needle-thin or partly invalid.

A plain helper module (numpy and the CPU oracle; no GPU, no torch): tests/test_triangle_boundaries.py
traces its scenes, tests/test_triangle_boundary_scenes.py checks on the CPU, with the oracle alone,
that every designed case sits where it is said to sit.

Every scene is a Scene with tris [n, 9] float32 {v, e1, e2} in the caller's (shuffled) order and
rays [R, 7] float32.  The index arrays of the designed cases name triangles of `tris`; the GPU
tests, which trace the array as the build sorted it, compare whole rays with brute force and need
only `designed`, the rays the cases were placed against.

Twins.  An EDGE twin pair differs by one float in one co-ordinate of the vertex v: the target ray's
u (sorts "u0", "u1"), v ("v0") or u + v ("uv1") is on the accepting side of 0 or 1 for one twin and
on the rejecting side for the other, found by walking the co-ordinate float by float until the
oracle's tri_intersect flips.  A LENGTH twin is two copies of one ray (the target and its neighbour
in the packet): the shortest length for which the hit at t still passes t <= length (1 + 1e-6), and
the float below it.

Placement follows trace_boundary_scenes.py: targets are the rays that bound a packet of 16, 32 or
64 consecutive rays, the triangle's bulk lies outward of the packet, and each designed triangle is
nearer along its target ray than any background triangle.
"""
import numpy as np

import trace_boundary_scenes as S

F32, F64 = np.float32, np.float64
T_EPS = F32(1e-14)                  # TRIANGLE_EPSILON: det and t are accepted from here on
LEN_FACTOR = F32(1.0) + F32(0.000001)   # RayEntry_tri: t_min = length * (1 + 1e-6), in float


class Scene:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _oracle():
    import oracle as O
    return O


def accepts(rays, tris):
    """The oracle's accept flag of (ray, triangle) pairs as the closest-hit loop applies it (the
    length aside): tri_intersect and t >= 1e-14.  Also returns (det, u, v, t)."""
    hit, det, u, v, t = _oracle().tri_intersect_pairs(rays, tris)
    return hit & (t >= T_EPS), det, u, v, t


# ---- exact ties ---------------------------------------------------------------------------------
TIE_SCALES = {"unit": (0.0, 1.0), "off1024": (1024.0, 1.0), "2^-10": (0.0, 2.0 ** -10)}
_PERM = {2: (0, 1, 2), 0: (1, 2, 0), 1: (2, 0, 1)}      # (p, q, a) with e_p x e_q = e_a


def _flat_sheet(cells, off, s, axis, facing):
    """2 cells^2 triangles over [off, off + s]^2 in the plane x_axis = s / 4, normal facing * e_axis."""
    p, q, a = _PERM[axis]
    k = np.arange(cells + 1) / cells
    P, Q = np.meshgrid(k, k)
    V = np.zeros((cells + 1, cells + 1, 3))
    V[..., p] = off + P * s; V[..., q] = off + Q * s; V[..., a] = 0.25 * s
    v00 = V[:-1, :-1]; v10 = V[:-1, 1:]; v01 = V[1:, :-1]; v11 = V[1:, 1:]
    t1 = np.concatenate([v00, v10 - v00, v01 - v00], -1).reshape(-1, 9)
    t2 = np.concatenate([v11, v01 - v11, v10 - v11], -1).reshape(-1, 9)
    tris = np.concatenate([t1, t2])
    if facing < 0:
        tris = tris[:, [0, 1, 2, 6, 7, 8, 3, 4, 5]]
    out = tris.astype(F32)
    assert np.array_equal(out.astype(F64), tris), "the tie mesh must be exact in float"
    return out


def tie_scene(scale="unit", coplanar=False, axis=2, sense=-1, cells=32, seed=0):
    """A flat mesh of cells x cells cells on power-of-two co-ordinates in the plane x_axis = s / 4,
    shuffled, and (2 cells + 1)^2 rays along sense * e_axis through every vertex, edge midpoint and
    cell diagonal: every ray hits at t = 0.75 s exactly, and all but the midpoints of the outer
    edges and two corners tie between two or more triangles.  coplanar: a second, 4 x 4 sheet in
    the same plane (then every ray ties, between triangles far apart in index)."""
    off, s = TIE_SCALES[scale]
    rng = np.random.default_rng(1000 + seed)
    tris = _flat_sheet(cells, off, s, axis, -sense)
    if coplanar:
        tris = np.concatenate([tris, _flat_sheet(4, off, s, axis, -sense)])
    tris = np.ascontiguousarray(tris[rng.permutation(len(tris))])
    p, q, a = _PERM[axis]
    m = 2 * cells + 1
    kp, kq = np.meshgrid(np.arange(m), np.arange(m))
    kp, kq = kp.ravel(), kq.ravel()
    rays = np.zeros((m * m, 7), F32)
    rays[:, a] = sense
    rays[:, 3 + p] = off + kp / (2 * cells) * s
    rays[:, 3 + q] = off + kq / (2 * cells) * s
    rays[:, 3 + a] = 0.25 * s - sense * 0.75 * s
    rays[:, 6] = 2 * s
    edge_p, edge_q = (kp == 0) | (kp == m - 1), (kq == 0) | (kq == m - 1)
    lone = (edge_q & (kp % 2 == 1)) | (edge_p & (kq % 2 == 1))                  # outer edge midpoints
    lone |= ((kp == 0) & (kq == 0)) | ((kp == m - 1) & (kq == m - 1))          # corners of one triangle
    tie = np.ones(m * m, bool) if coplanar else ~lone
    return Scene(tris=tris, rays=rays, designed=np.arange(m * m), tie=tie, t=F32(0.75 * s), kind="tie")


def brute_descending(rays, tris):
    """Brute force with the triangles presented in descending index: among exact ties the SMALLEST
    index wins (the oracle's loop, like the traversal, lets the last candidate win a tie)."""
    ref, t = _oracle().brute_closest_tri(rays, np.ascontiguousarray(tris[::-1]))
    return np.where(ref >= 0, len(tris) - 1 - ref, -1).astype(np.int32), t


# ---- edge, length, near-end and face cases ------------------------------------------------------
# Local shapes: (x, y) of A = v, B = v + e1, C = v + e2 in units of the triangle's size; the target
# ray passes through (0, 0), x points outward of the packet, y along the packet's boundary.
_SHAPES = {
    "u0": ((0, -.3), (1, .1), (0, .7)),        # u = 0, v = 0.3: on the edge A C
    "v0": ((0, -.3), (0, .7), (1, .1)),        # u = 0.3, v = 0: on the edge A B
    "uv1": ((1, .1), (0, .6), (0, -.4)),       # u = 0.4, v = 0.6: on the edge B C
    "u1": ((1, -.5), (0, 0), (1, .5)),         # u = 1, v = 0: through the corner B
    "in": ((-.3, -.3), (.7, -.3), (-.3, .7)),  # u = v = 0.3: inside
    "vtx": ((0, 0), (1, -.4), (1, .6)),        # u = v = 0: through the corner A
}
EDGE_SORTS = ("u0", "v0", "uv1", "u1")
TWIN_SORTS = EDGE_SORTS + ("len",)
# (sort, number of target rays): twins first -- the first targets drawn are the sharpest
_PLAN = (("u0", 34), ("v0", 34), ("uv1", 34), ("u1", 34), ("len", 34), ("near0", 8), ("nearf", 10),
         ("nearb", 8), ("edgeon", 12), ("back", 12))

# scale name -> (trace_boundary_scenes scale, background edge lengths relative to the box, exact sums)
TWIN_SCALES = {
    "unit": ("unit", (0.02, 0.08), False),
    "1e3": ("1e3", (0.02, 0.08), True),
    "1e3r": ("1e3", (0.02, 0.08), False),
    "1e5": ("1e5", (0.05 / 64, 0.5 / 64), True),
    "1e5r": ("1e5", (0.05 / 64, 0.5 / 64), False),
    "1e-3": ("1e-3", (0.02, 0.08), False),
}


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _from_vertices(A, B, C, exact):
    """{v, e1, e2} in float from double vertices.  exact: the edges are differences of the FLOAT
    vertices (formed in float: exact where the vertices share a binade, so that v + e1 and v + e2
    are representable); otherwise the double edges rounded (v + e1 is then ragged)."""
    a = A.astype(F32)
    if exact:
        e1 = B.astype(F32) - a; e2 = C.astype(F32) - a
    else:
        e1 = (B - A).astype(F32); e2 = (C - A).astype(F32)
    return np.concatenate([a, e1, e2], -1).astype(F32)


def _random_mesh(n, lo, size, edges, rng, exact):
    c = lo + rng.random((n, 3)) * size
    l1 = rng.uniform(edges[0], edges[1], (n, 1)) * size
    l2 = rng.uniform(edges[0], edges[1], (n, 1)) * size
    e1 = _unit(rng.normal(size=(n, 3))) * l1
    e2 = _unit(rng.normal(size=(n, 3))) * l2
    A = c - (e1 + e2) / 3
    return _from_vertices(A, A + e1, A + e2, exact)


def _shape_tri(shape, p, d, u_out, ell, tilt, exact, back=False):
    """One triangle of `shape` whose local origin is the point p of a ray of direction d; front
    facing for that ray unless back."""
    (ax, ay), (bx, by), (cx, cy) = _SHAPES[shape]
    s2 = np.sign((bx - ax) * (cy - ay) - (by - ay) * (cx - ax))
    sigma = s2 if back else -s2                  # (X x Y) . d = sigma; front: normal . d < 0
    a = _unit(np.cross(d, u_out))
    X = u_out + tilt[0] * d
    Y = sigma * a + tilt[1] * d
    P = lambda x, y: p + ell * (x * X + y * Y)
    return _from_vertices(P(ax, ay), P(bx, by), P(cx, cy), exact)


def _walk_component(tri, d, sort):
    """The vertex co-ordinate the walked quantity is most sensitive to."""
    e1, e2 = tri[3:6].astype(F64), tri[6:9].astype(F64)
    g = {"u0": np.cross(d, e2), "u1": np.cross(d, e2), "v0": np.cross(e1, d),
         "uv1": np.cross(d, e2) + np.cross(e1, d)}[sort]
    return int(np.argmax(np.abs(g)))


def _rejected_as(sort, u, v):
    """The rejecting twin fails the test its sort names (values of the oracle, NaN = not reached)."""
    with np.errstate(invalid="ignore"):
        return {"u0": u < 0, "u1": u > 1, "v0": v < 0,
                "uv1": (u >= 0) & (u <= 1) & (v >= 0) & ((u + v).astype(F32) > 1)}[sort]


def edge_twins(rays, tris, comps, sorts, steps=96):
    """Walks tris[i, comps[i]] float by float, up and down, until the oracle's accept flag of
    (rays[i], tris[i]) flips.  Returns (accepting twins, rejecting twins, found): adjacent floats in
    that one co-ordinate, the rejecting twin failing the test of its sort."""
    m = len(tris)
    idx = np.arange(m)
    acc_t = tris.copy(); rej_t = tris.copy(); found = np.zeros(m, bool)
    a0 = accepts(rays, tris)[0]
    for toward in (F32(np.inf), F32(-np.inf)):
        cur = tris.copy(); prev = a0.copy()
        for _ in range(steps):
            if found.all():
                break
            nxt = cur.copy()
            nxt[idx, comps] = np.nextafter(cur[idx, comps], toward)
            acc, _, u, v, _ = accepts(rays, nxt)
            flip = (acc != prev) & ~found
            for i in np.nonzero(flip)[0]:
                a_t, r_t = (nxt[i], cur[i]) if acc[i] else (cur[i], nxt[i])
                acc_t[i] = a_t; rej_t[i] = r_t
            found |= flip
            cur = nxt; prev = acc
    _, _, u, v, _ = accepts(rays, rej_t)
    for i in range(m):
        found[i] &= bool(_rejected_as(sorts[i], u[i:i + 1], v[i:i + 1])[0])
    return acc_t, rej_t, found


def length_twins(t):
    """(L_hit, L_miss): the shortest float length with t <= length * (1 + 1e-6) (float product, as
    RayEntry_tri forms it) and the float below it."""
    t = np.asarray(t, F32)
    L = t.copy()
    for _ in range(64):
        below = np.nextafter(L, F32(0))
        ok = t <= below * LEN_FACTOR
        if not ok.any():
            break
        L = np.where(ok, below, L)
    assert np.all(t <= L * LEN_FACTOR) and not np.any(t <= np.nextafter(L, F32(0)) * LEN_FACTOR)
    return L, np.nextafter(L, F32(0))


def _twin_rays(kind, scale, seed, rng):
    base, _, _ = TWIN_SCALES[scale]
    lo, size, _ = S.SCALES[base]
    if kind == "axis":
        axis, sense = seed % 3, (1 if (seed // 3) % 2 == 0 else -1)
        rays, sp = S.axis_rays(64, axis, sense, lo, size, rng, neg_zero=bool(seed % 2), ragged=bool((seed // 2) % 2))
        return rays, "axis", sp
    if kind in ("pinhole", "iso"):
        return S.pencil_rays(kind, 64, lo, size, rng), "pencil", None
    return S.general_rays(64, lo, size, rng), "general", None


def _targets(rays, klass, sp, rng):
    """{ray: (outward unit vector, spacing scale)} over the packet-bounding rays at widths 64, 32, 16."""
    out = {}
    for w in (64, 32, 16):
        for r, u, sc in S.extreme_placements(rays, klass, w, rng, sp):
            out.setdefault(int(r), (np.asarray(u, F64), float(sc)))
    return out


def edge_twin_scene(kind, scale, seed=0, n_background=8000):
    """Edge twins, length twins, near-end cases and face cases against the packet-bounding rays of
    an "axis", "pinhole", "iso" or "general" batch, in front of a random background mesh.

    Index arrays (triangles of `tris`, rays of `rays`):
      win_tri / win_ray / win_sort    the triangle is the closest hit of the ray
      lose_tri / lose_ray / lose_sort the triangle is NOT the closest hit of the ray
      pair_win / pair_lose            for the twin sorts: positions in win_* / lose_* of the two twins
    sorts: "u0", "v0", "uv1", "u1" (edge twins), "len" (length twins: one triangle, two rays),
    "near0" (a vertex on the ray's origin: t = 0), "nearf" / "nearb" (a plane just in front of / just
    behind the origin), "edgeon" (det = 0) and "back" (each nearer than a front face that wins)."""
    O = _oracle()
    rng = np.random.default_rng(7919 * seed + 31 * sum(map(ord, kind + scale)))
    base, edges, exact = TWIN_SCALES[scale]
    lo, size, _ = S.SCALES[base]
    rays, klass, sp = _twin_rays(kind, scale, seed, rng)
    rays = rays.copy()
    pencil = klass == "pencil"
    bg = _random_mesh(n_background, lo, size, edges, rng, exact)
    _, t_bg = O.brute_closest_tri(rays, bg)           # (a miss leaves length * (1 + 1e-6))
    t_free = np.minimum(t_bg.astype(F64), rays[:, 6].astype(F64))
    targets = _targets(rays, klass, sp, rng)
    order = list(targets)
    rng.shuffle(order)
    ulp = float(np.spacing(F32(np.abs(rays[:, 3:6]).max() + size)))
    taken = set()
    tris_new = []                                      # designed triangles, appended behind bg
    win, lose, pairs = [], [], []                      # (tri, ray, sort); (win position, lose position)
    edge_jobs = []

    def next_target(need_partner=False):
        while order:
            r = order.pop()
            if r in taken or (need_partner and ((r ^ 1) in taken or (r ^ 1) >= len(rays))):
                continue
            taken.add(r)
            if need_partner:
                taken.add(r ^ 1)
            return r
        return None

    def add(tri):
        tris_new.append(tri)
        return n_background + len(tris_new) - 1

    def geometry(r, near=None):
        u_out, sc = targets[r]
        d = rays[r, :3].astype(F64); o = rays[r, 3:6].astype(F64)
        u_out = _unit(u_out - (u_out @ d) * d)
        t0 = rng.uniform(0.3, 0.6) * t_free[r] if near is None else near
        if pencil and near:
            # a triangle this near the one origin must stay as narrow as the rays are apart there, or
            # it hides the other cases: move it out until that width is 32 floats of the co-ordinates
            t0 = np.sign(near) * min(max(abs(near), 32 * ulp / sc), 0.25 * t_free[r])
        ell = rng.uniform(0.8, 2.0) * sc * (abs(t0) if pencil and t0 else 1.0 if not pencil else 0.02 * t_free[r])
        ell = min(max(ell, 24 * ulp), 0.05 * size)
        return d, o, u_out, t0, ell, rng.uniform(-0.7, 0.7, 2)

    for sort, count in _PLAN:
        for _ in range(count):
            r = next_target(need_partner=(sort == "len"))
            if r is None:
                break
            if sort in EDGE_SORTS:
                # (through a corner the walk must leave by u > 1 before v < 0 or u + v > 1 do: a matter
                # of the last bits, so several shapes are tried and the first that does is kept)
                for _ in range(16 if sort == "u1" else 1):
                    d, o, u_out, t0, ell, tilt = geometry(r)
                    tri = _shape_tri(sort, o + t0 * d, d, u_out, ell, tilt, exact)
                    edge_jobs.append((r, sort, tri, _walk_component(tri, d, sort)))
            elif sort == "len":
                d, o, u_out, t0, ell, tilt = geometry(r)
                tri = _shape_tri("in", o + t0 * d, d, u_out, ell, tilt, exact)
                ok, _, _, _, t = accepts(rays[r:r + 1], tri[None])
                if not ok[0]:
                    continue
                L_hit, L_miss = length_twins(t)
                rays[r ^ 1] = rays[r]
                rays[r, 6] = L_hit[0]; rays[r ^ 1, 6] = L_miss[0]
                k = add(tri)
                pairs.append((len(win), len(lose)))
                win.append((k, r, sort)); lose.append((k, r ^ 1, sort))
            elif sort == "near0":
                d, o, u_out, _, ell, tilt = geometry(r, near=0.0)
                tri = _shape_tri("vtx", o, d, u_out, ell, tilt, exact)
                tri[:3] = rays[r, 3:6]                                  # the vertex IS the origin
                lose.append((add(tri), r, sort))
            elif sort in ("nearf", "nearb"):
                tau = 0.01 * t_free[r] if pencil else max(32 * ulp, 1e-5 * size)
                d, o, u_out, t0, ell, tilt = geometry(r, near=tau if sort == "nearf" else -tau)
                tri = _shape_tri("in", o + t0 * d, d, u_out, ell, tilt, exact)
                (win if sort == "nearf" else lose).append((add(tri), r, sort))
            else:
                d, o, u_out, t0, ell, tilt = geometry(r)
                gap = min(ell, 0.3 * t0)
                front = _shape_tri("in", o + t0 * d, d, u_out, ell, tilt, exact)
                if sort == "back":
                    near = _shape_tri("in", o + (t0 - gap) * d, d, u_out, ell, tilt, exact, back=True)
                else:
                    # e2 = d * 2^k exactly: d x e2 = 0 in the fp64 products, det = 0
                    e2 = rays[r, :3] * F32(2.0 ** round(np.log2(ell)))
                    e1 = (ell * u_out).astype(F32)
                    v = (o + (t0 - gap) * d - 0.3 * e1.astype(F64) - 0.3 * e2.astype(F64)).astype(F32)
                    near = np.concatenate([v, e1, e2]).astype(F32)
                win.append((add(front), r, sort)); lose.append((add(near), r, sort))
    if edge_jobs:
        er = np.array([j[0] for j in edge_jobs]); es = [j[1] for j in edge_jobs]
        et = np.array([j[2] for j in edge_jobs], F32); ec = np.array([j[3] for j in edge_jobs])
        acc_t, rej_t, found = edge_twins(rays[er], et, ec, es)
        seen = set()
        for i in np.nonzero(found)[0]:
            if int(er[i]) in seen:
                continue
            seen.add(int(er[i]))
            pairs.append((len(win), len(lose)))
            win.append((add(acc_t[i]), int(er[i]), es[i])); lose.append((add(rej_t[i]), int(er[i]), es[i]))
    tris = np.concatenate([bg, np.array(tris_new, F32).reshape(-1, 9)])
    # keep the cases the whole scene bears out (a designed triangle of another ray may lie in front)
    rays_used = np.unique([w[1] for w in win] + [l[1] for l in lose])
    ref = dict(zip(rays_used.tolist(), O.brute_closest_tri(rays[rays_used], tris)[0].tolist()))
    ok_w = [ref[r] == k for k, r, _ in win]
    ok_l = [ref[r] != k for k, r, _ in lose]
    for a, b in pairs:
        ok_w[a] = ok_l[b] = ok_w[a] and ok_l[b]
    # face cases: the loser counts only with its winner
    wf = {(r, s): ok for (k, r, s), ok in zip(win, ok_w) if s in ("edgeon", "back")}
    ok_l = [ok and wf.get((r, s), True) for (k, r, s), ok in zip(lose, ok_l)]
    pos_w = np.cumsum(ok_w) - 1; pos_l = np.cumsum(ok_l) - 1
    pairs = [(pos_w[a], pos_l[b]) for a, b in pairs if ok_w[a]]
    win = [w for w, ok in zip(win, ok_w) if ok]; lose = [l for l, ok in zip(lose, ok_l) if ok]
    perm = rng.permutation(len(tris))
    inv = np.empty_like(perm); inv[perm] = np.arange(len(perm))
    tris = np.ascontiguousarray(tris[perm])
    col = lambda rows, j, dt: np.array([x[j] for x in rows], dt)
    designed = np.unique(np.concatenate([col(win, 1, np.int64), col(lose, 1, np.int64)]))
    return Scene(tris=tris, rays=rays, kind=kind, scale=scale, exact=exact,
                 win_tri=inv[col(win, 0, np.int64)], win_ray=col(win, 1, np.int64), win_sort=col(win, 2, object),
                 lose_tri=inv[col(lose, 0, np.int64)], lose_ray=col(lose, 1, np.int64), lose_sort=col(lose, 2, object),
                 pair_win=np.array([a for a, _ in pairs], np.int64), pair_lose=np.array([b for _, b in pairs], np.int64),
                 designed=designed)


# ---- meshes -------------------------------------------------------------------------------------
MESH_KINDS = ("icosphere", "soup", "sheets", "repeated")


def _icosphere(level):
    """Unit icosphere: (vertices [V, 3], faces [20 * 4^level, 3]), outward counter-clockwise."""
    g = (1 + 5 ** 0.5) / 2
    V = _unit(np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g),
                        (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], F64))
    Fc = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2),
                   (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5),
                   (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)])
    for _ in range(level):
        nf = len(Fc)
        e = np.sort(np.concatenate([Fc[:, [0, 1]], Fc[:, [1, 2]], Fc[:, [2, 0]]]), axis=1)
        ue, inv = np.unique(e, axis=0, return_inverse=True)
        inv = inv.ravel()
        n = len(V)
        V = np.concatenate([V, _unit(V[ue[:, 0]] + V[ue[:, 1]])])
        m01, m12, m20 = n + inv[:nf], n + inv[nf:2 * nf], n + inv[2 * nf:]
        Fc = np.concatenate([np.stack([Fc[:, 0], m01, m20], 1), np.stack([Fc[:, 1], m12, m01], 1),
                             np.stack([Fc[:, 2], m20, m12], 1), np.stack([m01, m12, m20], 1)])
    nrm = np.cross(V[Fc[:, 1]] - V[Fc[:, 0]], V[Fc[:, 2]] - V[Fc[:, 0]])
    flip = (nrm * V[Fc].sum(axis=1)).sum(axis=1) < 0
    Fc[flip] = Fc[flip][:, [0, 2, 1]]
    return V, Fc


def _heightfield(g, z0, rng, amp=0.02):
    xs = np.linspace(0, 1, g + 1)
    X, Y = np.meshgrid(xs, xs)
    Z = z0 + amp * np.sin(6 * X + 40 * z0) * np.cos(5 * Y) + 0.2 * amp * rng.standard_normal(X.shape)
    V = np.stack([X, Y, Z], -1)
    v00 = V[:-1, :-1]; v10 = V[:-1, 1:]; v01 = V[1:, :-1]; v11 = V[1:, 1:]
    t1 = np.concatenate([v00, v10 - v00, v01 - v00], -1).reshape(-1, 9)
    t2 = np.concatenate([v11, v01 - v11, v10 - v11], -1).reshape(-1, 9)
    return np.concatenate([t1, t2])


def mesh_rays(rng):
    """4133 rays (64 * 64 + 37) around the unit box: a pinhole camera above it, a -z grid wider than
    it, one interior origin with all directions, and rays with mixed origins, directions, lengths."""
    g = (np.arange(32) + 0.5) / 32
    U, W = (a.ravel() for a in np.meshgrid(g, g))
    r = np.zeros((4133, 7), F32)
    o = np.array([0.6, 0.3, 2.0])
    aim = np.stack([-0.3 + 1.6 * U, -0.3 + 1.6 * W, np.full(1024, 0.5)], 1)
    r[:1024, :3] = S._normalise32(aim - o); r[:1024, 3:6] = o
    r[1024:2048, 2] = -1.0
    r[1024:2048, 3] = -0.1 + 1.2 * U; r[1024:2048, 4] = -0.1 + 1.2 * W; r[1024:2048, 5] = 1.5
    r[2048:3072, :3] = S._normalise32(rng.normal(size=(1024, 3))); r[2048:3072, 3:6] = (0.52, 0.47, 0.55)
    r[3072:, :3] = S._normalise32(rng.normal(size=(1061, 3)))
    r[3072:, 3:6] = rng.uniform(-0.2, 1.2, (1061, 3))
    r[:, 6] = 4.0
    r[3072:, 6] = rng.uniform(0.1, 2.0, 1061)
    return r


def invalid_triangles(k, rng, kinds=("zero", "nan", "inf")):
    """k triangles no ray can hit: zero area, or a NaN or an infinite vertex."""
    t = _random_mesh(k, np.zeros(3), 1.0, (0.02, 0.2), rng, False)
    for i in range(k):
        what = kinds[i % len(kinds)]
        j = int(rng.integers(3))
        if what == "zero":
            variant = i // len(kinds) % 3                   # e2 = e1, e1 = 0, e2 = 2 e1
            if variant == 1:
                t[i, 3:6] = 0.0
            else:
                t[i, 6:9] = t[i, 3:6] * (1 if variant == 0 else 2)
        elif what == "nan":
            t[i, (j, 3 + j, 6 + j)[i // len(kinds) % 3]] = np.nan
        else:
            t[i, (j, 6 + j)[i // len(kinds) % 2]] = np.inf if i % 2 else -np.inf
    return t


def mesh_scene(kind, n, seed=0, inf_at_build=False):
    """n triangles (shuffled) and mesh_rays: "icosphere" (closed shells of radius 0.4, 0.32, ...
    around the box centre, the last one cut off at n), "soup" (edge lengths over three decades,
    needles of aspect 1e3, three triangles as large as the box), "sheets" (eight stacked height
    fields), "repeated" (one triangle n times).  About 0.5 % of the triangles are invalid at build
    time (`invalid`; infinite vertices only with inf_at_build: an infinite centroid collapses every
    Morton key); `late` holds as many invalid triangles to write into the sorted array afterwards.
    sheet: per triangle, its sheet ("sheets") or -1."""
    rng = np.random.default_rng(104729 * seed + 17 * n + MESH_KINDS.index(kind))
    sheet = np.full(n, -1)
    if kind == "icosphere":
        level = 0
        while level < 5 and 20 * 4 ** (level + 1) <= n:
            level += 1
        V, Fc = _icosphere(level)
        parts, radius = [], 0.4
        while sum(map(len, parts)) < n:
            P = 0.5 + radius * V
            parts.append(np.concatenate([P[Fc[:, 0]], P[Fc[:, 1]] - P[Fc[:, 0]], P[Fc[:, 2]] - P[Fc[:, 0]]], 1))
            radius *= 0.8
        tris = np.concatenate(parts)[:n]
    elif kind == "soup":
        c = rng.random((n, 3))
        ell = 0.3 * 10.0 ** rng.uniform(-3, 0, (n, 1))
        e1 = _unit(rng.normal(size=(n, 3))) * ell
        e2 = _unit(rng.normal(size=(n, 3))) * ell
        needle = rng.random(n) < 0.1
        e2[needle] *= 1e-3
        tris = np.concatenate([c - (e1 + e2) / 3, e1, e2], 1)
        big = np.array([[0, 0, 0.3, 1, 0, 0.1, 0, 1, 0.2], [1, 1, 0.6, -1, 0, 0.1, 0, -1, -0.2],
                        [0, 0.1, 0.9, 1, 0.2, -0.1, 0.1, 0.9, 0.0]])
        tris[rng.choice(n, 3, replace=False)] = big
    elif kind == "sheets":
        g = int(np.ceil(np.sqrt(n / 16)))
        parts = [_heightfield(g, 0.1 + 0.1 * k, rng) for k in range(8)]
        ids = np.repeat(np.arange(8), [len(p) for p in parts])
        pick = rng.permutation(len(ids))[:n]
        tris, sheet = np.concatenate(parts)[pick], ids[pick]
    else:
        tris = np.tile(np.array([[0.2, 0.2, 0.5, 0.6, 0, 0.1, 0, 0.6, -0.1]]), (n, 1))
    tris = tris.astype(F32)
    perm = rng.permutation(n)
    tris, sheet = np.ascontiguousarray(tris[perm]), sheet[perm]
    k = max(1, n // 200)
    kinds = ("zero", "nan", "inf") if inf_at_build else ("zero", "nan")
    invalid = rng.choice(n, k, replace=False)
    tris[invalid] = invalid_triangles(k, rng, kinds)
    sheet[invalid] = -1
    rays = mesh_rays(rng)
    return Scene(tris=tris, rays=rays, kind=kind, n=n, invalid=invalid, late=invalid_triangles(k, rng),
                 sheet=sheet, designed=np.arange(0), inf_at_build=inf_at_build)
