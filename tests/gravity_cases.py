"""The tree gravity's contract (include/grace_hip.h, grace_gravity_moments_f4 and grace_gravity_points_f4)
restated in NumPy, and the scenes of test_gravity.py with the preconditions test_gravity_cases.py checks.
No GPU, no test functions.

A tree is (nodes int32 [n_nodes, 16], leaves int32 [n_leaves, 4], root): node i's children are
nodes[i, 0] (left) and nodes[i, 1] (right), an index >= n_nodes is leaf index - n_nodes; leaf l covers
the primitives [leaves[l, 0], leaves[l, 0] + leaves[l, 1]).

Every fp32 step is one NumPy float32 operation (each rounds once, none is fused; np.sqrt and the divide
are correctly rounded); the fp64 running sums are np.add.accumulate from a leading +0, never a pairwise
sum; the node sums are Python floats (IEEE doubles), one add each, left operand first."""
import numpy as np

F32 = np.float32
F64 = np.float64
INF = F32(np.inf)


# ---- moments ------------------------------------------------------------------------------------
def _inner_preorder(nodes, root):
    """The inner nodes reachable from the root, parents before children."""
    n_nodes = len(nodes)
    order, stack = [], [int(root)]
    left, right = nodes[:, 0].tolist(), nodes[:, 1].tolist()
    while stack:
        i = stack.pop()
        if i >= n_nodes:
            continue
        order.append(i)
        stack.append(right[i])
        stack.append(left[i])
    return order


def moments(nodes, leaves, root, spheres, masses):
    """The records of grace_gravity_moments_f4 as uint32 [n_nodes, 12]."""
    nodes = np.asarray(nodes, np.int32).reshape(-1, 16)
    n_nodes, nl = len(nodes), len(leaves)
    if n_nodes == 0 or nl < 2:
        return np.zeros((0, 12), np.uint32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    m = np.asarray(masses, F32)
    first, count = leaves[:, 0].astype(np.int64), leaves[:, 1].astype(np.int64)
    M = np.zeros(nl, F64)
    S = np.zeros((nl, 3), F64)
    lo = np.full((nl, 3), INF, F32)
    hi = np.full((nl, 3), -INF, F32)
    for k in range(int(count.max())):                      # the k-th primitive of every leaf that has one
        sel = np.nonzero(count > k)[0]
        j = first[sel] + k
        mj = m[j].astype(F64)
        M[sel] = M[sel] + mj
        S[sel] = S[sel] + mj[:, None] * X[j].astype(F64)   # the product is exact in fp64
        lo[sel] = np.minimum(lo[sel], X[j])
        hi[sel] = np.maximum(hi[sel], X[j])
    # everything indexed like the children: inner nodes first, leaf l at n_nodes + l (Python floats and ints)
    pad = [0.0] * n_nodes
    Ma = pad + M.tolist()
    Sa = [pad + S[:, k].tolist() for k in range(3)]
    loa = [pad + lo[:, k].tolist() for k in range(3)]      # (float32 values are exact as doubles; min and max stay so)
    hia = [pad + hi[:, k].tolist() for k in range(3)]
    s0 = [0] * n_nodes + first.tolist()
    s1 = [0] * n_nodes + (first + count).tolist()
    left, right = nodes[:, 0].tolist(), nodes[:, 1].tolist()
    for i in reversed(_inner_preorder(nodes, root)):       # children before parents
        l, r = left[i], right[i]
        Ma[i] = Ma[l] + Ma[r]
        for k in range(3):
            Sa[k][i] = Sa[k][l] + Sa[k][r]
            loa[k][i] = min(loa[k][l], loa[k][r])
            hia[k][i] = max(hia[k][l], hia[k][r])
        s0[i] = min(s0[l], s0[r])
        s1[i] = max(s1[l], s1[r])
    Mn = np.array(Ma[:n_nodes], F64)
    rec = np.zeros((n_nodes, 12), np.uint32)
    recf = rec.view(F32)
    for k in range(3):
        lok = np.array(loa[k][:n_nodes], F64).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (np.array(Sa[k][:n_nodes], F64) / Mn).astype(F32)   # an fp64 divide, rounded once
        recf[:, k] = np.where(Mn != 0.0, c, lok)
        recf[:, 4 + k] = lok
        recf[:, 8 + k] = np.array(hia[k][:n_nodes], F64).astype(F32)
    recf[:, 3] = Mn.astype(F32)
    rec[:, 7] = np.array(s0[:n_nodes], np.int64).astype(np.uint32)
    rec[:, 11] = np.array(s1[:n_nodes], np.int64).astype(np.uint32)
    return rec


def record_fields(rec):
    """(c [n, 3], M32 [n], lo [n, 3], hi [n, 3], span_lo [n], span_hi [n]) of uint32 records."""
    f = np.ascontiguousarray(rec, np.uint32).view(F32)
    return (f[:, 0:3], f[:, 3], f[:, 4:7], f[:, 8:11], rec[:, 7].astype(np.int64), rec[:, 11].astype(np.int64))


# ---- acceptance and the pair term -----------------------------------------------------------------
def d2min_size2(lo, hi, p):
    """fp32 (d2min, size2) of the box lo, hi [3] against the points p [m, 3]."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.maximum(np.maximum(lo[None, :] - p, p - hi[None, :]), F32(0))
        d2min = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        size = np.max(hi - lo)
        return d2min, F32(size * size)


def accepts(lo, hi, p, theta):
    theta2 = F32(theta) * F32(theta)
    d2min, size2 = d2min_size2(lo, hi, p)
    with np.errstate(over="ignore", invalid="ignore"):
        return size2 < theta2 * d2min


def _terms(p, x, m, eps):
    """The fp64 contributions (ax, ay, az, u) of the terms {x, m} [..., 3], [...] at the points p [..., 3]."""
    eps2 = F32(eps) * F32(eps)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        dx, dy, dz = x[..., 0] - p[..., 0], x[..., 1] - p[..., 1], x[..., 2] - p[..., 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        s = d2 + eps2
        ir = F32(1) / np.sqrt(s)
        u = m * ir
        f = m * ((ir * ir) * ir)
        none = d2 == 0
        zero = F64(0)
        assert ir.dtype == F32 and f.dtype == F32 and u.dtype == F32
        return [np.where(none, zero, (f * d).astype(F64)) for d in (dx, dy, dz)] + [np.where(none, zero, u.astype(F64))]


def _running_sums(cols):
    """The last column of the sequential fp64 sums along axis 1, from a leading +0."""
    z = np.zeros((cols.shape[0], 1), F64)
    return np.add.accumulate(np.concatenate([z, cols], axis=1), axis=1)[:, -1]


def direct_sum(points, spheres, masses, eps):
    """The contract at theta = 0 without a tree: (out float64 [m, 4], counts int32 [m, 2])."""
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    mm = np.asarray(masses, F32)
    on = np.all(np.isfinite(P), axis=1)
    out = np.zeros((len(P), 4), F64)
    cnt = np.zeros((len(P), 2), np.int32)
    cnt[on, 1] = len(X)
    rows = np.nonzero(on)[0]
    chunk = max(1, (1 << 21) // max(len(X), 1))
    for a in range(0, len(rows), chunk):
        r = rows[a:a + chunk]
        t = _terms(P[r][:, None, :], X[None, :, :], mm[None, :], eps)
        for k in range(3):
            out[r, k] = _running_sums(t[k])
        out[r, 3] = -_running_sums(t[3])
    return out, cnt


def walk(nodes, leaves, root, spheres, masses, rec, points, theta, eps):
    """grace_gravity_points_f4: (out float64 [m, 4], counts int32 [m, 2]).  rec: the moment records (uint32).
    The recursion runs once for all points: each node is visited with the points that rejected all its
    ancestors, left child first, so the terms a point collects are in its own recursion's order."""
    nodes = np.asarray(nodes, np.int32).reshape(-1, 16)
    n_nodes = len(nodes) if len(leaves) > 1 else 0
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    mm = np.asarray(masses, F32)
    m = len(P)
    on = np.nonzero(np.all(np.isfinite(P), axis=1))[0]
    if n_nodes:
        c, M32, lo, hi, _, _ = record_fields(rec)
    t_point, t_x, t_m, t_node = [], [], [], []
    stack = [(int(root), on)]
    while stack:
        idx, alive = stack.pop()
        if len(alive) == 0:
            continue
        if idx >= n_nodes:
            first, count = (int(v) for v in leaves[idx - n_nodes][:2])
            j = np.arange(first, first + count)
            t_point.append(np.repeat(alive, count))
            t_x.append(np.tile(X[j], (len(alive), 1)))
            t_m.append(np.tile(mm[j], len(alive)))
            t_node.append(np.zeros(len(alive) * count, bool))
            continue
        acc = accepts(lo[idx], hi[idx], P[alive], theta)
        took = alive[acc]
        t_point.append(took)
        t_x.append(np.tile(c[idx], (len(took), 1)))
        t_m.append(np.full(len(took), M32[idx], F32))
        t_node.append(np.ones(len(took), bool))
        rest = alive[~acc]
        stack.append((int(nodes[idx, 1]), rest))
        stack.append((int(nodes[idx, 0]), rest))           # popped first
    out = np.zeros((m, 4), F64)
    cnt = np.zeros((m, 2), np.int32)
    if not t_point:
        return out, cnt
    tp = np.concatenate(t_point)
    order = np.argsort(tp, kind="stable")                  # per point, still the recursion's order
    tp = tp[order]
    tx = np.concatenate(t_x)[order].astype(F32)
    tm = np.concatenate(t_m)[order].astype(F32)
    tn = np.concatenate(t_node)[order]
    cnt[:, 0] = np.bincount(tp[tn], minlength=m)
    cnt[:, 1] = np.bincount(tp[~tn], minlength=m)
    vals = _terms(P[tp], tx, tm, eps)
    per = np.bincount(tp, minlength=m)
    start = np.concatenate([[0], np.cumsum(per)])
    rank = np.arange(len(tp)) - start[tp]
    block = 256
    for a in range(0, m, block):
        b = min(a + block, m)
        s0, s1 = start[a], start[b]
        if s1 == s0:
            continue
        width = int(per[a:b].max())
        for k in range(4):
            cols = np.zeros((b - a, width), F64)
            cols[tp[s0:s1] - a, rank[s0:s1]] = vals[k][s0:s1]   # +0 beyond a point's last term: fl(x + 0) = x
            out[a:b, k] = _running_sums(cols)
    out[on, 3] = -out[on, 3]                               # phi = -P (an on point without a term: -0)
    return out, cnt


def walk_point_scalar(nodes, leaves, root, spheres, masses, rec, p, theta, eps):
    """The same recursion for one finite point in NumPy scalars, term by term: (out [4], counts [2])."""
    nodes = np.asarray(nodes, np.int32).reshape(-1, 16)
    n_nodes = len(nodes) if len(leaves) > 1 else 0
    p = np.asarray(p[:3], F32)
    theta2, eps2 = F32(theta) * F32(theta), F32(eps) * F32(eps)
    f = np.ascontiguousarray(rec, np.uint32).view(F32) if n_nodes else None
    A = [F64(0), F64(0), F64(0)]
    Pot = F64(0)
    cnt = [0, 0]

    def term(x, mass):
        nonlocal Pot
        d = [F32(x[k] - p[k]) for k in range(3)]
        d2 = F32(F32(F32(d[0] * d[0]) + F32(d[1] * d[1])) + F32(d[2] * d[2]))
        if d2 == 0:
            return
        ir = F32(F32(1) / np.sqrt(F32(d2 + eps2)))
        u = F32(mass * ir)
        ff = F32(mass * F32(F32(ir * ir) * ir))
        for k in range(3):
            A[k] = A[k] + F64(F32(ff * d[k]))
        Pot = Pot + F64(u)

    stack = [int(root)]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        while stack:
            idx = stack.pop()
            if idx >= n_nodes:
                first, count = (int(v) for v in leaves[idx - n_nodes][:2])
                for j in range(first, first + count):
                    term(spheres[j, :3].astype(F32), F32(masses[j]))
                    cnt[1] += 1
                continue
            lo, hi = f[idx, 4:7], f[idx, 8:11]
            e = [max(max(F32(lo[k] - p[k]), F32(p[k] - hi[k])), F32(0)) for k in range(3)]
            d2min = F32(F32(F32(e[0] * e[0]) + F32(e[1] * e[1])) + F32(e[2] * e[2]))
            size = max(F32(hi[k] - lo[k]) for k in range(3))
            if F32(size * size) < F32(theta2 * d2min):
                term(f[idx, 0:3], f[idx, 3])
                cnt[0] += 1
            else:
                stack.append(int(nodes[idx, 1]))
                stack.append(int(nodes[idx, 0]))
    return np.array(A + [-Pot], F64), np.array(cnt, np.int32)


def max_stack_entries(nodes, leaves, root):
    """The walk's push rule restated: an entry is an inner node or a range of primitives; a popped node
    pushes its right child, then its left; a leaf is pushed as its range, and a range pushed directly on
    a range that starts where it ends is merged into it.  Returns the largest number of entries while every
    node is opened.  A packet opens a subset of the nodes and always pushes both children of a node it
    opens, so what lies under a node when it is reached is the same in every walk: this is the bound for
    every packet and every theta."""
    nodes = np.asarray(nodes, np.int32).reshape(-1, 16)
    n_nodes = len(nodes) if len(leaves) > 1 else 0
    left, right = nodes[:, 0].tolist(), nodes[:, 1].tolist()
    lf = np.asarray(leaves)[:, :2].tolist()
    stack, most = [], 0

    def push(idx):
        if idx >= n_nodes:
            first, count = lf[idx - n_nodes]
            if count <= 0:
                return
            if stack and stack[-1][1] > 0 and stack[-1][0] == first + count:
                stack[-1] = (first, count + stack[-1][1])
                return
            stack.append((first, count))
        else:
            stack.append((idx, 0))

    push(int(root))
    while stack:
        most = max(most, len(stack))
        idx, count = stack.pop()
        if count == 0:
            push(right[idx])
            push(left[idx])
            most = max(most, len(stack))
    return most


def fp64_direct(points, spheres, masses, eps):
    """The accuracy yardstick: the softened direct sum in fp64 throughout (a, phi), self pairs skipped."""
    P = np.asarray(points[:, :3], F64)
    X = np.asarray(spheres[:, :3], F64)
    mm = np.asarray(masses, F64)
    out = np.zeros((len(P), 4), F64)
    for a in range(0, len(P), 256):
        d = X[None, :, :] - P[a:a + 256, None, :]
        d2 = np.sum(d * d, axis=2)
        with np.errstate(divide="ignore"):
            ir = np.where(d2 == 0, 0.0, 1.0 / np.sqrt(d2 + float(eps) ** 2))
        out[a:a + 256, :3] = np.sum((mm[None, :] * ir ** 3)[:, :, None] * d, axis=1)
        out[a:a + 256, 3] = -np.sum(mm[None, :] * ir, axis=1)
    return out


# ---- scenes -----------------------------------------------------------------------------------------
THETAS = (0.0, 0.3, 0.7, 1000.0)
SOFTENINGS = (0.0, 0.01)
LEAF_SIZES = (1, 8, 32)
FACE_THETA = 1e15          # theta^2 = 1e30: one ulp outside a face accepts any box of this scene


def random_scene(n=2000, seed=3):
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = (0.01 + 0.04 * rng.random(n)).astype(F32)
    return s


def clustered_scene(n=2000, seed=5):
    rng = np.random.default_rng(seed)
    centres = np.array([[0.3, 0.3, 0.3], [0.7, 0.6, 0.4], [0.5, 0.5, 0.8]])
    k = rng.integers(0, 3, n)
    s = np.empty((n, 4), F32)
    s[:, :3] = np.clip(centres[k] + rng.normal(0.0, 0.02, (n, 3)) * rng.random((n, 1)) ** 3, 0.001, 0.999)
    s[:, 3] = (0.004 + 0.02 * rng.random(n)).astype(F32)
    return s


def lattice_scene():
    """16 x 16 x 8 binary-exact sites: many equal distances and box edges."""
    gx = (np.arange(16, dtype=F32) + F32(0.5)) / F32(16)
    gz = (np.arange(8, dtype=F32) + F32(0.5)) / F32(8)
    z, y, x = np.meshgrid(gz, gx, gx, indexing="ij")
    s = np.empty((2048, 4), F32)
    s[:, 0], s[:, 1], s[:, 2] = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    s[:, 3] = F32(1.0 / 16)
    return s


def spine_scene():
    """300 coincident centres and 50 others: with max_per_leaf = 1 a spine of leaves deeper than the stack,
    size-0 nodes, a merged range longer than a cluster and d2 == 0 terms."""
    s = random_scene(350, 17)
    s[:300, :3] = np.array([0.625, 0.375, 0.125], F32)
    return s


SPINE_AT = np.array([0.625, 0.375, 0.125], F32)
SCENES = {"random": random_scene, "clustered": clustered_scene, "lattice": lattice_scene}


def masses_for(n, seed=23):
    """0.5 .. 1.5, every 37th zero."""
    m = (0.5 + np.random.default_rng(seed).random(n)).astype(F32)
    m[::37] = 0
    return m


def zero_mass_leaf(masses, leaves, which):
    """A copy of the masses with every primitive of leaf `which` at zero."""
    m = np.array(masses, F32)
    first, count = (int(v) for v in leaves[which][:2])
    m[first:first + count] = 0
    return m


def zero_mass_node(masses, rec):
    """A copy of the masses with every primitive under one inner node at zero -- the node with the narrowest
    span, two leaves at least -- so that its record has M == 0 and c = lo.  Returns (masses, node)."""
    _, _, _, _, s0, s1 = record_fields(rec)
    node = int(np.argmin(s1 - s0))
    m = np.array(masses, F32)
    m[s0[node]:s1[node]] = 0
    return m, node


def cpu_tree(s, max_per_leaf):
    """The library's build_tree on the CPU oracle: 30-bit keys in the unit box, a stable sort, Euclidean
    deltas, the ALBVH.  Returns (spheres in tree order, nodes, leaves, root)."""
    import oracle as O
    keys = O.morton_keys30(s, (0, 0, 0), (1, 1, 1))
    s = np.ascontiguousarray(s[np.argsort(keys, kind="stable")])
    nodes, leaves, root, _ = O.albvh(s, O.deltas_euclid(s), max_per_leaf)
    return s, nodes, leaves, root


def query_points(spheres, seed=11, n_random=650, n_centres=340):
    """About 1000 points: random ones in and around the box, sphere centres (self pairs), far ones that
    accept the root, and four with a non-finite coordinate; shuffled."""
    rng = np.random.default_rng(seed)
    far = np.array([[50.0, 50.0, 50.0], [-40.0, 0.5, 0.5], [0.5, 1e6, 0.5], [1e20, 0.5, 0.5], [-3.0, -3.0, 7.0],
                    [2.5, 0.5, 0.5]], F32)
    off = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan]], F32)
    pts = np.concatenate([rng.random((n_random, 3), dtype=F32) * F32(1.2) - F32(0.1),
                          spheres[rng.choice(len(spheres), min(n_centres, len(spheres)), replace=False), :3],
                          far, off]).astype(F32)
    return pts[rng.permutation(len(pts))]


def packet_points(counts=(63, 64, 65), total=2304, seed=29):
    """At least 2048 points, so that the packets are cut at the eight cells of the first Morton level as
    well as at every 64th point: `counts` points in each of the first octants of the unit box (away from
    its mid-planes), the rest in the last octant."""
    rng = np.random.default_rng(seed)
    parts = []
    sizes = list(counts) + [total - sum(counts)]
    for o, k in zip(list(range(len(counts))) + [7], sizes):
        corner = np.array([(o >> 0) & 1, (o >> 1) & 1, (o >> 2) & 1], F32) * F32(0.5)
        parts.append(corner[None, :] + F32(0.1) + F32(0.3) * rng.random((k, 3), dtype=F32))
    return np.concatenate(parts).astype(F32)


def mixed_points(rec, node=None, theta=0.7):
    """64 points on a line off the +x face of a node's box (the root's by default: the record with the
    widest span), from 2 % inside to 2 % beyond the distance size / theta at which it is accepted."""
    c, M32, lo, hi, s0, s1 = record_fields(rec)
    if node is None:
        node = int(np.argmax(s1 - s0))
    size = float(np.max(hi[node] - lo[node]))
    t = np.linspace(-0.02, 0.02, 64)
    pts = np.empty((64, 3), F32)
    pts[:, 0] = (float(hi[node, 0]) + size / theta * (1.0 + t)).astype(F32)
    pts[:, 1] = F32(0.5) * (lo[node, 1] + hi[node, 1])
    pts[:, 2] = F32(0.5) * (lo[node, 2] + hi[node, 2])
    return pts, node


def face_points(rec, n_boxes=8):
    """Points on the six faces of the widest-span nodes' boxes (the other two coordinates at the box's
    middle), and the same points moved one ulp outwards: (on [k, 3], outside [k, 3], node [k])."""
    c, M32, lo, hi, s0, s1 = record_fields(rec)
    pick = np.argsort(-(s1 - s0), kind="stable")[:n_boxes]
    on, out, which = [], [], []
    for i in pick:
        mid = (F32(0.5) * (lo[i] + hi[i])).astype(F32)
        for k in range(3):
            for bound, away in ((lo[i, k], -INF), (hi[i, k], INF)):
                p = mid.copy(); p[k] = bound
                q = mid.copy(); q[k] = np.nextafter(F32(bound), away)
                on.append(p); out.append(q); which.append(i)
    return np.array(on, F32), np.array(out, F32), np.array(which)
