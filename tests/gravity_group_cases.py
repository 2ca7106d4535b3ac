"""The contract of the gravity within groups (include/grace_hip.h, grace_gravity_group_moments_f4 and
grace_gravity_group_points_f4) restated in NumPy on top of gravity_cases.py, the labellings of
test_gravity_groups.py and the point sets whose preconditions test_gravity_group_cases.py checks.
No GPU, no test functions.

Trees, records, the fp32 steps and the fp64 running sums are gravity_cases.py's.  labels: int [n_spheres]
in tree order, < 0: in no group; ranges: int32 [n_nodes, 2] = {smallest, largest label >= 0 below the
node}, {INT32_MAX, -1} where there is none.

build_tree sorts its argument, so a labelling is a function of the sphere's record, evaluated on the spheres
in tree order: of the position, or -- for coincident centres -- of the bits of h."""
import numpy as np

import gravity_cases as G
from gravity_cases import (F32, F64, INF, _inner_preorder, _running_sums, _terms, accepts,  # noqa: F401
                           clustered_scene, cpu_tree, lattice_scene, random_scene, record_fields, spine_scene)

INT_MAX = np.iinfo(np.int32).max


# ---- moments ------------------------------------------------------------------------------------
def group_moments(nodes, leaves, root, spheres, masses, labels):
    """(records uint32 [n_nodes, 12], ranges int32 [n_nodes, 2]) of grace_gravity_group_moments_f4."""
    nodes = np.asarray(nodes, np.int32).reshape(-1, 16)
    n_nodes, nl = len(nodes), len(leaves)
    if n_nodes == 0 or nl < 2:
        return np.zeros((0, 12), np.uint32), np.zeros((0, 2), np.int32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    m = np.asarray(masses, F32)
    lab = np.asarray(labels, np.int64)
    first, count = leaves[:, 0].astype(np.int64), leaves[:, 1].astype(np.int64)
    M = np.zeros(nl, F64)
    S = np.zeros((nl, 3), F64)
    lo = np.full((nl, 3), INF, F32)
    hi = np.full((nl, 3), -INF, F32)
    l0 = np.full(nl, INT_MAX, np.int64)
    l1 = np.full(nl, -1, np.int64)
    for k in range(int(count.max())):                      # the k-th primitive of every leaf that has one ...
        sel = np.nonzero(count > k)[0]
        sel = sel[lab[first[sel] + k] >= 0]                # ... and where it is labelled: the others are skipped
        j = first[sel] + k
        mj = m[j].astype(F64)
        M[sel] = M[sel] + mj
        S[sel] = S[sel] + mj[:, None] * X[j].astype(F64)
        lo[sel] = np.minimum(lo[sel], X[j])
        hi[sel] = np.maximum(hi[sel], X[j])
        l0[sel] = np.minimum(l0[sel], lab[j])
        l1[sel] = np.maximum(l1[sel], lab[j])
    pad = [0.0] * n_nodes
    Ma = pad + M.tolist()
    Sa = [pad + S[:, k].tolist() for k in range(3)]
    loa = [pad + lo[:, k].tolist() for k in range(3)]
    hia = [pad + hi[:, k].tolist() for k in range(3)]
    s0 = [0] * n_nodes + first.tolist()
    s1 = [0] * n_nodes + (first + count).tolist()          # the spans cover every primitive
    la = [0] * n_nodes + l0.tolist()
    lb = [0] * n_nodes + l1.tolist()
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
        la[i] = min(la[l], la[r])
        lb[i] = max(lb[l], lb[r])
    Mn = np.array(Ma[:n_nodes], F64)
    rec = np.zeros((n_nodes, 12), np.uint32)
    recf = rec.view(F32)
    for k in range(3):
        lok = np.array(loa[k][:n_nodes], F64).astype(F32)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (np.array(Sa[k][:n_nodes], F64) / Mn).astype(F32)
        recf[:, k] = np.where(Mn != 0.0, c, lok)
        recf[:, 4 + k] = lok
        recf[:, 8 + k] = np.array(hia[k][:n_nodes], F64).astype(F32)
    recf[:, 3] = Mn.astype(F32)
    rec[:, 7] = np.array(s0[:n_nodes], np.int64).astype(np.uint32)
    rec[:, 11] = np.array(s1[:n_nodes], np.int64).astype(np.uint32)
    ranges = np.stack([np.array(la[:n_nodes], np.int64), np.array(lb[:n_nodes], np.int64)], axis=1).astype(np.int32)
    return rec, ranges


# ---- the walk -------------------------------------------------------------------------------------
def group_walk(nodes, leaves, root, spheres, masses, labels, rec, ranges, points, point_labels, theta, eps,
               stats=None):
    """grace_gravity_group_points_f4: (out float64 [m, 4], counts int32 [m, 2]).  The recursion runs once for
    all points: each node is visited with the points that are live there -- those that opened its parent and
    whose label its range holds -- left child first, so a point's terms are in its own recursion's order.
    stats: a dict that receives, per event the preconditions name, the list of (node, number of points)."""
    nodes = np.asarray(nodes, np.int32).reshape(-1, 16)
    n_nodes = len(nodes) if len(leaves) > 1 else 0
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    mm = np.asarray(masses, F32)
    lab = np.asarray(labels, np.int64)
    PL = np.asarray(point_labels, np.int64)
    m = len(P)
    on_mask = np.all(np.isfinite(P), axis=1) & (PL >= 0)
    on = np.nonzero(on_mask)[0]
    if n_nodes:
        c, M32, lo, hi, s0, s1 = record_fields(rec)
    if stats is not None:
        for key in ("empty", "pure_accepted", "pure_other", "range_only"):
            stats.setdefault(key, [])
    t_point, t_x, t_m, t_node = [], [], [], []
    stack = [(int(root), on)]
    while stack:
        idx, arrived = stack.pop()
        if len(arrived) == 0:
            continue
        if idx >= n_nodes:
            first, count = (int(v) for v in leaves[idx - n_nodes][:2])
            for j in range(first, first + count):          # ascending index; a point takes j iff the labels are equal
                took = arrived[PL[arrived] == lab[j]]
                t_point.append(took)
                t_x.append(np.tile(X[j], (len(took), 1)))
                t_m.append(np.full(len(took), mm[j], F32))
                t_node.append(np.zeros(len(took), bool))
            continue
        l0, l1 = int(ranges[idx, 0]), int(ranges[idx, 1])
        live = (PL[arrived] >= l0) & (PL[arrived] <= l1)
        alive = arrived[live]
        if stats is not None:
            if l1 < 0:
                stats["empty"].append((idx, len(arrived)))
            elif l0 == l1 and len(alive) < len(arrived):
                stats["pure_other"].append((idx, len(arrived) - len(alive)))
            elif l0 != l1 and len(alive):
                below = np.unique(lab[s0[idx]:s1[idx]])
                only = int(np.sum(~np.isin(PL[alive], below)))
                if only:
                    stats["range_only"].append((idx, only))
        if len(alive) == 0:
            continue
        acc = accepts(lo[idx], hi[idx], P[alive], theta) if l0 == l1 else np.zeros(len(alive), bool)
        took = alive[acc]
        if stats is not None and len(took):
            stats["pure_accepted"].append((idx, len(took)))
        t_point.append(took)
        t_x.append(np.tile(c[idx], (len(took), 1)))
        t_m.append(np.full(len(took), M32[idx], F32))
        t_node.append(np.ones(len(took), bool))
        rest = alive[~acc]
        stack.append((int(nodes[idx, 1]), rest))
        stack.append((int(nodes[idx, 0]), rest))           # popped first
    out = np.zeros((m, 4), F64)
    cnt = np.zeros((m, 2), np.int32)
    tp = np.concatenate(t_point) if t_point else np.zeros(0, np.int64)
    if len(tp):
        order = np.argsort(tp, kind="stable")              # per point, still the recursion's order
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
            a0, a1 = start[a], start[b]
            if a1 == a0:
                continue
            width = int(per[a:b].max())
            for k in range(4):
                cols = np.zeros((b - a, width), F64)
                cols[tp[a0:a1] - a, rank[a0:a1]] = vals[k][a0:a1]
                out[a:b, k] = _running_sums(cols)
    out[on, 3] = -out[on, 3]                               # phi = -P (an on point without a term: -0)
    return out, cnt


def group_walk_point_scalar(nodes, leaves, root, spheres, masses, labels, rec, ranges, p, label, theta, eps):
    """The same recursion for one finite point of label >= 0 in NumPy scalars, term by term: (out [4], counts [2])."""
    nodes = np.asarray(nodes, np.int32).reshape(-1, 16)
    n_nodes = len(nodes) if len(leaves) > 1 else 0
    p = np.asarray(p[:3], F32)
    L = int(label)
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
                    if int(labels[j]) == L:
                        term(spheres[j, :3].astype(F32), F32(masses[j]))
                        cnt[1] += 1
                continue
            l0, l1 = int(ranges[idx, 0]), int(ranges[idx, 1])
            if l0 > L or l1 < L:
                continue
            lo, hi = f[idx, 4:7], f[idx, 8:11]
            e = [max(max(F32(lo[k] - p[k]), F32(p[k] - hi[k])), F32(0)) for k in range(3)]
            d2min = F32(F32(F32(e[0] * e[0]) + F32(e[1] * e[1])) + F32(e[2] * e[2]))
            size = max(F32(hi[k] - lo[k]) for k in range(3))
            if l0 == l1 and F32(size * size) < F32(theta2 * d2min):
                term(f[idx, 0:3], f[idx, 3])
                cnt[0] += 1
            else:
                stack.append(int(nodes[idx, 1]))
                stack.append(int(nodes[idx, 0]))
    return np.array(A + [-Pot], F64), np.array(cnt, np.int32)


def masked_direct_sum(points, point_labels, spheres, masses, labels, eps):
    """The contract at theta = 0 without a tree: per label, gravity_cases.direct_sum over the spheres that
    carry it, at the points that carry it.  (out float64 [m, 4], counts int32 [m, 2])."""
    PL = np.asarray(point_labels, np.int64)
    lab = np.asarray(labels, np.int64)
    out = np.zeros((len(points), 4), F64)
    cnt = np.zeros((len(points), 2), np.int32)
    for L in np.unique(PL[PL >= 0]):
        rows, members = np.nonzero(PL == L)[0], lab == L
        out[rows], cnt[rows] = G.direct_sum(points[rows], spheres[members], np.asarray(masses, F32)[members], eps)
    return out, cnt


# ---- labellings -------------------------------------------------------------------------------------
BLOB_CENTRES = np.array([[0.3, 0.3, 0.3], [0.7, 0.6, 0.4], [0.5, 0.5, 0.8]])   # clustered_scene's
BLOB_CUT = 0.02            # further than this from its centre: in no group
LONELY = 7                 # carried by exactly one particle
ABSENT = 9                 # carried by no particle


def _nearest_blob(x):
    x = np.nan_to_num(np.asarray(x[:, :3], F64), nan=0.0, posinf=1e30, neginf=-1e30)
    d = np.linalg.norm(x[:, None, :] - BLOB_CENTRES[None, :, :], axis=2)
    k = np.argmin(d, axis=1)
    return k.astype(np.int32), d[np.arange(len(x)), k]


def blobs(s):
    """The nearest of clustered_scene's three centres; -1 beyond BLOB_CUT from it, so that the unlabelled
    particles sit around and inside the boxes of the labelled ones."""
    k, d = _nearest_blob(s)
    return np.where(d > BLOB_CUT, -1, k).astype(np.int32)


def slabs(s):
    """floor(8 x): monotone along one axis, pure nodes next to mixed ones."""
    x = np.nan_to_num(np.asarray(s[:, 0], F64), nan=0.0, posinf=0.0, neginf=0.0)
    return np.clip(np.floor(8.0 * x), -1, 8).astype(np.int32)


def scatter(s):
    """A hash of the coordinate bits mod 5, minus 1: -1 .. 3, uncorrelated with the tree."""
    b = np.ascontiguousarray(s[:, :3], F32).view(np.uint32).astype(np.uint64)
    h = (b[:, 0] * np.uint64(0x9E3779B1) + b[:, 1] * np.uint64(0x85EBCA77) + b[:, 2] * np.uint64(0xC2B2AE3D)) \
        & np.uint64(0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(13))
    return (h % np.uint64(5)).astype(np.int32) - 1


def single(s):
    return np.zeros(len(s), np.int32)


def lonely(s):
    """blobs, and the label LONELY on the one sphere whose centre is the smallest in (x, y, z) order."""
    lab = blobs(s)
    lab[np.lexsort((s[:, 2], s[:, 1], s[:, 0]))[0]] = LONELY
    return lab


def spine_labels(s):
    """Two labels by the lowest bit of h: interleaved along a run of coincident centres, whose order in the
    tree is the caller's (the sort is stable)."""
    return (np.ascontiguousarray(s[:, 3], F32).view(np.uint32) & 1).astype(np.int32)


LABELLINGS = {"blobs": blobs, "slabs": slabs, "scatter": scatter, "single": single, "lonely": lonely}


def point_labels(name, pts):
    """Labels for query points under a labelling: by position as for the spheres, but every point near or far
    gets its nearest blob (so far points meet pure nodes of their label), slabs are clipped into 0 .. 7 and
    scatter keeps its -1; lonely: every 50th point LONELY, the one after it ABSENT."""
    if name in ("blobs", "lonely"):
        lab = _nearest_blob(pts)[0].copy()
        if name == "lonely":
            lab[::50] = LONELY
            lab[1::50] = ABSENT
        return lab
    if name == "slabs":
        return np.clip(slabs(pts), 0, 7).astype(np.int32)
    if name == "scatter":
        return scatter(np.nan_to_num(np.asarray(pts[:, :3], F32), nan=0.0, posinf=0.0, neginf=0.0))
    return np.zeros(len(pts), np.int32)


def pure_node(rec, ranges):
    """The inner node with the widest span among those that hold exactly one label and have a box of nonzero size."""
    _, _, lo, hi, s0, s1 = record_fields(rec)
    ok = (ranges[:, 0] == ranges[:, 1]) & (np.max(hi - lo, axis=1) > 0)
    return int(np.argmax(np.where(ok, s1 - s0, -1)))


def mixed_label_packet(rec, ranges, theta=0.7):
    """gravity_cases.mixed_points off the +x face of pure_node, and point labels that alternate between the
    node's label, the next label up and the next but one: lanes of the first kind accept or open the node,
    the others pass it by.  (points [64, 3], point labels [64], node)."""
    node = pure_node(rec, ranges)
    pts, _ = G.mixed_points(rec, node=node, theta=theta)
    lab = (int(ranges[node, 0]) + np.arange(64) % 3).astype(np.int32)
    return pts, lab, node
