"""The point-query front end (csrc/point_packets.hip: Morton keys of the caller's points, the nested sort,
packets cut at every 64th sorted point and at every change of Morton cell) across the point counts at
which it changes behaviour, and on streams and contexts of its own.

The cell level L is the largest with 8^L * 256 <= m (steps at 2048, 16384, 131072 and 1048576 points),
the nested sort goes to the bucket sort at m >= 2^18, and the three packet kernels are grid-stride loops
over at most 2^20 threads.  Every family that goes through the front end (range counts / lists / gather
sums, k nearest neighbours, interpolation at points, pair counts / radial profiles, friends-of-friends)
is run on both sides of each of those counts, in two point layouts, and every output slot is compared
bit for bit with the NumPy restatement of the contract in include/grace_hip.h (the restatements of the
families' own test modules).  Output buffers are pre-filled with values the contract cannot produce
(-7, a NaN with a payload), so that a slot no packet wrote fails the comparison.

From 131071 points up the points are an index map into a pool of at most 16384 distinct (position,
radius) records: the restatement runs on the pool and is expanded by the map, and all m outputs are
still compared.  The duplicated points are long runs of equal keys, the sort's tie case."""
import threading

import numpy as np
import pytest

from test_fof import restate_catalogue, restate_labels
from test_neighbours import _build, brute_knn
from test_pair_counts import restate as restate_pairs
from test_range_queries import _same, restate, restate_sums
from test_sph_interpolation import pairs as field_pairs
from test_sph_interpolation import restate as restate_field

F32 = np.float32
SIZES = (2047, 2048, 2049, 16383, 16384, 16385, 131071, 131072, 131073, 262143, 262144, 262145,
         1048575, 1048576, 1048577, 1048576 + 4097)
LAYOUTS = ("spread", "clumped")
POOL = 16384                       # distinct records from 131071 points up
BUCKET_SORT = 1 << 18              # bucket_plan() of sort.hip
GRID_THREADS = 4096 * 256          # stream_grid(): the packet kernels' second iteration starts here
N_SCENE = 3000
R_SHARED = F32(0.03)
# per-point radii, log-uniform from 1e-3 to (spread; clumped; clumped from 2^20 - 1 points, where the lists would
# otherwise pass 2 10^7 entries: checked in the list test)
R_MAX = (0.15, 0.08, 0.03)
EDGES = np.array([0.004, 0.008, 0.015, 0.03, 0.06], F32)
K_SMALL, K_LARGE = 8, 64
FOF_SIZES = (2047, 2048, 2049, 16383, 16384, 16385)
N_OFF = 12
NAN_BITS = 0x7FC0BEEF              # the float32 sentinel: a NaN no arithmetic produces


# ---- the scene -------------------------------------------------------------------------------------
def make_scene(n=N_SCENE, seed=2):
    """Three Gaussian blobs over a uniform background and one coincident group of 100; the first blob
    sits where the clumped layout puts its clump."""
    rng = np.random.default_rng(seed)
    n_co = 100
    n_bg = n // 4
    n_blob = n - n_bg - n_co
    centres = np.array([[0.746, 0.746, 0.746], [0.3, 0.35, 0.4], [0.5, 0.25, 0.7]])
    s = np.empty((n, 4), F32)
    x = centres[rng.integers(0, 3, n_blob)] + rng.normal(0.0, 0.03, (n_blob, 3))
    s[:n_blob, :3] = np.clip(x, 0.1, 0.9)
    s[n_blob:n_blob + n_bg, :3] = 0.1 + 0.8 * rng.random((n_bg, 3))
    s[n_blob + n_bg:, :3] = np.array([0.375, 0.625, 0.5], F32)
    s[:, 3] = (0.01 + 0.03 * rng.random(n)).astype(F32)
    s[0, :3] = 0.1; s[1, :3] = 0.9                                 # the box does not depend on the draw
    return s[rng.permutation(n)]


def root_box(s):
    """The root box of the tree: the union of the spheres' boxes (to fp32 rounding)."""
    lo = (s[:, :3] - s[:, 3:4]).astype(F32).min(axis=0)
    hi = (s[:, :3] + s[:, 3:4]).astype(F32).max(axis=0)
    return lo, hi


# ---- packet_keys_kernel, restated --------------------------------------------------------------------
def cell_level(m):
    level = 0
    while level < 10 and (1 << (3 * (level + 1))) * 256 <= m:
        level += 1
    return level


def _spread_bits(c):
    c = c.astype(np.uint32)
    out = np.zeros_like(c)
    for b in range(10):
        out |= ((c >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def restate_keys(points, lo, hi):
    """The 30-bit keys: clamp into the box (NaN: to its lower corner), min(uint32(t * 1023), 1023) per axis,
    interleaved with x least significant."""
    P = np.asarray(points, F32)[:, :3]
    v = np.fmin(np.fmax(P, lo), hi)                                # fmaxf / fminf: NaN gives the other operand
    ext = (hi - lo).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(ext > 0, ((v - lo).astype(F32) / ext).astype(F32), F32(0))
    c = np.minimum((np.fmax(t, F32(0)) * F32(1023)).astype(F32).astype(np.uint32), np.uint32(1023))
    return (_spread_bits(c[:, 2]) << np.uint32(2)) | (_spread_bits(c[:, 1]) << np.uint32(1)) | _spread_bits(c[:, 0])


def restate_cells(points, lo, hi, level):
    return restate_keys(points, lo, hi) >> np.uint32(30 - 3 * level)


def cell_of(cx, cy, cz, level):
    """The cell number (key >> shift) of the cell with per-axis cell coordinates cx, cy, cz."""
    c = np.array([[cx, cy, cz]], np.uint32) << np.uint32(10 - level)
    key = (_spread_bits(c[:, 2]) << np.uint32(2)) | (_spread_bits(c[:, 1]) << np.uint32(1)) | _spread_bits(c[:, 0])
    return int(key[0] >> np.uint32(30 - 3 * level))


# ---- the point sets ----------------------------------------------------------------------------------
def _reserved(level):
    """Cells kept clear of the layouts' own draws: (those that get exactly one point, those that get a few)."""
    C = 1 << level
    if level == 0:
        return [], []
    if level == 1:
        return [(0, 0, 0)], [(C - 1, 0, 0)]
    return [(0, 0, 0), (1, 2, 3)], [(C - 1, 0, 0), (2, 1, 3)]


class PointSet:
    """records: float32 [n_rec, 3] positions and [n_rec] radii; index: int64 [m], the record of each point in
    caller order (a permutation below 131071 points: all positions distinct)."""

    def __init__(self, m, layout, lo, hi):
        self.m, self.layout, self.level = m, layout, cell_level(m)
        rng = np.random.default_rng(1000 * SIZES.index(m) + LAYOUTS.index(layout) if m in SIZES else m)
        L, C = self.level, 1 << self.level
        W = float(1 << (10 - L)) / 1023.0                          # a cell's width in t
        lo64, ext64 = lo.astype(np.float64), (hi.astype(np.float64) - lo.astype(np.float64))
        pooled = m >= 131071
        n_norm_pts = m - N_OFF
        single, few = _reserved(L)
        c75 = (3 * C) // 4
        self.clump = (c75, c75, c75)

        def in_cell(cell, u):
            """Positions at fractions u of a cell shrunk by a tenth of its width on every side."""
            t = (np.asarray(cell, np.float64) + 0.1 + 0.8 * u) * W
            return lo64 + t * ext64

        recs, mult = [], []                                        # positions [k, 3], points per record [k]

        def add(pos, counts):
            recs.append(np.atleast_2d(pos)); mult.append(np.atleast_1d(counts).astype(np.int64))

        def add_cell(cell, count):
            """count points in a cell: distinct records, or two records that share them."""
            if count == 1:
                add(in_cell(cell, np.full(3, 0.5)), 1)              # the cell's centre
            elif not pooled:
                add(in_cell(cell, rng.random((count, 3))), np.ones(count))
            else:
                add(in_cell(cell, rng.random((2, 3))), [count // 2, count - count // 2])

        used = 0
        for cell in single:
            add_cell(cell, 1); used += 1
        for j, cell in enumerate(few):
            add_cell(cell, 5 + 32 * j); used += 5 + 32 * j
        if layout == "spread":
            n_rec = min(n_norm_pts - used, POOL - N_OFF - 2 * len(single + few)) if pooled else n_norm_pts - used
            t = rng.random((n_rec, 3)) * 1.05 - 0.025              # a box 5 % larger: some points are clamped
            while True:
                bad = self._near(t, single + few, W)
                if not bad.any():
                    break
                t[bad] = rng.random((int(bad.sum()), 3)) * 1.05 - 0.025
            counts = rng.multinomial(n_norm_pts - used, np.full(n_rec, 1.0 / n_rec)) if pooled else np.ones(n_rec)
            add(lo64 + t * ext64, counts)
        else:
            if L > 0:
                for cz in range(C):
                    for cy in range(C):
                        for cx in range(C):
                            cell = (cx, cy, cz)
                            if cell == self.clump or cell in single or cell in few:
                                continue
                            c = int(rng.integers(1, 60))            # (up to 4 off points land on top)
                            add_cell(cell, c); used += c
            n_clump = n_norm_pts - used
            if (n_clump + 6) % 64 == 0:                            # (6 off points are in the clump's cell)
                add_cell(few[0] if few else self.clump, 1); n_clump -= 1
            n_rec = min(n_clump, POOL - N_OFF - sum(len(r) for r in recs)) if pooled else n_clump
            counts = rng.multinomial(n_clump, np.full(n_rec, 1.0 / n_rec)) if pooled else np.ones(n_rec)
            add(in_cell(self.clump, rng.random((n_rec, 3))), counts)
        pos = np.concatenate(recs).astype(F32)
        mult = np.concatenate(mult)
        assert mult.sum() == n_norm_pts and len(pos) + N_OFF <= (POOL if pooled else m)
        r_max = R_MAX[0 if layout == "spread" else 1 + (m >= GRID_THREADS - 1)]
        radii = np.exp(rng.uniform(np.log(1e-3), np.log(r_max), len(pos))).astype(F32)
        # off points: a NaN / +inf / -inf coordinate, a negative / NaN / +inf radius, two of each, at positions
        # 0.75 + a little of the box (the clump's cell) where the coordinate is finite
        off_pos = np.empty((N_OFF, 3), F32)
        off_r = np.full(N_OFF, 0.02, F32)
        for j in range(N_OFF):
            off_pos[j] = (lo64 + (0.75 + 0.002 * (j + 1)) * ext64).astype(F32)
            kind = j % 6
            if kind == 0: off_pos[j, 0] = np.nan
            if kind == 1: off_pos[j, 1] = np.inf
            if kind == 2: off_pos[j, 2] = -np.inf
            if kind == 3: off_r[j] = -0.5
            if kind == 4: off_r[j] = np.nan
            if kind == 5: off_r[j] = np.inf
        self.off_at = np.array([0, 1, 63, 64, 65, 1000, m // 3, m // 2, m // 2 + 1, m - 65, m - 2, m - 1])
        assert len(np.unique(self.off_at)) == N_OFF
        n_norm = len(pos)
        self.rec_points = np.concatenate([pos, off_pos])
        self.rec_radii = np.concatenate([radii, off_r])
        index = np.empty(m, np.int64)
        is_off = np.zeros(m, bool); is_off[self.off_at] = True
        index[self.off_at] = n_norm + np.arange(N_OFF)
        index[~is_off] = rng.permutation(np.repeat(np.arange(n_norm), mult))
        self.index = index
        self.n_rec = len(self.rec_points)

    @staticmethod
    def _near(t, cells, W):
        """Whether a point at box fraction t (clamped as the kernel clamps) is in one of `cells` or within 1e-3 of
        the box of it."""
        tc = np.clip(t, 0.0, 1.0)
        a_lo = np.floor(np.clip(tc - 1e-3, 0.0, 1.0) / W)
        a_hi = np.floor(np.clip(tc + 1e-3, 0.0, 1.0) / W)
        bad = np.zeros(len(t), bool)
        for cell in cells:
            c = np.asarray(cell, np.float64)
            bad |= np.all((a_lo <= c) & (c <= a_hi), axis=1)
        return bad

    @property
    def points(self):
        return self.rec_points[self.index]

    @property
    def radii(self):
        return self.rec_radii[self.index]


_scene_cache = {}


def scene_and_box():
    if "s" not in _scene_cache:
        s = make_scene()
        _scene_cache["s"] = (s, *root_box(s))
    return _scene_cache["s"]


_set_cache = {}


def point_set(m, layout):
    if (m, layout) not in _set_cache:
        _, lo, hi = scene_and_box()
        _set_cache[(m, layout)] = PointSet(m, layout, lo, hi)
    return _set_cache[(m, layout)]


def expand_lists(lists, index):
    """The CSR lists of the records -> those of the points index[p] (offsets int64)."""
    counts, offsets, idx, d2 = lists
    cm = counts[index].astype(np.int64)
    om = np.zeros(len(index) + 1, np.int64)
    np.cumsum(cm, out=om[1:])
    src = np.repeat(offsets[index].astype(np.int64) - om[:-1], cm) + np.arange(om[-1])
    return cm.astype(np.int32), om, idx[src], d2[src]


# ---- CPU ------------------------------------------------------------------------------------------
def test_key_restatement():
    lo, hi = np.zeros(3, F32), np.ones(3, F32)
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, -1, np.nan], [np.inf, -np.inf, 0.5],
                    [1.0 / 1023, 0, 0], [0.5, 0.5, 0.5]], F32)
    keys = restate_keys(pts, lo, hi)
    x_all = 0x09249249                                             # 1023 spread over every third bit
    assert keys[:4].tolist() == [0, x_all, x_all << 1, x_all << 2]
    assert keys[4] == x_all and keys[5] == (x_all | _spread_bits(np.array([511]))[0] << 2)
    assert keys[6] in (0, 1)                                       # fl(fl(1 / 1023) * 1023) is 1 or just below
    assert keys[7] == 7 * _spread_bits(np.array([511]))[0]
    assert restate_cells(pts[7:], lo, hi, 1)[0] == 0 and restate_cells(pts[1:2], lo, hi, 1)[0] == 1
    assert cell_of(1, 0, 0, 1) == 1 and cell_of(0, 1, 0, 1) == 2 and cell_of(3, 3, 3, 2) == 63
    assert [cell_level(m) for m in (1, 2047, 2048, 16383, 16384, 131071, 131072, 1048575, 1048576, 8388607)] \
        == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]


def test_list_expansion_is_the_restatement_of_the_expanded_points():
    s, lo, hi = scene_and_box()
    rng = np.random.default_rng(6)
    rec = (lo + rng.random((40, 3)) * (hi - lo)).astype(F32)
    r = np.exp(rng.uniform(np.log(1e-2), np.log(0.3), 40)).astype(F32)
    r[3] = np.nan; rec[5, 1] = np.inf
    index = rng.integers(0, 40, 300)
    got = expand_lists(restate(rec, r, s), index)
    ref = restate(rec[index], r[index], s)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1].astype(np.int64))
    assert np.array_equal(got[2], ref[2]) and _same(got[3], ref[3]) and got[0].max() > 64 and got[0].min() == 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m", SIZES)
def test_point_sets_are_sharp(m, layout):
    """The inputs reach what they are for: the intended cell level on both sides of each threshold, ragged
    packets (cells of one point, of 2 to 63, and of more than 64 that are no multiple of 64), one cell with
    at least half of the points in the clumped layout, off points first and last in caller order."""
    s, lo, hi = scene_and_box()
    ps = point_set(m, layout)
    pts, r = ps.points, ps.radii
    assert pts.shape == (m, 3) and pts.dtype == F32 and r.shape == (m,)
    want = {2047: 0, 2048: 1, 2049: 1, 16383: 1, 16384: 2, 16385: 2, 131071: 2, 131072: 3, 131073: 3,
            262143: 3, 262144: 3, 262145: 3, 1048575: 3, 1048576: 4, 1048577: 4, 1048576 + 4097: 4}[m]
    assert ps.level == want
    assert (m >= BUCKET_SORT) == (m in SIZES[10:]) and (m > GRID_THREADS) == (m in SIZES[14:])
    # off points, first and last included
    finite = np.all(np.isfinite(pts), axis=1)
    with np.errstate(invalid="ignore"):
        good_r = (r >= 0) & (r < np.inf)
    assert not finite[0] and not good_r[m - 1] and (~finite).sum() == 6 and (~good_r).sum() == 6
    assert np.isnan(pts[:, 0]).sum() == 2 and np.isposinf(pts[:, 1]).sum() == 2 and np.isneginf(pts[:, 2]).sum() == 2
    assert np.isnan(r).sum() == 2 and np.isposinf(r).sum() == 2 and (r < 0).sum() == 2
    if m < 131071:
        assert ps.n_rec == m and len(np.unique(pts[finite], axis=0)) == finite.sum()   # all positions distinct
    else:
        assert ps.n_rec <= POOL
    if layout == "spread":                                         # some points are outside the box
        outside = np.any((pts[finite] < lo) | (pts[finite] > hi), axis=1)
        assert 0.02 < outside.mean() < 0.3
    cells = restate_cells(pts, lo, hi, ps.level)
    pop = np.bincount(cells, minlength=1 << (3 * ps.level))
    if ps.level == 0:
        assert len(pop) == 1
        return
    single, few = _reserved(ps.level)
    for cell in single:
        assert pop[cell_of(*cell, ps.level)] == 1
    for cell in few:
        assert 2 <= pop[cell_of(*cell, ps.level)] <= 63
    big = pop[pop > 64]
    assert len(big) and np.any(big % 64 != 0)
    n_packets = int(np.sum((pop + 63) // 64))
    assert n_packets > (m + 63) // 64                              # more packets than a cut every 64 points gives
    assert n_packets <= (m + 63) // 64 + (1 << (3 * ps.level))
    if layout == "clumped":
        k = cell_of(*ps.clump, ps.level)
        assert pop[k] >= m // 2 and pop[k] % 64 != 0
        rest = np.delete(pop, k)
        assert rest.min() >= 1 and rest.max() <= 63                # the sparse tail: one ragged packet per cell
    else:
        assert np.mean(big % 64 != 0) > 0.5


# ---- references, computed once per (size, layout) and family ---------------------------------------------
def weights(n, n_ch):
    return (0.5 + np.random.default_rng(40 + n_ch).random((n, n_ch))).astype(F32)


_ref_cache = {}


def reference(ps, sh, what):
    """The restatement of family `what` on the records of point set ps against the spheres sh (tree order)."""
    key = (ps.m, ps.layout, what)
    if key in _ref_cache:
        return _ref_cache[key]
    P, r = ps.rec_points, ps.rec_radii
    with np.errstate(all="ignore"):
        if what == "lists":
            res = restate(P, r, sh)
        elif what == "shared":
            res = restate(P, np.full(len(P), R_SHARED, F32), sh)[0]
        elif what.startswith("sums:"):
            res = restate_sums(P, r, sh, weights(len(sh), 5), what[5:], reference(ps, sh, "lists"))
        elif what.startswith("knn:"):
            res = brute_knn(P, sh, int(what[4:]))
        elif what == "field":
            out, counts, _, _ = restate_field(len(P), field_pairs(P, sh), sh, weights(len(sh), 2), "cubic")
            res = (out, counts)
        elif what == "pairs":
            (_, counts, sums), = restate_pairs(P, [EDGES], sh, weights(len(sh), 2))
            res = (counts, sums)
        else:
            raise KeyError(what)
    _ref_cache[key] = res
    return res


# ---- GPU --------------------------------------------------------------------------------------------
def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _i32(shape, cuda):
    import torch
    return torch.full(shape, -7, dtype=torch.int32, device=cuda)


def _f32(shape, cuda):
    import torch
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=cuda).view(torch.float32)


def _eq(got, ref, what):
    """Bitwise equality of 32-bit arrays, with the first differing slots in the message."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    g, r = got.reshape(-1).view(np.uint32), ref.reshape(-1).view(np.uint32)
    bad = np.nonzero(g != r)[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got.reshape(-1)[bad[:5]], ref.reshape(-1)[bad[:5]])


@pytest.fixture(scope="module")
def scenes(gh, cuda):
    """{max_per_leaf: (spheres in tree order, tree)} and the spheres on the host (the same order in both)."""
    s, lo, hi = scene_and_box()
    built = {mpl: _build(gh, s, cuda, mpl) for mpl in (8, 1)}
    sh = built[8][0].cpu().numpy()
    assert np.array_equal(built[1][0].cpu().numpy(), sh)
    return built, sh


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


def run_counts(gh, inp, d, tree, cuda, shared=False, n_ch=5, period=None):
    """range_counts_sph into pre-filled buffers -> (counts, sums or None)."""
    pd, rd, wd = inp["points"], inp["radii"], inp["w5"]
    m = len(pd)
    cnt = _i32((m,), cuda)
    if shared:
        gh.range_counts_sph(pd, float(R_SHARED), d, tree, counts=cnt, check=True, period=period)
        return cnt.cpu().numpy(), None
    out = _f32((m, n_ch), cuda)
    gh.range_counts_sph(pd, rd, d, tree, weights=wd, counts=cnt, out=out, check=True, period=period)
    return cnt.cpu().numpy(), out.cpu().numpy()


def run_lists(gh, inp, d, tree, cuda, total, period=None):
    """The count, scan, fill sequence of range_neighbours_sph through the C ABI, into pre-filled buffers of
    the restated total -> (counts, offsets, indices, d2); stops after the counts if their sum is not `total`.
    period: the periodic entry points (the period goes before the stream)."""
    import ctypes as C
    pd, rd = inp["points"], inp["radii"]
    m = len(pd)
    offsets = _i32((m + 1,), cuda)
    offsets[m] = 0
    args = (gh._ptr(pd), C.c_size_t(m), C.c_int(pd.shape[1]), gh._ptr(rd), C.c_float(0.0), *gh._interp_scene(d, tree))
    if period is None:
        count_fn, fill_fn, tail = gh._lib.grace_range_counts_f4, gh._lib.grace_range_neighbours_f4, (gh._stream(),)
    else:
        per = np.ascontiguousarray(period, F32)
        count_fn, fill_fn = gh._lib.grace_range_counts_periodic_f4, gh._lib.grace_range_neighbours_periodic_f4
        tail = (per.ctypes.data_as(C.c_void_p), gh._stream())
    assert count_fn(*args, gh._ptr(None), C.c_int(0), gh._ptr(offsets), gh._ptr(None), *tail) == gh.GRACE_OK
    counts = offsets[:m].cpu().numpy()
    if int(counts.astype(np.int64).sum()) != total or counts.min() < 0:
        return counts, None, None, None
    assert gh.exclusive_scan(offsets, offsets) == total
    idx, d2 = _i32((total + 64,), cuda), _f32((total + 64,), cuda)
    assert fill_fn(*args, gh._ptr(offsets), gh._ptr(idx), gh._ptr(d2), *tail) == gh.GRACE_OK
    gh.trace_status()
    gi, gd = idx.cpu().numpy(), d2.cpu().numpy()
    assert np.all(gi[total:] == -7) and np.all(gd[total:].view(np.uint32) == NAN_BITS)   # nothing past the end
    return counts, offsets.cpu().numpy(), gi[:total], gd[:total]


def run_knn(gh, inp, d, tree, cuda, k=K_SMALL, period=None):
    pd = inp["points"]
    idx, d2 = _i32((len(pd), k), cuda), _f32((len(pd), k), cuda)
    gh.nearest_neighbours_sph(pd, d, tree, k, indices=idx, d2=d2, check=True, period=period)
    return idx.cpu().numpy(), d2.cpu().numpy()


def run_field(gh, inp, d, tree, cuda, period=None):
    pd = inp["points"]
    out, cnt = _f32((len(pd), 2), cuda), _i32((len(pd),), cuda)
    gh.interpolate_sph(pd, d, tree, inp["w2"], out=out, counts=cnt, check=True, period=period)
    return out.cpu().numpy(), cnt.cpu().numpy()


def run_pairs(gh, inp, d, tree, cuda, profiles=True, period=None):
    """(totals uint64 [E], counts int32 [m, E] or None, sums float32 [m, E, 2] or None) into pre-filled buffers."""
    import torch
    pd = inp["points"]
    m, ne = len(pd), len(EDGES)
    edges = gh._pair_edges(EDGES)
    totals = torch.full((ne,), -7, dtype=torch.int64, device=cuda)
    gh._pair_call(pd, edges, d, tree, None, 0, totals, None, None, True, period)
    tot = totals.cpu().numpy().view(np.uint64)
    if not profiles:
        return tot, None, None
    cnt, sums = _i32((m, ne), cuda), _f32((m, ne, 2), cuda)
    gh._pair_call(pd, edges, d, tree, inp["w2"], 2, None, cnt, sums, True, period)
    return tot, cnt.cpu().numpy(), sums.cpu().numpy()


def inputs(ps, sh, cuda, elems=3):
    """The device inputs of a point set (made on the current stream: synchronise before using them on another)."""
    pts = ps.points
    if elems != 3:
        wide = np.full((ps.m, elems), 9.0, F32); wide[:, :3] = pts
        pts = wide
    return {"points": _dev(pts, cuda), "radii": _dev(ps.radii, cuda), "w5": _dev(weights(len(sh), 5), cuda),
            "w2": _dev(weights(len(sh), 2), cuda)}


def check_counts(ps, sh, got, kernel="cubic", shared=False):
    cnt, sums = got
    if shared:
        _eq(cnt, reference(ps, sh, "shared")[ps.index], (ps.m, ps.layout, "shared radius"))
        return
    _eq(cnt, reference(ps, sh, "lists")[0][ps.index], (ps.m, ps.layout, "counts"))
    _eq(sums, reference(ps, sh, "sums:" + kernel)[ps.index], (ps.m, ps.layout, "sums", kernel))


def check_lists(ps, sh, got):
    ref = expand_lists(reference(ps, sh, "lists"), ps.index)
    what = (ps.m, ps.layout, "lists")
    _eq(got[0], ref[0], what + ("counts",))
    assert got[1] is not None and np.array_equal(got[1].astype(np.int64), ref[1]), what + ("offsets",)
    _eq(got[2], ref[2], what + ("indices",))
    _eq(got[3], ref[3], what + ("d2",))


def check_knn(ps, sh, got, k=K_SMALL):
    ref_i, ref_d = reference(ps, sh, "knn:%d" % k)
    _eq(got[0], ref_i[ps.index], (ps.m, ps.layout, "knn indices", k))
    _eq(got[1], ref_d[ps.index], (ps.m, ps.layout, "knn d2", k))


def check_field(ps, sh, got):
    out, counts = reference(ps, sh, "field")
    _eq(got[1], counts[ps.index], (ps.m, ps.layout, "field counts"))
    _eq(got[0], out[ps.index], (ps.m, ps.layout, "field"))


def check_pairs(ps, sh, got):
    counts, sums = reference(ps, sh, "pairs")
    tot, cnt, sm = got
    ref_tot = counts[ps.index].sum(axis=0, dtype=np.int64).astype(np.uint64)
    assert tot.dtype == np.uint64 and np.array_equal(tot, ref_tot), (ps.m, ps.layout, "totals", tot, ref_tot)
    if cnt is not None:
        _eq(cnt, counts[ps.index], (ps.m, ps.layout, "pair counts"))
        _eq(sm, sums[ps.index], (ps.m, ps.layout, "pair sums"))


def total_of(ps, sh):
    return int(reference(ps, sh, "lists")[0][ps.index].astype(np.int64).sum())


@pytest.mark.gpu
def test_the_restated_root_box_is_the_trees(gh, scenes, cuda):
    """The CPU test's cells are the kernel's: the box packet_keys_kernel reads from the root node is the
    restated one to within a few ulp -- far inside the margins of the point sets."""
    built, sh = scenes
    s, lo, hi = scene_and_box()
    for mpl in (8, 1):
        d, tree = built[mpl]
        root = int(tree.root_index.cpu()[0])
        node = tree.nodes[root].cpu().numpy().view(F32).reshape(4, 4)
        L, R, Z = node[1], node[2], node[3]
        t_lo = np.array([min(L[0], R[0]), min(L[2], R[2]), min(Z[0], Z[2])], F32)
        t_hi = np.array([max(L[1], R[1]), max(L[3], R[3]), max(Z[1], Z[3])], F32)
        assert np.allclose(t_lo, lo, rtol=0, atol=1e-6), (t_lo, lo)
        assert np.allclose(t_hi, hi, rtol=0, atol=1e-6), (t_hi, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m", SIZES)
def test_range_counts_and_gather_sums(gh, scenes, m, layout, cuda, kernel_reset):
    built, sh = scenes
    d, tree = built[8]
    ps = point_set(m, layout)
    inp = inputs(ps, sh, cuda)
    check_counts(ps, sh, run_counts(gh, inp, d, tree, cuda, shared=True), shared=True)
    check_counts(ps, sh, run_counts(gh, inp, d, tree, cuda))
    if m == 16385:
        gh.set_sph_kernel("wendland_c2")
        check_counts(ps, sh, run_counts(gh, inp, d, tree, cuda), kernel="wendland_c2")
    counts = reference(ps, sh, "lists")[0][ps.index]
    assert counts.min() == 0 and counts.max() > 64                 # rows from empty to beyond a wave of entries


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m", SIZES)
def test_range_lists(gh, scenes, m, layout, cuda):
    built, sh = scenes
    d, tree = built[8]
    ps = point_set(m, layout)
    total = total_of(ps, sh)
    assert total < 2 * 10 ** 7
    check_lists(ps, sh, run_lists(gh, inputs(ps, sh, cuda), d, tree, cuda, total))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m", SIZES)
def test_nearest_neighbours(gh, scenes, m, layout, cuda):
    built, sh = scenes
    d, tree = built[8]
    ps = point_set(m, layout)
    inp = inputs(ps, sh, cuda)
    for k in (K_SMALL, K_LARGE) if m <= 16385 else (K_SMALL,):
        got = run_knn(gh, inp, d, tree, cuda, k)
        check_knn(ps, sh, got, k)
        off = ps.off_at[::6]                                       # the padding rows of a non-finite point
        assert np.all(got[0][off] == -1) and np.all(np.isposinf(got[1][off]))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m", SIZES)
def test_interpolation_at_points(gh, scenes, m, layout, cuda):
    built, sh = scenes
    d, tree = built[8]
    ps = point_set(m, layout)
    check_field(ps, sh, run_field(gh, inputs(ps, sh, cuda), d, tree, cuda))
    counts = reference(ps, sh, "field")[1]
    assert counts.min() == 0 and counts.max() > 64


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("m", SIZES)
def test_pair_counts_and_profiles(gh, scenes, m, layout, cuda):
    built, sh = scenes
    d, tree = built[8]
    ps = point_set(m, layout)
    check_pairs(ps, sh, run_pairs(gh, inputs(ps, sh, cuda), d, tree, cuda))
    assert np.all(reference(ps, sh, "pairs")[0].sum(axis=0) > 0)   # every bin holds pairs


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["counts", "lists", "knn", "field", "pairs"])
def test_max_per_leaf_1(gh, scenes, family, cuda):
    """The same spheres as a tree of single-sphere leaves (the coincident group is a spine of 100)."""
    built, sh = scenes
    d, tree = built[1]
    ps = point_set(16385, "clumped")
    inp = inputs(ps, sh, cuda)
    if family == "counts":
        check_counts(ps, sh, run_counts(gh, inp, d, tree, cuda))
    elif family == "lists":
        check_lists(ps, sh, run_lists(gh, inp, d, tree, cuda, total_of(ps, sh)))
    elif family == "knn":
        check_knn(ps, sh, run_knn(gh, inp, d, tree, cuda))
    elif family == "field":
        check_field(ps, sh, run_field(gh, inp, d, tree, cuda))
    else:
        check_pairs(ps, sh, run_pairs(gh, inp, d, tree, cuda))


def fof_linking(n):
    """Coincident centres only, and a length at which the blobs link up while the background stays loose."""
    return [F32(0.0), F32(0.4 * n ** (-1.0 / 3.0))]


@pytest.mark.gpu
@pytest.mark.parametrize("n", FOF_SIZES)
def test_friends_of_friends_across_the_thresholds(gh, n, cuda):
    """Here the points are the particles: scenes of n particles on both sides of the level steps."""
    d, tree = _build(gh, make_scene(n, seed=n), cuda, 8)
    sh = d.cpu().numpy()
    bs = fof_linking(n)
    ref = restate_labels(sh, bs)
    for b, ref_labels in zip(bs, ref):
        labels = _i32((n,), cuda)
        gh.fof_labels_sph(d, tree, float(b), labels=labels, check=True)
        _eq(labels.cpu().numpy(), ref_labels, (n, b, "labels"))
        got = tuple(t.cpu().numpy() for t in gh.fof_groups_sph(labels, 2))
        for name, g, r in zip(("group_of", "sizes", "offsets", "members"), got, restate_catalogue(ref_labels, 2)):
            _eq(g, r, (n, b, name))
    sizes = np.bincount(ref[1])
    assert np.bincount(ref[0]).max() == 100 and sizes.max() > 200 and np.sum(sizes == 1) > n // 10


@pytest.mark.gpu
def test_repeated_clumped_calls_take_the_hinted_sort(gh, scenes, cuda):
    """Three calls in a row on one context with the sort's overflow hint on: the clump overflows its bucket on
    the first, the later ones skip the bucket sort.  The same bits every time, and the restatement's."""
    import torch
    built, sh = scenes
    d, tree = built[8]
    ps = point_set(262145, "clumped")
    inp = inputs(ps, sh, cuda)
    torch.cuda.synchronize()
    gh.set_sort_overflow_hint(True)
    try:
        with gh.Context():
            for rep in range(3):
                check_counts(ps, sh, run_counts(gh, inp, d, tree, cuda))
                check_knn(ps, sh, run_knn(gh, inp, d, tree, cuda))
                torch.cuda.synchronize()
    finally:
        gh.set_sort_overflow_hint(False)


# ---- B: wide points through the C ABI --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("elems", [3, 4, 7])
@pytest.mark.parametrize("m", [131073, 262145])
def test_wide_points(gh, scenes, m, elems, cuda):
    """elems_per_point 3, 4 and 7 (the unused columns hold 9.0) on each side of the bucket sort's threshold:
    grace_range_counts_f4, grace_nearest_neighbours_f4 and grace_pair_counts_f4 read x y z alone."""
    built, sh = scenes
    d, tree = built[8]
    ps = point_set(m, "clumped")
    inp = inputs(ps, sh, cuda, elems)
    assert inp["points"].shape[1] == elems                          # (the bindings pass it on as elems_per_point)
    check_counts(ps, sh, run_counts(gh, inp, d, tree, cuda))
    check_knn(ps, sh, run_knn(gh, inp, d, tree, cuda))
    check_pairs(ps, sh, run_pairs(gh, inp, d, tree, cuda))


# ---- C: streams and contexts -----------------------------------------------------------------------------
M_CONTEXT = 3003
GRID = dict(dims=(24, 20, 3))
FAMILIES = ("interpolate", "interpolate_grid", "neighbours", "smoothing_lengths", "range_counts", "range_lists",
            "fof", "pairs")


def run_family(gh, family, ps, inp, d, tree, sh, cuda):
    """One family's call on the current context and stream -> a tuple of host arrays."""
    if family == "interpolate":
        return run_field(gh, inp, d, tree, cuda)
    if family == "interpolate_grid":
        s, lo, hi = scene_and_box()
        nx, ny, nz = GRID["dims"]
        step = (hi - lo) / np.array([nx, ny, nz], F32)
        out, cnt = _f32((nz, ny, nx, 2), cuda), _i32((nz, ny, nx), cuda)
        gh.interpolate_grid_sph(lo + step / 2, (step[0], 0, 0), (0, step[1], 0), (0, 0, step[2]), (nx, ny, nz), d, tree,
                                inp["w2"], out=out, counts=cnt, check=True)
        return out.cpu().numpy(), cnt.cpu().numpy()
    if family == "neighbours":
        return run_knn(gh, inp, d, tree, cuda)
    if family == "smoothing_lengths":
        h = _f32((len(sh),), cuda)
        gh.smoothing_lengths_sph(d, tree, 16, 1.2, out=h, check=True)
        return (h.cpu().numpy(),)
    if family == "range_counts":
        gh.set_sph_kernel("wendland_c2")                            # (a fresh context starts with the cubic kernel)
        return run_counts(gh, inp, d, tree, cuda)
    if family == "range_lists":
        return run_lists(gh, inp, d, tree, cuda, total_of(ps, sh))
    if family == "fof":
        labels = _i32((len(sh),), cuda)
        gh.fof_labels_sph(d, tree, 0.02, labels=labels, check=True)
        return (labels.cpu().numpy(), *(t.cpu().numpy() for t in gh.fof_groups_sph(labels, 2)))
    if family == "pairs":
        return run_pairs(gh, inp, d, tree, cuda)
    raise KeyError(family)


def in_own_context(gh, fn):
    """fn() inside a context and a stream of its own."""
    import torch
    torch.cuda.synchronize()                                       # the inputs are complete for any stream
    stream = torch.cuda.Stream()
    ctx = gh.Context()
    try:
        ctx.make_current()
        with torch.cuda.stream(stream):
            got = fn()
            stream.synchronize()
    finally:
        gh.Context.reset_current()
        ctx.destroy()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_a_context_with_its_own_stream_gives_the_same_bits(gh, scenes, family, cuda, kernel_reset):
    built, sh = scenes
    d, tree = built[8]
    ps = point_set(M_CONTEXT, "spread")
    assert ps.level == 1
    inp = inputs(ps, sh, cuda)
    base = run_family(gh, family, ps, inp, d, tree, sh, cuda)
    # the default context's result is the restatement's (or, for the families the restatements above do not
    # cover at these inputs, the expected value as it stands: their own modules tie them to theirs)
    if family == "interpolate":
        check_field(ps, sh, base)
    elif family == "neighbours":
        check_knn(ps, sh, base)
    elif family == "range_counts":
        check_counts(ps, sh, base, kernel="wendland_c2")
    elif family == "range_lists":
        check_lists(ps, sh, base)
    elif family == "pairs":
        check_pairs(ps, sh, base)
    elif family == "fof":
        _eq(base[0], restate_labels(sh, [F32(0.02)])[0], "fof labels")
    got = in_own_context(gh, lambda: run_family(gh, family, ps, inp, d, tree, sh, cuda))
    assert len(got) == len(base)
    for k, (g, b) in enumerate(zip(got, base)):
        if g.dtype == np.uint64:
            assert np.array_equal(g, b), (family, k)
        else:
            _eq(g, b, (family, k))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_fresh_contexts_side_stream_carries_the_bucket_sort(gh, scenes, layout, cuda):
    """262145 points: the nested sort forks onto the context's side stream and joins it again (clumped: the
    gated fallback runs there) -- on a context and a stream that have never run anything before."""
    built, sh = scenes
    d, tree = built[8]
    ps = point_set(262145, layout)
    inp = inputs(ps, sh, cuda)
    base_c, base_k = run_counts(gh, inp, d, tree, cuda), run_knn(gh, inp, d, tree, cuda)
    check_counts(ps, sh, base_c)
    check_knn(ps, sh, base_k)
    for fn, base in ((lambda: run_counts(gh, inp, d, tree, cuda), base_c),
                     (lambda: run_knn(gh, inp, d, tree, cuda), base_k)):
        got = in_own_context(gh, fn)                               # a fresh context each
        for g, b in zip(got, base):
            _eq(g, b, (layout, "own context"))


@pytest.mark.gpu
def test_point_queries_on_alternating_streams_share_the_workspace_safely(gh, scenes, cuda):
    """Two point sets on either side of a level step (their frames are laid out differently), six calls
    back to back alternating between two streams without a host synchronisation in between: the frame fence
    alone keeps the second call's keys and packets off the first call's."""
    import ctypes as C
    import torch
    built, sh = scenes
    d, tree = built[8]
    sets = (point_set(2047, "spread"), point_set(2049, "clumped"))
    inps = [inputs(ps, sh, cuda) for ps in sets]
    streams = (torch.cuda.Stream(), torch.cuda.Stream())
    # range counts with sums, then k nearest neighbours
    outs = [(_i32((sets[rep % 2].m,), cuda), _f32((sets[rep % 2].m, 5), cuda)) for rep in range(6)]
    torch.cuda.synchronize()
    for rep in range(6):
        inp = inps[rep % 2]
        with torch.cuda.stream(streams[rep % 2]):
            gh.range_counts_sph(inp["points"], inp["radii"], d, tree, weights=inp["w5"], counts=outs[rep][0],
                                out=outs[rep][1])
    torch.cuda.synchronize()
    for rep in range(6):
        check_counts(sets[rep % 2], sh, (outs[rep][0].cpu().numpy(), outs[rep][1].cpu().numpy()))
    gh.trace_status()
    outs = [(_i32((sets[rep % 2].m, K_SMALL), cuda), _f32((sets[rep % 2].m, K_SMALL), cuda)) for rep in range(6)]
    torch.cuda.synchronize()
    for rep in range(6):
        with torch.cuda.stream(streams[rep % 2]):
            gh.nearest_neighbours_sph(inps[rep % 2]["points"], d, tree, K_SMALL, indices=outs[rep][0], d2=outs[rep][1])
    torch.cuda.synchronize()
    for rep in range(6):
        check_knn(sets[rep % 2], sh, (outs[rep][0].cpu().numpy(), outs[rep][1].cpu().numpy()))
    gh.trace_status()
    # the split list sequence: counts on stream 1, scan and fill on stream 2 (after stream 1, for the caller's
    # own dependency on the counts), an unrelated query on stream 1 in between
    ps, inp, other = sets[1], inps[1], inps[0]
    total = total_of(ps, sh)
    m = ps.m
    offsets = _i32((m + 1,), cuda); offsets[m] = 0
    idx, d2 = _i32((total,), cuda), _f32((total,), cuda)
    ki, kd = _i32((sets[0].m, K_SMALL), cuda), _f32((sets[0].m, K_SMALL), cuda)
    torch.cuda.synchronize()
    pd, rd = inp["points"], inp["radii"]
    args = (gh._ptr(pd), C.c_size_t(m), C.c_int(3), gh._ptr(rd), C.c_float(0.0), *gh._interp_scene(d, tree))
    with torch.cuda.stream(streams[0]):
        assert gh._lib.grace_range_counts_f4(*args, gh._ptr(None), C.c_int(0), gh._ptr(offsets), gh._ptr(None),
                                             gh._stream()) == gh.GRACE_OK
    streams[1].wait_stream(streams[0])
    with torch.cuda.stream(streams[0]):
        gh.nearest_neighbours_sph(other["points"], d, tree, K_SMALL, indices=ki, d2=kd)
    with torch.cuda.stream(streams[1]):
        assert gh.exclusive_scan(offsets, offsets) == total
        assert gh._lib.grace_range_neighbours_f4(*args, gh._ptr(offsets), gh._ptr(idx), gh._ptr(d2),
                                                 gh._stream()) == gh.GRACE_OK
    torch.cuda.synchronize()
    gh.trace_status()
    ref = expand_lists(reference(ps, sh, "lists"), ps.index)
    assert np.array_equal(offsets.cpu().numpy().astype(np.int64), ref[1])
    _eq(idx.cpu().numpy(), ref[2], "split lists: indices")
    _eq(d2.cpu().numpy(), ref[3], "split lists: d2")
    check_knn(sets[0], sh, (ki.cpu().numpy(), kd.cpu().numpy()))


@pytest.mark.gpu
def test_two_contexts_two_threads_run_point_queries_on_one_gpu(gh, scenes, cuda):
    """Each thread has a context and a stream of its own: one loops range counts and lists, the other k nearest
    neighbours and pair counts; every iteration gives the single-threaded reference's bits."""
    import torch
    built, sh = scenes
    d, tree = built[8]
    sets = (point_set(16385, "clumped"), point_set(16384, "spread"))
    inps = [inputs(ps, sh, cuda) for ps in sets]
    for ps in sets:                                                # (the references, before the threads start)
        reference(ps, sh, "lists"); reference(ps, sh, "sums:cubic"); reference(ps, sh, "knn:%d" % K_SMALL)
        reference(ps, sh, "pairs")
    total = total_of(sets[0], sh)
    torch.cuda.synchronize()
    errors = []

    def worker(k):
        try:
            torch.cuda.set_device(cuda)
            with gh.Context():
                stream = torch.cuda.Stream(device=cuda)
                with torch.cuda.stream(stream):
                    for it in range(3):
                        if k == 0:
                            check_counts(sets[0], sh, run_counts(gh, inps[0], d, tree, cuda))
                            check_lists(sets[0], sh, run_lists(gh, inps[0], d, tree, cuda, total))
                        else:
                            check_knn(sets[1], sh, run_knn(gh, inps[1], d, tree, cuda))
                            check_pairs(sets[1], sh, run_pairs(gh, inps[1], d, tree, cuda))
                    stream.synchronize()
                    gh.trace_status()
        except BaseException as e:      # noqa: BLE001 -- reported to the main thread
            errors.append((k, repr(e)[:2000]))

    threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a worker did not finish"
    assert not errors, errors
    check_counts(sets[0], sh, run_counts(gh, inps[0], d, tree, cuda))   # the default context afterwards
