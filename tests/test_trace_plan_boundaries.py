"""The planned column-density kernels against brute force at the edges of the recorder's cull.

plan_record_kernel (csrc/trace_planned.hip) carries its own text of the group and cluster box
tests, the beam bound, the origin-lattice cull, the lean and fat decisions and the dense-round
grouping, and the PLANNED consumer trusts what it recorded.  The boundary scenes
(trace_boundary_scenes.py) put radius twins and range twins against the extreme rays of packets;
here they are traced from a plan ON PURPOSE: every case asserts through last_plan_used() that the
planned kernel ran, and holds both the ordinary kernels (set_plan(False)) and the planned ones
against brute force on the scene's sub-sample of rays, and against each other on all rays.

A grazing radius twin contributes at most 5.64e-11 / h^2 to a sum whose other terms are ~1.9 / h^2
each: no unweighted or randomly weighted column density can see whether it was dropped.  The
SPOTLIGHT weights (B.spotlight_weights) are 0 on everything but the twins in channels 1, 2 and 4,
so that a ray's value there is the fp32 sum of its twins' terms alone; every scene has at least 100
radius hit twins whose term is nonzero (asserted on the CPU in test_trace_boundary_scenes.py, and
on the reference here).

Exact integrals: unweighted sums are the oracle's fp32 sum bit for bit, weighted sums are
test_weighted_column_density.restate()'s in every channel.  Fast integrals: the unweighted trace
and channel 0 stay within conftest.check_column_densities' bounds, planned == ordinary bit for bit;
no claim on channels 1 and 2 against brute force there (a grazing term is a few ulp of the table
position)."""
import numpy as np
import pytest

import trace_boundary_scenes as B
from conftest import check_column_densities

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
F0 = 1.91            # the kernel table's first entry, rounded up: the largest line integral times h^2


def _reset(gh):
    gh.set_ray_reorder(True); gh.set_packet_split(-1); gh.set_packet_width(-1)
    gh.set_exact_integrals(False); gh.set_plan(True); gh.set_cache_auto(True)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _plan_off(gh, call):
    """The call with the plan switched off: the ordinary kernels, whatever the caches hold."""
    gh.set_plan(False)
    try:
        out = call()
        assert gh.last_plan_used() == 0 and gh.plan_bytes() == 0
    finally:
        gh.set_plan(True)
    return out


def _from_plan(gh, call):
    """The call once a plan serves it: the third call on the same arrays at the latest (a call that
    traces twice -- more than four channels -- has its caches one call earlier); once more, from
    the plan again, with the same bits."""
    for _ in range(3):
        out = call()
        if gh.last_plan_used() == 1:
            break
    assert gh.last_plan_used() == 1
    again = call()
    assert gh.last_plan_used() == 1
    assert np.array_equal(_bits(out), _bits(again))
    return again


class _Traced:
    """A scene on the device: sorted spheres, tree, rays, weights in tree order, and its
    brute-force references on sc.sub (computed once, for both integrals and both paths)."""

    def __init__(self, gh, oracle, cuda, sc, mpl, n_channels, seed=7):
        import torch
        from test_weighted_column_density import restate
        self.gh, self.sc, self.cuda = gh, sc, cuda
        s = sc.spheres
        self.d = torch.from_numpy(np.ascontiguousarray(s)).to(cuda)
        self.tree, perm = gh.build_tree(self.d, gh.Tree(len(s), mpl, device=cuda), tuple(s[:, :3].min(axis=0)),
                                        tuple(s[:, :3].max(axis=0)), want_perm=True)
        self.perm = perm.cpu().numpy().astype(np.int64)       # perm[j]: the caller's index of sorted sphere j
        self.rays = torch.from_numpy(sc.rays).to(cuda)
        self.w_host = B.spotlight_weights(sc, n_channels, seed)[self.perm] if n_channels else None
        self.w = torch.from_numpy(self.w_host).to(cuda) if n_channels else None
        self.restate = restate
        self.refresh(oracle)

    def refresh(self, oracle):
        """(Re)computes the references from the spheres as they are on the device now."""
        ss = self.d.cpu().numpy()
        rr = self.sc.rays[self.sc.sub]
        self.ss = ss
        self.c32, self.c64 = oracle.brute_cumulative(rr, ss)
        self.max_term = F0 / float(ss[:, 3].min()) ** 2
        self.hits = oracle.brute_hits(rr, ss)
        if self.w is not None:
            self.w32 = self.reference(self.w_host)

    def reference(self, w_host):
        ro, ri, rw, _ = self.hits
        return self.restate(len(self.sc.sub), ro, ri, rw, w_host)[0]

    def unweighted(self):
        import torch
        out = torch.empty(len(self.rays), dtype=torch.float32, device=self.cuda)
        self.gh.trace_cumulative_sph(self.rays, self.d, self.tree, out, check=True)
        return out

    def weighted(self, w=None):
        return self.gh.trace_cumulative_weighted_sph(self.rays, self.d, self.tree, self.w if w is None else w,
                                                     check=True)

    def check_unweighted(self, got, exact):
        check_column_densities(got.cpu().numpy()[self.sc.sub], self.c32, self.c64, "exact" if exact else "fast",
                               self.max_term)

    def check_weighted(self, got, exact):
        g = got.cpu().numpy()[self.sc.sub]
        assert g.shape == self.w32.shape
        if exact:
            for c in range(g.shape[1]):
                bad = np.nonzero(g[:, c].view(np.uint32) != self.w32[:, c].view(np.uint32))[0]
                assert len(bad) == 0, ("channel", c, self.sc.sub[bad[:5]], g[bad[:5], c], self.w32[bad[:5], c])
        elif g.shape[1] > 1:         # (one channel is the twins' channel alone: no claim in fast mode)
            check_column_densities(g[:, 0], self.c32, self.c64, "fast", self.max_term)


def _both_paths(gh, t, planned=True):
    """Both integrals, the unweighted and the weighted trace: ordinary and planned kernels against
    brute force, and against each other bit for bit on every ray.  planned=False: the batch is
    unplannable by design, and must say so."""
    for exact in (True, False):
        gh.set_exact_integrals(exact)
        for call, check in ((t.unweighted, t.check_unweighted), (t.weighted, t.check_weighted)):
            if call == t.weighted and t.w is None:
                continue
            ordinary = _plan_off(gh, call)
            check(ordinary, exact)
            if planned:
                got = _from_plan(gh, call)
            else:
                for _ in range(4):
                    got = call()
                    assert gh.last_plan_used() == 0
            check(got, exact)
            assert np.array_equal(_bits(got), _bits(ordinary)), ("exact" if exact else "fast", call.__name__)


def _assert_not_blind(t):
    """On the reference alone: at least 100 sub-sample rays carry a nonzero sum of radius twins'
    terms, and (where the scene has range twins) of range twins' terms."""
    sc = t.sc
    ro, ri, rw, _ = t.hits
    n_hits = np.diff(np.append(ro, len(ri)))
    ray_of = np.repeat(np.arange(len(sc.sub)), n_hits)
    caller = t.perm[ri]
    radius = np.zeros(len(sc.spheres), bool); radius[sc.hit[:sc.n_radius]] = True
    rng_ = np.zeros(len(sc.spheres), bool); rng_[sc.hit[sc.n_radius:]] = True
    assert len(np.unique(ray_of[radius[caller] & (rw != 0)])) >= 100
    if len(sc.hit) > sc.n_radius:
        assert len(np.unique(ray_of[rng_[caller] & (rw != 0)])) >= 100
    missed = np.zeros(len(sc.spheres), bool); missed[sc.miss] = True
    assert not missed[caller].any()                # (and brute force hits no miss twin)


def _assert_twins(sc):
    h, m = B.twin_outcomes(sc)
    assert len(sc.hit) > 0 and h.all() and m.all(), "a twin is not on its side of the boundary"


# Six rows of B.PLAN_CASES switch the ray reordering off.  Such a batch is unplannable BY DESIGN
# ("packet plan": a plan lives "per context, beside the two caches and tied to
# their fills", and is sized by "the first call that both caches serve"; the ray cache holds "the
# order + extents of ONE ray batch", and a batch traced in the caller's order has no order to cache:
# trace.hip consults the ray cache only `if (p.reorder ...)`).  Those rows run as they stand and must
# say last_plan_used() == 0 on every call; each of them runs a second time with the reordering ON
# and everything else unchanged, and that run must be planned -- so every row's scene is traced from
# a plan: 3 rows as they stand, 6 through their reordered companions (15 runs, 9 of them planned).
PLAN_RUNS = [(c, False) for c in range(len(B.PLAN_CASES))] + \
    [(c, True) for c in range(len(B.PLAN_CASES)) if not B.PLAN_CASES[c][4]["reorder"]]


@pytest.mark.parametrize("case,reordered", PLAN_RUNS,
                         ids=["row%d%s" % (c + 1, "-reordered" if r else "") for c, r in PLAN_RUNS])
def test_planned_boundary_scene_equals_brute_force(gh, oracle, cuda, case, reordered):
    scale, axis, sense, opts, knobs, channels = B.PLAN_CASES[case]
    sc = B.plan_case_scene(case)
    _assert_twins(sc)
    assert len(sc.rays) <= 4096
    reorder = knobs["reorder"] or reordered
    with gh.Context():
        try:
            t = _Traced(gh, oracle, cuda, sc, knobs["mpl"], channels)
            _assert_not_blind(t)
            gh.set_packet_width(knobs["width"]); gh.set_ray_reorder(reorder)
            gh.set_packet_split(knobs["split"])
            _both_paths(gh, t, planned=reorder)
        finally:
            _reset(gh)


@pytest.mark.parametrize("scale", B.PLAN_LATTICE_SCALES)
def test_lattice_twins_from_a_plan(gh, oracle, cuda, scale):
    """Sub-pixel twins against the first and the 8th column and row of 8 x 8 tiles: the twins
    between columns 6 and 7 are kept only through the lattice's eighth value, in the recorder's own
    loop over the table.  The uncached call runs the LAT kernels (and says so); the planned call
    holds the lattice cull in its masks."""
    sc = B.plan_lattice_scene(scale)
    _assert_twins(sc)
    assert set(sc.lattice_cols.tolist()) >= {0, B.TILE - 1} and set(sc.lattice_rows.tolist()) >= {0, B.TILE - 1}
    with gh.Context():
        try:
            t = _Traced(gh, oracle, cuda, sc, 8, 4)
            _assert_not_blind(t)
            gh.set_cache_auto(False)
            gh.set_exact_integrals(True)
            got = t.unweighted()
            assert gh.last_lattice() == 1 and gh.last_plan_used() == 0
            t.check_unweighted(got, True)
            gh.set_cache_auto(True)
            _both_paths(gh, t)
        finally:
            _reset(gh)


def test_twins_swapped_in_place_are_recorded_again(gh, oracle, cuda):
    """The first row's scene under a plan (with the reordering on: see PLAN_RUNS); then, on the
    device, every radius hit twin exchanges its radius with its miss twin (same pointers, same
    sizes, the weights stay where they are).  The next call must notice, record again into the same
    room and equal brute force on the NEW arrays: the masks recorded before name the old hit twins,
    which now miss, and not the new ones.

    A pair shares its centre and both twins weigh 1 in channel 1, so the pair's term only moves
    from one index to the other: channel 1 itself cannot change (on the CPU: 0 of 290 nonzero
    values do).  What shows that the swap is seen is therefore a channel that is 1 on the radius
    HIT twins' indices alone: equal to channel 1 before the swap, zero after it."""
    import torch
    scale, axis, sense, opts, knobs, channels = B.PLAN_CASES[0]
    sc = B.plan_case_scene(0)
    nr = sc.n_radius
    with gh.Context():
        try:
            t = _Traced(gh, oracle, cuda, sc, knobs["mpl"], channels)
            gh.set_packet_width(knobs["width"]); gh.set_ray_reorder(True)
            gh.set_packet_split(knobs["split"]); gh.set_exact_integrals(True)
            hit_only = np.zeros((len(sc.spheres), 1), F32); hit_only[sc.hit[:nr]] = 1
            hit_only = hit_only[t.perm]
            w_hit = torch.from_numpy(hit_only).to(cuda)
            before = _from_plan(gh, t.weighted)
            t.check_weighted(before, True)
            before_hit = _from_plan(gh, lambda: t.weighted(w_hit))
            assert np.array_equal(_bits(before_hit)[:, 0], _bits(before)[:, 1])
            ref_hit_before = t.reference(hit_only)
            size = gh.plan_bytes()
            assert size > 0
            pos = np.empty(len(t.perm), np.int64); pos[t.perm] = np.arange(len(t.perm))
            ph = torch.from_numpy(pos[sc.hit[:nr]]).to(cuda); pm = torch.from_numpy(pos[sc.miss[:nr]]).to(cuda)
            rh, rm = t.d[ph, 3].clone(), t.d[pm, 3].clone()
            t.d[ph, 3] = rm; t.d[pm, 3] = rh
            got = t.weighted()
            assert gh.last_plan_used() == 1 and gh.plan_bytes() == size
            t.refresh(oracle)                                   # brute force on the arrays as they are now
            t.check_weighted(got, True)
            again = t.weighted()
            assert gh.last_plan_used() == 1 and gh.plan_bytes() == size
            assert np.array_equal(_bits(got), _bits(again))
            got_hit = t.weighted(w_hit)
            assert gh.last_plan_used() == 1
            ref_hit = t.reference(hit_only)
            assert np.array_equal(_bits(got_hit)[sc.sub], ref_hit.view(np.uint32))
            assert np.count_nonzero(ref_hit_before[:, 0]) >= 100 and not ref_hit.any()
            changed = _bits(got_hit)[:, 0] != _bits(before_hit)[:, 0]
            assert changed.sum() >= 100, int(changed.sum())
            plain = t.unweighted()
            assert gh.last_plan_used() == 1
            t.check_unweighted(plain, True)
            ordinary = _plan_off(gh, t.weighted)
            assert np.array_equal(_bits(ordinary), _bits(got))
        finally:
            _reset(gh)


# ---- the fat threshold ----------------------------------------------------------------------------
FAT_LEAD, FAT_COLUMN, FAT_TRAIL = 34, 60, 30      # sorted: 34 | 30 column || 30 column | 30


def _fat_scene(gh, cuda, rays, fat_first):
    """Under packet 0 (an 8 x 8 patch 0.1 wide at (0.15, 0.15)): a column of 60 spheres along z with
    one centre in projection, all wide (r = 0.2: fat whatever the threshold) but nine, whose radii
    are the nine CONSECUTIVE floats r_a - 4 ulp .. r_a + 4 ulp around r_a, the smallest radius with
    fl(r r) >= T = fat_radius2's value for the patch's rectangle.  (Squares of consecutive radii
    are 2 r ulp(r) apart, 2.7 ulp of T here, so not every fp32 neighbour of T is a square: these
    are the nine squares nearest to T -- at -11, -8, -6, -3, 0, +2, +5, +8, +10 ulp of it --, the
    first one at or above T and the last one below it among them.)

    fat is decided per cluster of 64 sorted spheres, on its survivors.  34 small spheres near the
    low corner, under no ray, sort before the column and 30 near the high corner after it, so the
    column's first 30 spheres are the survivors of cluster 0 and its last 30 those of cluster 1.
    The five radii with r^2 >= T go into one half and the four below T into the other: one cluster
    is fat (its smallest survivor is r_a itself), the other is not (its largest is one float below
    r_a), both are lean and together they hold 60 <= 64 survivors -- so in fast mode the recorder
    must close a round on differing bits (closed_by_flags == 1), and in exact mode, which has no
    fat rounds, they share one round."""
    import torch
    r = rays.cpu().numpy()
    e1 = F32(r[:64, 3].max()) - F32(r[:64, 3].min())
    e2 = F32(r[:64, 4].max()) - F32(r[:64, 4].min())
    T = F32(F32(F32(F32(e1 * e1) + F32(e2 * e2)) * F32(1.0 / 9.0)) * F32(1.0001))     # fat_radius2, unfused
    r_a = np.sqrt(F64(T)).astype(F32)
    for _ in range(4):
        r_a = np.nextafter(r_a, F32(0))
    while not F32(r_a * r_a) >= T:
        r_a = np.nextafter(r_a, F32(np.inf))
    below = np.nextafter(r_a, F32(0))
    assert F32(r_a * r_a) >= T and F32(below * below) < T
    at_or_above, under = [r_a], [below]
    for _ in range(4):
        at_or_above.append(np.nextafter(at_or_above[-1], F32(np.inf)))
    for _ in range(3):
        under.append(np.nextafter(under[-1], F32(0)))
    at_or_above, under = np.array(at_or_above, F32), np.array(under, F32)
    ulp = F64(np.spacing(T))
    assert np.all(at_or_above * at_or_above >= T) and np.all(under * under < T)
    assert np.all(np.abs((np.concatenate([at_or_above, under]) ** 2).astype(F64) - F64(T)) <= 12 * ulp)
    rng = np.random.default_rng(31)
    half = FAT_COLUMN // 2
    lead = F32(0.01) + F32(0.04) * rng.random((FAT_LEAD, 3), dtype=F32)
    trail = F32(0.95) + F32(0.04) * rng.random((FAT_TRAIL, 3), dtype=F32)
    z = F32(0.05) + F32(0.9) * (np.arange(FAT_COLUMN, dtype=F32) + F32(0.5)) / F32(FAT_COLUMN)
    col = np.stack([np.full(FAT_COLUMN, 0.2, F32), np.full(FAT_COLUMN, 0.2, F32), z], axis=1)
    h = np.full(FAT_COLUMN, 0.2, F32)
    first, second = (at_or_above, under) if fat_first else (under, at_or_above)
    h[2:half:6][:len(first)] = first                   # column spheres 2, 8, 14, 20, 26
    h[half + 2::6][:len(second)] = second              # and 32, 38, 44, 50(, 56)
    s = np.empty((FAT_LEAD + FAT_COLUMN + FAT_TRAIL, 4), F32)
    s[:, :3] = np.concatenate([lead, col, trail])
    s[:, 3] = 0.03
    s[FAT_LEAD:FAT_LEAD + FAT_COLUMN, 3] = h
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(len(s), 32, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    # the sorted order is what the docstring says: each group within one 64-aligned run
    hs = d.cpu().numpy()[:, 3]
    where_first = np.nonzero(np.isin(hs, first))[0]
    where_second = np.nonzero(np.isin(hs, second))[0]
    assert len(where_first) == len(first) and len(where_second) == len(second)
    assert np.all(where_first // 64 == 0) and np.all(where_second // 64 == 1)
    wide = np.nonzero(hs == F32(0.2))[0]
    assert len(wide) == FAT_COLUMN - 9 and wide.min() == FAT_LEAD and wide.max() == FAT_LEAD + FAT_COLUMN - 1
    return d, tree, T


@pytest.mark.parametrize("fat_first", [True, False], ids=["fat-then-clamped", "clamped-then-fat"])
def test_radii_at_the_fat_threshold(gh, oracle, cuda, fat_first):
    """fat: every survivor of a cluster has r^2 >= fat_radius2(rectangle), and its survivor loop
    omits the clamp of the table position.  Either decision must give the same sums: a cluster
    whose smallest survivor sits exactly on the threshold (fat) and one whose largest sits one
    float below it (clamped) are traced side by side, the recorder's tallies show that both
    decisions were taken, and fast and exact sums equal brute force on both paths."""
    import torch
    from test_trace_dense_rounds import _patches
    rays = _patches(cuda)                       # two packets: a batch of one packet has no plan
    d, tree, T = _fat_scene(gh, cuda, rays, fat_first)
    rr, ss = rays.cpu().numpy(), d.cpu().numpy()
    c32, c64 = oracle.brute_cumulative(rr, ss)
    assert float(c64[:64].min()) > 0.0 and float(c64[64:].max()) == 0.0
    near = np.abs(ss[:, 3].astype(F64) ** 2 - F64(T)) < 1e-3 * F64(T)
    assert near.sum() == 9 and (oracle.brute_hitcounts(rr, ss[near]) > 0).sum() >= 32     # the nine are hit

    def call():
        out = torch.empty(len(rays), dtype=torch.float32, device=cuda)
        gh.trace_cumulative_sph(rays, d, tree, out, check=True)
        return out
    with gh.Context():
        try:
            gh.set_packet_width(64)
            for exact in (True, False):
                gh.set_exact_integrals(exact)
                ordinary = _plan_off(gh, call)
                got = _from_plan(gh, call)
                st = gh.plan_stats()
                # two entries of 30 lean survivors each; 60 <= 64, so only differing fat bits close a
                # round between them: fast mode took both decisions, exact mode has none to take
                assert (st.entries, st.survivors, st.closed_by_capacity, st.largest_round) == \
                    (2, FAT_COLUMN, 0, 60 if exact else 30), (exact, st)
                assert (st.rounds, st.closed_by_flags) == ((1, 0) if exact else (2, 1)), (exact, st)
                for res in (ordinary, got):
                    check_column_densities(res.cpu().numpy(), c32, c64, "exact" if exact else "fast")
                assert np.array_equal(_bits(got), _bits(ordinary))
        finally:
            _reset(gh)
