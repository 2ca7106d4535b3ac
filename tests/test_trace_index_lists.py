"""The packet plan as index lists (PLAN_FORMAT 3, csrc/trace_state.hpp) and the fused survivor loops.

The recorder stores each class list's survivors as one contiguous run of primitive indices with a
4-byte header per dense round; the planned kernels gather "lane l takes index word l" instead of
inverting {cluster, mask} entries on every call, and the unweighted kernel with the fast integral
runs consecutive test-free rounds of equal bits as ONE survivor loop of up to 128 survivors
(planned_fuses).  plan_stats() still reports the entries and rounds the recorder forms;
plan_loops() reports the survivor loops the last call's kernel runs over them.

Every case compares three ways: the call that runs from the plan with the same call with the plan
switched off, bit for bit; both integrals with the oracle's brute force through
conftest.check_column_densities -- the exact integral is the oracle's fp32 sum bit for bit, the
fast one stays within 1e-5 and 3e-6 of its fp64 sum.  The fast check gets check_column_densities'
max_term allowance (2e-6 of the largest possible term, F(0) / h_min^2): rays of these scenes may
consist of a few grazing hits, the case that allowance is stated for.

The column scene: M wide spheres with one centre in projection, spread along the ray axis under
the 8 x 8 rays of packet 0, with F small spheres near the box's low corner (they sort before the
column whatever the order of the co-ordinates in the Morton key) and T near its high corner (after
it), under no ray.  The sorted array is [F fillers, M column, T fillers], so the column's survivors
per 64-primitive cluster are 64 - F % 64 in its first cluster, then 64 per cluster, then the rest;
F + M <= 1024 keeps the column in one summation class, hence one list."""
import numpy as np
import pytest

from conftest import check_column_densities

F32 = np.float32
WIDE_H = 0.2            # wider than a third of a packet's origin diagonal (0.1 sqrt 2 / 3): fat
BOX = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
LOOP_MAX = 128          # PLAN_LOOP_MAX


def _xyz(u, v, w, axis):
    """(first perpendicular, second perpendicular, along the axis) -> x, y, z."""
    return {0: (w, u, v), 1: (u, w, v), 2: (u, v, w)}[axis]


def _column_scene(gh, cuda, n_lead, n_column, n_trail, axis=2, at=0.2, seed=3):
    import torch
    rng = np.random.default_rng(seed)
    lead = F32(0.01) + F32(0.04) * rng.random((n_lead, 3), dtype=F32)
    trail = F32(0.95) + F32(0.04) * rng.random((n_trail, 3), dtype=F32)
    w = F32(0.05) + F32(0.4) * (np.arange(n_column, dtype=F32) + F32(0.5)) / F32(max(n_column, 1))
    col = np.stack([np.full(n_column, at, F32), np.full(n_column, at, F32), w], axis=1)
    uvw = np.concatenate([lead, col, trail]).astype(F32)
    s = np.empty((len(uvw), 4), F32)
    s[:, 0], s[:, 1], s[:, 2] = _xyz(uvw[:, 0], uvw[:, 1], uvw[:, 2], axis)
    s[:, 3] = 0.03
    s[n_lead:n_lead + n_column, 3] = WIDE_H
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(len(s), 32, device=cuda)
    gh.build_tree(d, tree, *BOX)       # sorts d
    return d, tree


def _ray_patches(cuda, axis=2, sense=1, corners=((0.15, 0.15), (0.6, 0.6)), last=64, length=2.0):
    """One 8 x 8 patch of rays, 0.1 wide, per corner (a packet each); the last patch keeps only its
    first `last` rays.  The rays start outside the box."""
    import torch
    g = (np.arange(8, dtype=F32) + F32(0.5)) * F32(0.1 / 8)
    a, b = [t.ravel() for t in np.meshgrid(g, g, indexing="ij")]
    rows = []
    for k, (u0, v0) in enumerate(corners):
        n = last if k == len(corners) - 1 else 64
        r = np.zeros((n, 7), F32)
        along = np.full(n, -0.5 if sense > 0 else 1.5, F32)
        r[:, 3], r[:, 4], r[:, 5] = _xyz(F32(u0) + a[:n], F32(v0) + b[:n], along, axis)
        r[:, axis] = sense
        r[:, 6] = length
        rows.append(r)
    return torch.from_numpy(np.concatenate(rows)).to(cuda)


def _uniform_scene(gh, cuda, n, seed, radius):
    import torch
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = radius(s[:, :3]).astype(F32)
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(n, 32, device=cuda)
    gh.build_tree(d, tree, *BOX)
    return d, tree


def _ray_grid(cuda, side, depth=-0.1, length=1.3):
    """side^2 rays along +z over the unit square."""
    import torch
    u = (np.arange(side, dtype=F32) + F32(0.5)) / F32(side)
    a, b = [t.ravel() for t in np.meshgrid(u, u, indexing="ij")]
    r = np.zeros((side * side, 7), F32)
    r[:, 2] = 1.0
    r[:, 3], r[:, 4], r[:, 5], r[:, 6] = a, b, depth, length
    return torch.from_numpy(r).to(cuda)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _unweighted(gh, rays, d, tree):
    import torch
    out = torch.empty(len(rays), dtype=torch.float32, device=rays.device)
    gh.trace_cumulative_sph(rays, d, tree, out, check=True)
    return out


def _plan_off(gh, call):
    gh.set_plan(False)
    out = call()
    assert gh.last_plan_used() == 0 and gh.plan_bytes() == 0
    gh.set_plan(True)
    return out


def _planned(gh, call):
    """The call once a plan serves it (the third on the same arrays at the latest), twice."""
    for _ in range(3):
        out = call()
        if gh.last_plan_used() == 1:
            break
    assert gh.last_plan_used() == 1
    again = call()
    assert gh.last_plan_used() == 1 and np.array_equal(_bits(out), _bits(again))
    return again


def _expected_loops(rounds, fuse):
    """The grouping of planned_fuses over one list's rounds [(survivors, bits)]: bits & 1 lean,
    bits & 2 fat.  A kernel that does not fuse runs one loop per round."""
    loops = []
    open_n, open_bits = 0, 0
    for n, bits in rounds:
        if fuse and open_n and (open_bits & 1) and bits == open_bits and open_n + min(n, 64) <= LOOP_MAX:
            open_n += n
        else:
            if open_n:
                loops.append(open_n)
            open_n, open_bits = n, bits
    if open_n:
        loops.append(open_n)
    return loops


class _ThreeWays:
    """One scene and ray batch: plan-off and planned results of both integrals in contexts of their
    own, the plan's tallies and loops, and the three comparisons."""

    def __init__(self, gh, oracle, rays, d, tree, split=-1):
        self.st, self.loops, self.got, self.bytes = {}, {}, {}, {}
        call = lambda: _unweighted(gh, rays, d, tree)
        for exact in (False, True):
            with gh.Context():
                gh.set_packet_width(64)
                gh.set_exact_integrals(exact)
                gh.set_packet_split(split)
                ref = _plan_off(gh, call)
                got = _planned(gh, call)
                self.st[exact], self.loops[exact] = gh.plan_stats(), gh.plan_loops()
                self.bytes[exact] = gh.plan_bytes()
            assert np.array_equal(_bits(got), _bits(ref)), "exact" if exact else "fast"   # 1. plan off, by bits
            self.got[exact] = got.cpu().numpy()
        ss, rr = d.cpu().numpy(), rays.cpu().numpy()
        ref32, ref64 = oracle.brute_cumulative(rr, ss)
        max_term = float(oracle.kernel_table()[0]) / float(ss[:, 3].min()) ** 2
        err = np.abs(self.got[False] - ref64)
        print("fast: largest |got - fp64| / (3e-6 |fp64| + 2e-6 max_term) = %.3g"
              % float(np.max(err / (3e-6 * np.abs(ref64) + 2e-6 * max_term))))
        check_column_densities(self.got[False], ref32, ref64, "fast", max_term)   # 2. fp64 brute force
        check_column_densities(self.got[True], ref32, ref64, "exact")             # 3. the oracle's fp32 sum
        self.ref64 = ref64


# ---- column scenes: known rounds, known loops --------------------------------------------------------

# (leading fillers, column spheres) -> the rounds the recorder forms
COLUMNS = {
    (20, 1): [1],
    (0, 64): [64],
    (20, 65): [44, 21],            # fused to 65
    (0, 128): [64, 64],            # fused to 128
    (0, 129): [64, 64, 1],         # 128, then 1
    (1, 129): [63, 64, 2],         # the first two fuse, the third does not fit (129)
    (40, 90): [24, 64, 2],         # all three: 90
}


@pytest.mark.gpu
@pytest.mark.parametrize("n_lead,n_column", list(COLUMNS))
def test_column_rounds_fuse_as_the_grouping_function_says(gh, cuda, oracle, n_lead, n_column):
    rounds = COLUMNS[(n_lead, n_column)]
    d, tree = _column_scene(gh, cuda, n_lead, n_column, 30)
    rays = _ray_patches(cuda)
    t = _ThreeWays(gh, oracle, rays, d, tree)
    assert float(t.got[False][:64].min()) > 0.0 and float(t.got[False][64:].max()) == 0.0
    for exact in (False, True):
        st = t.st[exact]
        assert (st.survivors, st.rounds, st.largest_round) == (n_column, len(rounds), max(rounds)), (exact, st)
    # the column's rounds are test-free (the rays cross the whole box) and fat (WIDE_H): bits 3
    fused = _expected_loops([(n, 3) for n in rounds], True)
    assert t.loops[False] == (len(fused), max(fused)), (t.loops, fused)
    assert max(fused) <= LOOP_MAX
    assert t.loops[True] == (len(rounds), max(rounds)), t.loops      # the exact integral does not fuse
    assert fused == {(20, 1): [1], (0, 64): [64], (20, 65): [65], (0, 128): [128], (0, 129): [128, 1],
                     (1, 129): [127, 2], (40, 90): [90]}[(n_lead, n_column)]


# ---- changes of bits -----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rays_ending_inside_the_box_do_not_fuse_across_lean_changes(gh, cuda, oracle):
    """Rays from z = -0.1 to z = 0.5: clusters wholly in front of the rays' ends are lean, the
    others are not, and they alternate along a class list.  Non-lean rounds never fuse, so the
    loops are fewer than the rounds by exactly the lean rounds that joined a loop, and a loop above
    64 exists only because lean rounds fused."""
    d, tree = _uniform_scene(gh, cuda, 20000, 31, lambda p: 0.06 + 0.03 * p[:, 0])
    rays = _ray_grid(cuda, 40, depth=-0.1, length=0.6)
    t = _ThreeWays(gh, oracle, rays, d, tree)
    st, (loops, largest) = t.st[False], t.loops[False]
    assert st.closed_by_flags > 0 and st.largest_round <= 64, st
    assert 0 < loops < st.rounds and 64 < largest <= LOOP_MAX, (st, loops, largest)
    # every change of bits still ends a loop: at least one loop per flag-closed round, plus one per list
    assert loops > st.closed_by_flags, (st, loops)
    assert t.loops[True] == (t.st[True].rounds, t.st[True].largest_round)


@pytest.mark.gpu
def test_wide_and_narrow_slabs_do_not_fuse_across_fat_changes(gh, cuda, oracle):
    """Slabs of spheres of radius 0.09 (fat for 64 x 64 rays: a third of a packet's origin diagonal
    is 0.052) and 0.03 alternate along z every 0.25, so fat and non-fat rounds alternate in the
    lists; all are lean."""
    d, tree = _uniform_scene(gh, cuda, 20000, 32,
                             lambda p: np.where(np.floor(p[:, 2] * 4.0) % 2 == 0, 0.09, 0.03))
    rays = _ray_grid(cuda, 64)
    t = _ThreeWays(gh, oracle, rays, d, tree)
    st, (loops, largest) = t.st[False], t.loops[False]
    assert st.closed_by_flags > 0 and st.largest_round <= 64, st
    assert st.closed_by_flags < loops < st.rounds and largest <= LOOP_MAX, (st, loops, largest)
    assert t.loops[True] == (t.st[True].rounds, t.st[True].largest_round)


# ---- small edges -----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_fewer_than_64_spheres(gh, cuda, oracle):
    """37 spheres: every gather's lanes past the list's few survivors hold slack or padding words
    and clamp against n_prims - 1 = 36."""
    d, tree = _uniform_scene(gh, cuda, 37, 33, lambda p: 0.1 + 0.2 * p[:, 1])
    rays = _ray_grid(cuda, 16)
    t = _ThreeWays(gh, oracle, rays, d, tree)
    assert 0 < t.st[False].survivors and t.st[False].largest_round <= 37 and float(t.ref64.max()) > 0.0


@pytest.mark.gpu
def test_a_ray_count_that_is_no_multiple_of_64(gh, cuda, oracle):
    d, tree = _column_scene(gh, cuda, 0, 128, 30, at=0.8)
    rays = _ray_patches(cuda, corners=((0.4, 0.4), (0.75, 0.75)), last=32)   # the column under the ragged last packet
    t = _ThreeWays(gh, oracle, rays, d, tree)
    assert len(t.got[False]) == 96 and float(t.got[False][64:].min()) > 0.0
    assert t.loops[False] == (1, 128) and t.loops[True] == (2, 64)
    d, tree = _uniform_scene(gh, cuda, 5000, 34, lambda p: 0.05 + 0.0 * p[:, 0])
    rays = _ray_grid(cuda, 24)[:544].contiguous()                            # 8 x 64 + 32
    _ThreeWays(gh, oracle, rays, d, tree)


@pytest.mark.gpu
def test_the_last_list_of_the_last_packet(gh, cuda, oracle):
    """The column is the array's tail, of class 7, and lies under the LAST packet: its list ends the
    index words and the headers, and the look-ahead of its only loop -- a fused one of 128 -- reads
    the padding behind them."""
    rays = _ray_patches(cuda, corners=((0.4, 0.4), (0.75, 0.75)))
    d, tree = _column_scene(gh, cuda, 7 * 1024, 128, 0, at=0.8)          # clusters 112 and 113: granule 7
    t = _ThreeWays(gh, oracle, rays, d, tree)
    st = t.st[False]
    assert (st.entries, st.rounds, st.full_rounds) == (2, 2, 2), st
    assert t.loops[False] == (1, 128) and t.loops[True] == (2, 64), t.loops
    assert float(t.got[False][:64].max()) == 0.0 and float(t.got[False][64:].min()) > 0.0


@pytest.mark.gpu
def test_a_plan_of_empty_lists(gh, cuda, oracle):
    rays = _ray_patches(cuda)
    d, tree = _column_scene(gh, cuda, 20, 0, 30)             # nothing under any ray
    call = lambda: _unweighted(gh, rays, d, tree)
    for exact in (False, True):
        with gh.Context():
            gh.set_packet_width(64)
            gh.set_exact_integrals(exact)
            ref = _plan_off(gh, call)
            got = _planned(gh, call)
            assert tuple(gh.plan_stats()) == (0,) * 7 and gh.plan_loops() == (0, 0)
            assert gh.plan_bytes() > 0
        assert np.array_equal(_bits(got), _bits(ref)) and float(got.max()) == 0.0
    ref32, ref64 = oracle.brute_cumulative(rays.cpu().numpy(), d.cpu().numpy())
    assert float(ref64.max()) == 0.0


# ---- the kernel's paths ------------------------------------------------------------------------------------

# 44 in the last cluster of class 0, 4 x 64 | 4 in class 1 (304 coincident terms: few enough for
# the fast evaluation's 3e-6 of an fp32 sum)
SWEEP_LEAD, SWEEP_COLUMN = 980, 304
SWEEP_ROUNDS = [[44], [64] * 4 + [4]]


def _sweep_loops(fuse):
    loops = sum((_expected_loops([(n, 3) for n in rounds], fuse) for rounds in SWEEP_ROUNDS), [])
    return len(loops), max(loops)


@pytest.mark.gpu
@pytest.mark.parametrize("sense", [1, -1])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_each_axis_and_sense_fast_and_exact(gh, cuda, oracle, axis, sense):
    d, tree = _column_scene(gh, cuda, SWEEP_LEAD, SWEEP_COLUMN, 30, axis=axis)
    rays = _ray_patches(cuda, axis=axis, sense=sense)
    t = _ThreeWays(gh, oracle, rays, d, tree)
    for exact in (False, True):
        st = t.st[exact]
        assert (st.entries, st.survivors, st.rounds, st.largest_round) == (6, SWEEP_COLUMN, 6, 64), st
        assert t.loops[exact] == _sweep_loops(not exact), (exact, t.loops)
    assert _sweep_loops(True) == (1 + 3, 128)        # 44 | 128, 128, 4
    assert float(t.got[False][:64].min()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [0, 1, 2, 3, 4])     # 0: the unweighted trace
def test_each_packet_split_and_channel_count(gh, cuda, oracle, channels):
    """One plan serves every packet split.  The weighted kernels run from the index lists too, one
    loop per dense round; their first channel carries weights of one, whose sums are the
    unweighted call's bit for bit (fl(1 x) = x) -- the call that the oracle checks here."""
    import torch
    d, tree = _column_scene(gh, cuda, SWEEP_LEAD, SWEEP_COLUMN, 30)
    rays = _ray_patches(cuda)
    if channels:
        rng = np.random.default_rng(50 + channels)
        w = rng.random((len(d), channels)).astype(F32) * F32(4.0) - F32(2.0)
        w[:, 0] = 1.0
        w = torch.from_numpy(w).to(cuda)
        call = lambda: gh.trace_cumulative_weighted_sph(rays, d, tree, w, check=True)
    else:
        call = lambda: _unweighted(gh, rays, d, tree)
    ss, rr = d.cpu().numpy(), rays.cpu().numpy()
    ref32, ref64 = oracle.brute_cumulative(rr, ss)
    max_term = float(oracle.kernel_table()[0]) / float(ss[:, 3].min()) ** 2
    for exact in (False, True):
        with gh.Context():
            gh.set_packet_width(64)
            gh.set_exact_integrals(exact)
            refs = {}
            gh.set_plan(False)
            for k in (1, 2, 4, 8):
                gh.set_packet_split(k)
                refs[k] = call()
                assert gh.last_plan_used() == 0
            gh.set_plan(True)
            _planned(gh, call)
            fuses = channels == 0 and not exact
            assert gh.plan_loops() == _sweep_loops(fuses), (channels, exact, gh.plan_loops())
            if channels:
                assert gh.plan_loops()[1] <= 64
            for k in (1, 2, 4, 8):
                gh.set_packet_split(k)
                got = call()
                assert gh.last_plan_used() == 1, k
                assert np.array_equal(_bits(got), _bits(refs[k])), (k, exact)
                first = got.cpu().numpy().reshape(len(rays), -1)[:, 0].copy()
                # the class sums are combined in one fixed order whatever the split
                check_column_densities(first, ref32, ref64, "exact" if exact else "fast",
                                       None if exact else max_term)
            unweighted = _unweighted(gh, rays, d, tree)
            assert np.array_equal(_bits(unweighted).ravel(), first.view(np.uint32)), (channels, exact)


# ---- re-record and budget --------------------------------------------------------------------------------

@pytest.mark.gpu
def test_an_edit_within_the_room_records_again_in_place(gh, cuda, oracle):
    """One filler of the column's first cluster grows until every ray of packet 0 meets it: the list
    has one survivor more (66 of a room of 65 + 8 + 2), the rounds and the loops shift, and the
    call that notices records again into the same room."""
    d, tree = _column_scene(gh, cuda, 20, 65, 30)
    rays = _ray_patches(cuda)
    for exact in (False, True):
        d2 = d.clone()
        call = lambda: _unweighted(gh, rays, d2, tree)
        with gh.Context():
            gh.set_packet_width(64)
            gh.set_exact_integrals(exact)
            first = _planned(gh, call)
            size, st0 = gh.plan_bytes(), gh.plan_stats()
            assert (st0.survivors, st0.rounds) == (65, 2) and gh.plan_loops() == ((2, 44) if exact else (1, 65))
            d2[5, 3] = 0.5                           # (0.03, 0.03) to the patch's far corner: 0.31
            got = call()
            assert gh.last_plan_used() == 1 and gh.plan_bytes() == size
            st1 = gh.plan_stats()
            assert (st1.survivors, st1.rounds, st1.largest_round) == (66, 2, 45), st1   # 45 | 21
            assert gh.plan_loops() == ((2, 45) if exact else (1, 66))
            again = call()
            assert gh.last_plan_used() == 1
            ref = _plan_off(gh, call)
        assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(_bits(again), _bits(ref))
        assert not np.array_equal(_bits(first), _bits(ref))
        ss = d2.cpu().numpy()
        ref32, ref64 = oracle.brute_cumulative(rays.cpu().numpy(), ss)
        max_term = float(oracle.kernel_table()[0]) / float(ss[:, 3].min()) ** 2
        check_column_densities(got.cpu().numpy(), ref32, ref64, "exact" if exact else "fast",
                               None if exact else max_term)


@pytest.mark.gpu
def test_an_edit_that_outgrows_the_room_falls_back(gh, cuda, oracle):
    """The fillers of the column's first cluster grow until every ray of packet 0 meets them: the
    list of 65 survivors (room 65 + 8 + 2) now holds 85, the plan is unusable and the ordinary
    kernels run."""
    d, tree = _column_scene(gh, cuda, 20, 65, 30)
    rays = _ray_patches(cuda)
    for exact in (False, True):
        d2 = d.clone()
        call = lambda: _unweighted(gh, rays, d2, tree)
        with gh.Context():
            gh.set_packet_width(64)
            gh.set_exact_integrals(exact)
            _planned(gh, call)
            assert gh.plan_stats().survivors == 65
            d2[:20, 3] = 0.5
            got = call()
            assert gh.last_plan_used() == 0
            assert tuple(gh.plan_stats()) == (0,) * 7 and gh.plan_loops() == (0, 0)
            ref = _plan_off(gh, call)
        assert np.array_equal(_bits(got), _bits(ref))
        ss = d2.cpu().numpy()
        ref32, ref64 = oracle.brute_cumulative(rays.cpu().numpy(), ss)
        max_term = float(oracle.kernel_table()[0]) / float(ss[:, 3].min()) ** 2
        check_column_densities(got.cpu().numpy(), ref32, ref64, "exact" if exact else "fast",
                               None if exact else max_term)


@pytest.mark.gpu
def test_a_budget_below_the_plans_size_falls_back(gh, cuda, oracle):
    d, tree = _uniform_scene(gh, cuda, 20000, 35, lambda p: 0.04 + 0.02 * p[:, 1])
    rays = _ray_grid(cuda, 24)
    t = _ThreeWays(gh, oracle, rays, d, tree)
    call = lambda: _unweighted(gh, rays, d, tree)
    with gh.Context():
        gh.set_packet_width(64)
        gh.set_plan_budget(t.bytes[False] - 1)
        for _ in range(4):
            got = call()
            assert gh.last_plan_used() == 0 and gh.plan_bytes() == 0
        assert gh.plan_loops() == (0, 0)
        gh.set_plan_budget(t.bytes[False])
        again = _planned(gh, call)
        assert gh.plan_bytes() == t.bytes[False]
    assert np.array_equal(_bits(got), t.got[False].view(np.uint32))
    assert np.array_equal(_bits(again), t.got[False].view(np.uint32))
