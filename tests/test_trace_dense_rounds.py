"""Dense survivor rounds of the planned column-density kernel (PLAN_ROUND_END in csrc/trace_state.hpp).

The plan's recorder groups consecutive entries of a list into rounds of at most 64 survivors and
one lean / fat class; the planned kernel gathers a round's survivors from all its clusters and
runs ONE survivor loop over them.  Every case here compares a call that runs from the plan, bit
for bit, with the same call of the same context with the plan switched off (set_plan(False): the
ordinary kernels), and reads through plan_stats() what the recorder formed.  One case per group is
also held against brute force: exact integrals are the oracle's fp32 sum bit for bit, fast ones
stay within conftest.check_column_densities' bounds.

The synthetic scene is a COLUMN: M wide spheres with one centre in projection, spread along the
ray axis under the 8 x 8 rays of packet 0, with F small spheres near the box's low corner and T
near its high corner, under no ray.  Whatever the order of the co-ordinates in the Morton key, the
low-corner spheres sort before the column and the high-corner ones after it (they differ from it
in the leading bits of all three co-ordinates), so the sorted array is [F fillers, M column,
T fillers] and the column's survivors per 64-primitive cluster are known: 64 - F % 64 in its first
cluster, then 64 per cluster, then the rest."""
import numpy as np
import pytest

from conftest import check_column_densities

F32 = np.float32
COLUMN_H = 0.2           # wider than a third of a packet's origin diagonal (0.1 sqrt 2 / 3): fat
BOX = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def _place(u, v, w, axis):
    """(first perpendicular, second perpendicular, along the axis) -> x, y, z."""
    return {0: (w, u, v), 1: (u, w, v), 2: (u, v, w)}[axis]


def _column(gh, cuda, n_lead, n_column, n_trail, axis=2, at=0.2, seed=1):
    """Sorted spheres and tree of a column scene; at: the column's centre in both perpendicular
    co-ordinates (0.2, or 0.8: then it lies under the patch that sorts LAST in the ray order)."""
    import torch
    rng = np.random.default_rng(seed)
    lead = F32(0.01) + F32(0.04) * rng.random((n_lead, 3), dtype=F32)
    trail = F32(0.95) + F32(0.04) * rng.random((n_trail, 3), dtype=F32)
    w = F32(0.05) + F32(0.4) * (np.arange(n_column, dtype=F32) + F32(0.5)) / F32(max(n_column, 1))
    col = np.stack([np.full(n_column, at, F32), np.full(n_column, at, F32), w], axis=1)
    uvw = np.concatenate([lead, col, trail]).astype(F32)
    s = np.empty((len(uvw), 4), F32)
    s[:, 0], s[:, 1], s[:, 2] = _place(uvw[:, 0], uvw[:, 1], uvw[:, 2], axis)
    s[:, 3] = 0.03
    s[n_lead:n_lead + n_column, 3] = COLUMN_H
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(len(s), 32, device=cuda)
    gh.build_tree(d, tree, *BOX)       # sorts d
    return d, tree


def _patches(cuda, axis=2, sense=1, corners=((0.15, 0.15), (0.6, 0.6)), last=64, length=2.0):
    """One 8 x 8 patch of rays, 0.1 wide, per corner (a packet each: the patches are far apart in
    the ray order); the last patch keeps only its first `last` rays.  The rays start outside the
    box, at -0.5 (sense +1) or 1.5 (sense -1) along the axis."""
    import torch
    g = (np.arange(8, dtype=F32) + F32(0.5)) * F32(0.1 / 8)
    a, b = [t.ravel() for t in np.meshgrid(g, g, indexing="ij")]
    rows = []
    for k, (u0, v0) in enumerate(corners):
        n = last if k == len(corners) - 1 else 64
        r = np.zeros((n, 7), F32)
        along = np.full(n, -0.5 if sense > 0 else 1.5, F32)
        r[:, 3], r[:, 4], r[:, 5] = _place(F32(u0) + a[:n], F32(v0) + b[:n], along, axis)
        r[:, axis] = sense
        r[:, 6] = length
        rows.append(r)
    return torch.from_numpy(np.concatenate(rows)).to(cuda)


def _random_scene(gh, cuda, n, seed, radius):
    """n uniform spheres; radius(xyz) -> their radii."""
    import torch
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = radius(s[:, :3]).astype(F32)
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(n, 32, device=cuda)
    gh.build_tree(d, tree, *BOX)
    return d, tree


def _grid(cuda, side, depth=-0.1, length=1.3):
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


def _cumulative(gh, rays, d, tree):
    import torch
    out = torch.empty(len(rays), dtype=torch.float32, device=rays.device)
    gh.trace_cumulative_sph(rays, d, tree, out, check=True)
    return out


def _plan_off(gh, call):
    """The call with the plan switched off: the ordinary kernels, whatever the caches hold."""
    gh.set_plan(False)
    out = call()
    assert gh.last_plan_used() == 0 and gh.plan_bytes() == 0
    gh.set_plan(True)
    return out


def _from_plan(gh, call):
    """The call once a plan serves it (recorded by the first call that both caches serve: the
    third on the same arrays at the latest), and the plan's tallies."""
    for _ in range(3):
        out = call()
        if gh.last_plan_used() == 1:
            break
    assert gh.last_plan_used() == 1
    again = call()
    assert gh.last_plan_used() == 1
    assert np.array_equal(_bits(out), _bits(again))
    return again, gh.plan_stats()


def _both(gh, call, exact=False, split=-1):
    """(plan-off result, planned result, plan stats) of `call` in a context of its own."""
    with gh.Context():
        gh.set_packet_width(64)
        gh.set_exact_integrals(exact)
        gh.set_packet_split(split)
        ref = _plan_off(gh, call)
        got, stats = _from_plan(gh, call)
    assert np.array_equal(_bits(got), _bits(ref))
    return ref, got, stats


def _against_brute_force(oracle, rays, d, exact_result, fast_result):
    ref32, ref64 = oracle.brute_cumulative(rays.cpu().numpy(), d.cpu().numpy())
    assert float(ref64.max()) > 0.0
    check_column_densities(exact_result.cpu().numpy(), ref32, ref64, "exact")
    check_column_densities(fast_result.cpu().numpy(), ref32, ref64, "fast")


# ---- round capacity -------------------------------------------------------------------------------

# (leading fillers, column spheres) -> the column's survivors per entry, and the rounds they form
CAPACITY = {
    (20, 63): ([44, 19], [63]),            # two entries, one round short of full
    (20, 64): ([44, 20], [64]),            # two entries fill a round exactly
    (20, 65): ([44, 21], [44, 21]),        # the second entry would pass 64: closed by capacity
    (0, 64): ([64], [64]),                 # one cluster, all 64 of 64 surviving
    (0, 128): ([64, 64], [64, 64]),
    (63, 65): ([1, 64], [1, 64]),          # 1 + 64
    (1, 127): ([63, 64], [63, 64]),
    (40, 90): ([24, 64, 2], [24, 64, 2]),  # a full cluster between two partial ones
    (60, 36): ([4, 32], [36]),
}


@pytest.mark.gpu
def test_rounds_fill_to_64_survivors_and_no_further(gh, cuda, oracle):
    rays = _patches(cuda)
    seen = []
    for (n_lead, n_col), (entries, rounds) in CAPACITY.items():
        d, tree = _column(gh, cuda, n_lead, n_col, 30)
        call = lambda: _cumulative(gh, rays, d, tree)
        ref, got, st = _both(gh, call)
        seen.append(st)
        assert float(got[:64].min()) > 0.0 and float(got[64:].max()) == 0.0
        # the scene is what the module's docstring says it is ...
        assert (st.entries, st.survivors) == (len(entries), n_col), (n_lead, n_col, st)
        # ... and its rounds are the ones rules (a) and (c) give
        closed_a = len(rounds) - 1      # (every round but the list's last is closed by capacity here)
        assert (st.rounds, st.full_rounds, st.closed_by_capacity, st.closed_by_flags, st.largest_round) == \
            (len(rounds), rounds.count(64), closed_a, 0, max(rounds)), (n_lead, n_col, st)
        if (n_lead, n_col) == (20, 65):
            _, exact, _ = _both(gh, call, exact=True)
            _against_brute_force(oracle, rays, d, exact, got)
    # conditions on the sweep itself
    assert any(s.full_rounds > 0 for s in seen)
    assert any(s.closed_by_capacity > 0 for s in seen)
    assert all(s.largest_round <= 64 for s in seen)


# ---- flag changes ---------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rays_ending_inside_the_box_close_rounds_at_lean_changes(gh, cuda, oracle):
    """Rays from z = -0.1 to z = 0.5: clusters wholly in front of the rays' ends are lean (no range
    tests), the others are not, and they alternate along a class list."""
    d, tree = _random_scene(gh, cuda, 20000, 21, lambda p: 0.06 + 0.03 * p[:, 0])
    rays = _grid(cuda, 40, depth=-0.1, length=0.6)
    call = lambda: _cumulative(gh, rays, d, tree)
    ref, got, st = _both(gh, call)
    assert st.closed_by_flags > 0 and st.closed_by_capacity > 0 and st.largest_round <= 64, st
    assert st.rounds < st.entries, st          # rounds do take several entries
    _, exact, st_exact = _both(gh, call, exact=True)
    assert st_exact.closed_by_flags > 0, st_exact
    _against_brute_force(oracle, rays, d, exact, got)


@pytest.mark.gpu
def test_wide_and_narrow_spheres_close_rounds_at_fat_changes(gh, cuda):
    """64 x 64 rays: a packet's origin diagonal is 7/64 sqrt 2 = 0.155, a third of it 0.052.  Slabs
    of spheres of radius 0.09 (fat: no clamp of the table position) and 0.03 alternate along z
    every 0.25, far thicker than a cluster, so that fat and non-fat clusters alternate in the lists."""
    d, tree = _random_scene(gh, cuda, 20000, 22,
                            lambda p: np.where(np.floor(p[:, 2] * 4.0) % 2 == 0, 0.09, 0.03))
    rays = _grid(cuda, 64)
    call = lambda: _cumulative(gh, rays, d, tree)
    ref, got, st = _both(gh, call)
    assert st.closed_by_flags > 0 and st.largest_round <= 64, st
    assert float(got.min()) > 0.0


# ---- edges ----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_list_of_one_entry_with_one_survivor(gh, cuda, oracle):
    rays = _patches(cuda)
    d, tree = _column(gh, cuda, 20, 1, 30)
    call = lambda: _cumulative(gh, rays, d, tree)
    ref, got, st = _both(gh, call)
    assert tuple(st) == (1, 1, 1, 0, 0, 0, 1), st      # every other list of both packets is empty
    assert float(got[:64].min()) > 0.0 and float(got[64:].max()) == 0.0
    _, exact, _ = _both(gh, call, exact=True)
    _against_brute_force(oracle, rays, d, exact, got)


@pytest.mark.gpu
def test_a_plan_of_empty_lists(gh, cuda):
    rays = _patches(cuda)
    d, tree = _column(gh, cuda, 20, 0, 30)             # nothing under any ray
    ref, got, st = _both(gh, lambda: _cumulative(gh, rays, d, tree))
    assert tuple(st) == (0, 0, 0, 0, 0, 0, 0), st
    assert float(got.max()) == 0.0


@pytest.mark.gpu
def test_the_last_list_of_the_last_packet(gh, cuda):
    """Every packet sees every class (20000 spheres are 20 granules), so the last packet's last
    list is the last thing in the plan and its look-ahead reads run into the padding behind it;
    in a second scene the column is the array's tail, so the very last entry is a full round."""
    d, tree = _random_scene(gh, cuda, 20000, 23, lambda p: 0.04 + 0.02 * p[:, 1])
    rays = _grid(cuda, 24)
    ref, got, st = _both(gh, lambda: _cumulative(gh, rays, d, tree))
    assert st.entries >= 9 * 8 and float(got.min()) > 0.0, st
    rays = _patches(cuda, corners=((0.4, 0.4), (0.75, 0.75)))    # the column under the LAST packet
    d, tree = _column(gh, cuda, 0, 7 * 1024 + 64, 0, at=0.8)     # its last cluster is of class 7
    ref, got, st = _both(gh, lambda: _cumulative(gh, rays, d, tree))
    assert (st.entries, st.rounds, st.full_rounds) == (113, 113, 113), st
    assert float(got[:64].max()) == 0.0 and float(got[64:].min()) > 0.0


@pytest.mark.gpu
def test_a_ray_count_that_is_no_multiple_of_64(gh, cuda):
    d, tree = _column(gh, cuda, 20, 65, 30, at=0.8)
    rays = _patches(cuda, corners=((0.4, 0.4), (0.75, 0.75)), last=32)   # the column under the ragged last packet
    ref, got, st = _both(gh, lambda: _cumulative(gh, rays, d, tree))
    assert (st.entries, st.rounds, st.closed_by_capacity) == (2, 2, 1), st
    assert len(got) == 96 and float(got[64:].min()) > 0.0
    d, tree = _random_scene(gh, cuda, 5000, 24, lambda p: 0.05 + 0.0 * p[:, 0])
    rays = _grid(cuda, 24)[:544].contiguous()                            # 544 = 8 x 64 + 32 (ray counts are multiples of 32)
    _both(gh, lambda: _cumulative(gh, rays, d, tree))


# ---- the round-capacity scene over the kernel's paths --------------------------------------------

SWEEP_LEAD, SWEEP_COLUMN = 20, 2100      # 44 | 32 full clusters | 8: three granules, classes 0, 1, 2


def _sweep_stats_ok(st):
    # the list of class 0 holds 44 | 15 x 64, those of classes 1 and 2 16 x 64 and 64 | 8
    return (st.entries, st.survivors, st.rounds, st.full_rounds, st.closed_by_capacity, st.closed_by_flags,
            st.largest_round) == (34, SWEEP_COLUMN, 34, 32, 31, 0, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("sense", [1, -1])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_each_axis_and_sense_fast_and_exact(gh, cuda, oracle, axis, sense, exact):
    d, tree = _column(gh, cuda, SWEEP_LEAD, SWEEP_COLUMN, 30, axis=axis)
    rays = _patches(cuda, axis=axis, sense=sense)
    ref, got, st = _both(gh, lambda: _cumulative(gh, rays, d, tree), exact=exact)
    assert _sweep_stats_ok(st), st
    assert float(got[:64].min()) > 0.0
    if axis == 0 and sense == -1 and exact:
        # (exact integrals only, as in test_trace_plan.py: 2100 coincident terms summed in fp32 leave
        # the fast evaluation's 3e-6 no room, with or without a plan)
        ref32, ref64 = oracle.brute_cumulative(rays.cpu().numpy(), d.cpu().numpy())
        check_column_densities(got.cpu().numpy(), ref32, ref64, "exact")


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("channels", [0, 1, 2, 3, 4])     # 0: the unweighted trace
def test_each_packet_split_and_channel_count(gh, cuda, channels, exact):
    import torch
    d, tree = _column(gh, cuda, SWEEP_LEAD, SWEEP_COLUMN, 30)
    rays = _patches(cuda)
    if channels:
        rng = np.random.default_rng(40 + channels)
        w = torch.from_numpy(rng.random((len(d), channels)).astype(F32) * F32(4.0) - F32(2.0)).to(cuda)
        call = lambda: gh.trace_cumulative_weighted_sph(rays, d, tree, w, check=True)
    else:
        call = lambda: _cumulative(gh, rays, d, tree)
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
        _, st = _from_plan(gh, call)
        assert _sweep_stats_ok(st), st
        for k in (1, 2, 4, 8):        # one plan serves every split
            gh.set_packet_split(k)
            got = call()
            assert gh.last_plan_used() == 1, k
            assert np.array_equal(_bits(got), _bits(refs[k])), k
        assert float(got.abs().max()) > 0.0


# ---- re-record ------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_stale_signature_forms_the_rounds_again_in_place(gh, cuda, oracle):
    """Both integrals; the re-recorded call is also held against brute force on the arrays as they
    are AFTER the change -- the plan-off call goes through the same re-derived caches, so equality
    with it alone would not show a stale record that both paths share."""
    results = {}
    for exact in (False, True):
        d, tree = _random_scene(gh, cuda, 20000, 25, lambda p: 0.05 + 0.03 * p[:, 2])
        rays = _grid(cuda, 40)
        call = lambda: _cumulative(gh, rays, d, tree)
        with gh.Context():
            gh.set_packet_width(64)
            gh.set_exact_integrals(exact)
            first, st0 = _from_plan(gh, call)
            size = gh.plan_bytes()
            d[::7, 3] *= 0.5                        # a few spheres shrink: lists get shorter, rounds shift
            rays[::3, 6] = 0.8                      # and some rays now end inside the box: other lean bits
            got = call()
            assert gh.last_plan_used() == 1 and gh.plan_bytes() == size
            st1 = gh.plan_stats()
            assert st1.survivors < st0.survivors and st1.rounds != st0.rounds and st1.largest_round <= 64, (st0, st1)
            assert st1.closed_by_flags > st0.closed_by_flags, (st0, st1)
            again = call()                          # ... and the call after runs from the plan as it stands
            assert gh.last_plan_used() == 1 and tuple(gh.plan_stats()) == tuple(st1)
            ref = _plan_off(gh, call)
        assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(_bits(again), _bits(ref))
        assert not np.array_equal(_bits(first), _bits(ref))
        results[exact] = got
    # (the same seed and the same changes both times: d and rays are the modified arrays of either pass)
    _against_brute_force(oracle, rays, d, results[True], results[False])


@pytest.mark.gpu
def test_a_list_that_outgrows_its_room_falls_back(gh, cuda, oracle):
    d, tree = _random_scene(gh, cuda, 20000, 26, lambda p: 0.02 + 0.0 * p[:, 0])
    rays = _grid(cuda, 40)
    call = lambda: _cumulative(gh, rays, d, tree)
    with gh.Context():
        gh.set_packet_width(64)
        _from_plan(gh, call)
        d[:, 3] *= 4.0                          # every packet now meets several times as many clusters
        got = call()
        assert gh.last_plan_used() == 0
        assert tuple(gh.plan_stats()) == (0,) * 7
        ref = _plan_off(gh, call)
    assert np.array_equal(_bits(got), _bits(ref))
    ref32, ref64 = oracle.brute_cumulative(rays.cpu().numpy(), d.cpu().numpy())     # the grown spheres
    check_column_densities(got.cpu().numpy(), ref32, ref64, "fast")
