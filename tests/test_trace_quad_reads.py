"""The planned column-density kernel's survivor loops at their exits, and its own packet split
(planned_split in csrc/trace_state.hpp).

Every case compares a call that runs from the plan, bit for bit, with the same call of the same
context with the plan switched off (set_plan(False): the ordinary kernels), and holds it against
brute force within the project's stated 1e-5 (relative to the oracle's fp64 sum).
The scenes are test_trace_dense_rounds.py's columns: M spheres with one centre in projection under
the 8 x 8 rays of packet 0, so the survivors of every 64-primitive cluster, and with them the
dense rounds the recorder forms, are known and are asserted through plan_stats().

Two things the library's front end decides shape the cases.  A batch of at most 64 rays is not
reordered, so neither cache serves it and it never runs from a plan: the one-packet cases assert
equality with the plan-off call and that no plan was used, and a two-packet batch stands in for
"the smallest planned batch".  The Python binding, like the reference, takes ray counts that are
multiples of 32 only: the 65- and 127-ray batches go to the C entry point directly."""
import numpy as np
import pytest

from conftest import check_column_densities
from test_trace_dense_rounds import (BOX, COLUMN_H, F32, _bits, _both, _column, _cumulative, _from_plan,
                                     _patches, _place, _plan_off)

# An 8 x 8 patch of _patches spans 7/8 of 0.1 in each perpendicular co-ordinate: a survivor is fat
# (no clamp of the table position) from h^2 >= 1.0001 (e1^2 + e2^2) / 9 on, h >= 0.041250.
PATCH_EXTENT = 0.1 * 7.0 / 8.0
FAT_H = float(np.sqrt(2.0 * PATCH_EXTENT ** 2 / 9.0 * 1.0001))


def _close_to_brute_force(oracle, rays, d, got, weights=None):
    """|got - fp64 brute force| <= 1e-5 |fp64 brute force| for every ray (and channel)."""
    r, s = rays.cpu().numpy(), d.cpu().numpy()
    got = got.cpu().numpy().astype(np.float64).reshape(len(r), -1)
    if weights is None:
        ref = oracle.brute_cumulative(r, s)[1].reshape(len(r), 1)
    else:
        # channel c: the trace of the same spheres with 1/h^2 scaled by w_c is not expressible in
        # the oracle's call; sum the oracle's per-sphere terms instead: one brute-force pass per
        # sphere subset would be slow, so use linearity -- spheres of weight w contribute w x term.
        w = weights.cpu().numpy().astype(np.float64).reshape(len(s), -1)
        ref = np.zeros((len(r), w.shape[1]))
        for wv in np.unique(w[:, 0]):       # (the weighted cases use few distinct weight rows)
            sel = w[:, 0] == wv
            part = oracle.brute_cumulative(r, s[sel])[1]
            for c in range(w.shape[1]):
                rows = np.unique(w[sel, c])
                assert len(rows) == 1
                ref[:, c] += rows[0] * part
    assert float(np.abs(ref).max()) > 0.0
    err = np.abs(got - ref)
    worst = float((err / np.maximum(np.abs(ref), 1e-300))[ref != 0.0].max()) if (ref != 0.0).any() else 0.0
    print("largest relative difference from fp64 brute force: %.3e" % worst)
    assert np.all(err <= 1e-5 * np.abs(ref)), worst


def _column_of(gh, cuda, n_lead, column_h, n_trail, axis=2, seed=1):
    """test_trace_dense_rounds._column with a radius per column sphere, in ascending order along
    the axis (the order the column has in the sorted array)."""
    import torch
    column_h = np.asarray(column_h, F32)
    n_column = len(column_h)
    rng = np.random.default_rng(seed)
    lead = F32(0.01) + F32(0.04) * rng.random((n_lead, 3), dtype=F32)
    trail = F32(0.95) + F32(0.04) * rng.random((n_trail, 3), dtype=F32)
    w = F32(0.05) + F32(0.4) * (np.arange(n_column, dtype=F32) + F32(0.5)) / F32(max(n_column, 1))
    col = np.stack([np.full(n_column, 0.2, F32), np.full(n_column, 0.2, F32), w], axis=1)
    uvw = np.concatenate([lead, col, trail]).astype(F32)
    s = np.empty((len(uvw), 4), F32)
    s[:, 0], s[:, 1], s[:, 2] = _place(uvw[:, 0], uvw[:, 1], uvw[:, 2], axis)
    s[:, 3] = 0.03
    s[n_lead:n_lead + n_column, 3] = column_h
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(len(s), 32, device=cuda)
    gh.build_tree(d, tree, *BOX)
    return d, tree


def _cumulative_c_abi(gh, rays, d, tree):
    """trace_cumulative_sph without the binding's multiple-of-32 check."""
    import torch
    out = torch.empty(len(rays), dtype=torch.float32, device=rays.device)
    gh._check(gh._lib.grace_trace_cumulative_f4(*gh._trace_args(rays, d, tree), gh._ptr(out), gh._stream()))
    gh.trace_status()
    return out


# ---- the exits of the three-way rotated survivor loop and the tile's last slots ----------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65])
def test_rounds_of_exactly_n_survivors(gh, cuda, oracle, n):
    """One cluster with n column spheres in front: one entry, one round of n survivors (the loop
    leaves at its first, second or third exit as n mod 3 says; 63 and 64 read the tile's last
    slots and the two past them); 65 spheres are a list of two entries that cannot share a round."""
    d, tree = _column(gh, cuda, 0, n, 40)      # (40 fillers behind: a tree wants more primitives than a leaf holds)
    rays = _patches(cuda)
    ref, got, st = _both(gh, lambda: _cumulative(gh, rays, d, tree))
    if n <= 64:
        assert (st.entries, st.survivors, st.rounds, st.closed_by_capacity, st.largest_round) == (1, n, 1, 0, n), st
        assert st.full_rounds == (1 if n == 64 else 0), st
    else:
        assert (st.entries, st.survivors, st.rounds, st.full_rounds, st.closed_by_capacity, st.largest_round) == \
            (2, 65, 2, 1, 1, 64), st
    assert st.closed_by_flags == 0, st
    assert float(got[:64].min()) > 0.0 and float(got[64:].max()) == 0.0
    _close_to_brute_force(oracle, rays, d, got)


# ---- the fat and the clamped body ---------------------------------------------------------------------

@pytest.mark.gpu
def test_a_fat_and_a_clamped_round_of_the_same_scene(gh, cuda, oracle):
    """44 column spheres, 24 in the first cluster and 20 in the second (40 fillers in front), with
    h just above or just below a third of the packet's origin diagonal.  All above, or all below:
    the two entries share their bits and form one round of 44.  The first cluster above and the
    second below: their fat bits differ and the round closes between them -- which shows that the
    two radii do lie on either side of the recorder's threshold, and runs both bodies in one call."""
    above, below = F32(FAT_H * 1.001), F32(FAT_H * 0.999)
    assert above * above >= F32(2.0 * PATCH_EXTENT ** 2 / 9.0 * 1.0001) > below * below
    rays = _patches(cuda)
    for column_h, rounds, by_flags in (([above] * 44, 1, 0), ([below] * 44, 1, 0), ([above] * 24 + [below] * 20, 2, 1)):
        d, tree = _column_of(gh, cuda, 40, column_h, 30)
        ref, got, st = _both(gh, lambda: _cumulative(gh, rays, d, tree))
        assert (st.entries, st.survivors, st.rounds, st.closed_by_flags, st.closed_by_capacity) == \
            (2, 44, rounds, by_flags, 0), (column_h[0], column_h[-1], st)
        assert float(got[:64].max()) > 0.0 and float(got[64:].max()) == 0.0
        _close_to_brute_force(oracle, rays, d, got)


# ---- full and partial last packets --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n_rays", [64, 65, 127, 128])
def test_full_and_partial_last_packets(gh, cuda, oracle, n_rays):
    """64 rays: one full packet (never planned: see the module's docstring); 65 and 127: a last
    packet with 1 and 63 live rays, its idle lanes re-tracing the last one, the column under it;
    128: two full packets."""
    d, tree = _column(gh, cuda, 20, 65, 30, at=0.8 if n_rays > 64 else 0.2)
    if n_rays == 64:
        rays = _patches(cuda, corners=((0.15, 0.15),))
    else:
        rays = _patches(cuda, corners=((0.4, 0.4), (0.75, 0.75)), last=n_rays - 64)
    assert len(rays) == n_rays
    call = lambda: _cumulative_c_abi(gh, rays, d, tree)
    if n_rays == 64:
        with gh.Context():
            gh.set_packet_width(64)
            ref = _plan_off(gh, call)
            got = call()
            got = call()
            assert gh.last_plan_used() == 0
        assert np.array_equal(_bits(got), _bits(ref))
    else:
        ref, got, st = _both(gh, call)
        assert (st.entries, st.rounds, st.closed_by_capacity) == (2, 2, 1), st
        assert float(got[:64].max()) == 0.0
    assert float(got[-(n_rays - 64 if n_rays > 64 else 64):].min()) > 0.0
    _close_to_brute_force(oracle, rays, d, got)


# ---- axes and senses ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sense", [1, -1])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_each_axis_and_sense(gh, cuda, oracle, axis, sense):
    d, tree = _column(gh, cuda, 20, 150, 30, axis=axis)      # 44 | 64 | 42: three rounds
    rays = _patches(cuda, axis=axis, sense=sense)
    ref, got, st = _both(gh, lambda: _cumulative(gh, rays, d, tree))
    assert (st.entries, st.survivors, st.rounds, st.full_rounds, st.largest_round) == (3, 150, 3, 1, 64), st
    assert float(got[:64].min()) > 0.0
    _close_to_brute_force(oracle, rays, d, got)


# ---- weighted sums ------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("fat", [True, False])
@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_weighted_sums_of_one_to_four_channels(gh, cuda, oracle, channels, fat):
    """Positive weights (a sum that cancels has no relative bound), one row of weights for the
    spheres of even index and one for the odd ones."""
    import torch
    h = COLUMN_H if fat else FAT_H * 0.999
    d, tree = _column_of(gh, cuda, 20, [h] * 150, 30)
    rays = _patches(cuda)
    rows = np.array([[0.5, 1.25, 2.0, 0.75], [1.5, 0.625, 1.0, 3.0]], F32)[:, :channels]
    w = torch.from_numpy(np.ascontiguousarray(rows[np.arange(len(d)) % 2])).to(cuda)
    ref, got, st = _both(gh, lambda: gh.trace_cumulative_weighted_sph(rays, d, tree, w, check=True))
    assert (st.entries, st.survivors, st.rounds) == (3, 150, 3), st
    assert tuple(got.shape) == (128, channels) and float(got[:64].max()) > 0.0
    _close_to_brute_force(oracle, rays, d, got, weights=w)


# ---- the packet split ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True])
def test_every_packet_split_gives_the_same_sums(gh, cuda, oracle, exact):
    """2100 column spheres lie in three granules, classes 0, 1 and 2: with K = 1, 2, 4, 8 waves per
    packet they fall to one, one, two and three waves.  The class sums and the order they are
    combined in are fixed, so every K -- and the automatic choice -- gives the same bits; each K's
    image is held against brute force: within 1e-5 of the fp64 sum on every ray, and with the
    exact integral the oracle's class-ordered fp32 sum bit for bit."""
    d, tree = _column(gh, cuda, 20, 2100, 30)
    rays = _patches(cuda)
    call = lambda: _cumulative(gh, rays, d, tree)
    ref32 = oracle.brute_cumulative(rays.cpu().numpy(), d.cpu().numpy())[0]
    with gh.Context():
        gh.set_packet_width(64)
        gh.set_exact_integrals(exact)
        ref = _plan_off(gh, call)
        auto, st = _from_plan(gh, call)
        assert st.survivors == 2100, st
        assert np.array_equal(_bits(auto), _bits(ref))
        _close_to_brute_force(oracle, rays, d, auto)
        for k in (1, 2, 4, 8):
            gh.set_packet_split(k)
            got = call()
            assert gh.last_plan_used() == 1, k
            assert np.array_equal(_bits(got), _bits(ref)), k
            _close_to_brute_force(oracle, rays, d, got)
            if exact:
                assert np.array_equal(_bits(got), ref32.view(np.uint32)), k
        gh.set_packet_split(-1)
        again = call()
        assert gh.last_plan_used() == 1
        assert np.array_equal(_bits(again), _bits(ref))
    assert float(ref[:64].min()) > 0.0


# 1 packet; one below the smallest shard of the sweep behind planned_split, that shard and the
# frame (2047, 2048, 16384); planned_split's threshold and its neighbour (8192, 8193).
PACKETS = [1, 2, 2047, 2048, 8192, 8193, 16384]


@pytest.fixture(scope="module")
def tiny_scene(gh, cuda):
    import torch
    rng = np.random.default_rng(77)
    s = np.empty((300, 4), F32)
    s[:, :3] = rng.random((300, 3), dtype=F32)
    s[:, 3] = F32(0.05) + F32(0.05) * rng.random(300, dtype=F32)
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(len(s), 32, device=cuda)
    gh.build_tree(d, tree, *BOX)
    # 1024 x 1024 rays along +z over the unit square, row by row
    u = (np.arange(1024, dtype=F32) + F32(0.5)) / F32(1024)
    a, b = [t.ravel() for t in np.meshgrid(u, u, indexing="ij")]
    r = np.zeros((1024 * 1024, 7), F32)
    r[:, 2] = 1.0
    r[:, 3], r[:, 4], r[:, 5], r[:, 6] = a, b, -0.2, 1.5
    return d, tree, torch.from_numpy(r).to(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("packets", PACKETS)
def test_the_automatic_split_on_n_packets(gh, cuda, oracle, tiny_scene, packets):
    """No override: the device chooses the ordinary kernels' split and the planned kernel's own.
    Both integrals.  Among 10^5 ... 10^6 rays through random spheres some graze a single sphere:
    the exact integral is the oracle's fp32 sum bit for bit and within 1e-5 of its fp64 sum on
    every ray; the fast one is held to conftest.check_column_densities, the project's 1e-5 with
    its allowance for a sum that is one grazing term (2e-6 of the largest possible term) -- a
    pure relative bound misses on such rays by 2e-4 ... 1e-3, planned and plan-off images being the
    same bits (profiles/trace_quad_reads_mi355x.txt, section 5)."""
    d, tree, all_rays = tiny_scene
    rays = all_rays[: packets * 64].contiguous()
    call = lambda: _cumulative(gh, rays, d, tree)
    ref32, ref64 = oracle.brute_cumulative(rays.cpu().numpy(), d.cpu().numpy())
    assert float(ref64.max()) > 0.0
    for exact in (False, True):
        with gh.Context():
            gh.set_packet_width(64)
            gh.set_exact_integrals(exact)
            ref = _plan_off(gh, call)
            if packets == 1:
                got = call()
                got = call()
                assert gh.last_plan_used() == 0     # (not reordered, hence not planned)
            else:
                got, st = _from_plan(gh, call)
                assert st.survivors > 0, st
        assert np.array_equal(_bits(got), _bits(ref))
        got = got.cpu().numpy()
        if exact:
            assert np.array_equal(got.view(np.uint32), ref32.view(np.uint32))
            assert np.all(np.abs(got - ref64) <= 1e-5 * np.abs(ref64))
        else:
            max_term = float(oracle.kernel_table()[0]) / float(d[:, 3].min()) ** 2
            check_column_densities(got, ref32, ref64, "fast", max_term=max_term)
