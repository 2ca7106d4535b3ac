"""The packet plan's sub-tile layout (PLAN_FORMAT_SUBTILE, csrc/trace_state.hpp): one survivor
stream per quadrant of 16 rays, consumed by trace_kernel<.., PLANNED, SUBTILE> (unweighted, fast
integral, packets of 64 rays).  The layout is forced with set_plan_subtiles(1) except where the
automatic rule is the subject.

Every case compares three ways, as tests/test_trace_index_lists.py does: the planned call with the
same call with the plan switched off, bit for bit; the fast result with the oracle's brute force
through conftest.check_column_densities with its max_term allowance; and plan_subtiles() -- the
steps of the lists and the index words that name a survivor -- with the NumPy restatement of the
streams in tests/subtile_cases.py wherever the batch is a power-of-two pixel grid (whose quadrants
the restatement knows); other batches (ragged, jittered) are held to what must hold for any
quadrants: steps <= survivors and steps <= slots <= min(4 steps, 4 survivors).

The sphere at distance h "to the last bit": the recorder's bound is the rays' own b^2 expression
under the negated comparison !(b^2 >= h^2), so at EQUALITY the sphere is dropped -- no ray hits it
either -- and one ulp more of h keeps it; the negation keeps NaN centres and NaN bounds.  Both
sides of the edge are cases here."""
import numpy as np
import pytest

from conftest import check_column_densities
import subtile_cases as sc

F32 = np.float32


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _scene(gh, cuda, spheres):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(spheres, dtype=F32)).to(cuda)
    tree = gh.Tree(len(spheres), 32, device=cuda)
    gh.build_tree(d, tree, *sc.BOX)      # sorts d
    return d, tree


def _uniform(gh, cuda, n, seed, radius):
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = radius(s[:, :3]).astype(F32)
    return _scene(gh, cuda, s)


def _trace(gh, rays, d, tree):
    """trace_cumulative_sph through the C ABI: the binding wants a multiple of 32 rays, the library
    does not (a last packet of 17)."""
    import torch
    out = torch.empty(len(rays), dtype=torch.float32, device=rays.device)
    gh._check(gh._lib.grace_trace_cumulative_f4(*gh._trace_args(rays, d, tree), gh._ptr(out), gh._stream()))
    gh.trace_status()
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


def _check_oracle(oracle, got, rays, d):
    ss, rr = d.cpu().numpy(), rays.cpu().numpy()
    ref32, ref64 = oracle.brute_cumulative(rr, ss)
    max_term = float(oracle.kernel_table()[0]) / float(ss[:, 3].min()) ** 2
    check_column_densities(got.cpu().numpy(), ref32, ref64, "fast", max_term)
    return ref64


class _ThreeWays:
    """Plan-off and planned (sub-tile layout forced) results of one scene and batch in a context of
    its own, the plan's figures, and the comparisons.  expect: the restatement (sc.streams) or None."""

    def __init__(self, gh, oracle, rays_np, d, tree, split=-1, expect=None, brute=True):
        import torch
        rays = torch.from_numpy(np.ascontiguousarray(rays_np)).to(d.device)
        call = lambda: _trace(gh, rays, d, tree)
        with gh.Context():
            gh.set_packet_width(64)
            gh.set_packet_split(split)
            gh.set_plan_subtiles(1)
            ref = _plan_off(gh, call)
            got = _planned(gh, call)
            self.used, self.steps, self.slots = gh.plan_subtiles()
            self.st, self.loops, self.bytes = gh.plan_stats(), gh.plan_loops(), gh.plan_bytes()
        print("sub-tiles: used %d steps %d slots %d | %s | loops %s" % (self.used, self.steps, self.slots, self.st, self.loops))
        assert self.used == 1
        assert np.array_equal(_bits(got), _bits(ref))                       # 1. plan off, by bits
        self.got = got.cpu().numpy()
        if brute:
            self.ref64 = _check_oracle(oracle, got, rays, d)                # 2. fp64 brute force
        surv = self.st.survivors                                            # 3. the streams
        if expect is not None:
            print("restated: steps %d slots %d survivors %d" % (expect["steps"], expect["slots"], expect["survivors"]))
            assert (self.steps, self.slots, surv) == (expect["steps"], expect["slots"], expect["survivors"])
        assert self.steps <= surv
        assert self.steps <= self.slots <= min(4 * self.steps, 4 * surv)
        assert self.loops[1] <= sc.LOOP_MAX and self.st.largest_round <= 64


# ---- the cases are what they claim (CPU) -----------------------------------------------------------------

def test_the_hand_made_cases_are_what_they_claim():
    rays = sc.patch_rays()
    packet, quadrant = sc.grid_cells(rays, 2)
    assert len(rays) == 128 and set(packet) == {0, 1} and np.all(np.bincount(packet * 4 + quadrant) == 16)
    # a quadrant is a 4 x 4 block of pixels
    for p in (0, 1):
        for q in range(4):
            o = rays[(packet == p) & (quadrant == q)]
            assert len(np.unique(o[:, 3])) == 4 and len(np.unique(o[:, 4])) == 4

    def lens(placed):
        s = sc.spheres_at(placed)
        return sc.streams(s, rays)["lens"]      # (unsorted: every hand-made sphere is of class 0 either way)

    one = lens(sc.case_one_quadrant())
    assert one.sum() == 1 and sorted(one[0, 0]) == [0, 0, 0, 1] and one[1].sum() == 0
    seam = lens(sc.case_on_the_seam())
    assert seam.sum() == 2 and sorted(seam[0, 0]) == [0, 0, 1, 1]
    assert lens(sc.case_at_distance_h(0)).sum() == 0          # b^2 == h^2: dropped, like the ray's own hit
    edge = lens(sc.case_at_distance_h(1))
    assert edge.sum() == 1 and sorted(edge[0, 0]) == [0, 0, 0, 1]
    (u, v, h), = sc.case_at_distance_h(0)
    assert F32(u - sc.pixel(7)) == h and v == sc.pixel(5)     # the distance IS h, and q2 = 0
    for want in ((0, 1, 33, 130), (0, 1, 5, 31), (0, 1, 5, 32), (0, 1, 5, 33)):
        got = lens(sc.case_unequal(want))
        assert sorted(got[0, 0]) == sorted(want) and got[1].sum() == 0
    assert sc.round_headers(31) == [64, 60] and sc.round_headers(32) == [64, 64] and sc.round_headers(33) == [64, 64, 4]
    assert sc.expected_loops(lens(sc.case_unequal((0, 1, 5, 31)))) == (1, 124)
    assert sc.expected_loops(lens(sc.case_unequal((0, 1, 5, 32)))) == (1, 128)
    assert sc.expected_loops(lens(sc.case_unequal((0, 1, 5, 33)))) == (2, 128)
    assert sc.expected_loops(lens(sc.case_unequal((0, 1, 33, 130)))) == (5, 128)
    # a wide sphere reaches every quadrant of both packets
    wide = lens([(sc.pixel(3), sc.pixel(7), F32(0.2))])
    assert np.array_equal(wide[:, 0], [[1, 1, 1, 1], [1, 1, 1, 1]])
    # ragged and jittered batches are no pixel grid
    assert len(sc.patch_rays(keep=96)) == 96 and len(sc.patch_rays(keep=81)) == 81
    jit = sc.patch_rays(jitter=np.random.default_rng(1))
    assert len(np.unique(jit[:, 3])) > 8 and len(np.unique(jit[:, 4])) > 16


# ---- spheres placed by hand ----------------------------------------------------------------------------------

HAND = {
    "one quadrant": (sc.case_one_quadrant, (1, 1)),
    "on the seam": (sc.case_on_the_seam, (1, 2)),
    "at distance h": (lambda: sc.case_at_distance_h(0), (0, 0)),
    "one ulp inside h": (lambda: sc.case_at_distance_h(1), (1, 1)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HAND))
def test_spheres_placed_by_hand(gh, cuda, oracle, name):
    make, (steps, slots) = HAND[name]
    d, tree = _scene(gh, cuda, sc.spheres_at(make()))
    rays = sc.patch_rays()
    t = _ThreeWays(gh, oracle, rays, d, tree, expect=sc.streams(d.cpu().numpy(), rays))
    assert (t.steps, t.slots) == (steps, slots)
    if slots == 0:
        assert float(t.got.max()) == 0.0
    elif not name.startswith("one ulp"):
        assert float(t.got.max()) > 0.0


@pytest.mark.gpu
def test_a_nan_centre_is_in_all_four_streams(gh, cuda, oracle):
    """One cluster (n < 64) that also holds a sphere over the patch, so that its box reaches the
    rays; a filler's first co-ordinate becomes NaN after the build.  The NaN sphere passes every
    negated comparison: all four streams of packet 0, beside the one stream of the sphere over the
    patch.  (Packet 1 never sees the cluster: its box, formed without the NaN, ends short of it --
    the one cull that the restatement, which would put the NaN sphere into packet 1's streams as
    well, leaves out.)"""
    d, tree = _scene(gh, cuda, sc.spheres_at(sc.case_one_quadrant()))
    d[3, 0] = float("nan")
    rays = sc.patch_rays()
    want = sc.streams(d.cpu().numpy(), rays)
    assert sorted(want["lens"][0, 0]) == [1, 1, 1, 2] and sorted(want["lens"][1, 0]) == [1, 1, 1, 1]
    t = _ThreeWays(gh, oracle, rays, d, tree, brute=False)
    assert (t.steps, t.slots, t.st.survivors) == (2, 5, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [(0, 1, 33, 130), (0, 1, 5, 31), (0, 1, 5, 32), (0, 1, 5, 33)])
def test_streams_of_unequal_length_pad_with_the_null_record(gh, cuda, oracle, lens):
    d, tree = _scene(gh, cuda, sc.spheres_at(sc.case_unequal(lens)))
    rays = sc.patch_rays()
    want = sc.streams(d.cpu().numpy(), rays)
    t = _ThreeWays(gh, oracle, rays, d, tree, expect=want)
    assert (t.steps, t.slots) == (max(lens), sum(lens))
    assert t.loops == sc.expected_loops(want["lens"]), t.loops
    assert t.st.rounds == len(sc.round_headers(max(lens)))


@pytest.mark.gpu
def test_the_column_has_four_equal_streams_and_stays_format_3_by_itself(gh, cuda, oracle):
    import torch
    placed = [(sc.pixel(3), sc.pixel(7), F32(0.2))] * 90
    d, tree = _scene(gh, cuda, sc.spheres_at(placed))
    rays = sc.patch_rays()
    t = _ThreeWays(gh, oracle, rays, d, tree, expect=sc.streams(d.cpu().numpy(), rays))
    assert (t.steps, t.slots, t.st.survivors) == (2 * 90, 8 * 90, 2 * 90)
    rays_t = torch.from_numpy(rays).to(cuda)
    with gh.Context():                                   # the automatic setting
        gh.set_packet_width(64)
        got = _planned(gh, lambda: _trace(gh, rays_t, d, tree))
        assert gh.plan_subtiles() == (0, 0, 0) and gh.plan_stats().survivors == 2 * 90
    assert np.array_equal(_bits(got), t.got.view(np.uint32))


# ---- batches that are no grid -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("keep", [96, 81])     # a last packet of 32 and of 17 rays
def test_a_ragged_last_packet(gh, cuda, oracle, keep):
    placed = sc.case_unequal((3, 1, 5, 40)) + [(sc.pixel(2), sc.pixel(9), sc.H), (sc.pixel(6), sc.pixel(14), sc.H),
                                               (sc.pixel(3), sc.pixel(11), F32(0.2))]
    d, tree = _scene(gh, cuda, sc.spheres_at(placed))
    t = _ThreeWays(gh, oracle, sc.patch_rays(keep=keep), d, tree)
    assert len(t.got) == keep and float(t.got[64:].max()) > 0.0


@pytest.mark.gpu
def test_jittered_origins_take_their_rectangles_from_the_lanes(gh, cuda, oracle):
    d, tree = _uniform(gh, cuda, 5000, 41, lambda p: 0.02 + 0.02 * p[:, 1])
    rays = sc.patch_rays(nu=16, nv=16, jitter=np.random.default_rng(7))
    t = _ThreeWays(gh, oracle, rays, d, tree)
    assert t.slots > t.steps > 0


# ---- the kernel's paths -------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("sense", [1, -1])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_each_axis_and_sense(gh, cuda, oracle, axis, sense):
    d, tree = _scene(gh, cuda, sc.spheres_at(sc.case_unequal((0, 1, 5, 33)), axis=axis))
    rays = sc.patch_rays(axis=axis, sense=sense)
    t = _ThreeWays(gh, oracle, rays, d, tree, expect=sc.streams(d.cpu().numpy(), rays, axis))
    assert (t.steps, t.slots) == (33, 39) and float(t.got.max()) > 0.0


@pytest.fixture(scope="module")
def uniform_20000(gh, cuda):
    """20 000 spheres, h = 0.01 ... 0.03, and the streams of a 64 x 64 grid through them (the
    smaller spheres fall between the rays: the origin-lattice cull runs)."""
    d, tree = _uniform(gh, cuda, 20000, 42, lambda p: 0.01 + 0.02 * p[:, 0])
    rays = sc.grid_rays(64)
    return d, tree, rays, sc.streams(d.cpu().numpy(), rays)


@pytest.mark.gpu
def test_a_uniform_scene_under_a_grid(gh, cuda, oracle, uniform_20000):
    d, tree, rays, want = uniform_20000
    t = _ThreeWays(gh, oracle, rays, d, tree, expect=want)
    assert t.steps < 0.9 * t.st.survivors           # the streams do drop steps here
    assert t.loops[0] >= sc.expected_loops(want["lens"])[0]      # (more where the bits change)


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 2, 4, 8])
def test_each_packet_split(gh, cuda, oracle, uniform_20000, split):
    d, tree, rays, want = uniform_20000
    _ThreeWays(gh, oracle, rays, d, tree, split=split, expect=want)


@pytest.mark.gpu
def test_rays_ending_inside_the_box_run_the_tested_loop(gh, cuda, oracle, uniform_20000):
    """Rays from z = -0.1 to z = 0.5: rounds that hold a sphere near or behind the rays' ends are
    not lean and go through the tested survivor loop, 16 steps at the most; groups wholly behind
    the ends are culled ahead of the bound, so the streams are at most the restated ones."""
    d, tree, _, want = uniform_20000
    t = _ThreeWays(gh, oracle, sc.grid_rays(64, length=0.6), d, tree)
    assert 0 < t.slots <= want["slots"] and t.steps <= want["steps"]
    assert float(t.ref64.max()) > 0.0


@pytest.mark.gpu
def test_slabs_of_fat_and_thin_spheres_and_the_bits_of_drifting_streams(gh, cuda, oracle):
    """Slabs of radius 0.09 (fat under 64 x 64 rays) and 0.03 alternate along z every 0.25.  The
    four streams of a list drift apart, so a round holds words of neighbouring slabs: it is fat
    only if every real survivor in it is -- a fat round that held a thin sphere would read past
    the table, and the bits would differ from the plan-off call's."""
    d, tree = _uniform(gh, cuda, 20000, 32, lambda p: np.where(np.floor(p[:, 2] * 4.0) % 2 == 0, 0.09, 0.03))
    rays = sc.grid_rays(64)
    t = _ThreeWays(gh, oracle, rays, d, tree, expect=sc.streams(d.cpu().numpy(), rays))
    assert t.loops[0] >= sc.expected_loops(sc.streams(d.cpu().numpy(), rays)["lens"])[0]


# ---- re-record, budget, other calls ---------------------------------------------------------------------------

@pytest.mark.gpu
def test_an_edit_that_moves_a_sphere_to_the_next_quadrant_records_again_in_place(gh, cuda, oracle):
    import torch
    d, tree = _scene(gh, cuda, sc.spheres_at(sc.case_unequal((0, 1, 5, 33))))
    rays = sc.patch_rays()
    rays_t = torch.from_numpy(rays).to(cuda)
    d2 = d.clone()
    call = lambda: _trace(gh, rays_t, d2, tree)
    moved = int(torch.nonzero((d2[:, 0] == float(sc.pixel(6))) & (d2[:, 1] == float(sc.pixel(1))))[0])
    with gh.Context():
        gh.set_packet_width(64)
        gh.set_plan_subtiles(1)
        first = _planned(gh, call)
        size = gh.plan_bytes()
        assert gh.plan_subtiles() == (1, 33, 39)
        d2[moved, 0] = float(sc.pixel(1))              # quadrant (1, 0) -> (0, 0): streams (1, 1, 4, 33)
        got = call()
        assert gh.last_plan_used() == 1 and gh.plan_bytes() == size
        assert gh.plan_subtiles() == (1, 33, 39)
        d2[moved, 1] = float(sc.pixel(6))              # -> (0, 1): streams (0, 2, 4, 33)
        got = call()
        assert gh.last_plan_used() == 1 and gh.plan_bytes() == size
        want = sc.streams(d2.cpu().numpy(), rays)
        assert gh.plan_subtiles() == (1, want["steps"], want["slots"]) == (1, 33, 39)
        assert sorted(want["lens"][0, 0]) == [0, 2, 4, 33]
        again = call()
        ref = _plan_off(gh, call)
    assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(_bits(again), _bits(ref))
    assert not np.array_equal(_bits(first), _bits(ref))
    _check_oracle(oracle, got, rays_t, d2)


@pytest.mark.gpu
def test_an_edit_that_outgrows_the_room_falls_back(gh, cuda, oracle):
    """Twenty fillers grow until every ray meets them: the lists of packet 1 held nothing (room: 2
    steps) and now hold 20; the plan is unusable and the ordinary kernels run."""
    import torch
    d, tree = _scene(gh, cuda, sc.spheres_at(sc.case_unequal((0, 1, 5, 33))))
    rays_t = torch.from_numpy(sc.patch_rays()).to(cuda)
    d2 = d.clone()
    call = lambda: _trace(gh, rays_t, d2, tree)
    with gh.Context():
        gh.set_packet_width(64)
        gh.set_plan_subtiles(1)
        _planned(gh, call)
        assert gh.plan_subtiles()[0] == 1
        d2[:20, 3] = 0.9
        got = call()
        assert gh.last_plan_used() == 0 and gh.plan_subtiles() == (0, 0, 0)
        ref = _plan_off(gh, call)
    assert np.array_equal(_bits(got), _bits(ref))
    _check_oracle(oracle, got, rays_t, d2)


@pytest.mark.gpu
def test_budgets_between_and_below_the_two_layouts(gh, cuda, oracle):
    import torch
    placed = [(sc.pixel(3), sc.pixel(7), F32(0.2))] * 90
    d, tree = _scene(gh, cuda, sc.spheres_at(placed))
    rays_t = torch.from_numpy(sc.patch_rays()).to(cuda)
    call = lambda: _trace(gh, rays_t, d, tree)
    with gh.Context():
        gh.set_packet_width(64)
        ref = _plan_off(gh, call)
        gh.set_plan_subtiles(0)
        _planned(gh, call)
        bytes3 = gh.plan_bytes()
        gh.set_plan_subtiles(1)
        got4 = _planned(gh, call)
        bytes4 = gh.plan_bytes()
        assert gh.plan_subtiles()[0] == 1 and bytes4 > bytes3 > 0
        gh.set_plan_budget(bytes4 - 1)                 # below the sub-tile plan, above format 3's
        got3 = _planned(gh, call)
        assert gh.plan_subtiles() == (0, 0, 0) and gh.plan_bytes() == bytes3
        gh.set_plan_budget(bytes4)
        _planned(gh, call)
        assert gh.plan_subtiles()[0] == 1 and gh.plan_bytes() == bytes4
        gh.set_plan_budget(bytes3 - 1)                 # below both
        for _ in range(4):
            none = call()
            assert gh.last_plan_used() == 0 and gh.plan_bytes() == 0
    for out in (got4, got3, none):
        assert np.array_equal(_bits(out), _bits(ref))
    _check_oracle(oracle, got4, rays_t, d)


@pytest.mark.gpu
def test_a_weighted_call_between_two_unweighted_ones(gh, cuda, oracle, uniform_20000):
    import torch
    d, tree, rays, want = uniform_20000
    rays_t = torch.from_numpy(rays).to(cuda)
    w = torch.from_numpy(np.random.default_rng(9).random((len(d), 2)).astype(F32)).to(cuda)
    plain = lambda: _trace(gh, rays_t, d, tree)
    weighted = lambda: gh.trace_cumulative_weighted_sph(rays_t, d, tree, w, check=True)
    with gh.Context():
        gh.set_packet_width(64)
        ref, ref_w = _plan_off(gh, plain), _plan_off(gh, weighted)
        gh.set_plan_subtiles(1)
        a = _planned(gh, plain)
        assert gh.plan_subtiles() == (1, want["steps"], want["slots"])
        b = _planned(gh, weighted)                      # format 3: the weighted kernels read no sub-tiles
        assert gh.plan_subtiles() == (0, 0, 0) and gh.plan_stats().survivors == want["survivors"]
        c = _planned(gh, plain)
        assert gh.plan_subtiles() == (1, want["steps"], want["slots"])
    assert np.array_equal(_bits(a), _bits(ref)) and np.array_equal(_bits(c), _bits(ref))
    assert np.array_equal(_bits(b), _bits(ref_w))


# ---- the automatic rule ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def floor_rays(cuda):
    import torch
    return torch.from_numpy(sc.grid_rays(256, depth=-0.2, length=1.5)).to(cuda)     # 1024 packets


@pytest.mark.gpu
@pytest.mark.parametrize("spheres,packets,used", [("small", 1024, 1), ("small", 1023, 0), ("wide", 1024, 0), ("wide", 1023, 0)])
def test_the_automatic_rule_at_the_floor(gh, cuda, oracle, floor_rays, spheres, packets, used):
    """No knob: 1024 packets is the floor (PLAN_SUB_MIN_PACKETS), and the streams must drop steps
    (PLAN_SUB_MAX_RATIO = 0.82 of the survivors).  small: 4000 spheres of 1 ... 1.5 pixels in a thin
    slab across the rays -- the slab keeps a packet's few survivors in one or two classes, and they
    spread over quadrants of 4 pixels; wide: 300 spheres of 51 pixels and more, which reach every
    quadrant (steps = survivors) and stay format 3."""
    rng = np.random.default_rng(77)
    n = 4000 if spheres == "small" else 300
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    if spheres == "small":
        s[:, 2] = F32(0.5) + s[:, 2] / F32(64)
        s[:, 3] = F32(0.004) + F32(0.002) * rng.random(n, dtype=F32)
    else:
        s[:, 3] = F32(0.2) + F32(0.1) * rng.random(n, dtype=F32)
    d, tree = _scene(gh, cuda, s)
    rays = floor_rays[: packets * 64].contiguous()
    call = lambda: _trace(gh, rays, d, tree)
    with gh.Context():
        gh.set_packet_width(64)
        ref = _plan_off(gh, call)
        got = _planned(gh, call)
        sub, st = gh.plan_subtiles(), gh.plan_stats()
        print("automatic: %s | %s" % (sub, st))
        assert sub[0] == used and st.survivors > 0
        if used:
            assert sub[1] < 0.82 * st.survivors
    assert np.array_equal(_bits(got), _bits(ref))
    _check_oracle(oracle, got, rays, d)
