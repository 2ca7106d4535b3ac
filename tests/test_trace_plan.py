"""Packet plans of the column-density traces (grace_trace_set_plan, PacketPlan in csrc/trace_state.hpp).

Every case compares a call that runs from a recorded plan, bit for bit, with the same call in a
context that caches nothing (set_cache_auto(False): the ordinary kernels on freshly derived
records), and asserts through last_plan_used() that the planned kernel really ran -- or really did
not, where the case says so.

A plan is recorded by the first call that both caches serve: with automatic caching that is the
third call on the same arrays (seen, cached, served).  Batches of at most 64 rays are one packet,
have no ray order to cache and therefore never a plan: the 8 x 8 grids below assert exactly that."""
import numpy as np
import pytest

F32 = np.float32
SIDES = (8, 24, 64)           # one packet; ragged packets; 64 full packets
PRIMS = (33, 4096, 4097, 70001)   # one cluster range; exactly one group; one primitive into the next
                                  # group; a short last group after a class wrap (8 granules = 8192)


def _scene(gh, cuda, n, seed, hlo, hhi):
    import torch
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = (hlo + (hhi - hlo) * rng.random(n)).astype(F32)
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(n, 32, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))     # sorts d
    return d, tree


def _grid(cuda, side, direction):
    """side^2 orthographic rays over the unit square, along +z or -x.  Most start outside the box
    and cross it; every fifth starts inside it and every seventh stops short of its far side, so
    that rounds with range tests (not lean) are planned beside the test-free ones."""
    import torch
    u = (np.arange(side, dtype=F32) + F32(0.5)) / F32(side)
    a, b = np.meshgrid(u, u, indexing="ij")
    a, b = a.ravel(), b.ravel()
    n = side * side
    k = np.arange(n)
    depth = np.where(k % 5 == 0, F32(0.4), F32(-0.1)).astype(F32)     # the origin along the axis: in front of the box, or inside it
    length = np.where(k % 7 == 0, F32(0.5), F32(1.3)).astype(F32)
    r = np.zeros((n, 7), F32)
    if direction == "+z":
        r[:, 2] = 1.0
        r[:, 3], r[:, 4], r[:, 5] = a, b, depth
    else:
        r[:, 0] = -1.0
        r[:, 3], r[:, 4], r[:, 5] = F32(1.0) - depth, a, b
    r[:, 6] = length
    return torch.from_numpy(r).to(cuda)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _cumulative(gh, rays, d, tree):
    import torch
    out = torch.empty(len(rays), dtype=torch.float32, device=rays.device)
    gh.trace_cumulative_sph(rays, d, tree, out, check=True)
    return out


def _fresh(gh, call, exact=False, split=-1, width=-1, back=None):
    """`call()` in a context of its own that caches nothing: no plan can exist.  back: the context
    to make current again afterwards (leaving a context resets to the default one)."""
    with gh.Context():
        gh.set_cache_auto(False)
        gh.set_exact_integrals(exact)
        gh.set_packet_split(split)
        gh.set_packet_width(width)
        out = call()
        assert gh.last_plan_used() == 0
    if back is not None:
        back.make_current()
    return out


def _planned(gh, call, used=1, warm_used=0):
    """Third call on the same arrays: both caches serve it, it records the plan and runs from it
    (used = 0: it must find the batch unplannable and run the ordinary kernels)."""
    call(); call()
    # neither a first sight nor a cache fill launches anything new (warm_used = 1: a call that
    # traces twice -- more than four weight channels -- has its caches one call earlier)
    assert gh.last_plan_used() == warm_used
    out = call()
    assert gh.last_plan_used() == used
    again = call()
    assert gh.last_plan_used() == used
    assert np.array_equal(_bits(out), _bits(again))
    return again


@pytest.fixture(scope="module")
def scenes(gh, cuda):
    made = {}
    for n in PRIMS:
        # radii well above the ray spacing of every grid here: no lattice cull in the reference
        made[n] = _scene(gh, cuda, n, 11 + n % 7, 0.05 if n > 100 else 0.1, 0.09 if n > 100 else 0.2)
    return made


@pytest.mark.gpu
@pytest.mark.parametrize("direction", ["+z", "-x"])
@pytest.mark.parametrize("n_prims", PRIMS)
def test_planned_call_equals_the_uncached_call(gh, cuda, scenes, n_prims, direction):
    d, tree = scenes[n_prims]
    for side in SIDES:
        rays = _grid(cuda, side, direction)
        call = lambda: _cumulative(gh, rays, d, tree)
        ref = _fresh(gh, call)
        assert float(ref.max()) > 0.0
        with gh.Context():
            got = _planned(gh, call, used=1 if side * side > 64 else 0)
            if side * side > 64:
                assert gh.plan_bytes() > 0
        assert np.array_equal(_bits(got), _bits(ref)), (n_prims, side, direction)


@pytest.mark.gpu
def test_one_plan_serves_every_packet_split(gh, cuda, scenes):
    d, tree = scenes[70001]
    rays = _grid(cuda, 64, "+z")
    call = lambda: _cumulative(gh, rays, d, tree)
    with gh.Context() as ctx:
        gh.set_packet_width(64)       # (the automatic width of a small batch depends on the split knob)
        _planned(gh, call)
        size = gh.plan_bytes()
        for k in (-1, 1, 2, 4, 8):
            gh.set_packet_split(k)
            got = call()
            assert gh.last_plan_used() == 1 and gh.plan_bytes() == size, k
            ref = _fresh(gh, call, split=k, width=64, back=ctx)
            assert np.array_equal(_bits(got), _bits(ref)), k


@pytest.mark.gpu
def test_fast_and_exact_integrals_each_under_their_own_plan(gh, cuda, scenes, oracle):
    d, tree = scenes[33]
    rays = _grid(cuda, 24, "+z")
    call = lambda: _cumulative(gh, rays, d, tree)
    ref_fast, ref_exact = _fresh(gh, call), _fresh(gh, call, exact=True)
    # the smallest scene against brute force: exact mode is the oracle's fp32 sum bit for bit
    ref32, ref64 = oracle.brute_cumulative(rays.cpu().numpy(), d.cpu().numpy())
    assert np.array_equal(_bits(ref_exact), ref32.view(np.uint32))
    with gh.Context():
        got = _planned(gh, call)
        assert np.array_equal(_bits(got), _bits(ref_fast))
        for exact, ref in ((True, ref_exact), (False, ref_fast), (True, ref_exact)):
            gh.set_exact_integrals(exact)      # the cull bounds another b^2 expression: recorded again
            got = call()
            assert gh.last_plan_used() == 1
            assert np.array_equal(_bits(got), _bits(ref)), exact
        assert np.array_equal(_bits(got), ref32.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("channels", [1, 5])
def test_weighted_channels_share_one_plan(gh, cuda, scenes, channels, exact):
    import torch
    d, tree = scenes[70001]
    rays = _grid(cuda, 24, "-x")
    rng = np.random.default_rng(5 + channels)
    w = torch.from_numpy((rng.random((len(d), channels)).astype(F32) * F32(4.0) - F32(2.0))).to(cuda)
    call = lambda: gh.trace_cumulative_weighted_sph(rays, d, tree, w, check=True)
    ref = _fresh(gh, call, exact=exact)
    with gh.Context():
        gh.set_exact_integrals(exact)
        got = _planned(gh, call, warm_used=1 if channels > 4 else 0)   # five channels: two launches, one plan
        size = gh.plan_bytes()
        plain = _cumulative(gh, rays, d, tree)   # ... which the unweighted trace of the batch shares
        assert gh.last_plan_used() == 1 and gh.plan_bytes() == size
    assert np.array_equal(_bits(got), _bits(ref))
    assert np.array_equal(_bits(plain), _bits(_fresh(gh, lambda: _cumulative(gh, rays, d, tree), exact=exact)))


@pytest.mark.gpu
def test_sub_spacing_spheres_lattice_cull_is_in_the_masks(gh, cuda):
    """Spheres far smaller than the ray spacing (1/64): the uncached call runs the LAT kernels;
    the plan holds the lattice cull's result and gives the same bits."""
    d, tree = _scene(gh, cuda, 70001, 3, 0.001, 0.004)
    rays = _grid(cuda, 64, "+z")
    call = lambda: _cumulative(gh, rays, d, tree)
    with gh.Context():
        gh.set_cache_auto(False)
        ref = call()
        assert gh.last_lattice() == 1 and gh.last_plan_used() == 0
    with gh.Context():
        got = _planned(gh, call)
    assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.gpu
def test_a_batch_with_one_oblique_ray_has_no_plan(gh, cuda, scenes):
    d, tree = scenes[4097]
    rays = _grid(cuda, 24, "+z")
    rays[100, 0:3] = rays.new_tensor([0.6, 0.0, 0.8])
    call = lambda: _cumulative(gh, rays, d, tree)
    ref = _fresh(gh, call)
    with gh.Context():
        got = _planned(gh, call, used=0)
        assert gh.plan_bytes() == 0
    assert np.array_equal(_bits(got), _bits(ref))


@pytest.mark.gpu
def test_a_plan_beyond_the_byte_budget_is_not_kept(gh, cuda, scenes):
    d, tree = scenes[70001]
    rays = _grid(cuda, 64, "-x")
    call = lambda: _cumulative(gh, rays, d, tree)
    ref = _fresh(gh, call)
    with gh.Context():
        gh.set_plan_budget(4096)
        got = _planned(gh, call, used=0)
        assert gh.plan_bytes() == 0
        gh.set_plan_budget(512 << 20)
        again = call()
        assert gh.last_plan_used() == 1 and gh.plan_bytes() > 4096
        gh.set_plan(False)
        off = call()
        assert gh.last_plan_used() == 0 and gh.plan_bytes() == 0
    for t in (got, again, off):
        assert np.array_equal(_bits(t), _bits(ref))


@pytest.mark.gpu
def test_arrays_modified_in_place_are_planned_again(gh, cuda):
    """Spheres shrunk in place, rays moved along their axis in place, the tree rebuilt in place:
    each time the next call's signature check re-records the plan on the device (the lists can
    only get shorter here, so they fit their room) and the result is a fresh context's."""
    import torch
    d, tree = _scene(gh, cuda, 20000, 9, 0.03, 0.07)
    storage = gh.Tree(len(d), 32, device=cuda)      # the tree's arrays at full length (a build shrinks its views)
    nodes, leaves = storage.nodes, storage.leaves
    tree = gh.build_tree(d, storage, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    rays = _grid(cuda, 64, "+z")
    call = lambda: _cumulative(gh, rays, d, tree)
    with gh.Context() as ctx:
        got = _planned(gh, call)
        assert np.array_equal(_bits(got), _bits(_fresh(gh, call, back=ctx)))
        d[:, 3] *= 0.5
        got = call()
        assert gh.last_plan_used() == 1
        assert np.array_equal(_bits(got), _bits(_fresh(gh, call, back=ctx)))
        rays[:, 5] += 0.35            # more rays now start inside the box: other lean bits, same masks
        got = call()
        assert gh.last_plan_used() == 1
        assert np.array_equal(_bits(got), _bits(_fresh(gh, call, back=ctx)))
        d[:, 3] *= 0.9
        tree.nodes, tree.leaves = nodes, leaves     # rebuilt into the same arrays
        gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        got = call()
        assert gh.last_plan_used() == 1
        assert np.array_equal(_bits(got), _bits(_fresh(gh, call, back=ctx)))
        # a hit-count call in between re-derives the stale records; the plan must still notice
        d[:, 3] *= 0.8
        counts = torch.empty(len(rays), dtype=torch.int32, device=cuda)
        gh.trace_hitcounts_sph(rays, d, tree, counts)
        got = call()
        assert gh.last_plan_used() == 1
        assert np.array_equal(_bits(got), _bits(_fresh(gh, call, back=ctx)))


@pytest.mark.gpu
def test_trusted_mode_release_streams_and_contexts(gh, cuda, scenes):
    import torch
    d, tree = scenes[70001]
    rays = _grid(cuda, 64, "-x")
    call = lambda: _cumulative(gh, rays, d, tree)
    ref = _fresh(gh, call)
    with gh.Context():
        gh.set_cache_validation(False)
        gh.trace_prepare(d, tree)
        gh.trace_prepare_rays(rays)
        got = call()                               # prepared caches: the first call records the plan
        assert gh.last_plan_used() == 1 and gh.plan_bytes() > 0
        assert np.array_equal(_bits(got), _bits(ref))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = call()
            assert gh.last_plan_used() == 1
        side.synchronize()
        assert np.array_equal(_bits(got), _bits(ref))
        gh.trace_release_rays()
        assert gh.plan_bytes() == 0
        got = call()
        assert gh.last_plan_used() == 0
        assert np.array_equal(_bits(got), _bits(ref))
        gh.trace_release()
    # two contexts, each with a plan of its own over the same arrays
    a, b = gh.Context(), gh.Context()
    try:
        a.make_current()
        got_a = _planned(gh, call)
        b.make_current()
        got_b = _planned(gh, call)
        a.make_current()
        got_a2 = call()
        assert gh.last_plan_used() == 1
    finally:
        gh.Context.reset_current()
        a.destroy(); b.destroy()
    for t in (got_a, got_b, got_a2):
        assert np.array_equal(_bits(t), _bits(ref))
