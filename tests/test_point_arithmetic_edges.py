"""The fp32 arithmetic of the point walks at its rounding edges, on the GPU: SPH field and gradient at points,
gather sums of range queries, nearest neighbours and smoothing lengths on the cases of
point_arithmetic_cases.py (test_point_arithmetic_cases.py checks the cases themselves on the CPU).

Every comparison is bit for bit against the NumPy restatement of include/grace_hip.h.  Outputs are pre-filled
with 7.0 / -7; where the restatement holds NaN the GPU must hold NaN (any payload), everything else must agree
in bits.  The square roots are compared with roots from integer arithmetic, not with np.sqrt."""
import numpy as np
import pytest

import point_arithmetic_cases as PC
from point_arithmetic_cases import F32, KERNELS
from test_point_arithmetic_cases import sqrt_chunks


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _check(got, ref, what):
    """Bit for bit, except that a NaN of the restatement asks for a NaN of any payload."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if got.dtype != np.float32:
        bad = np.nonzero(got != ref)
    else:
        nan = np.isnan(ref)
        bad = np.nonzero((np.isnan(got) != nan) | (~nan & (_bits(got) != _bits(ref))))
    assert len(bad[0]) == 0, (what, len(bad[0]), [b[:4] for b in bad], got[bad][:4], ref[bad][:4])


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _build(gh, s, cuda, mpl=32, low=None, high=None):
    """(spheres on the device in tree order, tree, tree order on the host, perm: tree position -> row of s)."""
    d = _dev(np.asarray(s, F32), cuda)
    tree = gh.Tree(len(s), mpl, device=cuda)
    tree, perm = gh.build_tree(d, tree, low, high, want_perm=True)   # sorts d
    perm = perm.cpu().numpy().astype(np.int64)
    sh = d.cpu().numpy()
    assert np.array_equal(_bits(sh), _bits(np.asarray(s, F32)[perm]))
    return d, tree, sh, perm


def _field(gh, pts, d, tree, w, cuda, period=None):
    import torch
    out = torch.full((len(pts), w.shape[1]), 7.0, dtype=torch.float32, device=cuda)
    counts = torch.full((len(pts),), -7, dtype=torch.int32, device=cuda)
    gh.interpolate_sph(_dev(pts, cuda), d, tree, _dev(w, cuda), out=out, counts=counts, check=True, period=period)
    return out.cpu().numpy(), counts.cpu().numpy()


def _grad(gh, pts, d, tree, w, cuda, period=None):
    import torch
    n, C = len(pts), w.shape[1]
    grad = torch.full((n, C, 3), 7.0, dtype=torch.float32, device=cuda)
    value = torch.full((n, C), 7.0, dtype=torch.float32, device=cuda)
    counts = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    gh.interpolate_gradient_sph(_dev(pts, cuda), d, tree, _dev(w, cuda), grad=grad, value=value, counts=counts,
                                check=True, period=period)
    return grad.cpu().numpy(), value.cpu().numpy(), counts.cpu().numpy()


def _gather(gh, pts, radii, d, tree, w, cuda):
    import torch
    out = torch.full((len(pts), w.shape[1]), 7.0, dtype=torch.float32, device=cuda)
    counts = torch.full((len(pts),), -7, dtype=torch.int32, device=cuda)
    gh.range_counts_sph(_dev(pts, cuda), _dev(np.asarray(radii, F32), cuda), d, tree, weights=_dev(w, cuda),
                        counts=counts, out=out, check=True)
    return out.cpu().numpy(), counts.cpu().numpy()


def _check_point_queries(gh, pts, radii, d, tree, sh, w, kernel, cuda, what, pr=None, period=None):
    """Field, gradient (with value and counts) and, for an open scene, gather sums at pts against the
    restatement; returns what the GPU gave."""
    pr = PC.pairs(pts, sh) if pr is None else pr
    with np.errstate(all="ignore"):
        ref_f, ref_c, _, _ = PC.restate(len(pts), pr, sh, w, kernel)
        ref_g, _, _ = PC.restate_gradient(pts, pr, sh, w, kernel, period)
    f, c = _field(gh, pts, d, tree, w, cuda, period)
    _check(c, ref_c, (what, "field counts")); _check(f, ref_f, (what, "field"))
    g, v, gc = _grad(gh, pts, d, tree, w, cuda, period)
    _check(gc, ref_c, (what, "gradient counts")); _check(v, ref_f, (what, "gradient value"))
    _check(g, ref_g, (what, "gradient"))
    res = {"field": f, "counts": c, "grad": g}
    if radii is not None:
        lists = PC.restate_range(pts, radii, sh)
        with np.errstate(all="ignore"):
            ref_s = PC.restate_sums(pts, radii, sh, w, kernel, lists)
        s, sc = _gather(gh, pts, radii, d, tree, w, cuda)
        _check(sc, lists[0], (what, "range counts")); _check(s, ref_s, (what, "gather sums"))
        res.update(sums=s, range_counts=sc)
    return res


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


# ---- 1. square roots ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scale_exp", PC.SCALE_EXPS)
def test_smoothing_lengths_round_hard_square_roots(gh, cuda, scale_exp):
    """h = fl(eta * sqrt_rn(D)) with D = n 2^(2 scale_exp - 24) formed exactly, against the root from integer
    arithmetic: at 0 and 40 sqrt_rn's corrected hardware root, at -47 the same just above its switch, at -50
    the general square root below it.  Perfect squares, their neighbours, and the n whose roots lie nearest a
    midpoint of two floats (within 1e-3 ulp and closer: a 1-ulp root fails them)."""
    import torch
    for chunk in sqrt_chunks():
        sc = PC.sqrt_scene(chunk, scale_exp)
        d, tree, sh, perm = _build(gh, sc["spheres"], cuda)
        n = len(sh)
        root, D = sc["root"][perm], sc["D"][perm]
        to_tree = np.empty(n, np.int64); to_tree[perm] = np.arange(n)
        for eta in (1.0, 3.0):
            h = gh.smoothing_lengths_sph(d, tree, 2, eta, out=torch.full((n,), 7.0, device=cuda), check=True)
            _check(h.cpu().numpy(), (F32(eta) * root).astype(F32), ("h", scale_exp, eta))
        idx, d2 = gh.nearest_neighbours_sph(d, d, tree, 2, indices=torch.full((n, 2), -7, dtype=torch.int32, device=cuda),
                                            d2=torch.full((n, 2), 7.0, device=cuda), check=True)
        idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
        _check(idx, np.stack([np.arange(n), to_tree[sc["partner"][perm]]], axis=1).astype(np.int32), ("knn", scale_exp))
        _check(d2, np.stack([np.zeros(n, F32), D], axis=1), ("d2", scale_exp))


# ---- 2. kernel knots ----------------------------------------------------------------------------------
def knot_weights(sh):
    """Three channels: all ones; random; random on the spheres that have a radius and 0 on the others, which
    leaves the term of the one sphere a point belongs to alone in the gather sums."""
    rng = np.random.default_rng(len(sh))
    w = np.ones((len(sh), 3), F32)
    w[:, 1] = (0.5 + rng.random(len(sh))).astype(F32)
    w[:, 2] = np.where(sh[:, 3] > 0, (0.5 + rng.random(len(sh))).astype(F32), F32(0))
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_field_gradient_and_gather_sums_at_kernel_knots(gh, cuda, kernel, kernel_reset):
    """q hit exactly at every knot and clamp of f and f' with their neighbours, at the last floats below 1 where
    the powers of u pass through the subnormals to 0 (times ih^3, ih^4 up to 2^80 at H = 2^-20), at q == 1
    inside the support (u == 0) and at d2 == fl(H H), in range for the gather form only."""
    gh.set_sph_kernel(kernel)
    for H in PC.KNOT_H:
        for i, qs in enumerate(PC.knot_chunks(kernel)):
            sc = PC.knot_scene(qs, H)
            d, tree, sh, _ = _build(gh, sc["spheres"], cuda, 4)      # (the last chunk has ten spheres)
            res = _check_point_queries(gh, sc["points"], sc["radii"], d, tree, sh, knot_weights(sh), kernel, cuda,
                                       (kernel, H, i))
            assert np.all(res["counts"][:-1] == 1) and res["counts"][-1] == 0 and np.all(res["range_counts"] >= 2)


# ---- 3. the centre ------------------------------------------------------------------------------------
def _centre_checks(gh, cuda, sc, kernel, w, radii):
    d, tree, sh, perm = _build(gh, sc["spheres"], cuda, 1)          # (max_per_leaf 1: a tree needs a node)
    w = w[perm]
    pts = sc["points"]
    full = _check_point_queries(gh, pts, radii, d, tree, sh, w, kernel, cuda, (kernel, "points"))
    # the grid entry: a 4 x 4 x 4 brick from each centre in steps of 2^-70 (zero, subnormal and tiny d2 in one brick)
    import torch
    step = float(PC.two(-70))
    for c in PC.CENTRES:
        spec = (tuple(float(x) for x in c), (step, 0.0, 0.0), (0.0, step, 0.0), (0.0, 0.0, step), (4, 4, 4))
        gp = PC.lattice(*spec)
        pr = PC.pairs(gp, sh)
        with np.errstate(all="ignore"):
            ref_g, _, _ = PC.restate_gradient(gp, pr, sh, w, kernel)
            ref_f, ref_c, _, _ = PC.restate(len(gp), pr, sh, w, kernel)
        g, v, cnt = gh.interpolate_gradient_grid_sph(
            *spec, d, tree, _dev(w, cuda), grad=torch.full((4, 4, 4, w.shape[1], 3), 7.0, device=cuda),
            value=torch.full((4, 4, 4, w.shape[1]), 7.0, device=cuda),
            counts=torch.full((4, 4, 4), -7, dtype=torch.int32, device=cuda), check=True)
        _check(cnt.cpu().numpy().reshape(-1), ref_c, (kernel, "grid counts"))
        _check(v.cpu().numpy().reshape(len(gp), -1), ref_f, (kernel, "grid value"))
        _check(g.cpu().numpy().reshape(len(gp), -1, 3), ref_g, (kernel, "grid gradient"))
    return d, tree, sh, w, full


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["cubic", "wendland_c6"])
def test_near_centre_separations_in_one_packet(gh, cuda, kernel, kernel_reset):
    """d2 on both sides of 2^-96, subnormal, flushed to zero off the centre and zero at it, in one packet with
    ordinary q: the lanes disagree about sqrt_rn's switch, r is the root of a subnormal and 1 / r is near 2^70,
    and d2 == 0 selects +0 whether or not the point is the centre.  (The smallest root of a non-zero d2 is
    2^-74.5, so a select on r > t in place of d2 > 0 computes the same for every t below that; with t = 1e-20
    this test fails.)"""
    gh.set_sph_kernel(kernel)
    sc = PC.centre_scene()
    d, tree, sh, w, full = _centre_checks(gh, cuda, sc, kernel, PC.centre_weights(6), sc["radii"])
    assert np.all(np.isfinite(full["grad"])) and np.abs(full["grad"]).max() > 0
    # the points that are never tiny, alone: their bits do not depend on the path the wave took for the others
    keep = PC.never_tiny(sc)
    assert 8 <= keep.sum() < len(keep)
    alone = _check_point_queries(gh, sc["points"][keep], sc["radii"][keep], d, tree, sh, w, kernel, cuda, (kernel, "alone"))
    for name, a in alone.items():
        _check(a, full[name][keep], (kernel, "alone against all", name))


# ---- 4. overflow ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["cubic", "wendland_c6"])
def test_overflowing_inverse_powers_follow_ieee(gh, cuda, kernel, kernel_reset):
    """H = 2^-33: fl(ih^4) = +inf, so G = fl(E * inf); H = 2^-43: fl(ih^3) = +inf as well.  Infinities keep
    their sign, inf - inf and 0 * inf are NaN where the restatement has them, and nowhere else."""
    gh.set_sph_kernel(kernel)
    sc = PC.overflow_scene()
    w = PC.centre_weights(6)
    w[:, 1] *= np.where(np.arange(6) % 2, F32(-1), F32(1))           # mixed signs: inf - inf
    radii = np.where(np.arange(len(sc["points"])) % 2, PC.GATHER_RADIUS, F32(PC.OVERFLOW_RADII[2])).astype(F32)
    full = _centre_checks(gh, cuda, sc, kernel, w, radii)[4]
    for name in ("field", "grad", "sums"):
        assert np.isinf(full[name]).any() and np.isnan(full[name]).any() and np.isfinite(full[name]).any(), name


# ---- 5. scaled scenes ---------------------------------------------------------------------------------
_unit = {}


def unit_reference():
    """Counts and neighbours of the unscaled scene, in the generator's sphere order (computed once)."""
    if not _unit:
        sc = PC.scaled_scene(0)
        _unit["counts"] = np.bincount(PC.pairs(sc["points"], sc["spheres"])[0], minlength=len(sc["points"]))
        _unit["range_counts"] = PC.restate_range(sc["points"], sc["radii"], sc["spheres"])[0]
        _unit["knn"] = PC.brute_knn(sc["points"], sc["spheres"], 8)[0]
    return _unit


@pytest.mark.gpu
@pytest.mark.parametrize("k", PC.SCALES)
def test_scenes_scaled_by_powers_of_two(gh, cuda, k, kernel_reset):
    """Every cull widens relatively and sqrt_rn's switch is far away: a scene times 2^k gives the restatement
    at that scale, and the counts, neighbours and range counts of the unscaled scene."""
    import torch
    sc = PC.scaled_scene(k)
    d, tree, sh, perm = _build(gh, sc["spheres"], cuda, 32, sc["low"], sc["high"])
    w, pts, radii = sc["weights"][perm], sc["points"], sc["radii"]
    unit = unit_reference()
    for kernel in ("cubic", "wendland_c2"):
        gh.set_sph_kernel(kernel)
        res = _check_point_queries(gh, pts, radii, d, tree, sh, w, kernel, cuda, (k, kernel))
        assert np.array_equal(res["counts"], unit["counts"]) and np.array_equal(res["range_counts"], unit["range_counts"])
        assert np.all(np.isfinite(res["grad"])) and np.abs(res["grad"]).max() > 0
    n = len(pts)
    idx, d2 = gh.nearest_neighbours_sph(_dev(pts, cuda), d, tree, 8, check=True,
                                        indices=torch.full((n, 8), -7, dtype=torch.int32, device=cuda),
                                        d2=torch.full((n, 8), 7.0, device=cuda))
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    ref_idx, ref_d2 = PC.brute_knn(pts, sh, 8)
    _check(idx, ref_idx, (k, "knn")); _check(d2, ref_d2, (k, "knn d2"))
    assert np.array_equal(np.where(idx >= 0, perm[idx], -1), unit["knn"])
    h = gh.smoothing_lengths_sph(d, tree, 8, 1.2, out=torch.full((len(sh),), 7.0, device=cuda), check=True)
    _check(h.cpu().numpy(), PC.brute_h(sh, 8, 1.2), (k, "h"))


# ---- 6. the seam ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["cubic", "wendland_c4"])
def test_wrapped_separation_that_rounds_to_zero(gh, cuda, kernel, kernel_reset):
    """fl(p - x) rounds to L and wraps to exactly 0 for a point 2^-60 from the centre: counted, a value of
    w W(0), a gradient of +0; around it subnormal and one-ulp separations on both sides of both x faces."""
    gh.set_sph_kernel(kernel)
    case = PC.seam_case()
    d, tree, sh, _ = _build(gh, case["spheres"], cuda, 1)
    w = PC.centre_weights(len(sh), 2, 9)
    pts = case["points"]
    pr = PC.PS.pairs(pts, sh, case["period"])
    res = _check_point_queries(gh, pts, None, d, tree, sh, w, kernel, cuda, kernel, pr=pr, period=case["period"])
    named = case["named"]
    assert np.all(res["counts"][named] == 1) and np.all(res["field"][named] != 0)
    assert np.all(_bits(res["grad"][named]) == 0)


# ---- 7. the divergence / curl wrapper -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_gradient_div_curl_wrapper(gh, cuda, n):
    """gradient_div_curl itself: caller-supplied outputs come back as the same tensors, a non-contiguous grad
    gives the bits of its contiguous copy, inf, -0 and NaN follow the stated combinations, and a refused call
    leaves the outputs alone."""
    import torch
    rng = np.random.default_rng(n)
    g = (rng.random((n, 3, 3)) * 4.0 - 2.0).astype(F32)
    if n >= 255:                                                    # rows of special values, by position
        g[200:204] = 0.0
        g[200, 2, 1] = -0.0                                         # curl_x = fl(-0 - +0) = -0
        g[201, 0, 0], g[201, 1, 1] = np.inf, -np.inf                # div = inf - inf = NaN
        g[202, 0, 0], g[202, 2, 2] = np.inf, 1.0                    # div = +inf
        g[203, 2, 1], g[203, 1, 2], g[203, 0, 2] = np.inf, np.inf, np.nan   # curl = (NaN, NaN, 0)
    with np.errstate(invalid="ignore"):
        ref_div = ((g[:, 0, 0] + g[:, 1, 1]).astype(F32) + g[:, 2, 2]).astype(F32)
        ref_curl = np.stack([g[:, 2, 1] - g[:, 1, 2], g[:, 0, 2] - g[:, 2, 0], g[:, 1, 0] - g[:, 0, 1]],
                            axis=1).astype(F32).reshape(n, 3)
    if n >= 255:
        assert _bits(ref_curl[200]).tolist() == [0x80000000, 0, 0] and _bits(ref_div[200:201])[0] == 0
        assert np.isnan(ref_div[201]) and ref_div[202] == np.inf
        assert np.isnan(ref_curl[203]).tolist() == [True, True, False] and not np.isnan(ref_div[203])
    gd = _dev(g, cuda)
    div, curl = gh.gradient_div_curl(gd)                              # allocated
    assert tuple(div.shape) == (n,) and tuple(curl.shape) == (n, 3)
    _check(div.cpu().numpy(), ref_div, (n, "div")); _check(curl.cpu().numpy(), ref_curl, (n, "curl"))
    own_div = torch.full((n,), 7.0, device=cuda)
    own_curl = torch.full((n, 3), 7.0, device=cuda)
    r_div, r_curl = gh.gradient_div_curl(gd, div=own_div, curl=own_curl)
    assert r_div is own_div and r_curl is own_curl
    _check(own_div.cpu().numpy(), ref_div, (n, "own div")); _check(own_curl.cpu().numpy(), ref_curl, (n, "own curl"))
    wide = torch.full((n, 3, 5), 9.0, device=cuda)                   # a slice of a wider tensor
    wide[:, :, 1:4] = gd
    view = wide[:, :, 1:4]
    assert n < 2 or not view.is_contiguous()
    s_div, s_curl = gh.gradient_div_curl(view)
    _check(s_div.cpu().numpy(), ref_div, (n, "slice div")); _check(s_curl.cpu().numpy(), ref_curl, (n, "slice curl"))
    # refusals: ValueError, and the outputs keep their marker
    m_div, m_curl = torch.full((n,), 7.0, device=cuda), torch.full((n, 3), 7.0, device=cuda)
    bad = [dict(grad=torch.zeros((n, 3, 2), device=cuda)), dict(grad=torch.zeros((n, 9), device=cuda)),
           dict(grad=gd.double()), dict(div=torch.full((n + 1,), 7.0, device=cuda)),
           dict(curl=torch.full((n, 4), 7.0, device=cuda)), dict(curl=torch.full((n * 3,), 7.0, device=cuda)),
           dict(div=torch.full((n,), 7, dtype=torch.float64, device=cuda)),
           dict(curl=torch.full((n, 3), 7, dtype=torch.int32, device=cuda))]
    for kw in bad:
        args = dict(grad=gd, div=m_div, curl=m_curl); args.update(kw)
        with pytest.raises(ValueError):
            gh.gradient_div_curl(**args)
        torch.cuda.synchronize()
        for t in (args["div"], args["curl"], m_div, m_curl):
            assert torch.all(t == 7)
