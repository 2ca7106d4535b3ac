"""SPH gradients at points in a periodic box (grace_interpolate_gradient_points_periodic_f4 /
grace_interpolate_gradient_grid_periodic_f4 through the `period` argument of interpolate_gradient_sph,
interpolate_gradient_grid_sph and divergence_curl_sph).

Bitwise against test_sph_gradients.restate_gradient with the wrapped separations, on the pairs and scenes of
periodic_point_scenes.py (interp_scene with special_H at its first spheres)."""
import numpy as np
import pytest

import periodic_point_scenes as PS
import periodic_query_scenes as S
from test_periodic_queries import _build, _dev
from test_sph_gradients import _grad, _same, restate_gradient
from test_sph_interpolation import lattice

F32 = np.float32
OPEN = (0.0, 0.0, 0.0)


def _weights(n, n_ch, seed):
    return (np.random.default_rng(seed).random((n, n_ch)) * 4.0 - 2.0).astype(F32)


def _face_points(box, offset, sh):
    """Points a few ulp and a small step inside and outside every face of the box, and at its low and high
    corners: with the spheres that S.uniform puts next to the faces, separations wrap on every axis."""
    ext = np.array([L if L > 0 else 1.0 for L in S.BOXES[box]], F32)
    o = F32(offset)
    mid = (o + F32(0.5) * ext).astype(F32)
    pts = []
    for k in range(3):
        for face in (o, o + ext[k]):
            for step in (-1e-3, -2.0 ** -20, 0.0, 2.0 ** -20, 1e-3):
                p = mid.copy(); p[k] = F32(face) + F32(step) * ext[k]
                pts.append(p)
    for step in (-1e-3, 0.0, 1e-3):
        pts.append((o + F32(step) * ext).astype(F32))
        pts.append((o + ext + F32(step) * ext).astype(F32))
    near = sh[np.argsort(np.min(np.minimum(sh[:, :3] - o, o + ext - sh[:, :3]), axis=1))[:60], :3]   # centres next to faces
    return np.concatenate([np.array(pts, F32), near]).astype(F32)


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


@pytest.mark.gpu
@pytest.mark.parametrize("offset", S.OFFSETS)
@pytest.mark.parametrize("box", list(S.BOXES))                      # slab: periodic x and y of unequal length, z open
def test_periodic_gradient_is_the_restatement_bit_for_bit(gh, cuda, box, offset, kernel_reset):
    period = S.BOXES[box]
    d, tree, sh = _build(gh, PS.interp_scene(box, offset, 11), cuda)
    pts = np.concatenate([_face_points(box, offset, sh), S.uniform_queries(sh, box, offset, 11, 300)[0]]).astype(F32)
    pr = PS.pairs(pts, sh, period)
    w = _weights(len(sh), 2, 13)
    for kernel in ("cubic", "wendland_c4"):
        gh.set_sph_kernel(kernel)
        grad, value, counts = _grad(gh, pts, d, tree, w, cuda, period)
        ref32, ref64, bound = restate_gradient(pts, pr, sh, w, kernel, period)
        bad = np.nonzero(grad.view(np.uint32) != ref32.view(np.uint32))
        assert len(bad[0]) == 0, (box, offset, kernel, bad[0][:5], grad[bad][:5], ref32[bad][:5])
        assert np.array_equal(counts, np.bincount(pr[0], minlength=len(pts)))
        assert np.all(np.abs(grad - ref64) <= bound + 1e-30)
        import torch
        f_cnt = torch.empty(len(pts), dtype=torch.int32, device=cuda)
        f_out, f_cnt = gh.interpolate_sph(_dev(pts, cuda), d, tree, _dev(w, cuda), counts=f_cnt, check=True, period=period)
        assert _same(value, f_out.cpu().numpy()) and np.array_equal(counts, f_cnt.cpu().numpy())
    # the wrap matters: the open gradient differs, and some separations were wrapped
    open_grad = _grad(gh, pts, d, tree, w, cuda)[0]
    assert np.sum(np.any(open_grad != grad, axis=(1, 2))) > 20
    # a sphere with H above half a period contributes nothing: alone with a weight, it leaves zeros
    off = ~PS.sphere_on(sh, period)
    assert off.sum() >= 1 and not np.any(np.isin(pr[1], np.nonzero(off)[0]))
    w_off = np.where(off[:, None], F32(3), F32(0)).astype(F32)
    g_off, v_off, _ = _grad(gh, pts, d, tree, w_off, cuda, period)
    assert np.all(g_off == 0) and np.all(v_off == 0)
    assert np.abs(_grad(gh, pts, d, tree, w_off, cuda)[0]).max() > 0   # (open, it covers points)


@pytest.mark.gpu
def test_no_wrap_periods_give_the_open_gradient(gh, cuda):
    import torch
    d, tree, sh = _build(gh, PS.interp_scene("cube", 0.0, 21), cuda)
    pts = S.uniform_queries(sh, "cube", 0.0, 21, 500)[0]
    w = _weights(len(sh), 3, 6)
    plain = _grad(gh, pts, d, tree, w, cuda)
    grid = ((0.0, 0.0, 0.0), (0.125, 0.0, 0.0), (0.0, 0.125, 0.0), (0.0, 0.0, 0.125), (8, 8, 8))
    plain_grid = gh.interpolate_gradient_grid_sph(*grid, d, tree, _dev(w, cuda), check=True)[0].cpu().numpy()
    for period in (OPEN, (1e6, 1e6, 1e6)):
        got = _grad(gh, pts, d, tree, w, cuda, period)
        assert _same(got[0], plain[0]) and _same(got[1], plain[1]) and np.array_equal(got[2], plain[2]), period
        g = gh.interpolate_gradient_grid_sph(*grid, d, tree, _dev(w, cuda), check=True, period=period)[0]
        assert _same(g.cpu().numpy(), plain_grid), period
    # the periodic grid entry is the periodic points entry on the lattice; divergence and curl follow the period
    cube = S.BOXES["cube"]
    g = gh.interpolate_gradient_grid_sph(*grid, d, tree, _dev(w, cuda), check=True, period=cube)[0].cpu().numpy()
    lp = lattice(*grid)
    per = _grad(gh, lp, d, tree, w, cuda, cube)[0]
    assert _same(g.reshape(-1, 3, 3), per) and not _same(g, plain_grid)
    div, curl = gh.divergence_curl_sph(_dev(lp, cuda), d, tree, _dev(w, cuda), period=cube)
    assert _same(div.cpu().numpy(), ((per[:, 0, 0] + per[:, 1, 1]).astype(F32) + per[:, 2, 2]).astype(F32))
    assert _same(curl.cpu().numpy()[:, 0], (per[:, 2, 1] - per[:, 1, 2]).astype(F32))
    torch.cuda.synchronize()
