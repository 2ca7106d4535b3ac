"""The periodic traces on the GPU (periodic_scene, periodic_sphere_images, periodic_ray_segments,
trace_hitcounts_periodic_sph, trace_cumulative_periodic_sph, trace_cumulative_weighted_periodic_sph,
project_sph(period=...)) against the NumPy restatement of periodic_trace_scenes.py, on its scenes;
test_periodic_trace_scenes.py checks the restatement itself.

Images, sources, segments and offsets are compared bit for bit, hit counts exactly, column densities
bit for bit with the stated fold of the open trace on the explicit segments and images, and within the
project's stated 1e-5 of the fp64 sum of the per-hit integrals over the restated hits."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import periodic_trace_scenes as S
from test_periodic_trace_scenes import compile_dropin
from test_range_queries import digest

F32, F64 = np.float32, np.float64
BOXES = sorted(S.BOXES)
OPEN = np.zeros(3, F32)


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(cuda)               # (a copy: the scenes are read-only)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@functools.lru_cache(maxsize=None)
def ordered_rays(box):
    """Every ray of the box, the ones with cuts first (so that the first 1 .. 257 are not all plain)."""
    r = S.rays(box)
    first = ("oblique", "plane", "from_face", "axis", "zero_length", "corner", "edge", "inside", "grid")
    return np.concatenate([r[k] for k in first])


@functools.lru_cache(maxsize=None)
def restated(box):
    """(images, source, image offsets, segments, segment offsets) of the box's scene, computed once."""
    lo, period = S.BOXES[box]
    imgs, source, ioff, _ = S.images(S.spheres(box), lo, period)
    segs, soff = S.segments(ordered_rays(box), lo, period)[:2]
    return imgs, source, ioff, segs, soff


def open_trace(gh, rays, spheres, tree, weights=None, counts=False):
    """The open traces through the C entry points, which take any number of rays."""
    import torch
    args = gh._trace_args(rays, spheres, tree)
    if counts:
        out = torch.empty(len(rays), dtype=torch.int32, device=rays.device)
        gh._check(gh._lib.grace_trace_hitcounts_f4(*args, gh._ptr(out), gh._stream()))
    elif weights is None:
        out = torch.empty(len(rays), dtype=torch.float32, device=rays.device)
        gh._check(gh._lib.grace_trace_cumulative_f4(*args, gh._ptr(out), gh._stream()))
    else:
        out = torch.empty((len(rays), weights.shape[1]), dtype=torch.float32, device=rays.device)
        gh._check(gh._lib.grace_trace_cumulative_weighted_f4(*args, gh._ptr(weights), C.c_int(weights.shape[1]),
                                                             gh._ptr(out), gh._stream()))
    gh.trace_status()
    return out.cpu().numpy()


def fp64_columns(gh, cuda, segs, soff, imgs, weights=None):
    """Per ray (and channel): the fp64 sum, over the restated hits of its segments, of w * the per-hit
    integral in the traversal's own arithmetic (hit_integrals); and the same sum of |w| I."""
    s, i, b2 = S.hits(segs, imgs)
    integ = gh.hit_integrals(_dev(b2, cuda), _dev(imgs[i, 3], cuda)).cpu().numpy().astype(F64)
    row = np.searchsorted(soff, s, side="right") - 1
    w = np.ones((len(imgs), 1), F64) if weights is None else weights.astype(F64)
    ref = np.zeros((len(soff) - 1, w.shape[1]), F64); mag = np.zeros_like(ref)
    np.add.at(ref, row, w[i] * integ[:, None])
    np.add.at(mag, row, np.abs(w[i]) * integ[:, None])
    return ref, mag


def check_columns(got, ref, mag, mode, max_term):
    """The project's stated tolerance (tests/conftest.py check_column_densities): 1e-5 of the fp64 sum; in the
    default mode a ray of a few grazing hits also gets the fast evaluation's absolute 2e-6 of its largest
    possible term.  Printed before it is asserted."""
    got = got.reshape(ref.shape).astype(F64)
    atol = 0.0 if mode == "exact" else 2e-6 * max_term
    err = np.abs(got - ref)
    print("column densities (%s): max err / (1e-5 sum + atol) = %.3g" % (mode, np.max(err / (1e-5 * mag + atol + 1e-300))))
    bad = np.nonzero(err > 1e-5 * mag + atol)
    assert len(bad[0]) == 0, (bad[0][:5], got[bad][:5], ref[bad][:5])


@pytest.fixture(scope="module")
def scenes(gh, cuda):
    """box -> (PeriodicScene, the caller's spheres on the device, all rays on the device)."""
    out = {}
    for box in BOXES:
        lo, period = S.BOXES[box]
        d = _dev(S.spheres(box), cuda)
        out[box] = (gh.periodic_scene(d, lo, period), d, _dev(ordered_rays(box), cuda))
    return out


# ---- the two sets ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES)
def test_images_and_segments_are_the_restatement_bit_for_bit(gh, cuda, box):
    lo, period = S.BOXES[box]
    s, r = S.spheres(box), ordered_rays(box)
    imgs, source, ioff, segs, soff = restated(box)
    for n in S.SIZES + (len(s),):
        g_img, g_src, g_off = (t.cpu().numpy() for t in gh.periodic_sphere_images(_dev(s[:n], cuda), lo, period))
        m = ioff[n]
        assert np.array_equal(g_off, ioff[:n + 1]), n
        assert _same(g_img, imgs[:m]) and np.array_equal(g_src, source[:m]), n
    for n in S.SIZES + (len(r),):
        g_seg, g_off = (t.cpu().numpy() for t in gh.periodic_ray_segments(_dev(r[:n], cuda), lo, period))
        m = soff[n]
        assert np.array_equal(g_off, soff[:n + 1]), n
        bad = np.nonzero(np.any(g_seg.view(np.uint32) != segs[:m].view(np.uint32), axis=1))[0]
        assert len(bad) == 0, (n, bad[:5], g_seg[bad[:2]], segs[bad[:2]])
    gh.trace_status()                                             # nothing was refused
    # open axes: images == spheres, source == identity, segments == rays
    g_img, g_src, _ = gh.periodic_sphere_images(_dev(s, cuda), lo, OPEN)
    assert _same(g_img.cpu().numpy(), s) and np.array_equal(g_src.cpu().numpy(), np.arange(len(s)))
    g_seg, g_off = gh.periodic_ray_segments(_dev(r, cuda), lo, OPEN)
    assert _same(g_seg.cpu().numpy(), r) and np.array_equal(g_off.cpu().numpy(), np.arange(len(r) + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES)
def test_scene_carries_the_sources_into_tree_order(gh, scenes, box):
    scene, d, _ = scenes[box]
    imgs, source = restated(box)[:2]
    g_img, g_src = scene.spheres.cpu().numpy(), scene.source.cpu().numpy()
    key = lambda im, src: np.lexsort((im[:, 3], im[:, 2], im[:, 1], im[:, 0], src))
    a, b = key(g_img, g_src), key(imgs, source)
    assert _same(g_img[a], imgs[b]) and np.array_equal(g_src[a], source[b])
    assert np.array_equal(S.spheres(box), d.cpu().numpy())          # the caller's array is untouched
    assert np.any(np.diff(g_src) < 0)                                # (tree order, not the caller's)


@pytest.mark.gpu
def test_refusals_set_the_status_word_and_emit_the_input(gh, cuda):
    for box in BOXES:
        lo, period = S.BOXES[box]
        s, r = S.refusals(box)
        ref_img, ref_src, ref_off, _ = S.images(s, lo, period)
        gh.trace_status()
        g_img, g_src, g_off = gh.periodic_sphere_images(_dev(s, cuda), lo, period)
        with pytest.raises(ValueError):
            gh.trace_status()
        assert _same(g_img.cpu().numpy(), ref_img) and np.array_equal(g_src.cpu().numpy(), ref_src)
        assert np.array_equal(g_off.cpu().numpy(), ref_off)
        with pytest.raises(ValueError):
            gh.periodic_scene(_dev(s, cuda), lo, period)
        for bad in (2, 5):                                           # each refusal on its own
            one = S.spheres(box)[:8].copy(); one[bad] = s[bad]
            gh.periodic_sphere_images(_dev(one, cuda), lo, period)
            with pytest.raises(ValueError):
                gh.trace_status()
        ref_seg, ref_off = S.segments(r, lo, period)[:2]
        g_seg, g_off = gh.periodic_ray_segments(_dev(r, cuda), lo, period)
        with pytest.raises(ValueError):
            gh.trace_status()
        assert _same(g_seg.cpu().numpy(), ref_seg) and np.array_equal(g_off.cpu().numpy(), ref_off)
        gh.trace_status()                                            # read once, then clean
    lo, period = S.BOXES["cube"]
    # 65 536 segments are legal, one more is not; a non-finite ray is emitted as itself without a report
    ray = np.array([[1, 0, 0, 0.5, 0.5, 0.5, 65535.25], [1, 0, 0, 0.5, np.nan, 0.5, 3.0]], F32)
    g_seg, g_off = gh.periodic_ray_segments(_dev(ray, cuda), lo, period)
    gh.trace_status()
    ref_seg, ref_off = S.segments(ray, lo, period)[:2]
    assert list(np.diff(ref_off)) == [65536, 1]
    assert np.array_equal(g_off.cpu().numpy(), ref_off)
    assert np.array_equal(g_seg.cpu().numpy().view(np.uint32), ref_seg.view(np.uint32))
    ray[0, 6] = 65536.75
    g_seg, g_off = gh.periodic_ray_segments(_dev(ray, cuda), lo, period)
    with pytest.raises(ValueError):
        gh.trace_status()
    assert list(np.diff(g_off.cpu().numpy())) == [1, 1] and np.array_equal(g_seg.cpu().numpy().view(np.uint32), ray.view(np.uint32))
    # a sphere with a non-finite member: once, no report
    s = S.spheres("cube")[:4].copy(); s[1, 0] = np.inf
    g_img, g_src, _ = gh.periodic_sphere_images(_dev(s, cuda), lo, period)
    gh.trace_status()
    ref = S.images(s, lo, period)
    assert np.array_equal(g_img.cpu().numpy().view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(g_src.cpu().numpy(), ref[1])
    # a bad box is refused before anything runs
    for bad in ((1.0, -1.0, 1.0), (1.0, np.inf, 1.0), (np.nan, 1.0, 1.0)):
        with pytest.raises(ValueError):
            gh.periodic_ray_segments(_dev(ray, cuda), lo, bad)
        with pytest.raises(ValueError):
            gh.periodic_sphere_images(_dev(s, cuda), lo, bad)
    with pytest.raises(ValueError):
        gh.periodic_ray_segments(_dev(ray, cuda), (0.0, np.inf, 0.0), period)


# ---- results --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES)
def test_hit_counts_are_the_restated_hits_summed(gh, cuda, scenes, box):
    scene, _, rays = scenes[box]
    imgs, _, _, segs, soff = restated(box)
    s, _, _ = S.hits(segs, imgs)
    ref = S.fold(np.bincount(s, minlength=len(segs)).astype(np.int32), soff)
    got = gh.trace_hitcounts_periodic_sph(rays, scene, check=True).cpu().numpy()
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (bad[:5], got[bad[:5]], ref[bad[:5]])
    assert ref.sum() > 20000
    lo, period = S.BOXES[box]
    open_counts = open_trace(gh, rays, scene.spheres, scene.tree, counts=True)
    assert np.count_nonzero(got != open_counts) > 100                # the box matters
    for n in S.SIZES:
        part = gh.trace_hitcounts_periodic_sph(rays[:n].contiguous(), scene, check=True).cpu().numpy()
        assert np.array_equal(part, ref[:n]), n


@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES)
def test_column_densities(gh, cuda, scenes, box, integral_mode):
    scene, _, rays = scenes[box]
    lo, period = S.BOXES[box]
    got = gh.trace_cumulative_periodic_sph(rays, scene, check=True).cpu().numpy()
    # the stated fold of the open trace on the explicit segments and images, bit for bit
    segs, soff = gh.periodic_ray_segments(rays, lo, period)
    per_segment = open_trace(gh, segs, scene.spheres, scene.tree)
    assert _same(got, S.fold(per_segment, soff.cpu().numpy()))
    # the fp64 sum over the restated hits
    imgs = scene.spheres.cpu().numpy()
    ref, mag = fp64_columns(gh, cuda, restated(box)[3], restated(box)[4], imgs)
    assert np.count_nonzero(ref) > 0.5 * len(ref)
    check_columns(got, ref, mag, integral_mode, 1.91 / float(imgs[:, 3].min()) ** 2)
    for n in (1, 65, 257):
        part = gh.trace_cumulative_periodic_sph(rays[:n].contiguous(), scene, check=True).cpu().numpy()
        ref_n, mag_n = ref[:n], mag[:n]
        check_columns(part, ref_n, mag_n, integral_mode, 1.91 / float(imgs[:, 3].min()) ** 2)


@pytest.mark.gpu
@pytest.mark.parametrize("n_ch", [1, 5])
@pytest.mark.parametrize("box", BOXES)
def test_weighted_column_densities(gh, cuda, scenes, box, n_ch, integral_mode):
    scene, d, rays = scenes[box]
    lo, period = S.BOXES[box]
    w = (0.5 + np.random.default_rng(7).random((len(d), n_ch))).astype(F32)
    wd = _dev(w[:, 0] if n_ch == 1 else w, cuda)
    got = gh.trace_cumulative_weighted_periodic_sph(rays, scene, wd, check=True).cpu().numpy()
    assert got.shape == ((len(rays),) if n_ch == 1 else (len(rays), n_ch))
    source = scene.source.cpu().numpy()
    segs, soff = gh.periodic_ray_segments(rays, lo, period)
    per_segment = open_trace(gh, segs, scene.spheres, scene.tree, weights=_dev(w[source], cuda))
    assert _same(got.reshape(len(rays), n_ch), S.fold(per_segment, soff.cpu().numpy()))
    imgs = scene.spheres.cpu().numpy()
    ref, mag = fp64_columns(gh, cuda, restated(box)[3], restated(box)[4], imgs, w[source])
    check_columns(got, ref, mag, integral_mode, 1.5 * 1.91 / float(imgs[:, 3].min()) ** 2)
    # unit weights give the unweighted bits
    ones = _dev(np.ones(len(d), F32), cuda)
    unit = gh.trace_cumulative_weighted_periodic_sph(rays, scene, ones, check=True).cpu().numpy()
    assert _same(unit, gh.trace_cumulative_periodic_sph(rays, scene, check=True).cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES)
def test_open_axes_and_a_huge_box_give_the_open_trace(gh, cuda, box):
    import torch
    lo, period = S.BOXES[box]
    s, r = S.spheres(box), ordered_rays(box)
    d = _dev(s, cuda)
    tree = gh.Tree(len(d), 32, device=cuda)
    gh.build_tree(d, tree)
    rays = _dev(r, cuda)
    want_c = open_trace(gh, rays, d, tree, counts=True)
    want = open_trace(gh, rays, d, tree)
    w = (0.5 + np.random.default_rng(9).random((len(s), 5))).astype(F32)
    for L, origin in ((OPEN, lo), (np.full(3, 4096.0, F32), np.full(3, -1024.0, F32))):
        scene = gh.periodic_scene(_dev(s, cuda), origin, L)
        assert _same(scene.spheres.cpu().numpy(), d.cpu().numpy())
        perm = scene.source.cpu().numpy()
        assert np.array_equal(s[perm], d.cpu().numpy())
        assert np.array_equal(gh.trace_hitcounts_periodic_sph(rays, scene, check=True).cpu().numpy(), want_c)
        assert _same(gh.trace_cumulative_periodic_sph(rays, scene, check=True).cpu().numpy(), want)
        got_w = gh.trace_cumulative_weighted_periodic_sph(rays, scene, _dev(w, cuda), check=True).cpu().numpy()
        assert _same(got_w, open_trace(gh, rays, d, tree, weights=_dev(w[perm], cuda)))
    assert want_c.sum() > 10000 and torch.cuda.is_available()


@pytest.mark.gpu
@pytest.mark.parametrize("box", BOXES)
def test_dyadic_torus_invariance(gh, cuda, box):
    """Coordinates, H and origins on the 2^-10 grid, axis-aligned rays: a shift of the centres (wrapped)
    and the origins by grid vectors is exact in fp32, so every hit count is unchanged."""
    lo, period = S.BOXES[box]
    s, r = S.dyadic(box)
    base = None
    for shift in ((0, 0, 0), (301, -77, 1030), (-1024, 512, 5), (2047, 2049, -3071)):
        s2, r2 = S.dyadic_shift(s, r, lo, period, np.array(shift) / 1024.0)
        scene = gh.periodic_scene(_dev(s2, cuda), lo, period)
        got = gh.trace_hitcounts_periodic_sph(_dev(r2, cuda), scene, check=True).cpu().numpy()
        if base is None:
            base = got
            assert np.array_equal(got, S.hitcounts(r, s, lo, period)[:len(got)]) and got.sum() > 2000
        assert np.array_equal(got, base), shift


@pytest.mark.gpu
def test_project_sph_maps_the_whole_box(gh, cuda):
    """project_sph(period=...): the frame is the box face, the rays span one period from the top face,
    and the map holds what sticks in through the side faces: every pixel is the restated periodic sum."""
    lo, period = S.BOXES["cube"]
    s = S.spheres("cube")
    image, scene, rays = gh.project_sph(_dev(s, cuda), 32, period=period, lo=lo)
    r = rays.cpu().numpy()
    assert np.all(r[:, 2] == -1) and np.all(r[:, 5] == lo[2] + period[2]) and np.all(r[:, 6] == period[2])
    assert r[:, 3].min() > lo[0] and r[:, 3].max() < lo[0] + period[0]
    assert np.allclose(np.sort(np.unique(r[:, 3])), lo[0] + (np.arange(32) + 0.5) / 32 * period[0], rtol=1e-6)
    segs, soff = S.segments(r, lo, period)[:2]
    ref, mag = fp64_columns(gh, cuda, segs, soff, scene.spheres.cpu().numpy())
    check_columns(image.cpu().numpy(), ref, mag, "fast", 1.91 / float(s[:, 3].min()) ** 2)
    # more than the open projection of the same frame: the images' mass
    tree = gh.Tree(len(s), 32, device=cuda)
    d = _dev(s, cuda)
    gh.build_tree(d, tree)
    open_image = open_trace(gh, rays, d, tree)
    assert image.sum().item() > 1.05 * open_image.sum()
    with pytest.raises(ValueError):
        gh.project_sph(_dev(s, cuda), 32, period=(1.0, 1.5, 1.0))


# ---- the C++ front ends ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mirror", [False, True])
def test_dropin_prints_the_digests_of_the_python_path(gh, cuda, scenes, tmp_path, mirror):
    box, n_ch = "slab", 3
    lo, period = S.BOXES[box]
    scene, d, rays = scenes[box]
    rays = rays[:1001].contiguous()
    w = (0.5 + np.random.default_rng(13).random((len(d), n_ch))).astype(F32)
    for name, a in (("s", S.spheres(box)), ("r", rays.cpu().numpy()), ("w", w)):
        np.ascontiguousarray(a).tofile(str(tmp_path / (name + ".f32")))
    exe = str(tmp_path / "dropin_periodic_trace")
    compile_dropin(exe, mirror)
    f = lambda x: str(tmp_path / (x + ".f32"))
    res = subprocess.run([exe, f("s"), f("r"), f("w"), str(n_ch), *(repr(float(v)) for v in lo),
                          *(repr(float(v)) for v in period)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    exp = {"images": scene.spheres.cpu().numpy(), "source": scene.source.cpu().numpy(),
           "counts": gh.trace_hitcounts_periodic_sph(rays, scene, check=True).cpu().numpy(),
           "cumulated": gh.trace_cumulative_periodic_sph(rays, scene, check=True).cpu().numpy(),
           "weighted": gh.trace_cumulative_weighted_periodic_sph(rays, scene, _dev(w, cuda), check=True).cpu().numpy()}
    got = {t[0]: (int(t[1]), int(t[2])) for t in (ln.split() for ln in res.stdout.splitlines())
           if len(t) == 3 and t[0] in exp}
    assert set(got) == set(exp)
    for name, a in exp.items():
        assert got[name] == digest(a), name
