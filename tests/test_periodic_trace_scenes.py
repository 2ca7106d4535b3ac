"""CPU checks of tests/periodic_trace_scenes.py: the restatement of the periodic traces' definition
(include/grace_hip.h, "Periodic boxes for traces") against an fp64 brute force over the infinite
lattice, the geometry of the segments, what the scenes contain, and that both C++ front ends compile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import periodic_trace_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
SYMBOLS = ("grace_periodic_image_counts_f4", "grace_periodic_images_f4", "grace_periodic_segment_counts",
           "grace_periodic_segments", "grace_periodic_fold_f32", "grace_periodic_fold_i32",
           "grace_periodic_gather_rows_f32")
F32, F64 = np.float32, np.float64
BOXES = sorted(S.BOXES)


def cpu_rays(box, lattice=False):
    """Every kind of ray of the box, the 64 x 64 grid thinned to 256 (the brute force is quadratic).
    lattice=True: without the rays through a box corner.  They run through the centre of every replica of
    the scene's corner spheres, so those spheres' closest approach falls exactly on a tied cut, where the
    fp32 rounding of dot against the segment's length decides (measured on the first version of this
    scene: 4 rays off by 16 hits, two corners of 8 spheres).  The scene was changed as the condition
    asks: the "edge" rays carry the tied cuts into the comparison with the brute force instead."""
    r = S.rays(box)
    skip = ("grid", "corner") if lattice else ("grid",)
    return np.concatenate([r["grid"][::16]] + [v for k, v in r.items() if k not in skip])


def test_periodic_trace_symbols_exported_and_declared():
    lib = C.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    header = open(os.path.join(ROOT, "include", "grace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"grace_status %s\(" % name, header), name
    assert "/* ---- Periodic boxes for traces" in header


@pytest.mark.parametrize("box", BOXES)
def test_restatement_counts_every_lattice_image_once(box):
    """Stated images x stated segments under hit_f32 against the fp64 brute force over the lattice
    (unsegmented rays, every replica in reach).  A condition on the scenes: at least 99 % of the rays
    agree and none differs by more than one hit (fp32 against fp64 at a grazing hit)."""
    lo, period = S.BOXES[box]
    rays = cpu_rays(box, lattice=True)
    got = S.hitcounts(rays, S.spheres(box), lo, period)
    ref = S.lattice_hitcounts(rays, S.spheres(box), lo, period)
    diff = np.abs(got.astype(np.int64) - ref)
    print(box, "hits", int(ref.sum()), "differing rays", int(np.count_nonzero(diff)), "of", len(rays))
    assert ref.sum() > 5000
    assert np.count_nonzero(diff) <= 0.01 * len(rays), np.nonzero(diff)[0][:10]
    assert diff.max() <= 1, (np.argmax(diff), diff.max())


@pytest.mark.parametrize("box", BOXES)
def test_segments_tile_their_ray(box):
    lo, period = S.BOXES[box]
    rays = cpu_rays(box)
    segs, offsets, refused, cells, t0 = S.segments(rays, lo, period)
    assert not refused.any() and offsets[-1] == len(segs)
    n = np.diff(offsets)
    row = np.repeat(np.arange(len(rays)), n)
    # lengths sum to the ray's within 4 * 2^-24 * l per segment
    total = np.zeros(len(rays), F64)
    np.add.at(total, row, segs[:, 6].astype(F64))
    ell = rays[:, 6].astype(F64)
    assert np.all(np.abs(total - ell) <= 4 * 2.0 ** -24 * ell * n), np.max(np.abs(total - ell) / np.maximum(ell, 1e-30))
    # direction bit for bit; the midpoint, moved back by its cell, lies on the original ray
    assert np.array_equal(segs[:, :3].view(np.uint32), rays[row, :3].view(np.uint32))
    d = rays[row, :3].astype(F64); o = rays[row, 3:6].astype(F64)
    half = 0.5 * segs[:, 6:7].astype(F64)
    mid = segs[:, 3:6].astype(F64) + half * d + cells * period.astype(F64)
    want = o + (t0[:, None] + half) * d
    scale = np.abs(lo).max() + 8 * period.max()
    assert np.max(np.abs(mid - want)) <= 4 * 2.0 ** -24 * scale, np.max(np.abs(mid - want))
    # every segment starts in the box (a rounding step of slack), whatever cell the ray was in
    for k in range(3):
        if period[k] > 0:
            eps = 4 * 2.0 ** -24 * scale
            long_enough = segs[:, 6] > 0
            assert np.all(segs[long_enough, 3 + k] >= lo[k] - eps) and np.all(segs[long_enough, 3 + k] <= lo[k] + period[k] + eps)
    # a ray that never leaves cell 0 is its own segment, bit for bit
    own = np.nonzero((n == 1) & np.all(cells[offsets[:-1]] == 0, axis=1))[0]
    assert len(own) > 50
    assert np.array_equal(segs[offsets[own]].view(np.uint32), rays[own].view(np.uint32))


@pytest.mark.parametrize("box", BOXES)
def test_scenes_hold_what_they_promise(box):
    lo, period = S.BOXES[box]
    s = S.spheres(box)
    per = [k for k in range(3) if period[k] > 0]
    lmin = min(period[k] for k in per)
    assert 400 <= len(s) <= 2000 and s[:, 3].max() == F32(0.5) * lmin
    imgs, source, offsets, refused = S.images(s, lo, period)
    assert not refused.any()
    n_img = np.diff(offsets)
    assert set(n_img) == ({1, 2, 4, 8} if len(per) == 3 else {1, 2, 4})     # faces, edges, corners cross
    top = (lo + period).astype(F32)
    on_face = sum(((s[:, k] == lo[k]) | (s[:, k] == top[k])).astype(int) for k in per)
    assert np.count_nonzero(on_face == 1) >= 8 and np.count_nonzero(on_face == 2) >= 8
    assert len(per) < 3 or np.count_nonzero(on_face == 3) >= 8
    assert np.array_equal(imgs[offsets[:-1]].view(np.uint32), s.view(np.uint32))   # subset 0 is the sphere itself
    assert np.array_equal(source, np.repeat(np.arange(len(s)), n_img))
    r = S.rays(box)
    assert len(r["grid"]) == 64 * 64 and np.all(r["grid"][:, 6] == period[2])
    assert np.any(np.signbit(r["plane"][:, :3]) & (r["plane"][:, :3] == 0))         # a -0 component
    assert np.all(r["zero_length"][:, 6] == 0)
    segs, offsets = S.segments(r["corner"], lo, period)[:2]
    assert np.any(segs[:, 6] == 0) and np.all(np.diff(offsets) >= 1 + len(per))     # tied cuts: a zero-length segment
    segs, offsets = S.segments(r["oblique"], lo, period)[:2]
    assert np.diff(offsets).max() >= 5
    # open axes: images == spheres, segments == rays
    imgs, source, _, _ = S.images(s, lo, np.zeros(3, F32))
    assert np.array_equal(imgs.view(np.uint32), s.view(np.uint32)) and np.array_equal(source, np.arange(len(s)))
    allr = S.all_rays(box)
    segs = S.segments(allr, lo, np.zeros(3, F32))[0]
    assert np.array_equal(segs.view(np.uint32), allr.view(np.uint32))


def test_refusals_are_what_the_definition_says():
    for box in BOXES:
        lo, period = S.BOXES[box]
        s, r = S.refusals(box)
        imgs, source, offsets, refused = S.images(s, lo, period)
        assert list(np.nonzero(refused)[0]) == [2, 5]
        for i in (2, 5):
            assert offsets[i + 1] - offsets[i] == 1
            assert np.array_equal(imgs[offsets[i]].view(np.uint32), s[i].view(np.uint32))
        segs, offsets, refused = S.segments(r, lo, period)[:3]
        assert list(np.nonzero(refused)[0]) == [3] and offsets[4] - offsets[3] == 1
        assert np.array_equal(segs[offsets[3]].view(np.uint32), r[3].view(np.uint32))
    # 65 536 segments are legal, one more is not
    lo, period = S.BOXES["cube"]
    ray = np.array([[1, 0, 0, 0.5, 0.5, 0.5, 65535.25], [1, 0, 0, 0.5, 0.5, 0.5, 65536.75]], F32)
    segs, offsets, refused = S.segments(ray, lo, period)[:3]
    assert list(refused) == [False, True] and list(np.diff(offsets)) == [65536, 1]


def test_dyadic_scene_is_translation_invariant_in_the_restatement():
    lo, period = S.BOXES["slab"]
    s, r = S.dyadic("slab", n=200, n_rays=96)
    ref = S.hitcounts(r, s, lo, period)
    assert ref.sum() > 200
    s2, r2 = S.dyadic_shift(s, r, lo, period, np.array([301, -77, 1030]) / 1024.0)
    assert np.array_equal(S.hitcounts(r2, s2, lo, period), ref)


def compile_dropin(exe, mirror=False):
    flags = ["-DDROPIN_MIRROR"] if mirror else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, *flags,
                           os.path.join(ROOT, "tests", "cpp", "dropin_periodic_trace.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


@pytest.mark.parametrize("mirror", [False, True])
def test_periodic_trace_dropin_compiles_with_hipcc(tmp_path, mirror):
    """tests/cpp/dropin_periodic_trace.hip against the drop-in header set and against the HIP-free mirror
    (one shared body: include/grace/detail/periodic_trace.h)."""
    exe = tmp_path / "dropin_periodic_trace"
    compile_dropin(exe, mirror)
    assert exe.exists()
