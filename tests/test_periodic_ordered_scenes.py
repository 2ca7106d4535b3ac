"""CPU checks of tests/periodic_ordered_scenes.py: the restated hit list of the periodic ordered traces
(include/grace_hip.h, "Periodic boxes for traces", "Ordered traces") against an fp64 brute force over
the infinite lattice -- unsegmented rays, every replica in reach, hits ordered by absolute distance --,
what the scenes contain, that the entry points are exported and declared, and that the C++ front end's
program compiles against both header sets.

A ray is left out of the comparison with the lattice only if some (ray, replica) pair of it lies within
rounding of an edge of the hit test: b against H, or the distance along the ray against 0, the ray's
length or a cut between two segments (where a segment's own test compares its dot with 0 and with its
length).  "Within rounding" is EDGE = 8 * 2^-24 of the scene's scale |lo| + 8 L: test_periodic_trace_scenes.py
bounds the fp32 positions along a segment by 4 * 2^-24 of that scale, and the hit test's own products and
sums add as much again.  At most 5 % of a scene's rays may be left out."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import periodic_ordered_scenes as S
import periodic_trace_scenes as P
import test_emission_absorption as EA
from test_periodic_trace_scenes import HIPCC_FLAGS, LIBDIR, ROOT

F32, F64 = np.float32, np.float64
BOXES = sorted(P.BOXES)
SYMBOLS = ("grace_periodic_segment_starts", "grace_trace_emission_absorption_periodic_f4",
           "grace_trace_absorption_deposit_periodic_f4", "grace_trace_spectra_periodic_f4")
EDGE = 8 * 2.0 ** -24
MAX_LEFT_OUT = 0.05


def compile_dropin(exe, mirror=False, source="dropin_periodic_ordered.hip"):
    """As test_periodic_trace_scenes.compile_dropin (same flags), for this feature's program."""
    flags = ["-DDROPIN_MIRROR"] if mirror else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, *flags, os.path.join(ROOT, "tests", "cpp", source),
                           "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


def test_periodic_ordered_symbols_exported_and_declared():
    lib = C.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    header = open(os.path.join(ROOT, "include", "grace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"grace_status %s\(" % name, header), name


@pytest.mark.parametrize("mirror", [False, True])
def test_periodic_ordered_dropin_compiles_with_hipcc(tmp_path, mirror):
    exe = tmp_path / "dropin_periodic_ordered"
    compile_dropin(exe, mirror)
    assert exe.exists()


def _scene(oracle, name):
    if name == "tiers":
        sph, rays, _ = S.tiers(oracle)
        lo, period = P.BOXES["cube"]
    else:
        sph, rays = S.seam(name)
        lo, period = P.BOXES[name]
    images, source = P.images(sph, lo, period)[:2]
    return sph, rays, lo, period, images, source, S.hit_list(oracle, rays, images, source, lo, period)


def test_scenes_hold_what_they_promise(oracle):
    for box in BOXES:
        sph, rays, lo, period, images, source, H = _scene(oracle, box)
        per = [k for k in range(3) if period[k] > 0]
        assert len(rays) == 257 and len(sph) <= 4000
        n_seg = np.diff(H.seg_off)
        assert n_seg.max() >= 4 and not H.refused.any()
        # the first rays run 2.25 periods along an axis from a face: whatever they hit in their first
        # period they hit again one and two periods on, as another replica
        m = S.replicas(H, sph, images, source, period)
        for r in range(3 * len(per)):
            sl = slice(H.off[r], H.off[r + 1])
            k = per[r % len(per)]
            src, mk = H.source[sl], m[sl, k]
            assert n_seg[r] == 3 and len(src) > 0
            first = set(src[mk == mk.min()])
            assert first and all(np.count_nonzero(src == i) >= 2 for i in first)
        # oblique rays through the corner region meet particles that have 2^len(per) images
        n_img = np.bincount(source, minlength=len(sph))
        corner = slice(H.off[3 * len(per)], H.off[3 * len(per) + 4])
        assert np.any(n_img[H.source[corner]] == 2 ** len(per))
    sph, rays, targets = S.tiers(oracle)
    _, _, lo, period, images, source, H = _scene(oracle, "tiers")
    assert 2500 <= len(sph) <= 4000 and len(rays) <= 257
    assert list(H.totals()[:6]) == targets == [511, 512, 513, 6143, 6144, 6145]
    for r in range(6):
        per_seg = H.seg_hits[H.seg_off[r]:H.seg_off[r + 1]]
        assert len(per_seg) >= 3 and 0 in per_seg and 1 in per_seg
    assert 200 <= H.seg_hits.max() <= 1000               # one axis crossing: a few hundred hits


def _left_out(rays, lo, period, lat, seg_off, seg_t0):
    """Rays with a pair within rounding of an edge of the hit test (the module's docstring)."""
    ray, _, _, dot, b2, h, _ = lat
    scale = float(np.abs(lo).max() + 8 * period.max())
    tol = EDGE * scale
    near = np.abs(np.sqrt(b2) - h) <= tol
    inside = np.sqrt(b2) < h + tol
    ell = rays[ray, 6].astype(F64)
    for r in np.unique(ray):
        cuts = np.concatenate([seg_t0[seg_off[r]:seg_off[r + 1]], [float(rays[r, 6])]])
        mine = np.nonzero(ray == r)[0]
        gap = np.min(np.abs(dot[mine, None] - cuts[None, :]), axis=1)
        near[mine] |= inside[mine] & (gap <= tol)
    near &= (dot > -tol) & (dot < ell + tol)
    out = np.zeros(len(rays), bool)
    out[ray[near]] = True
    return out


@pytest.mark.parametrize("name", BOXES + ["tiers"])
def test_restated_hit_list_is_the_lattice_ordered_by_distance(oracle, name):
    sph, rays, lo, period, images, source, H = _scene(oracle, name)
    lat = S.lattice_hits(rays, sph, lo, period)
    l_ray, l_src, l_m, l_dot, _, _, l_hit = lat
    skip = _left_out(rays, lo, period, lat, H.seg_off, H.seg_t0)
    print(name, "rays left out:", int(skip.sum()), "of", len(rays), "hits", len(H.source))
    assert skip.sum() <= MAX_LEFT_OUT * len(rays), np.nonzero(skip)[0]
    m = S.replicas(H, sph, images, source, period)
    rng = np.random.default_rng(1)
    emission = rng.random((len(sph), 2)).astype(F32)
    absorption = (5e-3 * sph[:, 3].astype(F64) ** 2 * (0.2 + 1.6 * rng.random(len(sph)))).astype(F32)
    checked = 0
    for r in np.nonzero(~skip)[0]:
        sl = slice(H.off[r], H.off[r + 1])
        mine = np.nonzero((l_ray == r) & l_hit)[0]
        got = np.column_stack([H.source[sl].astype(np.int64), m[sl]])
        want = np.column_stack([l_src[mine], l_m[mine]])
        # the multiset of (source, replica)
        assert len(got) == len(want), (r, len(got), len(want))
        go, wo = np.lexsort(got.T[::-1]), np.lexsort(want.T[::-1])
        assert np.array_equal(got[go], want[wo]), r
        assert len(np.unique(got, axis=0)) == len(got), r
        checked += 1
        if len(got) == 0:
            continue
        # the order, wherever neighbouring absolute distances differ by more than 2^-20 of the length
        dist = np.empty(len(got), F64)
        dist[go] = l_dot[mine][wo]                      # the lattice's distance of every restated hit, in list order
        back = np.diff(dist) < -2.0 ** -20 * float(rays[r, 6])
        assert not back.any(), (r, np.nonzero(back)[0][:5])
        # emission-absorption from the lattice's order against the restated one
        by_dist = np.argsort(dist, kind="stable")
        one = S.sub_list(H, [r])
        ref = S.emission_absorption(one, 1, emission, absorption)
        lat_order = S.Hits()
        lat_order.off, lat_order.source, lat_order.integral = one.off, one.source[by_dist], one.integral[by_dist]
        out, tau, _, _ = S.emission_absorption(lat_order, 1, emission, absorption)
        tol = EA.bound(ref[0], ref[2], ref[3], ref[1])
        assert np.all(np.abs(out - ref[0]) <= tol), (r, out, ref[0], tol)
    assert checked >= (1.0 - MAX_LEFT_OUT) * len(rays) - 1
