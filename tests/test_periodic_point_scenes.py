"""CPU checks for the periodic nearest neighbours, smoothing lengths and interpolation: the exported and
declared symbols, the drop-in program against both header sets, and the restatement of
periodic_point_scenes.py itself against a second method -- the fp64 minimum over the 27 explicit images
on lattices whose fp32 arithmetic is exact -- with the counts a torus must give on the scenes the GPU
tests of test_periodic_points.py use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import periodic_point_scenes as PS
import periodic_query_scenes as S
from test_neighbours import brute_knn
from test_range_queries import HIPCC_FLAGS, LIBDIR, ROOT
from test_sph_interpolation import pairs as open_pairs

F32 = np.float32
CUBE = S.BOXES["cube"]
OPEN = (0.0, 0.0, 0.0)
SYMBOLS = ("grace_nearest_neighbours_periodic_f4", "grace_smoothing_lengths_periodic_f4",
           "grace_interpolate_points_periodic_f4", "grace_interpolate_grid_periodic_f4")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_periodic_point_symbols_exported_and_declared():
    lib = C.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    header = open(os.path.join(ROOT, "include", "grace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"grace_status %s\(" % name, header), name
    block = header[header.index("/* ---- Periodic boxes"):]
    not_provided = block[block.index("Not provided:"):block.index("*/", block.index("Not provided:"))]
    assert "interpolat" not in not_provided and "neighbours" not in not_provided


def compile_dropin(exe, mirror=False):
    flags = ["-DDROPIN_MIRROR"] if mirror else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, *flags,
                           os.path.join(ROOT, "tests", "cpp", "dropin_periodic_points.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


@pytest.mark.parametrize("mirror", [False, True])
def test_periodic_points_dropin_compiles_with_hipcc(tmp_path, mirror):
    exe = tmp_path / "dropin_periodic_points"
    compile_dropin(exe, mirror)
    assert exe.exists()


def test_periodic_points_mirror_compiles_with_gcc(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& p, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::device_vector<float>& w, const grace::Tree& t)\n"
                   "{\n"
                   "    const grace::PeriodicBox box = { 1.0f, 0.5f, 0.0f };\n"
                   "    grace::device_vector<int> idx(p.size() * 8), counts(p.size());\n"
                   "    grace::device_vector<float> d2(p.size() * 8), h(s.size()), out(p.size() * 2), g(8 * 8 * 8 * 2);\n"
                   "    grace::nearest_neighbours_sph(p, s, t, 8, idx, d2, box);\n"
                   "    grace::smoothing_lengths_sph(s, t, 8, 1.2f, h, box);\n"
                   "    grace::interpolate_sph(p, s, t, w, 2, out, box);\n"
                   "    grace::interpolate_sph(p, s, t, w, 2, out, counts, box);\n"
                   "    const grace::float3 o = grace::make_float3(0, 0, 0), u = grace::make_float3(1, 0, 0),\n"
                   "                        v = grace::make_float3(0, 1, 0), z = grace::make_float3(0, 0, 1);\n"
                   "    grace::interpolate_grid_sph(o, u, v, z, 8, 8, 8, s, t, w, 2, g, box);\n"
                   "    const grace::int3 dims = { 8, 8, 8 };\n"
                   "    grace::interpolate_grid_sph(o, u, v, z, dims, s, t, w, 2, g, box);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


# ---- the restatement against explicit images ------------------------------------------------------------
@pytest.mark.parametrize("offset", S.OFFSETS)
def test_restated_lattice_against_explicit_images(offset):
    """The full 16^3 lattice: every coordinate, difference, wrap and square is exact in fp32, so the wrapped
    d2 is the fp64 minimum over the 27 images bit for bit; every site is every other's translate."""
    s = PS.lattice_H(offset)
    x = s[:, :3]
    rows = np.arange(0, len(s), 8)
    d2 = S.d2_rows(x[rows], x, CUBE)
    assert np.array_equal(d2.astype(np.float64), PS.image_min_d2(x[rows], x, CUBE))
    # neighbours: itself at 0, six at 1/256, the 8th at 2/256
    idx, dd = PS.knn(x, s, 8, CUBE)
    assert np.all(dd[:, 0] == 0) and np.all(idx[:, 0] == np.arange(len(s)))
    assert np.all(dd[:, 1:7] == F32(1.0 / 256.0)) and np.all(dd[:, 7] == F32(2.0 / 256.0))
    assert np.all(np.diff(idx[:, 1:7], axis=1) > 0)                  # ties in ascending index
    open_dd = brute_knn(x, s, 8)[1]
    assert np.all(open_dd >= dd) and np.any(open_dd[:, 6] > F32(1.0 / 256.0))   # the open faces miss theirs
    eta = 1.2
    h = PS.lengths(s, 7, eta, CUBE)
    assert np.all(h == F32(eta) * F32(1.0 / 16.0))
    assert PS.lengths(s, 7, eta, OPEN).max() > h[0]
    # interpolation: with H = 1.5/16 every site lies in 19 spheres (itself, 6 at 1/16, 12 at sqrt(2)/16)
    counts = PS.counts(x, s, CUBE)
    assert np.all(counts == 19)
    open_counts = PS.counts(x, s, OPEN)
    assert open_counts.min() == 7 and open_counts.max() == 19
    assert np.array_equal(open_counts, np.bincount(open_pairs(x, s)[0], minlength=len(s)))


def test_restated_one_sphere_is_translation_invariant():
    """One sphere of H = 0.25 on the 32^3 lattice of spacing 1/32: centred on the box corner or at the box
    centre, the multisets of wrapped d2 are identical, 2103 points inside; the open corner holds 341."""
    inside = []
    for centre in (0.0, 0.5):
        pts, sph = PS.one_sphere_grid(centre)
        d2 = S.d2_rows(pts, sph[:, :3], CUBE)[:, 0]
        assert np.array_equal(d2.astype(np.float64), PS.image_min_d2(pts, sph[:, :3], CUBE)[:, 0])
        inside.append(np.sort(d2))
        pi, si, dd = PS.pairs(pts, sph, CUBE)
        assert len(pi) == 2103 and _same(np.sort(dd), np.sort(d2[d2 < F32(0.0625)]))
    assert _same(inside[0], inside[1])
    pts, sph = PS.one_sphere_grid(0.0)
    assert len(open_pairs(pts, sph)[0]) == 341
    assert len(PS.pairs(pts, sph, OPEN)[0]) == 341


@pytest.mark.parametrize("period", [OPEN, (8.0, 300.0, 2.5)])
def test_restatement_without_wraps_is_the_open_restatements(period):
    s = PS.interp_scene("cube", 0.0, 5, 1500)
    pts, _ = S.uniform_queries(s, "cube", 0.0, 5, 400)
    pts[:3] = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [3.0, -2.0, 0.5]], F32)
    for k in (1, 9, 33):
        a, b = PS.knn(pts, s, k, period), brute_knn(pts, s, k)
        assert np.array_equal(a[0], b[0]) and _same(a[1], b[1])
    a, b = PS.pairs(pts, s, period), open_pairs(pts, s)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and _same(a[2], b[2])


@pytest.mark.parametrize("box", list(S.BOXES))
def test_special_H_switch_spheres_off_above_half_a_period(box):
    period = S.BOXES[box]
    s = PS.interp_scene(box, 0.0, 9, 500)
    lmin = min(L for L in period if L > 0)
    sp = PS.special_H(box)
    on = PS.sphere_on(s, period)
    assert np.array_equal(on[:len(sp)], sp <= S.half(lmin)) and np.all(on[len(sp):])
    pi, si, _ = PS.pairs(s[:, :3], s, period)                       # at the centres themselves
    hit = np.bincount(si, minlength=len(s))
    assert np.all(hit[:len(sp)][~on[:len(sp)]] == 0) and hit[len(sp) - 1] == 0       # off, and H = 0
    assert np.all(hit[:len(sp) - 1][on[:len(sp) - 1]] > 50)         # half the smallest period: on, and large
    # the seam is in the scene: the same spheres hold more points on the torus
    assert len(pi) > len(PS.pairs(s[:, :3], s[on], OPEN)[0]) + 200
