"""Mixed-precision SPH traces: float4 spheres with double column densities and per-hit outputs
(trace_cumulative_sph<float4, double>, trace_sph / trace_with_sentinels_sph<float4, int, double>).

Expected values come from a NumPy restatement of the reference's promotions for that pair
(generic/intersect.h:9-55, functors/trace.cuh:164-235, generic/interpolate.h:11-39): the hit test
subtracts in float and widens, the radius test compares against the float product w * w; the lerp's
fma is evaluated exactly (fractions.Fraction) and rounded once to double."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]

F32, F64 = np.float32, np.float64
TABLE = np.array([
    1.90986019771937, 1.90563449910964, 1.89304415940934, 1.87230928086763,
    1.84374947679902, 1.80776276033034, 1.76481079856299, 1.71540816859939,
    1.66011373131439, 1.59952322363667, 1.53426266082279, 1.46498233888091,
    1.39235130929287, 1.31705223652377, 1.23977618317103, 1.16121278415369,
    1.08201943664419, 1.00288866679720, 0.924475767210246, 0.847415371038733,
    0.772316688105931, 0.699736940377312, 0.630211918937167, 0.564194562399538,
    0.502076205853037, 0.444144023534733, 0.390518196140658, 0.341148855945766,
    0.295941946237307, 0.254782896476983, 0.217538645099225, 0.184059547649710,
    0.154181189781890, 0.127726122453554, 0.104505535066266,
    8.432088120445191E-002, 6.696547102921641E-002, 5.222604427168923E-002,
    3.988433820097490E-002, 2.971866601747601E-002, 2.150552303075515E-002,
    1.502124104014533E-002, 1.004371608622562E-002, 6.354242122978656E-003,
    3.739494884706115E-003, 1.993729589156428E-003, 9.212900163813992E-004,
    3.395908945333921E-004, 8.287326418242995E-005, 7.387919939044624E-006,
    0.000000000000000E+000], F64)


# ---- the restatement ----------------------------------------------------------------------------
def mixed_test(rays, s):
    """sphere_hit<float4, double> for every (ray, sphere): (hit, b2, dot) as [n_rays, n] arrays."""
    d = rays[:, 0:3].astype(F64)
    o = rays[:, 3:6]
    ln = rays[:, 6].astype(F64)[:, None]
    p = [(s[None, :, k] - o[:, k:k + 1]).astype(F64) for k in range(3)]      # float subtraction
    r = [d[:, k:k + 1] for k in range(3)]
    dot = p[0] * r[0] + p[1] * r[1] + p[2] * r[2]
    b = [p[k] - dot * r[k] for k in range(3)]
    b2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2]
    w2 = (s[:, 3] * s[:, 3]).astype(F64)[None, :]                              # float product
    hit = ~(b2 >= w2) & ~(dot < 0.0) & ~(dot >= ln)
    return hit, b2, dot


def float_test_counts(rays, s):
    """sphere_hit<float4, float> (the float path's test) counts, for the disagreement check."""
    d, o, ln = rays[:, 0:3], rays[:, 3:6], rays[:, 6][:, None]
    p = [s[None, :, k] - o[:, k:k + 1] for k in range(3)]
    r = [d[:, k:k + 1] for k in range(3)]
    dot = p[0] * r[0] + p[1] * r[1] + p[2] * r[2]
    b = [p[k] - dot * r[k] for k in range(3)]
    b2 = b[0] * b[0] + b[1] * b[1] + b[2] * b[2]
    hit = ~(b2 >= (s[:, 3] * s[:, 3])[None, :]) & ~(dot < 0) & ~(dot >= ln)
    return hit.sum(axis=1).astype(np.int32)


def _fma(t, dy, y0):
    """fma in double, exactly: one rounding of t * dy + y0."""
    return float(Fraction(float(t)) * Fraction(float(dy)) + Fraction(float(y0)))


def term_cumulative(b2, w):
    """OnHit_sphere_cumulate with Real4 = float4: the float term added to the double sum."""
    ir = F32(1) / F32(w)
    b = F32(50 * (math.sqrt(float(b2)) * float(ir)))
    x_idx = int(b)
    t = float(b) - x_idx
    if x_idx >= 50:
        t, x_idx = 1.0, 49
    y = F32(_fma(t, TABLE[x_idx + 1] - TABLE[x_idx], TABLE[x_idx]))
    return F32(y * F32(ir * ir))


def term_individual(b2, w):
    """OnHit_sphere_individual<int, double>: ir = 1.f / w in float, the rest in double."""
    ir = float(F32(1) / F32(w))
    x = 50 * (math.sqrt(float(b2)) * ir)
    x_idx = int(x)
    if x_idx >= 50:
        x, x_idx = 50.0, 49
    y = _fma(x - x_idx, TABLE[x_idx + 1] - TABLE[x_idx], TABLE[x_idx])
    return y * (ir * ir)


def restate(rays, s, chunk=512):
    """Per ray: ascending hit indices, their double per-hit terms and distances, and the float
    column-density terms.  Returns (counts, [(idx, w64, dist, w32)] per ray)."""
    counts, per_ray = [], []
    for r0 in range(0, len(rays), chunk):
        hit, b2, dot = mixed_test(rays[r0:r0 + chunk], s)
        for i in range(hit.shape[0]):
            idx = np.nonzero(hit[i])[0]
            counts.append(len(idx))
            w64 = np.array([term_individual(b2[i, j], s[j, 3]) for j in idx], F64)
            w32 = np.array([term_cumulative(b2[i, j], s[j, 3]) for j in idx], F32)
            per_ray.append((idx.astype(np.int32), w64, dot[i, idx], w32))
    return np.array(counts, np.int32), per_ray


def class_sum(idx, w32):
    """The class-ordered double sum: class (p >> 10) & 7, ascending within a class, pairwise."""
    cls = [0.0] * 8
    for p, w in zip(idx, w32):
        cls[(int(p) >> 10) & 7] += float(w)
    t = list(cls)
    step = 1
    while step < 8:
        for c in range(0, 8, 2 * step):
            t[c] = t[c] + t[c + step]
        step *= 2
    return t[0]


# ---- CPU: the new forms compile and the library exports them -------------------------------------
def test_mixed_precision_symbols_exported():
    import ctypes
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    for name in ("grace_trace_hitcounts_f4_f64", "grace_trace_cumulative_f4_f64", "grace_trace_hits_f4_f64"):
        assert hasattr(lib, name), name


def test_mixed_precision_dropin_compiles_with_hipcc(tmp_path):
    """trace_cumulative_sph<float4, double>, trace_sph<float4, int, double>,
    trace_with_sentinels_sph<float4, int, double>, sort_by_distance and exclusive_segmented_scan
    <double> through the reference's include paths (run on the GPU below)."""
    exe = tmp_path / "dropin_mixed_precision"
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_mixed_precision.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


def test_double4_with_float_outputs_is_a_clear_compile_error(tmp_path):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/trace_sph.cuh"\n'
                   "void f(const thrust::device_vector<grace::Ray>& r, const thrust::device_vector<double4>& s,\n"
                   "       const grace::Tree& t, thrust::device_vector<float>& out)\n"
                   "{ grace::trace_cumulative_sph(r, s, t, out); }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "double4 spheres with float outputs are not supported" in res.stderr


def test_mixed_precision_mirror_compiles_with_gxx(tmp_path):
    """The HIP-free mirror (include/grace/grace.h) has the same three forms over
    grace::device_vector<double>, plus the double sort_by_distance of the chain."""
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::Ray>& r, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::Tree& t)\n"
                   "{\n"
                   "    grace::device_vector<double> cum(r.size()), w, d, scanned;\n"
                   "    grace::device_vector<int> off(r.size()), idx;\n"
                   "    grace::trace_cumulative_sph(r, s, t, cum);\n"
                   "    grace::trace_sph(r, s, t, off, idx, w, d);\n"
                   "    grace::sort_by_distance(d, off, idx, w);\n"
                   "    scanned.resize(w.size());\n"
                   "    grace::exclusive_segmented_scan(off, w, scanned);\n"
                   "    grace::trace_with_sentinels_sph(r, s, t, off, idx, -1, w, -2.0, d, -3.0);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


# ---- GPU --------------------------------------------------------------------------------------------
def _scene(gh, cuda, n, seed, hlo=0.01, hhi=0.05):
    import torch
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = (hlo + (hhi - hlo) * rng.random(n)).astype(F32)
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(n, 32, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))     # sorts d
    return d, tree


def _ray_sets(gh, cuda):
    return {
        "orthographic": gh.orthogonal_rays_z(48, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0],
        "pinhole": gh.pinhole_camera_rays(48, 48, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0,
                                          device=cuda),
        "isotropic": gh.uniform_random_rays(2048, (0.5, 0.5, 0.5), 1.0, device=cuda),
    }


@pytest.mark.gpu
def test_mixed_hitcounts_equal_the_fp64_test(gh, cuda):
    import torch
    d, tree = _scene(gh, cuda, 20000, 11)
    s = d.cpu().numpy()
    for name, rays in _ray_sets(gh, cuda).items():
        got = torch.empty(len(rays), dtype=torch.int32, device=cuda)
        gh.trace_hitcounts_f4_f64(rays, d, tree, got, check=True)
        rr = rays.cpu().numpy()
        ref = np.concatenate([mixed_test(rr[i:i + 512], s)[0].sum(axis=1) for i in range(0, len(rr), 512)])
        assert np.array_equal(got.cpu().numpy(), ref.astype(np.int32)), name
        assert ref.sum() > 0, name


def _near_tangent_scene(gh, cuda, side=32, per_ray=2, seed=5):
    """Orthographic rays along +z over a side x side grid; for each ray, spheres whose double b2
    lies just below fl32(w w) while the float b2 is rounded up to or past it."""
    import torch
    rays = gh.orthogonal_rays_z(side, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    rr = rays.cpu().numpy()
    rng = np.random.default_rng(seed)
    out = []
    while sum(len(x) for x in out) < side * side * per_ray:
        k = 4 * side * side
        ri = rng.integers(0, len(rr), k)
        ox, oy = rr[ri, 3], rr[ri, 4]
        w0 = (0.004 + 0.01 * rng.random(k)).astype(F32)
        th = rng.random(k) * 2 * np.pi
        sx = (ox + w0 * np.cos(th)).astype(F32)
        sy = (oy + w0 * np.sin(th)).astype(F32)
        q1, q2 = (sx - ox).astype(F32), (sy - oy).astype(F32)
        b2d = q1.astype(F64) ** 2 + q2.astype(F64) ** 2
        b2f = (q1 * q1 + q2 * q2).astype(F32)
        w = np.sqrt(b2d).astype(F32)
        chosen = np.full(k, np.nan, F32)
        for step in range(-3, 4):
            c = (w.view(np.int32) + step).view(F32)
            w2 = (c * c).astype(F32)
            ok = (b2d < w2.astype(F64)) & ~(b2f.astype(F32) < w2) & np.isnan(chosen)
            chosen[ok] = c[ok]
        good = ~np.isnan(chosen)
        sz = (0.2 + 0.6 * rng.random(k)).astype(F32)
        out.append(np.stack([sx, sy, sz, chosen], axis=1)[good].astype(F32))
    s = np.concatenate(out)[: side * side * per_ray]
    d = torch.from_numpy(np.ascontiguousarray(s)).to(cuda)
    tree = gh.Tree(len(s), 16, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    return rays, d, tree


@pytest.mark.gpu
def test_near_tangent_scene_separates_the_two_tests(gh, cuda):
    import torch
    rays, d, tree = _near_tangent_scene(gh, cuda)
    s, rr = d.cpu().numpy(), rays.cpu().numpy()
    mixed = torch.empty(len(rays), dtype=torch.int32, device=cuda)
    flt = torch.empty(len(rays), dtype=torch.int32, device=cuda)
    gh.trace_hitcounts_f4_f64(rays, d, tree, mixed, check=True)
    gh.trace_hitcounts_sph(rays, d, tree, flt, check=True)
    ref = np.concatenate([mixed_test(rr[i:i + 512], s)[0].sum(axis=1) for i in range(0, len(rr), 512)])
    got = mixed.cpu().numpy()
    assert np.array_equal(got, ref.astype(np.int32)), "culling dropped pairs the fp64 test accepts"
    assert np.array_equal(flt.cpu().numpy(), float_test_counts(rr, s))
    assert np.count_nonzero(got != flt.cpu().numpy()) > len(rays) // 4, "the scene does not separate the tests"
    # and the column densities see the same hit set (a zero term is still a hit; compare via trace_sph)
    offs, idx, _, _ = gh.trace_sph(rays, d, tree, real=torch.float64)
    assert np.array_equal(np.diff(np.append(offs.cpu().numpy(), len(idx))), ref.astype(np.int32))


def _check_per_hit(offs, idx, w, dist, counts, per_ray, sentinels=False):
    offs, idx, w, dist = (t.cpu().numpy() for t in (offs, idx, w, dist))
    ref_offs = np.concatenate([[0], np.cumsum(counts + (1 if sentinels else 0))[:-1]]).astype(np.int32)
    assert np.array_equal(offs, ref_offs)
    for i, (ri, rw, rd, _) in enumerate(per_ray):
        a = offs[i]
        assert np.array_equal(idx[a:a + len(ri)], ri), i
        assert np.array_equal(w[a:a + len(ri)].view(np.uint64), rw.view(np.uint64)), i
        assert np.array_equal(dist[a:a + len(ri)].view(np.uint64), rd.astype(F64).view(np.uint64)), i
        if sentinels:
            e = a + len(ri)
            assert idx[e] == -1 and w[e] == -2.0 and dist[e] == -3.0, i


@pytest.mark.gpu
def test_mixed_per_hit_outputs_and_column_densities(gh, cuda):
    import torch
    d, tree = _scene(gh, cuda, 8000, 21)
    s = d.cpu().numpy()
    for name, rays in _ray_sets(gh, cuda).items():
        rays = rays[:1024]
        rr = rays.cpu().numpy()
        counts, per_ray = restate(rr, s)
        assert counts.sum() > 1000, name
        _check_per_hit(*gh.trace_sph(rays, d, tree, real=torch.float64), counts, per_ray)
        _check_per_hit(*gh.trace_with_sentinels_sph(rays, d, tree, -1, -2.0, -3.0, real=torch.float64),
                       counts, per_ray, sentinels=True)
        cum = torch.empty(len(rays), dtype=torch.float64, device=cuda)
        gh.trace_cumulative_sph(rays, d, tree, cum, check=True)
        got = cum.cpu().numpy()
        ref = np.array([class_sum(ri, w32) for ri, _, _, w32 in per_ray], F64)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), name
        exact = np.array([math.fsum(float(x) for x in w32) for _, _, _, w32 in per_ray], F64)
        nz = exact > 0
        assert np.all(np.abs(got[nz] - exact[nz]) <= 1e-13 * exact[nz]), name
        # the float path's sums (float test, fp32 sums) do not meet that bound
        f32 = torch.empty(len(rays), dtype=torch.float32, device=cuda)
        gh.trace_cumulative_sph(rays, d, tree, f32, check=True)
        rel = np.abs(f32.cpu().numpy()[nz].astype(F64) - exact[nz]) / exact[nz]
        assert rel.max() > 1e-13, name


@pytest.mark.gpu
def test_float_and_mixed_calls_interleave_with_the_scene_cache(gh, cuda):
    import torch
    d, tree = _scene(gh, cuda, 30000, 31)
    rays = gh.orthogonal_rays_z(64, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    n = len(rays)

    def f32():
        out = torch.empty(n, dtype=torch.float32, device=cuda)
        gh.trace_cumulative_sph(rays, d, tree, out, check=True)
        return out.cpu().numpy().view(np.uint32).copy()

    def f64():
        out = torch.empty(n, dtype=torch.float64, device=cuda)
        gh.trace_cumulative_sph(rays, d, tree, out, check=True)
        return out.cpu().numpy().view(np.uint64).copy()

    def counts(fn):
        out = torch.empty(n, dtype=torch.int32, device=cuda)
        fn(rays, d, tree, out, check=True)
        return out.cpu().numpy().copy()

    gh.trace_release(); gh.trace_release_rays()
    gh.set_cache_auto(False)
    try:
        base32, base64 = f32(), f64()
        base_c, base_cm = counts(gh.trace_hitcounts_sph), counts(gh.trace_hitcounts_f4_f64)
    finally:
        gh.set_cache_auto(True)
    for validation in (True, False):
        gh.set_cache_validation(validation)
        try:
            for order in range(2):
                seq = [f32, f64, f32, f32, f64, f64, f32] if order == 0 else [f64, f64, f32, f64, f32, f32]
                for fn in seq:
                    assert np.array_equal(fn(), base32 if fn is f32 else base64), (validation, order, fn.__name__)
                assert np.array_equal(counts(gh.trace_hitcounts_f4_f64), base_cm)
                assert np.array_equal(counts(gh.trace_hitcounts_sph), base_c)
            gh.trace_prepare(d, tree)
            for fn in (f64, f32, f64, f32):
                assert np.array_equal(fn(), base32 if fn is f32 else base64), ("prepared", validation)
            gh.trace_release()
        finally:
            gh.set_cache_validation(True)
    # a mixed call on a modified sphere array (validation on: the float cache must notice too)
    f32(); f32()
    d[:, 3] *= 1.5
    gh.set_cache_auto(False)
    try:
        new32, new64 = f32(), f64()
    finally:
        gh.set_cache_auto(True)
    assert not np.array_equal(new64, base64)
    assert np.array_equal(f64(), new64) and np.array_equal(f32(), new32) and np.array_equal(f64(), new64)
    gh.trace_release(); gh.trace_release_rays()


@pytest.mark.gpu
def test_mixed_precision_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    import torch
    n = 6000
    rng = np.random.default_rng(41)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = (0.02 + 0.04 * rng.random(n)).astype(F32)
    rays = gh.pinhole_camera_rays(32, 32, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0, device=cuda)
    s.tofile(str(tmp_path / "s.f32"))
    rays.cpu().numpy().tofile(str(tmp_path / "r.f32"))
    exe = str(tmp_path / "dropin_mixed_precision")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_mixed_precision.hip"), "-o", exe,
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    res = subprocess.run([exe, str(tmp_path / "s.f32"), str(tmp_path / "r.f32"), "32", str(tmp_path)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    rd = lambda name, dt: np.fromfile(str(tmp_path / name), dt)

    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(n, 32, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    cum = torch.empty(len(rays), dtype=torch.float64, device=cuda)
    gh.trace_cumulative_sph(rays, d, tree, cum, check=True)
    assert np.array_equal(cum.cpu().numpy().view(np.uint64), rd("cum.f64", np.uint64))
    offs, idx, w, dist = gh.trace_sph(rays, d, tree, real=torch.float64)
    assert len(idx) > 0
    for t, name, dt in ((offs, "off.i32", np.int32), (idx, "idx.i32", np.int32), (w, "w.f64", np.uint64),
                        (dist, "d.f64", np.uint64)):
        assert np.array_equal(t.cpu().numpy().view(dt), rd(name, dt)), name
    gh.sort_by_distance(dist, offs, idx, w)
    scanned = torch.empty_like(w)
    gh.exclusive_segmented_scan(offs, w, scanned)
    for t, name, dt in ((idx, "sorted_idx.i32", np.int32), (w, "sorted_w.f64", np.uint64),
                        (dist, "sorted_d.f64", np.uint64), (scanned, "scan.f64", np.uint64)):
        assert np.array_equal(t.cpu().numpy().view(dt), rd(name, dt)), name
    so, si, sw, sd = gh.trace_with_sentinels_sph(rays, d, tree, -1, -2.0, -3.0, real=torch.float64)
    for t, name, dt in ((so, "s_off.i32", np.int32), (si, "s_idx.i32", np.int32), (sw, "s_w.f64", np.uint64),
                        (sd, "s_d.f64", np.uint64)):
        assert np.array_equal(t.cpu().numpy().view(dt), rd(name, dt)), name


@pytest.mark.gpu
def test_mixed_zero_rays_is_a_no_op(gh, cuda):
    import torch
    d, tree = _scene(gh, cuda, 1000, 51)
    rays = torch.empty((0, 7), dtype=torch.float32, device=cuda)
    cum = torch.empty(0, dtype=torch.float64, device=cuda)
    gh.trace_cumulative_sph(rays, d, tree, cum, check=True)
    cnt = torch.empty(0, dtype=torch.int32, device=cuda)
    gh.trace_hitcounts_f4_f64(rays, d, tree, cnt, check=True)
