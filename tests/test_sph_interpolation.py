"""SPH interpolation at points (grace_interpolate_points_f4 / _grid_f4, interpolate_sph /
interpolate_grid_sph): out[p, c] = sum over spheres i containing p of fl32(w[i, c] W_ip), counts[p] =
the number of spheres containing p.

Expected values restate the contract of include/grace_hip.h in NumPy float32 (every operation
rounded, none fused): containment d2 < fl(H*H), q = fl(sqrt(d2) * fl(1/H)), the documented f(q)
forms, W = fl(K * fl(fl(ih*ih)*ih)), fp32 products, fp32 class sums (class (i >> 10) & 7) in
ascending index, classes added pairwise."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32, F64 = np.float32, np.float64
KERNELS = ("cubic", "quartic", "quintic", "wendland_c2", "wendland_c4", "wendland_c6")


def _gen():
    spec = importlib.util.spec_from_file_location(
        "gen_kernel_tables", os.path.join(ROOT, "grace-devel_amd", "tools", "gen_kernel_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the restatement ----------------------------------------------------------------------------
def f32_kernel(name, q):
    """f(q) in the fp32 forms of grace_hip.h (q: float32 array)."""
    q = np.asarray(q, F32)
    u = np.maximum(F32(1) - q, F32(0))
    p4 = lambda t: ((t * t) * (t * t)).astype(F32)
    if name == "cubic":
        inner = ((F32(6) * q - F32(6)) * (q * q)) + F32(1)
        outer = F32(2) * ((u * u) * u)
        return (np.where(q < F32(0.5), inner, outer) * F32(8.0 / np.pi)).astype(F32)
    if name == "quartic":
        t2 = np.maximum(u - F32(0.4), F32(0)); t3 = np.maximum(u - F32(0.8), F32(0))
        return (((p4(u) - F32(5) * p4(t2)) + F32(10) * p4(t3)) * F32(25.0 * 39.0625 / (32.0 * np.pi))).astype(F32)
    if name == "quintic":
        t2 = np.maximum(u - F32(1.0 / 3.0), F32(0)); t3 = np.maximum(u - F32(2.0 / 3.0), F32(0))
        p5 = lambda t: (p4(t) * t).astype(F32)
        return (((p5(u) - F32(6) * p5(t2)) + F32(15) * p5(t3)) * F32(9.0 * 243.0 / (40.0 * np.pi))).astype(F32)
    if name == "wendland_c2":
        return ((p4(u) * (F32(4) * q + F32(1))) * F32(21.0 / (2.0 * np.pi))).astype(F32)
    if name == "wendland_c4":
        u6 = p4(u) * (u * u)
        return ((u6 * (q * (q * F32(35.0 / 3.0) + F32(6)) + F32(1))) * F32(495.0 / (32.0 * np.pi))).astype(F32)
    if name == "wendland_c6":
        u4 = p4(u)
        return (((u4 * u4) * (q * (q * (F32(32) * q + F32(25)) + F32(8)) + F32(1)))
                * F32(1365.0 / (64.0 * np.pi))).astype(F32)
    raise ValueError(name)


def f64_kernel(name, q):
    """The fp64 functions of tools/gen_kernel_tables.py (cubic: the M4 spline with support 1)."""
    q = np.asarray(q, F64)
    if name == "cubic":
        u = np.maximum(1.0 - q, 0.0)
        return 8.0 / np.pi * np.where(q < 0.5, 1.0 - 6.0 * q * q + 6.0 * q ** 3, 2.0 * u ** 3)
    return getattr(_gen(), name)(q) * (q < 1.0)


def pairs(points, s, chunk=256):
    """(point index, sphere index, d2) of every containment d2 < fl(H*H), in fp32 as the contract."""
    P = np.ascontiguousarray(points[:, :3], F32)
    H2 = (s[:, 3] * s[:, 3]).astype(F32)
    out_p, out_s, out_d2 = [], [], []
    for a in range(0, len(P), chunk):
        p = P[a:a + chunk]
        dx = (p[:, None, 0] - s[None, :, 0]).astype(F32)
        dy = (p[:, None, 1] - s[None, :, 1]).astype(F32)
        dz = (p[:, None, 2] - s[None, :, 2]).astype(F32)
        d2 = ((dx * dx + dy * dy) + dz * dz).astype(F32)
        pi, si = np.nonzero(d2 < H2[None, :])
        out_p.append(pi + a); out_s.append(si); out_d2.append(d2[pi, si])
    return np.concatenate(out_p), np.concatenate(out_s), np.concatenate(out_d2).astype(F32)


def restate(n_points, pr, s, w, kernel):
    """(fp32 sums [n, C], counts [n], fp64 sums [n, C], fp64 bound [n, C]).  The bound is 1e-5 of
    sum |w| W plus the conditioning of W in q: q formed in fp32 is within ~4 ulp of the exact
    |p - x| / H, which near the support edge (u = 1 - q small) is a large relative change of W."""
    pi, si, d2 = pr
    H = s[si, 3]
    ih = (F32(1) / H).astype(F32)
    q = (np.sqrt(d2) * ih).astype(F32)
    W = (f32_kernel(kernel, q) * ((ih * ih) * ih)).astype(F32)
    counts = np.bincount(pi, minlength=n_points).astype(np.int32)
    cls = (si >> 10) & 7
    order = np.lexsort((si, cls, pi))
    pi_o, cls_o, si_o, W_o = pi[order], cls[order], si[order], W[order]
    group = pi_o * 8 + cls_o
    rank = np.arange(len(group)) - np.searchsorted(group, group, side="left")
    width = int(rank.max()) + 1 if len(group) else 1
    C = w.shape[1]
    out = np.zeros((n_points, C), F32)
    for c in range(C):
        terms = (w[si_o, c] * W_o).astype(F32)
        m = np.zeros((n_points * 8, width), F32)
        m[group, rank] = terms
        acc = np.zeros(n_points * 8, F32)
        for j in range(width):
            acc = (acc + m[:, j]).astype(F32)
        t = acc.reshape(n_points, 8)
        out[:, c] = (((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])) + ((t[:, 4] + t[:, 5]) + (t[:, 6] + t[:, 7])))
    H64 = H.astype(F64)
    W64 = f64_kernel(kernel, np.sqrt(d2.astype(F64)) / H64) / H64 ** 3
    wW = w[si].astype(F64) * W64[:, None]
    q64 = np.sqrt(d2.astype(F64)) / H64
    dq = 1e-7
    dW = np.abs(f64_kernel(kernel, q64 + dq) - f64_kernel(kernel, np.maximum(q64 - dq, 0.0))) / (2 * dq) / H64 ** 3
    cond = np.abs(w[si]).astype(F64) * (dW * q64 * 2.0 ** -21)[:, None]
    ref64 = np.zeros((n_points, C)); np.add.at(ref64, pi, wW)
    bound = np.zeros((n_points, C)); np.add.at(bound, pi, 1e-5 * np.abs(wW) + cond)
    return out, counts, ref64, bound


def lattice(origin, u, v, w, dims):
    """The grid's points in row-major order, fl(fl(fl(o + fl(i u)) + fl(j v)) + fl(k w))."""
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz, dtype=F32), np.arange(ny, dtype=F32), np.arange(nx, dtype=F32),
                          indexing="ij")
    i, j, k = i.reshape(-1), j.reshape(-1), k.reshape(-1)
    o, u, v, w = (np.asarray(x, F32) for x in (origin, u, v, w))
    p = np.empty((len(i), 3), F32)
    for d in range(3):
        p[:, d] = (((o[d] + i * u[d]).astype(F32) + (j * v[d]).astype(F32)).astype(F32) + (k * w[d]).astype(F32))
    return p


# ---- CPU ------------------------------------------------------------------------------------------
def test_interpolation_symbols_exported():
    import ctypes
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    for name in ("grace_interpolate_points_f4", "grace_interpolate_grid_f4", "grace_interpolate_enable_stats",
                 "grace_interpolate_last_stats"):
        assert hasattr(lib, name), name


def test_interpolation_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_interpolate"
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_interpolate.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


def test_interpolation_double4_is_a_clear_compile_error(tmp_path):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/interpolate_sph.cuh"\n'
                   "void f(const thrust::device_vector<float4>& p, const thrust::device_vector<double4>& s,\n"
                   "       const grace::Tree& t, const thrust::device_vector<float>& w,\n"
                   "       thrust::device_vector<float>& out)\n"
                   "{ grace::interpolate_sph(p, s, t, w, 1, out); }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "float4 spheres only" in res.stderr


def test_interpolation_mirror_compiles_with_hipcc(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& p, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::Tree& t, const grace::device_vector<float>& w)\n"
                   "{\n"
                   "    grace::device_vector<float> out(p.size() * 2);\n"
                   "    grace::device_vector<int> counts(p.size());\n"
                   "    grace::interpolate_sph(p, s, t, w, 2, out, &counts);\n"
                   "    grace::device_vector<float> g(8 * 8 * 2);\n"
                   "    grace::interpolate_grid_sph(grace::make_float3(0, 0, 0), grace::make_float3(1, 0, 0),\n"
                   "                                grace::make_float3(0, 1, 0), grace::make_float3(0, 0, 1),\n"
                   "                                8, 8, 1, s, t, w, 2, g);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    for cc in (["g++", "-std=c++14", "-O1", "-Wall", "-Werror"], ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950",
                                                                  "-std=c++17", "-O1", "-x", "c++"]):
        subprocess.check_call([*cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                               "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
        assert exe.exists()
        exe.unlink()


@pytest.mark.parametrize("kernel", KERNELS)
def test_fp32_forms_agree_with_the_fp64_functions(kernel):
    q = np.linspace(0.0, 1.0, 200001).astype(F32)
    got = f32_kernel(kernel, q).astype(F64)
    ref = f64_kernel(kernel, q.astype(F64))
    f0 = f64_kernel(kernel, np.zeros(1))[0]
    # a few ulp of the value, or of f(0) where the forms cancel (the spline pieces near q = 0) or the
    # value is subnormal in fp32 (u^8 near q = 1)
    err = np.abs(got - ref)
    assert np.all(err <= 16 * np.spacing(np.abs(ref).astype(F32)).astype(F64) + 16 * np.spacing(F32(f0))), \
        (kernel, float(np.max(err / np.maximum(np.abs(ref), 1e-30))))
    assert np.all(got >= 0.0) and got[-1] == 0.0


@pytest.mark.parametrize("kernel", KERNELS)
def test_restated_one_sphere_grid_integrates_to_one(kernel):
    n = 72
    h = F32(2.0 / n)
    H = F32(0.9)
    o = F32(-1.0) + h / F32(2)
    pts = lattice((o, o, o), (h, 0, 0), (0, h, 0), (0, 0, h), (n, n, n))
    s = np.array([[0.0, 0.0, 0.0, H]], F32)
    pr = pairs(pts, s, chunk=1 << 16)
    out, counts, _, _ = restate(len(pts), pr, s, np.ones((1, 1), F32), kernel)
    total = float(out[:, 0].astype(F64).sum()) * float(h) ** 3
    assert abs(total - 1.0) < 1e-3, (kernel, total)
    assert counts.max() == 1


# ---- GPU --------------------------------------------------------------------------------------------
N_SCENE = 20000   # > 8192: all eight summation classes hold spheres


def _build(gh, s, cuda):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(s, F32)).to(cuda)
    tree = gh.Tree(len(s), 32, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))     # sorts d
    return d, tree


def _random_scene(n=N_SCENE, seed=3, hlo=0.01, hhi=0.05):
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = (hlo + (hhi - hlo) * rng.random(n)).astype(F32)
    return s


def _clustered_scene(n=N_SCENE, seed=5):
    rng = np.random.default_rng(seed)
    centres = np.array([[0.3, 0.3, 0.3], [0.7, 0.6, 0.4], [0.5, 0.5, 0.8]])
    k = rng.integers(0, 3, n)
    s = np.empty((n, 4), F32)
    s[:, :3] = np.clip(centres[k] + rng.normal(0.0, 0.02, (n, 3)) * rng.random((n, 1)) ** 3, 0.001, 0.999)
    s[:, 3] = (0.004 + 0.02 * rng.random(n)).astype(F32)
    return s


def _weights(n, C, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random((n, C)) * 4.0 - 2.0)).astype(F32)


def _point_sets():
    rng = np.random.default_rng(11)
    th = 0.3
    return {
        "random": rng.random((3000, 3), dtype=F32) * F32(1.1) - F32(0.05),
        "slice128": ((0.0, 0.0, 0.5), (1 / 128, 0, 0), (0, 1 / 128, 0), (0, 0, 1), (128, 128, 1)),
        "oblique": ((0.05, 0.1, 0.2), (np.cos(th) / 100, 0.0, np.sin(th) / 100), (0.0, 1 / 96, 0.003),
                    (0, 0, 1), (100, 96, 1)),
        "grid32": ((0.01, 0.02, 0.03), (1 / 32, 0, 0), (0, 1 / 32, 0), (0, 0, 1 / 32), (32, 32, 32)),
    }


def _points_of(spec):
    return spec if isinstance(spec, np.ndarray) else lattice(*spec)


def _run(gh, spec, d, tree, w, cuda, counts=True):
    """The GPU's (out [n, C], counts [n]) for a point set: points entry point or grid entry point."""
    import torch
    wt = None if w is None else torch.from_numpy(w).to(cuda)
    if isinstance(spec, np.ndarray):
        pts = torch.from_numpy(np.ascontiguousarray(spec, F32)).to(cuda)
        n = len(spec)
        cnt = torch.empty(n, dtype=torch.int32, device=cuda) if counts else None
        out, cnt = gh.interpolate_sph(pts, d, tree, wt, counts=cnt, check=True)
    else:
        o, u, v, ww, dims = spec
        n = dims[0] * dims[1] * dims[2]
        cnt = torch.empty((dims[2], dims[1], dims[0]), dtype=torch.int32, device=cuda) if counts else None
        out, cnt = gh.interpolate_grid_sph(o, u, v, ww, dims, d, tree, wt, counts=cnt, check=True)
    out = None if out is None else out.cpu().numpy().reshape(n, -1)
    cnt = None if cnt is None else cnt.cpu().numpy().reshape(n)
    return out, cnt


@pytest.fixture(scope="module")
def scenes(gh, cuda):
    res = {}
    for name, s in (("random", _random_scene()), ("clustered", _clustered_scene())):
        d, tree = _build(gh, s, cuda)
        sh = d.cpu().numpy()
        sets = {}
        for pname, spec in _point_sets().items():
            pts = _points_of(spec)
            sets[pname] = (spec, pts, pairs(pts, sh))
        res[name] = (d, tree, sh, sets)
    return res


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["random", "clustered"])
def test_counts_equal_brute_force(gh, scenes, scene, cuda):
    d, tree, sh, sets = scenes[scene]
    for pname, (spec, pts, pr) in sets.items():
        _, got = _run(gh, spec, d, tree, None, cuda)
        ref = np.bincount(pr[0], minlength=len(pts))
        assert np.array_equal(got, ref), (scene, pname, np.nonzero(got != ref)[0][:5])
    gh.trace_status()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["random", "clustered"])
def test_field_is_the_restatement_bit_for_bit(gh, scenes, scene, kernel, cuda, kernel_reset):
    d, tree, sh, sets = scenes[scene]
    gh.set_sph_kernel(kernel)
    for C in (1, 2, 4, 6):
        w = _weights(len(sh), C, 7 + C)
        for pname, (spec, pts, pr) in sets.items():
            got, cnt = _run(gh, spec, d, tree, w, cuda)
            ref32, counts, ref64, bound = restate(len(pts), pr, sh, w, kernel)
            assert np.array_equal(cnt, counts), (pname, C)
            bad = np.nonzero(got.view(np.uint32) != ref32.view(np.uint32))
            assert len(bad[0]) == 0, (pname, C, bad[0][:5], got[bad][:5], ref32[bad][:5])
            assert np.all(np.abs(got - ref64) <= bound + 1e-30), (pname, C)


@pytest.mark.gpu
def test_edge_cases(gh, cuda):
    import torch
    s = _random_scene(4000, 21)
    # coincident spheres, and one huge sphere that covers everything
    s[100] = s[101] = s[102] = np.array([0.5, 0.5, 0.5, 0.1], F32)
    s[3999] = np.array([0.5, 0.5, 0.5, 3.0], F32)
    s[50] = np.array([0.5, 0.25, 0.75, 0.125], F32)                # (binary-exact: points exactly on its surface)
    d, tree = _build(gh, s, cuda)
    sh = d.cpu().numpy()
    i = int(np.nonzero(sh[:, 3] == F32(0.1))[0][0])
    rng = np.random.default_rng(2)
    pts = np.concatenate([
        sh[:64, :3],                                               # at sphere centres: f(0)
        np.array([[0.625, 0.25, 0.75], [0.5, 0.125, 0.75], [0.5, 0.25, 0.875]], F32),                # on a surface
        np.array([[50.0, 50.0, 50.0], [-40.0, 0.5, 0.5], [0.5, 1e6, 0.5]], F32),                     # far outside
        np.array([[np.nan, 0.5, 0.5], [0.5, np.nan, np.nan]], F32),                                  # NaN points
        rng.random((200, 3), dtype=F32),
        sh[i:i + 1, :3],
    ]).astype(F32)
    pr = pairs(pts, sh)
    w = _weights(len(sh), 3, 4)
    got, cnt = _run(gh, pts, d, tree, w, cuda)
    ref32, counts, _, _ = restate(len(pts), pr, sh, w, "cubic")
    assert np.array_equal(cnt, counts)
    assert np.array_equal(got.view(np.uint32), ref32.view(np.uint32))
    k = int(np.nonzero(np.all(sh == np.array([0.5, 0.25, 0.75, 0.125], F32), axis=1))[0][0])
    assert not np.any((pr[0] >= 64) & (pr[0] < 67) & (pr[1] == k))   # a surface point is not contained
    assert np.all(cnt[67:70] == 0) and np.all(got[67:70] == 0)
    assert np.all(cnt[70:72] == 0) and np.all(got[70:72] == 0)
    assert cnt[-1] >= 4                                            # the coincident spheres and the huge one
    assert np.all(cnt[:64] >= 2)                                   # its own sphere and the huge one
    # zero points: nothing written
    out, cn = gh.interpolate_sph(torch.empty((0, 3), dtype=torch.float32, device=cuda), d, tree,
                                 torch.from_numpy(w).to(cuda), check=True)
    assert tuple(out.shape) == (0, 3) and cn is None


@pytest.mark.gpu
def test_custom_table_and_bad_arguments_write_nothing(gh, scenes, cuda, kernel_reset):
    import ctypes as C
    import torch
    d, tree, sh, sets = scenes["random"]
    n = len(sh)
    pts = torch.rand((100, 4), dtype=torch.float32, device=cuda)
    w = torch.ones((n, 2), dtype=torch.float32, device=cuda)
    out = torch.full((100, 2), 7.0, dtype=torch.float32, device=cuda)
    cnt = torch.full((100,), 7, dtype=torch.int32, device=cuda)
    scene = gh._interp_scene(d, tree)
    lib = gh._lib

    def call(p=pts, n_pts=100, elems=4, wp=w, n_ch=2, op=out, cp=cnt):
        return lib.grace_interpolate_points_f4(gh._ptr(p), C.c_size_t(n_pts), C.c_int(elems), *scene, gh._ptr(wp),
                                               C.c_int(n_ch), gh._ptr(op), gh._ptr(cp), gh._stream())

    for kw in (dict(elems=2), dict(elems=17), dict(n_ch=0), dict(n_ch=65), dict(wp=None), dict(op=None, cp=None)):
        assert call(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    o3 = (C.c_float * 3)(0, 0, 0); uvw = (C.c_float * 9)(0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1)
    for dims in ((0, 10, 1), (10, -1, 1), (10, 10, 0)):
        d3 = (C.c_int * 3)(*dims)
        st = lib.grace_interpolate_grid_f4(o3, uvw, d3, *scene, gh._ptr(w), C.c_int(2), gh._ptr(out), gh._ptr(cnt),
                                           gh._stream())
        assert st == gh.GRACE_INVALID_ARGUMENT, dims
    gh.set_sph_kernel(gh.sph_kernel_table("quartic"))             # a custom table: no f(q)
    assert call() == gh.GRACE_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        gh.interpolate_sph(pts, d, tree, w)
    torch.cuda.synchronize()
    assert torch.all(out == 7.0) and torch.all(cnt == 7)
    gh.set_sph_kernel("cubic")
    assert call() == gh.GRACE_OK
    gh.trace_status()
    with pytest.raises(ValueError):
        gh.interpolate_sph(pts, d, tree, torch.ones(n - 1, dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        gh.interpolate_sph(pts, d, tree, torch.ones((n, 65), dtype=torch.float32, device=cuda))


@pytest.mark.gpu
def test_deep_clustered_tree_fits_the_stack(gh, cuda):
    rng = np.random.default_rng(9)
    n = 30000
    s = np.empty((n, 4), F32)
    # nested clusters: a quarter of the points each time ten times closer to one centre
    scale = 0.4 * 0.1 ** (rng.integers(0, 5, n))
    s[:, :3] = (0.5 + scale[:, None] * (rng.random((n, 3)) - 0.5)).astype(F32)
    s[:, 3] = (scale * (0.05 + 0.1 * rng.random(n))).astype(F32) + F32(1e-7)
    d, tree = _build(gh, s, cuda)
    sh = d.cpu().numpy()
    pts = (0.5 + (rng.random((2000, 3)) - 0.5) * 0.4 * 0.1 ** rng.integers(0, 5, (2000, 1))).astype(F32)
    pr = pairs(pts, sh)
    w = _weights(n, 1, 3)
    got, cnt = _run(gh, pts, d, tree, w, cuda)
    gh.trace_status()                                             # GRACE_OK: no packet ran out of stack
    ref32, counts, _, _ = restate(len(pts), pr, sh, w, "cubic")
    assert np.array_equal(cnt, counts)
    assert np.array_equal(got.view(np.uint32), ref32.view(np.uint32))


@pytest.mark.gpu
def test_results_do_not_depend_on_order_layout_or_entry_point(gh, scenes, cuda):
    import torch
    d, tree, sh, sets = scenes["clustered"]
    w = _weights(len(sh), 4, 31)
    spec = sets["oblique"][0]
    grid_out, grid_cnt = _run(gh, spec, d, tree, w, cuda)
    pts = sets["oblique"][1]
    pt_out, pt_cnt = _run(gh, pts, d, tree, w, cuda)                # the same fp32 points, points entry point
    assert np.array_equal(grid_out.view(np.uint32), pt_out.view(np.uint32))
    assert np.array_equal(grid_cnt, pt_cnt)
    perm = np.random.default_rng(1).permutation(len(pts))
    sh_out, sh_cnt = _run(gh, pts[perm], d, tree, w, cuda)           # shuffled order
    assert np.array_equal(sh_out.view(np.uint32), pt_out[perm].view(np.uint32))
    assert np.array_equal(sh_cnt, pt_cnt[perm])
    wide = np.zeros((len(pts), 4), F32); wide[:, :3] = pts; wide[:, 3] = 123.0
    w4_out, w4_cnt = _run(gh, wide, d, tree, w, cuda)                # elems_per_point 4
    assert np.array_equal(w4_out.view(np.uint32), pt_out.view(np.uint32)) and np.array_equal(w4_cnt, pt_cnt)
    # the cache knobs of the trace
    for auto, valid in ((False, True), (True, False), (True, True)):
        gh.set_cache_auto(auto); gh.set_cache_validation(valid)
        try:
            o, c = _run(gh, spec, d, tree, w, cuda)
        finally:
            gh.set_cache_auto(True); gh.set_cache_validation(True)
        assert np.array_equal(o.view(np.uint32), grid_out.view(np.uint32)) and np.array_equal(c, grid_cnt)
    # channels are independent of their walk: channel 5 of six = channel 1 of two
    w6 = np.concatenate([w, w[:, :2]], axis=1)
    o6, _ = _run(gh, pts, d, tree, w6, cuda)
    assert np.array_equal(o6[:, :4].view(np.uint32), pt_out.view(np.uint32))
    assert np.array_equal(o6[:, 4:].view(np.uint32), pt_out[:, :2].view(np.uint32))
    # counts only
    _, c0 = _run(gh, pts, d, tree, None, cuda)
    assert np.array_equal(c0, pt_cnt)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_interleaved_traces_stay_bit_identical(gh, scenes, cuda):
    import torch
    d, tree, sh, sets = scenes["random"]
    rays = gh.orthogonal_rays_z(64, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    w = _weights(len(sh), 2, 5)
    spec = sets["slice128"][0]

    def trace():
        out = torch.empty(len(rays), dtype=torch.float32, device=cuda)
        gh.trace_cumulative_sph(rays, d, tree, out, check=True)
        return out.cpu().numpy()

    alone = [trace() for _ in range(3)]
    ref_field, ref_cnt = _run(gh, spec, d, tree, w, cuda)
    for k in range(3):
        f, c = _run(gh, spec, d, tree, w, cuda)
        t = trace()
        assert np.array_equal(t.view(np.uint32), alone[k].view(np.uint32))
        assert np.array_equal(f.view(np.uint32), ref_field.view(np.uint32)) and np.array_equal(c, ref_cnt)


def _quadrature_tolerance(table, h_min, dz):
    """Largest |midpoint sum of W along a chord - lerp(F, 50 b / H) / H^2| over impact parameters and
    sampling phases, relative to F(0) / H^2, for the smallest sphere: the error per hit of comparing
    a sampled column with the traced one (quadrature of the restated W, plus the table lerp's bias)."""
    H = h_min
    worst = 0.0
    for b in np.linspace(0.0, 0.98, 50):
        x = 50.0 * b
        i = min(int(x), 49)
        lerp = (table[i] + (x - i) * (table[i + 1] - table[i])) / H ** 2
        for phase in np.linspace(0.0, 1.0, 8, endpoint=False):
            z = (np.arange(-H, H + dz, dz) + phase * dz)
            r = np.sqrt((b * H) ** 2 + z ** 2) / H
            quad = float(np.sum(f64_kernel("cubic", r) / H ** 3) * dz)
            worst = max(worst, abs(quad - lerp) / (table[0] / H ** 2))
    return worst


@pytest.mark.gpu
def test_sampled_columns_match_the_traced_column_densities(gh, cuda):
    import torch
    s = _random_scene(3000, 13, 0.05, 0.1)
    s[:, 2] = (0.2 + 0.6 * s[:, 2]).astype(F32)
    d, tree = _build(gh, s, cuda)
    n_side, nz = 32, 768
    z0, z1 = 0.0, 1.0
    dz = (z1 - z0) / nz
    tol = _quadrature_tolerance(gh.sph_kernel_table("cubic"), 0.05, dz)
    assert tol < 5e-3
    # rays along +z through the cell centres of an n_side^2 grid over the unit square
    xy = (np.arange(n_side) + 0.5) / n_side
    Y, X = np.meshgrid(xy, xy, indexing="ij")
    rays = np.zeros((n_side * n_side, 7), F32)
    rays[:, 0] = 0.0; rays[:, 1] = 0.0; rays[:, 2] = 1.0           # dx dy dz
    rays[:, 3] = X.reshape(-1); rays[:, 4] = Y.reshape(-1); rays[:, 5] = z0; rays[:, 6] = z1 - z0
    rt = torch.from_numpy(rays).to(cuda)
    traced = torch.empty(len(rays), dtype=torch.float32, device=cuda)
    gh.trace_cumulative_sph(rt, d, tree, traced, check=True)
    cnt = torch.empty(len(rays), dtype=torch.int32, device=cuda)
    gh.trace_hitcounts_sph(rt, d, tree, cnt, check=True)
    field, _ = gh.interpolate_grid_sph((0.5 / n_side, 0.5 / n_side, z0 + 0.5 * dz), (1 / n_side, 0, 0),
                                       (0, 1 / n_side, 0), (0, 0, dz), (n_side, n_side, nz), d, tree,
                                       torch.ones(len(s), dtype=torch.float32, device=cuda), check=True)
    sampled = field.double().sum(dim=0).cpu().numpy().reshape(-1) * dz
    traced = traced.cpu().numpy().astype(F64)
    bound = 2.0 * tol * cnt.cpu().numpy() * gh.sph_kernel_table("cubic")[0] / 0.05 ** 2 + 1e-3 * traced
    assert np.all(np.abs(sampled - traced) <= bound)
    well = traced > 0.1 * traced.max()
    assert np.median(np.abs(sampled[well] - traced[well]) / traced[well]) < 2e-3


@pytest.mark.gpu
def test_interpolation_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    import torch
    d, tree = _build(gh, _random_scene(9000, 41, 0.02, 0.06), cuda)
    s = d.cpu().numpy()                                               # tree order
    rng = np.random.default_rng(3)
    pts = rng.random((777, 4), dtype=F32)
    w = _weights(len(s), 5, 43)
    s.tofile(str(tmp_path / "s.f32")); pts.tofile(str(tmp_path / "p.f32")); w.tofile(str(tmp_path / "w.f32"))
    exe = str(tmp_path / "dropin_interpolate")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_interpolate.hip"), "-o", exe,
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    res = subprocess.run([exe, str(tmp_path / "s.f32"), str(tmp_path / "p.f32"), str(tmp_path / "w.f32"), "5",
                          str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got, cnt = _run(gh, pts, d, tree, w, cuda)
    assert np.array_equal(got.reshape(-1).view(np.uint32), np.fromfile(str(tmp_path / "points.f32"), np.uint32))
    assert np.array_equal(cnt, np.fromfile(str(tmp_path / "counts.i32"), np.int32))
    grid, _ = _run(gh, ((0, 0, 0.25), (1 / 16, 0, 0), (0, 1 / 32, 0), (0, 0, 0.25), (16, 32, 3)), d, tree, w, cuda)
    assert np.array_equal(grid.reshape(-1).view(np.uint32), np.fromfile(str(tmp_path / "grid.f32"), np.uint32))
