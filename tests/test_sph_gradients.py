"""SPH gradients at points (grace_interpolate_gradient_points_f4 / _grid_f4, grace_gradient_div_curl_f32;
interpolate_gradient_sph / interpolate_gradient_grid_sph / divergence_curl_sph):
grad[p, c, k] = sum over spheres i containing p of fl(fl(w[i, c] G) n_k), G = H^-4 f'(q), n the unit vector
from the sphere's centre to the point, +0 at the centre itself.

Expected values restate the contract of include/grace_hip.h ("SPH gradients at points") in NumPy float32
(every operation rounded, none fused) on top of test_sph_interpolation's restatement of the field: its
pairs (containment d2 < fl(H*H)), its f(q) forms, its class-ordered sums."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import periodic_query_scenes as S
import test_sph_interpolation as T
from test_periodic_queries import _build as build_small
from test_range_queries import digest
from test_sph_interpolation import F32, F64, HIPCC_FLAGS, KERNELS, LIBDIR, ROOT, f32_kernel, f64_kernel, lattice, pairs

EPS = 2.0 ** -24                                                   # fp32 unit roundoff
NORM = {"cubic": 8.0 / np.pi, "quartic": 25.0 * 39.0625 / (32.0 * np.pi), "quintic": 9.0 * 243.0 / (40.0 * np.pi),
        "wendland_c2": 21.0 / (2.0 * np.pi), "wendland_c4": 495.0 / (32.0 * np.pi),
        "wendland_c6": 1365.0 / (64.0 * np.pi)}
SYMBOLS = ("grace_interpolate_gradient_points_f4", "grace_interpolate_gradient_grid_f4",
           "grace_interpolate_gradient_points_periodic_f4", "grace_interpolate_gradient_grid_periodic_f4",
           "grace_gradient_div_curl_f32")


# ---- the restatement ----------------------------------------------------------------------------
def df32_kernel(name, q):
    """f'(q) in the fp32 forms of grace_hip.h (q: float32 array)."""
    q = np.asarray(q, F32)
    u = np.maximum(F32(1) - q, F32(0))
    p3 = lambda t: ((t * t) * t).astype(F32)
    p4 = lambda t: ((t * t) * (t * t)).astype(F32)
    if name == "cubic":
        inner = (F32(18) * q - F32(12)) * q
        outer = F32(-6) * (u * u)
        e = np.where(q < F32(0.5), inner, outer)
    elif name == "quartic":
        t2 = np.maximum(u - F32(0.4), F32(0)); t3 = np.maximum(u - F32(0.8), F32(0))
        e = (F32(20) * p3(t2) - F32(4) * p3(u)) - F32(40) * p3(t3)
    elif name == "quintic":
        t2 = np.maximum(u - F32(1.0 / 3.0), F32(0)); t3 = np.maximum(u - F32(2.0 / 3.0), F32(0))
        e = (F32(30) * p4(t2) - F32(5) * p4(u)) - F32(75) * p4(t3)
    elif name == "wendland_c2":
        e = (F32(-20) * q) * p3(u)
    elif name == "wendland_c4":
        e = ((F32(-56.0 / 3.0) * q) * (F32(5) * q + F32(1))) * (p4(u) * u)
    elif name == "wendland_c6":
        e = ((F32(-22) * q) * (q * (F32(16) * q + F32(7)) + F32(1))) * ((p4(u) * (u * u)) * u)
    else:
        raise ValueError(name)
    return (e.astype(F32) * F32(NORM[name])).astype(F32)


def _pieces(name, q):
    """The analytic f'(q) / normalisation in fp64 as signed pieces [(value, |d value / d t| dt)], t the piece's
    own clipped variable with the absolute error dt of its fp32 value: u = fl(1 - q) is within EPS of 1 - q
    (half an ulp of a value <= 1, with room), t2 and t3 within 2 EPS (u's error, the constant's rounding
    <= 2^-25, the subtraction's <= 2^-25)."""
    q = np.asarray(q, F64)
    u = np.maximum(1.0 - q, 0.0)
    du, dt = EPS, 2.0 * EPS
    if name == "cubic":
        lo = q < 0.5
        return [(np.where(lo, 18.0 * q * q, 0.0), 0.0), (np.where(lo, -12.0 * q, 0.0), 0.0),
                (np.where(lo, 0.0, -6.0 * u * u), np.where(lo, 0.0, 12.0 * u * du))]
    if name == "quartic":
        t2, t3 = np.maximum(u - 0.4, 0.0), np.maximum(u - 0.8, 0.0)
        return [(20.0 * t2 ** 3, 60.0 * t2 ** 2 * dt), (-4.0 * u ** 3, 12.0 * u ** 2 * du),
                (-40.0 * t3 ** 3, 120.0 * t3 ** 2 * dt)]
    if name == "quintic":
        t2, t3 = np.maximum(u - 1.0 / 3.0, 0.0), np.maximum(u - 2.0 / 3.0, 0.0)
        return [(30.0 * t2 ** 4, 120.0 * t2 ** 3 * dt), (-5.0 * u ** 4, 20.0 * u ** 3 * du),
                (-75.0 * t3 ** 4, 300.0 * t3 ** 3 * dt)]
    if name == "wendland_c2":
        return [(-20.0 * q * u ** 3, 60.0 * q * u ** 2 * du)]
    if name == "wendland_c4":
        return [(-56.0 / 3.0 * q * (5.0 * q + 1.0) * u ** 5, 56.0 / 3.0 * q * (5.0 * q + 1.0) * 5.0 * u ** 4 * du)]
    if name == "wendland_c6":
        poly = q * (16.0 * q + 7.0) + 1.0
        return [(-22.0 * q * poly * u ** 7, 22.0 * q * poly * 7.0 * u ** 6 * du)]
    raise ValueError(name)


def df64_kernel(name, q):
    """The analytic derivatives in fp64 of the functions of tools/gen_kernel_tables.py (0 from q = 1 on)."""
    q = np.asarray(q, F64)
    return NORM[name] * sum(v for v, _ in _pieces(name, q)) * (q < 1.0)


def df_margin(name, q):
    """|df32_kernel(q) - df64_kernel(q)| from the fp32 rounding of the forms: every form is a sum of pieces,
    each a chain of at most 14 rounded operations and rounded constants on top of its variable (Wendland C6,
    with the normalisation and the final sums: 16q, +7, *q, +1, -22q, *, four for p7, *, the normalisation,
    two constants), so a piece's relative error is below 16 EPS to first order; the error of the piece's
    variable enters through the piece's derivative (_pieces)."""
    return NORM[name] * sum(16.0 * EPS * np.abs(v) + dv for v, dv in _pieces(name, q))


def separations(points, s, pr, period=None):
    """fl(p - x) per component of the pairs, wrapped once in a periodic box; their d2 is the pairs'."""
    pi, si, d2 = pr
    P = np.ascontiguousarray(points[:, :3], F32)
    d = []
    for k in range(3):
        dk = (P[pi, k] - s[si, k]).astype(F32)
        d.append(dk if period is None else S.wrap(dk, period[k]))
    assert np.array_equal(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(F32), d2)
    return d


def class_sums(n_points, pi, si, terms):
    """Column-wise fp32 sums of terms [n_pairs, K] per point: class (i >> 10) & 7, ascending index within
    a class, the 8 class sums added pairwise (test_sph_interpolation.restate's order)."""
    cls = (si >> 10) & 7
    order = np.lexsort((si, cls, pi))
    group = (pi * 8 + cls)[order]
    rank = np.arange(len(group)) - np.searchsorted(group, group, side="left")
    width = int(rank.max()) + 1 if len(group) else 1
    out = np.zeros((n_points, terms.shape[1]), F32)
    for c in range(terms.shape[1]):
        m = np.zeros((n_points * 8, width), F32)
        m[group, rank] = terms[order, c]
        acc = np.zeros(n_points * 8, F32)
        for j in range(width):
            acc = (acc + m[:, j]).astype(F32)
        t = acc.reshape(n_points, 8)
        out[:, c] = (((t[:, 0] + t[:, 1]) + (t[:, 2] + t[:, 3])) + ((t[:, 4] + t[:, 5]) + (t[:, 6] + t[:, 7])))
    return out


def restate_gradient(points, pr, s, w, kernel, period=None):
    """(fp32 gradient [n, C, 3], fp64 gradient [n, C, 3], fp64 bound [n, C, 3]).  The fp64 gradient takes the
    fp32 separations as given.  The bound: the project's 1e-5 of sum |term|; the fp32 rounding of the f'
    form (df_margin); the conditioning of f' in q as in test_sph_interpolation.restate (q formed in fp32 is
    within ~4 ulp of |d| / H)."""
    n = len(points)
    pi, si, d2 = pr
    d = separations(points, s, pr, period)
    H = s[si, 3]
    ih = (F32(1) / H).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(d2).astype(F32)
        q = (r * ih).astype(F32)
        ih2 = (ih * ih).astype(F32)
        G = (df32_kernel(kernel, q) * (ih2 * ih2).astype(F32)).astype(F32)
        ir = (F32(1) / r).astype(F32)
        C_ = w.shape[1]
        terms = np.zeros((len(pi), C_ * 3), F32)
        for c in range(C_):
            wG = (w[si, c] * G).astype(F32)
            for k in range(3):
                nk = (d[k] * ir).astype(F32)
                terms[:, c * 3 + k] = np.where(d2 > F32(0), (wG * nk).astype(F32), F32(0))
    g32 = class_sums(n, pi, si, terms).reshape(n, C_, 3)
    # fp64
    H64 = H.astype(F64)
    d64 = np.stack([x.astype(F64) for x in d], axis=1)
    r64 = np.sqrt((d64 * d64).sum(axis=1))
    q64 = r64 / H64
    with np.errstate(divide="ignore", invalid="ignore"):
        n64 = np.where(r64[:, None] > 0, d64 / r64[:, None], 0.0)
    G64 = df64_kernel(kernel, q64) / H64 ** 4
    dq = 1e-7
    ddf = np.abs(df64_kernel(kernel, q64 + dq) - df64_kernel(kernel, np.maximum(q64 - dq, 0.0))) / (2 * dq)
    slack = (df_margin(kernel, q64) + ddf * q64 * 2.0 ** -21) / H64 ** 4
    ref = np.zeros((n, C_, 3)); bound = np.zeros((n, C_, 3))
    w64 = w[si].astype(F64)
    t64 = w64[:, :, None] * (G64[:, None] * n64)[:, None, :]
    np.add.at(ref, pi, t64)
    np.add.at(bound, pi, 1e-5 * np.abs(t64) + np.abs(w64)[:, :, None] * (slack[:, None] * np.abs(n64))[:, None, :])
    return g32, ref, bound


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ---- CPU ------------------------------------------------------------------------------------------
def test_gradient_symbols_exported_and_declared(gh):
    lib = gh._lib                                                   # (the binding's own handle: it loads torch's HIP runtime first)
    header = open(os.path.join(ROOT, "include", "grace_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"grace_status\s+%s\(" % name, header), name


def test_gradient_double4_is_a_clear_compile_error(tmp_path):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/interpolate_sph.cuh"\n'
                   "void f(const thrust::device_vector<float4>& p, const thrust::device_vector<double4>& s,\n"
                   "       const grace::Tree& t, const thrust::device_vector<float>& w,\n"
                   "       thrust::device_vector<float>& grad)\n"
                   "{ grace::interpolate_gradient_sph(p, s, t, w, 1, grad); }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "float4 spheres only" in res.stderr


def test_gradient_mirror_compiles_with_gcc(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& p, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::Tree& t, const grace::device_vector<float>& w)\n"
                   "{\n"
                   "    const grace::PeriodicBox box = { 1.0f, 0.5f, 0.0f };\n"
                   "    grace::device_vector<float> grad(p.size() * 9), value(p.size() * 3), div(p.size()), curl(p.size() * 3);\n"
                   "    grace::device_vector<int> counts(p.size());\n"
                   "    grace::interpolate_gradient_sph(p, s, t, w, 3, grad);\n"
                   "    grace::interpolate_gradient_sph(p, s, t, w, 3, grad, &value, &counts);\n"
                   "    grace::interpolate_gradient_sph(p, s, t, w, 3, grad, &value, &counts, box);\n"
                   "    grace::device_vector<float> g(8 * 8 * 3 * 3), gv(8 * 8 * 3);\n"
                   "    const grace::float3 o = grace::make_float3(0, 0, 0), u = grace::make_float3(1, 0, 0),\n"
                   "                        v = grace::make_float3(0, 1, 0), z = grace::make_float3(0, 0, 1);\n"
                   "    grace::interpolate_gradient_grid_sph(o, u, v, z, 8, 8, 1, s, t, w, 3, g);\n"
                   "    grace::interpolate_gradient_grid_sph(o, u, v, z, 8, 8, 1, s, t, w, 3, g, &gv, box);\n"
                   "    grace::divergence_curl_sph(p, s, t, w, div, curl);\n"
                   "    grace::divergence_curl_sph(p, s, t, w, div, curl, box);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


@pytest.mark.parametrize("kernel", KERNELS)
def test_fp32_derivative_forms_agree_with_the_analytic_fp64_derivatives(kernel):
    q = np.linspace(0.0, 1.0, 200001).astype(F32)
    got = df32_kernel(kernel, q).astype(F64)
    ref = df64_kernel(kernel, q.astype(F64))
    err = np.abs(got - ref)
    margin = df_margin(kernel, q.astype(F64)) + 1e-45              # (the smallest fp32 subnormal: u^7 near q = 1)
    assert np.all(err <= margin), (kernel, float(np.max(err / margin)), float(q[np.argmax(err / margin)]))
    assert got[-1] == 0.0 and np.all(got <= np.maximum(margin, 0.0))   # f' <= 0 to rounding
    # and the analytic derivative is the derivative of the table functions
    h = 1e-6
    qq = np.linspace(0.01, 0.99, 9801)
    cd = (f64_kernel(kernel, qq + h) - f64_kernel(kernel, qq - h)) / (2 * h)
    # central differences: h^2 / 6 |f'''| with |f'''| below 1e4 for these kernels, and fp64 rounding
    # 2^-52 |f| / h with |f| below 10: both far below 1e-6 of max |f'|
    assert np.max(np.abs(cd - df64_kernel(kernel, qq))) < 1e-6 * np.max(np.abs(df64_kernel(kernel, qq)))


def _one_sphere_fp64(p, x, H, kernel):
    """(field, gradient) of one sphere of weight 1 at points p in fp64."""
    d = p - x
    r = np.sqrt((d * d).sum(axis=1))
    A = f64_kernel(kernel, r / H) / H ** 3
    g = (df64_kernel(kernel, r / H) / H ** 4)[:, None] * d / r[:, None]
    return A, g


@pytest.mark.parametrize("kernel", KERNELS)
def test_central_differences_of_the_fp64_field_equal_the_fp64_gradient(kernel):
    rng = np.random.default_rng(5)
    x, H = np.array([0.3, -0.2, 0.5]), 0.7
    dirs = rng.normal(size=(400, 3)); dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    p = x + dirs * (rng.uniform(0.02, 1.05, 400) * H)[:, None]     # inside and just outside the support
    _, g = _one_sphere_fp64(p, x, H, kernel)
    h = 1e-5 * H
    scale = np.max(np.abs(df64_kernel(kernel, np.linspace(0, 1, 1001)))) / H ** 4
    for k in range(3):
        e = np.zeros(3); e[k] = h
        cd = (_one_sphere_fp64(p + e, x, H, kernel)[0] - _one_sphere_fp64(p - e, x, H, kernel)[0]) / (2 * h)
        # truncation (1e-5)^2 / 6 |f'''| / |f'| ~ 1e-8 (at a knot of the cubic, where f''' jumps, the same
        # order), rounding 2^-52 |f| / (1e-5 |f'|) ~ 1e-10
        assert np.max(np.abs(cd - g[:, k])) < 1e-6 * scale, (kernel, k)


@pytest.mark.parametrize("kernel", KERNELS)
def test_restated_gradient_of_one_sphere_sums_to_zero_over_a_grid(kernel):
    n = 32
    h = 2.0 / n                                                    # exact in binary: the lattice is symmetric
    o = -1.0 + h / 2
    pts = lattice((o, o, o), (h, 0, 0), (0, h, 0), (0, 0, h), (n, n, n))
    assert np.array_equal(np.sort(pts[:, 0]), np.sort(-pts[:, 0]))
    s = np.array([[0.0, 0.0, 0.0, 0.9]], F32)
    pr = pairs(pts, s, chunk=1 << 16)
    g32, g64, _ = restate_gradient(pts, pr, s, np.ones((1, 1), F32), kernel)
    total = np.abs(g32[:, 0, :].astype(F64).sum(axis=0))
    # mirrored points have exactly negated terms; what is left is the fp64 summation's rounding
    assert np.all(total <= len(pts) * 2.0 ** -52 * np.abs(g32).astype(F64).sum()), (kernel, total)
    assert np.abs(g32).max() > 0 and np.max(np.abs(g32 - g64)) < 1e-5 * np.abs(g64).max()
    # the gradient points inward: the kernels decrease with q
    inside = np.bincount(pr[0], minlength=len(pts)) > 0
    assert np.all((g32[inside, 0, :] * pts[inside]).sum(axis=1) <= 0)


# ---- GPU --------------------------------------------------------------------------------------------
N_BASE = 400
SURFACE = np.array([0.5, 0.25, 0.75, 0.125], F32)                  # binary-exact: points exactly on its surface


def _scene(name):
    s = T._random_scene() if name == "random" else T._clustered_scene()
    s[50] = SURFACE
    return s


def _base_points(sh, seed):
    """N_BASE points: a sphere's centre, a surface point, a NaN point, then points near centres and uniform."""
    rng = np.random.default_rng(seed)
    near = sh[rng.choice(len(sh), 250, replace=False)]
    near = near[:, :3] + (rng.random((250, 3), dtype=F32) - F32(0.5)) * near[:, 3:4]
    pts = np.concatenate([
        sh[7:8, :3],
        np.array([[0.625, 0.25, 0.75]], F32),
        np.array([[np.nan, 0.5, 0.5]], F32),
        near,
        rng.random((N_BASE - 253, 3), dtype=F32) * F32(1.1) - F32(0.05),
    ]).astype(F32)
    return pts


@pytest.fixture(scope="module")
def scenes(gh, cuda):
    res = {}
    for name in ("random", "clustered"):
        d, tree = T._build(gh, _scene(name), cuda)
        sh = d.cpu().numpy()
        pts = _base_points(sh, 17)
        res[name] = (d, tree, sh, pts, pairs(pts, sh))
    return res


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")
    gh.interpolate_gradient_channels_per_walk(0)


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _grad(gh, pts, d, tree, w, cuda, period=None):
    """The GPU's (grad [n, C, 3], value [n, C], counts [n]) at points, outputs prefilled with a marker."""
    import torch
    n, C_ = len(pts), w.shape[1]
    grad = torch.full((n, C_, 3), 7.0, dtype=torch.float32, device=cuda)
    value = torch.full((n, C_), 7.0, dtype=torch.float32, device=cuda)
    counts = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    gh.interpolate_gradient_sph(_dev(np.asarray(pts, F32), cuda), d, tree, _dev(w, cuda), grad=grad, value=value,
                                counts=counts, check=True, period=period)
    return grad.cpu().numpy(), value.cpu().numpy(), counts.cpu().numpy()


def _field(gh, pts, d, tree, w, cuda, period=None):
    import torch
    counts = torch.empty(len(pts), dtype=torch.int32, device=cuda)
    out, counts = gh.interpolate_sph(_dev(np.asarray(pts, F32), cuda), d, tree, _dev(w, cuda), counts=counts,
                                     check=True, period=period)
    return out.cpu().numpy().reshape(len(pts), -1), counts.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("scene", ["random", "clustered"])
def test_gradient_is_the_restatement_bit_for_bit(gh, scenes, scene, kernel, cuda, kernel_reset):
    d, tree, sh, pts, pr = scenes[scene]
    gh.set_sph_kernel(kernel)
    w = T._weights(len(sh), 3, 71)
    ref32, ref64, bound = restate_gradient(pts, pr, sh, w, kernel)
    ref_counts = np.bincount(pr[0], minlength=len(pts))
    for n in (1, 63, 64, 65, len(pts)):
        grad, value, counts = _grad(gh, pts[:n], d, tree, w, cuda)
        bad = np.nonzero(_bits(grad) != _bits(ref32[:n]))
        assert len(bad[0]) == 0, (n, bad[0][:5], grad[bad][:5], ref32[:n][bad][:5])
        assert np.array_equal(counts, ref_counts[:n]), n
        f_out, f_counts = _field(gh, pts[:n], d, tree, w, cuda)
        assert _same(value, f_out) and np.array_equal(counts, f_counts), n
    err = np.abs(grad - ref64)
    print(kernel, scene, "max |gpu - fp64| / bound:", float(np.max(err / (bound + 1e-30))))
    assert np.all(err <= bound + 1e-30), (kernel, scene, float(np.max(err / (bound + 1e-30))))
    # the centre: +0 from its own sphere, finite, counted; the surface point: not contained; NaN: zeros
    own = (pr[0] == 0) & (pr[1] == 7)
    assert own.sum() == 1 and pr[2][own][0] == 0 and np.all(np.isfinite(grad[0]))
    k = int(np.nonzero(np.all(sh == SURFACE, axis=1))[0][0])
    assert not np.any((pr[0] == 1) & (pr[1] == k))
    assert counts[2] == 0 and np.all(_bits(grad[2]) == 0) and np.all(_bits(value[2]) == 0)
    assert np.abs(ref32).max() > 0


@pytest.mark.gpu
def test_a_lone_sphere_gives_its_centre_plus_zero(gh, cuda):
    s = np.array([[0.5, 0.5, 0.5, 0.25], [0.1, 0.1, 0.1, 0.01]], F32)
    d, tree, sh = build_small(gh, s, cuda, 1)                        # (max_per_leaf 1: a tree needs a node)
    pts = np.array([[0.5, 0.5, 0.5], [0.75, 0.5, 0.5], [0.5, 0.5, 0.625]], F32)
    w = np.where(sh[:, 3:4] == F32(0.25), F32(-3), F32(2)).astype(F32)
    grad, value, counts = _grad(gh, pts, d, tree, w, cuda)
    assert list(counts) == [1, 0, 1]
    assert np.all(_bits(grad[0]) == 0) and value[0, 0] != 0         # +0, not -0 or NaN
    assert np.all(_bits(grad[1]) == 0)
    assert grad[2, 0, 2] != 0 and grad[2, 0, 0] == 0 and grad[2, 0, 1] == 0


@pytest.mark.gpu
def test_channels_are_independent_of_their_call_and_walk(gh, scenes, cuda, kernel_reset):
    d, tree, sh, pts, pr = scenes["clustered"]
    w = T._weights(len(sh), 64, 73)
    p = pts[:130]
    default = gh.interpolate_gradient_channels_per_walk(0)
    assert default in (1, 2)
    g64, v64, c64 = _grad(gh, p, d, tree, w, cuda)
    ref32, _, _ = restate_gradient(p, pairs(p, sh), sh, w[:, 62:], "cubic")
    assert _same(g64[:, 62:], ref32)
    for per_walk in (1, 2):
        assert gh.interpolate_gradient_channels_per_walk(per_walk) == per_walk
        for n_ch in sorted({1, per_walk, per_walk + 1, 64}):
            g, v, c = _grad(gh, p, d, tree, w[:, :n_ch], cuda)
            assert _same(g, g64[:, :n_ch]) and _same(v, v64[:, :n_ch]) and np.array_equal(c, c64), (per_walk, n_ch)
    assert gh.interpolate_gradient_channels_per_walk(3) == 2       # out of range: unchanged
    assert gh.interpolate_gradient_channels_per_walk(0) == default


@pytest.mark.gpu
def test_results_do_not_depend_on_entry_point_order_or_layout(gh, scenes, cuda):
    import torch
    d, tree, sh, _, _ = scenes["clustered"]
    w = T._weights(len(sh), 2, 31)
    th = 0.3
    for spec in (((0.05, 0.1, 0.2), (np.cos(th) / 50, 0.0, np.sin(th) / 50), (0.0, 1 / 47, 0.003), (0, 0, 1), (50, 47, 1)),
                 ((0.2, 0.2, 0.2), (1 / 40, 0, 0), (0, 1 / 40, 0), (0, 0, 1 / 40), (13, 9, 6))):
        o, u, v, ww, dims = spec
        pts = lattice(*spec)
        g_grid, v_grid, c_grid = gh.interpolate_gradient_grid_sph(
            o, u, v, ww, dims, d, tree, _dev(w, cuda), value=torch.empty((dims[2], dims[1], dims[0], 2), device=cuda),
            counts=torch.empty((dims[2], dims[1], dims[0]), dtype=torch.int32, device=cuda), check=True)
        assert tuple(g_grid.shape) == (dims[2], dims[1], dims[0], 2, 3)
        grad, value, counts = _grad(gh, pts, d, tree, w, cuda)
        assert _same(g_grid.cpu().numpy().reshape(-1, 2, 3), grad)
        assert _same(v_grid.cpu().numpy().reshape(-1, 2), value)
        assert np.array_equal(c_grid.cpu().numpy().reshape(-1), counts)
        assert np.abs(grad).max() > 0
    perm = np.random.default_rng(1).permutation(len(pts))
    g_sh, v_sh, c_sh = _grad(gh, pts[perm], d, tree, w, cuda)
    assert _same(g_sh, grad[perm]) and _same(v_sh, value[perm]) and np.array_equal(c_sh, counts[perm])
    wide = np.full((len(pts), 7), 123.0, F32); wide[:, :3] = pts
    g7, v7, c7 = _grad(gh, wide, d, tree, w, cuda)                   # elems_per_point 7 against 3
    assert _same(g7, grad) and _same(v7, value) and np.array_equal(c7, counts)
    for auto, valid in ((False, True), (True, False)):               # the cache knobs of the trace
        gh.set_cache_auto(auto); gh.set_cache_validation(valid)
        try:
            g, _, _ = _grad(gh, pts, d, tree, w, cuda)
        finally:
            gh.set_cache_auto(True); gh.set_cache_validation(True)
        assert _same(g, grad)
    # without the optional outputs
    only = gh.interpolate_gradient_sph(_dev(pts, cuda), d, tree, _dev(w, cuda), check=True)
    assert only[1] is None and only[2] is None and _same(only[0].cpu().numpy(), grad)
    # one channel as a vector of weights: [n, 3]
    g1 = gh.interpolate_gradient_sph(_dev(pts, cuda), d, tree, _dev(w[:, 1].copy(), cuda), check=True)[0]
    assert tuple(g1.shape) == (len(pts), 3) and _same(g1.cpu().numpy(), grad[:, 1])
    # zero points
    g0 = gh.interpolate_gradient_sph(torch.empty((0, 3), dtype=torch.float32, device=cuda), d, tree, _dev(w, cuda),
                                     check=True)[0]
    assert tuple(g0.shape) == (0, 2, 3)


@pytest.mark.gpu
def test_interleaved_traces_and_fields_change_nothing(gh, scenes, cuda):
    import torch
    d, tree, sh, pts, _ = scenes["random"]
    rays = gh.orthogonal_rays_z(64, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    w = T._weights(len(sh), 2, 5)

    def trace():
        out = torch.empty(len(rays), dtype=torch.float32, device=cuda)
        gh.trace_cumulative_sph(rays, d, tree, out, check=True)
        return out.cpu().numpy()

    t0, f0, g0 = trace(), _field(gh, pts, d, tree, w, cuda), _grad(gh, pts, d, tree, w, cuda)
    for _ in range(2):
        g = _grad(gh, pts, d, tree, w, cuda)
        t = trace()
        f = _field(gh, pts, d, tree, w, cuda)
        assert _same(t, t0) and _same(f[0], f0[0]) and np.array_equal(f[1], f0[1])
        assert _same(g[0], g0[0]) and _same(g[1], g0[1]) and np.array_equal(g[2], g0[2])


@pytest.mark.gpu
def test_refusals_write_nothing(gh, scenes, cuda, kernel_reset):
    import torch
    d, tree, sh, _, _ = scenes["random"]
    n = len(sh)
    pts = torch.rand((100, 4), dtype=torch.float32, device=cuda)
    w = torch.ones((n, 2), dtype=torch.float32, device=cuda)
    grad = torch.full((100, 2, 3), 7.0, dtype=torch.float32, device=cuda)
    value = torch.full((100, 2), 7.0, dtype=torch.float32, device=cuda)
    cnt = torch.full((100,), 7, dtype=torch.int32, device=cuda)
    scene = gh._interp_scene(d, tree)
    lib = gh._lib

    def call(elems=4, wp=w, n_ch=2, gp=grad):
        return lib.grace_interpolate_gradient_points_f4(gh._ptr(pts), C.c_size_t(100), C.c_int(elems), *scene,
                                                        gh._ptr(wp), C.c_int(n_ch), gh._ptr(gp), gh._ptr(value),
                                                        gh._ptr(cnt), gh._stream())

    for kw in (dict(elems=2), dict(n_ch=0), dict(n_ch=65), dict(wp=None), dict(gp=None)):
        assert call(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    o3 = (C.c_float * 3)(0, 0, 0); uvw = (C.c_float * 9)(0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1)
    for n_ch, gp, dims in ((0, grad, (5, 5, 4)), (65, grad, (5, 5, 4)), (2, None, (5, 5, 4)), (2, grad, (5, 0, 4))):
        st = lib.grace_interpolate_gradient_grid_f4(o3, uvw, (C.c_int * 3)(*dims), *scene, gh._ptr(w), C.c_int(n_ch),
                                                    gh._ptr(gp), gh._ptr(value), gh._ptr(cnt), gh._stream())
        assert st == gh.GRACE_INVALID_ARGUMENT, (n_ch, dims)
    assert lib.grace_gradient_div_curl_f32(gh._ptr(grad), C.c_size_t(10), None, None, gh._stream()) \
        == gh.GRACE_INVALID_ARGUMENT
    gh.set_sph_kernel(gh.sph_kernel_table("quartic"))               # a custom table: no f'(q)
    assert call() == gh.GRACE_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        gh.interpolate_gradient_sph(pts, d, tree, w)
    torch.cuda.synchronize()
    assert torch.all(grad == 7.0) and torch.all(value == 7.0) and torch.all(cnt == 7)
    gh.set_sph_kernel("cubic")
    assert call() == gh.GRACE_OK
    gh.trace_status()
    assert not torch.any(grad == 7.0)
    for bad in (None, torch.ones(n - 1, dtype=torch.float32, device=cuda),
                torch.ones((n, 65), dtype=torch.float32, device=cuda)):
        with pytest.raises(ValueError):
            gh.interpolate_gradient_sph(pts, d, tree, bad)
    with pytest.raises(ValueError):
        gh.interpolate_gradient_sph(pts, d, tree, w, grad=torch.empty((100, 2), dtype=torch.float32, device=cuda))


@pytest.mark.gpu
def test_deep_clustered_tree_fits_the_stack(gh, cuda):
    rng = np.random.default_rng(9)                                  # test_sph_interpolation's scene of that name
    n = 30000
    s = np.empty((n, 4), F32)
    scale = 0.4 * 0.1 ** (rng.integers(0, 5, n))
    s[:, :3] = (0.5 + scale[:, None] * (rng.random((n, 3)) - 0.5)).astype(F32)
    s[:, 3] = (scale * (0.05 + 0.1 * rng.random(n))).astype(F32) + F32(1e-7)
    d, tree = T._build(gh, s, cuda)
    sh = d.cpu().numpy()
    pts = (0.5 + (rng.random((500, 3)) - 0.5) * 0.4 * 0.1 ** rng.integers(0, 5, (500, 1))).astype(F32)
    w = T._weights(n, 1, 3)
    grad, value, counts = _grad(gh, pts, d, tree, w, cuda)
    gh.trace_status()                                               # GRACE_OK: no packet ran out of stack
    pr = pairs(pts, sh)
    assert _same(grad, restate_gradient(pts, pr, sh, w, "cubic")[0])
    assert np.array_equal(counts, np.bincount(pr[0], minlength=len(pts)))


@pytest.mark.gpu
def test_divergence_and_curl_are_the_stated_combinations(gh, scenes, cuda):
    d, tree, sh, pts, _ = scenes["random"]
    vec = T._weights(len(sh), 3, 91)
    g = _grad(gh, pts, d, tree, vec, cuda)[0]
    div, curl = gh.divergence_curl_sph(_dev(pts, cuda), d, tree, _dev(vec, cuda))
    div, curl = div.cpu().numpy(), curl.cpu().numpy()
    assert _same(div, ((g[:, 0, 0] + g[:, 1, 1]).astype(F32) + g[:, 2, 2]).astype(F32))
    ref = np.stack([g[:, 2, 1] - g[:, 1, 2], g[:, 0, 2] - g[:, 2, 0], g[:, 1, 0] - g[:, 0, 1]], axis=1).astype(F32)
    assert _same(curl, ref)
    assert np.abs(div).max() > 0 and np.abs(curl).max() > 0
    # either output alone
    import torch
    only = torch.full((len(pts),), 7.0, dtype=torch.float32, device=cuda)
    assert gh._lib.grace_gradient_div_curl_f32(gh._ptr(_dev(g, cuda)), C.c_size_t(len(pts)), gh._ptr(only), None,
                                               gh._stream()) == gh.GRACE_OK
    assert _same(only.cpu().numpy(), div)


@pytest.mark.gpu
@pytest.mark.parametrize("mirror", [False, True])
def test_gradient_dropin_program_matches_ctypes(gh, cuda, tmp_path, mirror):
    d, tree = T._build(gh, T._random_scene(6000, 41, 0.02, 0.06), cuda)
    s = d.cpu().numpy()                                             # tree order
    pts = np.random.default_rng(3).random((333, 4), dtype=F32)
    w = T._weights(len(s), 4, 43)
    s.tofile(str(tmp_path / "s.f32")); pts.tofile(str(tmp_path / "p.f32")); w.tofile(str(tmp_path / "w.f32"))
    exe = str(tmp_path / "dropin_gradient")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, *(["-DDROPIN_MIRROR"] if mirror else []),
                           os.path.join(ROOT, "tests", "cpp", "dropin_gradient.hip"), "-o", exe,
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    period = (1.0, 0.5, 0.0)
    n_grid = 9
    res = subprocess.run([exe, str(tmp_path / "s.f32"), str(tmp_path / "p.f32"), str(tmp_path / "w.f32"), "4",
                          str(n_grid), *(str(L) for L in period)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in res.stdout.splitlines()}
    ref = {}
    ref["grad"], ref["value"], ref["counts"] = _grad(gh, pts, d, tree, w, cuda)
    ref["periodic_grad"], ref["periodic_value"], ref["periodic_counts"] = _grad(gh, pts, d, tree, w, cuda, period)
    h = float(F32(1) / F32(n_grid))                                  # the program's 1.0f / float(n_grid)
    grid = ((0, 0, 0), (h, 0, 0), (0, h, 0), (0, 0, h), (n_grid,) * 3)
    import torch
    gg, gv, _ = gh.interpolate_gradient_grid_sph(*grid, d, tree, _dev(w, cuda), check=True,
                                                 value=torch.empty((n_grid,) * 3 + (4,), device=cuda))
    ref["grid_grad"], ref["grid_value"] = gg.cpu().numpy(), gv.cpu().numpy()
    ref["periodic_grid_grad"] = gh.interpolate_gradient_grid_sph(*grid, d, tree, _dev(w, cuda), check=True,
                                                                 period=period)[0].cpu().numpy()
    vec = _dev(w[:, :3].copy(), cuda)
    for name, per in (("", None), ("periodic_", period)):
        dv, cl = gh.divergence_curl_sph(_dev(pts, cuda), d, tree, vec, period=per)
        ref[name + "div"], ref[name + "curl"] = dv.cpu().numpy(), cl.cpu().numpy()
    assert set(got) == set(ref)
    for name, a in ref.items():
        assert got[name] == digest(a), name
    assert np.abs(ref["periodic_grad"] - ref["grad"]).max() > 0
