"""Selectable SPH kernels (grace_trace_set_sph_kernel*, set_sph_kernel): every integrating trace adds
lerp(F, 50 sqrt(b^2) / H) / H^2 with the selected kernel's 51-entry table F, in every mode, with the
same operations as the default cubic spline.

Expected values restate the per-hit integral in NumPy from b^2: fp32 sphere_hit without FMA (the
oracle's arithmetic), then the reference lerp with the kernel's table.  The restatement is checked
first against the oracle's own per-hit integrals with the cubic table, bit for bit.  Hit sets do not
depend on the kernel, so oracle.brute_hits supplies offsets and indices.  The fp64 lerp's fma is
evaluated exactly (fractions.Fraction) where the double result is the output; for fp32 outputs it is
evaluated in extended precision and rounded to double, then float."""
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
PI = math.pi

KERNELS = ("cubic", "quartic", "quintic", "wendland_c2", "wendland_c4", "wendland_c6")
F0 = {"cubic": 6 / PI, "quartic": 15 / (2 * PI), "quintic": 9 / PI, "wendland_c2": 7 / PI,
      "wendland_c4": 55 / (6 * PI), "wendland_c6": 91 / (8 * PI)}
# volume of the 51-point lerp of each table, minus one (part of the contract: tables not renormalised)
LERP_BIAS = {"cubic": 3.97e-4, "quartic": 5.00e-4, "quintic": 6.00e-4, "wendland_c2": 4.67e-4,
             "wendland_c4": 6.11e-4, "wendland_c6": 7.58e-4}


# ---- independent definitions of the kernels ---------------------------------------------------------
def _p(x):
    return np.maximum(x, 0.0)


F_OF_Q = {
    "quartic": (lambda q: 25 / (32 * PI) * (_p(2.5 - 2.5 * q) ** 4 - 5 * _p(1.5 - 2.5 * q) ** 4
                                            + 10 * _p(0.5 - 2.5 * q) ** 4), (0.2, 0.6)),
    "quintic": (lambda q: 9 / (40 * PI) * (_p(3 - 3 * q) ** 5 - 6 * _p(2 - 3 * q) ** 5
                                           + 15 * _p(1 - 3 * q) ** 5), (1 / 3, 2 / 3)),
    "wendland_c2": (lambda q: 21 / (2 * PI) * _p(1 - q) ** 4 * (1 + 4 * q), ()),
    "wendland_c4": (lambda q: 495 / (32 * PI) * _p(1 - q) ** 6 * (1 + 6 * q + 35 / 3 * q * q), ()),
    "wendland_c6": (lambda q: 1365 / (64 * PI) * _p(1 - q) ** 8 * (1 + 8 * q + 25 * q * q + 32 * q ** 3), ()),
}


def chord_panels(f, breaks, b, nodes=30):
    """2 int_0^sqrt(1-b^2) f(sqrt(b^2 + z^2)) dz on panels in z: split at the breakpoints and graded
    geometrically from z = b (the integrand's branch points sit at z = +-i b)."""
    x, w = np.polynomial.legendre.leggauss(nodes)
    zmax = math.sqrt(max(1 - b * b, 0.0))
    pts = {0.0, zmax} | {math.sqrt(q * q - b * b) for q in breaks if q > b}
    z = b
    while 0 < z < zmax:
        pts.add(z)
        z *= 1.5
    pts = sorted(pts)
    total = 0.0
    for a, c in zip(pts[:-1], pts[1:]):
        zz = 0.5 * (c - a) * x + 0.5 * (c + a)
        total += 0.5 * (c - a) * float(np.dot(w, f(np.sqrt(b * b + zz * zz))))
    return 2 * total


def lerp_volume(F):
    """2 pi int_0^1 b lerp(F)(b) db, exactly for the piecewise-linear lerp."""
    F = np.asarray(F, F64)
    d = 1 / 50
    v = 0.0
    for i in range(50):
        bi = i * d
        s = (F[i + 1] - F[i]) / d
        v += 2 * PI * (F[i] * (bi * d + d * d / 2) + s * (bi * d * d / 2 + d ** 3 / 3))
    return v


# ---- the restatement -----------------------------------------------------------------------------------
def hit_rays(offsets, n_hits):
    return np.repeat(np.arange(len(offsets)), np.diff(np.append(offsets, n_hits)))


def b2_f32(rays, s, ray, idx):
    """sphere_hit's b^2 in fp32, without FMA (generic/intersect.h; the oracle's arithmetic)."""
    r, sp = rays[ray], s[idx]
    p = [(sp[:, k] - r[:, 3 + k]).astype(F32) for k in range(3)]
    d = [r[:, k] for k in range(3)]
    dot = ((p[0] * d[0]).astype(F32) + (p[1] * d[1]).astype(F32)).astype(F32)
    dot = (dot + (p[2] * d[2]).astype(F32)).astype(F32)
    b = [(p[k] - (dot * d[k]).astype(F32)).astype(F32) for k in range(3)]
    b2 = ((b[0] * b[0]).astype(F32) + (b[1] * b[1]).astype(F32)).astype(F32)
    return (b2 + (b[2] * b[2]).astype(F32)).astype(F32)


def integrals_f32(b2, h, table):
    """OnHit_sphere_individual / _cumulate with Real = float: ir = 1/h, x = 50 (sqrt(b2) ir),
    lerp<double> over the table (fma in double, rounded to float), times ir^2."""
    ir = (F32(1) / h.astype(F32)).astype(F32)
    x = (F32(50) * (np.sqrt(b2.astype(F32)) * ir).astype(F32)).astype(F32)
    i = x.astype(np.int64)
    over = i >= 50
    x = np.where(over, F32(50), x)
    i = np.where(over, 49, i)
    t = x.astype(np.longdouble) - i
    y0 = table[i].astype(np.longdouble)
    dy = (table[i + 1] - table[i]).astype(np.longdouble)
    y = (t * dy + y0).astype(F64).astype(F32)
    return (y * (ir * ir).astype(F32)).astype(F32)


def _fma(t, dy, y0):
    """fma in double, exactly: one rounding of t * dy + y0."""
    return float(Fraction(float(t)) * Fraction(float(dy)) + Fraction(float(y0)))


def integral_f64(b2, ir, table):
    """lerp<double> in double from a double b^2 and ir (the mixed and double4 per-hit outputs)."""
    x = 50 * (math.sqrt(b2) * ir)
    i = int(x)
    if i >= 50:
        x, i = 50.0, 49
    return _fma(x - i, table[i + 1] - table[i], table[i]) * (ir * ir)


def class_sums(n_rays, offsets, idx, terms, dtype):
    """The class-ordered sum: class (p >> 10) & 7 in ascending index order, the 8 classes pairwise."""
    n_hits = len(idx)
    ray = hit_rays(offsets, n_hits)
    cls = (idx >> 10) & 7
    order = np.lexsort((idx, cls, ray))
    ray, cls, terms = ray[order], cls[order], terms[order]
    group = ray * 8 + cls
    start = np.searchsorted(group, group, side="left")
    rank = np.arange(n_hits) - start
    width = int(rank.max()) + 1 if n_hits else 1
    m = np.zeros((n_rays * 8, width), dtype)
    m[group, rank] = terms
    acc = np.zeros(n_rays * 8, dtype)
    for j in range(width):
        acc = (acc + m[:, j]).astype(dtype)
    t = acc.reshape(n_rays, 8)
    step = 1
    while step < 8:
        for k in range(0, 8, 2 * step):
            t[:, k] = (t[:, k] + t[:, k + step]).astype(dtype)
        step *= 2
    return t[:, 0].copy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


# ---- CPU ----------------------------------------------------------------------------------------------
def test_sph_kernel_symbols_exported():
    import ctypes
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    for name in ("grace_trace_set_sph_kernel", "grace_trace_set_sph_kernel_table", "grace_trace_get_sph_kernel",
                 "grace_sph_kernel_table"):
        assert hasattr(lib, name), name


def test_cubic_table_is_the_reference_table(gh, oracle):
    assert gh.SPH_KERNELS == KERNELS
    assert np.array_equal(_bits(gh.sph_kernel_table("cubic")), _bits(np.asarray(oracle.kernel_table(), F64)))


@pytest.mark.parametrize("name", KERNELS[1:])
def test_builtin_tables_are_the_chord_integrals(gh, name):
    t = gh.sph_kernel_table(name)
    assert t.dtype == F64 and t.shape == (51,)
    f, breaks = F_OF_Q[name]
    ref = np.array([chord_panels(f, breaks, i / 50) for i in range(51)])
    assert np.max(np.abs(t - ref)) < 1e-12, (name, np.max(np.abs(t - ref)))
    assert abs(t[0] - F0[name]) < 1e-12
    assert t[50] == 0.0 and np.all(t >= 0)


@pytest.mark.parametrize("name", KERNELS)
def test_lerp_volume_bias_is_the_stated_one(gh, name):
    assert abs(lerp_volume(gh.sph_kernel_table(name)) - 1 - LERP_BIAS[name]) < 1e-6


def test_bad_kernel_names_are_refused(gh):
    with pytest.raises(ValueError):
        gh.sph_kernel_table("gaussian")
    with pytest.raises(ValueError):
        gh.sph_kernel_table("custom")


def test_generated_header_is_up_to_date():
    script = os.path.join(ROOT, "grace-devel_amd", "tools", "gen_kernel_tables.py")
    res = subprocess.run(["python3", script, "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_sph_kernel_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_sph_kernels"
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_sph_kernels.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


def test_sph_kernel_mirror_compiles_with_gxx(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "int main()\n"
                   "{\n"
                   "    std::array<double, 51> t = grace::sph_kernel_table(grace::SphKernel::wendland_c4);\n"
                   "    if (t[50] != 0.0) return 1;\n"
                   "    grace::set_sph_kernel(grace::SphKernel::quintic);\n"
                   "    grace::set_sph_kernel_table(std::vector<double>(t.begin(), t.end()));\n"
                   "    return 0;\n"
                   "}\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


# ---- GPU ----------------------------------------------------------------------------------------------
N_SCENE = 20000   # > 8192: all eight summation classes hold spheres


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")
    gh.set_exact_integrals(False)


def _custom():
    """A caller's table: Wendland C2 scaled by 0.75 with a distorted tail (not a built-in)."""
    import grace_hip as gh
    t = gh.sph_kernel_table("wendland_c2") * 0.75
    t[40:50] *= np.linspace(1.0, 0.5, 10)
    return t


ALL = KERNELS + ("custom",)


def _table(gh, name):
    return _custom() if name == "custom" else gh.sph_kernel_table(name)


def _select(gh, name):
    gh.set_sph_kernel(_custom() if name == "custom" else name)


@pytest.fixture(scope="module")
def scene(gh, oracle, cuda):
    import torch
    rng = np.random.default_rng(3)
    s = np.empty((N_SCENE, 4), F32)
    s[:, :3] = rng.random((N_SCENE, 3), dtype=F32)
    s[:, 3] = (0.01 + 0.04 * rng.random(N_SCENE)).astype(F32)
    d = torch.from_numpy(s).to(cuda)
    tree = gh.Tree(N_SCENE, 32, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))     # sorts d
    sh = d.cpu().numpy()
    sets = {
        "orthographic": gh.orthogonal_rays_z(48, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0],
        "pinhole": gh.pinhole_camera_rays(48, 48, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0,
                                          device=cuda),
        "isotropic": gh.uniform_random_rays(2048, (0.5, 0.5, 0.5), 1.0, device=cuda),
    }
    out = {}
    for name, rays in sets.items():
        rh = rays.cpu().numpy()
        off, idx, integ, _ = oracle.brute_hits(rh, sh)
        assert len(idx) > 0
        b2 = b2_f32(rh, sh, hit_rays(off, len(idx)), idx)
        out[name] = (rays, off, idx, integ, b2)
    return d, tree, sh, out


def _cumulative(gh, rays, d, tree, dtype=None):
    import torch
    out = torch.empty(len(rays), dtype=dtype or torch.float32, device=rays.device)
    gh.trace_cumulative_sph(rays, d, tree, out, check=True)
    return out.cpu().numpy()


@pytest.mark.gpu
def test_restatement_reproduces_the_oracle_with_the_cubic_table(gh, scene):
    d, tree, sh, sets = scene
    table = gh.sph_kernel_table("cubic")
    for name, (rays, off, idx, integ, b2) in sets.items():
        mine = integrals_f32(b2, sh[idx, 3], table)
        assert np.array_equal(_bits(mine), _bits(integ)), name


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ALL)
def test_exact_column_densities_are_the_restated_sum(gh, scene, kernel, kernel_reset):
    d, tree, sh, sets = scene
    table = _table(gh, kernel)
    _select(gh, kernel)
    gh.set_exact_integrals(True)
    for name, (rays, off, idx, integ, b2) in sets.items():
        terms = integrals_f32(b2, sh[idx, 3], table)
        ref = class_sums(len(rays), off, idx, terms, F32)
        got = _cumulative(gh, rays, d, tree)
        assert np.array_equal(_bits(got), _bits(ref)), (kernel, name)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ALL)
def test_fast_column_densities_within_tolerance(gh, scene, kernel, kernel_reset):
    d, tree, sh, sets = scene
    table = _table(gh, kernel)
    _select(gh, kernel)
    h_min = float(sh[:, 3].min())
    atol = 2e-6 * table[0] / h_min ** 2                # check_column_densities' max_term allowance
    for name, (rays, off, idx, integ, b2) in sets.items():
        terms = integrals_f32(b2, sh[idx, 3], table).astype(F64)
        ray = hit_rays(off, len(idx))
        ref = np.zeros(len(rays)); np.add.at(ref, ray, terms)
        got = _cumulative(gh, rays, d, tree).astype(F64)
        bad = np.nonzero(np.abs(got - ref) > 1e-5 * ref + atol)[0]   # terms >= 0: sum |terms| = ref
        assert len(bad) == 0, (kernel, name, bad[:5], got[bad[:5]], ref[bad[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ALL)
def test_per_hit_integrals_follow_the_kernel(gh, scene, kernel, kernel_reset):
    import torch
    d, tree, sh, sets = scene
    table = _table(gh, kernel)
    _select(gh, kernel)
    for name, (rays, off, idx, integ, b2) in sets.items():
        o, i, w, _ = gh.trace_sph(rays, d, tree)
        assert np.array_equal(o.cpu().numpy(), off) and np.array_equal(i.cpu().numpy(), idx), (kernel, name)
        ref = integrals_f32(b2, sh[idx, 3], table)
        assert np.array_equal(_bits(w.cpu().numpy()), _bits(ref)), (kernel, name)
        # with sentinels: the same integrals, one sentinel slot per ray
        o2, i2, w2, _ = gh.trace_with_sentinels_sph(rays, d, tree, -1, -1.0, -1.0)
        keep = i2.cpu().numpy() != -1
        assert np.array_equal(_bits(w2.cpu().numpy()[keep]), _bits(ref)), (kernel, name)
    # hit_integrals on arrays: the same arithmetic
    rays, off, idx, integ, b2 = sets["pinhole"]
    got = gh.hit_integrals(torch.from_numpy(b2).to(d.device), torch.from_numpy(sh[idx, 3].copy()).to(d.device))
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(integrals_f32(b2, sh[idx, 3], table))), kernel


@pytest.fixture(scope="module")
def small_rays(gh, cuda):
    return gh.pinhole_camera_rays(32, 32, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0, device=cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ALL)
def test_mixed_precision_per_hit_and_sums_follow_the_kernel(gh, scene, small_rays, kernel, kernel_reset):
    """trace_sph<float4, int, double>: ir = 1.f / w in float, the rest in double (bit for bit);
    trace_cumulative_sph<float4, double>: the float term lerp<float> over the double table, summed in
    double in class order."""
    import torch
    d, tree, sh, _ = scene
    rays = small_rays
    table = _table(gh, kernel)
    _select(gh, kernel)
    off, idx, w, _ = gh.trace_sph(rays, d, tree, real=torch.float64)
    off, idx, w = off.cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy()
    rh = rays.cpu().numpy()
    ray = hit_rays(off, len(idx))
    r, sp = rh[ray], sh[idx]
    p = [(sp[:, k] - r[:, 3 + k]).astype(F32).astype(F64) for k in range(3)]   # float subtraction, widened
    dd = [r[:, k].astype(F64) for k in range(3)]
    dot = p[0] * dd[0] + p[1] * dd[1] + p[2] * dd[2]
    bb = [p[k] - dot * dd[k] for k in range(3)]
    b2 = bb[0] * bb[0] + bb[1] * bb[1] + bb[2] * bb[2]
    ir = (F32(1) / sp[:, 3]).astype(F32).astype(F64)
    ref = np.array([integral_f64(b2[j], ir[j], table) for j in range(len(idx))], F64)
    assert np.array_equal(_bits(w), _bits(ref)), kernel
    # the double column densities: float terms (x formed in double and rounded to float once; lerp in
    # double, rounded to float; times the float ir^2)
    x = (50 * (np.sqrt(b2) * ir)).astype(F32)
    i = x.astype(np.int64)
    over = i >= 50
    x = np.where(over, F32(50), x); i = np.where(over, 49, i)
    t = x.astype(F64) - i
    y = np.array([_fma(t[j], table[i[j] + 1] - table[i[j]], table[i[j]]) for j in range(len(idx))]).astype(F32)
    terms = (y * (ir.astype(F32) * ir.astype(F32)).astype(F32)).astype(F32).astype(F64)
    sums = class_sums(len(rh), off, idx, terms, F64)
    got = _cumulative(gh, rays, d, tree, torch.float64)
    assert np.array_equal(_bits(got), _bits(sums)), kernel


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ALL)
def test_double4_column_densities_follow_the_kernel(gh, scene, small_rays, cuda, kernel, kernel_reset):
    import torch
    _, _, sh, _ = scene
    table = _table(gh, kernel)
    s = torch.from_numpy(sh.astype(F64)).to(cuda)
    tree = gh.Tree(len(sh), 32, device=cuda)
    gh.build_tree_d4(s, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    _select(gh, kernel)
    rays = small_rays
    off, idx, w, _ = gh.trace_sph_d4(rays, s, tree)
    off, idx, w = off.cpu().numpy(), idx.cpu().numpy(), w.cpu().numpy()
    s64, rh = s.cpu().numpy(), rays.cpu().numpy()
    ray = hit_rays(off, len(idx))
    r, sp = rh[ray].astype(F64), s64[idx]
    p = [sp[:, k] - r[:, 3 + k] for k in range(3)]
    dot = p[0] * r[:, 0] + p[1] * r[:, 1] + p[2] * r[:, 2]
    bb = [p[k] - dot * r[:, k] for k in range(3)]
    b2 = bb[0] * bb[0] + bb[1] * bb[1] + bb[2] * bb[2]
    terms = np.array([integral_f64(b2[j], 1.0 / sp[j, 3], table) for j in range(len(idx))], F64)
    assert np.array_equal(_bits(w), _bits(terms)), kernel
    got = torch.empty(len(rays), dtype=torch.float64, device=cuda)
    gh.trace_cumulative_d4(rays, s, tree, got)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(class_sums(len(rh), off, idx, terms, F64))), kernel


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS[1:] + ("custom",))
def test_weights_of_one_give_the_kernels_unweighted_bits(gh, scene, cuda, kernel, integral_mode, kernel_reset):
    import torch
    d, tree, sh, sets = scene
    _select(gh, kernel)
    ones = torch.ones((len(d), 3), dtype=torch.float32, device=cuda)
    for name, (rays, *_) in sets.items():
        ref = _cumulative(gh, rays, d, tree)
        got = gh.trace_cumulative_weighted_sph(rays, d, tree, ones, check=True).cpu().numpy()
        for c in range(3):
            assert np.array_equal(_bits(got[:, c]), _bits(ref)), (kernel, integral_mode, name, c)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ALL)
def test_volume_integral_is_the_tables_lerp_volume(gh, cuda, kernel, kernel_reset):
    """The two spheres of test_volume_integral_kat_on_gpu: sum out * area / 2 is the lerp's volume,
    which tells the kernels apart (C2 - cubic: 7e-5)."""
    import torch
    _select(gh, kernel)
    s = torch.tensor([[-0.5, -0.5, -0.5, 0.2], [0.5, 0.5, 0.5, 0.2]], dtype=torch.float32, device=cuda)
    tree = gh.Tree(2, 1, device=cuda)
    gh.build_tree(s, tree, (-1, -1, -1), (1, 1, 1))
    rays, area = gh.orthogonal_rays_z(512, (-1, -1, -1, 0.2), (1, 1, 1, 0.2), device=cuda)
    out = _cumulative(gh, rays, s, tree)
    integral = float(out.astype(F64).sum()) * area / 2
    expect = lerp_volume(_table(gh, kernel))
    assert abs(integral - expect) < 2e-5, (kernel, integral, expect)


@pytest.mark.gpu
def test_custom_tables_set_get_and_refuse(gh, scene, kernel_reset):
    import ctypes as C
    d, tree, sh, sets = scene
    rays = sets["pinhole"][0]
    c2 = gh.sph_kernel_table("wendland_c2")
    gh.set_sph_kernel("wendland_c2")
    assert gh.sph_kernel()[0] == "wendland_c2"
    ref = _cumulative(gh, rays, d, tree)
    gh.set_sph_kernel(c2.copy())
    name, table = gh.sph_kernel()
    assert name == "custom" and np.array_equal(_bits(table), _bits(c2))
    assert np.array_equal(_bits(_cumulative(gh, rays, d, tree)), _bits(ref))
    user = _custom()
    gh.set_sph_kernel(user)
    before = _cumulative(gh, rays, d, tree)
    bad = [c2[:50], np.append(c2, 0.0), np.where(np.arange(51) == 7, np.nan, c2),
           np.where(np.arange(51) == 3, -1e-9, c2), np.where(np.arange(51) == 50, 1e-6, c2),
           np.where(np.arange(51) == 0, np.inf, c2)]
    for t in bad:
        with pytest.raises(ValueError):
            gh.set_sph_kernel(t)
        name, table = gh.sph_kernel()
        assert name == "custom" and np.array_equal(_bits(table), _bits(user))
    for nm in ("gaussian", "custom", ""):
        with pytest.raises(ValueError):
            gh.set_sph_kernel(nm)
    assert np.array_equal(_bits(_cumulative(gh, rays, d, tree)), _bits(before))
    # the C ABI: built-in kinds only, n must be 51, null refused
    for kind in (-1, 6, 100):
        assert gh._lib.grace_trace_set_sph_kernel(C.c_int(kind)) == gh.GRACE_INVALID_ARGUMENT
    arr = (C.c_double * 51)(*c2)
    assert gh._lib.grace_trace_set_sph_kernel_table(arr, C.c_int(50)) == gh.GRACE_INVALID_ARGUMENT
    assert gh._lib.grace_trace_set_sph_kernel_table(None, C.c_int(51)) == gh.GRACE_INVALID_ARGUMENT
    assert gh._lib.grace_sph_kernel_table(C.c_int(-1), arr) == gh.GRACE_INVALID_ARGUMENT
    assert gh.sph_kernel()[0] == "custom"


@pytest.mark.gpu
def test_cubic_is_the_default_and_switching_back_restores_it(gh, scene, integral_mode, kernel_reset):
    d, tree, sh, sets = scene
    assert gh.sph_kernel()[0] == "cubic"
    for name, (rays, *_) in sets.items():
        default = _cumulative(gh, rays, d, tree)
        gh.set_sph_kernel("cubic")
        assert np.array_equal(_bits(_cumulative(gh, rays, d, tree)), _bits(default)), name
        gh.set_sph_kernel("wendland_c2")
        c2 = _cumulative(gh, rays, d, tree)
        assert not np.array_equal(_bits(c2), _bits(default))
        gh.set_sph_kernel("cubic")
        assert np.array_equal(_bits(_cumulative(gh, rays, d, tree)), _bits(default)), name


@pytest.mark.gpu
def test_no_cached_record_depends_on_the_kernel(gh, scene, kernel_reset):
    d, tree, sh, sets = scene
    rays = sets["orthographic"][0]
    gh.set_cache_auto(False)
    try:
        gh.set_sph_kernel("wendland_c2")
        uncached = _cumulative(gh, rays, d, tree)
    finally:
        gh.set_cache_auto(True)
    gh.set_sph_kernel("cubic")
    for _ in range(3):                                   # seen twice: scene and rays cached
        _cumulative(gh, rays, d, tree)
    gh.set_sph_kernel("wendland_c2")
    assert np.array_equal(_bits(_cumulative(gh, rays, d, tree)), _bits(uncached))
    gh.trace_prepare(d, tree)                           # a prepared scene as well
    try:
        assert np.array_equal(_bits(_cumulative(gh, rays, d, tree)), _bits(uncached))
    finally:
        gh.trace_release()


@pytest.mark.gpu
def test_contexts_keep_their_own_kernels(gh, scene, kernel_reset):
    d, tree, sh, sets = scene
    rays = sets["isotropic"][0]
    ref_cubic = _cumulative(gh, rays, d, tree)
    gh.set_sph_kernel("wendland_c6")
    ref_c6 = _cumulative(gh, rays, d, tree)
    gh.set_sph_kernel("cubic")
    a, b = gh.Context(), gh.Context()
    try:
        a.make_current(); gh.set_sph_kernel("wendland_c6")
        b.make_current(); gh.set_sph_kernel(gh.sph_kernel_table("cubic"))
        for _ in range(2):
            a.make_current()
            assert gh.sph_kernel()[0] == "wendland_c6"
            assert np.array_equal(_bits(_cumulative(gh, rays, d, tree)), _bits(ref_c6))
            b.make_current()
            assert gh.sph_kernel()[0] == "custom"
            assert np.array_equal(_bits(_cumulative(gh, rays, d, tree)), _bits(ref_cubic))
    finally:
        gh.Context.reset_current()
        a.destroy(); b.destroy()
    assert gh.sph_kernel()[0] == "cubic"


@pytest.mark.gpu
def test_a_queued_trace_keeps_its_kernel(gh, cuda, kernel_reset):
    """A large trace enqueued just before a switch (built-in, then a custom table) computes with the
    kernel it was enqueued with."""
    import torch
    g = torch.Generator(device=cuda); g.manual_seed(9)
    n = 400_000
    s = torch.cat([torch.rand((n, 3), generator=g, device=cuda),
                   0.004 + 0.01 * torch.rand((n, 1), generator=g, device=cuda)], 1).contiguous()
    tree = gh.Tree(n, 32, device=cuda)
    gh.build_tree(s, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    rays = gh.pinhole_camera_rays(1024, 1024, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0, device=cuda)
    refs = {}
    for k in ("cubic", "wendland_c2"):
        gh.set_sph_kernel(k)
        refs[k] = _cumulative(gh, rays, s, tree)
    assert not np.array_equal(_bits(refs["cubic"]), _bits(refs["wendland_c2"]))
    torch.cuda.synchronize()
    out = torch.empty(len(rays), dtype=torch.float32, device=cuda)
    gh.set_sph_kernel("cubic")
    gh.trace_cumulative_sph(rays, s, tree, out)          # asynchronous
    gh.set_sph_kernel("wendland_c2")                     # a pointer switch, no synchronisation
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(refs["cubic"]))
    out2 = torch.empty_like(out)
    gh.trace_cumulative_sph(rays, s, tree, out2)
    gh.set_sph_kernel(gh.sph_kernel_table("cubic"))      # a custom table: synchronises, then copies
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(refs["wendland_c2"]))
    out3 = torch.empty_like(out)
    gh.trace_cumulative_sph(rays, s, tree, out3)
    gh.set_sph_kernel(gh.sph_kernel_table("wendland_c2"))   # overwrites the buffer out3's trace reads
    assert np.array_equal(_bits(out3.cpu().numpy()), _bits(refs["cubic"]))


@pytest.mark.gpu
def test_sph_kernel_dropin_program_matches_ctypes(gh, scene, small_rays, tmp_path, kernel_reset):
    d, tree, sh, _ = scene
    rays = small_rays
    sh.tofile(str(tmp_path / "s.f32"))
    rays.cpu().numpy().tofile(str(tmp_path / "r.f32"))
    exe = str(tmp_path / "dropin_sph_kernels")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_sph_kernels.hip"), "-o", exe,
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    res = subprocess.run([exe, str(tmp_path / "s.f32"), str(tmp_path / "r.f32"), str(tmp_path)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    gh.set_sph_kernel("wendland_c2")
    got = _cumulative(gh, rays, d, tree)
    assert np.array_equal(_bits(got), np.fromfile(str(tmp_path / "wc2.f32"), np.uint32))
