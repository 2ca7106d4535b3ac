"""Depth-ordered emission-absorption integrals (grace_trace_emission_absorption_f4,
trace_emission_absorption_sph).  The contract, from include/grace_hip.h: a ray's hits are those of
trace_sph (same hit test, per-hit integral I and distance d, bit for bit), ordered ascending by
(d as fp32, sphere index); then in fp64

    a_k   = absorption[i_k] * I_k
    tau_k = sum_{m<k} a_m
    phi(a) = -expm1(-a) / a   (1 for a == 0)
    out[r, c] = fl32( sum_k emission[i_k, c] * I_k * phi(a_k) * exp(-tau_k) ),   tau[r] = fl32( sum_k a_k )

Expected values restate this in NumPy from the oracle's per-hit outputs (oracle.brute_hits).

The tolerance is derived, not measured.  The inputs of the fp64 arithmetic are bit-equal on both
sides, so device and NumPy differ only by fp64 rounding, the two exp-family functions (a few ulp
each) and the order of the n_r additions; an absolute error delta in tau_k is a relative error
delta in exp(-tau_k).  Hence, with S = sum_k |term_k|,

    |out - ref| <= spacing(fl32(|ref|)) / 2  +  8 (n_r + 8) 2^-53 max(1, tau_r) S

the first term being the final rounding to fp32 and the second a loose bound on the fp64 error;
tau gets the same bound with S = tau_r."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32, F64 = np.float32, np.float64
ENTRY_POINTS = ["grace_trace_emission_absorption_f4", "grace_trace_set_ordered_budget",
                "grace_trace_ordered_limits", "grace_trace_ordered_enable_stats",
                "grace_trace_ordered_last_stats"]


# ---- the restatement ----------------------------------------------------------------------------
def restate(n_rays, offsets, idx, integ, dist, emission, absorption, reverse_ties=False):
    """(out [n_rays, C], tau [n_rays], S [n_rays, C], n_r [n_rays]) in fp64."""
    n_hits = len(idx)
    counts = np.diff(np.append(offsets, n_hits)).astype(np.int64)
    ray = np.repeat(np.arange(n_rays), counts)
    tie = -idx.astype(np.int64) if reverse_ties else idx.astype(np.int64)
    order = np.lexsort((tie, dist, ray))                 # by ray, distance (fp32), sphere index
    idx, I = idx[order], integ[order].astype(F64)
    C = emission.shape[1]
    out = np.zeros((n_rays, C), F64); S = np.zeros((n_rays, C), F64); tau = np.zeros(n_rays, F64)
    start = np.cumsum(counts) - counts
    for r in range(n_rays):
        if counts[r] == 0:
            continue
        sl = slice(start[r], start[r] + counts[r])
        i, Ir = idx[sl], I[sl]
        a = absorption[i].astype(F64) * Ir
        tau_k = np.concatenate(([0.0], np.cumsum(a)[:-1]))
        with np.errstate(divide="ignore", invalid="ignore"):
            phi = np.where(a != 0, -np.expm1(-a) / np.where(a != 0, a, 1.0), 1.0)
        term = emission[i].astype(F64) * Ir[:, None] * (phi * np.exp(-tau_k))[:, None]
        out[r] = term.sum(0); S[r] = np.abs(term).sum(0); tau[r] = a.sum()
    return out, tau, S, counts


def bound(ref, S, n_r, tau_r):
    n_r = np.asarray(n_r, F64); tau_r = np.asarray(tau_r, F64)
    if ref.ndim == 2:
        n_r, tau_r = n_r[:, None], tau_r[:, None]
    return np.spacing(np.abs(ref).astype(F32)).astype(F64) / 2 \
        + 8.0 * (n_r + 8.0) * 2.0 ** -53 * np.maximum(1.0, tau_r) * S


def check(got, got_tau, ref, tau, S, n_r, what=""):
    err, tol = np.abs(got.astype(F64) - ref), bound(ref, S, n_r, tau)
    print("%s: out max err/tol %.3g (max |ref| %.3g); tau range %.3g..%.3g" % (
        what, float(np.max(err / tol)) if err.size else 0.0, float(np.abs(ref).max()) if err.size else 0.0,
        float(tau.min()) if tau.size else 0.0, float(tau.max()) if tau.size else 0.0))
    bad = np.argwhere(err > tol)
    assert len(bad) == 0, (what, bad[:5], got[tuple(bad[0])], ref[tuple(bad[0])])
    if got_tau is not None:
        err, tol = np.abs(got_tau.astype(F64) - tau), bound(tau, np.abs(tau), n_r, tau)
        bad = np.nonzero(err > tol)[0]
        assert len(bad) == 0, (what, "tau", bad[:5], got_tau[bad[:5]], tau[bad[:5]])


# ---- CPU: exported, and the drop-in forms compile -------------------------------------------------
def test_entry_points_are_exported():
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_emission_absorption"
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_emission_absorption.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


def test_mirror_compiles_with_gxx(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::Ray>& r, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::Tree& t, const grace::device_vector<float>& e, const grace::device_vector<float>& k)\n"
                   "{\n"
                   "    grace::device_vector<float> out(r.size() * 3), tau(r.size());\n"
                   "    grace::trace_emission_absorption_sph(r, s, t, e, 3, k, out);\n"
                   "    grace::trace_emission_absorption_sph(r, s, t, e, 3, k, out, &tau);\n"
                   "    grace::set_ordered_budget(0);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


# ---- GPU --------------------------------------------------------------------------------------------
N_SCENE = 20000


def _build(gh, cuda, s):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(s, F32)).to(cuda)
    tree = gh.Tree(len(s), 32, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))     # sorts d
    return d, tree


def _coefficients(sh, C, seed, signed=True):
    """Emission of both signs; absorption ~ 1e-3 h^2 rising 3.5 decades along x, so that with
    I ~ 1/h^2 the optical depth of a ray spans roughly 0.01 to 30 across an image."""
    rng = np.random.default_rng(seed)
    e = rng.random((len(sh), C)).astype(F32) * F32(4.0)
    e = (e - F32(2.0)).astype(F32) if signed else (e + F32(0.25)).astype(F32)
    k = (6e-4 * sh[:, 3].astype(F64) ** 2 * 10.0 ** (3.5 * sh[:, 0].astype(F64))
         * (0.5 + rng.random(len(sh)))).astype(F32)
    return e, k


def _trace(gh, rays, d, tree, e, k, want_tau=True):
    import torch
    tau = torch.empty(len(rays), dtype=torch.float32, device=rays.device) if want_tau else None
    out = gh.trace_emission_absorption_sph(rays, d, tree, torch.from_numpy(e).to(rays.device),
                                           torch.from_numpy(k).to(rays.device), tau=tau, check=True)
    return out.cpu().numpy().reshape(len(rays), -1), (tau.cpu().numpy() if want_tau else None)


@pytest.fixture(autouse=True)
def _knobs_reset(request):
    yield
    if "gh" in request.fixturenames:
        gh = request.getfixturevalue("gh")
        gh.set_ordered_budget(0); gh.ordered_enable_stats(False)
        gh.set_packet_width(-1); gh.set_sph_kernel("cubic")


@pytest.fixture(scope="module")
def ea_scene(gh, oracle, cuda):
    import torch
    rng = np.random.default_rng(3)
    s = np.empty((N_SCENE, 4), F32)
    s[:, :3] = rng.random((N_SCENE, 3), dtype=F32)
    s[:, 3] = (0.01 + 0.04 * rng.random(N_SCENE)).astype(F32)     # radii spanning 5x
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()
    points = torch.from_numpy(rng.random((1024, 3), dtype=F32)).to(cuda)
    sets = {
        "orthographic": gh.orthogonal_rays_z(48, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0],
        "pinhole": gh.pinhole_camera_rays(48, 48, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0,
                                          device=cuda),
        "healpix": gh.healpix_rays(8, (0.5, 0.5, 0.5), 1.0, device=cuda),
        "one_to_many": gh.one_to_many_rays((0.45, 0.55, 0.5), points),
    }
    out = {}
    for name, rays in sets.items():
        hits = oracle.brute_hits(rays.cpu().numpy(), sh)
        assert len(hits[1]) > 0
        out[name] = (rays, hits)
    return d, tree, sh, out


RAY_SETS = ["orthographic", "pinhole", "healpix", "one_to_many"]


@pytest.mark.gpu
@pytest.mark.parametrize("rays_name", RAY_SETS)
@pytest.mark.parametrize("C", [1, 3, 5, 64])
def test_random_scenes_match_the_restatement(gh, ea_scene, rays_name, C):
    d, tree, sh, sets = ea_scene
    rays, (off, idx, integ, dist) = sets[rays_name]
    e, k = _coefficients(sh, C, 100 + C)
    got, got_tau = _trace(gh, rays, d, tree, e, k)
    ref, tau, S, n_r = restate(len(rays), off, idx, integ, dist, e, k)
    if rays_name in ("orthographic", "pinhole"):     # thin and thick rays in one image
        hit = tau[n_r > 0]
        assert hit.min() < 0.1 and hit.max() > 10.0, (hit.min(), hit.max())
    check(got, got_tau, ref, tau, S, n_r, "%s C=%d" % (rays_name, C))


@pytest.mark.gpu
@pytest.mark.parametrize("rays_name", RAY_SETS)
def test_random_scenes_with_a_wendland_kernel(gh, ea_scene, rays_name):
    from test_sph_kernels import b2_f32, hit_rays, integrals_f32   # the per-hit arithmetic, restated there
    d, tree, sh, sets = ea_scene
    rays, (off, idx, _, dist) = sets[rays_name]
    rh = rays.cpu().numpy()
    integ = integrals_f32(b2_f32(rh, sh, hit_rays(off, len(idx)), idx), sh[idx, 3],
                          gh.sph_kernel_table("wendland_c2"))
    gh.set_sph_kernel("wendland_c2")
    e, k = _coefficients(sh, 3, 7)
    got, got_tau = _trace(gh, rays, d, tree, e, k)
    ref, tau, S, n_r = restate(len(rays), off, idx, integ, dist, e, k)
    check(got, got_tau, ref, tau, S, n_r, "%s wendland_c2" % rays_name)


@pytest.mark.gpu
def test_ties_are_broken_by_ascending_index(gh, oracle, cuda):
    """12^3 lattice, rays along z: every ray has hits at bit-equal distance, and the other
    tie-break gives another answer -- asserted first, so the scene cannot stop testing it."""
    g = 12; sp = 1.0 / g
    x = (np.arange(g) + 0.5) * sp
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    s = np.stack([X.ravel(), Y.ravel(), Z.ravel(), np.full(g ** 3, 1.3 * sp)], 1).astype(F32)
    rng = np.random.default_rng(1)
    s = s[rng.permutation(len(s))]
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()
    rays_h, _ = oracle.orthogonal_rays_z(16, (0, 0, 0, 0), (1, 1, 1, 0))
    n = len(rays_h)
    off, idx, integ, dist = oracle.brute_hits(rays_h, sh)
    ray = np.repeat(np.arange(n), np.diff(np.append(off, len(idx))))
    key = ray.astype(np.int64) * (1 << 32) + dist.view(np.uint32)
    u, c = np.unique(key, return_counts=True)
    assert len(np.unique(u[c > 1] >> 32)) == n                   # every ray has tied hits
    e = rng.random((len(sh), 3)).astype(F32); k = (rng.random(len(sh)) * 0.2).astype(F32)
    ref, tau, S, n_r = restate(n, off, idx, integ, dist, e, k)
    other, _, _, _ = restate(n, off, idx, integ, dist, e, k, reverse_ties=True)
    rel = np.abs(other - ref).max(1) / np.abs(ref).max(1)
    assert np.all(rel > 2.0 ** -20), rel.min()                     # ... and the tie-break matters on every ray
    import torch
    rays = torch.from_numpy(np.ascontiguousarray(rays_h).view(F32).reshape(n, 7)).to(cuda)
    got, got_tau = _trace(gh, rays, d, tree, e, k)
    check(got, got_tau, ref, tau, S, n_r, "lattice")


def _collinear_scene(counts, cuda):
    """Rays along z on an 8-column grid of pitch 0.1; ray j's spheres (radius 0.01) sit on it."""
    import torch
    rays = np.zeros((len(counts), 7), F32)
    spheres = []
    for j, m in enumerate(counts):
        x, y = 0.1 + 0.1 * (j % 8), 0.1 + 0.1 * (j // 8)
        rays[j] = (0, 0, 1, x, y, -0.1, 1.2)
        if m:
            z = (np.arange(m) + 0.5) / m * 0.9 + 0.05
            spheres.append(np.stack([np.full(m, x), np.full(m, y), z, np.full(m, 0.01)], 1))
    s = np.concatenate(spheres).astype(F32)
    return torch.from_numpy(rays).to(cuda), s


@pytest.mark.gpu
def test_tier_edges(gh, oracle, cuda):
    w, b = gh.ordered_limits()
    assert 64 <= w < b
    counts = [0, 3, w - 1, w, w + 1, 40, b - 1, 0, b, b + 1, 4 * b, 1, 0, w // 2, 2 * w, 17,
              0, 0, 5, 0, 64, 65, 63, 0, 0, 0, 0, 0, 0, 0, 0, 2]
    rays, s = _collinear_scene(counts, cuda)
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()
    off, idx, integ, dist = oracle.brute_hits(rays.cpu().numpy(), sh)
    assert np.array_equal(np.diff(np.append(off, len(idx))), counts)     # exact hit counts
    rng = np.random.default_rng(5)
    e = (rng.random((len(sh), 5)).astype(F32) - F32(0.5)).astype(F32)
    k = (rng.random(len(sh)) * 2e-6).astype(F32)                          # I ~ 1.9e4: a ~ 0.02 per hit
    gh.ordered_enable_stats(True)
    got, got_tau = _trace(gh, rays, d, tree, e, k)
    st = gh.ordered_last_stats()
    c = np.array(counts)
    assert st["rays_wave"] == np.sum(c <= w) and st["rays_block"] == np.sum((c > w) & (c <= b))
    assert st["rays_global"] == np.sum(c > b) == 2 and st["total_hits"] == c.sum()
    ref, tau, S, n_r = restate(len(rays), off, idx, integ, dist, e, k)
    check(got, got_tau, ref, tau, S, n_r, "tier edges")
    assert np.all(got[c == 0] == 0) and np.all(got_tau[c == 0] == 0)
    # the same rays in batches: a ray longer than the budget is a batch of its own
    gh.set_ordered_budget(12 * (b + 1))
    again, again_tau = _trace(gh, rays, d, tree, e, k)
    assert gh.ordered_last_stats()["batches"] > 5
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    assert np.array_equal(again_tau.view(np.uint32), got_tau.view(np.uint32))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
def test_results_are_bitwise_invariant(gh, ea_scene, cuda):
    import torch
    d, tree, sh, sets = ea_scene
    rays, (off, idx, integ, dist) = sets["pinhole"]
    e, k = _coefficients(sh, 5, 11)
    gh.ordered_enable_stats(True)
    gh.set_ordered_budget(1 << 32)
    base, base_tau = _trace(gh, rays, d, tree, e, k)
    st = gh.ordered_last_stats()
    assert st["batches"] == 1 and st["total_hits"] == len(idx)
    same = lambda o, t, rows=slice(None): (np.array_equal(_bits(o), _bits(base[rows]))
                                           and np.array_equal(_bits(t), _bits(base_tau[rows])))
    assert same(*_trace(gh, rays, d, tree, e, k))                         # two runs
    gh.set_ordered_budget(12 * len(idx) // 7)
    assert same(*_trace(gh, rays, d, tree, e, k))
    assert gh.ordered_last_stats()["batches"] >= 5
    sub = slice(1000, 1256)
    gh.set_ordered_budget(1)                                              # one batch per ray
    assert same(*_trace(gh, rays[sub].contiguous(), d, tree, e, k), rows=sub)
    n_sub = np.diff(np.append(off, len(idx)))[sub]
    assert np.all(n_sub > 0) and gh.ordered_last_stats()["batches"] == 256
    gh.set_ordered_budget(0)
    for width in (64, 32, 16):
        gh.set_packet_width(width)
        assert same(*_trace(gh, rays, d, tree, e, k)), width
    gh.set_packet_width(-1)
    perm = torch.randperm(len(rays), generator=torch.Generator().manual_seed(3))
    o, t = _trace(gh, rays[perm.to(cuda)].contiguous(), d, tree, e, k)    # rays permuted: outputs permute
    assert np.array_equal(_bits(o), _bits(base[perm.numpy()])) and np.array_equal(_bits(t), _bits(base_tau[perm.numpy()]))
    r = 1234                                                               # a ray traced alone
    assert np.diff(np.append(off, len(idx)))[r] > 0
    alone = rays[r:r + 1].repeat(32, 1)                                   # (ray counts are multiples of 32:
    alone[1:, 3:6] += 10.0                                                 #  31 companions that miss the box)
    o, t = _trace(gh, alone.contiguous(), d, tree, e, k)
    assert np.array_equal(_bits(o[:1]), _bits(base[r:r + 1])) and np.array_equal(_bits(t[:1]), _bits(base_tau[r:r + 1]))
    assert np.all(o[1:] == 0) and np.all(t[1:] == 0)
    o, _ = _trace(gh, rays, d, tree, e, k, want_tau=False)                # tau is optional
    assert np.array_equal(_bits(o), _bits(base))


@pytest.mark.gpu
def test_zero_absorption_is_the_weighted_column_density(gh, ea_scene, cuda):
    import torch
    d, tree, sh, sets = ea_scene
    rays, _ = sets["orthographic"]
    e, _ = _coefficients(sh, 3, 13, signed=False)
    got, got_tau = _trace(gh, rays, d, tree, e, np.zeros(len(sh), F32))
    ref = gh.trace_cumulative_weighted_sph(rays, d, tree, torch.from_numpy(e).to(cuda)).cpu().numpy()
    assert np.all(np.abs(got - ref) <= 1e-5 * np.abs(ref))
    assert np.all(got_tau == 0)


@pytest.mark.gpu
def test_one_sphere_is_a_uniform_slab(gh, oracle, cuda):
    d, tree = _build_one(gh, cuda, np.array([[0.5, 0.5, 0.5, 0.2]], F32))
    sh = d.cpu().numpy()
    rays = gh.orthogonal_rays_z(16, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    off, idx, integ, dist = oracle.brute_hits(rays.cpu().numpy(), sh)
    n_r = np.diff(np.append(off, len(idx)))
    assert 0 < n_r.sum() < len(rays) and n_r.max() == 1 and np.all(sh[idx, 3] == F32(0.2))
    e = np.array([[3.0, -1.5]], F32); k = np.array([0.25], F32)
    got, got_tau = _trace(gh, rays, d, tree, np.repeat(e, len(sh), 0), np.repeat(k, len(sh)))
    a = np.zeros(len(rays), F64); a[n_r > 0] = F64(k[0]) * integ.astype(F64)
    ref = (e.astype(F64) / F64(k[0])) * -np.expm1(-a)[:, None]            # S (1 - e^-a)
    check(got, got_tau, ref, a, np.abs(ref), n_r, "one sphere")
    assert np.all(got[n_r == 0] == 0) and np.all(got_tau[n_r == 0] == 0)  # rays that hit nothing


def _build_one(gh, cuda, s):
    """A tree needs more spheres than fit a leaf: pad with spheres no ray of the test meets."""
    pad = np.tile(np.array([[0.01, 0.01, 0.99, 1e-4]], F32), (63, 1))
    pad[:, 0] += np.arange(63, dtype=F32) * F32(1e-3)
    full = np.concatenate([s, pad]).astype(F32)
    return _build(gh, cuda, full)


@pytest.mark.gpu
def test_underflowing_transmittance_stays_finite(gh, ea_scene):
    d, tree, sh, sets = ea_scene
    rays, (off, idx, integ, dist) = sets["orthographic"]
    e, k = _coefficients(sh, 3, 17)
    k = (k * F32(1e4)).astype(F32)
    got, got_tau = _trace(gh, rays, d, tree, e, k)
    ref, tau, S, n_r = restate(len(rays), off, idx, integ, dist, e, k)
    assert tau.max() > 800.0                                               # exp(-tau) underflows in fp64
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(got_tau))
    check(got, got_tau, ref, tau, S, n_r, "thick")


@pytest.mark.gpu
def test_argument_checks(gh, ea_scene, cuda):
    import torch
    d, tree, sh, sets = ea_scene
    rays, _ = sets["healpix"]
    n = len(sh)
    k = torch.zeros(n, device=cuda)
    out = torch.full((len(rays), 2), 7.0, device=cuda)
    args = gh._trace_args(rays, d, tree)
    call = lambda a, em, C, ab, o: gh._lib.grace_trace_emission_absorption_f4(
        *a, gh._ptr(em), ctypes.c_int(C), gh._ptr(ab), gh._ptr(o), gh._ptr(None), gh._stream())
    e2 = torch.zeros((n, 2), device=cuda)
    for C in (0, 65, -1):
        assert call(args, e2, C, k, out) == gh.GRACE_INVALID_ARGUMENT
    assert call(args, e2, 2, k, None) == gh.GRACE_INVALID_ARGUMENT
    assert call(args, None, 2, k, out) == gh.GRACE_INVALID_ARGUMENT
    assert call(args, e2, 2, None, out) == gh.GRACE_INVALID_ARGUMENT
    empty = (args[0], ctypes.c_size_t(0)) + args[2:]
    assert call(empty, e2, 2, k, out) == gh.GRACE_OK                       # zero rays: nothing written
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)
    with pytest.raises(ValueError):
        gh.trace_emission_absorption_sph(rays, d, tree, torch.zeros((n, 65), device=cuda), k)
    with pytest.raises(ValueError):
        gh.trace_emission_absorption_sph(rays, d, tree, torch.zeros((n, 0), device=cuda), k)
    with pytest.raises(ValueError):
        gh.trace_emission_absorption_sph(rays, d, tree, e2, k[:-1])
    with pytest.raises(ValueError):
        gh.trace_emission_absorption_sph(rays, d, tree, e2, k, out=out[:-1])
    with pytest.raises(ValueError):
        gh.trace_emission_absorption_sph(rays, d, tree, e2, k, tau=torch.zeros(3, device=cuda))


@pytest.mark.gpu
def test_more_hits_than_int32_can_index(gh, oracle, cuda):
    """1024^2 orthographic rays over 2 x 10^6 uniform particles: ~2.3e9 hits, on which trace_sph
    raises.  Three relations over the whole image, and the restatement on 64 of its rays."""
    import torch
    n = 2_000_000
    rng = np.random.default_rng(23)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = (0.0175 + 0.0025 * rng.random(n)).astype(F32)
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()
    rays = gh.orthogonal_rays_z(1024, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    counts = torch.empty(len(rays), dtype=torch.int32, device=cuda)
    gh.trace_hitcounts_sph(rays, d, tree, counts)
    total = int(counts.long().sum())
    assert total > 2 ** 31
    with pytest.raises(ValueError):
        gh.trace_sph(rays, d, tree)
    e = torch.from_numpy((0.25 + rng.random((n, 2))).astype(F32)).to(cuda)
    k = torch.from_numpy((1e-3 * sh[:, 3].astype(F64) ** 2 * 10.0 ** (1.5 * sh[:, 0])).astype(F32)).to(cuda)
    gh.ordered_enable_stats(True)
    tau0 = torch.empty(len(rays), device=cuda)
    thin = gh.trace_emission_absorption_sph(rays, d, tree, e, torch.zeros(n, device=cuda), tau=tau0, check=True)
    st = gh.ordered_last_stats()
    print("beyond int32:", st)
    assert st["total_hits"] == total and st["batches"] > 1
    col = gh.trace_cumulative_weighted_sph(rays, d, tree, e)
    assert torch.all((thin - col).abs() <= 1e-5 * col) and torch.all(tau0 == 0)
    tau = torch.empty(len(rays), device=cuda)
    thick = gh.trace_emission_absorption_sph(rays, d, tree, e, k, tau=tau, check=True)
    col_k = gh.trace_cumulative_weighted_sph(rays, d, tree, k)
    assert torch.all((tau - col_k).abs() <= 1e-5 * col_k)
    assert torch.all(thick >= 0) and torch.all(thick <= thin * (1 + 1e-5))
    assert float(tau.max()) > 1.0 and float((thick / thin).min()) < 0.7     # absorption did something
    # ... and 64 rays spread over the image against the restatement
    sub = torch.from_numpy(_spread(len(rays), 64)).to(cuda)
    off, idx, integ, dist = oracle.brute_hits(rays[sub].cpu().numpy(), sh)
    eh, kh = e.cpu().numpy(), k.cpu().numpy()
    ref, rtau, S, n_r = restate(64, off, idx, integ, dist, eh, kh)
    assert n_r.min() > 1000
    check(thick[sub].cpu().numpy(), tau[sub].cpu().numpy(), ref, rtau, S, n_r, "beyond int32, thick")
    ref, rtau, S, n_r = restate(64, off, idx, integ, dist, eh, np.zeros(n, F32))
    check(thin[sub].cpu().numpy(), tau0[sub].cpu().numpy(), ref, rtau, S, n_r, "beyond int32, thin")


def _spread(n_rays, k):
    """k ray indices spread over an image of n_rays, off the rows' starts."""
    return (np.arange(k, dtype=np.int64) * (n_rays // k) + (n_rays // k) // 3 + 7 * np.arange(k)) % n_rays


@pytest.mark.gpu
def test_more_batches_than_the_first_table_copy_holds(gh, oracle, ea_scene, cuda):
    """Budget 1 on 72^2 = 5184 rays that all hit: one batch a ray, more than the 4096 - 8 ends
    the first read of the batch table holds.  The bits of the single-batch call, and the
    restatement on a sample."""
    import torch
    d, tree, sh, _ = ea_scene
    rays = gh.orthogonal_rays_z(72, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    counts = torch.empty(len(rays), dtype=torch.int32, device=cuda)
    gh.trace_hitcounts_sph(rays, d, tree, counts, check=True)
    assert len(rays) >= 4200 and int(counts.min()) > 0
    e, k = _coefficients(sh, 3, 29)
    gh.ordered_enable_stats(True)
    gh.set_ordered_budget(1 << 32)
    base, base_tau = _trace(gh, rays, d, tree, e, k)
    assert gh.ordered_last_stats()["batches"] == 1
    gh.set_ordered_budget(1)
    got, got_tau = _trace(gh, rays, d, tree, e, k)
    st = gh.ordered_last_stats()
    assert st["batches"] == len(rays) > 4088 and st["total_hits"] == int(counts.long().sum())
    assert np.array_equal(_bits(got), _bits(base)) and np.array_equal(_bits(got_tau), _bits(base_tau))
    sub = _spread(len(rays), 128)
    off, idx, integ, dist = oracle.brute_hits(rays.cpu().numpy()[sub], sh)
    ref, tau, S, n_r = restate(len(sub), off, idx, integ, dist, e, k)
    check(got[sub], got_tau[sub], ref, tau, S, n_r, "5184 batches")


@pytest.mark.gpu
def test_a_call_whose_rays_hit_nothing(gh, ea_scene, cuda):
    """No hit in the whole call: the per-hit walk is not run; zeros come back, and the next
    ordinary call is what it was."""
    d, tree, sh, sets = ea_scene
    rays, (off, idx, _, _) = sets["healpix"]
    e, k = _coefficients(sh, 5, 37)
    before = _trace(gh, rays, d, tree, e, k)
    away = rays.clone()
    away[:, 3:6] += 10.0                                                   # length 1, ten box lengths off
    gh.ordered_enable_stats(True)
    got, got_tau = _trace(gh, away.contiguous(), d, tree, e, k)
    st = gh.ordered_last_stats()
    assert st["total_hits"] == 0 and st["batches"] == 1 and st["rays_wave"] == len(rays)
    assert not np.any(_bits(got)) and not np.any(_bits(got_tau))          # +0.0, every one
    after = _trace(gh, rays, d, tree, e, k)
    assert gh.ordered_last_stats()["total_hits"] == len(idx) > 0
    assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(_bits(after[1]), _bits(before[1]))


def clustered_scene(n, seed):
    """Gaussian blobs over a uniform third, radii log-uniform over 1.5 decades (0.003 ... 0.1)."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0.2, 0.8, (8, 3)); sigma = 10.0 ** rng.uniform(-1.5, -0.8, 8)
    which = rng.integers(0, 8, n)
    p = centre[which] + rng.normal(size=(n, 3)) * sigma[which, None]
    free = rng.random(n) < 1.0 / 3.0
    p[free] = rng.random((int(free.sum()), 3))
    s = np.empty((n, 4), F32)
    s[:, :3] = np.clip(p, 0.0, 1.0)
    s[:, 3] = 0.003 * 10.0 ** (1.5 * rng.random(n) + math.log10(0.1 / 0.003) - 1.5)
    return s


@pytest.mark.gpu
def test_one_batch_of_4096_packets_on_a_clustered_scene(gh, oracle, cuda):
    """512^2 rays in one batch: 4096 packets of 64, from where on the nested per-hit walk is the
    one-wave variant that stages in LDS.  The restatement on 256 sampled rays."""
    d, tree = _build(gh, cuda, clustered_scene(20000, 47))
    sh = d.cpu().numpy()
    assert sh[:, 3].max() / sh[:, 3].min() > 25.0
    rays = gh.orthogonal_rays_z(512, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    e, k = _coefficients(sh, 3, 53)
    gh.ordered_enable_stats(True)
    got, got_tau = _trace(gh, rays, d, tree, e, k)
    st = gh.ordered_last_stats()
    assert st["batches"] == 1 and len(rays) // 64 >= 4096
    sub = _spread(len(rays), 256)
    off, idx, integ, dist = oracle.brute_hits(rays.cpu().numpy()[sub], sh)
    assert len(idx) > 10000
    ref, tau, S, n_r = restate(len(sub), off, idx, integ, dist, e, k)
    check(got[sub], got_tau[sub], ref, tau, S, n_r, "4096 packets")


@pytest.mark.gpu
def test_heavy_packets_take_the_staged_split_walk(gh, oracle, cuda):
    """test_trace_boundaries' scene of heavy packets (100 000 spheres with h ~ 0.12, 16 packets of
    64 rays, ~4500 hits a ray: at least 200 000 hits a packet) through the nested per-hit walk,
    with hit staging on and off: the same bits, and the restatement on 40 rays."""
    import torch
    rng = np.random.default_rng(8)
    n = 100_000
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = rng.uniform(0.1, 0.14, n).astype(F32)
    side = 32
    g = (0.35 + 0.3 * (np.arange(side) + 0.5) / side)
    rays_h = np.zeros((side * side, 7), F32)
    rays_h[:, 2] = 1
    rays_h[:, 3] = np.repeat(g, side).astype(F32); rays_h[:, 4] = np.tile(g, side).astype(F32)
    rays_h[:, 5] = -0.1; rays_h[:, 6] = 1.2
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()
    rays = torch.from_numpy(rays_h).to(cuda)
    rng = np.random.default_rng(9)
    e = (rng.random((n, 3)) * 4.0 - 2.0).astype(F32)
    k = (2e-3 * sh[:, 3].astype(F64) ** 2 * 10.0 ** (2.0 * sh[:, 0].astype(F64)) * (0.5 + rng.random(n))).astype(F32)
    gh.ordered_enable_stats(True)
    try:
        gh.set_hits_staging(True)
        on = _trace(gh, rays, d, tree, e, k)
        st = gh.ordered_last_stats()
        assert st["batches"] == 1 and st["total_hits"] / (len(rays) / 64) >= 200_000, "below the staging threshold"
        gh.set_hits_staging(False)
        off_ = _trace(gh, rays, d, tree, e, k)
    finally:
        gh.set_hits_staging(True)
    assert np.array_equal(_bits(on[0]), _bits(off_[0])) and np.array_equal(_bits(on[1]), _bits(off_[1]))
    sub = np.sort(rng.choice(len(rays), 40, replace=False))
    off, idx, integ, dist = oracle.brute_hits(rays_h[sub], sh)
    ref, tau, S, n_r = restate(len(sub), off, idx, integ, dist, e, k)
    check(on[0][sub], on[1][sub], ref, tau, S, n_r, "heavy packets")


@pytest.mark.gpu
def test_a_context_with_its_own_stream_gives_the_same_bits(gh, ea_scene, cuda):
    import torch
    d, tree, sh, sets = ea_scene
    rays, _ = sets["healpix"]
    e, k = _coefficients(sh, 3, 19)
    base, base_tau = _trace(gh, rays, d, tree, e, k)
    stream = torch.cuda.Stream()
    ctx = gh.Context()
    try:
        ctx.make_current()
        with torch.cuda.stream(stream):
            got, got_tau = _trace(gh, rays, d, tree, e, k)
    finally:
        gh.Context.reset_current()
        ctx.destroy()
    assert np.array_equal(_bits(got), _bits(base)) and np.array_equal(_bits(got_tau), _bits(base_tau))


@pytest.mark.gpu
def test_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    rng = np.random.default_rng(41)
    s = np.empty((9000, 4), F32)
    s[:, :3] = rng.random((9000, 3), dtype=F32)
    s[:, 3] = (0.02 + 0.04 * rng.random(9000)).astype(F32)
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()                                               # tree order
    rays = gh.pinhole_camera_rays(32, 32, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0, device=cuda)
    e, k = _coefficients(sh, 5, 43)
    for name, a in (("s", sh), ("r", rays.cpu().numpy()), ("e", e), ("k", k)):
        a.tofile(str(tmp_path / (name + ".f32")))
    exe = str(tmp_path / "dropin_emission_absorption")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_emission_absorption.hip"), "-o", exe,
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    res = subprocess.run([exe, str(tmp_path / "s.f32"), str(tmp_path / "r.f32"), str(tmp_path / "e.f32"), "5",
                          str(tmp_path / "k.f32"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got, got_tau = _trace(gh, rays, d, tree, e, k)
    assert np.array_equal(_bits(got).reshape(-1), np.fromfile(str(tmp_path / "ea.f32"), np.uint32))
    assert np.array_equal(_bits(got_tau), np.fromfile(str(tmp_path / "tau.f32"), np.uint32))
