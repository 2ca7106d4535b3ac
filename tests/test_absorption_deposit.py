"""Absorbed radiation deposited on the particles (grace_trace_absorption_deposit_f4,
trace_absorption_deposit_sph).  The contract, from include/grace_hip.h: a ray's hits are those of
trace_sph (same hit test, integral I and distance d, bit for bit), ordered ascending by (d as fp32,
sphere index); then in fp64, per channel c, with L the ray's luminosity

    a_kc   = absorption[i_k, c] * I_k
    tau_kc = sum_{m<k} a_mc
    dep_kc = L[r, c] * exp(-tau_kc) * (-expm1(-a_kc))
    transmitted[r, c] = fl32( L[r, c] * exp(-sum_k a_kc) )
    deposit[i, c]     = q_c * sum over (ray, hit) with i_k == i of round-half-even( dep_kc / q_c )

with the quantum q_c = 2^(e_c + b - 62), 2^(e_c - 1) <= max_r |L[r, c]| < 2^e_c, b = ceil(log2 n_rays).
Expected values restate this in NumPy from the oracle's per-hit outputs (oracle.brute_hits): lexsort
by (ray, distance, index), fp64 cumsum per channel, np.add.at onto the spheres -- without the
quantisation, which the tolerance accounts for.

The tolerances are derived, not measured.  With m_i the number of rays that hit sphere i, n_r and
tau_rc the hits and optical depth of ray r:

    |deposit[i, c] - ref| <= m_i q_c + sum over the hits on i of 8 (n_r + 8) 2^-53 max(1, tau_rc) |dep_kc|
    |transmitted - ref|   <= spacing(fl32(|ref|)) / 2 + 8 (n_r + 8) 2^-53 max(1, tau_rc) |ref|

m_i q_c is half a unit of rounding per hit plus half a unit where a last-bit difference in exp /
expm1 moves dep / q across a rounding boundary; the other term is the fp64 bound of the
emission-absorption contract (tests/test_emission_absorption.py, bound()), applied per hit.  q_c
itself is recomputed here from the stated rule and compared exactly."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_emission_absorption import _build, _build_one, _collinear_scene, _spread, clustered_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32, F64 = np.float32, np.float64
EPS = 8.0 * 2.0 ** -53


# ---- the restatement ----------------------------------------------------------------------------
def quantum(L, n_rays):
    """q_c from the stated rule.  L: [n_rays, C] fp32."""
    M = np.abs(L).max(0).astype(F64) if len(L) else np.zeros(L.shape[1])
    _, e = np.frexp(M)                                   # M = f 2^e with 1/2 <= f < 1
    b = (n_rays - 1).bit_length() if n_rays > 0 else 0    # ceil(log2(n_rays))
    return np.where(M > 0, np.ldexp(1.0, e + b - 62), 0.0)


class Ref:
    pass


def restate(n_rays, n_spheres, offsets, idx, integ, dist, L, absorption, reverse_ties=False):
    """fp64 expected values and the parts of the bounds: .dep [n, C], .dep_err [n, C] (the fp64
    term), .m [n] (rays per sphere), .trans [n_rays, C], .trans_err [n_rays, C] (fp64 term), .tau
    [n_rays, C], .n_r [n_rays], .q [C]."""
    counts = np.diff(np.append(offsets, len(idx))).astype(np.int64)
    ray = np.repeat(np.arange(n_rays), counts)
    tie = -idx.astype(np.int64) if reverse_ties else idx.astype(np.int64)
    order = np.lexsort((tie, dist, ray))                 # by ray, distance (fp32), sphere index
    idx, I = idx[order], integ[order].astype(F64)
    C = L.shape[1]
    R = Ref()
    R.dep = np.zeros((n_spheres, C), F64); R.dep_err = np.zeros((n_spheres, C), F64)
    R.m = np.zeros(n_spheres, np.int64)
    R.trans = L.astype(F64).copy(); R.trans_err = np.zeros((n_rays, C), F64)
    R.tau = np.zeros((n_rays, C), F64); R.n_r = counts; R.q = quantum(L, n_rays)
    start = np.cumsum(counts) - counts
    for r in range(n_rays):
        if counts[r] == 0:
            continue
        sl = slice(start[r], start[r] + counts[r])
        i, Ir = idx[sl], I[sl]
        a = absorption[i].astype(F64) * Ir[:, None]
        cs = np.cumsum(a, 0)
        tau_k = np.concatenate((np.zeros((1, C)), cs[:-1]))
        Lr = L[r].astype(F64)
        dep = Lr * np.exp(-tau_k) * -np.expm1(-a)
        f = EPS * (counts[r] + 8.0) * np.maximum(1.0, cs[-1])
        np.add.at(R.dep, i, dep)
        np.add.at(R.dep_err, i, f * np.abs(dep))
        np.add.at(R.m, i, 1)
        R.tau[r] = cs[-1]
        R.trans[r] = Lr * np.exp(-cs[-1])
        R.trans_err[r] = f * np.abs(R.trans[r])
    return R


def deposit_bound(R):
    return R.m[:, None] * R.q[None, :] + R.dep_err


def transmitted_bound(R):
    return np.spacing(np.abs(R.trans).astype(F32)).astype(F64) / 2 + R.trans_err


def check(got, R, what=""):
    dep, trans, q = got
    assert np.array_equal(q.view(np.uint64), R.q.view(np.uint64)), (what, q, R.q)
    err, tol = np.abs(dep - R.dep), deposit_bound(R)
    terr, ttol = np.abs(trans.astype(F64) - R.trans), transmitted_bound(R)
    ok = tol > 0
    print("%s: deposit max err/tol %.3g (max |ref| %.3g, hit spheres %d); transmitted max err/tol %.3g; "
          "tau range %.3g..%.3g" % (what, float(np.max(err[ok] / tol[ok])) if ok.any() else 0.0,
                                    float(np.abs(R.dep).max()), int((R.m > 0).sum()),
                                    float(np.max(terr / ttol)) if terr.size else 0.0,
                                    float(R.tau.min()) if R.tau.size else 0.0,
                                    float(R.tau.max()) if R.tau.size else 0.0))
    bad = np.argwhere(~(err <= tol))
    assert len(bad) == 0, (what, "deposit", bad[:5], dep[tuple(bad[0])], R.dep[tuple(bad[0])])
    bad = np.argwhere(~(terr <= ttol))
    assert len(bad) == 0, (what, "transmitted", bad[:5], trans[tuple(bad[0])], R.trans[tuple(bad[0])])
    assert np.all(dep[R.m == 0] == 0) and not np.any(np.signbit(dep[R.m == 0]))     # +0.0 where nobody hits
    none = R.n_r == 0                                                                # no hits: L unchanged
    assert np.array_equal(trans[none].view(np.uint32), R.trans[none].astype(F32).view(np.uint32))


# ---- CPU: exported, and the drop-in forms compile -------------------------------------------------
def test_entry_point_is_exported():
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    assert hasattr(lib, "grace_trace_absorption_deposit_f4")


def test_python_function_exists():
    import grace_hip
    assert callable(grace_hip.trace_absorption_deposit_sph)


def _compile_dropin(tmp_path):
    exe = tmp_path / "dropin_absorption_deposit"
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_absorption_deposit.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def test_dropin_compiles_with_hipcc(tmp_path):
    assert _compile_dropin(tmp_path).exists()


def test_mirror_compiles_with_gxx(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::Ray>& r, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::Tree& t, const grace::device_vector<float>& l, const grace::device_vector<float>& k)\n"
                   "{\n"
                   "    grace::device_vector<double> dep(s.size() * 3), q(3);\n"
                   "    grace::device_vector<float> tr(r.size() * 3);\n"
                   "    grace::trace_absorption_deposit_sph(r, s, t, l, 3, k, dep);\n"
                   "    grace::trace_absorption_deposit_sph(r, s, t, l, 3, k, dep, &tr);\n"
                   "    grace::trace_absorption_deposit_sph(r, s, t, l, 3, k, dep, &tr, &q);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


# ---- GPU --------------------------------------------------------------------------------------------
N_SCENE = 20000


def _coefficients(sh, n_rays, C, seed):
    """Luminosities of both signs spanning three decades; absorption ~ 1e-3 h^2 rising 3.5 decades
    along x (per channel within +-25 %), so that with I ~ 1/h^2 the optical depth of a ray spans
    roughly 0.01 to 30 across an image."""
    rng = np.random.default_rng(seed)
    L = (10.0 ** (3.0 * rng.random((n_rays, C))) * np.where(rng.random((n_rays, C)) < 0.5, -1.0, 1.0)).astype(F32)
    k = (6e-4 * sh[:, 3].astype(F64) ** 2 * 10.0 ** (3.5 * sh[:, 0].astype(F64))
         * (0.5 + rng.random(len(sh))))[:, None] * (0.75 + 0.5 * rng.random((1, C)))
    return L, k.astype(F32)


def _trace(gh, rays, d, tree, L, k, want=True):
    """(deposit [n, C] fp64, transmitted [n_rays, C] fp32, quantum [C] fp64) as NumPy arrays."""
    import torch
    dev = rays.device
    C = L.shape[1]
    tr = torch.empty((len(rays), C), dtype=torch.float32, device=dev) if want else None
    q = torch.empty(C, dtype=torch.float64, device=dev) if want else None
    dep = gh.trace_absorption_deposit_sph(rays, d, tree, torch.from_numpy(np.ascontiguousarray(L)).to(dev),
                                          torch.from_numpy(np.ascontiguousarray(k)).to(dev),
                                          transmitted=tr, quantum=q, check=True)
    assert dep.dtype == torch.float64 and tuple(dep.shape) == (len(d), C)
    return dep.cpu().numpy(), (tr.cpu().numpy() if want else None), (q.cpu().numpy() if want else None)


@pytest.fixture(autouse=True)
def _knobs_reset(request):
    yield
    if "gh" in request.fixturenames:
        gh = request.getfixturevalue("gh")
        gh.set_ordered_budget(0); gh.ordered_enable_stats(False)
        gh.set_packet_width(-1); gh.set_sph_kernel("cubic")


@pytest.fixture(scope="module")
def ad_scene(gh, oracle, cuda):
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
def test_random_scenes_match_the_restatement(gh, ad_scene, rays_name, C):
    d, tree, sh, sets = ad_scene
    rays, (off, idx, integ, dist) = sets[rays_name]
    L, k = _coefficients(sh, len(rays), C, 100 + C)
    assert (L > 0).any() and (L < 0).any() and np.abs(L).max() / np.abs(L).min() > 500.0
    got = _trace(gh, rays, d, tree, L, k)
    R = restate(len(rays), len(sh), off, idx, integ, dist, L, k)
    if rays_name in ("orthographic", "pinhole"):     # thin and thick rays in one image
        hit = R.tau[R.n_r > 0]
        assert hit.min() < 0.1 and hit.max() > 10.0, (hit.min(), hit.max())
    check(got, R, "%s C=%d" % (rays_name, C))


@pytest.mark.gpu
@pytest.mark.parametrize("rays_name", RAY_SETS)
def test_photons_are_conserved(gh, ad_scene, rays_name):
    """sum_i deposit + sum_r transmitted = sum_r L per channel, within the sum of the per-element
    bounds (each output is within its bound of an exact value, and the exact values telescope:
    L e^-tau_k (1 - e^-a_k) = L e^-tau_k - L e^-tau_(k+1)); the fp64 sums of up to 22304 terms
    add 22304 2^-53 of the terms' magnitudes."""
    d, tree, sh, sets = ad_scene
    rays, (off, idx, integ, dist) = sets[rays_name]
    L, k = _coefficients(sh, len(rays), 3, 31)
    dep, trans, q = _trace(gh, rays, d, tree, L, k)
    R = restate(len(rays), len(sh), off, idx, integ, dist, L, k)
    total = dep.sum(0) + trans.astype(F64).sum(0)
    n_terms = len(sh) + len(rays)
    tol = deposit_bound(R).sum(0) + transmitted_bound(R).sum(0) \
        + n_terms * 2.0 ** -53 * (np.abs(dep).sum(0) + np.abs(trans.astype(F64)).sum(0) + np.abs(L.astype(F64)).sum(0))
    err = np.abs(total - L.astype(F64).sum(0))
    print("%s: conservation err/tol %s, absorbed share %s" % (
        rays_name, err / tol, np.abs(dep).sum(0) / np.abs(L.astype(F64)).sum(0)))
    assert np.all(err <= tol), (err, tol)
    L1 = np.abs(L)                                      # one sign: nothing cancels, the shares are fractions
    dep, trans, q = _trace(gh, rays, d, tree, L1, k)
    assert np.all(dep >= 0) and np.all(trans >= 0) and np.all(trans <= L1)
    R = restate(len(rays), len(sh), off, idx, integ, dist, L1, k)
    err = np.abs(dep.sum(0) + trans.astype(F64).sum(0) - L1.astype(F64).sum(0))
    tol = deposit_bound(R).sum(0) + transmitted_bound(R).sum(0) + 3 * n_terms * 2.0 ** -53 * L1.astype(F64).sum(0)
    assert np.all(err <= tol), (err, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("rays_name", RAY_SETS)
def test_random_scenes_with_a_wendland_kernel(gh, ad_scene, rays_name):
    from test_sph_kernels import b2_f32, hit_rays, integrals_f32   # the per-hit arithmetic, restated there
    d, tree, sh, sets = ad_scene
    rays, (off, idx, _, dist) = sets[rays_name]
    rh = rays.cpu().numpy()
    integ = integrals_f32(b2_f32(rh, sh, hit_rays(off, len(idx)), idx), sh[idx, 3],
                          gh.sph_kernel_table("wendland_c2"))
    gh.set_sph_kernel("wendland_c2")
    L, k = _coefficients(sh, len(rays), 3, 7)
    got = _trace(gh, rays, d, tree, L, k)
    check(got, restate(len(rays), len(sh), off, idx, integ, dist, L, k), "%s wendland_c2" % rays_name)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.gpu
def test_results_are_bitwise_invariant(gh, ad_scene, cuda):
    import torch
    d, tree, sh, sets = ad_scene
    rays, (off, idx, integ, dist) = sets["pinhole"]
    L, k = _coefficients(sh, len(rays), 5, 11)
    gh.ordered_enable_stats(True)
    base = _trace(gh, rays, d, tree, L, k)
    st = gh.ordered_last_stats()
    assert st["batches"] == 1 and st["total_hits"] == len(idx)
    same = lambda got: _same(got[0], base[0]) and _same(got[1], base[1]) and _same(got[2], base[2])
    assert same(_trace(gh, rays, d, tree, L, k))                           # two runs in a row
    gh.set_ordered_budget(64 << 10)                                        # many batches
    assert same(_trace(gh, rays, d, tree, L, k))
    assert gh.ordered_last_stats()["batches"] >= 5
    gh.set_ordered_budget(0)
    for width in (64, 32, 16):
        gh.set_packet_width(width)
        assert same(_trace(gh, rays, d, tree, L, k)), width
    gh.set_packet_width(-1)
    # the rays in another order, L alike: transmitted moves with the rays, the deposit does not move
    # at all -- what a floating-point atomic sum would fail
    perms = [np.arange(len(rays))[::-1].copy(),
             torch.randperm(len(rays), generator=torch.Generator().manual_seed(3)).numpy()]
    for p in perms:
        got = _trace(gh, rays[torch.from_numpy(p).to(cuda)].contiguous(), d, tree, L[p], k)
        assert _same(got[0], base[0]) and _same(got[1], base[1][p]) and _same(got[2], base[2])
    gh.set_ordered_budget(64 << 10)                                        # ... and batched as well
    got = _trace(gh, rays[torch.from_numpy(perms[1]).to(cuda)].contiguous(), d, tree, L[perms[1]], k)
    assert _same(got[0], base[0]) and _same(got[1], base[1][perms[1]])
    gh.set_ordered_budget(0)
    dep, none, _ = _trace(gh, rays, d, tree, L, k, want=False)             # the optional outputs are optional
    assert none is None and _same(dep, base[0])
    stream = torch.cuda.Stream()                                           # a context with its own stream
    ctx = gh.Context()
    try:
        ctx.make_current()
        with torch.cuda.stream(stream):
            got = _trace(gh, rays, d, tree, L, k)
    finally:
        gh.Context.reset_current()
        ctx.destroy()
    assert same(got)


def _lattice(gh, oracle, cuda):
    g = 12; sp = 1.0 / g
    x = (np.arange(g) + 0.5) * sp
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    s = np.stack([X.ravel(), Y.ravel(), Z.ravel(), np.full(g ** 3, 1.3 * sp)], 1).astype(F32)
    rng = np.random.default_rng(1)
    s = s[rng.permutation(len(s))]
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()
    rays_h, _ = oracle.orthogonal_rays_z(16, (0, 0, 0, 0), (1, 1, 1, 0))
    return d, tree, sh, rays_h, rng


@pytest.mark.gpu
def test_ties_are_broken_by_ascending_index(gh, oracle, cuda):
    """12^3 lattice, rays along z: every ray has hits at bit-equal distance, and the other
    tie-break gives other deposits -- asserted first, so the scene cannot stop testing it."""
    import torch
    d, tree, sh, rays_h, rng = _lattice(gh, oracle, cuda)
    n = len(rays_h)
    off, idx, integ, dist = oracle.brute_hits(rays_h, sh)
    ray = np.repeat(np.arange(n), np.diff(np.append(off, len(idx))))
    key = ray.astype(np.int64) * (1 << 32) + dist.view(np.uint32)
    u, c = np.unique(key, return_counts=True)
    assert len(np.unique(u[c > 1] >> 32)) == n                   # every ray has tied hits
    L = (0.5 + rng.random((n, 3))).astype(F32)
    k = (rng.random((len(sh), 3)) * 0.004).astype(F32)            # tau of a ray: 2..6
    R = restate(n, len(sh), off, idx, integ, dist, L, k)
    other = restate(n, len(sh), off, idx, integ, dist, L, k, reverse_ties=True)
    moved = np.abs(other.dep - R.dep) > 2.0 * deposit_bound(R)  # outside both answers' bounds
    assert np.all(R.m > 0) and np.all(moved)                     # ... and the tie-break matters for every sphere
    rays = torch.from_numpy(np.ascontiguousarray(rays_h).view(F32).reshape(n, 7)).to(cuda)
    check(_trace(gh, rays, d, tree, L, k), R, "lattice")


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
    L = ((rng.random((len(counts), 5)) - 0.5) * 8).astype(F32)
    k = (rng.random((len(sh), 5)) * 2e-6).astype(F32)                     # I ~ 1.9e4: a ~ 0.02 per hit
    gh.ordered_enable_stats(True)
    got = _trace(gh, rays, d, tree, L, k)
    st = gh.ordered_last_stats()
    c = np.array(counts)
    assert st["rays_wave"] == np.sum(c <= w) and st["rays_block"] == np.sum((c > w) & (c <= b))
    assert st["rays_global"] == np.sum(c > b) == 2 and st["total_hits"] == c.sum()
    check(got, restate(len(rays), len(sh), off, idx, integ, dist, L, k), "tier edges")
    # the same rays in batches: a ray longer than the budget is a batch of its own
    gh.set_ordered_budget(12 * (b + 1))
    again = _trace(gh, rays, d, tree, L, k)
    assert gh.ordered_last_stats()["batches"] > 5
    assert _same(again[0], got[0]) and _same(again[1], got[1]) and _same(again[2], got[2])


def _one_ray(cuda, x, y):
    """32 rays along z (ray counts are multiples of 32): ray 0 through (x, y), 31 far outside the box."""
    import torch
    rays = np.zeros((32, 7), F32)
    rays[:] = (0, 0, 1, x, y, -0.1, 1.2)
    rays[1:, 3] += 10.0
    return torch.from_numpy(rays).to(cuda)


@pytest.mark.gpu
def test_closed_forms(gh, oracle, cuda, ad_scene):
    d, tree = _build_one(gh, cuda, np.array([[0.5, 0.5, 0.5, 0.2]], F32))
    sh = d.cpu().numpy()
    me = int(np.nonzero(sh[:, 3] == F32(0.2))[0][0])
    rays = _one_ray(cuda, 0.55, 0.5)
    off, idx, integ, dist = oracle.brute_hits(rays.cpu().numpy(), sh)
    assert len(idx) == 1 and idx[0] == me and off[1] == 1                 # one sphere, one ray
    L = np.zeros((32, 3), F32); L[0] = (3.0, -1.5, 0.0); L[1:, 0] = 0.25  # channel 2 carries nothing
    k = np.zeros((len(sh), 3), F32); k[:] = (0.25, 2.0, 1.0)
    dep, trans, q = _trace(gh, rays, d, tree, L, k)
    a = k[me].astype(F64) * F64(integ[0])
    assert np.array_equal(q.view(np.uint64), quantum(L, 32).view(np.uint64)) and q[2] == 0 and np.all(q[:2] > 0)
    ref_dep, ref_tr = L[0].astype(F64) * -np.expm1(-a), L[0].astype(F64) * np.exp(-a)
    assert np.all(np.abs(dep[me] - ref_dep) <= q + EPS * 9 * np.maximum(1, a) * np.abs(ref_dep)), (dep[me], ref_dep)
    assert np.all(np.abs(trans[0] - ref_tr) <= np.spacing(np.abs(ref_tr).astype(F32)) / 2
                  + EPS * 9 * np.maximum(1, a) * np.abs(ref_tr)), (trans[0], ref_tr)
    assert dep[me, 2] == 0 and trans[0, 2] == 0 and dep[me, 0] > 0 > dep[me, 1]
    rest = np.arange(len(sh)) != me
    assert np.all(dep[rest] == 0) and not np.any(np.signbit(dep[rest]))
    assert _same(trans[1:], L[1:])                                         # rays without hits transmit L
    # zero absorption on a full scene: nothing deposited, everything transmitted, bit for bit
    d, tree, sh, sets = ad_scene
    rays, _ = sets["orthographic"]
    L, k = _coefficients(sh, len(rays), 3, 13)
    dep, trans, q = _trace(gh, rays, d, tree, L, np.zeros_like(k))
    assert np.all(dep == 0) and _same(trans, L)
    # L == 0 in one channel: its quantum is 0, its outputs zero, the other channels as they were
    base = _trace(gh, rays, d, tree, L, k)
    L0 = L.copy(); L0[:, 1] = 0
    dep, trans, q = _trace(gh, rays, d, tree, L0, k)
    assert q[1] == 0 and np.all(dep[:, 1] == 0) and np.all(trans[:, 1] == 0)
    for c in (0, 2):
        assert _same(dep[:, c], base[0][:, c]) and _same(trans[:, c], base[1][:, c]) and q[c] == base[2][c]


@pytest.mark.gpu
def test_quantisation_floor(gh, oracle, cuda):
    """40 collinear spheres of optical depth 3 each: tau in front of sphere k is 3 k.  A hit that
    absorbs less than q / 2 deposits exactly nothing: here q = 2^(1 + 5 - 62) (L = 1, 32 rays), so
    every sphere behind tau >= 60 (e^-60 < 2^-86) gets 0.0, and those in front of tau <= 30
    (e^-30 (1 - e^-3) > 2^-44) a finite positive value; L e^-120 underflows fp32 to zero."""
    counts = [40] + [0] * 31
    rays, s = _collinear_scene(counts, cuda)
    d, tree = _build_one(gh, cuda, s)                                      # (padding: a tree needs > 32 spheres)
    sh = d.cpu().numpy()
    off, idx, integ, dist = oracle.brute_hits(rays.cpu().numpy(), sh)
    assert np.array_equal(np.diff(np.append(off, len(idx))), counts)
    assert np.all(integ == integ[0])                                       # all hits central: one integral
    L = np.ones((32, 1), F32)
    k = np.full((len(sh), 1), 3.0 / F64(integ[0])).astype(F32)
    dep, trans, q = _trace(gh, rays, d, tree, L, k)
    R = restate(32, len(sh), off, idx, integ, dist, L, k)
    assert q[0] == 2.0 ** -56
    order = idx[np.argsort(dist, kind="stable")]                           # (distances are distinct)
    tau_front = R.tau[0, 0] / 40 * np.arange(40)
    assert abs(R.tau[0, 0] - 120.0) < 1e-3
    behind, front = order[tau_front >= 60.0], order[tau_front <= 30.0]
    assert len(behind) >= 19 and len(front) >= 10
    assert np.all(dep[behind, 0] == 0.0) and np.all(R.dep[behind, 0] > 0)  # absorbed in exact arithmetic, below the floor
    assert np.all(np.isfinite(dep)) and np.all(dep[front, 0] > 0)
    check((dep, trans, q), R, "floor")
    assert np.all(np.isfinite(trans)) and trans[0, 0] == 0.0 and 0 < R.trans[0, 0] < 1e-50


@pytest.mark.gpu
def test_argument_checks(gh, ad_scene, cuda):
    import torch
    d, tree, sh, sets = ad_scene
    rays, _ = sets["healpix"]
    n, m = len(sh), len(rays)
    args = gh._trace_args(rays, d, tree)
    call = lambda a, lum, ab, C, dep, tr=None, q=None: gh._lib.grace_trace_absorption_deposit_f4(
        *a, gh._ptr(lum), gh._ptr(ab), ctypes.c_int(C), gh._ptr(dep), gh._ptr(tr), gh._ptr(q), gh._stream())
    L2 = torch.ones((m, 2), device=cuda); k2 = torch.zeros((n, 2), device=cuda)
    dep = torch.full((n, 2), 7.0, dtype=torch.float64, device=cuda)
    for C in (0, 65, -1):
        assert call(args, L2, k2, C, dep) == gh.GRACE_INVALID_ARGUMENT
    assert call(args, L2, k2, 2, None) == gh.GRACE_INVALID_ARGUMENT
    assert call(args, None, k2, 2, dep) == gh.GRACE_INVALID_ARGUMENT
    assert call(args, L2, None, 2, dep) == gh.GRACE_INVALID_ARGUMENT
    too_many = (args[0], ctypes.c_size_t(1 << 31)) + args[2:]
    assert call(too_many, L2, k2, 2, dep) == gh.GRACE_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.all(dep == 7.0)                                           # ... each before any launch
    q = torch.full((2,), 7.0, dtype=torch.float64, device=cuda)
    empty = (args[0], ctypes.c_size_t(0)) + args[2:]
    assert call(empty, L2, k2, 2, dep, None, q) == gh.GRACE_OK             # zero rays: the deposit is zeroed
    torch.cuda.synchronize()
    assert torch.all(dep == 0) and torch.all(q == 0)
    # overwritten, not added to: a buffer full of NaN comes back finite
    dep.fill_(float("nan"))
    out = gh.trace_absorption_deposit_sph(rays, d, tree, L2, k2 + 1e-4, deposit=dep, check=True)
    assert out is dep and bool(torch.all(torch.isfinite(dep))) and float(dep.sum()) > 0
    one = gh.trace_absorption_deposit_sph(rays, d, tree, L2[:, 0].contiguous(), k2[:, 0].contiguous() + 1e-4)
    assert tuple(one.shape) == (n,) and torch.equal(one, dep[:, 0])       # 1-d in, 1-d out
    bad = [dict(luminosity=torch.ones((m, 65), device=cuda), absorption=torch.zeros((n, 65), device=cuda)),
           dict(luminosity=torch.ones((m, 0), device=cuda), absorption=torch.zeros((n, 0), device=cuda)),
           dict(luminosity=L2[:-1], absorption=k2), dict(luminosity=L2, absorption=k2[:-1]),
           dict(luminosity=L2, absorption=k2[:, 0].contiguous()), dict(luminosity=L2.double(), absorption=k2),
           dict(luminosity=L2, absorption=k2, deposit=dep[:-1]),
           dict(luminosity=L2, absorption=k2, deposit=dep.float()),
           dict(luminosity=L2, absorption=k2, transmitted=torch.zeros((m, 3), device=cuda)),
           dict(luminosity=L2, absorption=k2, quantum=torch.zeros(3, dtype=torch.float64, device=cuda))]
    for kw in bad:
        with pytest.raises(ValueError):
            gh.trace_absorption_deposit_sph(rays, d, tree, kw.pop("luminosity"), kw.pop("absorption"), **kw)


@pytest.mark.gpu
def test_values_outside_the_domain_do_not_fault(gh, ad_scene, cuda):
    """Negative absorption, infinite and NaN inputs: the affected channels are unspecified, the
    call returns, and a channel of its own stays exact."""
    d, tree, sh, sets = ad_scene
    rays, (off, idx, integ, dist) = sets["healpix"]
    L, k = _coefficients(sh, len(rays), 4, 53)
    base = _trace(gh, rays, d, tree, L, k)
    Lb, kb = L.copy(), k.copy()
    kb[:, 0] = -50.0 * kb[:, 0]; kb[::7, 1] = np.nan; kb[::5, 1] = np.inf
    Lb[3, 2] = np.inf; Lb[5, 2] = np.nan
    dep, trans, q = _trace(gh, rays, d, tree, Lb, kb)
    assert _same(dep[:, 3], base[0][:, 3]) and _same(trans[:, 3], base[1][:, 3]) and q[3] == base[2][3]


@pytest.mark.gpu
def test_more_hits_than_int32_can_index(gh, oracle, cuda):
    """1024^2 orthographic rays over 2 x 10^6 uniform particles: ~2.3e9 hits (the scene of
    test_emission_absorption's test of the same name).  Conservation over the whole call, and two
    spheres against the restatement on all the rays that can meet them."""
    import torch
    n = 2_000_000
    rng = np.random.default_rng(23)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = (0.0175 + 0.0025 * rng.random(n)).astype(F32)
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()
    rays = gh.orthogonal_rays_z(1024, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    m = len(rays)
    L = (0.5 + rng.random((m, 2))).astype(F32)
    k = ((1e-3 * sh[:, 3].astype(F64) ** 2 * 10.0 ** (1.5 * sh[:, 0]))[:, None] * np.array([[1.0, 0.3]])).astype(F32)
    gh.ordered_enable_stats(True)
    dep, trans, q = _trace(gh, rays, d, tree, L, k)
    st = gh.ordered_last_stats()
    print("beyond int32:", st)
    assert st["total_hits"] > 2 ** 31 and st["batches"] > 1
    assert np.array_equal(q.view(np.uint64), quantum(L, m).view(np.uint64))
    assert np.all(dep >= 0) and np.all(trans >= 0) and np.all(trans <= L)
    # conservation: every hit within q of its exact share and within the fp64 bound (n_r <= 8000,
    # tau <= 100: 8 * 8008 * 100 * 2^-53 < 1e-9 relative), transmitted within 2^-24 relative
    Lsum = L.astype(F64).sum(0)
    err = np.abs(dep.sum(0) + trans.astype(F64).sum(0) - Lsum)
    tol = st["total_hits"] * q + (1e-9 + 2.0 ** -24 + 3 * (n + m) * 2.0 ** -53) * Lsum
    print("beyond int32: conservation err %s tol %s, absorbed share %s" % (err, tol, dep.sum(0) / Lsum))
    assert np.all(err <= tol) and np.all(dep.sum(0) > 0.2 * Lsum)
    rh = rays.cpu().numpy()
    for i in (123456, 1777777):
        near = np.nonzero((rh[:, 3] - sh[i, 0]) ** 2 + (rh[:, 4] - sh[i, 1]) ** 2 <= (1.01 * sh[i, 3]) ** 2)[0]
        # (spheres those rays can meet: h <= 0.02; a subset in array order keeps the tie-break)
        cand = np.nonzero((sh[:, 0] - sh[i, 0]) ** 2 + (sh[:, 1] - sh[i, 1]) ** 2 <= (1.01 * sh[i, 3] + 0.0201) ** 2)[0]
        off, idx, integ, dist = oracle.brute_hits(rh[near], sh[cand])
        R = restate(len(near), n, off, cand[idx], integ, dist, L[near], k)
        R.q = q
        assert R.m[i] > 100
        err, tol = np.abs(dep[i] - R.dep[i]), deposit_bound(R)[i]
        print("beyond int32: sphere %d hit by %d rays, err/tol %s" % (i, R.m[i], err / tol))
        assert np.all(err <= tol), (i, dep[i], R.dep[i])
        terr = np.abs(trans[near].astype(F64) - R.trans)
        assert np.all(terr <= transmitted_bound(R))
    # ... and what 64 rays spread over the image transmit, against the restatement
    sub = _spread(m, 64)
    _check_transmitted(oracle, rh[sub], sh, L[sub], k, trans[sub], "beyond int32", least=1000)


def _check_transmitted(oracle, rays_h, sh, L, k, trans, what, least=1):
    """transmitted of some of a call's rays against the restatement (the deposit needs all rays)."""
    off, idx, integ, dist = oracle.brute_hits(rays_h, sh)
    R = restate(len(rays_h), len(sh), off, idx, integ, dist, L, k)
    assert R.n_r.min() >= least
    terr, ttol = np.abs(trans.astype(F64) - R.trans), transmitted_bound(R)
    print("%s: transmitted max err/tol %.3g; tau range %.3g..%.3g" % (what, float(np.max(terr / ttol)),
                                                                      float(R.tau.min()), float(R.tau.max())))
    assert np.all(terr <= ttol), (what, np.argwhere(~(terr <= ttol))[:5])


@pytest.mark.gpu
def test_more_batches_than_the_first_table_copy_holds(gh, oracle, ad_scene, cuda):
    """Budget 1 on 72^2 = 5184 rays that all hit: more batches than the first read of the batch
    table holds (this translation unit's copy of the sequence).  The bits of the single-batch
    call; transmitted against the restatement on a sample."""
    import torch
    d, tree, sh, _ = ad_scene
    rays = gh.orthogonal_rays_z(72, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    counts = torch.empty(len(rays), dtype=torch.int32, device=cuda)
    gh.trace_hitcounts_sph(rays, d, tree, counts, check=True)
    assert len(rays) >= 4200 and int(counts.min()) > 0
    L, k = _coefficients(sh, len(rays), 3, 29)
    gh.ordered_enable_stats(True)
    base = _trace(gh, rays, d, tree, L, k)
    assert gh.ordered_last_stats()["batches"] == 1
    gh.set_ordered_budget(1)
    got = _trace(gh, rays, d, tree, L, k)
    st = gh.ordered_last_stats()
    assert st["batches"] == len(rays) > 4088 and st["total_hits"] == int(counts.long().sum())
    assert _same(got[0], base[0]) and _same(got[1], base[1]) and _same(got[2], base[2])
    sub = _spread(len(rays), 128)
    _check_transmitted(oracle, rays.cpu().numpy()[sub], sh, L[sub], k, got[1][sub], "5184 batches")
    assert float(np.abs(got[0]).sum()) > 0


@pytest.mark.gpu
def test_a_call_whose_rays_hit_nothing(gh, ad_scene, cuda):
    """No hit in the whole call: nothing deposited (+0.0), every luminosity transmitted bit for
    bit, and the next ordinary call is what it was."""
    d, tree, sh, sets = ad_scene
    rays, (off, idx, _, _) = sets["healpix"]
    L, k = _coefficients(sh, len(rays), 5, 37)
    before = _trace(gh, rays, d, tree, L, k)
    away = rays.clone()
    away[:, 3:6] += 10.0                                                   # length 1, ten box lengths off
    gh.ordered_enable_stats(True)
    dep, trans, q = _trace(gh, away.contiguous(), d, tree, L, k)
    st = gh.ordered_last_stats()
    assert st["total_hits"] == 0 and st["batches"] == 1
    assert not np.any(dep.view(np.uint64)) and _same(trans, L)
    assert np.array_equal(q.view(np.uint64), quantum(L, len(rays)).view(np.uint64))
    after = _trace(gh, rays, d, tree, L, k)
    assert gh.ordered_last_stats()["total_hits"] == len(idx) > 0
    assert _same(after[0], before[0]) and _same(after[1], before[1]) and _same(after[2], before[2])


@pytest.mark.gpu
def test_one_batch_of_4096_packets_on_a_clustered_scene(gh, oracle, cuda):
    """512^2 rays in one batch: 4096 packets of 64, from where on the nested per-hit walk is the
    one-wave variant that stages in LDS.  Transmitted against the restatement on 256 sampled
    rays; photons conserved over the whole call within test_more_hits_than_int32_can_index's bound."""
    d, tree = _build(gh, cuda, clustered_scene(20000, 47))
    sh = d.cpu().numpy()
    rays = gh.orthogonal_rays_z(512, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    m, n = len(rays), len(sh)
    rng = np.random.default_rng(59)
    L = (0.5 + rng.random((m, 2))).astype(F32)
    k = _coefficients(sh, 1, 2, 53)[1]
    gh.ordered_enable_stats(True)
    dep, trans, q = _trace(gh, rays, d, tree, L, k)
    st = gh.ordered_last_stats()
    assert st["batches"] == 1 and m // 64 >= 4096
    sub = _spread(m, 256)
    _check_transmitted(oracle, rays.cpu().numpy()[sub], sh, L[sub], k, trans[sub], "4096 packets")
    # every hit within q of its exact share and within the fp64 bound (n_r <= n = 20000, tau <= 1000:
    # 8 * 20008 * 1000 * 2^-53 < 2e-8 relative), transmitted within 2^-24 relative
    Lsum = L.astype(F64).sum(0)
    err = np.abs(dep.sum(0) + trans.astype(F64).sum(0) - Lsum)
    tol = st["total_hits"] * q + (2e-8 + 2.0 ** -24 + 3 * (n + m) * 2.0 ** -53) * Lsum
    assert np.all(err <= tol) and np.all(dep >= 0) and np.all(dep.sum(0) > 0.05 * Lsum), (err, tol)


@pytest.mark.gpu
def test_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    rng = np.random.default_rng(41)
    s = np.empty((9000, 4), F32)
    s[:, :3] = rng.random((9000, 3), dtype=F32)
    s[:, 3] = (0.02 + 0.04 * rng.random(9000)).astype(F32)
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()                                               # tree order
    nside = 8
    rays = gh.healpix_rays(nside, (0.45, 0.55, 0.5), 1.0, device=cuda)
    L, k = _coefficients(sh, len(rays), 5, 43)
    for name, a in (("s", sh), ("l", L), ("k", k)):
        a.tofile(str(tmp_path / (name + ".f32")))
    exe = str(_compile_dropin(tmp_path))
    res = subprocess.run([exe, str(tmp_path / "s.f32"), str(nside), str(tmp_path / "l.f32"), "5",
                          str(tmp_path / "k.f32")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr
    lines = res.stdout.split("\n")
    words = lambda tag: np.array([int(x[2:], 16) for x in lines if x.startswith(tag + " ")], np.uint64)
    dep, trans, q = _trace(gh, rays, d, tree, L, k)
    assert np.array_equal(q.view(np.uint64), words("q"))
    assert np.array_equal(dep.view(np.uint64).reshape(-1), words("d"))
    assert np.array_equal(trans.view(np.uint32).reshape(-1).astype(np.uint64), words("t"))
    assert dep.sum() != 0
