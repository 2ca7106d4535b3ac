"""Weighted, multi-channel column densities (grace_trace_cumulative_weighted_f4,
trace_cumulative_weighted_sph): out[r, c] = sum over ray r's hits i of fl32(w[i, c] * I_ri).

Expected values restate the contract in NumPy from the oracle's per-hit outputs (oracle.brute_hits:
the reference's per-hit integral, which exact mode adds): each ray's hits in ascending index, fp32
products, fp32 class sums (class (i >> 10) & 7) in ascending order, classes added pairwise."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32, F64 = np.float32, np.float64
F0 = 1.90986019771937   # the kernel table's first entry: the largest line integral times h^2


# ---- the restatement ----------------------------------------------------------------------------
def restate(n_rays, offsets, idx, integ, w):
    """(fp32 class-ordered sums, fp64 sums, fp64 sums of |w| I), each [n_rays, C]."""
    n_hits = len(idx)
    ray = np.repeat(np.arange(n_rays), np.diff(np.append(offsets, n_hits)))
    cls = (idx >> 10) & 7
    order = np.lexsort((idx, cls, ray))                  # by ray, class, ascending index
    ray, cls, idx, integ = ray[order], cls[order], idx[order], integ[order]
    group = ray * 8 + cls
    start = np.searchsorted(group, group, side="left")
    rank = np.arange(n_hits) - start
    width = int(rank.max()) + 1 if n_hits else 1
    C = w.shape[1]
    out32 = np.zeros((n_rays, C), F32)
    for c in range(C):
        terms = (w[idx, c].astype(F32) * integ.astype(F32)).astype(F32)   # fl32(w I)
        m = np.zeros((n_rays * 8, width), F32)
        m[group, rank] = terms
        acc = np.zeros(n_rays * 8, F32)
        for j in range(width):                           # ascending order within each class
            acc = (acc + m[:, j]).astype(F32)
        t = acc.reshape(n_rays, 8)
        step = 1
        while step < 8:
            for k in range(0, 8, 2 * step):
                t[:, k] = (t[:, k] + t[:, k + step]).astype(F32)
            step *= 2
        out32[:, c] = t[:, 0]
    wi = w[idx].astype(F64) * integ.astype(F64)[:, None]
    ref64 = np.zeros((n_rays, C), F64); np.add.at(ref64, ray, wi)
    abs64 = np.zeros((n_rays, C), F64); np.add.at(abs64, ray, np.abs(wi))
    return out32, ref64, abs64


# ---- CPU: the drop-in forms compile ------------------------------------------------------------------
def test_weighted_symbol_exported():
    import ctypes
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    assert hasattr(lib, "grace_trace_cumulative_weighted_f4")


def test_weighted_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_weighted"
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_weighted.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


def test_weighted_double4_is_a_clear_compile_error(tmp_path):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/trace_sph.cuh"\n'
                   "void f(const thrust::device_vector<grace::Ray>& r, const thrust::device_vector<double4>& s,\n"
                   "       const grace::Tree& t, const thrust::device_vector<float>& w,\n"
                   "       thrust::device_vector<float>& out)\n"
                   "{ grace::trace_cumulative_weighted_sph(r, s, t, w, 2, out); }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "float4 spheres only" in res.stderr


def test_weighted_mirror_compiles_with_gxx(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::Ray>& r, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::Tree& t, const grace::device_vector<float>& w)\n"
                   "{\n"
                   "    grace::device_vector<float> out(r.size() * 3);\n"
                   "    grace::trace_cumulative_weighted_sph(r, s, t, w, 3, out);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


# ---- GPU --------------------------------------------------------------------------------------------
N_SCENE = 20000   # > 8192: all eight summation classes hold spheres


def _scene(gh, cuda, n=N_SCENE, seed=3, hlo=0.01, hhi=0.05):
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


def _weights(n, C, seed, signed=True):
    rng = np.random.default_rng(seed)
    w = rng.random((n, C)).astype(F32) * F32(4.0)
    if signed:
        w = (w - F32(2.0)).astype(F32)
    else:
        w = (w + F32(0.25)).astype(F32)
    return w


def _trace(gh, rays, d, tree, w):
    import torch
    out = gh.trace_cumulative_weighted_sph(rays, d, tree, torch.from_numpy(w).to(rays.device), check=True)
    return out.cpu().numpy().reshape(len(rays), -1)


@pytest.fixture(scope="module")
def weighted_scene(gh, oracle, cuda):
    d, tree = _scene(gh, cuda)
    sh = d.cpu().numpy()
    sets = {}
    for name, rays in _ray_sets(gh, cuda).items():
        off, idx, integ, _ = oracle.brute_hits(rays.cpu().numpy(), sh)
        assert len(idx) > 0
        sets[name] = (rays, (off, idx, integ))
    return d, tree, sets


@pytest.mark.gpu
@pytest.mark.parametrize("rays_name", ["orthographic", "pinhole", "isotropic"])
def test_weighted_exact_mode_is_the_restatement_bit_for_bit(gh, weighted_scene, rays_name):
    d, tree, sets = weighted_scene
    rays, (off, idx, integ) = sets[rays_name]
    n = len(d)
    gh.set_exact_integrals(True)
    try:
        for C in (1, 2, 3, 4, 6):
            w = _weights(n, C, 100 + C)
            got = _trace(gh, rays, d, tree, w)
            ref32, _, _ = restate(len(rays), off, idx, integ, w)
            assert np.array_equal(got.view(np.uint32), ref32.view(np.uint32)), (rays_name, C)
    finally:
        gh.set_exact_integrals(False)


@pytest.mark.gpu
@pytest.mark.parametrize("rays_name", ["orthographic", "pinhole", "isotropic"])
def test_weighted_fast_mode_within_tolerance(gh, weighted_scene, rays_name):
    d, tree, sets = weighted_scene
    rays, (off, idx, integ) = sets[rays_name]
    n = len(d)
    h_min = float(d[:, 3].min())
    for C in (1, 2, 4, 6):
        w = _weights(n, C, 200 + C, signed=False)
        got = _trace(gh, rays, d, tree, w)
        _, ref64, abs64 = restate(len(rays), off, idx, integ, w)
        atol = 2e-6 * F0 / h_min ** 2 * float(np.abs(w).max())   # check_column_densities' grazing-ray term
        err = np.abs(got.astype(F64) - ref64)
        bad = np.nonzero(err > 1e-5 * abs64 + atol)
        assert len(bad[0]) == 0, (rays_name, C, bad[0][:5], got[bad][:5], ref64[bad][:5])


@pytest.mark.gpu
def test_weights_of_one_give_the_unweighted_bits(gh, weighted_scene, integral_mode, cuda):
    import torch
    d, tree, sets = weighted_scene
    ones = np.ones((len(d), 1), F32)
    for name, (rays, _) in sets.items():
        ref = torch.empty(len(rays), dtype=torch.float32, device=cuda)
        gh.trace_cumulative_sph(rays, d, tree, ref, check=True)
        got = _trace(gh, rays, d, tree, ones)[:, 0]
        assert np.array_equal(got.view(np.uint32), ref.cpu().numpy().view(np.uint32)), (name, integral_mode)
        # every channel of a multi-channel call
        got4 = _trace(gh, rays, d, tree, np.ones((len(d), 5), F32))
        for c in range(5):
            assert np.array_equal(got4[:, c].view(np.uint32), ref.cpu().numpy().view(np.uint32)), (name, c)


@pytest.mark.gpu
def test_weights_of_one_on_a_clustered_frame_take_the_lattice_path(gh, cuda, integral_mode):
    """1024^2 orthographic rays through a clustered scene with sub-pixel spheres: the lattice
    instantiation runs, and weights of one give trace_cumulative_sph's bits."""
    import math
    import torch
    g = torch.Generator(device=cuda); g.manual_seed(5)
    n, nb = 600_000, 150_000
    pos = torch.rand((nb, 3), generator=g, device=cuda)
    dens = torch.full((nb,), float(nb), device=cuda)
    n_clumps = 20; nc = n - nb
    centres = torch.rand((n_clumps, 3), generator=g, device=cuda) * 0.8 + 0.1
    sig = 10 ** (torch.rand(n_clumps, generator=g, device=cuda) * 1.2 - 2.8)
    which = torch.randint(0, n_clumps, (nc,), generator=g, device=cuda)
    p = centres[which] + torch.randn((nc, 3), generator=g, device=cuda) * sig[which, None]
    r2 = ((p - centres[which]) ** 2).sum(1) / sig[which] ** 2
    dd = (nc / n_clumps) * torch.exp(-0.5 * r2) / ((2 * math.pi) ** 1.5 * sig[which] ** 3) + nb
    pos = torch.cat([pos, p.clamp(0, 1)]); dens = torch.cat([dens, dd])
    h = (3 * 48 / (4 * math.pi * dens)) ** (1 / 3)
    s = torch.cat([pos, h[:, None]], 1).float().contiguous()
    assert float(h.min()) < 0.5 / 1024
    lo, hi = gh.min_max_vec4(s); lo[3] = hi[3] = 0
    tree = gh.Tree(n, 32, device=cuda); gh.build_tree(s, tree, lo[:3], hi[:3])
    rays, _ = gh.orthogonal_rays_z(1024, lo, hi, device=cuda)
    ref = torch.empty(len(rays), dtype=torch.float32, device=cuda)
    gh.trace_cumulative_sph(rays, s, tree, ref, check=True)
    ones = torch.ones((n, 2), dtype=torch.float32, device=cuda)
    got = gh.trace_cumulative_weighted_sph(rays, s, tree, ones, check=True)
    assert gh.last_lattice() == 1
    assert torch.equal(got[:, 0].contiguous().view(torch.int32), ref.view(torch.int32))
    assert torch.equal(got[:, 1].contiguous().view(torch.int32), ref.view(torch.int32))
    got1 = gh.trace_cumulative_weighted_sph(rays, s, tree, ones[:, 0].contiguous(), check=True)
    assert torch.equal(got1.view(torch.int32), ref.view(torch.int32))


@pytest.mark.gpu
def test_weighted_channels_are_independent(gh, weighted_scene):
    d, tree, sets = weighted_scene
    w = _weights(len(d), 6, 7)
    gh.set_exact_integrals(True)
    try:
        for name, (rays, _) in sets.items():
            all6 = _trace(gh, rays, d, tree, w)
            for c in range(6):
                one = _trace(gh, rays, d, tree, np.ascontiguousarray(w[:, c:c + 1]))[:, 0]
                assert np.array_equal(one.view(np.uint32), all6[:, c].view(np.uint32)), (name, c)
    finally:
        gh.set_exact_integrals(False)


@pytest.mark.gpu
def test_weighted_results_do_not_depend_on_the_knobs(gh, weighted_scene, integral_mode):
    d, tree, sets = weighted_scene
    w = _weights(len(d), 3, 11)
    knobs = [(gh.set_packet_split, k, -1) for k in (1, 2, 4, 8)] \
        + [(gh.set_packet_width, k, -1) for k in (64, 32, 16)] \
        + [(gh.set_treelet_size, k, -1) for k in (0, 64, 4096)] \
        + [(gh.set_ray_reorder, False, True), (gh.set_lattice_split, 0, 4), (gh.set_lattice_split, 8, 4),
           (gh.set_cache_auto, False, True)]
    for name, (rays, _) in sets.items():
        base = _trace(gh, rays, d, tree, w)
        for setter, value, default in knobs:
            setter(value)
            try:
                got = _trace(gh, rays, d, tree, w)
            finally:
                setter(default)
            assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (name, setter.__name__, value)


@pytest.mark.gpu
def test_weights_are_never_cached(gh, weighted_scene, cuda):
    import torch
    d, tree, sets = weighted_scene
    rays = sets["pinhole"][0]
    w = torch.from_numpy(_weights(len(d), 2, 13, signed=False)).to(cuda)
    ref = torch.empty(len(rays), dtype=torch.float32, device=cuda)
    first = gh.trace_cumulative_weighted_sph(rays, d, tree, w, check=True).clone()
    again = gh.trace_cumulative_weighted_sph(rays, d, tree, w, check=True).clone()   # scene cached now
    assert torch.equal(first, again)
    w.mul_(2.0)                                                    # in place, same pointer
    doubled = gh.trace_cumulative_weighted_sph(rays, d, tree, w, check=True).clone()
    assert torch.equal(doubled, first * 2.0)                      # exact: fl(2 x) = 2 fl(x)
    w[: len(d) // 2].zero_()
    halved = gh.trace_cumulative_weighted_sph(rays, d, tree, w, check=True).clone()
    assert not torch.equal(halved, doubled)
    # interleaved with unweighted calls on the same scene: both stay right
    gh.trace_cumulative_sph(rays, d, tree, ref, check=True)
    base = ref.clone()
    for _ in range(2):
        assert torch.equal(gh.trace_cumulative_weighted_sph(rays, d, tree, w, check=True), halved)
        gh.trace_cumulative_sph(rays, d, tree, ref, check=True)
        assert torch.equal(ref, base)
    ones = torch.ones(len(d), dtype=torch.float32, device=cuda)
    assert torch.equal(gh.trace_cumulative_weighted_sph(rays, d, tree, ones, check=True), base)


@pytest.mark.gpu
def test_weighted_argument_checks(gh, weighted_scene, cuda):
    import ctypes as C
    import torch
    d, tree, sets = weighted_scene
    rays = sets["pinhole"][0]
    n = len(d)
    with pytest.raises(ValueError):
        gh.trace_cumulative_weighted_sph(rays, d, tree, torch.ones((n, 0), dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        gh.trace_cumulative_weighted_sph(rays, d, tree, torch.ones((n, 65), dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        gh.trace_cumulative_weighted_sph(rays, d, tree, torch.ones(n - 1, dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        gh.trace_cumulative_weighted_sph(rays, d, tree, torch.ones(n, dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError):
        gh.trace_cumulative_weighted_sph(rays, d, tree, torch.ones((n, 2), dtype=torch.float32, device=cuda),
                                         out=torch.empty(len(rays), dtype=torch.float32, device=cuda))
    # the C ABI itself: channel count and null weights
    out = torch.empty((len(rays), 64), dtype=torch.float32, device=cuda)
    w = torch.ones((n, 64), dtype=torch.float32, device=cuda)
    args = gh._trace_args(rays, d, tree)
    for n_ch, wp in ((0, w), (65, w), (-1, w), (2, None)):
        st = gh._lib.grace_trace_cumulative_weighted_f4(*args, gh._ptr(wp), C.c_int(n_ch), gh._ptr(out), gh._stream())
        assert st == gh.GRACE_INVALID_ARGUMENT, (n_ch, wp is None)
    # 64 channels: sixteen launches, each channel the sum of the unweighted terms
    gh.trace_cumulative_weighted_sph(rays, d, tree, w, out=out, check=True)
    ref = torch.empty(len(rays), dtype=torch.float32, device=cuda)
    gh.trace_cumulative_sph(rays, d, tree, ref, check=True)
    assert torch.equal(out, ref[:, None].expand(-1, 64))
    # zero rays: a no-op
    none = torch.empty((0, 7), dtype=torch.float32, device=cuda)
    got = gh.trace_cumulative_weighted_sph(none, d, tree, torch.ones((n, 3), dtype=torch.float32, device=cuda),
                                           check=True)
    assert tuple(got.shape) == (0, 3)


@pytest.mark.gpu
def test_build_tree_returns_the_sort_permutation(gh, cuda):
    import torch
    n = 12000
    rng = np.random.default_rng(17)
    s = rng.random((n, 4)).astype(F32)
    s[:, 3] = (0.01 + 0.03 * s[:, 3]).astype(F32)
    d = torch.from_numpy(s).to(cuda)
    d2 = d.clone()
    tree, perm = gh.build_tree(d, gh.Tree(n, 32, device=cuda), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_perm=True)
    tree2 = gh.build_tree(d2, gh.Tree(n, 32, device=cuda), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    assert torch.equal(d, d2)                                         # same sort either way
    assert torch.equal(tree.nodes, tree2.nodes) and torch.equal(tree.leaves, tree2.leaves)
    p = perm.long().cpu()
    assert torch.equal(torch.from_numpy(s)[p], d.cpu())                # perm brings caller data into tree order


@pytest.mark.gpu
def test_weighted_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    import torch
    d, tree = _scene(gh, cuda, 9000, 41, 0.02, 0.06)
    s = d.cpu().numpy()                                               # tree order
    rays = gh.pinhole_camera_rays(32, 32, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0, device=cuda)
    w = _weights(len(s), 5, 43)
    s.tofile(str(tmp_path / "s.f32"))
    rays.cpu().numpy().tofile(str(tmp_path / "r.f32"))
    w.tofile(str(tmp_path / "w.f32"))
    exe = str(tmp_path / "dropin_weighted")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_weighted.hip"), "-o", exe,
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    res = subprocess.run([exe, str(tmp_path / "s.f32"), str(tmp_path / "r.f32"), str(tmp_path / "w.f32"), "5",
                          str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = _trace(gh, rays, d, tree, w)
    assert np.array_equal(got.reshape(-1).view(np.uint32), np.fromfile(str(tmp_path / "wcum.f32"), np.uint32))
