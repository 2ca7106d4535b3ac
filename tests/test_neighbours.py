"""Nearest neighbours and smoothing lengths (grace_nearest_neighbours_f4 / grace_smoothing_lengths_f4,
nearest_neighbours_sph / smoothing_lengths_sph), and read_gadget_particles.

Expected values restate the contract of include/grace_hip.h in NumPy: d2 in float32 in the stated
order fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)), spheres ranked by (d2, tree index) with np.lexsort,
the first k kept, -1 / +inf padding, and h = fl(eta * sqrt(d2 of slot k-1))."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32 = np.float32
KERNELS = ("cubic", "quartic", "quintic", "wendland_c2", "wendland_c4", "wendland_c6")
INF = F32(np.inf)


# ---- the restatement ----------------------------------------------------------------------------
def d2_rows(p, x):
    """fp32 d2 of points p [m, 3] to centres x [n, 3], in the stated operation order."""
    dx = (p[:, None, 0] - x[None, :, 0]).astype(F32)
    dy = (p[:, None, 1] - x[None, :, 1]).astype(F32)
    dz = (p[:, None, 2] - x[None, :, 2]).astype(F32)
    return ((dx * dx + dy * dy) + dz * dz).astype(F32)


def brute_knn(points, spheres, k):
    """(indices int32 [m, k], d2 float32 [m, k]) of the stated ranking."""
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    n = len(X)
    idx = np.full((len(P), k), -1, np.int32)
    dd = np.full((len(P), k), INF, F32)
    finite = np.all(np.isfinite(P), axis=1)
    kk = min(k, n)
    chunk = max(1, min(64, (1 << 22) // max(n, 1)))   # rows per pass: a few M distances at a time
    for a in range(0, len(P), chunk):
        d2 = d2_rows(P[a:a + chunk], X)
        kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
        for r in range(len(d2)):
            if not finite[a + r]:
                continue
            cand = np.nonzero(d2[r] <= kth[r])[0]           # every candidate that ties the k-th too
            order = np.lexsort((cand, d2[r, cand]))[:kk]
            idx[a + r, :kk] = cand[order]
            dd[a + r, :kk] = d2[r, cand[order]]
    return idx, dd


def brute_h(spheres, k, eta, rows=None):
    rows = np.arange(len(spheres)) if rows is None else rows
    _, d2 = brute_knn(spheres[rows], spheres, k)
    return (F32(eta) * np.sqrt(d2[:, k - 1])).astype(F32)


def _random_scene(n=20000, seed=3):
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = (0.01 + 0.04 * rng.random(n)).astype(F32)
    return s


def _clustered_scene(n=20000, seed=5):
    """The interpolation tests' clustered generator."""
    rng = np.random.default_rng(seed)
    centres = np.array([[0.3, 0.3, 0.3], [0.7, 0.6, 0.4], [0.5, 0.5, 0.8]])
    k = rng.integers(0, 3, n)
    s = np.empty((n, 4), F32)
    s[:, :3] = np.clip(centres[k] + rng.normal(0.0, 0.02, (n, 3)) * rng.random((n, 1)) ** 3, 0.001, 0.999)
    s[:, 3] = (0.004 + 0.02 * rng.random(n)).astype(F32)
    return s


def _lattice_scene(m=16):
    """Exactly representable lattice positions: many equal distances, ties broken by index."""
    g = (np.arange(m, dtype=F32) + F32(0.5)) / F32(m)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    s = np.empty((m ** 3, 4), F32)
    s[:, 0], s[:, 1], s[:, 2] = x.reshape(-1), y.reshape(-1), z.reshape(-1)
    s[:, 3] = F32(1.0 / m)
    return s


def _coincident_scene(n=6000, seed=7):
    """More than 64 particles at each of two positions."""
    s = _random_scene(n, seed)
    s[:100, :3] = np.array([0.25, 0.5, 0.75], F32)
    s[100:300, :3] = np.array([0.625, 0.375, 0.125], F32)
    return s


SCENES = {"random": _random_scene, "clustered": _clustered_scene, "lattice": _lattice_scene,
          "coincident": _coincident_scene}


def _point_sets(sh):
    rng = np.random.default_rng(11)
    lat = (np.floor(rng.random((500, 3)) * 32) / 32).astype(F32)      # binary-exact, between lattice sites
    return {
        "random": (rng.random((1500, 3), dtype=F32) * F32(1.1) - F32(0.05)),
        "centres": sh[rng.choice(len(sh), 1000, replace=False), :3].copy(),
        "far": np.array([[50.0, 50.0, 50.0], [-40.0, 0.5, 0.5], [0.5, 1e6, 0.5], [1e20, 0.5, 0.5],
                         [-3.0, -3.0, 7.0]], F32),
        "exact": lat,
    }


# ---- CPU ------------------------------------------------------------------------------------------
def test_neighbour_symbols_exported():
    import ctypes
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    for name in ("grace_nearest_neighbours_f4", "grace_smoothing_lengths_f4", "grace_neighbours_enable_stats",
                 "grace_neighbours_last_stats"):
        assert hasattr(lib, name), name


def test_neighbours_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_neighbours"
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_neighbours.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


@pytest.mark.parametrize("call", ["grace::nearest_neighbours_sph(p, s, t, 8, idx, d2);",
                                  "grace::smoothing_lengths_sph(s, t, 8, 1.0f, d2);"])
def test_neighbours_double4_is_a_clear_compile_error(tmp_path, call):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/neighbours_sph.cuh"\n'
                   "void f(const thrust::device_vector<float4>& p, const thrust::device_vector<double4>& s,\n"
                   "       const grace::Tree& t, thrust::device_vector<int>& idx, thrust::device_vector<float>& d2)\n"
                   "{ " + call + " }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "float4 spheres only" in res.stderr


def test_neighbours_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& p, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::Tree& t)\n"
                   "{\n"
                   "    grace::device_vector<int> idx(p.size() * 8);\n"
                   "    grace::device_vector<float> d2(p.size() * 8), h(s.size());\n"
                   "    grace::nearest_neighbours_sph(p, s, t, 8, idx, d2);\n"
                   "    grace::smoothing_lengths_sph(s, t, 8, 1.2f, h);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    for cc in (["g++", "-std=c++14", "-O1", "-Wall", "-Werror"], ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950",
                                                                  "-std=c++17", "-O1", "-x", "c++"]):
        subprocess.check_call([*cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                               "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
        assert exe.exists()
        exe.unlink()


def _write_snapshot(fname, pos, npart, mass, mass_block):
    """A Gadget-2 format-1 snapshot with every particle type (the layout gadget.py documents)."""
    def block(f, payload):
        nb = np.array([len(payload)], np.int32).tobytes()
        f.write(nb); f.write(payload); f.write(nb)

    n = int(sum(npart))
    with open(fname, "wb") as f:
        header = np.array(npart, np.int32).tobytes() + np.array(mass, np.float64).tobytes()
        block(f, header + bytes(256 - len(header)))
        block(f, np.ascontiguousarray(pos, F32).tobytes())
        block(f, np.zeros((n, 3), F32).tobytes())
        block(f, np.arange(n, dtype=np.int32).tobytes())
        if mass_block is not None:
            block(f, np.ascontiguousarray(mass_block, F32).tobytes())
        if npart[0]:
            block(f, np.zeros(npart[0], F32).tobytes())            # U
            block(f, np.ones(npart[0], F32).tobytes())             # RHO
            block(f, np.full(npart[0], 0.01, F32).tobytes())       # HSML


def test_read_gadget_particles_every_type(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "grace-devel_amd"))
    from grace_hip.gadget import read_gadget_particles
    rng = np.random.default_rng(1)
    npart = [5, 7, 0, 3, 4, 2]
    n = sum(npart)
    pos = rng.random((n, 3), dtype=F32)
    first = np.cumsum([0] + npart)
    # header masses for types 1 and 5; per-particle masses (MASS block) for 0, 3 and 4
    mass = [0.0, 2.5, 0.0, 0.0, 0.0, 0.125]
    per = {t: rng.random(npart[t], dtype=F32) for t in (0, 3, 4)}
    fname = str(tmp_path / "snap")
    _write_snapshot(fname, pos, npart, mass, np.concatenate([per[0], per[3], per[4]]))
    for t in range(6):
        p, m = read_gadget_particles(fname, t)
        assert p.dtype == F32 and m.dtype == F32 and p.shape == (npart[t], 3) and m.shape == (npart[t],)
        assert np.array_equal(p, pos[first[t]:first[t + 1]])
        ref = per[t] if t in per else np.full(npart[t], mass[t], F32)
        assert np.array_equal(m, ref), t
    # dark matter only, header masses, no gas and no MASS block
    npart = [0, 9, 0, 0, 0, 0]
    pos = rng.random((9, 3), dtype=F32)
    _write_snapshot(fname, pos, npart, [0, 0.75, 0, 0, 0, 0], None)
    p, m = read_gadget_particles(fname, 1)
    assert np.array_equal(p, pos) and np.array_equal(m, np.full(9, 0.75, F32))
    for t in (0, 2, 3, 4, 5):                                      # absent types: empty, header mass 0 or not
        p, m = read_gadget_particles(fname, t)
        assert p.shape == (0, 3) and m.shape == (0,) and p.dtype == F32 and m.dtype == F32
    with pytest.raises(ValueError):
        read_gadget_particles(fname, 6)


def test_restatement_agrees_with_a_kd_tree():
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(4)
    s = rng.random((3000, 4), dtype=F32)
    pts = rng.random((400, 3), dtype=F32)
    for k in (1, 7, 32):
        idx, d2 = brute_knn(pts, s, k)
        _, ref = spatial.cKDTree(s[:, :3].astype(np.float64)).query(pts.astype(np.float64), k=k)
        ref = np.asarray(ref).reshape(len(pts), k)
        assert np.array_equal(idx, ref.astype(np.int32)), k          # no ties in this scene
        exact = np.sum((pts[:, None, :].astype(np.float64) - s[idx, :3]) ** 2, axis=2)
        assert np.allclose(d2, exact, rtol=1e-5, atol=0)


def test_restatement_ties_and_padding():
    s = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0], [2, 0, 0, 0]], F32)
    idx, d2 = brute_knn(np.array([[0, 0, 0], [np.nan, 0, 0]], F32), s, 7)
    assert idx[0].tolist() == [0, 1, 2, 3, 4, -1, -1]
    assert d2[0].tolist() == [0, 1, 1, 1, 4, np.inf, np.inf]
    assert np.all(idx[1] == -1) and np.all(d2[1] == np.inf)


# ---- GPU --------------------------------------------------------------------------------------------
def _build(gh, s, cuda, mpl=32):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(s, F32)).to(cuda)
    tree = gh.Tree(len(s), mpl, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))     # sorts d
    return d, tree


def _knn(gh, pts, d, tree, k, cuda):
    import torch
    p = torch.from_numpy(np.ascontiguousarray(pts, F32)).to(cuda)
    idx, d2 = gh.nearest_neighbours_sph(p, d, tree, k, check=True)
    return idx.cpu().numpy(), d2.cpu().numpy()


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def built(gh, cuda):
    res = {}
    for name, gen in SCENES.items():
        d, tree = _build(gh, gen(), cuda)
        res[name] = (d, tree, d.cpu().numpy())
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 7, 32, 64])
@pytest.mark.parametrize("scene", list(SCENES))
def test_neighbours_are_the_restatement_bit_for_bit(gh, built, scene, k, cuda):
    d, tree, sh = built[scene]
    for pname, pts in _point_sets(sh).items():
        idx, d2 = _knn(gh, pts, d, tree, k, cuda)
        ref_i, ref_d = brute_knn(pts, sh, k)
        bad = np.nonzero(np.any(idx != ref_i, axis=1))[0]
        assert len(bad) == 0, (pname, bad[:5], idx[bad[:1]], ref_i[bad[:1]])
        assert _same(d2, ref_d), pname


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 7, 32, 64])
@pytest.mark.parametrize("scene", list(SCENES))
def test_smoothing_lengths_bit_for_bit(gh, built, scene, k, cuda):
    import torch
    d, tree, sh = built[scene]
    eta = 1.2
    before = d.clone()
    h = gh.smoothing_lengths_sph(d, tree, k, eta, check=True).cpu().numpy()
    assert torch.equal(d, before)                                  # the spheres are only read
    _, d2 = _knn(gh, sh[:, :3], d, tree, k, cuda)                  # the centres' own query
    assert _same(h, (F32(eta) * np.sqrt(d2[:, k - 1])).astype(F32))
    rows = np.random.default_rng(k).choice(len(sh), 1500, replace=False)
    assert _same(h[rows], brute_h(sh, k, eta, rows))
    if scene == "coincident":
        same = np.all(sh[:, :3] == np.array([0.25, 0.5, 0.75], F32), axis=1)
        assert same.sum() == 100 and np.all(h[same] == 0.0)


@pytest.mark.gpu
def test_results_do_not_depend_on_H_leaf_size_layout_or_knobs(gh, cuda, kernel_reset):
    import torch
    base = _clustered_scene(12000, 8)
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.random((700, 3), dtype=F32), base[:300, :3]])
    k = 24
    runs = []
    for H, mpl in (("zero", 32), ("random", 32), ("zero", 1), ("random", 1)):
        s = base.copy()
        s[:, 3] = 0.0 if H == "zero" else (0.1 * rng.random(len(s))).astype(F32)
        d, tree = _build(gh, s, cuda, mpl)
        h = gh.smoothing_lengths_sph(d, tree, k, 1.0, check=True).cpu().numpy()
        runs.append((d[:, :3].cpu().numpy(), _knn(gh, pts, d, tree, k, cuda), h))
    x0, (i0, d0), h0 = runs[0]
    for x, (i, dd), h in runs[1:]:
        assert np.array_equal(x, x0)                               # the same tree order
        assert np.array_equal(i, i0) and _same(dd, d0) and _same(h, h0)
    d, tree = _build(gh, base, cuda)
    perm = rng.permutation(len(pts))
    i, dd = _knn(gh, pts[perm], d, tree, k, cuda)                  # shuffled point order
    assert np.array_equal(i, i0[perm]) and _same(dd, d0[perm])
    wide = np.full((len(pts), 4), 9.0, F32); wide[:, :3] = pts     # elems_per_point 4
    i, dd = _knn(gh, wide, d, tree, k, cuda)
    assert np.array_equal(i, i0) and _same(dd, d0)
    for kern in KERNELS:
        gh.set_sph_kernel(kern)
        i, dd = _knn(gh, pts, d, tree, k, cuda)
        assert np.array_equal(i, i0) and _same(dd, d0), kern
    gh.set_sph_kernel("cubic")
    for auto, valid in ((False, True), (True, False)):
        gh.set_cache_auto(auto); gh.set_cache_validation(valid)
        try:
            i, dd = _knn(gh, pts, d, tree, k, cuda)
        finally:
            gh.set_cache_auto(True); gh.set_cache_validation(True)
        assert np.array_equal(i, i0) and _same(dd, d0)
    torch.cuda.synchronize()


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


@pytest.mark.gpu
def test_edges(gh, cuda):
    import torch
    # fewer spheres than k: padding
    s = _random_scene(20, 9)
    d, tree = _build(gh, s, cuda, 1)
    sh = d.cpu().numpy()
    pts = np.array([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.1, np.inf, 0.2], [2.0, 2.0, -1.0]], F32)
    idx, d2 = _knn(gh, pts, d, tree, 32, cuda)
    ref_i, ref_d = brute_knn(pts, sh, 32)
    assert np.array_equal(idx, ref_i) and _same(d2, ref_d)
    assert np.all(idx[0, 20:] == -1) and np.all(d2[0, 20:] == np.inf) and np.all(idx[0, :20] >= 0)
    assert np.all(idx[1:3] == -1) and np.all(d2[1:3] == np.inf)   # non-finite points
    # a single sphere: a one-leaf tree without nodes
    one = torch.tensor([[0.25, 0.5, 0.75, 0.0]], dtype=torch.float32, device=cuda)
    t1 = gh.Tree(1, 1, device=cuda)
    t1.leaves[0] = torch.tensor([0, 1, 0, 0], dtype=torch.int32)
    t1.root_index.zero_()
    idx, d2 = _knn(gh, np.array([[0.25, 0.5, 0.75], [0.0, 0.0, 0.0]], F32), one, t1, 3, cuda)
    assert idx.tolist() == [[0, -1, -1], [0, -1, -1]]
    assert d2[0, 0] == 0.0 and _same(d2[1, :1], brute_knn(np.zeros((1, 3), F32), one.cpu().numpy(), 1)[1][0])
    h = gh.smoothing_lengths_sph(one, t1, 1, 2.0, check=True).cpu().numpy()
    assert h.tolist() == [0.0]
    # zero points: GRACE_OK and nothing written, also into a caller's buffers
    import ctypes as C
    i0, d0 = gh.nearest_neighbours_sph(torch.empty((0, 3), dtype=torch.float32, device=cuda), d, tree, 5, check=True)
    assert tuple(i0.shape) == (0, 5) and tuple(d0.shape) == (0, 5)
    pts = torch.rand((8, 3), dtype=torch.float32, device=cuda)
    idx = torch.full((8, 5), 7, dtype=torch.int32, device=cuda)
    dd = torch.full((8, 5), 7.0, dtype=torch.float32, device=cuda)
    st = gh._lib.grace_nearest_neighbours_f4(gh._ptr(pts), C.c_size_t(0), C.c_int(3), *gh._interp_scene(d, tree),
                                             C.c_int(5), gh._ptr(idx), gh._ptr(dd), gh._stream())
    assert st == gh.GRACE_OK
    torch.cuda.synchronize()
    assert torch.all(idx == 7) and torch.all(dd == 7.0)


@pytest.mark.gpu
def test_stats_hook_counts_every_active_lane(gh, built, cuda):
    d, tree, sh = built["random"]
    n, k = len(sh), 32
    gh.neighbours_enable_stats(True)
    try:
        gh.smoothing_lengths_sph(d, tree, k, 1.0, check=True)
        tests, packets, steps = gh.neighbours_last_stats()
    finally:
        gh.neighbours_enable_stats(False)
    # every lane's own centre survives its packet's culling: a packet of m points has >= m survivors,
    # each tested by its m lanes, so tests >= sum of m^2 >= n^2 / packets
    assert packets >= (n + 63) // 64
    assert tests >= n * n // packets, (tests, n, packets)
    # every lane inserts at least k times to fill its list
    assert k * packets <= steps <= tests


@pytest.mark.gpu
def test_bad_arguments_write_nothing(gh, built, cuda):
    import ctypes as C
    import torch
    d, tree, sh = built["random"]
    n = len(sh)
    pts = torch.rand((100, 4), dtype=torch.float32, device=cuda)
    idx = torch.full((100, 64), 7, dtype=torch.int32, device=cuda)
    dd = torch.full((100, 64), 7.0, dtype=torch.float32, device=cuda)
    h = torch.full((n,), 7.0, dtype=torch.float32, device=cuda)
    scene = gh._interp_scene(d, tree)
    lib = gh._lib

    def knn(k=8, elems=4, ip=idx, dp=dd):
        return lib.grace_nearest_neighbours_f4(gh._ptr(pts), C.c_size_t(100), C.c_int(elems), *scene, C.c_int(k),
                                               gh._ptr(ip), gh._ptr(dp), gh._stream())

    def sml(k=8, eta=1.0, hp=h, n_s=n):
        sc = list(scene); sc[1] = C.c_size_t(n_s)
        return lib.grace_smoothing_lengths_f4(*sc, C.c_int(k), C.c_float(eta), gh._ptr(hp), gh._stream())

    for kw in (dict(k=0), dict(k=65), dict(k=-3), dict(elems=2), dict(elems=17), dict(ip=None, dp=None)):
        assert knn(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    for kw in (dict(k=0), dict(k=65), dict(eta=0.0), dict(eta=-1.0), dict(eta=float("nan")), dict(eta=float("inf")),
               dict(hp=None), dict(k=33, n_s=32)):
        assert sml(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    torch.cuda.synchronize()
    assert torch.all(idx == 7) and torch.all(dd == 7.0) and torch.all(h == 7.0)
    with pytest.raises(ValueError):
        gh.smoothing_lengths_sph(d[:40], tree, 41)
    with pytest.raises(ValueError):
        gh.nearest_neighbours_sph(pts, d, tree, 65)
    # one output only
    assert knn(ip=None) == gh.GRACE_OK and knn(dp=None) == gh.GRACE_OK
    gh.trace_status()


@pytest.mark.gpu
def test_dark_matter_recipe_round_trip(gh, cuda):
    import torch
    rng = np.random.default_rng(12)
    n = 30000
    x = rng.random((n, 3), dtype=F32)                              # no coincident particles: every h > 0
    m = (0.5 + rng.random(n)).astype(F32)
    s = torch.zeros((n, 4), dtype=torch.float32, device=cuda)     # w = 0: no H yet
    s[:, :3] = torch.from_numpy(x).to(cuda)
    tree = gh.Tree(n, 32, device=cuda)
    tree, perm = gh.build_tree(s, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_perm=True)
    mass = torch.from_numpy(m).to(cuda)[perm.long()]
    h = gh.smoothing_lengths_sph(s, tree, 32, 1.2, check=True)
    s[:, 3] = h
    tree2 = gh.Tree(n, 32, device=cuda)
    tree2, perm2 = gh.build_tree(s, tree2, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_perm=True)
    assert torch.equal(perm2.cpu(), torch.arange(n, dtype=perm2.dtype))   # the order is unchanged
    assert torch.all(s[:, 3] > 0)
    rays = gh.orthogonal_rays_z(64, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    col = torch.empty(len(rays), dtype=torch.float32, device=cuda)
    gh.trace_cumulative_sph(rays, s, tree2, col, check=True)
    assert float(col.max()) > 0.0
    rho, cnt = gh.interpolate_sph(s[:2000, :3].contiguous(), s, tree2, mass,
                                  counts=torch.empty(2000, dtype=torch.int32, device=cuda), check=True)
    assert torch.all(cnt >= 1) and torch.all(rho > 0)


@pytest.mark.gpu
def test_scale_million_clustered(gh, cuda):
    n, k = 1_000_000, 32
    s = _clustered_scene(n, 21)
    d, tree = _build(gh, s, cuda)
    h = gh.smoothing_lengths_sph(d, tree, k, 1.0, check=True).cpu().numpy()
    sh = d.cpu().numpy()
    rows = np.random.default_rng(5).choice(n, 2000, replace=False)
    assert _same(h[rows], brute_h(sh, k, 1.0, rows))


@pytest.mark.gpu
def test_deep_clustered_tree_fits_the_stack(gh, cuda):
    rng = np.random.default_rng(9)
    n = 30000
    s = np.empty((n, 4), F32)
    scale = 0.4 * 0.1 ** (rng.integers(0, 5, n))                  # nested clusters, ten times closer each time
    s[:, :3] = (0.5 + scale[:, None] * (rng.random((n, 3)) - 0.5)).astype(F32)
    s[:, 3] = 0.0
    d, tree = _build(gh, s, cuda)
    sh = d.cpu().numpy()
    pts = (0.5 + (rng.random((1500, 3)) - 0.5) * 0.4 * 0.1 ** rng.integers(0, 5, (1500, 1))).astype(F32)
    idx, d2 = _knn(gh, pts, d, tree, 32, cuda)                     # check=True: GRACE_OK, no stack overflow
    ref_i, ref_d = brute_knn(pts, sh, 32)
    assert np.array_equal(idx, ref_i) and _same(d2, ref_d)
    h = gh.smoothing_lengths_sph(d, tree, 32, 1.0, check=True).cpu().numpy()
    rows = rng.choice(n, 1000, replace=False)
    assert _same(h[rows], brute_h(sh, 32, 1.0, rows))


@pytest.mark.gpu
def test_neighbours_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    d, tree = _build(gh, _random_scene(9000, 41), cuda)
    s = d.cpu().numpy()                                            # tree order
    pts = np.random.default_rng(3).random((777, 4), dtype=F32)
    k, eta = 19, 1.5
    s.tofile(str(tmp_path / "s.f32")); pts.tofile(str(tmp_path / "p.f32"))
    exe = str(tmp_path / "dropin_neighbours")
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_neighbours.hip"), "-o", exe,
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    res = subprocess.run([exe, str(tmp_path / "s.f32"), str(tmp_path / "p.f32"), str(k), str(eta), str(tmp_path)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    idx, d2 = _knn(gh, pts, d, tree, k, cuda)
    h = gh.smoothing_lengths_sph(d, tree, k, eta, check=True).cpu().numpy()
    assert np.array_equal(idx.reshape(-1), np.fromfile(str(tmp_path / "indices.i32"), np.int32))
    assert _same(d2.reshape(-1), np.fromfile(str(tmp_path / "d2.f32"), F32))
    assert _same(h, np.fromfile(str(tmp_path / "h.f32"), F32))
