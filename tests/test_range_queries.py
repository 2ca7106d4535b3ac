"""Range queries (grace_range_counts_f4 / grace_range_neighbours_f4, range_counts_sph /
range_neighbours_sph): every sphere centre within the query point's own radius, as counts, CSR lists
and gather sums of the SPH kernel.

Expected values restate the contract of include/grace_hip.h in NumPy: d2 in float32 in the stated
order (d2_rows of test_neighbours.py), R2 = fl(r * r), membership d2 <= R2, rows in ascending tree
index, off points (non-finite coordinate; r negative, NaN or +inf) empty, and the gather sums as a
plain float32 running sum in ascending index of fl(w * W) with W the interpolation's arithmetic at
H := r_p (f32_kernel of test_sph_interpolation.py).  Every comparison is bitwise.

Radii are log-uniform per scene so that rows run from empty to a few hundred entries.  The lattice
scene takes the exact radii 1/16, 2/16 and fl(sqrt(2)/16) (at most 33 lattice sites are in range of
those), and log-uniform radii at every fourth point for the long rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_neighbours import (SCENES, _build, _clustered_scene, _coincident_scene, _point_sets, _random_scene,
                             brute_knn, built, d2_rows)  # noqa: F401  (built: the module's scenes fixture)
from test_sph_interpolation import f32_kernel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32 = np.float32
KERNELS = ("cubic", "quartic", "quintic", "wendland_c2", "wendland_c4", "wendland_c6")
R_MAX = {"random": 0.2, "clustered": 0.002, "lattice": 0.3, "coincident": 0.3}
LATTICE_RADII = np.array([1.0 / 16.0, 2.0 / 16.0, np.sqrt(2.0) / 16.0]).astype(F32)


# ---- the restatement ----------------------------------------------------------------------------
def is_on(points, radii):
    with np.errstate(invalid="ignore"):
        return np.all(np.isfinite(points[:, :3]), axis=1) & (radii >= 0) & (radii < np.inf)


def restate(points, radii, spheres):
    """(counts int32 [m], offsets int32 [m + 1], indices int32 [total], d2 float32 [total]) of the contract.
    radii: float32 [m]."""
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    r = np.asarray(radii, F32)
    on = is_on(P, r)
    with np.errstate(over="ignore", invalid="ignore"):
        R2 = (r * r).astype(F32)
    chunk = max(1, (1 << 22) // max(len(X), 1))
    rows, cols, vals = [], [], []
    for a in range(0, len(P), chunk):
        with np.errstate(over="ignore", invalid="ignore"):
            d2 = d2_rows(P[a:a + chunk], X)
            hit = (d2 <= R2[a:a + chunk, None]) & on[a:a + chunk, None]
        pi, si = np.nonzero(hit)                       # row-major: ascending sphere index within a point
        rows.append(pi + a); cols.append(si); vals.append(d2[pi, si])
    pi = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    si = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    dd = np.concatenate(vals).astype(F32) if vals else np.zeros(0, F32)
    counts = np.bincount(pi, minlength=len(P)).astype(np.int32)
    offsets = np.zeros(len(P) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    return counts, offsets.astype(np.int32), si.astype(np.int32), dd


def restate_sums(points, radii, spheres, w, kernel, lists=None):
    """float32 [m, C]: the gather sums of the contract (w: float32 [n, C])."""
    counts, offsets, si, d2 = restate(points, radii, spheres) if lists is None else lists
    m = len(points)
    pi = np.repeat(np.arange(m), counts)
    r = np.asarray(radii, F32)[pi]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ih = (F32(1) / r).astype(F32)
        q = (np.sqrt(d2) * ih).astype(F32)
        W = (f32_kernel(kernel, q) * ((ih * ih) * ih).astype(F32)).astype(F32)
    rank = np.arange(len(pi)) - offsets[pi]
    width = int(counts.max()) if m else 0
    out = np.zeros((m, w.shape[1]), F32)
    keep = r > 0                                       # r == 0: the sum is 0
    for c in range(w.shape[1]):
        terms = np.zeros((m, max(width, 1)), F32)
        with np.errstate(invalid="ignore", over="ignore"):
            terms[pi[keep], rank[keep]] = (w[si[keep], c] * W[keep]).astype(F32)
        acc = np.zeros(m, F32)
        for j in range(width):
            acc = (acc + terms[:, j]).astype(F32)      # adding fl(0) past a row's end changes nothing
        out[:, c] = acc
    return out


def scene_radii(scene, pname, n):
    rng = np.random.default_rng(sum(map(ord, scene + pname)))
    r = np.exp(rng.uniform(np.log(1e-4), np.log(R_MAX[scene]), n)).astype(F32)
    if scene == "lattice":
        exact = LATTICE_RADII[np.arange(n) % 3]
        r = np.where(np.arange(n) % 4 == 3, r, exact).astype(F32)
    return r


_ref_cache = {}


def reference(scene, sh):
    """{point set: (points, radii, restatement)} of a scene (tree order sh), computed once."""
    if scene not in _ref_cache:
        res = {}
        for pname, pts in _point_sets(sh).items():
            r = scene_radii(scene, pname, len(pts))
            res[pname] = (pts, r, restate(pts, r, sh))
        _ref_cache[scene] = res
    return _ref_cache[scene]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def digest(a):
    """The drop-in program's digest of 32-bit words: sum of v[i] (2 i + 1) modulo 2^64."""
    v = np.ascontiguousarray(a).reshape(-1).view(np.uint32).astype(np.uint64)
    i = np.arange(len(v), dtype=np.uint64)
    with np.errstate(over="ignore"):
        return len(v), int(np.sum(v * (np.uint64(2) * i + np.uint64(1)), dtype=np.uint64))


# ---- CPU ------------------------------------------------------------------------------------------
def test_range_symbols_exported():
    lib = C.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    for name in ("grace_range_counts_f4", "grace_range_neighbours_f4"):
        assert hasattr(lib, name), name


def _compile_dropin(exe):
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, os.path.join(ROOT, "tests", "cpp", "dropin_range.hip"),
                           "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


def test_range_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_range"
    _compile_dropin(exe)
    assert exe.exists()


@pytest.mark.parametrize("call", ["grace::range_counts_sph(p, r, s, t, cnt);",
                                  "grace::range_counts_sph(p, 0.1f, s, t, w, 1, cnt, d2);",
                                  "grace::range_neighbours_sph(p, r, s, t, off, cnt, d2);"])
def test_range_double4_is_a_clear_compile_error(tmp_path, call):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/range_sph.cuh"\n'
                   "void f(const thrust::device_vector<float4>& p, const thrust::device_vector<double4>& s,\n"
                   "       const thrust::device_vector<float>& r, const thrust::device_vector<float>& w,\n"
                   "       const grace::Tree& t, thrust::device_vector<int>& cnt, thrust::device_vector<int>& off,\n"
                   "       thrust::device_vector<float>& d2)\n"
                   "{ " + call + " }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "float4 spheres only" in res.stderr


def test_range_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& p, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::device_vector<float>& r, const grace::device_vector<float>& w,\n"
                   "       const grace::Tree& t)\n"
                   "{\n"
                   "    grace::device_vector<int> cnt(p.size()), off, idx;\n"
                   "    grace::device_vector<float> sums(p.size() * 2), d2;\n"
                   "    grace::range_counts_sph(p, r, s, t, cnt);\n"
                   "    grace::range_counts_sph(p, 0.25f, s, t, cnt);\n"
                   "    grace::range_counts_sph(p, r, s, t, w, 2, cnt, sums);\n"
                   "    grace::range_counts_sph(p, 0.25f, s, t, w, 2, cnt, sums);\n"
                   "    grace::range_neighbours_sph(p, r, s, t, off, idx, d2);\n"
                   "    grace::range_neighbours_sph(p, 0.25f, s, t, off, idx, d2);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


def test_restated_counts_agree_with_a_kd_tree():
    """A second method: a kd-tree in float64.  Its test |p - x| <= r and the contract's fl(d2) <= fl(r r)
    may differ for a centre within rounding of the radius (d2 carries 3 rounded products and 2 rounded
    sums, R2 one: below 4 ulp = 2.4e-7 relative in the square), so the restated count is bracketed by the
    kd-tree's counts at r (1 -+ 1e-6), which are mostly equal."""
    spatial = pytest.importorskip("scipy.spatial")
    rng = np.random.default_rng(4)
    s = rng.random((3000, 4), dtype=F32)
    pts = (rng.random((2000, 3), dtype=F32) * F32(1.1) - F32(0.05))
    r = np.exp(rng.uniform(np.log(1e-3), np.log(0.3), len(pts))).astype(F32)
    counts, offsets, idx, d2 = restate(pts, r, s)
    tree = spatial.cKDTree(s[:, :3].astype(np.float64))
    p64, r64 = pts.astype(np.float64), r.astype(np.float64)
    lo = tree.query_ball_point(p64, r64 * (1 - 1e-6), return_length=True)
    hi = tree.query_ball_point(p64, r64 * (1 + 1e-6), return_length=True)
    assert np.all(lo <= counts) and np.all(counts <= hi)
    assert np.mean(lo == hi) > 0.99 and counts.min() == 0 and counts.max() > 256
    # the lists: ascending, and their d2 the exact ones to fp32 accuracy
    assert offsets[-1] == counts.sum() == len(idx)
    for p in (int(np.argmax(counts)), 5):
        row = idx[offsets[p]:offsets[p + 1]]
        assert np.all(np.diff(row) > 0)
        exact = np.sum((p64[p] - s[row, :3].astype(np.float64)) ** 2, axis=1)
        assert np.allclose(d2[offsets[p]:offsets[p + 1]], exact, rtol=1e-5, atol=0)


def test_restatement_edges():
    s = np.array([[0, 0, 0, 9], [1, 0, 0, 9], [-1, 0, 0, 9], [0, 1, 0, 9], [2, 0, 0, 9], [0, 0, 0, 9]], F32)
    pts = np.zeros((7, 3), F32)
    pts[5, 0] = np.nan
    r = np.array([0.0, 1.0, 2.0, -1.0, np.inf, 1.0, np.nan], F32)
    counts, offsets, idx, d2 = restate(pts, r, s)
    assert counts.tolist() == [2, 5, 6, 0, 0, 0, 0]               # inclusive: d2 == R2 is in range
    assert idx[:7].tolist() == [0, 5, 0, 1, 2, 3, 5] and d2[:7].tolist() == [0, 0, 0, 1, 1, 1, 0]
    w = np.ones((6, 1), F32)
    sums = restate_sums(pts, r, s, w, "cubic")
    assert sums[0, 0] == 0.0 and sums[3, 0] == 0.0                 # r == 0 and off points: 0
    assert sums[1, 0] == F32(2) * f32_kernel("cubic", np.zeros(1, F32))[0]   # the edge terms are W(q = 1) = 0


@pytest.mark.parametrize("scene", list(SCENES))
def test_reference_rows_run_from_empty_to_hundreds(scene):
    s = SCENES[scene]()                                            # (the generators' order: any order serves here)
    counts = np.concatenate([restate(p, scene_radii(scene, n, len(p)), s)[0] for n, p in _point_sets(s).items()])
    assert counts.min() == 0 and counts.max() > 256, (counts.min(), counts.max())


# ---- GPU --------------------------------------------------------------------------------------------
def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _radii_arg(r, cuda):
    return float(r) if np.ndim(r) == 0 else _dev(np.asarray(r, F32), cuda)


def _counts(gh, pts, r, d, tree, cuda, weights=None):
    cnt, sums = gh.range_counts_sph(_dev(np.asarray(pts, F32), cuda), _radii_arg(r, cuda), d, tree, weights=weights,
                                    check=True)
    return cnt.cpu().numpy(), None if sums is None else sums.cpu().numpy()


def _lists(gh, pts, r, d, tree, cuda):
    off, idx, d2 = gh.range_neighbours_sph(_dev(np.asarray(pts, F32), cuda), _radii_arg(r, cuda), d, tree, check=True)
    return off.cpu().numpy(), idx.cpu().numpy(), d2.cpu().numpy()


def _check_lists(got, ref, what):
    off, idx, d2 = got
    counts, r_off, r_idx, r_d2 = ref
    assert np.array_equal(off, r_off), what
    assert np.array_equal(idx, r_idx), what
    assert _same(d2, r_d2), what


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_counts_and_lists_are_the_restatement_bit_for_bit(gh, built, scene, cuda):
    d, tree, sh = built[scene]
    all_counts = []
    for pname, (pts, r, ref) in reference(scene, sh).items():
        cnt, sums = _counts(gh, pts, r, d, tree, cuda)
        assert sums is None
        bad = np.nonzero(cnt != ref[0])[0]
        assert len(bad) == 0, (pname, bad[:5], cnt[bad[:5]], ref[0][bad[:5]])
        _check_lists(_lists(gh, pts, r, d, tree, cuda), ref, pname)
        all_counts.append(ref[0])
        # one radius for all points against a filled radii array
        r1 = F32(np.median(r))
        c_s, _ = _counts(gh, pts, float(r1), d, tree, cuda)
        c_a, _ = _counts(gh, pts, np.full(len(pts), r1, F32), d, tree, cuda)
        assert np.array_equal(c_s, c_a) and np.array_equal(c_s, restate(pts, np.full(len(pts), r1, F32), sh)[0]), pname
        l_s = _lists(gh, pts, float(r1), d, tree, cuda)
        l_a = _lists(gh, pts, np.full(len(pts), r1, F32), d, tree, cuda)
        assert all(_same(x, y) for x, y in zip(l_s, l_a)), pname
    all_counts = np.concatenate(all_counts)
    assert all_counts.min() == 0 and all_counts.max() > 256
    if scene == "lattice":                                         # d2 == R2 ties at the exact radii
        pts, r, ref = reference(scene, sh)["centres"]
        row = np.nonzero(r == F32(1.0 / 16.0))[0][0]
        dd = ref[3][ref[1][row]:ref[1][row + 1]]
        assert np.any(dd == F32(1.0 / 256.0))
    if scene == "coincident":
        same = np.nonzero(np.all(sh[:, :3] == np.array([0.625, 0.375, 0.125], F32), axis=1))[0]
        assert len(same) == 200
        cnt, _ = _counts(gh, sh[same[:3], :3], 0.0, d, tree, cuda)  # r = 0: the coincident centres, > 3 clusters
        assert cnt.tolist() == [200, 200, 200]
        off, idx, d2 = _lists(gh, sh[same[:1], :3], 0.0, d, tree, cuda)
        assert np.array_equal(idx, same) and np.all(d2 == 0.0)


@pytest.mark.gpu
def test_coincident_spine_deeper_than_the_stack(gh, cuda):
    """max_per_leaf 1: the 200 coincident particles are a spine of 200 leaves, deeper than the 128-entry
    stack; check=True raises if a packet exhausts it."""
    s = _coincident_scene()
    d, tree = _build(gh, s, cuda, 1)
    sh = d.cpu().numpy()
    rng = np.random.default_rng(17)
    pts = np.concatenate([sh[:400, :3], rng.random((400, 3), dtype=F32)])
    r = np.exp(rng.uniform(np.log(1e-4), np.log(0.3), len(pts))).astype(F32)
    ref = restate(pts, r, sh)
    cnt, _ = _counts(gh, pts, r, d, tree, cuda)
    assert np.array_equal(cnt, ref[0])
    _check_lists(_lists(gh, pts, r, d, tree, cuda), ref, "mpl 1")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_gather_sums_bit_for_bit(gh, built, kernel, cuda, kernel_reset):
    import torch
    gh.set_sph_kernel(kernel)
    for scene in ("random", "coincident"):
        d, tree, sh = built[scene]
        n = len(sh)
        h = gh.smoothing_lengths_sph(d, tree, 32, 1.2, check=True).cpu().numpy()
        rows = np.random.default_rng(23).choice(n, 700, replace=False)
        if scene == "coincident":                                   # h == 0 there: the sum is 0
            rows[:20] = np.nonzero(np.all(sh[:, :3] == np.array([0.25, 0.5, 0.75], F32), axis=1))[0][:20]
        pts, r = sh[rows, :3], h[rows]
        lists = restate(pts, r, sh)
        for n_ch in (1, 4, 5, 64):
            w = (0.5 + np.random.default_rng(n_ch).random((n, n_ch))).astype(F32)
            wd = _dev(w[:, 0] if n_ch == 1 else w, cuda)
            cnt, sums = _counts(gh, pts, r, d, tree, cuda, weights=wd)
            assert np.array_equal(cnt, lists[0])
            ref = restate_sums(pts, r, sh, w, kernel, lists)
            assert _same(sums.reshape(len(pts), n_ch), ref), (scene, n_ch)
            if scene == "coincident":
                assert np.all(r[:20] == 0) and np.all(sums.reshape(len(pts), n_ch)[:20] == 0) and np.all(cnt[:20] >= 100)
        # sums without counts
        out = torch.full((len(pts),), 7.0, dtype=torch.float32, device=cuda)
        w1 = _dev(np.ones(n, F32), cuda)
        pd, rd = _dev(pts, cuda), _dev(r, cuda)                     # (named: alive until the call has run)
        st = gh._lib.grace_range_counts_f4(gh._ptr(pd), C.c_size_t(len(pts)), C.c_int(3),
                                           gh._ptr(rd), C.c_float(0.0), *gh._interp_scene(d, tree),
                                           gh._ptr(w1), C.c_int(1), gh._ptr(None), gh._ptr(out), gh._stream())
        assert st == gh.GRACE_OK
        gh.trace_status()
        assert _same(out.cpu().numpy()[:, None], restate_sums(pts, r, sh, np.ones((n, 1), F32), kernel, lists))


@pytest.mark.gpu
def test_custom_table_is_refused_and_writes_nothing(gh, built, cuda, kernel_reset):
    import torch
    d, tree, sh = built["random"]
    pts = torch.rand((50, 3), dtype=torch.float32, device=cuda)
    w = torch.ones(len(sh), dtype=torch.float32, device=cuda)
    cnt = torch.full((50,), 7, dtype=torch.int32, device=cuda)
    out = torch.full((50,), 7.0, dtype=torch.float32, device=cuda)
    gh.set_sph_kernel(gh.sph_kernel_table("quartic"))              # a custom table: no f(q)
    with pytest.raises(ValueError):
        gh.range_counts_sph(pts, 0.1, d, tree, weights=w, counts=cnt, out=out)
    torch.cuda.synchronize()
    assert torch.all(cnt == 7) and torch.all(out == 7.0)
    c2, _ = gh.range_counts_sph(pts, 0.1, d, tree, check=True)      # counts and lists need no f(q)
    off, idx, d2 = gh.range_neighbours_sph(pts, 0.1, d, tree, check=True)
    gh.set_sph_kernel("cubic")
    c3, _ = gh.range_counts_sph(pts, 0.1, d, tree, weights=w, counts=cnt, out=out, check=True)
    assert torch.equal(c2, c3) and int(off[-1]) == int(c2.sum())


@pytest.mark.gpu
def test_short_rows_are_the_nearest_neighbours_in_range(gh, built, cuda):
    d, tree, sh = built["random"]
    import torch
    for pname in ("random", "centres"):
        pts, r, ref = reference("random", sh)[pname]
        off, idx, d2 = _lists(gh, pts, r, d, tree, cuda)
        ki, kd = gh.nearest_neighbours_sph(_dev(pts, cuda), d, tree, 64, check=True)
        ki, kd = ki.cpu().numpy(), kd.cpu().numpy()
        with np.errstate(over="ignore"):
            R2 = (r * r).astype(F32)
        checked = 0
        for p in np.nonzero(np.diff(off) <= 64)[0]:
            if not np.all(np.isfinite(pts[p])):
                continue
            m = kd[p] <= R2[p]
            order = np.argsort(ki[p][m])
            assert np.array_equal(ki[p][m][order], idx[off[p]:off[p + 1]]), (pname, p)
            assert _same(kd[p][m][order], d2[off[p]:off[p + 1]]), (pname, p)
            checked += 1
        assert checked > 100
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_results_do_not_depend_on_order_layout_tree_or_kernel(gh, cuda, kernel_reset):
    import torch
    base = _clustered_scene(12000, 8)
    base[:150, :3] = np.array([0.5, 0.25, 0.75], F32)              # a coincident group: a spine at max_per_leaf 1
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.random((700, 3), dtype=F32), base[:300, :3]])
    r = np.exp(rng.uniform(np.log(1e-4), np.log(0.02), len(pts))).astype(F32)
    w = (0.5 + rng.random((len(base), 2))).astype(F32)
    runs = []
    for hscale, mpl in ((0.0, 32), (1.0, 32), (3.0, 32), (1.0, 1), (0.0, 1)):
        s = base.copy()
        s[:, 3] *= F32(hscale)
        d = torch.from_numpy(s).to(cuda)
        tree = gh.Tree(len(s), mpl, device=cuda)
        tree, perm = gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_perm=True)
        wd = _dev(w, cuda)[perm.long()].contiguous()
        cnt, sums = _counts(gh, pts, r, d, tree, cuda, weights=wd)
        runs.append((d[:, :3].cpu().numpy(), cnt, sums, _lists(gh, pts, r, d, tree, cuda), wd))
    x0, c0, s0, l0, wd = runs[0]
    assert np.array_equal(c0, restate(pts, r, x0)[0]) and c0.max() > 64
    for x, c, s, l, _ in runs[1:]:
        assert np.array_equal(x, x0)                               # the same tree order
        assert np.array_equal(c, c0) and _same(s, s0) and all(_same(a, b) for a, b in zip(l, l0))
    d, tree = _build(gh, base, cuda)
    perm = rng.permutation(len(pts))                               # shuffled point order
    c, s = _counts(gh, pts[perm], r[perm], d, tree, cuda, weights=wd)
    assert np.array_equal(c, c0[perm]) and _same(s, s0[perm])
    off, idx, d2 = _lists(gh, pts[perm], r[perm], d, tree, cuda)
    for k, p in enumerate(perm[:200]):
        assert np.array_equal(idx[off[k]:off[k + 1]], l0[1][l0[0][p]:l0[0][p + 1]])
        assert _same(d2[off[k]:off[k + 1]], l0[2][l0[0][p]:l0[0][p + 1]])
    for elems in (4, 7):                                           # elems_per_point
        wide = np.full((len(pts), elems), 9.0, F32); wide[:, :3] = pts
        c, s = _counts(gh, wide, r, d, tree, cuda, weights=wd)
        assert np.array_equal(c, c0) and _same(s, s0), elems
        assert all(_same(a, b) for a, b in zip(_lists(gh, wide, r, d, tree, cuda), l0)), elems
    for kern in KERNELS:                                           # counts and lists: not the SPH kernel
        gh.set_sph_kernel(kern)
        c, _ = _counts(gh, pts, r, d, tree, cuda)
        assert np.array_equal(c, c0), kern
        assert all(_same(a, b) for a, b in zip(_lists(gh, pts, r, d, tree, cuda), l0)), kern
    gh.set_sph_kernel("cubic")
    for auto, valid in ((False, True), (True, False)):             # the trace's knobs
        gh.set_cache_auto(auto); gh.set_cache_validation(valid)
        try:
            c, s = _counts(gh, pts, r, d, tree, cuda, weights=wd)
            l = _lists(gh, pts, r, d, tree, cuda)
        finally:
            gh.set_cache_auto(True); gh.set_cache_validation(True)
        assert np.array_equal(c, c0) and _same(s, s0) and all(_same(a, b) for a, b in zip(l, l0))
    # a trace between the count and the fill
    pd, rd = _dev(pts, cuda), _dev(r, cuda)
    offsets = torch.zeros(len(pts) + 1, dtype=torch.int32, device=cuda)
    gh.range_counts_sph(pd, rd, d, tree, counts=offsets[:len(pts)])
    rays = gh.orthogonal_rays_z(32, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0]
    col = torch.empty(len(rays), dtype=torch.float32, device=cuda)
    gh.trace_cumulative_sph(rays, d, tree, col, check=True)
    total = gh.exclusive_scan(offsets, offsets)
    idx = torch.empty(total, dtype=torch.int32, device=cuda)
    d2 = torch.empty(total, dtype=torch.float32, device=cuda)
    st = gh._lib.grace_range_neighbours_f4(gh._ptr(pd), C.c_size_t(len(pts)), C.c_int(3), gh._ptr(rd), C.c_float(0.0),
                                           *gh._interp_scene(d, tree), gh._ptr(offsets), gh._ptr(idx), gh._ptr(d2),
                                           gh._stream())
    assert st == gh.GRACE_OK
    gh.trace_status()
    assert all(_same(a, b) for a, b in zip((offsets.cpu().numpy(), idx.cpu().numpy(), d2.cpu().numpy()), l0))


@pytest.mark.gpu
def test_edges(gh, cuda):
    import torch
    # one sphere: a one-leaf tree without nodes; two spheres: one node
    one = torch.tensor([[0.25, 0.5, 0.75, 0.0]], dtype=torch.float32, device=cuda)
    t1 = gh.Tree(1, 1, device=cuda)
    t1.leaves[0] = torch.tensor([0, 1, 0, 0], dtype=torch.int32)
    t1.root_index.zero_()
    pts = np.array([[0.25, 0.5, 0.75], [0.0, 0.0, 0.0], [0.25, 0.5, 0.5]], F32)
    r = np.array([0.0, 1.0, 0.25], F32)
    ref = restate(pts, r, one.cpu().numpy())
    assert ref[0].tolist() == [1, 1, 1]
    assert np.array_equal(_counts(gh, pts, r, one, t1, cuda)[0], ref[0])
    _check_lists(_lists(gh, pts, r, one, t1, cuda), ref, "one sphere")
    two, t2 = _build(gh, np.array([[0.25, 0.5, 0.75, 0.1], [0.75, 0.5, 0.25, 0.1]], F32), cuda, 1)
    ref = restate(pts, r, two.cpu().numpy())
    assert np.array_equal(_counts(gh, pts, r, two, t2, cuda)[0], ref[0])
    _check_lists(_lists(gh, pts, r, two, t2, cuda), ref, "two spheres")

    s = _random_scene(3000, 9)
    d, tree = _build(gh, s, cuda)
    sh = d.cpu().numpy()
    rng = np.random.default_rng(5)
    # packet sizes around a wave
    for n in (0, 1, 63, 64, 65):
        pts = rng.random((n, 3), dtype=F32)
        r = np.full(n, 0.1, F32)
        ref = restate(pts, r, sh)
        assert np.array_equal(_counts(gh, pts, r, d, tree, cuda)[0], ref[0]), n
        _check_lists(_lists(gh, pts, r, d, tree, cuda), ref, n)
        assert np.array_equal(_counts(gh, pts, 0.1, d, tree, cuda)[0], ref[0]), n
    # off points and radii among good ones; r = 0 at a centre; R2 underflows to 0
    pts = rng.random((12, 3), dtype=F32)
    pts[8:] = sh[100:104, :3]
    pts[0, 0] = np.nan; pts[1, 1] = np.inf; pts[2, 2] = -np.inf
    r = np.array([0.2, 0.2, 0.2, 0.0, -0.1, np.nan, np.inf, 0.2, 0.0, 1e-30, -0.0, 0.2], F32)
    ref = restate(pts, r, sh)
    assert ref[0][:7].tolist() == [0] * 7 and ref[0][7] > 0 and ref[0][8:11].tolist() == [1, 1, 1]
    assert F32(1e-30) * F32(1e-30) == 0
    w = _dev(np.ones(len(sh), F32), cuda)
    cnt, sums = _counts(gh, pts, r, d, tree, cuda, weights=w)
    assert np.array_equal(cnt, ref[0])
    assert _same(sums[:, None], restate_sums(pts, r, sh, np.ones((len(sh), 1), F32), "cubic", ref))
    assert np.all(sums[:7] == 0) and sums[8] == 0 and sums[10] == 0
    _check_lists(_lists(gh, pts, r, d, tree, cuda), ref, "off points")
    # one radius that covers the whole scene
    pts = rng.random((8, 3), dtype=F32)
    off, idx, d2 = _lists(gh, pts, 2.0, d, tree, cuda)
    assert off.tolist() == [3000 * i for i in range(9)]
    assert np.array_equal(idx, np.tile(np.arange(3000, dtype=np.int32), 8))
    assert _same(d2, d2_rows(pts, sh[:, :3]).reshape(-1))
    assert np.array_equal(_counts(gh, pts, 2.0, d, tree, cuda)[0], np.full(8, 3000, np.int32))
    # want_d2=False
    off2, idx2, none = gh.range_neighbours_sph(_dev(pts, cuda), 2.0, d, tree, want_d2=False, check=True)
    assert none is None and np.array_equal(idx2.cpu().numpy(), idx)
    # zero points: GRACE_OK and nothing written
    cnt = torch.full((8,), 7, dtype=torch.int32, device=cuda)
    pd = _dev(pts, cuda)
    st = gh._lib.grace_range_counts_f4(gh._ptr(pd), C.c_size_t(0), C.c_int(3), gh._ptr(None), C.c_float(0.1),
                                       *gh._interp_scene(d, tree), gh._ptr(None), C.c_int(0), gh._ptr(cnt),
                                       gh._ptr(None), gh._stream())
    assert st == gh.GRACE_OK
    torch.cuda.synchronize()
    assert torch.all(cnt == 7)


@pytest.mark.gpu
def test_fill_never_writes_outside_its_row(gh, built, cuda):
    import torch
    d, tree, sh = built["random"]
    pts, r, ref = reference("random", sh)["centres"]
    pts, r = pts[:300], np.full(300, 0.08, F32)
    counts, off, r_idx, r_d2 = restate(pts, r, sh)
    pad = 64
    total = int(off[-1])
    short = int(np.nonzero(counts >= 2)[0][0])                     # keeps an entry when one short
    long_ = int(np.nonzero(counts >= 1)[0][-1])
    assert short + 1 < long_
    # row `short` one entry short, row `long_` one entry long: the rows between them move down by one
    bad = off.copy()
    bad[short + 1:long_ + 1] -= 1
    pd, rd = _dev(pts, cuda), _dev(r, cuda)
    idx = torch.full((total + 2 * pad,), -7, dtype=torch.int32, device=cuda)
    d2 = torch.full((total + 2 * pad,), -7.0, dtype=torch.float32, device=cuda)

    def fill(offsets):
        o = _dev(offsets.astype(np.int32) + np.int32(pad), cuda)
        st = gh._lib.grace_range_neighbours_f4(gh._ptr(pd), C.c_size_t(len(pts)), C.c_int(3), gh._ptr(rd), C.c_float(0.0),
                                               *gh._interp_scene(d, tree), gh._ptr(o), gh._ptr(idx), gh._ptr(d2),
                                               gh._stream())
        assert st == gh.GRACE_OK
        torch.cuda.synchronize()
        return idx.cpu().numpy(), d2.cpu().numpy()

    gi, gd = fill(bad)
    with pytest.raises(ValueError):                                # GRACE_INVALID_ARGUMENT in the status word
        gh.trace_status()
    gh.trace_status()                                              # read and cleared
    assert np.all(gi[:pad] == -7) and np.all(gi[pad + total:] == -7)
    assert np.all(gd[:pad] == -7.0) and np.all(gd[pad + total:] == -7.0)
    exp_i = np.full(total, -7, np.int32); exp_d = np.full(total, -7.0, F32)
    for p in range(len(pts)):
        n_row = min(bad[p + 1] - bad[p], counts[p])                # the short row is truncated
        exp_i[bad[p]:bad[p] + n_row] = r_idx[off[p]:off[p] + n_row]
        exp_d[bad[p]:bad[p] + n_row] = r_d2[off[p]:off[p] + n_row]
    assert np.array_equal(gi[pad:pad + total], exp_i) and _same(gd[pad:pad + total], exp_d)
    assert gi[pad + bad[long_ + 1] - 1] == -7                      # the long row's tail keeps the sentinel
    idx.fill_(-7); d2.fill_(-7.0)
    gi, gd = fill(off)                                             # a following correct call
    gh.trace_status()
    assert np.array_equal(gi[pad:pad + total], r_idx) and _same(gd[pad:pad + total], r_d2)
    assert np.all(gi[:pad] == -7) and np.all(gi[pad + total:] == -7)


@pytest.mark.gpu
def test_bad_arguments_write_nothing(gh, built, cuda):
    import torch
    d, tree, sh = built["random"]
    n = len(sh)
    pts = torch.rand((100, 4), dtype=torch.float32, device=cuda)
    rad = torch.full((100,), 0.05, dtype=torch.float32, device=cuda)
    w = torch.ones((n, 2), dtype=torch.float32, device=cuda)
    cnt = torch.full((100,), 7, dtype=torch.int32, device=cuda)
    sums = torch.full((100, 2), 7.0, dtype=torch.float32, device=cuda)
    off = torch.zeros(101, dtype=torch.int32, device=cuda)
    idx = torch.full((100,), 7, dtype=torch.int32, device=cuda)
    dd = torch.full((100,), 7.0, dtype=torch.float32, device=cuda)
    scene = gh._interp_scene(d, tree)
    lib = gh._lib

    def counts(elems=4, rp=rad, radius=0.0, sc=scene, wp=w, n_ch=2, cp=cnt, sp=sums):
        return lib.grace_range_counts_f4(gh._ptr(pts), C.c_size_t(100), C.c_int(elems), gh._ptr(rp), C.c_float(radius),
                                         *sc, gh._ptr(wp), C.c_int(n_ch), gh._ptr(cp), gh._ptr(sp), gh._stream())

    def lists(elems=4, rp=rad, radius=0.0, sc=scene, op=off, ip=idx, dp=dd):
        return lib.grace_range_neighbours_f4(gh._ptr(pts), C.c_size_t(100), C.c_int(elems), gh._ptr(rp),
                                             C.c_float(radius), *sc, gh._ptr(op), gh._ptr(ip), gh._ptr(dp), gh._stream())

    empty = list(scene); empty[1] = C.c_size_t(0)
    no_leaves = list(scene); no_leaves[4] = C.c_void_p(0)
    common = (dict(elems=2), dict(elems=17), dict(sc=empty), dict(sc=no_leaves), dict(rp=None, radius=-1.0),
              dict(rp=None, radius=float("nan")), dict(rp=None, radius=float("inf")))
    for kw in common + (dict(n_ch=0), dict(n_ch=65), dict(wp=None), dict(cp=None, sp=None)):
        assert counts(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    for kw in common + (dict(op=None), dict(ip=None, dp=None)):
        assert lists(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    torch.cuda.synchronize()
    assert torch.all(cnt == 7) and torch.all(sums == 7.0) and torch.all(idx == 7) and torch.all(dd == 7.0)
    with pytest.raises(ValueError):
        gh.range_counts_sph(pts, rad[:50], d, tree)
    with pytest.raises(ValueError):
        gh.range_counts_sph(pts, -1.0, d, tree)
    with pytest.raises(ValueError):
        gh.range_counts_sph(pts, rad, d, tree, weights=torch.ones(n - 1, dtype=torch.float32, device=cuda))
    # accepted: counts alone, sums alone, one list output only (empty rows: offsets all 0)
    assert counts(wp=None, n_ch=0, sp=None) == gh.GRACE_OK and counts(cp=None) == gh.GRACE_OK
    cnt0 = torch.zeros(100, dtype=torch.int32, device=cuda)
    neg = torch.full((100,), -1.0, dtype=torch.float32, device=cuda)
    assert counts(rp=neg, cp=cnt0, wp=None, n_ch=0, sp=None) == gh.GRACE_OK
    assert lists(rp=neg, ip=None) == gh.GRACE_OK and lists(rp=neg, dp=None) == gh.GRACE_OK
    gh.trace_status()
    assert torch.all(cnt0 == 0)


@pytest.mark.gpu
def test_range_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    d, tree = _build(gh, _random_scene(9000, 41), cuda)
    s = d.cpu().numpy()                                            # tree order
    rng = np.random.default_rng(3)
    pts = rng.random((777, 4), dtype=F32)
    r = np.exp(rng.uniform(np.log(1e-3), np.log(0.15), len(pts))).astype(F32)
    n_ch, radius = 3, 0.0625
    w = (0.5 + rng.random((len(s), n_ch))).astype(F32)
    for name, a in (("s", s), ("p", pts), ("r", r), ("w", w)):
        a.tofile(str(tmp_path / (name + ".f32")))
    exe = str(tmp_path / "dropin_range")
    _compile_dropin(exe)
    res = subprocess.run([exe, *(str(tmp_path / (x + ".f32")) for x in "sprw"), str(n_ch), str(radius)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    names = ("counts", "sums", "counts_one", "offsets", "indices", "d2")
    got = {t[0]: (int(t[1]), int(t[2])) for t in (ln.split() for ln in res.stdout.splitlines())
           if len(t) == 3 and t[0] in names}
    cnt, sums = _counts(gh, pts, r, d, tree, cuda, weights=_dev(w, cuda))
    one, _ = _counts(gh, pts, radius, d, tree, cuda)
    off, idx, d2 = _lists(gh, pts, r, d, tree, cuda)
    exp = {"counts": cnt, "sums": sums, "counts_one": one, "offsets": off, "indices": idx, "d2": d2}
    assert set(got) == set(exp)
    for name, a in exp.items():
        assert got[name] == digest(a), name
    assert cnt.max() > 64 and np.array_equal(cnt, restate(pts, r, s)[0])


@pytest.mark.gpu
def test_scale_million_clustered(gh, cuda):
    n, k = 1_000_000, 32
    s = _clustered_scene(n, 21)
    d, tree = _build(gh, s, cuda)
    h = gh.smoothing_lengths_sph(d, tree, k, 1.0, check=True)
    cnt, _ = gh.range_counts_sph(d, h, d, tree, check=True)         # check=True: the stack holds
    cnt = cnt.cpu().numpy()
    sh, hh = d.cpu().numpy(), h.cpu().numpy()
    rows = np.sort(np.random.default_rng(5).choice(n, 2000, replace=False))
    # The restatement over the slab of spheres near each sampled particle in x instead of all 10^6: a
    # sphere in range has fl(dx*dx) <= fl(r*r), so |dx| < 1.001 r + 1e-6, and the slab drops none of those.
    order = np.argsort(sh[:, 0], kind="stable")
    xs = sh[order, 0].astype(np.float64)
    for i in rows:
        margin = 1.001 * float(hh[i]) + 1e-6
        lo, hi = np.searchsorted(xs, [float(sh[i, 0]) - margin, float(sh[i, 0]) + margin])
        slab = sh[order[max(lo - 1, 0):hi + 1]]
        assert cnt[i] == restate(sh[i:i + 1], hh[i:i + 1], slab)[0][0], i
    assert cnt.min() >= 1                                          # every particle finds itself
