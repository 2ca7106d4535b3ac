"""Pair counts in separation bins and radial profiles (grace_pair_counts_f4, pair_counts_sph /
radial_profiles_sph, an extension the reference lacks) against a NumPy restatement of the contract in
include/grace_hip.h.

d2 is the range queries' fp32 sequence (d2_rows of test_neighbours.py); E2_k = fl(e_k * e_k); the bin of
a pair is the smallest k with d2 <= E2_k, i.e. np.searchsorted(E2, d2, side="left"); entries that land
at n_edges (d2 beyond the last edge, and NaN) are dropped.  Counts are a bincount, totals their sum over
the points in 64 bits, sums a sequential float32 accumulation of the weights in ascending tree index
(np.add.accumulate, never a pairwise sum).  Counts and totals are compared with array_equal, sums on
their bit patterns: no tolerance anywhere."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_neighbours import (SCENES, _build, _clustered_scene, _lattice_scene, _point_sets, _random_scene,
                             built, d2_rows)  # noqa: F401  (built: the module's scenes fixture)
from test_range_queries import digest
from test_range_queries import restate as restate_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32 = np.float32
R_MAX = {"random": 0.2, "clustered": 0.002, "lattice": 0.3, "coincident": 0.3}   # a few hundred centres in range


def f32(*v):
    return np.array(v, F32).reshape(-1)


def log_edges(lo, hi, n):
    e = np.exp(np.linspace(np.log(lo), np.log(hi), n)).astype(F32)
    assert np.all(np.diff(e) > 0)
    return e


def edge_lists(scene):
    """One edge, 9 (with e_0 = 0), 16 and 64 (with e_0 = 0) edges: with bin capacities of 8, 16 and 64
    these are one list per capacity and one just past a boundary; on the lattice also edges exactly at
    and one ulp below the first two site distances."""
    r = R_MAX[scene]
    lists = {"one": f32(r / 2), "zero+8": np.concatenate([f32(0), log_edges(r / 50, r, 8)]),
             "16": log_edges(r / 100, r, 16), "zero+63": np.concatenate([f32(0), log_edges(r / 100, r, 63)])}
    if scene == "lattice":
        a, b = F32(1.0 / 16.0), F32(1.0 / 8.0)
        lists["ties"] = f32(np.nextafter(a, F32(0)), a, np.nextafter(b, F32(0)), b)
    return lists


ALL_IN_RANGE = f32(0.05, 0.5, 4.0)          # the last edge is beyond the unit box's diagonal


# ---- the restatement ----------------------------------------------------------------------------
def restate(points, edge_lists_, spheres, weights=None):
    """For each edge list: (totals uint64 [E], counts int32 [m, E], sums float32 [m, E, C] or None) of the
    contract; weights: float32 [n, C] or None.  d2 is computed once for all lists."""
    P = np.ascontiguousarray(points[:, :3], F32)
    X = np.ascontiguousarray(spheres[:, :3], F32)
    m = len(P)
    E2s = [(np.asarray(e, F32) * np.asarray(e, F32)).astype(F32) for e in edge_lists_]
    counts = [np.zeros((m, len(E2)), np.int64) for E2 in E2s]
    sums = [None if weights is None else np.zeros((m, len(E2), weights.shape[1]), F32) for E2 in E2s]
    chunk = max(1, (1 << 22) // max(len(X), 1))
    for a in range(0, m, chunk):
        with np.errstate(over="ignore", invalid="ignore"):
            d2 = d2_rows(P[a:a + chunk], X)
        rows = len(d2)
        for E2, cnt, sm in zip(E2s, counts, sums):
            ne = len(E2)
            with np.errstate(invalid="ignore"):
                pi, si = np.nonzero(d2 <= E2[-1])              # row-major: ascending sphere index within a point
            k = np.searchsorted(E2, d2[pi, si], side="left")   # (the mask only spares the search: k < ne there)
            assert np.all(k < ne)
            cell = pi * ne + k
            per_cell = np.bincount(cell, minlength=rows * ne)
            cnt[a:a + rows] = per_cell.reshape(rows, ne)
            if sm is None or len(cell) == 0:
                continue
            order = np.argsort(cell, kind="stable")            # inside a cell: still ascending sphere index
            start = np.concatenate([[0], np.cumsum(per_cell)])[cell[order]]
            rank = np.arange(len(cell)) - start
            for c in range(weights.shape[1]):
                terms = np.zeros((rows * ne, int(per_cell.max())), F32)
                terms[cell[order], rank] = weights[si[order], c]
                acc = np.add.accumulate(terms, axis=1, dtype=F32)[:, -1]   # sequential; fl(x + 0) = x past a cell's end
                sm[a:a + rows, :, c] = acc.reshape(rows, ne)
    return [(cnt.sum(axis=0).astype(np.uint64), cnt.astype(np.int32), sm) for cnt, sm in zip(counts, sums)]


def restate_all_lists_naive(points, edges, spheres):
    """The same counts with np.searchsorted over every d2 (NaN and out of range land at n_edges)."""
    e = np.asarray(edges, F32)
    E2 = (e * e).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        d2 = d2_rows(np.ascontiguousarray(points[:, :3], F32), np.ascontiguousarray(spheres[:, :3], F32))
    k = np.searchsorted(E2, d2, side="left")
    return np.array([np.bincount(row[row < len(E2)], minlength=len(E2)) for row in k]).astype(np.int32)


def query_points(sh):
    """About 3000 points: random ones in and around the box, sphere centres, far ones, binary-exact ones
    and four with a non-finite coordinate."""
    sets = _point_sets(sh)
    off = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan]], F32)
    pts = np.concatenate([sets["random"], sets["centres"], sets["far"], sets["exact"], off]).astype(F32)
    return pts[np.random.default_rng(31).permutation(len(pts))]


_ref_cache = {}


def reference(scene, sh):
    """(points, {list name: (edges, totals, counts)}) of a scene (tree order sh), computed once."""
    if scene not in _ref_cache:
        pts = query_points(sh)
        lists = edge_lists(scene)
        res = restate(pts, list(lists.values()), sh)
        _ref_cache[scene] = (pts, {name: (e, r[0], r[1]) for (name, e), r in zip(lists.items(), res)})
    return _ref_cache[scene]


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- CPU ------------------------------------------------------------------------------------------
def test_pair_symbol_exported():
    lib = C.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    assert hasattr(lib, "grace_pair_counts_f4")


def _compile_dropin(exe):
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, os.path.join(ROOT, "tests", "cpp", "dropin_pairs.hip"),
                           "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


def test_pairs_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_pairs"
    _compile_dropin(exe)
    assert exe.exists()


@pytest.mark.parametrize("call", ["grace::pair_counts_sph(p, e, s, t, tot);",
                                  "grace::radial_profiles_sph(p, e, s, t, cnt);",
                                  "grace::radial_profiles_sph(p, e, s, t, cnt, w, 1, sums);"])
def test_pairs_double4_is_a_clear_compile_error(tmp_path, call):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/pairs_sph.cuh"\n'
                   "void f(const thrust::device_vector<float4>& p, const thrust::device_vector<double4>& s,\n"
                   "       const std::vector<float>& e, const thrust::device_vector<float>& w, const grace::Tree& t,\n"
                   "       thrust::device_vector<unsigned long long>& tot, thrust::device_vector<int>& cnt,\n"
                   "       thrust::device_vector<float>& sums)\n"
                   "{ " + call + " }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "float4 spheres only" in res.stderr


def test_pairs_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& p, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::device_vector<float>& w, const grace::Tree& t)\n"
                   "{\n"
                   "    std::vector<float> edges(3, 0.0f);\n"
                   "    edges[1] = 0.125f; edges[2] = 0.25f;\n"
                   "    grace::device_vector<unsigned long long> totals;\n"
                   "    grace::device_vector<int> counts;\n"
                   "    grace::device_vector<float> sums;\n"
                   "    grace::pair_counts_sph(p, edges, s, t, totals);\n"
                   "    grace::radial_profiles_sph(p, edges, s, t, counts);\n"
                   "    grace::radial_profiles_sph(p, edges, s, t, counts, w, 2, sums);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


def test_restatement_edges():
    #              d2 = 0        1          4          0          9          1 (two squares)
    s = np.array([[0, 0, 0, 9], [1, 0, 0, 9], [2, 0, 0, 9], [0, 0, 0, 9], [3, 0, 0, 9], [0, -1, 0, 9]], F32)
    pts = np.zeros((2, 3), F32)
    pts[1, 0] = np.nan
    w = np.array([[1], [2], [4], [8], [16], [32]], F32)
    (tot, cnt, sums), = restate(pts, [f32(0, 1, 2)], s, w)
    assert cnt.tolist() == [[2, 2, 1], [0, 0, 0]]                 # d2 == E2_k is in bin k; e_0 = 0: the coincident pairs
    assert tot.tolist() == [2, 2, 1] and tot.dtype == np.uint64
    assert sums[:, :, 0].tolist() == [[9, 34, 4], [0, 0, 0]]      # the sphere at d2 = 9 is in no bin; NaN: zeros
    # E2 ties: fl(1e-30^2) == fl(2e-30^2) == 0, so the upper of the two bins is empty
    e = f32(1e-30, 2e-30, 1.5)
    assert (e * e)[0] == 0 and (e * e)[1] == 0
    (tot, cnt, _), = restate(pts, [e], s)
    assert cnt.tolist() == [[2, 0, 2], [0, 0, 0]]
    # one ulp below an edge that a distance meets exactly: the pair moves up one bin
    below = np.nextafter(F32(1), F32(0))
    (tot, cnt, _), = restate(pts, [f32(below, 1, 2)], s)
    assert cnt.tolist() == [[2, 2, 1], [0, 0, 0]]
    (tot, cnt, _), = restate(pts, [f32(below, 2)], s)
    assert cnt.tolist() == [[2, 3], [0, 0]]
    # the sequential sum is not the pairwise one: 2^24 + 1 + 1 stays 2^24 term by term
    s3 = np.zeros((3, 4), F32)
    (tot, cnt, sums), = restate(pts[:1], [f32(0)], s3, f32(2 ** 24, 1, 1)[:, None])
    assert sums[0, 0, 0] == F32(2 ** 24) and cnt.tolist() == [[3]]
    # the masked search and the plain np.searchsorted over every d2 agree
    rng = np.random.default_rng(8)
    s = rng.random((500, 4), dtype=F32)
    pts = np.concatenate([rng.random((60, 3), dtype=F32), s[:30, :3], pts[1:]])
    e = np.concatenate([f32(0), log_edges(0.01, 0.4, 12)])
    (tot, cnt, _), = restate(pts, [e], s)
    assert np.array_equal(cnt, restate_all_lists_naive(pts, e, s)) and cnt[60:90, 0].tolist() == [1] * 30


def test_restated_prefix_sums_are_the_restated_range_counts():
    s = _random_scene(3000, 4)
    rng = np.random.default_rng(14)
    pts = np.concatenate([rng.random((300, 3), dtype=F32) * F32(1.1) - F32(0.05), s[:200, :3]])
    pts[7, 1] = np.nan
    e = np.concatenate([f32(0), log_edges(0.01, 0.3, 10)])
    (tot, cnt, _), = restate(pts, [e], s)
    cum = cnt.cumsum(axis=1)
    for k, ek in enumerate(e):
        assert np.array_equal(cum[:, k], restate_range(pts, np.full(len(pts), ek, F32), s)[0]), k
    assert np.array_equal(tot, cnt.sum(axis=0).astype(np.uint64)) and cum[:, -1].max() > 256 and np.all(cnt[7] == 0)
    assert cnt[300:, 0].tolist() == [1] * 200                     # e_0 = 0: a centre finds itself only


# ---- GPU --------------------------------------------------------------------------------------------
def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _totals(gh, pts, edges, d, tree, cuda):
    import torch
    t = gh.pair_counts_sph(_dev(np.asarray(pts, F32), cuda), edges, d, tree, check=True)
    assert t.dtype == torch.uint64 and tuple(t.shape) == (len(edges),)
    return t.cpu().numpy()


def _profiles(gh, pts, edges, d, tree, cuda, weights=None):
    cnt, sums = gh.radial_profiles_sph(_dev(np.asarray(pts, F32), cuda), edges, d, tree, weights=weights, check=True)
    assert tuple(cnt.shape) == (len(pts), len(edges))
    return cnt.cpu().numpy(), None if sums is None else sums.cpu().numpy()


def _check(got_totals, got_counts, ref_totals, ref_counts, what):
    bad = np.argwhere(got_counts != ref_counts)
    assert got_counts.dtype == np.int32 and len(bad) == 0, (what, bad[:5], got_counts[tuple(bad[:5].T)],
                                                            ref_counts[tuple(bad[:5].T)])
    assert got_totals.dtype == np.uint64 and np.array_equal(got_totals, ref_totals), (what, got_totals, ref_totals)


@pytest.fixture
def kernel_reset(gh):
    yield
    gh.set_sph_kernel("cubic")


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_totals_and_counts_are_the_restatement_bit_for_bit(gh, built, scene, cuda):
    d, tree, sh = built[scene]
    pts, lists = reference(scene, sh)
    for name, (e, ref_totals, ref_counts) in lists.items():
        cnt, sums = _profiles(gh, pts, e, d, tree, cuda)
        assert sums is None
        _check(_totals(gh, pts, e, d, tree, cuda), cnt, ref_totals, ref_counts, (scene, name))
        assert ref_counts.sum(axis=1).max() > 256 or name in ("one", "ties")
    nan_rows = np.nonzero(~np.all(np.isfinite(pts), axis=1))[0]
    assert len(nan_rows) == 4 and np.all(lists["zero+8"][2][nan_rows] == 0)
    # the last edge beyond the scene's diagonal: every centre is in some bin of every point in the box
    sub = pts[::10]
    (ref_totals, ref_counts, _), = restate(sub, [ALL_IN_RANGE], sh)
    cnt, _ = _profiles(gh, sub, ALL_IN_RANGE, d, tree, cuda)
    _check(_totals(gh, sub, ALL_IN_RANGE, d, tree, cuda), cnt, ref_totals, ref_counts, (scene, "all"))
    inside = np.all((sub >= 0) & (sub <= 1), axis=1)
    assert inside.sum() > 100 and np.all(cnt[inside].sum(axis=1) == len(sh))
    if scene == "lattice":                                         # the ties d2 == E2, met from both sides
        rc = lists["ties"][2]
        at_site = np.nonzero((rc[:, 0] == 1) & (rc[:, 1] == 6))[0]   # a lattice site: itself, then 6 at exactly 1/16
        assert len(at_site) > 100 and rc[at_site, 3].max() == 6        # and 6 more at exactly 1/8
    if scene == "coincident":                                      # e_0 = 0: the coincident sets and nothing else
        same = np.nonzero(np.all(pts == np.array([0.625, 0.375, 0.125], F32), axis=1))[0]
        assert np.all(lists["zero+8"][2][same, 0] == 200)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_prefix_sums_are_the_range_counts_and_totals_the_column_sums(gh, built, scene, cuda):
    """The existing range query is the witness: counts.cumsum(1)[:, k] is its count at radius e_k."""
    d, tree, sh = built[scene]
    pts = query_points(sh)
    pd = _dev(pts, cuda)
    lists = edge_lists(scene)
    for name in ("zero+8", "zero+63") if scene == "random" else ("zero+8",):
        e = lists[name]
        cnt, _ = _profiles(gh, pts, e, d, tree, cuda)
        cum = cnt.cumsum(axis=1)
        for k, ek in enumerate(e):
            witness, _ = gh.range_counts_sph(pd, float(ek), d, tree, check=True)
            assert np.array_equal(cum[:, k], witness.cpu().numpy()), (name, k)
        assert np.array_equal(cnt.sum(axis=0, dtype=np.uint64), _totals(gh, pts, e, d, tree, cuda)), name
        assert cum[:, -1].max() > 256


@pytest.mark.gpu
def test_totals_past_32_bits_over_a_coincident_spine(gh, cuda):
    """2^16 + 64 coincident centres queried from themselves at e = 0: 65600^2 > 2^32 ordered pairs in bin 0,
    from a spine of leaves deeper than the stack (check=True raises if a packet exhausts it)."""
    n = 65600
    s = np.full((n, 4), 0.01, F32)
    s[:, :3] = np.array([0.25, 0.5, 0.75], F32)
    d, tree = _build(gh, s, cuda)
    totals = _totals(gh, d.cpu().numpy(), f32(0), d, tree, cuda)
    assert totals.tolist() == [n * n] and n * n > 2 ** 32
    cnt, _ = _profiles(gh, d.cpu().numpy()[:130], f32(0, 0.5), d, tree, cuda)
    assert np.all(cnt[:, 0] == n) and np.all(cnt[:, 1] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_edges,n_ch", [(64, 1), (16, 4), (9, 3), (5, 2), (1, 4)])
def test_sums_bit_for_bit(gh, built, n_edges, n_ch, cuda):
    for scene in ("random", "coincident"):
        d, tree, sh = built[scene]
        n = len(sh)
        pts = query_points(sh)[:400]
        pts[5] = np.array([0.5, np.nan, 0.5], F32)
        pts[6:26] = np.array([0.625, 0.375, 0.125] if scene == "coincident" else sh[77, :3], F32)
        e = np.concatenate([f32(0), log_edges(0.004, 0.12, n_edges - 1)]) if n_edges > 1 else f32(0.1)
        assert len(e) == n_edges
        w = (0.5 + np.random.default_rng(n_ch).random((n, n_ch))).astype(F32)
        (_, ref_counts, ref_sums), = restate(pts, [e], sh, w)
        cnt, sums = _profiles(gh, pts, e, d, tree, cuda, weights=_dev(w, cuda))
        assert np.array_equal(cnt, ref_counts) and ref_counts.sum(axis=1).max() > 64
        assert sums.dtype == F32 and _same(sums, ref_sums), (scene, n_edges, n_ch)
        assert np.all(sums[5] == 0) and np.all(cnt[5] == 0)        # the off point's rows
        if n_ch == 1:                                              # weights [n] give sums [m, E]
            c1, s1 = _profiles(gh, pts, e, d, tree, cuda, weights=_dev(w[:, 0], cuda))
            assert s1.shape == (len(pts), n_edges) and _same(s1, ref_sums[:, :, 0]) and np.array_equal(c1, cnt)


@pytest.mark.gpu
def test_results_do_not_depend_on_order_layout_tree_or_kernel(gh, cuda, kernel_reset):
    import torch
    base = _clustered_scene(12000, 8)
    base[:150, :3] = np.array([0.5, 0.25, 0.75], F32)              # a coincident group
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.random((700, 3), dtype=F32), base[:300, :3]])
    pts[3, 2] = np.nan
    e = np.concatenate([f32(0), log_edges(2e-4, 0.02, 8)])
    w = (0.5 + rng.random((len(base), 2))).astype(F32)

    def run(d, tree, wd, p=pts):
        cnt, sums = _profiles(gh, p, e, d, tree, cuda, weights=wd)
        return _totals(gh, p, e, d, tree, cuda), cnt, sums

    runs = []
    for hscale, mpl in ((0.0, 8), (3.0, 8), (1.0, 128), (0.0, 128)):   # H = 0 and large H; max_per_leaf 8 and 128
        s = base.copy()
        s[:, 3] *= F32(hscale)
        d = torch.from_numpy(s).to(cuda)
        tree = gh.Tree(len(s), mpl, device=cuda)
        tree, perm = gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_perm=True)
        wd = _dev(w, cuda)[perm.long()].contiguous()
        runs.append((d[:, :3].cpu().numpy(),) + run(d, tree, wd))
    x0, t0, c0, s0 = runs[0]
    (rt, rc, rs), = restate(pts, [e], x0, wd.cpu().numpy())
    assert np.array_equal(t0, rt) and np.array_equal(c0, rc) and _same(s0, rs) and c0.max() > 64
    for x, t, c, s in runs[1:]:
        assert np.array_equal(x, x0)                               # the same tree order
        assert np.array_equal(t, t0) and np.array_equal(c, c0) and _same(s, s0)
    order = rng.permutation(len(pts))                              # shuffled point order
    t, c, s = run(d, tree, wd, pts[order])
    assert np.array_equal(t, t0) and np.array_equal(c, c0[order]) and _same(s, s0[order])
    for elems in (3, 8):                                           # elems_per_point
        wide = np.full((len(pts), elems), 9.0, F32); wide[:, :3] = pts
        t, c, s = run(d, tree, wd, wide)
        assert np.array_equal(t, t0) and np.array_equal(c, c0) and _same(s, s0), elems
    gh.set_sph_kernel("wendland_c4")                               # no SPH kernel in the sums
    t, c, s = run(d, tree, wd)
    gh.set_sph_kernel("cubic")
    assert np.array_equal(t, t0) and np.array_equal(c, c0) and _same(s, s0)
    again = run(d, tree, wd)                                       # run to run
    assert [digest(a) for a in again] == [digest(a) for a in (t0, c0, s0)]


def _raw(gh, pts, edges, scene, w, n_ch, totals, counts, sums, n_points=None, elems=None, n_edges=None,
         null_edges=False):
    e = np.ascontiguousarray(edges, F32)
    return gh._lib.grace_pair_counts_f4(
        gh._ptr(pts), C.c_size_t(len(pts) if n_points is None else n_points),
        C.c_int(pts.shape[1] if elems is None else elems),
        C.c_void_p(0) if null_edges else e.ctypes.data_as(C.c_void_p), C.c_int(len(e) if n_edges is None else n_edges),
        *scene, gh._ptr(w), C.c_int(n_ch), gh._ptr(totals), gh._ptr(counts), gh._ptr(sums), gh._stream())


@pytest.mark.gpu
def test_small_shapes_and_single_outputs(gh, cuda):
    import torch
    # one sphere: a one-leaf tree without nodes
    one = torch.tensor([[0.25, 0.5, 0.75, 0.0]], dtype=torch.float32, device=cuda)
    t1 = gh.Tree(1, 1, device=cuda)
    t1.leaves[0] = torch.tensor([0, 1, 0, 0], dtype=torch.int32)
    t1.root_index.zero_()
    pts = np.array([[0.25, 0.5, 0.75], [0.0, 0.0, 0.0], [0.25, 0.5, 0.5], [9.0, 9.0, 9.0]], F32)
    e = f32(0, 0.25, 1.0)
    (rt, rc, _), = restate(pts, [e], one.cpu().numpy())
    assert rc.tolist() == [[1, 0, 0], [0, 0, 1], [0, 1, 0], [0, 0, 0]]
    cnt, _ = _profiles(gh, pts, e, one, t1, cuda)
    _check(_totals(gh, pts, e, one, t1, cuda), cnt, rt, rc, "one sphere")

    s = _random_scene(3000, 9)
    d, tree = _build(gh, s, cuda)
    sh = d.cpu().numpy()
    rng = np.random.default_rng(5)
    e = np.concatenate([f32(0), log_edges(0.01, 0.2, 8)])
    w = (0.5 + rng.random((len(sh), 2))).astype(F32)
    wd = _dev(w, cuda)
    for n in (1, 63, 64, 65):                                      # around a packet
        pts = np.concatenate([sh[:n // 2, :3], rng.random((n - n // 2, 3), dtype=F32)])
        (rt, rc, rs), = restate(pts, [e], sh, w)
        cnt, sums = _profiles(gh, pts, e, d, tree, cuda, weights=wd)
        _check(_totals(gh, pts, e, d, tree, cuda), cnt, rt, rc, n)
        assert _same(sums, rs), n
    # outputs one at a time: every combination of NULLs is the full call's
    scene = gh._interp_scene(d, tree)
    pd = _dev(pts, cuda)
    m, ne = len(pts), len(e)
    for want in itertools.product((False, True), repeat=3):
        if not any(want):
            continue
        tot = torch.full((ne,), -7, dtype=torch.int64, device=cuda) if want[0] else None
        cn = torch.full((m, ne), -7, dtype=torch.int32, device=cuda) if want[1] else None
        sm = torch.full((m, ne, 2), -7.0, dtype=torch.float32, device=cuda) if want[2] else None
        assert _raw(gh, pd, e, scene, wd if want[2] else None, 2 if want[2] else 0, tot, cn, sm) == gh.GRACE_OK, want
        gh.trace_status()
        assert tot is None or np.array_equal(tot.cpu().numpy().view(np.uint64), rt), want
        assert cn is None or np.array_equal(cn.cpu().numpy(), rc), want
        assert sm is None or _same(sm.cpu().numpy(), rs), want
    # zero points: GRACE_OK, the totals are zeroed, nothing else is written (null outputs are accepted)
    tot = torch.full((ne,), -7, dtype=torch.int64, device=cuda)
    cn = torch.full((m, ne), -7, dtype=torch.int32, device=cuda)
    assert _raw(gh, pd, e, scene, None, 0, tot, cn, None, n_points=0) == gh.GRACE_OK
    assert _raw(gh, pd, e, scene, None, 0, None, None, None, n_points=0) == gh.GRACE_OK
    torch.cuda.synchronize()
    assert torch.all(tot == 0) and torch.all(cn == -7)
    empty = gh.pair_counts_sph(torch.empty((0, 3), dtype=torch.float32, device=cuda), e, d, tree, check=True)
    assert empty.cpu().numpy().tolist() == [0] * ne
    cnt, sums = gh.radial_profiles_sph(torch.empty((0, 4), dtype=torch.float32, device=cuda), e, d, tree, weights=wd)
    assert tuple(cnt.shape) == (0, ne) and tuple(sums.shape) == (0, ne, 2)


@pytest.mark.gpu
def test_bad_arguments_write_nothing(gh, built, cuda):
    import torch
    d, tree, sh = built["random"]
    n = len(sh)
    pts = torch.rand((100, 4), dtype=torch.float32, device=cuda)
    good = f32(0, 0.05, 0.1)
    w = torch.ones((n, 2), dtype=torch.float32, device=cuda)
    tot = torch.full((65,), -7, dtype=torch.int64, device=cuda)
    cnt = torch.full((100, 65), -7, dtype=torch.int32, device=cuda)
    sums = torch.full((100, 65, 5), -7.0, dtype=torch.float32, device=cuda)
    scene = gh._interp_scene(d, tree)

    def call(edges=good, sc=scene, wp=w, n_ch=2, tp=tot, cp=cnt, sp=sums, **kw):
        return _raw(gh, pts, edges, sc, wp, n_ch, tp, cp, sp, **kw)

    empty = list(scene); empty[1] = C.c_size_t(0)
    no_leaves = list(scene); no_leaves[4] = C.c_void_p(0)
    no_root = list(scene); no_root[5] = C.c_void_p(0)
    nan, inf = float("nan"), float("inf")
    ramp = np.arange(1, 66, dtype=F32) / F32(100)
    cases = (dict(elems=2), dict(elems=17), dict(n_edges=0), dict(edges=ramp), dict(edges=ramp[:64], n_edges=65),
             dict(null_edges=True), dict(edges=f32(0.1, 0.05)), dict(edges=f32(0.05, 0.05)), dict(edges=f32(0, 0.1, 0.1)),
             dict(edges=f32(-0.1, 0.1)), dict(edges=f32(-0.0, -0.1)), dict(edges=f32(nan)), dict(edges=f32(0.1, nan)),
             dict(edges=f32(0.1, inf)), dict(wp=None), dict(n_ch=0), dict(n_ch=5), dict(edges=ramp[:13], n_ch=5),
             dict(edges=ramp[:17], n_ch=4), dict(edges=ramp[:33], n_ch=2), dict(tp=None, cp=None, sp=None),
             dict(sc=empty), dict(sc=no_leaves), dict(sc=no_root))
    for kw in cases:
        assert call(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    torch.cuda.synchronize()
    assert torch.all(tot == -7) and torch.all(cnt == -7) and torch.all(sums == -7.0)
    for bad in ([0.1, 0.05], [0.1, nan], [-1.0], [], list(ramp)):
        with pytest.raises(ValueError):
            gh.pair_counts_sph(pts, bad, d, tree)
    with pytest.raises(ValueError):
        gh.radial_profiles_sph(pts, good, d, tree, weights=torch.ones((n, 5), dtype=torch.float32, device=cuda))
    with pytest.raises(ValueError):
        gh.radial_profiles_sph(pts, ramp[:33], d, tree, weights=w)
    with pytest.raises(ValueError):
        gh.radial_profiles_sph(pts, good, d, tree, weights=w[:-1])
    # accepted: the caps themselves, -0 as an edge, sums alone
    assert call(edges=ramp[:64], wp=None, n_ch=0, sp=None) == gh.GRACE_OK
    w4 = torch.ones((n, 4), dtype=torch.float32, device=cuda)      # (named: alive until the call has run)
    assert call(edges=ramp[:16], wp=w4, n_ch=4) == gh.GRACE_OK
    assert call(edges=f32(-0.0, 0.1), tp=None, cp=None) == gh.GRACE_OK
    gh.trace_status()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_pairs_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    d, tree = _build(gh, _clustered_scene(9000, 41), cuda)
    s = d.cpu().numpy()                                            # tree order
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.random((400, 4), dtype=F32), s[:377]]).astype(F32)
    n_ch = 3
    e = np.concatenate([f32(0), log_edges(1e-4, 0.01, 11)])
    w = (0.5 + rng.random((len(s), n_ch))).astype(F32)
    for name, a in (("s", s), ("p", pts), ("w", w), ("e", e)):
        a.tofile(str(tmp_path / (name + ".f32")))
    exe = str(tmp_path / "dropin_pairs")
    _compile_dropin(exe)
    f = lambda x: str(tmp_path / (x + ".f32"))
    res = subprocess.run([exe, f("s"), f("p"), f("w"), str(n_ch), f("e")], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    names = ("totals", "counts_only", "counts", "sums")
    got = {t[0]: (int(t[1]), int(t[2])) for t in (ln.split() for ln in res.stdout.splitlines())
           if len(t) == 3 and t[0] in names}
    totals = _totals(gh, pts, e, d, tree, cuda)
    cnt, sums = _profiles(gh, pts, e, d, tree, cuda, weights=_dev(w, cuda))
    exp = {"totals": totals, "counts_only": cnt, "counts": cnt, "sums": sums}
    assert set(got) == set(exp)
    for name, a in exp.items():
        assert got[name] == digest(a), name
    assert cnt.sum(axis=1).max() > 64 and np.array_equal(cnt, restate(pts, [e], s)[0][1])
