"""Tree gravity (grace_gravity_moments_f4 / grace_gravity_points_f4, gravity_moments_sph / gravity_sph, an
extension the reference lacks) against the NumPy restatement of the contract in include/grace_hip.h
(gravity_cases.py), which is fed the tree read back from the device.  Everything is compared on bit
patterns -- moment records as uint32, outputs as uint64, counts with array_equal: no tolerance anywhere.
The scenes and the preconditions they are chosen for are checked without a GPU in test_gravity_cases.py."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import gravity_cases as G
from test_range_queries import digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32 = np.float32


# ---- CPU ------------------------------------------------------------------------------------------
def test_gravity_symbols_exported():
    import grace_hip
    lib = grace_hip.exported_symbols()
    assert hasattr(lib, "grace_gravity_moments_f4") and hasattr(lib, "grace_gravity_points_f4")


def _compile_dropin(exe):
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, os.path.join(ROOT, "tests", "cpp", "dropin_gravity.hip"),
                           "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


def test_gravity_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_gravity"
    _compile_dropin(exe)
    assert exe.exists()


@pytest.mark.parametrize("call", ["grace::gravity_moments_sph(s, m, t, mom);",
                                  "grace::gravity_sph(p, s, m, t, mom, 0.5f, 0.0f, out);",
                                  "grace::gravity_sph(p, s, m, t, mom, 0.5f, 0.0f, out, cnt);"])
def test_gravity_double4_is_a_clear_compile_error(tmp_path, call):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/gravity_sph.cuh"\n'
                   "void f(const thrust::device_vector<float4>& p, const thrust::device_vector<double4>& s,\n"
                   "       const thrust::device_vector<float>& m, const grace::Tree& t,\n"
                   "       thrust::device_vector<float>& mom, thrust::device_vector<double>& out,\n"
                   "       thrust::device_vector<int>& cnt)\n"
                   "{ " + call + " }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "float4 spheres only" in res.stderr


def test_gravity_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& p, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::device_vector<float>& m, const grace::Tree& t)\n"
                   "{\n"
                   "    grace::device_vector<float> moments;\n"
                   "    grace::device_vector<double> out;\n"
                   "    grace::device_vector<int> counts;\n"
                   "    grace::gravity_moments_sph(s, m, t, moments);\n"
                   "    grace::gravity_sph(p, s, m, t, moments, 0.5f, 0.0f, out);\n"
                   "    grace::gravity_sph(p, s, m, t, moments, 0.5f, 0.01f, out, counts);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


# ---- GPU --------------------------------------------------------------------------------------------
def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _setup(gh, s, mpl, cuda, masses=None):
    """A scene on the device and read back: spheres in tree order, the tree, masses, the moment records."""
    import torch
    d = _dev(np.ascontiguousarray(s, F32), cuda)
    if len(s) > mpl:
        tree = gh.Tree(len(s), mpl, device=cuda)
        gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))        # sorts d
    else:                                                              # one sphere: a one-leaf tree without nodes
        tree = gh.Tree(len(s), mpl, device=cuda)
        tree.leaves[0] = torch.tensor([0, len(s), 0, 0], dtype=torch.int32)
        tree.root_index.zero_()
    t = types.SimpleNamespace(d=d, tree=tree, sh=d.cpu().numpy(), nodes=tree.nodes.cpu().numpy(),
                              leaves=tree.leaves.cpu().numpy(), root=int(tree.root_index.item()))
    _set_masses(gh, t, G.masses_for(len(s)) if masses is None else masses, cuda)
    return t


def _set_masses(gh, t, masses, cuda):
    t.m = np.ascontiguousarray(masses, F32)
    t.md = _dev(t.m, cuda)
    t.mom = gh.gravity_moments_sph(t.d, t.md, t.tree)
    assert tuple(t.mom.shape) == (t.tree.n_nodes, 12)
    t.rec = t.mom.cpu().numpy().view(np.uint32)
    t.ref_rec = G.moments(t.nodes, t.leaves, t.root, t.sh, t.m)


def _run(gh, t, pts, theta, eps, cuda, want_counts=True):
    import torch
    out, cnt = gh.gravity_sph(_dev(np.asarray(pts, F32), cuda), t.d, t.md, t.tree, t.mom, theta=theta, eps=eps,
                              counts=True if want_counts else None, check=True)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(pts), 4)
    return out.cpu().numpy(), None if cnt is None else cnt.cpu().numpy()


def _restate(t, pts, theta, eps):
    return G.walk(t.nodes, t.leaves, t.root, t.sh, t.m, t.ref_rec, np.asarray(pts, F32), theta, eps)


def _check(got, ref, what):
    (out, cnt), (ref_out, ref_cnt) = got, ref
    bad = np.argwhere(cnt != ref_cnt)
    assert cnt.dtype == np.int32 and len(bad) == 0, (what, bad[:5], cnt[bad[:5, 0]], ref_cnt[bad[:5, 0]])
    bad = np.argwhere(out.view(np.uint64) != ref_out.view(np.uint64))
    assert out.dtype == np.float64 and len(bad) == 0, (what, bad[:5], out[bad[:5, 0]], ref_out[bad[:5, 0]])


def _check_walk(gh, t, pts, theta, eps, cuda, what):
    got = _run(gh, t, pts, theta, eps, cuda)
    ref = _restate(t, pts, theta, eps)
    _check(got, ref, what)
    return got


@pytest.fixture(scope="module")
def built(gh, cuda):
    return {(name, mpl): _setup(gh, gen(), mpl, cuda) for name, gen in G.SCENES.items() for mpl in G.LEAF_SIZES}


_direct = {}


def _direct_sum(name, t, pts, eps):
    """The tree-free direct sum of a scene (the tree order is the same for every max_per_leaf), once."""
    if (name, eps) not in _direct:
        _direct[name, eps] = (t.sh.copy(), G.direct_sum(pts, t.sh, t.m, eps))
    sh, ref = _direct[name, eps]
    assert np.array_equal(sh, t.sh)
    return ref


@pytest.fixture
def knobs_reset(gh):
    yield
    gh.set_sph_kernel("cubic")
    gh.set_cache_auto(True)
    gh.set_cache_validation(True)


@pytest.mark.gpu
@pytest.mark.parametrize("mpl", G.LEAF_SIZES)
@pytest.mark.parametrize("scene", list(G.SCENES))
def test_moments_are_the_restatement_bit_for_bit(built, scene, mpl):
    t = built[scene, mpl]
    assert t.rec.shape == t.ref_rec.shape and len(t.rec) == len(t.leaves) - 1
    bad = np.argwhere(t.rec != t.ref_rec)
    assert len(bad) == 0, (bad[:5], t.rec[bad[:5, 0]], t.ref_rec[bad[:5, 0]])
    assert G.max_stack_entries(t.nodes, t.leaves, t.root) < 128


@pytest.mark.gpu
@pytest.mark.parametrize("mpl", G.LEAF_SIZES)
@pytest.mark.parametrize("scene", list(G.SCENES))
def test_walk_is_the_restatement_bit_for_bit(gh, built, scene, mpl, cuda):
    t = built[scene, mpl]
    pts = G.query_points(t.sh)
    off = ~np.all(np.isfinite(pts), axis=1)
    for eps in G.SOFTENINGS:
        for theta in G.THETAS:
            out, cnt = got = _run(gh, t, pts, theta, eps, cuda)
            if theta == 0.0:                                   # the direct sum, whatever the tree
                _check(got, _direct_sum(scene, t, pts, eps), (scene, mpl, theta, eps, "direct"))
                assert np.all(cnt[~off] == (0, len(t.sh)))
            else:
                _check(got, _restate(t, pts, theta, eps), (scene, mpl, theta, eps))
                assert np.sum(np.all(cnt == (1, 0), axis=1)) >= 4            # the far points take the root
            assert off.sum() == 4 and np.all(out[off].view(np.uint64) == 0) and np.all(cnt[off] == 0)
            assert np.all(np.isfinite(out))
    out_only, none = _run(gh, t, pts, 0.7, 0.01, cuda, want_counts=False)      # the outputs alone
    assert none is None and np.array_equal(out_only.view(np.uint64), _run(gh, t, pts, 0.7, 0.01, cuda)[0].view(np.uint64))


@pytest.mark.gpu
def test_theta_zero_does_not_depend_on_the_tree(gh, cuda):
    import torch
    base = G.clustered_scene(2000, 8)
    pts = G.query_points(base, seed=13, n_random=200, n_centres=100)
    m_caller = G.masses_for(len(base), 31)
    runs = []
    for hscale, mpl in ((0.0, 1), (3.0, 1), (0.0, 8), (1.0, 32), (30.0, 32)):   # H = 0 and large H, every leaf size
        s = base.copy()
        s[:, 3] *= F32(hscale)
        d = torch.from_numpy(s).to(cuda)
        tree = gh.Tree(len(s), mpl, device=cuda)
        tree, perm = gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_perm=True)
        md = _dev(m_caller, cuda)[perm.long()].contiguous()
        mom = gh.gravity_moments_sph(d, md, tree)
        for eps in G.SOFTENINGS:
            out, cnt = gh.gravity_sph(_dev(pts, cuda), d, md, tree, mom, theta=0.0, eps=eps, counts=True, check=True)
            runs.append((eps, d[:, :3].cpu().numpy(), md.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy()))
    for eps in G.SOFTENINGS:
        same = [r for r in runs if r[0] == eps]
        _, x0, m0, out0, cnt0 = same[0]
        _check((out0, cnt0), G.direct_sum(pts, x0, m0, eps), ("direct", eps))
        for _, x, m, out, cnt in same[1:]:
            assert np.array_equal(x, x0) and np.array_equal(m, m0)         # the same tree order
            assert np.array_equal(out.view(np.uint64), out0.view(np.uint64)) and np.array_equal(cnt, cnt0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_trees(gh, n, cuda):
    s = np.array([[0.25, 0.5, 0.75, 0.01], [0.75, 0.25, 0.5, 0.01], [0.5, 0.75, 0.25, 0.01]], F32)[:n]
    t = _setup(gh, s, 1, cuda, masses=np.array([1.5, 0.25, 3.0], F32)[:n])
    assert t.tree.n_nodes == n - 1 and len(t.rec) == n - 1 and np.array_equal(t.rec, t.ref_rec)
    pts = np.concatenate([t.sh[:, :3], np.array([[0.5, 0.5, 0.5], [9.0, 9.0, 9.0], [0.0, np.nan, 0.0]], F32)])
    for theta in G.THETAS:
        for eps in G.SOFTENINGS:
            got = _check_walk(gh, t, pts, theta, eps, cuda, (n, theta, eps))
            if theta == 0.0:
                _check(got, G.direct_sum(pts, t.sh, t.m, eps), (n, eps, "direct"))
    if n == 1:                                                       # no nodes: a null moments pointer is accepted
        scene = gh._interp_scene(t.d, t.tree)
        assert t.mom.numel() == 0
        assert gh._lib.grace_gravity_moments_f4(*scene, gh._ptr(t.md), C.c_void_p(0), gh._stream()) == gh.GRACE_OK


@pytest.mark.gpu
def test_packet_sizes(gh, built, cuda):
    t = built["random", 8]
    pts = G.packet_points()                                          # 63, 64 and 65 points in cells of their own
    _check_walk(gh, t, pts, 0.5, 0.0, cuda, "cells")
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65):                                        # around one packet
        p = np.concatenate([t.sh[:n // 2, :3], rng.random((n - n // 2, 3), dtype=F32)])
        _check_walk(gh, t, p, 0.5, 0.01, cuda, n)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(G.SCENES))
def test_mixed_decisions_in_one_packet(gh, built, scene, cuda):
    t = built[scene, 8]
    pts, node = G.mixed_points(t.ref_rec)
    out, cnt = _check_walk(gh, t, pts, 0.7, 0.0, cuda, scene)
    took_root = np.all(cnt == (1, 0), axis=1)
    assert node == t.root and 8 < took_root.sum() < 56 and np.all(cnt[~took_root, 0] > 1)
    deeper = G.mixed_points(t.ref_rec, node=int(t.nodes[t.root, 0]))[0]      # and about the root's left child
    _, cnt = _check_walk(gh, t, deeper, 0.7, 0.01, cuda, (scene, "left"))
    assert len(np.unique(cnt[:, 0])) > 1


@pytest.mark.gpu
def test_points_on_node_faces_and_one_ulp_outside(gh, built, cuda):
    for mpl in (1, 8):
        t = built["random", mpl]
        on, outside, which = G.face_points(t.ref_rec)
        for theta in (G.FACE_THETA, 1000.0, 0.7):
            _, c_on = _check_walk(gh, t, on, theta, 0.0, cuda, ("on", mpl, theta))
            _, c_out = _check_walk(gh, t, outside, theta, 0.0, cuda, ("outside", mpl, theta))
        _, c_on = _run(gh, t, on, G.FACE_THETA, 0.0, cuda)
        _, c_out = _run(gh, t, outside, G.FACE_THETA, 0.0, cuda)
        at_root = which == t.root
        assert at_root.sum() == 6 and np.all(c_out[at_root] == (1, 0)) and np.all(c_on[at_root, 0] > 1)


@pytest.mark.gpu
def test_leaf_ranges_across_cluster_boundaries(gh, cuda):
    t = _setup(gh, G.random_scene(200, 4), 32, cuda)
    first, end = t.leaves[:, 0], t.leaves[:, 0] + t.leaves[:, 1]
    assert np.sum((first >> 6) != ((end - 1) >> 6)) >= 1 and np.array_equal(t.rec, t.ref_rec)
    pts = G.query_points(t.sh, n_random=120, n_centres=200)
    for theta in G.THETAS:
        _check_walk(gh, t, pts, theta, 0.0, cuda, theta)


@pytest.mark.gpu
def test_coincident_spine(gh, cuda):
    """300 coincident centres under max_per_leaf = 1: a spine of leaves deeper than the stack, which the
    merged ranges keep off it (check=True raises on an overflow), size-0 nodes, d2 == 0 terms."""
    t = _setup(gh, G.spine_scene(), 1, cuda)
    assert len(t.leaves) == 350 and np.array_equal(t.rec, t.ref_rec)
    assert G.max_stack_entries(t.nodes, t.leaves, t.root) < 128
    rng = np.random.default_rng(3)
    near = G.SPINE_AT + (rng.random((40, 3), dtype=F32) - F32(0.5)) * F32(1e-3)
    pts = np.concatenate([np.tile(G.SPINE_AT, (70, 1)), near, t.sh[300:, :3], rng.random((60, 3), dtype=F32),
                          np.array([[40.0, 0.5, 0.5]], F32)]).astype(F32)
    for theta in G.THETAS:
        for eps in G.SOFTENINGS:
            out, cnt = _check_walk(gh, t, pts, theta, eps, cuda, (theta, eps))
    others = ~np.all(t.sh[:, :3] == G.SPINE_AT, axis=1)                 # the 300 coincident terms contribute nothing
    ref0, _ = G.direct_sum(pts[:1], t.sh[others], t.m[others], 0.01)
    out0, cnt0 = _run(gh, t, pts[:1], 0.0, 0.01, cuda)
    assert cnt0.tolist() == [[0, 350]] and np.array_equal(out0.view(np.uint64), ref0.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("mpl", G.LEAF_SIZES)
def test_zero_masses_a_massless_leaf_and_a_massless_node(gh, mpl, cuda):
    t = _setup(gh, G.random_scene(2000, 6), mpl, cuda)
    m0, node = G.zero_mass_node(G.zero_mass_leaf(t.m, t.leaves, len(t.leaves) // 2), t.ref_rec)
    _set_masses(gh, t, m0, cuda)
    assert np.array_equal(t.rec, t.ref_rec)
    c, M32, lo, _, _, _ = G.record_fields(t.rec)
    assert M32[node] == 0 and np.array_equal(c[node], lo[node])
    pts = G.query_points(t.sh, n_random=300, n_centres=100)
    for theta in (0.0, 0.7, 1000.0):
        _check_walk(gh, t, pts, theta, 0.0, cuda, (mpl, theta))


@pytest.mark.gpu
def test_moments_at_scale_across_workgroups(gh, cuda):
    """2 10^5 clustered particles, one per leaf: hundreds of workgroups on every XCD hand their fp64
    partial sums up the tree to each other."""
    t = _setup(gh, G.clustered_scene(200000, 5), 1, cuda)
    assert len(t.leaves) > 150000 and t.rec.shape == t.ref_rec.shape
    bad = np.argwhere(t.rec != t.ref_rec)
    assert len(bad) == 0, (len(bad), bad[:5], t.rec[bad[:5, 0]], t.ref_rec[bad[:5, 0]])
    again = gh.gravity_moments_sph(t.d, t.md, t.tree).cpu().numpy().view(np.uint32)
    assert np.array_equal(again, t.rec)
    pts = np.concatenate([t.sh[::40000, :3], np.array([[0.5, 0.5, 0.5], [3.0, 0.5, 0.5]], F32)])
    _check_walk(gh, t, pts, 0.5, 0.0, cuda, "walk")


@pytest.mark.gpu
def test_results_do_not_depend_on_order_layout_knobs_or_stream(gh, built, cuda, knobs_reset):
    import torch
    t = built["clustered", 8]
    pts = G.query_points(t.sh)
    out0, cnt0 = _check_walk(gh, t, pts, 0.5, 0.01, cuda, "base")

    def same(got, order=None):
        out, cnt = got
        ref_out, ref_cnt = (out0, cnt0) if order is None else (out0[order], cnt0[order])
        return np.array_equal(out.view(np.uint64), ref_out.view(np.uint64)) and np.array_equal(cnt, ref_cnt)

    order = np.random.default_rng(2).permutation(len(pts))           # shuffled point order
    assert same(_run(gh, t, pts[order], 0.5, 0.01, cuda), order)
    for elems in (3, 7):                                             # elems_per_point
        wide = np.full((len(pts), elems), 9.0, F32); wide[:, :3] = pts
        assert same(_run(gh, t, wide, 0.5, 0.01, cuda)), elems
    gh.set_sph_kernel("wendland_c4")                                 # no SPH kernel in it
    assert same(_run(gh, t, pts, 0.5, 0.01, cuda))
    gh.set_sph_kernel("cubic")
    gh.set_cache_auto(False)                                         # nor the trace's caches
    gh.set_cache_validation(False)
    assert same(_run(gh, t, pts, 0.5, 0.01, cuda))
    gh.set_cache_auto(True)
    gh.set_cache_validation(True)
    stream = torch.cuda.Stream(device=cuda)                          # a stream of the caller's
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        mom = gh.gravity_moments_sph(t.d, t.md, t.tree)
        got = _run(gh, t, pts, 0.5, 0.01, cuda)
    stream.synchronize()
    assert np.array_equal(mom.cpu().numpy().view(np.uint32), t.rec) and same(got)
    assert same(_run(gh, t, pts, 0.5, 0.01, cuda))                    # run to run


def _raw(gh, t, pts, out, cnt, theta=0.5, eps=0.0, scene=None, masses="own", moments="own", n_points=None,
         elems=None):
    scene = gh._interp_scene(t.d, t.tree) if scene is None else scene
    return gh._lib.grace_gravity_points_f4(
        gh._ptr(pts), C.c_size_t(len(pts) if n_points is None else n_points),
        C.c_int(pts.shape[1] if elems is None else elems), *scene,
        gh._ptr(t.md if isinstance(masses, str) else masses), gh._ptr(t.mom if isinstance(moments, str) else moments),
        C.c_float(theta), C.c_float(eps), gh._ptr(out), gh._ptr(cnt), gh._stream())


@pytest.mark.gpu
def test_bad_arguments_write_nothing(gh, built, cuda):
    import torch
    t = built["random", 8]
    pts = torch.rand((100, 4), dtype=torch.float32, device=cuda)
    out = torch.full((100, 4), -7.0, dtype=torch.float64, device=cuda)
    cnt = torch.full((100, 2), -7, dtype=torch.int32, device=cuda)
    mom = torch.full((t.tree.n_nodes, 12), -7.0, dtype=torch.float32, device=cuda)
    scene = gh._interp_scene(t.d, t.tree)
    empty = list(scene); empty[1] = C.c_size_t(0)
    no_leaves = list(scene); no_leaves[4] = C.c_void_p(0)
    no_root = list(scene); no_root[5] = C.c_void_p(0)
    no_nodes = list(scene); no_nodes[2] = C.c_void_p(0)
    nan, inf = float("nan"), float("inf")
    cases = (dict(theta=-0.5), dict(theta=nan), dict(theta=inf), dict(eps=-0.01), dict(eps=nan), dict(eps=inf),
             dict(elems=2), dict(elems=17), dict(masses=None), dict(moments=None), dict(scene=empty),
             dict(scene=no_leaves), dict(scene=no_root), dict(scene=no_nodes))
    for kw in cases:
        assert _raw(gh, t, pts, out, cnt, **kw) == gh.GRACE_INVALID_ARGUMENT, kw
    assert _raw(gh, t, pts, None, None) == gh.GRACE_INVALID_ARGUMENT                 # no output
    for sc, md in ((empty, t.md), (no_leaves, t.md), (no_root, t.md), (no_nodes, t.md), (scene, None)):
        assert gh._lib.grace_gravity_moments_f4(*sc, gh._ptr(md), gh._ptr(mom), gh._stream()) == gh.GRACE_INVALID_ARGUMENT
    assert gh._lib.grace_gravity_moments_f4(*scene, gh._ptr(t.md), C.c_void_p(0), gh._stream()) == gh.GRACE_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(cnt == -7) and torch.all(mom == -7.0)
    for kw in (dict(theta=-1.0), dict(eps=-1.0), dict(theta=nan), dict(eps=inf)):
        with pytest.raises(ValueError):
            gh.gravity_sph(pts, t.d, t.md, t.tree, t.mom, **kw)
    with pytest.raises(ValueError):
        gh.gravity_sph(pts, t.d, t.md[:-1], t.tree, t.mom)
    with pytest.raises(ValueError):
        gh.gravity_sph(pts, t.d, t.md, t.tree, t.mom[:-1])
    with pytest.raises(ValueError):
        gh.gravity_sph(pts[:, :2], t.d, t.md, t.tree, t.mom)
    with pytest.raises(ValueError):
        gh.gravity_moments_sph(t.d, t.md[:-1], t.tree)
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(cnt == -7)
    # accepted: zero points (null outputs too), -0 as theta and eps, one output at a time
    assert _raw(gh, t, pts, out, cnt, n_points=0) == gh.GRACE_OK
    assert _raw(gh, t, pts, None, None, n_points=0) == gh.GRACE_OK
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(cnt == -7)
    assert _raw(gh, t, pts, out, None, theta=-0.0, eps=-0.0) == gh.GRACE_OK
    assert _raw(gh, t, pts, None, cnt) == gh.GRACE_OK
    gh.trace_status()
    torch.cuda.synchronize()
    assert torch.all(cnt[:, 1] > 0) and torch.all(out[:, 3] < 0)
    e_out, e_cnt = gh.gravity_sph(torch.empty((0, 3), dtype=torch.float32, device=cuda), t.d, t.md, t.tree, t.mom,
                                  counts=True)
    assert tuple(e_out.shape) == (0, 4) and tuple(e_cnt.shape) == (0, 2)


@pytest.mark.gpu
def test_gravity_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    t = _setup(gh, G.clustered_scene(9000, 41), 32, cuda)
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.random((400, 4), dtype=F32), t.sh[:377]]).astype(F32)
    for name, a in (("s", t.sh), ("p", pts), ("m", t.m)):
        a.tofile(str(tmp_path / (name + ".f32")))
    exe = str(tmp_path / "dropin_gravity")
    _compile_dropin(exe)
    f = lambda x: str(tmp_path / (x + ".f32"))
    res = subprocess.run([exe, f("s"), f("p"), f("m"), "0.5", "0.01"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    names = ("moments", "out_only", "out", "counts")
    got = {w[0]: (int(w[1]), int(w[2])) for w in (ln.split() for ln in res.stdout.splitlines())
           if len(w) == 3 and w[0] in names}
    out, cnt = _check_walk(gh, t, pts, 0.5, 0.01, cuda, "ctypes")
    exp = {"moments": t.rec, "out_only": out, "out": out, "counts": cnt}
    assert set(got) == set(exp)
    for name, a in exp.items():
        assert got[name] == digest(a), name
    assert np.array_equal(t.rec, t.ref_rec) and cnt[:, 0].max() > 1
