"""Gravity within groups (grace_gravity_group_moments_f4 / grace_gravity_group_points_f4,
gravity_group_moments_sph / gravity_groups_sph, an extension the reference lacks) against the NumPy restatement
of the contract in include/grace_hip.h (gravity_group_cases.py), which is fed the tree read back from the
device.  Everything is compared on bit patterns -- moment records as uint32, outputs as uint64, counts and label
ranges with array_equal: no tolerance anywhere.  The scenes, the labellings and the preconditions they are
chosen for are checked without a GPU in test_gravity_group_cases.py."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import gravity_cases as G
import gravity_group_cases as GG
from test_range_queries import digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32 = np.float32


# ---- CPU ------------------------------------------------------------------------------------------
def test_gravity_group_symbols_exported():
    import grace_hip
    lib = grace_hip.exported_symbols()
    assert hasattr(lib, "grace_gravity_group_moments_f4") and hasattr(lib, "grace_gravity_group_points_f4")
    assert callable(grace_hip.gravity_group_moments_sph) and callable(grace_hip.gravity_groups_sph)


def _compile_dropin(exe):
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_gravity_groups.hip"),
                           "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


def test_gravity_groups_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_gravity_groups"
    _compile_dropin(exe)
    assert exe.exists()


@pytest.mark.parametrize("call", ["grace::gravity_group_moments_sph(s, m, l, t, mom, rng);",
                                  "grace::gravity_groups_sph(p, pl, s, m, l, t, mom, rng, 0.5f, 0.0f, out);",
                                  "grace::gravity_groups_sph(p, pl, s, m, l, t, mom, rng, 0.5f, 0.0f, out, cnt);"])
def test_gravity_groups_double4_is_a_clear_compile_error(tmp_path, call):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/gravity_sph.cuh"\n'
                   "void f(const thrust::device_vector<float4>& p, const thrust::device_vector<int>& pl,\n"
                   "       const thrust::device_vector<double4>& s, const thrust::device_vector<float>& m,\n"
                   "       const thrust::device_vector<int>& l, const grace::Tree& t,\n"
                   "       thrust::device_vector<float>& mom, thrust::device_vector<int>& rng,\n"
                   "       thrust::device_vector<double>& out, thrust::device_vector<int>& cnt)\n"
                   "{ " + call + " }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "float4 spheres only" in res.stderr


def test_gravity_groups_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& p, const grace::device_vector<int>& pl,\n"
                   "       const grace::device_vector<grace::float4>& s, const grace::device_vector<float>& m,\n"
                   "       const grace::device_vector<int>& l, const grace::Tree& t)\n"
                   "{\n"
                   "    grace::device_vector<float> moments;\n"
                   "    grace::device_vector<int> ranges;\n"
                   "    grace::device_vector<double> out;\n"
                   "    grace::device_vector<int> counts;\n"
                   "    grace::gravity_group_moments_sph(s, m, l, t, moments, ranges);\n"
                   "    grace::gravity_groups_sph(p, pl, s, m, l, t, moments, ranges, 0.5f, 0.0f, out);\n"
                   "    grace::gravity_groups_sph(p, pl, s, m, l, t, moments, ranges, 0.5f, 0.01f, out, counts);\n"
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


def _setup(gh, s, mpl, cuda, labelling, masses=None):
    """A scene on the device and read back: spheres in tree order, the tree, masses, and under the labelling
    (a function of the spheres in tree order) the labels, the moment records and the label ranges."""
    import torch
    d = _dev(np.ascontiguousarray(s, F32), cuda)
    tree = gh.Tree(len(s), mpl, device=cuda)
    if len(s) > mpl:
        gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))        # sorts d
    else:                                                              # one sphere: a one-leaf tree without nodes
        tree.leaves[0] = torch.tensor([0, len(s), 0, 0], dtype=torch.int32)
        tree.root_index.zero_()
    t = types.SimpleNamespace(d=d, tree=tree, sh=d.cpu().numpy(), nodes=tree.nodes.cpu().numpy(),
                              leaves=tree.leaves.cpu().numpy(), root=int(tree.root_index.item()))
    t.m = np.ascontiguousarray(G.masses_for(len(s)) if masses is None else masses, F32)
    t.md = _dev(t.m, cuda)
    _set_labels(gh, t, labelling(t.sh), cuda)
    return t


def _set_labels(gh, t, labels, cuda):
    import torch
    t.lab = np.ascontiguousarray(labels, np.int32)
    t.ld = _dev(t.lab, cuda)
    t.mom, t.rng = gh.gravity_group_moments_sph(t.d, t.md, t.ld, t.tree)
    assert tuple(t.mom.shape) == (t.tree.n_nodes, 12) and tuple(t.rng.shape) == (t.tree.n_nodes, 2)
    assert t.mom.dtype == torch.float32 and t.rng.dtype == torch.int32
    t.rec = t.mom.cpu().numpy().view(np.uint32)
    t.ranges = t.rng.cpu().numpy()
    t.ref_rec, t.ref_ranges = GG.group_moments(t.nodes, t.leaves, t.root, t.sh, t.m, t.lab)


def _moments_match(t):
    bad = np.argwhere(t.rec != t.ref_rec)
    assert t.rec.shape == t.ref_rec.shape and len(bad) == 0, (len(bad), bad[:5], t.rec[bad[:5, 0]], t.ref_rec[bad[:5, 0]])
    bad = np.argwhere(t.ranges != t.ref_ranges)
    assert t.ranges.shape == t.ref_ranges.shape and len(bad) == 0, (bad[:5], t.ranges[bad[:5, 0]], t.ref_ranges[bad[:5, 0]])


def _run(gh, t, pts, pl, theta, eps, cuda, want_counts=True):
    import torch
    out, cnt = gh.gravity_groups_sph(_dev(np.asarray(pts, F32), cuda), _dev(np.asarray(pl, np.int32), cuda), t.d, t.md,
                                     t.ld, t.tree, t.mom, t.rng, theta=theta, eps=eps,
                                     counts=True if want_counts else None, check=True)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(pts), 4)
    return out.cpu().numpy(), None if cnt is None else cnt.cpu().numpy()


def _restate(t, pts, pl, theta, eps):
    return GG.group_walk(t.nodes, t.leaves, t.root, t.sh, t.m, t.lab, t.ref_rec, t.ref_ranges, np.asarray(pts, F32),
                         pl, theta, eps)


def _check(got, ref, what):
    (out, cnt), (ref_out, ref_cnt) = got, ref
    bad = np.argwhere(cnt != ref_cnt)
    assert cnt.dtype == np.int32 and len(bad) == 0, (what, bad[:5], cnt[bad[:5, 0]], ref_cnt[bad[:5, 0]])
    bad = np.argwhere(out.view(np.uint64) != ref_out.view(np.uint64))
    assert out.dtype == np.float64 and len(bad) == 0, (what, bad[:5], out[bad[:5, 0]], ref_out[bad[:5, 0]])


def _check_walk(gh, t, pts, pl, theta, eps, cuda, what):
    got = _run(gh, t, pts, pl, theta, eps, cuda)
    _check(got, _restate(t, pts, pl, theta, eps), what)
    return got


@pytest.fixture(scope="module")
def built(gh, cuda):
    """get(scene, labelling, mpl): the scene on the device under the labelling, built on first use."""
    made = {}

    def get(scene, labelling, mpl):
        if (scene, labelling, mpl) not in made:
            made[scene, labelling, mpl] = _setup(gh, G.SCENES[scene](), mpl, cuda, GG.LABELLINGS[labelling])
        return made[scene, labelling, mpl]
    return get


_direct = {}


def _direct_sum(scene, labelling, t, pts, pl, eps):
    """The tree-free masked direct sum (the tree order is the same for every max_per_leaf), once."""
    key = (scene, labelling, eps)
    if key not in _direct:
        _direct[key] = (t.sh.copy(), GG.masked_direct_sum(pts, pl, t.sh, t.m, t.lab, eps))
    sh, ref = _direct[key]
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
@pytest.mark.parametrize("labelling", list(GG.LABELLINGS))
@pytest.mark.parametrize("scene", list(G.SCENES))
def test_group_moments_and_label_ranges_are_the_restatement_bit_for_bit(built, scene, labelling, mpl):
    t = built(scene, labelling, mpl)
    assert len(t.rec) == len(t.leaves) - 1
    _moments_match(t)
    _, _, _, _, s0, s1 = G.record_fields(t.rec)
    assert s0.min() == 0 and s1.max() == len(t.sh)                     # the spans cover every primitive


WALKS = [("clustered", "blobs", 1), ("clustered", "lonely", 8), ("clustered", "scatter", 32),
         ("random", "slabs", 1), ("random", "scatter", 8), ("random", "slabs", 32),
         ("lattice", "scatter", 1), ("lattice", "slabs", 8), ("lattice", "single", 32),
         ("random", "blobs", 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("scene,labelling,mpl", WALKS)
def test_group_walk_is_the_restatement_bit_for_bit(gh, built, scene, labelling, mpl, cuda):
    t = built(scene, labelling, mpl)
    pts = G.query_points(t.sh)
    pl = GG.point_labels(labelling, pts)
    off = ~np.all(np.isfinite(pts), axis=1) | (pl < 0)
    for eps in G.SOFTENINGS:
        for theta in G.THETAS:
            out, cnt = got = _run(gh, t, pts, pl, theta, eps, cuda)
            if theta == 0.0:                                   # the direct sum over the label's members
                _check(got, _direct_sum(scene, labelling, t, pts, pl, eps), (scene, labelling, mpl, eps, "direct"))
                assert np.all(cnt[:, 0] == 0)
            else:
                _check(got, _restate(t, pts, pl, theta, eps), (scene, labelling, mpl, theta, eps))
            assert off.sum() >= 4 and np.all(out[off].view(np.uint64) == 0) and np.all(cnt[off] == 0)
            assert np.all(np.isfinite(out))
    out_only, none = _run(gh, t, pts, pl, 0.7, 0.01, cuda, want_counts=False)    # the outputs alone
    assert none is None
    assert np.array_equal(out_only.view(np.uint64), _run(gh, t, pts, pl, 0.7, 0.01, cuda)[0].view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("mpl", G.LEAF_SIZES)
def test_one_label_everywhere_is_gravity_sph_bit_for_bit(gh, mpl, cuda):
    t = _setup(gh, G.clustered_scene(), mpl, cuda, GG.single)         # (its labels are changed below)
    mom = gh.gravity_moments_sph(t.d, t.md, t.tree)
    assert np.array_equal(mom.cpu().numpy().view(np.uint32), t.rec) and np.all(t.ranges == 0)
    pts = G.query_points(t.sh)
    dp = _dev(pts, cuda)
    for value in (0, 5):
        _set_labels(gh, t, np.full(len(t.sh), value, np.int32), cuda)
        assert np.array_equal(mom.cpu().numpy().view(np.uint32), t.rec) and np.all(t.ranges == value)
        for theta, eps in ((0.0, 0.0), (0.5, 0.01), (0.7, 0.0), (1000.0, 0.0)):
            ref_out, ref_cnt = gh.gravity_sph(dp, t.d, t.md, t.tree, mom, theta=theta, eps=eps, counts=True, check=True)
            got = _run(gh, t, pts, np.full(len(pts), value, np.int32), theta, eps, cuda)
            _check(got, (ref_out.cpu().numpy(), ref_cnt.cpu().numpy()), (mpl, value, theta, eps))


@pytest.mark.gpu
def test_theta_zero_does_not_depend_on_the_tree(gh, built, cuda):
    runs = []
    for mpl in G.LEAF_SIZES:
        t = built("clustered", "lonely", mpl)
        pts = G.query_points(t.sh, seed=13, n_random=200, n_centres=100)
        pl = GG.point_labels("lonely", pts)
        runs.append((t, _run(gh, t, pts, pl, 0.0, 0.01, cuda)))
    t0, (out0, cnt0) = runs[0]
    _check((out0, cnt0), GG.masked_direct_sum(pts, pl, t0.sh, t0.m, t0.lab, 0.01), "direct")
    for t, (out, cnt) in runs[1:]:
        assert np.array_equal(t.sh, t0.sh) and np.array_equal(t.lab, t0.lab)   # the same tree order, another tree
        assert not np.array_equal(t.leaves, t0.leaves)
        assert np.array_equal(out.view(np.uint64), out0.view(np.uint64)) and np.array_equal(cnt, cnt0)


@pytest.mark.gpu
@pytest.mark.parametrize("scene,labelling,mpl", [("clustered", "blobs", 8), ("random", "slabs", 8),
                                                 ("clustered", "lonely", 1)])
def test_mixed_labels_and_decisions_in_one_packet(gh, built, scene, labelling, mpl, cuda):
    t = built(scene, labelling, mpl)
    pts, pl, node = GG.mixed_label_packet(t.ref_rec, t.ref_ranges)
    assert len(pts) == 64 and len(np.unique(pl)) == 3 and t.ref_ranges[node, 0] == t.ref_ranges[node, 1]
    out, cnt = _check_walk(gh, t, pts, pl, 0.7, 0.0, cuda, (scene, labelling))
    mine = pl == t.ref_ranges[node, 0]
    assert len(np.unique(cnt[mine], axis=0)) > 1
    _check_walk(gh, t, pts, pl, 0.7, 0.01, cuda, (scene, labelling, "softened"))
    _check_walk(gh, t, pts[::-1], pl, 0.7, 0.0, cuda, (scene, labelling, "labels the other way round"))


@pytest.mark.gpu
def test_packet_sizes_with_per_point_labels(gh, built, cuda):
    t = built("random", "slabs", 8)
    pts = G.packet_points()                                          # 63, 64 and 65 points in cells of their own
    rng = np.random.default_rng(7)
    _check_walk(gh, t, pts, GG.point_labels("slabs", pts), 0.5, 0.0, cuda, "cells, labels by position")
    _check_walk(gh, t, pts, rng.integers(-1, 9, len(pts)).astype(np.int32), 0.5, 0.0, cuda, "cells, any label")
    for n in (1, 63, 64, 65):                                        # around one packet
        p = np.concatenate([t.sh[:n // 2, :3], rng.random((n - n // 2, 3), dtype=F32)])
        _check_walk(gh, t, p, rng.integers(-1, 9, n).astype(np.int32), 0.5, 0.01, cuda, n)
        _check_walk(gh, t, p, GG.point_labels("slabs", p), 0.7, 0.0, cuda, (n, "by position"))


@pytest.mark.gpu
def test_leaf_ranges_with_two_labels_across_cluster_boundaries(gh, cuda):
    t = _setup(gh, G.random_scene(200, 4), 32, cuda, GG.scatter)
    first, end = t.leaves[:, 0], t.leaves[:, 0] + t.leaves[:, 1]
    assert np.sum((first >> 6) != ((end - 1) >> 6)) >= 1
    _moments_match(t)
    pts = G.query_points(t.sh, n_random=120, n_centres=200)
    for theta in G.THETAS:
        _check_walk(gh, t, pts, GG.point_labels("scatter", pts), theta, 0.0, cuda, theta)


@pytest.mark.gpu
def test_coincident_spine_with_two_labels_interleaved(gh, cuda):
    """300 coincident centres under max_per_leaf = 1, labelled 0 and 1 in turn by the bits of h: merged ranges
    longer than a cluster in which every lane takes the records of its own label only (check=True raises on a
    stack overflow)."""
    t = _setup(gh, G.spine_scene(), 1, cuda, GG.spine_labels)
    assert len(t.leaves) == 350
    _moments_match(t)
    assert G.max_stack_entries(t.nodes, t.leaves, t.root) < 128
    at = np.all(t.sh[:, :3] == G.SPINE_AT, axis=1)
    assert at.sum() == 300 and 100 < t.lab[at].sum() < 200
    rng = np.random.default_rng(3)
    near = G.SPINE_AT + (rng.random((40, 3), dtype=F32) - F32(0.5)) * F32(1e-3)
    pts = np.concatenate([np.tile(G.SPINE_AT, (70, 1)), near, t.sh[300:, :3], rng.random((60, 3), dtype=F32),
                          np.array([[40.0, 0.5, 0.5]], F32)]).astype(F32)
    pl = (np.arange(len(pts)) % 3 - (np.arange(len(pts)) % 7 == 0)).astype(np.int32)     # -1, 0, 1, 2
    for theta in G.THETAS:
        for eps in G.SOFTENINGS:
            _check_walk(gh, t, pts, pl, theta, eps, cuda, (theta, eps))
    _, cnt0 = _run(gh, t, pts[:3], np.array([0, 1, 2], np.int32), 0.0, 0.01, cuda)
    assert cnt0.tolist() == [[0, int(np.sum(t.lab == 0))], [0, int(np.sum(t.lab == 1))], [0, 0]]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny_trees(gh, n, cuda):
    s = np.array([[0.25, 0.5, 0.75, 0.01], [0.75, 0.25, 0.5, 0.01], [0.5, 0.75, 0.25, 0.01]], F32)[:n]
    for labels in ([3, 3, 3], [3, 4, 3], [4, -1, 3], [-1, -1, -1]):
        t = _setup(gh, s, 1, cuda, lambda sh: np.array(labels[:len(sh)], np.int32),
                   masses=np.array([1.5, 0.25, 3.0], F32)[:n])
        assert t.tree.n_nodes == n - 1 and len(t.rec) == n - 1
        _moments_match(t)
        pts = np.concatenate([t.sh[:, :3], np.array([[0.5, 0.5, 0.5], [9.0, 9.0, 9.0], [9.0, 9.0, 9.0],
                                                     [0.0, np.nan, 0.0]], F32)])
        pl = np.array(labels[:n] + [3, 3, 4, 3], np.int32)
        for theta in G.THETAS:
            for eps in G.SOFTENINGS:
                got = _check_walk(gh, t, pts, pl, theta, eps, cuda, (n, labels, theta, eps))
                if theta == 0.0:
                    _check(got, GG.masked_direct_sum(pts, pl, t.sh, t.m, t.lab, eps), (n, labels, eps, "direct"))
    if n == 1:                                                       # no nodes: null moments and ranges are accepted
        scene = gh._interp_scene(t.d, t.tree)
        assert t.mom.numel() == 0 and t.rng.numel() == 0
        assert gh._lib.grace_gravity_group_moments_f4(*scene, gh._ptr(t.md), gh._ptr(t.ld), C.c_void_p(0),
                                                      C.c_void_p(0), gh._stream()) == gh.GRACE_OK


@pytest.mark.gpu
def test_negative_and_absent_point_labels_and_non_finite_points(gh, built, cuda):
    t = built("clustered", "lonely", 8)
    pts = G.query_points(t.sh)
    pl = GG.point_labels("lonely", pts)
    pl[2::50] = -1
    pl[3::50] = -(2 ** 31)
    pl[4::50] = 2 ** 31 - 1                                           # absent, at the end of the int range
    finite = np.all(np.isfinite(pts), axis=1)
    assert np.sum(t.lab == GG.LONELY) == 1 and np.sum(t.lab == GG.ABSENT) == 0 and np.sum(~finite) == 4
    pl[np.nonzero(~finite)[0][:2]] = 0                                # off points with a label that exists
    for theta in (0.0, 0.7):
        out, cnt = _check_walk(gh, t, pts, pl, theta, 0.0, cuda, theta)
        off = ~finite | (pl < 0)
        assert off.sum() >= 40 and np.all(out[off].view(np.uint64) == 0) and np.all(cnt[off] == 0)   # +0 throughout
        absent = finite & ((pl == GG.ABSENT) | (pl == 2 ** 31 - 1))
        assert absent.sum() > 30 and np.all(cnt[absent] == 0)
        assert np.all(out[absent].view(np.uint64) == np.array([0, 0, 0, 1 << 63], np.uint64))        # phi = -0
        lonely = finite & (pl == GG.LONELY)
        # one term: the particle itself, or the monopole of a node that holds it and unlabelled ones only
        assert lonely.sum() > 15 and np.all(cnt[lonely].sum(axis=1) == 1) and np.all(out[lonely, 3] < 0)
        assert theta > 0 or np.all(cnt[lonely] == (0, 1))


@pytest.mark.gpu
def test_an_unbinding_pass(gh, cuda):
    """A third of one blob leaves: its labels become -1, the moments are computed again, and the walk is still
    the restatement -- over fewer members; the particles that left, used as points, get +0."""
    t = _setup(gh, G.clustered_scene(), 8, cuda, GG.blobs)
    pts = np.ascontiguousarray(t.sh[:, :3])                            # every particle, with its own label
    before = _check_walk(gh, t, pts, t.lab, 0.7, 0.01, cuda, "before")
    members = np.nonzero(t.lab == 1)[0]
    leaving = members[::3]
    lab = t.lab.copy()
    lab[leaving] = -1
    old_rec = t.rec.copy()
    _set_labels(gh, t, lab, cuda)
    _moments_match(t)
    assert len(leaving) > 150 and not np.array_equal(t.rec, old_rec)
    out, cnt = _check_walk(gh, t, pts, t.lab, 0.7, 0.01, cuda, "after")
    assert np.all(out[leaving].view(np.uint64) == 0) and np.all(cnt[leaving] == 0)
    stay = np.setdiff1d(members, leaving)
    assert np.all(out[stay, 3] > before[0][stay, 3])                   # less bound than before
    _, cnt0 = _run(gh, t, pts[stay[:5]], np.ones(5, np.int32), 0.0, 0.0, cuda)
    assert np.all(cnt0 == (0, len(stay)))
    # asking with the old labels: the leavers feel the remaining members, but attract nobody
    old = np.ones(len(leaving), np.int32)
    _check_walk(gh, t, pts[leaving], old, 0.7, 0.01, cuda, "leavers as tracers")


@pytest.mark.gpu
def test_group_moments_at_scale_across_workgroups(gh, cuda):
    """2 10^5 clustered particles, one per leaf, under the blobs: hundreds of workgroups on every XCD hand their
    fp64 partial sums and label ranges up the tree to each other."""
    t = _setup(gh, G.clustered_scene(200000, 5), 1, cuda, GG.blobs)
    assert len(t.leaves) > 150000 and np.sum(t.lab < 0) > 10000 and np.sum(t.ref_ranges[:, 1] < 0) > 1000
    _moments_match(t)
    mom, rng = gh.gravity_group_moments_sph(t.d, t.md, t.ld, t.tree)
    assert np.array_equal(mom.cpu().numpy().view(np.uint32), t.rec) and np.array_equal(rng.cpu().numpy(), t.ranges)
    pts = np.concatenate([t.sh[::40000, :3], np.array([[0.5, 0.5, 0.5], [3.0, 0.5, 0.5]], F32)])
    _check_walk(gh, t, pts, GG.point_labels("blobs", pts), 0.5, 0.0, cuda, "walk")


@pytest.mark.gpu
def test_results_do_not_depend_on_order_layout_knobs_or_stream(gh, cuda, knobs_reset):
    import torch
    t = _setup(gh, G.clustered_scene(), 8, cuda, GG.lonely)           # (its labels are changed at the end)
    pts = G.query_points(t.sh)
    pl = GG.point_labels("lonely", pts)
    out0, cnt0 = _check_walk(gh, t, pts, pl, 0.5, 0.01, cuda, "base")

    def same(got, order=None):
        out, cnt = got
        ref_out, ref_cnt = (out0, cnt0) if order is None else (out0[order], cnt0[order])
        return np.array_equal(out.view(np.uint64), ref_out.view(np.uint64)) and np.array_equal(cnt, ref_cnt)

    order = np.random.default_rng(2).permutation(len(pts))           # shuffled point order
    assert same(_run(gh, t, pts[order], pl[order], 0.5, 0.01, cuda), order)
    order = np.argsort(pl, kind="stable")                            # ... and sorted by label
    assert same(_run(gh, t, pts[order], pl[order], 0.5, 0.01, cuda), order)
    for elems in (3, 7):                                             # elems_per_point
        wide = np.full((len(pts), elems), 9.0, F32); wide[:, :3] = pts
        assert same(_run(gh, t, wide, pl, 0.5, 0.01, cuda)), elems
    gh.set_sph_kernel("wendland_c4")                                 # no SPH kernel in it
    assert same(_run(gh, t, pts, pl, 0.5, 0.01, cuda))
    gh.set_sph_kernel("cubic")
    gh.set_cache_auto(False)                                         # nor the trace's caches
    gh.set_cache_validation(False)
    assert same(_run(gh, t, pts, pl, 0.5, 0.01, cuda))
    gh.set_cache_auto(True)
    gh.set_cache_validation(True)
    stream = torch.cuda.Stream(device=cuda)                          # a stream of the caller's
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        mom, rng = gh.gravity_group_moments_sph(t.d, t.md, t.ld, t.tree)
        got = _run(gh, t, pts, pl, 0.5, 0.01, cuda)
    stream.synchronize()
    assert np.array_equal(mom.cpu().numpy().view(np.uint32), t.rec) and np.array_equal(rng.cpu().numpy(), t.ranges)
    assert same(got)
    assert same(_run(gh, t, pts, pl, 0.5, 0.01, cuda))                # run to run
    # label values matter only through equality and order: a monotone relabelling of spheres and points alike
    relabel = lambda a: np.where(a >= 0, 3 * a + 11, a - 5).astype(np.int32)
    lab = t.lab.copy()
    _set_labels(gh, t, relabel(lab), cuda)
    assert np.array_equal(t.rec, GG.group_moments(t.nodes, t.leaves, t.root, t.sh, t.m, lab)[0])
    assert same(_run(gh, t, pts, relabel(pl), 0.5, 0.01, cuda))


def _raw(gh, t, pts, pl, out, cnt, theta=0.5, eps=0.0, scene=None, masses="own", labels="own", moments="own",
         ranges="own", n_points=None, elems=None):
    scene = gh._interp_scene(t.d, t.tree) if scene is None else scene
    own = lambda given, mine: mine if isinstance(given, str) else given
    return gh._lib.grace_gravity_group_points_f4(
        gh._ptr(pts), C.c_size_t(len(pts) if n_points is None else n_points),
        C.c_int(pts.shape[1] if elems is None else elems), *scene, gh._ptr(own(masses, t.md)),
        gh._ptr(own(labels, t.ld)), gh._ptr(own(moments, t.mom)), gh._ptr(own(ranges, t.rng)), gh._ptr(pl),
        C.c_float(theta), C.c_float(eps), gh._ptr(out), gh._ptr(cnt), gh._stream())


@pytest.mark.gpu
def test_bad_arguments_write_nothing(gh, built, cuda):
    import torch
    t = built("random", "slabs", 8)
    pts = torch.rand((100, 4), dtype=torch.float32, device=cuda)
    pl = torch.randint(0, 8, (100,), dtype=torch.int32, device=cuda)
    out = torch.full((100, 4), -7.0, dtype=torch.float64, device=cuda)
    cnt = torch.full((100, 2), -7, dtype=torch.int32, device=cuda)
    mom = torch.full((t.tree.n_nodes, 12), -7.0, dtype=torch.float32, device=cuda)
    rng = torch.full((t.tree.n_nodes, 2), -7, dtype=torch.int32, device=cuda)
    scene = gh._interp_scene(t.d, t.tree)
    empty = list(scene); empty[1] = C.c_size_t(0)
    no_leaves = list(scene); no_leaves[4] = C.c_void_p(0)
    no_root = list(scene); no_root[5] = C.c_void_p(0)
    no_nodes = list(scene); no_nodes[2] = C.c_void_p(0)
    nan, inf = float("nan"), float("inf")
    cases = (dict(theta=-0.5), dict(theta=nan), dict(theta=inf), dict(eps=-0.01), dict(eps=nan), dict(eps=inf),
             dict(elems=2), dict(elems=17), dict(masses=None), dict(labels=None), dict(moments=None), dict(ranges=None),
             dict(scene=empty), dict(scene=no_leaves), dict(scene=no_root), dict(scene=no_nodes))
    for kw in cases:
        assert _raw(gh, t, pts, pl, out, cnt, **kw) == gh.GRACE_INVALID_ARGUMENT, kw
    assert _raw(gh, t, pts, None, out, cnt) == gh.GRACE_INVALID_ARGUMENT             # null point labels
    assert _raw(gh, t, pts, pl, None, None) == gh.GRACE_INVALID_ARGUMENT             # no output
    moments_f4 = gh._lib.grace_gravity_group_moments_f4
    for sc, md, ld in ((empty, t.md, t.ld), (no_leaves, t.md, t.ld), (no_root, t.md, t.ld), (no_nodes, t.md, t.ld),
                       (scene, None, t.ld), (scene, t.md, None)):
        assert moments_f4(*sc, gh._ptr(md), gh._ptr(ld), gh._ptr(mom), gh._ptr(rng), gh._stream()) \
            == gh.GRACE_INVALID_ARGUMENT
    for m_, r_ in ((None, rng), (mom, None)):                                        # null moments, null label ranges
        assert moments_f4(*scene, gh._ptr(t.md), gh._ptr(t.ld), gh._ptr(m_), gh._ptr(r_), gh._stream()) \
            == gh.GRACE_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(cnt == -7) and torch.all(mom == -7.0) and torch.all(rng == -7)
    args = (pts, pl, t.d, t.md, t.ld, t.tree, t.mom, t.rng)
    for kw in (dict(theta=-1.0), dict(eps=-1.0), dict(theta=nan), dict(eps=inf)):
        with pytest.raises(ValueError):
            gh.gravity_groups_sph(*args, **kw)
    bad = {0: pts[:, :2], 1: pl[:-1], 3: t.md[:-1], 4: t.ld[:-1], 6: t.mom[:-1], 7: t.rng[:-1]}
    bad_dtype = {1: pl.long(), 4: t.ld.long(), 7: t.rng.float()}
    for swaps in (bad, bad_dtype):
        for k, v in swaps.items():
            with pytest.raises(ValueError):
                gh.gravity_groups_sph(*(args[:k] + (v,) + args[k + 1:]))
    with pytest.raises(ValueError):
        gh.gravity_group_moments_sph(t.d, t.md[:-1], t.ld, t.tree)
    with pytest.raises(ValueError):
        gh.gravity_group_moments_sph(t.d, t.md, t.ld[:-1], t.tree)
    with pytest.raises(ValueError):
        gh.gravity_group_moments_sph(t.d, t.md, t.ld.long(), t.tree)
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(cnt == -7)
    # accepted: zero points (null outputs and point labels too), -0 as theta and eps, one output at a time
    assert _raw(gh, t, pts, pl, out, cnt, n_points=0) == gh.GRACE_OK
    assert _raw(gh, t, pts, None, None, None, n_points=0) == gh.GRACE_OK
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(cnt == -7)
    assert _raw(gh, t, pts, pl, out, None, theta=-0.0, eps=-0.0) == gh.GRACE_OK
    assert _raw(gh, t, pts, pl, None, cnt) == gh.GRACE_OK
    gh.trace_status()
    torch.cuda.synchronize()
    assert torch.all(cnt[:, 1] > 0) and torch.all(out[:, 3] < 0)
    e_out, e_cnt = gh.gravity_groups_sph(torch.empty((0, 3), dtype=torch.float32, device=cuda),
                                         torch.empty((0,), dtype=torch.int32, device=cuda), *args[2:], counts=True)
    assert tuple(e_out.shape) == (0, 4) and tuple(e_cnt.shape) == (0, 2)


@pytest.mark.gpu
def test_gravity_groups_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    t = _setup(gh, G.clustered_scene(9000, 41), 32, cuda, GG.lonely)
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.random((400, 4), dtype=F32), t.sh[:377]]).astype(F32)
    pl = GG.point_labels("lonely", pts)
    for name, a in (("s", t.sh), ("p", pts), ("m", t.m), ("l", t.lab), ("pl", pl)):
        a.tofile(str(tmp_path / (name + ".bin")))
    exe = str(tmp_path / "dropin_gravity_groups")
    _compile_dropin(exe)
    f = lambda x: str(tmp_path / (x + ".bin"))
    res = subprocess.run([exe, f("s"), f("p"), f("m"), f("l"), f("pl"), "0.5", "0.01"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    names = ("moments", "label_ranges", "out_only", "out", "counts")
    got = {w[0]: (int(w[1]), int(w[2])) for w in (ln.split() for ln in res.stdout.splitlines())
           if len(w) == 3 and w[0] in names}
    out, cnt = _check_walk(gh, t, pts, pl, 0.5, 0.01, cuda, "ctypes")
    exp = {"moments": t.rec, "label_ranges": t.ranges, "out_only": out, "out": out, "counts": cnt}
    assert set(got) == set(exp)
    for name, a in exp.items():
        assert got[name] == digest(a), name
    _moments_match(t)
    assert cnt[:, 0].max() > 1 and pl.dtype == np.int32 and t.lab.dtype == np.int32
