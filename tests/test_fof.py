"""Friends-of-friends groups (grace_fof_labels_f4 / grace_fof_groups / grace_fof_members, an extension
the reference lacks) against a NumPy restatement of the contract in include/grace_hip.h.

Link: spheres i and j, in tree order, are linked iff d2(i, j) <= B2, B2 = fl(b * b), d2 the range
queries' fp32 sequence fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)) -- inclusive; w is ignored; b = 0
links coincident centres; a sphere with a non-finite coordinate links to nothing.  Groups are the
connected components; labels[i] is the smallest tree index in i's group.  Kept groups (at least
min_members members) are numbered in ascending label: group_of[i] (or -1), sizes[g], and the CSR
lists offsets / members, each row in ascending tree index.  Every comparison is array_equal on int32.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_neighbours import SCENES, _build, _clustered_scene, _lattice_scene, _random_scene, d2_rows
from test_range_queries import digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32 = np.float32
N_SCENE = 20000
# linking lengths per scene: sub-percolating, near-percolating and percolated (random); inside the
# cores only up to most of a cluster (clustered); coincident centres only, and a little more; the
# lattice's exact tie d2 == B2 == 2^-8 from both sides
LINKING = {"random": [F32(f) * F32(N_SCENE ** (-1.0 / 3.0)) for f in (0.5, 0.8, 1.0, 1.3)],
           "clustered": [F32(2e-4), F32(1e-3), F32(5e-3)],
           "coincident": [F32(0.0), F32(1e-2)],
           "lattice": [F32(1.0 / 16.0), np.nextafter(F32(1.0 / 16.0), F32(0.0))]}
MIN_MEMBERS = (1, 2, 20)


# ---- the restatement ----------------------------------------------------------------------------
def unite(parent, i, j):
    """A plain union-find over the edges (i[k], j[k]), every hook towards the smaller root."""
    while len(i):
        while True:                                                # full compression
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent[:] = up
        ri, rj = parent[i], parent[j]
        open_ = ri != rj
        if not open_.any():
            return
        i, j, ri, rj = i[open_], j[open_], ri[open_], rj[open_]
        np.minimum.at(parent, np.maximum(ri, rj), np.minimum(ri, rj))   # roots only: parent[hi] was hi


def restate_labels(x, bs):
    """labels [len(bs), n] int32 of centres x [n, 3] (fp32) for each linking length of bs."""
    x = np.ascontiguousarray(x[:, :3], F32)
    n = len(x)
    parents = [np.arange(n, dtype=np.int64) for _ in bs]
    B2 = [F32(b) * F32(b) for b in bs]
    rows = max(1, min(1024, (1 << 24) // max(n, 1)))
    for a in range(0, n, rows):
        e = min(a + rows, n)
        d2 = d2_rows(x[a:e], x[:e])                                # j < e; (i, j) and (j, i) are one link
        for parent, b2 in zip(parents, B2):
            i, j = np.nonzero(d2 <= b2)                            # (NaN: never)
            unite(parent, i + a, j)
    out = []
    for parent in parents:
        unite(parent, np.zeros(1, np.int64), np.zeros(1, np.int64))    # compress
        out.append(parent.astype(np.int32))
    return np.array(out)


def restate_catalogue(labels, min_members):
    """(group_of, sizes, offsets, members) of the labels, restated with np.unique."""
    uniq, inverse, counts = np.unique(labels, return_inverse=True, return_counts=True)   # ascending label
    keep = counts >= min_members
    number = np.cumsum(keep) - 1
    group_of = np.where(keep[inverse], number[inverse], -1).astype(np.int32)
    sizes = counts[keep].astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    kept = np.nonzero(group_of >= 0)[0]
    members = kept[np.argsort(group_of[kept], kind="stable")].astype(np.int32)
    return group_of, sizes, offsets, members


def _line(keep_every=None):
    """4096 points on a line at spacing 2^-12 (exact), the other coordinates 0.5; optionally without
    every 512th."""
    k = np.arange(4096)
    if keep_every:
        k = k[k % keep_every != keep_every - 1]
    s = np.full((len(k), 4), 0.5, F32)
    s[:, 0] = (k * 2.0 ** -12).astype(F32)
    return s


# ---- CPU ------------------------------------------------------------------------------------------
def test_fof_symbols_exported():
    lib = C.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    for name in ("grace_fof_labels_f4", "grace_fof_groups", "grace_fof_members"):
        assert hasattr(lib, name), name


def _compile_dropin(exe):
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, os.path.join(ROOT, "tests", "cpp", "dropin_fof.hip"),
                           "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


def test_fof_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_fof"
    _compile_dropin(exe)
    assert exe.exists()


def test_fof_double4_is_a_clear_compile_error(tmp_path):
    src = tmp_path / "refused.hip"
    src.write_text('#include "grace/cuda/fof_sph.cuh"\n'
                   "void f(const thrust::device_vector<double4>& s, const grace::Tree& t,\n"
                   "       thrust::device_vector<int>& labels)\n"
                   "{ grace::fof_labels_sph(s, t, 0.1f, labels); }\n")
    res = subprocess.run(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, "-c", str(src), "-o", str(tmp_path / "x.o")],
                         capture_output=True, text=True)
    assert res.returncode != 0
    assert "float4 spheres only" in res.stderr


def test_fof_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& s, const grace::Tree& t)\n"
                   "{\n"
                   "    grace::device_vector<int> labels, group_of, sizes, offsets, members;\n"
                   "    grace::fof_labels_sph(s, t, 0.25f, labels);\n"
                   "    grace::fof_groups_sph(labels, 32, group_of, sizes, offsets, members);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


def test_restatement_agrees_with_scipy_connected_components():
    """A second method: scipy's connected components of the same link matrix, relabelled by minimum."""
    sparse = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    n = 3000
    x = np.random.default_rng(12).random((n, 3), dtype=F32)
    bs = [F32(f) * F32(n ** (-1.0 / 3.0)) for f in (0.5, 0.9, 1.3)]
    labels = restate_labels(x, bs)
    d2 = d2_rows(x, x)
    n_comp = []
    for b, lab in zip(bs, labels):
        i, j = np.nonzero(d2 <= b * b)
        graph = sparse.coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n)).tocsr()
        k, comp = connected_components(graph, directed=False)
        smallest = np.full(k, n, np.int64)
        np.minimum.at(smallest, comp, np.arange(n))
        assert np.array_equal(lab, smallest[comp].astype(np.int32))
        n_comp.append(k)
    assert n_comp[0] > n // 2 and n_comp[-1] < n // 20            # from mostly singletons to percolated


def test_restatement_ties_chains_and_catalogue():
    x = _lattice_scene()                                           # spacing exactly 1/16: d2 == B2 == 2^-8
    b = F32(1.0 / 16.0)
    assert b * b == F32(2.0 ** -8) and d2_rows(x[:1], x[1:2])[0, 0] == F32(2.0 ** -8)
    lab = restate_labels(x, [b, np.nextafter(b, F32(0.0))])
    assert np.all(lab[0] == 0) and np.array_equal(lab[1], np.arange(4096))
    lab = restate_labels(_line(), [F32(2.0 ** -12)])[0]
    assert np.all(lab == 0)
    lab = restate_labels(_line(512), [F32(2.0 ** -12)])[0]
    group_of, sizes, offsets, members = restate_catalogue(lab, 1)
    assert sizes.tolist() == [511] * 8 and np.array_equal(members, np.arange(8 * 511))
    # coincident centres at b = 0, a NaN coordinate, and min_members
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0, 0, 0], [2, 0, 0]], F32)
    lab = restate_labels(x, [F32(0.0), F32(1.0)])
    assert lab[0].tolist() == [0, 1, 0, 3, 1, 0, 6] and lab[1].tolist() == [0, 0, 0, 3, 0, 0, 0]
    group_of, sizes, offsets, members = restate_catalogue(lab[0], 2)
    assert group_of.tolist() == [0, 1, 0, -1, 1, 0, -1] and sizes.tolist() == [3, 2]
    assert offsets.tolist() == [0, 3, 5] and members.tolist() == [0, 2, 5, 1, 4]
    group_of, sizes, offsets, members = restate_catalogue(lab[0], 4)
    assert np.all(group_of == -1) and len(sizes) == 0 and offsets.tolist() == [0] and len(members) == 0


# ---- GPU --------------------------------------------------------------------------------------------
def _labels(gh, d, tree, b):
    return gh.fof_labels_sph(d, tree, float(b), check=True)


def _catalogue(gh, labels, min_members, cuda):
    import torch
    if not torch.is_tensor(labels):
        labels = torch.from_numpy(np.ascontiguousarray(labels, np.int32)).to(cuda)
    out = gh.fof_groups_sph(labels, min_members)
    assert all(t.dtype == torch.int32 for t in out)
    return tuple(t.cpu().numpy() for t in out)


def _check_catalogue(got, ref, what):
    for name, g, r in zip(("group_of", "sizes", "offsets", "members"), got, ref):
        assert g.shape == r.shape and np.array_equal(g, r), (what, name)


@pytest.fixture(scope="module")
def built(gh, cuda):
    res = {}
    for name, gen in SCENES.items():
        d, tree = _build(gh, gen(), cuda)
        res[name] = (d, tree, d.cpu().numpy())
    return res


_ref_cache = {}


def reference(scene, sh):
    """The restated labels of a scene (tree order) for each of its linking lengths, computed once."""
    if scene not in _ref_cache:
        _ref_cache[scene] = restate_labels(sh, LINKING[scene])
    return _ref_cache[scene]


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_labels_and_catalogue_are_the_restatement(gh, built, scene, cuda):
    d, tree, sh = built[scene]
    ref = reference(scene, sh)
    for b, ref_labels in zip(LINKING[scene], ref):
        labels = _labels(gh, d, tree, b)
        got = labels.cpu().numpy()
        bad = np.nonzero(got != ref_labels)[0]
        assert got.dtype == np.int32 and len(bad) == 0, (scene, b, bad[:5], got[bad[:5]], ref_labels[bad[:5]])
        for mm in MIN_MEMBERS:
            _check_catalogue(_catalogue(gh, labels, mm, cuda), restate_catalogue(ref_labels, mm), (scene, b, mm))
    n_groups = [len(np.unique(r)) for r in ref]
    if scene == "random":                                          # from mostly singletons to one giant group
        assert n_groups[0] > len(sh) // 2 and np.bincount(ref[-1]).max() > len(sh) // 2
    if scene == "lattice":                                         # the tie: one group labelled 0, or 4096 singletons
        assert np.all(ref[0] == 0) and np.array_equal(ref[1], np.arange(4096))
    if scene == "coincident":                                      # b = 0: exactly the two coincident sets
        assert sorted(np.bincount(ref[0])[np.bincount(ref[0]) > 1].tolist()) == [100, 200]


@pytest.mark.gpu
def test_chains_across_packets(gh, cuda):
    """One group only if hooks between waves of different workgroups all arrive."""
    rng = np.random.default_rng(6)
    b = F32(2.0 ** -12)
    for s, n_groups in ((_line(), 1), (_line(512), 8)):
        d, tree = _build(gh, s[rng.permutation(len(s))], cuda)     # the caller's order is not the line's
        sh = d.cpu().numpy()
        # tree order is still along the line: the keys do not decrease with x, and one of the 1024
        # Morton cells along x holds at most 5 of the points (the stable sort keeps the caller's order
        # inside a cell), so points 8 apart in tree order are in different cells
        assert np.all(sh[8:, 0] > sh[:-8, 0]) and not np.all(np.diff(sh[:, 0]) > 0)
        labels = _labels(gh, d, tree, b)
        ref = restate_labels(sh, [b])[0]
        assert np.array_equal(labels.cpu().numpy(), ref)
        cat = _catalogue(gh, labels, 1, cuda)
        _check_catalogue(cat, restate_catalogue(ref, 1), n_groups)
        assert len(cat[1]) == n_groups and cat[1].tolist() == [len(s) // n_groups] * n_groups


@pytest.mark.gpu
def test_everyone_links_everyone(gh, cuda):
    rng = np.random.default_rng(9)
    s = np.empty((N_SCENE, 4), F32)
    s[:, :3] = F32(0.5) + (rng.random((N_SCENE, 3), dtype=F32) - F32(0.5)) * F32(0.01)   # diameter < 0.0174
    s[:, 3] = 0.01
    d, tree = _build(gh, s, cuda)
    labels = _labels(gh, d, tree, 0.02)
    assert np.all(labels.cpu().numpy() == 0)
    group_of, sizes, offsets, members = _catalogue(gh, labels, 20, cuda)
    assert np.all(group_of == 0) and sizes.tolist() == [N_SCENE] and offsets.tolist() == [0, N_SCENE]
    assert np.array_equal(members, np.arange(N_SCENE, dtype=np.int32))


@pytest.mark.gpu
def test_coincident_spine_deeper_than_the_stack(gh, cuda):
    s = np.full((200, 4), 0.1, F32)
    s[:, :3] = np.array([0.25, 0.5, 0.75], F32)
    d, tree = _build(gh, s, cuda, 1)                               # max_per_leaf = 1: a spine of 200 leaves
    labels = _labels(gh, d, tree, 0.0)                             # check=True: trace_status() is clean
    gh.trace_status()
    assert np.all(labels.cpu().numpy() == 0)


def _caller_partition(labels, perm):
    """Tree-order labels -> per caller's particle, the smallest caller's index of its group."""
    n = len(labels)
    smallest = np.full(n, n, np.int64)
    np.minimum.at(smallest, labels, perm)
    out = np.empty(n, np.int64)
    out[perm] = smallest[labels]
    return out


@pytest.mark.gpu
def test_partition_does_not_depend_on_H_leaf_size_or_races(gh, cuda):
    import torch
    base = _clustered_scene(12000, 8)
    b = 1e-3
    parts, raw = [], []
    for H in ("zero", "scene"):
        for mpl in (1, 32, 128):
            s = base.copy()
            if H == "zero":
                s[:, 3] = 0.0
            d = torch.from_numpy(s).to(cuda)
            tree = gh.Tree(len(s), mpl, device=cuda)
            tree, perm = gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), want_perm=True)
            perm = perm.cpu().numpy().astype(np.int64)
            for _ in range(3):
                labels = _labels(gh, d, tree, b)
                cat = _catalogue(gh, labels, 2, cuda)
                parts.append(_caller_partition(labels.cpu().numpy(), perm))
                raw.append((labels.cpu().numpy(),) + cat)
            for r in raw[-2:]:                                     # the three repeats: bit-identical
                assert all(np.array_equal(x, y) for x, y in zip(r, raw[-3]))
    for p in parts[1:]:
        assert np.array_equal(p, parts[0])
    sizes = np.bincount(parts[0])
    assert sizes.max() > 1000 and np.sum(sizes == 1) > 100        # cores and field particles


@pytest.mark.gpu
def test_edges(gh, cuda):
    import torch
    # one sphere: a one-leaf tree without nodes
    one = torch.tensor([[0.25, 0.5, 0.75, 0.0]], dtype=torch.float32, device=cuda)
    t1 = gh.Tree(1, 1, device=cuda)
    t1.leaves[0] = torch.tensor([0, 1, 0, 0], dtype=torch.int32)
    t1.root_index.zero_()
    labels = _labels(gh, one, t1, 0.5)
    assert labels.cpu().numpy().tolist() == [0]
    cat = _catalogue(gh, labels, 1, cuda)
    assert [c.tolist() for c in cat] == [[0], [1], [0, 1], [0]]
    # n = max_per_leaf + 1
    d, tree = _build(gh, _random_scene(33, 2), cuda, 32)
    ref = restate_labels(d.cpu().numpy(), [F32(0.3)])[0]
    assert np.array_equal(_labels(gh, d, tree, 0.3).cpu().numpy(), ref) and len(np.unique(ref)) < 33
    # a NaN or infinite coordinate (set after the build: the tree is that of the other spheres): a group
    # of one that does not link its neighbours -- the line falls apart at each of them
    d, tree = _build(gh, _line()[:300], cuda)
    d[100, 0] = float("nan"); d[200, 1] = float("inf"); d[250, 2] = float("nan")
    b = F32(2.0 ** -12)
    ref = restate_labels(d.cpu().numpy(), [b])[0]
    assert sorted(np.bincount(ref)[np.unique(ref)].tolist()) == [1, 1, 1, 49, 49, 99, 100]
    labels = _labels(gh, d, tree, b)
    assert np.array_equal(labels.cpu().numpy(), ref)
    # min_members larger than every group
    group_of, sizes, offsets, members = _catalogue(gh, labels, 101, cuda)
    assert np.all(group_of == -1) and len(sizes) == 0 and offsets.tolist() == [0] and len(members) == 0
    _check_catalogue(_catalogue(gh, labels, 100, cuda), restate_catalogue(ref, 100), "min_members 100")
    group_of, sizes, none, none2 = gh.fof_groups_sph(labels, 2, want_members=False)
    assert none is None and none2 is None and sizes.cpu().numpy().tolist() == [100, 99, 49, 49]


@pytest.mark.gpu
def test_bad_arguments_write_nothing(gh, built, cuda):
    import torch
    d, tree, sh = built["random"]
    n = len(sh)
    labels = torch.full((n,), -7, dtype=torch.int32, device=cuda)
    other = [torch.full((n + 1,), -7, dtype=torch.int32, device=cuda) for _ in range(4)]
    group_of, sizes, offsets, members = other
    counts = torch.full((2,), -7, dtype=torch.int32, device=cuda)
    scene = gh._interp_scene(d, tree)
    lib = gh._lib

    def link(sc=scene, b=0.01, lp=labels):
        return lib.grace_fof_labels_f4(*sc, C.c_float(b), gh._ptr(lp), gh._stream())

    def groups(lp=labels, count=n, mm=1, gp=group_of, sp=sizes, cp=counts):
        return lib.grace_fof_groups(gh._ptr(lp), C.c_size_t(count), C.c_int(mm), gh._ptr(gp), gh._ptr(sp), gh._ptr(cp),
                                    gh._stream())

    def lists(gp=group_of, count=n, sp=sizes, ng=5, op=offsets, mp=members):
        return lib.grace_fof_members(gh._ptr(gp), C.c_size_t(count), gh._ptr(sp), C.c_size_t(ng), gh._ptr(op),
                                     gh._ptr(mp), gh._stream())

    no_spheres = list(scene); no_spheres[0] = C.c_void_p(0)
    no_leaves = list(scene); no_leaves[4] = C.c_void_p(0)
    no_root = list(scene); no_root[5] = C.c_void_p(0)
    too_many = list(scene); too_many[1] = C.c_size_t(2 ** 31)
    for kw in (dict(b=-1.0), dict(b=float("nan")), dict(b=float("inf")), dict(lp=None), dict(sc=no_spheres),
               dict(sc=no_leaves), dict(sc=no_root), dict(sc=too_many)):
        assert link(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    for kw in (dict(mm=0), dict(mm=-3), dict(count=2 ** 31), dict(lp=None), dict(gp=None), dict(sp=None), dict(cp=None)):
        assert groups(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    for kw in (dict(count=2 ** 31), dict(ng=n + 1), dict(gp=None), dict(op=None), dict(sp=None), dict(mp=None)):
        assert lists(**kw) == gh.GRACE_INVALID_ARGUMENT, kw
    # n == 0: GRACE_OK, nothing written
    empty = list(scene); empty[1] = C.c_size_t(0)
    assert link(sc=empty) == gh.GRACE_OK and groups(count=0) == gh.GRACE_OK and lists(count=0, ng=0) == gh.GRACE_OK
    torch.cuda.synchronize()
    assert torch.all(labels == -7) and torch.all(counts == -7) and all(torch.all(t == -7) for t in other)
    with pytest.raises(ValueError):
        gh.fof_labels_sph(d, tree, -1.0)
    with pytest.raises(ValueError):
        gh.fof_labels_sph(d, tree, 0.01, labels=labels[:5])
    with pytest.raises(ValueError):
        gh.fof_groups_sph(labels, 0)
    # labels that are none of the library's (here: the sentinels) belong to no group
    group_of, sizes, offsets, members = _catalogue(gh, labels, 1, cuda)
    assert np.all(group_of == -1) and len(sizes) == 0 and offsets.tolist() == [0] and len(members) == 0
    gh.trace_status()


@pytest.mark.gpu
def test_agrees_with_the_librarys_own_neighbour_lists(gh, cuda):
    """Every pair range_neighbours_sph lists has equal labels, and there are as many labels as the
    list's graph has components."""
    import torch
    n, b = 100_000, 2e-6                                           # (5.8e6 list entries: 58 per particle, cores only)
    d, tree = _build(gh, _clustered_scene(n, 13), cuda)
    counts, _ = gh.range_counts_sph(d, b, d, tree, check=True)
    total = int(counts.sum(dtype=torch.int64))
    print("list entries:", total)
    assert 2_000_000 < total < 10_000_000
    offsets, indices, _ = gh.range_neighbours_sph(d, b, d, tree, want_d2=False, check=True)
    labels = _labels(gh, d, tree, b).cpu().numpy()
    offsets, j = offsets.cpu().numpy(), indices.cpu().numpy().astype(np.int64)
    i = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    assert len(j) == total and np.array_equal(labels[i], labels[j])
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        n_comp = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n)).tocsr(),
                                      directed=False)[0]
    except ImportError:
        parent = np.arange(n, dtype=np.int64)
        unite(parent, i, j)
        unite(parent, i[:1], i[:1])
        n_comp = len(np.unique(parent))
    assert len(np.unique(labels)) == n_comp
    # the graph is no trivial one: a particle with a friend is in a group of k >= 2, which takes
    # k - 1 >= k / 2 off the component count
    befriended = int(np.sum(np.diff(offsets) > 1))
    assert befriended > 1000 and n_comp <= n - befriended // 2


@pytest.mark.gpu
def test_fof_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    d, tree = _build(gh, _clustered_scene(9000, 41), cuda)
    d.cpu().numpy().tofile(str(tmp_path / "s.f32"))                # tree order
    b, mm = 0.001, 3
    exe = str(tmp_path / "dropin_fof")
    _compile_dropin(exe)
    res = subprocess.run([exe, str(tmp_path / "s.f32"), str(b), str(mm)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    names = ("labels", "sizes", "group_of", "offsets", "members")
    got = {t[0]: (int(t[1]), int(t[2])) for t in (ln.split() for ln in res.stdout.splitlines())
           if len(t) == 3 and t[0] in names}
    labels = _labels(gh, d, tree, b)
    group_of, sizes, offsets, members = _catalogue(gh, labels, mm, cuda)
    exp = {"labels": labels.cpu().numpy(), "sizes": sizes, "group_of": group_of, "offsets": offsets, "members": members}
    assert set(got) == set(exp)
    for name, a in exp.items():
        assert got[name] == digest(a), name
    assert len(sizes) > 3 and sizes.max() > 64
