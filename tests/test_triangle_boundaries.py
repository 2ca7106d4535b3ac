"""The closest-hit triangle trace against brute force at its edges, ties, scales and caches.

The scenes (triangle_boundary_scenes.py; tests/test_triangle_boundary_scenes.py checks them on the
CPU) hold exact ties in t, triangles one float inside or outside Moeller-Trumbore's accept tests for
a packet-bounding ray, rays one float longer or shorter than their hit, hits at t = 0, edge-on and
back faces, and meshes that are closed, self-overlapping, stacked, repeated, needle-thin or partly
invalid, at co-ordinates from 1e-3 to 1e5.  Every comparison is of triangle indices with
oracle.brute_closest_tri over the array as the build sorted it, and exact.  Outputs are pre-filled
with -7 so that an unwritten slot fails.  Knobs are covered pairwise under fixed seeds."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import threading

import numpy as np
import pytest
import torch

import triangle_boundary_scenes as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNWRITTEN = -7
BRUTE_LIMIT = 5e8          # rays x triangles above which only the designed rays + 2000 others are compared


def _reset(gh):
    gh.set_ray_reorder(True); gh.set_packet_split(-1); gh.set_treelet_size(-1)
    gh.set_packet_width(-1); gh.set_lattice_split(4)
    gh.set_cache_auto(True); gh.set_cache_validation(True)
    gh.trace_release(); gh.trace_release_rays()


def _knobs(gh, k):
    gh.set_ray_reorder(k.get("reorder", True))
    gh.set_packet_width(k.get("width", -1))
    gh.set_treelet_size(k.get("treelet", -1))
    gh.set_packet_split(k.get("split", -1))
    gh.set_lattice_split(k.get("lat", 4))


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _build(gh, cuda, tris, mpl=8):
    d = _dev(tris, cuda)
    tree = gh.Tree(len(tris), mpl, device=cuda)
    gh.build_tree_tris(d, tree)
    return d, tree


def _trace(gh, rays, d, tree, out=None):
    """trace_closest_tri into an output pre-filled with -7, then trace_status().  Ray counts that are
    no multiple of 32 go to the C entry point, which accepts any count (include/grace_hip.h); the
    Python mirror enforces the reference's multiple of 32."""
    n_rays = len(rays)
    if out is None:
        out = torch.full((n_rays,), UNWRITTEN, dtype=torch.int32, device=d.device)
    if n_rays and n_rays % 32 == 0:
        gh.trace_closest_tri(rays, d, tree, out)
    else:
        gh._check(gh._lib.grace_trace_closest_tri(
            gh._ptr(rays), C.c_size_t(n_rays), gh._ptr(d), C.c_size_t(len(d)), gh._ptr(tree.nodes),
            C.c_size_t(tree.n_nodes), gh._ptr(tree.leaves), gh._ptr(tree.root_index), gh._ptr(out), gh._stream()))
    gh.trace_status()
    return out


def _subset(sc, n_rays, n_tris):
    if n_rays * n_tris <= BRUTE_LIMIT:
        return np.arange(n_rays)
    extra = np.random.default_rng(11).choice(n_rays, 2000, replace=False)
    return np.unique(np.concatenate([sc.designed, extra]))


def _brute(O, rays_np, sorted_tris, sub):
    return O.brute_closest_tri(rays_np[sub], sorted_tris)[0]


def _assert_equal(got, ref, sub, what=""):
    got = got.cpu().numpy()[sub]
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (what, len(bad), sub[bad[:8]], got[bad[:8]], ref[bad[:8]])


# ---- scenes -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _scene(spec):
    what = spec[0]
    if what == "tie":
        return T.tie_scene(*spec[1:])
    if what == "twin":
        return T.edge_twin_scene(*spec[1:])
    return T.mesh_scene(spec[1], spec[2], inf_at_build=spec[3])


TIE_SPECS = [("tie", "unit", False, 2, -1), ("tie", "unit", True, 2, -1), ("tie", "off1024", False, 2, -1),
             ("tie", "off1024", True, 0, 1), ("tie", "2^-10", False, 1, -1), ("tie", "2^-10", True, 2, 1),
             ("tie", "unit", False, 0, -1), ("tie", "unit", False, 1, 1)]
# (axis scenes: seeds 0..5 are +x, +y, +z, -x, -y, -z; odd seeds carry -0.0 components)
TWIN_SPECS = [("twin", kind, scale, i) for kind in ("axis", "pinhole", "iso", "general")
              for i, scale in enumerate(T.TWIN_SCALES)]
# n = 0 stands for max_per_leaf + 1, the smallest mesh a tree can be built over
MESH_SPECS = [("mesh", "icosphere", 0, False), ("mesh", "icosphere", 512, False), ("mesh", "icosphere", 70001, False),
              ("mesh", "soup", 511, False), ("mesh", "soup", 513, True), ("mesh", "soup", 4097, False),
              ("mesh", "sheets", 512, False), ("mesh", "sheets", 4097, False), ("mesh", "sheets", 70001, False),
              ("mesh", "repeated", 0, False), ("mesh", "repeated", 513, False), ("mesh", "repeated", 4097, False)]
SPECS = TIE_SPECS + TWIN_SPECS + MESH_SPECS

KNOBS = {"reorder": (True, False), "width": (-1, 64, 32, 16), "treelet": (-1, 0, 64, 512, 4096),
         "mpl": (1, 8, 32, 100), "split": (1, 4, 8), "lat": (0, 8)}


def _pairwise_rows(seed=5):
    """Knob rows that cover every pair of values of every two knobs (greedy, fixed seed)."""
    names = list(KNOBS)
    rng = np.random.default_rng(seed)
    todo = {(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in KNOBS[a] for vb in KNOBS[b]}
    rows = []
    while todo:
        best, gain = None, -1
        for _ in range(60):
            row = {k: KNOBS[k][rng.integers(len(KNOBS[k]))] for k in names}
            g = sum((a, row[a], b, row[b]) in todo for a, b in itertools.combinations(names, 2))
            if g > gain:
                best, gain = row, g
        rows.append(best)
        todo -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(names, 2)}
    return rows


ROWS = _pairwise_rows()
assert len(ROWS) <= len(SPECS)
# every scene once; the rows in turn, starting with another row in each scene family
CASES = [(spec, ROWS[(i * 7 + 3) % len(ROWS)] if i >= len(ROWS) else ROWS[i]) for i, spec in enumerate(SPECS)]


def _case_id(case):
    spec, k = case
    return "-".join(str(x) for x in spec) + "|" + ",".join("%s=%s" % kv for kv in k.items())


def _materialise(gh, cuda, spec, mpl, late=True):
    """(scene, rays tensor, sorted triangles on the device, tree); a mesh scene's late invalid
    triangles are written into the sorted array after the build."""
    if spec[0] == "mesh" and spec[2] == 0:
        spec = (spec[0], spec[1], mpl + 1, spec[3])
    sc = _scene(spec)
    d, tree = _build(gh, cuda, sc.tris, mpl)
    if late and spec[0] == "mesh":
        pos = np.random.default_rng(5).choice(len(d), len(sc.late), replace=False)
        for i, tri in zip(pos, sc.late):
            d[int(i)] = torch.from_numpy(tri).to(cuda)
    return sc, _dev(sc.rays, cuda), d, tree


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_scene_equals_brute_force(gh, oracle, cuda, case):
    spec, k = case
    try:
        sc, rays, d, tree = _materialise(gh, cuda, spec, k["mpl"])
        st = d.cpu().numpy()
        sub = _subset(sc, len(rays), len(st))
        ref = _brute(oracle, sc.rays, st, sub)
        if spec[0] != "mesh" or spec[2] != 0:
            assert (ref >= 0).any()
        _knobs(gh, k)
        _assert_equal(_trace(gh, rays, d, tree), ref, sub, "first call")
        # packet and lattice splitting have nothing to act on here: the result is the same
        gh.set_packet_split(-1); gh.set_lattice_split(4)
        _assert_equal(_trace(gh, rays, d, tree), ref, sub, "default splits")
    finally:
        _reset(gh)


@pytest.mark.parametrize("n", [511, 512, 513, 4097])
def test_treelet_thresholds(gh, oracle, cuda, n):
    """Meshes one below, at and one above the automatic treelet of 512 (and well above it), under
    every treelet size: subtrees switch between the sweep and the walk at different nodes, the
    closest hit stays the same."""
    try:
        for kind in ("sheets", "icosphere"):
            sc, rays, d, tree = _materialise(gh, cuda, ("mesh", kind, n, False), 8)
            st = d.cpu().numpy()
            sub = np.arange(len(rays))
            ref = _brute(oracle, sc.rays, st, sub)
            assert (ref >= 0).any() and (ref < 0).any()
            for treelet in (-1, 0, 64, 511, 512, 513, 4096):
                for reorder in (True, False):
                    gh.set_treelet_size(treelet); gh.set_ray_reorder(reorder)
                    _assert_equal(_trace(gh, rays, d, tree), ref, sub, (kind, treelet, reorder))
    finally:
        _reset(gh)


@pytest.mark.parametrize("spec", [("tie", "unit", True, 2, -1), ("twin", "general", "1e3r", 2), ("twin", "axis", "unit", 5),
                                  ("mesh", "sheets", 4097, False)], ids=lambda s: "-".join(map(str, s)))
def test_ray_counts(gh, oracle, cuda, spec):
    """1, 63, 65 rays and the whole batch (4133 and 4225 are no multiples of 64 above 4096); a
    zero-ray call is a no-op that leaves the output untouched."""
    try:
        sc, rays, d, tree = _materialise(gh, cuda, spec, 8)
        st = d.cpu().numpy()
        full = _brute(oracle, sc.rays, st, np.arange(len(rays)))
        first = int(np.nonzero(full >= 0)[0][0])
        counts = [1, 63, 65] + ([len(rays)] if len(rays) % 64 else [len(rays) - 27])
        for reorder, width in ((True, -1), (False, 16), (False, 64), (True, 32)):
            gh.set_ray_reorder(reorder); gh.set_packet_width(width)
            for n_rays in counts:
                lo = min(first, len(rays) - n_rays)
                part = rays[lo:lo + n_rays]
                got = _trace(gh, part, d, tree)
                _assert_equal(got, full[lo:lo + n_rays], np.arange(n_rays), (reorder, width, n_rays))
        out = torch.full((64,), UNWRITTEN, dtype=torch.int32, device=cuda)
        _trace(gh, rays[:0], d, tree, out)
        assert bool((out == UNWRITTEN).all())
    finally:
        _reset(gh)


# ---- the caller-functor path --------------------------------------------------------------------
@pytest.fixture(scope="module")
def dropin_exe(tmp_path_factory):
    from test_gpu_dropin import build_dropin
    return build_dropin(tmp_path_factory.mktemp("dropin_tri"), "dropin_triangles")


@pytest.mark.parametrize("spec", [("tie", "unit", True, 2, -1), ("twin", "pinhole", "1e3r", 2)],
                         ids=lambda s: "-".join(map(str, s)))
def test_ties_and_twins_through_the_caller_functor_path(tmp_path, dropin_exe, oracle, cuda, spec):
    """tests/cpp/dropin_triangles.hip (the generic forms of the drop-in headers with the caller's own
    primitive and functors) on a tie scene and a twin scene: its closest hits equal brute force over
    the triangles as it sorted them."""
    sc = _scene(spec)
    rays = sc.rays[: len(sc.rays) // 32 * 32]                    # (the header mirror wants a multiple of 32)
    sc.tris.tofile(str(tmp_path / "tris.f32")); rays.tofile(str(tmp_path / "rays.f32"))
    prefix = str(tmp_path / "out")
    r = subprocess.run([dropin_exe, str(tmp_path / "tris.f32"), str(tmp_path / "rays.f32"), "8", prefix],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    st = np.fromfile(prefix + ".tris", np.float32).reshape(-1, 9)
    got = np.fromfile(prefix + ".closest", np.int32)
    ref = oracle.brute_closest_tri(rays, st)[0]
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (len(bad), bad[:8], got[bad[:8]], ref[bad[:8]])
    assert (ref >= 0).sum() > len(ref) // 8


# ---- caches -------------------------------------------------------------------------------------
CACHE_SPECS = [("tie", "off1024", True, 2, -1), ("twin", "iso", "1e5r", 4), ("mesh", "sheets", 4097, False)]


@pytest.mark.parametrize("validation", [True, False])
@pytest.mark.parametrize("spec", CACHE_SPECS, ids=lambda s: "-".join(map(str, s)))
def test_every_caching_regime_gives_the_same_answer(gh, oracle, cuda, spec, validation):
    """trace_prepare_tri followed by two traces, the automatic cache over three calls on the same
    arrays, and set_cache_auto(False): all equal brute force, with validation on and off."""
    try:
        sc, rays, d, tree = _materialise(gh, cuda, spec, 8)
        sub = np.arange(len(rays))
        ref = _brute(oracle, sc.rays, d.cpu().numpy(), sub)
        gh.set_cache_validation(validation)
        gh.trace_prepare_tri(d, tree)
        for rep in range(2):
            _assert_equal(_trace(gh, rays, d, tree), ref, sub, ("prepared", rep))
        gh.trace_release(); gh.trace_release_rays()
        for rep in range(3):                                       # the second call fills the cache
            _assert_equal(_trace(gh, rays, d, tree), ref, sub, ("automatic", rep))
        gh.trace_release(); gh.trace_release_rays()
        gh.set_cache_auto(False)
        for rep in range(2):
            _assert_equal(_trace(gh, rays, d, tree), ref, sub, ("no cache", rep))
    finally:
        _reset(gh)


def _move_away(d, ref, count=50):
    """Moves `count` of the triangles that are some ray's closest hit far out of every ray's reach
    (in place: same addresses).  Returns their indices."""
    hit = np.unique(ref[ref >= 0])
    pick = hit[np.linspace(0, len(hit) - 1, min(count, len(hit))).astype(np.int64)]
    for i in pick:
        d[int(i), 0:3] = d[int(i), 0:3] + 4096.0
    return pick


@pytest.mark.parametrize("spec", CACHE_SPECS, ids=lambda s: "-".join(map(str, s)))
def test_triangles_changed_in_place_under_the_automatic_cache(gh, oracle, cuda, spec):
    """Two traces fill the cache (bounding spheres, cluster boxes, the fp64 copy of every triangle).
    Then 50 triangles that were closest hits move out of their rays' way, in place and without a
    rebuild: the next trace equals brute force over the new array."""
    try:
        sc, rays, d, tree = _materialise(gh, cuda, spec, 8)
        sub = np.arange(len(rays))
        ref = _brute(oracle, sc.rays, d.cpu().numpy(), sub)
        for rep in range(3):
            _assert_equal(_trace(gh, rays, d, tree), ref, sub, ("before", rep))
        moved = _move_away(d, ref)
        ref2 = _brute(oracle, sc.rays, d.cpu().numpy(), sub)
        assert (ref2 != ref).sum() >= len(moved) // 2 and not np.isin(ref2, moved).any()
        for rep in range(2):
            _assert_equal(_trace(gh, rays, d, tree), ref2, sub, ("after", rep))
    finally:
        _reset(gh)


def test_tree_rebuilt_in_place_after_a_reshuffle(gh, oracle, cuda):
    """The cached scene's three arrays keep their addresses and sizes while the triangles are
    reshuffled, 50 of them replaced, and the tree rebuilt into the same buffers."""
    try:
        sc = _scene(("mesh", "sheets", 4097, False))
        rays = _dev(sc.rays, cuda)
        d = _dev(sc.tris, cuda)
        tree = gh.Tree(len(d), 8, device=cuda)
        nodes0, leaves0 = tree.nodes, tree.leaves                  # full-capacity buffers, reused below
        gh.build_tree_tris(d, tree)
        sub = np.arange(len(rays))
        ref = _brute(oracle, sc.rays, d.cpu().numpy(), sub)
        for rep in range(3):
            _assert_equal(_trace(gh, rays, d, tree), ref, sub, ("before", rep))
        rng = np.random.default_rng(2)
        new = d.cpu().numpy()[rng.permutation(len(d))]
        new[:50, 2] = new[:50, 2] + 0.07                               # 50 triangles lifted above their sheet
        new[50:100] = new[50:100][:, [0, 1, 2, 6, 7, 8, 3, 4, 5]]      # 50 turned into back faces
        d.copy_(torch.from_numpy(new).to(cuda))
        tree2 = gh.Tree.__new__(gh.Tree)
        tree2.max_per_leaf = 8; tree2.nodes = nodes0; tree2.leaves = leaves0; tree2.root_index = tree.root_index
        gh.build_tree_tris(d, tree2)
        assert tree2.nodes.data_ptr() == tree.nodes.data_ptr() and tree2.leaves.data_ptr() == tree.leaves.data_ptr()
        ref2 = _brute(oracle, sc.rays, d.cpu().numpy(), sub)
        for rep in range(3):
            _assert_equal(_trace(gh, rays, d, tree2), ref2, sub, ("after", rep))
    finally:
        _reset(gh)


def test_triangles_freed_and_reallocated_at_the_same_address(gh, oracle, cuda):
    """torch's allocator hands the address of a freed mesh to the next one of the same size: the
    freed mesh's cached records must not come back."""
    try:
        rays_np = T.mesh_rays(np.random.default_rng(1))
        rays = _dev(rays_np, cuda)
        sub = np.arange(len(rays))
        answers, ptrs = [], []
        for k in range(3):
            sc = T.mesh_scene("sheets", 4097, seed=k + 1)
            d, tree = _build(gh, cuda, sc.tris, 8)
            ref = _brute(oracle, rays_np, d.cpu().numpy(), sub)
            for rep in range(3):
                _assert_equal(_trace(gh, rays, d, tree), ref, sub, (k, rep))
            answers.append(ref); ptrs.append(d.data_ptr())
            del d, tree
        assert not np.array_equal(answers[0], answers[1])
    finally:
        _reset(gh)


def test_trusted_pinned_scene_keeps_its_answer_until_released(gh, oracle, cuda):
    """set_cache_validation(False) with a prepared (pinned) scene: the records computed by
    trace_prepare_tri are used on the caller's promise, so triangles changed behind the library's
    back keep giving the prepared scene's answer; trace_release() ends that."""
    try:
        sc, rays, d, tree = _materialise(gh, cuda, ("mesh", "sheets", 4097, False), 8)
        sub = np.arange(len(rays))
        ref = _brute(oracle, sc.rays, d.cpu().numpy(), sub)
        gh.set_cache_validation(False)
        gh.trace_prepare_tri(d, tree)
        for rep in range(2):
            _assert_equal(_trace(gh, rays, d, tree), ref, sub, ("trusted", rep))
        _move_away(d, ref)
        ref2 = _brute(oracle, sc.rays, d.cpu().numpy(), sub)
        assert not np.array_equal(ref, ref2)
        for rep in range(2):
            _assert_equal(_trace(gh, rays, d, tree), ref, sub, ("trusted, changed behind its back", rep))
        gh.trace_release()
        for rep in range(3):
            _assert_equal(_trace(gh, rays, d, tree), ref2, sub, ("released", rep))
    finally:
        _reset(gh)


# ---- streams and contexts -----------------------------------------------------------------------
STREAM_SPECS = [("tie", "unit", True, 2, -1), ("twin", "pinhole", "1e5", 3)]


def test_a_second_context_on_its_own_stream(gh, oracle, cuda):
    try:
        for spec in STREAM_SPECS:
            sc, rays, d, tree = _materialise(gh, cuda, spec, 8)
            sub = np.arange(len(rays))
            ref = _brute(oracle, sc.rays, d.cpu().numpy(), sub)
            base = _trace(gh, rays, d, tree)
            _assert_equal(base, ref, sub, "default context")
            torch.cuda.synchronize()
            stream = torch.cuda.Stream()
            ctx = gh.Context()
            try:
                ctx.make_current()
                with torch.cuda.stream(stream):
                    outs = [_trace(gh, rays, d, tree) for _ in range(3)]
                    stream.synchronize()
            finally:
                gh.Context.reset_current()
                ctx.destroy()
            for o in outs:
                assert torch.equal(o, base)
    finally:
        _reset(gh)


def test_calls_alternating_between_two_streams(gh, oracle, cuda):
    """Six calls back to back, alternating between two streams and two scenes on the default context,
    without a host synchronisation in between."""
    try:
        built = [_materialise(gh, cuda, spec, 8) for spec in STREAM_SPECS]
        refs = [_brute(oracle, sc.rays, d.cpu().numpy(), np.arange(len(rays))) for sc, rays, d, tree in built]
        outs = [torch.full((len(built[rep % 2][1]),), UNWRITTEN, dtype=torch.int32, device=cuda) for rep in range(6)]
        streams = (torch.cuda.Stream(), torch.cuda.Stream())
        torch.cuda.synchronize()
        for rep in range(6):
            sc, rays, d, tree = built[rep % 2]
            with torch.cuda.stream(streams[rep % 2]):
                _trace(gh, rays, d, tree, outs[rep])
        torch.cuda.synchronize()
        gh.trace_status()
        for rep in range(6):
            _assert_equal(outs[rep], refs[rep % 2], np.arange(len(refs[rep % 2])), rep)
    finally:
        _reset(gh)


def test_two_threads_with_a_context_and_a_mesh_each(gh, oracle, cuda):
    try:
        built = [_materialise(gh, cuda, spec, 8) for spec in STREAM_SPECS]
        refs = [_brute(oracle, sc.rays, d.cpu().numpy(), np.arange(len(rays))) for sc, rays, d, tree in built]
        for (sc, rays, d, tree), ref in zip(built, refs):
            _assert_equal(_trace(gh, rays, d, tree), ref, np.arange(len(ref)), "default stream")
        torch.cuda.synchronize()
        errors = []

        def worker(k):
            try:
                torch.cuda.set_device(cuda)
                sc, rays, d, tree = built[k]
                with gh.Context():
                    stream = torch.cuda.Stream(device=cuda)
                    with torch.cuda.stream(stream):
                        for it in range(4):
                            out = _trace(gh, rays, d, tree)
                            stream.synchronize()
                            if not np.array_equal(out.cpu().numpy(), refs[k]):
                                errors.append((k, it, "differs"))
            except BaseException as e:      # noqa: BLE001 -- reported to the main thread
                errors.append((k, repr(e)[:2000]))

        threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads), "a worker did not finish"
        assert not errors, errors
    finally:
        _reset(gh)
