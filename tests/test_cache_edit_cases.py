"""CPU checks of tests/cache_edit_cases.py: every one-word edit sits in the chunk of the signature
pass it is meant for, keeps the tree valid, can be undone bit for bit, and changes the brute-force
answer of enough rays that a trace from stale records cannot pass for a fresh one."""
import os
import re

import numpy as np
import pytest

import cache_edit_cases as K

F32, F64, U32 = np.float32, np.float64, np.uint32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "grace-devel_amd", "csrc")
SPHERE_CASES = [("small", p) for p in ("first", "mid", "last", "cut")] + \
    [("wide", p) for p in ("first", "stride_end", "stride_begin", "last", "cut")]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_constants_are_the_sources():
    sig = _source("trace_cache.hip")
    assert re.search(r"constexpr int SIG_BLOCK = %d;" % K.SIG_BLOCK, sig)
    assert re.search(r"constexpr int SIG_GRID = %d;" % K.SIG_GRID, sig)
    assert "c += stride" in sig and "stride = size_t(gridDim.x) * blockDim.x" in sig
    assert "n_chunks = (a.words[k] + 3) / 4" in sig and "reinterpret_cast<const uint4*>(w)[c]" in sig
    assert K.SIG_THREADS == 262144 and K.CHUNK_BYTES == 4 * K.CHUNK_WORDS == 16
    order = _source("trace_coherence.hip")
    assert "while ((size_t(1) << (want_bits - 2)) < packets64 && want_bits < 30) ++want_bits;" in order
    assert "want_bits = ((want_bits + 7) / 8) * 8;" in order
    trace = _source("trace.hip")
    assert "rq.nodes_bytes = n_nodes * 64" in trace and "rq.leaves_bytes = (n_nodes + 1) * 16" in trace
    assert "rq.rays_bytes = n_rays * 28" in trace


def test_the_batches_reach_one_two_and_three_gated_sort_passes():
    n = {name: len(K.batch(name)) for name in K.BATCHES}
    assert (n["z4096"], n["z4128"], n["z1024"]) == (4096, 4096 + 32, 2 ** 20 + 64)
    assert [K.sort_passes(n[b]) for b in ("z4096", "z4128", "z388", "z1024")] == [1, 2, 2, 3]
    assert K.sort_passes(2 ** 20) == 2                       # the third pass starts above 2^20 rays
    for name in ("full4096", "z4096", "z4128", "z388", "z1024", "y4096"):
        assert n[name] % 32 == 0, name                       # what the Python wrappers admit
    # 388 x 388 = 150544 is 16 * 97^2: 16 copies of the first ray make it a multiple of 32
    assert n["z388"] == 150560 and K.STRADDLE_SIDE ** 2 == 150544 and K.STRADDLE_RAY < 150544
    assert (7 * n["x4097"]) % 4 == 3 and (7 * n["x4098"]) % 4 == 2


def test_signature_strides_and_chunks():
    # the straddling ray: its words 0..3 end chunk SIG_THREADS - 1, its word 4 (oy) begins the next
    i, w = K.STRADDLE_RAY, K.STRADDLE_WORD
    assert (i, w) == (149796, K.OY)
    assert K.chunk_of(7 * i + w - 1) == K.SIG_THREADS - 1 and K.chunk_of(7 * i + w) == K.SIG_THREADS
    assert (7 * i + w) % 4 == 0
    assert K.iteration_of(K.chunk_of(7 * (i - 1) + 6)) == 0 and 7 * 149797 * 4 > K.SIG_THREADS * 16
    c = K.ray_case("small", "z388", "inside", i, w)
    assert c.edit.words == [K.SIG_THREADS * 4] and K.iteration_of(c.edit.chunks[0]) == 1
    c = K.ray_case("small", "z388", "inside", -1, K.OX)
    assert c.ray == len(c.rays) - 1 and K.iteration_of(c.edit.chunks[0]) == 1
    # wide: the probes' chunks are their sorted indices (16 bytes a sphere)
    w_ = K.wide()
    assert len(w_.spheres) == K.SIG_THREADS + 64
    assert w_.probes == {"first": 0, "stride_end": 262143, "stride_begin": 262144, "last": len(w_.spheres) - 1}
    its = {p: K.iteration_of(K.shrink(w_, j).chunks[0]) for p, j in w_.probes.items()}
    assert its == {"first": 0, "stride_end": 0, "stride_begin": 1, "last": 1}
    for p, j in w_.probes.items():
        e = K.shrink(w_, j)
        assert e.chunks == [j] and e.words[0] % 4 == 3
        assert (e.chunks[0] % K.SIG_THREADS == K.SIG_THREADS - 1) == (p == "stride_end")
        assert (e.chunks[0] % K.SIG_THREADS == 0) == (p in ("first", "stride_begin"))


def test_views_are_unaligned_and_last_chunks_partial():
    assert [K.view_offset_bytes(k, K.RAY_WORDS) for k in (1, 2, 3)] == [28, 56, 84]
    assert [K.view_offset_bytes(k, K.RAY_WORDS) % 16 for k in (1, 2, 3)] == [12, 8, 4]
    assert K.view_offset_bytes(1, K.TRI_WORDS) == 36 and 36 % 16 == 4
    # C entry point: 4097 / 4098 rays end in a chunk of 3 / 2 words, which holds the edited word
    for name, coord, held in (("x4097", K.OY, 3), ("x4098", K.OZ, 2)):
        for kind in ("inside", "outside"):
            c = K.ray_case("small", name, kind, -1, coord)
            words = 7 * len(c.rays)
            assert words % 4 == held and c.edit.chunks == [(words + 3) // 4 - 1]
            assert c.edit.words[0] >= words - held and K.batch_axis(name) == 0
    # the triangles: 9 n % 4 != 0; the last triangle's last word is alone in the final chunk
    t = K.tris()
    words = 9 * len(t.tris)
    assert words % 4 == 1 and t.probes["last"] == len(t.tris) - 1
    e = K.collapse(t, t.probes["last"])
    assert e.words == [words - 4, words - 1] and e.chunks[1] == (words + 3) // 4 - 1
    # (in an aligned array words - 4 lies in a whole chunk: the one-word fold touches the partial chunk alone)
    assert K.fold(t, t.probes["last"]).words == [words - 1] and (words - 4) // 4 != (words - 1) // 4
    assert 0.25 * len(t.tris) < t.probes["mid"] < 0.75 * len(t.tris)


@pytest.fixture(scope="module")
def trees(oracle):
    out = {}
    for name, fn in K.SCENES.items():
        s = fn().spheres
        out[name] = oracle.albvh(s, oracle.deltas_euclid(s), fn().mpl)
    return out


@pytest.mark.parametrize("name", ["small", "wide"])
def test_scenes_are_in_tree_order_in_the_unit_box(oracle, name):
    sc = K.SCENES[name]()
    s = sc.spheres
    assert np.all(s[:, :3] > 0) and np.all(s[:, :3] < 1) and np.all(s[:, 3] > 0)
    keys = oracle.morton_keys30(s, *K.UNIT)
    assert np.all(np.diff(keys.astype(np.int64)) >= 0), "not in Morton order: the build would move spheres"
    assert sc.probes["first"] == 0 and sc.probes["last"] == len(s) - 1
    if name == "small":
        assert 2900 <= len(s) <= 3100 and 0.25 * len(s) < sc.probes["mid"] < 0.75 * len(s)
        # the lattice rule of choose_variants: r2_min < 2 e1 e2 / n, before and after any shrink
        for b in ("full4096", "z4096", "z4128"):
            r = K.batch(b)
            e1, e2 = (F32(r[:, k].max()) - F32(r[:, k].min()) for k in (K.OX, K.OY))
            assert F32(s[:, 3].min()) ** 2 < F32(2) * (e1 * e2 / F32(len(r))), b
    else:
        sub = np.arange(0, 4096, 16)
        assert oracle.brute_hitcounts(K.batch("full4096")[sub], s).mean() < 16      # short hit lists


def test_the_triangles_are_in_tree_order(oracle):
    t = K.tris().tris
    bot, top = oracle.tri_centroid_bounds(t)
    keys = oracle.morton_keys30_tri(t, bot, top)
    assert np.all(np.diff(keys.astype(np.int64)) >= 0)
    assert len(t) == K.N_TRIS and 1900 <= len(t) <= 2100


@pytest.mark.parametrize("scene,probe", SPHERE_CASES)
def test_sphere_edits_are_not_blind_and_keep_the_tree(oracle, trees, scene, probe):
    c = K.sphere_case(scene, "full4096", probe)
    s = c.scene.spheres
    nodes, leaves, root, _ = trees[scene]
    assert len(c.affected) >= 8, (scene, probe, len(c.affected))
    assert set(c.affected) <= set(c.sub) and len(c.sub) <= len(c.affected) + 256
    if probe == "cut":
        # the last leaf ends the array, holds more than one sphere, and the sphere that leaves is a probe
        assert leaves[0, 0] == 0 and leaves[-1, 0] + leaves[-1, 1] == len(s) and leaves[-1, 1] > 1
        e = K.cut_last_leaf(leaves)
        n_nodes = len(leaves) - 1
        assert e.words == [4 * n_nodes + 1] and e.chunks == [n_nodes]           # the leaves' last chunk ...
        assert K.scene_chunk(len(s), n_nodes, e) == [len(s) + 4 * n_nodes + n_nodes]   # ... of the third array
        assert c.j == c.scene.probes["last"] == len(s) - 1
        cut = e.apply(leaves.copy())
        assert cut[-1, 0] + cut[-1, 1] == len(s) - 1 and np.array_equal(cut[:-1], leaves[:-1])
        assert np.array_equal(e.inverse().apply(cut), leaves)
        return
    after = c.edit.apply(s.copy())
    j = c.j
    assert c.edit.array == "spheres" and len(c.edit.words) == 1
    assert np.array_equal(after[:, :3], s[:, :3]) and 0 < after[j, 3] < s[j, 3]   # the radius only decreases
    assert np.array_equal(np.delete(after, j, axis=0), np.delete(s, j, axis=0))
    # the shrunk sphere inside its leaf's box (the union of its spheres' boxes as they were built)
    leaf = int(np.searchsorted(leaves[:, 0], j, side="right")) - 1
    members = s[leaves[leaf, 0]:leaves[leaf, 0] + leaves[leaf, 1]]
    assert leaves[leaf, 0] <= j < leaves[leaf, 0] + leaves[leaf, 1]
    lo = (members[:, :3] - members[:, 3:4]).min(axis=0); hi = (members[:, :3] + members[:, 3:4]).max(axis=0)
    assert np.all(after[j, :3] - after[j, 3] >= lo) and np.all(after[j, :3] + after[j, 3] <= hi)
    assert np.array_equal(c.edit.inverse().apply(after).view(U32), s.view(U32))


def _lattice_around(centre, axis, pitch):
    """17 x 17 rays along +e_axis with the batch's spacing, centred on `centre`."""
    t0, t1 = [k for k in range(3) if k != axis]
    g = np.arange(-8, 9) * pitch
    r = np.zeros((17 * 17, 7), F32)
    r[:, axis] = 1
    r[:, 3 + t0] = (centre[t0] + np.repeat(g, 17)).astype(F32)
    r[:, 3 + t1] = (centre[t1] + np.tile(g, 17)).astype(F32)
    r[:, 3 + axis] = K.RAY_START; r[:, 6] = K.RAY_LEN
    return r


@pytest.mark.parametrize("case", K.RAY_CASES, ids=lambda c: "-".join(map(str, c)))
def test_ray_edits_are_not_blind(oracle, case):
    name, kind, i, coord = case
    c = K.ray_case("small", *case)
    s = c.scene.spheres
    rays, new = c.rays, K.edited_rays(name, c.edit)
    i = c.ray
    assert i in (0, len(rays) - 1) or name in ("z388", "z1024")
    # from no hit to some: the column above the ray's first position is empty, its new path crosses a probe
    assert c.counts[0] == 0 and c.counts[1] > 0 and list(c.affected) == [i] and i in c.sub
    probe = K._probe_for(*case).astype(F32)
    # (cases whose probes would lie within 1e-3 of each other share one)
    row = np.nonzero((np.abs(s - probe).max(axis=1) < 1e-3) & (s[:, 3] == probe[3]))[0]
    assert len(row) == 1 and oracle.brute_hitcounts(new[i:i + 1], s[row])[0] == 1
    # the probe is wide enough for eight rays at the batch's spacing
    side, axis, (lo, span), _ = K.BATCHES[name]
    assert oracle.brute_hitcounts(_lattice_around(probe[:3], axis, span / side), s[row]).sum() >= 8
    # one or two words of ray i alone, undone bit for bit
    assert len(c.edit.words) <= 2 and all(w // 7 == i for w in c.edit.words)
    changed = np.nonzero((new.view(U32) != rays.view(U32)).any(axis=1))[0]
    assert list(changed) == [i]
    assert np.array_equal(c.edit.inverse().apply(new.copy()).view(U32), rays.view(U32))
    ext = lambda r: (r[:, :6].min(axis=0), r[:, :6].max(axis=0))
    (lo0, hi0), (lo1, hi1) = ext(rays), ext(new)
    if kind == "inside":
        assert np.array_equal(lo0, lo1) and np.array_equal(hi0, hi1)        # the extents do not move
    elif kind == "outside":
        assert hi1[coord] == F32(F64(hi0[coord]) + K.OUTSIDE) and np.array_equal(lo0, lo1)
        assert np.all(probe[:3] > 0) and np.all(probe[:3] < 1)              # inside the scene's own bounds
        assert oracle.brute_hitcounts(rays, s[row]).sum() == 0               # beyond every ray of the batch
    else:
        assert np.array_equal(lo0[:3], hi0[:3]) and not np.array_equal(lo1[:3], hi1[:3])   # no longer one direction
        assert np.array_equal(lo0[3:], lo1[3:]) and np.array_equal(hi0[3:], hi1[3:])       # (the origins stay)
        assert tuple(new[i, :3]) == K.TILT


@pytest.mark.parametrize("probe,kind", [("mid", "collapse"), ("last", "collapse"), ("last", "fold")])
def test_collapsed_triangles_are_not_blind(oracle, probe, kind):
    c = K.tri_case(probe, kind)
    t = c.scene.tris
    after = c.edit.apply(t.copy())
    assert len(c.affected) >= 8 and np.all(c.before[c.affected] == c.j) and not np.any(c.after == c.j)
    assert c.before[c.ray] == c.j and c.after[c.ray] == -1            # nothing behind it on its own ray
    # zero area, and inside the box of the original
    e1, e2 = after[c.j, 3:6].astype(F64), after[c.j, 6:9].astype(F64)
    assert not np.any(np.cross(e1, e2)) and np.any(np.cross(t[c.j, 3:6].astype(F64), t[c.j, 6:9].astype(F64)))
    corners = lambda x: np.stack([x[0:3], x[0:3] + x[3:6], x[0:3] + x[6:9]])
    was, now = corners(t[c.j]), corners(after[c.j])
    assert np.all(now.min(axis=0) >= was.min(axis=0)) and np.all(now.max(axis=0) <= was.max(axis=0))
    assert np.array_equal(np.delete(after, c.j, axis=0), np.delete(t, c.j, axis=0))
    assert np.array_equal(c.edit.inverse().apply(after).view(U32), t.view(U32))
