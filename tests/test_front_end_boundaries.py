"""The stages that feed the pipeline -- Morton keys and centroid bounds (morton.hip), adjacent deltas
(deltas.hip), ray generators (rays.hip) -- at their edges: the second pass of the grid-stride loops
(more than 2^20 elements), cell boundaries and box corners, a degenerate axis, the wave and block
edges of the delta kernels, every HEALPix resolution class, and the random generators compared with
an independent evaluation of the map (seed, index) -> ray.

Inputs and restatements come from tests/front_end_cases.py, whose claims tests/test_front_end_cases.py
proves on the CPU.  Every output buffer is pre-filled with a value the contract cannot produce (a NaN
with a payload, 0xDEADBEEF words), so a slot no thread wrote fails its comparison.

What no comparison of outputs here can see: a grid-stride step that is too short (blockDim.x for
gridDim.x * blockDim.x) in a key or min/max kernel.  Every element is then still written, with the
same value, by several threads; only the run time changes.  A step that is too long leaves pre-filled
slots and fails.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import front_end_cases as F

pytestmark = pytest.mark.gpu

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _signed(value, bits):
    return value - (1 << bits) if value >= 1 << (bits - 1) else value


def _filled(shape, dtype, cuda):
    """A device tensor of `dtype` holding the pre-fill pattern of its type."""
    if dtype == torch.float32:
        return torch.full(shape, F.NAN_BITS, dtype=torch.int32, device=cuda).view(torch.float32)
    if dtype == torch.float64:
        return torch.full(shape, F.NAN64_BITS, dtype=torch.int64, device=cuda).view(torch.float64)
    if dtype == torch.int32:
        return torch.full(shape, _signed(F.KEY32_FILL, 32), dtype=torch.int32, device=cuda)
    return torch.full(shape, _signed(F.KEY64_FILL, 64), dtype=torch.int64, device=cuda)


def _unsigned(t):
    a = t.cpu().numpy()
    return a.view({4: U32, 8: U64}[a.itemsize])


def _bits(t):
    """Float tensors as unsigned words, for bit-for-bit comparison (NaNs and signed zeros included)."""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view({4: U32, 8: U64}[a.itemsize])


def _vec(v, real=F32):
    ct = C.c_float if real == F32 else C.c_double
    return (ct * len(v))(*[float(x) for x in v])


def _raw(gh, name, *args):
    gh._check(getattr(gh.exported_symbols(), name)(*args, gh._stream()))


def _keys(gh, cuda, kind, data, lo, hi, bits, real):
    """Keys of spheres / generic points / triangles through the raw entry points (the Python binding
    has no 30-bit double-bounds form), into a pre-filled buffer."""
    n = len(data)
    keys = _filled((n,), torch.int32 if bits == 30 else torch.int64, cuda)
    d3 = "_d3" if real == F64 else ""
    b, t = _vec(lo, real), _vec(hi, real)
    if kind == "spheres":
        _raw(gh, "grace_morton_keys%d_f4%s" % (bits, d3), gh._ptr(data), C.c_size_t(n), b, t, gh._ptr(keys))
    elif kind == "points":
        _raw(gh, "grace_morton_keys%d_points%s" % (bits, d3), gh._ptr(data), C.c_size_t(n),
             C.c_int(int(data.dtype == torch.float64)), C.c_int(data.shape[1]), b, t, gh._ptr(keys))
    else:
        assert bits == 30 and real == F32
        _raw(gh, "grace_morton_keys30_tri", gh._ptr(data), C.c_size_t(n), b, t, gh._ptr(keys))
    return _unsigned(keys)


def _oracle_keys(oracle, s, lo, hi, bits, real):
    if bits == 30:
        return oracle.morton_keys30(s, lo, hi) if real == F32 else oracle.morton_keys30_d3(s, lo, hi)
    return oracle.morton_keys63(s, lo, hi, double_bounds=(real == F64))


# ---------------------------------------------------------------------------------------------------
# 1. Morton keys
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("real", [F32, F64], ids=["float_bounds", "double_bounds"])
@pytest.mark.parametrize("bits", [30, 63])
def test_sphere_keys_at_the_block_and_grid_sizes(gh, oracle, cuda, bits, real):
    lo, hi = F.box("offset", real)
    pool = F.pool_points("offset")
    ref = _oracle_keys(oracle, pool, lo, hi, bits, real)
    dpool = _dev(pool, cuda)
    for n in F.SIZES:
        idx = F.pool_index(n)
        got = _keys(gh, cuda, "spheres", dpool[_dev(idx, cuda)].contiguous(), lo, hi, bits, real)
        assert np.array_equal(got, ref[idx]), n


@pytest.mark.parametrize("dtype,cols", F.POINT_LAYOUTS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_point_keys_and_bounds_at_the_block_and_grid_sizes(gh, oracle, cuda, dtype, cols):
    pool = F.pool_points("negative", cols=cols, dtype=dtype)
    dpool = _dev(pool, cuda)
    refs = {(bits, real): oracle.morton_keys_points(pool, *F.box("negative", real), bits, real == F64)
            for bits in (30, 63) for real in (F32, F64)}
    for n in F.SIZES:
        idx = F.pool_index(n)
        d = dpool[_dev(idx, cuda)].contiguous()
        for (bits, real), ref in refs.items():
            lo, hi = F.box("negative", real)
            assert np.array_equal(_keys(gh, cuda, "points", d, lo, hi, bits, real), ref[idx]), (n, bits, real)
        b, t = (C.c_float * 3)(), (C.c_float * 3)()
        _raw(gh, "grace_centroid_bounds_points", gh._ptr(d), C.c_size_t(n), C.c_int(int(dtype == F64)),
             C.c_int(cols), b, t)
        rb, rt = oracle.centroid_bounds_points(pool[idx[:min(n, F.POOL)]])
        assert np.array_equal(np.array(b, F32), rb) and np.array_equal(np.array(t, F32), rt), n


def test_triangle_keys_and_centroid_bounds_at_the_block_and_grid_sizes(gh, oracle, cuda):
    lo, hi = F.box("aniso")
    tris, spheres = F.pool_triangles("aniso"), F.pool_points("aniso")
    ref = oracle.morton_keys30_tri(tris, lo, hi)
    dtris, dsph = _dev(tris, cuda), _dev(spheres, cuda)
    for n in F.SIZES:
        idx = F.pool_index(n)
        di = _dev(idx, cuda)
        d = dtris[di].contiguous()
        assert np.array_equal(_keys(gh, cuda, "tris", d, lo, hi, 30, F32), ref[idx]), n
        head = idx[:min(n, F.POOL)]
        b, t = (C.c_float * 3)(), (C.c_float * 3)()
        _raw(gh, "grace_centroid_bounds_tri", gh._ptr(d), C.c_size_t(n), b, t)
        rb, rt = oracle.tri_centroid_bounds(tris[head])
        assert np.array_equal(np.array(b, F32), rb) and np.array_equal(np.array(t, F32), rt), n
        gb, gt = gh.centroid_bounds(dsph[di].contiguous())
        rb, rt = oracle.centroid_bounds(spheres[head])
        assert np.array_equal(gb, rb) and np.array_equal(gt, rt), n


@pytest.mark.parametrize("real", [F32, F64], ids=["float_bounds", "double_bounds"])
@pytest.mark.parametrize("bits", [30, 63])
@pytest.mark.parametrize("name", list(F.BOXES))
def test_keys_on_cell_boundaries_and_box_corners(gh, oracle, cuda, name, bits, real):
    """(a) the oracle's float restatement bit for bit; (b) every axis cell within 1 of
    floor(span (c - bot) / (top - bot)) evaluated exactly, and equal to it wherever the exact value is
    farther from an integer than front_end_cases.rounding_bound; in the unit box the corner `top` has
    the all-ones key."""
    lo, hi = F.box(name, real)
    edge, _ = F.boundary_points(name, bits)
    s = np.concatenate([edge, F.pool_points(name)[:400]])
    got = _keys(gh, cuda, "spheres", _dev(s, cuda), lo, hi, bits, real)
    assert np.array_equal(got, _oracle_keys(oracle, s, lo, hi, bits, real))
    for axis in range(3):
        cells, firm = F.exact_cells(s[:, axis], lo[axis], hi[axis], bits, real)
        mine = F.compact(got, axis, bits)
        assert np.abs(mine - cells).max() <= 1, axis
        assert np.array_equal(mine[firm], cells[firm]), axis
    if name == "unit":
        assert got[len(edge) - 2] == 0
        assert int(got[len(edge) - 1]) == (0x3FFFFFFF if bits == 30 else 0x7FFFFFFFFFFFFFFF)


@pytest.mark.parametrize("real", [F32, F64], ids=["float_bounds", "double_bounds"])
@pytest.mark.parametrize("bits", [30, 63])
def test_one_hot_cells_land_on_their_key_bit(gh, cuda, bits, real):
    """Bit b of axis a is key bit 3 b + a, x least significant: the convention of tests/golden/kat.json,
    pinned on the host by tests/cpp/morton_key_kat.cpp, here through the kernels."""
    s, want = F.one_hot_points(bits)
    lo, hi = F.box("unit", real)
    assert np.array_equal(_keys(gh, cuda, "spheres", _dev(s, cuda), lo, hi, bits, real), want)
    p = np.ascontiguousarray(s[:, :3].astype(F64))
    assert np.array_equal(_keys(gh, cuda, "points", _dev(p, cuda), lo, hi, bits, real), want)


@pytest.mark.parametrize("bits", [30, 63])
def test_planar_scene_gets_cell_zero_on_its_flat_axis(gh, oracle, cuda, bits):
    """All centres on one plane: the bounds-free overload finds top == bot on that axis.  Every
    primitive gets all-zero bits there, the other axes equal the restatement, two calls agree bit for
    bit, and the tree built from these keys counts the hits brute force counts."""
    s = F.planar_scene()
    lo, hi = oracle.centroid_bounds(s)
    assert lo[2] == hi[2]
    kt = torch.int32 if bits == 30 else torch.int64
    runs = []
    for _ in range(2):
        keys = _filled((len(s),), kt, cuda)
        gh.morton_keys_sph(_dev(s, cuda), keys)                       # bounds-free
        runs.append(_unsigned(keys))
    assert np.array_equal(runs[0], runs[1])
    assert np.all(F.compact(runs[0], 2, bits) == 0)
    ref = oracle.morton_keys30(s, lo, hi) if bits == 30 else oracle.morton_keys63(s, lo, hi)
    assert np.array_equal(runs[0], ref)
    for real in (F32, F64):
        got = _keys(gh, cuda, "spheres", _dev(s, cuda), lo.astype(real), hi.astype(real), bits, real)
        assert np.array_equal(got, _oracle_keys(oracle, s, lo.astype(real), hi.astype(real), bits, real))
        assert np.all(F.compact(got, 2, bits) == 0)
    pts = np.ascontiguousarray(s[:, :3].astype(F64))
    assert np.array_equal(_keys(gh, cuda, "points", _dev(pts, cuda), lo, hi, bits, F32), ref)
    # the tree from these keys, bounds from the data
    d = _dev(s, cuda)
    tree = gh.Tree(len(s), 4, device=cuda)
    if bits == 30:
        gh.build_tree(d, tree)                                         # bounds from the data
    else:
        keys = torch.empty(len(s), dtype=torch.int64, device=cuda)
        gh.morton_keys_sph(d, keys)                                    # bounds from the data
        gh.sort_by_key(keys, d, 0, 63)
        deltas = torch.empty(len(s) + 1, dtype=torch.float32, device=cuda)
        gh.euclidean_deltas_sph(d, deltas)
        gh.ALBVH_sph(d, deltas, tree)
    order = np.argsort(ref, kind="stable")
    assert np.array_equal(d.cpu().numpy(), s[order])
    mins, maxs = np.append(lo, 0).astype(F32), np.append(hi, 0.05).astype(F32)
    rays, _ = gh.orthogonal_rays_z(16, mins, maxs, device=cuda)
    rays[:, 5] = 1.0                                   # from above the plane, through it
    rays[:, 6] = 2.0
    counts = _filled((len(rays),), torch.int32, cuda)
    gh.trace_hitcounts_sph(rays, d, tree, counts)
    want = oracle.brute_hitcounts(rays.cpu().numpy(), s)
    assert want.sum() > 100 and np.array_equal(counts.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------
# 2. Deltas
# ---------------------------------------------------------------------------------------------------
DELTA_KINDS = {
    # name: (entry point, input builder, output dtype, oracle restatement)
    "euclid_f4": ("grace_deltas_euclid_f4", F.delta_base, torch.float32, lambda O, s: O.deltas_euclid(s)),
    "area_f4": ("grace_deltas_area_f4", F.delta_base, torch.float32, lambda O, s: O.deltas_area(s)),
    "euclid_d4": ("grace_deltas_euclid_d4", F.delta_base_d4, torch.float32, lambda O, s: O.deltas_euclid_d4(s)),
    "euclid_d4_f64": ("grace_deltas_euclid_d4_f64", F.delta_base_d4, torch.float64,
                      lambda O, s: O.deltas_euclid_d4_f64(s)),
    "area_d4": ("grace_deltas_area_d4", F.delta_base_d4, torch.float32, lambda O, s: O.deltas_area_d4(s)),
    "area_d4_f64": ("grace_deltas_area_d4_f64", F.delta_base_d4, torch.float64,
                    lambda O, s: O.deltas_area_d4(s, True)),
    "xor_u32": ("grace_deltas_xor_u32", lambda: F.delta_keys(U32), torch.int32, lambda O, k: O.deltas_xor(k)),
    "xor_u64": ("grace_deltas_xor_u64", lambda: F.delta_keys(U64), torch.int64, lambda O, k: O.deltas_xor(k)),
}


@pytest.mark.parametrize("kind", list(DELTA_KINDS))
def test_deltas_at_the_wave_and_block_edges(gh, oracle, cuda, kind):
    """deltas[0 .. n] bit for bit the oracle's, both sentinels included, at sizes that put the last
    element on either side of the wave's lane 63 and the block's thread 255; nothing is written past
    deltas[n].  The inputs carry coincident neighbours (delta exactly 0), subnormal results (IEEE
    value, no flush), overflowing squares, and pairs whose delta a fused multiply-add would change."""
    entry, build, out_dtype, ref_fn = DELTA_KINDS[kind]
    base = build()
    view = (lambda a: a.view(np.int32)) if base.dtype == U32 else (lambda a: a.view(np.int64)) \
        if base.dtype == U64 else (lambda a: a)
    dbase = _dev(view(base), cuda)
    fill = _bits(_filled((1,), out_dtype, cuda))[0]
    for n in F.DELTA_SIZES:
        out = _filled((n + 2,), out_dtype, cuda)
        _raw(gh, entry, gh._ptr(dbase[:n].contiguous()), C.c_size_t(n), gh._ptr(out))
        got = _bits(out)
        with np.errstate(over="ignore", invalid="ignore"):
            ref = ref_fn(oracle, base[:n])
        assert len(ref) == n + 1 and np.array_equal(got[:n + 1], _bits(ref)), n
        assert got[n + 1] == fill, n
        if kind.startswith("xor"):
            assert got[0] == got[n] == np.iinfo(got.dtype).max
        else:
            assert np.isposinf(out[0].item()) and np.isposinf(out[n].item())
        if n >= 2 and kind in ("euclid_f4", "euclid_d4", "euclid_d4_f64"):
            assert out[1].item() == 0.0


# ---------------------------------------------------------------------------------------------------
# 3. Ray generators
# ---------------------------------------------------------------------------------------------------
def _nan_rays(n, cuda):
    return _filled((n, 7), torch.float32, cuda)


def _f(v):
    return C.c_float(float(v))


def _healpix(gh, cuda, nside, origin=(0.5, 0.25, 0.125), length=3.0):
    rays = _nan_rays(12 * nside * nside, cuda)
    _raw(gh, "grace_rays_healpix", C.c_int(nside), _f(origin[0]), _f(origin[1]), _f(origin[2]), _f(length),
         gh._ptr(rays))
    return rays


@pytest.mark.parametrize("nside", F.HEALPIX_NSIDES)
def test_healpix_rays_at_every_resolution_class(gh, oracle, cuda, nside):
    """Every pixel centre within the existing tolerance (float-rounded fp64, atol 1.2e-7) of the
    reference's own pix2vec_nest where oracle/_ref is built (all pixels up to nside 64; every 61st
    pixel at 512, where the per-pixel call is too slow) and of the oracle's restatement, which the CPU
    tests tie to the reference's committed outputs.  nside 512 is three passes of the 2^20-thread grid.
    Independently: all directions distinct; the z values are the ring formula's multiset; origin and
    length on every ray."""
    rays = _healpix(gh, cuda, nside)
    r = rays.cpu().numpy()
    assert np.all(r[:, 3:6] == np.array([0.5, 0.25, 0.125], F32)) and np.all(r[:, 6] == 3.0)
    d = r[:, :3]
    ref = oracle.healpix_dirs_all(nside)
    assert np.allclose(d, ref.astype(F32), rtol=0, atol=F.HEALPIX_ATOL)
    pix = np.arange(len(d)) if nside <= 64 else np.arange(0, len(d), 61)
    own = oracle.ref_healpix_dirs(nside, pix)
    if own is not None:
        assert np.allclose(d[pix], own.astype(F32), rtol=0, atol=F.HEALPIX_ATOL)
    if nside in F.HEALPIX_FIXTURES + (4,):
        fixture = np.load(os.path.join(GOLD, "healpix_nside%d_ref.npy" % nside))
        assert np.allclose(d, fixture.astype(F32), rtol=0, atol=F.HEALPIX_ATOL)
    assert len(np.unique(F.row_hashes(d))) == len(d)
    assert np.abs(np.sort(d[:, 2].astype(F64)) - F.healpix_ring_z(nside)).max() <= F.HEALPIX_ATOL


@pytest.mark.parametrize("nside", F.HEALPIX_NSIDES)
def test_healpix_children_surround_their_parent(gh, cuda, nside):
    """Nested scheme: the normalised mean of pixels 4p .. 4p+3 at 2 nside lies within the parent
    pixel's radius of pixel p at nside (a wrong bit de-interleave or face offset scatters them)."""
    parent = _healpix(gh, cuda, nside)[:, :3].double()
    child = _healpix(gh, cuda, 2 * nside)[:, :3].double().reshape(-1, 4, 3).mean(dim=1)
    child = child / child.norm(dim=1, keepdim=True)
    parent = parent / parent.norm(dim=1, keepdim=True)
    angle = 2.0 * torch.asin(((child - parent).norm(dim=1) / 2.0).clamp(max=1.0))
    assert not torch.isnan(angle).any()
    assert float(angle.max()) < F.healpix_pixel_radius(nside)


def _scale(*parts):
    return float(sum(np.abs(np.asarray(p, F64)).max() for p in parts))


@pytest.mark.parametrize("name", list(F.ORTHO_Z_BOXES))
def test_orthogonal_rays_z_grids(gh, oracle, cuda, name):
    """Bit for bit the oracle's restatement, and within 8 roundings (centre, extent, image-plane
    co-ordinate, product, sum) of the float64 geometry relative to the box's scale; 1031^2 rays is
    more than one pass of the grid, with a prime side."""
    lo, hi = F.ORTHO_Z_BOXES[name]
    S = 2 * _scale(lo, hi)
    for n_side in F.ORTHO_Z_SIDES:
        rays = _nan_rays(n_side * n_side, cuda)
        area = C.c_float(0)
        gh._check(gh.exported_symbols().grace_rays_orthogonal_z(
            C.c_int(n_side), _vec(lo), _vec(hi), gh._ptr(rays), C.byref(area), gh._stream()))
        ref, ref_area = oracle.orthogonal_rays_z(n_side, lo, hi)
        assert np.array_equal(_bits(rays), ref.view(U32).reshape(-1, 7)), n_side
        assert area.value == ref_area
        o, length, a64 = F.orthogonal_z_f64(n_side, lo, hi)
        r = rays.cpu().numpy().astype(F64)
        assert np.abs(r[:, 3:6] - o).max() <= 8 * F.U * S, n_side
        assert np.all(r[:, :3] == [0, 0, -1]) and np.abs(r[:, 6] - length).max() <= 4 * F.U * S
        assert abs(area.value - a64) <= 8 * F.U * a64


@pytest.mark.parametrize("cam", list(F.CAMERAS))
def test_orthographic_projection_grids(gh, oracle, cuda, cam):
    """Bit for bit the oracle's restatement, and within front_end_cases.GRID_TOL_ROUNDINGS float
    roundings of the float64 geometry relative to the scene scale, for oblique cameras at scale 1e5
    and 1e-3; 1031 x 1033 is more than one pass of the grid, prime in both dimensions."""
    c, look, up, extent = F.camera(cam)
    tol = F.GRID_TOL_ROUNDINGS * F.U
    for rx, ry in F.GRID_RES:
        rays = _nan_rays(rx * ry, cuda)
        _raw(gh, "grace_rays_orthographic_projection", C.c_int(rx), C.c_int(ry), _vec(c), _vec(look), _vec(up),
             _f(extent), _f(2 * extent), gh._ptr(rays))
        ref = oracle.orthographic_projection_rays(rx, ry, c, look, up, extent, 2 * extent)
        assert np.array_equal(_bits(rays), ref.view(U32).reshape(-1, 7)), (rx, ry)
        d, o = F.orthographic_f64(rx, ry, c, look, up, extent)
        r = rays.cpu().numpy().astype(F64)
        S = _scale(c) + extent * max(rx / ry, 1.0)
        assert np.abs(r[:, :3] - d).max() <= tol and np.abs(r[:, 3:6] - o).max() <= tol * S, (rx, ry)
        assert np.all(r[:, 6] == F32(2 * extent))


@pytest.mark.parametrize("cam", list(F.CAMERAS))
def test_pinhole_camera_grids(gh, oracle, cuda, cam):
    """As for the orthographic grids: the oracle bit for bit, the float64 directions within the derived
    tolerance (times the aspect ratio, which scales the unnormalised direction)."""
    c, look, up, extent = F.camera(cam)
    tol = F.GRID_TOL_ROUNDINGS * F.U
    for rx, ry in F.GRID_RES:
        rays = _nan_rays(rx * ry, cuda)
        _raw(gh, "grace_rays_pinhole", C.c_int(rx), C.c_int(ry), _vec(c), _vec(look), _vec(up), _f(0.9),
             _f(2 * extent), gh._ptr(rays))
        ref = oracle.pinhole_rays(rx, ry, c, look, up, 0.9, 2 * extent)
        assert np.array_equal(_bits(rays), ref.view(U32).reshape(-1, 7)), (rx, ry)
        r = rays.cpu().numpy().astype(F64)
        g = F.pinhole_f64(rx, ry, c, look, up, 0.9)
        assert np.abs(r[:, :3] - g).max() <= tol * max(rx / ry, 1.0), (rx, ry)
        assert np.all(r[:, 3:6] == c.astype(F64)) and np.all(r[:, 6] == F32(2 * extent))


def test_pinhole_refuses_a_ray_count_that_wraps(gh, cuda):
    """65536 x 32768 = 2^31 rays: invalid argument, like orthogonal_rays_z and
    plane_parallel_random_rays, and the buffer is untouched.  (Without the guard the kernel's int
    product wraps negative, nothing is written and the call reports success.)"""
    rays = _nan_rays(1, cuda)
    status = gh.exported_symbols().grace_rays_pinhole(
        C.c_int(65536), C.c_int(32768), _vec((0, 0, 0)), _vec((0, 0, -1)), _vec((0, 1, 0)), _f(0.9), _f(1.0),
        gh._ptr(rays), gh._stream())
    torch.cuda.synchronize()
    assert np.all(_bits(rays) == F.NAN_BITS)
    assert status == gh.GRACE_INVALID_ARGUMENT


def _isotropic(gh, cuda, n, seed, octant, origin=(1.0, 2.0, 3.0), length=5.0):
    rays = _nan_rays(n, cuda)
    head = (C.c_size_t(n), _f(origin[0]), _f(origin[1]), _f(origin[2]), _f(length))
    if octant < 0:
        _raw(gh, "grace_rays_isotropic", *head, C.c_uint64(seed), gh._ptr(rays))
    else:
        _raw(gh, "grace_rays_isotropic_octant", *head, C.c_int(octant), C.c_uint64(seed), gh._ptr(rays))
    return rays.cpu().numpy()


@pytest.mark.parametrize("octant", (-1,) + F.ISO_OCTANTS)
def test_isotropic_rays_are_the_restated_map_as_a_set(gh, cuda, octant):
    """4096 rays per seed: every output ray has exactly one direction of the float64 restatement of
    (seed, index) -> direction within T (componentwise), and the matches form a permutation.
    T = 4 x the largest deviation of the float32 NumPy chain from the float64 one for that seed:
    measured on the CPU 1.2e-6, 1.2e-6, 1.1e-6, 2.5e-6 for seeds 1234, 11, 9, 0, so T = 4.8e-6, 4.8e-6,
    4.2e-6, 1.0e-5, each under a tenth of the seed's smallest separation (2.6e-4 rad for seed 1234 on
    the whole sphere, 7.4e-5 rad for seed 9 in an octant).
    Observed on an MI355X: 1.17e-6, 1.19e-6, 1.05e-6, 2.53e-6 for those seeds, the same for the
    whole sphere and every octant -- the device's chain lands where NumPy's float32 chain does."""
    from scipy.spatial import cKDTree
    for seed in F.ISO_SEEDS:
        T, _ = F.isotropic_tolerance(seed, octant)
        r = _isotropic(gh, cuda, F.ISO_N, seed, octant)
        assert np.all(r[:, 3:6] == np.array([1, 2, 3], F32)) and np.all(r[:, 6] == 5.0)
        dist, idx = cKDTree(F.isotropic_dirs(seed, F.ISO_N, octant)).query(r[:, :3].astype(F64), k=2, p=np.inf)
        print("isotropic octant %d seed %d: max deviation %.3e (T %.3e)" % (octant, seed, dist[:, 0].max(), T))
        assert np.all(dist[:, 0] <= T), (seed, dist[:, 0].max(), T)
        assert np.all(dist[:, 1] > T), seed
        assert np.array_equal(np.sort(idx[:, 0]), np.arange(F.ISO_N)), seed


@pytest.mark.parametrize("octant", [-1, 5])
def test_isotropic_payload_sort_keeps_every_ray(gh, oracle, cuda, octant):
    """At each size, across the nested sort's switch to the bucket sort at 2^18 and past one grid pass:
    unit norms, non-decreasing direction keys, no duplicated row, and -- ray t depending on (seed, t)
    alone -- the rows of one size a subset of the rows of the next.  A sort that dropped, duplicated or
    tore a 28-byte record breaks one of them."""
    previous = None
    for n in F.ISO_SIZES:
        r = _isotropic(gh, cuda, n, 1234, octant)
        assert np.abs(np.linalg.norm(r[:, :3].astype(F64), axis=1) - 1).max() <= 3e-7, n
        assert np.all(r[:, 3:6] == np.array([1, 2, 3], F32)) and np.all(r[:, 6] == 5.0), n
        keys = oracle.ray_dir_keys_all(r)
        assert np.all(keys[1:] >= keys[:-1]), n
        h = F.row_hashes(r)
        assert len(np.unique(h)) == n, n
        if previous is not None:
            assert np.isin(previous, h).all(), n
        previous = h


@pytest.mark.parametrize("dtype,cols", F.OTM_LAYOUTS, ids=lambda v: getattr(v, "__name__", str(v)))
def test_one_to_many_rays_at_the_block_and_grid_sizes(gh, oracle, cuda, dtype, cols):
    """Unsorted: the oracle bit for bit (double points near the origin included: the difference is
    formed before narrowing).  Sorted by direction / by end point: a stable sort of the unsorted rays
    by the restated keys, with end points tied on their Morton key."""
    pool = F.otm_pool(dtype, cols)
    dpool = _dev(pool, cuda)
    lo, hi = F.OTM_BOX
    ref_pool = oracle.one_to_many_rays(F.OTM_ORIGIN, pool).view(F32).reshape(-1, 7)
    dir_keys = oracle.ray_dir_keys_all(ref_pool)
    end_keys = oracle.morton_keys_points(pool, lo, hi, 30)
    head = [_f(v) for v in F.OTM_ORIGIN]
    for n in F.OTM_SIZES:
        idx = F.pool_index(n)
        d = dpool[_dev(idx, cuda)].contiguous()
        ref = ref_pool[idx]
        for sort_type, keys in ((gh.NoSort, None), (gh.DirectionSort, dir_keys), (gh.EndPointSort, end_keys)):
            rays = _nan_rays(n, cuda)
            _raw(gh, "grace_rays_one_to_many", C.c_size_t(n), *head, gh._ptr(d), C.c_int(int(dtype == F64)),
                 C.c_int(cols), C.c_int(sort_type), _vec(lo), _vec(hi), gh._ptr(rays))
            want = ref if keys is None else ref[np.argsort(keys[idx], kind="stable")]
            assert np.array_equal(_bits(rays), want.view(U32)), (n, sort_type)


def test_plane_parallel_random_rays_are_the_restated_map(gh, cuda):
    """Each origin is base + (i + rw) w / W + (j + rh) h / H in float64, rw and rh from the same
    splitmix64 stream, within front_end_cases.PLANE_TOL_ROUNDINGS float roundings of the plane's
    scale (a cell is hundreds of times wider); the direction is normalize(cross(w, h)) to 1 ulp."""
    base, w, h = F.PLANE["base"], F.PLANE["w"], F.PLANE["h"]
    S = _scale(base) + _scale(w) + _scale(h)
    tol = F.PLANE_TOL_ROUNDINGS * F.U * S
    for W, H in F.PLANE_RES:
        assert min(_scale(w) / W, _scale(h) / H) > 50 * tol
        rays = _nan_rays(W * H, cuda)
        _raw(gh, "grace_rays_plane_parallel_random", C.c_int(W), C.c_int(H), _vec(base), _vec(w), _vec(h),
             _f(7.5), C.c_uint64(3), gh._ptr(rays))
        r = rays.cpu().numpy()
        o, d = F.plane_parallel_f64(W, H, base, w, h, 3)
        assert np.abs(r[:, 3:6].astype(F64) - o).max() <= tol, (W, H)
        assert np.all(np.abs(r[:, :3].astype(F64) - d) <= np.spacing(np.abs(d).astype(F32)).astype(F64)), (W, H)
        assert np.all(r[:, :3] == r[0, :3]) and np.all(r[:, 6] == 7.5)
