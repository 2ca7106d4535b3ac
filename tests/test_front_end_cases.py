"""CPU checks of tests/front_end_cases.py: every builder hits what it claims, the restatements agree
with the C oracle and with each other, and the caps the GPU tests rely on hold for the inputs chosen
(boundary points straddle their cell, the FMA-sensitive set is sensitive, the isotropic tolerance sits
below the separation cap, the HEALPix restatement equals the reference's fixtures)."""
import json
import os
from fractions import Fraction

import numpy as np
import pytest

import front_end_cases as F

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _oracle_keys(oracle, s, lo, hi, bits, real):
    if bits == 30:
        return oracle.morton_keys30(s, lo, hi) if real == F32 else oracle.morton_keys30_d3(s, lo, hi)
    return oracle.morton_keys63(s, lo, hi, double_bounds=(real == F64))


def _check_against_exact(keys, coords, lo, hi, bits, real):
    """Reference (b): every axis cell within 1 of the exact floor, equal wherever the exact scaled
    value is farther from an integer than the rounding bound.  Returns the share of firm cells."""
    firm_all = []
    for axis in range(3):
        cells, firm = F.exact_cells(coords[:, axis], lo[axis], hi[axis], bits, real)
        got = F.compact(keys, axis, bits)
        assert np.abs(got - cells).max() <= 1, (axis, np.abs(got - cells).max())
        assert np.array_equal(got[firm], cells[firm]), axis
        firm_all.append(firm)
    return np.mean(firm_all)


# ---- Morton keys ----------------------------------------------------------------------------------
def test_kat_convention_puts_x_on_the_least_significant_bit():
    kat = json.load(open(os.path.join(GOLD, "kat.json")))
    for name, bits in (("morton30", 30), ("morton63", 63)):
        k = kat[name]
        assert k["key"] == k["spaced_x"] | k["spaced_y"] << 1 | k["spaced_z"] << 2
        key = np.array([k["key"]], U64)
        assert [int(F.compact(key, a, bits)[0]) for a in range(3)] == [k["x"], k["y"], k["z"]]
        assert k["spaced_x"] == sum(((k["x"] >> b) & 1) << (3 * b) for b in range(21))


@pytest.mark.parametrize("bits", [30, 63])
def test_one_hot_points_sit_half_a_cell_inside_their_cell(oracle, bits):
    s, keys = F.one_hot_points(bits)
    lo, hi = F.box("unit")
    nb = 10 if bits == 30 else 21
    for a in range(3):
        for b in range(nb):
            v = F.scaled_exact(s[a * nb + b, a], 0.0, 1.0, F.SPAN[bits])
            assert abs(v - (1 << b) - Fraction(1, 2)) < Fraction(1, 4)
    for real in (F32, F64):
        assert np.array_equal(_oracle_keys(oracle, s, lo, hi, bits, real), keys)
    assert len(set(keys.tolist())) == 3 * nb and all(bin(int(k)).count("1") == 1 for k in keys)


@pytest.mark.parametrize("bits", [30, 63])
@pytest.mark.parametrize("name", list(F.BOXES))
def test_boundary_points_straddle_their_cell_and_the_oracle_meets_the_exact_cells(oracle, name, bits):
    s, meta = F.boundary_points(name, bits)
    lo, hi = F.box(name)
    span = F.SPAN[bits]
    seen = set()
    for p, (axis, k, label) in zip(s, meta):
        if axis < 0:
            assert np.array_equal(p[:3], lo if label == "bot" else hi)
            continue
        assert lo[axis] <= p[axis] <= hi[axis]
        v = F.scaled_exact(p[axis], lo[axis], hi[axis], span)
        assert (v < k) if label == "below" else (v >= k) if label == "at" else (v > k)
        if label == "at":
            below = F.scaled_exact(np.nextafter(p[axis], F32(-np.inf)), lo[axis], hi[axis], span)
            assert below < k
        seen.add((axis, k, label))
    for axis in range(3):
        for k in F.CELL_KS[bits]:
            assert (axis, k, "at") in seen
            assert ((axis, k, "below") in seen) == (k > 0)
            # (a float32 step can exceed a 63-bit cell: near the top corner "above" may leave the box)
            assert ((axis, k, "above") in seen) == (k < span) or (bits == 63 and k == span - 1)
    for real in (F32, F64):
        blo, bhi = F.box(name, real)
        keys = _oracle_keys(oracle, s, blo, bhi, bits, real)
        _check_against_exact(keys, s[:, :3], blo, bhi, bits, real)
        if name == "unit":
            assert keys[-2] == 0 and int(keys[-1]) == (1 << bits) - 1


@pytest.mark.parametrize("name", list(F.BOXES))
def test_pool_points_are_inside_their_box_and_rarely_near_a_cell_edge(oracle, name):
    p = F.pool_points(name)
    lo, hi = F.box(name)
    assert np.all(p[:, :3] >= lo) and np.all(p[:, :3] <= hi)
    share = _check_against_exact(oracle.morton_keys30(p, lo, hi), p[:, :3], lo, hi, 30, F32)
    assert 1.0 - share < 0.01, share
    d = F.pool_points(name, cols=7, dtype=F64)
    c = d[:, :3].astype(F32)
    assert np.all(c >= lo) and np.all(c <= hi) and np.all(d[:, 3:] > 1e5)
    idx = F.pool_index(F.GRID + 257)
    assert np.any(p[idx[:257]] != p[idx[F.GRID:]])          # a second pass reads other records


def test_oracle_point_keys_are_the_sphere_keys_of_the_narrowed_points(oracle):
    for name in F.BOXES:
        lo, hi = F.box(name)
        for dtype, cols in F.POINT_LAYOUTS:
            p = F.pool_points(name, cols=cols, dtype=dtype)
            s = np.zeros((len(p), 4), F32); s[:, :3] = p[:, :3].astype(F32)
            for bits in (30, 63):
                for real in (F32, F64):
                    blo, bhi = F.box(name, real)
                    assert np.array_equal(oracle.morton_keys_points(p, blo, bhi, bits, real == F64),
                                          _oracle_keys(oracle, s, blo, bhi, bits, real))
            b, t = oracle.centroid_bounds_points(p)
            assert np.array_equal(b, s[:, :3].min(0)) and np.array_equal(t, s[:, :3].max(0))


def test_pool_triangles_have_their_centroids_inside_the_box(oracle):
    for name in F.BOXES:
        lo, hi = F.box(name)
        b, t = oracle.tri_centroid_bounds(F.pool_triangles(name))
        assert np.all(b >= lo) and np.all(t <= hi) and np.all(t > b)


def test_degenerate_axis_has_scale_zero_in_the_oracle(oracle):
    s = F.planar_scene()
    lo, hi = oracle.centroid_bounds(s)
    assert lo[2] == hi[2] and lo[0] < hi[0] and lo[1] < hi[1]
    flat = s.copy(); flat[:, 2] = 0.0
    for bits in (30, 63):
        for real in (F32, F64):
            keys = _oracle_keys(oracle, s, lo.astype(real), hi.astype(real), bits, real)
            assert np.all(F.compact(keys, 2, bits) == 0)
            # x and y: the keys of the same scene in a box that does extend along z
            ref = _oracle_keys(oracle, flat, np.array([lo[0], lo[1], 0], real),
                               np.array([hi[0], hi[1], 1], real), bits, real)
            assert np.array_equal(keys, ref)
    assert np.array_equal(oracle.morton_keys_points(s, lo, hi, 30), oracle.morton_keys30(s, lo, hi))


# ---- deltas ---------------------------------------------------------------------------------------
def test_fma_sensitive_pairs_are_sensitive():
    p = F.fma_sensitive_pairs()
    a, b = p[0::2], p[1::2]
    half = len(a) // 2
    assert np.all(F.euclid_chain(a[:half], b[:half], False) != F.euclid_chain(a[:half], b[:half], True))
    assert np.all(F.area_chain(a[half:], b[half:], False) != F.area_chain(a[half:], b[half:], True))


def test_plain_delta_chains_are_the_oracle_and_the_specials_hold_their_values(oracle):
    s = F.delta_base()
    n0 = len(F.delta_specials())
    e, a = oracle.deltas_euclid(s), oracle.deltas_area(s)
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.array_equal(e[1:-1].view(U32), F.euclid_chain(s[:-1], s[1:], False).view(U32))
        assert np.array_equal(a[1:-1].view(U32), F.area_chain(s[:-1], s[1:], False).view(U32))
    tiny = np.finfo(F32).tiny
    assert e[1] == 0.0                                     # coincident
    assert 0 < e[3] < tiny and 0 < a[3] < tiny             # subnormal, not flushed
    assert np.isposinf(e[5]) and np.isposinf(a[5])         # squares overflow
    # the FMA-sensitive pairs are where delta_specials put them
    with np.errstate(over="ignore", invalid="ignore"):
        fe = F.euclid_chain(s[:-1], s[1:], True)[:n0]
        fa = F.area_chain(s[:-1], s[1:], True)[:n0]
    assert np.any(fe[6:] != e[7:n0 + 1][:len(fe) - 6]) and np.any(fa[6:] != a[7:n0 + 1][:len(fa) - 6])


def test_delta_inputs_are_distinct_at_the_wave_and_block_edges(oracle):
    s, d = F.delta_base(), F.delta_base_d4()
    for arr in (s, d):
        rows = arr[list(F.EDGES) + [e + 1 for e in F.EDGES]]
        assert len(np.unique(rows, axis=0)) == len(np.unique(np.array(list(F.EDGES) + [e + 1 for e in F.EDGES])))
    for deltas in (oracle.deltas_euclid(s), oracle.deltas_area(s), oracle.deltas_euclid_d4(d),
                   oracle.deltas_area_d4(d)):
        at = deltas[[e + 1 for e in F.EDGES] + [e for e in F.EDGES]]
        assert len(np.unique(at)) == len(np.unique(np.array([e + 1 for e in F.EDGES] + list(F.EDGES))))
    # double inputs whose float narrowing loses what the differences need
    assert not np.array_equal(oracle.deltas_euclid_d4(d)[1:-1], oracle.deltas_euclid(d.astype(F32))[1:-1])
    for dt in (U32, U64):
        k = F.delta_keys(dt)
        x = oracle.deltas_xor(k)
        assert x[1] == 0 and len(np.unique(x[[62, 63, 64, 65, 255, 256, 257, 258]])) == 8


def test_double_output_deltas_are_the_float_values_widened(oracle):
    d = F.delta_base_d4()[:300]
    assert np.array_equal(oracle.deltas_euclid_d4_f64(d), oracle.deltas_euclid_d4(d).astype(F64))
    assert np.array_equal(oracle.deltas_area_d4(d, True), oracle.deltas_area_d4(d).astype(F64))
    # area of double4 spheres that are float4 spheres widened: the float4 delta
    s = F.delta_base()[:300]
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.array_equal(oracle.deltas_area_d4(s.astype(F64)).view(U32), oracle.deltas_area(s).view(U32))


# ---- HEALPix --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nside", F.HEALPIX_FIXTURES + (4,))
def test_healpix_restatement_equals_the_references_fixtures(oracle, nside):
    ref = np.load(os.path.join(GOLD, "healpix_nside%d_ref.npy" % nside))
    got = oracle.healpix_dirs_all(nside)
    assert ref.shape == got.shape == (12 * nside * nside, 3)
    assert np.abs(got - ref).max() <= 4 * np.finfo(F64).eps
    if nside <= 4:
        assert np.array_equal(got, oracle.healpix_dirs(nside))


@pytest.mark.parametrize("nside", F.HEALPIX_NSIDES)
def test_healpix_restatement_has_the_ring_structure_and_nested_children(oracle, nside):
    d = oracle.healpix_dirs_all(nside)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-15
    assert len(np.unique(F.row_hashes(d.astype(F32)))) == len(d)    # distinct even as float32
    z = F.healpix_ring_z(nside)
    assert np.abs(np.sort(d[:, 2]) - z).max() < 1e-15
    gaps = np.diff(np.unique(z))
    assert len(gaps) == 4 * nside - 2 and gaps.min() > 10 * F.HEALPIX_ATOL   # rings stay apart under the tolerance
    ang = F.children_mean_angle(d, oracle.healpix_dirs_all(2 * nside))
    assert ang.max() < F.healpix_pixel_radius(nside), (ang.max(), F.healpix_pixel_radius(nside))
    r = oracle.ref_healpix_dirs(nside, range(0, len(d), 61))
    if r is not None:
        assert np.abs(d[::61] - r).max() <= 4 * np.finfo(F64).eps


# ---- grids ----------------------------------------------------------------------------------------
def _scale(*parts):
    return float(sum(np.abs(np.asarray(p, F64)).max() for p in parts))


@pytest.mark.parametrize("cam", list(F.CAMERAS))
@pytest.mark.parametrize("res", [(1, 1), (1, 257), (257, 1), (255, 3)])
def test_grid_oracles_meet_the_float64_geometry(oracle, cam, res):
    c, look, up, extent = F.camera(cam)
    vd = (look - c).astype(F64)
    cos = abs(vd @ up) / np.linalg.norm(vd) / np.linalg.norm(up.astype(F64))
    assert cos < np.cos(np.pi / 4)                          # view_up at least 45 degrees off the view
    tol = F.GRID_TOL_ROUNDINGS * F.U
    r = oracle.orthographic_projection_rays(res[0], res[1], c, look, up, extent, 2 * extent)
    r = r.view(F32).reshape(-1, 7).astype(F64)
    d, o = F.orthographic_f64(res[0], res[1], c, look, up, extent)
    S = _scale(c) + extent * max(res[0] / res[1], 1.0)
    assert np.abs(r[:, :3] - d).max() <= tol and np.abs(r[:, 3:6] - o).max() <= tol * S
    p = oracle.pinhole_rays(res[0], res[1], c, look, up, 0.9, 2 * extent).view(F32).reshape(-1, 7).astype(F64)
    g = F.pinhole_f64(res[0], res[1], c, look, up, 0.9)
    assert np.abs(p[:, :3] - g).max() <= tol * max(res[0] / res[1], 1.0)
    assert np.all(p[:, 3:6] == c.astype(F64))


@pytest.mark.parametrize("name", list(F.ORTHO_Z_BOXES))
def test_orthogonal_z_oracle_meets_the_float64_geometry(oracle, name):
    lo, hi = F.ORTHO_Z_BOXES[name]
    for n_side in (1, 3, 255):
        r, area = oracle.orthogonal_rays_z(n_side, lo, hi)
        r = r.view(F32).reshape(-1, 7).astype(F64)
        o, length, a64 = F.orthogonal_z_f64(n_side, lo, hi)
        S = _scale(lo, hi) * 2
        assert np.abs(r[:, 3:6] - o).max() <= 8 * F.U * S and np.all(r[:, :3] == [0, 0, -1])
        assert abs(r[0, 6] - length) <= 4 * F.U * S and abs(area - a64) <= 8 * F.U * a64


# ---- random generators ----------------------------------------------------------------------------
def test_splitmix64_known_answers():
    # the published splitmix64 sequence from state 0: successive outputs are splitmix64(k * gamma)
    gamma = 0x9E3779B97F4A7C15
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = F.splitmix64(np.array([(k * gamma) % 2 ** 64 for k in range(3)], U64))
    assert [int(g) for g in got] == want
    assert F.u01(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], U64)).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]


@pytest.mark.parametrize("octant", (-1,) + F.ISO_OCTANTS)
def test_isotropic_tolerance_sits_below_the_separation_cap(octant):
    from scipy.spatial import cKDTree
    for seed in F.ISO_SEEDS:
        T, dev = F.isotropic_tolerance(seed, octant)
        assert 0 < dev < 1e-5
        d = F.isotropic_dirs(seed, F.ISO_N, octant)
        assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-15
        if octant >= 0:
            sign = np.array([1 if octant & 4 else -1, 1 if octant & 2 else -1, 1 if octant & 1 else -1])
            assert np.all(d * sign > 0)
        sep = cKDTree(d).query(d, k=2)[0][:, 1].min()       # chord = angle at this size, rad
        # 2.6e-4 rad for seed 1234 on the whole sphere; 7.4e-5 rad for seed 9 folded into an octant
        assert T < sep / 10, (octant, seed, T, sep)
    # ray t depends on (seed, t) only
    assert np.array_equal(F.isotropic_dirs(9, 300, octant)[:255], F.isotropic_dirs(9, 255, octant))


def test_row_hashes_tell_rows_apart():
    r = np.zeros((5, 7), F32)
    r[1, 0] = 1; r[2, 6] = 1; r[3] = r[1]; r[4, 0] = -0.0
    h = F.row_hashes(r)
    assert h[1] == h[3] and len(set(h.tolist())) == 4


def test_plane_restatement_and_its_exact_cross_product():
    w, h = np.asarray(F.PLANE["w"], F32), np.asarray(F.PLANE["h"], F32)
    c32 = np.array([w[1] * h[2] - w[2] * h[1], w[2] * h[0] - w[0] * h[2], w[0] * h[1] - w[1] * h[0]], F32)
    assert np.array_equal(c32.astype(F64), np.cross(w.astype(F64), h.astype(F64)))
    assert np.all(c32 != 0)                                 # oblique to every axis
    o, d = F.plane_parallel_f64(7, 5, F.PLANE["base"], w, h, 3)
    t = np.arange(35)
    B = np.linalg.lstsq(np.stack([w, h], 1).astype(F64), (o - np.asarray(F.PLANE["base"])).T, rcond=None)[0].T
    assert np.all((B[:, 0] * 7 > t % 7 - 1e-9) & (B[:, 0] * 7 <= t % 7 + 1 + 1e-9))
    assert np.all((B[:, 1] * 5 > t // 7 - 1e-9) & (B[:, 1] * 5 <= t // 7 + 1 + 1e-9))
    assert abs(np.linalg.norm(d) - 1) < 1e-15


def test_one_to_many_pools_hold_their_near_origin_and_tied_points(oracle):
    lo, hi = F.OTM_BOX
    for dtype, cols in F.OTM_LAYOUTS:
        p = F.otm_pool(dtype, cols)
        assert p.dtype == dtype and p.shape == (F.POOL, cols)
        keys = oracle.morton_keys_points(p, lo, hi, 30)
        groups = keys[64:128].reshape(8, 8)
        assert np.all(groups == groups[:, :1]) and len(np.unique(groups[:, 0])) == 8
        rays = oracle.one_to_many_rays(F.OTM_ORIGIN, p).view(F32).reshape(-1, 7)
        assert np.all(np.isfinite(rays))
        if dtype == F64:
            narrowed = oracle.one_to_many_rays(F.OTM_ORIGIN, p.astype(F32).astype(F64)).view(F32).reshape(-1, 7)
            assert np.abs(rays[:64, :3] - narrowed[:64, :3]).max() > 0.05
            assert np.array_equal(rays[128:], narrowed[128:]) or np.abs(rays[128:, :3] - narrowed[128:, :3]).max() < 1e-6
            assert len(np.unique(rays[:64, :3], axis=0)) == 64


def test_vectorised_oracle_entries_equal_the_per_item_ones(oracle):
    rng = np.random.default_rng(1)
    r = np.zeros((500, 7), F32)
    d = rng.standard_normal((500, 3)); r[:, :3] = d / np.linalg.norm(d, axis=1)[:, None]
    assert np.array_equal(oracle.ray_dir_keys_all(r), oracle.ray_dir_keys(r))
