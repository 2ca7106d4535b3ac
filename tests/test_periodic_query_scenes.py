"""CPU checks for the periodic point queries: the exported symbols, the front ends that compile, the
Gadget header, and the restatement of periodic_query_scenes.py itself -- that it is antisymmetric, that
it is the open queries' restatements where nothing wraps, and that it gives the counts a torus must
give on the scenes the GPU tests of test_periodic_queries.py use."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import periodic_query_scenes as S
from test_fof import restate_labels as open_labels
from test_pair_counts import restate as open_bins
from test_range_queries import HIPCC_FLAGS, LIBDIR, ROOT, restate as open_restate

F32 = np.float32
SYMBOLS = ("grace_range_counts_periodic_f4", "grace_range_neighbours_periodic_f4", "grace_fof_labels_periodic_f4",
           "grace_pair_counts_periodic_f4")


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_periodic_symbols_exported():
    lib = C.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def compile_dropin(exe):
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS, os.path.join(ROOT, "tests", "cpp", "dropin_periodic.hip"),
                           "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


def test_periodic_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_periodic"
    compile_dropin(exe)
    assert exe.exists()


def test_periodic_mirror_compiles(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::float4>& p, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::device_vector<float>& r, const grace::device_vector<float>& w,\n"
                   "       const grace::Tree& t)\n"
                   "{\n"
                   "    const grace::PeriodicBox box = { 1.0f, 0.5f, 0.0f };\n"
                   "    grace::device_vector<int> cnt(p.size()), off, idx, labels, shells;\n"
                   "    grace::device_vector<float> sums(p.size() * 2), d2, shell_sums;\n"
                   "    grace::device_vector<unsigned long long> totals;\n"
                   "    const std::vector<float> edges(3, 0.1f);\n"
                   "    grace::range_counts_sph(p, r, s, t, cnt, box);\n"
                   "    grace::range_counts_sph(p, 0.25f, s, t, cnt, box);\n"
                   "    grace::range_counts_sph(p, r, s, t, w, 2, cnt, sums, box);\n"
                   "    grace::range_counts_sph(p, 0.25f, s, t, w, 2, cnt, sums, box);\n"
                   "    grace::range_neighbours_sph(p, r, s, t, off, idx, d2, box);\n"
                   "    grace::range_neighbours_sph(p, 0.25f, s, t, off, idx, d2, box);\n"
                   "    grace::fof_labels_sph(s, t, 0.01f, labels, box);\n"
                   "    grace::pair_counts_sph(p, edges, s, t, totals, box);\n"
                   "    grace::radial_profiles_sph(p, edges, s, t, shells, box);\n"
                   "    grace::radial_profiles_sph(p, edges, s, t, shells, w, 2, shell_sums, box);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


# ---- Gadget header --------------------------------------------------------------------------------
def test_gadget_header_round_trips_the_box_size(tmp_path):
    from grace_hip import gadget
    rng = np.random.default_rng(1)
    pos, hsml = rng.random((50, 3), dtype=F32), rng.random(50, dtype=F32)
    f = str(tmp_path / "box.gad")
    gadget.write_gadget(f, pos, hsml, box_size=25000.0)
    hdr = gadget.read_gadget_header(f)
    assert hdr["box_size"] == 25000.0 and hdr["npart"] == [50, 0, 0, 0, 0, 0] and hdr["mass"][0] == 1.0
    assert hdr["time"] == 0.0 and hdr["redshift"] == 0.0
    raw = open(f, "rb").read()
    assert np.frombuffer(raw[4 + 128:4 + 136], np.float64)[0] == 25000.0      # the float64 at byte 128 of the header
    assert np.array_equal(gadget.read_gadget(f)[:, :3], pos)                  # the blocks behind it are where they were
    # a header written by other means: time, redshift and box size where Gadget-2 puts them
    hdr_bytes = bytearray(raw[4:260])
    hdr_bytes[72:88] = np.array([0.25, 3.0], np.float64).tobytes()
    with open(f, "wb") as out:
        out.write(raw[:4] + bytes(hdr_bytes) + raw[260:])
    hdr = gadget.read_gadget_header(f)
    assert (hdr["time"], hdr["redshift"], hdr["box_size"]) == (0.25, 3.0, 25000.0)


@pytest.mark.parametrize("masses_in_header", [True, False])
def test_write_gadget_default_bytes_are_unchanged(tmp_path, masses_in_header):
    """The file as write_gadget wrote it before box_size existed, assembled here block by block."""
    from grace_hip import gadget
    rng = np.random.default_rng(2)
    n = 37
    pos, hsml = rng.random((n, 3), dtype=F32), rng.random(n, dtype=F32)
    vel, u = rng.random((n, 3), dtype=F32), rng.random(n, dtype=F32)
    f = str(tmp_path / "plain.gad")
    gadget.write_gadget(f, pos, hsml, masses_in_header=masses_in_header, vel=vel, u=u)

    def block(payload):
        nbytes = np.array([len(payload)], np.int32).tobytes()
        return nbytes + payload + nbytes
    header = np.array([n, 0, 0, 0, 0, 0], np.int32).tobytes() \
        + np.array([1.0 if masses_in_header else 0.0, 0, 0, 0, 0, 0], np.float64).tobytes()
    blocks = [header + bytes(256 - len(header)), pos.tobytes(), vel.tobytes(), np.arange(n, dtype=np.int32).tobytes()]
    if not masses_in_header:
        blocks.append(np.ones(n, F32).tobytes())
    blocks += [u.tobytes(), np.ones(n, F32).tobytes(), hsml.tobytes()]
    assert open(f, "rb").read() == b"".join(block(b) for b in blocks)
    assert gadget.read_gadget_header(f)["box_size"] == 0.0


# ---- the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", S.OFFSETS)
@pytest.mark.parametrize("box", list(S.BOXES))
def test_restated_separation_is_antisymmetric(box, offset):
    """d(p, x) == -d(x, p) bit for bit per component, so d2 is symmetric: uniform points, points within ulps
    of the faces, and pairs at exactly half a period."""
    period = S.BOXES[box]
    x = np.concatenate([S.uniform(400, box, offset, 3)[:, :3], S.seam(offset)[0][:400, :3]])
    halfway = x[:50].copy()
    halfway[:, 0] += S.half(period[0])                              # (rounded: at and next to half a period)
    x = np.concatenate([x, halfway]).astype(F32)
    for a, L in enumerate(period):
        d = S.wrap((x[:, None, a] - x[None, :, a]).astype(F32), L)
        assert np.array_equal(d, -d.T)
        if L > 0:                                                    # points inside one period: one wrap brings them in
            assert np.all(np.abs(d[:400, :400]) <= S.half(L))
    d2 = S.d2_rows(x, x, period)
    assert _same(d2, d2.T)


def test_wrap_edges():
    d = np.array([0.5, np.nextafter(F32(0.5), F32(1)), -0.5, np.nextafter(F32(-0.5), F32(-1)), 1.0, -1.0, 1.75, -1.75,
                  np.nan, 0.0], F32)
    got = S.wrap(d, 1.0)
    # exactly half a period stays; beyond it one wrap, and only one
    assert got[0] == 0.5 and got[2] == -0.5 and got[1] < 0 and got[3] > 0
    assert got[4:8].tolist() == [0.0, 0.0, 0.75, -0.75] and np.isnan(got[8]) and got[9] == 0.0
    assert np.array_equal(S.wrap(d, 0.0), d, equal_nan=True)


@pytest.mark.parametrize("offset", S.OFFSETS)
def test_restated_lattice_counts(offset):
    """Every site of the full lattice is every other's translate: 7 within 1/16, 33 within 2/16, 7 within
    fl(sqrt(2)/16) (whose square rounds below 2/256); without the period the faces, edges and corners miss
    theirs."""
    s = S.lattice(offset)
    for r, n_torus, open_min in zip(S.LATTICE_RADII, S.LATTICE_COUNTS, (4, 11, 4)):
        counts, offsets, idx, d2 = S.restate(s[:, :3], r, s, S.BOXES["cube"])
        assert np.all(counts == n_torus), (offset, r, counts.min(), counts.max())
        open_counts = S.restate(s[:, :3], r, s, (0.0, 0.0, 0.0))[0]
        assert open_counts.min() == open_min and open_counts.max() == n_torus and np.any(open_counts < n_torus)
        if r == F32(1.0 / 16.0):                                     # d2 == R2 across the seam
            assert np.sum(d2 == F32(1.0 / 256.0)) == 6 * len(s)
        # translation invariance: every row is the first row's, as wrapped offsets from its own site
        rel = S.wrap((s[idx, 0] - np.repeat(s[:, 0], counts)).astype(F32), 1.0)
        assert np.array_equal(np.sort(rel.reshape(len(s), n_torus), axis=1),
                              np.tile(np.sort(rel[:n_torus]), (len(s), 1)))


def test_restated_pair_counts_on_the_torus_exceed_the_open_ones():
    """3000 uniform points, r = 0.05: 7812 ordered pairs (self pairs included) against 7582 without the
    period."""
    x = np.random.default_rng(1).random((3000, 3)).astype(F32)
    s = S.spheres_of(x)
    assert int(S.restate(x, 0.05, s, S.BOXES["cube"])[0].sum()) == 7812
    assert int(S.restate(x, 0.05, s, (0.0, 0.0, 0.0))[0].sum()) == 7582
    totals = S.restate_bins(x, [0.0, 0.025, 0.05], s, S.BOXES["cube"])[0]
    assert totals.tolist()[0] == 3000 and int(totals.sum()) == 7812


@pytest.mark.parametrize("period", [(0.0, 0.0, 0.0), (8.0, 300.0, 2.5)])
def test_restatement_without_wraps_is_the_open_restatements(period):
    """L = 0 and any L above twice the extent: the open queries' own restatements, bit for bit."""
    s = S.uniform(1500, "cube", 0.0, 5)
    pts, r = S.uniform_queries(s, "cube", 0.0, 5, 400)
    r[:12] = np.array([0.0, -1.0, np.nan, np.inf, 0.3, 0.6, 1.0, 1.2, 0.2, 0.1, 0.05, 1e-3], F32)
    assert all(_same(a, b) for a, b in zip(S.restate(pts, r, s, period), open_restate(pts, r, s)))
    w = (0.5 + np.random.default_rng(3).random((len(s), 2))).astype(F32)
    edges = np.array([0.0, 0.01, 0.05, 0.11], F32)
    totals, counts, sums = S.restate_bins(pts, edges, s, period, w)
    o_totals, o_counts, o_sums = open_bins(pts, [edges], s, w)[0]
    assert np.array_equal(totals, o_totals) and np.array_equal(counts, o_counts) and _same(sums, o_sums)
    for b in (0.03, 0.06):
        assert np.array_equal(S.restate_labels(s, b, period), open_labels(s, [F32(b)])[0])


@pytest.mark.parametrize("offset", (0.0, 100.0))
def test_restated_seam(offset):
    s, q, r = S.seam(offset)
    period = S.BOXES["cube"]
    counts = S.restate(q, r, s, period)[0]
    o = F32(offset)
    # a centre at o and one at o + L, queried at o with r = 0: both (and the corner at o + L on all three axes)
    assert np.all(q[0] == o) and r[0] == 0 and counts[0] >= 3
    assert S.restate(q[:1], r[:1], s[:2], period)[0][0] == 2
    assert S.restate(q[:1], r[:1], s[:2], (0.0, 0.0, 0.0))[0][0] == 1
    # the coincident corner queries find each other at r = 0 and more through the faces at the larger radii
    corner = slice(len(q) - 80, len(q))
    assert np.all(counts[corner][r[corner] == 0] >= 80)
    open_counts = S.restate(q, r, s, (0.0, 0.0, 0.0))[0]
    assert np.all(counts >= open_counts) and np.sum(counts > open_counts) > 200
    small = r <= F32(1e-6)
    assert np.sum(counts[small] > open_counts[small]) > 20            # wraps decided within a few ulp of the faces


@pytest.mark.parametrize("offset", S.OFFSETS)
def test_restated_groups_across_the_seam(offset):
    """The straddling clump is one group with the period and two without; the chain with a gap closes around
    the torus.  unite() against plain label propagation."""
    period = S.BOXES["cube"]
    s = S.straddling_clump(offset)
    b = F32(0.012)
    lab, lab_open = S.restate_labels(s, b, period), S.restate_labels(s, b, (0.0, 0.0, 0.0))
    clump = np.arange(400)
    big = np.bincount(lab[clump]).argmax()
    assert np.sum(lab[clump] == big) > 380
    sizes_open = np.sort(np.bincount(lab_open[clump]))[::-1]
    assert sizes_open[0] < 300 and sizes_open[1] > 100                # two halves
    assert np.array_equal(lab, S.components(len(s), *S.links(s, b, period)))
    c = S.torus_chain(offset)
    b = F32(1.0 / 64.0)
    assert len(np.unique(S.restate_labels(c, b, period))) == 1
    assert len(np.unique(S.restate_labels(c, b, (0.0, 0.0, 0.0)))) == 2
    assert len(np.unique(S.restate_labels(c, b, (0.0, 1.0, 1.0)))) == 2   # x open: the seam does not link


def test_special_radii_switch_points_off_above_half_a_period():
    for box, period in S.BOXES.items():
        s = S.uniform(500, box, 0.0, 9)
        pts, r = S.uniform_queries(s, box, 0.0, 9, 200)
        counts = S.restate(pts, r, s, period)[0]
        sp = S.special_radii(box)
        k = len(sp)
        assert counts[0] == 1 and counts[1] == 1 and np.all(counts[2:5] == 0)      # r = 0, -0 at a centre; off
        lmin = min(L for L in period if L > 0)
        for i in range(5, k, 2):                                      # (half a period: on, its successor: off)
            assert (counts[i] > 0) == (sp[i] <= S.half(lmin)) and counts[i + 1] == 0
        assert np.all(counts[k:k + 20] > 20)                          # r = half the smallest period
