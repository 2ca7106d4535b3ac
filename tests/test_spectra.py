"""Velocity-space absorption spectra along rays (grace_trace_spectra_f4, trace_spectra_sph).  The
contract, from include/grace_hip.h: a ray's hits, their integrals I and distances d and their order
are those of trace_emission_absorption_sph; then in fp64, for hit k on sphere i_k and channel c,

    N_kc = amount[i_k, c] * I_k            v_k = hubble * d_k + ((vx dx + vy dy) + vz dz)
    b_kc = width[i_k, c]                   e_u = v0 + u dv
    P_kc(u) = 0.5 (erf((e_{u+1} - v_k) / b_kc) - erf((e_u - v_k) / b_kc))
    window: u_lo = floor((v_k - 6 b_kc - v0) / dv) .. u_hi = floor((v_k + 6 b_kc - v0) / dv)
    tau[r, c, j] = fl32( (1 / dv) sum_k sum_{u in window, u == j (window mode) or u mod n_bins == j (periodic)} N_kc P_kc(u) )
    column[r, c] = fl32( sum_k N_kc )

Expected values restate this in NumPy (scipy.special.erf) from the oracle's per-hit outputs
(oracle.brute_hits), so the inputs of the fp64 arithmetic are bit-equal on both sides.

The tolerance is derived, not measured.  With eps = 2^-53 and V_k = |v0| + n_bins dv + |hubble d_k|
+ |vx dx| + |vy dy| + |vz dz| (every intermediate of e_u and v_k is at most V_k in magnitude): e_u
and v_k carry a few eps V_k each, so an argument of erf carries a few eps V_k / b_kc absolute, plus
a relative eps or two from the division (the device multiplies by 1 / b_kc: one more), which
matters only where erf' does not vanish, and there |x| erf'(x) <= 0.5; erf' <= 1.13; each erf is
evaluated to a few eps absolute (|erf| <= 1).  Two erf values make one P, so
|P - P_exact| <= 16 eps (1 + V_k / b_kc) with room to spare, and it is multiplied by |N_kc| / dv.
The n_r additions into a bin and the products cost 8 (n_r + 8) eps of the sum S of |terms| (the
neighbouring files' bound).  A window edge is a floor(): where the quotient lies within 1e-6 of an
integer (ten thousand times the rounding that could move it, for V_k / b_kc < 1e6) the two sides may
disagree on whether the bin beyond that edge belongs to the window, and that bin lies wholly
outside v_k -+ 6 b_kc, so its term is at most |N_kc| / dv * erfc(6) / 2; erfc(6) is allowed.  Hence,
per bin, summing over the hits k that reach it,

    |tau - ref| <= spacing(fl32(|ref|)) / 2 + eps sum_k (|N_kc| / dv) 16 (1 + V_k / b_kc)
                   + 8 (n_r + 8) eps S + sum_{k: an edge within 1e-6 of this bin's} |N_kc| / dv erfc(6)

(the second sum is taken over the hits that reach the bin, not over all hits of the ray: tighter
than the header's).  A bin that no hit reaches must be exactly zero.  column gets
spacing / 2 + 8 (n_r + 8) eps sum_k |N_kc|.  Scenes keep V_k / b_kc below 1e6 (asserted)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
from scipy.special import erf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grace-devel_amd", "lib")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off",
               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "cpp")]
F32, F64 = np.float32, np.float64
EPS = 2.0 ** -53
ERFC6 = math.erfc(6.0)


# ---- the restatement ----------------------------------------------------------------------------
def restate(rays_h, hits, amount, width, vel, v0, dv, n_bins, periodic, hubble):
    """(tau [n_rays, C, n_bins], tol_tau, column [n_rays, C], tol_column) in fp64.  rays_h: [n, 7]
    float32 (direction first); hits: oracle.brute_hits' (offsets, idx, integrals, distances);
    amount, width: [n_spheres, C] float32; vel: [n_spheres, 3] float32."""
    off, idx, integ, dist = hits
    n_rays, n_hits, C = len(rays_h), len(idx), amount.shape[1]
    counts = np.diff(np.append(off, n_hits)).astype(np.int64)
    ray = np.repeat(np.arange(n_rays), counts)
    n_r = counts[ray].astype(F64)
    dirs = rays_h[:, :3].astype(F64)[ray]
    w = vel[idx].astype(F64)
    flow = F64(hubble) * dist.astype(F64)
    v = flow + ((w[:, 0] * dirs[:, 0] + w[:, 1] * dirs[:, 1]) + w[:, 2] * dirs[:, 2])
    V = abs(v0) + n_bins * dv + np.abs(flow) + np.abs(w * dirs).sum(1)
    size = n_rays * n_bins
    tau = np.zeros((n_rays, C, n_bins), F64); tol = np.zeros_like(tau)
    col = np.zeros((n_rays, C), F64); tol_col = np.zeros_like(col)
    for c in range(C):
        N = amount[idx, c].astype(F64) * integ.astype(F64)
        b = width[idx, c].astype(F64)
        col[:, c] = np.bincount(ray, N, n_rays)
        tol_col[:, c] = 8.0 * (counts + 8.0) * EPS * np.bincount(ray, np.abs(N), n_rays)
        ok = (b > 0) & np.isfinite(b) & np.isfinite(v)
        with np.errstate(all="ignore"):
            q_lo, q_hi = ((v - 6.0 * b) - v0) / dv, ((v + 6.0 * b) - v0) / dv
            lo, hi = np.floor(q_lo), np.floor(q_hi)
            if periodic:
                mid = np.floor((v - v0) / dv)
                lo, hi = np.maximum(lo, mid - n_bins), np.minimum(hi, mid + n_bins)
            else:
                lo, hi = np.maximum(lo, 0.0), np.minimum(hi, n_bins - 1.0)
            ok &= hi >= lo
            if np.any(ok):
                assert np.max(V[ok] / b[ok]) < 1e6
        h = np.nonzero(ok)[0]
        ln = (hi[h] - lo[h]).astype(np.int64) + 1
        rep = np.repeat(h, ln)
        u = lo[rep] + (np.arange(ln.sum()) - np.repeat(np.cumsum(ln) - ln, ln))
        P = 0.5 * (erf(((v0 + (u + 1.0) * dv) - v[rep]) / b[rep]) - erf(((v0 + u * dv) - v[rep]) / b[rep]))
        term = N[rep] * P / dv
        flat = ray[rep] * n_bins + np.mod(u, n_bins).astype(np.int64)
        t = np.bincount(flat, term, size)
        S = np.bincount(flat, np.abs(term), size)
        A = np.bincount(flat, np.abs(N[rep]) / dv * 16.0 * (1.0 + V[rep] / b[rep]), size)
        nr = np.zeros(size); nr[flat] = n_r[rep]
        slack = np.zeros(size)
        for q, du in ((q_lo, -1), (q_hi, 0)):   # a window edge a rounding could move: the bin in dispute
            near = np.nonzero(ok & (np.abs(q - np.rint(q)) < 1e-6))[0]
            e = np.rint(q[near]) + du
            keep = np.ones(len(near), bool) if periodic else (e >= 0) & (e < n_bins)
            np.add.at(slack, ray[near[keep]] * n_bins + np.mod(e[keep], n_bins).astype(np.int64),
                      np.abs(N[near[keep]]) / dv * ERFC6)
        tau[:, c, :] = t.reshape(n_rays, n_bins)
        tol[:, c, :] = (EPS * A + 8.0 * (nr + 8.0) * EPS * S + slack).reshape(n_rays, n_bins)
    tol += np.spacing(np.abs(tau).astype(F32)).astype(F64) / 2
    tol_col += np.spacing(np.abs(col).astype(F32)).astype(F64) / 2
    return tau, tol, col, tol_col


def check(got, got_col, ref, tol, col, tol_col, what=""):
    err = np.abs(got.astype(F64) - ref)
    lit = ref != 0
    print("%s: tau max err/tol %.3g over %d bins (%d lit, peak %.3g)" % (
        what, float(np.max(err / tol)) if err.size else 0.0, err.size, int(lit.sum()),
        float(np.abs(ref).max()) if err.size else 0.0))
    half = np.spacing(np.abs(ref).astype(F32)).astype(F64) / 2      # the final rounding's share of the bound
    over = (err - half)[lit] / (tol - half)[lit]
    print("%s: tau beyond the fp32 rounding: max (err - ulp32 / 2) / (tol - ulp32 / 2) %.3g" % (
        what, max(float(over.max()), 0.0) if over.size else 0.0))
    assert not np.any(np.isnan(got))
    bad = np.argwhere(err > tol)
    assert len(bad) == 0, (what, bad[:5], got[tuple(bad[0])], ref[tuple(bad[0])], tol[tuple(bad[0])])
    if got_col is not None:
        err = np.abs(got_col.astype(F64) - col)
        print("%s: column max err/tol %.3g" % (what, float(np.max(err / tol_col)) if err.size else 0.0))
        bad = np.argwhere(err > tol_col)
        assert len(bad) == 0, (what, "column", bad[:5])


def _fields(sh, C, seed, span, signed=False):
    """amount (positive, or of both signs), width log-uniform over two decades (span / 2000 ..
    span / 20: below a quarter of a period of `span`), velocities of both signs."""
    rng = np.random.default_rng(seed)
    amount = (0.25 + rng.random((len(sh), C))).astype(F32)
    if signed:
        amount = (amount - F32(0.75)).astype(F32)
    width = (span / 2000.0 * 100.0 ** rng.random((len(sh), C))).astype(F32)
    vel = ((rng.random((len(sh), 3)) - 0.5) * 0.3 * span).astype(F32)
    return amount, width, vel


def _random_scene(n, seed):
    rng = np.random.default_rng(seed)
    s = np.empty((n, 4), F32)
    s[:, :3] = rng.random((n, 3), dtype=F32)
    s[:, 3] = (0.01 + 0.04 * rng.random(n)).astype(F32)     # radii spanning 5x
    return s


# ---- CPU: exported, and the drop-in forms compile -------------------------------------------------
def test_entry_point_is_exported():
    lib = ctypes.CDLL(os.path.join(LIBDIR, "libgrace_hip.so"))
    assert hasattr(lib, "grace_trace_spectra_f4")
    import grace_hip
    assert callable(grace_hip.trace_spectra_sph)


def _compile_dropin(exe):
    subprocess.check_call(["/opt/rocm/bin/hipcc", *HIPCC_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "dropin_spectra.hip"), "-o", str(exe),
                           "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])


def test_dropin_compiles_with_hipcc(tmp_path):
    exe = tmp_path / "dropin_spectra"
    _compile_dropin(exe)
    assert exe.exists()


def test_mirror_compiles_with_gxx(tmp_path):
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "grace/grace.h"\n'
                   "void f(const grace::device_vector<grace::Ray>& r, const grace::device_vector<grace::float4>& s,\n"
                   "       const grace::Tree& t, const grace::device_vector<float>& a, const grace::device_vector<float>& w,\n"
                   "       const grace::device_vector<float>& v)\n"
                   "{\n"
                   "    grace::SpectrumGrid g = { -1.0, 0.5, 64, 1, 70.0 };\n"
                   "    grace::device_vector<float> tau(r.size() * 3 * 64), col(r.size() * 3);\n"
                   "    grace::trace_spectra_sph(r, s, t, a, w, v, 3, g, tau);\n"
                   "    grace::trace_spectra_sph(r, s, t, a, w, v, 3, g, tau, &col);\n"
                   "}\n"
                   "int main() { return 0; }\n")
    exe = tmp_path / "mirror"
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L" + LIBDIR, "-lgrace_hip", "-Wl,-rpath," + LIBDIR])
    assert exe.exists()


# ---- CPU: the restatement itself --------------------------------------------------------------------
def test_restatement_conserves_the_column_in_periodic_mode(oracle):
    sh = _random_scene(2000, 7)
    rays_h = np.ascontiguousarray(oracle.orthogonal_rays_z(16, (0, 0, 0, 0), (1, 1, 1, 0))[0]).view(F32).reshape(-1, 7)
    hits = oracle.brute_hits(rays_h, sh)
    assert len(hits[1]) > 1000
    span = 100.0
    amount, width, vel = _fields(sh, 3, 1, span, signed=True)
    tau, tol, col, tol_col = restate(rays_h, hits, amount, width, vel, -13.0, span / 128, 128, True, span)
    # dv sum_j tau against the column: the bins' bounds add up (without the final fp32 roundings,
    # which the restatement does not make), and every hit may lose erfc(6) of its column
    room = (span / 128) * (tol - np.spacing(np.abs(tau).astype(F32)).astype(F64) / 2).sum(2)
    n_r = np.diff(np.append(hits[0], len(hits[1])))
    lost = ERFC6 * np.stack([np.bincount(np.repeat(np.arange(len(rays_h)), n_r),
                                         np.abs(amount[hits[1], c].astype(F64) * hits[2]), len(rays_h))
                             for c in range(3)], 1)
    err = np.abs((span / 128) * tau.sum(2) - col)
    print("restated conservation: max err / bound %.3g" % float(np.max(err / (room + lost + 1e-300))))
    assert np.all(err <= room + lost)
    assert np.abs(col).max() > 0


def test_restatement_of_one_sphere_is_a_gaussian_and_narrow_lines_fill_one_bin(oracle):
    sh = np.array([[0.5, 0.5, 0.5, 0.2]], F32)
    rays_h = np.array([[0, 0, 1, 0.5, 0.5, -0.25, 2.0]], F32)           # through the centre: d = 0.75
    hits = oracle.brute_hits(rays_h, sh)
    assert len(hits[1]) == 1 and hits[3][0] == F32(0.75)
    hubble, dv, n_bins = 64.0, 0.125, 512                                 # the line sits at v = 48
    b = 20 * dv
    amount = np.array([[3.0]], F32); width = np.array([[b]], F32); vel = np.zeros((1, 3), F32)
    tau, tol, col, _ = restate(rays_h, hits, amount, width, vel, 16.0, dv, n_bins, False, hubble)
    N = 3.0 * F64(hits[2][0])
    assert col[0, 0] == N and abs(dv * tau.sum() - N) <= 1e-14 * N
    centre = 16.0 + (np.arange(n_bins) + 0.5) * dv
    assert abs(dv * (tau[0, 0] * centre).sum() / N - hubble * 0.75) <= 1e-12 * 48
    g = N / (b * math.sqrt(math.pi)) * np.exp(-((centre - 48.0) / b) ** 2)
    # the bin average against the value at the centre: dv^2 / 24 max |g''|, and max |g''| = 2 peak / b^2
    assert np.max(np.abs(tau[0, 0] - g)) <= g.max() * (dv / b) ** 2 / 12 * 1.01
    # narrow lines: width = dv / 100, hits at least a tenth of a bin from the edges
    sh = _random_scene(2000, 9)
    rays_h = np.ascontiguousarray(oracle.orthogonal_rays_z(8, (0, 0, 0, 0), (1, 1, 1, 0))[0]).view(F32).reshape(-1, 7)
    off, idx, integ, dist = oracle.brute_hits(rays_h, sh)
    amount = np.ones((2000, 1), F32); vel = np.zeros((2000, 3), F32)
    dv = 0.01; width = np.full((2000, 1), dv / 100, F32)
    frac = np.mod(32.0 * dist.astype(F64) / dv, 1.0)
    keep = (frac > 0.1) & (frac < 0.9) & (dist > 0) & (dist < 1)
    assert keep.sum() > 100
    for k in np.nonzero(keep)[0][:200]:
        r = np.searchsorted(off, k, side="right") - 1
        one = (np.array([0]), idx[k:k + 1], integ[k:k + 1], dist[k:k + 1])
        tau, _, col, _ = restate(rays_h[r:r + 1], one, amount, width, vel, 0.0, dv, 3200, False, 32.0)
        j = int(np.floor(32.0 * F64(dist[k]) / dv))
        assert np.count_nonzero(tau) == 1 and abs(tau[0, 0, j] * dv - col[0, 0]) <= 1e-15 * col[0, 0]


# ---- CPU: the snapshot reader ---------------------------------------------------------------------------
def _write_gadget_as_before(fname, pos, hsml, masses_in_header=True):
    """write_gadget as it was before it took vel= and u=."""
    pos = np.ascontiguousarray(pos, np.float32); hsml = np.ascontiguousarray(hsml, np.float32)
    n = len(pos)
    npart = np.array([n, 0, 0, 0, 0, 0], np.int32)
    mass = np.array([1.0 if masses_in_header else 0.0, 0, 0, 0, 0, 0], np.float64)

    def block(f, payload):
        nbytes = np.array([len(payload)], np.int32).tobytes()
        f.write(nbytes); f.write(payload); f.write(nbytes)

    with open(fname, "wb") as f:
        header = npart.tobytes() + mass.tobytes()
        block(f, header + bytes(256 - len(header)))
        block(f, pos.tobytes())
        block(f, np.zeros((n, 3), np.float32).tobytes())
        block(f, np.arange(n, dtype=np.int32).tobytes())
        if not masses_in_header:
            block(f, np.ones(n, np.float32).tobytes())
        block(f, np.zeros(n, np.float32).tobytes())
        block(f, np.ones(n, np.float32).tobytes())
        block(f, hsml.tobytes())


@pytest.mark.parametrize("masses_in_header", [True, False])
def test_gadget_fields_round_trip(tmp_path, masses_in_header):
    from grace_hip import gadget
    rng = np.random.default_rng(5)
    n = 1000
    pos = rng.random((n, 3)).astype(F32); hsml = (0.01 + rng.random(n)).astype(F32)
    vel = (rng.random((n, 3)) - 0.5).astype(F32) * F32(300); u = (rng.random(n) * 1e4).astype(F32)
    a, b, c = (str(tmp_path / x) for x in ("before.gad", "plain.gad", "fields.gad"))
    _write_gadget_as_before(a, pos, hsml, masses_in_header)
    gadget.write_gadget(b, pos, hsml, masses_in_header)
    assert open(a, "rb").read() == open(b, "rb").read()               # without the keywords: the same bytes
    gadget.write_gadget(c, pos, hsml, masses_in_header, vel=vel, u=u)
    f = gadget.read_gadget_fields(c, 0)
    assert np.array_equal(f["pos"], pos) and np.array_equal(f["vel"], vel) and np.array_equal(f["u"], u)
    assert np.array_equal(f["hsml"], hsml) and np.all(f["rho"] == 1)
    assert np.array_equal(gadget.read_gadget(c), gadget.read_gadget(a))
    p, m = gadget.read_gadget_particles(c, 0)
    assert np.array_equal(p, pos) and np.all(m == 1)
    f = gadget.read_gadget_fields(b, 0)
    assert np.all(f["vel"] == 0) and np.all(f["u"] == 0)
    f = gadget.read_gadget_fields(c, 1)                                 # a type the file does not hold
    assert f["pos"].shape == (0, 3) and f["vel"].shape == (0, 3) and "u" not in f
    with pytest.raises(ValueError):
        gadget.read_gadget_fields(c, 6)
    with pytest.raises(ValueError):
        gadget.write_gadget(c, pos, hsml, vel=vel[:-1])


# ---- GPU --------------------------------------------------------------------------------------------
N_SCENE = 20000
SPAN = 96.0            # the velocity range of the scenes: hubble * (a ray's length) and the grids' period
HUBBLE = 64.0


def _build(gh, cuda, s):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(s, F32)).to(cuda)
    tree = gh.Tree(len(s), 32, device=cuda)
    gh.build_tree(d, tree, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))     # sorts d
    return d, tree


def _trace(gh, rays, d, tree, amount, width, vel, v0, dv, n_bins, periodic, hubble, want_column=True):
    import torch
    dev = rays.device
    col = torch.empty((len(rays), amount.shape[1]), dtype=torch.float32, device=dev) if want_column else None
    tau = gh.trace_spectra_sph(rays, d, tree, torch.from_numpy(amount).to(dev), torch.from_numpy(width).to(dev),
                               torch.from_numpy(vel).to(dev), v0, dv, n_bins, periodic=periodic, hubble=hubble,
                               column=col, check=True)
    assert tuple(tau.shape) == (len(rays), amount.shape[1], n_bins)
    return tau.cpu().numpy(), (col.cpu().numpy() if want_column else None)


def _sub_hits(hits, n):
    """The hits of the first n rays."""
    off, idx, integ, dist = hits
    end = off[n] if n < len(off) else len(idx)
    return off[:n], idx[:end], integ[:end], dist[:end]


@pytest.fixture(autouse=True)
def _knobs_reset(request):
    yield
    if "gh" in request.fixturenames:
        gh = request.getfixturevalue("gh")
        gh.set_ordered_budget(0); gh.ordered_enable_stats(False)
        gh.set_packet_width(-1); gh.set_sph_kernel("cubic")


@pytest.fixture(scope="module")
def sp_scene(gh, oracle, cuda):
    import torch
    s = _random_scene(N_SCENE, 3)
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()
    rng = np.random.default_rng(4)
    points = torch.from_numpy(rng.random((1024, 3), dtype=F32)).to(cuda)
    sets = {
        "orthographic": gh.orthogonal_rays_z(48, (0, 0, 0, 0), (1, 1, 1, 0), device=cuda)[0],
        "pinhole": gh.pinhole_camera_rays(48, 48, (0.5, 0.5, -1.5), (0.5, 0.5, 0.5), (0, 1, 0), 0.6, 4.0,
                                          device=cuda),
        "healpix": gh.healpix_rays(8, (0.5, 0.5, 0.5), 1.0, device=cuda),
        "one_to_many": gh.one_to_many_rays((0.45, 0.55, 0.5), points),
    }
    out = {}
    for name, rays in sets.items():
        hits = oracle.brute_hits(rays.cpu().numpy(), sh)
        assert len(hits[1]) > 0
        out[name] = (rays, hits)
    return d, tree, sh, out


RAY_SETS = ["orthographic", "pinhole", "healpix", "one_to_many"]
# (C, n_bins, periodic, hubble, rays used): every C, n_bins, mode and hubble of the issue, the long
# grids on fewer rays so that the restatement stays small
CONFIGS = [(1, 4096, False, HUBBLE, 256), (3, 1000, True, HUBBLE, 512), (4, 64, False, 0.0, 0),
           (5, 65, True, 0.0, 0), (16, 63, True, HUBBLE, 512), (3, 1, True, 0.0, 0), (1, 1, False, HUBBLE, 0),
           (4, 4096, True, 0.0, 256), (5, 1000, False, HUBBLE, 512), (16, 64, False, HUBBLE, 512)]


def _grid(n_bins, periodic, hubble):
    """Periodic: one period of SPAN from -SPAN / 3.  Window: the middle of the range the lines
    cover, so that some windows leave it on either side (for n_bins == 1 a single wide bin)."""
    lo, hi = (-0.15 * SPAN, 0.15 * SPAN) if hubble == 0.0 else (-0.15 * SPAN, 1.15 * SPAN)
    if periodic:
        return -SPAN / 3.0, SPAN / n_bins
    return lo + 0.2 * (hi - lo), 0.6 * (hi - lo) / n_bins


@pytest.mark.gpu
@pytest.mark.parametrize("rays_name", RAY_SETS)
@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "C%d-bins%d-%s-H%g-n%d" % (c[0], c[1], "per" if c[2] else "win", c[3], c[4]))
def test_random_scenes_match_the_restatement(gh, sp_scene, rays_name, config):
    C, n_bins, periodic, hubble, n_used = config
    d, tree, sh, sets = sp_scene
    rays, hits = sets[rays_name]
    if n_used:
        rays, hits = rays[:n_used].contiguous(), _sub_hits(hits, n_used)
    amount, width, vel = _fields(sh, C, 100 + C, SPAN, signed=True)
    v0, dv = _grid(n_bins, periodic, hubble)
    got, got_col = _trace(gh, rays, d, tree, amount, width, vel, v0, dv, n_bins, periodic, hubble)
    ref = restate(rays.cpu().numpy(), hits, amount, width, vel, v0, dv, n_bins, periodic, hubble)
    assert np.count_nonzero(ref[0]) > 0
    check(got, got_col, *ref, what="%s %s" % (rays_name, config))


def _collinear_scene(counts, cuda):
    """Rays along z on an 8-column grid of pitch 0.1; ray j's spheres (radius 0.01) sit on it."""
    import torch
    rays = np.zeros((len(counts), 7), F32)
    spheres = []
    for j, m in enumerate(counts):
        x, y = 0.1 + 0.1 * (j % 8), 0.1 + 0.1 * (j // 8)
        rays[j] = (0, 0, 1, x, y, -0.1, 1.2)
        if m:
            z = (np.arange(m) + 0.5) / m * 0.9 + 0.05
            spheres.append(np.stack([np.full(m, x), np.full(m, y), z, np.full(m, 0.01)], 1))
    s = np.concatenate(spheres).astype(F32)
    return torch.from_numpy(rays).to(cuda), s


@pytest.mark.gpu
@pytest.mark.parametrize("periodic", [False, True])
def test_tier_edges(gh, oracle, cuda, periodic):
    w, b = gh.ordered_limits()
    assert 64 <= w < b
    counts = [0, 3, w - 1, w, w + 1, 40, b - 1, 0, b, b + 1, 4 * b, 1, 0, w // 2, 2 * w, 17,
              0, 0, 5, 0, 64, 65, 63, 0, 0, 0, 0, 0, 0, 0, 0, 2]
    rays, s = _collinear_scene(counts, cuda)
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()
    hits = oracle.brute_hits(rays.cpu().numpy(), sh)
    assert np.array_equal(np.diff(np.append(hits[0], len(hits[1]))), counts)     # exact hit counts
    amount, width, vel = _fields(sh, 2, 5, SPAN, signed=True)
    amount = (amount * F32(1e-4)).astype(F32)                                     # I ~ 1.9e4 per hit
    width = (width * F32(0.25)).astype(F32)                                       # windows of ~25 bins
    n_bins = 300
    v0, dv = _grid(n_bins, periodic, HUBBLE)
    gh.ordered_enable_stats(True)
    got, got_col = _trace(gh, rays, d, tree, amount, width, vel, v0, dv, n_bins, periodic, HUBBLE)
    st = gh.ordered_last_stats()
    c = np.array(counts)
    assert st["rays_wave"] == np.sum(c <= w) and st["rays_block"] == np.sum((c > w) & (c <= b))
    assert st["rays_global"] == np.sum(c > b) == 2 and st["total_hits"] == c.sum()
    ref = restate(rays.cpu().numpy(), hits, amount, width, vel, v0, dv, n_bins, periodic, HUBBLE)
    check(got, got_col, *ref, what="tier edges, periodic=%s" % periodic)
    assert np.all(got[c == 0] == 0) and np.all(got_col[c == 0] == 0)
    # the same rays in batches: a ray longer than the budget is a batch of its own
    gh.set_ordered_budget(12 * (b + 1))
    again, again_col = _trace(gh, rays, d, tree, amount, width, vel, v0, dv, n_bins, periodic, HUBBLE)
    assert gh.ordered_last_stats()["batches"] > 5
    assert np.array_equal(_bits(again), _bits(got)) and np.array_equal(_bits(again_col), _bits(got_col))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("periodic", [False, True])
def test_results_are_bitwise_invariant(gh, sp_scene, cuda, periodic):
    import torch
    d, tree, sh, sets = sp_scene
    rays, (off, idx, integ, dist) = sets["pinhole"]
    amount, width, vel = _fields(sh, 3, 11, SPAN, signed=True)
    n_bins = 200
    v0, dv = _grid(n_bins, periodic, HUBBLE)
    run = lambda r, **kw: _trace(gh, r, d, tree, amount, width, vel, v0, dv, n_bins, periodic, HUBBLE, **kw)
    gh.ordered_enable_stats(True)
    gh.set_ordered_budget(1 << 32)
    base, base_col = run(rays)
    st = gh.ordered_last_stats()
    assert st["batches"] == 1 and st["total_hits"] == len(idx)
    assert np.count_nonzero(base) > 0
    same = lambda o, t, rows=slice(None): (np.array_equal(_bits(o), _bits(base[rows]))
                                           and np.array_equal(_bits(t), _bits(base_col[rows])))
    assert same(*run(rays))                                               # two runs
    gh.set_ordered_budget(12 * len(idx) // 7)
    assert same(*run(rays))
    assert gh.ordered_last_stats()["batches"] >= 5
    sub = slice(1000, 1256)
    gh.set_ordered_budget(1)                                              # one batch per ray
    assert same(*run(rays[sub].contiguous()), rows=sub)
    n_sub = np.diff(np.append(off, len(idx)))[sub]
    assert np.all(n_sub > 0) and gh.ordered_last_stats()["batches"] == 256
    gh.set_ordered_budget(0)
    for width_ in (64, 32, 16):
        gh.set_packet_width(width_)
        assert same(*run(rays)), width_
    gh.set_packet_width(-1)
    perm = torch.randperm(len(rays), generator=torch.Generator().manual_seed(3))
    o, t = run(rays[perm.to(cuda)].contiguous())                          # rays permuted: rows permute
    assert np.array_equal(_bits(o), _bits(base[perm.numpy()])) and np.array_equal(_bits(t), _bits(base_col[perm.numpy()]))
    r = 1234                                                               # a ray traced alone
    assert np.diff(np.append(off, len(idx)))[r] > 0
    alone = rays[r:r + 1].repeat(32, 1)                                   # (ray counts are multiples of 32:
    alone[1:, 3:6] += 10.0                                                 #  31 companions that miss the box)
    o, t = run(alone.contiguous())
    assert np.array_equal(_bits(o[:1]), _bits(base[r:r + 1])) and np.array_equal(_bits(t[:1]), _bits(base_col[r:r + 1]))
    assert np.all(o[1:] == 0) and np.all(t[1:] == 0)
    o, _ = run(rays, want_column=False)                                   # column is optional
    assert np.array_equal(_bits(o), _bits(base))
    stream = torch.cuda.Stream()                                          # another context and stream
    ctx = gh.Context()
    try:
        ctx.make_current()
        with torch.cuda.stream(stream):
            o, t = run(rays)
    finally:
        gh.Context.reset_current()
        ctx.destroy()
    assert same(o, t)


@pytest.mark.gpu
def test_conservation_on_the_devices_output(gh, sp_scene):
    """Periodic mode, positive amounts: dv sum_j tau[r, c, j] and column[r, c] are sums of the same
    non-negative terms up to erfc(6) per hit, each bin rounded to fp32 once (2^-24 relative, so
    2^-24 of the sum), the column once, and the fp64 sums to n 2^-53: 2.5 x 2^-24 of the column."""
    d, tree, sh, sets = sp_scene
    rays, hits = sets["orthographic"]
    amount, width, vel = _fields(sh, 4, 21, SPAN)
    n_bins = 256
    got, got_col = _trace(gh, rays, d, tree, amount, width, vel, -SPAN / 3, SPAN / n_bins, n_bins, True, HUBBLE)
    total = (SPAN / n_bins) * got.astype(F64).sum(2)
    err = np.abs(total - got_col)
    print("device conservation: max err / column %.3g" % float(np.max(err[got_col > 0] / got_col[got_col > 0])))
    assert np.all(got_col[np.diff(np.append(hits[0], len(hits[1]))) > 0] > 0)
    assert np.all(err <= 2.5 * 2.0 ** -24 * got_col)


@pytest.mark.gpu
def test_windows_partly_and_wholly_outside_the_grid(gh, oracle, cuda):
    """One sphere per ray along z, at rest; hubble * d places the lines at chosen places about a
    window grid of 32 bins of width 1 (given here relative to its lower edge): inside, across
    either edge, just outside, far outside.  Widths of 0.5: windows of -+3."""
    import torch
    centres = [16.5, 0.3, -0.3, 31.9, 32.2, -3.1, 35.5, -6.0, 45.0, 0.0, 32.0, 5.0]
    hubble, b = 100.0, 0.5
    rays = np.zeros((32, 7), F32)
    s = np.zeros((len(centres), 4), F32)
    for j in range(32):
        x, y = 0.1 + 0.1 * (j % 8), 0.1 + 0.1 * (j // 8)
        rays[j] = (0, 0, 1, x, y, -3.0, 6.0)                                # d = z + 3: v = 100 z + 300
        if j < len(centres):
            s[j] = (x, y, 0.45 + centres[j] / hubble, 0.01)                 # v = centre + 345
    pad = np.tile(np.array([[0.95, 0.95, 0.5, 1e-4]], F32), (64, 1)); pad[:, 2] += np.arange(64, dtype=F32) * F32(1e-3)
    d, tree = _build(gh, cuda, np.concatenate([s, pad]).astype(F32))
    sh = d.cpu().numpy()
    hits = oracle.brute_hits(rays, sh)
    n_r = np.diff(np.append(hits[0], len(hits[1])))
    assert np.array_equal(n_r, [1] * len(centres) + [0] * (32 - len(centres)))
    amount = np.full((len(sh), 2), 2.0, F32); width = np.full((len(sh), 2), b, F32); vel = np.zeros((len(sh), 3), F32)
    got, got_col = _trace(gh, torch.from_numpy(rays).to(cuda), d, tree, amount, width, vel, 345.0, 1.0, 32, False, hubble)
    ref = restate(rays, hits, amount, width, vel, 345.0, 1.0, 32, False, hubble)
    check(got, got_col, *ref, what="windows")
    lit = np.array([np.count_nonzero(got[j, 0]) for j in range(len(centres))])
    assert lit[0] == 7 and 0 < lit[1] < 7 and 0 < lit[2] < 7 and 0 < lit[3] < 7 and 0 < lit[4] < 7
    assert lit[5] == 0 and lit[6] == 0 and lit[7] == 0 and lit[8] == 0       # wholly outside: the row stays zero
    assert np.all(got_col[:len(centres)] > 0)                                  # ... but the column counts them


@pytest.mark.gpu
def test_periodic_wrap(gh, sp_scene, oracle, cuda):
    d, tree, sh, sets = sp_scene
    rays, hits = sets["healpix"]
    amount, width, vel = _fields(sh, 3, 31, SPAN, signed=True)
    n_bins, dv = 96, 1.0                                                      # the period, 96, is exact
    rays_h = rays.cpu().numpy()
    base, _ = _trace(gh, rays, d, tree, amount, width, vel, -32.0, dv, n_bins, True, HUBBLE)
    _, tol0, _, _ = restate(rays_h, hits, amount, width, vel, -32.0, dv, n_bins, True, HUBBLE)
    for shift in (1, -1, 3):
        v0 = -32.0 + shift * n_bins * dv
        got, _ = _trace(gh, rays, d, tree, amount, width, vel, v0, dv, n_bins, True, HUBBLE)
        _, tol1, _, _ = restate(rays_h, hits, amount, width, vel, v0, dv, n_bins, True, HUBBLE)
        err = np.abs(got.astype(F64) - base.astype(F64))
        print("v0 shifted by %d periods: max err/tol %.3g" % (shift, float(np.max(err / (tol0 + tol1)))))
        assert np.all(err <= tol0 + tol1)
    # a narrow line on the seam: one sphere at d = 0.75 exactly, v = 48 = v0 (mod the period)
    one, tree1 = _build_one(gh, cuda, np.array([[0.5, 0.5, 0.5, 0.2]], F32))
    s1 = one.cpu().numpy()
    import torch
    ray = np.zeros((32, 7), F32); ray[:] = (0, 0, 1, 5.0, 5.0, -0.25, 2.0); ray[0, 3:5] = 0.5
    h1 = oracle.brute_hits(ray, s1)
    assert len(h1[1]) == 1 and h1[3][0] == F32(0.75) and np.all(s1[h1[1][0]] == F32([0.5, 0.5, 0.5, 0.2]))
    a1 = np.ones((len(s1), 1), F32); w1 = np.full((len(s1), 1), 0.05, F32); z1 = np.zeros((len(s1), 3), F32)
    got, col = _trace(gh, torch.from_numpy(ray).to(cuda), one, tree1, a1, w1, z1, 48.0 - 64.0, 1.0, 64, True, 64.0)
    check(got, col, *restate(ray, h1, a1, w1, z1, 48.0 - 64.0, 1.0, 64, True, 64.0), what="seam")
    N = F64(h1[2][0])
    assert got[0, 0, 0] == got[0, 0, 63] == F32(0.5 * N) and np.all(got[0, 0, 1:63] == 0) and np.all(got[1:] == 0)


def _build_one(gh, cuda, s):
    """A tree needs more spheres than fit a leaf: pad with spheres no ray of the test meets."""
    pad = np.tile(np.array([[0.01, 0.01, 0.99, 1e-4]], F32), (63, 1))
    pad[:, 0] += np.arange(63, dtype=F32) * F32(1e-3)
    return _build(gh, cuda, np.concatenate([s, pad]).astype(F32))


@pytest.mark.gpu
@pytest.mark.parametrize("periodic", [False, True])
def test_bad_widths_add_nothing(gh, sp_scene, periodic):
    d, tree, sh, sets = sp_scene
    rays, hits = sets["one_to_many"]
    amount, width, vel = _fields(sh, 4, 41, SPAN, signed=True)
    n_bins = 128
    v0, dv = _grid(n_bins, periodic, HUBBLE)
    _, good_col = _trace(gh, rays, d, tree, amount, width, vel, v0, dv, n_bins, periodic, HUBBLE)
    rng = np.random.default_rng(2)
    bad = width.copy()
    pick = rng.integers(0, 8, size=width.shape)
    for code, value in ((0, 0.0), (1, -1.0), (2, np.nan), (3, np.inf), (4, -np.inf), (5, -0.0)):
        bad[pick == code] = value
    bad[:, 3] = np.nan                                                       # a channel without any line
    got, got_col = _trace(gh, rays, d, tree, amount, bad, vel, v0, dv, n_bins, periodic, HUBBLE)
    assert not np.any(np.isnan(got)) and not np.any(np.isinf(got))
    assert np.array_equal(_bits(got_col), _bits(good_col))                   # the column does not see widths
    assert np.all(got[:, 3, :] == 0)
    with np.errstate(all="ignore"):
        ref = restate(rays.cpu().numpy(), hits, amount, bad, vel, v0, dv, n_bins, periodic, HUBBLE)
    check(got, got_col, *ref, what="bad widths, periodic=%s" % periodic)
    # a non-finite velocity: the hit adds nothing to tau
    vbad = vel.copy(); vbad[::3, 1] = np.inf; vbad[1::3, 0] = np.nan
    got, got_col = _trace(gh, rays, d, tree, amount, width, vbad, v0, dv, n_bins, periodic, HUBBLE)
    assert not np.any(np.isnan(got)) and np.array_equal(_bits(got_col), _bits(good_col))
    with np.errstate(all="ignore"):
        ref = restate(rays.cpu().numpy(), hits, amount, width, vbad, v0, dv, n_bins, periodic, HUBBLE)
    ok = np.isfinite(ref[1])                                                 # (rows whose bound the bad values spoil)
    assert np.all(np.abs(got.astype(F64) - ref[0])[ok] <= ref[1][ok]) and ok.mean() > 0.2


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["cubic", "quartic", "quintic", "wendland_c2", "wendland_c4", "wendland_c6"])
def test_the_integral_follows_the_sph_kernel(gh, sp_scene, kernel):
    from test_sph_kernels import b2_f32, hit_rays, integrals_f32   # the per-hit arithmetic, restated there
    d, tree, sh, sets = sp_scene
    rays, (off, idx, _, dist) = sets["healpix"]
    rh = rays.cpu().numpy()
    integ = integrals_f32(b2_f32(rh, sh, hit_rays(off, len(idx)), idx), sh[idx, 3], gh.sph_kernel_table(kernel))
    gh.set_sph_kernel(kernel)
    amount, width, vel = _fields(sh, 2, 51, SPAN)
    got, got_col = _trace(gh, rays, d, tree, amount, width, vel, -SPAN / 3, SPAN / 160, 160, True, HUBBLE)
    ref = restate(rh, (off, idx, integ, dist), amount, width, vel, -SPAN / 3, SPAN / 160, 160, True, HUBBLE)
    check(got, got_col, *ref, what=kernel)


@pytest.mark.gpu
def test_argument_checks(gh, sp_scene, cuda):
    import torch
    d, tree, sh, sets = sp_scene
    rays, _ = sets["healpix"]
    n = len(sh)
    am = torch.ones((n, 2), device=cuda); wi = torch.ones((n, 2), device=cuda); ve = torch.zeros((n, 3), device=cuda)
    tau = torch.full((len(rays), 2, 8), 7.0, device=cuda); col = torch.full((len(rays), 2), 7.0, device=cuda)
    args = gh._trace_args(rays, d, tree)

    def call(a=args, amount=am, width=wi, velocity=ve, C=2, grid=(0.0, 1.0, 8, 0, 0.0), out=tau, null_grid=False):
        g = gh._SpectrumGrid(*grid)
        return gh._lib.grace_trace_spectra_f4(*a, gh._ptr(amount), gh._ptr(width), gh._ptr(velocity), ctypes.c_int(C),
                                              None if null_grid else ctypes.byref(g), gh._ptr(out), gh._ptr(col),
                                              gh._stream())
    bad = gh.GRACE_INVALID_ARGUMENT
    for C in (0, 17, -1):
        assert call(C=C) == bad
    for n_bins in (0, -1, 4097):
        assert call(grid=(0.0, 1.0, n_bins, 0, 0.0)) == bad
    for dv in (0.0, -1.0, float("nan"), float("inf")):
        assert call(grid=(0.0, dv, 8, 0, 0.0)) == bad
    for v0 in (float("nan"), float("inf"), -float("inf")):
        assert call(grid=(v0, 1.0, 8, 0, 0.0)) == bad
        assert call(grid=(0.0, 1.0, 8, 1, v0)) == bad
    assert call(null_grid=True) == bad
    assert call(amount=None) == bad and call(width=None) == bad and call(velocity=None) == bad and call(out=None) == bad
    huge = (args[0], ctypes.c_size_t(1 << 31)) + args[2:]
    assert call(a=huge) == bad
    torch.cuda.synchronize()
    assert torch.all(tau == 7.0) and torch.all(col == 7.0)                  # the outputs were not touched
    empty = (args[0], ctypes.c_size_t(0)) + args[2:]
    assert call(a=empty) == gh.GRACE_OK                                      # zero rays: nothing written
    torch.cuda.synchronize()
    assert torch.all(tau == 7.0) and torch.all(col == 7.0)
    assert call() == gh.GRACE_OK                                             # ... and the good call writes all of it
    torch.cuda.synchronize()
    assert not torch.any(tau == 7.0) and not torch.any(col == 7.0)
    with pytest.raises(ValueError):
        gh.trace_spectra_sph(rays, d, tree, torch.ones((n, 17), device=cuda), torch.ones((n, 17), device=cuda), ve, 0.0, 1.0, 8)
    with pytest.raises(ValueError):
        gh.trace_spectra_sph(rays, d, tree, am, wi[:, :1].contiguous(), ve, 0.0, 1.0, 8)
    with pytest.raises(ValueError):
        gh.trace_spectra_sph(rays, d, tree, am, wi, ve[:-1], 0.0, 1.0, 8)
    with pytest.raises(ValueError):
        gh.trace_spectra_sph(rays, d, tree, am, wi, ve, 0.0, 1.0, 4097)
    with pytest.raises(ValueError):
        gh.trace_spectra_sph(rays, d, tree, am, wi, ve, 0.0, 0.0, 8)
    with pytest.raises(ValueError):
        gh.trace_spectra_sph(rays, d, tree, am, wi, ve, 0.0, 1.0, 8, tau=tau[:-1])
    with pytest.raises(ValueError):
        gh.trace_spectra_sph(rays, d, tree, am, wi, ve, 0.0, 1.0, 8, column=col[:, :1].contiguous())
    one = gh.trace_spectra_sph(rays, d, tree, am[:, 0].contiguous(), wi[:, 0].contiguous(), ve, 0.0, 1.0, 8)
    assert tuple(one.shape) == (len(rays), 1, 8)                             # 1-D fields: one channel


@pytest.mark.gpu
def test_the_other_ordered_traces_are_left_as_found(gh, sp_scene, cuda):
    import torch
    d, tree, sh, sets = sp_scene
    rays, hits = sets["healpix"]
    rng = np.random.default_rng(61)
    e = torch.from_numpy(rng.random((len(sh), 3)).astype(F32)).to(cuda)
    k = torch.from_numpy((rng.random(len(sh)) * 1e-3).astype(F32)).to(cuda)
    L = torch.from_numpy((0.5 + rng.random((len(rays), 3))).astype(F32)).to(cuda)
    k3 = torch.from_numpy((rng.random((len(sh), 3)) * 1e-3).astype(F32)).to(cuda)

    def others():
        tau = torch.empty(len(rays), device=cuda); tr = torch.empty_like(L)
        out = gh.trace_emission_absorption_sph(rays, d, tree, e, k, tau=tau, check=True)
        dep = gh.trace_absorption_deposit_sph(rays, d, tree, L, k3, transmitted=tr, check=True)
        return [t.cpu().numpy().tobytes() for t in (out, tau, dep, tr)]
    gh.ordered_enable_stats(True)
    before = others()
    st_before = gh.ordered_last_stats()
    amount, width, vel = _fields(sh, 4, 71, SPAN)
    gh.set_ordered_budget(12 * len(hits[1]) // 3)
    _trace(gh, rays, d, tree, amount, width, vel, -SPAN / 3, SPAN / 2048, 2048, True, HUBBLE)
    st = gh.ordered_last_stats()
    assert st["batches"] >= 3 and st["total_hits"] == len(hits[1])             # the hook covers the new call
    assert st["rays_wave"] + st["rays_block"] + st["rays_global"] == len(rays)
    gh.set_ordered_budget(0)
    assert others() == before
    st_after = gh.ordered_last_stats()
    for key in ("batches", "total_hits", "rays_wave", "rays_block", "rays_global", "budget_bytes", "frame_bytes"):
        assert st_after[key] == st_before[key], key


@pytest.mark.gpu
def test_a_call_whose_rays_hit_nothing(gh, sp_scene, cuda):
    """No hit in the whole call: every bin and column is +0.0, and the next ordinary call is what
    it was."""
    d, tree, sh, sets = sp_scene
    rays, hits = sets["healpix"]
    amount, width, vel = _fields(sh, 3, 81, SPAN, signed=True)
    v0, dv = _grid(96, True, HUBBLE)
    run = lambda r: _trace(gh, r, d, tree, amount, width, vel, v0, dv, 96, True, HUBBLE)
    before = run(rays)
    assert np.count_nonzero(before[0]) > 0
    away = rays.clone()
    away[:, 3:6] += 10.0                                                   # length 1, ten box lengths off
    gh.ordered_enable_stats(True)
    got, got_col = run(away.contiguous())
    st = gh.ordered_last_stats()
    assert st["total_hits"] == 0 and st["batches"] == 1
    assert not np.any(_bits(got)) and not np.any(_bits(got_col))
    after = run(rays)
    assert gh.ordered_last_stats()["total_hits"] == len(hits[1])
    assert np.array_equal(_bits(after[0]), _bits(before[0])) and np.array_equal(_bits(after[1]), _bits(before[1]))


def _fnv1a(a):
    h = 1469598103934665603
    for byte in np.ascontiguousarray(a).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xffffffffffffffff
    return h


@pytest.mark.gpu
def test_dropin_program_matches_ctypes(gh, cuda, tmp_path):
    s = _random_scene(9000, 41)
    d, tree = _build(gh, cuda, s)
    sh = d.cpu().numpy()                                               # tree order
    amount, width, vel = _fields(sh, 2, 43, SPAN)
    for name, a in (("s", sh), ("a", amount), ("w", width), ("v", vel)):
        a.tofile(str(tmp_path / (name + ".f32")))
    exe = str(tmp_path / "dropin_spectra")
    _compile_dropin(exe)
    n_bins, v0, dv = 128, -32.0, 0.75
    res = subprocess.run([exe, str(tmp_path / "s.f32"), "4", str(tmp_path / "a.f32"), str(tmp_path / "w.f32"),
                          str(tmp_path / "v.f32"), "2", str(n_bins), repr(v0), repr(dv), repr(HUBBLE)],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    rays = gh.healpix_rays(4, (0.45, 0.55, 0.5), 1.0, device=cuda)
    got, got_col = _trace(gh, rays, d, tree, amount, width, vel, v0, dv, n_bins, True, HUBBLE)
    lines = dict(l.split()[:2] for l in res.stdout.splitlines() if l.startswith(("tau ", "column ")))
    assert int(lines["tau"], 16) == _fnv1a(got) and int(lines["column"], 16) == _fnv1a(got_col)
