"""Randomised differential test of the five traces added after tests/test_gpu_fuzz.py was written:
weighted column densities, float4 spheres with double outputs ("f4d"), emission-absorption,
absorption deposits and sightline spectra.  case(seed) draws scene size, leaf size, layout
(uniform / clustered with h over two decades / lattice with distance ties), frame (scale and
offset), bounds (given or computed), ray generator and count, every traversal knob, SPH kernel,
ordered budget, channel count, spectrum grid and context; the body builds it, calls every entry
point three times in a row (no cache, filling, validated cache: the same bits) and compares a
sample of the rays with the restatements of the modules that own the entry points, under their
tolerances.  The restatements are imported, not copied.

The samples: `sub` (about 128 rays) for hit counts, weighted sums, emission-absorption and the
transmitted luminosities; prefixes of it, cut where hits x channels pass a cap, for the restatements
whose cost grows with that product (spectra, deposits, the per-hit f4d outputs, which are a Python
loop over exact fractions).  f4d is compared under the cubic kernel, whose table its restatement
holds.

test_fuzz_cases_are_sharp (no GPU) asserts on the oracle alone that no case is empty and that the
seed list covers every value of every axis; rays whose generator has no CPU twin
(uniform_random_rays, plane_parallel_random_rays) are drawn there from NumPy with the same
distribution, and the twins of the generators that sort their rays return them unsorted, so the
sampled rays differ from the GPU's while their statistics do not; the GPU test asserts the same
sharpness on the rays it traced.

`python tests/test_gpu_fuzz_extensions.py FIRST LAST` runs the same loop over any seed range."""
import math
import os
import sys

import numpy as np
import pytest

F32, F64 = np.float32, np.float64

SEEDS = list(range(24))

N_SPHERES = [33, 150, 4095, 4096, 4097, 20000, 60000, 200000]
MAX_PER_LEAF = [1, 8, 32, 100]
LAYOUTS = ["uniform", "clustered", "lattice"]
SCALES = [1e-3, 1.0, 1e4]
BOUNDS = ["given", "computed"]
GENERATORS = ["axis", "pinhole", "healpix", "isotropic", "one_to_many", "plane_parallel"]
RAY_COUNTS = {32: (4, 8), 96: (8, 12), 2080: (40, 52), 3072: (48, 64)}     # count: a grid of that many
HEALPIX_NSIDE = {32: 2, 96: 4, 2080: 16, 3072: 16}                          # 12 nside^2 >= count, then cut
SPLITS = [-1, 1, 2, 4, 8]
WIDTHS = [-1, 64, 32, 16]
TREELETS = [-1, 0, 64, 512]
LATTICE_SPLITS = [0, 4, 8]
KERNELS = ["cubic", "other", "custom"]
OTHER_KERNELS = ["quartic", "quintic", "wendland_c2", "wendland_c4", "wendland_c6"]
BUDGETS = ["default", "one", "cut"]
CHANNELS = [1, 3, 4, 5, 64]
SPECTRA_MAX_CHANNELS = 16
N_BINS = [1, 63, 64, 200]
DEPTHS = ["thin", "medium", "block", "global"]      # hits per ray aimed at: see _radius
OPTICAL_DEPTHS = [0.02, 1.0, 40.0]
ENTRY_POINTS = ["weighted", "f4d", "emission_absorption", "spectra", "deposit"]
# Every axis whose values test_fuzz_cases_are_sharp counts, with the values it must see.
AXES = {"n": N_SPHERES, "max_per_leaf": MAX_PER_LEAF, "layout": LAYOUTS, "scale": SCALES, "bounds": BOUNDS,
        "generator": GENERATORS, "n_rays": list(RAY_COUNTS), "reorder": [False, True], "split": SPLITS,
        "width": WIDTHS, "treelet": TREELETS, "staging": [False, True], "lattice_split": LATTICE_SPLITS,
        "exact": [False, True], "kernel": KERNELS, "budget": BUDGETS, "channels": CHANNELS,
        "periodic": [False, True], "hubble": [False, True], "context": [False, True],
        "inside": [False, True], "offset": [False, True]}
N_SAMPLE, N_SAMPLE_FEW = 128, 512      # sampled rays; the larger where n <= 150 (few spheres: few hits a ray)
SPECTRA_CAP, DEPOSIT_CAP, F4D_CAP = 60_000, 1_500_000, 6_000


# ---- the configuration: a pure function of the seed ----------------------------------------------------
def case(seed):
    """One configuration, a pure function of the seed.  Touches no device.  The axes are stratified:
    every run of len(values) consecutive seeds holds each value of an axis once, in an order drawn
    per axis and run, so that a short seed list covers every value; the continuous parameters come
    from np.random.default_rng(seed)."""
    rng = np.random.default_rng(seed)

    def pick(axis, values):
        run, pos = divmod(seed, len(values))
        order = np.random.default_rng([sum(map(ord, axis)), run]).permutation(len(values))
        return values[int(order[pos])]
    c = {"seed": int(seed)}
    c["n"] = pick("n", N_SPHERES)
    c["max_per_leaf"] = pick("max_per_leaf", MAX_PER_LEAF)
    c["leaf"] = min(c["max_per_leaf"], c["n"] - 1)                         # clamped below n
    c["layout"] = pick("layout", LAYOUTS)
    c["scale"] = pick("scale", SCALES)
    c["offset"] = pick("offset", [False, True, True])
    c["origin"] = (rng.uniform(-1.5, 1.5, 3) * c["scale"]) if c["offset"] else np.zeros(3)
    c["bounds"] = pick("bounds", BOUNDS)
    c["generator"] = pick("generator", GENERATORS)
    c["budget"] = pick("budget", BUDGETS)
    counts = list(RAY_COUNTS)
    if c["n"] <= 150:
        counts = counts[2:]         # few spheres: only a large sample can hold 1000 hits
    elif c["budget"] == "one":
        counts = counts[:2]         # a batch per ray: the launches of thousands of batches are all one would time
    c["n_rays"] = pick("n_rays", counts)
    c["axis"], c["sense"] = int(rng.integers(0, 3)), (1 if rng.random() < 0.5 else -1)
    c["inside"] = pick("inside", [False, True])     # axis rays start inside the box
    c["geometry"] = rng.random(12)                  # the generator's own parameters: see _unit_rays
    c["ray_seed"] = int(rng.integers(1, 1 << 30))
    depths = DEPTHS[:2] + (DEPTHS[2:3] if c["n"] >= 4095 else []) + (DEPTHS[3:] if c["n"] >= 60000 else [])
    c["depth"] = pick("depth", depths)
    c["reorder"] = pick("reorder", [True, True, False])
    c["split"], c["width"], c["treelet"] = pick("split", SPLITS), pick("width", WIDTHS), pick("treelet", TREELETS)
    c["staging"] = pick("staging", [False, True])
    c["lattice_split"] = pick("lattice_split", LATTICE_SPLITS)
    c["exact"] = pick("exact", [False, True])
    c["kernel"] = pick("kernel", KERNELS)
    c["kernel_name"] = pick("kernel_name", OTHER_KERNELS) if c["kernel"] == "other" else c["kernel"]
    c["cut"] = int(rng.integers(5, 26))             # budget "cut": the call's hits / cut per batch
    c["channels"] = pick("channels", CHANNELS)
    c["n_bins"], c["periodic"], c["hubble"] = pick("n_bins", N_BINS), pick("periodic", [False, True]), \
        pick("hubble", [False, True])
    c["optical_depth"] = pick("optical_depth", OPTICAL_DEPTHS)
    c["context"] = pick("context", [True] + [False] * 7)
    R = c["n_rays"]
    k = N_SAMPLE if c["n"] > 150 else N_SAMPLE_FEW
    c["sub"] = np.arange(R) if R <= k else np.unique(rng.integers(0, R, k))
    c["scene_seed"] = int(rng.integers(1, 1 << 30))
    return c


def _radius(c):
    """The mean radius, in box lengths, that gives a ray crossing the box about T hits: T = n pi h^2.
    thin: enough that the sample holds 1000 hits with room; block / global: the ordered traces'
    middle and upper tiers (512 < hits <= 6144 < hits).  Rays that start inside the box see a
    fraction of it: T is raised for them.  Capped at 0.7 box lengths."""
    T = {"thin": max(30.0, 4000.0 / min(c["n_rays"], N_SAMPLE)), "medium": 150.0, "block": 1500.0,
         "global": 9000.0}[c["depth"]]
    if c["generator"] in ("healpix", "isotropic", "one_to_many") or (c["generator"] == "axis" and c["inside"]):
        T *= 2.5
    return min(math.sqrt(T / (c["n"] * math.pi)), 0.7)


def scene(c):
    """The spheres in the caller's order, float32 [n, 4], and the bounds to pass (None: computed)."""
    rng = np.random.default_rng(c["scene_seed"])
    n, h0 = c["n"], _radius(c)
    if c["layout"] == "uniform":
        u = rng.random((n, 3))
        h = h0 * rng.uniform(0.6, 1.4, n)
    elif c["layout"] == "clustered":
        # a third uniform, the rest in Gaussian blobs; h log-uniform over 2 decades (stratified: the
        # span is there for any n), its mean square, which sets the hits per ray, kept:
        # E[10^(-4 t)] = (1 - 1e-4) / (4 ln 10) = 0.1086
        n_blobs = int(rng.integers(3, 9))
        centre = rng.uniform(0.25, 0.75, (n_blobs, 3))
        sigma = 10.0 ** rng.uniform(-1.3, -0.6, n_blobs)
        which = rng.integers(0, n_blobs, n)
        u = centre[which] + rng.normal(size=(n, 3)) * sigma[which, None]
        free = rng.random(n) < 1.0 / 3.0
        u[free] = rng.random((int(free.sum()), 3))
        u = np.clip(u, 0.0, 1.0)
        h = min(h0 / math.sqrt(0.1086), 1.0) * 10.0 ** (-2.0 * rng.permutation(n) / (n - 1.0))
    else:
        # a lattice, most spheres exactly on its sites (equal coordinates: equal distances along axis
        # rays, whatever the frame), one in five off it
        g = int(math.ceil(n ** (1.0 / 3.0)))
        site = rng.permutation(g ** 3)[:n]
        u = (np.stack([site // (g * g), (site // g) % g, site % g], 1) + 0.5) / g
        off = rng.random(n) < 0.2
        u[off] += rng.uniform(-0.3, 0.3, (int(off.sum()), 3)) / g
        h = h0 * rng.uniform(0.8, 1.2, n)
    s = np.empty((n, 4), F32)
    s[:, :3] = (c["origin"][None, :] + c["scale"] * u).astype(F32)
    s[:, 3] = (c["scale"] * h).astype(F32)
    low, high = c["origin"], c["origin"] + c["scale"]
    return s, ((tuple(low), tuple(high)) if c["bounds"] == "given" else None)


def _unit_rays(c):
    """The generator's parameters in the unit frame."""
    g = c["geometry"]
    p = {}
    if c["generator"] == "axis":
        p["length"] = 0.5 + 0.8 * g[0]
    elif c["generator"] == "pinhole":
        v = np.array([g[0] - 0.5, g[1] - 0.5, g[2] - 0.5]); v /= np.linalg.norm(v) + 1e-9
        p["camera"] = 0.5 + (1.3 + 0.9 * g[3]) * v
        p["up"] = (0.1, 1.0, 0.2) if abs(v[1]) < 0.9 else (1.0, 0.1, 0.2)
        p["fovy"], p["length"] = 0.35 + 0.3 * g[4], 4.0
    elif c["generator"] in ("healpix", "isotropic", "one_to_many"):
        p["origin"] = 0.3 + 0.4 * g[:3]
        p["length"] = 0.5 + 0.7 * g[3]
    else:
        p["length"] = 1.3
    return p


def _frame(c, x):
    return c["origin"] + c["scale"] * np.asarray(x, F64)


def axis_rays(c):
    """nx x ny rays along +-axis over the box's face, starting outside or (each ray at its own
    depth) inside."""
    nx, ny = RAY_COUNTS[c["n_rays"]]
    rng = np.random.default_rng(c["ray_seed"])
    a, sense = c["axis"], c["sense"]
    perp = [k for k in range(3) if k != a]
    U, V = np.meshgrid((np.arange(nx) + 0.5) / nx, (np.arange(ny) + 0.5) / ny, indexing="ij")
    o = np.zeros((nx * ny, 3))
    o[:, perp[0]], o[:, perp[1]] = U.ravel(), V.ravel()
    start = rng.uniform(-0.1, 0.5, nx * ny) if c["inside"] else np.full(nx * ny, -0.1)
    o[:, a] = start if sense > 0 else 1.0 - start
    r = np.zeros((nx * ny, 7), F32)
    r[:, a] = sense
    r[:, 3:6] = _frame(c, o).astype(F32)
    r[:, 6] = F32(c["scale"] * _unit_rays(c)["length"])
    return r


def _points(c):
    rng = np.random.default_rng(c["ray_seed"])
    return _frame(c, rng.random((c["n_rays"], 3))).astype(F32)


def _plane(c):
    """base, w, h of a plane under the box whose normal w x h points into it."""
    a = c["axis"]
    w, h = np.zeros(3), np.zeros(3)
    w[(a + 1) % 3] = c["scale"]; h[(a + 2) % 3] = c["scale"]       # e_(a+1) x e_(a+2) = e_a
    base = np.zeros(3); base[a] = -0.1
    return _frame(c, base), w, h


def cpu_rays(c, O):
    """The case's rays without a device: the oracle's generators, or NumPy where there is no twin."""
    p, R, S = _unit_rays(c), c["n_rays"], c["scale"]
    as_rows = lambda rays: np.ascontiguousarray(rays).view(F32).reshape(-1, 7)
    rng = np.random.default_rng(c["ray_seed"])
    if c["generator"] == "axis":
        return axis_rays(c)
    if c["generator"] == "pinhole":
        nx, ny = RAY_COUNTS[R]
        return as_rows(O.pinhole_rays(nx, ny, _frame(c, p["camera"]), _frame(c, (0.5, 0.5, 0.5)), p["up"],
                                      p["fovy"], S * p["length"]))
    if c["generator"] == "one_to_many":
        return as_rows(O.one_to_many_rays(_frame(c, p["origin"]).astype(F32), _points(c)))
    if c["generator"] == "plane_parallel":
        nx, ny = RAY_COUNTS[R]
        base, w, h = _plane(c)
        i, j = np.arange(R) % nx, np.arange(R) // nx
        o = base + ((i + rng.random(R)) / nx)[:, None] * w + ((j + rng.random(R)) / ny)[:, None] * h
        d = np.cross(w, h); d /= np.linalg.norm(d)
    else:
        if c["generator"] == "healpix":
            d = O.healpix_dirs(HEALPIX_NSIDE[R])[:R]
        else:
            d = rng.normal(size=(R, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
        o = np.broadcast_to(_frame(c, p["origin"]), (R, 3))
    r = np.empty((R, 7), F32)
    r[:, :3], r[:, 3:6], r[:, 6] = np.asarray(d, F32), o.astype(F32), F32(S * p["length"])
    return r


def gpu_rays(c, gh, dev):
    import torch
    p, R, S = _unit_rays(c), c["n_rays"], c["scale"]
    nx, ny = RAY_COUNTS[R]
    if c["generator"] == "axis":
        return torch.from_numpy(axis_rays(c)).to(dev)
    if c["generator"] == "pinhole":
        return gh.pinhole_camera_rays(nx, ny, _frame(c, p["camera"]), _frame(c, (0.5, 0.5, 0.5)), p["up"],
                                      p["fovy"], S * p["length"], device=dev)
    if c["generator"] == "healpix":
        return gh.healpix_rays(HEALPIX_NSIDE[R], _frame(c, p["origin"]), S * p["length"], device=dev)[:R].contiguous()
    if c["generator"] == "isotropic":
        return gh.uniform_random_rays(R, _frame(c, p["origin"]), S * p["length"], seed=c["ray_seed"], device=dev)
    if c["generator"] == "one_to_many":
        return gh.one_to_many_rays(_frame(c, p["origin"]), torch.from_numpy(_points(c)).to(dev))
    base, w, h = _plane(c)
    return gh.plane_parallel_random_rays(nx, ny, base, w, h, S * p["length"], seed=c["ray_seed"], device=dev)


def kernel_table(c):
    import grace_hip as gh
    if c["kernel"] == "custom":
        from test_sph_kernels import _custom
        return _custom()
    return gh.sph_kernel_table(c["kernel_name"])


# ---- the reference side, shared by the CPU test and the GPU test ---------------------------------------
class Sample:
    pass


def sample(c, O, rays_h, sh):
    """The oracle's hits of rays_h[sub] on the tree-ordered spheres sh, with the active kernel's
    integrals, and the absorption that gives the median hit ray the case's optical depth."""
    from test_sph_kernels import b2_f32, hit_rays, integrals_f32
    m = Sample()
    m.rays = np.ascontiguousarray(rays_h[c["sub"]])
    off, idx, integ, dist = O.brute_hits(m.rays, sh)
    if c["kernel"] != "cubic":
        integ = integrals_f32(b2_f32(m.rays, sh, hit_rays(off, len(idx)), idx), sh[idx, 3], kernel_table(c))
    m.hits = (off, idx, integ, dist)
    m.counts = np.diff(np.append(off, len(idx))).astype(np.int64)
    m.ray = np.repeat(np.arange(len(m.rays)), m.counts)
    rng = np.random.default_rng([c["seed"], 7])
    xu = (sh[:, 0].astype(F64) - c["origin"][0]) / c["scale"]
    k0 = sh[:, 3].astype(F64) ** 2 * 10.0 ** (2.0 * (xu - 0.5)) * (0.5 + rng.random(len(sh)))
    tau0 = np.bincount(m.ray, k0[idx] * integ.astype(F64), len(m.rays))
    med = float(np.median(tau0[m.counts > 0])) if np.any(m.counts > 0) else 1.0
    m.absorption = (k0 * (c["optical_depth"] / med)).astype(F32)
    m.emission = (rng.random((len(sh), c["channels"])) * 4.0 - 2.0).astype(F32)
    return m


def prefix(m, cap, least=2):
    """How many of the sampled rays, from the first on, hold at most `cap` hits (at least `least`)."""
    return max(min(least, len(m.counts)), int(np.searchsorted(np.cumsum(m.counts), cap, side="right")))


def head(m, k):
    """The hits of the first k sampled rays."""
    off, idx, integ, dist = m.hits
    end = off[k] if k < len(off) else len(idx)
    return off[:k], idx[:end], integ[:end], dist[:end]


def sort_as_build_tree(c, O, s, bounds):
    """build_tree's order on the CPU: 30-bit keys over the given or the centroids' bounds, stable sort."""
    low, high = bounds if bounds is not None else O.centroid_bounds(s)
    return np.ascontiguousarray(O.sort_by_key(O.morton_keys30(s, low, high), s)[1])


def assert_sharp(c, m):
    assert np.mean(m.counts > 0) >= 0.25 and m.counts.sum() >= 1000, \
        (c["seed"], "an empty case", float(np.mean(m.counts > 0)), int(m.counts.sum()))


def tied_rays(m):
    """The sampled rays that have hits at bit-equal fp32 distance."""
    off, idx, integ, dist = m.hits
    key = m.ray.astype(np.int64) * (1 << 32) + dist.view(np.uint32)
    u, n = np.unique(key, return_counts=True)
    return np.unique(u[n > 1] >> 32)


# ---- CPU: the cases are sharp --------------------------------------------------------------------------
def test_fuzz_cases_are_sharp(oracle):
    """On the oracle alone: every committed seed gives a case whose sample has hits; the seed list
    holds every value of every axis at least twice, all three ordered tiers, distance ties whose
    tie-break matters, and optical depths below 0.1 and above 10."""
    import grace_hip as gh
    import test_emission_absorption as EA
    O = oracle
    w_max, b_max = gh.ordered_limits()
    assert (w_max, b_max) == (512, 6144)
    seen = {axis: {} for axis in AXES}
    pairs, tiers, tie_cases, tau_lo, tau_hi, done = set(), [0, 0, 0], 0, False, False, 0
    for seed in SEEDS:
        c = case(seed)
        s, bounds = scene(c)
        sh = sort_as_build_tree(c, O, s, bounds)
        rays_h = cpu_rays(c, O)
        assert len(rays_h) == c["n_rays"] and c["n_rays"] % 32 == 0 and c["leaf"] < c["n"]
        m = sample(c, O, rays_h, sh)
        assert_sharp(c, m)
        h = sh[:, 3] / c["scale"]
        if c["layout"] == "clustered":
            assert h.max() / h.min() > 10.0 ** 1.5
        for axis in AXES:
            seen[axis][c[axis]] = seen[axis].get(c[axis], 0) + 1
        pairs.update((e, c["generator"]) for e in ENTRY_POINTS)       # every seed runs every entry point
        tiers[0] += int(np.any(m.counts <= w_max))
        tiers[1] += int(np.any((m.counts > w_max) & (m.counts <= b_max)))
        tiers[2] += int(np.any(m.counts > b_max))
        ref, tau, S, n_r = EA.restate(len(m.rays), *m.hits, m.emission, m.absorption)
        hit = tau[n_r > 0]
        tau_lo |= bool(hit.min() < 0.1); tau_hi |= bool(hit.max() > 10.0)
        if c["layout"] == "lattice" and c["generator"] == "axis":
            tied = tied_rays(m)
            if len(tied):
                other, _, _, _ = EA.restate(len(m.rays), *m.hits, m.emission, m.absorption, reverse_ties=True)
                rel = np.abs(other - ref)[tied].max(1) / np.maximum(np.abs(ref)[tied].max(1), 1e-300)
                tie_cases += int(np.any(rel > 2.0 ** -20))       # the other tie-break is another answer
        done += 1
    assert done == len(SEEDS)                                        # no seed skipped, none returned early
    for axis, values in AXES.items():
        for v in values:
            assert seen[axis].get(v, 0) >= 2, (axis, v, seen[axis])
    assert pairs == {(e, g) for e in ENTRY_POINTS for g in GENERATORS}, pairs
    assert all(t > 0 for t in tiers), tiers
    assert tie_cases >= 1
    assert tau_lo and tau_hi
    print("sharp: tiers %s, tie cases %d" % (tiers, tie_cases))


# ---- GPU -----------------------------------------------------------------------------------------------
def _reset(gh):
    gh.set_ray_reorder(True); gh.set_packet_split(-1); gh.set_packet_width(-1); gh.set_treelet_size(-1)
    gh.set_hits_staging(True); gh.set_lattice_split(4); gh.set_exact_integrals(False)
    gh.set_sph_kernel("cubic"); gh.set_ordered_budget(0); gh.ordered_enable_stats(False)


def _same(a, b):
    import torch
    return all(x.dtype == y.dtype and x.shape == y.shape
               and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
               for x, y in zip(a, b))


def thrice(gh, call, what):
    """The call three times in a row from an empty cache -- no cache, filling, validated cache --
    each followed by the status word: the same bits.  Returns the first call's tensors."""
    gh.trace_release(); gh.trace_release_rays()
    got = []
    for _ in range(3):
        got.append(call())
        gh.trace_status()
    assert _same(got[0], got[1]) and _same(got[0], got[2]), (what, "the cache changed the result")
    return got[0]


def run_case(gh, O, dev, c):
    """Builds the case on the device, runs the five entry points and compares.  Returns the
    per-entry-point err / tol maxima where the owning module's check exposes them."""
    import torch
    import test_absorption_deposit as AD
    import test_emission_absorption as EA
    import test_mixed_precision as MP
    import test_spectra as SP
    import test_weighted_column_density as WC
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    what = {k: c[k] for k in ("seed", "n", "leaf", "layout", "generator", "n_rays", "kernel_name", "budget")}
    s, bounds = scene(c)
    d = up(s)
    tree = gh.Tree(c["n"], c["leaf"], device=dev)
    gh.build_tree(d, tree, *(bounds if bounds is not None else (None, None)))     # sorts d
    sh = d.cpu().numpy()
    assert np.array_equal(sh.view(np.uint32), sort_as_build_tree(c, O, s, bounds).view(np.uint32))
    rays = gpu_rays(c, gh, dev)
    R, n, C = len(rays), c["n"], c["channels"]
    assert R == c["n_rays"]
    rays_h, sub = rays.cpu().numpy(), c["sub"]
    sub_d = up(sub.astype(np.int64))
    m = sample(c, O, rays_h, sh)
    assert_sharp(c, m)
    ratios = {}

    gh.set_ray_reorder(c["reorder"]); gh.set_packet_split(c["split"]); gh.set_packet_width(c["width"])
    gh.set_treelet_size(c["treelet"]); gh.set_hits_staging(c["staging"]); gh.set_lattice_split(c["lattice_split"])

    # ---- f4d, under the cubic kernel ---------------------------------------------------------------
    def f4d():
        hc = torch.empty(R, dtype=torch.int32, device=dev)
        gh.trace_hitcounts_f4_f64(rays, d, tree, hc)
        cum = torch.empty(R, dtype=torch.float64, device=dev)
        gh.trace_cumulative_sph(rays, d, tree, cum)
        return (hc, cum) + tuple(gh.trace_sph(rays, d, tree, real=torch.float64))
    hc, cum, offs, idx, w, dist = thrice(gh, f4d, (what, "f4d"))
    hc_h, offs_h = hc.cpu().numpy(), offs.cpu().numpy()
    assert np.array_equal(hc_h[sub], O.brute_hitcounts_f4d(m.rays, sh)), (what, "f4d hit counts")
    assert np.array_equal(offs_h, np.concatenate([[0], np.cumsum(hc_h)[:-1]])) and len(idx) == hc_h.sum()
    kf = prefix(m, F4D_CAP, least=1)
    counts, per_ray = MP.restate(m.rays[:kf], sh, chunk=4)
    cum_h = cum[sub_d[:kf]].cpu().numpy()
    for j, (ri, rw, rd, w32) in enumerate(per_ray):
        a = int(offs_h[sub[j]]); b = a + int(hc_h[sub[j]])
        assert b - a == len(ri) and np.array_equal(idx[a:b].cpu().numpy(), ri), (what, "f4d indices", j)
        assert np.array_equal(w[a:b].cpu().numpy().view(np.uint64), rw.view(np.uint64)), (what, "f4d integrals", j)
        assert np.array_equal(dist[a:b].cpu().numpy().view(np.uint64), rd.astype(F64).view(np.uint64)), (what, "f4d distances", j)
        assert cum_h[j:j + 1].view(np.uint64)[0] == np.array([MP.class_sum(ri, w32)], F64).view(np.uint64)[0], \
            (what, "f4d column density", j)
    del offs, idx, w, dist

    # ---- the float hit counts: the call's total, for the cut budget ---------------------------------
    gh.set_sph_kernel(kernel_table(c) if c["kernel"] == "custom" else c["kernel_name"])
    hc = torch.empty(R, dtype=torch.int32, device=dev)
    gh.trace_hitcounts_sph(rays, d, tree, hc, check=True)
    assert np.array_equal(hc[sub_d].cpu().numpy(), m.counts), (what, "hit counts")
    total = int(hc.long().sum())

    # ---- weighted ------------------------------------------------------------------------------------
    gh.set_exact_integrals(c["exact"])
    wts = WC._weights(n, C, c["seed"] + 100, signed=c["exact"])
    wts_d = up(wts)
    got = thrice(gh, lambda: (gh.trace_cumulative_weighted_sph(rays, d, tree, wts_d),), (what, "weighted"))[0]
    got = got.reshape(R, -1)[sub_d].cpu().numpy()
    ref32, ref64, abs64 = WC.restate(len(m.rays), m.hits[0], m.hits[1], m.hits[2], wts)
    if c["exact"]:
        assert np.array_equal(got.view(np.uint32), ref32.view(np.uint32)), (what, "weighted, exact")
    else:
        atol = 2e-6 * kernel_table(c)[0] / float(sh[:, 3].min()) ** 2 * float(np.abs(wts).max())
        err, tol = np.abs(got.astype(F64) - ref64), 1e-5 * abs64 + atol
        ratios["weighted"] = float(np.max(err / tol))
        assert np.all(err <= tol), (what, "weighted, fast", ratios["weighted"])
    gh.set_exact_integrals(False)

    # ---- the ordered traces ----------------------------------------------------------------------------
    gh.ordered_enable_stats(True)
    gh.set_ordered_budget({"default": 0, "one": 1, "cut": 12 * max(1, -(-total // c["cut"]))}[c["budget"]])

    def batches_are_as_drawn(name):
        st = gh.ordered_last_stats()
        assert st["total_hits"] == total, (what, name, st)
        if c["budget"] == "default":
            assert st["batches"] == (1 if 12 * total <= 1 << 30 else st["batches"]), (what, name, st)
        else:
            assert st["batches"] >= (5 if c["budget"] == "cut" else int((hc_f > 0).sum())), (what, name, st)
    hc_f = hc.cpu().numpy()

    em_d, ab_d = up(m.emission), up(m.absorption)

    def ea():
        tau = torch.empty(R, dtype=torch.float32, device=dev)
        return gh.trace_emission_absorption_sph(rays, d, tree, em_d, ab_d, tau=tau), tau
    out, tau = thrice(gh, ea, (what, "emission-absorption"))
    batches_are_as_drawn("emission-absorption")
    ref, rtau, S, n_r = EA.restate(len(m.rays), *m.hits, m.emission, m.absorption)
    got, got_tau = out.reshape(R, -1)[sub_d].cpu().numpy(), tau[sub_d].cpu().numpy()
    ratios["emission_absorption"] = float(np.max(np.abs(got.astype(F64) - ref) / EA.bound(ref, S, n_r, rtau)))
    EA.check(got, got_tau, ref, rtau, S, n_r, "seed %d emission-absorption" % c["seed"])
    assert np.all(got[n_r == 0] == 0) and np.all(got_tau[n_r == 0] == 0)

    # spectra: at most 16 channels, a prefix of the sample
    Cs = min(C, SPECTRA_MAX_CHANNELS)
    ks = prefix(m, SPECTRA_CAP // Cs)
    amount, width, vel = SP._fields(sh, Cs, c["seed"] + 200, SP.SPAN, signed=True)
    hubble_unit = SP.HUBBLE if c["hubble"] else 0.0
    v0, dv = SP._grid(c["n_bins"], c["periodic"], hubble_unit)
    hubble = hubble_unit / c["scale"]                  # velocities as in the unit frame
    am_d, wi_d, ve_d = up(amount), up(width), up(vel)

    def spectra():
        col = torch.empty((R, Cs), dtype=torch.float32, device=dev)
        return gh.trace_spectra_sph(rays, d, tree, am_d, wi_d, ve_d, v0, dv, c["n_bins"], periodic=c["periodic"],
                                    hubble=hubble, column=col), col
    stau, scol = thrice(gh, spectra, (what, "spectra"))
    batches_are_as_drawn("spectra")
    sref = SP.restate(m.rays[:ks], head(m, ks), amount, width, vel, v0, dv, c["n_bins"], c["periodic"], hubble)
    got, got_col = stau[sub_d[:ks]].cpu().numpy(), scol[sub_d[:ks]].cpu().numpy()
    ratios["spectra"] = float(np.max(np.abs(got.astype(F64) - sref[0]) / sref[1]))
    SP.check(got, got_col, *sref, what="seed %d spectra" % c["seed"])
    del stau

    # deposits: transmitted on the sample ...
    rng = np.random.default_rng([c["seed"], 11])
    L = (10.0 ** (3.0 * rng.random((R, C))) * np.where(rng.random((R, C)) < 0.5, -1.0, 1.0)).astype(F32)
    k = (m.absorption.astype(F64)[:, None] * (0.75 + 0.5 * rng.random((1, C)))).astype(F32)
    L_d, k_d = up(L), up(k)

    def deposit(r=rays, lum=L_d):
        tr = torch.empty((len(r), C), dtype=torch.float32, device=dev)
        q = torch.empty(C, dtype=torch.float64, device=dev)
        return gh.trace_absorption_deposit_sph(r, d, tree, lum, k_d, transmitted=tr, quantum=q), tr, q
    dep, tr, q = thrice(gh, deposit, (what, "deposit"))
    batches_are_as_drawn("deposit")
    kd = prefix(m, DEPOSIT_CAP // C)
    Rf = AD.restate(kd, n, *head(m, kd), L[sub[:kd]], k)
    assert np.array_equal(q.cpu().numpy().view(np.uint64), AD.quantum(L, R).view(np.uint64)), (what, "quantum")
    terr, ttol = np.abs(tr[sub_d[:kd]].cpu().numpy().astype(F64) - Rf.trans), AD.transmitted_bound(Rf)
    ratios["transmitted"] = float(np.max(terr / ttol))
    assert np.all(terr <= ttol), (what, "transmitted", ratios["transmitted"])
    del dep
    # ... and the deposit itself on a call of those rays alone, padded with rays that miss the box,
    # so that the oracle holds every hit
    pad = (-kd) % 32
    away = np.zeros((pad, 7), F32)
    away[:, 2] = 1.0; away[:, 3:6] = _frame(c, (0.5, 0.5, 50.0)).astype(F32); away[:, 6] = F32(c["scale"])
    rays2_h = np.concatenate([m.rays[:kd], away])
    assert O.brute_hitcounts(away, sh).sum() == 0 if pad else True
    rays2, L2 = up(rays2_h), L[:kd + pad]
    L2_d = up(L2)
    gh.set_ordered_budget(0 if c["budget"] == "default" else 1 if c["budget"] == "one"
                          else 12 * max(1, int(m.counts[:kd].sum()) // c["cut"]))
    got = tuple(t.cpu().numpy() for t in thrice(gh, lambda: deposit(rays2, L2_d), (what, "deposit, sampled rays")))
    off2 = np.concatenate([head(m, kd)[0], np.full(pad, len(head(m, kd)[1]), np.int32)])
    R2 = AD.restate(kd + pad, n, off2, *head(m, kd)[1:], L2, k)
    AD.check(got, R2, "seed %d deposit" % c["seed"])
    tol = AD.deposit_bound(R2)
    ok = tol > 0
    ratios["deposit"] = float(np.max(np.abs(got[0] - R2.dep)[ok] / tol[ok])) if ok.any() else 0.0
    # photons are conserved (test_photons_are_conserved's bound)
    Lsum = L2.astype(F64).sum(0)
    err = np.abs(got[0].sum(0) + got[1].astype(F64).sum(0) - Lsum)
    tol = AD.deposit_bound(R2).sum(0) + AD.transmitted_bound(R2).sum(0) + (n + kd + pad) * 2.0 ** -53 * (
        np.abs(got[0]).sum(0) + np.abs(got[1].astype(F64)).sum(0) + np.abs(L2.astype(F64)).sum(0))
    assert np.all(err <= tol), (what, "conservation", err, tol)
    print("seed %d ratios %s" % (c["seed"], {k_: "%.3g" % v for k_, v in ratios.items()}))
    return ratios


def run_seed(gh, O, dev, seed):
    """One seed, in a context of its own on its own stream where the case says so; knobs restored."""
    import torch
    c = case(seed)
    ctx = stream = None
    try:
        if c["context"]:
            torch.cuda.synchronize()
            stream, ctx = torch.cuda.Stream(), gh.Context()
            ctx.make_current()
            with torch.cuda.stream(stream):
                try:
                    return run_case(gh, O, dev, c)
                finally:
                    _reset(gh)
                    stream.synchronize()
        return run_case(gh, O, dev, c)
    finally:
        if ctx is not None:
            gh.Context.reset_current()
            ctx.destroy()
        _reset(gh)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_random_configuration(gh, oracle, cuda, seed):
    run_seed(gh, oracle, cuda, seed)


def main(first, last):
    """The same loop over any seed range, for a wider offline run: prints failures and the largest
    err / tol per entry point."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for p in (os.path.join(root, "grace-devel_amd"), os.path.join(root, "oracle"), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import grace_hip as gh
    import oracle as O
    O.build()
    gh.set_sort_overflow_hint(False)
    dev, worst, bad = torch.device("cuda:0"), {}, 0
    for seed in range(first, last):
        try:
            for k, v in run_seed(gh, O, dev, seed).items():
                worst[k] = max(worst.get(k, 0.0), v)
        except AssertionError as e:
            bad += 1
            print("FAIL seed", seed, str(e)[:400], flush=True)
    print("done: %d configurations, %d failures, largest err / tol %s" % (last - first, bad, worst))
    return bad


if __name__ == "__main__":
    sys.exit(1 if main(int(sys.argv[1]), int(sys.argv[2])) else 0)
