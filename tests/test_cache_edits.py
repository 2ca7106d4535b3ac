"""Cached trace records against one-word edits made in place.

include/grace_hip.h, "Cached trace records": a context keeps the records of the scene and of the ray
batch it was last given, validates them by signature before every use, and *results are always
those of a fresh derivation*.  Every test here warms a context's caches, changes one or two 32-bit
words of ONE device array in place (tests/cache_edit_cases.py: at the signature pass's chunk, stride
and alignment edges, and where the ray extents change), and holds the next call against brute force
on the arrays as they are now, against a context that has never seen them, and against the warm
result, which it must no longer equal.  Then the edit is undone: the signature returns to a value
the cache has held before, and the bits must be the warm ones.

The edited scenes stay valid without a rebuild (a radius shrinks, a triangle collapses inside its
box, the last leaf gives up its last sphere: a tree over a prefix of the array).  Edits to `nodes`
alone, the fp64 and mixed modes, the periodic traces and the point queries are out of scope: see
cache_edit_cases.py.

Where the warm and the new result must differ: on every ray whose hit count changes (hit counts,
per-hit outputs, closest triangle).  A sum of fp32 terms need not change its bits when a grazing
hit (a term far below half an ulp of the sum) comes or goes, so the float families must differ on
the affected rays whose reference value moves by more than 1e-4 of itself -- at least one per case,
in practice nearly all."""
import numpy as np
import pytest
import torch

import cache_edit_cases as K
from conftest import check_column_densities
from test_trace_boundaries import _check_hits
from test_trace_plan_boundaries import _from_plan

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
F0 = 1.91            # the kernel table's first entry, rounded up


def _reset(gh):
    gh.set_ray_reorder(True); gh.set_packet_split(-1); gh.set_packet_width(-1); gh.set_treelet_size(-1)
    gh.set_exact_integrals(False); gh.set_plan(True); gh.set_cache_auto(True); gh.set_cache_validation(True)
    gh.set_ordered_budget(0); gh.ordered_enable_stats(False)
    gh.trace_release(); gh.trace_release_rays()


def _same(a, b):
    """Two results (tuples of tensors) bit for bit."""
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8),
                                                                       y.contiguous().view(torch.uint8))
                                    for x, y in zip(a, b))


def _rows_differ(a, b):
    """Per row of two [n, ...] arrays: any bit differs."""
    a = np.ascontiguousarray(a).reshape(len(a), -1); b = np.ascontiguousarray(b).reshape(len(b), -1)
    return (a.view(np.uint8) != b.view(np.uint8)).any(axis=1)


def _apply(arrays, edit):
    """The edit on the device, on the current stream: one fill kernel a word, no synchronisation."""
    flat = arrays[edit.array].view(torch.int32).reshape(-1)
    assert flat.data_ptr() == arrays[edit.array].data_ptr()
    for w, v in zip(edit.words, edit.new):
        flat[w] = v - (1 << 32) if v >= (1 << 31) else v


def _addresses(arrays):
    return {k: (t.data_ptr(), t.numel()) for k, t in arrays.items()}


# ---- device arrays -------------------------------------------------------------------------------------
class _Spheres:
    """A scene of cache_edit_cases on the device.  Its spheres are in tree order already: the build
    leaves every sphere where it is (asserted), so the module's sorted indices hold here."""

    def __init__(self, gh, cuda, scene):
        self.scene, self.host = scene, scene.spheres
        self.d = torch.from_numpy(scene.spheres.copy()).to(cuda)
        self.tree, perm = gh.build_tree(self.d, gh.Tree(len(self.host), scene.mpl, device=cuda), *K.UNIT, want_perm=True)
        perm = perm.cpu().numpy().astype(np.int64)
        for name, j in scene.probes.items():
            assert perm[j] == j, ("the build moved probe", name)
        assert np.array_equal(self.d.cpu().numpy().view(np.uint32), self.host.view(np.uint32))
        self.leaves0 = self.tree.leaves.clone()
        assert int(self.leaves0[-1, 0] + self.leaves0[-1, 1]) == len(self.host) and int(self.leaves0[0, 0]) == 0
        assert int(self.leaves0[-1, 1]) > 1, "the last leaf holds one sphere: it cannot be cut"

    def restore(self):
        self.d.copy_(torch.from_numpy(self.host.copy())); self.tree.leaves.copy_(self.leaves0)

    def now(self):
        """The spheres the tree covers, as they are on the device now."""
        last = self.tree.leaves[-1].cpu().numpy()
        return self.d.cpu().numpy()[: int(last[0] + last[1])]

    def arrays(self, rays):
        return {"spheres": self.d, "leaves": self.tree.leaves, "rays": rays}


@pytest.fixture(scope="module")
def small_dev(gh, cuda):
    return _Spheres(gh, cuda, K.small())


@pytest.fixture(scope="module")
def wide_dev(gh, cuda):
    return _Spheres(gh, cuda, K.wide())


def _rays_on(cuda, host, k=0):
    """The batch as the view pool[k:] of a pool of k more rows: k * 28 bytes from an aligned base."""
    pool = torch.empty((len(host) + k, K.RAY_WORDS), dtype=torch.float32, device=cuda)
    view = pool[k:]
    view.copy_(torch.from_numpy(np.array(host)))
    assert pool.data_ptr() % 16 == 0 and view.is_contiguous()
    assert view.data_ptr() - pool.data_ptr() == K.view_offset_bytes(k, K.RAY_WORDS)
    assert (view.data_ptr() % 16 == 0) == (k == 0)
    return view


# ---- families: a trace call, its brute-force check on `sub`, its per-ray value ----------------------------
class _Family:
    integer = False          # its per-ray value changes with every change of a ray's hits
    reorder = True

    def __init__(self, gh, O, cuda, S, rays, sub):
        self.gh, self.O, self.cuda, self.S, self.rays, self.sub = gh, O, cuda, S, rays, np.asarray(sub)
        self.R = len(rays)
        self.prepare()

    def prepare(self):
        pass

    def setup(self):
        """This family's knobs, in the current context."""
        self.gh.set_ray_reorder(self.reorder)
        self.knobs()

    def knobs(self):
        pass

    def per_ray(self, out):
        return out[0].cpu().numpy()

    def _sub(self):
        return self.rays.cpu().numpy()[self.sub], self.S.now()


class Counts(_Family):
    integer = True

    def call(self):
        out = torch.empty(self.R, dtype=torch.int32, device=self.cuda)
        self.gh.trace_hitcounts_sph(self.rays, self.S.d, self.S.tree, out, check=True)
        return (out,)

    def check(self, out):
        ref = self.O.brute_hitcounts(*self._sub())
        got = out[0].cpu().numpy()[self.sub]
        assert np.array_equal(got, ref), (self.sub[got != ref][:5], got[got != ref][:5], ref[got != ref][:5])
        return ref


class CountsCApi(Counts):
    """Through the C entry point, which takes any ray count (include/grace_hip.h)."""

    def call(self):
        gh = self.gh
        out = torch.full((self.R,), -7, dtype=torch.int32, device=self.cuda)
        gh._check(gh._lib.grace_trace_hitcounts_f4(*gh._trace_args(self.rays, self.S.d, self.S.tree), gh._ptr(out),
                                                   gh._stream()))
        gh.trace_status()
        return (out,)


class Cumulative(_Family):
    exact = True

    def knobs(self):
        self.gh.set_exact_integrals(self.exact)

    def call(self):
        out = torch.empty(self.R, dtype=torch.float32, device=self.cuda)
        self.gh.trace_cumulative_sph(self.rays, self.S.d, self.S.tree, out, check=True)
        return (out,)

    def check(self, out):
        rr, ss = self._sub()
        c32, c64 = self.O.brute_cumulative(rr, ss)
        check_column_densities(out[0].cpu().numpy()[self.sub], c32, c64, "exact" if self.exact else "fast",
                               F0 / float(ss[:, 3].min()) ** 2)
        return c64


class CumulativeFast(Cumulative):
    exact = False


class CumulativeCApi(Cumulative):
    """Exact column densities through the C entry point (any ray count, as for the hit counts)."""

    def call(self):
        gh = self.gh
        out = torch.full((self.R,), -7.0, dtype=torch.float32, device=self.cuda)
        gh._check(gh._lib.grace_trace_cumulative_f4(*gh._trace_args(self.rays, self.S.d, self.S.tree), gh._ptr(out),
                                                    gh._stream()))
        gh.trace_status()
        return (out,)


class Weighted(_Family):
    def prepare(self):
        self.w = np.random.default_rng(17).uniform(-2, 2, (len(self.S.host), 3)).astype(F32)
        self.w_dev = torch.from_numpy(self.w).to(self.cuda)

    def knobs(self):
        self.gh.set_exact_integrals(True)

    def call(self):
        return (self.gh.trace_cumulative_weighted_sph(self.rays, self.S.d, self.S.tree, self.w_dev, check=True),)

    def check(self, out):
        from test_weighted_column_density import restate
        rr, ss = self._sub()
        ro, ri, rw, _ = self.O.brute_hits(rr, ss)
        ref32 = restate(len(self.sub), ro, ri, rw, self.w)[0]
        got = out[0].cpu().numpy()[self.sub]
        assert np.array_equal(got.view(np.uint32), ref32.view(np.uint32))
        return ref32.astype(F64)


class Hits(_Family):
    integer = True

    def call(self):
        return tuple(self.gh.trace_sph(self.rays, self.S.d, self.S.tree))

    def per_ray(self, out):
        return np.diff(np.append(out[0].cpu().numpy(), len(out[1])))

    def check(self, out):
        rr, ss = self._sub()
        ref = self.O.brute_hits(rr, ss)
        _check_hits(out, ref, self.sub, F32)
        return np.diff(np.append(ref[0], len(ref[1])))


class Sentinels(Hits):
    SENT = (-9, -1.5, 7.25)

    def call(self):
        return tuple(self.gh.trace_with_sentinels_sph(self.rays, self.S.d, self.S.tree, *self.SENT))

    def _strip(self, out):
        """The sentinel slot that ends every ray's segment checked and taken out: trace_sph's layout."""
        offs, idx, w, dist = (t.cpu().numpy() for t in out)
        end = np.append(offs[1:], len(idx)) - 1
        assert np.all(end >= offs)
        assert np.all(idx[end] == self.SENT[0]) and np.all(w[end] == F32(self.SENT[1])) and np.all(dist[end] == F32(self.SENT[2]))
        keep = np.ones(len(idx), bool); keep[end] = False
        return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in
                     ((offs - np.arange(len(offs))).astype(np.int32), idx[keep], w[keep], dist[keep]))

    def per_ray(self, out):
        return Hits.per_ray(self, self._strip(out))

    def check(self, out):
        return Hits.check(self, self._strip(out))


class _Ordered(_Family):
    batched = False

    def prepare(self):
        self.fields()
        if self.batched:       # a budget of a seventh of the batch's hits: at least five batches, mostly seven
            total = int(self.O.brute_hitcounts(self.rays.cpu().numpy(), self.S.now()).sum())
            self.budget = 12 * total // 7

    def knobs(self):
        if self.batched:
            self.gh.ordered_enable_stats(True); self.gh.set_ordered_budget(self.budget)

    def after_call(self):
        if self.batched:       # the per-batch nested walks each meet the scene cache
            assert self.gh.ordered_last_stats()["batches"] >= 5, self.gh.ordered_last_stats()

    def _t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.cuda)


class EmissionAbsorption(_Ordered):
    def fields(self):
        from test_emission_absorption import _coefficients
        self.e, self.k = _coefficients(self.S.host, 3, 41)
        self.e_dev, self.k_dev = self._t(self.e), self._t(self.k)

    def call(self):
        tau = torch.empty(self.R, dtype=torch.float32, device=self.cuda)
        out = self.gh.trace_emission_absorption_sph(self.rays, self.S.d, self.S.tree, self.e_dev, self.k_dev, tau=tau,
                                                    check=True)
        self.after_call()
        return (out, tau)

    def check(self, out):
        from test_emission_absorption import check, restate
        rr, ss = self._sub()
        ref, tau, S, n_r = restate(len(self.sub), *self.O.brute_hits(rr, ss), self.e, self.k)
        check(out[0].cpu().numpy()[self.sub], out[1].cpu().numpy()[self.sub], ref, tau, S, n_r, "cache edit")
        return ref


class AbsorptionDeposit(_Ordered):
    """(The deposit sums over every ray: its reference takes brute force on the whole batch.)"""

    def fields(self):
        from test_absorption_deposit import _coefficients
        self.L, self.k = _coefficients(self.S.host, self.R, 2, 43)
        self.L_dev, self.k_dev = self._t(self.L), self._t(self.k)

    def call(self):
        tr = torch.empty((self.R, 2), dtype=torch.float32, device=self.cuda)
        q = torch.empty(2, dtype=torch.float64, device=self.cuda)
        dep = self.gh.trace_absorption_deposit_sph(self.rays, self.S.d, self.S.tree, self.L_dev, self.k_dev,
                                                   transmitted=tr, quantum=q, check=True)
        self.after_call()
        return (tr, dep, q)

    def check(self, out):
        from test_absorption_deposit import check, restate
        rr, ss = self.rays.cpu().numpy(), self.S.now()
        R = restate(self.R, len(self.S.host), *self.O.brute_hits(rr, ss), self.L, self.k)
        check((out[1].cpu().numpy(), out[0].cpu().numpy(), out[2].cpu().numpy()), R, "cache edit")
        return R.trans[self.sub]


class Spectra(_Ordered):
    N_BINS = 64

    def fields(self):
        from test_spectra import HUBBLE, SPAN, _fields, _grid
        self.amount, self.width, self.vel = _fields(self.S.host, 2, 47, SPAN, signed=True)
        self.grid = _grid(self.N_BINS, False, HUBBLE) + (self.N_BINS, False, HUBBLE)
        self.dev = [self._t(a) for a in (self.amount, self.width, self.vel)]

    def call(self):
        v0, dv, n_bins, periodic, hubble = self.grid
        col = torch.empty((self.R, 2), dtype=torch.float32, device=self.cuda)
        tau = self.gh.trace_spectra_sph(self.rays, self.S.d, self.S.tree, *self.dev, v0, dv, n_bins, periodic=periodic,
                                        hubble=hubble, column=col, check=True)
        self.after_call()
        return (col, tau)

    def check(self, out):
        from test_spectra import check, restate
        rr, ss = self._sub()
        ref = restate(rr, self.O.brute_hits(rr, ss), self.amount, self.width, self.vel, *self.grid)
        check(out[1].cpu().numpy()[self.sub], out[0].cpu().numpy()[self.sub], *ref, what="cache edit")
        return ref[2]


def _batched(cls):
    return type(cls.__name__ + "Batched", (cls,), {"batched": True})


FAMILIES = {"counts": Counts, "exact": Cumulative, "fast": CumulativeFast, "weighted": Weighted, "trace_sph": Hits,
            "sentinels": Sentinels, "emission_absorption": EmissionAbsorption, "absorption_deposit": AbsorptionDeposit,
            "spectra": Spectra, "emission_absorption-batched": _batched(EmissionAbsorption),
            "absorption_deposit-batched": _batched(AbsorptionDeposit), "spectra-batched": _batched(Spectra)}


# ---- the protocol ----------------------------------------------------------------------------------------
def _fresh(gh, fam, back_to):
    """The family's call as a context that has never seen the arrays makes it."""
    with gh.Context():
        try:
            fam.setup()
            out = fam.call()
            torch.cuda.synchronize()
        finally:
            _reset(gh)
    back_to.make_current()
    fam.setup()              # (the ordered traces' budget and stats hook are process-wide: set again)
    return out


def _must_differ(fam, affected, key0, key1, warm, got, what):
    """(c): the new result differs from the warm one on every affected ray (see the module docstring)."""
    pos = {int(r): k for k, r in enumerate(fam.sub)}
    assert all(int(r) in pos for r in affected)
    k = np.array([pos[int(r)] for r in affected], np.int64)
    a, b = np.asarray(key0, F64).reshape(len(fam.sub), -1)[k], np.asarray(key1, F64).reshape(len(fam.sub), -1)[k]
    if fam.integer:
        must = np.ones(len(k), bool)
        assert np.all((a != b).any(axis=1)), (what, "the reference does not change on an affected ray")
    else:
        must = (np.abs(a - b) > 1e-4 * np.maximum(np.abs(a), np.abs(b))).any(axis=1)
    assert must.sum() >= 1, (what, "no affected ray changes the reference")
    differs = _rows_differ(fam.per_ray(got), fam.per_ray(warm))[np.asarray(affected, np.int64)]
    assert np.all(differs[must]), (what, "yesterday's result on rays", np.asarray(affected)[must & ~differs][:8])


def _edit_cycle(gh, fam, arrays, edit, affected, what, warm=None, after=None):
    """Warm, edit, call, call again, revert -- in a context of its own.  warm: how the caches are
    warmed (default: three calls, all equal); after(stage): further assertions after the call
    of stage "warm", "edit", "again" or "revert"."""
    after = after or (lambda stage: None)
    ctx = gh.Context()
    ctx.make_current()
    try:
        fam.setup()
        # 1. warm
        if warm is None:
            outs = [fam.call() for _ in range(3)]
            assert _same(outs[0], outs[1]) and _same(outs[0], outs[2]), what
            w = outs[2]
        else:
            w = warm()
        gh.trace_status()
        key0 = fam.check(w)
        after("warm")
        where = _addresses(arrays)
        # 2. edit: same pointers, same sizes, nothing between the edit and the call
        _apply(arrays, edit)
        assert _addresses(arrays) == where
        # 3. call
        got = fam.call()
        gh.trace_status()
        after("edit")
        key1 = fam.check(got)                                                        # (a) brute force, now
        assert _same(got, _fresh(gh, fam, ctx)), (what, "differs from a fresh context")   # (b)
        _must_differ(fam, affected, key0, key1, w, got, what)                        # (c)
        # 4. again: the re-derived records are the cached ones now
        again = fam.call()
        gh.trace_status()
        assert _same(again, got), (what, "second call after the edit")
        after("again")
        # 5. revert: A -> B -> A
        _apply(arrays, edit.inverse())
        assert _addresses(arrays) == where
        back = fam.call()
        gh.trace_status()
        assert _same(back, w), (what, "after the revert")
        after("revert")
    finally:
        _reset(gh)
        gh.Context.reset_current()
        ctx.destroy()


def _cycle_guarded(S, *args, **kw):
    try:
        _edit_cycle(*args, **kw)
    finally:
        S.restore()


# ---- tests -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FAMILIES))
def test_one_sphere_shrunk_in_place(gh, oracle, cuda, small_dev, family):
    """One radius of ~3000 times a quarter, at sorted index 0, in the middle and at n - 1, under
    every trace call that may run on cached scene records; the ordered traces also in at least five
    batches, whose nested per-hit walks meet the cache one after the other."""
    S = small_dev
    rays = _rays_on(cuda, K.batch("full4096"))
    for probe in ("first", "mid", "last"):
        c = K.sphere_case("small", "full4096", probe)
        fam = FAMILIES[family](gh, oracle, cuda, S, rays, c.sub)
        _cycle_guarded(S, gh, fam, S.arrays(rays), c.edit, c.affected, (family, probe))


STRIDE_CASES = [("wide", p) for p in ("first", "stride_end", "stride_begin", "last")] + \
    [("rays", "straddle"), ("rays", "last")]


@pytest.mark.parametrize("family", ["counts", "exact"])
@pytest.mark.parametrize("what,where", STRIDE_CASES, ids=["-".join(c) for c in STRIDE_CASES])
def test_edits_at_the_signatures_strides(gh, oracle, cuda, small_dev, wide_dev, what, where, family):
    """The signature kernel's 262144 threads take an array's chunks in grid-stride iterations.
    wide: 262144 + 64 spheres, one radius changed in the first chunk, in the last chunk of the first
    iteration, in the first chunk of the second and in the last chunk.  rays: 388 x 388 rays (padded
    to 150560) over the small scene; ray 149796 straddles chunks 262143 and 262144 of the ray array,
    and its oy -- word 0 of the second iteration's first chunk -- moves it across the rectangle;
    likewise the last ray, in the array's last chunk."""
    if what == "wide":
        S, c = wide_dev, K.sphere_case("wide", "full4096", where)
    else:
        case = ("z388", "inside", K.STRADDLE_RAY, K.STRADDLE_WORD) if where == "straddle" else ("z388", "inside", -1, K.OX)
        S, c = small_dev, K.ray_case("small", *case)
    rays = _rays_on(cuda, c.rays)
    fam = FAMILIES[family](gh, oracle, cuda, S, rays, c.sub)
    _cycle_guarded(S, gh, fam, S.arrays(rays), c.edit, c.affected, (what, where, family))


@pytest.mark.parametrize("reorder", [True, False], ids=["reordered", "caller-order"])
@pytest.mark.parametrize("scene", ["small", "wide"])
def test_last_leaf_cut_in_place(gh, oracle, cuda, small_dev, wide_dev, scene, reorder):
    """leaves[n_nodes].y -= 1: one word in the last chunk of the third array of the scene group.  The
    tree then covers spheres[:n - 1]; the flat group passes read that bound from the cached C."""
    S = small_dev if scene == "small" else wide_dev
    rays = _rays_on(cuda, K.batch("full4096"))
    c = K.sphere_case(scene, "full4096", "cut")
    edit = K.cut_last_leaf(S.tree.leaves.cpu().numpy())
    assert edit.chunks == [S.tree.n_nodes]
    for family in ("counts", "exact", "trace_sph"):
        fam = FAMILIES[family](gh, oracle, cuda, S, rays, c.sub)
        fam.reorder = reorder
        _cycle_guarded(S, gh, fam, S.arrays(rays), edit, c.affected, (scene, family, reorder))


@pytest.mark.parametrize("view", [0, 1, 2, 3], ids=lambda k: "aligned" if k == 0 else "pool[%d:]" % k)
@pytest.mark.parametrize("batch", K.MOVED_BATCHES)
def test_one_ray_moved(gh, oracle, cuda, small_dev, batch, view):
    """One ray of a batch under the lattice kernel moves across the rectangle (extents unchanged),
    beyond it (extents grow), or turns oblique (no lattice any more): one and two gated sort passes,
    an aligned ray array and the three unaligned views, whose every chunk is read word by word."""
    S = small_dev
    rays = _rays_on(cuda, K.batch(batch), view)
    for kind in ("inside", "outside", "tilt"):
        for i, coord in K.MOVED_RAYS[batch]:
            c = K.ray_case("small", batch, kind, i, coord)
            for family in ("counts", "exact", "fast"):
                fam = FAMILIES[family](gh, oracle, cuda, S, rays, c.sub)

                def after(stage, kind=kind):
                    lat = gh.last_lattice()
                    if stage in ("warm", "revert"):
                        assert lat == 1, (stage, "the case is about the lattice kernel's use of the extents")
                    elif kind == "tilt":
                        assert lat == 0, (stage, "an oblique ray under the lattice kernel")
                _cycle_guarded(S, gh, fam, S.arrays(rays), c.edit, c.affected, (batch, view, kind, i, family), after=after)


@pytest.mark.parametrize("family", ["exact", "weighted"])
def test_one_ray_moved_under_a_plan(gh, oracle, cuda, small_dev, family):
    """The same ray edits and one shrunk sphere under a packet plan: the call that notices records
    the plan again in place (or, if the new lists outgrow their room, falls back -- correct either
    way); an oblique ray makes the batch unplannable until it is undone."""
    S = small_dev
    rays = _rays_on(cuda, K.batch("z4096"))
    cases = [(kind, K.ray_case("small", "z4096", kind, 0, K.OX)) for kind in ("inside", "outside", "tilt")]
    cases.append(("shrink", K.sphere_case("small", "z4096", "mid")))
    for kind, c in cases:
        fam = FAMILIES[family](gh, oracle, cuda, S, rays, c.sub)
        size = {}

        def warm(fam=fam, size=size):
            out = _from_plan(gh, lambda: fam.call()[0])
            size["bytes"] = gh.plan_bytes()
            assert size["bytes"] > 0
            return (out,)

        def after(stage, kind=kind, fam=fam, size=size):
            used = gh.last_plan_used()
            if stage == "warm":
                assert used == 1
            elif kind == "tilt" and stage in ("edit", "again"):
                assert used == 0, "a batch with an oblique ray ran from a plan"
            elif stage in ("edit", "again"):
                assert used in (0, 1)
                if used == 1:                       # re-recorded in place
                    assert gh.plan_bytes() in (size["bytes"], 0)
            elif kind == "tilt":                    # undone: a plan serves again within three calls
                for _ in range(3):
                    if gh.last_plan_used() == 1:
                        break
                    fam.call()
                assert gh.last_plan_used() == 1
        _cycle_guarded(S, gh, fam, S.arrays(rays), c.edit, c.affected, (family, kind), warm=warm, after=after)


def test_three_pass_ray_order_after_an_edit(gh, oracle, cuda, small_dev):
    """2^20 + 64 rays: the gated radix sort of the ray order takes three passes.  One ray near the
    middle moves, then a call with NO edit (the not-stale branch of every gated pass must leave perm
    a permutation: checked by the results and against the caller's order), then the first ray moves."""
    S = small_dev
    first = K.ray_case("small", "z1024", "inside", K.THREE_PASS_RAYS // 2 + 7, K.OX)
    second = K.ray_case("small", "z1024", "inside", 0, K.OX)
    assert K.sort_passes(len(first.rays)) == 3
    rays = _rays_on(cuda, first.rays)
    sub = np.unique(np.concatenate([first.sub, second.sub]))
    fam = Counts(gh, oracle, cuda, S, rays, sub)
    arrays = S.arrays(rays)
    ctx = gh.Context()
    ctx.make_current()
    try:
        outs = [fam.call() for _ in range(3)]
        assert _same(outs[0], outs[1]) and _same(outs[0], outs[2])
        warm, key0 = outs[2], fam.check(outs[2])
        _apply(arrays, first.edit)
        got = fam.call()
        key1 = fam.check(got)
        assert _same(got, _fresh(gh, fam, ctx))
        _must_differ(fam, first.affected, key0, key1, warm, got, "middle ray")
        unedited = fam.call()                                   # no edit: nothing is stale
        assert _same(unedited, got)
        gh.set_ray_reorder(False)
        plain = fam.call()
        gh.set_ray_reorder(True)
        assert _same(plain, got), "the caller's order gives other hit counts than the cached order"
        _apply(arrays, second.edit)
        got2 = fam.call()
        key2 = fam.check(got2)
        assert _same(got2, _fresh(gh, fam, ctx))
        _must_differ(fam, second.affected, key1, key2, got, got2, "first ray")
        assert _same(fam.call(), got2)
        _apply(arrays, second.edit.inverse()); _apply(arrays, first.edit.inverse())
        assert _same(fam.call(), warm)
        gh.trace_status()
    finally:
        _reset(gh)
        gh.Context.reset_current()
        ctx.destroy()


class _Tris:
    def __init__(self, gh, cuda, scene, k):
        """The triangles as pool[k:] (k * 36 bytes in); the tree is built over an aligned copy in
        the same (tree) order, which the build leaves as it is."""
        self.host = scene.tris
        aligned = torch.from_numpy(self.host.copy()).to(cuda)
        self.tree = gh.Tree(len(self.host), scene.mpl, device=cuda)
        gh.build_tree_tris(aligned, self.tree)
        assert np.array_equal(aligned.cpu().numpy().view(np.uint32), self.host.view(np.uint32)), "the build moved triangles"
        pool = torch.empty((len(self.host) + k, K.TRI_WORDS), dtype=torch.float32, device=cuda)
        self.d = pool[k:]
        self.d.copy_(aligned)
        assert pool.data_ptr() % 16 == 0 and self.d.data_ptr() - pool.data_ptr() == K.view_offset_bytes(k, K.TRI_WORDS)
        assert (self.d.data_ptr() % 16 == 0) == (k == 0)

    def now(self):
        return self.d.cpu().numpy()

    def restore(self):
        self.d.copy_(torch.from_numpy(self.host.copy()))


class Closest(_Family):
    integer = True

    def call(self):
        out = torch.full((self.R,), -7, dtype=torch.int32, device=self.cuda)
        self.gh.trace_closest_tri(self.rays, self.S.d, self.S.tree, out)
        return (out,)

    def check(self, out):
        ref = self.O.brute_closest_tri(*self._sub())[0]
        got = out[0].cpu().numpy()[self.sub]
        assert np.array_equal(got, ref), (self.sub[got != ref][:5], got[got != ref][:5], ref[got != ref][:5])
        return ref


@pytest.mark.parametrize("view", [0, 1], ids=["aligned", "pool[1:]"])
def test_one_triangle_collapsed_in_place(gh, oracle, cuda, view):
    """The last triangle (in the view: the final, partial chunk of a word-by-word pass) and one in the
    middle lose their area; the rays that found them find what lies behind, their own rays nothing.
    "fold" changes the array's last word alone: the partial chunk of an aligned array too."""
    S = _Tris(gh, cuda, K.tris(), view)
    rays = _rays_on(cuda, K.batch("y4096"))
    for probe, kind in (("last", "collapse"), ("mid", "collapse"), ("last", "fold")):
        c = K.tri_case(probe, kind)
        fam = Closest(gh, oracle, cuda, S, rays, c.sub)
        assert c.ray in c.sub and c.after[c.ray] == -1          # (held against brute force with the rest of sub)
        _cycle_guarded(S, gh, fam, {"tris": S.d, "rays": rays}, c.edit, c.affected, (view, probe, kind))


@pytest.mark.parametrize("family", ["counts", "exact"])
@pytest.mark.parametrize("kind", ["inside", "outside"])
@pytest.mark.parametrize("batch,coord", [("x4097", K.OY), ("x4098", K.OZ)])
def test_partial_last_chunk_of_the_rays(gh, oracle, cuda, small_dev, batch, coord, kind, family):
    """4097 and 4098 rays through the C entry point (the Python wrappers admit multiples of 32 only,
    whose arrays end on a chunk boundary): the ray array ends in a chunk of 3 and of 2 words, and the
    edited word -- oy, oz of the last ray, both transverse in a +x batch -- lies in it.  Moved across
    the rectangle, and beyond it.  Hit counts, and the exact column densities, whose packet plan is
    recorded from the ray order: a ray left in its old packet's lists loses its new hits."""
    S = small_dev
    c = K.ray_case("small", batch, kind, -1, coord)
    assert (7 * len(c.rays)) % 4 in (2, 3) and c.edit.chunks[0] == (7 * len(c.rays) + 3) // 4 - 1
    rays = _rays_on(cuda, c.rays)
    fam = (CountsCApi if family == "counts" else CumulativeCApi)(gh, oracle, cuda, S, rays, c.sub)
    _cycle_guarded(S, gh, fam, S.arrays(rays), c.edit, c.affected, (batch, kind, family))


def test_two_contexts_each_notice(gh, oracle, cuda, small_dev):
    """Two contexts hold records of the same arrays.  After the edit each must notice on its own: b's
    signature is b's, and a's re-derivation does not excuse it."""
    S = small_dev
    rays = _rays_on(cuda, K.batch("full4096"))
    c = K.sphere_case("small", "full4096", "mid")
    arrays = S.arrays(rays)
    fams = {"counts": Counts(gh, oracle, cuda, S, rays, c.sub), "exact": Cumulative(gh, oracle, cuda, S, rays, c.sub)}
    a, b = gh.Context(), gh.Context()
    try:
        warm, keys = {}, {}
        for ctx in (a, b):
            ctx.make_current()
            gh.set_exact_integrals(True)
            for name, fam in fams.items():
                outs = [fam.call() for _ in range(3)]
                assert _same(outs[0], outs[2]) and (name not in warm or _same(outs[2], warm[name]))
                warm[name], keys[name] = outs[2], fam.check(outs[2])
        _apply(arrays, c.edit)
        for ctx in (a, b):
            ctx.make_current()
            for name, fam in fams.items():
                got = fam.call()
                gh.trace_status()
                _must_differ(fam, c.affected, keys[name], fam.check(got), warm[name], got, name)
                assert _same(fam.call(), got)
        _apply(arrays, c.edit.inverse())
        for ctx in (a, b):
            ctx.make_current()
            for name, fam in fams.items():
                assert _same(fam.call(), warm[name]), name
                gh.trace_status()
    finally:
        for ctx in (a, b):
            ctx.make_current()
            _reset(gh)
        gh.Context.reset_current()
        a.destroy(); b.destroy()
        S.restore()


def test_validation_switched_back_on_notices(gh, oracle, cuda, small_dev):
    """A trusted period (set_cache_validation(False), no edit: the promise is kept), then validation
    on again and an edit: the signature the records were derived under is still the one compared."""
    S = small_dev
    rays = _rays_on(cuda, K.batch("full4096"))
    c = K.sphere_case("small", "full4096", "last")
    for family in ("counts", "exact"):
        fam = FAMILIES[family](gh, oracle, cuda, S, rays, c.sub)

        def warm(fam=fam):
            outs = [fam.call() for _ in range(3)]
            gh.set_cache_validation(False)
            outs += [fam.call() for _ in range(2)]
            gh.set_cache_validation(True)
            assert all(_same(o, outs[0]) for o in outs)
            return outs[-1]
        _cycle_guarded(S, gh, fam, S.arrays(rays), c.edit, c.affected, family, warm=warm)


def test_prepared_caches_are_validated_too(gh, oracle, cuda, small_dev):
    """set_cache_auto(False), trace_prepare and trace_prepare_rays: pinned caches, validated like the
    automatic ones.  A shrunk sphere, then a ray moved beyond the rectangle; after each, a further
    unedited call gives the same bits (the caches are still there and hold the new records)."""
    S = small_dev
    rays = _rays_on(cuda, K.batch("z4096"))
    edits = [K.sphere_case("small", "z4096", "mid"), K.ray_case("small", "z4096", "outside", 0, K.OX)]
    for family in ("counts", "exact"):
        for c in edits:
            fam = FAMILIES[family](gh, oracle, cuda, S, rays, c.sub)

            def warm(fam=fam):
                gh.set_cache_auto(False)
                gh.trace_prepare(S.d, S.tree)
                gh.trace_prepare_rays(rays)
                outs = [fam.call() for _ in range(2)]
                assert _same(outs[0], outs[1])
                return outs[1]
            # (both are released in the cycle's own finally, before its context goes)
            _cycle_guarded(S, gh, fam, S.arrays(rays), c.edit, c.affected, (family, c.edit.array), warm=warm)
