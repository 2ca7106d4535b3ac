"""The radix sort, the scans, the per-segment distance sort and the extrema at the sizes where their
code changes path.

Every build, every trace_sph, every sorting ray generator and every point query that returns lists
goes through csrc/sort.hip, csrc/scan.hip, csrc/segsort.hip and csrc/extrema.hip; their other tests
use random sizes and uniform keys.  The cases of sort_scan_boundary_cases.py sit on the constants
instead: both sides of every size at which the bucket plan changes its digit, its tile or its verdict,
a bucket holding exactly its capacity and one record more, every pass count of the index sort's
permutation ping-pong, the tails and slab edges of the scans, the second level of their recursion,
both sides of the distance sort's switch.  Every sort asserts through sort_last_stats() that the path
it was written for is the one that ran; every result is compared with a stable NumPy reference."""
import ctypes as C

import numpy as np
import pytest
import torch

import sort_scan_boundary_cases as S

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64


def _dev(a, cuda):
    a = np.ascontiguousarray(a)
    if a.dtype == U32:
        a = a.view(np.int32)          # torch stores the unsigned keys as signed words
    elif a.dtype == U64:
        a = a.view(np.int64)
    return torch.from_numpy(a).to(cuda)


def _assert_stats(gh, want):
    """The path the last sort planned, and -- once its stream is idle -- whether a bucket overflowed.
    A context without the pinned flag word reports -1: then only that comparison is left out."""
    torch.cuda.synchronize()
    st = gh.sort_last_stats()
    assert (st["msd_bits"], st["tile"], st["hint_skipped"]) == (want["msd_bits"], want["tile"], 0), (st, want)
    if want["overflowed"] == -1:
        assert st["overflowed"] == -1, (st, want)
    elif st["overflowed"] != -1:
        assert st["overflowed"] == want["overflowed"], (st, want)


def _check_sort(gh, cuda, keys, vals, begin, end, want_perm=True):
    kd = _dev(keys, cuda)
    vd = torch.from_numpy(vals).to(cuda) if vals is not None else None
    perm = gh.sort_by_key(kd, vd, begin, end, want_perm=want_perm)
    _assert_stats(gh, S.expected_stats(keys, 0 if vals is None else vals.shape[1], begin, end))
    order = S.stable_order(keys, begin, end)
    assert np.array_equal(kd.cpu().numpy().view(keys.dtype), keys[order])
    if vals is not None:
        assert np.array_equal(vd.cpu().numpy(), vals[order])          # int32 words: bit for bit
    if want_perm:
        assert np.array_equal(perm.cpu().numpy().view(U32), order.astype(U32))


def _case_id(v):
    if isinstance(v, type):
        return np.dtype(v).name
    return None


# ---- bucket plan -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype,words,begin,end", S.plan_boundary_cases(), ids=_case_id)
def test_sort_on_both_sides_of_every_plan_boundary(gh, cuda, n, dtype, words, begin, end):
    """Uniform keys with duplicates at the last size of one plan and the first of the next: the index
    sort below 2^18, m = 6 / 7 and 8 / 9 on the 8192-record tile, 8 / 9 on the 4096-record one, 31- and
    32-bit keys refused at m = 6 and sorted by the buckets where 24 bits are left below the digit."""
    keys = S.uniform_keys(n, dtype, end, seed=1)
    _check_sort(gh, cuda, keys, S.payload(n, words, seed=2), begin, end, want_perm=True)


@pytest.mark.parametrize("n", S.BIG_SORT_NS)
def test_sort_at_the_mean_bucket_refusal(gh, cuda, n):
    """12 587 007 64-bit keys are the last size the bucket sort takes (m = 12, mean bucket 3072 of
    4096); one more and the mean bucket is above 75 % of a workgroup: the index sort, eight passes.
    Keys and permutation only; checked on the device, the keys once against np.sort."""
    keys = S.uniform_keys(n, U64, 63, seed=1)
    want = S.expected_stats(keys, 0, 0, 63)
    assert want["msd_bits"] == (12 if n == S.BIG_SORT_NS[0] else 0)
    k_in = _dev(keys, cuda)
    kd = k_in.clone()
    perm = gh.sort_by_key(kd, None, 0, 63, want_perm=True)
    _assert_stats(gh, want)
    assert bool((kd[1:] >= kd[:-1]).all())                  # (63-bit keys: signed compares are right)
    p = perm.to(torch.int64)
    assert int(p.min()) == 0 and int(p.max()) == n - 1
    assert torch.equal(k_in[p], kd)
    same = kd[1:] == kd[:-1]
    assert int(same.sum()) > 0 and bool((p[1:][same] > p[:-1][same]).all())
    assert np.array_equal(kd.cpu().numpy().view(U64), np.sort(keys))


CAPACITY = [(U32, 4, 30), (U64, 0, 63), (U32, 9, 30)]
# bucket (-1: the last), records beyond the capacity, equal keys, one aligned run of the input
CAPACITY_FILLS = [(5, 0, False, False), (5, 0, True, False), (5, 1, False, False), (5, 0, True, True),
                  (0, 0, True, False), (0, 0, False, False), (-1, 0, True, False), (-1, 0, False, False),
                  (0, 1, True, False), (-1, 1, True, False)]


@pytest.mark.parametrize("bucket,extra,equal,contiguous", CAPACITY_FILLS)
@pytest.mark.parametrize("dtype,words,bits", CAPACITY, ids=_case_id)
def test_sort_with_a_bucket_at_its_capacity(gh, cuda, dtype, words, bits, bucket, extra, equal, contiguous):
    """n = 262144: one bucket holds exactly the tile (8192 records of 30-bit keys + 16 B; 4096 of
    64-bit keys, and of 30-bit keys + 36 B) -- the bucket kernels must run, the per-wave counters reach
    1024 (512) and the rank field its maximum when the keys are equal -- or one record more: the flag
    kernel must turn them off and the gated index sort on."""
    n = 262144
    kb = np.dtype(dtype).itemsize
    m, cap = S.plan(n, kb, words, bits), S.tile(kb, words)
    b = bucket if bucket >= 0 else (1 << m) - 1
    keys = S.capacity_keys(n, dtype, 0, bits, m, b, cap + extra, equal=equal, contiguous=contiguous)
    assert S.expected_stats(keys, words, 0, bits) == {"msd_bits": m, "tile": cap, "hint_skipped": 0,
                                                      "overflowed": extra}
    _check_sort(gh, cuda, keys, S.payload(n, words, seed=3), 0, bits, want_perm=True)


@pytest.mark.parametrize("run", [8, 9])
@pytest.mark.parametrize("words", [0, 4])
def test_sort_tie_runs_in_a_full_bucket(gh, cuda, run, words):
    """A bucket of exactly 4096 63-bit records in runs that agree on every bit the LDS passes cover:
    512 runs of 8 (the longest the insertion sort settles) and 455 runs of 9 (the bucket is sorted
    again over all its bits)."""
    n = 262144
    keys = S.tie_run_keys(n, 7, 5, run)
    _check_sort(gh, cuda, keys, S.payload(n, words, seed=4), 0, 63, want_perm=True)


def test_sort_stats_follow_the_context_and_the_hint(gh, cuda):
    """sort_last_stats() reports the calling thread's context: a fresh one has no record; with the
    overflow hint on, the sort after an overflow plans its buckets, is sent to the index sort and says
    so; the record of the context outside is untouched."""
    n = 262144
    uniform = S.uniform_keys(n, U32, 30, seed=8)
    crowded = S.capacity_keys(n, U32, 0, 30, 6, 5, 8193, seed=8)
    vals = S.payload(n, 4, seed=8)
    _check_sort(gh, cuda, uniform, vals, 0, 30)
    outside = gh.sort_last_stats()
    assert outside["msd_bits"] == 6
    gh.set_sort_overflow_hint(True)
    try:
        with gh.Context():
            assert gh.sort_last_stats() == {"msd_bits": 0, "tile": 0, "hint_skipped": 0, "overflowed": -1}
            _check_sort(gh, cuda, crowded, vals, 0, 30)              # overflows (asserted inside)
            have_word = gh.sort_last_stats()["overflowed"] == 1
            kd, vd = _dev(uniform, cuda), torch.from_numpy(vals).to(cuda)
            gh.sort_by_key(kd, vd, 0, 30)
            torch.cuda.synchronize()
            st = gh.sort_last_stats()
            if have_word:
                assert st == {"msd_bits": 6, "tile": 8192, "hint_skipped": 1, "overflowed": -1}
            order = S.stable_order(uniform, 0, 30)
            assert np.array_equal(kd.cpu().numpy().view(U32), uniform[order])
            assert np.array_equal(vd.cpu().numpy(), vals[order])
    finally:
        gh.set_sort_overflow_hint(False)
    assert gh.sort_last_stats() == outside


# ---- index sort ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,begin,end",
                         [(U32, b, e) for b, e in S.INDEX_RANGES_U32] + [(U64, b, e) for b, e in S.INDEX_RANGES_U64],
                         ids=_case_id)
def test_index_sort_every_pass_count(gh, cuda, dtype, begin, end):
    """1 to 4 passes over 32-bit keys, 1 to 8 over 64-bit keys: the permutation buffer enters the
    ping-pong on the side the parity of the pass count asks for.  Tiles of 4096: one short, one full,
    one record into the second, two and a record."""
    for n in S.INDEX_NS:
        keys = S.uniform_keys(n, dtype, 8 * np.dtype(dtype).itemsize, seed=begin * 64 + end)
        if n > 2:
            keys[: n // 3] = keys[n // 3: 2 * (n // 3)]      # stability has something to keep
        for want_perm in (True, False):
            vals = S.payload(n, 2, seed=n) if want_perm else None
            _check_sort(gh, cuda, keys, vals, begin, end, want_perm=want_perm)
            _check_sort(gh, cuda, keys, S.payload(n, 4, seed=n) if not want_perm else None, begin, end,
                        want_perm=want_perm)


@pytest.mark.parametrize("words", S.PAYLOAD_WORDS)
@pytest.mark.parametrize("dtype", [U32, U64], ids=_case_id)
def test_index_sort_every_payload_width(gh, cuda, dtype, words):
    n = 4097
    keys = S.uniform_keys(n, dtype, 20, seed=words)
    keys[1000:2000] = keys[:1000]
    _check_sort(gh, cuda, keys, S.payload(n, words, seed=5), 0, 20, want_perm=(words % 2 == 0))


def _raw_sort(gh, kbuf, vbuf, pbuf, off, n, words, begin, end):
    """The C entry point on n elements starting at element `off` of the buffers."""
    es = kbuf.element_size()
    fn = gh._lib.grace_sort_pairs_u32 if es == 4 else gh._lib.grace_sort_pairs_u64
    vp = C.c_void_p(vbuf.data_ptr() + off * words * 4) if vbuf is not None else C.c_void_p(0)
    pp = C.c_void_p(pbuf.data_ptr() + off * 4) if pbuf is not None else C.c_void_p(0)
    gh._check(fn(C.c_void_p(kbuf.data_ptr() + off * es), vp, C.c_size_t(n), C.c_int(words * 4),
                 C.c_int(begin), C.c_int(end), pp, gh._stream()))


@pytest.mark.parametrize("n", [0, 1])
@pytest.mark.parametrize("dtype", [U32, U64], ids=_case_id)
def test_sort_of_nothing_and_of_one(gh, cuda, dtype, n):
    """n = 0 touches nothing, n = 1 writes perm[0] = 0 and nothing else: guard elements on both sides
    of every array keep their values."""
    tdt = torch.int32 if dtype == U32 else torch.int64
    for with_vals in (False, True):
        for with_perm in (False, True):
            kbuf = torch.arange(100, 108, dtype=tdt, device=cuda)
            vbuf = torch.arange(200, 232, dtype=torch.int32, device=cuda) if with_vals else None
            pbuf = torch.full((8,), -7, dtype=torch.int32, device=cuda) if with_perm else None
            _raw_sort(gh, kbuf, vbuf, pbuf, 4, n, 4, 0, 8 * kbuf.element_size())
            _assert_stats(gh, {"msd_bits": 0, "tile": 4096 if dtype == U64 else 8192, "overflowed": -1})
            assert kbuf.tolist() == list(range(100, 108))
            if with_vals:
                assert vbuf.tolist() == list(range(200, 232))
            if with_perm:
                assert pbuf.tolist() == [-7] * 4 + ([0] if n else [-7]) + [-7] * 3


@pytest.mark.parametrize("dtype,begin,end", [(U32, 3, 27), (U32, 0, 31), (U64, 5, 29), (U64, 16, 64), (U64, 1, 63)],
                         ids=_case_id)
def test_sort_ignores_the_bits_outside_its_range(gh, cuda, dtype, begin, end):
    """All ones outside [begin, end) and zeros inside: every key is equal, the sort is the identity."""
    n = 8193
    keys = S.outside_ones_keys(n, dtype, begin, end)
    vals = S.payload(n, 3, seed=6)
    kd, vd = _dev(keys, cuda), torch.from_numpy(vals).to(cuda)
    perm = gh.sort_by_key(kd, vd, begin, end, want_perm=True)
    _assert_stats(gh, S.expected_stats(keys, 3, begin, end))
    assert np.array_equal(kd.cpu().numpy().view(dtype), keys)
    assert np.array_equal(vd.cpu().numpy(), vals)
    assert np.array_equal(perm.cpu().numpy(), np.arange(n, dtype=np.int32))


def test_index_sort_past_the_gather_grid(gh, cuda):
    """16-bit keys stay with the index sort at any size: at 1 048 577 records the payload gather's
    4096 workgroups reach their last record by striding."""
    n = S.GATHER_GRID_STRIDE_N
    keys = S.uniform_keys(n, U32, 16, seed=7)
    assert S.plan(n, 4, 4, 16) is None
    _check_sort(gh, cuda, keys, S.payload(n, 4, seed=7), 0, 16, want_perm=True)


# ---- exclusive scan --------------------------------------------------------------------------------
def _check_scan(gh, cuda, n, in_place):
    v = S.scan_values(n, seed=1)
    ref, total = S.scan_ref(v)
    d = torch.from_numpy(v).to(cuda)
    out = d if in_place else torch.full_like(d, -1)
    got_total = gh.exclusive_scan(d, out)
    assert got_total == total
    assert np.array_equal(out.cpu().numpy(), ref)
    if not in_place:
        assert np.array_equal(d.cpu().numpy(), v)


@pytest.mark.parametrize("n", S.SCAN_NS)
def test_exclusive_scan_at_vector_chunk_and_slab_edges(gh, cuda, n):
    assert S.levels(n) == (1 if n <= S.SLAB else 2)
    _check_scan(gh, cuda, n, in_place=False)
    _check_scan(gh, cuda, n, in_place=True)


@pytest.mark.parametrize("n,in_place", [(S.SCAN_BIG_NS[0], False), (S.SCAN_BIG_NS[1], True)])
def test_exclusive_scan_second_recursion(gh, cuda, n, in_place):
    """8192 slabs of 8192 still scan their sums in one workgroup; one element more and the slab sums
    need a scan with carries of their own."""
    assert S.levels(n) == (2 if n == S.SLAB * S.SLAB else 3)
    _check_scan(gh, cuda, n, in_place)


# ---- segmented scan --------------------------------------------------------------------------------
def _check_segscan(gh, cuda, offsets, data, in_place, ref=None):
    ref = S.segscan_ref(offsets, data) if ref is None else ref
    d_off = torch.from_numpy(np.asarray(offsets, np.int32)).to(cuda)
    d = torch.from_numpy(data).to(cuda)
    out = d if in_place else torch.full_like(d, -77.0)
    gh.exclusive_segmented_scan(d_off, d, out)
    got = out.cpu().numpy()
    assert got.dtype == data.dtype
    bad = np.flatnonzero(got.astype(np.float64) != ref)
    assert len(bad) == 0, (bad[:6], got[bad[:6]], ref[bad[:6]])
    if not in_place:
        assert np.array_equal(d.cpu().numpy(), data)


@pytest.mark.parametrize("pattern", S.SEG_PATTERNS)
def test_segmented_scan_head_patterns(gh, cuda, pattern):
    """Heads on, one before and one after every slab (8192), chunk (1024) and thread (4) edge; a
    segment that crosses every later slab without a head; empty segments stacked at the first element,
    on a slab edge, on the last element and behind it; no listed segment at all.  Integer-valued data:
    the sums are exact, so equality."""
    for n in S.SEG_NS:
        offsets = S.seg_offsets(pattern, n)
        if offsets is None:
            continue
        for dtype in (np.float32, np.float64):
            data = S.seg_integer_data(n, dtype, seed=2)
            ref = S.segscan_ref(offsets, data)
            for in_place in (False, True):
                _check_segscan(gh, cuda, offsets, data, in_place, ref)


def test_segmented_scan_two_level_spine(gh, cuda):
    """8194 slabs: their aggregates need a spine of two slabs and a third level above it.  The second
    segment runs headless through all but the last three elements of the first spine slab."""
    offsets, data = S.two_level_case()
    assert S.levels(len(data)) == 3
    ref = S.segscan_ref(offsets, data, acc=np.int32)
    d_off = torch.from_numpy(offsets).to(cuda)
    d = torch.from_numpy(data).to(cuda)
    out = torch.full_like(d, -77.0)
    gh.exclusive_segmented_scan(d_off, d, out)
    got = out.cpu().numpy()
    bad = np.flatnonzero(got != ref)
    assert len(bad) == 0, (bad[:6], got[bad[:6]], ref[bad[:6]])


def test_segmented_scan_real_values_within_the_summation_bound(gh, cuda):
    """Uniform values in [-1, 1): whatever the order of the additions, a float32 sum of L terms is
    within (L - 1) 2^-24 sum|x| (1 + O(L 2^-24)) of the exact one; a lost or doubled slab carry is
    orders of magnitude outside."""
    n = 24577
    data = np.random.default_rng(8).uniform(-1.0, 1.0, n).astype(np.float32)
    offsets = np.array([0, 5], np.int32)
    ref = S.segscan_ref(offsets, data)
    length = np.arange(n) - S.seg_head_index(offsets, n)
    bound = np.maximum(length - 1, 0) * 2.0 ** -24 * S.segscan_ref(offsets, np.abs(data)) * 1.01
    d = torch.from_numpy(data).to(cuda)
    out = torch.empty_like(d)
    gh.exclusive_segmented_scan(torch.from_numpy(offsets).to(cuda), d, out)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref)
    print("segmented scan, real values: max error %.3e, max error / bound %.3f" % (
        err.max(), float(np.max(err[bound > 0] / bound[bound > 0]))))
    bad = np.flatnonzero(err > bound)
    assert len(bad) == 0, (bad[:6], err[bad[:6]], bound[bad[:6]])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_weighted_segmented_scan(gh, cuda, dtype):
    n = 3 * S.SLAB + 5
    offsets = S.seg_offsets("slab-1", n)
    rng = np.random.default_rng(9)
    x = S.seg_integer_data(n, dtype, seed=3)
    w = rng.integers(-3, 4, 37).astype(dtype)
    wmap = rng.integers(0, 37, n).astype(np.int32)
    ref = S.segscan_ref(offsets, (w[wmap] * x).astype(np.float64))
    out = torch.full((n,), -77.0, dtype=torch.from_numpy(x).dtype, device=cuda)
    gh.weighted_exclusive_segmented_scan(torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda),
                                         torch.from_numpy(wmap).to(cuda), torch.from_numpy(offsets).to(cuda), out)
    assert np.array_equal(out.cpu().numpy().astype(np.float64), ref)


# ---- sort_by_distance ------------------------------------------------------------------------------
def _check_segsort(gh, cuda, dist, sizes, with_idx=True, with_data=True):
    n = len(dist)
    assert n == sum(sizes)
    rng = np.random.default_rng(n)
    idx = rng.permutation(n).astype(np.int32)
    data = rng.standard_normal(n).astype(dist.dtype)
    dd = torch.from_numpy(dist).to(cuda)
    di = torch.from_numpy(idx).to(cuda) if with_idx else None
    dw = torch.from_numpy(data).to(cuda) if with_data else None
    gh.sort_by_distance(dd, torch.from_numpy(S.sizes_to_offsets(sizes)).to(cuda), di, dw)
    torch.cuda.synchronize()
    order = S.segsort_order(dist, sizes)
    bits = U32 if dist.dtype == np.float32 else U64
    # bit for bit: a -0.0 stays a -0.0, in input order among the zeros of its segment
    assert np.array_equal(dd.cpu().numpy().view(bits), dist[order].view(bits))
    if with_idx:
        assert np.array_equal(di.cpu().numpy(), idx[order])
    if with_data:
        assert np.array_equal(dw.cpu().numpy().view(bits), data[order].view(bits))


def _mark_stats(gh, cuda):
    """A two-record sort of 32-bit keys leaves tile = 8192 in the context's record: a distance sort
    that takes the composite path overwrites it (64-bit keys: 4096), the wave path leaves it."""
    gh.sort_by_key(torch.tensor([2, 1], dtype=torch.int32, device=cuda))
    assert gh.sort_last_stats()["tile"] == 8192


@pytest.mark.parametrize("sizes", [[65537, 0], [65538, 0], [1, 65537], [32769, 32769]], ids=str)
def test_distance_sort_on_both_sides_of_its_switch(gh, cuda, sizes):
    """n_hits / n_rays = 32768: one wavefront per segment (a segment of 65537 hits); 32769: the
    composite 64-bit keys, 33 bits = five index passes with a permutation."""
    dist = S.distances(sum(sizes), np.float32, seed=1)
    _mark_stats(gh, cuda)
    _check_segsort(gh, cuda, dist, sizes)
    st = gh.sort_last_stats()
    if S.is_composite(sizes, np.float32):
        assert (st["msd_bits"], st["tile"], st["overflowed"]) == (0, 4096, -1)
    else:
        assert st["tile"] == 8192


@pytest.mark.parametrize("sizes", [[150000, 0, 120000, 0], [150000, 0, 120000, 0, 0]], ids=str)
def test_distance_sort_composite_keys_reach_the_bucket_plan(gh, cuda, sizes):
    """270 000 composite keys plan the 64-bit bucket sort (m = 7); the segment bits and the few
    exponents of the distances crowd them into a handful of buckets, so the flag kernel turns the
    bucket kernels off and the gated index sort finishes: asserted, not assumed.  Empty segments in
    the middle and at offset = n_hits."""
    dist = S.distances(sum(sizes), np.float32, seed=2)
    want = S.expected_stats(S.composite_keys(dist, sizes), 0, 0, S.composite_bits(len(sizes)))
    assert (want["msd_bits"], want["overflowed"]) == (7, 1)
    _mark_stats(gh, cuda)
    _check_segsort(gh, cuda, dist, sizes)
    _assert_stats(gh, want)
    assert gh.sort_last_stats()["overflowed"] in (1, -1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_distance_sort_wave_path_lengths(gh, cuda, dtype):
    """Segments of 0, 1, 2 hits, one short of / exactly / one past one and two rounds of 64 lanes, and
    4097; 1, 3, 4, 5 and 8 segments: the last workgroup of four waves is partly idle."""
    _mark_stats(gh, cuda)
    sizes = list(S.WAVE_LENGTHS)
    _check_segsort(gh, cuda, S.distances(sum(sizes), dtype, seed=3), sizes)
    rotated = [129, 64, 4097, 0, 65, 1, 2, 63]
    for k in (1, 3, 4, 5, 8):
        _check_segsort(gh, cuda, S.distances(sum(rotated[:k]), dtype, seed=k), rotated[:k])
    assert gh.sort_last_stats()["tile"] == 8192          # no composite sort ran


def test_distance_sort_f64_below_float_precision(gh, cuda):
    """Distances 1 + k 2^-40: equal as floats, ordered only by all eight digit passes."""
    sizes = list(S.WAVE_LENGTHS)
    _check_segsort(gh, cuda, S.fine_distances(sum(sizes), seed=4), sizes)
    sizes = [65538, 0]                                    # float64 has no composite path
    _check_segsort(gh, cuda, S.fine_distances(sum(sizes), seed=5), sizes)


@pytest.mark.parametrize("with_idx,with_data", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_distance_sort_null_arguments(gh, cuda, dtype, with_idx, with_data):
    sizes = [129, 0, 4097, 64]
    _check_segsort(gh, cuda, S.distances(sum(sizes), dtype, seed=6), sizes, with_idx, with_data)
    if dtype == np.float32:
        sizes = [65538, 0]
        _check_segsort(gh, cuda, S.distances(sum(sizes), dtype, seed=7), sizes, with_idx, with_data)


# ---- extrema ---------------------------------------------------------------------------------------
def _places(n):
    return [p for p in (0, n - 1, S.EXTREMA_FIRST_STRIDED) if p < n]


@pytest.mark.parametrize("n", S.EXTREMA_NS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_min_max_components_extreme_rows(gh, cuda, dtype, n):
    """The extreme row first, last and at 262144 (the first row a grid capped at 1024 workgroups
    reaches by striding); +-inf and INT32_MIN / INT32_MAX are returned as they are."""
    for place in _places(n):
        a = S.extrema_rows(n, dtype, place, seed=1)
        lo, hi = gh.min_max_components(torch.from_numpy(a).to(cuda), 4)
        want_lo, want_hi = S.extrema_ref(a)
        assert lo.dtype == a.dtype and np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (place, lo, hi)
    # a record stride wider than the components asked for
    lo, hi = gh.min_max_components(torch.from_numpy(a).to(cuda), 2, first=1)
    assert np.array_equal(lo, want_lo[1:3]) and np.array_equal(hi, want_hi[1:3])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_min_max_components_skip_nan(gh, cuda, dtype):
    n = 262145
    a = S.extrema_rows(n, dtype, n - 1, seed=2)
    a[::7, 0] = np.nan
    a[0, 0] = a[n - 1, 2] = np.nan
    a[:, 1] = np.nan
    lo, hi = gh.min_max_components(torch.from_numpy(a).to(cuda), 4)
    want_lo, want_hi = S.extrema_ref(a)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)
    assert np.isposinf(lo[1]) and np.isneginf(hi[1])      # a column of NaN only


@pytest.mark.parametrize("n", S.EXTREMA_NS)
def test_min_max_vec4_and_centroid_bounds(gh, cuda, n):
    for place in _places(n):
        a = S.extrema_rows(n, np.float32, place, seed=3)
        d = torch.from_numpy(a).to(cuda)
        want_lo, want_hi = S.extrema_ref(a)
        lo, hi = gh.min_max_vec4(d)
        assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (place, lo, hi)
        bot, top = gh.centroid_bounds(d)
        assert np.array_equal(bot, want_lo[:3]) and np.array_equal(top, want_hi[:3])
    # an all-negative column, a column with -0.0 as its maximum, NaN skipped
    a = S.extrema_rows(n, np.float32, n - 1, seed=4)
    a[:, 0] = -np.abs(a[:, 0]) - 1.0
    a[:, 1] = -np.abs(a[:, 1])
    a[n // 2, 1] = -0.0
    a[::5, 2] = np.nan
    a[0, 2] = a[n - 1, 2] = np.nan
    d = torch.from_numpy(a).to(cuda)
    want_lo, want_hi = S.extrema_ref(a)
    assert want_hi[0] < 0 and want_hi[1] == 0
    lo, hi = gh.min_max_vec4(d)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)     # (zeros compare by value)
    bot, top = gh.centroid_bounds(d)
    assert np.array_equal(bot, want_lo[:3]) and np.array_equal(top, want_hi[:3])
