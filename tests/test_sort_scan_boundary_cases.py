"""CPU checks of tests/sort_scan_boundary_cases.py: the restated decisions of csrc/sort.hip,
csrc/scan.hip and csrc/segsort.hip are pinned to numbers worked out from the source, the references
agree with the oracle and with plain loops, and every generated case is what its name says (the
bucket at capacity holds exactly the capacity, the fallback case one more, the heads sit where the
pattern puts them, the two-level cases have more than 8192 slabs)."""
import numpy as np
import pytest

import sort_scan_boundary_cases as S

U32, U64 = np.uint32, np.uint64


# ---- the sort's plan -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,key_bytes,words,bits,m", S.PLAN_TABLE)
def test_plan_table(n, key_bytes, words, bits, m):
    assert S.plan(n, key_bytes, words, bits) == m


def test_plan_tiles_and_refusals():
    assert S.tile(4, 0) == S.tile(4, 4) == 8192
    assert S.tile(4, 7) == S.tile(4, 9) == S.tile(8, 0) == S.tile(8, 4) == 4096
    assert S.plan(1 << 20, 4, 4, 16) is None            # two index passes: a draw
    assert S.plan(1 << 20, 4, 4, 17) is not None
    assert S.plan(1 << 20, 4, 10, 30) is None
    # the 75 % refusal is first met where m has hit its ceiling of 12 bits
    assert S.plan(12587007, 8, 0, 63) == S.MAX_MSD_BITS
    for n in range(1 << 18, 1 << 22, 4099):
        for kb, w in ((4, 4), (8, 0), (4, 9)):
            m = S.plan(n, kb, w, 63 if kb == 8 else 30)
            assert m is not None and (n >> m) * 10 <= S.tile(kb, w) * 6 and (m == 1 or (n >> (m - 1)) * 10 > S.tile(kb, w) * 6)
    # 32-bit keys: a plan exists exactly where at most 24 bits stay below the digit
    assert S.plan(629248, 4, 4, 32) == 8 and S.plan(629247, 4, 4, 32) is None
    assert S.plan(314624, 4, 4, 31) == 7 and S.plan(314623, 4, 4, 31) is None
    assert [S.n_passes(b, e) for b, e in S.INDEX_RANGES_U32] == [1, 2, 3, 4, 4, 1]
    assert [S.n_passes(b, e) for b, e in S.INDEX_RANGES_U64] == [1, 2, 3, 4, 5, 6, 7, 8, 8]


def test_digits_counts_and_order():
    keys = np.array([0xFFFFFFFF, 0x80000001, 0x00000010, 0x80000000, 0x7FFFFFF0], dtype=U32)
    assert S.digits(keys, 0, 32).tolist() == keys.tolist()
    assert S.digits(keys, 4, 8).tolist() == [15, 0, 1, 0, 15]
    assert S.digits(keys, 31, 32).tolist() == [1, 1, 0, 1, 0]
    assert S.bucket_counts(keys, 0, 32, 1).tolist() == [2, 3]
    assert S.bucket_counts(keys, 4, 8, 2).tolist() == [3, 0, 0, 2]
    assert S.stable_order(keys, 4, 8).tolist() == [1, 3, 2, 0, 4]
    k64 = np.array([1 << 63, (1 << 63) - 1, 0], dtype=U64)
    assert S.digits(k64, 0, 64).tolist() == k64.tolist()
    assert S.stable_order(k64, 0, 64).tolist() == [2, 1, 0]
    assert S.stable_order(k64, 0, 63).tolist() == [0, 2, 1]
    assert np.all(S.digits(S.outside_ones_keys(9, U32, 3, 27), 3, 27) == 0)
    assert np.all(S.outside_ones_keys(9, U32, 3, 27) == U32(0xF8000007))
    assert np.all(S.outside_ones_keys(9, U64, 0, 64) == 0) and np.all(S.outside_ones_keys(9, U64, 16, 64) == 0xFFFF)


@pytest.mark.parametrize("n,dtype,words,begin,end", S.plan_boundary_cases())
def test_plan_boundary_cases_take_the_path_they_name(n, dtype, words, begin, end):
    keys = S.uniform_keys(n, dtype, end, seed=1)
    assert keys.dtype == dtype and len(keys) == n
    st = S.expected_stats(keys, words, begin, end)
    m = S.plan(n, np.dtype(dtype).itemsize, words, end - begin)
    assert st["msd_bits"] == (m or 0) and st["tile"] == S.tile(np.dtype(dtype).itemsize, words)
    if m is None:
        assert st["overflowed"] == -1
    else:
        # uniform keys: every bucket fits, and the duplicates are there
        assert st["overflowed"] == 0 and S.bucket_counts(keys, begin, end, m).max() <= st["tile"]
    assert len(np.unique(S.digits(keys, begin, end))) < n - n // 500
    if end - begin >= 31:
        assert int(S.digits(keys, begin, end).max()) >> (end - begin - 1) == 1   # the top bit is in use


def test_plan_boundary_cases_cover_the_table():
    cases = {(n, np.dtype(d).itemsize, w, e - b) for n, d, w, b, e in S.plan_boundary_cases()}
    for n, kb, w, bits, _ in S.PLAN_TABLE:
        assert n in S.BIG_SORT_NS or (n, kb, w, bits) in cases, (n, kb, w, bits)
    assert {(12587007, 8, 0, 63, 12), (12587008, 8, 0, 63, None)} <= set(S.PLAN_TABLE)


def test_big_sort_keys_fit_their_buckets():
    """12 587 007 uniform 63-bit keys in 4096 buckets of 4096: the bucket path, no overflow."""
    n = S.BIG_SORT_NS[0]
    keys = S.uniform_keys(n, U64, 63, seed=1)
    st = S.expected_stats(keys, 0, 0, 63)
    assert st == {"msd_bits": 12, "tile": 4096, "hint_skipped": 0, "overflowed": 0}
    assert S.plan(S.BIG_SORT_NS[1], 8, 0, 63) is None


CAP_CONFIGS = [(U32, 4, 30), (U64, 0, 63), (U32, 9, 30)]


@pytest.mark.parametrize("dtype,words,bits", CAP_CONFIGS)
def test_capacity_cases(dtype, words, bits):
    n = 262144
    kb = np.dtype(dtype).itemsize
    m, cap = S.plan(n, kb, words, bits), S.tile(kb, words)
    assert (m, cap) == {(U32, 4): (6, 8192), (U64, 0): (7, 4096), (U32, 9): (7, 4096)}[(dtype, words)]
    for bucket in (0, 5, (1 << m) - 1):
        for equal in (False, True):
            for contiguous in (False, True):
                keys = S.capacity_keys(n, dtype, 0, bits, m, bucket, cap, equal=equal, contiguous=contiguous)
                c = S.bucket_counts(keys, 0, bits, m)
                assert c[bucket] == cap and np.all(np.delete(c, bucket) < cap) and c.sum() == n
                assert S.expected_stats(keys, words, 0, bits)["overflowed"] == 0
                mine = keys[(S.digits(keys, 0, bits) >> np.uint64(bits - m)) == bucket]
                assert (len(np.unique(mine)) == 1) == equal
                if contiguous:
                    where = np.nonzero((S.digits(keys, 0, bits) >> np.uint64(bits - m)) == bucket)[0]
                    assert where[0] % cap == 0 and where[-1] - where[0] == cap - 1
        keys = S.capacity_keys(n, dtype, 0, bits, m, bucket, cap + 1)
        c = S.bucket_counts(keys, 0, bits, m)
        assert c[bucket] == cap + 1 and np.all(np.delete(c, bucket) < cap)
        assert S.expected_stats(keys, words, 0, bits)["overflowed"] == 1


@pytest.mark.parametrize("run", [8, 9])
def test_tie_run_case(run):
    n, m, bucket = 262144, 7, 5
    keys = S.tie_run_keys(n, m, bucket, run)
    c = S.bucket_counts(keys, 0, 63, m)
    assert c[bucket] == 4096 and np.all(np.delete(c, bucket) < 4096)
    mine = np.sort(keys[(keys >> np.uint64(56)) == bucket])
    _, lengths = np.unique(mine >> np.uint64(32), return_counts=True)
    want = [run] * (4096 // run) + [1] * (4096 % run)
    assert sorted(lengths.tolist(), reverse=True) == want
    assert (len(want), sum(want)) == {8: (512, 4096), 9: (456, 4096)}[run]
    assert len(np.unique(mine)) < 4096                   # fully equal keys as well
    assert len(np.unique(mine & U64(0xFFFFFFFF))) > 3000  # and runs that differ in the low bits


# ---- scans ---------------------------------------------------------------------------------------
def test_slabs_and_levels():
    assert [S.n_slabs(n) for n in (1, 8192, 8193, 16384, 16385)] == [1, 1, 2, 2, 3]
    assert [S.levels(n) for n in (1, 8192, 8193, 8192 * 8192, 8192 * 8192 + 1)] == [1, 1, 2, 2, 3]
    assert all(S.levels(n) <= 2 for n in S.SCAN_NS + S.SEG_NS)
    assert [S.levels(n) for n in S.SCAN_BIG_NS] == [2, 3]
    assert S.n_slabs(S.SCAN_BIG_NS[0]) == 8192 and S.n_slabs(S.SCAN_BIG_NS[1]) == 8193
    assert S.n_slabs(S.SEG_TWO_LEVEL_N) == 8194 and S.levels(S.SEG_TWO_LEVEL_N) == 3
    # below 31 a slab sums to less than 2^18 and the largest case to less than 2^31
    assert 30 * S.SCAN_BIG_NS[1] < 1 << 31
    v = S.scan_values(1025)
    assert v.dtype == np.int32 and v.min() >= 0 and v.max() <= 30
    ex, tot = S.scan_ref(v)
    assert ex[0] == 0 and tot == int(v.sum()) and all(ex[i] == int(v[:i].sum()) for i in (1, 2, 1023, 1024))


def _segscan_loop(offsets, data):
    out = np.zeros(len(data), np.float64)
    heads = set(int(o) for o in offsets)
    run = 0.0
    for i in range(len(data)):
        if i in heads:
            run = 0.0
        out[i] = run
        run += float(data[i])
    return out


def test_segscan_reference_against_a_loop_and_the_oracle(oracle):
    rng = np.random.default_rng(3)
    n = 3000
    cuts = np.sort(rng.choice(np.arange(1, n), 40, replace=False))
    offsets = np.concatenate(([0], cuts, cuts[:3], [n])).astype(np.int32)      # empties too
    offsets.sort()
    for dtype in (np.float32, np.float64):
        data = S.seg_integer_data(n, dtype, seed=1)
        ref = S.segscan_ref(offsets, data)
        assert np.array_equal(ref, _segscan_loop(offsets, data))
        assert np.array_equal(oracle.segscan(offsets, data).astype(np.float64), ref)
        assert np.array_equal(S.segscan_ref(offsets, data, acc=np.int32).astype(np.float64), ref)
    # a headless prefix scans as one segment
    data = S.seg_integer_data(50, np.float64)
    assert np.array_equal(S.segscan_ref([3, 10], data), _segscan_loop([0, 3, 10], data))
    assert np.array_equal(S.segscan_ref([], data), _segscan_loop([0], data))


@pytest.mark.parametrize("n", S.SEG_NS)
def test_head_patterns_sit_where_they_say(n):
    seen = set()
    for p in S.SEG_PATTERNS:
        o = S.seg_offsets(p, n)
        if o is None:
            assert (p == "slab-1" and n < 8192) or (p == "empty3_at_slab" and n <= 8192)
            continue
        seen.add(p)
        assert o.dtype == np.int32 and np.all(np.diff(o) >= 0) and (len(o) == 0 or (o[0] >= 0 and o[-1] <= n))
        heads = np.unique(o[o < n]).tolist()
        want = {
            "one": [0], "none": [], "first_at_3": [3], "every": list(range(n)),
            "slab": list(range(0, n, 8192)), "slab-1": list(range(8191, n, 8192)),
            "slab+1": list(range(1, n, 8192)), "chunk": list(range(0, n, 1024)),
            "mod4_0": list(range(0, n, 4)), "mod4_1": list(range(1, n, 4)),
            "mod4_2": list(range(2, n, 4)), "mod4_3": list(range(3, n, 4)),
            "0_and_5": [h for h in (0, 5) if h < n],
            "empty3_at_0": [0, n // 2], "empty3_at_slab": [0, 8192], "empty3_at_last": [0, n - 1],
            "empty3_trailing": [0],
        }[p]
        assert heads == want, p
        if p.startswith("empty3"):
            at = {"empty3_at_0": 0, "empty3_at_slab": 8192, "empty3_at_last": n - 1, "empty3_trailing": n}[p]
            assert int(np.sum(o == at)) == 3
    assert ("one" in seen) and len(seen) >= len(S.SEG_PATTERNS) - 2
    assert set(S.seg_cases()) >= {(p, n) for p in seen}


def test_two_level_case():
    offsets, data = S.two_level_case()
    n = len(data)
    assert n == 8192 * 8192 + 8193 and S.n_slabs(n) > 8192 and S.levels(n) == 3
    assert offsets.tolist() == [0, 5, 8192 * 8192 - 3, 8192 * 8192 + 8192]
    nz = np.flatnonzero(data)
    assert np.all(nz % 4099 == 0) and len(nz) == (n + 4098) // 4099 and np.all(data[nz] == 1.0)
    assert len(nz) < 1 << 15                              # every partial sum is exact in float32
    # the second segment crosses every slab of the first spine slab without a head
    assert offsets[2] - offsets[1] > 8191 * 8192


# ---- sort_by_distance ----------------------------------------------------------------------------
def test_distance_sort_switch_and_keys():
    f32, f64 = np.float32, np.float64
    assert not S.is_composite([65537, 0], f32) and S.is_composite([65538, 0], f32)
    assert S.is_composite([1, 65537], f32) and S.is_composite([32769, 32769], f32)
    assert not S.is_composite([65538, 0], f64)
    assert S.is_composite([150000, 0, 120000, 0], f32) and S.is_composite([150000, 0, 120000, 0, 0], f32)
    assert not S.is_composite(list(S.WAVE_LENGTHS), f32)
    assert [S.composite_bits(r) for r in (1, 2, 3, 4, 5, 8, 9)] == [33, 33, 34, 34, 35, 35, 36]
    assert S.sizes_to_offsets([3, 0, 2, 0]).tolist() == [0, 3, 3, 5]
    d = np.array([-np.inf, -1.5, -0.0, 0.0, 0.125, np.inf, 2.0], f32)
    k = S.composite_keys(d, [3, 4])
    assert (k >> np.uint64(32)).tolist() == [0, 0, 0, 1, 1, 1, 1]
    lo = (k & U64(0xFFFFFFFF)).astype(np.int64)
    assert lo[2] == lo[3] == 0x80000000 and lo[0] < lo[1] < lo[2] < lo[4] < lo[6] < lo[5]
    # the composite case that reaches the 64-bit bucket plan overflows a bucket there
    for sizes in ([150000, 0, 120000, 0], [150000, 0, 120000, 0, 0]):
        dist = S.distances(sum(sizes), f32, seed=2)
        keys = S.composite_keys(dist, sizes)
        bits = S.composite_bits(len(sizes))
        st = S.expected_stats(keys, 0, 0, bits)
        assert st["msd_bits"] == 7 and st["tile"] == 4096 and st["overflowed"] == 1
        assert S.sizes_to_offsets(sizes)[-1] == sum(sizes)
    for sizes in ([65538, 0], [1, 65537], [32769, 32769]):
        assert S.plan(sum(sizes), 8, 0, S.composite_bits(2)) is None and S.n_passes(0, 33) == 5


def test_distances_and_their_order():
    d = S.distances(5000, np.float32, seed=1)
    fin = d[np.isfinite(d)]
    assert np.all(fin * 8 == np.rint(fin * 8)) and fin.min() >= -250 and fin.max() <= 250
    assert np.isposinf(d).any() and np.isneginf(d).any() and not np.isnan(d).any()
    z = d.view(U32)[d == 0]
    assert (z == 0x80000000).any() and (z == 0).any()
    assert len(np.unique(d)) < len(d)
    sizes = [1000, 0, 2500, 1500]
    order = S.segsort_order(d, sizes)
    seg = np.repeat(np.arange(4), sizes)
    assert np.array_equal(seg[order], seg)
    s = d[order]
    for a, b in ((0, 1000), (1000, 3500), (3500, 5000)):
        assert np.all(s[a + 1:b] >= s[a:b - 1])
        same = s[a + 1:b] == s[a:b - 1]
        assert np.all(order[a + 1:b][same] > order[a:b - 1][same])       # -0.0 and +0.0 in input order too
    f = S.fine_distances(4097, seed=1)
    assert np.all(f.astype(np.float32) == 1.0) and len(np.unique(f)) > 2000 and len(np.unique(f)) < 4097


# ---- extrema -------------------------------------------------------------------------------------
def test_extrema_cases():
    assert S.EXTREMA_FIRST_STRIDED == 1024 * 256
    for dtype in (np.float32, np.float64, np.int32):
        for n in (262145,):
            for place in (0, n - 1, S.EXTREMA_FIRST_STRIDED):
                a = S.extrema_rows(n, dtype, place)
                lo, hi = S.extrema_ref(a)
                assert a.dtype == dtype and np.argmin(a[:, 0]) == place and np.argmax(a[:, 1]) == place
                assert lo[2] == a[place, 2] and hi[3] == a[place, 3]
                if dtype == np.int32:
                    assert lo[2] == -2 ** 31 and hi[3] == 2 ** 31 - 1
                else:
                    assert np.isneginf(lo[2]) and np.isposinf(hi[3])
    a = S.extrema_rows(100, np.float32, 7)
    a[::3, 0] = np.nan
    a[:, 1] = np.nan
    lo, hi = S.extrema_ref(a)
    assert lo[0] == np.nanmin(a[:, 0]) and hi[0] == np.nanmax(a[:, 0])
    assert np.isposinf(lo[1]) and np.isneginf(hi[1])
