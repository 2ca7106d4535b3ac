"""Cases and references for the sort, the scans, the per-segment distance sort and the extrema at the
sizes where their code changes path (tests/test_sort_scan_boundaries.py runs them on the GPU,
tests/test_sort_scan_boundary_cases.py pins this module on the CPU).  NumPy only.

The decisions of csrc/sort.hip (bucket_plan, local_tile), csrc/scan.hip (slabs, levels) and
csrc/segsort.hip (wave sort or composite keys) are restated here so that a GPU case can say which
path it expects and assert it through grace_sort_last_stats; the CPU tests pin the restatement to
numbers worked out by hand from the source."""
import numpy as np

U32, U64 = np.uint32, np.uint64

# ---- csrc/sort.hip -------------------------------------------------------------------------------
INDEX_SORT_BELOW = 1 << 18      # bucket_plan refuses smaller inputs
MAX_MSD_BITS = 12               # LS_MAX_MSD_BITS
RADIX_BITS = 8                  # digit of an index-sort pass


def tile(key_bytes, words):
    """local_tile: records per bucket tile = the capacity of a bucket."""
    return 4096 if key_bytes == 8 or words > 4 else 8192


def plan(n, key_bytes, words, bits):
    """bucket_plan: the bucket digit's width m, or None where the index sort runs."""
    if words > 9 or n < INDEX_SORT_BELOW or bits <= 16:
        return None
    t = tile(key_bytes, words)
    m = 1
    while m < MAX_MSD_BITS and (n >> m) * 10 > t * 6:
        m += 1
    if (n >> m) * 4 > t * 3:            # mean bucket above 75 % of a workgroup
        return None
    if m > bits:
        return None
    if bits - m > 24 and key_bytes < 8:  # 32-bit keys: at most 24 bits below the digit
        return None
    return m


def n_passes(begin, end):
    return (end - begin + RADIX_BITS - 1) // RADIX_BITS


def digits(keys, begin, end):
    """The sort key proper: bits [begin, end) of the stored key, as uint64."""
    mask = np.uint64((1 << (end - begin)) - 1)
    return (keys.astype(U64) >> np.uint64(begin)) & mask


def bucket_counts(keys, begin, end, m):
    """Histogram over the top m bits of the bit range: what bucket_bases_kernel compares with the
    capacity."""
    d = digits(keys, begin, end) >> np.uint64(end - begin - m)
    return np.bincount(d.astype(np.int64), minlength=1 << m)


def expected_stats(keys, words, begin, end):
    """msd_bits / tile / overflowed of grace_sort_last_stats for sort_by_key(keys, values of `words`
    32-bit words, begin, end) with the overflow hint off."""
    kb = keys.dtype.itemsize
    m = plan(len(keys), kb, words, end - begin)
    t = tile(kb, words)
    if m is None:
        return {"msd_bits": 0, "tile": t, "hint_skipped": 0, "overflowed": -1}
    over = int(bucket_counts(keys, begin, end, m).max() > t)
    return {"msd_bits": m, "tile": t, "hint_skipped": 0, "overflowed": over}


def stable_order(keys, begin, end):
    return np.argsort(digits(keys, begin, end), kind="stable")


def _random_keys(rng, n, dtype, bits):
    if bits == 64:
        k = rng.integers(0, 1 << 63, n, dtype=U64) | (rng.integers(0, 2, n, dtype=U64) << np.uint64(63))
    else:
        k = rng.integers(0, 1 << bits, n, dtype=U64)
    return k.astype(dtype)


def uniform_keys(n, dtype, bits, seed=0):
    """Uniform keys of `bits` bits; 2 % of them keep only their top 14 bits (more than any bucket
    digit: the histogram stays uniform), so that equal keys exist and stability is visible."""
    rng = np.random.default_rng([seed, n, bits])
    k = _random_keys(rng, n, dtype, bits)
    if bits > 14:
        keep = dtype(((1 << 14) - 1) << (bits - 14))
        k[: n // 50] &= keep
        k = k[rng.permutation(n)]
    return k


def payload(n, words, seed=0):
    if words == 0:
        return None
    return np.random.default_rng([seed, n, words]).integers(-(1 << 31), 1 << 31, (n, words), dtype=np.int64).astype(np.int32)


# (n, key dtype, words, begin, end): both sides of every size at which bucket_plan changes m, tile
# or verdict.  16 B on the 8192-record tile, 0 B and 28 B on the 4096-record one.
PLAN_TABLE = [
    # n, key bytes, words, bits, m
    (262143, 4, 4, 30, None), (262144, 4, 4, 30, 6),
    (314623, 4, 4, 30, 6), (314624, 4, 4, 30, 7),
    (1258495, 4, 4, 30, 8), (1258496, 4, 4, 30, 9),
    (629247, 8, 0, 63, 8), (629248, 8, 0, 63, 9),
    (12587007, 8, 0, 63, 12), (12587008, 8, 0, 63, None),
    (262144, 4, 4, 31, None), (262144, 4, 4, 32, None),
    (262144, 4, 7, 30, 7), (262144, 8, 4, 63, 7),
]
BIG_SORT_NS = (12587007, 12587008)


def plan_boundary_cases():
    """(n, dtype, words, begin, end) of the GPU's plan-boundary sorts (the 12.6 M pair runs apart)."""
    out = []
    for n in (262143, 262144, 314623, 314624, 1258495, 1258496):
        out.append((n, U32, 4, 0, 30))
    for n in (262143, 262144):
        for w in (0, 7):                 # (32-bit keys: 0 B sorts on the 8192-record tile, 28 B on the 4096 one)
            out.append((n, U32, w, 0, 30))
    for n in (629247, 629248):
        for w in (0, 7):
            out.append((n, U64, w, 0, 63))
    for bits in (31, 32):
        out.append((262144, U32, 4, 0, bits))
    out.append((262144, U64, 4, 0, 63))
    # full-width 32-bit keys where 24 bits or fewer are left below the digit
    out.append((629248, U32, 4, 0, 32))
    out.append((314624, U32, 4, 0, 31))
    out.append((314624, U32, 4, 1, 32))
    return out


def capacity_keys(n, dtype, begin, end, m, bucket, count, equal=False, contiguous=False, seed=0):
    """n keys of which exactly `count` fall into `bucket` (top m bits of [begin, end)), the others
    uniform over the other buckets.  equal: the bucket's keys are one value.  contiguous: they are
    one aligned run of the input (a tile of the scatter kernel holds nothing else)."""
    rng = np.random.default_rng([seed, n, m, bucket, count])
    bits = end - begin
    low = bits - m
    others = np.array([b for b in range(1 << m) if b != bucket], dtype=U64)
    d = others[rng.integers(0, len(others), n)]
    lo = rng.integers(0, 1 << min(low, 62), n, dtype=U64)
    if equal:
        lo_b = np.full(count, 0x5555555555555555 & ((1 << low) - 1), dtype=U64)
    else:
        lo_b = rng.integers(0, 1 << min(low, 62), count, dtype=U64)
    if contiguous:
        start = 3 * count if 4 * count <= n else 0
        where = np.arange(start, start + count)
    else:
        where = np.sort(rng.choice(n, count, replace=False))
    d[where] = np.uint64(bucket)
    lo[where] = lo_b
    k = ((d << np.uint64(low)) | lo) << np.uint64(begin)
    # bits outside [begin, end) are noise the sort must ignore
    if begin:
        k |= rng.integers(0, 1 << begin, n, dtype=U64)
    return k.astype(dtype)


def tie_run_keys(n, m, bucket, run, cap=4096, seed=0):
    """63-bit keys (bits [0, 63), 64-bit tile): `bucket` holds exactly `cap` records in runs of `run`
    records that agree on every bit the LDS passes cover (bits 32 and up) and differ, or not, in the 32
    bits below; cap % run single records fill the bucket up.  Every other bucket: uniform keys."""
    rng = np.random.default_rng([seed, n, run])
    k = capacity_keys(n, U64, 0, 63, m, bucket, cap, seed=seed)
    where = np.nonzero((k >> np.uint64(63 - m)) == np.uint64(bucket))[0]
    n_runs = cap // run
    n_pref = n_runs + cap % run
    mid_bits = 63 - m - 32
    pref = rng.choice(1 << mid_bits, n_pref, replace=False).astype(U64)
    reps = np.concatenate([np.full(n_runs, run), np.ones(cap % run, dtype=np.int64)]).astype(np.int64)
    mid = np.repeat(pref, reps)
    low = rng.integers(0, 1 << 32, cap, dtype=U64)
    low[::5] = 0                                        # fully equal keys too: stability
    kb = (np.uint64(bucket) << np.uint64(63 - m)) | (mid << np.uint64(32)) | low
    k[where] = kb[rng.permutation(cap)]
    return k


INDEX_NS = (2, 4095, 4096, 4097, 8193)
INDEX_RANGES_U32 = ((0, 8), (4, 20), (3, 27), (0, 30), (0, 32), (24, 32))
INDEX_RANGES_U64 = ((0, 8), (0, 16), (5, 29), (0, 32), (0, 40), (16, 64), (0, 56), (0, 63), (0, 64))
PAYLOAD_WORDS = (0, 1, 2, 3, 4, 7, 8, 9)
GATHER_GRID_STRIDE_N = 1048577          # gather_words_kernel: 4096 workgroups of 256 = 1048576 threads


def outside_ones_keys(n, dtype, begin, end):
    """All ones outside [begin, end), all zeros inside: every key's digit is 0."""
    full = (1 << (8 * np.dtype(dtype).itemsize)) - 1
    inside = ((1 << (end - begin)) - 1) << begin
    return np.full(n, full & ~inside, dtype=dtype)


# ---- csrc/scan.hip -------------------------------------------------------------------------------
SLAB, CHUNK, VEC = 8192, 1024, 4
SCAN_NS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 8191, 8192, 8193, 16384, 16385)
SCAN_BIG_NS = (SLAB * SLAB, SLAB * SLAB + 1)
SEG_NS = (5, 1023, 1024, 1025, 8191, 8192, 8193, 24576, 24577, 3 * SLAB + 5)
SEG_TWO_LEVEL_N = SLAB * SLAB + SLAB + 1


def n_slabs(n):
    return (n + SLAB - 1) // SLAB


def levels(n):
    """Kernels stacked by the recursion of exclusive_scan_u32 / seg_spine: 1 for a single slab, one
    more for every time the slab sums themselves need more than a slab."""
    k = 1
    while n_slabs(n) > 1:
        n = n_slabs(n)
        k += 1
    return k


def scan_values(n, seed=0):
    """int32 below 31: every total of the sizes used here stays below 2^31."""
    return np.random.default_rng([seed, n]).integers(0, 31, n, dtype=np.int32)


def scan_ref(v):
    """(exclusive prefix, total) in int64."""
    c = np.cumsum(v, dtype=np.int64)
    return np.concatenate(([0], c[:-1])), int(c[-1]) if len(v) else 0


SEG_PATTERNS = ("one", "none", "first_at_3", "every", "slab", "slab-1", "slab+1", "chunk",
                "mod4_0", "mod4_1", "mod4_2", "mod4_3", "0_and_5",
                "empty3_at_0", "empty3_at_slab", "empty3_at_last", "empty3_trailing")


def seg_offsets(pattern, n):
    """CSR segment starts (int32, one per segment) of a head pattern over n elements, or None where
    the pattern does not exist at this n.  Elements before the first start belong to no listed
    segment: they scan as one headless segment."""
    a = np.arange(n, dtype=np.int64)
    if pattern == "one":
        o = [0]
    elif pattern == "none":
        o = []
    elif pattern == "first_at_3":
        o = [3]
    elif pattern == "every":
        o = a
    elif pattern == "slab":
        o = a[::SLAB]
    elif pattern == "slab-1":
        o = a[SLAB - 1::SLAB]
        if len(o) == 0:
            return None
    elif pattern == "slab+1":
        o = a[1::SLAB]
    elif pattern == "chunk":
        o = a[::CHUNK]
    elif pattern.startswith("mod4_"):
        o = a[int(pattern[-1])::VEC]
    elif pattern == "0_and_5":
        o = [0, 5]
    elif pattern == "empty3_at_0":
        o = [0, 0, 0, n // 2]
    elif pattern == "empty3_at_slab":
        if n <= SLAB:
            return None
        o = [0, SLAB, SLAB, SLAB]
    elif pattern == "empty3_at_last":
        o = [0, n - 1, n - 1, n - 1]
    elif pattern == "empty3_trailing":
        o = [0, n, n, n]
    else:
        raise ValueError(pattern)
    return np.asarray(o, dtype=np.int32)


def seg_cases():
    return [(p, n) for n in SEG_NS for p in SEG_PATTERNS if seg_offsets(p, n) is not None]


def seg_head_index(offsets, n, dtype=np.int64):
    """For every element the index of its segment's first element (0 for the headless prefix)."""
    head = np.zeros(n, dtype=dtype)
    o = np.asarray(offsets, dtype=np.int64)
    o = o[o < n]
    head[o] = o
    return np.maximum.accumulate(head)


def segscan_ref(offsets, data, acc=np.float64):
    """Exclusive segmented scan in `acc` precision: the exclusive running sum minus its value at the
    element's segment head."""
    n = len(data)
    c = np.cumsum(data, dtype=acc)
    excl = np.empty(n, dtype=acc)
    excl[0] = 0
    excl[1:] = c[:-1]
    del c
    head = seg_head_index(offsets, n, np.int64 if n >= 1 << 31 else np.int32)
    return excl - excl[head]


def seg_integer_data(n, dtype, seed=0):
    """Integer-valued reals in [-15, 15]: every partial sum of the sizes used here is exact."""
    return np.random.default_rng([seed, n]).integers(-15, 16, n).astype(dtype)


def two_level_case():
    """(offsets, data) of the one case whose slab aggregates need a spine of their own."""
    n = SEG_TWO_LEVEL_N
    data = np.zeros(n, np.float32)
    data[::4099] = 1.0
    offsets = np.array([0, 5, SLAB * SLAB - 3, SLAB * SLAB + SLAB], dtype=np.int32)
    return offsets, data


# ---- csrc/segsort.hip ----------------------------------------------------------------------------
WAVE_SORT_MAX_MEAN = 32768
WAVE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4097)


def sizes_to_offsets(sizes):
    s = np.asarray(sizes, dtype=np.int64)
    return (np.cumsum(s) - s).astype(np.int32)


def is_composite(sizes, dtype):
    """sort_by_distance: float32 distances with a mean segment above 32768 take the composite-key
    sort; everything else one wavefront per segment."""
    n_hits, n_rays = int(np.sum(sizes)), len(sizes)
    return np.dtype(dtype) == np.float32 and n_hits >= 2 and n_rays > 0 and n_hits // n_rays > WAVE_SORT_MAX_MEAN


def composite_bits(n_rays):
    seg_bits = 1
    while (1 << seg_bits) < n_rays and seg_bits < 31:
        seg_bits += 1
    return 32 + seg_bits


def composite_keys(dist, sizes):
    """segment << 32 | order-preserving bits of the float32 distance (-0 counts as +0)."""
    d = np.asarray(dist, np.float32) + np.float32(0.0)          # -0 + 0 = +0
    u = d.view(U32)
    u = np.where(u & U32(0x80000000), ~u, u | U32(0x80000000))
    seg = np.repeat(np.arange(len(sizes), dtype=U64), sizes)
    return (seg << np.uint64(32)) | u.astype(U64)


def distances(n, dtype, seed=0):
    """Multiples of 0.125 in [-250, 250] (4001 values: ties from a few thousand hits on), a few -0.0,
    +inf and -inf.  No NaN."""
    rng = np.random.default_rng([seed, n])
    d = (rng.integers(-2000, 2001, n) * 0.125).astype(dtype)
    for value in (-0.0, 0.0, np.inf, -np.inf):
        k = max(1, n // 500) if n >= 8 else 0
        d[rng.integers(0, max(n, 1), k)] = value
    return d


def fine_distances(n, seed=0):
    """float64 distances that differ only below float32 precision: 1 + k 2^-40."""
    k = np.random.default_rng([seed, n]).integers(0, 1 << 14, n)
    return 1.0 + k.astype(np.float64) * 2.0 ** -40


def segsort_order(dist, sizes):
    """Per-segment stable order by distance (np.lexsort compares -0.0 == +0.0 and is stable)."""
    seg = np.repeat(np.arange(len(sizes)), sizes)
    return np.lexsort((np.arange(len(dist)), dist, seg))


# ---- csrc/extrema.hip ----------------------------------------------------------------------------
EXTREMA_NS = (262144, 262145, 1048577)
EXTREMA_FIRST_STRIDED = 262144          # 1024 workgroups of 256: the first element reached by striding


def extrema_rows(n, dtype, place, seed=0):
    """(n, 4) rows of moderate values with one extreme row at index `place`: column 0 the finite
    minimum, column 1 the finite maximum, column 2 -inf / INT32_MIN, column 3 +inf / INT32_MAX."""
    rng = np.random.default_rng([seed, n, place])
    dtype = np.dtype(dtype)
    if dtype.kind == "i":
        a = rng.integers(-1000, 1001, (n, 4)).astype(dtype)
        a[place] = [-(1 << 20), 1 << 20, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    else:
        a = rng.uniform(-100.0, 100.0, (n, 4)).astype(dtype)
        a[place] = [-1e6, 1e6, -np.inf, np.inf]
    return a


def extrema_ref(a):
    """Column minima and maxima, NaN skipped; a column of NaN only gives (+inf, -inf)."""
    if a.dtype.kind == "i":
        return a.min(axis=0), a.max(axis=0)
    lo = np.where(np.isnan(a), np.inf, a).min(axis=0).astype(a.dtype)
    hi = np.where(np.isnan(a), -np.inf, a).max(axis=0).astype(a.dtype)
    return lo, hi
