"""The library sorts as the suffix sorter reaches them - rocPRIM under the wrappers of csrc/prims.hip, with their hand-set
onesweep configurations (KeysCfg 1024 x 8 with 9-bit digits, PairsCfg 1024 x 7 from kTunedPairsMin = 6 * 2^20 elements), the
segmented sort's tile (SegCfg) and the work-around for the library's merge path (up to 2^22 elements) - against numpy's
stable argsort.  pfp_debug_lib_sort goes through the wrappers themselves, so a retune of a threshold or a configuration in
prims.hip is what these tests see.

Values are arange(n): the suffix sorter relies on stability for its ties, and any instability shows in them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MERGE_LIMIT = 1 << 20            # the library sorts up to here by merging today (prims.hip: sort_keys_db)
KEYS_WORKAROUND = 1 << 22        # sort_keys_db / sort_keys_raw: begin_bit = 0 up to here when end_bit == 64
TUNED_PAIRS_MIN = 6 << 20        # kTunedPairsMin: PairsCfg from here on
PIV_BITS = 23                    # sufsort.hip kPivBits

TRIVIAL = [1, 2, 255, 256, 257]
DISTS = ("uniform", "half_equal", "constant", "seven")


def around(t):
    return [t - 1, t, t + 1]


def bits_for(n):
    return max(1, int(n).bit_length())


def make_keys(rng, n, dist, bits=64):
    top = np.uint64((1 << bits) - 1)
    if dist == "uniform":
        k = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    elif dist == "half_equal":
        k = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
        k[rng.random(n) < 0.5] = np.uint64(0x9234567890ABCDEF)
    elif dist == "constant":
        k = np.full(n, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    else:
        seven = rng.integers(0, 1 << 63, 7, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
        k = seven[rng.integers(0, 7, n)]
    return np.ascontiguousarray(k & top)


def dists_for(n, i):
    """all four distributions up to the merge limit; on the multi-million sizes (where numpy's argsort is what costs) one per
    bit range, rotating with the range and the size, so that the three sizes around a threshold see all four between them"""
    return DISTS if n <= MERGE_LIMIT + 1 else (DISTS[(i + n) % 4],)


def mask_of(lo, hi):
    return np.uint64(((1 << hi) - 1) ^ ((1 << lo) - 1))


@pytest.mark.parametrize("n", TRIVIAL + around(MERGE_LIMIT) + around(KEYS_WORKAROUND) + around(TUNED_PAIRS_MIN))
def test_pair_sorts_at_the_wrappers_thresholds(ctx, n):
    """sort_pairs_db<u64,u32> and <u64,u64> with the bit ranges of `doubling`: (0, kbits + 1) of the first round (a full and a
    37-bit key), (0, nb + kPivBits) of a pivot round and (0, 2 nb) of a doubling round.  Keys carry random bits above end_bit:
    the sort must ignore them."""
    rng = np.random.default_rng(n)
    nb = bits_for(n)
    for i, (lo, hi) in enumerate(((0, 64), (0, 37), (0, nb + PIV_BITS), (0, 2 * nb))):
        for dist in dists_for(n, i):
            keys = make_keys(rng, n, dist)
            order = np.argsort(keys & mask_of(lo, hi), kind="stable")
            for kind, vt in (("pairs_u64_u32", np.uint32), ("pairs_u64_u64", np.uint64)):
                got, vals = keys.copy(), np.arange(n, dtype=vt)
                ctx.debug_lib_sort(kind, got, vals, lo, hi)
                assert np.array_equal(vals, order.astype(vt)), (kind, n, lo, hi, dist, "order / stability")
                assert np.array_equal(got, keys[order]), (kind, n, lo, hi, dist, "keys")


@pytest.mark.parametrize("n", TRIVIAL + around(MERGE_LIMIT) + around(KEYS_WORKAROUND) + around(TUNED_PAIRS_MIN))
def test_key_sorts_at_the_wrappers_thresholds(ctx, n):
    """sort_keys_db / sort_keys_raw as the keys-only first round calls them: the word is (key << idx_bits | position), sorted
    on (idx_bits, 64) - the combination the library's merge path gets wrong, worked around up to 2^22 elements - and on
    (idx_bits, idx_bits + 36) where the key was shortened to whole 9-bit passes"""
    rng = np.random.default_rng(n + 1)
    ib = bits_for(n - 1)
    for i, (lo, hi) in enumerate(((ib, 64), (ib, ib + 36))):
        for dist in dists_for(n, i):
            keys = (make_keys(rng, n, dist, hi - lo) << np.uint64(lo)) | np.arange(n, dtype=np.uint64)
            want = keys[np.argsort(keys & mask_of(lo, hi), kind="stable")]
            for kind in ("keys_db", "keys_raw"):
                got = keys.copy()
                ctx.debug_lib_sort(kind, got, None, lo, hi)
                assert np.array_equal(got, want), (kind, n, lo, hi, dist)


def seg_layouts():
    """name -> segment lengths (in order; None = a gap of 5 elements that belongs to no segment)"""
    rng = np.random.default_rng(99)
    # SegCfg (prims.hip): warp sorts of up to 8 x 4 = 32 and 16 x 8 = 128 elements, a workgroup tile of 256 x 4 = 1024,
    # radix passes above that; segments are partitioned by size once there are more than a few dozen of them
    edges = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097]
    return {
        "config_edges_x4": edges * 4,
        "config_edges_once_with_gaps": [x for e in edges for x in (e, None)],
        "exactly_2^15": [5, (1 << 15), 0, (1 << 15) - 1, 1, 2, (1 << 15)],      # the longest segment the sorter hands over
        "thousands_of_24_to_64": [int(x) for x in rng.integers(24, 65, size=5000)],
        "ones_and_twos_and_empty": [int(x) for x in rng.integers(0, 3, size=3000)],
    }


def segments(lengths):
    begin, end, pos = [], [], 0
    for ln in lengths:
        if ln is None:
            pos += 5
            continue
        begin.append(pos)
        end.append(pos + ln)
        pos += ln
    return np.array(begin, dtype=np.uint32), np.array(end, dtype=np.uint32), pos


@pytest.mark.parametrize("layout", list(seg_layouts()))
def test_segmented_sorts_per_segment(ctx, layout):
    """segsort_pairs_u32 (u32 and u64 values) on (0, kPivBits) and (0, bits_for(N)), segsort_pairs_u64_u32 on (0, 32 + 12) of the
    parse's pivot rounds: every segment against numpy's stable argsort of its own keys; what lies outside every segment
    stays where it was"""
    begin, end, n = segments(seg_layouts()[layout])
    rng = np.random.default_rng(len(begin))
    for kind, kt, vt, ranges in (("seg_u32_u32", np.uint32, np.uint32, ((0, PIV_BITS), (0, bits_for(n)))),
                                 ("seg_u32_u64", np.uint32, np.uint64, ((0, PIV_BITS),)),
                                 ("seg_u64_u32", np.uint64, np.uint32, ((0, 32 + 12),))):
        for lo, hi in ranges:
            for dist in DISTS:
                keys = make_keys(rng, n, dist)
                if kt == np.uint32:
                    keys = np.ascontiguousarray((keys >> np.uint64(17)).astype(np.uint32))
                masked = keys & kt(((1 << hi) - 1) ^ ((1 << lo) - 1))
                order = np.arange(n)
                for b, e in zip(begin.tolist(), end.tolist()):
                    order[b:e] = b + np.argsort(masked[b:e], kind="stable")
                got, vals = keys.copy(), np.arange(n, dtype=vt)
                ctx.debug_lib_sort(kind, got, vals, lo, hi, begin, end)
                assert np.array_equal(vals, order.astype(vt)), (kind, layout, lo, hi, dist, "order / stability")
                assert np.array_equal(got, keys[order]), (kind, layout, lo, hi, dist, "keys")


@pytest.mark.parametrize("n", TRIVIAL + [4095, 4096, 4097] + around(MERGE_LIMIT) + [KEYS_WORKAROUND + 1, TUNED_PAIRS_MIN + 1])
def test_scans_and_selection(ctx, n):
    """inclusive_max_u32, exclusive_sum_u32_u64 and select_index (4096 flags per workgroup), which sort_int_suffixes and
    `doubling` build on"""
    rng = np.random.default_rng(n + 2)
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    a[rng.random(n) < 0.7] = 0                 # (the callers' marks: mostly 0)
    got = a.copy()
    ctx.debug_lib_sort("inclusive_max_u32", got)
    assert np.array_equal(got, np.maximum.accumulate(a))
    out = np.zeros(n, dtype=np.uint64)
    big = rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64).astype(np.uint32)      # sums beyond 32 bits after two elements
    ctx.debug_lib_sort("exclusive_sum_u32_u64", big, out)
    want = np.zeros(n, dtype=np.uint64)
    want[1:] = np.cumsum(big.astype(np.uint64))[:-1]
    assert np.array_equal(out, want)
    for density in (0.0, 0.01, 0.5, 1.0):
        flags = (rng.random(n) < density).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)      # any non-zero byte counts
        sel = np.full(n + 1, 0xFFFFFFFF, dtype=np.uint32)
        ctx.debug_lib_sort("select_index", flags, sel)
        want = np.flatnonzero(flags).astype(np.uint32)
        assert int(sel[n]) == len(want), (n, density)
        assert np.array_equal(sel[:len(want)], want), (n, density)
