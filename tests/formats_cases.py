"""Inputs of tests/test_output_formats.py: byte arrays built from run lengths - pfp_sample_runs_dev needs no real BWT, only bytes and
one 64-bit value per byte - with their cut lists, and the text of the distributed case.  tests/test_formats_reference.py asserts that
each array holds the runs the tables of tests/README.md name; nothing here calls the library."""
import functools

import numpy as np

import formats_reference as FR

CHUNK, TILE = 16, 4096          # positions per thread and per workgroup of run_count_kernel / run_place_kernel
EDGE_POINTS = (15, 16, 17, 4095, 4096, 4097, 8192)          # a run begins at each of these, and a run ends at each of these
SPECIAL_SA = (0, (1 << 32) - 1, 1 << 32, (1 << 40) - 1)      # both halves of the pair store's v << 40 / v >> 24 split
POS_BASES = ("zero", "small", "top")
SLICE_LENGTHS = (1, 2, 15, 16, 17, 31, 33, 0, 4095, 4096, 4097)
PACK_COUNTS = tuple(range(1, 18)) + (255, 256, 257, 819, 820, 4095, 4096, 4097, 65537)
PACK_OUT_OFFSETS = (0, 1, 5, 15)


def from_runs(lengths, symbols):
    return np.repeat(np.asarray(symbols, dtype=np.uint8), np.asarray(lengths, dtype=np.int64))


def run_starts(a):
    return np.flatnonzero(FR.run_marks(a, 0, len(a), -1, -1, False))


def _distinct_symbols(rng, k, alphabet):
    """k symbols of the alphabet, no two neighbours equal: every run keeps the length it was given"""
    alphabet = np.asarray(alphabet, dtype=np.uint8)
    idx = np.empty(k, dtype=np.int64)
    idx[0] = rng.integers(len(alphabet))
    step = rng.integers(1, len(alphabet), size=k)
    for i in range(1, k):
        idx[i] = (idx[i - 1] + step[i]) % len(alphabet)
    return alphabet[idx]


@functools.lru_cache(maxsize=None)
def array(name):
    """the named byte array (read-only)"""
    rng = np.random.default_rng(2024)
    if name == "constant":              # one run over three tiles and a part: no boundary but the array's ends
        a = np.full(3 * TILE + 777, ord("G"), dtype=np.uint8)
    elif name == "alternating":         # every position a boundary: a tile holds 4096 pairs, 1024 per wave
        a = np.tile(np.frombuffer(b"AC", dtype=np.uint8), 2 * TILE)[: 3 * TILE + 537].copy()
    elif name == "random_runs":         # runs of 1..40
        lengths = rng.integers(1, 41, size=800)
        a = from_runs(lengths, _distinct_symbols(rng, len(lengths), np.frombuffer(b"ACGTN", dtype=np.uint8)))
    elif name == "edges":               # runs that begin, and runs that end, exactly at 15, 16, 17, 4095, 4096, 4097, 8192
        starts = sorted({0} | set(EDGE_POINTS) | {x + 1 for x in EDGE_POINTS})
        ends = starts[1:] + [2 * TILE + 50]
        a = from_runs([e - s for s, e in zip(starts, ends)], _distinct_symbols(rng, len(starts), np.frombuffer(b"ACG", dtype=np.uint8)))
    elif name == "extremes":            # bytes 0 and 255 next to each other, in both orders; 1 and 254 next to them
        lengths = rng.integers(1, 6, size=1200)
        a = from_runs(lengths, _distinct_symbols(rng, len(lengths), [0, 255, 1, 254]))
    else:
        raise KeyError(name)
    a.setflags(write=False)
    return a


ARRAYS = ("constant", "alternating", "random_runs", "edges", "extremes")
SLICED = ("random_runs", "alternating", "constant")          # long enough for cut_list


@functools.lru_cache(maxsize=None)
def sa_values(name):
    """one u64 below 2^40 per byte of array(name), all different, as a suffix array's are; the special values sit at boundaries"""
    a = array(name)
    rng = np.random.default_rng(len(a))
    v = (rng.permutation(len(a)).astype(np.uint64) * np.uint64(104729977) + np.uint64(12345)) & np.uint64(FR.MASK40)
    b = np.flatnonzero(FR.boundary_mask(a))
    for i, j in enumerate(b[:8]):
        v[j] = SPECIAL_SA[i % 4]
    v.setflags(write=False)
    return v


def pos_base(kind, count):
    return {"zero": 0, "small": 12345, "top": (1 << 40) - count}[kind]


@functools.lru_cache(maxsize=None)
def embedded(name):
    """array(name) as the slice [lo, hi) of a larger array with random runs on either side: (big, sa of big, lo, hi)"""
    a = array(name)
    rng = np.random.default_rng(7)
    sym = np.frombuffer(b"ACGT", dtype=np.uint8)
    before = from_runs(rng.integers(1, 9, size=150), _distinct_symbols(rng, 150, sym))
    after = from_runs(rng.integers(1, 9, size=150), _distinct_symbols(rng, 150, sym))
    lo = len(before) | 1          # an odd offset
    big = np.concatenate([before, before[: lo - len(before)], a, after])
    sa = (np.random.default_rng(8).permutation(len(big)).astype(np.uint64) * np.uint64(2654435761) + np.uint64(99)) & np.uint64(FR.MASK40)
    sa[lo: lo + len(a)] = sa_values(name)
    big.setflags(write=False)
    sa.setflags(write=False)
    return big, sa, lo, lo + len(a)


@functools.lru_cache(maxsize=None)
def cut_list(name):
    """cuts of array(name), one of SLICED: slices of the lengths of SLICE_LENGTHS from the front, then - where the array has runs of
    7 or more behind them - around one run start s (one before it, on it, one after it) and around the middle of a later long run,
    then the rest.  (An array of one run, or of runs of one, is cut at the same places: every cut is alike there.)"""
    a = array(name)
    cuts = [0]
    for ln in SLICE_LENGTHS:
        cuts.append(cuts[-1] + ln)
    starts = run_starts(a)
    lengths = np.diff(np.append(starts, len(a)))
    later = np.flatnonzero((starts > cuts[-1] + 8) & (lengths >= 7) & (starts + lengths < len(a)))
    if len(later) >= 2:
        s = int(starts[later[0]])
        mid = int(starts[later[1]]) + int(lengths[later[1]]) // 2          # at least three positions from either end of its run
    else:
        s, mid = cuts[-1] + 100, cuts[-1] + 300
    cuts += [s - 1, s, s + 1, mid, mid + 1, len(a)]
    assert cuts == sorted(cuts)
    return tuple(cuts)


def pack_values(count, kind):
    """u64[count]: "low" = 0 and 2^40 - 1 at fixed places among random 40-bit values; "high" = the same with random bits 40..63;
    "ones" = all 64 bits set"""
    rng = np.random.default_rng(count)
    v = rng.integers(0, 1 << 40, size=count, dtype=np.uint64)
    v[0::7] = 0
    v[3::7] = FR.MASK40
    if count >= 2:
        v[-1] = FR.MASK40
    if kind == "high":
        hi = rng.integers(1, 1 << 24, size=count, dtype=np.uint64)
        v = v | (hi << np.uint64(40))
    elif kind == "ones":
        v = np.full(count, np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    else:
        assert kind == "low"
    return v


# ---------------------------------------------------------------------------------------- the distributed case
RUN = 16000


def dist_case(O, R):
    """share_cases.run_text: random DNA on either side of RUN copies of one letter, -w 4 -p 11; the text is cut into R shards so that
    the run - which holds no phrase end - lies inside one of them.  Returns dict(text, cuts, w, p, halo)."""
    import share_cases
    text, cuts4 = share_cases.run_text(O, RUN)
    n = len(text)
    if R == 4:
        cuts = cuts4
    else:
        head = [3000 * r // (R // 2) for r in range(R // 2)]                   # R/2 - 1 shards before the run, one that holds it
        tail = [3000 + RUN + 3000 * r // (R - R // 2 + 1) for r in range(1, R - R // 2 + 1)]
        cuts = tuple(head + tail + [n])
    assert len(cuts) == R + 1 and list(cuts) == sorted(set(cuts))
    return dict(text=text, cuts=tuple(cuts), w=4, p=11, halo=1 << 16)


def longest_run(bwt):
    """[a, b) of the longest run of equal bytes"""
    s = run_starts(bwt)
    ln = np.diff(np.append(s, len(bwt)))
    k = int(np.argmax(ln))
    return int(s[k]), int(s[k] + ln[k])
