"""Plain numpy reference of the output formats that csrc/runsample.hip writes: 5-byte little-endian integers (`.sa`, utils.c:112-129)
and the `<position, SA value>` pairs at the run boundaries of a BWT (`.ssa` / `.esa`, pfbwt.cpp:169-189, 225-229, 605-676), for the whole
BWT or for a slice that knows one byte of either neighbour.  It calls neither the library nor the oracle; tests/test_formats_reference.py
checks it against the oracle, tests/test_output_formats.py checks the library against it.

A boundary is found by comparing the bytes with themselves shifted by one position; nothing here works in chunks or tiles."""
import numpy as np

MASK40 = (1 << 40) - 1


def pack5(values):
    """the low 40 bits of every value as 5 bytes, little endian"""
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    out = np.empty((len(v), 5), dtype=np.uint8)
    for b in range(5):
        out[:, b] = ((v >> np.uint64(8 * b)) & np.uint64(0xFF)).astype(np.uint8)
    return out.reshape(-1)


def unpack5(packed):
    b = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1, 5).astype(np.uint64)
    v = np.zeros(len(b), dtype=np.uint64)
    for k in range(5):
        v |= b[:, k] << np.uint64(8 * k)
    return v


def run_marks(bwt, lo, hi, left, right, run_end):
    """bool[hi - lo]: which positions of bwt[lo:hi) start (run_end false) or end (run_end true) a run, when the byte just outside the
    slice is `left` / `right` (-1: there is none, the edge position counts).  Only bwt[lo:hi) is read."""
    s = np.ascontiguousarray(bwt, dtype=np.uint8)[lo:hi]
    m = np.ones(len(s), dtype=bool)
    if len(s) == 0:
        return m
    if run_end:
        m[:-1] = s[:-1] != s[1:]
        m[-1] = right < 0 or right != int(s[-1])
    else:
        m[1:] = s[1:] != s[:-1]
        m[0] = left < 0 or left != int(s[0])
    return m


def run_pairs(bwt, sa, lo, hi, left, right, run_end, pos_base):
    """the slice's piece of .ssa / .esa: <pos_base + j - lo, sa[j]> for the marked j of [lo, hi), as 5 + 5 byte records (uint8 array)"""
    j = lo + np.flatnonzero(run_marks(bwt, lo, hi, left, right, run_end))
    pairs = np.empty((len(j), 2), dtype=np.uint64)
    pairs[:, 0] = (j - lo).astype(np.uint64) + np.uint64(pos_base)
    pairs[:, 1] = np.ascontiguousarray(sa).view(np.uint64)[j] if len(j) else 0
    return pack5(pairs.reshape(-1))


def count_pairs(bwt, lo, hi, left, right, run_end):
    return int(run_marks(bwt, lo, hi, left, right, run_end).sum())


def boundary_mask(bwt):
    """the positions whose SA value -s / -e sample: start or end of a run of the whole BWT (j = 0 and the last position among them)"""
    n1 = len(bwt)
    return run_marks(bwt, 0, n1, -1, -1, False) | run_marks(bwt, 0, n1, -1, -1, True)


def true_neighbours(bwt, lo, hi):
    """the bytes just outside [lo, hi) of the whole array, -1 at its ends"""
    return (int(bwt[lo - 1]) if lo > 0 else -1), (int(bwt[hi]) if hi < len(bwt) else -1)


def sliced_pairs(bwt, sa, cuts, run_end):
    """the slices' run_pairs under their true neighbours and pos_base = lo, one array per slice"""
    return [run_pairs(bwt, sa, lo, hi, *true_neighbours(bwt, lo, hi), run_end, lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
