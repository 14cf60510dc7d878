"""The numpy reference of seed extension (extend_reference.py) against a brute force: a textbook Levenshtein distance of the pattern
to every T[s..e) with lo <= s <= e <= hi, then the definition's choice among them (include/pfpgpu.h, "Extending seeds": the
smallest e that attains d*, then the largest s)."""
import numpy as np

import extend_reference as E


def levenshtein(a, b):
    """unit costs; a byte 0 of a equals nothing"""
    prev = list(range(len(b) + 1))
    for x in a:
        cur = [prev[0] + 1]
        for j, y in enumerate(b):
            cur.append(min(prev[j] + (x != y or x == 0), prev[j + 1] + 1, cur[j] + 1))
        prev = cur
    return prev[-1]


def brute(text, pat, delta, k):
    n, m = len(text), len(pat)
    lo, hi = E.window(n, m, delta, k)
    d = {(s, e): levenshtein(pat, text[s:e]) for s in range(lo, hi + 1) for e in range(s, hi + 1)}
    best = min(d.values())
    if best > k:
        return E.NONE
    e = min(e for (s, e), v in d.items() if v == best)
    s = max(s for (s, e2), v in d.items() if e2 == e and v == best)
    return best, s, e


def test_random_tiny_cases():
    rng = np.random.default_rng(11)
    kinds = set()
    for case in range(1200):
        sigma = int(rng.integers(2, 5))
        n, m = int(rng.integers(0, 30)), int(rng.integers(0, 9))
        text = bytes(rng.integers(1, sigma + 1, n, dtype=np.uint8))
        pat = bytes(rng.integers(0 if case % 7 == 0 else 1, sigma + 2, m, dtype=np.uint8))      # (a byte 0, an absent byte)
        delta = int(rng.integers(-12, n + 13))
        k = (0, 1, 2, 5)[case % 4]
        want = brute(text, pat, delta, k)
        got = E.extend_one(np.frombuffer(text, dtype=np.uint8), pat, delta, k)
        assert got == want, (text, pat, delta, k, got, want)
        kinds.add("none" if want == E.NONE else "hit" if want[0] == 0 else "short" if want[2] - want[1] < m else "long" if want[2] - want[1] > m else "sub")
    assert kinds >= {"none", "hit", "short", "sub"}


def test_hand_cases():
    t = np.frombuffer(b"GATTACA", dtype=np.uint8)
    assert E.extend_one(t, b"", 3, 2) == (0, 1, 1)                 # the empty pattern: (0, lo, lo)
    assert E.extend_one(t, b"", -5, 1) == (0, 0, 0)
    assert E.extend_one(t, b"", 50, 1) == (0, 7, 7)
    assert E.extend_one(t, b"TTA", 40, 2) == E.NONE                # an empty window
    assert E.extend_one(t, b"TTA", 40, 3) == (3, 7, 7)             # ... and k >= m: three insertions
    assert E.extend_one(t, b"TTA", -40, 5) == (3, 0, 0)
    assert E.extend_one(t, b"TTA", 2, 0) == (0, 2, 5)
    assert E.extend_one(t, b"TTA", 3, 0) == E.NONE
    assert E.extend_one(t, b"TTA", 3, 1) == (0, 2, 5)
    assert E.extend_one(t, b"XYZ", 0, 3) == (3, 0, 0) == brute(b"GATTACA", b"XYZ", 0, 3)
    assert E.extend_one(t, b"GATTACAGATTACA", 0, 7) == (7, 0, 7)   # m > n
    assert E.extend_one(t, b"A\x00T", 1, 1) == (1, 1, 3)           # a byte 0 equals nothing: it is deleted
    assert E.extend_one(t, b"A\x00T", 1, 0) == E.NONE
    u = np.frombuffer(b"ZZABXCDZZ", dtype=np.uint8)
    assert E.extend_one(u, b"ABCD", 2, 1) == (1, 2, 7) == brute(b"ZZABXCDZZ", b"ABCD", 2, 1)      # a span longer than the pattern
    assert E.extend_one(u, b"ABXXCD", 2, 1) == (1, 2, 7) == brute(b"ZZABXCDZZ", b"ABXXCD", 2, 1)  # ... and a shorter one
    for pat, delta, k in ((b"TTA", 40, 3), (b"GATTACAGATTACA", 0, 7), (b"A\x00T", 1, 1), (b"TAC", 2, 2)):
        assert E.extend_one(t, pat, delta, k) == brute(b"GATTACA", pat, delta, k)


def test_composite_orders_deduplicates_and_caps():
    t = np.frombuffer(b"ACGTACGTTTACGAACGT", dtype=np.uint8)
    pats = [b"ACGT", b"", b"ACGA"]
    mems = np.array([[0, 4, 14], [0, 4, 0], [0, 4, 4], [1, 3, 1], [0, 4, 10]], dtype=np.uint64)
    mem_off = np.array([0, 4, 4, 5], dtype=np.uint64)
    off, s, e, d = E.align(t, pats, mem_off, mems, 1)
    assert off.tolist() == [0, 3, 3, 4] and s.tolist() == [0, 4, 14, 10] and e.tolist() == [4, 8, 18, 14] and d.tolist() == [0, 0, 0, 0]
    off, s, e, d = E.align(t, pats, mem_off, mems, 1, 2)
    assert off.tolist() == [0, 2, 2, 3] and s.tolist() == [0, 4, 10]
    assert off.dtype == np.uint64 and s.dtype == np.uint64 and e.dtype == np.uint64 and d.dtype == np.uint8
