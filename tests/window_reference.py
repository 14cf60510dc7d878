"""Plain numpy reference for aligning in a window (include/pfpgpu.h, "Aligning in a window"): a full Sellers dynamic programme over
T[lo..hi), one row per pattern byte, the horizontal moves resolved by minimum.accumulate(v - j) + j.  A forward pass with a free
start gives d* and the smallest end e; a second pass of the reversed pattern over the reversed T[lo..e), with a fixed end, gives the
largest start s.  Nothing here comes from the feature under test: last_row is extend_reference's, which test_extend_reference.py
checks against a brute force of its own, and test_window_reference.py checks this file against another."""
import numpy as np

from extend_reference import last_row

NONE = (0xFF, 2**64 - 1, 2**64 - 1)
MAX_W = 16384


def window_one(text, pat, lo, hi, k):
    """(d, s, e) of one candidate; text a uint8 array, pat bytes"""
    t = np.asarray(text, dtype=np.uint8)
    p = np.frombuffer(bytes(pat), dtype=np.uint8)
    lo, hi = int(lo), int(hi)
    if lo > hi or hi > len(t):
        return NONE
    fwd = last_row(p, t[lo:hi], True)                      # entry j: min over s of Levenshtein(P, T[s:lo+j))
    d = int(fwd.min())
    if d > k:
        return NONE
    e = lo + int(np.argmax(fwd == d))
    back = last_row(p[::-1], t[lo:e][::-1], False)         # entry j: Levenshtein(P, T[e-j:e))
    j = int(np.argmax(back == d))
    assert back[j] == d
    return d, e - j, e


def window(text, pats, cand_pat, lo, hi, k):
    """(dist, start, end) as FmIndex.window returns them"""
    res = [window_one(text, pats[p], a, b, k) if 0 <= p < len(pats) else NONE for p, a, b in zip(cand_pat, lo, hi)]
    col = lambda i, dt: np.array([r[i] for r in res], dtype=dt)
    return col(0, np.uint8), col(1, np.uint64), col(2, np.uint64)


def levenshtein(a, b):
    """unit-cost edit distance of two byte strings, the textbook table; a byte 0 of a (the pattern) equals nothing"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        row = [i]
        for j, y in enumerate(b, 1):
            row.append(min(prev[j - 1] + (x != y or x == 0), prev[j] + 1, row[j - 1] + 1))
        prev = row
    return prev[-1]


def brute(text, pat, lo, hi, k):
    """the definition word for word: every pair lo <= s <= e <= hi"""
    tb = bytes(text)
    if lo > hi or hi > len(tb):
        return NONE
    d = {(s, e): levenshtein(pat, tb[s:e]) for s in range(lo, hi + 1) for e in range(s, hi + 1)}
    best = min(d.values())
    if best > k:
        return NONE
    e = min(e for (s, e), v in d.items() if v == best)
    s = max(s for (s, e2), v in d.items() if e2 == e and v == best)
    return best, s, e
