"""The reference of test_fm_window.py (window_reference.py) against three things that do not share its code path: a brute force over
every pair (s, e) with a textbook Levenshtein table, literals worked by hand, and extend_reference on the window that a diagonal
gives - there the two sections of pfpgpu.h define the same thing.  No GPU."""
import numpy as np
import pytest

import extend_reference as E
import window_reference as W

NONE = W.NONE


@pytest.mark.parametrize("alphabet", [b"ab", b"ACGT"])
def test_against_brute_force(alphabet):
    rng = np.random.default_rng(len(alphabet))
    letters = np.frombuffer(alphabet, dtype=np.uint8)
    seen = set()
    for _ in range(600):
        n, m = int(rng.integers(0, 13)), int(rng.integers(0, 6))
        text = rng.choice(letters, n).astype(np.uint8)
        pat = bytes(rng.choice(letters, m).astype(np.uint8))
        lo = int(rng.integers(0, n + 1))
        hi = int(rng.integers(lo, n + 1))
        for k in (0, 1, 2, 5):
            got, want = W.window_one(text, pat, lo, hi, k), W.brute(text, pat, lo, hi, k)
            assert got == want, (bytes(text), pat, lo, hi, k, got, want)
            seen.add("none" if want == NONE else "exact" if want[0] == 0 else "edits")
            if want != NONE and want[1] == want[2] and m:
                seen.add("empty span")
    assert seen == {"none", "exact", "edits", "empty span"}


# (text, pattern, lo, hi, k) -> (d, s, e), each worked by hand from the definition
LITERALS = [
    # two exact occurrences: the one that ends first (a tie in e)
    ((b"abab", b"ab", 0, 4, 0), (0, 0, 2)),
    # d(0, 2) = d(1, 2) = 1 ("ca" and "a" against "ba"): the largest start (a tie in s); no end below 2 reaches 1
    ((b"caa", b"ba", 0, 3, 1), (1, 1, 2)),
    # the same with d* = k + 1
    ((b"caa", b"ba", 0, 3, 0), NONE),
    # d* = k = 2: nothing of "zz" is in the text, the empty span at lo is the first end
    ((b"abc", b"zz", 1, 3, 2), (2, 1, 1)),
    ((b"abc", b"zz", 1, 3, 1), NONE),
    # a pattern byte 0 equals nothing, not even a text byte 0: "a" against "a\0" costs the insertion
    ((b"a\x00a", b"a\x00", 0, 3, 1), (1, 0, 1)),
    ((b"a\x00a", b"a\x00", 0, 3, 0), NONE),
    # the empty pattern
    ((b"abc", b"", 1, 3, 0), (0, 1, 1)),
    ((b"abc", b"", 3, 3, 4), (0, 3, 3)),
    # lo = hi: only the empty span
    ((b"abc", b"b", 1, 1, 1), (1, 1, 1)),
    ((b"abc", b"b", 1, 1, 0), NONE),
    # lo > hi, hi > n
    ((b"abc", b"b", 2, 1, 1), NONE),
    ((b"abc", b"b", 0, 4, 1), NONE),
    ((b"abc", b"", 0, 4, 1), NONE),
    # the window hides the first occurrence; and the second one too: then "b" at [1, 2) is one deletion away
    ((b"abcab", b"ab", 1, 5, 0), (0, 3, 5)),
    ((b"abcab", b"ab", 1, 4, 1), (1, 1, 2)),
    # every end from 2 on holds an exact match: the first; every start would do at cost 1 for a longer span: the exact one
    ((b"aaaaaa", b"aa", 0, 6, 1), (0, 0, 2)),
    ((b"aaaaaa", b"aa", 3, 6, 0), (0, 3, 5)),
]


@pytest.mark.parametrize("args,want", LITERALS)
def test_literals(args, want):
    text, pat, lo, hi, k = args
    assert W.window_one(np.frombuffer(text, dtype=np.uint8), pat, lo, hi, k) == want
    assert W.brute(text, pat, lo, hi, k) == want


def test_arrays():
    text = np.frombuffer(b"abcab", dtype=np.uint8)
    dist, start, end = W.window(text, [b"ab", b""], [0, 1, 2, 0], [1, 2, 0, 3], [5, 2, 5, 2], 0)
    assert dist.dtype == np.uint8 and start.dtype == np.uint64 and end.dtype == np.uint64
    assert dist.tolist() == [0, 0, 0xFF, 0xFF]
    assert start.tolist() == [3, 2, 2**64 - 1, 2**64 - 1] and end.tolist() == [5, 2, 2**64 - 1, 2**64 - 1]


@pytest.mark.parametrize("name", ["ab", "dna"])
def test_agrees_with_extend_reference(name):
    """on the window [delta - k, delta + m + k), clipped to the text, both references define the same triple"""
    import approx_reference as R
    text = R.make_text(name)
    tb, n = text.tobytes(), len(text)
    rng = np.random.default_rng(5)
    alphabet = sorted(set(tb))
    found = 0
    for q in range(120):
        m, k = int(rng.choice([0, 1, 5, 16, 40])), int(rng.choice([0, 1, 3, 8]))
        i = int(rng.integers(0, n - m + 1))
        pat = E.planted(rng, tb[i:i + m], int(rng.integers(0, k + 2)), alphabet, at_ends=q % 2 == 0)
        delta = int(rng.choice([i, i - k, i + k + 1, -3, n - len(pat) // 2, 2995, n + 4]))
        lo, hi = E.window(n, len(pat), delta, k)
        want = E.extend_one(text, pat, delta, k)
        assert W.window_one(text, pat, lo, hi, k) == want, (name, pat, delta, k)
        found += want != NONE
    assert 30 < found < 120
