"""The CPU reference of the LCP / thresholds tests (lcp_reference.py) against brute force on tiny texts, without a GPU: the LCP
array against direct comparison, the PLCP identity, thresholds against the definition, and the two-pass matching statistics of
the header (include/pfpgpu.h, "The LCP array and thresholds") against ms_reference.brute_lengths."""
import numpy as np

import lcp_reference as L
import ms_reference as R
from test_ms_reference import tiny_cases


def brute_lcp(tb, sa):
    out = [0]
    for j in range(1, len(sa)):
        out.append(R._lcp(tb[sa[j - 1]:], tb[sa[j]:]))
    return np.array(out, dtype=np.int64)


def test_lcp_against_brute_force_and_plcp_identity():
    for tb, _ in tiny_cases(400, 4):
        sa = R.naive_sa(tb)
        lcp = L.kasai_lcp(tb, sa)
        assert np.array_equal(lcp, brute_lcp(tb, sa)), tb
        assert lcp[0] == 0 and lcp[1] == 0
        L.plcp(tb, sa, lcp)                          # asserts LCP[j] = PLCP[SA[j]] on every row


def test_run_starts_are_the_irreducible_rows():
    """at a run start LCP[j] is the LCE of two samples: SA[j] (.ssa) and SA[j-1] (.esa of the run before)"""
    for tb, _ in tiny_cases(200, 5):
        sa = R.naive_sa(tb)
        lcp = L.kasai_lcp(tb, sa)
        starts, ends, _ = L.runs_of(L.bwt_of(tb, sa))
        for k in range(1, len(starts)):
            assert ends[k - 1] + 1 == starts[k]
            assert lcp[starts[k]] == R._lcp(tb[sa[starts[k]]:], tb[sa[ends[k - 1]]:])


def test_thresholds_by_the_definition():
    for tb, _ in tiny_cases(300, 6):
        sa = R.naive_sa(tb)
        lcp = L.kasai_lcp(tb, sa)
        bwt = L.bwt_of(tb, sa)
        thr = L.thresholds(bwt, lcp)
        starts, ends, byte = L.runs_of(bwt)
        for k in range(len(starts)):
            prev = [p for p in range(k) if byte[p] == byte[k]]
            if not prev:
                assert thr[k] == 0
                continue
            lo, hi = ends[prev[-1]] + 1, starts[k]
            seg = lcp[lo:hi + 1]
            assert lo <= thr[k] <= hi and lcp[thr[k]] == seg.min()
            assert np.all(seg[:thr[k] - lo] > seg.min())         # the smallest row with the minimum


def test_smallest_row_wins_a_tie():
    """T = abaab, rows and values written out by hand: its last run has a prev, and LCP values put in by hand make the ties"""
    tb = b"abaab"
    sa = R.naive_sa(tb)
    assert list(sa) == [5, 2, 3, 0, 4, 1]           # "", aab, ab, abaab, b, baab
    bwt = L.bwt_of(tb, sa)
    assert bytes(bwt) == b"bba\0aa"                 # runs: b (rows 0-1), a (row 2), 0 (row 3), a (rows 4-5)
    lcp = L.kasai_lcp(tb, sa)
    assert list(lcp) == [0, 0, 1, 2, 0, 1]
    thr = L.thresholds(bwt, lcp)
    # run 3 (a, starts at row 4) has prev = run 1 (a, ends at row 2): range rows 3..4, LCP 2, 0 -> row 4
    assert list(thr) == [0, 0, 0, 4]
    # a tie made by hand: LCP values 1 1 over the range -> the smaller row
    fake = np.array([0, 0, 1, 1, 1, 1])
    assert list(L.thresholds(bwt, fake)) == [0, 0, 0, 3]
    fake = np.array([0, 0, 1, 2, 2, 1])
    assert list(L.thresholds(bwt, fake)) == [0, 0, 0, 3]
    fake = np.array([0, 0, 1, 2, 1, 1])
    assert list(L.thresholds(bwt, fake)) == [0, 0, 0, 4]


def test_two_passes_give_the_lengths():
    for tb, pat in tiny_cases(400, 3):
        sa = R.naive_sa(tb)
        ln, ps, matched = L.ms_thresholds(tb, sa, pat)
        assert ln == list(R.brute_lengths(tb, pat)), (tb, pat)
        for i, (l, p) in enumerate(zip(ln, ps)):
            assert (p == L.NONE) if l == 0 else (p + l <= len(tb) and tb[p:p + l] == pat[i:i + l])
        assert matched <= len(pat), (tb, pat, matched)


def test_gattaca_literals():
    from test_ms_reference import GATTACA
    tb = b"GATTACA"
    sa = R.naive_sa(tb)
    for pat, (ln, _) in GATTACA.items():
        got, ps, matched = L.ms_thresholds(tb, sa, pat)
        assert got == ln and matched <= len(pat)
