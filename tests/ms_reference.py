"""CPU reference for matching statistics and maximal exact matches (include/pfpgpu.h, "Matching statistics"), written from
the definitions and independent of the feature: a binary search over the suffix array, numpy + Python.

For a text T of n bytes with suffix array SA[0..n] (SA[0] = n) and a pattern P of m bytes:
  len[i] = the largest l <= m - i such that P[i .. i+l) occurs in T; 0 where P[i] is byte 0.
  a MEM is (i, len[i]) with len[i] >= min_len and (i = 0 or len[i-1] <= len[i]).
The cost is m x log n x (bytes compared): patterns of up to about 1000 bytes."""
import numpy as np


def _lcp(a, b):
    m = min(len(a), len(b))
    if a[:m] == b[:m]:
        return m
    lo, hi = 0, m                                   # a[:lo] == b[:lo], a[:hi] != b[:hi]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if a[:mid] == b[:mid]:
            lo = mid
        else:
            hi = mid
    return lo


def ms_lengths(tb, sa, pat):
    """len[i] for every byte of pat; tb: the text as bytes, sa: SA[0..n] with SA[0] = n"""
    n1, m = len(sa), len(pat)
    out = np.zeros(m, dtype=np.int64)
    for i in range(m):
        if pat[i] == 0:
            continue
        z = pat.find(b"\0", i)
        s = pat[i:] if z < 0 else pat[i:z]          # (a match never holds byte 0: T does not)
        lo, hi = 0, n1                              # insertion point of s among the suffixes
        while lo < hi:
            mid = (lo + hi) // 2
            if tb[sa[mid]:sa[mid] + len(s)] < s:
                lo = mid + 1
            else:
                hi = mid
        best = 0
        for j in (lo - 1, lo):                      # the longest common prefix is with a neighbour in suffix order
            if 0 <= j < n1:
                best = max(best, _lcp(tb[sa[j]:sa[j] + len(s)], s))
        out[i] = best
    return out


def mems_from_lengths(ln, min_len):
    """[(i, len[i])] by increasing i"""
    return [(i, int(l)) for i, l in enumerate(ln) if l >= min_len and (i == 0 or ln[i - 1] <= l)]


def brute_lengths(tb, pat):
    """the same lengths by bytes.find: tiny inputs only"""
    m = len(pat)
    out = np.zeros(m, dtype=np.int64)
    for i in range(m):
        l = 0
        while i + l < m and pat[i + l] != 0 and tb.find(pat[i:i + l + 1]) >= 0:
            l += 1
        out[i] = l
    return out


def naive_sa(tb):
    """SA[0..n] of a tiny text by sorting its suffixes (SA[0] = n: the empty suffix first)"""
    n = len(tb)
    return np.array(sorted(range(n + 1), key=lambda i: tb[i:]), dtype=np.int64)
