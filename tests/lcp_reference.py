"""CPU reference for the LCP array, thresholds and matching statistics with thresholds (include/pfpgpu.h, "The LCP array and
thresholds"), written from the definitions and independent of the feature: numpy + Python over plain arrays.

For a text T of n bytes with suffix array SA[0..n] (SA[0] = n):
  LCP[0] = 0, LCP[j] = the common prefix of T[SA[j-1]:] and T[SA[j]:]                                  (Kasai et al.)
  runs k = 0..r-1 of the BWT with start row s_k, end row e_k, byte c_k; prev(k) = the largest k' < k with c_k' = c_k
  thr[k] = 0 without a prev(k), else the SMALLEST row t in (e_prev(k), s_k] with LCP[t] = min LCP(e_prev(k), s_k]
  PLCP[i] = PLCP[i0] - (i - i0) with i0 the largest run-start SA value <= i                             (asserted by plcp)."""
import numpy as np

NONE = 2**64 - 1


def bwt_of(tb, sa):
    return np.array([tb[s - 1] if s else 0 for s in sa], dtype=np.uint8)


def kasai_lcp(tb, sa):
    """LCP[0..n] from the text and SA[0..n]"""
    n = len(tb)
    sa = np.asarray(sa, dtype=np.int64)
    isa = np.empty(n + 1, dtype=np.int64)
    isa[sa] = np.arange(n + 1)
    lcp = np.zeros(n + 1, dtype=np.int64)
    h = 0
    for i in range(n):
        j = int(isa[i])                             # j >= 1: row 0 is the empty suffix
        p = int(sa[j - 1])
        while i + h < n and p + h < n and tb[i + h] == tb[p + h]:
            h += 1
        lcp[j] = h
        if h:
            h -= 1
    return lcp


def runs_of(bwt):
    """(start rows, end rows, bytes) of the runs"""
    b = np.asarray(bwt)
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    ends = np.flatnonzero(np.concatenate([b[1:] != b[:-1], [True]]))
    return starts, ends, b[starts]


def thresholds(bwt, lcp):
    """thr[k] by the definition: per run the first minimum of LCP over the rows (e_prev(k), s_k]"""
    starts, ends, byte = runs_of(bwt)
    lcp = np.asarray(lcp)
    thr = np.zeros(len(starts), dtype=np.int64)
    last = {}
    for k in range(len(starts)):
        c = int(byte[k])
        if c in last:
            lo, hi = int(ends[last[c]]) + 1, int(starts[k])       # rows lo..hi inclusive
            assert lo <= hi
            thr[k] = lo + int(np.argmin(lcp[lo:hi + 1]))          # (argmin: the first of equal minima)
        last[c] = k
    return thr


def plcp(tb, sa, lcp):
    """PLCP[0..n] by the identity over the run-start SA values; asserts LCP[j] = PLCP[SA[j]] for every row"""
    n = len(tb)
    bwt = bwt_of(tb, sa)
    starts, _, _ = runs_of(bwt)
    val = {int(sa[j]): int(lcp[j]) for j in starts}
    assert 0 in val or n == 0                       # the byte before position 0 is the 0: its row starts a run
    out = np.zeros(n + 1, dtype=np.int64)
    i0 = None
    for i in range(n + 1):
        if i in val:
            i0 = i
        assert i0 is not None
        out[i] = val[i0] - (i - i0)
    assert np.array_equal(out[np.asarray(sa, dtype=np.int64)], lcp), (tb, out, lcp)
    return out


class Model:
    """what the two passes read, over plain arrays: the BWT, its runs, the thresholds, SA and its inverse"""

    def __init__(self, tb, sa, thr=None):
        self.tb, self.n = tb, len(tb)
        self.sa = np.asarray(sa, dtype=np.int64)
        self.bwt = np.zeros(self.n + 1, dtype=np.uint8)
        t = np.frombuffer(tb, dtype=np.uint8)
        nz = self.sa > 0
        self.bwt[nz] = t[self.sa[nz] - 1]
        self.isa = np.empty(self.n + 1, dtype=np.int64)
        self.isa[self.sa] = np.arange(self.n + 1)
        self.starts, _, _ = runs_of(self.bwt)
        self.thr = thresholds(self.bwt, kasai_lcp(tb, sa)) if thr is None else np.asarray(thr).astype(np.int64)
        self.rows = {c: np.flatnonzero(self.bwt == c) for c in set(tb)}

    def ms(self, pat):
        """-> (len, pos, bytes matched by pass 2, steps of pass 1 that jumped); pos is 2^64 - 1 where len is 0"""
        tb, n, m, sa, isa, bwt = self.tb, self.n, len(pat), self.sa, self.isa, self.bwt
        q, pos, jumps = 0, n, 0
        ps = [NONE] * m
        for i in range(m - 1, -1, -1):
            c = pat[i]
            rows = self.rows.get(c) if c else None
            if rows is None:
                continue
            if bwt[q] == c:
                q, pos = int(isa[pos - 1]), pos - 1
            else:
                at = int(np.searchsorted(rows, q))          # rows[at - 1] < q < rows[at]
                qp = int(rows[at - 1]) if at > 0 else None
                qs = int(rows[at]) if at < len(rows) else None
                if qs is None:
                    x = qp
                elif qp is None:
                    x = qs
                else:
                    k = int(np.searchsorted(self.starts, qs))
                    assert self.starts[k] == qs             # q_s starts a run
                    x = qp if q < self.thr[k] else qs
                pos = int(sa[x]) - 1
                q = int(isa[pos])
                jumps += 1
            ps[i] = pos
        ln = [0] * m
        l = matched = 0
        for i in range(m):
            if ps[i] == NONE:
                l = 0
            else:
                l = max(l - 1, 0)
                while i + l < m and ps[i] + l < n and pat[i + l] == tb[ps[i] + l]:
                    l += 1
                    matched += 1
            ln[i] = l
            if l == 0:
                ps[i] = NONE
        return ln, ps, matched, jumps


def ms_thresholds(tb, sa, pat, thr=None):
    """the two passes of the header -> (len, pos, bytes matched by pass 2)"""
    return Model(tb, sa, thr).ms(pat)[:3]
