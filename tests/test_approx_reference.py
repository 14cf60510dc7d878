"""The brute-force reference of the k-mismatch search (approx_reference.py) against an independent method: recursive backtracking
over a numpy occurrence table of the BWT.  The two share the oracle's suffix array and nothing else."""
import numpy as np
import pytest

import approx_reference as R


class Backtrack:
    def __init__(self, text, sa):
        t = np.asarray(text, dtype=np.uint8)
        n = len(t)
        self.n, self.sa = n, sa
        bwt = np.where(sa > 0, t[np.maximum(sa, 1) - 1], 0).astype(np.uint8)          # rows 0..n; the row of suffix 0 holds 0
        self.syms = np.array(sorted(set(t.tolist())), dtype=np.int64)
        # occ[s, i] = occurrences of symbol s among the first i rows; C[s] = 1 + bytes smaller than s (the 1: row 0, the empty suffix)
        self.occ = np.zeros((len(self.syms), n + 2), dtype=np.int64)
        for s, c in enumerate(self.syms):
            self.occ[s, 1:] = np.cumsum(bwt == c)
        tot = self.occ[:, n + 1]
        self.C = 1 + np.concatenate([[0], np.cumsum(tot)[:-1]])
        self.code = {int(c): s for s, c in enumerate(self.syms)}

    def hits(self, pat, k):
        out = []

        def go(t, sp, ep, d):
            if t == 0:
                out.append((sp, ep, int(self.sa[sp]), d))
                return
            nsp = self.C + self.occ[:, sp]
            nep = self.C + self.occ[:, ep]
            want = self.code.get(pat[t - 1], -1)
            for s in np.flatnonzero(nep > nsp):
                cost = 0 if s == want else 1
                if d + cost <= k:
                    go(t - 1, int(nsp[s]), int(nep[s]), d + cost)
        go(len(pat), 0, self.n + 1, 0)
        return sorted(out)


@pytest.mark.parametrize("name", R.TEXTS)
def test_reference_agrees_with_backtracking(O, name):
    text = R.make_text(name)
    ref = R.Reference(O, text, R.KMAX[name])
    bt = Backtrack(text, ref.sa)
    pats = [p for p in R.patterns_for(text, seed=9, lengths=(1, 2, 7, 20, 40)) if len(p) <= 64]
    assert any(b"\x00" in p for p in pats) and b"" in pats
    for k in range(R.KMAX[name] + 1):
        for p in pats:
            got = [h[:4] for h in ref.hits(p, k)]
            assert got == bt.hits(p, k), (name, k, p[:40])
        if k == 0:                          # exactly count: one hit, or none
            assert all(len(ref.hits(p, 0)) <= 1 for p in pats)


def test_special_cases(O):
    text = R.make_text("GATTACA")
    ref = R.Reference(O, text)
    assert ref.hits(b"", 2) == [h for h in ref.hits(b"", 0)] and ref.hits(b"", 0)[0][:4] == (0, 8, 7, 0)
    assert ref.hits(b"GATTACAG", 3) == []                                   # m > n
    assert [h[3] for h in ref.hits(b"\x00", 1)] == [1, 1, 1, 1]              # m <= k: every string of m bytes, A C G T
    assert len(ref.hits(b"NN", 2)) == len({bytes(text[i:i + 2]) for i in range(6)})
    off, pos, dist = ref.located([b"GATTACA", b"TA"], 1, max_occ=2)
    assert list(off) == [0, 1, 3] and list(pos[:1]) == [0] and list(dist[:1]) == [0]
