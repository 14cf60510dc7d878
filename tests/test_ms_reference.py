"""The CPU reference of the matching-statistics tests (ms_reference.py) against brute force, without a GPU; and the algorithm
the header states (PHONI, include/pfpgpu.h "Matching statistics"), modelled in Python, against the same brute force."""
import numpy as np

import ms_reference as R

GATTACA = {  # pattern -> (len, MEMs with min_len = 2 as (i, len)); checked by brute force below
    b"TTACAG": ([5, 4, 3, 2, 1, 1], [(0, 5)]),
    b"CATTAG": ([2, 4, 3, 2, 1, 1], [(0, 2), (1, 4)]),
    b"GATTACAGATTA": ([7, 6, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1], [(0, 7), (7, 5)]),
}


def tiny_cases(count, seed):
    rng = np.random.default_rng(seed)
    for k in range(count):
        sigma = int(rng.integers(1, 5))
        n = int(rng.integers(1, 40))
        if k % 3 == 0:          # periodic
            unit = bytes(rng.integers(97, 97 + sigma, int(rng.integers(1, 6)), dtype=np.uint8))
            tb = (unit * n)[:n]
        else:
            tb = bytes(rng.integers(97, 97 + sigma, n, dtype=np.uint8))
        m = int(rng.integers(0, 30))
        pat = bytearray(rng.integers(97, 97 + sigma + 1, m, dtype=np.uint8))     # (one byte the text may not hold)
        if m and k % 4 == 0:
            i = int(rng.integers(0, n))
            s = tb[i:i + m]
            pat[:len(s)] = s
        if m and k % 7 == 0:
            pat[int(rng.integers(0, m))] = 0
        yield tb, bytes(pat)


def test_lengths_against_brute_force():
    for tb, pat in tiny_cases(400, 1):
        sa = R.naive_sa(tb)
        assert np.array_equal(R.ms_lengths(tb, sa, pat), R.brute_lengths(tb, pat)), (tb, pat)


def test_mem_rule_is_left_maximality():
    """(i = 0 or len[i-1] <= len[i]) <=> P[i-1 .. i+len[i]) does not occur (or i = 0), and len[i-1] <= len[i] + 1 always"""
    for tb, pat in tiny_cases(400, 2):
        ln = R.brute_lengths(tb, pat)
        for L in (1, 2, 3):
            got = R.mems_from_lengths(ln, L)
            want = [(i, int(ln[i])) for i in range(len(pat))
                    if ln[i] >= L and (i == 0 or pat[i - 1] == 0 or tb.find(pat[i - 1:i + int(ln[i])]) < 0)]
            assert got == want, (tb, pat, L)
        for i in range(1, len(pat)):
            assert ln[i - 1] <= ln[i] + 1


def test_gattaca_literals():
    tb = b"GATTACA"
    sa = R.naive_sa(tb)
    for pat, (ln, mems) in GATTACA.items():
        assert list(R.brute_lengths(tb, pat)) == ln
        assert list(R.ms_lengths(tb, sa, pat)) == ln
        assert R.mems_from_lengths(ln, 2) == mems


def phoni_model(tb, sa, pat):
    """the algorithm of the header, step by step, over plain arrays -> (len, pos); asserts its invariant and that the rows it
    jumps to are a run end (predecessor) and a run start (successor)"""
    n = len(tb)
    bwt = [tb[s - 1] if s else 0 for s in sa]
    isa = {int(s): j for j, s in enumerate(sa)}
    lf = lambda j: isa[int(sa[j]) - 1]
    lce = lambda x, y: R._lcp(tb[x:], tb[y:])
    present = set(tb)
    q, pos, l = 0, n, 0
    ln, ps = [0] * len(pat), [2**64 - 1] * len(pat)
    for i in range(len(pat) - 1, -1, -1):
        c = pat[i]
        if c == 0 or c not in present:
            l = 0
            continue
        if bwt[q] == c:
            q, pos, l = lf(q), pos - 1, l + 1
        else:
            qp = max((j for j in range(q) if bwt[j] == c), default=None)
            qs = min((j for j in range(q + 1, n + 1) if bwt[j] == c), default=None)
            lp = min(l, lce(int(sa[qp]), pos)) if qp is not None else -1
            ls = min(l, lce(int(sa[qs]), pos)) if qs is not None else -1
            if qp is not None:
                assert bwt[qp + 1] != c
            if qs is not None:
                assert bwt[qs - 1] != c
            x, lx = (qp, lp) if lp >= ls else (qs, ls)
            q, pos, l = lf(x), int(sa[x]) - 1, lx + 1
        assert int(sa[q]) == pos and tb[pos:pos + l] == pat[i:i + l]
        ln[i], ps[i] = l, pos
    return ln, ps


def test_stated_algorithm_gives_the_lengths():
    for tb, pat in tiny_cases(400, 3):
        ln, ps = phoni_model(tb, R.naive_sa(tb), pat)
        assert ln == list(R.brute_lengths(tb, pat)), (tb, pat)
        for i, (l, p) in enumerate(zip(ln, ps)):
            assert (p == 2**64 - 1) if l == 0 else tb[p:p + l] == pat[i:i + l]
