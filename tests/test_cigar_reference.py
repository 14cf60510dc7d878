"""The edit-script reference (cigar_reference.py) against a brute force over all scripts, and on the alignments that the extension
reference (extend_reference.py) finds.  include/pfpgpu.h, "Edit scripts": the script read backwards by rules 1-4 is the optimal
script whose reversed operation string is the smallest under '=' < X < I < D, it has at most 2d + 1 runs, and for a result (d, s, e)
of an extension its cost is d and it neither begins nor ends with D."""
import numpy as np

import cigar_reference as G
import extend_reference as E

RANK = {G.OP_EQ: 0, G.OP_X: 1, G.OP_I: 2, G.OP_D: 3}


def all_scripts(p, t):
    """every operation string that turns p into t: '=' where the bytes are equal and not 0, X where they differ"""
    out = []

    def go(i, j, ops):
        if i == len(p) and j == len(t):
            out.append(tuple(ops))
            return
        if i < len(p) and j < len(t):
            go(i + 1, j + 1, ops + [G.OP_EQ if p[i] == t[j] and p[i] != 0 else G.OP_X])
        if i < len(p):
            go(i + 1, j, ops + [G.OP_I])
        if j < len(t):
            go(i, j + 1, ops + [G.OP_D])
    go(0, 0, [])
    return out


def test_against_all_scripts():
    rng = np.random.default_rng(5)
    for _ in range(400):
        m, L = int(rng.integers(0, 5)), int(rng.integers(0, 5))
        p, t = rng.integers(0, 3, m).astype(np.uint8), rng.integers(0, 3, L).astype(np.uint8)
        scripts = all_scripts(p.tolist(), t.tolist())
        cost = lambda ops: sum(op != G.OP_EQ for op in ops)
        best = min(scripts, key=lambda ops: (cost(ops), [RANK[op] for op in reversed(ops)]))
        D = G.matrix(p, t)
        got = tuple(G.traceback(p, t, D))
        assert int(D[m, L]) == cost(best) and got == best, (p, t, got, best)
        runs = G.rle(got)
        assert len(runs) <= 2 * cost(best) + 1
        G.validate(p.tobytes(), t.tobytes(), runs, cost(best))
        text = np.concatenate([np.full(3, 1, dtype=np.uint8), t, np.full(2, 2, dtype=np.uint8)])
        assert G.script(text, p.tobytes(), 3, 3 + L, 8) == (cost(best), runs)


def test_the_run_bound_is_attained():
    d, runs = G.script(np.frombuffer(b"abababa", dtype=np.uint8), b"axaxaxa", 0, 7, 3)
    assert d == 3 and len(runs) == 2 * d + 1 and G.cigar_string(runs) == "1=1X1=1X1=1X1="


def test_no_script_and_format():
    text = np.frombuffer(b"GATTACA", dtype=np.uint8)
    assert G.script(text, b"GATT", 0, 4, 0) == (0, [4 << 4 | G.OP_EQ])
    assert G.script(text, b"GCTT", 0, 4, 0) == (G.NONE, [])        # cost k + 1
    assert G.script(text, b"GATT", 0, 6, 1) == (G.NONE, [])        # |L - m| = k + 1
    assert G.script(text, b"GATT", 5, 4, 2) == (G.NONE, [])        # s > e
    assert G.script(text, b"ACA", 4, 8, 2) == (G.NONE, [])         # e = n + 1
    assert G.script(text, b"", 3, 3, 0) == (0, [])
    assert G.script(text, b"", 3, 5, 2) == (2, [2 << 4 | G.OP_D])
    assert G.script(text, b"G\x00TT", 0, 4, 1) == (1, [1 << 4 | G.OP_EQ, 1 << 4 | G.OP_X, 2 << 4 | G.OP_EQ])
    assert G.cigar_string([]) == "*" and G.cigar_string([57 << 4 | 7, 1 << 4 | 8, 20 << 4 | 7, 1 << 4 | 1, 72 << 4 | 7]) == "57=1X20=1I72="
    dist, off, cig = G.cigar(text, [b"GATT", b"ACA"], [0, 2, 1], [0, 0, 4], [4, 4, 7], 1)
    assert dist.tolist() == [0, G.NONE, 0] and off.tolist() == [0, 1, 1, 2] and cig.tolist() == [4 << 4 | 7, 3 << 4 | 7]
    assert (dist.dtype, off.dtype, cig.dtype) == (np.uint8, np.uint64, np.uint32)


def test_on_extensions():
    """what extend_one finds: the script costs d, passes the validator, and has no D at either end"""
    rng = np.random.default_rng(6)
    texts = {"ab": np.frombuffer(b"a" * 60 + b"b" + b"a" * 40, dtype=np.uint8),
             "dna": rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 400)}
    seen = 0
    for name, text in texts.items():
        tb, n = text.tobytes(), len(text)
        alphabet = sorted(set(tb))
        for k in (0, 1, 3, 8):
            for m in (0, 1, 5, 16, 33, 70):
                for i in {0, n - m, int(rng.integers(0, n - m + 1)), 60 - m // 2 if name == "ab" else 7}:
                    for edits in sorted({0, min(1, k), k}):
                        pat = E.planted(rng, tb[i:i + m], edits, alphabet, at_ends=(i + edits) % 2 == 0)
                        for delta in (i, i - k, i + 1):
                            d, s, e = E.extend_one(text, pat, delta, k)
                            if d == 0xFF:
                                continue
                            dist, runs = G.script(text, pat, s, e, k)
                            assert dist == d, (name, k, pat, delta, d, dist)
                            G.validate(pat, tb[s:e], runs, d)
                            assert len(runs) <= 2 * d + 1
                            assert not runs or (runs[0] & 15 != G.OP_D and runs[-1] & 15 != G.OP_D), (name, k, pat, delta, G.cigar_string(runs))
                            seen += 1
    assert seen > 300
