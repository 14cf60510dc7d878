"""Plain numpy reference for edit scripts (include/pfpgpu.h, "Edit scripts"): the full, unbanded matrix D[i][j] = Levenshtein(P[:i],
T[s:s+j]) computed row by row as extend_reference.last_row does (the in-row dependency by minimum.accumulate(x - arange) + arange),
kept as int16; the traceback by the definition's rules 1-4; the run-length encoding; a validator that replays a script against
the two strings; and the formatter.  Nothing here calls the library."""
import numpy as np

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8           # the BAM codes
LETTER = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
NONE = 0xFF


def matrix(p, t):
    """D as an (m + 1) x (L + 1) int16 array; p, t uint8 arrays; a pattern byte 0 equals nothing"""
    m, L = len(p), len(t)
    assert m + L < 2**15
    ar = np.arange(L + 1, dtype=np.int16)
    D = np.empty((m + 1, L + 1), dtype=np.int16)
    D[0] = ar
    for i in range(1, m + 1):
        c, row = p[i - 1], D[i - 1]
        new = np.empty(L + 1, dtype=np.int16)
        new[0] = row[0] + 1
        new[1:] = np.minimum(row[:-1] + ((t != c) | (c == 0)), row[1:] + 1)
        D[i] = np.minimum.accumulate(new - ar) + ar
    return D


def traceback(p, t, D):
    """the operations of the script of (p, t), listed from the pattern's first byte"""
    i, j = len(p), len(t)
    ops = []
    while i or j:
        c = int(D[i, j])
        if i and j and p[i - 1] == t[j - 1] and p[i - 1] != 0:
            ops.append(OP_EQ)
            i, j = i - 1, j - 1
        elif i and j and int(D[i - 1, j - 1]) == c - 1:
            ops.append(OP_X)
            i, j = i - 1, j - 1
        elif i and int(D[i - 1, j]) == c - 1:
            ops.append(OP_I)
            i -= 1
        else:
            assert j and int(D[i, j - 1]) == c - 1
            ops.append(OP_D)
            j -= 1
    return ops[::-1]


def rle(ops):
    """one uint32 per run: length << 4 | op"""
    runs = []
    for op in ops:
        if runs and runs[-1] & 15 == op:
            runs[-1] += 16
        else:
            runs.append(16 | op)
    return runs


def script(text, pat, s, e, k):
    """(dist, runs) of one alignment; text a uint8 array, pat bytes"""
    n = len(text)
    p = np.frombuffer(bytes(pat), dtype=np.uint8)
    if s > e or e > n or abs((e - s) - len(p)) > k:
        return NONE, []
    t = np.asarray(text[s:e], dtype=np.uint8)
    D = matrix(p, t)
    d = int(D[len(p), len(t)])
    if d > k:
        return NONE, []
    return d, rle(traceback(p, t, D))


def cigar(text, pats, aln_pat, start, end, k, memo=None):
    """(dist, cig_off, cig) as FmIndex.cigar returns them; memo: a dict that keeps the scripts of ONE text and ONE k"""
    memo = {} if memo is None else memo
    dist, off, cig = [], [0], []
    for a, s, e in zip(aln_pat, start, end):
        a, s, e = int(a), int(s), int(e)
        if not 0 <= a < len(pats):
            d, runs = NONE, []
        else:
            key = (bytes(pats[a]), s, e)
            if key not in memo:
                memo[key] = script(text, pats[a], s, e, k)
            d, runs = memo[key]
        dist.append(d)
        cig += runs
        off.append(len(cig))
    return np.array(dist, dtype=np.uint8), np.array(off, dtype=np.uint64), np.array(cig, dtype=np.uint32)


def validate(pat, span, runs, dist):
    """replays the runs: they consume exactly pat and span, '=' only where the bytes are equal and not 0, X only where they
    differ, no empty run, no two neighbours of one operation, and dist is the number of operations other than '='"""
    p, t = bytes(pat), bytes(span)
    i = j = cost = 0
    last = None
    for r in runs:
        ln, op = int(r) >> 4, int(r) & 15
        assert ln >= 1 and op in LETTER and op != last, (ln, op, last)
        last = op
        for _ in range(ln):
            if op in (OP_EQ, OP_X):
                assert i < len(p) and j < len(t), (i, j)
                same = p[i] == t[j] and p[i] != 0
                assert same == (op == OP_EQ), (i, j, op)
                i, j = i + 1, j + 1
            elif op == OP_I:
                assert i < len(p), i
                i += 1
            else:
                assert j < len(t), j
                j += 1
            cost += op != OP_EQ
    assert (i, j) == (len(p), len(t)), (i, j, len(p), len(t))
    assert cost == dist, (cost, dist)


def cigar_string(runs):
    return "".join("%d%s" % (int(r) >> 4, LETTER[int(r) & 15]) for r in runs) or "*"
