"""Plain numpy reference for seed extension (include/pfpgpu.h, "Extending seeds"): a full, unbanded Sellers dynamic programme over
the window, one row per pattern byte, the in-row dependency resolved by minimum.accumulate(x - arange) + arange.  A forward pass
with a free start gives d* and the smallest end e; a second pass of the reversed pattern over the reversed T[lo..e), with a fixed
end, gives the largest start s.  Also the composite: the triples from a list of MEMs, deduplicated, ordered and capped.  Nothing
here comes from the feature under test."""
import numpy as np

NONE = (0xFF, 2**64 - 1, 2**64 - 1)


def window(n, m, delta, k):
    lo = min(max(delta - k, 0), n)
    hi = min(max(delta + m + k, 0), n)
    return lo, hi


def last_row(p, t, free_start):
    """row m of the DP of pattern bytes p against text bytes t: entry j = min over starts (free) or from start 0 (fixed) of
    Levenshtein(p, t[start:j]); a pattern byte 0 equals nothing"""
    L = len(t)
    ar = np.arange(L + 1, dtype=np.int64)
    row = np.zeros(L + 1, dtype=np.int64) if free_start else ar.copy()
    for c in p:
        sub = row[:-1] + ((t != c) | (c == 0))
        new = np.empty(L + 1, dtype=np.int64)
        new[0] = row[0] + 1
        new[1:] = np.minimum(sub, row[1:] + 1)
        row = np.minimum.accumulate(new - ar) + ar
    return row


def extend_one(text, pat, delta, k):
    """(d, s, e) of one candidate; text a uint8 array, pat bytes"""
    t = np.asarray(text, dtype=np.uint8)
    p = np.frombuffer(bytes(pat), dtype=np.uint8)
    n, m = len(t), len(p)
    lo, hi = window(n, m, int(delta), k)
    fwd = last_row(p, t[lo:hi], True)
    d = int(fwd.min())
    if d > k:
        return NONE
    e = lo + int(np.argmax(fwd == d))
    back = last_row(p[::-1], t[lo:e][::-1], False)         # entry j: Levenshtein(P, T[e-j:e))
    j = int(np.argmax(back == d))
    assert back[j] == d
    return d, e - j, e


def extend(text, pats, cand_pat, cand_diag, k):
    """(dist, start, end) as FmIndex.extend returns them"""
    res = [extend_one(text, pats[p], dg, k) if 0 <= p < len(pats) else NONE for p, dg in zip(cand_pat, cand_diag)]
    col = lambda i, dt: np.array([r[i] for r in res], dtype=dt)
    return col(0, np.uint8), col(1, np.uint64), col(2, np.uint64)


def align(text, pats, mem_off, mems, k, max_aln=0, memo=None):
    """(aln_off, start, end, dist) as FmIndex.align returns them, from the MEMs FmIndex.mems listed: rows (i, len, pos); memo: a
    dict that keeps the extensions of ONE text and ONE k between calls"""
    memo = {} if memo is None else memo
    off, start, end, dist = [0], [], [], []
    for p, pat in enumerate(pats):
        found = set()
        for i, _, pos in np.asarray(mems, dtype=np.uint64)[int(mem_off[p]):int(mem_off[p + 1])].tolist():
            key = (bytes(pat), int(pos) - int(i))
            if key not in memo:
                memo[key] = extend_one(text, pat, key[1], k)
            d, s, e = memo[key]
            if d <= k:
                found.add((d, s, e))
        rows = sorted(found)
        if max_aln:
            rows = rows[:max_aln]
        for d, s, e in rows:
            start.append(s), end.append(e), dist.append(d)
        off.append(len(start))
    return np.array(off, dtype=np.uint64), np.array(start, dtype=np.uint64), np.array(end, dtype=np.uint64), np.array(dist, dtype=np.uint8)


def planted(rng, s, edits, alphabet, at_ends):
    """s with `edits` unit edits: substitutions, insertions and deletions at random places; at_ends: the first two at the first
    and at the last byte"""
    s = bytearray(s)
    letter = lambda not_this=None: int(rng.choice([c for c in alphabet if c != not_this]))
    for t in range(edits):
        j = 0 if at_ends and t == 0 else max(len(s) - 1, 0) if at_ends and t == 1 else int(rng.integers(0, len(s) + 1))
        op = (t + int(rng.integers(0, 3))) % 3
        if j >= len(s):
            s.append(letter())
        elif op == 0:
            s[j] = letter(s[j])
        elif op == 1:
            del s[j]
        else:
            s.insert(j, letter())
    return bytes(s)
