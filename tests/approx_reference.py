"""Brute-force reference for the k-mismatch search (include/pfpgpu.h, "Approximate search"), and the texts and patterns its tests
share.  The pattern slides over the text, numpy counts the mismatches of every window, the windows with at most k are grouped by
their bytes, and each distinct string's row range comes from a binary search over the oracle's suffix array; every range must
hold exactly the grouped positions.  Nothing here comes from the feature under test."""
import functools

import numpy as np

MAX_K = 3


def full_sa(O, text):
    """SA[0..n] (SA[0] = n) from the oracle's SA[1..n]"""
    return np.concatenate([[len(text)], np.asarray(O.sacak(text), dtype=np.int64)]).astype(np.int64)


def row_range(tb, sa, s):
    """[sp, ep) of the suffixes that start with the bytes s, by binary search over the suffix array"""
    m, n1 = len(s), len(sa)

    def bound(strict):
        lo, hi = 0, n1
        while lo < hi:
            mid = (lo + hi) // 2
            x = tb[sa[mid]:sa[mid] + m]
            if x < s or (strict and x == s):
                lo = mid + 1
            else:
                hi = mid
        return lo
    return bound(False), bound(True)


def hits_upto(text, sa, pat, kmax):
    """every hit of pat with at most kmax mismatches as (sp, ep, first, d, positions), by increasing sp"""
    t = np.asarray(text, dtype=np.uint8)
    tb = t.tobytes()
    n, m = len(t), len(pat)
    if m == 0:
        return [(0, n + 1, n, 0, np.asarray(sa, dtype=np.int64))]
    if m > n:
        return []
    p = np.frombuffer(pat, dtype=np.uint8)
    win = np.lib.stride_tricks.sliding_window_view(t, m)
    mis = np.count_nonzero(win != p[None, :], axis=1)          # (a byte 0 or an absent byte of the pattern differs everywhere)
    where = np.flatnonzero(mis <= kmax)
    if not len(where):
        return []
    strings, inv = np.unique(win[where], axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(inv, kind="stable")
    cuts = np.searchsorted(inv[order], np.arange(len(strings) + 1))
    out = []
    for g in range(len(strings)):
        pos = where[order[cuts[g]:cuts[g + 1]]]
        sp, ep = row_range(tb, sa, strings[g].tobytes())
        assert ep - sp == len(pos) and np.array_equal(np.sort(sa[sp:ep]), pos), (pat[:40], g)
        d = int(mis[pos[0]])
        assert np.all(mis[pos] == d)
        out.append((sp, ep, int(sa[sp]), d, np.asarray(sa[sp:ep], dtype=np.int64)))
    out.sort(key=lambda h: h[0])
    for a, b in zip(out, out[1:]):
        assert a[1] <= b[0]                                    # disjoint ranges
    return out


class Reference:
    """the hits of patterns over one text; a pattern is searched once, with the largest budget, and filtered for the smaller"""

    def __init__(self, O, text, kmax=MAX_K):
        self.text = np.asarray(text, dtype=np.uint8)
        self.sa = full_sa(O, self.text)
        self.kmax = kmax
        self._memo = {}

    def hits(self, pat, k):
        assert 0 <= k <= self.kmax
        pat = bytes(pat)
        if pat not in self._memo:
            self._memo[pat] = hits_upto(self.text, self.sa, pat, self.kmax)
        return [h for h in self._memo[pat] if h[3] <= k]

    def arrays(self, pats, k):
        """(hit_off, sp, ep, dist, first) as FmIndex.approx(pats, k, toehold=True) returns them"""
        per = [self.hits(p, k) for p in pats]
        off = np.zeros(len(pats) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(h) for h in per])
        flat = [h for hs in per for h in hs]
        col = lambda i, dt: np.array([h[i] for h in flat], dtype=dt)
        return off, col(0, np.uint64), col(1, np.uint64), col(3, np.uint8), col(2, np.uint64)

    def located(self, pats, k, max_occ=0):
        """(off, pos, dist) as FmIndex.approx_locate(pats, k, max_occ) returns them"""
        off, pos, dist = [0], [], []
        for p in pats:
            rows = [(x, h[3]) for h in self.hits(p, k) for x in h[4]]
            if max_occ:
                rows = rows[:max_occ]
            pos += [x for x, _ in rows]
            dist += [d for _, d in rows]
            off.append(len(pos))
        return np.array(off, dtype=np.uint64), np.array(pos, dtype=np.uint64), np.array(dist, dtype=np.uint8)


TEXTS = ("dna", "copies", "bytes", "GATTACA", "ab")
KMAX = {"dna": 3, "copies": 3, "bytes": 2, "GATTACA": 3, "ab": 3}        # sigma = 253 fans out widely: k <= 2


def make_text(name):
    rng = np.random.default_rng(20)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    if name == "dna":                       # every 7-mer occurs: the walk branches fully near the pattern's right end
        return rng.choice(acgt, 20_000)
    if name == "copies":                    # real 1- and 2-mismatch hits with several positions per hit
        base = rng.choice(acgt, 4000)
        parts = []
        for _ in range(5):
            c = base.copy()
            at = np.flatnonzero(rng.random(len(c)) < 0.01)
            c[at] = acgt[(np.searchsorted(acgt, c[at]) + rng.integers(1, 4, len(at))) % 4]
            parts.append(c)
        return np.concatenate(parts)
    if name == "bytes":                     # sigma = 253: wide fan-out, tiny ranges
        return np.concatenate([np.arange(3, 256, dtype=np.uint8), rng.integers(3, 256, 4000, dtype=np.uint8)])
    if name == "GATTACA":                   # m <= k, m = n and m > n all occur
        return np.frombuffer(b"GATTACA", dtype=np.uint8).copy()
    if name == "ab":                        # long single runs, hits that differ only around the b
        return np.frombuffer(b"a" * 3000 + b"b" + b"a" * 2000, dtype=np.uint8).copy()
    raise KeyError(name)


LENGTHS = (1, 2, 3, 7, 16, 17, 20, 40, 64)


def patterns_for(text, seed=5, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    tb = bytes(np.asarray(text, dtype=np.uint8))
    n = len(tb)
    alphabet = sorted(set(tb))
    absent = bytes([min(c for c in range(1, 256) if c not in alphabet)])
    pats = [b"", b"\x00", b"A\x00C", absent, tb[:3] + absent + tb[4:9], tb, tb + tb[:1]]

    def substituted(s, places):
        s = bytearray(s)
        for j in places:
            others = [c for c in alphabet if c != s[j]]
            s[j] = others[int(rng.integers(0, len(others)))] if others else s[j]
        return bytes(s)
    for m in lengths:
        if m > n:
            continue
        subs = [tb[i:i + m] for i in (int(rng.integers(0, n - m + 1)) for _ in range(2))]
        for s in subs:
            pats.append(s)
            pats.append(substituted(s, rng.choice(m, 1, replace=False)))
            pats.append(substituted(s, rng.choice(m, min(2, m), replace=False)))
        pats.append(substituted(subs[0], [0]))
        pats.append(substituted(subs[1], [m - 1]))
    return pats


@functools.lru_cache(maxsize=None)
def case(name):
    """(text, patterns) of one of TEXTS"""
    text = make_text(name)
    return text, patterns_for(text)


def searched(name, pats, k):
    """the patterns of a text that are searched with budget k: all of them, but for `ab` with k >= 1 not the whole text and the
    whole text plus one byte.  A pattern's walk is serial, and there every a^j b (j < 2000) opens a branch that walks a one-row
    range for thousands of steps before it dies: 2.0 M steps at k = 1 and 6 M at k >= 2 per walk of that one pattern (counted
    with a CPU model of the walk), against at most 43 000 for any other pattern here.  m = n and m > n with k >= 1 stay covered
    by the other four texts, and `ab` by its patterns of up to 64 bytes."""
    if name == "ab" and k >= 1:
        return [p for p in pats if len(p) < 5001]
    return list(pats)


_refs = {}


def reference(O, name):
    """the Reference of a text, computed once and shared by the tests that need it"""
    if name not in _refs:
        _refs[name] = Reference(O, case(name)[0], KMAX[name])
    return _refs[name]
