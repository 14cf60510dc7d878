"""Plain numpy restatement of stage 1a as the fused chain runs it (csrc/scan.hip): the window hash and its
trigger, the Karp-Rabin hash of every window, extra triggers, the contract of the window hash's seed and the rule that chooses
the phrase length.  Written from the comments of scan.hip, independent of the library: nothing here calls into libpfpgpu.so.

Conventions: a text is a uint8 array; hashes of "every window" come as an array of n - w + 1 values, entry j belonging to the
window that ENDS at text position j + w - 1 (the first valid phrase end is w - 1: newscan.cpp:248); cut sets are sorted uint64
arrays of end positions.  Parsing stops at the first byte <= 2 (newscan.cpp:364): every cut function works on that prefix."""
from fractions import Fraction

import numpy as np

M32 = 0xFFFFFFFF
KR_PRIME = 1999999973
FAST_K = 0x9E3779B1          # the multiplicative-hashing constant of the trigger test
# byte multipliers of the window hash, oldest byte of the window first
FAST_MUL = np.array([0xB5, 0x6B, 0xD3, 0x97, 0xE9, 0x4F, 0xC7, 0x8D, 0xF1, 0x59, 0xA3, 0x3D, 0xDF, 0x75, 0xBB, 0x67, 0xCD,
                     0x9B, 0xE5, 0x53], dtype=np.uint64)
DNA_LETTERS = b"ACGTNacgtn"
CONTEXT = 64                 # bytes of context before (and including) a sampled cut
SAMPLE_SHIFT = 16            # sampled cuts: x < fthr_nom / 16


def usable_len(text):
    """bytes parsed: up to the first byte <= 2"""
    t = np.asarray(text, dtype=np.uint8)
    bad = np.flatnonzero(t <= 2)
    return int(bad[0]) if len(bad) else len(t)


def window_hashes(text, w):
    """h(window) = sum_i c_i * m_i mod 2^32 for every window of w bytes"""
    t = np.asarray(text, dtype=np.uint8)
    if len(t) < w:
        return np.zeros(0, dtype=np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(t, w)
    h = np.zeros(len(win), dtype=np.uint64)
    for i in range(w):          # (column by column: the product win * FAST_MUL[:w] without the n x w array of 64-bit values)
        h += win[:, i].astype(np.uint64) * FAST_MUL[i]
    return h & np.uint64(M32)


def trigger_values(h, seed):
    """x = (h + seed) * K mod 2^32: a window triggers when x < threshold"""
    return ((np.asarray(h, dtype=np.uint64) + np.uint64(seed)) & np.uint64(M32)) * np.uint64(FAST_K) & np.uint64(M32)


def kr_window_hashes(text, w):
    """the reference's Karp-Rabin hash of every window: Horner over the w columns, mod 1999999973 (newscan.cpp:168-202)"""
    t = np.asarray(text, dtype=np.uint8)
    if len(t) < w:
        return np.zeros(0, dtype=np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(t, w)
    h = np.zeros(len(win), dtype=np.uint64)
    for i in range(w):
        h = (h * np.uint64(256) + win[:, i].astype(np.uint64)) % np.uint64(KR_PRIME)
    return h


def auto_density(p):
    """the dense candidate of the automatic choice: phrases of about 48 bytes"""
    return min(Fraction(8), max(Fraction(1), Fraction(p, 48)))


def thresholds(p, density_setting=0.0):
    """(fthr, fthr_nom, fauto): the threshold the first pass cuts at, the nominal one, whether the density is a candidate.
    density_setting 0 = automatic; > 0 = pinned (then there is one threshold only)"""
    def sat(x):
        return min(int(x), M32)          # floor, saturated
    nom = Fraction(1 << 32, p)
    if density_setting > 0:
        thr = sat(nom * Fraction(density_setting))
        return thr, thr, 0
    d = auto_density(p)
    return sat(nom * d), sat(nom), 1 if d > 1 else 0


def _cuts(mask, w):
    return (np.flatnonzero(mask) + (w - 1)).astype(np.uint64)


def fast_cuts(text, w, seed, thr, extras=()):
    """phrase ends of the window hash: ((h + seed) * K mod 2^32) < thr, or the seeded hash is one of `extras`"""
    t = np.asarray(text, dtype=np.uint8)
    t = t[:usable_len(t)]
    hs = (window_hashes(t, w) + np.uint64(seed)) & np.uint64(M32)
    mask = (hs * np.uint64(FAST_K) & np.uint64(M32)) < np.uint64(thr)
    if len(extras):
        mask |= np.isin(hs, np.array(list(extras), dtype=np.uint64))
    return _cuts(mask, w)


def kr_cuts(text, w, p, extras=()):
    """phrase ends of the reference's trigger hash % p == 0 (plus extra Karp-Rabin hashes)"""
    t = np.asarray(text, dtype=np.uint8)
    t = t[:usable_len(t)]
    h = kr_window_hashes(t, w)
    mask = (h % np.uint64(p)) == 0
    if len(extras):
        mask |= np.isin(h, np.array(list(extras), dtype=np.uint64))
    return _cuts(mask, w)


def zero_hash_window(w):
    """w bytes, all >= 3, whose Karp-Rabin hash is 0: the big-endian digits of a multiple of 1999999973 - the only windows a
    modulus of 2^31 or more ever cuts"""
    m = 1
    while True:
        b = (m * KR_PRIME).to_bytes(w, "big")
        if min(b) >= 3:
            return np.frombuffer(b, dtype=np.uint8)
        m += 1


def seed_contract_violations(first_window, w, p, seed, fthr, fthr_nom):
    """The contract of the window hash's seed; returns the list of violated clauses (empty: the seed is right).
      1. the first window lies inside the NOMINAL threshold exactly when the reference's Karp-Rabin hash of it is 0 mod p,
         and otherwise outside the threshold the scan cuts at (so it decides like the reference at either density);
      2. for p >= 32 no run of one letter of ACGTNacgtn triggers - unless its hash is the first window's;
      3. the seed is the smallest value below 2^20 with 1 and 2.
    first_window: the text's first w bytes, or None for a text shorter than a window (clause 1 is then void)."""
    seeds = np.arange(seed + 1, dtype=np.uint64)
    ok = np.ones(seed + 1, dtype=bool)
    out = []
    h_first = None
    if first_window is not None:
        fw = np.frombuffer(bytes(first_window), dtype=np.uint8)
        assert len(fw) == w
        h_first = int(window_hashes(fw, w)[0])
        ref_fires = int(kr_window_hashes(fw, w)[0]) % p == 0
        x = trigger_values(np.uint64(h_first), seeds)
        first_ok = (x < np.uint64(fthr_nom)) if ref_fires else (x >= np.uint64(fthr))
        if not first_ok[seed]:
            out.append("first window decides unlike the reference (reference fires: %s)" % ref_fires)
        ok &= first_ok
    if p >= 32:
        for ch in DNA_LETTERS:
            hr = int(window_hashes(np.full(w, ch, dtype=np.uint8), w)[0])
            if hr == h_first:
                continue
            fires = trigger_values(np.uint64(hr), seeds) < np.uint64(fthr)
            if fires[seed]:
                out.append("a run of %r triggers" % chr(ch))
            ok &= ~fires
    if seed >= (1 << 20):
        out.append("seed not below 2^20")
    if ok[:seed].any():
        out.append("seed %d is not the smallest: %d would do" % (seed, int(np.flatnonzero(ok)[0])))
    return out


def density_rule(ns, distinct, singles, p):
    """the rule above sample_says_dense: (dense, ratios).  Every ratio >= 1 <=> dense; the ratios tell by which factor each
    inequality holds or fails:  ns >= 1024,  loci >= 64,  2 singles <= ns,  singles p >= 64 loci   (loci = distinct - singles)"""
    loci = distinct - singles
    inf = float("inf")
    ratios = dict(sample=ns / 1024, loci=loci / 64, collection=(ns / (2 * singles)) if singles else inf,
                  variants=(singles * p / (64 * loci)) if loci else inf)
    dense = ns >= 1024 and loci >= 64 and 2 * singles <= ns and singles * p >= 64 * loci
    assert dense == all(r >= 1 for r in ratios.values())
    return dense, ratios


def density_choice(text, w, p, seed, fthr_nom, dense_ends, min_end=0):
    """The choice of the phrase length from the cuts of the dense pass: sampled cuts are those with x < fthr_nom / 16 and
    end >= min_end; their contexts are the 64 bytes ending at the cut, compared AS BYTES; contexts seen once are singles.
    Returns dict(sampled, distinct, singles, dense, ratios, first_sampled)."""
    t = np.asarray(text, dtype=np.uint8)
    e = np.asarray(dense_ends, dtype=np.int64)
    h = window_hashes(t, w)
    x = trigger_values(h[e - (w - 1)], seed)
    smp = e[(x < np.uint64(fthr_nom // SAMPLE_SHIFT)) & (e >= min_end)]
    first = int(smp[0]) if len(smp) else None
    assert first is None or first >= CONTEXT - 1, "a sampled cut's context starts before the text: the reference is not defined there"
    ctx = np.lib.stride_tricks.sliding_window_view(t, CONTEXT)[smp - (CONTEXT - 1)] if len(smp) else np.zeros((0, CONTEXT), np.uint8)
    seen = {}
    for row in ctx:
        k = row.tobytes()
        seen[k] = seen.get(k, 0) + 1
    distinct = len(seen)
    singles = sum(1 for v in seen.values() if v == 1)
    dense, ratios = density_rule(len(smp), distinct, singles, p)
    return dict(sampled=len(smp), distinct=distinct, singles=singles, dense=dense, ratios=ratios, first_sampled=first)


def max_phrase_len(ends, n, w):
    """longest phrase of a parse, counted as the chain counts it (in T' = Dollar . T . Dollar^w: a phrase runs from the first
    byte of the previous trigger window to the last byte of its own; the first starts at the Dollar, the last ends with the w
    Dollars)"""
    e = np.asarray(ends, dtype=np.int64)
    last = np.concatenate([e + 1, [n + w]])
    first = np.concatenate([[0], e + 2 - w])
    return int((last - first + 1).max())
