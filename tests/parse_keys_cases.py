"""Inputs for the tests of the integer sorter's first-round keys (two-symbol keys of a string without equal neighbours) and of the
parse's pivot round with batched loads, with a plain numpy model of the first pivot round that says which path an input reaches.
test_parse_keys_cases.py checks, without a GPU, that every input has the property its name claims; test_parse_first_keys.py
runs them on the GPU.  tests/README_parse_keys.md has the table of which case reaches which path."""
import numpy as np

CAP = 1024          # kIntPivCap: symbols compared per member and pivot round
BATCH = 4           # kIntPivBatch: 16-byte steps a member loads together (4 symbols each)
PIVOT_MIN = 64      # PFP_PARSE_PIVOT_MIN of the pivot cases
RUN_BITS_MIN = 6    # the run layout (and with it the two-symbol layout) is taken while 64 - 2 sb >= 6


def bits_for(v):
    return max(1, int(v).bit_length())


# ------------------------------------------------------------------------------------------ first round
def run_free(n, top, seed, pair_at=None):
    """n symbols ending in the unique 0: a walk over 1..top whose steps are never 0, so that no two neighbours are equal - but for
    pair_at, where s[pair_at] == s[pair_at + 1] is the only equal pair.  `top` itself occurs (it sets the symbol width)."""
    assert n >= 2 and top >= 3
    rng = np.random.default_rng(seed)
    m = n - 1
    steps = rng.integers(1, top, size=m, dtype=np.int64)          # 1 .. top - 1: never 0 mod top
    if pair_at is not None:
        assert 0 <= pair_at and pair_at + 1 < m
        steps[pair_at + 1] = 0
    s = (np.cumsum(steps) % top) + 1
    # move the walk so that `top` occurs: a rotation of the alphabet keeps neighbours unequal
    s = (s - 1 + (top - int(s[0]))) % top + 1
    return np.ascontiguousarray(np.concatenate([s, [0]]).astype(np.uint32))


SMALL_SIZES = (2, 3, 64, 65, 257, 70_001)
MERGE_SWITCH = 1 << 20            # the library sorts up to this many elements by merging
TUNED_MIN = 6 << 20               # kTunedPairsMin: from here on the flagship's sort configuration


def first_round_cases():
    """name -> (builder, layout the trace line must name, pair position or None)"""
    cases = {}
    for n in SMALL_SIZES:
        cases["free_%d" % n] = (lambda n=n: run_free(n, 50, n), "two symbols", None)
        m = n - 1          # symbols before the final 0
        seen = set()
        for where, at in (("first", 0), ("middle", m // 2 - 1), ("last", m - 2)):
            if 0 <= at <= m - 2 and at not in seen:          # (2 symbols: no room for a pair; 3: the three places are one)
                seen.add(at)
                cases["pair_%d_%s" % (n, where)] = (lambda n=n, at=at: run_free(n, 50, n, at), "run", at)
    cases["top_2^29-1"] = (lambda: run_free(3001, (1 << 29) - 1, 5), "two symbols", None)
    cases["top_2^29"] = (lambda: run_free(3001, 1 << 29, 6), "plain", None)
    cases["below_merge_switch"] = (lambda: run_free(MERGE_SWITCH - 3, 3000, 7), "two symbols", None)
    cases["above_merge_switch"] = (lambda: run_free(MERGE_SWITCH + 5, 3000, 8), "two symbols", None)
    cases["tuned_sort"] = (lambda: run_free(TUNED_MIN + 1000, 3000, 9), "two symbols", None)
    return cases


FIRST_ROUND = first_round_cases()


def equal_pairs(s):
    """positions i with s[i] == s[i + 1]"""
    s = np.asarray(s)
    return np.flatnonzero(s[:-1] == s[1:])


def trace_line(n, top, layout):
    """the line PFP_TRACE_ROUNDS makes the sorter write for the first-round keys of n symbols up to top"""
    sb = bits_for(top)
    bits = 2 * sb if layout == "two symbols" else 64
    return "[pfp] integer first-round keys N=%d sb=%d: %s layout, sorted bits [0, %d)" % (n, sb, layout, bits)


# ------------------------------------------------------------------------------------------ pivot round
def copies_parse(base, copies, edits, seed=1):
    """(parse, last, occ): symbol 1 once, then `copies` copies of `base` (symbols >= 2), with edits {(copy, offset): symbol};
    symbol None = a symbol of that place's own.  occ counts the symbols 1..d."""
    base = np.asarray(base, dtype=np.uint32)
    S = len(base)
    body = np.tile(base, copies)
    nxt = int(base.max()) + 1
    for (c, t), sym in sorted(edits.items()):
        if sym is None:
            sym, nxt = nxt, nxt + 1
        body[c * S + t] = sym
    parse = np.concatenate([np.ones(1, np.uint32), body]).astype(np.uint32)
    occ = np.bincount(parse)[1:].astype(np.uint32)
    assert occ.min() >= 1, "a symbol of the alphabet does not occur"
    last = np.random.default_rng(seed).integers(65, 69, size=len(parse)).astype(np.uint8)
    return parse, last, occ


def perm_base(S, seed):
    return np.random.default_rng(seed).permutation(S).astype(np.uint32) + 2


def pivot_cases():
    cases = {}
    # 40 copies x 200 symbols, three private variants a copy (the generator of sorter_cases.py's parse_tiny_forced, restated)
    rng = np.random.default_rng(23)
    ed = {(c, int(t)): None for c in range(40) for t in rng.choice(np.arange(1, 199), size=3, replace=False)}
    cases["private"] = lambda ed=ed: copies_parse(perm_base(200, 23), 40, ed)
    # two forms of one place, each in half of the copies, both symbols common elsewhere: members differ where nothing is rare
    def shared():
        base = perm_base(120, 31)
        b, c = int(base[10]), int(base[20])
        base = np.concatenate([base[:70], [b], base[70:]]).astype(np.uint32)      # b twice in every copy; c too, in half of them
        ed = {(k, 70): c for k in range(0, 30, 2)}
        ed.update({(k, 100 + (k % 7)): None for k in range(30)})
        return copies_parse(base, 30, ed)
    cases["shared_variant"] = shared
    # one private variant a copy, far from the start: most members equal the pivot for more than one batch of 4 BATCH symbols
    cases["long_equal_batch"] = lambda: copies_parse(perm_base(300, 41), 6, {(k, 250 + 5 * k): None for k in range(6)})
    # ... and for more than CAP symbols: the class "equal to the pivot for cap"
    cases["long_equal_cap"] = lambda: copies_parse(perm_base(1500, 43), 3, {(k, 1450 + 7 * k): None for k in range(3)})
    # variants two symbols before the end of a copy, the last copy without one: the compare's last step crosses the end of the string
    cases["tail"] = lambda: copies_parse(perm_base(90, 47), 5, {(k, 88): None for k in range(4)})
    # list lengths around a wave and a workgroup: 3 copies of S distinct symbols leave 3 S - 1 members in groups of three (and
    # one of two), every private variant takes two away; no group size divides 64 or 256
    cases["members_63"] = lambda: copies_parse(perm_base(22, 51), 3, {(1, 9): None})
    cases["members_64"] = lambda: copies_parse(perm_base(23, 52), 3, {(1, 9): None, (2, 15): None})
    cases["members_65"] = lambda: copies_parse(perm_base(22, 53), 3, {})
    cases["members_257"] = lambda: copies_parse(perm_base(86, 54), 3, {})
    # one copy with a variant at every fourth place next to three copies without any: distances 1 and more than 4 BATCH in one wave
    cases["mixed_wave"] = lambda: copies_parse(perm_base(60, 57), 4, {(1, t): None for t in range(3, 58, 4)})
    return cases


PIVOT = pivot_cases()
MEMBERS = {"members_63": 63, "members_64": 64, "members_65": 65, "members_257": 257}


def rare_dist(s, occ):
    """dist[i] of the sorter: how far the next rare symbol is from i (0 at a rare symbol).  s ends in its 0; rare = 0, a symbol
    above the alphabet, or one with fewer occurrences than max(2, N // d)."""
    s = np.asarray(s, dtype=np.int64)
    N, d = len(s), len(occ)
    below = max(2, N // d)
    occ = np.asarray(occ, dtype=np.int64)
    rare = (s == 0) | (s > d) | (occ[np.clip(s - 1, 0, d - 1)] < below)
    nxt = np.where(rare, np.arange(N), N)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]
    assert nxt[-1] == N - 1
    return nxt - np.arange(N)


def first_pivot_round(parse, occ):
    """The model of the first pivot round (h = 2).  Members: the positions whose pair of symbols another position shares, in the
    order of the first sort (pair, then position).  Per member: its group's pivot (largest dist[i + 2], ties the first), dv =
    its own dist[i + 2], lcp = symbols from i + 2 that equal the pivot's (capped at CAP; -1 for the pivot itself).
    -> dict(pos, grp, piv, dv, lcp, N)"""
    s = np.concatenate([np.asarray(parse, dtype=np.int64), [0]])
    N = len(s)
    dist = rare_dist(s, occ)
    pair = s * (int(s.max()) + 1) + np.concatenate([s[1:], [0]])
    order = np.lexsort((np.arange(N), pair))
    ps = pair[order]
    head = np.concatenate([[True], ps[1:] != ps[:-1]])
    gid = np.cumsum(head) - 1
    size = np.bincount(gid)
    keep = size[gid] >= 2
    pos, grp = order[keep], gid[keep]
    h = 2
    dv = np.where(pos + h < N, dist[np.minimum(pos + h, N - 1)], 0)
    piv = np.empty_like(pos)
    for g in np.unique(grp):
        at = np.flatnonzero(grp == g)
        piv[at] = pos[at[int(np.argmax(dv[at]))]]          # (argmax: the first of equal maxima)
    lcp = np.empty(len(pos), dtype=np.int64)
    for a, (i, p) in enumerate(zip(pos, piv)):
        if i == p:
            lcp[a] = -1
            continue
        x, y = s[i + h:i + h + CAP], s[p + h:p + h + CAP]
        n = min(len(x), len(y))
        ne = np.flatnonzero(x[:n] != y[:n])
        assert len(ne) or n == CAP          # (the final 0 is unique: two suffixes differ before the shorter one ends)
        lcp[a] = int(ne[0]) if len(ne) else CAP
    return dict(pos=pos, grp=grp, piv=piv, dv=dv, lcp=lcp, N=N)
