"""Chaining anchors in plain Python: include/pfpgpu.h, "Chaining anchors", restated - the anchors by brute force on the text (no
index, no PHONI), the programme and the peel as written there, the strand merge and MAPQ.  Everything is exact integer work; the
GPU tests compare with it array by array (test_fm_chain.py), test_chain_reference.py checks it on the CPU."""
import numpy as np

from map_reference import revcomp, seq_of

H = 64                      # PFP_FM_CHAIN_PRED
NO_SEQ = 0xFFFFFFFF
NAMES = ("hit_off", "mapq", "nchains", "strand", "seq", "off", "ts", "te", "qs", "qe", "score", "n", "match")
CHAIN_NAMES = ("chain_off", "score", "n", "qs", "qe", "ts", "te", "match")
_CHAIN_TYPES = (np.uint32, np.uint32, np.uint32, np.uint32, np.uint64, np.uint64, np.uint32)
_LONG_TYPES = (np.uint8, np.uint32, np.uint64, np.uint64, np.uint64, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32)


def ms_lengths(tb, pat):
    """len[i] = the longest prefix of pat[i:] that occurs in tb, by direct comparison (bytes.find); byte 0 never matches"""
    m = len(pat)
    out = [0] * m
    l = 0
    for i in range(m):
        l = max(l - 1, 0)                               # (len[i] >= len[i-1] - 1)
        while i + l < m and pat[i + l] != 0 and tb.find(pat[i:i + l + 1]) >= 0:
            l += 1
        out[i] = l
    return out


def occurrences(tb, s, limit):
    """the starts of s in tb, at most limit + 1 of them"""
    out, at = [], tb.find(s)
    while at >= 0 and len(out) <= limit:
        out.append(at)
        at = tb.find(s, at + 1)
    return out


def rec_of(starts, n, t):
    if starts is None:
        return 0
    return seq_of(starts, t) if t < n else NO_SEQ


def anchors_of(tb, starts, pat, min_seed, max_occ):
    """-> (anchors [(i, len, t)] by (t + len, i + len), MEMs skipped, anchors dropped at a record border)"""
    n = len(tb)
    ln = ms_lengths(tb, pat)
    mems = [(i, l) for i, l in enumerate(ln) if l >= min_seed and (i == 0 or ln[i - 1] <= l)]
    out, skipped, dropped = [], 0, 0
    for i, l in mems:
        occ = occurrences(tb, pat[i:i + l], max_occ)
        if len(occ) > max_occ:
            skipped += 1
            continue
        for t in occ:
            if starts is not None and t + l > int(starts[seq_of(starts, t) + 1]):
                dropped += 1
                continue
            out.append((i, l, t))
    out.sort(key=lambda a: (a[2] + a[1], a[0] + a[1]))
    return out, skipped, dropped


def anchor_arrays(per_pattern):
    """[(anchors, skipped, dropped)] per pattern -> (anc_off, anc, skipped) as FmIndex.anchors returns them"""
    off = np.zeros(len(per_pattern) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(a) for a, _, _ in per_pattern], dtype=np.uint64)
    rows = [a for anc, _, _ in per_pattern for a in anc]
    return off, np.array(rows, dtype=np.uint64).reshape(-1, 3), np.array([s for _, s, _ in per_pattern], dtype=np.uint32)


def sorted_strictly(anc):
    keys = [(t + l, i + l) for i, l, t in anc]
    return all(a < b for a, b in zip(keys, keys[1:]))


def programme(anc, starts, n, G, B):
    """-> (f, parent): parent[x] = None or the index of x's parent"""
    A = len(anc)
    qe = [i + l for i, l, _ in anc]
    te = [t + l for _, l, t in anc]
    rec = [rec_of(starts, n, t) for _, _, t in anc]
    f, parent = [0] * A, [None] * A
    for x in range(A):
        best, arg = None, None
        for j in range(max(0, x - H), x):
            dq, dt = qe[x] - qe[j], te[x] - te[j]
            if rec[j] != rec[x] or dq < 1 or dt < 1 or dq > G or dt > G or abs(dt - dq) > B:
                continue
            v = f[j] + min(dq, dt, anc[x][1]) - ((abs(dt - dq) + 3) >> 2)
            if best is None or v >= best:               # (among equal values the largest j)
                best, arg = v, j
        f[x] = anc[x][1]
        if best is not None and best > anc[x][1]:
            f[x], parent[x] = best, arg
    return f, parent


def peel(anc, f, parent, S):
    """-> (kept, dropped, stopped): chains as dicts with their fields and `anchors` (indices, increasing); stopped = walks that
    ended at a visited anchor"""
    A = len(anc)
    visited = [False] * A
    kept, dropped, stopped = [], [], 0
    for x in sorted(range(A), key=lambda a: (-f[a], a)):
        if visited[x]:
            continue
        walk, y = [], x
        while y is not None and not visited[y]:
            visited[y] = True
            walk.append(y)
            y = parent[y]
        stopped += y is not None
        walk.reverse()
        match = anc[walk[0]][1]
        for a, b in zip(walk, walk[1:]):
            dq = anc[b][0] + anc[b][1] - anc[a][0] - anc[a][1]
            dt = anc[b][2] + anc[b][1] - anc[a][2] - anc[a][1]
            match += min(dq, dt, anc[b][1])
        ch = dict(score=f[x] - (f[y] if y is not None else 0), n=len(walk), qs=min(anc[a][0] for a in walk), qe=anc[x][0] + anc[x][1],
                  ts=min(anc[a][2] for a in walk), te=anc[x][2] + anc[x][1], match=match, anchors=walk)
        (kept if ch["score"] >= S else dropped).append(ch)
    return kept, dropped, stopped


def chains_of(anc, starts, n, G, B, S, max_chains=0):
    """the chains of one pattern in the order of output, as dicts"""
    f, parent = programme(anc, starts, n, G, B)
    kept = sorted(peel(anc, f, parent, S)[0], key=lambda c: (-c["score"], c["te"], c["qe"]))
    return kept[:max_chains] if max_chains else kept


def chain_arrays(per_pattern):
    """[chains] per pattern -> the arrays FmIndex.chain returns (CHAIN_NAMES)"""
    off = np.zeros(len(per_pattern) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(c) for c in per_pattern], dtype=np.uint64)
    flat = [c for cs in per_pattern for c in cs]
    return (off,) + tuple(np.array([c[k] for c in flat], dtype=dt) for k, dt in zip(CHAIN_NAMES[1:], _CHAIN_TYPES))


def mapq_of(scores):
    if not scores:
        return 0
    if len(scores) == 1:
        return 60
    return min(60, 60 * (scores[0] - scores[1]) // scores[0])


def read_chains(tb, starts, read, min_seed, max_occ, G, B, S):
    """the chains of one read, both strands, in the order of output: [(strand, chain)]; and its layer-1 results per strand"""
    n = len(tb)
    both, layer1 = [], []
    for strand, pat in enumerate((bytes(read), revcomp(read))):
        res = anchors_of(tb, starts, pat, min_seed, max_occ)
        layer1.append(res)
        both += [(strand, c) for c in chains_of(res[0], starts, n, G, B, S)]
    both.sort(key=lambda sc: (-sc[1]["score"], sc[0], sc[1]["te"], sc[1]["qe"]))
    return both, layer1


def map_long(tb, starts, reads, min_seed, max_occ, G, B, S, max_sec=0):
    """-> the arrays FmIndex.map_long returns (NAMES)"""
    hit_off, mapq, nchains, rows = [0], [], [], []
    for read in reads:
        read = read.encode() if isinstance(read, str) else bytes(read)
        m = len(read)
        both, _ = read_chains(tb, starts, read, min_seed, max_occ, G, B, S)
        nchains.append(len(both))
        mapq.append(mapq_of([c["score"] for _, c in both]))
        for strand, c in both[:1 + max_sec]:
            q = 0 if starts is None else seq_of(starts, c["ts"])
            off = c["ts"] if starts is None else c["ts"] - int(starts[q])
            qs, qe = (m - c["qe"], m - c["qs"]) if strand else (c["qs"], c["qe"])
            rows.append((strand, q, off, c["ts"], c["te"], qs, qe, c["score"], c["n"], c["match"]))
        hit_off.append(len(rows))
    cols = tuple(np.array([r[k] for r in rows], dtype=dt) for k, dt in enumerate(_LONG_TYPES))
    return (np.array(hit_off, dtype=np.uint64), np.array(mapq, dtype=np.uint8), np.array(nchains, dtype=np.uint64)) + cols


def per_read(res):
    """[(mapq, nchains, [rows of the returned chains as tuples])] from the arrays"""
    hit_off = [int(x) for x in res[0]]
    return [(int(res[1][p]), int(res[2][p]), [tuple(int(col[i]) for col in res[3:]) for i in range(hit_off[p], hit_off[p + 1])])
            for p in range(len(hit_off) - 1)]


def paf_lines(names, starts, n, base_name, qnames, reads, res, secondary=0):
    """the PAF lines bwtsearch --paf --secondary N prints, from the arrays of map_long with max_sec = max(N, 1) (the runner-up's
    score goes into the primary line): one per chain, the primary and at most N more"""
    out = []
    for p, (mq, nc, rows) in enumerate(per_read(res)):
        for r, (strand, q, off, ts, te, qs, qe, score, cn, match) in enumerate(rows[:1 + secondary]):
            tname = names[q] if names else base_name
            tlen = int(starts[q + 1]) - int(starts[q]) if names else n
            tags = ["tp:A:%s" % ("S" if r else "P"), "cm:i:%d" % cn, "s1:i:%d" % score]
            if r == 0 and len(rows) > 1:
                tags.append("s2:i:%d" % rows[1][7])
            out.append("\t".join([qnames[p], str(len(reads[p])), str(qs), str(qe), "-" if strand else "+", tname, str(tlen), str(off),
                                  str(off + te - ts), str(match), str(max(qe - qs, te - ts)), str(0 if r else mq)] + tags))
    return out
