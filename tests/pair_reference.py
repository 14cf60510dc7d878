"""Plain Python reference for mapping read pairs (include/pfpgpu.h, "Mapping read pairs"), written from the definitions: anchors,
proper, the rescue windows, the pairs of a pair of reads, the pair key, the same-locus rule, the pair MAPQ, TLEN, and the paired
SAM formatter.  It is applied to a per-read hit list - what FmIndex.map_reads returns with max_sec = C - 1, a call with its own
tests - and to a rescue callable (window_reference in the GPU tests, a table in the literals); nothing else here calls the library."""
import numpy as np

import cigar_reference as G
import map_reference as M

NONE = (0xFF, 2**64 - 1, 2**64 - 1)


def proper(starts, a, b, min_ins, max_ins):
    """a, b: (d, strand, s, e) of mate 1 and of mate 2, each inside one record"""
    if a[1] == b[1] or M.seq_of(starts, a[2]) != M.seq_of(starts, b[2]):
        return False
    f, r = (a, b) if a[1] == 0 else (b, a)
    return f[2] <= r[2] and f[3] <= r[3] and min_ins <= r[3] - f[2] <= max_ins


def rescue_window(starts, a, max_ins):
    """(lo, hi) in which the mate of anchor a is looked for"""
    q = M.seq_of(starts, a[2])
    b0, b1 = int(starts[q]), int(starts[q + 1])
    if a[1] == 0:
        return a[2], min(a[2] + max_ins, b1)
    return max(a[3] - min(a[3], max_ins), b0), a[3]


def pairs_of(starts, anchors1, anchors2, rescue, min_ins, max_ins):
    """[(a, b, which)]: which = None for two anchors, else the mate (0 or 1) that was rescued.  rescue(mate, strand, lo, hi) ->
    (d, s, e) of that mate's strand pattern in T[lo..hi), or NONE"""
    out = [(a, b, None) for a in anchors1 for b in anchors2 if proper(starts, a, b, min_ins, max_ins)]

    def rescued(a, mate):
        lo, hi = rescue_window(starts, a, max_ins)
        d, s, e = rescue(mate, 1 - a[1], lo, hi)
        return (d, 1 - a[1], s, e) if d != 0xFF and s < e else None
    for a in anchors1:
        if not any(proper(starts, a, b, min_ins, max_ins) for b in anchors2):
            b = rescued(a, 1)
            if b is not None and proper(starts, a, b, min_ins, max_ins):
                out.append((a, b, 1))
    for b in anchors2:
        if not any(proper(starts, a, b, min_ins, max_ins) for a in anchors1):
            a = rescued(b, 0)
            if a is not None and proper(starts, a, b, min_ins, max_ins):
                out.append((a, b, 0))
    assert len({(a, b) for a, b, _ in out}) == len(out)     # (distinct as values: see the header's argument)
    return out


def intersects(x, y):
    return max(x[2], y[2]) < min(x[3], y[3])


def pair_key(p):
    return (p[0][0] + p[1][0], p[0], p[1])


def pair_mapq(npairs, d1, d2):
    if npairs == 1:
        return 60
    return 0 if d2 == d1 else min(60, 10 * (d2 - d1))


def tlens(x, y):
    """x, y: (strand, s, e) of mates 1 and 2, or None -> their TLEN; the caller has checked that they share a record"""
    if x is None or y is None:
        return 0, 0
    span = max(x[2], y[2]) - min(x[1], y[1])
    return (span, -span) if x[1] <= y[1] else (-span, span)


def pair(starts, hits1, hits2, single1, single2, rescue, min_ins, max_ins, C):
    """hits: the hits of the mate in hit order, (d, strand, s, e), at least the first C; single = (mapq, nhits) of the mate alone.
    -> (proper, npairs, [per mate: (mapped, rescued, mapq, nhits, strand, s, e, d, tlen)])"""
    a1, a2 = list(hits1[:C]), list(hits2[:C])
    pairs = pairs_of(starts, a1, a2, rescue, min_ins, max_ins)
    rows = []
    if pairs:
        best = min(pairs, key=pair_key)
        others = [p for p in pairs if p is not best and
                  not (p[0][1] == best[0][1] and p[1][1] == best[1][1] and intersects(p[0], best[0]) and intersects(p[1], best[1]))]
        npairs = 1 + len(others)
        d1 = best[0][0] + best[1][0]
        mq = pair_mapq(npairs, d1, min((p[0][0] + p[1][0] for p in others), default=None))
        chosen = [(best[0], best[2] == 0, mq), (best[1], best[2] == 1, mq)]
    else:
        npairs = 0
        chosen = [(h[0], False, sg[0]) if h else None for h, sg in ((a1, single1), (a2, single2))]
    place = [None if c is None else (c[0][1], c[0][2], c[0][3]) for c in chosen]
    tl = (0, 0)
    if place[0] and place[1] and M.seq_of(starts, place[0][1]) == M.seq_of(starts, place[1][1]):
        tl = tlens(place[0], place[1])
    for c, sg, t in zip(chosen, (single1, single2), tl):
        if c is None:
            rows.append((0, 0, sg[0], sg[1], 0, 2**64 - 1, 2**64 - 1, 0xFF, 0))
        else:
            (d, strand, s, e), resc, mq = c
            rows.append((1, int(resc), mq, sg[1], strand, s, e, d, t))
    return int(bool(pairs)), npairs, rows


PAIR_NAMES = ("proper", "npairs", "mapped", "rescued", "mapq", "nhits", "strand", "seq", "off", "start", "dist", "tlen", "cig_off", "cig",
              "md_off", "md")


def hits_with_ends(res):
    """per read: ((mapq, nhits), [(d, strand, s, e)]) from a result of FmIndex.map_reads"""
    out = []
    for mq, nh, hits in M.per_read(res):
        out.append(((mq, nh), [(d, strand, s, s + sum(r >> 4 for r in runs if r & 15 != G.OP_I)) for strand, _, _, s, d, runs, _ in hits]))
    return out


def map_pairs(text, starts, reads, res, rescue, k, min_ins, max_ins, C, memo=None):
    """what FmIndex.map_pairs returns (PAIR_NAMES), from res = FmIndex.map_reads(reads, k, min_seed, C - 1).  rescue(r, strand, lo,
    hi): read r's strand pattern in T[lo..hi); memo: a dict that keeps the scripts of ONE text and ONE k"""
    memo = {} if memo is None else memo
    per = hits_with_ends(res)
    pats = M.interleaved(reads)
    prop, npairs, rows, cig_off, cig, md_off, md = [], [], [], [0], [], [0], bytearray()
    for q in range(len(reads) // 2):
        (sg1, h1), (sg2, h2) = per[2 * q], per[2 * q + 1]
        pr, n_p, two = pair(starts, h1, h2, sg1, sg2, lambda mate, strand, lo, hi: rescue(2 * q + mate, strand, lo, hi), min_ins, max_ins, C)
        prop.append(pr)
        npairs.append(n_p)
        for mate, (mapped, resc, mq, nh, strand, s, e, d, tl) in enumerate(two):
            r = 2 * q + mate
            if mapped:
                key = (pats[2 * r + strand], s, e)
                if key not in memo:
                    memo[key] = G.script(text, key[0], s, e, k)
                d2, runs = memo[key]
                assert d2 == d, (key, d, d2)
                sq = M.seq_of(starts, s)
                rows.append((mapped, resc, mq, nh, strand, sq, s - int(starts[sq]), s, d, tl))
                cig += runs
                md += M.md_of(text, runs, s)
            else:
                rows.append((0, 0, mq, nh, 0, 0xFFFFFFFF, 2**64 - 1, 2**64 - 1, 0xFF, 0))
            cig_off.append(len(cig))
            md_off.append(len(md))
    col = lambda i, dt: np.array([r[i] for r in rows], dtype=dt)
    u64 = lambda a: np.array(a, dtype=np.uint64)
    return (np.array(prop, dtype=np.uint8), u64(npairs), col(0, np.uint8), col(1, np.uint8), col(2, np.uint8), col(3, np.uint64), col(4, np.uint8),
            col(5, np.uint32), col(6, np.uint64), col(7, np.uint64), col(8, np.uint8), col(9, np.int64), u64(cig_off),
            np.array(cig, dtype=np.uint32), u64(md_off), np.frombuffer(bytes(md), dtype=np.uint8).copy())


def per_pair_read(res):
    """a result as one entry per read: (proper, npairs, mapped, rescued, mapq, nhits, strand, seq, off, start, dist, tlen, runs, md)"""
    prop, npairs, mapped, resc, mapq, nhits, strand, seq, off, start, dist, tlen, cig_off, cig, md_off, md = (np.asarray(x) for x in res)
    out = []
    for r in range(len(mapped)):
        out.append((int(prop[r // 2]), int(npairs[r // 2]), int(mapped[r]), int(resc[r]), int(mapq[r]), int(nhits[r]), int(strand[r]), int(seq[r]),
                    int(off[r]), int(start[r]), int(dist[r]), int(tlen[r]), tuple(cig[int(cig_off[r]):int(cig_off[r + 1])].tolist()),
                    bytes(md[int(md_off[r]):int(md_off[r + 1])])))
    return out


def strip_names(q1, q2):
    """the QNAME of a pair: a trailing /1 and /2 go when mate 1 ends in /1 and mate 2 in /2; else mate 1's name for both"""
    q1, q2 = bytes(q1), bytes(q2)
    return q1[:-2] if q1.endswith(b"/1") and q2.endswith(b"/2") else q1


def sam_lines_paired(names, qnames, reads, res):
    """the records of a result of FmIndex.map_pairs: one line per read, mate 1 then mate 2"""
    per = per_pair_read(res)
    out = []
    for q in range(len(reads) // 2):
        qn = strip_names(qnames[2 * q], qnames[2 * q + 1])
        for mate in (0, 1):
            me, other = per[2 * q + mate], per[2 * q + 1 - mate]
            prop, npairs, mapped, resc, mapq, nhits, strand, seq, off, _, d, tlen, runs, md = me
            read = reads[2 * q + mate]
            read = read.encode() if isinstance(read, str) else bytes(read)
            flag = 1 | (2 if prop else 0) | (0 if mapped else 4) | (0 if other[2] else 8) | (16 if mapped and strand else 0) | \
                (32 if other[2] and other[6] else 0) | (128 if mate else 64)
            rname, pos = (bytes(names[seq]), off + 1) if mapped else (bytes(names[other[7]]), other[8] + 1) if other[2] else (b"*", 0)
            if not other[2]:
                rnext, pnext = b"*", 0
            elif not mapped or other[7] == seq:
                rnext, pnext = b"=", other[8] + 1
            else:
                rnext, pnext = bytes(names[other[7]]), other[8] + 1
            sq = (M.revcomp(read) if mapped and strand else read) or b"*"
            line = b"%s\t%d\t%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t*" % (qn, flag, rname, pos, mapq if mapped else 0,
                                                               G.cigar_string(runs).encode() if mapped else b"*", rnext, pnext, tlen, sq)
            if mapped:
                line += b"\tNM:i:%d\tMD:Z:%s\tNH:i:%d" % (d, md, npairs if prop else nhits)
                if resc:
                    line += b"\tYR:i:1"
            out.append(line)
    return b"".join(x + b"\n" for x in out)
