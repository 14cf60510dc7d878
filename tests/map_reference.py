"""Plain Python reference for mapping reads (include/pfpgpu.h, "Mapping reads"), written from the definitions: the reverse
complement by a dict, inside by numpy.searchsorted on the table, shadowing over all pairs, the order by Python's tuple sort, the
MAPQ rule as written, the MD string by the walk over cigar_reference.script, and a SAM formatter.  It starts from the alignments
FmIndex.align lists for the reads and their reverse complements (that call has its own tests); nothing else here calls the
library."""
import numpy as np

import cigar_reference as G

COMPLEMENT = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C"),
              ord("a"): ord("t"), ord("t"): ord("a"), ord("c"): ord("g"), ord("g"): ord("c")}


def revcomp(p):
    return bytes(COMPLEMENT.get(b, b) for b in reversed(bytes(p)))


def interleaved(reads):
    """pattern 2p = read p, 2p + 1 = its reverse complement: what FmIndex.align is asked"""
    out = []
    for r in reads:
        r = r.encode() if isinstance(r, str) else bytes(r)
        out += [r, revcomp(r)]
    return out


def seq_of(starts, x):
    """the one k with starts[k] <= x < starts[k+1]"""
    return int(np.searchsorted(np.asarray(starts, dtype=np.uint64), np.uint64(x), side="right")) - 1


def is_inside(starts, s, e):
    return s < e and e <= int(starts[seq_of(starts, s) + 1])


def hits_of(starts, cands):
    """cands: [(d, strand, s, e)] of one read -> its hits: inside, not shadowed, in key order.  Shadowing by the definition, over
    all pairs"""
    ins = [c for c in cands if is_inside(starts, c[2], c[3])]
    keep = [a for a in ins if not any(b < a and max(a[2], b[2]) < min(a[3], b[3]) for b in ins)]
    return sorted(keep)


def hits_by_window(starts, cands, m, k):
    """the same by the sorted-window method: the candidates ordered by s, each looks left while s_b > s_a - (m + k) and right
    while s_b < e_a"""
    ins = sorted((c for c in cands if is_inside(starts, c[2], c[3])), key=lambda c: c[2])
    keep = []
    for i, a in enumerate(ins):
        shadowed = False
        t = i - 1
        while t >= 0 and ins[t][2] + m + k > a[2] and not shadowed:
            b = ins[t]
            shadowed = b < a and b[3] > a[2]
            t -= 1
        t = i + 1
        while t < len(ins) and ins[t][2] < a[3] and not shadowed:
            shadowed = ins[t] < a
            t += 1
        if not shadowed:
            keep.append(a)
    return sorted(keep)


def mapq_of(dists):
    """dists: the hits' distances in hit order"""
    if not dists:
        return 0
    d1 = dists[0]
    if any(d == d1 for d in dists[1:]):
        return 0
    if len(dists) == 1:
        return 60
    return min(60, 10 * (min(d for d in dists if d > d1) - d1))


def md_of(text, runs, s):
    """the MD string (bytes) of a script against the text from position s on"""
    out = bytearray()
    j, run = int(s), 0
    for r in runs:
        ln, op = int(r) >> 4, int(r) & 15
        if op == G.OP_EQ:
            run += ln
            j += ln
        elif op == G.OP_X:
            for _ in range(ln):
                out += b"%d" % run
                out.append(int(text[j]))
                run = 0
                j += 1
        elif op == G.OP_D:
            out += b"%d^" % run
            out += bytes(bytearray(int(c) for c in text[j:j + ln]))
            run = 0
            j += ln
    out += b"%d" % run
    return bytes(out)


def rebuild_span(pat, runs, md):
    """T[s..e) from the strand's pattern, the script and the MD string alone (asserts that the three agree)"""
    pat, md = bytes(pat), bytes(md)
    out = bytearray()
    i = q = run = 0

    def number():
        nonlocal q
        digits = b"%d" % run
        assert md[q:q + len(digits)] == digits, (md, q, run)
        q += len(digits)
    for r in runs:
        ln, op = int(r) >> 4, int(r) & 15
        if op == G.OP_EQ:
            out += pat[i:i + ln]
            i += ln
            run += ln
        elif op == G.OP_X:
            for _ in range(ln):
                number()
                out.append(md[q])
                q += 1
                i += 1
                run = 0
        elif op == G.OP_I:
            i += ln
        else:
            number()
            assert md[q:q + 1] == b"^", (md, q)
            out += md[q + 1:q + 1 + ln]
            q += 1 + ln
            run = 0
    number()
    assert q == len(md) and i == len(pat), (md, q, i, len(pat))
    return bytes(out)


def map_reads(text, starts, reads, aln, k, max_sec=0, memo=None):
    """what FmIndex.map_reads returns, from aln = FmIndex.align(interleaved(reads), k, min_seed): (hit_off, mapq, nhits, strand,
    seq, off, start, dist, cig_off, cig, md_off, md); memo: a dict that keeps the scripts of ONE text and ONE k"""
    memo = {} if memo is None else memo
    aln_off, a_start, a_end, a_dist = (np.asarray(x).tolist() for x in aln)
    pats = interleaved(reads)
    hit_off, mapq, nhits, rows, cig_off, cig, md_off, md = [0], [], [], [], [0], [], [0], bytearray()
    for p in range(len(reads)):
        cands = [(a_dist[j], strand, a_start[j], a_end[j]) for strand in (0, 1) for j in range(aln_off[2 * p + strand], aln_off[2 * p + strand + 1])]
        hits = hits_of(starts, cands)
        nhits.append(len(hits))
        mapq.append(mapq_of([h[0] for h in hits]))
        for d, strand, s, e in hits[:1 + max_sec]:
            key = (pats[2 * p + strand], s, e)
            if key not in memo:
                memo[key] = G.script(text, key[0], s, e, k)
            d2, runs = memo[key]
            assert d2 == d, (key, d, d2)
            q = seq_of(starts, s)
            rows.append((strand, q, s - int(starts[q]), s, d))
            cig += runs
            cig_off.append(len(cig))
            md += md_of(text, runs, s)
            md_off.append(len(md))
        hit_off.append(len(rows))
    col = lambda i, dt: np.array([r[i] for r in rows], dtype=dt)
    u64 = lambda a: np.array(a, dtype=np.uint64)
    return (u64(hit_off), np.array(mapq, dtype=np.uint8), u64(nhits), col(0, np.uint8), col(1, np.uint32), col(2, np.uint64), col(3, np.uint64),
            col(4, np.uint8), u64(cig_off), np.array(cig, dtype=np.uint32), u64(md_off), np.frombuffer(bytes(md), dtype=np.uint8).copy())


NAMES = ("hit_off", "mapq", "nhits", "strand", "seq", "off", "start", "dist", "cig_off", "cig", "md_off", "md")


def per_read(res):
    """a result as one entry per read: (mapq, nhits, [(strand, seq, off, start, dist, runs, md)])"""
    hit_off, mapq, nhits, strand, seq, off, start, dist, cig_off, cig, md_off, md = (np.asarray(x) for x in res)
    out = []
    for p in range(len(mapq)):
        hits = [(int(strand[i]), int(seq[i]), int(off[i]), int(start[i]), int(dist[i]), tuple(cig[int(cig_off[i]):int(cig_off[i + 1])].tolist()),
                 bytes(md[int(md_off[i]):int(md_off[i + 1])])) for i in range(int(hit_off[p]), int(hit_off[p + 1]))]
        out.append((int(mapq[p]), int(nhits[p]), hits))
    return out


def sam_header(names, starts):
    """names: bytes, in table order"""
    out = [b"@HD\tVN:1.6\tSO:unsorted"]
    for k, nm in enumerate(names):
        ln = int(starts[k + 1]) - int(starts[k])
        if ln:
            out.append(b"@SQ\tSN:%s\tLN:%d" % (bytes(nm), ln))
    out.append(b"@PG\tID:bwtsearch")
    return b"".join(x + b"\n" for x in out)


def sam_lines(names, qnames, reads, res):
    """the records of a result, reads in order: the primary, then the secondary hits returned"""
    out = []
    for p, (mq, nh, hits) in enumerate(per_read(res)):
        read = reads[p].encode() if isinstance(reads[p], str) else bytes(reads[p])
        qn = bytes(qnames[p])
        if not hits:
            out.append(b"%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t*" % (qn, read or b"*"))
        for t, (strand, q, off, _, d, runs, md) in enumerate(hits):
            flag = (16 if strand else 0) | (256 if t else 0)
            seq = revcomp(read) if strand else read
            out.append(b"%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t*\tNM:i:%d\tMD:Z:%s\tNH:i:%d" %
                       (qn, flag, bytes(names[q]), off + 1, 0 if t else mq, G.cigar_string(runs).encode(), seq or b"*", d, md, nh))
    return b"".join(x + b"\n" for x in out)
