"""Aligning chains in plain Python: include/pfpgpu.h, "Aligning chains", restated - the script of a gap by the full, unbanded matrix
and the traceback of cigar_reference.py, the members of a chain as chain_reference.py's peel lists them, trimming, stitching with
merged seams, nm and unfilled, the strand turn of long reads and the PAF line of bwtsearch --paf --cigar.  Everything is exact
integer work; the GPU tests compare with it array by array (test_fm_fill.py), test_fill_reference.py checks it on the CPU.
Nothing here calls the library."""
import functools

import numpy as np

import chain_reference as R
import cigar_reference as CR
from map_reference import seq_of

NONE = 0xFFFFFFFF
MAX_F, MAX_LEN = 4096, 65535
CHAIN_ALN_NAMES = R.CHAIN_NAMES + ("aqs", "ats", "nm", "unfilled", "cig_off", "cig", "mem_off", "mem")
LONG_ALN_NAMES = R.NAMES + ("aqs", "ats", "nm", "unfilled", "cig_off", "cig")


def full_script(p, t, memo=None):
    """(D, runs) of pattern bytes p against text bytes t on the full matrix; memo: a dict that keeps them"""
    key = (bytes(p), bytes(t))
    if memo is not None and key in memo:
        return memo[key]
    pa, ta = np.frombuffer(key[0], dtype=np.uint8), np.frombuffer(key[1], dtype=np.uint8)
    D = CR.matrix(pa, ta)
    out = (int(D[len(pa), len(ta)]), CR.rle(CR.traceback(pa, ta, D)))
    if memo is not None:
        memo[key] = out
    return out


def gap_script(p, t, F, memo=None):
    """(dist, runs) of layer 1 for two strings that passed the range tests: (NONE, []) above F"""
    if len(p) > MAX_LEN or len(t) > MAX_LEN or abs(len(p) - len(t)) > F:
        return NONE, []
    if not len(p) or not len(t):                            # (no matrix needed; F >= |a - b| holds)
        ln, op = (len(t), CR.OP_D) if not len(p) else (len(p), CR.OP_I)
        return ln, ([ln << 4 | op] if ln else [])
    d, runs = full_script(p, t, memo)
    return (d, runs) if d <= F else (NONE, [])


def segment(text, pats, p, q0, q1, t0, t1, F, memo=None):
    if not 0 <= p < len(pats) or q0 > q1 or q1 > len(pats[p]) or t0 > t1 or t1 > len(text):
        return NONE, []
    return gap_script(bytes(pats[p])[q0:q1], bytes(text[t0:t1]), F, memo)


def fill(text, pats, segs, F, memo=None):
    """(dist, cig_off, cig) as FmIndex.fill returns them; segs: [(p, q0, q1, t0, t1)]"""
    dist, off, cig = [], [0], []
    for p, q0, q1, t0, t1 in segs:
        d, runs = segment(text, pats, int(p), int(q0), int(q1), int(t0), int(t1), F, memo)
        dist.append(d)
        cig += runs
        off.append(len(cig))
    return np.array(dist, dtype=np.uint32), np.array(off, dtype=np.uint64), np.array(cig, dtype=np.uint32)


def trimmed(anc, members):
    """the members' anchors (i, len, t) after trimming, and each one's o"""
    out, cut = [], []
    for r, x in enumerate(members):
        i, ln, t = anc[x]
        o = 0
        if r:
            pi, pl, pt = anc[members[r - 1]]
            o = max(0, pi + pl - i, pt + pl - t)
            assert o <= ln - 1, (anc[members[r - 1]], anc[x])
        out.append((i + o, ln - o, t + o))
        cut.append(o)
    return out, cut


def merge(runs):
    out = []
    for r in runs:
        if r >> 4 == 0:
            continue
        if out and out[-1] & 15 == r & 15:
            out[-1] += r >> 4 << 4
        else:
            out.append(r)
    return out


def chain_script(text, pat, anc, members, F, memo=None):
    """-> dict(aqs, ats, nm, unfilled, runs, gaps): gaps = [(a, b, dist or NONE, o)] of members 1 ..; the pattern may be shorter
    than a caller's anchors claim: such a gap has no script"""
    tr, cut = trimmed(anc, members)
    runs, gaps, unfilled = [tr[0][1] << 4 | CR.OP_EQ], [], 0
    for r in range(1, len(tr)):
        pi, pl, pt = anc[members[r - 1]]
        q0, t0 = pi + pl, pt + pl
        q1, t1 = tr[r][0], tr[r][2]
        a, b = q1 - q0, t1 - t0
        d = 0
        if a or b:
            d, g = segment(text, [pat], 0, q0, q1, t0, t1, F, memo)
            if d == NONE:
                unfilled += 1
                g = [a << 4 | CR.OP_I, b << 4 | CR.OP_D]
            runs += g
        gaps.append((a, b, d, cut[r]))
        runs.append(tr[r][1] << 4 | CR.OP_EQ)
    runs = merge(runs)
    return dict(aqs=anc[members[0]][0], ats=anc[members[0]][2], nm=sum(r >> 4 for r in runs if r & 15 != CR.OP_EQ), unfilled=unfilled,
                runs=runs, gaps=gaps)


def chain_align(text, starts, pats, anchor_sets, G, B, S, max_chains, F, memo=None):
    """-> the arrays FmIndex.chain_align returns (CHAIN_ALN_NAMES)"""
    n = len(text)
    per = [R.chains_of(a, starts, n, G, B, S, max_chains) for a in anchor_sets]
    first = R.chain_arrays(per)
    rows, cig_off, cig, mem_off, mem = [], [0], [], [0], []
    for p, chains in enumerate(per):
        for c in chains:
            s = chain_script(text, bytes(pats[p]), anchor_sets[p], c["anchors"], F, memo)
            rows.append((s["aqs"], s["ats"], s["nm"], s["unfilled"]))
            cig += s["runs"]
            cig_off.append(len(cig))
            mem += c["anchors"]
            mem_off.append(len(mem))
    cols = tuple(np.array([r[k] for r in rows], dtype=dt) for k, dt in enumerate((np.uint32, np.uint64, np.uint32, np.uint32)))
    return first + cols + (np.array(cig_off, dtype=np.uint64), np.array(cig, dtype=np.uint32), np.array(mem_off, dtype=np.uint64),
                           np.array(mem, dtype=np.uint32))


@functools.lru_cache(maxsize=None)
def _read_chains(tb, starts_key, read, min_seed, max_occ, G, B, S):
    """chain_reference.read_chains, once per read and setting (the brute-force anchors are what takes long)"""
    starts = None if starts_key is None else np.array(starts_key, dtype=np.uint64)
    return R.read_chains(tb, starts, read, min_seed, max_occ, G, B, S)


def read_chains(tb, starts, read, min_seed, max_occ, G, B, S):
    return _read_chains(bytes(tb), None if starts is None else tuple(int(x) for x in starts), bytes(read), min_seed, max_occ, G, B, S)


def read_alignments(tb, starts, read, min_seed, max_occ, G, B, S, max_sec, F, memo=None):
    """the returned chains of one read: [(strand, chain, script)], script as chain_script gives it over the strand's pattern (aqs
    not yet turned); and the read's number of chains"""
    from map_reference import revcomp
    both, layer1 = read_chains(tb, starts, read, min_seed, max_occ, G, B, S)
    strands = (bytes(read), revcomp(read))
    return [(st, c, chain_script(tb, strands[st], layer1[st][0], c["anchors"], F, memo)) for st, c in both[:1 + max_sec]], both


def map_long_aln(tb, starts, reads, min_seed, max_occ, G, B, S, max_sec, F, memo=None):
    """-> the arrays FmIndex.map_long_aln returns (LONG_ALN_NAMES)"""
    hit_off, mapq, nchains, head, rows, cig_off, cig = [0], [], [], [], [], [0], []
    for read in reads:
        read = read.encode() if isinstance(read, str) else bytes(read)
        m = len(read)
        kept, both = read_alignments(tb, starts, read, min_seed, max_occ, G, B, S, max_sec, F, memo)
        nchains.append(len(both))
        mapq.append(R.mapq_of([c["score"] for _, c in both]))
        for strand, c, s in kept:
            q = 0 if starts is None else seq_of(starts, c["ts"])                # (pfp_fm_map_long's fields, as chain_reference.map_long)
            off = c["ts"] if starts is None else c["ts"] - int(starts[q])
            qs, qe = (m - c["qe"], m - c["qs"]) if strand else (c["qs"], c["qe"])
            head.append((strand, q, off, c["ts"], c["te"], qs, qe, c["score"], c["n"], c["match"]))
            rows.append((len(read) - s["aqs"] if strand else s["aqs"], s["ats"], s["nm"], s["unfilled"]))       # the strand turn
            cig += s["runs"]
            cig_off.append(len(cig))
        hit_off.append(len(rows))
    first = (np.array(hit_off, dtype=np.uint64), np.array(mapq, dtype=np.uint8), np.array(nchains, dtype=np.uint64)) + \
        tuple(np.array([r[k] for r in head], dtype=dt) for k, dt in enumerate(R._LONG_TYPES))
    cols = tuple(np.array([r[k] for r in rows], dtype=dt) for k, dt in enumerate((np.uint32, np.uint64, np.uint32, np.uint32)))
    return first + cols + (np.array(cig_off, dtype=np.uint64), np.array(cig, dtype=np.uint32))


def validate_chain(pat, text, aqs, qe, ats, te, runs, nm):
    """replays a chain's script: it consumes exactly pat[aqs:qe] and text[ats:te], '=' where the bytes are equal and not 0, X where
    they differ, no two neighbouring runs of one operation, and nm is the number of edits"""
    CR.validate(bytes(pat)[aqs:qe], bytes(text[ats:te]), runs, nm)


def paf_lines(names, starts, n, base_name, qnames, reads, res, secondary=0):
    """the PAF lines bwtsearch --paf --cigar --secondary N prints, from the arrays of map_long_aln with max_sec = max(N, 1)"""
    out = []
    hit_off = [int(x) for x in res[0]]
    cig_off = [int(x) for x in res[17]]
    for p, (mq, nc, rows) in enumerate(R.per_read(res[:13])):
        for r, (strand, q, off, ts, te, qs, qe, score, cn, match) in enumerate(rows[:1 + secondary]):
            h = hit_off[p] + r
            aqs, ats, nm, unf = (int(res[k][h]) for k in (13, 14, 15, 16))
            runs = [int(x) for x in res[18][cig_off[h]:cig_off[h + 1]]]
            tname = names[q] if names else base_name
            tlen = int(starts[q + 1]) - int(starts[q]) if names else n
            tags = ["tp:A:%s" % ("S" if r else "P"), "cm:i:%d" % cn, "s1:i:%d" % score]
            if r == 0 and len(rows) > 1:
                tags.append("s2:i:%d" % rows[1][7])
            tags.append("NM:i:%d" % nm)
            if unf:
                tags.append("uf:i:%d" % unf)
            tags.append("cg:Z:" + CR.cigar_string(runs))
            a, b = (qs, aqs) if strand else (aqs, qe)
            out.append("\t".join([qnames[p], str(len(reads[p])), str(a), str(b), "-" if strand else "+", tname, str(tlen), str(off + ats - ts),
                                  str(off + te - ts), str(sum(x >> 4 for x in runs if x & 15 == CR.OP_EQ)), str(sum(x >> 4 for x in runs)),
                                  str(0 if r else mq)] + tags))
    return out
