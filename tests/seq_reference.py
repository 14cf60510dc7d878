"""CPU reference for the sequences of a collection (include/pfpgpu.h, "Sequences of a collection").  It shares nothing with the
feature: occurrences come from a suffix array the caller got from the oracle (or from bytes.find), the mapping is
numpy.searchsorted, the filter is the definition x + m <= starts[k + 1], documents are numpy.unique.

A table is starts[0..nseq] with starts[0] = 0, non-decreasing, starts[nseq] = n; sequence k is text[starts[k]:starts[k+1]]."""
import numpy as np

NOSEQ, NOOFF = 2**32 - 1, 2**64 - 1


def seqmap(starts, positions):
    """(seq, off) per position: the one k with starts[k] <= x < starts[k+1] (never an empty sequence); (NOSEQ, NOOFF) for x >= n"""
    st = np.asarray(starts, dtype=np.uint64)
    x = np.asarray(positions, dtype=np.uint64)
    k = np.searchsorted(st, x, side="right").astype(np.int64) - 1
    inside = x < st[-1]
    k = np.where(inside, k, 0)
    seq = np.where(inside, k, NOSEQ).astype(np.uint32)
    off = np.where(inside, x - st[k], np.uint64(NOOFF)).astype(np.uint64)
    return seq, off


def keep(starts, positions, m):
    """mask of the positions of a pattern of m bytes that lie inside one sequence: x < n and x + m <= starts[seq(x) + 1]"""
    st = np.asarray(starts, dtype=np.uint64)
    x = np.asarray(positions, dtype=np.uint64)
    inside = x < st[-1]
    k = np.where(inside, np.searchsorted(st, x, side="right").astype(np.int64) - 1, 0)
    return inside & (x + np.uint64(m) <= st[k + 1])


def occurrences_find(text, pat):
    """every position of pat in text by bytes.find, ascending (the empty pattern: 0..n)"""
    tb, out, i = bytes(text), [], 0
    if 0 in pat:
        return np.zeros(0, dtype=np.uint64)
    while True:
        i = tb.find(pat, i)
        if i < 0:
            break
        out.append(i)
        i += 1
    return np.array(out, dtype=np.uint64)


def locate_seqs(starts, rows_pos, m, max_occ=0):
    """rows_pos: the pattern's positions in row order (SA[sp:ep]).  -> (seq, off) of the kept ones among the first max_occ rows"""
    x = np.asarray(rows_pos, dtype=np.uint64)
    if max_occ:
        x = x[:max_occ]
    x = x[keep(starts, x, m)]
    return seqmap(starts, x)


def doclist(starts, positions, m):
    """(docs ascending, counts) over all kept positions"""
    x = np.asarray(positions, dtype=np.uint64)
    seq, _ = seqmap(starts, x[keep(starts, x, m)])
    docs, cnt = np.unique(seq, return_counts=True)
    return docs.astype(np.uint32), cnt.astype(np.uint64)


def reverse_complement(p):
    comp = {65: 84, 84: 65, 67: 71, 71: 67, 97: 116, 116: 97, 99: 103, 103: 99}
    out = bytearray()
    for b in reversed(bytes(p)):
        out.append(comp.get(b, b))
    return bytes(out)


def parse_fasta_table(raw):
    """(names, lengths) of a well-formed multi-line FASTA as the reader delivers it: name up to white space, bytes of the sequence
    lines without their line ends.  For the tests' own inputs only (no FASTQ, no special bytes)."""
    names, lens = [], []
    for rec in raw.split(b">")[1:]:
        lines = rec.split(b"\n")
        names.append(lines[0].split()[0] if lines[0].split() else b"")
        lens.append(sum(len(ln.rstrip(b"\r")) for ln in lines[1:]))
    return names, lens
