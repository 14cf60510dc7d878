"""The tables and reads of the read-mapping tests (test_map_reference.py on the CPU, test_fm_map.py on the GPU): the texts of
approx_reference.make_text cut into records, and reads planted in them.  Nothing here calls the library."""
import functools

import numpy as np

import approx_reference as R
import map_reference as M
from extend_reference import planted

# record tables: a zero-length record, a 1-byte record, a first and a last record; "one": a single-record table
TABLES = {
    ("copies", "records"): [0, 4000, 4000, 4001, 8000, 12000, 16000, 20000],
    ("copies", "one"): [0, 20000],
    ("dna", "records"): [0, 1, 1, 5000, 12345, 20000],
    ("ab", "records"): [0, 0, 1500, 3500, 5001],
}
SANITY_SEED = 7          # the generator seed of sanity_reads (test_map_reference.py confirms it on the CPU)


@functools.lru_cache(maxsize=None)
def text_of(name):
    return R.make_text(name)


def starts_of(name, table):
    return np.array(TABLES[(name, table)], dtype=np.uint64)


def sanity_reads(seed=SANITY_SEED, count=16):
    """[(read, strand, i)]: 100 bytes of `dna` at position i, inside one record, with 0..3 edits, given as they are (strand 0) or
    as their reverse complement (strand 1)"""
    tb = text_of("dna").tobytes()
    starts = TABLES[("dna", "records")]
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        i = int(rng.integers(0, len(tb) - 100 + 1))
        if not M.is_inside(starts, i, i + 100):
            continue
        q = len(out)
        read = planted(rng, tb[i:i + 100], q % 4, sorted(set(tb)), at_ends=q % 8 >= 4)
        strand = (q // 4) % 2
        out.append((M.revcomp(read) if strand else read, strand, i))
    return out


def hybrids(name, table, rng, count, m=160):
    """reads of `copies` that follow one copy up to a difference between two copies and the other copy behind it: several seeds
    that lead into different records, at different distances"""
    tb = text_of(name).tobytes()
    out = []
    for _ in range(count):
        i = int(rng.integers(0, 4000 - m))
        a, b = (int(x) for x in rng.choice(5, 2, replace=False))
        wa, wb = tb[4000 * a + i:4000 * a + i + m], tb[4000 * b + i:4000 * b + i + m]
        diff = [j for j in range(m) if wa[j] != wb[j]]
        cut = diff[len(diff) // 3] + 1 if diff else m // 2
        out.append(wa[:cut] + wb[cut:])
    return out


@functools.lru_cache(maxsize=None)
def reads_of(name, table, k):
    """the reads of one (text, table, k): planted with 0..k edits on both strands, across record boundaries, repeated in several
    records, their own reverse complement, dense candidates, an absent byte, m <= k, empty, unmappable"""
    tb = text_of(name).tobytes()
    n = len(tb)
    starts = TABLES[(name, table)]
    rng = np.random.default_rng(1000 * sorted(TABLES).index((name, table)) + k)
    alphabet = sorted(set(tb))
    absent = min(c for c in range(1, 256) if c not in alphabet)
    reads = []
    levels = sorted({0, min(1, k), k // 2, k})
    for q, m in enumerate((40, 64, 100, 100, 150, 150, 33, 300)):
        i = int(rng.integers(0, n - m + 1))
        r = planted(rng, tb[i:i + m], levels[q % len(levels)], alphabet, at_ends=q % 3 == 0)
        reads.append(M.revcomp(r) if q % 2 else r)
    for b in starts[1:-1]:                                  # across a boundary by 1 byte and by half, from either side
        for m, before in ((60, 1), (60, 30), (60, 59)):
            if b - before >= 0 and b - before + m <= n:
                r = tb[b - before:b - before + m]
                reads.append(r)
                reads.append(M.revcomp(r))
    if name == "copies":
        reads += hybrids(name, table, rng, 10)
        reads += [M.revcomp(r) for r in hybrids(name, table, rng, 2)]
        i = int(rng.integers(0, 3900))
        reads.append(tb[i:i + 80])                          # as it is in every copy that has no change there
    if name == "ab":
        c = bytes([absent])
        reads += [b"a" * 60, b"a" * 30 + b"b" + b"a" * 30, (b"a" * 20 + c) * 5 + b"a" * 20, (b"a" * 13 + b"b") + (b"a" * 25 + c) * 4 + b"a" * 25,
                  b"a" * 20 + b"b" + b"a" * 20 + c + b"a" * 20,
                  # four seeds that hold the text's one b, so each has one place: four diagonals 33 bytes apart, the spans overlap
                  c.join(b"a" * (15 + t) + b"b" + b"a" * 15 for t in range(4))]
    if name == "dna":
        reads += [tb[1642:1656], tb[1630:1670]]                 # AATCGAGCTCGATT is its own reverse complement
    reads += [b"ACGT" * 10, b"AATT", tb[100:140][:19] + bytes([absent]) + tb[120:160], bytes([absent]) * 30, b"", tb[7:7 + max(k, 1)], tb[50:52],
              bytes(rng.choice(alphabet, 25).astype(np.uint8)), b"\x00" + tb[300:350]]
    return reads
