"""The read pairs of the pairing tests (test_pair_reference.py on the CPU, test_fm_pairs.py and test_fm_pairs_cli.py on the GPU):
fragments of `dna` and `copies` (approx_reference.make_text, cut into the records of map_cases.TABLES) whose two ends are the
mates, forward/reverse.  Nothing here calls the library."""
import functools

import numpy as np

import map_cases as K
import map_reference as M
from extend_reference import planted

MIN_SEED, MIN_INS, MAX_INS = 12, 100, 500
TEXTS = (("dna", "records"), ("copies", "records"))


def ends(tb, i, F, m1, m2=None):
    """the mates of the fragment tb[i:i+F]: its first m1 bytes, and the reverse complement of its last m2"""
    m2 = m1 if m2 is None else m2
    return tb[i:i + m1], M.revcomp(tb[i + F - m2:i + F])


def every_tenth(read):
    """a substitution at bytes 5, 15, 25, ...: no exact stretch of 12 bytes is left"""
    r = bytearray(read)
    for j in range(5, len(r), 10):
        r[j] = ord("ACGT"["ACGT".index(chr(r[j])) ^ 1])
    return bytes(r)


@functools.lru_cache(maxsize=None)
def pairs_of(name):
    """[(kind, mate 1, mate 2)]: kind says what the pair was built to be; what it is, the reference decides"""
    tb = K.text_of(name).tobytes()
    rng = np.random.default_rng(60 + len(name))
    out = []
    add = lambda kind, pair: out.append((kind, pair[0], pair[1]))
    swap = lambda pair: (pair[1], pair[0])
    if name == "dna":                                       # records [1, 5000), [5000, 12345), [12345, 20000)
        add("plain", ends(tb, 2000, 300, 60))
        add("plain, mate 1 reversed", swap(ends(tb, 6000, 320, 60, 75)))
        a, b = ends(tb, 7000, 400, 100)
        add("edits", (planted(rng, a, 2, b"ACGT", True), planted(rng, b, 3, b"ACGT", False)))
        a, b = ends(tb, 8000, 350, 60, 40)
        add("rescue of mate 2", (a, every_tenth(b)))
        a, b = ends(tb, 13000, 280, 40, 60)
        add("rescue of mate 1", (every_tenth(a), b))
        a, b = ends(tb, 14000, 300, 40)
        add("both unseedable", (every_tenth(a), every_tenth(b)))
        add("same strand", (tb[3000:3060], tb[3240:3300]))
        add("facing outwards", (M.revcomp(tb[3500:3560]), tb[3740:3800]))
        for F in (MIN_INS - 1, MIN_INS, MAX_INS, MAX_INS + 1, MAX_INS + 60):
            add("insert %d" % F, ends(tb, 9000, F, 60))
        add("insert %d reversed" % (MAX_INS + 1), swap(ends(tb, 15000, MAX_INS + 1, 60)))
        add("two records", ends(tb, 4900, 300, 60))
        a, b = ends(tb, 4700, 290, 60, 40)                  # the mate ends 10 bytes before the record does: the window is clipped
        add("rescue at a record's end", (a, every_tenth(b)))
        a, b = ends(tb, 5010, 290, 40, 60)
        add("rescue at a record's start", (every_tenth(a), b))
        a, b = ends(tb, 4800, 300, 60, 40)                  # the mate lies across the boundary: nothing to rescue
        add("rescue across a boundary", (a, every_tenth(b)))
        add("the same span", (tb[10000:10060], M.revcomp(tb[10000:10060])))
        add("mate 2 unmapped", (tb[11000:11060], b"\x01" * 40))
        add("mate 1 unmapped", (bytes(rng.choice(list(b"ACGT"), 50).astype(np.uint8)), M.revcomp(tb[11500:11560])))
        add("both unmapped", (b"\x01" * 30, b""))
        add("empty mates", (b"", b""))
    else:                                                   # five copies of 4000 bytes that differ in 1 % of their bytes
        base = [tb[4000 * c:4000 * (c + 1)] for c in range(5)]
        diff = lambda i, j: [c for c in range(5) if base[c][i:j] != base[0][i:j]]
        same = next(i for i in range(100, 3000) if not diff(i, i + 50) and not diff(i + 250, i + 300))      # (both mates)
        add("every copy alike", ends(tb, same, 300, 50))
        # mates that are exact in some copies and one substitution away in the others
        one = next(i for i in range(100, 3000) if 0 < len(diff(i, i + 50)) < 5 and not diff(i + 250, i + 300) and
                   all(sum(x != y for x, y in zip(base[c][i:i + 50], base[0][i:i + 50])) == 1 for c in diff(i, i + 50)))
        add("one edit apart", ends(tb, one, 300, 50))
        add("rescue in every copy", (tb[same:same + 50], every_tenth(M.revcomp(tb[same + 260:same + 300]))))
        add("plain", ends(tb, 4001 + 1234, 250, 70))
        # mate 1 follows one copy up to a difference between two copies and the other copy behind it (map_cases.hybrids): seeds that
        # lead into different records, so more hits than a small C keeps
        for h in K.hybrids(name, "records", rng, 6):
            j = max(tb.find(h[:20]), 0)                      # the first copy that holds the read's first bytes
            add("hybrid", (h, M.revcomp(tb[j + 250:j + 310])))
    return out


@functools.lru_cache(maxsize=None)
def reads_of(name):
    """the interleaved reads: mate 1, mate 2, mate 1, ..."""
    out = []
    for _, a, b in pairs_of(name):
        out += [a, b]
    return out
