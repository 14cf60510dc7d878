"""The reads and anchor sets of the chaining tests (test_chain_reference.py on the CPU, test_fm_chain.py on the GPU): reads cut
from the texts and record tables of map_cases.py, and caller-made anchor sets that need no text.  Nothing here calls the library."""
import functools

import numpy as np

import map_cases as K
from map_reference import revcomp

H = 64

# (text, table or None, min_seed, max_occ, G, B, S, max_sec): the read cases of layers 1 and 3
READ_CASES = {
    "dna": ("dna", "records", 12, 500, 5000, 500, 40, 3),
    "dna small gap": ("dna", "records", 12, 500, 64, 500, 20, 3),
    "dna small band": ("dna", "records", 12, 500, 5000, 30, 20, 3),
    "dna no table": ("dna", None, 12, 500, 5000, 500, 40, 0),
    "copies": ("copies", "records", 16, 5, 5000, 500, 40, 2),
    "copies filtered": ("copies", "records", 16, 4, 5000, 500, 40, 2),
    "copies one record": ("copies", "one", 16, 500, 5000, 500, 40, 8),
    "ab": ("ab", "records", 10, 65536, 5000, 500, 15, 1),
}


def starts_of(name, table):
    return None if table is None else K.starts_of(name, table)


def with_substitutions(s, every, first=None):
    """s with every `every`-th byte (from `first` on) turned into another letter of ACGT"""
    b = bytearray(s)
    for j in range(every // 2 if first is None else first, len(b), every):
        b[j] = b"ACGT"[(b"ACGT".index(bytes([b[j]])) + 1 + j % 3) % 4]
    return bytes(b)


def common_window(tb, m, count):
    """the first i < 4000 - m where tb[i:i+m] occurs exactly `count` times in tb (copies: once per copy)"""
    for i in range(0, 4000 - m):
        if tb.count(tb[i:i + m]) == count and all(tb[4000 * c + i:4000 * c + i + m] == tb[i:i + m] for c in range(count)):
            return i
    raise AssertionError("no window occurs %d times" % count)


@functools.lru_cache(maxsize=None)
def reads_of(case):
    name, table, min_seed, max_occ, G, B, S, _ = READ_CASES[case]
    tb = K.text_of(name).tobytes()
    absent = bytes([min(c for c in range(1, 256) if c not in set(tb))])
    reads = []
    if name == "dna":
        a = 6000                                            # record 3 = [5000, 12345)
        reads.append(with_substitutions(tb[a:a + 1000], 40))                    # a chain of some 25 anchors
        reads.append(revcomp(with_substitutions(tb[a + 1500:a + 2300], 37)))    # the same on strand 1
        reads.append(tb[a:a + 300] + b"T" + tb[a + 300:a + 600])                # a 1-byte insertion
        reads.append(tb[a:a + 300] + tb[a + 301:a + 600])                       # a 1-byte deletion
        reads.append(tb[a:a + 300] + tb[17000:17030] + tb[a + 300:a + 600])     # a 30-byte insertion
        reads.append(tb[a:a + 300] + tb[a + 330:a + 600])                       # a 30-byte deletion
        for d in (G - 20, G - 19, G, G + 1) if G < 1000 else (B, B + 1):        # deletions around G (short anchors behind them), or B
            tail = with_substitutions(tb[a + 200 + d:a + 400 + d], 20, 19)
            reads.append(tb[a:a + 200] + tail)
        for d in (B, B + 1):                                                    # an insertion that shifts the diagonal by B, B + 1
            if d <= 600:
                reads.append(tb[a:a + 150] + tb[15000:15000 + d] + with_substitutions(tb[a + 150:a + 300], 25, 24))
        reads.append(tb[2000:2300] + tb[13000:13600])                           # a chimera of records 2 and 4: 300 against 600
        reads.append(revcomp(tb[13000:13600]) + tb[2000:2030])                  # a 30-byte half: below S
        reads.append(with_substitutions(tb[4800:5300], 45))                     # across the border at 5000
        reads.append(tb[4980:5020])                                             # one MEM, across the border: nothing
        reads.append(tb[12300:12345] + tb[12345:12400])                         # across the border at 12345, exact
        reads += [tb[100:100 + min_seed - 1], b"", tb[300:340] + absent + tb[341:400], absent * 50, b"\x00" + tb[700:760]]
        reads.append(revcomp(tb[9000:9200]) + absent + tb[9300:9700])           # both strands in one read
    elif name == "copies":
        i5 = common_window(tb, 80, 5)
        reads.append(tb[i5:i5 + 80])                                            # one MEM with 5 occurrences: max_occ and max_occ + 1
        reads.append(revcomp(tb[4000 + i5:4000 + i5 + 80]))
        reads.append(tb[8100:8900])                                             # copy 2 as it is: its differences cut the others' chains
        reads.append(with_substitutions(tb[12200:13000], 50))                   # copy 3 with substitutions
        reads.append(revcomp(tb[16500:17500]))
        reads.append(tb[3900:4100])                                             # across the copies' border (records: 4000, 4001)
        reads.append(tb[500:900] + tb[6000:6400])                               # a chimera of two copies, and of two places
        reads += [b"", tb[10:20], absent * 20]
    else:                                                                       # ab: a^3000 b a^2000
        reads += [b"a" * 20 + b"b" + b"a" * 20, b"a" * 3000 + b"b", b"a" * 40, b"b" + b"a" * 1999, b"a" * 9, b"ab" * 30,
                  b"a" * 1990 + absent + b"a" * 1995]
    return reads


# ---------------------------------------------------------------- caller-made anchor sets (layer 2)
# They are chained over `dna` with its record table [0, 1, 1, 5000, 12345, 20000]: t in [1, 5000) is record 2.
CHAIN_TEXT, CHAIN_TABLE = "dna", "records"


def diagonal(A, step=10, length=8, i0=0, t0=1000):
    return [(i0 + step * k, length, t0 + step * k) for k in range(A)]


def h_back(fillers):
    """anchor 0, `fillers` anchors that are no predecessors of the last (their qe lies above its), and the last: its one
    predecessor lies fillers + 1 back"""
    return [(0, 40, 1000)] + [(90 + k, 10, 1031 + k) for k in range(fillers)] + [(50, 20, 1031 + fillers + 30)]


def random_set(rng, A):
    """A anchors around a few diagonals, two records, with ties in te and in qe"""
    out = set()
    while len(out) < A:
        d = int(rng.choice([1000, 1040, 3000, 6000]))
        i = int(rng.integers(0, 400))
        out.add((i, int(rng.integers(1, 30)), d + i + int(rng.integers(-3, 4))))
    seen, rows = set(), []
    for a in sorted(out, key=lambda a: (a[2] + a[1], a[0] + a[1])):
        if (a[2] + a[1], a[0] + a[1]) not in seen:
            seen.add((a[2] + a[1], a[0] + a[1]))
            rows.append(a)
    return rows


# name: ([anchor sets, one per pattern], G, B, S, max_chains)
@functools.lru_cache(maxsize=None)
def chain_sets():
    rng = np.random.default_rng(11)
    worked = [(0, 30, 1000), (31, 25, 1031), (60, 40, 1062), (101, 30, 1103), (10, 22, 5000), (40, 35, 5030)]
    shared = [(0, 50, 1000), (60, 20, 1060), (60, 20, 1064)]             # two anchors with one parent: scores 70 and 69 - 50 = 19
    sets = {
        "worked example": ([worked], 5000, 500, 20, 0),
        "sizes": ([diagonal(A) for A in (0, 1, 63, 64, 65, 129)], 5000, 500, 8, 0),
        "H back": ([h_back(63), h_back(64)], 5000, 500, 1, 0),
        "dq = 0, dt = 0": ([[(10, 20, 1000), (10, 20, 1050)], [(10, 20, 2000), (20, 20, 2000)]], 5000, 500, 1, 0),
        "two equal predecessors": ([[(40, 20, 990), (0, 20, 1028), (170, 30, 1159)]], 5000, 500, 1, 0),
        "f + gain = len": ([[(0, 10, 1000), (30, 20, 1068)]], 5000, 500, 1, 0),
        "negative gain": ([[(0, 50, 1000), (51, 5, 1151), (60, 30, 1170)]], 5000, 500, 1, 0),
        "shared parent, S": ([shared], 5000, 500, 19, 0),
        "shared parent, S - 1": ([shared], 5000, 500, 20, 0),
        "max_chains = 1": ([worked, shared, diagonal(5)], 5000, 500, 1, 1),
        "two records": ([[(0, 20, 4960), (20, 19, 4980), (40, 20, 5001), (60, 20, 5021)]], 5000, 500, 1, 0),
        "G": ([[(0, 10, 1000), (100, 10, 1100)], [(0, 10, 1000), (101, 10, 1101)], [(0, 10, 1000), (100, 10, 1090)]], 100, 500, 1, 0),
        "B": ([[(0, 30, 1000), (50, 30, 1080)], [(0, 30, 1000), (50, 30, 1081)]], 5000, 30, 1, 0),
        "random": ([random_set(rng, A) for A in (129, 100, 7, 64, 0, 129)], 300, 40, 10, 0),
        "random, max_chains = 2": ([random_set(rng, A) for A in (129, 65)], 5000, 500, 5, 2),
        "no patterns": ([], 5000, 500, 1, 0),
    }
    return sets


def offsets_and_rows(anchor_sets):
    off = np.zeros(len(anchor_sets) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(a) for a in anchor_sets], dtype=np.uint64)
    rows = [a for s in anchor_sets for a in s]
    return off, np.array(rows, dtype=np.uint64).reshape(-1, 3)
