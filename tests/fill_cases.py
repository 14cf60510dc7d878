"""The segments, anchor sets and reads of the chain-alignment tests (test_fill_reference.py on the CPU, test_fm_fill.py and
test_fm_fill_cli.py on the GPU), over the texts and record tables of map_cases.py; and the reference's answers to them, computed
once per process.  Nothing here calls the library."""
import functools

import numpy as np

import chain_cases as C
import fill_reference as F
import map_cases as K
from map_reference import revcomp

with_substitutions = C.with_substitutions


def subs(s, count, first=3, step=5):
    """s with `count` bytes, `step` apart from `first` on, turned into another letter of ACGT"""
    b = bytearray(s)
    assert first + step * (count - 1) < len(b)
    for k in range(count):
        j = first + step * k
        b[j] = b"ACGT"[(b"ACGT".index(bytes([b[j]])) + 1 + j % 3) % 4]
    return bytes(b)


# ---------------------------------------------------------------- segments (layer 1)
# name: (text, max_fill, patterns, [(p, q0, q1, t0, t1)], {segment index: the distance the case is about})
@functools.lru_cache(maxsize=None)
def segment_sets():
    tb = K.text_of("dna").tobytes()
    rng = np.random.default_rng(23)
    other = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 1100).astype(np.uint8))
    sets = {}
    # the shapes: empty sides, one byte, and every pair of lengths around the group's 16 and the wave's 64
    pats, segs = [tb[3000:3100]], [(0, 0, 0, 3000, 3000), (0, 0, 0, 3000, 3005), (0, 10, 17, 3010, 3010), (0, 5, 6, 3005, 3006), (0, 5, 6, 3006, 3007)]
    assert tb[3005] != tb[3006]
    for a in (15, 16, 17, 63, 64, 65):
        for b in (15, 16, 17, 63, 64, 65):
            pats.append(subs(tb[3000:3000 + a], 2))
            segs.append((len(pats) - 1, 0, a, 3000, 3000 + b))
    sets["shapes"] = ("dna", 40, pats, segs, {0: 0, 1: 5, 2: 7, 3: 0, 4: 1})
    # the slack steps: the distances the issue names, and those at which this schedule moves on (17 | 18 at slack 8, 65 | 66 at 32)
    want = (8, 9, 17, 18, 33, 34, 65, 66)
    sets["slack steps"] = ("dna", 100, [subs(tb[7000:7400], d) for d in want], [(k, 0, 400, 7000, 7400) for k in range(len(want))],
                           dict(enumerate(want)))
    # |a - b| = F and F + 1; D = F and F + 1
    sets["length difference at F"] = ("dna", 20, [tb[9000:9030]], [(0, 0, 30, 9000, 9050), (0, 0, 30, 9000, 9051), (0, 0, 30, 9020, 9020)],
                                      {0: 20, 1: F.NONE, 2: F.NONE})
    sets["distance at F"] = ("dna", 12, [subs(tb[9000:9100], 12), subs(tb[9000:9100], 13)], [(0, 0, 100, 9000, 9100), (1, 0, 100, 9000, 9100)],
                             {0: 12, 1: F.NONE})
    # insertions of random bytes, three substitutions around them (the alignment absorbs those): 100 bytes (a band of 256 cells),
    # 400 bytes (1024 cells), 1030 bytes (4160 cells)
    ins = lambda k: subs(tb[11000:11100], 2) + other[:k] + subs(tb[11100:11200], 1)
    sets["insertion 100"] = ("dna", 150, [ins(100)], [(0, 0, 300, 11000, 11200)], {0: 102})
    sets["insertion 400"] = ("dna", 500, [ins(400)], [(0, 0, 600, 11000, 11200)], {0: 400})
    sets["insertion 1030"] = ("dna", 1100, [ins(1030)], [(0, 0, 1230, 11000, 11200), (0, 0, 200, 11000, 12230)], {0: 1030})
    sets["pattern byte 0"] = ("dna", 10, [tb[5000:5020] + b"\x00" + tb[5021:5040], b"\x00"], [(0, 0, 40, 5000, 5040), (1, 0, 1, 5020, 5021)],
                              {0: 1, 1: 1})
    # many optimal scripts: the tie rule decides (text ab: a^3000 b a^2000)
    sets["ties"] = ("ab", 10, [b"aaaa", b"ababab", b"aaa", b"baab", b"abababababababababab"],
                    [(0, 0, 4, 100, 103), (1, 0, 6, 2998, 3003), (2, 0, 3, 100, 104), (3, 0, 4, 2999, 3002), (4, 0, 20, 2990, 3010), (0, 1, 3, 2999, 3002)],
                    {0: 1, 2: 1})
    long_pat = tb[:20000] * 4
    sets["invalid"] = ("dna", 50, [tb[100:200], long_pat],
                       [(2, 0, 10, 100, 110), (0, 11, 10, 100, 110), (0, 0, 101, 100, 201), (0, 0, 10, 111, 110), (0, 0, 10, 19995, 20001),
                        (1, 0, 66000, 0, 20000), (0xFFFFFFFF, 0, 0, 0, 0), (0, 0, 100, 100, 200), (0, 0, 10, 19990, 20000)],
                       {0: F.NONE, 1: F.NONE, 2: F.NONE, 3: F.NONE, 4: F.NONE, 5: F.NONE, 6: F.NONE, 7: 0})
    sets["F = 0"] = ("dna", 0, [tb[4000:4050], subs(tb[4000:4050], 1)],
                     [(0, 0, 50, 4000, 4050), (1, 0, 50, 4000, 4050), (0, 0, 0, 4000, 4000), (0, 3, 4, 4003, 4004), (1, 3, 4, 4003, 4004), (0, 0, 1, 4000, 4000)],
                     {0: 0, 1: F.NONE, 2: 0, 3: 0, 4: F.NONE, 5: F.NONE})
    sets["none"] = ("dna", 5, [], [], {})
    return sets


@functools.lru_cache(maxsize=None)
def expected_segments(name):
    text, max_fill, pats, segs, _ = segment_sets()[name]
    return F.fill(K.text_of(text), pats, segs, max_fill)


# whole patterns within 32 edits of a span: fill() and cigar() at k = 32 give the same runs
@functools.lru_cache(maxsize=None)
def whole_patterns():
    tb = K.text_of("dna").tobytes()
    pats = [subs(tb[6000:6200], d) for d in (0, 1, 9, 32)] + [tb[6000:6100] + tb[6110:6200], tb[6000:6100] + b"ACGTACGT" + subs(tb[6100:6200], 5), b""]
    spans = [(6000, 6200)] * 4 + [(6000, 6200), (6000, 6200), (6000, 6000)]
    return pats, spans


# ---------------------------------------------------------------- anchor sets (layer 2), over dna with its record table
# name: (patterns, [anchor sets, one per pattern], G, B, S, max_chains)
@functools.lru_cache(maxsize=None)
def anchor_sets():
    tb = K.text_of("dna").tobytes()
    rng = np.random.default_rng(29)
    rnd = lambda m: bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), m).astype(np.uint8))
    sets = {}
    # true anchors: a read cut from the text, with a substitution, an insertion and a deletion between its anchors
    read = tb[1000:1030] + (b"A" if tb[1030:1031] != b"A" else b"C") + tb[1031:1060] + b"GG" + tb[1060:1100] + tb[1103:1150]
    true = [(0, 30, 1000), (31, 29, 1031), (62, 40, 1060), (102, 47, 1103)]
    sets["true anchors"] = ([read], [true], 5000, 500, 20, 0)
    sets["overlaps"] = ([rnd(80), rnd(80), rnd(80), rnd(80)],
                        [[(0, 30, 1000), (25, 40, 1035)],         # in the read only
                         [(0, 30, 1000), (40, 40, 1025)],         # in the text only
                         [(0, 30, 1000), (25, 40, 1027)],         # in both
                         [(0, 30, 1000), (30, 40, 1030)]],        # touching: one run
                        5000, 500, 1, 0)
    sets["first member is not the least"] = ([rnd(110), rnd(150)],
                                             [[(0, 20, 1000), (5, 100, 930)],
                                              [(0, 50, 1000), (60, 30, 1058), (60, 20, 1070), (55, 40, 1066), (95, 50, 1093)]], 5000, 10, 1, 0)
    sets["single anchors"] = ([rnd(40), rnd(10), b""], [[(3, 30, 1500)], [], []], 5000, 500, 1, 0)
    shared = [(0, 50, 1000), (60, 20, 1060), (60, 20, 1064)]
    sets["shared parent"] = ([rnd(90)], [shared], 5000, 500, 19, 0)
    sets["unfilled"] = ([rnd(100), rnd(100), rnd(35)], [[(0, 30, 1000), (60, 30, 1050)], [(0, 30, 1000), (40, 30, 1040)], [(0, 30, 1000), (40, 30, 1040)]],
                        5000, 500, 1, 0)                          # (the third pattern ends inside its gap: no script at any F)
    for name in ("worked example", "sizes", "random", "random, max_chains = 2", "no patterns", "two records"):
        anc, G, B, S, mc = C.chain_sets()[name]
        sets["chain_cases: " + name] = ([rnd(max([i + ln for i, ln, _ in a] + [0]) + 7) for a in anc], [list(a) for a in anc], G, B, S, mc)
    for name, (pats, anc, *_rest) in sets.items():
        for a in anc:
            a.sort(key=lambda x: (x[2] + x[1], x[0] + x[1]))
    return sets


ANCHOR_FILLS = (500, 4)


@functools.lru_cache(maxsize=None)
def expected_anchor_set(name, max_fill):
    pats, anc, G, B, S, mc = anchor_sets()[name]
    return F.chain_align(K.text_of("dna"), K.starts_of("dna", "records"), pats, anc, G, B, S, mc, max_fill, _memo)


# ---------------------------------------------------------------- reads (layer 3)
# chain_cases.READ_CASES, and reads whose gaps need the band: stretches without a seed of min_seed bytes
READ_CASES = dict(C.READ_CASES)
READ_CASES["dna noisy"] = ("dna", "records", 12, 500, 5000, 500, 40, 1)
READ_FILLS = (500, 4)


@functools.lru_cache(maxsize=None)
def reads_of(case):
    if case in C.READ_CASES:
        return C.reads_of(case)
    tb = K.text_of("dna").tobytes()
    a = 14000
    noisy = lambda s, every: with_substitutions(s, every, every - 1)
    reads = [tb[a:a + 200] + noisy(tb[a + 200:a + 500], 8) + tb[a + 500:a + 700],                             # 37 substitutions in one gap
             revcomp(tb[a:a + 200] + noisy(tb[a + 200:a + 320], 8) + tb[a + 380:a + 600]),                    # and a 60-byte deletion inside one
             tb[a:a + 150] + noisy(tb[a + 150:a + 250], 9) + tb[16000:16090] + noisy(tb[a + 250:a + 330], 9) + tb[a + 330:a + 500],
             tb[a:a + 100] + noisy(tb[a + 100:a + 140], 6) + tb[a + 140:a + 300]]                             # a narrow band
    return reads


_memo = {}


@functools.lru_cache(maxsize=None)
def expected_reads(case, max_fill):
    name, table, min_seed, max_occ, G, B, S, max_sec = READ_CASES[case]
    return F.map_long_aln(K.text_of(name).tobytes(), C.starts_of(name, table), reads_of(case), min_seed, max_occ, G, B, S, max_sec, max_fill, _memo)


@functools.lru_cache(maxsize=None)
def read_alignments(case, max_fill):
    """per read [(strand, chain, script)] of the returned chains, as fill_reference.read_alignments gives them"""
    name, table, min_seed, max_occ, G, B, S, max_sec = READ_CASES[case]
    tb, starts = K.text_of(name).tobytes(), C.starts_of(name, table)
    return [F.read_alignments(tb, starts, bytes(r), min_seed, max_occ, G, B, S, max_sec, max_fill, _memo)[0] for r in reads_of(case)]
