"""The reference of the chain-alignment tests, checked on the CPU (fill_reference.py; definitions: include/pfpgpu.h, "Aligning
chains"): the worked examples as literals, a replay of every script against the two strings, equality with cigar_reference.py
where both apply, and conditions on the cases themselves - so that a change of the cases cannot hollow out the GPU tests
(test_fm_fill.py) without a failure here."""
import numpy as np
import pytest

import chain_reference as R
import cigar_reference as CR
import fill_cases as FC
import fill_reference as F
import map_cases as K
from map_reference import revcomp


def runs_of(res, off_at, cig_at, k):
    return [int(x) for x in res[cig_at][int(res[off_at][k]):int(res[off_at][k + 1])]]


def test_worked_gaps():
    """the tie rule on strings with many optimal scripts, and the edges of layer 1"""
    d, off, cig = FC.expected_segments("ties")
    got = [(int(d[k]), CR.cigar_string(cig[int(off[k]):int(off[k + 1])])) for k in range(len(d))]
    assert got == [(1, "1I3="), (2, "1=1I3=1X"), (1, "1D3="), (3, "1I1=2X"), (10, "1D1=1X1=1X1=1X1=1X3=1I1=1X1=1X1=1X1=1X"), (1, "1=1D1=")]
    assert F.gap_script(b"", b"", 0) == (0, [])
    assert F.gap_script(b"", b"ACG", 3) == (3, [3 << 4 | CR.OP_D]) and F.gap_script(b"", b"ACG", 2) == (F.NONE, [])
    assert F.gap_script(b"AC", b"", 5) == (2, [2 << 4 | CR.OP_I])
    assert F.gap_script(b"A", b"A", 0) == (0, [16 | CR.OP_EQ]) and F.gap_script(b"A", b"C", 0) == (F.NONE, [])
    assert F.gap_script(b"\x00", b"\x00", 1) == (1, [16 | CR.OP_X])        # a pattern byte 0 equals nothing


def test_worked_chains():
    res = FC.expected_anchor_set("first member is not the least", 500)
    by = dict(zip(F.CHAIN_ALN_NAMES, res))
    # the pair that would differ does not chain; the chain the peel cuts off at a visited anchor does differ
    assert by["chain_off"].tolist() == [0, 2, 4] and by["n"].tolist() == [1, 1, 3, 2]
    assert by["qs"].tolist() == [5, 0, 0, 55] and by["aqs"].tolist() == [5, 0, 0, 60]
    assert by["ts"].tolist() == [930, 1000, 1000, 1066] and by["ats"].tolist() == [930, 1000, 1000, 1070]
    assert by["mem_off"].tolist() == [0, 1, 2, 5, 7] and by["mem"].tolist() == [1, 0, 0, 1, 4, 2, 3]
    assert CR.cigar_string(runs_of(res, 12, 13, 3)) == "20=1D15=" and int(by["nm"][3]) == 1
    assert F.trimmed([(60, 20, 1070), (55, 40, 1066)], [0, 1]) == ([(60, 20, 1070), (80, 15, 1091)], [0, 25])
    res = FC.expected_anchor_set("true anchors", 500)
    assert CR.cigar_string(res[13]) == "30=1X29=2I40=3D47=" and [int(res[k][0]) for k in (8, 9, 10, 11)] == [0, 1000, 6, 0]
    res = FC.expected_anchor_set("overlaps", 500)
    assert [CR.cigar_string(runs_of(res, 12, 13, k)) for k in range(4)] == ["30=10D35=", "30=15I35=", "30=2D35=", "70="]
    assert res[11].tolist() == [0, 0, 0, 0] and FC.expected_anchor_set("overlaps", 4)[11].tolist() == [1, 1, 0, 0]
    res = FC.expected_anchor_set("overlaps", 4)
    assert [CR.cigar_string(runs_of(res, 12, 13, k)) for k in range(2)] == ["30=10D35=", "30=15I35="]      # unfilled: a I then b D
    res = FC.expected_anchor_set("unfilled", 4)
    assert res[11].tolist() == [1, 1, 1] and CR.cigar_string(runs_of(res, 12, 13, 0)) == "30=30I20D30="
    assert FC.expected_anchor_set("unfilled", 500)[11].tolist() == [0, 0, 1]
    assert FC.expected_anchor_set("shared parent", 500)[0].tolist() == [0, 2]


def test_segment_cases_are_what_they_say():
    for name, (text, max_fill, pats, segs, want) in FC.segment_sets().items():
        d, off, cig = FC.expected_segments(name)
        assert d.dtype == np.uint32 and off.dtype == np.uint64 and cig.dtype == np.uint32 and len(off) == len(segs) + 1
        assert {k: int(d[k]) for k in want} == want, name
        tb = K.text_of(text).tobytes()
        for k, (p, q0, q1, t0, t1) in enumerate(segs):
            runs = cig[int(off[k]):int(off[k + 1])]
            if int(d[k]) == F.NONE:
                assert len(runs) == 0
            else:
                assert int(d[k]) <= max_fill
                CR.validate(pats[p][q0:q1], tb[t0:t1], runs, int(d[k]))
    kinds = {int(d) == F.NONE for d in FC.expected_segments("invalid")[0]}
    assert kinds == {True, False}


def test_equal_to_the_edit_scripts_where_both_apply():
    text = K.text_of("dna")
    pats, spans = FC.whole_patterns()
    dists = []
    for p, (s, e) in zip(pats, spans):
        d, runs = CR.script(text, p, s, e, 32)
        assert d != CR.NONE
        assert F.segment(text, [p], 0, 0, len(p), s, e, 32) == (d, runs)
        assert F.segment(text, [p], 0, 0, len(p), s, e, 500) == (d, runs)
        dists.append(d)
    assert max(dists) == 32 and min(dists) == 0


@pytest.mark.parametrize("case", sorted(FC.READ_CASES))
def test_scripts_replay(case):
    """every script consumes exactly P[aqs..qe) and T[ats..te) of its strand, '=' runs match, X runs differ, nm adds up, no two
    neighbouring runs share an operation; the arrays say the same, with aqs turned"""
    name = FC.READ_CASES[case][0]
    tb = K.text_of(name).tobytes()
    reads = FC.reads_of(case)
    for max_fill in FC.READ_FILLS:
        res = FC.expected_reads(case, max_fill)
        per = FC.read_alignments(case, max_fill)
        h = 0
        for read, kept in zip(reads, per):
            for strand, c, s in kept:
                pat = revcomp(read) if strand else bytes(read)
                F.validate_chain(pat, tb, s["aqs"], c["qe"], s["ats"], c["te"], s["runs"], s["nm"])
                assert s["nm"] == sum(a + b if d == F.NONE else d for a, b, d, _ in s["gaps"])
                assert s["unfilled"] == sum(d == F.NONE for a, b, d, _ in s["gaps"])
                assert s["aqs"] >= c["qs"] and s["ats"] >= c["ts"]
                assert runs_of(res, 17, 18, h) == s["runs"] and int(res[15][h]) == s["nm"] and int(res[16][h]) == s["unfilled"]
                m = len(read)
                if strand:
                    assert int(res[13][h]) == m - s["aqs"] and int(res[8][h]) == m - c["qe"]       # the script covers [qs, aqs)
                else:
                    assert int(res[13][h]) == s["aqs"] and int(res[9][h]) == c["qe"]               # the script covers [aqs, qe)
                h += 1
        assert h == len(res[3])


def test_the_first_arrays_are_map_longs():
    case = "copies"
    name, table, min_seed, max_occ, G, B, S, max_sec = FC.READ_CASES[case]
    want = R.map_long(K.text_of(name).tobytes(), FC.C.starts_of(name, table), FC.reads_of(case), min_seed, max_occ, G, B, S, max_sec)
    got = FC.expected_reads(case, 500)[:13]
    assert all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))
    assert F.LONG_ALN_NAMES[:13] == R.NAMES and F.CHAIN_ALN_NAMES[:8] == R.CHAIN_NAMES


def test_the_read_cases_are_not_vacuous():
    kinds = set()
    for case in FC.READ_CASES:
        for kept in FC.read_alignments(case, 500):
            for strand, c, s in kept:
                for a, b, d, o in s["gaps"]:
                    trivial = (a == 0) != (b == 0) or (a == 1 and b == 1)
                    kinds |= {"trimmed anchor"} if o else set()
                    kinds |= {"trivial gap"} if trivial else set()
                    if (a or b) and not trivial and d != F.NONE:
                        kinds.add("band-filled gap")
                        kinds |= {"D > 32"} if d > 32 else set()
                        kinds |= {"wide gap"} if abs(a - b) + 2 * 8 + 1 > 64 or d > 17 else set()      # more than 64 cells: a wave's band
        for kept in FC.read_alignments(case, 4):
            kinds |= {"unfilled at F = 4"} if any(s["unfilled"] for _, _, s in kept) else set()
    want = {"trimmed anchor", "trivial gap", "band-filled gap", "D > 32", "wide gap", "unfilled at F = 4"}
    assert want <= kinds, want - kinds
    assert not FC.expected_reads("dna", 500)[16].any()                  # every returned chain of "dna" is filled at the default F
    assert FC.expected_reads("dna", 4)[16].any()


def test_paf_lines():
    case = "dna noisy"
    name, table, min_seed, max_occ, G, B, S, max_sec = FC.READ_CASES[case]
    reads = FC.reads_of(case)
    res = FC.expected_reads(case, 500)
    starts = K.starts_of(name, table)
    names = [b"r%d" % k for k in range(len(starts) - 1)]
    lines = F.paf_lines([x.decode() for x in names], starts, 20000, "t", ["q%d" % k for k in range(len(reads))], reads, res, 0)
    assert len(lines) == sum(1 for p in range(len(reads)) if res[0][p + 1] > res[0][p])
    for line in lines:
        f = line.split("\t")
        cg = [t for t in f[12:] if t.startswith("cg:Z:")][0][5:]
        import re
        ops = [(int(n), o) for n, o in re.findall(r"(\d+)([=XID])", cg)]
        assert int(f[3]) - int(f[2]) == sum(n for n, o in ops if o in "=XI") and int(f[8]) - int(f[7]) == sum(n for n, o in ops if o in "=XD")
        assert int(f[9]) == sum(n for n, o in ops if o == "=") and int(f[10]) == sum(n for n, o in ops)
        assert ("NM:i:%d" % sum(n for n, o in ops if o != "=")) in f
