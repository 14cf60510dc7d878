"""The reference of test_fm_pairs.py (pair_reference.py) against literals worked by hand from the definitions of pfpgpu.h, "Mapping
read pairs": hit lists and rescue results are written out, so nothing here needs a text or the GPU.  Table: two records,
[0, 1000) and [1000, 2000); min_ins = 100, max_ins = 500."""
import numpy as np
import pytest

import pair_reference as P

STARTS = [0, 1000, 2000]
NOPOS = 2**64 - 1
UNMAPPED = (0, 0, 0, 0, 0, NOPOS, NOPOS, 0xFF, 0)


def run(h1, h2, rescues=None, C=8, singles=((60, 1), (60, 1))):
    """rescues: {(mate, strand, lo, hi): (d, s, e)}; a window that is not listed must not be asked for"""
    rescues = rescues or {}
    asked = []

    def rescue(mate, strand, lo, hi):
        asked.append((mate, strand, lo, hi))
        return rescues[(mate, strand, lo, hi)]
    s1 = singles[0] if h1 else (0, 0)
    s2 = singles[1] if h2 else (0, 0)
    out = P.pair(STARTS, h1, h2, s1, s2, rescue, 100, 500, C)
    assert sorted(asked) == sorted(rescues), (asked, rescues)
    return out


def test_proper_by_anchors():
    assert run([(0, 0, 100, 150)], [(1, 1, 350, 400)]) == (1, 1, [(1, 0, 60, 1, 0, 100, 150, 0, 300), (1, 0, 60, 1, 1, 350, 400, 1, -300)])
    # mate 1 on the reverse strand, to the right: TLEN is positive for the mate with the smaller start
    assert run([(0, 1, 350, 400)], [(2, 0, 100, 150)]) == (1, 1, [(1, 0, 60, 1, 1, 350, 400, 0, -300), (1, 0, 60, 1, 0, 100, 150, 2, 300)])


def test_proper_by_rescue_only():
    got = run([(0, 0, 100, 150)], [], {(1, 1, 100, 600): (3, 350, 398)})
    assert got == (1, 1, [(1, 0, 60, 1, 0, 100, 150, 0, 298), (1, 1, 60, 0, 1, 350, 398, 3, -298)])
    # the anchor is on the reverse strand: the window ends with it; here it starts at the record's start, 260 < max_ins
    got = run([], [(0, 1, 200, 260)], {(0, 0, 0, 260): (1, 20, 80)})
    assert got == (1, 1, [(1, 1, 60, 0, 0, 20, 80, 1, 240), (1, 0, 60, 1, 1, 200, 260, 0, -240)])
    # a rescue that gives an empty span, or a pair outside the bounds, is no pair
    assert run([(0, 0, 100, 150)], [], {(1, 1, 100, 600): (8, 100, 100)})[0] == 0
    assert run([(0, 0, 100, 150)], [], {(1, 1, 100, 600): (0, 120, 180)})[:2] == (0, 0)       # insert 80


def test_wrong_orientation():
    none = P.NONE
    got = run([(0, 0, 100, 150)], [(0, 0, 350, 400)], {(1, 1, 100, 600): none, (0, 1, 350, 850): none}, singles=((60, 1), (10, 2)))
    assert got == (0, 0, [(1, 0, 60, 1, 0, 100, 150, 0, 300), (1, 0, 10, 2, 0, 350, 400, 0, -300)])
    # facing outwards: the reverse mate lies to the left
    got = run([(0, 1, 100, 150)], [(0, 0, 350, 400)], {(1, 0, 0, 150): none, (0, 1, 350, 850): none})
    assert got[:2] == (0, 0) and [r[8] for r in got[2]] == [300, -300]


@pytest.mark.parametrize("e_r,proper", [(199, 0), (200, 1), (600, 1), (601, 0)])
def test_insert_bounds(e_r, proper):
    """e_r - s_f one below min_ins, at min_ins, at max_ins, one above max_ins"""
    rescues = {} if proper else {(1, 1, 100, 600): P.NONE, (0, 0, max(e_r - 500, 0), e_r): P.NONE}
    got = run([(0, 0, 100, 150)], [(0, 1, e_r - 50, e_r)], rescues)
    assert got[:2] == (proper, proper) and [r[8] for r in got[2]] == [e_r - 100, 100 - e_r]


def test_different_records_and_clipped_windows():
    """the anchors lie 50 bytes on either side of the boundary at 1000: the window of the first is clipped by its record's end, the
    window of the second by its record's start"""
    got = run([(0, 0, 900, 950)], [(0, 1, 1100, 1150)], {(1, 1, 900, 1000): P.NONE, (0, 0, 1000, 1150): P.NONE})
    assert got == (0, 0, [(1, 0, 60, 1, 0, 900, 950, 0, 0), (1, 0, 60, 1, 1, 1100, 1150, 0, 0)])


def test_pair_mapq():
    h1 = [(0, 0, 100, 150), (0, 0, 1100, 1150)]
    # two equal pairs: MAPQ 0; the primary is the one with the smaller key
    got = run(h1, [(0, 1, 350, 400), (0, 1, 1350, 1400)], singles=((0, 2), (0, 2)))
    assert got == (1, 2, [(1, 0, 0, 2, 0, 100, 150, 0, 300), (1, 0, 0, 2, 1, 350, 400, 0, -300)])
    # the second pair is one edit worse: MAPQ 10; two edits worse and a third pair: still by the nearest, 20
    got = run(h1, [(0, 1, 350, 400), (1, 1, 1350, 1400)], singles=((0, 2), (10, 2)))
    assert got[:2] == (1, 2) and [r[2] for r in got[2]] == [10, 10]
    got = run(h1 + [(7, 0, 500, 550)], [(0, 1, 350, 400), (2, 1, 1350, 1400), (0, 1, 700, 760)], singles=((0, 3), (0, 3)))
    assert got[:2] == (1, 3) and [r[2] for r in got[2]] == [20, 20]
    # the better pair wins although mate 1's own first hit is elsewhere
    got = run([(0, 0, 1100, 1150), (1, 0, 100, 150)], [(0, 1, 350, 400)], {(1, 1, 1100, 1600): P.NONE})
    assert got == (1, 1, [(1, 0, 60, 1, 0, 100, 150, 1, 300), (1, 0, 60, 1, 1, 350, 400, 0, -300)])
    # C = 1: only the first hit of each mate is an anchor
    got = run([(0, 0, 1100, 1150), (1, 0, 100, 150)], [(0, 1, 350, 400)], {(1, 1, 1100, 1600): P.NONE, (0, 0, 0, 400): P.NONE}, C=1)
    assert got[:2] == (0, 0) and [r[5] for r in got[2]] == [1100, 350] and [r[8] for r in got[2]] == [0, 0]


def test_a_pair_at_the_primarys_locus_does_not_count():
    """the anchors are 501 apart.  Each has its mate rescued one byte shorter, for one edit: two pairs of sum 1.  The smaller key
    (the anchor of mate 1, d = 0) is the primary; the other pair has the same strands and intersects it in both mates"""
    got = run([(0, 0, 100, 160)], [(0, 1, 541, 601)], {(1, 1, 100, 600): (1, 541, 600), (0, 0, 101, 601): (1, 101, 160)})
    assert got == (1, 1, [(1, 0, 60, 1, 0, 100, 160, 0, 500), (1, 1, 60, 1, 1, 541, 600, 1, -500)])


def test_unmapped_mates():
    got = run([(0, 0, 100, 150)], [], {(1, 1, 100, 600): P.NONE}, singles=((10, 3), None))
    assert got == (0, 0, [(1, 0, 10, 3, 0, 100, 150, 0, 0), UNMAPPED])
    assert run([], []) == (0, 0, [UNMAPPED, UNMAPPED])


def test_tlen_tie():
    """both mates start at 100: mate 1 takes the positive sign (insert 60: not proper)"""
    got = run([(0, 0, 100, 160)], [(0, 1, 100, 160)], {(1, 1, 100, 600): (0, 100, 160), (0, 0, 0, 160): P.NONE})
    assert got[:2] == (0, 0) and [r[8] for r in got[2]] == [60, -60]
    got = run([(0, 1, 100, 160)], [(0, 0, 100, 160)], {(1, 0, 0, 160): P.NONE, (0, 1, 100, 600): (0, 100, 160)})
    assert got[:2] == (0, 0) and [r[8] for r in got[2]] == [60, -60]


def test_sam_lines_paired():
    u8, u64 = (lambda *a: np.array(a, dtype=np.uint8)), (lambda *a: np.array(a, dtype=np.uint64))
    eq = lambda n: n << 4 | 7
    res = (u8(1, 0, 0), u64(2, 0, 0),                      # proper, npairs
           u8(1, 1, 1, 0, 0, 0), u8(0, 1, 0, 0, 0, 0), u8(10, 10, 60, 0, 0, 0), u64(1, 0, 3, 0, 0, 0), u8(0, 1, 1, 0, 0, 0),
           np.array([0, 0, 1, 2**32 - 1, 2**32 - 1, 2**32 - 1], dtype=np.uint32), u64(9, 19, 5, NOPOS, NOPOS, NOPOS), u64(9, 19, 1005, NOPOS, NOPOS, NOPOS),
           u8(0, 1, 0, 0xFF, 0xFF, 0xFF), np.array([14, -14, 0, 0, 0, 0], dtype=np.int64),
           u64(0, 1, 4, 5, 5, 5, 5), np.array([eq(4), eq(1), 1 << 4 | 8, eq(2), eq(4)], dtype=np.uint32), u64(0, 1, 4, 5, 5, 5, 5),
           np.frombuffer(b"4" + b"1C2" + b"4", dtype=np.uint8))
    reads = [b"ACGT", b"AAGT", b"TTTT", b"GG", b"", b"C"]
    names = [b"r1/1", b"r1/2", b"r2", b"other", b"r3/1", b"r3/1"]
    got = P.sam_lines_paired([b"chrA", b"chrB"], names, reads, res)
    want = (b"r1\t99\tchrA\t10\t10\t4=\t=\t20\t14\tACGT\t*\tNM:i:0\tMD:Z:4\tNH:i:2\n"
            b"r1\t147\tchrA\t20\t10\t1=1X2=\t=\t10\t-14\tACTT\t*\tNM:i:1\tMD:Z:1C2\tNH:i:2\tYR:i:1\n"
            b"r2\t89\tchrB\t6\t60\t4=\t*\t0\t0\tAAAA\t*\tNM:i:0\tMD:Z:4\tNH:i:3\n"
            b"r2\t165\tchrB\t6\t0\t*\t=\t6\t0\tGG\t*\n"
            b"r3/1\t77\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
            b"r3/1\t141\t*\t0\t0\t*\t*\t0\t0\tC\t*\n")
    assert got == want
