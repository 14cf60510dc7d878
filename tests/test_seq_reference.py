"""The CPU reference of the sequence-aware searches (tests/seq_reference.py) on cases small enough to check by eye."""
import numpy as np

import seq_reference as R


def test_spanning_occurrence_is_dropped():
    # ACGT|ACGT: "TA" occurs once, at 3, and T is the last byte of sequence 0
    text, starts = b"ACGTACGT", [0, 4, 8]
    occ = R.occurrences_find(text, b"TA")
    assert occ.tolist() == [3]
    assert R.keep(starts, occ, 2).tolist() == [False]
    seq, off = R.locate_seqs(starts, occ, 2)
    assert len(seq) == 0 and len(off) == 0
    docs, cnt = R.doclist(starts, occ, 2)
    assert len(docs) == 0 and len(cnt) == 0
    # "ACG" occurs at 0 and 4, once in each sequence, at offset 0
    occ = R.occurrences_find(text, b"ACG")
    assert occ.tolist() == [0, 4]
    seq, off = R.locate_seqs(starts, occ, 3)
    assert seq.tolist() == [0, 1] and off.tolist() == [0, 0]
    docs, cnt = R.doclist(starts, occ, 3)
    assert docs.tolist() == [0, 1] and cnt.tolist() == [1, 1]
    # "GTAC" spans; "CGT" ends exactly at the border and at the end of the text: both kept
    assert R.keep(starts, [2], 4).tolist() == [False]
    assert R.keep(starts, [1, 5], 3).tolist() == [True, True]
    # row order is kept, and max_occ cuts the rows before the filter
    seq, off = R.locate_seqs(starts, [4, 3, 0], 1, max_occ=2)
    assert seq.tolist() == [1, 0] and off.tolist() == [0, 3]


def test_empty_sequences_are_never_an_answer():
    # sequences: 0 = [], 1 = [], 2 = [0, 3), 3 = [], 4 = [3, 5), 5 = [], 6 = []
    starts = [0, 0, 0, 3, 3, 5, 5, 5]
    seq, off = R.seqmap(starts, [0, 1, 2, 3, 4, 5, 6, 2**64 - 1])
    assert seq.tolist() == [2, 2, 2, 4, 4, R.NOSEQ, R.NOSEQ, R.NOSEQ]
    assert off.tolist() == [0, 1, 2, 0, 1, R.NOOFF, R.NOOFF, R.NOOFF]
    assert R.keep(starts, [0, 2, 2, 3, 4, 5], 1).tolist() == [True, True, True, True, True, False]
    assert R.keep(starts, [2, 3, 4], 2).tolist() == [False, True, False]
    docs, cnt = R.doclist(starts, [4, 0, 3, 1], 1)
    assert docs.tolist() == [2, 4] and cnt.tolist() == [2, 2]


def test_empty_pattern_keeps_every_position_below_n():
    text, starts = b"ACGTACGT", [0, 4, 8]
    occ = R.occurrences_find(text, b"")
    assert occ.tolist() == list(range(9))            # 0..n
    assert R.keep(starts, occ, 0).tolist() == [True] * 8 + [False]
    docs, cnt = R.doclist(starts, occ, 0)
    assert docs.tolist() == [0, 1] and cnt.tolist() == [4, 4]


def test_reverse_complement():
    assert R.reverse_complement(b"AACGTn") == b"nACGTT"
    assert R.reverse_complement(b"acgtX") == b"Xacgt"
    assert R.reverse_complement(b"") == b""


def test_fasta_table_helper():
    names, lens = R.parse_fasta_table(b">a x\nACG\nT\n>b:1\r\nAC\r\n>e\n>f\nA")
    assert names == [b"a", b"b:1", b"e", b"f"] and lens == [4, 2, 0, 1]
    assert np.cumsum([0] + lens).tolist() == [0, 4, 6, 6, 7]
