"""CPU: the inputs of tests/test_phrase_text_order.py are what they claim to be - the block sizes they are placed around are
those of csrc/phrase.hip, the texts are cut at their planted windows alone and have the lane layout they name, and so have the
word lists."""
import os
import re

import numpy as np
import pytest

import phrase_block_cases as BC
import phrase_cases as PC
import phrase_reference as PR
import scan_reference as R

PHRASE_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "big-bwt_amd", "csrc", "phrase.hip")


def test_block_sizes_restate_the_source():
    """phrase_block_cases.py places its phrase counts around two constants of csrc/phrase.hip: a retune has to move them with it"""
    src = open(PHRASE_HIP).read()
    m = re.search(r"constexpr\s+uint32_t\s+kHashBlockPhrases\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == BC.HASH_BLOCK, "kHashBlockPhrases changed: move HASH_BLOCK of tests/phrase_block_cases.py with it"
    m = re.search(r"constexpr\s+uint32_t\s+kVerifyBlockPhrases\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == BC.VERIFY_BLOCK, "kVerifyBlockPhrases changed: move VERIFY_BLOCK of tests/phrase_block_cases.py with it"
    for G in (BC.HASH_BLOCK, BC.VERIFY_BLOCK):
        assert {1, 2, 3, G - 1, G, G + 1, 2 * G, 2 * G + 1} <= set(BC.block_counts())


@pytest.mark.parametrize("lanes", [4, 8])
def test_block_texts_are_cut_where_planted(lanes):
    """P phrases exactly, none of them long, the lane layout the text is named for, and copies among them"""
    lo, hi, _ = BC.LANE_RANGES[lanes]
    for P in BC.block_counts():
        text, ends = BC.block_text(P, lanes)
        assert len(ends) == P - 1 and np.array_equal(R.kr_cuts(text, BC.W, PC.P_EXACT), ends), P
        assert (BC.mean_bytes(text, P) <= PC.LANES4_MEAN_MAX) == (lanes == 4), P
        words, _, _ = PR.phrases(text, ends, BC.W)
        assert len(words) == P and max(len(x) for x in words) <= PC.LONG_PHRASE
        if P > 200:
            assert {len(x) for x in words[1:-1]} == set(range(lo, hi + 1)), "every length of the cycle"
            assert P - P // 3 <= len(set(words)) < P, "every third phrase a copy"


@pytest.mark.parametrize("lanes", [4, 8])
def test_word_lists_have_their_lanes_and_their_variants(lanes):
    size = BC.BASE_SIZES[lanes]
    lists = [BC.representative_words(lanes), BC.prefix_words(lanes, True), BC.prefix_words(lanes, False)]
    for words in lists:
        mean = sum(len(x) + 1 for x in words) // len(words)
        assert (mean <= PC.LANES4_MEAN_MAX) == (lanes == 4)
        assert all(min(x) >= 3 for x in words)
    words = lists[0]
    base = max(set(words), key=words.count)
    assert words.count(base) == 150 and len(base) == size
    offs = {next(i for i in range(size) if x[i] != base[i]) for x in set(words) if len(x) == size and x != base}
    assert offs == {0, size - 1} | {o for o in PC.EDGE_OFFSETS if o < size}
    assert {len(x) for x in words} == {size - 16, size - 1, size, size + 1, size + 16}
    assert all(x == base[:len(x)] for x in words if len(x) < size) and all(x[:size] == base for x in words if len(x) > size)
    up, down = lists[1], lists[2]
    assert [len(x) for x in up[:5]] == sorted(len(x) for x in up[:5]) and down[:5] == up[:5][::-1] and len(set(up)) == 5
