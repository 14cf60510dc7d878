"""CPU: tests/phrase_reference.py against the oracle, so that the GPU tests of the phrase stage and of the parse's BWT compare with
a reference that is not trusted on its own; and the inputs of tests/phrase_cases.py against what they claim to be - a planted text
is cut at its planted windows and nowhere else, which is what gives its phrases their lengths."""
import os
import re

import numpy as np
import pytest

import phrase_cases as PC
import phrase_reference as PR
import scan_reference as R
from textgen import make_text

PHRASE_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "big-bwt_amd", "csrc", "phrase.hip")


def same_stage1(got, want):
    for k in ("dict", "occ", "parse", "last", "sai"):
        assert np.array_equal(got[k], want[k]), k
    assert got["n_used"] == want["n_used"]


def same_stage2(O, c):
    want = O.bwtparse(c["parse"], c["last"], c["sai"], c["occ"])
    got = PR.stage2(c["parse"], c["last"], c["sai"], c["occ"])
    assert np.array_equal(got["ilist"], want[0]) and np.array_equal(got["bwlast"], want[1]) and np.array_equal(got["bwsai"], want[2])
    none = PR.stage2(c["parse"], c["last"], None, c["occ"])
    assert none["bwsai"] is None and np.array_equal(none["ilist"], want[0]) and np.array_equal(none["bwlast"], want[1])
    return got


def test_both_stages_on_the_golden_texts(golden, O):
    """stage1 and stage2 = the oracle's on every golden text of at most 100 KB, cut by the oracle's scan"""
    seen = 0
    for c in golden:
        if c["n"] > 100000:
            continue
        text = make_text(c["spec"], O)
        want = O.parse(text, c["w"], c["p"])
        got = PR.stage1(text, O.scan(text, c["w"], c["p"]), c["w"])
        same_stage1(got, want)
        if len(got["parse"]) >= 2:
            same_stage2(O, got)
        seen += 1
    assert seen >= 5


@pytest.mark.parametrize("name", PC.PARSE_CASES)
def test_planted_texts_are_cut_where_planted(O, name):
    """the Karp-Rabin cuts of a planted text under p = 2^31 are exactly its planted ends (a filler that holds a window of hash 0 by
    chance fails here: change the seed), so its phrases have the lengths the case was built for; and both stages = the oracle's"""
    c = PC.case(name)
    text, w = c["text"], c["w"]
    assert 50000 <= len(text) <= 150000 and text.min() >= 3
    assert np.array_equal(R.kr_cuts(text, w, PC.P_EXACT), c["ends"])
    words, _, _ = PR.phrases(text, c["ends"], w)
    assert [len(x) for x in words] == c["lengths"]
    got = PR.stage1(text, c["ends"], w)
    same_stage1(got, O.parse(text, w, PC.P_EXACT))
    if len(got["parse"]) >= 2:
        same_stage2(O, got)


def test_sibling_text_is_cut_where_planted():
    text, ends = PC.sibling_text()
    w = PC.case("lanes8")["w"]
    assert np.array_equal(R.kr_cuts(text, w, PC.P_EXACT), ends)
    mine, theirs = set(PR.phrases(text, ends, w)[0]), set(PR.phrases(PC.case("lanes8")["text"], PC.case("lanes8")["ends"], w)[0])
    assert len(mine & theirs) > 100 and len(mine - theirs) > 100


def test_cases_reach_the_paths_they_name():
    """what tests/README.md says of each case, as assertions on the cases' lengths and contents"""
    for name in ("lanes8", "w5", "w7", "long"):
        assert PC.mean_phrase_bytes(PC.case(name)) > PC.LANES4_MEAN_MAX, name
    assert PC.mean_phrase_bytes(PC.case("lanes4")) <= PC.LANES4_MEAN_MAX
    for name in ("lanes8", "lanes4", "w5", "w7"):
        c = PC.case(name)
        short = [a for a in c["lengths"] if a <= PC.LONG_PHRASE]
        assert {a % 16 for a in short} == set(range(16)), name          # every partial last piece, with and without a second chunk
        assert set(PC.CLASS_LENGTHS) <= set(short) and (name == "lanes4" or c["lengths"][0] == c["w"] + 1)
        words = PR.phrases(c["text"], c["ends"], c["w"])[0]
        counts = sorted(words.count(x) for x in set(words))
        assert counts[-1] == 50 and 7 in counts and 3 in counts and counts.count(2) >= len(PC.CLASS_LENGTHS)
        # near-equal pairs: two phrases of one length that differ in exactly one byte, at every offset of the list
        offs = set()
        by_len = {}
        for x in set(words):
            by_len.setdefault(len(x), []).append(x)
        for length in (200, 203):
            group = by_len[length]
            for i, a in enumerate(group):
                for b in group[i + 1:]:
                    d = [q for q in range(length) if a[q] != b[q]]
                    if len(d) == 1:
                        offs.add(d[0] if d[0] != length - c["w"] - 1 else "last")
        assert offs == set(PC.EDGE_OFFSETS) | {"last"}, (name, offs)
    assert sorted(a for a in PC.case("lanes4")["lengths"] if a > PC.LONG_PHRASE) == [PC.LONG_PHRASE + 1, PC.LONG_PHRASE + 8, PC.LONG_PHRASE + 16]
    assert {191, 192, 193} <= set(PC.case("lanes4")["lengths"])
    c = PC.case("long")
    L = PC.LONG_PHRASE
    assert {L - 1, L, L + 1, L + 16, 20000, 3 * L + 5} <= set(c["lengths"])
    assert c["lengths"][0] > L and c["lengths"][-1] > L and sum(a > L for a in c["lengths"]) >= 10
    words = PR.phrases(c["text"], c["ends"], c["w"])[0]
    assert sum(len(x) == L + 1 for x in words) == 2 and sum(len(x) == L + 1 for x in set(words)) == 1          # two equal long phrases
    N = PC.LONG_NEAR_EQUAL
    group = [np.frombuffer(x, dtype=np.uint8) for x in set(words) if len(x) == N]
    diffs = [np.flatnonzero(a != b) for i, a in enumerate(group) for b in group[i + 1:]]
    assert sorted({int(d[0]) for d in diffs if len(d) == 1}) == [L - 1, L, N - c["w"] - 1]
    assert N - c["w"] - 1 >= N // 16 * 16, "the last difference lies in the partial last piece: a hash that drops it calls the two equal"
    assert len(PC.case("one_phrase")["ends"]) == 0 and len(PC.case("two_phrases")["ends"]) == 1


def test_constants_restate_the_source():
    """phrase_cases.py places its lengths around two constants of csrc/phrase.hip: a retune has to move the cases with it"""
    src = open(PHRASE_HIP).read()
    m = re.search(r"constexpr\s+uint32_t\s+kLongPhrase\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == PC.LONG_PHRASE, "kLongPhrase changed: move LONG_PHRASE of tests/phrase_cases.py (and its cases) with it"
    m = re.search(r"lanes_log2_for\([^)]*\)\s*\{\s*return\s+phrases\s*&&\s*bytes\s*/\s*phrases\s*<=\s*(\d+)\s*\?\s*2\s*:\s*3\s*;", src)
    assert m and int(m.group(1)) == PC.LANES4_MEAN_MAX, "lanes_log2_for changed: move LANES4_MEAN_MAX of tests/phrase_cases.py with it"


def test_device_order_by_hand():
    words = [b"b", b"a", b"b", b"c", b"a", b"d", b"e", b"c", b"b", b"f"]
    pid, ordered, total = PR.device_order(words)
    assert ordered == [b"b", b"a", b"c", b"d", b"e", b"f"]          # 3, 2, 2 (a before c: first seen earlier), then the singles in order
    assert total.tolist() == [3, 2, 2, 1, 1, 1] and pid.tolist() == [0, 1, 0, 2, 1, 3, 4, 2, 0, 5]
    weights = [1, 1, 1, 5, 1, 7, 3, 2, 1, 3]
    pid, ordered, total = PR.device_order(words, weights)
    assert ordered == [b"c", b"d", b"b", b"e", b"f", b"a"]          # c 5 + 2 = d 7 (c first), b 3 = e 3 = f 3 (in order), a 2
    assert total.tolist() == [7, 7, 3, 3, 3, 2] and pid.tolist() == [2, 5, 2, 0, 5, 1, 3, 0, 2, 4]
    assert PR.split_blob(PR.words_blob(ordered)) == ordered


def test_owner_words_hold_what_they_promise():
    words, weights = PC.owner_words()
    assert len(words) == 3000 == len(weights) and weights.min() >= 1 and weights.max() <= 1000
    assert set(PC.OWNER_WORD_CLASSES) <= {len(x) for x in words} and all(1 not in x and 0 not in x for x in words)
    _, ordered, total = PR.device_order(words, weights)
    assert len(ordered) < len(words) - 20
    tied = [x for x, t in zip(ordered, total) if t == 1000]
    assert len(tied) >= 5 and any(words.count(x) == 2 for x in tied)


def test_verify_lists_differ_only_where_they_say():
    for name, size, lo, hi in (("stripe8", 300, 128, 256), ("stripe4", 70, 64, 70)):
        words = [np.frombuffer(x, dtype=np.uint8) for x in PC.verify_words(name)]
        assert len({x.tobytes() for x in words}) == 200 and all(len(x) == size for x in words)
        assert all(np.array_equal(x[:lo], words[0][:lo]) and np.array_equal(x[hi:], words[0][hi:]) for x in words)
        assert (size + 1 <= PC.LANES4_MEAN_MAX) == (name == "stripe4")          # with the terminator: what the dedup divides
    words = PC.verify_words("prefixes")
    assert len(set(words)) == 200 and all(a.startswith(b) and len(a) == len(b) + 1 for a, b in zip(words, words[1:]))


@pytest.mark.parametrize("name", PC.PARSE_BWT_CASES)
def test_stage2_on_the_synthetic_parses(O, name):
    c = PC.parse_case(name)
    P = len(c["parse"])
    assert 2 <= P <= 5000
    got = same_stage2(O, c)
    assert got["ilist"][0] == 1 and got["sa"][0] == P
    if name[0] == "d":
        d = int(name[1:])
        assert len(c["occ"]) == d and got["bwtp"][0] == d and d in got["bwtp"][P - 2:]
    if name == "stable":
        assert c["occ"][1] == 2000
    if name == "big_sai":
        assert set(PC.BIG_SAI) <= set(got["bwsai"].tolist()) and got["bwsai"][0] == PC.BIG_SAI[1]
    if name in ("P2", "P3"):
        assert (got["bwlast"] == 255).sum() == 1 and got["bwlast"][list(got["sa"]).index(1)] == 255


def test_one_word_is_not_a_parse(O):
    """[1] * 1000: the row of SA[j] = 0 is the last one, so ilist[0] = 1000, and the reference's assertion (bwtparse.c:305) ends
    the run; the oracle refuses likewise"""
    c = PC.parse_case("one_word")
    got = PR.stage2(c["parse"], c["last"], c["sai"], c["occ"])
    assert got["ilist"][0] == 1000 and got["sa"].tolist() == list(range(1000, -1, -1))
    with pytest.raises(RuntimeError):
        O.bwtparse(c["parse"], c["last"], c["sai"], c["occ"])
