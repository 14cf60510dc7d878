"""GPU: stage 2 (csrc/parsebwt.hip: the BWT of the parse, the cyclic predecessor's last byte, the sai of the phrase in front and
the inverted lists) through Context.bwtparse against the plain restatement of tests/phrase_reference.py, which
test_phrase_reference.py checks against the oracle.  The integer sorter's own paths are pinned by sorter_cases.py; the parses here
(tests/phrase_cases.py: parse_case) pin what parsebwt.hip adds to it.  Every comparison is exact.  tests/README.md, "Tests of the
phrase stage and the parse's BWT, path by path", lists the cases."""
import functools

import numpy as np
import pytest

import phrase_cases as PC
import phrase_reference as PR

pytestmark = pytest.mark.gpu

ESHORT, EFORMAT = -8, -6


@functools.lru_cache(maxsize=None)
def wanted(name):
    c = PC.parse_case(name)
    return PR.stage2(c["parse"], c["last"], c["sai"], c["occ"])


@pytest.mark.parametrize("with_sai", [True, False], ids=["sai", "no_sai"])
@pytest.mark.parametrize("name", PC.PARSE_BWT_CASES)
def test_bwt_of_the_parse(pkg, wctx, name, with_sai):
    """ilist, bwlast and - 5 bytes a value, packed and unpacked here - bwsai of every synthetic parse = the reference's"""
    c, want = PC.parse_case(name), wanted(name)
    ilist, bwlast, bwsai = wctx.bwtparse(c["parse"], c["last"], c["occ"], sai=pkg.pack5(c["sai"]) if with_sai else None)
    assert np.array_equal(bwlast, want["bwlast"]), "bwlast: the last byte of the phrase before the one in front of the suffix"
    assert np.array_equal(ilist, want["ilist"]), "ilist: rows grouped by symbol, ascending inside a group"
    if with_sai:
        assert np.array_equal(pkg.unpack5(bwsai), want["bwsai"]), "bwsai"
    else:
        assert bwsai is None


def test_a_parse_of_one_phrase_is_too_short(pkg, wctx):
    with pytest.raises(pkg.PfpError) as ei:
        wctx.bwtparse(np.array([1], dtype=np.uint32), np.array([65], dtype=np.uint8), np.array([1], dtype=np.uint32),
                      sai=pkg.pack5(np.array([9], dtype=np.uint64)))
    assert ei.value.code == ESHORT


def test_one_word_only_is_refused_like_the_reference_does(pkg, wctx):
    """parse = [1] * 1000 is sorted (one symbol, the width bits_for(1)) but is no parse of a text: its first symbol is not the only
    smallest one, the row of SA[j] = 0 comes last, and ilist[0] = 1000 where bwtparse.c:305 asserts 1.  The library answers
    PFP_EFORMAT, as test_phrase_reference.py shows the oracle to refuse; the next call is exact."""
    c = PC.parse_case("one_word")
    for sai in (pkg.pack5(c["sai"]), None):
        with pytest.raises(pkg.PfpError) as ei:
            wctx.bwtparse(c["parse"], c["last"], c["occ"], sai=sai)
        assert ei.value.code == EFORMAT and "ilist[0]" in str(ei.value)
    c, want = PC.parse_case("P3"), wanted("P3")
    ilist, bwlast, _ = wctx.bwtparse(c["parse"], c["last"], c["occ"])
    assert np.array_equal(ilist, want["ilist"]) and np.array_equal(bwlast, want["bwlast"])
