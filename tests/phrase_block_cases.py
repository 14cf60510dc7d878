"""Inputs of tests/test_phrase_text_order.py (GPU) and tests/test_phrase_blocks.py (CPU): texts with a chosen NUMBER of phrases
around the block sizes of csrc/phrase.hip, and word lists on which the verification against a word's dictionary copy alone stands
between a hash collision and a wrong dictionary.

phrase_hash_kernel and phrase_verify_kernel give a workgroup a contiguous block of phrases: it reads their ends[] once, takes a
phrase's start from its left neighbour's end, and its lane groups walk several phrases at a time.  What can go wrong there is the
block's edge: the first phrase of a block (its start comes from ends[] of the block before), the last block with fewer phrases
than a block holds, a lane group some of whose phrases are not there.  The two constants below restate the source;
test_phrase_blocks.py reads it and fails when they drift."""
import functools

import numpy as np

import phrase_cases as PC

HASH_BLOCK = 256          # kHashBlockPhrases: phrases per workgroup of phrase_hash_kernel
VERIFY_BLOCK = 256        # kVerifyBlockPhrases: phrases per workgroup of phrase_verify_kernel
W = 4


def block_counts():
    """numbers of phrases around the blocks of both kernels"""
    out = []
    for G in sorted({HASH_BLOCK, VERIFY_BLOCK}):
        out += [1, 2, 3, G - 1, G, G + 1, 2 * G, 2 * G + 1]
    return sorted(set(out))


LANE_RANGES = {4: (20, 70, 30), 8: (100, 160, 120)}      # lanes per phrase -> shortest, longest phrase, bytes of the tail


@functools.lru_cache(maxsize=None)
def block_text(P, lanes):
    """-> (text, ends) of exactly P phrases, w = 4.  The lengths cycle through 20 .. 70 (4 lanes per phrase, every residue mod 16)
    or 100 .. 160 (8 lanes); every third phrase is a copy of an earlier one (never of phrase 0, which begins with the Dollar), so
    equal phrases lie in different blocks and different lane groups; the last phrase is Z . tail . Dollar^w"""
    lo, hi, tail = LANE_RANGES[lanes]
    rng = np.random.default_rng(1000 * lanes + P)
    lengths, fillers = [], []
    for k in range(P - 1):
        if k % 3 == 2 and k >= 3:
            src = 1 + (7 * k) % (k - 1)
            lengths.append(lengths[src])
            fillers.append(fillers[src])
        else:
            length = lo + (k - k // 3) % (hi - lo + 1)      # (counts the phrases that are no copies: every length comes up)
            lengths.append(length)
            fillers.append(PC.random_filler(rng, PC.filler_len(k, length, W)))
    return PC.planted_text(lengths, fillers, W, PC.random_filler(rng, tail))


def mean_bytes(text, P):
    """what lanes_log2_for divides (phrase_cases.mean_phrase_bytes)"""
    return (len(text) + W * P) // P


# ---------------------------------------------------------------- word lists: a phrase against its word's representative

BASE_SIZES = {4: 70, 8: 300}      # lanes per word -> bytes of the base word (the list's mean decides the lanes)


def _family(lanes):
    """base word, its one-byte variants, its two prefixes and its two extensions"""
    size = BASE_SIZES[lanes]
    rng = np.random.default_rng(1100 + lanes)
    base = PC.random_filler(rng, size)
    offsets = sorted({0, size - 1} | {o for o in PC.EDGE_OFFSETS if o < size})
    variants = [PC.one_byte_variant(base, o).tobytes() for o in offsets]
    ext = PC.random_filler(rng, 16).tobytes()
    base = base.tobytes()
    return base, variants, [base[:-16], base[:-1]], [base + ext[:1], base + ext]


@functools.lru_cache(maxsize=None)
def representative_words(lanes):
    """150 copies of W and, twice each, W with one byte changed (offset 0, the EDGE_OFFSETS inside W, the last byte), W[:-1],
    W[:-16], W + one byte, W + 16 bytes; shuffled.  With one or two hash bits most of them share W's class on the first attempt:
    a compare that misses an offset, a partial last piece or the length keeps a dictionary of two or four words."""
    base, variants, shorter, longer = _family(lanes)
    words = [base] * 150 + 2 * (variants + shorter + longer)
    order = np.random.default_rng(1200 + lanes).permutation(len(words))
    return [words[i] for i in order]


@functools.lru_cache(maxsize=None)
def prefix_words(lanes, shorter_first):
    """W[:-16], W[:-1], W, W + one byte, W + 16 bytes, the whole sequence twice, shortest first or longest first: whichever word
    of a class comes first is its representative, so the length rule is tried with the representative the shorter one and with
    the representative the longer one (whose bytes behind the phrase's length are the next word's in one direction, and the
    phrase's own in the other)"""
    base, _, shorter, longer = _family(lanes)
    seq = shorter + [base] + longer
    if not shorter_first:
        seq = seq[::-1]
    return seq + seq
