"""Inputs of tests/test_phrase_stage.py and tests/test_phrase_reference.py: texts whose phrases have exactly chosen lengths and
contents, and a word list for the explicit geometry.

pfp_parse cuts with the reference's Karp-Rabin hash; under a modulus p >= 2^31 - 1 only a window whose hash is 0 is cut, and
scan_reference.zero_hash_window(w) is such a window Z.  A text  fill_0 Z fill_1 Z ... fill_m-1 Z tail  of random filler bytes
3..255 is therefore cut at the Z's and nowhere else (test_phrase_reference.py asserts it for every text here): phrase 0 is
Dollar fill_0 Z, phrase k is Z fill_k Z, the last phrase Z tail Dollar^w.  Two phrases are equal exactly when their fillers are.

The two constants below restate csrc/phrase.hip; test_phrase_reference.py reads the source and fails when they drift."""
import functools

import numpy as np

from scan_reference import zero_hash_window

P_EXACT = 1 << 31          # the modulus of every case: no cut but the planted ones
LONG_PHRASE = 8192         # kLongPhrase: longer phrases are hashed and copied by the whole device
LANES4_MEAN_MAX = 72       # lanes_log2_for: 4 lanes per phrase up to this mean phrase length, 8 beyond
EDGE_OFFSETS = (7, 8, 15, 16, 17, 63, 64, 127, 128)      # phrase offsets at which near-equal phrases differ
CLASS_LENGTHS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
LONG_NEAR_EQUAL = LONG_PHRASE + 23      # length of the long phrases that differ in one byte: 513 pieces of 16 bytes and one of 7


def random_filler(rng, n):
    return rng.integers(3, 256, size=n, dtype=np.uint8)


def filler_len(k, length, w):
    """filler bytes of phrase k (not the last) of a given length: phrase 0 is Dollar . filler . Z, the others Z . filler . Z"""
    return length - (1 + w if k == 0 else 2 * w)


def planted_text(lengths, fillers, w, tail):
    """-> (text, ends): the text whose phrases 0 .. m-1 have these lengths and whose last phrase is Z . tail . Dollar^w, and the
    text positions of the last byte of every planted window.  fillers[k] is phrase k's filler (filler_len(k, lengths[k], w) bytes
    3..255): handing one array to two phrases makes them equal, a copy with one byte changed makes them differ in that byte."""
    z = zero_hash_window(w)
    parts, ends, pos = [], [], 0
    for k, (length, f) in enumerate(zip(lengths, fillers)):
        f = np.asarray(f, dtype=np.uint8)
        assert len(f) == filler_len(k, length, w) and (len(f) == 0 or f.min() >= 3), (k, length, len(f))
        parts += [f, z]
        pos += len(f) + w
        ends.append(pos - 1)
    parts.append(np.asarray(tail, dtype=np.uint8))
    return np.concatenate(parts), np.array(ends, dtype=np.uint64)


def one_byte_variant(f, at):
    """a copy of a filler with the byte at index `at` changed (and still >= 3)"""
    g = np.array(f, dtype=np.uint8)
    g[at] = g[at] - 1 if g[at] == 255 else g[at] + 1
    return g


def edge_bundle(rng, w):
    """[(length, filler)] - phrases (none of them the first) that every lane layout is tried on: the lengths around 16, 32, 64, 128
    and 256 twice each (an equal pair per length), phrases with 3, 7 and 50 occurrences, pairs that differ in one byte at the
    phrase offsets of EDGE_OFFSETS and at the last byte in front of the closing window, and fillers that are a prefix of another"""
    out = []
    for length in CLASS_LENGTHS:
        if length >= 2 * w:
            f = random_filler(rng, length - 2 * w)
            out += [(length, f), (length, f)]
    for length, copies in ((100, 50), (40, 7), (150, 3)):
        f = random_filler(rng, length - 2 * w)
        out += [(length, f)] * copies
    for length in (200, 203):
        for off in EDGE_OFFSETS + (length - w - 1,):
            f = random_filler(rng, length - 2 * w)
            out += [(length, f), (length, one_byte_variant(f, off - w))]
    f = random_filler(rng, 60)
    out += [(60 + 2 * w, f), (59 + 2 * w, f[:59]), (44 + 2 * w, f[:44])]
    return out


def _assemble(rng, w, first, entries, tail, last_entries=()):
    """shuffle the entries (copies and variants end up scattered), put `first` in front and `last_entries` at the end"""
    order = rng.permutation(len(entries))
    seq = [first] + [entries[i] for i in order] + list(last_entries)
    lengths = [a for a, _ in seq]
    text, ends = planted_text(lengths, [b for _, b in seq], w, tail)
    return dict(w=w, text=text, ends=ends, lengths=lengths + [len(tail) + 2 * w])


def _first(rng, length, w):
    return (length, random_filler(rng, filler_len(0, length, w)))


def _fresh(rng, lengths, w):
    return [(a, random_filler(rng, a - 2 * w)) for a in lengths]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(w, text, ends, lengths) of a named case; `lengths` are the phrase lengths the case was built for, the last phrase's
    included"""
    if name in ("lanes8", "w5", "w7"):
        # mean phrase length > 72: 8 lanes per phrase, striding 128 bytes.  The first phrase is the shortest there is: Dollar . Z
        w = {"lanes8": 4, "w5": 5, "w7": 7}[name]
        rng = np.random.default_rng(100 + w)
        body = edge_bundle(rng, w) + _fresh(rng, [100 + (7 * i) % 61 for i in range(330)], w)
        return _assemble(rng, w, _first(rng, w + 1, w), body, random_filler(rng, 37))
    if name == "lanes4":
        # mean phrase length <= 72: 4 lanes per phrase, striding 64 bytes; three long phrases among 1800 short ones
        w, rng = 4, np.random.default_rng(204)
        body = edge_bundle(rng, w) + _fresh(rng, [20 + (11 * i) % 51 for i in range(1800)], w)
        body += _fresh(rng, [191, 192, 193, LONG_PHRASE + 1, LONG_PHRASE + 8, LONG_PHRASE + 16], w)
        return _assemble(rng, w, _first(rng, 30, w), body, random_filler(rng, 21))
    if name == "long":
        # phrases around kLongPhrase and far beyond it; several long ones (nlong > 1), two of them equal, four that differ in one
        # byte; the first and the last phrase of the text long
        w, rng = 4, np.random.default_rng(304)
        body = _fresh(rng, [LONG_PHRASE - 1, LONG_PHRASE, LONG_PHRASE + 16, 3 * LONG_PHRASE + 5, 50, 51, 52, 53, 54, 55], w)
        f = random_filler(rng, LONG_PHRASE + 1 - 2 * w)
        body += [(LONG_PHRASE + 1, f), (LONG_PHRASE + 1, f)]
        length = LONG_NEAR_EQUAL      # (the byte in front of the closing window lies in the last, partial 16-byte piece)
        f = random_filler(rng, length - 2 * w)
        body += [(length, f)] + [(length, one_byte_variant(f, off - w)) for off in (LONG_PHRASE - 1, LONG_PHRASE, length - w - 1)]
        return _assemble(rng, w, _first(rng, 20000, w), body, random_filler(rng, 9000))
    if name == "one_phrase":
        w, rng = 4, np.random.default_rng(404)
        return dict(w=w, text=random_filler(rng, 50000), ends=np.zeros(0, dtype=np.uint64), lengths=[1 + 50000 + w])
    if name == "two_phrases":
        w, rng = 4, np.random.default_rng(504)
        text, ends = planted_text([1 + 25000 + w], [random_filler(rng, 25000)], w, random_filler(rng, 25000))
        return dict(w=w, text=text, ends=ends, lengths=[1 + 25000 + w, 25000 + 2 * w])
    raise KeyError(name)


PARSE_CASES = ("lanes8", "lanes4", "long", "w5", "w7", "one_phrase", "two_phrases")


def mean_phrase_bytes(c):
    """what lanes_log2_for divides: the bytes the phrases cover (text + one window per phrase) by the number of phrases"""
    phrases = len(c["ends"]) + 1
    return (len(c["text"]) + c["w"] * phrases) // phrases


@functools.lru_cache(maxsize=None)
def sibling_text():
    """a second text that shares about half of its phrases with case("lanes8"): words both texts hold must go to one owner"""
    c = case("lanes8")
    w, rng = c["w"], np.random.default_rng(604)
    text, ends = c["text"], c["ends"].astype(np.int64)
    lengths, fillers = [w + 1], [np.zeros(0, dtype=np.uint8)]
    for k in range(1, len(ends)):
        length = int(ends[k] - ends[k - 1]) + w
        own = text[ends[k - 1] + 1:ends[k] - w + 1]
        lengths.append(length)
        fillers.append(own if k % 2 else random_filler(rng, length - 2 * w))
    return planted_text(lengths, fillers, w, random_filler(rng, 37))


OWNER_WORD_CLASSES = (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 8191, 8192, 8193, 20000)


@functools.lru_cache(maxsize=None)
def owner_words():
    """-> (words, weights): 3000 words (bytes 3..255) for the weighted dedup of a caller-made list.  Lengths 1 .. 40 for most -
    among the one- and two-byte words many are equal by chance - and of every class of OWNER_WORD_CLASSES a word, an equal copy
    and, from 7 bytes on, a copy whose last byte differs; for the 8-byte class also copies that differ in the first byte and are
    cut short by one.  Weights 1 .. 1000; five distinct words, one of them with two copies, are given the total 1000."""
    rng = np.random.default_rng(704)
    words = []
    for length in OWNER_WORD_CLASSES:
        f = random_filler(rng, length)
        words += [f.tobytes(), f.tobytes()]
        if length >= 7:
            words.append(one_byte_variant(f, length - 1).tobytes())
        if length == 8:
            words += [one_byte_variant(f, 0).tobytes(), f[:7].tobytes()]
    ties = [random_filler(rng, 12).tobytes() for _ in range(5)]
    words += ties + [ties[2]]
    special = len(words)
    while len(words) < 3000:
        r = rng.random()
        n = 1 if r < 0.1 else 2 if r < 0.2 else int(rng.integers(3, 41))
        words.append(random_filler(rng, n).tobytes())
    order = rng.permutation(len(words))
    weights = rng.integers(1, 1001, size=len(words)).astype(np.uint32)
    for i in range(special - 6, special):
        weights[i] = 1000
    weights[special - 4], weights[special - 1] = 400, 600          # ties[2] twice: 400 + 600
    return [words[i] for i in order], weights[order]


# Word lists on which the byte verification alone stands between a hash collision and a wrong dictionary.  Under
# PFP_TEST_HASH_BITS=1 half of the words share a hash on the first attempt; the dedup goes on to a second seed only if the
# verification of SOME neighbours in hash order sees a difference - so every pair of words must differ only where the lists say.
# (No text can do this: its first phrase begins with the Dollar and betrays any class it falls into.)
VERIFY_LISTS = ("stripe8", "stripe4", "prefixes")


@functools.lru_cache(maxsize=None)
def verify_words(name):
    """200 distinct words.  stripe8: 300 bytes each, mean above LANES4_MEAN_MAX - 8 lanes stride 128 bytes - alike but for bytes
    128 .. 255, the second 128-byte step of every lane group.  stripe4: 70 bytes each (71 with the terminator: 4 lanes, stride
    64), alike but for bytes 64 .. 69, the second step.  prefixes: the first 300, 299, .. 101 bytes of one string, longest first:
    a later word equals the beginning of every earlier one, only the lengths differ."""
    rng = np.random.default_rng(sum(name.encode()) + 800)
    if name == "prefixes":
        base = random_filler(rng, 300).tobytes()
        return [base[:300 - i] for i in range(200)]
    size, lo, hi = (300, 128, 256) if name == "stripe8" else (70, 64, 70)
    base, words = random_filler(rng, size), set()
    while len(words) < 200:
        f = base.copy()
        f[lo:hi] = random_filler(rng, hi - lo)
        words.add(f.tobytes())
    return sorted(words)


# ---------------------------------------------------------------- synthetic parses for stage 2 (tests/test_parse_bwt.py)

DISTINCT_COUNTS = (2, 3, 255, 256, 257, 4095, 4096, 4097)      # around the widths bits_for(d) of the inverted list's sort
BIG_SAI = ((1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 40) - 1)
PARSE_BWT_CASES = ("P2", "P3", "big_sai", "stable") + tuple("d%d" % d for d in DISTINCT_COUNTS)


def _parse_case(rng, parse):
    """a parse as stage 2 wants it - symbol 1 first and only there, every symbol 1 .. d present - with its occ, last bytes (the last
    phrase's is 255, every other below it: the cyclic predecessor of row SA[j] = 1 is told apart) and ascending sai values"""
    parse = np.asarray(parse, dtype=np.uint32)
    P = len(parse)
    occ = np.bincount(parse)[1:].astype(np.uint32)
    assert parse[0] == 1 and occ[0] == 1 and occ.min() >= 1
    last = rng.integers(0, 255, size=P, dtype=np.uint8)
    last[P - 1] = 255
    sai = np.cumsum(rng.integers(5, 300, size=P)).astype(np.uint64)
    return dict(parse=parse, occ=occ, last=last, sai=sai)


@functools.lru_cache(maxsize=None)
def parse_case(name):
    """dict(parse, occ, last, sai) of a named synthetic parse, 2 <= P <= 5000"""
    rng = np.random.default_rng(sum(name.encode()) + 900)
    if name == "P2":
        return _parse_case(rng, [1, 2])
    if name == "P3":
        return _parse_case(rng, [1, 3, 2])
    if name == "one_word":          # not a parse of any text: the row of SA[j] = 0 comes last, not second (bwtparse.c:305 asserts)
        P = 1000
        return dict(parse=np.ones(P, dtype=np.uint32), occ=np.array([P], dtype=np.uint32), last=np.full(P, 65, dtype=np.uint8),
                    sai=np.arange(5, 5 * P + 5, 5, dtype=np.uint64))
    if name == "big_sai":
        c = _parse_case(rng, np.concatenate([[1], rng.permutation(np.concatenate([np.arange(2, 51), rng.integers(2, 51, size=250)]))]))
        at = rng.choice(len(c["sai"]), size=2 * len(BIG_SAI), replace=False)
        c["sai"][at] = np.array(BIG_SAI + BIG_SAI, dtype=np.uint64)          # twice each, the last phrase's among them
        c["sai"][-1] = BIG_SAI[1]
        return c
    if name == "stable":            # symbol 2 two thousand times: its inverted list must come out ascending
        body = np.concatenate([np.full(2000, 2), np.arange(3, 41), rng.integers(3, 41, size=900)])
        return _parse_case(rng, np.concatenate([[1], rng.permutation(body)]))
    d = int(name[1:])
    # every symbol 2 .. d, 300 more at random; the largest symbol d in front of the terminator (row 0 of the BWT) and, as a run of
    # three in the middle, in front of one of the largest suffixes (the last rows; the very last cannot hold it: d in front of
    # the largest suffix would make a larger one)
    body = rng.permutation(np.concatenate([np.arange(2, d + 1), rng.integers(2, d + 1, size=300)]))
    half = len(body) // 2
    return _parse_case(rng, np.concatenate([[1], body[:half], [d, d, d], body[half:], [d]]))
