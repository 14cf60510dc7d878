"""Plain Python / numpy restatement of what lies between the scan and the merge: stage 1 from the phrase ends on (newscan.cpp:229-441:
the phrases, the dictionary, the occurrence counts, the parse, .last and .sai), the order of the words in the device dictionary
(csrc/phrase.hip), and stage 2 (bwtparse.c:212-322: the BWT of the parse and its inverted lists).  Written from the formats, not
from the kernels: nothing here calls into libpfpgpu.so or the oracle, and nothing here hashes.

Conventions: a text is a uint8 array; `ends` are the scan's phrase ends, the text position of the last byte of every trigger
window; T' = 0x02 . text . 0x02^w; a word is a Python bytes object."""
import numpy as np

DOLLAR, END_OF_WORD, END_OF_DICT = 2, 1, 0


def usable(text):
    """the bytes that are parsed: up to the first byte <= 2 (newscan.cpp:364)"""
    t = np.asarray(text, dtype=np.uint8)
    bad = np.flatnonzero(t <= DOLLAR)
    return t[:int(bad[0])] if len(bad) else t


def phrases(text, ends, w):
    """-> (words, last, sai).  Phrase k ends at T' index ends[k] + 1 - the last one at n + w - and the next phrase starts w - 1
    before that end: neighbours share a trigger window.  last[k] = T'[e - w] is the byte in front of the phrase's closing window,
    sai[k] = e."""
    t = usable(text)
    n = len(t)
    tp = bytes([DOLLAR]) + t.tobytes() + bytes([DOLLAR]) * w
    stops = [int(e) + 1 for e in ends] + [n + w]
    assert all(a < b for a, b in zip(stops, stops[1:])) and stops[0] >= w, "ends must ascend, the first at w - 1 or later"
    words, start = [], 0
    for e in stops:
        words.append(tp[start:e + 1])
        start = e - w + 1
    last = np.array([tp[e - w] for e in stops], dtype=np.uint8)
    return words, last, np.array(stops, dtype=np.uint64)


def stage1(text, ends, w):
    """the files of newscan: dict (the distinct phrases in byte order, each closed by 0x01, the whole by 0x00), occ (per word of
    the dictionary), parse (1-based ranks), last, sai"""
    words, last, sai = phrases(text, ends, w)
    distinct = sorted(set(words))
    rank = {x: r + 1 for r, x in enumerate(distinct)}
    parse = np.array([rank[x] for x in words], dtype=np.uint32)
    occ = np.bincount(parse, minlength=len(distinct) + 1)[1:].astype(np.uint32)
    blob = b"".join(x + bytes([END_OF_WORD]) for x in distinct) + bytes([END_OF_DICT])
    return dict(n_used=len(usable(text)), dict=np.frombuffer(blob, dtype=np.uint8), occ=occ, parse=parse, last=last, sai=sai)


def device_order(words, weights=None):
    """The contract of the device dictionary's order: the distinct words by descending total weight (every copy counts once
    where no weights are given), ties by the smallest index of a copy.  -> (pid, ordered, total): pid[i] is the place of words[i]'s
    distinct word in `ordered`, total[j] the summed weight of ordered[j]."""
    first, total = {}, {}
    for i, x in enumerate(words):
        first.setdefault(x, i)
        total[x] = total.get(x, 0) + (1 if weights is None else int(weights[i]))
    ordered = sorted(first, key=lambda x: (-total[x], first[x]))
    place = {x: j for j, x in enumerate(ordered)}
    return (np.array([place[x] for x in words], dtype=np.uint32), ordered,
            np.array([total[x] for x in ordered], dtype=np.uint64))


def words_blob(words):
    """words, each closed by 0x01, back to back (a dictionary without its final 0x00)"""
    return np.frombuffer(b"".join(x + bytes([END_OF_WORD]) for x in words), dtype=np.uint8)


def split_blob(blob):
    """the inverse of words_blob"""
    parts = bytes(np.asarray(blob, dtype=np.uint8)).split(bytes([END_OF_WORD]))
    assert parts[-1] == b"", "the last word is not closed"
    return parts[:-1]


def suffix_array(symbols):
    """suffix array of a sequence of integers below 2^32 that ends with its only, smallest symbol: a plain sort of the suffixes
    (written big-endian, four bytes a symbol, so that bytes compare like tuples of integers)"""
    enc = np.asarray(symbols, dtype=">u4").tobytes()
    return sorted(range(len(symbols)), key=lambda i: enc[4 * i:])


def stage2(parse, last, sai, occ):
    """the files of bwtparse -> dict(sa, bwtp, ilist, bwlast, bwsai).  SA = suffix array of parse . 0; row j holds the phrase in
    front of suffix SA[j]: bwtp[j] = parse[SA[j] - 1], bwsai[j] = that phrase's sai, bwlast[j] = last of the phrase before that
    one - cyclically, last[P - 1] for SA[j] = 1; the row of SA[j] = 0 holds zeros.  ilist = the rows grouped by bwtp, ascending
    inside a group.  occ must count the parse's symbols: the reference cuts ilist into the words' lists by it."""
    parse = [int(x) for x in parse]
    P = len(parse)
    assert P >= 2 and min(parse) >= 1
    assert np.array_equal(np.bincount(parse, minlength=len(occ) + 1)[1:], np.asarray(occ, dtype=np.int64)), "occ does not count the parse"
    sa = suffix_array(parse + [0])
    bwtp = np.zeros(P + 1, dtype=np.uint32)
    bwlast = np.zeros(P + 1, dtype=np.uint8)
    bwsai = np.zeros(P + 1, dtype=np.uint64) if sai is not None else None
    for j, s in enumerate(sa):
        if s == 0:
            continue
        bwtp[j] = parse[s - 1]
        bwlast[j] = last[s - 2]          # (s = 1: index -1, the last phrase)
        if sai is not None:
            bwsai[j] = sai[s - 1]
    ilist = np.argsort(bwtp, kind="stable").astype(np.uint32)
    return dict(sa=np.array(sa, dtype=np.uint64), bwtp=bwtp, ilist=ilist, bwlast=bwlast, bwsai=bwsai)
