"""GPU: stage 1b (csrc/phrase.hip: phrase hashing, deduplication, word order, dictionary copy, .last / .sai) in its three
geometries, against the plain restatement of tests/phrase_reference.py (itself checked against the oracle on the CPU by
test_phrase_reference.py).  The implicit geometry runs through Context.parse on texts whose phrases have exactly chosen lengths
and contents (tests/phrase_cases.py); the word-list geometry through dist_owner_dedup on a caller-made list; the shard geometry
through dist_local_parse with a halo; the hash partition through dist_partition_words.  Every comparison is exact: these are
integers and bytes.  tests/README.md, "Tests of the phrase stage and the parse's BWT, path by path", lists which case reaches
which path."""
import functools

import numpy as np
import pytest

import phrase_cases as PC
import phrase_reference as PR

pytestmark = pytest.mark.gpu

ECOLLISION, ELIMIT = -4, -5


@functools.lru_cache(maxsize=None)
def wanted(name):
    c = PC.case(name)
    return PR.stage1(c["text"], c["ends"], c["w"])


def check_parse(pkg, ctx, name):
    c, want = PC.case(name), wanted(name)
    got = ctx.parse(c["text"], c["w"], PC.P_EXACT, want_sai=True)
    assert got["n_used"] == len(c["text"]) == want["n_used"]
    assert len(got["parse"]) == len(want["parse"]) and len(got["occ"]) == len(want["occ"]), "phrases or distinct words"
    for k in ("occ", "parse", "last", "dict"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert np.array_equal(pkg.unpack5(got["sai"]), want["sai"]), (name, "sai")


# ---------------------------------------------------------------- implicit geometry: Context.parse

@pytest.mark.parametrize("name", PC.PARSE_CASES)
def test_parse_of_planted_phrases(pkg, wctx, name):
    """dict, occ, parse, last and sai of every planted text = the reference's, in both index widths; no reseed: a verification
    that read past a phrase's end, or hashed bytes behind it, would call equal phrases different"""
    check_parse(pkg, wctx, name)
    assert wctx.stats()["hash_reseeds"] == 0


@pytest.mark.parametrize("bits", [1, 4])
@pytest.mark.parametrize("name", ["lanes8", "long"])
def test_collisions_are_found_and_cured(pkg, ctx, monkeypatch, name, bits):
    """PFP_TEST_HASH_BITS = n: the first attempt keeps n bits of every hash, so phrases of different lengths, near-equal phrases
    and long phrases share hashes; the byte verification finds it, the pass is repeated with another seed and the outputs are
    the reference's.  -n: every attempt collides and the call fails with PFP_ECOLLISION; without the variable the next call is
    exact again."""
    monkeypatch.setenv("PFP_TEST_HASH_BITS", str(bits))
    check_parse(pkg, ctx, name)
    assert ctx.stats()["hash_reseeds"] >= 1
    if bits == 1:
        c = PC.case(name)
        monkeypatch.setenv("PFP_TEST_HASH_BITS", "-1")
        with pytest.raises(pkg.PfpError) as ei:
            ctx.parse(c["text"], c["w"], PC.P_EXACT, want_sai=True)
        assert ei.value.code == ECOLLISION
    monkeypatch.delenv("PFP_TEST_HASH_BITS")
    check_parse(pkg, ctx, name)
    assert ctx.stats()["hash_reseeds"] == 0


# ---------------------------------------------------------------- device buffers for the dist_* calls

@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Dev:
    """numpy arrays to device tensors and back; the library works on its own stream, so every upload is waited for"""

    def __init__(self, torch, ctx):
        self.torch, self.dev = torch, torch.device("cuda", ctx.device)

    def up(self, a, pad=16):
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        t = self.torch.zeros(len(b) + pad, dtype=self.torch.uint8, device=self.dev)
        if len(b):
            t[:len(b)] = self.torch.from_numpy(b.copy())
        self.torch.cuda.synchronize(self.dev)
        return t

    def room(self, nbytes):
        t = self.torch.full((int(nbytes) + 16,), 0xEE, dtype=self.torch.uint8, device=self.dev)
        self.torch.cuda.synchronize(self.dev)
        return t

    def down(self, t, count, dtype):
        self.torch.cuda.synchronize(self.dev)
        return t.cpu().numpy()[:int(count) * np.dtype(dtype).itemsize].view(dtype).copy()


@pytest.fixture
def dist(torch, ctx):
    """the context with its distributed state in place (one tiny local parse), released afterwards"""
    dv = Dev(torch, ctx)
    text, _ = PC.planted_text([1 + 20 + 4], [np.full(20, 65, dtype=np.uint8)], 4, np.full(30, 66, dtype=np.uint8))
    d_text = dv.up(text)
    info = ctx.dist_local_parse(d_text.data_ptr(), len(text), 0, 4, PC.P_EXACT, True, True, 0, 0)
    assert info["phrases"] == 2 and info["words"] == 2
    yield dv
    ctx.dist_release()


def local_parse(ctx, dv, text, lo, hi, halo, w, first, last):
    """dist_local_parse of text[lo - halo : hi] + dist_export_local -> (info, words, occ, last, sai)"""
    local = text[lo - halo:hi]
    d_text = dv.up(local)
    info = ctx.dist_local_parse(d_text.data_ptr(), len(local), halo, w, PC.P_EXACT, first, last, lo, 1)
    d_dict, d_occ = dv.room(info["dict_bytes"]), dv.room(4 * info["words"])
    d_last, d_sai = dv.room(info["phrases"]), dv.room(8 * info["phrases"])
    ctx.dist_export_local(d_dict.data_ptr(), d_occ.data_ptr(), d_last.data_ptr(), d_sai.data_ptr())
    return (info, PR.split_blob(dv.down(d_dict, info["dict_bytes"], np.uint8)), dv.down(d_occ, info["words"], np.uint32),
            dv.down(d_last, info["phrases"], np.uint8), dv.down(d_sai, info["phrases"], np.uint64))


# ---------------------------------------------------------------- explicit geometry, weighted: dist_owner_dedup

def owner_dedup(ctx, dv, words, weights):
    blob = PR.words_blob(words)
    d_bytes, d_occ, d_pid = dv.up(blob), dv.up(np.asarray(weights, dtype=np.uint32)), dv.room(4 * len(words))
    distinct, nbytes = ctx.dist_owner_dedup(d_bytes.data_ptr(), len(blob), d_occ.data_ptr(), len(words), d_pid.data_ptr())
    d_ownb, d_owno = dv.room(nbytes), dv.room(4 * distinct)
    ctx.dist_export_owned(d_ownb.data_ptr(), d_owno.data_ptr())
    return (distinct, nbytes, dv.down(d_pid, len(words), np.uint32), PR.split_blob(dv.down(d_ownb, nbytes, np.uint8)),
            dv.down(d_owno, distinct, np.uint32))


def check_owner_dedup(ctx, dv):
    words, weights = PC.owner_words()
    pid, ordered, total = PR.device_order(words, weights)
    distinct, nbytes, got_pid, got_words, got_occ = owner_dedup(ctx, dv, words, weights)
    assert distinct == len(ordered) and nbytes == sum(len(x) + 1 for x in ordered)
    assert got_words == ordered, "the owned words, or their order: descending summed weight, ties by first copy"
    assert np.array_equal(got_occ, total) and np.array_equal(got_pid, pid)


def test_owner_dedup_of_a_word_list(ctx, dist, monkeypatch):
    """build_dictionary_words with weights: 3000 words of 1 .. 20000 bytes with copies and one-byte variants; the distinct words
    come out by descending summed weight, ties (five words of total 1000, one of them from two copies, and many more by chance)
    in the order of their first copies; pid_out names every input word's distinct word.  The same under colliding hashes."""
    check_owner_dedup(ctx, dist)
    monkeypatch.setenv("PFP_TEST_HASH_BITS", "2")
    check_owner_dedup(ctx, dist)
    monkeypatch.delenv("PFP_TEST_HASH_BITS")
    # nobody sent a word: nothing owned, nothing to export
    assert ctx.dist_owner_dedup(0, 0, 0, 0, 0) == (0, 0)
    ctx.dist_export_owned(0, 0)
    # a list of one word, and one of copies only
    for words, weights in (([b"solo"], [9]), ([b"twin"] * 5, [1, 2, 3, 4, 5])):
        distinct, nbytes, got_pid, got_words, got_occ = owner_dedup(ctx, dist, words, weights)
        assert (distinct, nbytes, got_words, got_occ.tolist(), got_pid.tolist()) == (1, len(words[0]) + 1, words[:1], [sum(weights)], [0] * len(words))


@pytest.mark.parametrize("name", PC.VERIFY_LISTS)
def test_verification_reads_every_stripe_and_the_lengths(ctx, dist, monkeypatch, name):
    """dedup_verify_kernel alone: under PFP_TEST_HASH_BITS=1 half of the 200 words share a hash on the first attempt, and they
    differ only in the second step of a lane group's stride (stripe8: 8 lanes, stripe4: 4 lanes) or only in their lengths
    (prefixes).  A verification that skipped that step, or compared the shorter word's bytes only, would see equal words, keep the
    first attempt and hand back two words for 200."""
    words = PC.verify_words(name)
    weights = np.arange(1, len(words) + 1, dtype=np.uint32)
    pid, ordered, total = PR.device_order(words, weights)
    assert len(ordered) == 200
    for bits in (None, "1"):
        if bits:
            monkeypatch.setenv("PFP_TEST_HASH_BITS", bits)
        distinct, _, got_pid, got_words, got_occ = owner_dedup(ctx, dist, words, weights)
        assert distinct == 200 and got_words == ordered, (name, bits)
        assert np.array_equal(got_occ, total) and np.array_equal(got_pid, pid)
    monkeypatch.delenv("PFP_TEST_HASH_BITS")


# ---------------------------------------------------------------- shard geometry: dist_local_parse with a halo

HALO = 600      # longer than any phrase of the case: a planted end always lies inside


def shard_offsets(ends, n, ranks, delta):
    """the ranks' first text positions: near r n / ranks, placed on a planted end (delta 0), one byte before it or one after"""
    offs = [0]
    for r in range(1, ranks):
        offs.append(int(ends[np.searchsorted(ends, r * n // ranks)]) + delta)
    return offs + [n]


@pytest.mark.parametrize("delta", [0, -1, 1], ids=["on_the_end", "one_before", "one_after"])
@pytest.mark.parametrize("ranks", [2, 3])
def test_shards_own_the_phrases_that_end_inside_them(ctx, dist, ranks, delta):
    """The ownership rule (count_below_kernel: k0 = the first cut with ends[k] >= halo_len): a rank owns the phrases whose
    closing window has its LAST byte at a text position inside the rank's shard - a window that begins in the halo and ends on the
    shard's first byte is the rank's own, one that ends on the halo's last byte is the previous rank's - and the last rank the
    text's last phrase.  Each rank's count, dictionary and occ are those of its own phrases, in the device dictionary's order;
    last and sai of all ranks, back to back, are the whole text's (sai in global positions)."""
    c = PC.case("lanes8")
    text, w, ends = c["text"], c["w"], c["ends"].astype(np.int64)
    words, last, sai = PR.phrases(text, ends, w)
    offs = shard_offsets(ends, len(text), ranks, delta)
    got_last, got_sai = [], []
    for r in range(ranks):
        lo, hi = offs[r], offs[r + 1]
        owned = [k for k in range(len(ends)) if lo <= ends[k] < hi] + ([len(ends)] if r == ranks - 1 else [])
        info, d_words, d_occ, d_last, d_sai = local_parse(ctx, dist, text, lo, hi, HALO if r else 0, w, r == 0, r == ranks - 1)
        assert info["phrases"] == len(owned), (r, "phrases owned")
        _, ordered, total = PR.device_order([words[k] for k in owned])
        assert info["words"] == len(ordered) and info["dict_bytes"] == sum(len(x) + 1 for x in ordered)
        assert d_words == ordered, (r, "local dictionary, or its order")
        assert np.array_equal(d_occ, total), (r, "occ")
        assert info["last_trigger"] == int(ends[ends < hi][-1]) - (lo - (HALO if r else 0))
        got_last.append(d_last)
        got_sai.append(d_sai)
    assert np.array_equal(np.concatenate(got_last), last) and np.array_equal(np.concatenate(got_sai), sai)


def test_a_halo_without_a_phrase_end_is_refused(pkg, ctx, dist):
    """a halo that does not reach back to the last planted end: the phrase that crosses the boundary has no start in the local text"""
    c = PC.case("lanes8")
    text, w, ends = c["text"], c["w"], c["ends"].astype(np.int64)
    k = next(k for k in range(len(ends) // 2, len(ends)) if ends[k] - ends[k - 1] >= 150)
    lo = int(ends[k]) - 20
    with pytest.raises(pkg.PfpError) as ei:
        local_parse(ctx, dist, text, lo, len(text), 16, w, False, True)
    assert ei.value.code == ELIMIT and "halo" in str(ei.value)
    info = local_parse(ctx, dist, text, lo, len(text), 200, w, False, True)[0]
    assert info["phrases"] == len(ends) - k + 1


# ---------------------------------------------------------------- the hash partition: dist_partition_words

def partition(ctx, dv, parts, local_words, local_occ):
    """dist_partition_words + dist_export_partition -> {word: owner}, after the checks that concern one text"""
    counts = ctx.dist_partition_words(parts)
    assert len(counts) == parts
    assert sum(k for k, _ in counts) == len(local_words) and sum(b for _, b in counts) == sum(len(x) + 1 for x in local_words)
    d_bytes, d_occ = dv.room(sum(b for _, b in counts)), dv.room(4 * len(local_words))
    ctx.dist_export_partition(d_bytes.data_ptr(), d_occ.data_ptr())
    sent = PR.split_blob(dv.down(d_bytes, sum(b for _, b in counts), np.uint8))
    occ = dv.down(d_occ, len(local_words), np.uint32)
    index = {x: j for j, x in enumerate(local_words)}
    assert sorted(index[x] for x in sent) == list(range(len(local_words))), "every local word once"
    assert all(occ[i] == local_occ[index[x]] for i, x in enumerate(sent)), "a word travels with its own count"
    owner, at = {}, 0
    for o, (k, b) in enumerate(counts):
        mine = sent[at:at + k]
        assert sum(len(x) + 1 for x in mine) == b, (o, "bytes of an owner")
        assert [index[x] for x in mine] == sorted(index[x] for x in mine), (o, "local order inside an owner")
        owner.update({x: o for x in mine})
        at += k
    return owner


def test_partition_of_the_local_words(ctx, dist):
    """parts = 1, 3, 8: the counts sum to the local dictionary, every word is sent once with its count, an owner's words keep
    their local order, and a word that two texts share goes to one owner from both (the hash itself is free to change)"""
    c = PC.case("lanes8")
    w = c["w"]
    other, _ = PC.sibling_text()
    owners = []
    for text in (c["text"], other):
        _, local_words, local_occ, _, _ = local_parse(ctx, dist, text, 0, len(text), 0, w, True, True)
        owners.append({parts: partition(ctx, dist, parts, local_words, local_occ) for parts in (1, 3, 8)})
    shared = set(owners[0][1]) & set(owners[1][1])
    assert len(shared) > 100
    for parts in (3, 8):
        a, b = owners[0][parts], owners[1][parts]
        assert all(a[x] == b[x] for x in shared), parts
        assert len(set(a.values())) == parts, "an owner without a word among several hundred"
