"""GPU: the phrase stage's block-wise kernels (csrc/phrase.hip: phrase_hash_kernel takes a block of phrases per workgroup, a lane
group several of them one after the other; phrase_verify_kernel compares every phrase, in text order, with the dictionary copy of the word it
was given and writes .last / .sai) against the plain restatement of tests/phrase_reference.py.  Inputs: tests/phrase_block_cases.py
(checked on the CPU by test_phrase_blocks.py) and tests/phrase_cases.py.  Every comparison is exact.

tests/README_phrase_text_order.md lists which case reaches which path."""
import functools

import numpy as np
import pytest

import phrase_block_cases as BC
import phrase_cases as PC
import phrase_reference as PR

pytestmark = pytest.mark.gpu


def check_stage1(pkg, ctx, text, ends, w, what):
    want = wanted_stage1(text.tobytes(), ends.tobytes(), w)
    got = ctx.parse(text, w, PC.P_EXACT, want_sai=True)
    assert got["n_used"] == len(text) == want["n_used"]
    assert len(got["parse"]) == len(want["parse"]) and len(got["occ"]) == len(want["occ"]), (what, "phrases or distinct words")
    for k in ("occ", "parse", "last", "dict"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(pkg.unpack5(got["sai"]), want["sai"]), (what, "sai")


@functools.lru_cache(maxsize=None)
def wanted_stage1(text, ends, w):
    return PR.stage1(np.frombuffer(text, dtype=np.uint8), np.frombuffer(ends, dtype=np.uint64), w)


def check_case(pkg, ctx, name):
    c = PC.case(name)
    check_stage1(pkg, ctx, c["text"], c["ends"], c["w"], name)


# ---------------------------------------------------------------- 1. block edges

@pytest.mark.parametrize("lanes", [4, 8])
@pytest.mark.parametrize("P", BC.block_counts())
def test_block_edges(pkg, ctx, P, lanes):
    """1, 2, 3 phrases, one short of a block, a block, one more, two blocks, one more: the tail block, the first phrase of a block
    (whose start is the end of a phrase of the block before) and a lane group some of whose phrases are not there; copies of a phrase lie
    in other blocks.  No reseed: a kernel that hashed or compared a neighbour's bytes would call equal phrases different."""
    text, ends = BC.block_text(P, lanes)
    check_stage1(pkg, ctx, text, ends, BC.W, (P, lanes))
    assert ctx.stats()["hash_reseeds"] == 0


# ---------------------------------------------------------------- 2. a phrase against its word's dictionary copy (word lists)

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


def owner_dedup(ctx, dv, words, weights):
    blob = PR.words_blob(words)
    d_bytes, d_occ, d_pid = dv.up(blob), dv.up(np.asarray(weights, dtype=np.uint32)), dv.room(4 * len(words))
    distinct, nbytes = ctx.dist_owner_dedup(d_bytes.data_ptr(), len(blob), d_occ.data_ptr(), len(words), d_pid.data_ptr())
    d_ownb, d_owno = dv.room(nbytes), dv.room(4 * distinct)
    ctx.dist_export_owned(d_ownb.data_ptr(), d_owno.data_ptr())
    return (distinct, dv.down(d_pid, len(words), np.uint32), PR.split_blob(dv.down(d_ownb, nbytes, np.uint8)),
            dv.down(d_owno, distinct, np.uint32))


def check_word_list(ctx, dv, monkeypatch, words, what):
    """the distinct words, their order, occ and pid are device_order's under no hook and under one and two hash bits"""
    weights = np.arange(1, len(words) + 1, dtype=np.uint32)
    pid, ordered, total = PR.device_order(words, weights)
    for bits in (None, "1", "2"):
        if bits:
            monkeypatch.setenv("PFP_TEST_HASH_BITS", bits)
        distinct, got_pid, got_words, got_occ = owner_dedup(ctx, dv, words, weights)
        assert distinct == len(ordered) and got_words == ordered, (what, bits)
        assert np.array_equal(got_occ, total) and np.array_equal(got_pid, pid), (what, bits)
    monkeypatch.delenv("PFP_TEST_HASH_BITS")


@pytest.mark.parametrize("lanes", [4, 8])
def test_every_copy_is_compared_with_its_representative(ctx, dist, monkeypatch, lanes):
    """150 copies of a word among its one-byte variants (offset 0, the offsets around every piece and stride, the last byte), its
    prefixes and its extensions: with one or two hash bits most of them share the word's class on the first attempt, and only a
    compare of every piece, the partial last one included, and of the lengths sends the dedup on to the next seed"""
    check_word_list(ctx, dist, monkeypatch, BC.representative_words(lanes), ("representative", lanes))


@pytest.mark.parametrize("shorter_first", [True, False], ids=["shorter_first", "longer_first"])
@pytest.mark.parametrize("lanes", [4, 8])
def test_lengths_are_compared_before_bytes(ctx, dist, monkeypatch, lanes, shorter_first):
    """equal-prefix words, the representative of a class the shortest or the longest of them: a phrase longer than its word would
    read the next word's bytes behind the terminator, a shorter one agrees with the word in every byte it has"""
    check_word_list(ctx, dist, monkeypatch, BC.prefix_words(lanes, shorter_first), ("prefixes", lanes, shorter_first))


def test_empty_words_of_a_list_are_one_word(ctx, dist, monkeypatch):
    """two adjacent terminators in a caller's blob are a word of no bytes: it has a hash like any other (its length's), so its
    copies, in different blocks of the hash kernel, are one dictionary entry - also under colliding hashes, where the empty word
    shares a class with longer ones and only the length tells them apart"""
    rng = np.random.default_rng(1300)
    words = [PC.random_filler(rng, int(n)).tobytes() for n in rng.integers(1, 40, size=2 * BC.HASH_BLOCK + 10)]
    for at in (3, BC.HASH_BLOCK - 1, BC.HASH_BLOCK, 2 * BC.HASH_BLOCK + 5):
        words[at] = b""
    check_word_list(ctx, dist, monkeypatch, words, "empty words")


# ---------------------------------------------------------------- 3. long phrases

def test_long_phrases_are_verified_by_the_whole_grid(pkg, ctx, monkeypatch):
    """the `long` case under one hash bit: equal long phrases, long phrases that differ at byte kLongPhrase - 1, kLongPhrase and
    the last one share a class on the first attempt; phrase_verify_long_kernel tells them apart"""
    monkeypatch.setenv("PFP_TEST_HASH_BITS", "1")
    check_case(pkg, ctx, "long")
    assert ctx.stats()["hash_reseeds"] >= 1
    monkeypatch.delenv("PFP_TEST_HASH_BITS")


# ---------------------------------------------------------------- 4. a failed attempt leaves nothing behind

def test_a_failed_attempt_leaves_nothing_behind(pkg, ctx, monkeypatch):
    """the dictionary of an attempt that collided is dropped: the same outputs and the same live device bytes after a call that
    reseeded and after one that did not"""
    monkeypatch.setenv("PFP_TEST_HASH_BITS", "1")
    check_case(pkg, ctx, "lanes4")
    assert ctx.stats()["hash_reseeds"] >= 1
    live_after_reseed = ctx.mem_stats()["live"]
    monkeypatch.delenv("PFP_TEST_HASH_BITS")
    check_case(pkg, ctx, "lanes4")
    assert ctx.stats()["hash_reseeds"] == 0
    assert ctx.mem_stats()["live"] == live_after_reseed
