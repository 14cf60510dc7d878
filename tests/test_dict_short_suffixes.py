"""The dictionary suffixes that emit nothing - at most w bytes long, and the final 0x00 - are left out of the dictionary's
suffix sort and of everything per slot after it (csrc/sufsort.hip `sort_dict_suffixes` with a minimum length; csrc/chain.hip
passes w).  PFP_DROP_SHORT=0 (read per call) sorts every position as before.

Every case runs the fused chain in a context with PFP_DEBUG=1 - the validators then check the shortened suffix array slot by
slot (`validate_suffix_order`), the keys of the kept positions and which positions were kept (`check_keys_kernel`) - and
compares whole outputs with the CPU oracle; the same call with PFP_DROP_SHORT=0, in a context without PFP_DEBUG (lazy ranks,
the whole words' ranks through wordrank[]), must give the same bytes and the same statistics.  The kernel trace is the
witness of which path ran: `pfp::short_words_kernel` opens only where a list is attempted, the first round's key kernel
runs a second time only where the list was given up, and the merge's per-slot rows carry their slot count in their bytes.

The contexts parse with the reference's window hash (PFP_WINDOW_HASH=kr), so the oracle's dictionary is the chain's and the
directed inputs can be checked for what they are meant to hold.  (A dictionary with a single word cannot come out of a parse:
one phrase is an error, bwtparse.c:244, and the first phrase of two starts with 0x02.  The smallest dictionary here has two
words.)"""
import json
import os

import numpy as np
import pytest

from textgen import make_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLAGS = (0, 1, 2, 4, 6)
WIDTHS = (32, 64)
SWITCHES = ("PFP_DROP_SHORT", "PFP_KEYSONLY", "PFP_PREC_DIRECT")
STATS = ("n", "n_phrases", "n_words", "dict_size", "hard_groups", "hard_chars", "hard_big_groups", "hard_max_chars",
         "hard_max_members", "hard_minor_groups", "hard_minor_chars")
COUNT_ROW, KEYS_ROW = "pfp::short_words_kernel", "pfp::init_keys_packed_kernel"
SLOT_ROWS = ("pfp::slot_records_kernel", "pfp::slot_payload_kernel")
WORD_PASS_ROW = "pfp::word_slots_range_kernel"
KEY_TILE = 224                       # positions per workgroup of the first round's key kernel (kKeyPos)


def _dna(seed, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)].copy()


def two_word_text(O, w, p):
    """a text with exactly one trigger window, placed so that both words of its dictionary are KEY_TILE + w bytes long:
    whichever comes first has its last w bytes in the second key tile"""
    before, n = KEY_TILE - 2 + w, 2 * KEY_TILE - 1
    big = _dna(41, 200000)
    ends = [int(e) for e in O.scan(big, w, p)]
    for k, e in enumerate(ends):
        lo = ends[k - 1] if k else -1
        hi = ends[k + 1] if k + 1 < len(ends) else len(big) + n
        if e >= before and lo < e - before and hi > e - before + n + w and e - before + n <= len(big):
            return big[e - before:e - before + n].copy()
    raise AssertionError("no isolated trigger window in the sample")


DENSE = (("w4p10", 4, 10), ("w4p11", 4, 11), ("w5p10", 5, 10))


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as fh:
        return [c for c in json.load(fh) if c["n"] <= 100000]


def build_cases():
    """{name: dict(text=callable(O), w, p, env)}"""
    cases = {}
    for c in _golden():
        cases["golden_" + c["name"]] = dict(text=lambda O, s=c["spec"]: make_text(s, O), w=c["w"], p=c["p"], env={})
    # words of exactly w + 1 bytes (two trigger windows one position apart), each with one kept suffix; dozens of words per key tile
    # (w = 4 and p = 10 are the smallest the reference takes, newscan.cpp:537-544)
    for tag, w, p in DENSE:
        cases["dense_" + tag] = dict(text=lambda O, w=w, p=p: _dna(20 + w + p, 700), w=w, p=p, env={})
    # two words, the first reaching w bytes into the second key tile
    cases["two_words_w4"] = dict(text=lambda O: two_word_text(O, 4, 211), w=4, p=211, env={})
    # w beyond what a first-round key covers (63 bits of 2-bit codes: 31 characters)
    cases["wide_w40"] = dict(text=lambda O: _dna(31, 6000), w=40, p=37, env={})
    # the keys-only first round (32-bit positions only): the position rides in the key word, no value array
    for name in ("golden_gen_small", "dense_w4p10", "two_words_w4", "wide_w40"):
        cases[name + "/keysonly"] = dict(cases[name], env={"PFP_KEYSONLY": "1"})
    return cases


CASES = build_cases()
# the dictionaries of these texts (one phrase of 30 000 / 12 000 equal bytes) reach a doubling round: the list is given up
FALLBACK = ("golden_n_run", "golden_gen_nblock")
# opened by the dictionary's first doubling round alone (the parse's rounds keep no lazy ranks; without PFP_DEBUG)
DOUBLING_ROW = "pfp::repair_ranks_kernel"
_texts, _wants, _dicts, _runs = {}, {}, {}, {}


def text_of(O, name):
    key = name.split("/")[0]
    if key not in _texts:
        _texts[key] = CASES[name]["text"](O)
    return _texts[key]


def want_of(O, name, flags):
    key = (name.split("/")[0], flags)
    if key not in _wants:
        c = CASES[name]
        _wants[key] = O.bigbwt(text_of(O, name), c["w"], c["p"], flags)
    return _wants[key]


def words_of(O, name):
    """lengths of the words of the oracle's dictionary"""
    key = name.split("/")[0]
    if key not in _dicts:
        c = CASES[name]
        d = O.parse(text_of(O, name), c["w"], c["p"])["dict"].tobytes()
        assert d[-1] == 0 and d[-2] == 1
        _dicts[key] = [len(x) for x in d[:-2].split(b"\x01")]
    return _dicts[key]


class switches:
    """the switches (read per call) in os.environ for the duration of a call, all others of them unset"""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in SWITCHES}
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def new_context(pkg, **env):
    env = dict(env, PFP_WINDOW_HASH="kr")
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.Context(0)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def dctx(pkg):
    c = new_context(pkg, PFP_DEBUG="1")
    yield c
    c.close()


@pytest.fixture(scope="module")
def pctx(pkg):
    c = new_context(pkg)
    yield c
    c.close()


def run(O, ctx, tag, name, flags, width, drop):
    """one traced call of the fused chain, once per (context, case, flags, width, path): outputs, trace rows, statistics"""
    key = (tag, name, flags, width, drop)
    if key not in _runs:
        c = CASES[name]
        ctx.set_index_bits(64 if width == 64 else 0)
        ctx.set_kernel_trace(True)
        try:
            with switches(**dict(c["env"], **({} if drop else {"PFP_DROP_SHORT": "0"}))):
                got = ctx.bigbwt(text_of(O, name), c["w"], c["p"], flags)
            rows = {r["name"]: r for r in ctx.kernel_trace()}
            st = ctx.stats()
        finally:
            ctx.set_kernel_trace(False)
            ctx.set_index_bits(0)
        _runs[key] = (got, rows, {k: st[k] for k in STATS})
    return _runs[key]


def check_outputs(O, pkg, got, want, flags):
    assert np.array_equal(got["bwt"], want["bwt"])
    if flags & pkg.FLAG_SA:
        assert np.array_equal(pkg.unpack5(got["sa"]), want["sa"])
    if flags & pkg.FLAG_SSA:
        assert np.array_equal(pkg.unpack5(got["ssa"]).reshape(-1, 2), want["ssa"])
    if flags & pkg.FLAG_ESA:
        assert np.array_equal(pkg.unpack5(got["esa"]).reshape(-1, 2), want["esa"])


def same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def slots_of(rows):
    """the slot count the merge's per-slot row was opened with: its algorithmic bytes per launch are a whole number of
    bytes per slot (14 from the sort keys; up to 160 for the gathered records, by index width and outputs)"""
    row = [rows[r] for r in SLOT_ROWS if r in rows]
    assert len(row) == 1
    return row[0]["algo_bytes"] // row[0]["launches"], row[0]["algo_bytes"] % row[0]["launches"]


def check_witness(name, rows, st, w, drop):
    per_launch, rest = slots_of(rows)
    assert rest == 0
    kept = st["dict_size"] - (w + 1) * st["n_words"] - 1
    if not drop:
        assert COUNT_ROW not in rows and rows[KEYS_ROW]["launches"] == 1
        slots = st["dict_size"]
    elif name.split("/")[0] in FALLBACK:
        # the list was attempted, then every position sorted as before: the old path's kernels ran after it
        assert rows[COUNT_ROW]["launches"] == 1 and rows[KEYS_ROW]["launches"] == 2
        slots = st["dict_size"]
    else:
        assert rows[COUNT_ROW]["launches"] == 1 and rows[KEYS_ROW]["launches"] == 1
        slots = kept
    assert per_launch % slots == 0 and 8 <= per_launch // slots <= 160, (per_launch, slots)
    # the whole words' slots come from the sorter's ranks (wordrank[] / the search over the sorted keys), not from a pass over
    # the slots as in a multi-GPU share (gather_slots_range, which opens this row: test_share_pass_opens_its_row)
    assert WORD_PASS_ROW not in rows
    return [r for r in SLOT_ROWS if r in rows][0], per_launch // slots


# ---------------------------------------------------------------- what the directed inputs hold

def test_directed_inputs_are_what_they_are_meant_to_be(O):
    for tag, w, _ in DENSE:
        lens = words_of(O, "dense_" + tag)
        assert min(lens) == w + 1 and len(lens) > 3 * (700 // KEY_TILE)
    assert words_of(O, "two_words_w4") == [KEY_TILE + 4, KEY_TILE + 4]
    assert min(words_of(O, "wide_w40")) > 40
    for name in CASES:
        assert min(words_of(O, name)) > CASES[name]["w"]


# ---------------------------------------------------------------- parity under PFP_DEBUG, and the two paths against each other

@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(CASES))
def test_shortened_order_matches_the_oracle(O, pkg, dctx, name, flags, width):
    got, rows, st = run(O, dctx, "debug", name, flags, width, True)
    check_outputs(O, pkg, got, want_of(O, name, flags), flags)
    lens = words_of(O, name)
    assert st["n_words"] == len(lens) and st["dict_size"] == sum(lens) + len(lens) + 1
    check_witness(name, rows, st, CASES[name]["w"], True)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", list(CASES))
def test_both_paths_agree(O, pkg, dctx, pctx, name, flags, width):
    got1, rows1, st1 = run(O, pctx, "plain", name, flags, width, True)
    got0, rows0, st0 = run(O, pctx, "plain", name, flags, width, False)
    check_outputs(O, pkg, got0, want_of(O, name, flags), flags)
    same_bytes(got0, got1)
    same_bytes(got1, run(O, dctx, "debug", name, flags, width, True)[0])
    assert st0 == st1
    # the same bytes per slot on both paths: what differs in the row is the number of slots.  (The source of the records is
    # chosen by the share of slots re-ordered after the first round: with w beyond the key's reach the short suffixes are
    # most of those, and the two paths may choose differently)
    (row1, per1), (row0, per0) = check_witness(name, rows1, st1, CASES[name]["w"], True), check_witness(name, rows0, st0, CASES[name]["w"], False)
    assert row1 != row0 or per1 == per0
    # the list is given up exactly where the sort of every position runs a doubling round
    assert (name.split("/")[0] in FALLBACK) == (DOUBLING_ROW in rows0)


@pytest.mark.parametrize("width", WIDTHS)
def test_old_path_under_debug(O, pkg, dctx, width):
    """PFP_DROP_SHORT=0 with the validators on: the whole order is still what they accept"""
    for name in ("golden_gen_small", "dense_w4p10"):
        got, rows, st = run(O, dctx, "debug", name, 6, width, False)
        check_outputs(O, pkg, got, want_of(O, name, 6), 6)
        check_witness(name, rows, st, CASES[name]["w"], False)


# ---------------------------------------------------------------- the staged entry: dictionaries no parse makes

def staged_files(O, ctx, name):
    """the stage files of a case, from the staged entry points"""
    c = CASES[name]
    ps = ctx.parse(text_of(O, name), c["w"], c["p"], want_sai=True)
    ilist, bwlast, bwsai = ctx.bwtparse(ps["parse"], ps["last"], ps["occ"], ps["sai"])
    return ps, ilist, bwlast, bwsai


def traced_merge(ctx, files, w, flags, **env):
    ps, ilist, bwlast, bwsai = files
    ctx.set_kernel_trace(True)
    try:
        with switches(**env):
            got = ctx.merge(ps["dict"], ps["occ"], ilist, bwlast, bwsai, w, flags)
        rows = {r["name"]: r for r in ctx.kernel_trace()}
    finally:
        ctx.set_kernel_trace(False)
    return got, rows


@pytest.mark.parametrize("flags", (0, 6))
def test_staged_merge_takes_the_list(O, pkg, dctx, flags):
    """pfp_merge passes w too: the files of a parse merge to the oracle's outputs through the shortened order"""
    name = "dense_w4p10"
    files = staged_files(O, dctx, name)
    got, rows = traced_merge(dctx, files, CASES[name]["w"], flags)
    check_outputs(O, pkg, got, want_of(O, name, flags), flags)
    lens = words_of(O, name)
    dsize = sum(lens) + len(lens) + 1
    per_launch, rest = slots_of(rows)
    assert rows[COUNT_ROW]["launches"] == 1 and rows[KEYS_ROW]["launches"] == 1
    assert rest == 0 and per_launch % (dsize - (CASES[name]["w"] + 1) * len(lens) - 1) == 0


@pytest.mark.parametrize("flags", (0, 6))
def test_dictionary_with_a_word_of_at_most_w_bytes_is_sorted_whole(O, pkg, dctx, pctx, flags):
    """The files of a parse with w = 4 (words of 5 and 6 bytes among them) merged with w = 6: a dictionary no parse with that
    w makes.  The guard finds the short words, every position is sorted once, and the outputs are those of PFP_DROP_SHORT=0"""
    name, w = "dense_w4p10", 6
    lens = words_of(O, name)
    assert min(lens) <= w < max(lens)
    dsize = sum(lens) + len(lens) + 1
    for ctx in (dctx, pctx):
        files = staged_files(O, ctx, name)
        got, rows = traced_merge(ctx, files, w, flags)
        per_launch, rest = slots_of(rows)
        assert rows[COUNT_ROW]["launches"] == 1 and rows[KEYS_ROW]["launches"] == 1
        assert rest == 0 and per_launch % dsize == 0 and 8 <= per_launch // dsize <= 160
        old, rows0 = traced_merge(ctx, files, w, flags, PFP_DROP_SHORT="0")
        assert COUNT_ROW not in rows0
        same_bytes(got, old)


def test_zero_byte_inside_a_word_is_an_error(O, pkg, pctx):
    """a dictionary file with 0x00 inside a word: PFP_EFORMAT before anything is sorted, and the context goes on working"""
    name = "dense_w4p10"
    ps, ilist, bwlast, bwsai = staged_files(O, pctx, name)
    bad = np.array(ps["dict"], dtype=np.uint8, copy=True)
    at = int(np.flatnonzero(bad == 1)[3]) + 3          # the third byte of the fifth word
    assert bad[at] > 1
    bad[at] = 0
    for flags in (0, 6):
        with pytest.raises(pkg.PfpError):
            pctx.merge(bad, ps["occ"], ilist, bwlast, bwsai, CASES[name]["w"], flags)
    got = pctx.merge(ps["dict"], ps["occ"], ilist, bwlast, bwsai, CASES[name]["w"], 0)
    check_outputs(O, pkg, got, want_of(O, name, 0), 0)


def test_share_pass_opens_its_row(O, pkg):
    """the witness of check_witness can move: two virtual ranks that hold key-range shares of the suffix array find their whole
    words by the pass over their slots, and the row is there"""
    import importlib

    import torch
    d = importlib.import_module("bigbwt_amd.dist")
    text = text_of(O, "golden_gen_small")
    n = len(text)
    cuts = [0, n // 2 - 2, n]
    ctxs = [pkg.Context(0) for _ in range(2)]
    try:
        for c in ctxs:
            c.set_kernel_trace(True)
        shards = [torch.from_numpy(text[cuts[r]:cuts[r + 1]].copy()).cuda() for r in range(2)]
        res = d.simulate(ctxs, shards, 10, 100, 0, halo=8192, shard_sa=True)
        assert np.array_equal(torch.cat([r["bwt"] for r in res]).cpu().numpy(), want_of(O, "golden_gen_small", 0)["bwt"])
        for c in ctxs:
            assert WORD_PASS_ROW in {r["name"] for r in c.kernel_trace()}
    finally:
        for c in ctxs:
            c.close()
