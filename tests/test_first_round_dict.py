"""GPU: the dictionary's first round with its counts folded in (PFP_DICT_FOLD): write_back0_kernel counts the kept slots and kept
heads per tile (no active_count_kernel launch in round 0), and keep0 is the first round's keep[] itself, moved and not copied.
PFP_DICT_FOLD=0 is the path before it.

Every case runs the fused chain as test_dict_short_suffixes.py drives it: in a context with PFP_DEBUG=1 (validate_suffix_order
and check_keys_kernel look at every slot; eager ranks) and in one without (lazy ranks, wordrank[]), in both index widths, with
flags 0, 2, 4, 6 and 1, with PFP_KEYSONLY=1 (small inputs take the keys-only round in the 32-bit build) and PFP_KEYSONLY=0
(pairs).  Outputs against the CPU oracle, and byte for byte with the same statistics against the same call with PFP_DICT_FOLD=0.
The kernel trace says which first round ran: pfp::split_keys_kernel opens on the keys-only path alone, pfp::heads0_kernel on
every path."""
import json
import os

import numpy as np
import pytest

import first_round_cases as F
from textgen import make_text

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLAGS = (0, 2, 4, 6, 1)
STATS = ("n", "n_phrases", "n_words", "dict_size", "hard_groups", "hard_chars", "hard_big_groups", "hard_max_chars",
         "hard_max_members", "hard_minor_groups", "hard_minor_chars")
SWITCHES = ("PFP_DICT_FOLD", "PFP_KEYSONLY")
SPLIT, HEADS0, KEYS_ROW = "pfp::split_keys_kernel", "pfp::heads0_kernel", "pfp::init_keys_packed_kernel"
# rows only a round after the dictionary's first one opens (in a trace of the merge stage alone)
DICT_LATER = ("pfp::build_keys_pivot_kernel", "pfp::build_keys_kernel", "pfp::build_keys32_kernel", "pfp::write_back_kernel",
              "pfp::finish_rank_kernel", "pfp::heads_kernel", "pfp::heads32_kernel")
# one phrase of 30 000 / 12 000 equal bytes: the list of the suffixes that emit is given up, the first round runs twice
FALLBACK = ("golden_n_run", "golden_gen_nblock")


def build_cases():
    cases = {}
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as fh:
        for c in json.load(fh):
            if c["n"] <= 100000:
                cases["golden_" + c["name"]] = (c["spec"], c["w"], c["p"])
    cases.update(F.TEXTS)
    return cases


CASES = build_cases()
_texts, _wants = {}, {}


def text_of(O, name):
    if name not in _texts:
        _texts[name] = make_text(CASES[name][0], O)
    return _texts[name]


def want_of(O, name, flags):
    if (name, flags) not in _wants:
        _, w, p = CASES[name]
        _wants[(name, flags)] = O.bigbwt(text_of(O, name), w, p, flags)
    return _wants[(name, flags)]


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


def run(O, ctx, name, flags, width, **env):
    """one traced call of the fused chain: outputs, trace rows, statistics"""
    _, w, p = CASES[name]
    ctx.set_index_bits(64 if width == 64 else 0)
    ctx.set_kernel_trace(True)
    try:
        with switches(**env):
            got = ctx.bigbwt(text_of(O, name), w, p, flags)
        rows = {r["name"]: r["launches"] for r in ctx.kernel_trace()}
        st = ctx.stats()
    finally:
        ctx.set_kernel_trace(False)
        ctx.set_index_bits(0)
    return got, rows, {k: st[k] for k in STATS}


def check_outputs(pkg, got, want, flags):
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


@pytest.mark.parametrize("keysonly", ("1", "0"))
@pytest.mark.parametrize("width", (32, 64))
@pytest.mark.parametrize("name", list(CASES))
def test_folded_first_round(O, pkg, dctx, pctx, name, width, keysonly):
    combined = keysonly == "1" and width == 32          # the words are (key << idx_bits | position): 32-bit positions only
    for flags in FLAGS:
        want = want_of(O, name, flags)
        for ctx in (dctx, pctx):
            got, rows, st = run(O, ctx, name, flags, width, PFP_KEYSONLY=keysonly)
            old, rows0, st0 = run(O, ctx, name, flags, width, PFP_KEYSONLY=keysonly, PFP_DICT_FOLD="0")
            check_outputs(pkg, got, want, flags)
            same_bytes(got, old)
            assert st == st0
            # each case reaches the path it is named for
            assert (SPLIT in rows) == combined and HEADS0 in rows, rows
            assert (SPLIT in rows0) == combined and HEADS0 in rows0, rows0
            sorts = 2 if name in FALLBACK else 1
            assert rows[KEYS_ROW] == sorts and rows0[KEYS_ROW] == sorts
            if combined:
                assert rows[SPLIT] == sorts and rows0[SPLIT] == sorts


def test_the_first_round_settles_the_resolved_text(O, pkg, dctx, pctx):
    """m2 == 0: traced alone, the merge stage of this text opens no row of a later round of the dictionary's sort, on either path
    (the kept-slot counts of write_back0_kernel said so; no list, no keep0)"""
    name = "golden_" + F.RESOLVED
    _, w, p = CASES[name]
    for ctx in (dctx, pctx):
        with switches():
            ps = ctx.parse(text_of(O, name), w, p, want_sai=True)
            ilist, bwlast, bwsai = ctx.bwtparse(ps["parse"], ps["last"], ps["occ"], ps["sai"])
        for env in ({"PFP_KEYSONLY": "1"}, {"PFP_KEYSONLY": "0"}, {"PFP_KEYSONLY": "1", "PFP_DICT_FOLD": "0"}):
            ctx.set_kernel_trace(True)
            try:
                with switches(**env):
                    got = ctx.merge(ps["dict"], ps["occ"], ilist, bwlast, bwsai, w, 6)
                rows = {r["name"] for r in ctx.kernel_trace()}
            finally:
                ctx.set_kernel_trace(False)
            check_outputs(pkg, got, want_of(O, name, 6), 6)
            assert HEADS0 in rows and not [r for r in DICT_LATER if r in rows], (env, rows)
