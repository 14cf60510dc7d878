"""GPU: plain mode's first round by tiles (PFP_PLAIN_TILES) and its late rank[] (PFP_PLAIN_LAZY_RANK), on the inputs of
first_round_cases.py and parse_keys_cases.py.

Every case is sorted with both switches on (the default), with each one at 0 and with both at 0; the arrays must be the same in
every byte, guard bands included, and right by tests/sacheck.py (Context.sacak_int) or tests/phrase_reference.py
(Context.bwtparse).  The kernel trace and the line PFP_TRACE_ROUNDS writes when rank[] is allocated late tell the histories apart:

  a  first round only (every group a singleton)              no later-round kernel, no line
  b  first round, then doubling rounds (no counts)           the line names round 1
  c  first round, pivot round, finisher (counts)             pfp::ipivot_keys_kernel ran, no line
  d  first round, pivot round, doubling rounds               pfp::ipivot_keys_kernel ran, the line names round 2"""
import contextlib
import functools
import os

import numpy as np
import pytest

import first_round_cases as F
import parse_keys_cases as K
import phrase_reference as PR
import sacheck

pytestmark = pytest.mark.gpu

GUARD = 64
HEADS0, WRITE0 = "pfp::heads0_kernel", "pfp::write_back0_kernel"
HEADS, WRITE = "pfp::heads_kernel", "pfp::write_back_kernel"
IPIVOT = "pfp::ipivot_keys_kernel"
LATER = (HEADS, WRITE, IPIVOT, "pfp::heads32_kernel", "pfp::heads64seg_kernel", "pfp::build_keys_kernel", "pfp::build_keys32_kernel",
         "pfp::seg_small_sort_kernel", "pfp::finish_rank_kernel", "pfp::finish_write_kernel", "pfp::scatter_settled_kernel")
OFF = ({"PFP_PLAIN_LAZY_RANK": "0"}, {"PFP_PLAIN_TILES": "0"}, {"PFP_PLAIN_LAZY_RANK": "0", "PFP_PLAIN_TILES": "0"})


def late_line(n, rnd):
    return "[pfp] doubling N=%d round=%d: rank[] allocated late and filled from the slots" % (n, rnd)


@contextlib.contextmanager
def environment(**kv):
    saved = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def traced(ctx, capfd, fn, **env):
    """fn() with the kernel trace on and the switches of env: (result, {row: launches}, what the sorter wrote to stderr)"""
    capfd.readouterr()
    ctx.set_kernel_trace(True)
    try:
        with environment(PFP_TRACE_ROUNDS="1", **env):
            out = fn()
        rows = {r["name"]: r["launches"] for r in ctx.kernel_trace()}
    finally:
        ctx.set_kernel_trace(False)
    return out, rows, capfd.readouterr().err


def guarded_sa(ctx, s):
    buf = np.full(len(s) + 2 * GUARD, 0xA5A5A5A5, dtype=np.uint32)
    ctx._check(ctx.lib.pfp_sacak_int(ctx._h, s, buf[GUARD:GUARD + len(s)], len(s), 0))
    return buf


@functools.lru_cache(maxsize=None)
def string(name):
    s = F.STRINGS[name]()
    s.setflags(write=False)
    _, head = F.first_round_groups(s)
    return s, F.unresolved(head)


@pytest.mark.parametrize("name", list(F.STRINGS))
def test_strings_by_tiles_and_with_late_ranks(ctx, capfd, name):
    s, m2 = string(name)
    n = len(s)
    buf, rows, err = traced(ctx, capfd, lambda: guarded_sa(ctx, s))
    assert (buf[:GUARD] == 0xA5A5A5A5).all() and (buf[-GUARD:] == 0xA5A5A5A5).all(), "guard bands"
    sacheck.assert_sa(s, buf[GUARD:GUARD + n], "int", name)
    assert rows.get(HEADS0) == 1 and rows.get(WRITE0) == 1, rows
    if m2 == 0:      # history a: the first round settles everything, no list is ever made
        assert not [r for r in LATER if r in rows], rows
        assert "allocated late" not in err, err
    else:            # history b: no counts, no pivot round - the first doubling round asks for rank[]
        assert late_line(n, 1) in err and err.count("allocated late") == 1, err
        assert rows.get("pfp::scatter_settled_kernel") == 1 and IPIVOT not in rows, rows
    for off in OFF:
        buf0, rows0, err0 = traced(ctx, capfd, lambda: guarded_sa(ctx, s), **off)
        assert np.array_equal(buf0, buf), off
        assert (HEADS0 in rows0) == ("PFP_PLAIN_TILES" not in off), (off, rows0)
        assert ("allocated late" in err0) == (m2 > 0 and "PFP_PLAIN_LAZY_RANK" not in off), (off, err0)
        if "PFP_PLAIN_TILES" in off:
            assert rows0.get(HEADS, 0) >= 1 and WRITE0 not in rows0, (off, rows0)


def guarded_bwtparse(ctx, p, last, occ):
    P = len(p)
    ib = np.full(P + 1 + 2 * GUARD, 0xA5A5A5A5, dtype=np.uint32)
    lb = np.full(P + 1 + 2 * GUARD, 0xA5, dtype=np.uint8)
    ctx._check(ctx.lib.pfp_bwtparse(ctx._h, p, P, last, None, occ, len(occ), ib[GUARD:GUARD + P + 1], lb[GUARD:GUARD + P + 1], None))
    return ib, lb


PARSES = dict(K.PIVOT, far_variants=F.far_variants)
# history d; of parse_keys_cases.py's inputs long_equal_cap may take either history (its share left by the pivot round is near a quarter)
DOUBLING_AFTER_PIVOT = ("far_variants",)
EITHER = ("long_equal_cap",)


@functools.lru_cache(maxsize=None)
def parse(name):
    p, last, occ = PARSES[name]()
    return p, last, occ, PR.stage2(p, last, None, occ)


@pytest.mark.parametrize("name", list(PARSES))
def test_parses_by_tiles_and_with_late_ranks(ctx, capfd, name):
    p, last, occ, want = parse(name)
    P = len(p)
    with environment(PFP_PARSE_PIVOT_MIN=str(K.PIVOT_MIN)):
        (ib, lb), rows, err = traced(ctx, capfd, lambda: guarded_bwtparse(ctx, p, last, occ))
        for band in (ib[:GUARD], ib[-GUARD:]):
            assert (band == 0xA5A5A5A5).all(), "guard bands of ilist"
        assert (lb[:GUARD] == 0xA5).all() and (lb[-GUARD:] == 0xA5).all(), "guard bands of bwlast"
        assert np.array_equal(ib[GUARD:GUARD + P + 1], want["ilist"]), "ilist"
        assert np.array_equal(lb[GUARD:GUARD + P + 1], want["bwlast"]), "bwlast"
        assert rows.get(HEADS0) == 1 and rows.get(WRITE0) == 1, rows
        assert (IPIVOT in rows) == (name != "members_63"), rows
        if name in DOUBLING_AFTER_PIVOT:
            assert late_line(P + 1, 2) in err and err.count("allocated late") == 1, err
        elif name == "members_63":      # below PFP_PARSE_PIVOT_MIN: doubling straight after the first round
            assert late_line(P + 1, 1) in err, err
        elif name not in EITHER:        # history c: the pivot round and the finisher settle it, nobody asks for rank[]
            assert "allocated late" not in err, err
        for off in OFF:
            (ib0, lb0), rows0, err0 = traced(ctx, capfd, lambda: guarded_bwtparse(ctx, p, last, occ), **off)
            assert np.array_equal(ib0, ib) and np.array_equal(lb0, lb), off
            assert (HEADS0 in rows0) == ("PFP_PLAIN_TILES" not in off), (off, rows0)
            assert ("allocated late" in err0) == ("allocated late" in err and "PFP_PLAIN_LAZY_RANK" not in off), (off, err0)


BYTE_TEXTS = {
    "abc_513": lambda: np.concatenate([np.arange(512) % 3 + 97, [0]]).astype(np.uint8),
    "abc_1500": lambda: np.concatenate([np.arange(1499) % 3 + 97, [0]]).astype(np.uint8),
    "aaa_1500": lambda: np.concatenate([np.full(1499, 97), [0]]).astype(np.uint8),
    "random_700": lambda: np.concatenate([np.random.default_rng(7).integers(1, 256, size=699), [0]]).astype(np.uint8),
}


@pytest.mark.parametrize("name", list(BYTE_TEXTS))
def test_byte_texts_in_both_index_widths(wctx, capfd, name):
    """the byte sorter is plain mode too, in the 32-bit and in the 64-bit index build"""
    s = BYTE_TEXTS[name]()
    sa, rows, err = traced(wctx, capfd, lambda: wctx.sacak(s))
    sacheck.assert_sa(s, sa, "bytes", name)
    assert rows.get(HEADS0) == 1 and rows.get(WRITE0) == 1, rows
    assert ("allocated late" in err) == (name != "random_700"), err
    for off in OFF:
        sa0, rows0, _ = traced(wctx, capfd, lambda: wctx.sacak(s), **off)
        assert np.array_equal(sa0, sa), off
        assert (HEADS0 in rows0) == ("PFP_PLAIN_TILES" not in off), (off, rows0)
