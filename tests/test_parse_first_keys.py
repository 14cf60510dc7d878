"""GPU: the integer sorter's first-round keys and the parse's pivot round, on the inputs of parse_keys_cases.py.

First round (Context.sacak_int: no counts, so no pivot round): a string without equal neighbours takes two-symbol keys of 2 sb
bits, any other the 64-bit run keys; the line PFP_TRACE_ROUNDS writes is the witness.  The suffix array is checked with
tests/sacheck.py and is, guard bands included, the array that PFP_PARSE_KEYBITS=0 (run keys always) gives.

Pivot round (Context.bwtparse with counts, PFP_PARSE_PIVOT_MIN=64): ilist and bwlast against the plain reference that
test_parse_bwt.py uses, and the same arrays again from the one-step loop (PFP_IPIVOT_BATCH=0)."""
import contextlib
import functools
import os

import numpy as np
import pytest

import parse_keys_cases as K
import phrase_reference as PR
import sacheck

pytestmark = pytest.mark.gpu

GUARD = 64
IPIVOT = "pfp::ipivot_keys_kernel"


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


@functools.lru_cache(maxsize=None)
def string(name):
    s = K.FIRST_ROUND[name][0]()
    s.setflags(write=False)
    return s


def guarded_sa(ctx, s):
    """pfp_sacak_int into the middle of a larger array: (the whole array, the suffix array inside it)"""
    buf = np.full(len(s) + 2 * GUARD, 0xA5A5A5A5, dtype=np.uint32)
    sa = buf[GUARD:GUARD + len(s)]
    ctx._check(ctx.lib.pfp_sacak_int(ctx._h, s, sa, len(s), 0))
    return buf, sa


@pytest.mark.parametrize("name", list(K.FIRST_ROUND))
def test_first_round_keys(ctx, capfd, name):
    _, layout, _ = K.FIRST_ROUND[name]
    s = string(name)
    capfd.readouterr()
    with environment(PFP_TRACE_ROUNDS="1"):
        buf, sa = guarded_sa(ctx, s)
        mid = capfd.readouterr().err
        with environment(PFP_PARSE_KEYBITS="0"):
            buf0, _ = guarded_sa(ctx, s)
        old = capfd.readouterr().err
    top = int(s.max())
    assert K.trace_line(len(s), top, layout) in mid, mid
    assert K.trace_line(len(s), top, "plain" if layout == "plain" else "run") in old, old
    assert (buf[:GUARD] == 0xA5A5A5A5).all() and (buf[-GUARD:] == 0xA5A5A5A5).all(), "guard bands"
    assert np.array_equal(buf, buf0), "the array of the 64-bit run keys, guard bands included"
    sacheck.assert_sa(s, sa, "int", name)


@functools.lru_cache(maxsize=None)
def parse(name):
    p, last, occ = K.PIVOT[name]()
    want = PR.stage2(p, last, None, occ)
    return p, last, occ, want


def guarded_bwtparse(ctx, p, last, occ):
    P = len(p)
    ib = np.full(P + 1 + 2 * GUARD, 0xA5A5A5A5, dtype=np.uint32)
    lb = np.full(P + 1 + 2 * GUARD, 0xA5, dtype=np.uint8)
    ctx._check(ctx.lib.pfp_bwtparse(ctx._h, p, P, last, None, occ, len(occ), ib[GUARD:GUARD + P + 1], lb[GUARD:GUARD + P + 1], None))
    return ib, lb


def traced(ctx, fn):
    ctx.set_kernel_trace(True)
    try:
        out = fn()
        rows = {r["name"]: r["launches"] for r in ctx.kernel_trace()}
    finally:
        ctx.set_kernel_trace(False)
    return out, rows


@pytest.mark.parametrize("name", list(K.PIVOT))
def test_pivot_round_batches(ctx, name):
    p, last, occ, want = parse(name)
    P = len(p)
    got = {}
    with environment(PFP_PARSE_PIVOT_MIN=str(K.PIVOT_MIN)):
        for batch in ("1", "0"):
            with environment(PFP_IPIVOT_BATCH=batch):
                got[batch], rows = traced(ctx, lambda: guarded_bwtparse(ctx, p, last, occ))
            # (63 members: below PFP_PARSE_PIVOT_MIN, no pivot round - the sizes on either side of it run one)
            assert (IPIVOT in rows) == (name != "members_63"), rows
    ib, lb = got["1"]
    for band in (ib[:GUARD], ib[-GUARD:]):
        assert (band == 0xA5A5A5A5).all(), "guard bands of ilist"
    assert (lb[:GUARD] == 0xA5).all() and (lb[-GUARD:] == 0xA5).all(), "guard bands of bwlast"
    assert np.array_equal(ib[GUARD:GUARD + P + 1], want["ilist"]), "ilist"
    assert np.array_equal(lb[GUARD:GUARD + P + 1], want["bwlast"]), "bwlast"
    assert np.array_equal(got["0"][0], ib) and np.array_equal(got["0"][1], lb), "PFP_IPIVOT_BATCH=0: the one-step loop"
