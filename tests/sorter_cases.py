"""Directed inputs for the suffix sorters of csrc/sufsort.hip, one per path of `doubling`, and the code that runs one of them
against the two references (the oracle's prefix-doubling sorter and the linear checker of sacheck.py) while the kernel trace
records which launches happened.  tests/test_suffix_sorters.py asserts the witnesses; tests/README.md has the table.

As a program it runs the named cases in both index widths and prints one JSON line per (case, width):

    python tests/sorter_cases.py CASE [CASE ...]
    {"case": ..., "width": 32, "ok": true, "error": null, "witnesses": {"pfp::build_keys_pivot_kernel": 1, ...}}

which is how the switches that force an alternative path (PFP_NO_FINFLAG, PFP_PIVOT_CAP, ...) get tested on many cases at once:
a fresh child process per switch, with the switch in its environment from the start.  (The sorter reads every switch at each
call, so a case can also set one around its own run: the `env` of a case.)  The exit status is 1 when a case differed from a
reference.

A gsacak collection is words of bytes >= 2, each followed by a 1, and one final 0.  "F families of V variants of L bytes with k
substitutions" gives suffix groups of known size (V) and depth (the distance to the next substitution).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from sacheck import sa_error  # noqa: E402

ALPHA20 = np.arange(65, 85, dtype=np.uint8)      # twenty letters: a first-round key covers about fifteen of them
CHECKER_MIN = 1 << 20                            # above this many entries the checker gives its second opinion


# ---------------------------------------------------------------------------------------------- builders
def family_block(rng, F, V, L, k, lo=0, hi=None, alphabet=ALPHA20):
    """F random base words of L bytes, V copies of each, k random substitutions per copy at offsets [lo, hi); every word
    followed by its separator"""
    base = rng.choice(alphabet, size=(F, L))
    w = np.repeat(base, V, axis=0)
    hi = L if hi is None else hi
    rows = np.arange(F * V)
    for _ in range(k):
        w[rows, rng.integers(lo, hi, size=F * V)] = rng.choice(alphabet, size=F * V)
    return np.concatenate([w, np.ones((F * V, 1), np.uint8)], axis=1).reshape(-1)


def collection(*blocks):
    return np.ascontiguousarray(np.concatenate(list(blocks) + [np.zeros(1, np.uint8)]), dtype=np.uint8)


def filler(rng, nbytes, L=100):
    """random words: the first round settles (nearly) all of their suffixes"""
    return family_block(rng, nbytes // (L + 1), 1, L, 0)


def byte_text(kind, n):
    """n bytes, the last one the unique 0"""
    m = n - 1
    rng = np.random.default_rng(n)
    if kind == "a^n":
        t = np.full(m, 97, np.uint8)
    elif kind == "(ab)^n":
        t = np.tile(np.frombuffer(b"ab", np.uint8), m // 2 + 1)[:m]
    elif kind == "fibonacci":
        a, b = b"b", b"a"
        while len(b) < m:
            a, b = b, b + a
        t = np.frombuffer(b[:m], np.uint8)
    elif kind == "period37":
        t = np.tile(rng.integers(3, 256, size=37).astype(np.uint8), m // 37 + 1)[:m].copy()
        if m:
            t[(2 * m) // 3] = 3 + (int(t[(2 * m) // 3]) + 97) % 253      # (another value of 3..255)
    elif kind == "all253":
        t = rng.integers(3, 256, size=m).astype(np.uint8)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(np.concatenate([t, np.zeros(1, np.uint8)]), dtype=np.uint8)


BYTE_KINDS = ("a^n", "(ab)^n", "fibonacci", "period37", "all253")
BYTE_SIZES = (1, 2, 3, 255, 256, 257, (1 << 16) - 1, (1 << 16) + 1, (1 << 20) - 1, (1 << 20) + 1, 2_000_000)


def int_text(shift):
    """symbols 1..50 with two long runs of one symbol (a real parse showed a run of 300 000) and a periodic stretch, every
    non-zero symbol moved up by `shift`; ends in the unique 0"""
    rng = np.random.default_rng(3)
    per = np.tile(rng.integers(1, 5, size=100), 300)
    s = np.concatenate([rng.integers(1, 51, size=150_000), np.full(300_000, 7), rng.integers(1, 51, size=60_000), per,
                        np.full(50_000, 7), rng.integers(1, 51, size=40_000), [50]]).astype(np.uint64)
    s += np.uint64(shift)
    return np.ascontiguousarray(np.concatenate([s, [0]]).astype(np.uint32))


def parse_copies(copies, S, rare_per_copy, seed):
    """a hand-built parse: symbol 1 once at the start (the smallest word starts the text), then `copies` copies of one
    sequence of S distinct common symbols, every copy with `rare_per_copy` places replaced by a symbol of its own;
    returns (parse, last, occ) with occ the true counts of the symbols 1..d"""
    rng = np.random.default_rng(seed)
    base = rng.permutation(S).astype(np.uint32) + 2
    body = np.tile(base, copies)
    nr = copies * rare_per_copy
    at = (np.repeat(np.arange(copies), rare_per_copy) * S + rng.integers(0, S, size=nr)).astype(np.int64)
    at = np.unique(at)
    body[at] = np.arange(len(at), dtype=np.uint32) + np.uint32(S + 2)
    parse = np.concatenate([np.ones(1, np.uint32), body]).astype(np.uint32)
    occ = np.bincount(parse)[1:].astype(np.uint32)
    # (a common symbol whose every copy was replaced would have a count of 0: no real parse has that)
    assert occ.min() >= 1
    last = rng.integers(65, 69, size=len(parse)).astype(np.uint8)
    return parse, last, occ


# ---------------------------------------------------------------------------------------------- cases
# name -> dict(kind, build, expect, env).  expect(width) -> W(...): what the kernel trace of the case must show.
# A row matches a name exactly, or the name followed by a sort tag " [...]".
PIVOT = "pfp::build_keys_pivot_kernel"
SMALL = "pfp::seg_small_sort_kernel"
SEG32 = "rocprim::segmented_radix_sort_pairs<u32,u32>"
SEG64 = "rocprim::segmented_radix_sort_pairs<u64,u32>"
FINISH = "pfp::finish_rank_kernel"
DBL = "pfp::build_keys_kernel"
DBL32 = "pfp::build_keys32_kernel"
SCATTER = "pfp::scatter_settled_kernel"
REPAIR = "pfp::repair_ranks_kernel"
SPLIT = "pfp::split_keys_kernel"
IPIVOT = "pfp::ipivot_keys_kernel"
INT_RUN = "pfp::init_keys_int_run_kernel"
INT_PLAIN = "pfp::init_keys_int_kernel"
BYTES0 = "pfp::init_keys_bytes_kernel"
PACKED0 = "pfp::init_keys_packed_kernel"
FINISH_WRITE = "pfp::finish_write_kernel"
KEYS0 = "rocprim::radix_sort_keys<u64> [dictionary, first round]"


def W(present, absent=(), minimum=None, fewer=(), maximum=None):
    """what a case expects of the kernel trace: rows that must be there, rows that must not, least and most launches per row,
    and pairs (a, b): fewer launches of a than of b"""
    return dict(present=list(present), absent=list(absent), minimum=dict(minimum or {}), maximum=dict(maximum or {}), fewer=list(fewer))


def later_pairs(width):
    """the device-wide pair sort of a later dictionary round (the wide build carries 64-bit positions)"""
    return ("rocprim::radix_sort_pairs<u64,u64>" if width == 64 else "rocprim::radix_sort_pairs<u64,u32>") + " [dictionary, later rounds]"


def first_pairs(width):
    return ("rocprim::radix_sort_pairs<u64,u64>" if width == 64 else "rocprim::radix_sort_pairs<u64,u32>") + " [dictionary, first round]"


def _rng(seed):
    return np.random.default_rng(seed)


CASES = {}


def case(name, kind, build, expect, env=None):
    CASES[name] = dict(kind=kind, build=build, expect=expect, env=env or {})


# pivot round, device-wide sort.  Families of 40: the first pivot round has m / ngrp above kSmallSeg / 2 = 32 (kSmallSeg / 4 = 16
# in the wide build) and fewer than 2^20 unresolved suffixes, so neither the placement in LDS nor the segmented sort is chosen
# for it (what it leaves - smaller groups - may be placed in LDS: fewer such launches than pivot rounds)
case("fam_moderate", "gsa", lambda: collection(family_block(_rng(1), 100, 40, 150, 2)),
     lambda w: W([PACKED0, PIVOT, later_pairs(w)], [SEG32, DBL, DBL32], fewer=[(SMALL, PIVOT)]))
# pivot rounds, small families placed in LDS: m / ngrp <= kSmallSeg / 2 (kSmallSeg / 4 wide), every family has 8 members;
# no round needs a device-wide sort
case("fam_small", "gsa", lambda: collection(family_block(_rng(2), 1000, 8, 150, 2)),
     lambda w: W([PIVOT, SMALL], [SEG32, later_pairs(w), DBL, DBL32]))
# the placement gives up: one family of 100 (> kSmallSeg = 64) among families of 8.  32-bit build: the long groups go through
# one pair sort of their own in the same round; wide build: the whole round goes to the device-wide sort
case("fam_small_one_big", "gsa", lambda: collection(family_block(_rng(3), 1000, 8, 150, 2), family_block(_rng(4), 1, 100, 150, 2)),
     lambda w: W([PIVOT, SMALL, later_pairs(w)], [SEG32]))
# pivot round, segmented sort: m >= 2^20 unresolved, average family >= kSegMinAvg = 24, longest <= 2^15
case("fam_segmented", "gsa", lambda: collection(family_block(_rng(5), 300, 40, 150, 2)),
     lambda w: W([PIVOT, SEG32]))
# the same with one family above 2^15 (40 000 words that differ in their first four bytes only): the device-wide sort
case("fam_segmented_giant", "gsa",
     lambda: collection(family_block(_rng(6), 300, 40, 100, 2), family_block(_rng(7), 1, 40000, 40, 2, 0, 4)),
     lambda w: W([PIVOT, later_pairs(w)], [SEG32]))
# comparison finisher: after the first pivot round (window SorterSwitches::pivot_cap = 512) what is left - variants that agree for more than
# 512 bytes - is below kFinishMax = 2^17, in groups of 4 <= kFinishGrp, with common prefixes below kFinishCmp = 8192
case("finisher", "gsa", lambda: collection(family_block(_rng(8), 20, 4, 1500, 2)),
     lambda w: W([PIVOT, FINISH, FINISH_WRITE], [DBL, DBL32], maximum={PIVOT: 1}))
# the finisher refuses a group above kFinishGrp = 64 (one family of 100) and writes nothing: the rounds go on
case("finisher_big_group", "gsa", lambda: collection(family_block(_rng(9), 1, 100, 1500, 2)),
     lambda w: W([PIVOT, FINISH, DBL], [FINISH_WRITE]))
# window growth 512 -> 2 K -> 8 K (kPivCapMax - 16), then doubling: two variants of two 9 000-byte words that differ only
# beyond offset 8 700, in 2 MB of filler (a wider window is tried only while m x window < 128 N: 36 000 suffixes at most).
# The finisher refuses the common prefixes above kFinishCmp = 8192.  The doubling rounds are lazy (m * kLazyRatio <= N: no
# scatter of the settled ranks); their groups of two are "small groups" in the 32-bit build
case("deep_growth", "gsa", lambda: collection(filler(_rng(10), 2_000_000), family_block(_rng(11), 2, 2, 9000, 2, 8700, 9000)),
     lambda w: W([PIVOT, FINISH, REPAIR, DBL32 if w == 32 else DBL], [SCATTER, FINISH_WRITE], {PIVOT: 3}))
# doubling with the ranks scattered: nearly all of the dictionary agrees beyond the 512-byte window, no wider window is
# affordable (m x 2048 >= 128 N), and m * kLazyRatio > N.  Groups of 8: build_keys32_kernel in the 32-bit build
case("deep_scatter", "gsa", lambda: collection(family_block(_rng(12), 16, 8, 5000, 2)),
     lambda w: W([PIVOT, SCATTER, REPAIR, DBL32 if w == 32 else DBL], [], maximum={PIVOT: 1}))
# doubling, lazy lookup, groups of 60 (no small-group keys in either build): one family of 60 x 3 000 bytes that differ beyond
# offset 2 900 leaves 143 000 suffixes after the 512-byte window - above kFinishMax, too many for a wider window (m >= N / 16),
# few enough for the lazy lookup (m <= N / kLazyRatio)
case("deep_lazy", "gsa", lambda: collection(filler(_rng(13), 1_420_000), family_block(_rng(14), 1, 60, 3000, 2, 2900, 3000)),
     lambda w: W([PIVOT, DBL, REPAIR], [SCATTER, DBL32], maximum={PIVOT: 1}))
# keys-only first round (PFP_KEYSONLY=1; 32-bit build only): dictionaries below 2^20, between 2^20 and 2^22
# (sort_keys_db sorts the whole word there) and above 2^22 bytes
_ko = lambda w: W([SPLIT, KEYS0, PIVOT], [first_pairs(w)]) if w == 32 else W([PIVOT, first_pairs(w)], [SPLIT, KEYS0])      # noqa: E731
case("keysonly_below_2^20", "gsa", lambda: collection(family_block(_rng(15), 80, 40, 150, 2)), _ko, {"PFP_KEYSONLY": "1"})
case("keysonly_above_2^20", "gsa", lambda: collection(family_block(_rng(16), 300, 40, 150, 2)), _ko, {"PFP_KEYSONLY": "1"})
case("keysonly_above_2^22", "gsa", lambda: collection(family_block(_rng(17), 720, 40, 150, 2)), _ko, {"PFP_KEYSONLY": "1"})

# integer sorter: run keys while the largest symbol is below 2^29 (64 - 2 * sb >= 6), plain keys from there on; the same string
# moved up, the last one with every symbol above 2^31
case("int_runs", "int", lambda: int_text(0), lambda w: W([INT_RUN], [INT_PLAIN]))
case("int_runs_max_2^29-1", "int", lambda: int_text((1 << 29) - 1 - 50), lambda w: W([INT_RUN], [INT_PLAIN]))
case("int_plain_max_2^29", "int", lambda: int_text((1 << 29) - 50), lambda w: W([INT_PLAIN], [INT_RUN]))
case("int_plain_above_2^31", "int", lambda: int_text((1 << 32) - 1 - 50), lambda w: W([INT_PLAIN], [INT_RUN]))
# the 1.5 M-symbol string of the parse cases below, without its counts: no pivot rounds
case("int_copies", "int", lambda: np.concatenate([parse_copies(300, 5000, 20, 21)[0], np.zeros(1, np.uint32)]),
     lambda w: W([INT_RUN], [IPIVOT]))

# parse pivot rounds (only parse_bwt hands the sorter the counts): 2^16 phrases or more, groups of 300 -> segmented sort of
# 64-bit keys; groups of 8 (<= kSmallSeg / 2) -> placed in LDS; a small parse with PFP_PARSE_PIVOT_MIN=64,
# and the same parse without it: no pivot round
case("parse_segmented", "parse", lambda: parse_copies(300, 5000, 20, 21), lambda w: W([INT_RUN, IPIVOT, SEG64]))
case("parse_small_groups", "parse", lambda: parse_copies(8, 30000, 20, 22), lambda w: W([INT_RUN, IPIVOT, SMALL], [SEG64]))
case("parse_tiny_forced", "parse", lambda: parse_copies(40, 200, 3, 23), lambda w: W([IPIVOT, SEG64]), {"PFP_PARSE_PIVOT_MIN": "64"})
case("parse_tiny_default", "parse", lambda: parse_copies(40, 200, 3, 23), lambda w: W([INT_RUN], [IPIVOT]))

for _k in BYTE_KINDS:
    for _n in BYTE_SIZES:
        case(f"bytes_{_k}_{_n}", "bytes", (lambda k=_k, n=_n: byte_text(k, n)), lambda w: W([BYTES0]))

DICT_CASES = [n for n, c in CASES.items() if c["kind"] == "gsa"]
INT_CASES = [n for n, c in CASES.items() if c["kind"] == "int"]
PARSE_CASES = [n for n, c in CASES.items() if c["kind"] == "parse"]
BYTE_CASES = [n for n, c in CASES.items() if c["kind"] == "bytes"]


# ---------------------------------------------------------------------------------------------- running a case
def row_launches(trace, name):
    """launches of the trace rows called `name`, with or without a sort tag"""
    return sum(v for k, v in trace.items() if k == name or k.startswith(name + " ["))


def witness_errors(trace, expect):
    n = lambda name: row_launches(trace, name)      # noqa: E731
    errs = [f"witness missing: {w}" for w in expect["present"] if n(w) == 0]
    errs += [f"launched though its path should not run: {w}" for w in expect["absent"] if n(w) > 0]
    errs += [f"{w}: {n(w)} launches, expected at least {k}" for w, k in expect["minimum"].items() if n(w) < k]
    errs += [f"{w}: {n(w)} launches, expected at most {k}" for w, k in expect["maximum"].items() if n(w) > k]
    errs += [f"{a}: {n(a)} launches, expected fewer than the {n(b)} of {b}" for a, b in expect["fewer"] if n(a) >= n(b)]
    return errs


_oracle_cache = {}


def reference(O, name):
    """(input, the oracle's outputs) of a case, computed once per process"""
    if name not in _oracle_cache:
        c = CASES[name]
        data = c["build"]()
        if c["kind"] == "gsa":
            ref = O.gsacak(data, want_lcp=True)
        elif c["kind"] == "bytes":
            ref = O.sacak(data)
        elif c["kind"] == "int":
            ref = O.sacak_int(data)
        else:
            ref = O.bwtparse(data[0], data[1], None, data[2])[:2]
        _oracle_cache[name] = (data, ref)
    return _oracle_cache[name]


def _traced(ctx, fn):
    ctx.set_kernel_trace(True)
    try:
        out = fn()
        trace = {r["name"]: r["launches"] for r in ctx.kernel_trace()}
    finally:
        ctx.set_kernel_trace(False)
    return out, trace


def run_case(ctx, O, name, width):
    """run one case in one index width against the oracle (and the checker); returns the kernel trace {row: launches} of
    the first sort.  Raises AssertionError with the first difference."""
    c = CASES[name]
    data, ref = reference(O, name)
    saved = {k: os.environ.get(k) for k in c["env"]}
    os.environ.update(c["env"])
    ctx.set_index_bits(64 if width == 64 else 0)
    try:
        if c["kind"] == "gsa":
            osa, olcp = ref
            sa, trace = _traced(ctx, lambda: ctx.gsacak(data))
            assert np.array_equal(sa, osa), f"{name}: gsacak differs from the oracle at slot {int(np.flatnonzero(sa != osa)[0])}"
            if len(data) > CHECKER_MIN:
                err = sa_error(data, sa, "gsa")
                assert err is None, f"{name}: checker: {err}"
            assert np.array_equal(ctx.gsacak64(data), osa.astype(np.uint64)), f"{name}: gsacak64 differs from the oracle"
            word_of = np.concatenate([[0], np.cumsum(data == 1)[:-1]])
            for wide in (False, True):
                gsa, glcp, gda = ctx.gsacak_lcp_da(data, wide)
                assert np.array_equal(gsa.astype(np.uint32), osa), f"{name}: gsacak_lcp_da(wide={wide}): SA differs"
                assert np.array_equal(glcp.astype(np.int32), olcp), f"{name}: gsacak_lcp_da(wide={wide}): LCP differs"
                assert np.array_equal(gda.astype(np.int64), word_of[osa]), f"{name}: gsacak_lcp_da(wide={wide}): DA differs"
        elif c["kind"] == "bytes":
            sa, trace = _traced(ctx, lambda: ctx.sacak(data))
            assert np.array_equal(sa, ref), f"{name}: sacak differs from the oracle"
            err = sa_error(data, sa, "bytes")
            assert err is None, f"{name}: checker: {err}"
            assert np.array_equal(ctx.sacak64(data), ref.astype(np.uint64)), f"{name}: sacak64 differs from the oracle"
        elif c["kind"] == "int":
            k = int(data.max()) + 1
            sa, trace = _traced(ctx, lambda: ctx.sacak_int(data, k))
            assert np.array_equal(sa, ref), f"{name}: sacak_int differs from the oracle"
            if len(data) > CHECKER_MIN:
                err = sa_error(data, sa, "int")
                assert err is None, f"{name}: checker: {err}"
            assert np.array_equal(ctx.sacak_int64(data, k), ref.astype(np.uint64)), f"{name}: sacak_int64 differs from the oracle"
        else:
            parse, last, occ = data
            (ilist, bwlast, _), trace = _traced(ctx, lambda: ctx.bwtparse(parse, last, occ))
            assert np.array_equal(ilist, ref[0]), f"{name}: ilist differs from the oracle"
            assert np.array_equal(bwlast, ref[1]), f"{name}: bwlast differs from the oracle"
    finally:
        ctx.set_index_bits(0)
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return trace


def main(argv):
    import __graft_entry__ as entry
    names = argv[1:]
    unknown = [n for n in names if n not in CASES]
    if unknown or not names:
        print("usage: sorter_cases.py CASE [CASE ...]; unknown: %s; cases: %s" % (unknown, " ".join(CASES)), file=sys.stderr)
        return 2
    pkg = entry.load_package()
    O = entry.load_oracle()
    bad = 0
    with pkg.Context(0) as ctx:
        for name in names:
            for width in (32, 64):
                trace, err = {}, None
                try:
                    trace = run_case(ctx, O, name, width)
                except AssertionError as ex:
                    err = str(ex)
                    bad += 1
                except Exception as ex:      # an error of the library (a GPU fault among them): nothing more is started
                    print(json.dumps(dict(case=name, width=width, ok=False, error=f"{type(ex).__name__}: {ex}", witnesses={})), flush=True)
                    return 3
                print(json.dumps(dict(case=name, width=width, ok=err is None, error=err, witnesses=trace)), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
