"""Small inputs for the share sorters of csrc/sufsort.hip (sort_dict_suffixes_range, sort_int_suffixes_range: one rank's key range
of the dictionary's and of the parse's suffix array), run as R virtual ranks on one GPU through dist.simulate with the kernel
trace on in every rank's context.  tests/test_distributed.py asserts what the shares must add up to on these same runs;
tests/README.md has the note.

As a program it runs every case (or the named ones) in both index widths and prints one JSON line per (case, width, rank):

    PFP_TRACE_HOST=1 python tests/share_cases.py [CASE ...]
    {"case": "copies_R3", "width": 32, "rank": 0, "glob": {"slots": ..., "slot_base": ..., "complete": ..., "emits": ..., "rounds": ..., ...},
     "parse": {"entries": ..., "slot_base": ..., "complete": ..., "rounds": ...}, "phrases": 18750, "sa_shares": 3, "parse_shares": 3,
     "trace": {"pfp::range_flags_cmp4_kernel": [1, 123456], ...}, "peak": 123456, "waits": 57, "sha256": "..."}

`glob` is the rank's report of its (last) dictionary sort, `parse` what pfp_dist_parse_sort reported (null where it was not
called), `phrases` the length of the whole parse, `trace` holds (launches, algo_bytes) of every row of Context.kernel_trace()
over the whole chain, `peak` the pool's peak bytes, `waits` the host waits on the stream over the context's life as
PFP_TRACE_HOST=1 makes the library print them when the context goes (null without it), `sha256` a digest of the rank's pieces
of the output files and of their offsets.  Nothing is compared with a reference here: two builds that print the same lines cut,
launch, wait, allocate and answer alike.
"""
import functools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from fm_host_cases import _close_and_count_waits, digest  # noqa: E402

FLAG_SA, FLAG_SSA, FLAG_ESA = 1, 2, 4
EMPTY_RUN = 16000      # case (d): length of the run of one letter


@functools.lru_cache(maxsize=None)
def tiny_text():
    """the 2.8 KB text of test_many_ranks_on_a_tiny_dictionary: a dictionary of ~120 suffixes"""
    return np.frombuffer((b"ACGTACGTTTGACA" * 40 + b"GGGTTTAAACCC" * 30) * 3, dtype=np.uint8).copy()


@functools.lru_cache(maxsize=None)
def run_text(O, run):
    """3 KB of random DNA on either side of `run` copies of one letter - the first of ACGT whose window is no trigger under
    -w 4 -p 11, so that the run stays inside one phrase: one dictionary word then holds `run` suffixes that no first-round key
    tells apart, more than a quarter of all of them.  Returns (text, cuts): the run lies inside the second of four shards."""
    rng = np.random.default_rng(run)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    letter = next(c for c in b"ACGT" if O.kr_window(bytes([c]) * 4) % 11 != 0)
    text = np.concatenate([rng.choice(acgt, 3000), np.full(run, letter, np.uint8), rng.choice(acgt, 3000)])
    return np.ascontiguousarray(text, dtype=np.uint8), (0, 1500, 3000 + run + 750, 3000 + run + 1875, len(text))


def _even(n, R):
    return tuple(n * r // R for r in range(R + 1))


def _run_case(run):
    def build(O):
        text, cuts = run_text(O, run)
        return dict(text=text, cuts=cuts, w=4, p=11, flags=FLAG_SA, halo=1 << 16, window_hash=False)
    return build


# name -> build(O) -> dict(text, cuts, w, p, flags, halo[, window_hash, max_phrase])
CASES = {
    # (a) many ranks on a tiny dictionary: shares of a few dozen slots, emit counts from 1 up
    "tiny_R4": lambda O: dict(text=tiny_text(), cuts=_even(len(tiny_text()), 4), w=4, p=11, flags=FLAG_SA, halo=256, window_hash=False),
    "tiny_R6": lambda O: dict(text=tiny_text(), cuts=_even(len(tiny_text()), 6), w=4, p=11, flags=FLAG_SA, halo=256, window_hash=False),
    # (b) a collection of copies: both the dictionary's and the parse's suffix array are sorted in shares
    "copies_R3": lambda O: (lambda t: dict(text=t, cuts=_even(len(t), 3), w=10, p=100, flags=FLAG_SSA | FLAG_ESA, halo=8192))(
        O.gen_fasta(150000, 12, 0.002, 61)),
    # (c) an N run kept as one giant phrase: a key range cannot finish alone, every rank falls back to the replicated sort
    "fallback_R2": lambda O: (lambda t: dict(text=t, cuts=_even(len(t), 2), w=10, p=100, flags=0, halo=1 << 17, max_phrase=0))(
        O.gen_fasta(120000, 2, 0.001, 47, n_blocks=[(20000, 80000)])),
    # (d) meant to leave one of four ranks an empty share of the dictionary (see run_text).  It does not get that far: the run's
    # suffixes agree for longer than a pivot round or the comparison finisher looks, no key range finishes alone, and every rank
    # falls back to the replicated sort (runs of 4000 and of 16000 alike).  What it does pin: splitters whose boundaries repeat.
    "run_R4": _run_case(EMPTY_RUN),
}

_PIECES = ("bwt", "sa", "sa5", "ssa", "esa")


def run_case(pkg, O, name, width, profiling=False):
    """one case in one index width: R contexts, one dist.simulate; returns the records that main() prints, rank by rank (each
    with "total_ms" of its trace rows and its stage times next to what the docstring lists where `profiling` is on)"""
    import importlib
    import torch
    d = importlib.import_module("bigbwt_amd.dist")
    c = CASES[name](O)
    text, cuts = c["text"], c["cuts"]
    R = len(cuts) - 1
    ctxs = [pkg.Context(0) for _ in range(R)]
    pinfo = [None] * R
    try:
        for r, ctx in enumerate(ctxs):
            ctx.set_index_bits(width if width == 64 else 0)
            if "window_hash" in c:
                ctx.set_window_hash(c["window_hash"])
            if "max_phrase" in c:
                ctx.set_max_phrase(c["max_phrase"])
            if profiling:
                ctx.set_profiling(True)

            def parse_sort(*a, _r=r, _call=ctx.dist_parse_sort):      # (dist.phases keeps the report to itself)
                pinfo[_r] = _call(*a)
                return pinfo[_r]
            ctx.dist_parse_sort = parse_sort
            ctx.set_kernel_trace(True)
        shards = [torch.from_numpy(text[cuts[r]:cuts[r + 1]].copy()).cuda() for r in range(R)]
        res = d.simulate(ctxs, shards, c["w"], c["p"], c["flags"], halo=c["halo"])
        recs = []
        for r, ctx in enumerate(ctxs):
            rows = ctx.kernel_trace()
            ctx.set_kernel_trace(False)
            st = res[r]["stats"]
            pieces = [res[r][k].cpu().numpy() for k in _PIECES if res[r].get(k) is not None]
            offs = np.array([res[r]["lo"], res[r]["hi"]] + [res[r].get(k + "_off", -1) for k in _PIECES], dtype=np.int64)
            rec = dict(case=name, width=width, rank=r, glob=st["glob"], parse=pinfo[r], phrases=st["phrases_total"],
                       sa_shares=st["sa_shares"], parse_shares=st["parse_shares"],
                       trace={x["name"]: [x["launches"], x["algo_bytes"]] for x in rows}, peak=ctx.mem_stats()["peak"],
                       sha256=digest(pieces + [offs]))
            if profiling:
                s = ctx.stats()
                rec["total_ms"] = {x["name"]: x["total_ms"] for x in rows}
                rec["ms_sa"] = s["ms_sa_dict"] + s["ms_sa_parse"]
            recs.append(rec)
    except BaseException:
        for ctx in ctxs:
            ctx.close()
        raise
    for rec, ctx in zip(recs, ctxs):
        rec["waits"] = _close_and_count_waits(ctx)
    return recs


def main(argv):
    import __graft_entry__ as entry
    names = argv[1:] or list(CASES)
    unknown = [n for n in names if n not in CASES]
    if unknown:
        print("unknown: %s; cases: %s" % (unknown, " ".join(CASES)), file=sys.stderr)
        return 2
    pkg = entry.load_package()
    O = entry.load_oracle()
    for name in names:
        for width in (32, 64):
            try:      # an error of the library (a GPU fault among them): nothing more is started
                recs = run_case(pkg, O, name, width)
            except Exception as ex:
                print(json.dumps(dict(case=name, width=width, error=f"{type(ex).__name__}: {ex}")), flush=True)
                return 3
            for rec in recs:
                print(json.dumps(rec, sort_keys=True), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
