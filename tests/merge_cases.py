"""Which path of the merge (csrc/merge.hip, `merge_bwt`) an input takes: the inputs the parity tests already use, and the code
that runs one of them while the kernel trace records the launches.  tests/test_merge_paths.py asserts the witnesses;
tests/README.md has the table.

As a program it runs every case (or the named ones) and prints one JSON line per (case, flags, index width):

    python tests/merge_cases.py [CASE ...]
    {"case": ..., "env": {...}, "flags": 6, "width": 32, "launches": {"pfp::expand_kernel": 1, ...},
     "stats": {"hard_groups": ..., ...}, "peak": 123456}

`launches` holds the rows the merge opens (`KScope` names), `stats` the merge's fields of `Context.stats()`, `peak` the
pool's peak bytes of a context that ran nothing but this call.  Nothing is compared with a reference here - the parity tests
do that on the same inputs; two builds that print the same lines take the same path on every input.

The switches (PFP_PREC_DIRECT, PFP_BIG_BUDGET, PFP_BIG_CAP) are read per call, so one process runs them all.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from textgen import make_text  # noqa: E402

FLAG_SETS = (0, 1, 6)          # BWT only, FLAG_SA (dense), FLAG_SSA | FLAG_ESA (sparse)
WIDTHS = (32, 64)

# the rows `merge_bwt` opens, and the one library sort it tags
MERGE_ROWS = tuple("pfp::" + k for k in (
    "pprec16_kernel", "slot_records_kernel", "slot_payload_kernel", "slot_loc_kernel", "group_flags_kernel",
    "hard_classify_kernel", "hard_minor_fill_kernel", "expand_kernel", "expand_heavy_kernel", "hard_minor_kernel",
    "hard_groups_kernel", "hard_sort_kernel", "hard_big_kernel", "big_keys_kernel", "big_place_kernel",
    "run_bitmap_kernel", "word_sa_kernel", "unit_edges_kernel"))
MERGE_SORT_TAG = "[large hard groups]"
MERGE_STATS = ("hard_groups", "hard_chars", "hard_big_groups", "hard_max_chars", "hard_max_members", "hard_minor_groups",
               "hard_minor_chars")


def copies_text(ncopies=1200):
    """the text of test_large_hard_groups_without_a_dominating_char: ncopies copies of a random sequence, 40 of them mutated"""
    rng = np.random.default_rng(5)
    base = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1500)]
    copies = np.tile(base, (ncopies, 1))
    for c_ in rng.integers(0, ncopies, size=40):
        copies[c_, rng.integers(0, 1500)] = ord("N")
    return copies.reshape(-1).copy()


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as fh:
        return json.load(fh)


def build_cases():
    """{name: dict(text=callable(O), w, p, env)} in the order they are printed"""
    cases = {}
    for c in _golden()[:8]:
        for tag, env in (("", {}), ("/direct0", {"PFP_PREC_DIRECT": "0"}), ("/direct1", {"PFP_PREC_DIRECT": "1"})):
            cases["golden_" + c["name"] + tag] = dict(text=lambda O, s=c["spec"]: make_text(s, O), w=c["w"], p=c["p"], env=env)
    for tag, env in (("", {}), ("/budget6000", {"PFP_BIG_BUDGET": "6000"}), ("/budget100", {"PFP_BIG_BUDGET": "100"}),
                     ("/cap2", {"PFP_BIG_CAP": "2"})):
        cases["copies1200" + tag] = dict(text=lambda O: copies_text(1200), w=4, p=11, env=env)
    # the same with 400 copies (no existing test reaches hard_sort_kernel): two words of ~400 occurrences that share a suffix make a
    # hard group of 513 .. 1024 occurrences, which one wave sorts in LDS
    cases["copies400"] = dict(text=lambda O: copies_text(400), w=4, p=11, env={})
    cases["snp48"] = dict(text=lambda O: O.gen_fasta(100000, 48, 0.01, 77), w=10, p=100, env={})
    return cases


CASES = build_cases()
# two virtual ranks on one device (bigbwt_amd.dist.simulate, as tests/test_distributed.py drives them): the suffix array of
# the dictionary replicated - every rank emits a slice [out_lo, out_hi) of the whole order - or sharded by key range - every
# rank holds one contiguous range of slots
DIST_CASES = {"dist2_slice": False, "dist2_range": True}

_texts = {}


def text_of(O, name):
    key = name.split("/")[0]
    if key not in _texts:
        _texts[key] = CASES[name]["text"](O)
    return _texts[key]


class _Env:
    """the case's switches in os.environ for the duration of a call"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in ("PFP_PREC_DIRECT", "PFP_BIG_BUDGET", "PFP_BIG_CAP")}
        for k in self.saved:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def merge_rows(trace_rows):
    return {r["name"]: r["launches"] for r in trace_rows if r["name"] in MERGE_ROWS or r["name"].endswith(MERGE_SORT_TAG)}


def _record(ctx, **head):
    st = ctx.stats()
    return dict(head, launches=merge_rows(ctx.kernel_trace()), stats={k: st[k] for k in MERGE_STATS},
                peak=ctx.mem_stats()["peak"])


def run_case(pkg, O, name, flags, width):
    """one call of the fused chain in a context of its own; returns the record that main() prints"""
    c = CASES[name]
    text = text_of(O, name)
    with pkg.Context(0) as ctx, _Env(c["env"]):
        ctx.set_index_bits(64 if width == 64 else 0)
        ctx.set_kernel_trace(True)
        ctx.bigbwt(text, c["w"], c["p"], flags)
        rec = _record(ctx, case=name, env=c["env"], flags=flags, width=width)
        ctx.set_kernel_trace(False)
        if os.environ.get("PFP_POOL_DEBUG"):      # (a context of its own: the checking pool's bands are looked at here)
            ctx.debug_check()
    return rec


def run_dist_case(pkg, O, name, flags, width):
    """two virtual ranks; returns one record per rank"""
    import importlib

    import torch
    d = importlib.import_module("bigbwt_amd.dist")
    text = O.gen_fasta(60000, 8, 0.003, 59)          # (test_baseline_flag_sets_across_ranks)
    n, R = len(text), 2
    cuts = [0, n // 2 - 2, n]
    ctxs = [pkg.Context(0) for _ in range(R)]
    try:
        with _Env({}):
            for c in ctxs:
                c.set_index_bits(64 if width == 64 else 0)
                c.set_kernel_trace(True)
            shards = [torch.from_numpy(text[cuts[r]:cuts[r + 1]].copy()).cuda() for r in range(R)]
            res = d.simulate(ctxs, shards, 10, 100, flags, halo=8192, shard_sa=DIST_CASES[name])
            return [_record(ctxs[r], case=name, rank=r, sa_shares=res[r]["stats"]["sa_shares"], env={}, flags=flags, width=width)
                    for r in range(R)]
    finally:
        for c in ctxs:
            c.close()


def main(argv):
    import __graft_entry__ as entry
    names = argv[1:] or list(CASES) + list(DIST_CASES)
    unknown = [n for n in names if n not in CASES and n not in DIST_CASES]
    if unknown:
        print("unknown: %s; cases: %s" % (unknown, " ".join(list(CASES) + list(DIST_CASES))), file=sys.stderr)
        return 2
    pkg = entry.load_package()
    O = entry.load_oracle()
    for name in names:
        for flags in FLAG_SETS:
            for width in WIDTHS:
                try:      # an error of the library (a GPU fault among them): nothing more is started
                    recs = run_dist_case(pkg, O, name, flags, width) if name in DIST_CASES else [run_case(pkg, O, name, flags, width)]
                except Exception as ex:
                    print(json.dumps(dict(case=name, flags=flags, width=width, error=f"{type(ex).__name__}: {ex}")), flush=True)
                    return 3
                for rec in recs:
                    print(json.dumps(rec, sort_keys=True), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
