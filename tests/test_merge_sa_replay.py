"""Sparse SA (-s / -e): the second round of the merge (csrc/merge.hip, `sa_round`) replays the ranks that the first round
staged for the hard groups without a dominating char, instead of ranking their occurrences again.

Every case runs in a context with PFP_DEBUG=1 - a run boundary of the BWT that received no SA value fails the call
(`check_boundaries_set`), and so does a staged entry that the replay reads and nobody wrote - and compares the sampled SA
files with the CPU oracle; the same call with PFP_SA_REPLAY=0 (the second round ranks again) must give the same bytes
and the same statistics.  The kernel trace is the witness of which path ran.  Inputs: merge_cases.py."""
import importlib
import os

import numpy as np
import pytest

import merge_cases as mc

pytestmark = pytest.mark.gpu

BWT_ONLY, DENSE, SPARSE = mc.FLAG_SETS
SAMPLED = (2, 4, 6)                  # FLAG_SSA, FLAG_ESA, both
SWITCHES = ("PFP_PREC_DIRECT", "PFP_BIG_BUDGET", "PFP_BIG_CAP", "PFP_SA_REPLAY", "PFP_SA_REPLAY_BUDGET")
# input -> what it exercises
CASES = {
    "snp48": "groups ranked in LDS, all-pairs and by search",
    "copies400": "hard_sort_kernel: 513 .. 1024 occurrences",
    "copies1200": "the device-wide sort",
    "copies1200/budget6000": "several sort chunks",
    "copies1200/budget100": "one group beyond the budget: hard_big_kernel",
    "copies1200/cap2": "queue overflow: the BWT round runs again and stages twice",
}
CASES.update({name: "golden" for name in mc.CASES if name.startswith("golden_") and "/" not in name})
REPLAY_ROW, GROUPS_ROW = "pfp::hard_replay_kernel", "pfp::hard_groups_kernel"
SORT_ROWS = ("pfp::big_keys_kernel", "pfp::big_place_kernel")


class switches:
    """the merge's switches (read per call) in os.environ for the duration of a call, all others of them unset"""

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


def debug_context(pkg, **env):
    """a context with PFP_DEBUG=1 (read, like the window hash of `env`, when a context is made)"""
    env = dict(env, PFP_DEBUG="1")
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
    c = debug_context(pkg)
    yield c
    c.close()


_wants, _runs = {}, {}


def want_of(O, name, flags):
    """the oracle's outputs, once per (text, flags)"""
    key = (name.split("/")[0], flags)
    if key not in _wants:
        c = mc.CASES[name]
        _wants[key] = O.bigbwt(mc.text_of(O, name), c["w"], c["p"], flags)
    return _wants[key]


def rows_of(trace):
    """{row: launches} of the rows this file looks at (merge_cases.MERGE_ROWS does not know the replay's row)"""
    return {r["name"]: r["launches"] for r in trace
            if r["name"] in (REPLAY_ROW, GROUPS_ROW, "pfp::hard_sort_kernel", "pfp::hard_big_kernel") + SORT_ROWS
            or r["name"].endswith(mc.MERGE_SORT_TAG)}


def sort_launches(rows):
    return sum(n for r, n in rows.items() if r.endswith(mc.MERGE_SORT_TAG)), rows.get(SORT_ROWS[0], 0), rows.get(SORT_ROWS[1], 0)


def run(O, ctx, name, flags, width, **env):
    """one traced call of the fused chain: (outputs, {row: launches}, the merge's statistics)"""
    c = mc.CASES[name]
    ctx.set_index_bits(64 if width == 64 else 0)
    ctx.set_kernel_trace(True)
    try:
        with switches(**dict(c["env"], **env)):
            got = ctx.bigbwt(mc.text_of(O, name), c["w"], c["p"], flags)
        rows = rows_of(ctx.kernel_trace())
        st = ctx.stats()
    finally:
        ctx.set_kernel_trace(False)
        ctx.set_index_bits(0)
    return got, rows, {k: st[k] for k in mc.MERGE_STATS}


def run_once(O, ctx, name, flags, width, replay):
    """... with PFP_SA_REPLAY=replay in the module's debug context, kept for the tests that compare the two paths"""
    key = (name, flags, width, replay)
    if key not in _runs:
        _runs[key] = run(O, ctx, name, flags, width, PFP_SA_REPLAY=str(replay))
    return _runs[key]


def check_sampled(pkg, got, want, flags):
    assert np.array_equal(got["bwt"], want["bwt"])
    if flags & pkg.FLAG_SSA:
        assert np.array_equal(pkg.unpack5(got["ssa"]).reshape(-1, 2), want["ssa"])
    if flags & pkg.FLAG_ESA:
        assert np.array_equal(pkg.unpack5(got["esa"]).reshape(-1, 2), want["esa"])


def same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


# ---------------------------------------------------------------- parity, and the two paths against each other

@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", SAMPLED)
@pytest.mark.parametrize("name", list(CASES))
def test_replayed_ranks_match_the_oracle(O, pkg, dctx, name, flags, width):
    got, rows, _ = run_once(O, dctx, name, flags, width, 1)
    check_sampled(pkg, got, want_of(O, name, flags), flags)
    # nothing of the SA round ranks: the sorts are those of the BWT round, and hard_groups_kernel runs once per round
    # (more often in the BWT round where the queue overflowed)
    if GROUPS_ROW in rows:
        bwt_only = run_once(O, dctx, name, BWT_ONLY, width, 1)[1]
        assert rows[GROUPS_ROW] == bwt_only[GROUPS_ROW] + 1
        for row in ("pfp::hard_sort_kernel", "pfp::hard_big_kernel"):
            assert rows.get(row, 0) == bwt_only.get(row, 0), row
        assert (REPLAY_ROW in rows) == any(r in rows for r in ("pfp::hard_sort_kernel", "pfp::hard_big_kernel") + SORT_ROWS)


@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", SAMPLED)
@pytest.mark.parametrize("name", list(CASES))
def test_both_paths_agree(O, pkg, dctx, name, flags, width):
    got1, rows1, st1 = run_once(O, dctx, name, flags, width, 1)
    got0, rows0, st0 = run_once(O, dctx, name, flags, width, 0)
    check_sampled(pkg, got0, want_of(O, name, flags), flags)
    same_bytes(got0, got1)
    assert st0 == st1
    assert REPLAY_ROW not in rows0 and rows0.get(GROUPS_ROW, 0) == rows1.get(GROUPS_ROW, 0)


# ---------------------------------------------------------------- the witness that the replay ran

@pytest.mark.parametrize("width", mc.WIDTHS)
def test_second_round_sorts_nothing(O, dctx, width):
    """copies1200: groups of more than 1024 occurrences go through the device-wide sort.  With the replay the sampled run
    sorts as often as the BWT-only run; without it, twice as often"""
    base = sort_launches(run_once(O, dctx, "copies1200", BWT_ONLY, width, 1)[1])
    assert min(base) >= 1
    on = run_once(O, dctx, "copies1200", SPARSE, width, 1)[1]
    assert sort_launches(on) == base and on.get(REPLAY_ROW, 0) >= 1 and on[GROUPS_ROW] == 2
    off = run_once(O, dctx, "copies1200", SPARSE, width, 0)[1]
    assert sort_launches(off) == tuple(2 * n for n in base) and REPLAY_ROW not in off and off[GROUPS_ROW] == 2


@pytest.mark.parametrize("width", mc.WIDTHS)
def test_no_budget_ranks_again(O, dctx, width):
    """PFP_SA_REPLAY_BUDGET=0 and nothing forced: the staging does not fit, the second round ranks again - same outputs"""
    got, rows, st = run(O, dctx, "copies1200", SPARSE, width, PFP_SA_REPLAY_BUDGET="0")
    assert rows == run_once(O, dctx, "copies1200", SPARSE, width, 0)[1] and REPLAY_ROW not in rows
    ref, _, st1 = run_once(O, dctx, "copies1200", SPARSE, width, 1)
    same_bytes(got, ref)
    assert st == st1
    # ... and by default (an eighth of the device) it fits
    assert REPLAY_ROW in run(O, dctx, "copies1200", SPARSE, width)[1]


# ---------------------------------------------------------------- slices and slot ranges (two virtual ranks on one device)

def _pieces(res, key):
    off, parts = 0, []
    for r in res:
        assert r[key + "_off"] == off, (key, r[key + "_off"], off)
        parts.append(r[key].cpu().numpy())
        off += r[key].numel()
    return np.concatenate(parts)


def run_ranks(pkg, text, w, p, flags, width, shard_sa, replay, **ctx_env):
    """the text through two ranks, each with a debug context: (the ranks' outputs joined, fallback groups per rank, the
    position where the second rank's slice begins)"""
    import torch
    d = importlib.import_module("bigbwt_amd.dist")
    n = len(text)
    cuts = [0, n // 2 - 2, n]
    ctxs = [debug_context(pkg, **ctx_env) for _ in range(2)]
    try:
        for x in ctxs:
            x.set_index_bits(64 if width == 64 else 0)
        shards = [torch.from_numpy(text[cuts[r]:cuts[r + 1]].copy()).cuda() for r in range(2)]
        with switches(PFP_SA_REPLAY=str(replay)):
            res = d.simulate(ctxs, shards, w, p, flags, halo=8192, shard_sa=shard_sa)
        assert res[0]["lo"] == 0 and res[0]["hi"] == res[1]["lo"] and res[1]["hi"] == n + 1
        out = {"bwt": torch.cat([r["bwt"] for r in res]).cpu().numpy()}
        for key, flag in (("ssa", pkg.FLAG_SSA), ("esa", pkg.FLAG_ESA)):
            if flags & flag:
                out[key] = _pieces(res, key)
        stats = [x.stats() for x in ctxs]
        return out, [s["hard_groups"] - s["hard_minor_groups"] for s in stats], res[1]["lo"]
    finally:
        for x in ctxs:
            x.close()


@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", SAMPLED)
@pytest.mark.parametrize("dist", list(mc.DIST_CASES))
@pytest.mark.parametrize("name", ["copies1200", "snp48"])
def test_ranks_replay_their_slices(O, pkg, dctx, name, dist, flags, width):
    """dist2_slice: every rank holds all slots and emits one half of the BWT; dist2_range: every rank holds one range of
    slots.  A rank stages and replays only the groups that meet its slice (in these two texts the boundary falls between two
    fallback groups: the ranks' counts add up to the whole's); the other path gives the same bytes"""
    c, text, want = mc.CASES[name], mc.text_of(O, name), want_of(O, name, flags)
    got1, fb1, _ = run_ranks(pkg, text, c["w"], c["p"], flags, width, mc.DIST_CASES[dist], 1)
    check_sampled(pkg, got1, want, flags)
    got0, fb0, _ = run_ranks(pkg, text, c["w"], c["p"], flags, width, mc.DIST_CASES[dist], 0)
    same_bytes(got0, got1)
    whole = run_once(O, dctx, name, flags, width, 1)[2]
    assert fb0 == fb1 and sum(fb1) >= whole["hard_groups"] - whole["hard_minor_groups"]


@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", SAMPLED)
def test_group_cut_by_the_slice_boundary_is_replayed_in_parts(O, pkg, flags, width):
    """`sliced_groups` of test_merge_chains.py: the second rank's slice begins inside a fallback group.  Both ranks rank the
    group, each stages and replays the occurrences of its own slice - the rest of the group's staging stays unwritten and
    must not be read (PFP_DEBUG would fail the call).  (The reference's window hash, as there: the layout is computed from
    the oracle's dictionary)"""
    import test_merge_chains as chains
    _, w, p = chains.INPUTS["sliced_groups"]
    text = chains.text_of(O, "sliced_groups")
    fb = [u for u in chains.layout_of(O, "sliced_groups")["units"] if chains.kind(u) == "fallback"]
    want = O.bigbwt(text, w, p, flags)
    got1, fb1, cut = run_ranks(pkg, text, w, p, flags, width, False, 1, PFP_WINDOW_HASH="kr")
    assert any(u["base"] < cut < u["base"] + u["E"] for u in fb) and sum(fb1) == len(fb) + 1
    check_sampled(pkg, got1, want, flags)
    got0, fb0, _ = run_ranks(pkg, text, w, p, flags, width, False, 0, PFP_WINDOW_HASH="kr")
    same_bytes(got0, got1)
    assert fb0 == fb1
