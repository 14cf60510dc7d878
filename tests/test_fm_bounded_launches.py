"""The one loop that repeats a bounded launch (csrc/fmdev.hpp, bounded_launches) under a small PFP_FM_MS_STEPS, on the input of
fm_host_cases.py (a 3000-byte text; 30 patterns of 0 to 40 bytes, among them the empty one, an absent byte and the repeated
segment), in both index widths: what a call returns does not depend on the budget, and under the budget the kernel trace shows
more than one launch of every kernel that resumes from a record, so the resume paths ran."""
import numpy as np
import pytest

import fm_host_cases as H

pytestmark = pytest.mark.gpu

K_APPROX = 2
# budget -> name -> (the call, the kernel-trace rows that must show more than one launch under the budget)
CASES = {
    "1": {
        "ms": (lambda fm, P: fm.matching_statistics(P), ("fm_ms",)),
        "ms_thr": (lambda fm, P: fm.matching_statistics(P, thresholds=True), ("fm_ms_thr1", "fm_ms_thr2")),
        "doclist": (lambda fm, P: fm.doclist(P), ()),      # (the budget is the chunk of hits a workgroup counts: no record, no loop)
    },
    "7": {
        "approx": (lambda fm, P: fm.approx(P, K_APPROX, toehold=True), ("fm_approx",)),      # hit_off: the counting walk; the rest: the fill
    },
}


def launches(trace, name):
    return sum(r["launches"] for r in trace if r["name"] == name)


@pytest.fixture(scope="module", params=[0, 64], ids=["idx32", "idx64"])
def fm(request, O, pkg, ctx):
    ctx.set_index_bits(request.param)
    try:
        with H.index_of(O, pkg, ctx, thresholds=True) as f:
            assert f.info()["row_bits"] == (64 if request.param else 32)
            yield f
    finally:
        ctx.set_index_bits(0)


@pytest.mark.parametrize("budget,name", [(b, n) for b, calls in CASES.items() for n in calls])
def test_budget_does_not_change_the_answer(fm, ctx, monkeypatch, budget, name):
    call, resumed = CASES[budget][name]
    P = list(H.patterns())
    monkeypatch.delenv("PFP_FM_MS_STEPS", raising=False)
    monkeypatch.delenv("PFP_FM_SEQ_BUDGET", raising=False)
    want = call(fm, P)
    monkeypatch.setenv("PFP_FM_MS_STEPS", budget)
    ctx.set_kernel_trace(True)
    try:
        got = call(fm, P)
        trace = ctx.kernel_trace()
    finally:
        ctx.set_kernel_trace(False)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, budget, i)
    for row in resumed:
        assert launches(trace, row) > 1, (row, trace)
