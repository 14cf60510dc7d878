"""The suffix sorters of csrc/sufsort.hip path by path.  `doubling` chooses between about a dozen paths per round by sizes
and shapes that small inputs never produce; every case here is built to go down one of them (tests/sorter_cases.py has the
inputs and says, by the constants of sufsort.hip, why), is compared with two references that share no code with the
library - the oracle's prefix-doubling sorter and, above 2^20 entries, the linear checker of tests/sacheck.py - and asserts a
WITNESS: the kernel-trace row only that path launches.  A retune that moves a threshold makes the case fail with "witness
missing" rather than silently test another path.  tests/README.md has the table path -> case -> witness.

Dictionaries run through gsacak, gsacak64 and gsacak_lcp_da (LCP and DA against the oracle), every case in both index widths.
"""
import json
import os
import subprocess
import sys

import pytest

import sorter_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_and_check(O, wctx, request, name):
    width = request.node.callspec.params["wctx"]
    trace = sc.run_case(wctx, O, name, width)
    print(name, width, json.dumps(trace))
    errs = sc.witness_errors(trace, sc.CASES[name]["expect"](width))
    assert not errs, f"{name} (idx{width}): " + "; ".join(errs) + f"; trace: {trace}"


@pytest.mark.parametrize("name", sc.DICT_CASES)
def test_dictionary_sorter_paths(O, wctx, request, name):
    """pivot rounds (device-wide, placed in LDS, placement giving up, segmented, segmented refused by a giant family), window
    growth, the comparison finisher and its two refusals, doubling with scattered ranks / lazy lookup / small groups, the
    keys-only first round below and above the thresholds of sort_keys_db"""
    run_and_check(O, wctx, request, name)


@pytest.mark.parametrize("name", sc.INT_CASES)
def test_integer_sorter_run_keys_and_plain_keys(O, wctx, request, name):
    """sort_int_suffixes with long runs of one symbol: run keys while the largest symbol is below 2^29, plain keys from
    there on, the same string moved up - the last one with every symbol above 2^31"""
    run_and_check(O, wctx, request, name)


@pytest.mark.parametrize("name", sc.PARSE_CASES)
def test_parse_pivot_rounds(O, wctx, request, name):
    """the pivot rounds of the parse need the occurrence counts, which only parse_bwt hands over: hand-built parses through
    Context.bwtparse against the oracle's ilist / bwlast"""
    run_and_check(O, wctx, request, name)


@pytest.mark.parametrize("n", sc.BYTE_SIZES)
@pytest.mark.parametrize("kind", sc.BYTE_KINDS)
def test_byte_sorter(O, wctx, request, kind, n):
    """sort_byte_suffixes (doubling from 8-byte keys) on the texts that need the most rounds, at the trivial sizes and around
    2^16 and 2^20: oracle and checker"""
    run_and_check(O, wctx, request, f"bytes_{kind}_{n}")


# ---- the switches that force an alternative path, each on every case below.  The sorter reads its switches at every call
# (sorter_switches() in sufsort.hip; test_switches_are_read_per_call), so a child is not needed for them to take effect: it
# gives each switch a process that has never run without it.
SWITCH_CASES = ["fam_moderate", "fam_small", "finisher", "finisher_big_group", "deep_scatter", "int_runs", "parse_small_groups",
                "bytes_fibonacci_65537", "bytes_a^n_65537"]
SWITCHES = ["PFP_NO_FINFLAG=1", "PFP_PIVOT_CAP=0", "PFP_PIVOT_CAP=16", "PFP_NO_SMALLSEG=1", "PFP_NO_FINISHER=1", "PFP_KEYBITS=23", "PFP_KEYBITS=63"]
CHILD_TIMEOUT = 300      # nine cases x two widths: a few seconds of oracle and sorting plus start-up; generous for a busy host
_child_faulted = False


def switch_errors(switch, rows):
    """what a switch must change in the traces {(case, width): trace} of the child"""
    errs = []
    for (name, width), trace in rows.items():
        kind = sc.CASES[name]["kind"]
        n = lambda w: sc.row_launches(trace, w)      # noqa: E731
        tag = f"{name} idx{width}: "
        if switch in ("PFP_NO_FINFLAG=1", "PFP_PIVOT_CAP=0") and n(sc.PIVOT):      # no finished flag / no window: no pivot round
            errs.append(tag + "a pivot round ran")
        if switch == "PFP_NO_FINISHER=1" and n(sc.FINISH):
            errs.append(tag + "the finisher ran")
        if switch == "PFP_NO_SMALLSEG=1" and kind != "parse" and n(sc.SMALL):       # (the parse's pivot round places small groups regardless)
            errs.append(tag + "small groups were placed in LDS")
        if switch in ("PFP_PIVOT_CAP=16", "PFP_KEYBITS=23", "PFP_KEYBITS=63") and kind == "gsa" and not n(sc.PIVOT):
            errs.append(tag + "no pivot round")
    return errs


@pytest.mark.parametrize("switch", SWITCHES)
def test_process_wide_switches(switch):
    """every switch that forces an alternative path: the cases still match the oracle and the checker, and where the switch
    exists to remove a path, that path's witness is absent"""
    global _child_faulted
    if _child_faulted:
        pytest.skip("an earlier child faulted")
    key, val = switch.split("=")
    env = dict(os.environ)
    env[key] = val
    cmd = [sys.executable, os.path.join(ROOT, "tests", "sorter_cases.py")] + SWITCH_CASES
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as ex:
        _child_faulted = True
        pytest.fail(f"{switch}: the child ran into its time limit of {CHILD_TIMEOUT} s; output so far: {ex.stdout!r}")
    if out.returncode < 0 or out.returncode >= 124:
        _child_faulted = True
        pytest.fail(f"{switch}: the child ended with status {out.returncode}: {out.stderr[-2000:]}")
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    print(switch, out.stdout)
    rows = {(r["case"], r["width"]): r["witnesses"] for r in lines}
    assert set(rows) == {(c, w) for c in SWITCH_CASES for w in (32, 64)}, f"{switch}: cases missing from the child's output: {out.stderr[-2000:]}"
    wrong = [f"{r['case']} idx{r['width']}: {r['error']}" for r in lines if not r["ok"]]
    assert not wrong, f"{switch}: " + "; ".join(wrong)
    assert out.returncode == 0, f"{switch}: the child ended with status {out.returncode}: {out.stderr[-2000:]}"
    errs = switch_errors(switch, rows)
    assert not errs, f"{switch}: " + "; ".join(errs)


@pytest.mark.parametrize("switch,name,witness", [("PFP_NO_FINISHER", "finisher", sc.FINISH), ("PFP_NO_SMALLSEG", "fam_small", sc.SMALL)])
def test_switches_are_read_per_call(O, wctx, request, switch, name, witness):
    """the sorter reads its switches when it is called, not when the library is loaded: inside one process the same case runs
    with the switch in the environment (right output, the witness of the switched-off path absent) and then without it (right
    output, the witness back)"""
    width = request.node.callspec.params["wctx"]
    saved = os.environ.get(switch)
    try:
        os.environ[switch] = "1"
        off = sc.run_case(wctx, O, name, width)
        del os.environ[switch]
        on = sc.run_case(wctx, O, name, width)
    finally:
        if saved is None:
            os.environ.pop(switch, None)
        else:
            os.environ[switch] = saved
    print(switch, name, width, json.dumps(off), json.dumps(on))
    assert sc.row_launches(off, witness) == 0, f"{name} (idx{width}) under {switch}=1: {witness} was launched; trace: {off}"
    assert sc.row_launches(on, witness) >= 1, f"{name} (idx{width}) without {switch}: no launch of {witness}; trace: {on}"
