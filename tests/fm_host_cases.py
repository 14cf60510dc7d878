"""The calls of FmIndex that take host patterns (csrc/api_fm.hip: one upload of the patterns, one budget, one rule that cuts a
call into groups of patterns), on one small input that makes every one of them work in several groups under a small
PFP_FM_SEQ_BUDGET.  Mapping reads and pairs run on inputs of their own tests instead, which those tests show to have hits,
secondary hits, rescues and groups: the reads of map_cases over `copies`, the pairs of pair_cases over `dna`.
tests/test_fm_host_calls.py asserts the answers; tests/README.md has the note.

As a program it runs every call (or the named ones) without a budget and under its budgets and prints one JSON line per (call,
environment):

    PFP_TRACE_HOST=1 python tests/fm_host_cases.py [CALL ...]
    {"call": "locate", "env": {"PFP_FM_SEQ_BUDGET": "7"}, "launches": {"pfp::fm_count_kernel": [1, 0], ...}, "peak": 123456,
     "sha256": "...", "waits": 12}

`launches` holds (launches, algo_bytes) of every row of Context.kernel_trace() that the call opened, `peak` the pool's peak bytes
of a context that built the index and ran this one call, `sha256` a digest of the arrays the call returned (dtype, shape and
bytes of each), `waits` the host waits on the stream over the context's life as PFP_TRACE_HOST=1 makes the library print them
when the context goes (null without it).  "<call>/empty" is the call without patterns.  Nothing is compared with a reference
here: two builds that print the same lines launch, wait, allocate and answer alike.
"""
import collections
import functools
import hashlib
import json
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import map_cases  # noqa: E402
import pair_cases  # noqa: E402

BUDGETS = ("1", "7")      # every pattern alone; some groups
K_MISMATCH, K_EDIT, MIN_SEED, MIN_MEM = 1, 2, 6, 4
SEG_COPIES, NPARTS = 12, 8
K_CAP, CAP_SEED = 16, 4      # align_cap: edits and seeds at which several patterns have more alignments than max_aln = 2 keeps
K_MAP, MAP_MIN_SEED, MAP_MAX_SEC = 8, 12, 2     # as test_fm_map.py maps the reads of (`copies`, `records`, 8)


@functools.lru_cache(maxsize=None)
def text_and_segment():
    """a DNA text of 3000 bytes that holds one 40-byte segment SEG_COPIES times, and the segment"""
    rng = np.random.default_rng(2718)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    text = rng.choice(acgt, 3000)
    seg = rng.choice(acgt, 40)
    for i in range(SEG_COPIES):
        at = 100 + 240 * i + int(rng.integers(0, 50))
        text[at:at + 40] = seg
    assert text.tobytes().count(seg.tobytes()) == SEG_COPIES
    return text, seg.tobytes()


def seq_starts():
    """a sequence table of NPARTS parts of unequal lengths: NPARTS + 1 starts"""
    n = len(text_and_segment()[0])
    return np.array([0, 150, 700, 701, 1400, 1900, 2300, 2950, n][:NPARTS] + [n], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def patterns():
    """30 patterns of 0 to 40 bytes: the empty one, one byte, an absent one, the repeated segment, the segment with one
    substitution, and substrings of 12 to 40 bytes, every third with one substitution"""
    text, seg = text_and_segment()
    tb = text.tobytes()
    rng = np.random.default_rng(31)
    sub = lambda s, i: s[:i] + bytes([ord("A") if s[i] != ord("A") else ord("C")]) + s[i + 1:]
    pats = [tb[500:530], b"", b"A", b"ACGTN" * 4, seg, sub(seg, 17), tb[:12], tb[-40:]]
    while len(pats) < 30:
        m = int(rng.integers(12, 41))
        i = int(rng.integers(0, len(tb) - m + 1))
        s = tb[i:i + m]
        pats.append(sub(s, int(rng.integers(0, m))) if len(pats) % 3 == 0 else s)
    assert tb.count(pats[3]) == 0
    return tuple(pats)


@functools.lru_cache(maxsize=None)
def candidates():
    """(cand_pat uint32, cand_diag int64) for extend: every non-empty pattern on three diagonals"""
    tb = text_and_segment()[0].tobytes()
    cp, cd = [], []
    for p, s in enumerate(patterns()):
        if s:
            at = max(tb.find(s[:8]), 0)
            for dg in (at, at - 1, at + 300):
                cp.append(p)
                cd.append(dg)
    return np.array(cp, dtype=np.uint32), np.array(cd, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def windows():
    """(cand_pat uint32, lo uint64, hi uint64) for window: per candidate of candidates() a window that starts 3 bytes before its
    diagonal and ends 3 bytes behind the pattern's length from there, or 2 bytes short of it"""
    n = len(text_and_segment()[0])
    cp, cd = candidates()
    lo, hi = [], []
    for p, dg in zip(cp.tolist(), cd.tolist()):
        m = len(patterns()[p])
        a = min(max(dg, 0), n)
        lo.append(max(a - 3, 0))
        hi.append(max(min(a + m + (3 if dg % 2 else -2), n), lo[-1]))
    return cp, np.array(lo, dtype=np.uint64), np.array(hi, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def spans():
    """(aln_pat uint32, start uint64, end uint64) for cigar: every non-empty pattern against a span of its length at the place
    of its first 8 bytes, one byte further, and elsewhere"""
    n = len(text_and_segment()[0])
    cp, cd = candidates()
    st = np.clip(cd, 0, n)
    en = np.array([min(s + len(patterns()[p]), n) for p, s in zip(cp.tolist(), st.tolist())], dtype=np.uint64)
    return cp, st.astype(np.uint64), en


def _or_none(arrays, P):
    """the arrays that go with the patterns, or empty ones of their types for the call without patterns"""
    return arrays if P else tuple(a[:0] for a in arrays)


# What a call needs and gives.  thresholds: the index gets them; run(fm, patterns) -> the tuple of arrays the call returns; index: which
# text it runs on ("text": this module's, with patterns(); else a text of map_cases with its `records` table and the reads INPUTS
# names); offsets: which of the returned arrays are offsets ([0] without patterns, where every other array is empty); budgets: the
# values of PFP_FM_SEQ_BUDGET that cut it into groups
Call = collections.namedtuple("Call", "thresholds run index offsets budgets", defaults=("text", (0,), BUDGETS))
_map = lambda fm, P, **kw: fm.map_reads(P, K_MAP, MAP_MIN_SEED, MAP_MAX_SEC, **kw)
CALLS = {
    "count": Call(False, lambda fm, P: fm.count(P), offsets=()),
    "count_toehold": Call(False, lambda fm, P: fm.count(P, toehold=True), offsets=()),
    "locate": Call(False, lambda fm, P: fm.locate(P, ranges=True)),
    "approx": Call(False, lambda fm, P: fm.approx(P, K_MISMATCH, toehold=True)),
    "approx_locate": Call(False, lambda fm, P: fm.approx_locate(P, K_MISMATCH)),
    "ms": Call(False, lambda fm, P: fm.matching_statistics(P)),
    "ms_thr": Call(True, lambda fm, P: fm.matching_statistics(P, thresholds=True)),
    "mems": Call(False, lambda fm, P: fm.mems(P, MIN_MEM)),
    "mems_thr": Call(True, lambda fm, P: fm.mems(P, MIN_MEM, thresholds=True)),
    "extend": Call(False, lambda fm, P: fm.extend(P, *_or_none(candidates(), P), K_EDIT), offsets=()),
    "align": Call(False, lambda fm, P: fm.align(P, K_EDIT, MIN_SEED)),
    "align_thr": Call(True, lambda fm, P: fm.align(P, K_EDIT, MIN_SEED, thresholds=True)),
    "locate_seqs": Call(False, lambda fm, P: fm.locate_seqs(P, ranges=True)),
    "doclist": Call(False, lambda fm, P: fm.doclist(P)),
    "window": Call(False, lambda fm, P: fm.window(P, *_or_none(windows(), P), K_EDIT), offsets=()),
    "cigar": Call(False, lambda fm, P: fm.cigar(P, *_or_none(spans(), P), K_EDIT), offsets=(1,)),
    "align_cap": Call(False, lambda fm, P: fm.align(P, K_CAP, CAP_SEED, max_aln=2)),
    "map": Call(False, _map, "copies", (0, 8, 10), ("1", "40")),
    "map_thr": Call(True, lambda fm, P: _map(fm, P, thresholds=True), "copies", (0, 8, 10), ("1", "40")),
    "map_pairs": Call(False, lambda fm, P: fm.map_pairs(P, K_MAP, pair_cases.MIN_SEED, pair_cases.MIN_INS, pair_cases.MAX_INS), "dna", (12, 14),
                      ("1", "9")),
}
INPUTS = {"text": patterns, "copies": lambda: map_cases.reads_of("copies", "records", K_MAP), "dna": lambda: pair_cases.reads_of("dna")}

_parts = {}


def index_of(O, pkg, ctx, thresholds=False, index="text"):
    """an index with text, samples and a sequence table (the BWT and the samples are computed once per text): this module's text
    and seq_starts(), or a text of map_cases with its `records` table"""
    text = text_and_segment()[0] if index == "text" else map_cases.text_of(index)
    if index not in _parts:
        bwt = np.asarray(O.simplebwt(text))
        sa = np.concatenate([[len(text)], np.asarray(O.sacak(text), dtype=np.int64)]).astype(np.int64)
        starts = np.flatnonzero(np.concatenate([[True], bwt[1:] != bwt[:-1]]))
        ends = np.flatnonzero(np.concatenate([bwt[1:] != bwt[:-1], [True]]))
        pk = lambda rows: pkg.pack5(np.stack([rows, sa[rows]], axis=1).reshape(-1).astype(np.uint64))
        _parts[index] = (bwt, pk(starts), pk(ends))
    fm = ctx.fm_index_ms(*_parts[index], text)
    fm.set_sequences(seq_starts() if index == "text" else map_cases.starts_of(index, "records"))
    if thresholds:
        fm.add_thresholds()
    return fm


class Env:
    """PFP_FM_SEQ_BUDGET as the case sets it, for the duration of a call (the library reads it once per call)"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = os.environ.pop("PFP_FM_SEQ_BUDGET", None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        os.environ.pop("PFP_FM_SEQ_BUDGET", None)
        if self.saved is not None:
            os.environ["PFP_FM_SEQ_BUDGET"] = self.saved


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _close_and_count_waits(ctx):
    """close the context; the number in the line PFP_TRACE_HOST=1 makes the library write to stderr then (None without one)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            ctx.close()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        said = tmp.read().decode(errors="replace")
    m = re.search(r"host waits on the stream over the context's life: (\d+)", said)
    return int(m.group(1)) if m else None


def run_case(pkg, O, name, env, empty=False):
    """one host call in a context of its own; returns the record that main() prints"""
    call = CALLS[name]
    ctx = pkg.Context(0)
    try:
        with index_of(O, pkg, ctx, call.thresholds, call.index) as fm, Env(env):
            ctx.set_kernel_trace(True)
            out = call.run(fm, [] if empty else list(INPUTS[call.index]()))
            rows = {r["name"]: [r["launches"], r["algo_bytes"]] for r in ctx.kernel_trace()}
            ctx.set_kernel_trace(False)
        peak = ctx.mem_stats()["peak"]
        if os.environ.get("PFP_POOL_DEBUG"):
            ctx.debug_check()
    except BaseException:
        ctx.close()
        raise
    return dict(call=name + ("/empty" if empty else ""), env=env, launches=rows, peak=peak, sha256=digest(out),
                waits=_close_and_count_waits(ctx))


def main(argv):
    import __graft_entry__ as entry
    names = argv[1:] or list(CALLS)
    unknown = [n for n in names if n not in CALLS]
    if unknown:
        print("unknown: %s; calls: %s" % (unknown, " ".join(CALLS)), file=sys.stderr)
        return 2
    pkg = entry.load_package()
    O = entry.load_oracle()
    for name in names:
        envs = [{}] + [{"PFP_FM_SEQ_BUDGET": b} for b in CALLS[name].budgets]
        for env, empty in [(e, False) for e in envs] + [({}, True)]:
            try:      # an error of the library (a GPU fault among them): nothing more is started
                rec = run_case(pkg, O, name, env, empty)
            except Exception as ex:
                print(json.dumps(dict(call=name, env=env, empty=empty, error=f"{type(ex).__name__}: {ex}")), flush=True)
                return 3
            print(json.dumps(rec, sort_keys=True), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
