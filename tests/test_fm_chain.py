"""Chaining anchors on the GPU (csrc/fmchain.hip): FmIndex.anchors / chain / map_long and their _dev variants.

Definitions: include/pfpgpu.h, "Chaining anchors".  Every expected value comes from chain_reference.py - the definitions in plain
Python, anchors by brute force on the text, checked on the CPU in test_chain_reference.py - and every array is compared exactly,
dtype included.  Reads and anchor sets: chain_cases.py."""
import functools

import numpy as np
import pytest

import chain_cases as C
import chain_reference as R
import map_cases as K
from test_fm_map import index_of, samples

pytestmark = pytest.mark.gpu

EINVAL = -1


def same(got, want, names, what):
    assert len(got) == len(want) == len(names)
    for g, w, nm in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, nm, g[:12], w[:12])


@functools.lru_cache(maxsize=None)
def expected_reads(case):
    """(anchors of every read as FmIndex.anchors returns them, map_long's arrays) by the reference, once per case"""
    name, table, min_seed, max_occ, G, B, S, max_sec = C.READ_CASES[case]
    tb, starts = K.text_of(name).tobytes(), C.starts_of(name, table)
    reads = C.reads_of(case)
    layer1 = R.anchor_arrays([R.anchors_of(tb, starts, bytes(r), min_seed, max_occ) for r in reads])
    return layer1, R.map_long(tb, starts, reads, min_seed, max_occ, G, B, S, max_sec)


@functools.lru_cache(maxsize=None)
def expected_chains(name):
    sets, G, B, S, max_chains = C.chain_sets()[name]
    starts = K.starts_of(C.CHAIN_TEXT, C.CHAIN_TABLE)
    return R.chain_arrays([R.chains_of(a, starts, len(K.text_of(C.CHAIN_TEXT)), G, B, S, max_chains) for a in sets])


def run_reads(fm, case):
    name, table, min_seed, max_occ, G, B, S, max_sec = C.READ_CASES[case]
    reads = C.reads_of(case)
    return fm.anchors(reads, min_seed, max_occ), fm.map_long(reads, min_seed, max_occ, G, B, S, max_sec)


def run_chains(fm, name):
    sets, G, B, S, max_chains = C.chain_sets()[name]
    off, rows = C.offsets_and_rows(sets)
    return fm.chain(off, rows, G, B, S, max_chains)


@pytest.mark.parametrize("case", sorted(C.READ_CASES))
def test_anchors_and_map_long(O, pkg, wctx, case):
    name, table = C.READ_CASES[case][:2]
    with index_of(O, pkg, wctx, name, table) as fm:
        got1, got3 = run_reads(fm, case)
    want1, want3 = expected_reads(case)
    same(got1, want1, ("anc_off", "anc", "skipped"), case)
    same(got3, want3, R.NAMES, case)
    assert pkg.LONG_NAMES == R.NAMES


@pytest.mark.parametrize("name", sorted(C.chain_sets()))
def test_chain(O, pkg, wctx, name):
    with index_of(O, pkg, wctx, C.CHAIN_TEXT, C.CHAIN_TABLE) as fm:
        same(run_chains(fm, name), expected_chains(name), R.CHAIN_NAMES, name)


def test_chain_of_the_anchors_of_reads(O, pkg, wctx):
    """layer 2 over layer 1's output, against the reference on the same anchors"""
    case = "copies one record"
    name, table, min_seed, max_occ, G, B, S, _ = C.READ_CASES[case]
    starts = C.starts_of(name, table)
    with index_of(O, pkg, wctx, name, table) as fm:
        off, anc, _ = fm.anchors(C.reads_of(case), min_seed, max_occ)
        got = fm.chain(off, anc, G, B, S, 3)
    per = [[tuple(int(v) for v in row) for row in anc[int(off[p]):int(off[p + 1])]] for p in range(len(off) - 1)]
    want = R.chain_arrays([R.chains_of(a, starts, len(K.text_of(name)), G, B, S, 3) for a in per])
    same(got, want, R.CHAIN_NAMES, case)


@pytest.mark.parametrize("case", ["copies", "dna"])
def test_thresholds_do_not_change_the_anchors(O, pkg, ctx, case):
    name, table, min_seed, max_occ, G, B, S, max_sec = C.READ_CASES[case]
    reads = C.reads_of(case)
    with index_of(O, pkg, ctx, name, table) as fm:
        fm.add_thresholds()
        same(fm.anchors(reads, min_seed, max_occ, thresholds=True), fm.anchors(reads, min_seed, max_occ), ("anc_off", "anc", "skipped"), case)
        same(fm.map_long(reads, min_seed, max_occ, G, B, S, max_sec, thresholds=True), expected_reads(case)[1], R.NAMES, case)


def test_steps_and_budget_do_not_matter(O, pkg, wctx, monkeypatch):
    for v in ("PFP_FM_CHAIN_STEPS", "PFP_FM_SEQ_BUDGET"):
        monkeypatch.delenv(v, raising=False)
    cases, names = ("copies one record", "ab"), ("sizes", "random", "H back", "shared parent, S")
    for settings in (("PFP_FM_CHAIN_STEPS", "1"), ("PFP_FM_CHAIN_STEPS", "7"), ("PFP_FM_SEQ_BUDGET", "3"), ("PFP_FM_SEQ_BUDGET", "1")):
        monkeypatch.setenv(*settings)
        for case in cases:
            if settings == ("PFP_FM_CHAIN_STEPS", "1") and case == "ab":
                continue                                    # (thousands of launches for its 4844 anchors: 7 covers it)
            with index_of(O, pkg, wctx, *C.READ_CASES[case][:2]) as fm:
                got1, got3 = run_reads(fm, case)
            same(got1, expected_reads(case)[0], ("anc_off", "anc", "skipped"), (case, settings))
            same(got3, expected_reads(case)[1], R.NAMES, (case, settings))
        with index_of(O, pkg, wctx, C.CHAIN_TEXT, C.CHAIN_TABLE) as fm:
            for name in names:
                same(run_chains(fm, name), expected_chains(name), R.CHAIN_NAMES, (name, settings))
        monkeypatch.delenv(settings[0])


def test_device_calls(O, pkg, wctx):
    """the _dev variants equal the host calls; the offsets-only forms give the same offsets; what lies behind the outputs stays"""
    import torch
    case = "copies"
    name, table, min_seed, max_occ, G, B, S, max_sec = C.READ_CASES[case]
    reads = C.reads_of(case)
    dev = torch.device("cuda", wctx.device)
    pat, off = pkg.pfp._patterns(reads)
    npat = len(reads)
    up = lambda a, view: torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).to(dev)
    filled = lambda count, dt, v: torch.full((count,), v, dtype=dt, device=dev)
    host = lambda t, count, dt: t[:count].cpu().numpy().view(dt)
    d_pat, d_poff = up(pat, np.uint8), up(off, np.int64)
    with index_of(O, pkg, wctx, name, table) as fm:
        want1, want3 = run_reads(fm, case)
        A = int(want1[0][-1])
        assert A >= 20
        # anchors
        d_aoff, d_skip = filled(npat + 3, torch.int64, -7), filled(npat + 2, torch.int32, -9)
        torch.cuda.synchronize()
        fm.anchors_dev(d_pat.data_ptr(), d_poff.data_ptr(), npat, min_seed, d_aoff.data_ptr(), None, None, max_occ=max_occ)
        assert np.array_equal(host(d_aoff, npat + 1, np.uint64), want1[0]) and (d_aoff[npat + 1:] == -7).all()
        d_anc = filled(3 * A + 3, torch.int64, -7)
        torch.cuda.synchronize()
        fm.anchors_dev(d_pat.data_ptr(), d_poff.data_ptr(), npat, min_seed, d_aoff.data_ptr(), d_anc.data_ptr(), d_skip.data_ptr(), max_occ=max_occ)
        same((host(d_aoff, npat + 1, np.uint64), host(d_anc, 3 * A, np.uint64).reshape(-1, 3), host(d_skip, npat, np.uint32)), want1,
             ("anc_off", "anc", "skipped"), "anchors_dev")
        assert (d_anc[3 * A:] == -7).all() and (d_skip[npat:] == -9).all()
        # chains of those anchors
        want2 = fm.chain(want1[0], want1[1], G, B, S)
        Cn = int(want2[0][-1])
        assert Cn >= 5
        d_coff = filled(npat + 3, torch.int64, -7)
        torch.cuda.synchronize()
        fm.chain_dev(d_aoff.data_ptr(), d_anc.data_ptr(), npat, d_coff.data_ptr(), max_gap=G, band=B, min_score=S)
        assert np.array_equal(host(d_coff, npat + 1, np.uint64), want2[0]) and (d_coff[npat + 1:] == -7).all()
        d32 = [filled(Cn + 2, torch.int32, -9) for _ in range(5)]
        d64 = [filled(Cn + 2, torch.int64, -7) for _ in range(2)]
        torch.cuda.synchronize()
        fm.chain_dev(d_aoff.data_ptr(), d_anc.data_ptr(), npat, d_coff.data_ptr(), d32[0].data_ptr(), d32[1].data_ptr(), d32[2].data_ptr(),
                     d32[3].data_ptr(), d64[0].data_ptr(), d64[1].data_ptr(), d32[4].data_ptr(), max_gap=G, band=B, min_score=S)
        got2 = (host(d_coff, npat + 1, np.uint64),) + tuple(host(t, Cn, np.uint32) for t in d32[:4]) + tuple(host(t, Cn, np.uint64) for t in d64) + \
            (host(d32[4], Cn, np.uint32),)
        same(got2, want2, R.CHAIN_NAMES, "chain_dev")
        assert all((t[Cn:] == -9).all() for t in d32) and all((t[Cn:] == -7).all() for t in d64)
        # long reads
        H = int(want3[0][-1])
        assert H >= 5
        for fill in (False, True):
            d_hoff, d_mapq, d_nc = filled(npat + 3, torch.int64, -7), filled(npat + 16, torch.uint8, 0x5A), filled(npat + 2, torch.int64, -7)
            outs = [filled(H + 16, torch.uint8, 0x5A), filled(H + 2, torch.int32, -9)] + [filled(H + 2, torch.int64, -7) for _ in range(3)] + \
                [filled(H + 2, torch.int32, -9) for _ in range(5)]
            torch.cuda.synchronize()
            fm.map_long_dev(d_pat.data_ptr(), d_poff.data_ptr(), npat, min_seed, d_hoff.data_ptr(), d_mapq.data_ptr(), d_nc.data_ptr(),
                            *([t.data_ptr() for t in outs] if fill else [None] * 10), max_occ=max_occ, max_gap=G, band=B, min_score=S,
                            max_sec=max_sec)
            got3 = [host(d_hoff, npat + 1, np.uint64), host(d_mapq, npat, np.uint8), host(d_nc, npat, np.uint64)]
            assert (d_hoff[npat + 1:] == -7).all() and (d_mapq[npat:] == 0x5A).all() and (d_nc[npat:] == -7).all()
            if fill:
                got3 += [host(t, H, w.dtype) for t, w in zip(outs, want3[3:])]
                assert (outs[0][H:] == 0x5A).all() and all((t[H:] == (-7 if t.dtype == torch.int64 else -9)).all() for t in outs[1:])
            else:
                got3 += list(want3[3:])
                assert (outs[0] == 0x5A).all()
            same(got3, want3, R.NAMES, ("map_long_dev", fill))


def test_no_patterns_and_empty_reads(O, pkg, ctx):
    with index_of(O, pkg, ctx, "dna", "records") as fm:
        off, anc, skipped = fm.anchors([], 12)
        assert off.tolist() == [0] and anc.shape == (0, 3) and anc.dtype == np.uint64 and skipped.dtype == np.uint32 and len(skipped) == 0
        assert [a.tolist() for a in fm.chain(off, anc)] == [[0]] + [[]] * 7
        assert [a.tolist() for a in fm.map_long([], 12)] == [[0]] + [[]] * 12
        res = fm.map_long([b"", b"\x01" * 40, b""], 12, max_sec=5)
        assert res[0].tolist() == [0, 0, 0, 0] and res[1].tolist() == [0, 0, 0] and res[2].tolist() == [0, 0, 0]
        same(res, R.map_long(K.text_of("dna").tobytes(), K.starts_of("dna", "records"), [b"", b"\x01" * 40, b""], 12, 500, 5000, 500, 40, 5),
             R.NAMES, "empty reads")


def test_bad_arguments(O, pkg, ctx):
    text = K.text_of("dna")
    reads = [text[100:400].tobytes()]
    sets = C.chain_sets()["worked example"][0]
    off, rows = C.offsets_and_rows(sets)
    with index_of(O, pkg, ctx, "dna", "records") as fm:
        def refused(call):
            with pytest.raises(pkg.PfpError) as e:
                call()
            assert e.value.code == EINVAL, e.value
        unsorted = rows[[1, 0, 2, 3, 4, 5]]
        refused(lambda: fm.chain(off, unsorted))
        refused(lambda: fm.chain(off, np.concatenate([rows[:3], rows[2:5]])))            # equal neighbours: not strictly increasing
        zero = rows.copy()
        zero[2, 1] = 0
        refused(lambda: fm.chain(off, zero))
        wide = rows.copy()
        wide[5, 0] = 2**32 - 35                                                           # i + len = 2^32
        refused(lambda: fm.chain(off, wide))
        refused(lambda: fm.chain(np.array([0, 4, 3, 6], dtype=np.uint64), rows))          # offsets that decrease
        refused(lambda: fm.anchors(reads, 12, max_occ=0))
        refused(lambda: fm.anchors(reads, 12, max_occ=65537))
        refused(lambda: fm.anchors(reads, 0))
        refused(lambda: fm.map_long(reads, 0))
        refused(lambda: fm.map_long(reads, 12, max_occ=0))
        refused(lambda: fm.chain(off, rows, max_gap=0))
        refused(lambda: fm.chain(off, rows, max_gap=2**31))
        refused(lambda: fm.chain(off, rows, band=0))
        refused(lambda: fm.chain(off, rows, min_score=0))
        refused(lambda: fm.map_long(reads, 12, max_gap=0))
        refused(lambda: fm.anchors(reads, 12, thresholds=True))                           # an index without thresholds
        assert fm.chain(off, rows, min_score=20)[1].tolist() == [124, 57]                 # and the index still works
        assert fm.map_long(reads, 12)[2].tolist() == [1]
    bwt = O.simplebwt(text)
    with ctx.fm_index(bwt, *samples(pkg, bwt, R_full_sa(O, text))) as plain:              # an index without text
        refused_plain = []
        for call in (lambda: plain.anchors(reads, 12), lambda: plain.chain(off, rows), lambda: plain.map_long(reads, 12)):
            with pytest.raises(pkg.PfpError) as e:
                call()
            refused_plain.append(e.value.code)
        assert refused_plain == [EINVAL] * 3


def R_full_sa(O, text):
    import approx_reference
    return approx_reference.full_sa(O, text)


def test_the_cases_are_not_vacuous():
    """asserted on the reference's own output: the reads and the anchor sets reach every kind of answer"""
    kinds = set()
    for case, (name, table, min_seed, max_occ, G, B, S, max_sec) in C.READ_CASES.items():
        tb, starts = K.text_of(name).tobytes(), C.starts_of(name, table)
        for read in C.reads_of(case):
            both, layer1 = R.read_chains(tb, starts, read, min_seed, max_occ, G, B, S)
            mq = R.mapq_of([c["score"] for _, c in both])
            kinds.add("mapq 0" if both and mq == 0 else "mapq 60" if mq == 60 else "mapq between" if both else "no chain")
            kinds |= {"n >= 3"} if any(c["n"] >= 3 for _, c in both) else set()
            kinds |= {"two kept chains"} if len(both) >= 2 else set()
            kinds |= {"strand-1 primary"} if both and both[0][0] == 1 else set()
            for anc, skipped, dropped in layer1:
                kinds |= ({"skipped MEM"} if skipped else set()) | ({"dropped at a border"} if dropped else set())
                _, gone, stopped = R.peel(anc, *R.programme(anc, starts, len(tb), G, B), S)
                kinds |= ({"dropped chain"} if gone else set()) | ({"stopped at a visited anchor"} if stopped else set())
    starts = K.starts_of(C.CHAIN_TEXT, C.CHAIN_TABLE)
    for name, (sets, G, B, S, max_chains) in C.chain_sets().items():
        for anc in sets:
            _, gone, stopped = R.peel(anc, *R.programme(anc, starts, 20000, G, B), S)
            kinds |= ({"dropped chain"} if gone else set()) | ({"stopped at a visited anchor"} if stopped else set())
    want = {"n >= 3", "two kept chains", "dropped chain", "stopped at a visited anchor", "skipped MEM", "dropped at a border", "strand-1 primary",
            "mapq 0", "mapq 60", "mapq between", "no chain"}
    assert want <= kinds, want - kinds
