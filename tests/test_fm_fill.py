"""Aligning chains on the GPU (csrc/fmfill.hip): FmIndex.fill / chain_align / map_long_aln and their _dev variants.

Definitions: include/pfpgpu.h, "Aligning chains".  Every expected value comes from fill_reference.py - the full, unbanded matrix
and the definitions in plain Python, checked on the CPU in test_fill_reference.py - and every array is compared exactly, dtype
included.  Segments, anchor sets and reads: fill_cases.py."""
import numpy as np
import pytest

import chain_cases as C
import chain_reference as R
import fill_cases as FC
import fill_reference as F
import map_cases as K
from test_fm_chain import same
from test_fm_map import index_of, samples

pytestmark = pytest.mark.gpu

EINVAL = -1
SEG_NAMES = ("dist", "cig_off", "cig")


def columns(segs):
    a = np.array(segs, dtype=np.uint64).reshape(-1, 5)
    return a[:, 0].astype(np.uint32), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy(), a[:, 4].copy()


def run_segments(fm, name):
    text, max_fill, pats, segs, _ = FC.segment_sets()[name]
    return fm.fill(pats, *columns(segs), max_fill)


def run_anchor_set(fm, name, max_fill):
    pats, anc, G, B, S, mc = FC.anchor_sets()[name]
    off, rows = C.offsets_and_rows(anc)
    return fm.chain_align(pats, off, rows, G, B, S, mc, max_fill)


def run_reads(fm, case, max_fill):
    name, table, min_seed, max_occ, G, B, S, max_sec = FC.READ_CASES[case]
    return fm.map_long_aln(FC.reads_of(case), min_seed, max_occ, G, B, S, max_sec, max_fill=max_fill)


@pytest.mark.parametrize("name", sorted(FC.segment_sets()))
def test_fill(O, pkg, wctx, name):
    with index_of(O, pkg, wctx, FC.segment_sets()[name][0]) as fm:
        same(run_segments(fm, name), FC.expected_segments(name), SEG_NAMES, name)


def test_fill_equals_cigar_on_whole_patterns(O, pkg, wctx):
    pats, spans = FC.whole_patterns()
    idx = np.arange(len(pats), dtype=np.uint32)
    s, e = np.array([x[0] for x in spans], dtype=np.uint64), np.array([x[1] for x in spans], dtype=np.uint64)
    q1 = np.array([len(p) for p in pats], dtype=np.uint64)
    with index_of(O, pkg, wctx, "dna") as fm:
        d8, off8, cig8 = fm.cigar(pats, idx, s, e, 32)
        for max_fill in (32, 500):
            d, off, cig = fm.fill(pats, idx, np.zeros(len(pats), dtype=np.uint64), q1, s, e, max_fill)
            assert d.dtype == np.uint32 and np.array_equal(d, d8.astype(np.uint32)) and int(d.max()) == 32
            same((off, cig), (off8, cig8), SEG_NAMES[1:], max_fill)


@pytest.mark.parametrize("max_fill", FC.ANCHOR_FILLS)
@pytest.mark.parametrize("name", sorted(FC.anchor_sets()))
def test_chain_align(O, pkg, wctx, name, max_fill):
    with index_of(O, pkg, wctx, "dna", "records") as fm:
        got = run_anchor_set(fm, name, max_fill)
        same(got, FC.expected_anchor_set(name, max_fill), F.CHAIN_ALN_NAMES, (name, max_fill))
        pats, anc, G, B, S, mc = FC.anchor_sets()[name]
        same(got[:8], fm.chain(*C.offsets_and_rows(anc), G, B, S, mc), R.CHAIN_NAMES, name)          # chain()'s fields, untouched
    assert pkg.CHAIN_ALN_NAMES == F.CHAIN_ALN_NAMES


@pytest.mark.parametrize("max_fill", FC.READ_FILLS)
@pytest.mark.parametrize("case", sorted(FC.READ_CASES))
def test_map_long_aln(O, pkg, wctx, case, max_fill):
    name, table, min_seed, max_occ, G, B, S, max_sec = FC.READ_CASES[case]
    with index_of(O, pkg, wctx, name, table) as fm:
        got = run_reads(fm, case, max_fill)
        same(got, FC.expected_reads(case, max_fill), F.LONG_ALN_NAMES, (case, max_fill))
        same(got[:13], fm.map_long(FC.reads_of(case), min_seed, max_occ, G, B, S, max_sec), R.NAMES, case)    # bit-equal to map_long
    assert pkg.LONG_ALN_NAMES == F.LONG_ALN_NAMES


def test_chain_align_of_the_anchors_of_reads(O, pkg, wctx):
    """layer 2 over layer 1's output: true anchors of real reads, against the reference on the same anchors"""
    case = "dna noisy"
    name, table, min_seed, max_occ, G, B, S, _ = FC.READ_CASES[case]
    reads = [bytes(r) for r in FC.reads_of(case)]
    with index_of(O, pkg, wctx, name, table) as fm:
        off, anc, _ = fm.anchors(reads, min_seed, max_occ)
        got = fm.chain_align(reads, off, anc, G, B, S, 3, 500)
    per = [[tuple(int(v) for v in row) for row in anc[int(off[p]):int(off[p + 1])]] for p in range(len(off) - 1)]
    want = F.chain_align(K.text_of(name), K.starts_of(name, table), reads, per, G, B, S, 3, 500)
    same(got, want, F.CHAIN_ALN_NAMES, case)
    assert int(got[10].max()) > 32


SETTINGS = (("PFP_FM_FILL_SCRATCH", "4096"), ("PFP_FM_CHAIN_STEPS", "1"), ("PFP_FM_CHAIN_STEPS", "7"), ("PFP_FM_SEQ_BUDGET", "3"))


@pytest.mark.parametrize("setting", SETTINGS, ids=["%s=%s" % s for s in SETTINGS])
def test_scratch_steps_and_budget_do_not_matter(O, pkg, wctx, monkeypatch, setting):
    for v in ("PFP_FM_FILL_SCRATCH", "PFP_FM_CHAIN_STEPS", "PFP_FM_SEQ_BUDGET"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(*setting)
    for text in ("dna", "ab"):
        with index_of(O, pkg, wctx, text) as fm:
            for name, s in FC.segment_sets().items():
                if s[0] == text:
                    same(run_segments(fm, name), FC.expected_segments(name), SEG_NAMES, (name, setting))
    with index_of(O, pkg, wctx, "dna", "records") as fm:
        for name in FC.anchor_sets():
            for max_fill in FC.ANCHOR_FILLS:
                same(run_anchor_set(fm, name, max_fill), FC.expected_anchor_set(name, max_fill), F.CHAIN_ALN_NAMES, (name, max_fill, setting))
    for case in sorted(FC.READ_CASES):
        if setting == ("PFP_FM_CHAIN_STEPS", "1") and case == "ab":
            continue                                        # (thousands of launches for its 4844 anchors: 7 covers it)
        with index_of(O, pkg, wctx, *FC.READ_CASES[case][:2]) as fm:
            for max_fill in FC.READ_FILLS:
                same(run_reads(fm, case, max_fill), FC.expected_reads(case, max_fill), F.LONG_ALN_NAMES, (case, max_fill, setting))


def test_device_calls(O, pkg, wctx):
    """the _dev variants equal the host calls; the forms without runs give the same offsets; what lies behind the outputs stays"""
    import torch
    dev = torch.device("cuda", wctx.device)
    up = lambda a, view: torch.from_numpy(np.ascontiguousarray(a).view(view).copy()).to(dev)
    filled = lambda count, dt, v: torch.full((count,), v, dtype=dt, device=dev)
    host = lambda t, count, dt: t[:count].cpu().numpy().view(dt)
    ptr = lambda t: t.data_ptr()
    # layer 1
    text, max_fill, pats, segs, _ = FC.segment_sets()["shapes"]
    pat, off = pkg.pfp._patterns(pats)
    sp, q0, q1, t0, t1 = columns(segs)
    ns = len(segs)
    with index_of(O, pkg, wctx, "dna", "records") as fm:
        want = fm.fill(pats, sp, q0, q1, t0, t1, max_fill)
        d_pat, d_poff = up(pat, np.uint8), up(off, np.int64)
        d_seg = [up(sp, np.int32)] + [up(a, np.int64) for a in (q0, q1, t0, t1)]
        total = int(want[1][-1])
        assert total >= 50
        for with_runs in (False, True):
            d_dist, d_coff, d_cig = filled(ns + 2, torch.int32, -9), filled(ns + 3, torch.int64, -7), filled(total + 2, torch.int32, -9)
            torch.cuda.synchronize()
            fm.fill_dev(ptr(d_pat), ptr(d_poff), len(pats), *(ptr(t) for t in d_seg), ns, max_fill, ptr(d_dist), ptr(d_coff),
                        ptr(d_cig) if with_runs else None)
            same((host(d_dist, ns, np.uint32), host(d_coff, ns + 1, np.uint64)), want[:2], SEG_NAMES[:2], "fill_dev")
            assert (d_dist[ns:] == -9).all() and (d_coff[ns + 1:] == -7).all()
            if with_runs:
                assert np.array_equal(host(d_cig, total, np.uint32), want[2]) and (d_cig[total:] == -9).all()
            else:
                assert (d_cig == -9).all()
        # layer 2
        pats, anc, G, B, S, mc = FC.anchor_sets()["chain_cases: random"]
        aoff, rows = C.offsets_and_rows(anc)
        want = fm.chain_align(pats, aoff, rows, G, B, S, mc, 500)
        pat, off = pkg.pfp._patterns(pats)
        npat = len(pats)
        d_pat, d_poff, d_aoff, d_anc = up(pat, np.uint8), up(off, np.int64), up(aoff, np.int64), up(rows.reshape(-1), np.int64)
        Cn, Rn, Mn = int(want[0][-1]), int(want[12][-1]), int(want[14][-1])
        assert Cn >= 20 and Rn >= 100 and Mn >= 100
        d_coff = filled(npat + 3, torch.int64, -7)
        torch.cuda.synchronize()
        fm.chain_align_dev(ptr(d_pat), ptr(d_poff), npat, ptr(d_aoff), ptr(d_anc), ptr(d_coff), max_gap=G, band=B, min_score=S, max_chains=mc)
        assert np.array_equal(host(d_coff, npat + 1, np.uint64), want[0]) and (d_coff[npat + 1:] == -7).all()
        kinds = [torch.int64 if w.dtype == np.uint64 else torch.int32 for w in want[1:12]]
        for with_runs in (False, True):
            outs = [filled(Cn + 2, k, -7 if k == torch.int64 else -9) for k in kinds]
            d_goff, d_cig = filled(Cn + 4, torch.int64, -7), filled(Rn + 2, torch.int32, -9)
            d_moff, d_mem = filled(Cn + 4, torch.int64, -7), filled(Mn + 2, torch.int32, -9)
            torch.cuda.synchronize()
            fm.chain_align_dev(ptr(d_pat), ptr(d_poff), npat, ptr(d_aoff), ptr(d_anc), ptr(d_coff), *(ptr(t) for t in outs), ptr(d_goff),
                               ptr(d_cig) if with_runs else None, ptr(d_moff) if with_runs else None, ptr(d_mem) if with_runs else None,
                               max_gap=G, band=B, min_score=S, max_chains=mc, max_fill=500)
            got = [host(d_coff, npat + 1, np.uint64)] + [host(t, Cn, w.dtype) for t, w in zip(outs, want[1:12])] + [host(d_goff, Cn + 1, np.uint64)]
            same(got, want[:13], F.CHAIN_ALN_NAMES[:13], ("chain_align_dev", with_runs))
            assert all((t[Cn:] == (-7 if t.dtype == torch.int64 else -9)).all() for t in outs) and (d_goff[Cn + 1:] == -7).all()
            if with_runs:
                same((host(d_cig, Rn, np.uint32), host(d_moff, Cn + 1, np.uint64), host(d_mem, Mn, np.uint32)), want[13:], F.CHAIN_ALN_NAMES[13:], "runs")
                assert (d_cig[Rn:] == -9).all() and (d_moff[Cn + 1:] == -7).all() and (d_mem[Mn:] == -9).all()
            else:
                assert (d_cig == -9).all() and (d_moff == -7).all() and (d_mem == -9).all()
        # layer 3
        case = "dna noisy"
        name, table, min_seed, max_occ, G, B, S, max_sec = FC.READ_CASES[case]
        reads = FC.reads_of(case)
        want = run_reads(fm, case, 500)
        pat, off = pkg.pfp._patterns(reads)
        npat = len(reads)
        d_pat, d_poff = up(pat, np.uint8), up(off, np.int64)
        H, Rn = int(want[0][-1]), int(want[17][-1])
        assert H >= 5 and Rn >= 100
        tk = lambda w: torch.uint8 if w.dtype == np.uint8 else torch.int64 if w.dtype == np.uint64 else torch.int32
        fv = lambda k: 0x5A if k == torch.uint8 else -7 if k == torch.int64 else -9
        for mode in ("offsets", "fields", "runs"):
            d_hoff, d_mapq, d_nc = filled(npat + 3, torch.int64, -7), filled(npat + 16, torch.uint8, 0x5A), filled(npat + 2, torch.int64, -7)
            outs = [filled(H + 16, tk(w), fv(tk(w))) for w in want[3:17]]
            d_goff, d_cig = filled(H + 4, torch.int64, -7), filled(Rn + 2, torch.int32, -9)
            torch.cuda.synchronize()
            rest = [None] * 16 if mode == "offsets" else [ptr(t) for t in outs] + [ptr(d_goff), ptr(d_cig) if mode == "runs" else None]
            fm.map_long_aln_dev(ptr(d_pat), ptr(d_poff), npat, min_seed, ptr(d_hoff), ptr(d_mapq), ptr(d_nc), *rest, max_occ=max_occ, max_gap=G,
                                band=B, min_score=S, max_sec=max_sec, max_fill=500)
            same([host(d_hoff, npat + 1, np.uint64), host(d_mapq, npat, np.uint8), host(d_nc, npat, np.uint64)], want[:3], F.LONG_ALN_NAMES[:3], mode)
            assert (d_hoff[npat + 1:] == -7).all() and (d_mapq[npat:] == 0x5A).all() and (d_nc[npat:] == -7).all()
            if mode == "offsets":
                assert all((t == fv(t.dtype)).all() for t in outs) and (d_goff == -7).all()
                continue
            same([host(t, H, w.dtype) for t, w in zip(outs, want[3:17])] + [host(d_goff, H + 1, np.uint64)], want[3:18], F.LONG_ALN_NAMES[3:18], mode)
            assert all((t[H:] == fv(t.dtype)).all() for t in outs) and (d_goff[H + 1:] == -7).all()
            if mode == "runs":
                assert np.array_equal(host(d_cig, Rn, np.uint32), want[18]) and (d_cig[Rn:] == -9).all()
            else:
                assert (d_cig == -9).all()


def test_nothing_to_align(O, pkg, ctx):
    with index_of(O, pkg, ctx, "dna", "records") as fm:
        z64 = np.zeros(0, dtype=np.uint64)
        got = fm.fill([], np.zeros(0, dtype=np.uint32), z64, z64, z64, z64, 10)
        assert [a.tolist() for a in got] == [[], [0], []] and got[0].dtype == np.uint32
        got = fm.chain_align([], np.zeros(1, dtype=np.uint64), np.zeros((0, 3), dtype=np.uint64))
        assert [a.tolist() for a in got] == [[0]] + [[]] * 11 + [[0], [], [0], []]
        got = fm.map_long_aln([], 12)
        assert [a.tolist() for a in got] == [[0]] + [[]] * 16 + [[0], []]
        reads = [b"", b"\x01" * 40, b""]
        same(fm.map_long_aln(reads, 12, max_sec=5), F.map_long_aln(K.text_of("dna").tobytes(), K.starts_of("dna", "records"), reads, 12, 500, 5000, 500,
                                                                    40, 5, 500), F.LONG_ALN_NAMES, "empty reads")


def test_bad_arguments(O, pkg, ctx):
    text = K.text_of("dna")
    reads = [text[100:400].tobytes()]
    pats, anc, G, B, S, mc = FC.anchor_sets()["true anchors"]
    off, rows = C.offsets_and_rows(anc)
    one = (np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.full(1, 10, dtype=np.uint64), np.full(1, 100, dtype=np.uint64),
           np.full(1, 110, dtype=np.uint64))

    def refused(call):
        with pytest.raises(pkg.PfpError) as e:
            call()
        assert e.value.code == EINVAL, e.value

    with index_of(O, pkg, ctx, "dna", "records") as fm:
        for bad in (pkg.FM_FILL_MAX_F + 1, 2**40):
            refused(lambda: fm.fill(reads, *one, bad))
            refused(lambda: fm.chain_align(pats, off, rows, max_fill=bad))
            refused(lambda: fm.map_long_aln(reads, 12, max_fill=bad))
        refused(lambda: fm.chain_align(pats, off, rows[::-1].copy()))                     # pfp_fm_chain's refusals hold
        refused(lambda: fm.chain_align(pats, off, rows, max_gap=0))
        refused(lambda: fm.map_long_aln(reads, 0))
        assert fm.fill(reads, *one, pkg.FM_FILL_MAX_F)[0].tolist() == [0]                 # and the index still works
        assert fm.map_long_aln(reads, 12)[2].tolist() == [1]
        assert pkg.FM_FILL_MAX_F == 4096 and pkg.FM_FILL_MAX_LEN == 65535
    bwt = O.simplebwt(text)
    import approx_reference
    with ctx.fm_index(bwt, *samples(pkg, bwt, approx_reference.full_sa(O, text))) as plain:      # an index without text
        refused(lambda: plain.fill(reads, *one, 10))
        refused(lambda: plain.chain_align(pats, off, rows))
        refused(lambda: plain.map_long_aln(reads, 12))
