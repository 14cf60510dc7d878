"""Mapping read pairs on the GPU (csrc/fmpair.hip): FmIndex.map_pairs / map_pairs_dev.

Definitions (include/pfpgpu.h, "Mapping read pairs").  Every expected value comes from pair_reference.py - the definitions in
plain Python, checked against hand-worked literals in test_pair_reference.py - applied to what FmIndex.map_reads returns with
max_sec = C - 1 and to window_reference as the rescue (both lower calls have their own tests), and every array is compared exactly.
Every returned script also goes through cigar_reference.validate and every MD string through the rebuild of the text's span.

Pairs: pair_cases.py - fragments of `dna` and `copies` cut into the records of map_cases.TABLES."""
import numpy as np
import pytest

import approx_reference as R
import cigar_reference as G
import map_cases as K
import map_reference as M
import ms_reference as MS
import pair_cases as PC
import pair_reference as P
import window_reference as W

pytestmark = pytest.mark.gpu

EINVAL = -1
L, LO, HI = PC.MIN_SEED, PC.MIN_INS, PC.MAX_INS


def samples(pkg, bwt, sa):
    """.ssa / .esa bytes from the BWT and SA[0..n]: <j, SA[j]> of the run starts / ends"""
    b = np.asarray(bwt)
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    ends = np.flatnonzero(np.concatenate([b[1:] != b[:-1], [True]]))
    pk = lambda rows: pkg.pack5(np.stack([rows, sa[rows]], axis=1).reshape(-1).astype(np.uint64))
    return pk(starts), pk(ends)


_parts = {}


def index_of(O, pkg, ctx, name, table="records"):
    if name not in _parts:
        text = K.text_of(name)
        bwt = O.simplebwt(text)
        _parts[name] = (bwt,) + samples(pkg, bwt, R.full_sa(O, text))
    bwt, ssa, esa = _parts[name]
    return ctx.fm_index_ms(bwt, ssa, esa, K.text_of(name)).set_sequences(K.starts_of(name, table))


_memo, _rescues = {}, {}


def expected(fm, name, reads, k, C, thresholds=False, table="records"):
    """the reference's arrays, from FmIndex.map_reads and window_reference"""
    text = K.text_of(name)
    pats = M.interleaved(reads)
    memo = _rescues.setdefault((name, k), {})

    def rescue(r, strand, lo, hi):
        key = (pats[2 * r + strand], lo, hi)
        if key not in memo:
            memo[key] = W.window_one(text, key[0], lo, hi, k)
        return memo[key]
    res = fm.map_reads(reads, k, L, C - 1, thresholds)
    return P.map_pairs(text, K.starts_of(name, table), reads, res, rescue, k, LO, HI, C, _memo.setdefault((name, k), {}))


def same(got, want, what):
    assert len(got) == len(want) == len(P.PAIR_NAMES)
    for g, w, nm in zip(got, want, P.PAIR_NAMES):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, nm, np.flatnonzero(g != w)[:8] if g.shape == w.shape else (g.shape, w.shape))


def check_alignments(name, reads, res, k):
    """every reported alignment lies inside its record, its script replays against the strand's pattern and its span, and its MD
    string rebuilds the span"""
    tb = K.text_of(name).tobytes()
    starts = K.TABLES[(name, "records")]
    pats = M.interleaved(reads)
    for r, (_, _, mapped, _, _, _, strand, q, off, s, d, _, runs, md) in enumerate(P.per_pair_read(res)):
        if not mapped:
            assert (q, off, s, d, runs, md) == (2**32 - 1, 2**64 - 1, 2**64 - 1, 0xFF, (), b""), r
            continue
        e = s + sum(x >> 4 for x in runs if x & 15 != G.OP_I)
        assert starts[q] + off == s and starts[q] <= s < e <= starts[q + 1], (r, s, e, q)
        G.validate(pats[2 * r + strand], tb[s:e], runs, d)
        assert M.rebuild_span(pats[2 * r + strand], runs, md) == tb[s:e], (r, md)


@pytest.mark.parametrize("C", [1, 2, 8])
@pytest.mark.parametrize("k", [0, 1, 8])
def test_map_pairs(O, pkg, wctx, k, C):
    assert pkg.PAIR_NAMES == P.PAIR_NAMES
    for name, _ in PC.TEXTS:
        reads = PC.reads_of(name)
        with index_of(O, pkg, wctx, name) as fm:
            got = fm.map_pairs(reads, k, L, LO, HI, anchors=C)
            same(got, expected(fm, name, reads, k, C), (name, k, C))
            check_alignments(name, reads, got, k)


def test_map_pairs_with_thresholds(O, pkg, ctx):
    reads = PC.reads_of("dna")
    with index_of(O, pkg, ctx, "dna") as fm:
        fm.add_thresholds()
        got = fm.map_pairs(reads, 8, L, LO, HI, thresholds=True)
        same(got, expected(fm, "dna", reads, 8, 8, thresholds=True), "thresholds")
        check_alignments("dna", reads, got, 8)


def test_the_cases_are_not_vacuous(O, pkg, ctx):
    """asserted on the reference's own output: the pairs reach every kind of answer"""
    kinds = set()
    for name, k, C in (("dna", 8, 8), ("dna", 0, 8), ("copies", 8, 8), ("copies", 8, 1)):
        reads = PC.reads_of(name)
        starts = K.TABLES[(name, "records")]
        with index_of(O, pkg, ctx, name) as fm:
            res = expected(fm, name, reads, k, C)
        per = P.per_pair_read(res)
        for q, (kind, _, _) in enumerate(PC.pairs_of(name)):
            a, b = per[2 * q], per[2 * q + 1]
            prop, npairs = a[0], a[1]
            if C < max(a[5], b[5]):
                kinds.add("C smaller than nhits")
            if prop:
                kinds.add("proper by rescue" if a[3] or b[3] else "proper by anchors")
                kinds.add("pair mapq %s" % ({0: "0", 60: "60"}.get(a[4], "between")))
                kinds |= {"rescued mate %d" % (t + 1) for t in (0, 1) if per[2 * q + t][3]}
                if kind == "insert %d" % (HI + 1) and npairs == 1 and k:
                    kinds.add("a same-locus pair not counted")
                if kind.startswith("rescue at a record"):
                    kinds.add("a rescue window clipped by a record boundary")
            elif a[2] and b[2]:
                kinds.add("discordant by record" if a[7] != b[7] else "discordant by orientation" if a[6] == b[6] or kind == "facing outwards"
                          else "discordant by distance")
                kinds.add("tlen %s" % ("0" if a[11] == 0 else "tie" if a[9] == b[9] else "+-"))
            else:
                kinds.add("both mates unmapped" if not a[2] and not b[2] else "one mate unmapped")
    want = {"proper by anchors", "proper by rescue", "rescued mate 1", "rescued mate 2", "pair mapq 0", "pair mapq 60", "pair mapq between",
            "a same-locus pair not counted", "a rescue window clipped by a record boundary", "C smaller than nhits", "discordant by record",
            "discordant by orientation", "discordant by distance", "one mate unmapped", "both mates unmapped", "tlen 0", "tlen tie", "tlen +-"}
    assert want <= kinds, want - kinds
    # the rescued mate of 40 bytes, an edit every 10 bytes, has no maximal exact match of min_seed bytes on either strand
    tb = K.text_of("dna").tobytes()
    sa = R.full_sa(O, K.text_of("dna"))
    mate = next(b for kind, _, b in PC.pairs_of("dna") if kind == "rescue of mate 2")
    assert len(mate) == 40
    for p in (mate, M.revcomp(mate)):
        assert not MS.mems_from_lengths(MS.ms_lengths(tb, sa, p), L)


def test_order_and_groups_do_not_matter(O, pkg, wctx, monkeypatch):
    """shuffled pairs give the shuffled results; PFP_FM_SEQ_BUDGET cuts the host call into groups of whole pairs, PFP_FM_WINDOW_CELLS
    the rescues into pieces: nothing changes"""
    for v in ("PFP_FM_SEQ_BUDGET", "PFP_FM_WINDOW_CELLS"):
        monkeypatch.delenv(v, raising=False)
    reads = PC.reads_of("dna")
    npair = len(reads) // 2
    with index_of(O, pkg, wctx, "dna") as fm:
        base = P.per_pair_read(fm.map_pairs(reads, 8, L, LO, HI))
        order = np.random.default_rng(3).permutation(npair).tolist()
        shuffled = [reads[2 * q + t] for q in order for t in (0, 1)]
        assert P.per_pair_read(fm.map_pairs(shuffled, 8, L, LO, HI)) == [base[2 * q + t] for q in order for t in (0, 1)]
        for budget in ("1", "9"):                           # every pair alone; groups of a few pairs
            monkeypatch.setenv("PFP_FM_SEQ_BUDGET", budget)
            assert P.per_pair_read(fm.map_pairs(reads, 8, L, LO, HI)) == base, budget
        monkeypatch.delenv("PFP_FM_SEQ_BUDGET")
        monkeypatch.setenv("PFP_FM_WINDOW_CELLS", "30000")
        assert P.per_pair_read(fm.map_pairs(reads, 8, L, LO, HI)) == base


def test_device_call(O, pkg, ctx):
    """map_pairs = map_pairs_dev; what lies behind the outputs stays; the library's two buffers go back to the pool"""
    import torch
    reads = PC.reads_of("dna")
    dev = torch.device("cuda", ctx.device)
    pat, off = pkg.pfp._patterns(reads)
    npat = len(reads)
    up = lambda a, view: torch.from_numpy(a.view(view).copy()).to(dev)
    d_pat, d_poff = up(pat, np.uint8), up(off, np.int64)
    sizes = [npat // 2, npat // 2] + [npat] * 10 + [npat + 1, npat + 1]
    kinds = [np.uint8, np.uint64, np.uint8, np.uint8, np.uint8, np.uint64, np.uint8, np.uint32, np.uint64, np.uint64, np.uint8, np.int64, np.uint64, np.uint64]
    tdt = {np.uint8: torch.uint8, np.uint32: torch.int32, np.uint64: torch.int64, np.int64: torch.int64}
    bufs = [torch.full((s + 4,), 0x5A, dtype=tdt[dt], device=dev) for s, dt in zip(sizes, kinds)]
    torch.cuda.synchronize()
    with index_of(O, pkg, ctx, "dna") as fm:
        want = fm.map_pairs(reads, 8, L, LO, HI)
        d_cig, d_md = fm.map_pairs_dev(d_pat.data_ptr(), d_poff.data_ptr(), npat, 8, L, LO, HI, *[b.data_ptr() for b in bufs])
        host = [b[:s].cpu().numpy().view(dt) for b, s, dt in zip(bufs, sizes, kinds)]
        got = host[:12] + [host[12], ctx.fetch_dev(d_cig, 4 * int(host[12][-1])).view(np.uint32), host[13], ctx.fetch_dev(d_md, int(host[13][-1]))]
        ctx.dev_free(d_cig)
        ctx.dev_free(d_md)
    same(got, want, "device")
    assert all((b[s:] == 0x5A).all() for b, s in zip(bufs, sizes))


def test_no_pairs_and_bad_arguments(O, pkg, ctx):
    tb = K.text_of("dna").tobytes()
    pair = list(PC.ends(tb, 2000, 300, 60))
    with index_of(O, pkg, ctx, "dna") as fm:
        res = fm.map_pairs([], 2, L, LO, HI)
        assert [len(x) for x in res] == [0] * 12 + [1, 0, 1, 0] and [x.dtype for x in res] == [x.dtype for x in expected(fm, "dna", [], 2, 8)]
        assert fm.map_pairs(pair, 2, L, LO, HI)[0].tolist() == [1]
        bad = [dict(min_ins=HI + 1, max_ins=HI), dict(min_ins=0, max_ins=pkg.FM_WINDOW_MAX_W + 1), dict(min_ins=LO, max_ins=HI, anchors=0),
               dict(min_ins=LO, max_ins=HI, anchors=pkg.FM_PAIR_MAX_ANCHORS + 1)]
        for kw in bad:
            with pytest.raises(pkg.PfpError) as e:
                fm.map_pairs(pair, 2, L, **kw)
            assert e.value.code == EINVAL, kw
        with pytest.raises(pkg.PfpError) as e:
            fm.map_pairs(pair + pair[:1], 2, L, LO, HI)     # an odd number of reads
        assert e.value.code == EINVAL
        for k, min_seed in ((33, L), (2, 0)):
            with pytest.raises(pkg.PfpError) as e:
                fm.map_pairs(pair, k, min_seed, LO, HI)
            assert e.value.code == EINVAL
        assert fm.map_pairs(pair, 2, L, 0, pkg.FM_WINDOW_MAX_W, anchors=pkg.FM_PAIR_MAX_ANCHORS)[0].tolist() == [1]
