"""Mapping reads on the GPU (csrc/fmmap.hip): FmIndex.map_reads / map_reads_dev.

Definitions (include/pfpgpu.h, "Mapping reads").  Every expected value comes from map_reference.py - the definitions in plain
Python, checked on the CPU in test_map_reference.py - applied to what FmIndex.align returns for the reads and their reverse
complements (that call has its own tests), and every array is compared exactly.  Every returned script also goes through
cigar_reference.validate, every MD string through the rebuild of the text's span, and every hit through the inside test.

Tables and reads: map_cases.py - `copies`, `dna` and `ab` of approx_reference.make_text cut into records (a zero-length record, a
1-byte record, a first and a last record, a single-record table); reads planted with 0..k edits on both strands, across record
boundaries by 1 byte and by half, repeated in several records, equal to their own reverse complement, dense in a^3000, with a
byte the text does not hold, with m <= k, empty and unmappable."""
import numpy as np
import pytest

import approx_reference as R
import cigar_reference as G
import map_cases as K
import map_reference as M

pytestmark = pytest.mark.gpu

EINVAL, ELIMIT = -1, -5
MIN_SEED = 12
CASES = [(name, table, k) for (name, table) in sorted(K.TABLES) for k in (0, 1, 8, 32)]


def samples(pkg, bwt, sa):
    """.ssa / .esa bytes from the BWT and SA[0..n]: <j, SA[j]> of the run starts / ends"""
    b = np.asarray(bwt)
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    ends = np.flatnonzero(np.concatenate([b[1:] != b[:-1], [True]]))
    pk = lambda rows: pkg.pack5(np.stack([rows, sa[rows]], axis=1).reshape(-1).astype(np.uint64))
    return pk(starts), pk(ends)


_parts = {}


def index_of(O, pkg, ctx, name, table=None):
    """an index with text over one of the texts (the BWT and the samples are computed once), with a table of map_cases"""
    if name not in _parts:
        text = K.text_of(name)
        bwt = O.simplebwt(text)
        _parts[name] = (bwt,) + samples(pkg, bwt, R.full_sa(O, text))
    bwt, ssa, esa = _parts[name]
    fm = ctx.fm_index_ms(bwt, ssa, esa, K.text_of(name))
    return fm.set_sequences(K.starts_of(name, table)) if table else fm


_memo = {}


def expected(fm, name, table, reads, k, min_seed, max_secs, thresholds=False):
    """the reference's results for every cap of max_secs, from one call of FmIndex.align"""
    aln = fm.align(M.interleaved(reads), k, min_seed, 0, thresholds)
    return [M.map_reads(K.text_of(name), K.starts_of(name, table), reads, aln, k, ms, _memo.setdefault((name, k), {})) for ms in max_secs]


def same(got, want, what):
    assert len(got) == len(want) == len(M.NAMES)
    for g, w, nm in zip(got, want, M.NAMES):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, nm, np.flatnonzero(g != w)[:8] if g.shape == w.shape else (g.shape, w.shape))


def check_hits(name, table, reads, res, k):
    """every hit lies inside its record, its script replays against the strand's pattern and its span, and its MD string rebuilds
    the span"""
    tb = K.text_of(name).tobytes()
    starts = K.TABLES[(name, table)]
    pats = M.interleaved(reads)
    for p, (mq, nh, hits) in enumerate(M.per_read(res)):
        assert len(hits) <= nh and (nh == 0) == (len(hits) == 0)
        for strand, q, off, s, d, runs, md in hits:
            e = s + sum(r >> 4 for r in runs if r & 15 != G.OP_I)
            assert starts[q] + off == s and starts[q] <= s < e <= starts[q + 1], (p, s, e, q)
            G.validate(pats[2 * p + strand], tb[s:e], runs, d)
            assert M.rebuild_span(pats[2 * p + strand], runs, md) == tb[s:e], (p, md)
        assert [(h[4], h[0], h[3]) for h in hits] == sorted((h[4], h[0], h[3]) for h in hits), p


@pytest.mark.parametrize("name,table,k", CASES)
def test_map_reads(O, pkg, wctx, name, table, k):
    reads = K.reads_of(name, table, k)
    with index_of(O, pkg, wctx, name, table) as fm:
        caps = (0, 1, 1000)
        for max_sec, want in zip(caps, expected(fm, name, table, reads, k, MIN_SEED, caps)):
            got = fm.map_reads(reads, k, MIN_SEED, max_sec)
            same(got, want, (name, table, k, max_sec))
            assert np.array_equal(np.diff(got[0]), np.minimum(got[2], 1 + max_sec))
        check_hits(name, table, reads, got, k)


@pytest.mark.parametrize("name,table", [("copies", "records"), ("dna", "records")])
def test_map_reads_with_thresholds(O, pkg, ctx, name, table):
    reads = K.reads_of(name, table, 8)
    with index_of(O, pkg, ctx, name, table) as fm:
        fm.add_thresholds()
        got = fm.map_reads(reads, 8, MIN_SEED, 2, thresholds=True)
        same(got, expected(fm, name, table, reads, 8, MIN_SEED, (2,), thresholds=True)[0], (name, "thresholds"))
        check_hits(name, table, reads, got, 8)


def test_the_cases_are_not_vacuous(O, pkg, ctx):
    """asserted on the reference's own output: the reads reach every kind of answer"""
    kinds, most = set(), 0
    for name, table, k in (("copies", "records", 8), ("ab", "records", 8), ("dna", "records", 1)):
        reads = K.reads_of(name, table, k)
        starts = K.TABLES[(name, table)]
        with index_of(O, pkg, ctx, name, table) as fm:
            aln = fm.align(M.interleaved(reads), k, MIN_SEED)
            res = M.per_read(M.map_reads(K.text_of(name), starts, reads, aln, k, 1000, _memo.setdefault((name, k), {})))
        off, st, en, _ = (x.tolist() for x in aln)
        for p, (mq, nh, hits) in enumerate(res):
            cands = [(st[j], en[j]) for j in range(off[2 * p], off[2 * p + 2])]
            kinds.add("mapq %d" % mq)
            kinds |= {"unmapped"} if not nh else {"strand %d" % hits[0][0]}
            kinds |= {"several hits"} if nh > 1 else set()
            kinds |= {"across a boundary"} if any(s < e and not M.is_inside(starts, s, e) for s, e in cands) else set()
            kinds |= {"shadowed"} if sum(M.is_inside(starts, s, e) for s, e in cands) > nh else set()
            kinds |= {"dense"} if len(cands) >= 5 else set()
            most = max(most, len(cands))
            kinds |= {"secondary on the other strand"} if len({h[0] for h in hits}) == 2 else set()
            kinds |= {"record %d" % h[1] for h in hits if starts[h[1] + 1] - starts[h[1]] == 1}
            kinds |= {"first record"} if any(h[3] == 0 for h in hits) else set()
            for h in hits:
                kinds |= {G.LETTER[r & 15] for r in h[5]}
    want = {"mapq 0", "mapq 10", "mapq 60", "unmapped", "strand 0", "strand 1", "several hits", "across a boundary", "shadowed", "dense",
            "=", "X", "I", "D"}
    assert want <= kinds, (want - kinds, most)


def test_a_read_that_is_its_own_reverse_complement(O, pkg, wctx):
    """both strands give the same candidates: one hit, on strand 0.  dna[1642:1656] is such a read, and occurs once"""
    text = K.text_of("dna")
    read = text[1642:1656].tobytes()
    assert read == b"AATCGAGCTCGATT" == M.revcomp(read) and text.tobytes().count(read) == 1
    with index_of(O, pkg, wctx, "dna", "records") as fm:
        for k in (0, 1):
            assert fm.align([read, read], k, 12)[0].tolist() == [0, 1, 2]
            hit_off, mapq, nhits, strand, seq, off, start, dist, _, cig, _, md = fm.map_reads([read], k, 12, 1000)
            assert nhits.tolist() == [1] and mapq.tolist() == [60] and strand.tolist() == [0] and dist.tolist() == [0]
            assert start.tolist() == [1642] and seq.tolist() == [2] and off.tolist() == [1641]
            assert cig.tolist() == [14 << 4 | 7] and bytes(md) == b"14"


def test_sanity_on_dna(O, pkg, wctx):
    """`dna` is random: every planted read of 100 bytes with at most 3 edits has, at min_seed = 20, a primary on the planted strand
    that overlaps the planted span, with MAPQ 60 (three edits leave an exact stretch of at least 24 bytes; the CPU references
    alone satisfy this for the same reads: test_map_reference.py)"""
    planted = K.sanity_reads()
    with index_of(O, pkg, wctx, "dna", "records") as fm:
        res = M.per_read(fm.map_reads([r for r, _, _ in planted], 8, 20, 3))
    for (mq, nh, hits), (_, strand, i) in zip(res, planted):
        assert nh >= 1 and mq == 60, (mq, nh, i)
        h = hits[0]
        end = h[3] + sum(r >> 4 for r in h[5] if r & 15 != G.OP_I)
        assert h[0] == strand and max(h[3], i) < min(end, i + 100) and h[4] <= 3, (h, strand, i)


def test_batch_order_budget_and_chunks_do_not_matter(O, pkg, wctx, monkeypatch):
    name, table, k = "copies", "records", 8
    reads = K.reads_of(name, table, k)
    with index_of(O, pkg, wctx, name, table) as fm:
        for v in ("PFP_FM_SEQ_BUDGET", "PFP_FM_CIGAR_SCRATCH"):
            monkeypatch.delenv(v, raising=False)
        base = M.per_read(fm.map_reads(reads, k, MIN_SEED, 2))
        assert sum(nh for _, nh, _ in base) > 20
        order = np.random.default_rng(9).permutation(len(reads)).tolist()
        got = M.per_read(fm.map_reads([reads[i] for i in order], k, MIN_SEED, 2))
        assert got == [base[i] for i in order]
        assert M.per_read(fm.map_reads(reads[5:6] + reads[5:6], k, MIN_SEED, 2)) == [base[5], base[5]]
        for budget in ("1", "40"):                          # every read alone; groups of a few reads
            monkeypatch.setenv("PFP_FM_SEQ_BUDGET", budget)
            assert M.per_read(fm.map_reads(reads, k, MIN_SEED, 2)) == base, budget
        monkeypatch.delenv("PFP_FM_SEQ_BUDGET")
        monkeypatch.setenv("PFP_FM_CIGAR_SCRATCH", str(4 * 2 * 160))
        wctx.set_kernel_trace(True)
        got = M.per_read(fm.map_reads(reads, k, MIN_SEED, 2))
        trace = wctx.kernel_trace()
        wctx.set_kernel_trace(False)
        assert got == base and sum(r["launches"] for r in trace if r["name"] == "fm_cigar") > 1


def test_device_call_and_offsets_only(O, pkg, wctx):
    """map_reads = map_reads_dev; the call without the per-hit outputs gives the same hit_off, mapq and nhits; what lies behind the
    outputs stays; the library's two buffers go back to the pool"""
    import torch
    name, table, k, max_sec = "copies", "records", 8, 1
    reads = K.reads_of(name, table, k)
    dev = torch.device("cuda", wctx.device)
    pat, off = pkg.pfp._patterns(reads)
    npat = len(reads)
    up = lambda a, view: torch.from_numpy(a.view(view).copy()).to(dev)
    d_pat, d_poff = up(pat, np.uint8), up(off, np.int64)
    filled = lambda count, dt, v: torch.full((count,), v, dtype=dt, device=dev)
    host = lambda t, count, dt: t[:count].cpu().numpy().view(dt)
    with index_of(O, pkg, wctx, name, table) as fm:
        want = fm.map_reads(reads, k, MIN_SEED, max_sec)
        H = int(want[0][-1])
        assert H >= 20                                      # (enough hits for the canaries behind the outputs to mean something)
        for fill in (False, True):
            d_hoff, d_mapq, d_nh = filled(npat + 3, torch.int64, -7), filled(npat + 16, torch.uint8, 0x5A), filled(npat + 2, torch.int64, -7)
            d_strand, d_dist = filled(H + 16, torch.uint8, 0x5A), filled(H + 16, torch.uint8, 0x5A)
            d_seq, d_off, d_start = filled(H + 2, torch.int32, -9), filled(H + 2, torch.int64, -7), filled(H + 2, torch.int64, -7)
            d_coff, d_moff = filled(H + 3, torch.int64, -7), filled(H + 3, torch.int64, -7)
            torch.cuda.synchronize()
            per_hit = [t.data_ptr() for t in (d_strand, d_seq, d_off, d_start, d_dist, d_coff, d_moff)] if fill else [None] * 7
            out = fm.map_reads_dev(d_pat.data_ptr(), d_poff.data_ptr(), npat, k, MIN_SEED, d_hoff.data_ptr(), d_mapq.data_ptr(), d_nh.data_ptr(),
                                   *per_hit, max_sec=max_sec)
            got = [host(d_hoff, npat + 1, np.uint64), host(d_mapq, npat, np.uint8), host(d_nh, npat, np.uint64)]
            assert (d_hoff[npat + 1:] == -7).all() and (d_mapq[npat:] == 0x5A).all() and (d_nh[npat:] == -7).all()
            if not fill:
                assert out is None and (d_strand == 0x5A).all() and (d_coff == -7).all()
                same(got + list(want[3:]), want, "offsets only")
                continue
            d_cig, d_md = out
            got += [host(d_strand, H, np.uint8), host(d_seq, H, np.uint32), host(d_off, H, np.uint64), host(d_start, H, np.uint64),
                    host(d_dist, H, np.uint8), host(d_coff, H + 1, np.uint64)]
            moff = host(d_moff, H + 1, np.uint64)
            got += [wctx.fetch_dev(d_cig, 4 * int(got[-1][-1])).view(np.uint32), moff, wctx.fetch_dev(d_md, int(moff[-1]))]
            wctx.dev_free(d_cig)
            wctx.dev_free(d_md)
            same(got, want, "device")
            assert (d_strand[H:] == 0x5A).all() and (d_seq[H:] == -9).all() and (d_coff[H + 1:] == -7).all() and (d_moff[H + 1:] == -7).all()


def test_no_reads_and_reads_without_hits(O, pkg, ctx):
    with index_of(O, pkg, ctx, "dna", "records") as fm:
        res = fm.map_reads([], 2, MIN_SEED)
        assert [x.tolist() for x in res] == [[0], [], [], [], [], [], [], [], [0], [], [0], []]
        assert [x.dtype for x in res] == [x.dtype for x in M.map_reads(K.text_of("dna"), [0, 20000], [], fm.align([], 2, MIN_SEED), 2)]
        res = fm.map_reads([b"", b"\x01" * 40, b""], 2, MIN_SEED, 5)
        assert res[0].tolist() == [0, 0, 0, 0] and res[1].tolist() == [0, 0, 0] and res[2].tolist() == [0, 0, 0]
        assert res[8].tolist() == [0] and res[10].tolist() == [0] and len(res[9]) == 0 and len(res[11]) == 0


def test_bad_arguments(O, pkg, ctx):
    text = K.text_of("dna")
    reads = [text[100:160].tobytes()]
    with index_of(O, pkg, ctx, "dna") as fm:                # no table
        with pytest.raises(pkg.PfpError) as e:
            fm.map_reads(reads, 2, MIN_SEED)
        assert e.value.code == EINVAL and "sequence table" in str(e.value)
        fm.set_sequences(K.starts_of("dna", "records"))
        assert fm.map_reads(reads, 2, MIN_SEED)[2].tolist() == [1]
        for k, min_seed in ((33, MIN_SEED), (-1, MIN_SEED), (2, 0)):
            with pytest.raises(pkg.PfpError) as e:
                fm.map_reads(reads, k, min_seed)
            assert e.value.code == EINVAL
        with pytest.raises(pkg.PfpError) as e:              # thresholds asked of an index without them
            fm.map_reads(reads, 2, MIN_SEED, thresholds=True)
        assert e.value.code == EINVAL
        with pytest.raises(pkg.PfpError) as e:
            fm.map_reads(reads + [b"A" * (pkg.pfp.FM_EXTEND_MAX_M + 1)], 2, MIN_SEED)
        assert e.value.code == ELIMIT
        assert fm.map_reads(reads, 2, MIN_SEED)[2].tolist() == [1]
    bwt = O.simplebwt(text)
    with ctx.fm_index(bwt, *samples(pkg, bwt, R.full_sa(O, text))) as plain:      # an index without text
        plain.set_sequences(K.starts_of("dna", "records"))
        with pytest.raises(pkg.PfpError) as e:
            plain.map_reads(reads, 2, MIN_SEED)
        assert e.value.code == EINVAL
