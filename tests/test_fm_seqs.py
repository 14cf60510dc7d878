"""Sequence-aware locate, position -> (sequence, offset) and document listing on the GPU (csrc/seqmap.hip): FmIndex.set_sequences /
seqmap / locate_seqs / doclist and their _dev variants.

Definitions: include/pfpgpu.h, "Sequences of a collection".  Every expected value comes from tests/seq_reference.py over the
oracle's suffix array: numpy.searchsorted for the mapping, the definition x + m <= starts[k + 1] for the filter, numpy.unique for
the documents."""
import numpy as np
import pytest

import seq_reference as R
from test_fm_search import expected, full_sa, patterns_for, samples, small_texts

pytestmark = pytest.mark.gpu

EINVAL = -1
TEXTS = ["fasta", "dna", "a_n", "all_bytes"]
TABLES = ["one", "parts64", "bytes", "empties", "big"]
_cache = {}


def text_case(O, pkg, which):
    """text, SA[0..n], BWT and samples of a text of test_fm_search.small_texts (dna cut to 120 000 bytes), made once"""
    if which not in _cache:
        text = dict(small_texts(O))[which]
        if which == "dna":
            text = text[:120_000]
        text = np.ascontiguousarray(text, dtype=np.uint8)
        sa = full_sa(O, text)
        bwt = O.simplebwt(text)
        ssa, esa = samples(pkg, bwt, sa)
        _cache[which] = dict(text=text, tb=text.tobytes(), sa=sa, bwt=bwt, ssa=ssa, esa=esa)
    return _cache[which]


def make_table(n, kind):
    if kind == "one":
        st = [0, n]
    elif kind == "parts64":
        st = (np.arange(65, dtype=np.uint64) * np.uint64(n)) // np.uint64(64)
    elif kind == "bytes":
        st = np.arange(n + 1)
    elif kind == "empties":          # runs of empty sequences at the front, in the middle and at the end
        st = [0, 0, 0, n // 5, n // 2, n // 2, n // 2, n // 2, 3 * n // 4, n, n, n]
    else:                             # more than 200 000 sequences: most of them empty or a few bytes long
        rng = np.random.default_rng(99)
        st = np.concatenate([[0], np.sort(rng.integers(0, n + 1, 200_499)), [n]])
    return np.asarray(st, dtype=np.uint64)


def patterns(tb, starts, seed):
    n = len(tb)
    pats = patterns_for(np.frombuffer(tb, dtype=np.uint8), seed)
    inner = np.unique(starts[(starts > 0) & (starts < n)])
    for b in inner[np.linspace(0, len(inner) - 1, min(len(inner), 5)).astype(int)] if len(inner) else []:
        b = int(b)
        for k in (1, 2, 5, 16):                      # cut from the text, centred on a boundary: at least that occurrence spans
            if b - k >= 0 and b + k <= n:
                pats.append(tb[b - k:b + k])
    longest = int(np.max(np.diff(starts.astype(np.int64))))
    if longest < n:
        pats.append(tb[:longest + 1])                # longer than the longest sequence: nothing is kept
    if tb[:1] == b"a":
        pats += [b"a", b"aa", b"a" * 1000]
    return pats


def reference(case, starts, pats, max_occ=0):
    """per pattern (seq, off) of locate_seqs and (docs, cnt) of doclist, plus the numbers of kept and dropped occurrences"""
    sa = case["sa"]
    loc, docs, kept, dropped = [], [], 0, 0
    for p, (s, e) in zip(pats, expected(case["text"], sa, pats)):
        rows = sa[s:e].astype(np.uint64)
        loc.append(R.locate_seqs(starts, rows, len(p), max_occ))
        docs.append(R.doclist(starts, rows, len(p)))
        k = R.keep(starts, rows, len(p))
        kept += int(k.sum())
        dropped += int((~k & (rows < starts[-1])).sum())
    return loc, docs, kept, dropped


def check_locate(got, want):
    off, seq, offset = got
    assert len(off) == len(want) + 1 and int(off[0]) == 0 and int(off[-1]) == len(seq) == len(offset)
    for k, (ws, wo) in enumerate(want):
        a, b = int(off[k]), int(off[k + 1])
        assert b - a == len(ws), (k, b - a, len(ws))
        assert np.array_equal(seq[a:b], ws) and np.array_equal(offset[a:b], wo), k


def check_docs(got, want):
    off, doc, cnt = got
    assert len(off) == len(want) + 1 and int(off[0]) == 0 and int(off[-1]) == len(doc) == len(cnt)
    for k, (wd, wc) in enumerate(want):
        a, b = int(off[k]), int(off[k + 1])
        assert np.array_equal(doc[a:b], wd) and np.array_equal(cnt[a:b], wc), k


def dev_calls(fm, pats, max_occ):
    """the same answers through the device-pointer calls: (off, seq, offset), (doc_off, doc, cnt), and the offsets-only results"""
    import torch
    dev = torch.device("cuda", 0)
    npat = len(pats)
    lens = np.array([len(p) for p in pats], dtype=np.int64)
    d_pat = torch.from_numpy(np.frombuffer(b"".join(pats) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    z = lambda k, dt=torch.int64: torch.zeros(k, dtype=dt, device=dev)
    sp, ep, first, uoff = z(npat), z(npat), z(npat), z(npat + 1)
    torch.cuda.synchronize()
    fm.count_dev(d_pat.data_ptr(), d_off.data_ptr(), npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr())
    fm.locate_dev(npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr(), max_occ, uoff.data_ptr())
    U = int(uoff[-1])
    only, off, seq, offset = z(npat + 1), z(npat + 1), z(U + 1, torch.int32), z(U + 1)
    torch.cuda.synchronize()
    args = (d_off.data_ptr(), npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr())
    fm.locate_seqs_dev(*args, max_occ, only.data_ptr())
    fm.locate_seqs_dev(*args, max_occ, off.data_ptr(), seq.data_ptr(), offset.data_ptr())
    K = int(off[-1])
    assert K <= U
    donly, doff = z(npat + 1), z(npat + 1)
    fm.doclist_dev(*args, donly.data_ptr())
    D = int(donly[-1])
    doc, cnt = z(D + 1, torch.int32), z(D + 1)
    torch.cuda.synchronize()
    fm.doclist_dev(*args, doff.data_ptr(), doc.data_ptr(), cnt.data_ptr())
    u = lambda t, dt: t.cpu().numpy().view(dt)
    return ((u(off, np.uint64), u(seq, np.uint32)[:K], u(offset, np.uint64)[:K]), u(only, np.uint64),
            (u(doff, np.uint64), u(doc, np.uint32)[:D], u(cnt, np.uint64)[:D]), u(donly, np.uint64))


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("which", TEXTS)
def test_against_the_reference(O, pkg, wctx, which, table):
    case = text_case(O, pkg, which)
    tb, n = case["tb"], len(case["tb"])
    starts = make_table(n, table)
    pats = patterns(tb, starts, 11)
    with wctx.fm_index(case["bwt"], case["ssa"], case["esa"]) as fm:
        before = fm.info()
        assert before["nseq"] == 0
        fm.set_sequences(starts)
        inf = fm.info()
        nseq = len(starts) - 1
        assert inf["nseq"] == nseq
        assert inf["device_bytes"] - before["device_bytes"] <= (inf["row_bits"] // 8 + 8) * (nseq + 1) + 16
        # seqmap: the ends of the text, "none", every start and the position before it, and random positions
        rng = np.random.default_rng(3)
        st = starts[starts < n]
        u64 = lambda a: np.asarray(a, dtype=np.uint64)
        pos = np.concatenate([u64([0, max(n - 1, 0), n, n + 1, 2**63, 2**64 - 1]), st[:5000], st[-5000:],
                              np.maximum(st[:5000], np.uint64(1)) - np.uint64(1), u64(rng.integers(0, n + 2, 20_000))])
        seq, off = fm.seqmap(pos)
        wseq, woff = R.seqmap(starts, pos)
        assert np.array_equal(seq, wseq) and np.array_equal(off, woff)
        for max_occ in (0, 1, 7):
            loc, docs, kept, dropped = reference(case, starts, pats, max_occ)
            if max_occ == 0 and nseq > 1:        # the case tests something: hits are kept and spanning occurrences are dropped
                assert kept >= 1 and dropped >= 1, (kept, dropped)
            got = fm.locate_seqs(pats, max_occ=max_occ)
            check_locate(got, loc)
            dloc, only, ddocs, donly = dev_calls(fm, pats, max_occ)
            assert same(dloc, got) and np.array_equal(only, got[0])
            if max_occ == 0:
                gdocs = fm.doclist(pats)
                check_docs(gdocs, docs)
                assert same(ddocs, gdocs) and np.array_equal(donly, gdocs[0])
        # the plain locate is what it was
        o1, p1 = fm.locate(pats[:20])
        for k, (s, e) in enumerate(expected(case["text"], case["sa"], pats[:20])):
            assert np.array_equal(p1[o1[k]:o1[k + 1]].astype(np.int64), case["sa"][s:e])


@pytest.mark.parametrize("which,table", [("fasta", "parts64"), ("a_n", "parts64"), ("dna", "big"), ("fasta", "empties")])
def test_batch_and_schedule_independence(O, pkg, wctx, which, table, monkeypatch):
    """one call, batches of 3, a small bound on the hits a workgroup counts, a small budget of located positions per group"""
    case = text_case(O, pkg, which)
    tb, n = case["tb"], len(case["tb"])
    starts = make_table(n, table)
    pats = patterns(tb, starts, 5)[:20 if which == "a_n" else 60] + [b"", tb[:1], tb[:2]]      # (a^n: every chain is n steps long)
    with wctx.fm_index(case["bwt"], case["ssa"], case["esa"]) as fm:
        fm.set_sequences(starts)
        base_l, base_d = fm.locate_seqs(pats, max_occ=0), fm.doclist(pats)
        loc, docs, _, _ = reference(case, starts, pats)
        check_locate(base_l, loc)
        check_docs(base_d, docs)

        def in_batches(call):
            parts = [call(pats[i:i + 3]) for i in range(0, len(pats), 3)]
            off = np.concatenate([np.zeros(1, dtype=np.uint64)] +
                                 [p[0][1:] + np.uint64(sum(int(q[0][-1]) for q in parts[:k])) for k, p in enumerate(parts)])
            return (off, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]))
        assert same(in_batches(fm.locate_seqs), base_l)
        assert same(in_batches(fm.doclist), base_d)
        for env in ({"PFP_FM_MS_STEPS": "50"}, {"PFP_FM_SEQ_BUDGET": "1000"}, {"PFP_FM_MS_STEPS": "3", "PFP_FM_SEQ_BUDGET": "17"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            assert same(fm.locate_seqs(pats, max_occ=0), base_l), env
            assert same(fm.doclist(pats), base_d), env
            for k in env:
                monkeypatch.delenv(k)


@pytest.mark.parametrize("which", ["fasta", "a_n"])
def test_one_sequence_keeps_what_locate_lists(O, pkg, wctx, which):
    case = text_case(O, pkg, which)
    n = len(case["tb"])
    pats = patterns_for(case["text"], 2) + [b"", case["tb"][:1]]
    with wctx.fm_index(case["bwt"], case["ssa"], case["esa"]) as fm:
        fm.set_sequences([0, n])
        for max_occ in (0, 5):
            off, pos = fm.locate(pats, max_occ=max_occ)
            koff, seq, offset = fm.locate_seqs(pats, max_occ=max_occ)
            for k in range(len(pats)):
                want = pos[off[k]:off[k + 1]]
                want = want[want < n]
                assert np.array_equal(offset[koff[k]:koff[k + 1]], want), k
            assert not seq.any()
        doff, doc, cnt = fm.doclist(pats)
        sp, ep = fm.count(pats)
        for k, p in enumerate(pats):
            c = int(ep[k] - sp[k]) - (1 if p == b"" else 0)          # the empty pattern's row 0 is position n
            assert (doc[doff[k]:doff[k + 1]].tolist(), cnt[doff[k]:doff[k + 1]].tolist()) == (([0], [c]) if c else ([], []))


def test_errors(O, pkg, ctx):
    case = text_case(O, pkg, "fasta")
    n = len(case["tb"])
    pats = [b"ACG", b""]
    with ctx.fm_index(case["bwt"], case["ssa"], case["esa"]) as fm:
        for call in (lambda: fm.seqmap([0, 1]), lambda: fm.locate_seqs(pats), lambda: fm.doclist(pats)):
            with pytest.raises(pkg.PfpError) as e:            # no table yet
                call()
            assert e.value.code == EINVAL and "sequence table" in str(e.value)
        for bad, word in (([0, 10, 5, n], "entry 2"), ([1, 10, n], "entry 0"), ([0, 10, n - 1], "entry 2"), ([0, 10, n + 1], "entry 2"),
                          ([0], "1 .."), ([], "1 ..")):
            with pytest.raises(pkg.PfpError) as e:
                fm.set_sequences(bad)
            assert e.value.code == EINVAL and word in str(e.value), (bad, str(e.value))
        assert fm.info()["nseq"] == 0
        fm.set_sequences([0, 100, n])
        with pytest.raises(pkg.PfpError):                      # a refused table leaves the one before in place
            fm.set_sequences([0, n + 5])
        assert fm.info()["nseq"] == 2
        a = fm.seqmap([50, 100, n - 1])
        assert a[0].tolist() == [0, 1, 1] and a[1].tolist() == [50, 0, n - 101]
        fm.set_sequences([0, 50, 60, n])                       # the second table rules
        assert fm.info()["nseq"] == 3
        b = fm.seqmap([50, 100, n - 1])
        assert b[0].tolist() == [1, 2, 2] and b[1].tolist() == [0, 40, n - 61]
        want = reference(case, np.array([0, 50, 60, n], dtype=np.uint64), pats)
        check_locate(fm.locate_seqs(pats), want[0])
        check_docs(fm.doclist(pats), want[1])
    with ctx.fm_index(case["bwt"]) as fm:                      # a table, but no samples
        fm.set_sequences([0, n])
        assert fm.seqmap([3])[0].tolist() == [0]
        for call in (lambda: fm.locate_seqs(pats), lambda: fm.doclist(pats)):
            with pytest.raises(pkg.PfpError) as e:
                call()
            assert e.value.code == EINVAL and ".ssa" in str(e.value)


def test_sequence_file(O, pkg, ctx, tmp_path):
    case = text_case(O, pkg, "fasta")
    n = len(case["tb"])
    f = tmp_path / "t.seqs"
    f.write_bytes(b"first\t0\t1000\nsecond:2\t1000\t0\nthird\t1000\t%d\n" % (n - 1000))
    with ctx.fm_index(case["bwt"], case["ssa"], case["esa"]) as fm:
        assert fm.set_sequences_file(str(f)) == [b"first", b"second:2", b"third"]
        assert fm.info()["nseq"] == 3
        assert fm.seqmap([999, 1000])[0].tolist() == [0, 2]
        f.write_bytes(b"first\t0\t1000\n")
        with pytest.raises(pkg.PfpError) as e:
            fm.set_sequences_file(str(f))
        assert "line 1" in str(e.value)
