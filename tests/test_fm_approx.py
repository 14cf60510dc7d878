"""k-mismatch search over a BWT on the GPU (csrc/fmapprox.hip): FmIndex.approx / approx_locate / approx_dev.

Definitions (include/pfpgpu.h, "Approximate search"): a hit of pattern P is a distinct string S of len(P) bytes that occurs in
the text with d = Hamming(S, P) <= k, reported as (sp, ep, first, d) with [sp, ep) the row range of the suffixes that start with
S and first = SA[sp]; a pattern's hits come by increasing sp.  Every expected value here comes from the brute-force reference
(approx_reference.py), not from the feature.

Texts and patterns: approx_reference.TEXTS / patterns_for.  One cut, made for time (approx_reference.searched): on `ab` the whole
text and the whole text plus one byte are searched with k = 0 only.  With k >= 1 their walks take 2.0 M (k = 1) and 6.0 M
(k = 2, 3) serial steps each; run once on an MI355X with them in, every test here passed, test_hits[ab-1] in 15 s, [ab-2] in
47 s and [ab-3] in 54 s (six walks each), which is no test to run with every change."""
import ctypes as C

import numpy as np
import pytest

import approx_reference as R

pytestmark = pytest.mark.gpu

EINVAL = -1
CASES = [(name, k) for name in R.TEXTS for k in range(R.KMAX[name] + 1)]


def samples(pkg, bwt, sa):
    """.ssa / .esa bytes from the BWT and SA[0..n]: <j, SA[j]> of the run starts / ends"""
    b = np.asarray(bwt)
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    ends = np.flatnonzero(np.concatenate([b[1:] != b[:-1], [True]]))
    pk = lambda rows: pkg.pack5(np.stack([rows, sa[rows]], axis=1).reshape(-1).astype(np.uint64))
    return pk(starts), pk(ends)


def index_of(O, pkg, ctx, name, with_samples=True):
    ref = R.reference(O, name)
    bwt = O.simplebwt(ref.text)
    if not with_samples:
        return ctx.fm_index(bwt)
    ssa, esa = samples(pkg, bwt, ref.sa)
    return ctx.fm_index(bwt, ssa, esa)


def same(got, want, what):
    for g, w, nm in zip(got, want, ("hit_off", "sp", "ep", "dist", "first")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, nm, g[:8], w[:8])


@pytest.mark.parametrize("name,k", CASES)
def test_hits(O, pkg, wctx, name, k):
    ref = R.reference(O, name)
    pats = R.searched(name, R.case(name)[1], k)
    want = ref.arrays(pats, k)
    with index_of(O, pkg, wctx, name) as fm:
        same(fm.approx(pats, k, toehold=True), want, (name, k))
        same(fm.approx(pats, k), want[:4], (name, k, "no toehold"))
    with index_of(O, pkg, wctx, name, with_samples=False) as fm:
        same(fm.approx(pats, k), want[:4], (name, k, "count only"))
        with pytest.raises(pkg.PfpError) as e:
            fm.approx(pats, k, toehold=True)
        assert e.value.code == EINVAL


@pytest.mark.parametrize("name", R.TEXTS)
def test_k0_is_count(O, pkg, ctx, name):
    pats = R.case(name)[1]
    with index_of(O, pkg, ctx, name) as fm:
        sp, ep, first = fm.count(pats, toehold=True)
        off, hsp, hep, dist, hfirst = fm.approx(pats, 0, toehold=True)
        found = ep > sp
        assert np.array_equal(np.diff(off.astype(np.int64)), found.astype(np.int64))
        assert np.array_equal(hsp, sp[found]) and np.array_equal(hep, ep[found]) and np.array_equal(hfirst, first[found])
        assert not dist.any()


def test_bad_arguments(O, pkg, ctx):
    with index_of(O, pkg, ctx, "GATTACA") as fm:
        for k in (4, -1):
            with pytest.raises(pkg.PfpError) as e:
                fm.approx([b"GAT"], k)
            assert e.value.code == EINVAL
            with pytest.raises(pkg.PfpError) as e:
                fm.approx_locate([b"GAT"], k)
            assert e.value.code == EINVAL
        pat = np.frombuffer(b"GATTACAGATTACA", dtype=np.uint8).copy()
        u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        for off in ([0, 7, 3], [5, 2, 9]):
            off = np.array(off, dtype=np.uint64)
            hit_off = np.zeros(3, dtype=np.uint64)
            sp, ep, dist = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)()
            rc = fm.lib.pfp_fm_approx(fm._h, pat.ctypes.data_as(C.POINTER(C.c_uint8)), u64(off), C.c_uint64(2), C.c_int(1), u64(hit_off),
                                      C.byref(sp), C.byref(ep), None, C.byref(dist))
            assert rc == EINVAL and "decrease" in ctx.lib.pfp_last_error(ctx._h).decode() and not sp and not ep and not dist
            pos = C.POINTER(C.c_uint64)()
            rc = fm.lib.pfp_fm_approx_locate(fm._h, pat.ctypes.data_as(C.POINTER(C.c_uint8)), u64(off), C.c_uint64(2), C.c_int(1),
                                             C.c_uint64(0), u64(hit_off), C.byref(pos), C.byref(dist))
            assert rc == EINVAL and not pos and not dist
        off, sp, ep, dist = fm.approx([b"GATTACA"], 1)          # (the index is still usable)
        assert list(off) == [0, 1] and (int(sp[0]), int(ep[0]), int(dist[0])) == (5, 6, 0)


@pytest.mark.parametrize("name", ["copies", "ab"])
@pytest.mark.parametrize("max_occ", [0, 1, 5])
def test_locate(O, pkg, wctx, name, max_occ):
    ref = R.reference(O, name)
    pats = R.case(name)[1]
    with index_of(O, pkg, wctx, name) as fm:
        for k in range(R.KMAX[name] + 1):
            pats = R.searched(name, R.case(name)[1], k)
            got = fm.approx_locate(pats, k, max_occ)
            for g, w, nm in zip(got, ref.located(pats, k, max_occ), ("off", "pos", "dist")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (name, k, max_occ, nm)


@pytest.mark.parametrize("name", ["copies", "ab"])
def test_locate_cap_inside_and_between_hits(O, pkg, ctx, name):
    """max_occ that ends inside a hit's rows, and one that ends exactly between two hits"""
    ref = R.reference(O, name)
    k = 1
    pats = R.searched(name, R.case(name)[1], k)
    rows_of = lambda p: [len(h[4]) for h in ref.hits(p, k)]
    # a pattern with a hit of several rows that is not its last hit
    p = next(p for p in pats + [b"a" * 20] if any(r >= 2 for r in rows_of(p)[:-1]))
    rows = rows_of(p)
    i = next(i for i, r in enumerate(rows[:-1]) if r >= 2)
    inside, between = sum(rows[:i]) + rows[i] - 1, sum(rows[:i + 1])
    assert sum(rows[:i]) < inside < between < sum(rows)
    with index_of(O, pkg, ctx, name) as fm:
        for cap in (inside, between, between + 1):
            got = fm.approx_locate([p, pats[-1], p], k, cap)
            want = ref.located([p, pats[-1], p], k, cap)
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (name, cap)
            assert int(got[0][1]) == cap


@pytest.mark.parametrize("name", ["dna", "bytes", "ab"])
def test_resume(O, pkg, ctx, monkeypatch, name):
    """a budget of 7 iterations per launch: the same answers from many launches"""
    pats = [p for p in R.case(name)[1] if len(p) <= 64]        # (a launch of 7 iterations per pattern: the short patterns)
    with index_of(O, pkg, ctx, name) as fm:
        for k in range(R.KMAX[name] + 1):
            monkeypatch.delenv("PFP_FM_MS_STEPS", raising=False)
            fm.approx_stats()
            want = fm.approx(pats, k, toehold=True)
            wloc = fm.approx_locate(pats[:40], k, 5)
            usual = fm.approx_stats()["launches"]
            monkeypatch.setenv("PFP_FM_MS_STEPS", "7")
            got = fm.approx(pats, k, toehold=True)
            gloc = fm.approx_locate(pats[:40], k, 5)
            many = fm.approx_stats()["launches"]
            same(got, want, (name, k))
            for g, w in zip(gloc, wloc):
                assert np.array_equal(g, w)
            assert many > usual and many > 4, (name, k, many, usual)
    same(want[:5], R.reference(O, name).arrays(pats, R.KMAX[name]), name)


def per_pattern(res, p):
    off = res[0]
    return tuple(a[int(off[p]):int(off[p + 1])].tolist() for a in res[1:])


@pytest.mark.parametrize("name", ["dna", "copies"])
def test_batch_independence(O, pkg, ctx, monkeypatch, name):
    pats = R.case(name)[1]
    k = 2
    order = np.random.default_rng(3).permutation(len(pats))
    with index_of(O, pkg, ctx, name) as fm:
        whole = fm.approx(pats, k, toehold=True)
        shuffled = fm.approx([pats[i] for i in order], k, toehold=True)
        half = len(pats) // 2
        a, b = fm.approx(pats[:half], k, toehold=True), fm.approx(pats[half:], k, toehold=True)
        monkeypatch.setenv("PFP_FM_SEQ_BUDGET", "50")          # the host call cuts its patterns into many groups
        grouped = fm.approx(pats, k, toehold=True)
        gloc = fm.approx_locate(pats, k, 7)
        monkeypatch.delenv("PFP_FM_SEQ_BUDGET")
        wloc = fm.approx_locate(pats, k, 7)
    same(grouped, whole, "groups")
    for g, w in zip(gloc, wloc):
        assert np.array_equal(g, w)
    for j, i in enumerate(order):
        assert per_pattern(shuffled, j) == per_pattern(whole, int(i))
    for p in range(len(pats)):
        assert per_pattern(a if p < half else b, p if p < half else p - half) == per_pattern(whole, p)


@pytest.mark.parametrize("name", ["copies", "ab"])
def test_device_call(O, pkg, ctx, name):
    """offsets only, then fill; the hits as patterns of locate_dev list what approx_locate lists"""
    import torch
    ref = R.reference(O, name)
    k = 2
    pats = R.searched(name, R.case(name)[1], k)
    dev = torch.device("cuda", ctx.device)
    pat, off = pkg.pfp._patterns(pats)
    npat = len(pats)
    d_pat = torch.from_numpy(pat.copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_hoff = torch.zeros(npat + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with index_of(O, pkg, ctx, name) as fm:
        fm.approx_dev(d_pat.data_ptr(), d_off.data_ptr(), npat, k, d_hoff.data_ptr())
        want = ref.arrays(pats, k)
        assert np.array_equal(d_hoff.cpu().numpy().view(np.uint64), want[0])
        H = int(d_hoff[-1])
        d_sp, d_ep, d_first = (torch.zeros(H + 1, dtype=torch.int64, device=dev) for _ in range(3))
        d_dist = torch.zeros(H + 1, dtype=torch.uint8, device=dev)
        d_hoff.zero_()
        torch.cuda.synchronize()
        with pytest.raises(pkg.PfpError) as e:                 # sp, ep and dist come together
            fm.approx_dev(d_pat.data_ptr(), d_off.data_ptr(), npat, k, d_hoff.data_ptr(), d_sp.data_ptr(), d_ep.data_ptr())
        assert e.value.code == EINVAL
        fm.approx_dev(d_pat.data_ptr(), d_off.data_ptr(), npat, k, d_hoff.data_ptr(), d_sp.data_ptr(), d_ep.data_ptr(), d_dist.data_ptr(),
                      d_first.data_ptr())
        got = (d_hoff.cpu().numpy().view(np.uint64), d_sp[:H].cpu().numpy().view(np.uint64), d_ep[:H].cpu().numpy().view(np.uint64),
               d_dist[:H].cpu().numpy(), d_first[:H].cpu().numpy().view(np.uint64))
        same(got, want, name)
        d_loff = torch.zeros(H + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        fm.locate_dev(H, d_sp.data_ptr(), d_ep.data_ptr(), d_first.data_ptr(), 0, d_loff.data_ptr())
        total = int(d_loff[-1])
        d_pos = torch.zeros(total + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        fm.locate_dev(H, d_sp.data_ptr(), d_ep.data_ptr(), d_first.data_ptr(), 0, d_loff.data_ptr(), d_pos.data_ptr())
        aoff, apos, adist = fm.approx_locate(pats, k, 0)
        assert np.array_equal(d_pos[:total].cpu().numpy().view(np.uint64), apos)
        loff = d_loff.cpu().numpy().view(np.uint64)
        assert np.array_equal(loff[want[0].astype(np.int64)], aoff)
        assert np.array_equal(np.repeat(got[3], np.diff(loff.astype(np.int64))), adist)
