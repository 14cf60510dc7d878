"""The LCP array, thresholds and matching statistics with thresholds on the GPU (csrc/lcp.hip), through the C ABI via pfp.py.

Definitions: include/pfpgpu.h, "The LCP array and thresholds".  Expected arrays come from lcp_reference.py (Kasai over the
oracle's suffix array, thresholds by the definition, the two passes modelled over plain arrays); lengths are also compared with
the index's own PHONI answers; at full size, where no CPU LCP exists, the arrays are checked by their properties against longest
common extensions computed with numpy on the host."""
import os

import numpy as np
import pytest

import lcp_reference as L
from test_fm_ms import case, ms_patterns, closed_forms, check_positions, TEXTS
from test_fm_search import _fullsize

pytestmark = pytest.mark.gpu

EFORMAT, EINVAL = -6, -1
NONE = 2**64 - 1
RESUME = ("a_n", "periodic", "fibonacci")       # texts whose irreducible values outlast a lowered launch budget

_models = {}


def model(O, pkg, which):
    """(the CPU model of a named text, its LCP array): computed once"""
    if which not in _models:
        tb, sa, bwt, ssa, esa = case(O, pkg, which)
        lcp = L.kasai_lcp(tb, sa)
        _models[which] = (L.Model(tb, sa, L.thresholds(np.asarray(bwt), lcp)), lcp)
    return _models[which]


def launches(trace, name):
    return sum(r["launches"] for r in trace if r["name"] == name)


def write_base(tmp_path, bwt, ssa, esa):
    base = str(tmp_path / "t")
    for ext, a in ((".bwt", bwt), (".ssa", ssa), (".esa", esa)):
        with open(base + ext, "wb") as fh:
            fh.write(np.asarray(a, dtype=np.uint8).tobytes())
    return base


@pytest.mark.parametrize("which", TEXTS)
def test_small_texts(O, pkg, wctx, which, tmp_path, monkeypatch):
    tb, sa, bwt, ssa, esa = case(O, pkg, which)
    mdl, lcp = model(O, pkg, which)
    text = np.frombuffer(tb, dtype=np.uint8)
    monkeypatch.delenv("PFP_FM_MS_STEPS", raising=False)
    for tx in (text, None):                                    # the text given, and inverted from the BWT
        got = wctx.lcp(bwt, ssa, esa, tx)
        assert np.array_equal(got["lcp"].astype(np.int64), lcp), which
        assert np.array_equal(got["thr"].astype(np.int64), mdl.thr), which
    only = wctx.lcp(bwt, ssa, esa, text, want=("thr",))
    assert set(only) == {"thr"} and np.array_equal(only["thr"], got["thr"])
    if which in RESUME:                                        # a small budget: the blocks resume over several launches
        monkeypatch.setenv("PFP_FM_MS_STEPS", "1")
        wctx.set_kernel_trace(True)
        again = wctx.lcp(bwt, ssa, esa, text)
        trace = wctx.kernel_trace()
        wctx.set_kernel_trace(False)
        monkeypatch.delenv("PFP_FM_MS_STEPS")
        assert launches(trace, "lcp_irr_group") == 1 and launches(trace, "lcp_irr_block") > 1, trace
        assert np.array_equal(again["lcp"], got["lcp"]) and np.array_equal(again["thr"], got["thr"])
    # the files form, and thresholds from the file against computed ones
    base = write_base(tmp_path, bwt, ssa, esa)
    wctx.lcp_files(base, text)
    with open(base + ".lcp", "rb") as fh:
        assert np.array_equal(pkg.unpack5(fh.read()).astype(np.int64), lcp)
    with open(base + ".thr_pos", "rb") as fh:
        thr5 = fh.read()
    assert np.array_equal(pkg.unpack5(thr5).astype(np.int64), mdl.thr)
    os.remove(base + ".lcp")
    wctx.lcp_files(base, None, want=("thr",))
    assert not os.path.exists(base + ".lcp") and open(base + ".thr_pos", "rb").read() == thr5
    pats = ms_patterns(tb, 11)
    with wctx.fm_index_ms(bwt, ssa, esa, text) as a, wctx.fm_index_ms(bwt, ssa, esa) as b, wctx.fm_index_ms(bwt, ssa, esa, text) as d:
        assert a.info()["has_thresholds"] == 0
        before = a.info()["device_bytes"]
        if which in RESUME:
            monkeypatch.setenv("PFP_FM_MS_STEPS", "1")
            a.ms_stats()
        a.add_thresholds()
        if which in RESUME:
            assert a.ms_stats()["launches"] > 2              # the launch counter sees the resumed blocks too
            monkeypatch.delenv("PFP_FM_MS_STEPS")
        inf = a.info()
        assert inf["has_thresholds"] == 1 and inf["device_bytes"] - before >= inf["runs"] * inf["row_bits"] // 8
        assert inf["device_bytes"] - before <= inf["runs"] * inf["row_bits"] // 8 + 512
        b.add_thresholds(thr5)                                 # the file's bytes
        d.add_thresholds(base)                                 # the file itself
        want = a.matching_statistics(pats, thresholds=True)
        for fm in (b, d):
            for x, y in zip(fm.matching_statistics(pats, thresholds=True), want):
                assert np.array_equal(x, y)


@pytest.mark.parametrize("which", TEXTS)
def test_matching_statistics(O, pkg, wctx, which):
    """len is PHONI's, pos is the CPU model's and valid, MEMs agree in (i, len)"""
    tb, sa, bwt, ssa, esa = case(O, pkg, which)
    mdl, _ = model(O, pkg, which)
    pats = ms_patterns(tb, 11)
    with wctx.fm_index_ms(bwt, ssa, esa, np.frombuffer(tb, dtype=np.uint8)) as fm:
        fm.add_thresholds()
        off, ln, pos = fm.matching_statistics(pats, thresholds=True)
        off0, ln0, _ = fm.matching_statistics(pats)
        assert np.array_equal(off, off0) and np.array_equal(ln, ln0)
        for k, p in enumerate(pats):
            a, b = int(off[k]), int(off[k + 1])
            check_positions(tb, p, ln[a:b], pos[a:b])
            wl, wp, matched, _ = mdl.ms(p)
            assert list(ln[a:b]) == wl and [int(x) for x in pos[a:b]] == wp, (which, k, p[:40])
            assert matched <= len(p)
        for L_ in (1, 2, 8, 31):
            m0, mems0 = fm.mems(pats, L_)
            m1, mems1 = fm.mems(pats, L_, thresholds=True)
            assert np.array_equal(m0, m1) and np.array_equal(mems0[:, :2], mems1[:, :2])
            for k in range(len(pats)):
                for i, l, ps in mems1[int(m1[k]):int(m1[k + 1])]:
                    assert int(ps) == int(pos[int(off[k]) + int(i)])
        rng = np.random.default_rng(3)
        for p, want in closed_forms(which, tb):
            _, ln, pos = fm.matching_statistics([p], thresholds=True)
            assert np.array_equal(ln.astype(np.int64), want), (which, len(p))
            assert np.array_equal(ln, fm.matching_statistics([p])[1])
            check_positions(tb, p, ln, pos, sample=rng.integers(0, len(p), 200))
            wl, wp, _, _ = mdl.ms(p)
            assert np.array_equal(pos, np.array(wp, dtype=np.uint64)), (which, len(p))


@pytest.mark.parametrize("which", ["fasta", "a_n", "periodic", "collection"])
def test_invariance(O, pkg, wctx, which, monkeypatch):
    """the outputs (pos included) do not depend on the launch budget, the batch, the order of the patterns or the call"""
    import torch
    tb, sa, bwt, ssa, esa = case(O, pkg, which)
    pats = ms_patterns(tb, 5, lengths=(1, 2, 7, 16, 33, 64, 1000)) + [tb[:5000]]
    with wctx.fm_index_ms(bwt, ssa, esa, np.frombuffer(tb, dtype=np.uint8)) as fm:
        fm.add_thresholds()
        monkeypatch.delenv("PFP_FM_MS_STEPS", raising=False)
        base = fm.matching_statistics(pats, thresholds=True)
        off = base[0]
        for k, p in enumerate(pats):                       # one at a time
            _, ln, pos = fm.matching_statistics([p], thresholds=True)
            assert np.array_equal(ln, base[1][off[k]:off[k + 1]]) and np.array_equal(pos, base[2][off[k]:off[k + 1]]), k
        order = np.random.default_rng(1).permutation(len(pats))
        o2, l2, p2 = fm.matching_statistics([pats[i] for i in order], thresholds=True)
        for j, i in enumerate(order):
            assert np.array_equal(l2[o2[j]:o2[j + 1]], base[1][off[i]:off[i + 1]]) and np.array_equal(p2[o2[j]:o2[j + 1]], base[2][off[i]:off[i + 1]])
        half = len(pats) // 2                              # the batch split in two
        for part, k0 in ((pats[:half], 0), (pats[half:], half)):
            o3, l3, p3 = fm.matching_statistics(part, thresholds=True)
            a, b = int(off[k0]), int(off[k0 + len(part)])
            assert np.array_equal(l3, base[1][a:b]) and np.array_equal(p3, base[2][a:b])
        for budget in ("1", "7", "64"):
            monkeypatch.setenv("PFP_FM_MS_STEPS", budget)
            wctx.set_kernel_trace(True)
            got = fm.matching_statistics(pats, thresholds=True)
            trace = wctx.kernel_trace()
            wctx.set_kernel_trace(False)
            for x, y in zip(base, got):
                assert np.array_equal(x, y), budget
            if budget == "7":                              # the witnesses that both resume paths ran
                assert launches(trace, "fm_ms_thr1") > 1 and launches(trace, "fm_ms_thr2") > 1, trace
        monkeypatch.delenv("PFP_FM_MS_STEPS")
        mem_a = fm.mems(pats, 3, thresholds=True)
        monkeypatch.setenv("PFP_FM_MS_STEPS", "7")
        mem_b = fm.mems(pats, 3, thresholds=True)
        assert np.array_equal(mem_a[0], mem_b[0]) and np.array_equal(mem_a[1], mem_b[1])
        monkeypatch.delenv("PFP_FM_MS_STEPS")
        # device pointers, patterns without padding behind them, pos left out
        dev = torch.device("cuda", 0)
        pat = torch.from_numpy(np.frombuffer(b"".join(pats), dtype=np.uint8).copy()).to(dev)
        d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
        d_len = torch.zeros(int(off[-1]) + 1, dtype=torch.int32, device=dev)
        d_pos = torch.zeros(int(off[-1]) + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        fm.matching_statistics_dev(pat.data_ptr(), d_off.data_ptr(), len(pats), d_len.data_ptr(), d_pos.data_ptr(), thresholds=True)
        assert np.array_equal(d_len.cpu().numpy()[:-1].view(np.uint32), base[1]) and np.array_equal(d_pos.cpu().numpy()[:-1].view(np.uint64), base[2])
        d_len.zero_()
        torch.cuda.synchronize()
        fm.matching_statistics_dev(pat.data_ptr(), d_off.data_ptr(), len(pats), d_len.data_ptr(), None, thresholds=True)
        assert np.array_equal(d_len.cpu().numpy()[:-1].view(np.uint32), base[1])
        d_mem_off = torch.zeros(len(pats) + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        fm.mems_dev(d_off.data_ptr(), len(pats), d_len.data_ptr(), d_pos.data_ptr(), 3, d_mem_off.data_ptr())
        assert np.array_equal(d_mem_off.cpu().numpy().view(np.uint64), mem_a[0])


def test_work_bound(O, pkg, wctx, monkeypatch):
    """pass 2 matches at most as many bytes as the call's patterns hold: a condition (the right end i + len[i] of the match
    never moves left, and every byte matched moves it right), asserted on the inputs that make PHONI quadratic"""
    monkeypatch.setenv("PFP_FM_MS_STATS", "1")
    rng = np.random.default_rng(8)
    sets = {}
    tb = case(O, pkg, "a_n")[0]
    sets["a_n"] = [[b"a" * 150_000], [b"a" * 50_000 + b"b" + b"a" * 50_000], [b"a" * 150_000, b"a" * 50_000 + b"b" + b"a" * 50_000, b"ab" * 500]]
    tc = case(O, pkg, "collection")[0]
    sub = lambda m: tc[(i := int(rng.integers(0, len(tc) - m))):i + m]
    chim = [sub(2000) + sub(2000) for _ in range(40)] + [b"".join(sub(50) for _ in range(80)) for _ in range(40)]
    sets["collection"] = [chim, chim[:1], [tc]]
    for which, calls in sets.items():
        tb, sa, bwt, ssa, esa = case(O, pkg, which)
        with wctx.fm_index_ms(bwt, ssa, esa, np.frombuffer(tb, dtype=np.uint8)) as fm:
            fm.add_thresholds()
            for pats in calls:
                total = sum(len(p) for p in pats)
                fm.ms_stats()
                off, ln, pos = fm.matching_statistics(pats, thresholds=True)
                st = fm.ms_stats()
                assert st["launches"] >= 2 and st["matched"] <= total, (which, st, total)
                assert st["matched"] >= int(ln[off[:-1][np.diff(off) > 0]].max())       # (the counter is alive)
                if which == "collection":                      # (a_n against PHONI: test_matching_statistics)
                    assert np.array_equal(ln, fm.matching_statistics(pats)[1])
                    assert st["jumps"] > 0 or len(pats) == 1


def test_errors(O, pkg, ctx, tmp_path):
    tb, sa, bwt, ssa, esa = case(O, pkg, "fasta")
    text = np.frombuffer(tb, dtype=np.uint8)
    n = len(tb)
    pats = ms_patterns(tb, 6)
    for make in (lambda: ctx.fm_index(bwt, ssa, esa), lambda: ctx.fm_index(bwt)):      # a plain and a count-only index
        with make() as plain:
            for call in (lambda: plain.add_thresholds(), lambda: plain.add_thresholds(b"\0" * 5), lambda: plain.add_thresholds(str(tmp_path / "x")),
                         lambda: plain.matching_statistics([b"ACG"], thresholds=True), lambda: plain.mems([b"ACG"], thresholds=True)):
                with pytest.raises(pkg.PfpError) as e:
                    call()
                assert e.value.code == EINVAL and "pfp_fm_build_ms_" in str(e.value)
    with pytest.raises(pkg.PfpError) as e:
        ctx.lcp(bwt, None, None)
    assert e.value.code == EINVAL
    with pytest.raises(pkg.PfpError) as e:
        ctx.lcp(bwt, ssa, esa, text[:-1])
    assert e.value.code == EINVAL
    with pytest.raises(pkg.PfpError) as e:
        ctx.lcp(bwt, ssa[:-10], esa)
    assert e.value.code == EFORMAT
    base = write_base(tmp_path, bwt, ssa, esa)
    with pytest.raises(pkg.PfpError) as e:
        ctx.lcp_files(base, text[:-1])
    assert e.value.code == EINVAL and str(n) in str(e.value)
    with pytest.raises(pkg.PfpError) as e:
        ctx.lcp_files(str(tmp_path / "nothing"), text)
    assert e.value.code == EINVAL and "nothing.bwt" in str(e.value)
    with ctx.fm_index_ms(bwt, ssa, esa, text) as fm:
        r = fm.info()["runs"]
        for call in (lambda: fm.matching_statistics(pats, thresholds=True), lambda: fm.mems(pats, 2, thresholds=True)):
            with pytest.raises(pkg.PfpError) as e:                 # no thresholds yet
                call()
            assert e.value.code == EINVAL and "pfp_fm_thresholds_" in str(e.value)
        with pytest.raises(pkg.PfpError) as e:
            fm.add_thresholds(base)                                # no such file
        assert e.value.code == EINVAL and "t.thr_pos" in str(e.value)
        for bad in (5 * r - 5, 5 * r + 5, 5 * r - 1, 0):           # short, long, not whole, empty
            with pytest.raises(pkg.PfpError) as e:
                fm.add_thresholds(b"\1" * bad)
            assert e.value.code == EFORMAT and str(5 * r) in str(e.value)
            with open(base + ".thr_pos", "wb") as fh:
                fh.write(b"\1" * bad)
            with pytest.raises(pkg.PfpError) as e:
                fm.add_thresholds(base)
            assert e.value.code == EFORMAT
        assert fm.info()["has_thresholds"] == 0
        want = fm.matching_statistics(pats)
        # wrong thresholds: all zeros, all n, beyond every row: some answer, lengths within the pattern, positions within the text
        for thr in (np.zeros(r, dtype=np.uint64), np.full(r, n, dtype=np.uint64), np.full(r, 2**40 - 1, dtype=np.uint64)):
            fm.add_thresholds(pkg.pack5(thr))
            off, ln, pos = fm.matching_statistics(pats, thresholds=True)
            for k, p in enumerate(pats):
                a, b = int(off[k]), int(off[k + 1])
                assert np.all(ln[a:b].astype(np.int64) <= np.arange(len(p), 0, -1))
            assert np.all((pos < n) | (pos == NONE)) and np.all(pos[ln == 0] == NONE)
            fm.mems(pats, 2, thresholds=True)
        fm.add_thresholds()                                        # (the index is still usable)
        for x, y in zip(fm.matching_statistics(pats, thresholds=True)[:2], want[:2]):
            assert np.array_equal(x, y)
    # a text of the right length but other content: answers for no text, never an access outside the index
    with ctx.fm_index_ms(bwt, ssa, esa, text[::-1].copy()) as fm:
        fm.add_thresholds()
        off, ln, pos = fm.matching_statistics(pats, thresholds=True)
        for k, p in enumerate(pats):
            a, b = int(off[k]), int(off[k + 1])
            assert np.all(ln[a:b].astype(np.int64) <= np.arange(len(p), 0, -1))
        assert np.all((pos <= n) | (pos == NONE))
        fm.mems(pats, 2, thresholds=True)
    got = ctx.lcp(bwt, ssa, esa, text[::-1].copy())
    assert len(got["lcp"]) == n + 1 and np.all(got["lcp"] <= n) and np.all(got["thr"] <= n)


@pytest.mark.parametrize("bits", [0, 64])
def test_memory(O, pkg, ctx, bits):
    """the documented bound (pfpgpu.h), from the allocation list of csrc/lcp.hip: computing thresholds peaks at the index with
    text + (3 w + 0.1875) bytes per row (PLCP, LCP, the walk's LF and its tile histograms) + (16 + 7.75 w) bytes per run (the run
    minima and their rows, the table, the sort's four arrays and the library's copy of two) + the library's scratch (4 MiB
    here); the index keeps w bytes per run; everything else goes back"""
    import torch
    text = O.gen_fasta(250_000, 4, 0.002, 7)
    got = ctx.bigbwt(text, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    with pkg.Context(0) as c:
        c.set_index_bits(bits)
        keep = [torch.from_numpy(np.asarray(x).copy()).cuda() for x in (got["bwt"], got["ssa"], got["esa"], text)]
        torch.cuda.synchronize()
        assert c.mem_stats()["live"] == 0
        fm = c.fm_index_ms_dev(keep[0].data_ptr(), keep[0].numel(), keep[1].data_ptr(), keep[1].numel(), keep[2].data_ptr(), keep[2].numel(),
                               keep[3].data_ptr())
        inf = fm.info()
        n1, r, wb = inf["n"] + 1, inf["runs"], inf["row_bits"] // 8
        assert wb == (8 if bits == 64 else 4)
        fm.add_thresholds()
        st = c.mem_stats()
        bound = inf["device_bytes"] + n1 * (3 * wb + 0.1875) + r * (16 + 7.75 * wb) + (4 << 20)
        assert st["peak"] <= bound, (st, inf, bound)
        assert st["peak"] >= inf["device_bytes"] + 3 * wb * n1          # (the three arrays per row are what it is made of)
        after = fm.info()
        assert r * wb <= after["device_bytes"] - inf["device_bytes"] <= r * wb + 512
        tb = bytes(text)
        fm.matching_statistics([tb[10:500], tb[1000:1100] + b"#" + tb[5:50]], thresholds=True)
        fm.close()
        assert c.mem_stats()["live"] == 0
        d_lcp = torch.zeros(n1 + 1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        assert c.lcp_dev(keep[0].data_ptr(), keep[0].numel(), keep[1].data_ptr(), keep[1].numel(), keep[2].data_ptr(), keep[2].numel(),
                         keep[3].data_ptr(), d_lcp=d_lcp.data_ptr()) == r
        assert c.mem_stats()["live"] == 0                               # pfp_lcp_dev keeps nothing


def host_lce(t, x, y, n):
    """the common prefix of t[x:] and t[y:] (numpy, doubling chunks)"""
    l, step = 0, 64
    while True:
        k = min(step, n - max(x, y) - l)
        if k <= 0:
            return l
        d = np.flatnonzero(t[x + l:x + l + k] != t[y + l:y + l + k])
        if len(d):
            return l + int(d[0])
        l += k
        step *= 4


@pytest.mark.parametrize("name,need_gb,npat", [("c3", 40, 100_000)])
def test_fullsize(pkg, ctx, synth, name, need_gb, npat):
    """configs[2] (0.79 GB, 15.6 M runs).  No CPU LCP at this size: run starts against the LCE of their two samples, rows inside
    located ranges against the LCE of consecutive SA values, thresholds by the range-minimum property, and matching statistics
    with thresholds against PHONI.  (The 12.6 GB collection does not fit: DESIGN.md 6g has the arithmetic.)"""
    import torch
    m = 100
    text, bwt, outs = _fullsize(pkg, ctx, synth, name, need_gb)
    dev = text.device
    n = text.numel()
    try:
        (ssa, ssa_b), (esa, esa_b) = outs["ssa"], outs["esa"]
        r = ssa_b // 10
        sp_ = pkg.unpack5(ctx.fetch_dev(ssa, ssa_b)).reshape(-1, 2).astype(np.int64)
        ep_ = pkg.unpack5(ctx.fetch_dev(esa, esa_b)).reshape(-1, 2).astype(np.int64)
        with pkg.Context(0) as c:
            d_lcp = torch.zeros(n + 2, dtype=torch.int64, device=dev)
            d_thr = torch.zeros(r + 1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            c.mem_stats()
            assert c.lcp_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr(), d_lcp.data_ptr(), d_thr.data_ptr()) == r
            assert c.mem_stats()["live"] == 0
            fm = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
            for p, _ in outs.values():
                ctx.dev_free(p)
            outs = {}
            t = text.cpu().numpy()
            rng = np.random.default_rng(4)
            assert int(d_lcp[0]) == 0 and int(d_lcp[1]) == 0
            # run starts: lcp[s_k] = LCE(SA[s_k], SA[e_{k-1}])
            ks = rng.integers(1, r, 2000)
            at = d_lcp[torch.from_numpy(sp_[ks, 0]).to(dev)].cpu().numpy()
            for k, v in zip(ks, at):
                assert int(v) == host_lce(t, int(sp_[k, 1]), int(ep_[k - 1, 1]), n), k
            # rows inside located ranges: lcp[j] = LCE(SA[j-1], SA[j])
            tb = t[:1 << 22].tobytes()
            pats = [tb[i:i + 16] for i in rng.integers(0, len(tb) - 16, 50)]
            off, pos, sp, ep = fm.locate(pats, max_occ=200, ranges=True)
            for k in range(len(pats)):
                a, b = int(off[k]), int(off[k + 1])
                rows = d_lcp[int(sp[k]):int(sp[k]) + (b - a)].cpu().numpy()
                for j in range(1, b - a):
                    assert int(rows[j]) == host_lce(t, int(pos[a + j - 1]), int(pos[a + j]), n), (k, j)
                    assert int(rows[j]) >= 16
            # thresholds: the smallest row of the minimum over (e_prev, s_k], whose value is the LCE of the range's two ends
            byte = bwt[torch.from_numpy(sp_[:, 0]).to(dev)].cpu().numpy()
            prev = np.full(r, -1, dtype=np.int64)
            for cb in np.unique(byte):
                idx = np.flatnonzero(byte == cb)
                prev[idx[1:]] = idx[:-1]
            thr = d_thr[:r].cpu().numpy()
            assert np.all(thr[prev < 0] == 0)
            have = np.flatnonzero(prev >= 0)
            lo, hi = ep_[prev[have], 0] + 1, sp_[have, 0]
            assert np.all((thr[have] >= lo) & (thr[have] <= hi))
            short = have[(hi - lo) < (1 << 20)]
            for k in rng.choice(short, 300, replace=False):
                a, b, x = int(ep_[prev[k], 0]) + 1, int(sp_[k, 0]), int(thr[k])
                seg = d_lcp[a:b + 1].cpu().numpy()
                assert int(seg[x - a]) == host_lce(t, int(ep_[prev[k], 1]), int(sp_[k, 1]), n), k
                assert np.all(seg[:x - a] > seg[x - a]) and np.all(seg[x - a:] >= seg[x - a]), k
            del d_lcp
            # matching statistics with thresholds (loaded from the computed rows) against PHONI on sampled and mutated patterns
            thr5 = torch.zeros(5 * r + 16, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            c.pack5_dev(d_thr.data_ptr(), r, thr5.data_ptr())
            fm.add_thresholds_dev(thr5.data_ptr(), 5 * r)
            assert fm.info()["has_thresholds"] == 1
            g = torch.Generator(device="cpu").manual_seed(5)
            start = torch.randint(0, n - m, (npat,), generator=g).to(dev)
            ar = torch.arange(m, device=dev)
            P = text[start[:, None] + ar[None, :]]
            mut = torch.rand(npat, generator=g).to(dev) < 0.1
            col = torch.randint(0, m, (npat,), generator=g).to(dev)
            rows = torch.arange(npat, device=dev)
            P[rows[mut], col[mut]] = torch.where(P[rows[mut], col[mut]] == ord("A"), ord("C"), ord("A")).to(torch.uint8)
            pat = P.reshape(-1).contiguous()
            off = torch.arange(0, npat * m + 1, m, dtype=torch.int64, device=dev)
            ln, ln0 = (torch.zeros(npat * m, dtype=torch.int32, device=dev) for _ in range(2))
            pos = torch.zeros(npat * m, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            fm.matching_statistics_dev(pat.data_ptr(), off.data_ptr(), npat, ln.data_ptr(), pos.data_ptr(), thresholds=True)
            fm.matching_statistics_dev(pat.data_ptr(), off.data_ptr(), npat, ln0.data_ptr(), None)
            assert torch.equal(ln, ln0)
            Lm, Q = ln.view(npat, m).to(torch.int64), pos.view(npat, m)
            assert bool((Lm >= 1).all()) and bool((Q >= 0).all()) and bool((Q + Lm <= n).all())
            wide = torch.zeros(npat, 2 * m, dtype=torch.uint8, device=dev)
            wide[:, :m] = P
            for k in range(m):                               # text[pos + k] == P[i + k] for k < len, at every i
                live = Lm > k
                idx = (Q + k).clamp(max=n - 1)
                assert bool(((text[idx] == wide[:, k:k + m]) | ~live).all()), k
            fm.close()
            assert c.mem_stats()["live"] == 0
    finally:
        for p, _ in outs.values():
            ctx.dev_free(p)
        del text, bwt
        ctx.pool_trim()
        torch.cuda.empty_cache()
