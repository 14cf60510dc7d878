"""Matching statistics and maximal exact matches on the GPU (csrc/fmsearch.hip: PHONI), through the C ABI via pfp.py.

Definitions (include/pfpgpu.h, "Matching statistics"): len[i] = the longest prefix of P[i:] that occurs in the text, pos[i] one
place where it occurs (2^64 - 1 where len[i] = 0); a MEM is (i, len[i], pos[i]) with len[i] >= min_len and (i = 0 or
len[i-1] <= len[i]).  Expected lengths come from ms_reference.py (binary search over the oracle's suffix array) or, for the long
patterns, from closed forms; positions are checked against the text."""
import numpy as np
import pytest

import ms_reference as R
from test_fm_search import full_sa, samples, small_texts, _fullsize
from textgen import make_text

pytestmark = pytest.mark.gpu

EFORMAT, EINVAL = -6, -1
NONE = 2**64 - 1
LITERALS = {b"TTACAG": [5, 4, 3, 2, 1, 1], b"CATTAG": [2, 4, 3, 2, 1, 1], b"GATTACAGATTA": [7, 6, 5, 4, 3, 2, 1, 5, 4, 3, 2, 1]}
TEXTS = ["fasta", "dna", "all_bytes", "GATTACA", "a_n", "periodic", "fibonacci", "collection"]


def ms_texts(O):
    yield from small_texts(O)
    rng = np.random.default_rng(17)
    per = np.tile(rng.integers(97, 123, 37, dtype=np.uint8), 5000)
    at = rng.integers(0, len(per), 20)
    per[at] = (per[at] - 97 + 1 + rng.integers(0, 25, 20)) % 26 + 97          # 20 substitutions
    yield "periodic", per
    a, b = b"a", b"ab"
    while len(b) < 100_000:
        a, b = b, b + a
    yield "fibonacci", np.frombuffer(b, dtype=np.uint8)
    base = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 20_000)
    copies = []
    for _ in range(8):
        c = base.copy()
        at = rng.integers(0, len(c), len(c) // 200)                            # 0.5 % substitutions
        c[at] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), len(at))
        copies.append(c)
    yield "collection", np.concatenate(copies)


_cache = {}


def case(O, pkg, which):
    """(text bytes, SA[0..n], bwt, ssa, esa) of a named text, computed once"""
    if which not in _cache:
        text = np.ascontiguousarray(dict(ms_texts(O))[which], dtype=np.uint8)
        sa = full_sa(O, text)
        bwt = O.simplebwt(text)
        ssa, esa = samples(pkg, bwt, sa)
        _cache[which] = (text.tobytes(), sa, bwt, ssa, esa)
    return _cache[which]


def ms_patterns(tb, seed, lengths=tuple(range(1, 65)) + (1000,)):
    rng = np.random.default_rng(seed)
    n = len(tb)
    present = set(tb)
    absent = [c for c in range(1, 256) if c not in present]
    sub = lambda m: tb[(i := int(rng.integers(0, n - m + 1))):i + m]
    pats = [b""] + list(LITERALS)
    for m in lengths:
        if m > n:
            continue
        s = bytearray(sub(m))
        pats.append(bytes(s))
        k = int(rng.integers(0, m))
        s[k] = (s[k] + 1 + int(rng.integers(0, 200))) % 253 + 3              # a mutated copy (never byte 0)
        pats.append(bytes(s))
    for m1, m2 in ((5, 9), (40, 17), (100, 300), (1, 64)):                   # chimeras of two substrings
        if max(m1, m2) <= n:
            pats.append(sub(m1) + sub(m2))
    m = min(n, 30)
    pats.append(sub(m) + b"\0" + sub(m))                                     # byte 0 in the middle
    if absent:
        pats.append(sub(m) + bytes([absent[0]]) + sub(m))                    # a byte the text does not hold
        pats.append(bytes([absent[-1]]))
    pats.append(b"\0")
    return pats


_ref_cache = {}


def reference(which, tb, sa, pats, seed):
    key = (which, seed, len(pats))
    if key not in _ref_cache:
        _ref_cache[key] = [R.ms_lengths(tb, sa, p) for p in pats]
    return _ref_cache[key]


def check_positions(tb, pat, ln, pos, sample=None):
    """where len > 0 the text matches at pos and pos + len <= n; where len = 0 pos is 2^64 - 1"""
    n, m = len(tb), len(pat)
    ln, pos = np.asarray(ln).astype(np.int64), np.asarray(pos)
    assert np.all(pos[ln == 0] == NONE)
    nz = np.flatnonzero(ln > 0)
    assert np.all(pos[nz].astype(np.int64) + ln[nz] <= n) and np.all(pos[nz] <= n)
    for i in (nz if sample is None else sample):
        i = int(i)
        if ln[i]:
            p, l = int(pos[i]), int(ln[i])
            assert tb[p:p + l] == pat[i:i + l], (i, p, l)


def check_ms(fm, which, tb, sa, pats, seed):
    want = reference(which, tb, sa, pats, seed)
    off, ln, pos = fm.matching_statistics(pats)
    assert len(off) == len(pats) + 1 and len(ln) == len(pos) == int(off[-1])
    for k, p in enumerate(pats):
        a, b = int(off[k]), int(off[k + 1])
        assert b - a == len(p)
        assert np.array_equal(ln[a:b].astype(np.int64), want[k]), (which, k, p[:40], ln[a:b][:20], want[k][:20])
        check_positions(tb, p, ln[a:b], pos[a:b])
    return off, ln, pos


def closed_forms(which, tb):
    """long patterns with their lengths in closed form"""
    n = len(tb)
    out = [(tb, np.arange(n, 0, -1, dtype=np.int64))]                         # the whole text: len[i] = n - i
    if which == "a_n":
        for m in (100_000, 150_000):
            out.append((b"a" * m, np.minimum(np.arange(m, 0, -1, dtype=np.int64), n)))
        m = 100_001
        want = np.concatenate([np.arange(50_000, 0, -1), [0], np.arange(50_000, 0, -1)]).astype(np.int64)
        out.append((b"a" * 50_000 + b"b" + b"a" * 50_000, want))
        assert len(want) == m
    return out


@pytest.mark.parametrize("which", TEXTS)
def test_small_texts(O, pkg, wctx, which):
    tb, sa, bwt, ssa, esa = case(O, pkg, which)
    pats = ms_patterns(tb, 11)
    rng = np.random.default_rng(3)
    with wctx.fm_index_ms(bwt, ssa, esa, np.frombuffer(tb, dtype=np.uint8)) as fm, wctx.fm_index_ms(bwt, ssa, esa) as inv:
        inf = fm.info()
        assert inf["n"] == len(tb) and inf["has_samples"] == 1 and inf["device_bytes"] == inv.info()["device_bytes"]
        got = check_ms(fm, which, tb, sa, pats, 11)
        for x, y in zip(got, inv.matching_statistics(pats)):                 # the inverted text: identical, pos included
            assert np.array_equal(x, y)
        if which == "GATTACA":
            off, ln, _ = got
            for k, p in enumerate(pats):
                if p in LITERALS:
                    assert list(ln[off[k]:off[k + 1]]) == LITERALS[p]
        for p, want in closed_forms(which, tb):
            off, ln, pos = fm.matching_statistics([p])
            assert np.array_equal(ln.astype(np.int64), want), (which, len(p))
            check_positions(tb, p, ln, pos, sample=rng.integers(0, len(p), 200))
            if len(p) == 100_001:
                assert pos[50_000] == NONE
            off2, ln2, pos2 = inv.matching_statistics([p])
            assert np.array_equal(ln, ln2) and np.array_equal(pos, pos2)


GOLDEN_NOT_A_BWT = {"kat_q1", "tiny_bytes_w5"}


@pytest.mark.parametrize("idx", range(15))
def test_golden_texts(golden, O, pkg, wctx, idx):
    c = golden[idx]
    text = make_text(c["spec"], O)
    got = wctx.bigbwt(text, c["w"], c["p"], pkg.FLAG_SSA | pkg.FLAG_ESA)
    bwt = got["bwt"]
    n = len(bwt) - 1
    t = np.ascontiguousarray(text[:n], dtype=np.uint8)
    if np.count_nonzero(bwt == 0) != 1:          # the reference quirk's output is not a BWT
        assert c["name"] in GOLDEN_NOT_A_BWT, c["name"]
        for tx in (t, None):
            with pytest.raises(pkg.PfpError) as e:
                wctx.fm_index_ms(bwt, got["ssa"], got["esa"], tx)
            assert e.value.code == EFORMAT
        return
    assert c["name"] not in GOLDEN_NOT_A_BWT
    sa = full_sa(O, t, O.bigbwt(text, c["w"], c["p"], O.FLAG_SA)["sa"])
    tb = t.tobytes()
    pats = ms_patterns(tb, idx, lengths=(1, 2, 3, 5, 8, 13, 21, 34, 55, 64, 300))
    with wctx.fm_index_ms(bwt, got["ssa"], got["esa"], t) as fm, wctx.fm_index_ms(bwt, got["ssa"], got["esa"]) as inv:
        got1 = check_ms(fm, "golden%d" % idx, tb, sa, pats, idx)
        for x, y in zip(got1, inv.matching_statistics(pats)):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("which", ["fasta", "GATTACA", "a_n", "collection"])
def test_mems(O, pkg, wctx, which):
    import torch
    tb, sa, bwt, ssa, esa = case(O, pkg, which)
    pats = ms_patterns(tb, 11)
    want_len = reference(which, tb, sa, pats, 11)
    dev = torch.device("cuda", 0)
    with wctx.fm_index_ms(bwt, ssa, esa, np.frombuffer(tb, dtype=np.uint8)) as fm:
        off, ln, pos = fm.matching_statistics(pats)
        pat = torch.from_numpy(np.frombuffer(b"".join(pats) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
        d_len = torch.zeros(int(off[-1]) + 1, dtype=torch.int32, device=dev)
        d_pos = torch.zeros(int(off[-1]) + 1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        fm.matching_statistics_dev(pat.data_ptr(), d_off.data_ptr(), len(pats), d_len.data_ptr(), d_pos.data_ptr())
        assert np.array_equal(d_len.cpu().numpy()[:-1].view(np.uint32), ln) and np.array_equal(d_pos.cpu().numpy()[:-1].view(np.uint64), pos)
        for L in (1, 2, 8, 31, 1000):
            mem_off, mems = fm.mems(pats, L)
            assert mems.shape == (int(mem_off[-1]), 3) and mem_off[0] == 0
            for k, p in enumerate(pats):
                want = R.mems_from_lengths(want_len[k], L)
                rows = mems[int(mem_off[k]):int(mem_off[k + 1])]
                assert [(int(i), int(l)) for i, l, _ in rows] == want, (which, L, k)
                for i, l, ps in rows:
                    assert int(ps) == int(pos[int(off[k]) + int(i)])
            if which == "GATTACA" and L == 2:
                by = {p: [(int(i), int(l)) for i, l, _ in mems[int(mem_off[k]):int(mem_off[k + 1])]] for k, p in enumerate(pats)}
                assert by[b"TTACAG"] == [(0, 5)] and by[b"CATTAG"] == [(0, 2), (1, 4)] and by[b"GATTACAGATTA"] == [(0, 7), (7, 5)]
            d_mem_off = torch.zeros(len(pats) + 1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            fm.mems_dev(d_off.data_ptr(), len(pats), d_len.data_ptr(), d_pos.data_ptr(), L, d_mem_off.data_ptr())      # offsets only
            assert np.array_equal(d_mem_off.cpu().numpy().view(np.uint64), mem_off)
            d_mem = torch.zeros(3 * int(mem_off[-1]) + 1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            fm.mems_dev(d_off.data_ptr(), len(pats), d_len.data_ptr(), d_pos.data_ptr(), L, d_mem_off.data_ptr(), d_mem.data_ptr())
            assert np.array_equal(d_mem.cpu().numpy()[:-1].view(np.uint64).reshape(-1, 3), mems)


@pytest.mark.parametrize("which", ["fasta", "a_n", "periodic"])
def test_invariance(O, pkg, wctx, which, monkeypatch):
    """the outputs (pos included) do not depend on the launch budget, the batch or the call"""
    tb, sa, bwt, ssa, esa = case(O, pkg, which)
    pats = ms_patterns(tb, 5, lengths=(1, 2, 7, 16, 33, 64, 1000))
    with wctx.fm_index_ms(bwt, ssa, esa, np.frombuffer(tb, dtype=np.uint8)) as fm:
        monkeypatch.delenv("PFP_FM_MS_STEPS", raising=False)
        base = fm.matching_statistics(pats)
        again = fm.matching_statistics(pats)
        for x, y in zip(base, again):
            assert np.array_equal(x, y)
        off = base[0]
        for k, p in enumerate(pats):                       # one at a time
            _, ln, pos = fm.matching_statistics([p])
            assert np.array_equal(ln, base[1][off[k]:off[k + 1]]) and np.array_equal(pos, base[2][off[k]:off[k + 1]]), k
        for budget in ("1", "7", "64"):
            monkeypatch.setenv("PFP_FM_MS_STEPS", budget)
            wctx.set_kernel_trace(True)
            got = fm.matching_statistics(pats)
            trace = wctx.kernel_trace()
            wctx.set_kernel_trace(False)
            for x, y in zip(base, got):
                assert np.array_equal(x, y), budget
            launches = sum(r["launches"] for r in trace if r["name"] == "fm_ms")
            assert launches >= 1
            if budget == "7":
                assert launches > 1, trace                   # the witness that the resume path ran
        monkeypatch.delenv("PFP_FM_MS_STEPS")
        mem_a = fm.mems(pats, 3)
        monkeypatch.setenv("PFP_FM_MS_STEPS", "7")
        mem_b = fm.mems(pats, 3)
        assert np.array_equal(mem_a[0], mem_b[0]) and np.array_equal(mem_a[1], mem_b[1])


@pytest.mark.parametrize("which", ["dna", "collection", "fibonacci"])
def test_against_count(O, pkg, wctx, which):
    """the index's own count: P[i : i+len] occurs, P[i : i+len+1] does not"""
    tb, sa, bwt, ssa, esa = case(O, pkg, which)
    pats = [p for p in ms_patterns(tb, 23) if p]
    rng = np.random.default_rng(9)
    with wctx.fm_index_ms(bwt, ssa, esa) as fm:
        off, ln, pos = fm.matching_statistics(pats)
        hit, miss = [], []
        for _ in range(400):
            k = int(rng.integers(0, len(pats)))
            p = pats[k]
            i = int(rng.integers(0, len(p)))
            l = int(ln[int(off[k]) + i])
            if l > 0:
                hit.append(p[i:i + l])
            if i + l < len(p):
                miss.append(p[i:i + l + 1])
        sp, ep = fm.count(hit)
        assert np.all(ep > sp)
        sp, ep = fm.count(miss)
        assert np.all(ep == sp)


@pytest.mark.parametrize("name,need_gb,npat", [("c3", 40, 100_000), ("huge_s", 200, 20_000)])
def test_fullsize(pkg, ctx, synth, name, need_gb, npat):
    """configs[2] and the 12.6 GB collection (u64 rows, SA values above 2^32): patterns of 100 bytes sampled on the device, 10 %
    with one byte changed; every answer is checked against the text with torch"""
    import torch
    m = 100
    text, bwt, outs = _fullsize(pkg, ctx, synth, name, need_gb)
    dev = text.device
    n = text.numel()
    try:
        (ssa, ssa_b), (esa, esa_b) = outs["ssa"], outs["esa"]
        with pkg.Context(0) as c:
            torch.cuda.synchronize()
            fm = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, text.data_ptr())
            inv = c.fm_index_ms_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b, None) if name == "c3" else None
            for p, _ in outs.values():
                ctx.dev_free(p)
            outs = {}
            inf = fm.info()
            assert inf["n"] == n and inf["row_bits"] == (64 if n + 1 >= 2**32 else 32)
            g = torch.Generator(device="cpu").manual_seed(5)
            start = torch.randint(0, n - m, (npat,), generator=g).to(dev)
            ar = torch.arange(m, device=dev)
            P = text[start[:, None] + ar[None, :]]
            mut = torch.rand(npat, generator=g).to(dev) < 0.1
            col = torch.randint(0, m, (npat,), generator=g).to(dev)
            rows = torch.arange(npat, device=dev)
            P[rows[mut], col[mut]] = torch.where(P[rows[mut], col[mut]] == ord("A"), ord("C"), ord("A")).to(torch.uint8)
            pat = torch.cat([P.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)]).contiguous()
            off = torch.arange(0, npat * m + 1, m, dtype=torch.int64, device=dev)
            ln = torch.zeros(npat * m, dtype=torch.int32, device=dev)
            pos = torch.zeros(npat * m, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            fm.matching_statistics_dev(pat.data_ptr(), off.data_ptr(), npat, ln.data_ptr(), pos.data_ptr())
            L, Q = ln.view(npat, m).to(torch.int64), pos.view(npat, m)
            assert bool((L >= 1).all()) and bool((L <= (m - ar)[None, :]).all())
            assert bool((Q >= 0).all()) and bool((Q + L <= n).all())
            assert bool((L[~mut, 0] == m).all())
            assert bool((L[:, :-1] <= L[:, 1:] + 1).all())
            wide = torch.zeros(npat, 2 * m, dtype=torch.uint8, device=dev)
            wide[:, :m] = P
            for k in range(m):                               # text[pos + k] == P[i + k] for k < len, at every i
                live = L > k
                idx = (Q + k).clamp(max=n - 1)
                pk = wide[:, k:k + m]
                assert bool(((text[idx] == pk) | ~live).all()), k
            # the index's own count on a sample: P[i : i+len] occurs, P[i : i+len+1] does not
            Lc, Pc = L.cpu().numpy(), P.cpu().numpy()
            rng = np.random.default_rng(2)
            hit, miss = [], []
            for _ in range(300):
                k, i = int(rng.integers(0, npat)), int(rng.integers(0, m))
                l = int(Lc[k, i])
                hit.append(Pc[k, i:i + l].tobytes())
                if i + l < m:
                    miss.append(Pc[k, i:i + l + 1].tobytes())
            sp, ep = fm.count(hit)
            assert np.all(ep > sp)
            if miss:
                sp, ep = fm.count(miss)
                assert np.all(ep == sp)
            if inv is not None:                              # built by inversion: all outputs identical
                ln2, pos2 = torch.zeros_like(ln), torch.zeros_like(pos)
                torch.cuda.synchronize()
                inv.matching_statistics_dev(pat.data_ptr(), off.data_ptr(), npat, ln2.data_ptr(), pos2.data_ptr())
                assert torch.equal(ln, ln2) and torch.equal(pos, pos2)
                inv.close()
            fm.close()
            assert c.mem_stats()["live"] == 0
    finally:
        for p, _ in outs.values():
            ctx.dev_free(p)
        del text, bwt
        ctx.pool_trim()
        torch.cuda.empty_cache()


def test_same_answers_as_a_plain_index(O, pkg, wctx):
    tb, sa, bwt, ssa, esa = case(O, pkg, "fasta")
    pats = ms_patterns(tb, 3)
    with wctx.fm_index_ms(bwt, ssa, esa) as a, wctx.fm_index(bwt, ssa, esa) as b:
        for x, y in zip(a.count(pats, toehold=True), b.count(pats, toehold=True)):
            assert np.array_equal(x, y)
        for x, y in zip(a.locate(pats, max_occ=7), b.locate(pats, max_occ=7)):
            assert np.array_equal(x, y)
        ia, ib = a.info(), b.info()
        assert {k: v for k, v in ia.items() if k != "device_bytes"} == {k: v for k, v in ib.items() if k != "device_bytes"}


def test_errors(O, pkg, ctx, tmp_path):
    import ctypes as C
    tb, sa, bwt, ssa, esa = case(O, pkg, "fasta")
    text = np.frombuffer(tb, dtype=np.uint8)
    n = len(tb)
    with ctx.fm_index(bwt, ssa, esa) as plain:
        for call in (lambda: plain.matching_statistics([b"ACG"]), lambda: plain.mems([b"ACG"])):
            with pytest.raises(pkg.PfpError) as e:
                call()
            assert e.value.code == EINVAL and "pfp_fm_build_ms_" in str(e.value)
    with pytest.raises(pkg.PfpError) as e:
        ctx.fm_index_ms(bwt, None, None)
    assert e.value.code == EINVAL
    with pytest.raises(pkg.PfpError) as e:
        ctx.fm_index_ms_dev(1, len(bwt), None, 0, None, 0)      # (refused before anything is read)
    assert e.value.code == EINVAL
    base = str(tmp_path / "t")
    ctx.bigbwt_files(text, base, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    for bad in (text[:-1], np.concatenate([text, text[:1]])):
        with pytest.raises(pkg.PfpError) as e:
            ctx.fm_index_ms_files(base, bad)
        assert e.value.code == EINVAL and str(len(bad)) in str(e.value) and str(n) in str(e.value)
        with pytest.raises(pkg.PfpError) as e:
            ctx.fm_index_ms(bwt, ssa, esa, bad)
        assert e.value.code == EINVAL and str(len(bad)) in str(e.value) and str(n) in str(e.value)
    with ctx.fm_index_ms_files(base, text) as a, ctx.fm_index_ms_files(base) as b, ctx.fm_index_ms(bwt, ssa, esa, text) as d:
        pats = ms_patterns(tb, 4, lengths=(3, 20, 64))
        want = d.matching_statistics(pats)
        for fm in (a, b):
            for x, y in zip(fm.matching_statistics(pats), want):
                assert np.array_equal(x, y)
    # one 0 but three LF cycles: the plain build takes it, the inversion does not
    odd = np.frombuffer(b"a\0ab", dtype=np.uint8)
    rows = np.array([0, 1, 2, 3], dtype=np.uint64)
    pk = lambda r: pkg.pack5(np.stack([r, np.array([3, 1, 2, 0], dtype=np.uint64)[:len(r)]], axis=1).reshape(-1))
    ossa, oesa = pk(rows), pk(rows)                             # every row is a run of its own: a, 0, a, b
    with pytest.raises(pkg.PfpError) as e:
        ctx.fm_index_ms(odd, ossa, oesa)
    assert e.value.code == EFORMAT and "more than one cycle" in str(e.value)
    with ctx.fm_index(odd, ossa, oesa):
        pass
    with ctx.fm_index_ms(odd, ossa, oesa, b"aba") as fm:
        off, ln, pos = fm.matching_statistics([b"ab", b"zz"])
        assert len(ln) == 4
    with ctx.fm_index_ms(bwt, ssa, esa, text) as fm:
        with pytest.raises(pkg.PfpError) as e:
            fm.mems([b"ACGT"], 0)
        assert e.value.code == EINVAL and "min_len" in str(e.value)
        pat = np.frombuffer(b"ACGTACGT" * 8, dtype=np.uint8).copy()
        u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        for off in ([0, 40, 20], [30, 10, 64], [0, 64, 8]):
            off = np.array(off, dtype=np.uint64)
            ln, ps = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint64)
            rc = fm.lib.pfp_fm_ms(fm._h, pat.ctypes.data_as(C.POINTER(C.c_uint8)), u64(off), C.c_uint64(2), ln.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  u64(ps))
            assert rc == EINVAL and "decrease" in ctx.lib.pfp_last_error(ctx._h).decode()
            mo = np.zeros(3, dtype=np.uint64)
            out = C.POINTER(C.c_uint64)()
            rc = fm.lib.pfp_fm_mems(fm._h, pat.ctypes.data_as(C.POINTER(C.c_uint8)), u64(off), C.c_uint64(2), C.c_uint64(1), u64(mo), C.byref(out))
            assert rc == EINVAL and not out
        off, ln, pos = fm.matching_statistics([tb[100:140]])    # (the index is still usable)
        assert list(ln) == list(range(40, 0, -1))
    # a text of the right length but other content: answers for no text, never an access outside the index
    with ctx.fm_index_ms(bwt, ssa, esa, text[::-1].copy()) as fm:
        pats = ms_patterns(tb, 6)
        off, ln, pos = fm.matching_statistics(pats)
        for k, p in enumerate(pats):
            a, b = int(off[k]), int(off[k + 1])
            assert np.all(ln[a:b].astype(np.int64) <= np.arange(len(p), 0, -1))
        assert np.all((pos <= n) | (pos == NONE))
        fm.mems(pats, 2)


@pytest.mark.parametrize("bits", [0, 64])
def test_memory(O, pkg, ctx, bits):
    """the documented bounds (pfpgpu.h): an index with text holds at most (n + 256) bytes and w bytes per run more than the
    plain index with samples; everything goes back at close()"""
    import torch
    text = O.gen_fasta(250_000, 4, 0.002, 7)
    got = ctx.bigbwt(text, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    with pkg.Context(0) as c:
        c.set_index_bits(bits)
        keep = [torch.from_numpy(np.asarray(x).copy()).cuda() for x in (got["bwt"], got["ssa"], got["esa"])]
        torch.cuda.synchronize()
        assert c.mem_stats()["live"] == 0
        for d_text in (torch.from_numpy(np.asarray(text).copy()).cuda(), None):
            torch.cuda.synchronize()
            fm = c.fm_index_ms_dev(keep[0].data_ptr(), keep[0].numel(), keep[1].data_ptr(), keep[1].numel(), keep[2].data_ptr(), keep[2].numel(),
                                   d_text.data_ptr() if d_text is not None else None)
            inf = fm.info()
            n1, r, wb, sigma = inf["n"] + 1, inf["runs"], inf["row_bits"] // 8, inf["sigma"]
            plain = n1 * (1 + sigma / 128 + sigma / 8192 + 0.140625) + 6 * r * wb + 8192
            assert inf["device_bytes"] <= plain + (n1 + 256) + r * wb, (inf, plain)
            tb = bytes(text)
            fm.matching_statistics([tb[10:500], tb[1000:1100] + b"#" + tb[5:50]])
            fm.mems([tb[10:500]], 5)
            fm.close()
            assert c.mem_stats()["live"] == 0
