"""Counting and locating patterns over a BWT and its run samples on the GPU (csrc/fmsearch.hip): FmIndex / pfp_fm_*.

Definitions (include/pfpgpu.h): rows j = 0..n with SA[0] = n; count(P) = the row range [sp, ep) of the suffixes that start with P
(sp = ep = 0 when empty), with samples also SA[sp]; locate(P) = SA[sp], SA[sp+1], ... in row order.  Every expected value here
comes from the oracle's suffix array, not from the feature."""
import numpy as np
import pytest

from textgen import make_text

pytestmark = pytest.mark.gpu

EFORMAT, EINVAL = -6, -1


def full_sa(O, text, sa1=None):
    """SA[0..n] (SA[0] = n) from the oracle's SA[1..n]"""
    sa1 = O.sacak(text) if sa1 is None else sa1
    return np.concatenate([[len(text)], np.asarray(sa1, dtype=np.int64)]).astype(np.int64)


def samples(pkg, bwt, sa):
    """.ssa / .esa bytes from the BWT and SA[0..n]: <j, SA[j]> of the run starts / ends"""
    b = np.asarray(bwt)
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    ends = np.flatnonzero(np.concatenate([b[1:] != b[:-1], [True]]))
    pk = lambda rows: pkg.pack5(np.stack([rows, sa[rows]], axis=1).reshape(-1).astype(np.uint64))
    return pk(starts), pk(ends)


def expected(text, sa, pats):
    """(sp, ep) of each pattern by binary search over the suffix array"""
    tb = bytes(np.asarray(text, dtype=np.uint8))
    n1 = len(sa)
    out = []
    for p in pats:
        if 0 in p:
            out.append((0, 0))
            continue
        m = len(p)

        def bound(strict):
            lo, hi = 0, n1
            while lo < hi:
                mid = (lo + hi) // 2
                s = tb[sa[mid]:sa[mid] + m]
                if s < p or (strict and s == p):
                    lo = mid + 1
                else:
                    hi = mid
            return lo
        sp, ep = bound(False), bound(True)
        out.append((sp, ep) if ep > sp else (0, 0))
    return out


def patterns_for(text, seed):
    rng = np.random.default_rng(seed)
    tb = bytes(np.asarray(text, dtype=np.uint8))
    n = len(tb)
    present = set(tb)
    pats = [b"", b"\x00", tb, tb + tb[:1], b"A\x00C"]
    absent = [c for c in range(1, 256) if c not in present]
    if absent:
        pats += [bytes([absent[0]]), tb[:3] + bytes([absent[-1]])]
    for m in list(range(1, 65)) + [1000]:
        if m > n:
            continue
        for _ in range(2):
            i = int(rng.integers(0, n - m + 1))
            s = bytearray(tb[i:i + m])
            pats.append(bytes(s))
            k = int(rng.integers(0, m))
            s[k] = (s[k] + 1 + int(rng.integers(0, 200))) % 253 + 3          # a mutated copy (never byte 0)
            pats.append(bytes(s))
    return pats


def check_index(fm, text, sa, pats, locate=True):
    want = expected(text, sa, pats)
    sp, ep, first = fm.count(pats, toehold=True)
    for k, (s, e) in enumerate(want):
        assert (int(sp[k]), int(ep[k])) == (s, e), (k, pats[k][:40], (sp[k], ep[k]), (s, e))
        assert int(first[k]) == (int(sa[s]) if e > s else 2**64 - 1), (k, pats[k][:40])
    sp2, ep2 = fm.count(pats)
    assert np.array_equal(sp, sp2) and np.array_equal(ep, ep2)
    if locate:
        off, pos = fm.locate(pats)
        for k, (s, e) in enumerate(want):
            assert int(off[k + 1] - off[k]) == e - s
            assert np.array_equal(pos[off[k]:off[k + 1]].astype(np.int64), sa[s:e]), (k, pats[k][:40])


def small_texts(O):
    rng = np.random.default_rng(7)
    yield "fasta", O.gen_fasta(60000, 4, 0.002, 5)
    yield "dna", rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 300_000)
    yield "all_bytes", np.concatenate([np.arange(3, 256, dtype=np.uint8), rng.integers(3, 256, 100_000, dtype=np.uint8)])
    yield "GATTACA", np.frombuffer(b"GATTACA", dtype=np.uint8)
    yield "a_n", np.full(100_000, ord("a"), dtype=np.uint8)


@pytest.mark.parametrize("which", ["fasta", "dna", "all_bytes", "GATTACA", "a_n"])
def test_small_texts(O, pkg, wctx, which):
    text = dict(small_texts(O))[which]
    sa = full_sa(O, text)
    bwt = O.simplebwt(text)
    ssa, esa = samples(pkg, bwt, sa)
    with wctx.fm_index(bwt, ssa, esa) as fm:
        inf = fm.info()
        assert inf["n"] == len(text) and inf["has_samples"] == 1 and inf["runs"] == len(ssa) // 10
        assert inf["row_bits"] in (32, 64) and inf["sigma"] == len(set(bytes(text)))
        pats = patterns_for(text, 11)
        if which == "a_n":                  # one run of n rows: the chains resume over several launches
            pats += [b"a", b"a" * 1000, b"a" * len(text), b"b"]
        check_index(fm, text, sa, pats)


@pytest.mark.parametrize("idx", range(15))
def test_golden_texts(golden, O, pkg, wctx, idx):
    c = golden[idx]
    text = make_text(c["spec"], O)
    got = wctx.bigbwt(text, c["w"], c["p"], pkg.FLAG_SSA | pkg.FLAG_ESA)
    bwt = got["bwt"]
    if np.count_nonzero(bwt == 0) != 1:          # the reference quirk's output is not a BWT
        with pytest.raises(pkg.PfpError) as e:
            wctx.fm_index(bwt, got["ssa"], got["esa"])
        assert e.value.code == EFORMAT and "bytes 0" in str(e.value)
        return
    n = len(bwt) - 1
    t = text[:n]
    sa = full_sa(O, t, O.bigbwt(text, c["w"], c["p"], O.FLAG_SA)["sa"])
    with wctx.fm_index(bwt, got["ssa"], got["esa"]) as fm:
        check_index(fm, t, sa, patterns_for(t, idx))


def test_max_occ(O, pkg, ctx):
    text = O.gen_fasta(60000, 4, 0.002, 5)
    sa = full_sa(O, text)
    got = ctx.bigbwt(text, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    pats = [b"", b"A", b"ACG", bytes(text[100:110]), bytes(text[5000:5040]), b"\x00"]
    want = expected(text, sa, pats)
    with ctx.fm_index(got["bwt"], got["ssa"], got["esa"]) as fm:
        for K in (1, 2, 3, 64, 1000, len(text) + 5):
            off, pos, sp, ep = fm.locate(pats, max_occ=K, ranges=True)
            for k, (s, e) in enumerate(want):
                assert (int(sp[k]), int(ep[k])) == (s, e)
                cap = min(e - s, K)
                assert np.array_equal(pos[off[k]:off[k + 1]].astype(np.int64), sa[s:s + cap]), (K, k)


def test_dev_and_files_agree(O, pkg, ctx, tmp_path):
    text = O.gen_fasta(50000, 4, 0.002, 11)
    base = str(tmp_path / "t")
    ctx.bigbwt_files(text, base, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    got = ctx.bigbwt(text, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    pats = patterns_for(text, 3)
    with ctx.fm_index_files(base, pkg.FLAG_SSA | pkg.FLAG_ESA) as a, ctx.fm_index(got["bwt"], got["ssa"], got["esa"]) as b:
        assert a.info() == b.info()
        for x, y in zip(a.count(pats, toehold=True), b.count(pats, toehold=True)):
            assert np.array_equal(x, y)
        for x, y in zip(a.locate(pats, max_occ=7), b.locate(pats, max_occ=7)):
            assert np.array_equal(x, y)
    with ctx.fm_index_files(base) as c:             # count only: the .bwt alone
        assert c.info()["has_samples"] == 0
        sp, ep = c.count(pats)
        want = expected(text, full_sa(O, text), pats)
        assert [(int(s), int(e)) for s, e in zip(sp, ep)] == want


def test_bad_input(O, pkg, ctx, tmp_path):
    text = O.gen_fasta(50000, 4, 0.002, 11)
    got = ctx.bigbwt(text, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    bwt, ssa, esa = got["bwt"], got["ssa"], got["esa"]
    for bad in (bwt[bwt != 0], np.concatenate([bwt, [0]]).astype(np.uint8), b""):
        with pytest.raises(pkg.PfpError) as e:
            ctx.fm_index(bad)
        assert e.value.code == EFORMAT
    with pytest.raises(pkg.PfpError) as e:
        ctx.fm_index(bwt[bwt != 0])
    assert "not a BWT: 0 bytes 0" in str(e.value)
    for s, es in ((ssa[:-10], esa), (ssa, esa[:-1]), (np.concatenate([ssa, ssa[-10:]]), esa)):
        with pytest.raises(pkg.PfpError) as e:
            ctx.fm_index(bwt, s, es)
        assert e.value.code == EFORMAT
    pairs = pkg.unpack5(ssa).reshape(-1, 2)
    for i in (0, 3, len(pairs) // 2, len(pairs) - 1):
        moved = pairs.copy()
        moved[i, 0] += 1
        with pytest.raises(pkg.PfpError) as e:
            ctx.fm_index(bwt, pkg.pack5(moved.reshape(-1)), esa)
        assert e.value.code == EFORMAT and ".ssa pair %d" % i in str(e.value)
    epairs = pkg.unpack5(esa).reshape(-1, 2)
    epairs[5, 0] -= 1
    with pytest.raises(pkg.PfpError) as e:
        ctx.fm_index(bwt, ssa, pkg.pack5(epairs.reshape(-1)))
    assert e.value.code == EFORMAT and ".esa pair 5" in str(e.value)
    with pytest.raises(pkg.PfpError) as e:
        ctx.fm_index(bwt, ssa)
    assert e.value.code == EINVAL
    with ctx.fm_index(bwt) as fm:
        with pytest.raises(pkg.PfpError) as e:
            fm.locate([b"ACG"])
        assert e.value.code == EINVAL and ".ssa" in str(e.value) and ".esa" in str(e.value)
        with pytest.raises(pkg.PfpError) as e:
            fm.count([b"ACG"], toehold=True)
        assert e.value.code == EINVAL
    base = str(tmp_path / "t")
    ctx.bigbwt_files(text, base, 10, 100, pkg.FLAG_SSA)
    with pytest.raises(pkg.PfpError) as e:
        ctx.fm_index_files(base, pkg.FLAG_SSA | pkg.FLAG_ESA)
    assert e.value.code == EINVAL and base + ".esa" in str(e.value)


def test_host_offsets_checked(O, pkg, ctx):
    """the host variants copy pat_off[npat] bytes: offsets that decrease are refused before any kernel runs"""
    import ctypes as C
    text = O.gen_fasta(50000, 4, 0.002, 11)
    got = ctx.bigbwt(text, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    pat = np.frombuffer(b"ACGTACGT" * 8, dtype=np.uint8).copy()
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    with ctx.fm_index(got["bwt"], got["ssa"], got["esa"]) as fm:
        for off in ([0, 40, 20], [30, 10, 64], [0, 64, 8]):
            off = np.array(off, dtype=np.uint64)
            sp, ep = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
            rc = fm.lib.pfp_fm_count(fm._h, pat.ctypes.data_as(C.POINTER(C.c_uint8)), u64(off), C.c_uint64(2), u64(sp), u64(ep), None)
            assert rc == EINVAL and "decrease" in ctx.lib.pfp_last_error(ctx._h).decode()
            oo = np.zeros(3, dtype=np.uint64)
            pos = C.POINTER(C.c_uint64)()
            rc = fm.lib.pfp_fm_locate(fm._h, pat.ctypes.data_as(C.POINTER(C.c_uint8)), u64(off), C.c_uint64(2), C.c_uint64(0), None, None,
                                      u64(oo), C.byref(pos))
            assert rc == EINVAL and not pos
        sp, ep = fm.count([b"ACGT", b"TTT"])          # (the index is still usable)
        want = expected(text, full_sa(O, text), [b"ACGT", b"TTT"])
        assert [(int(a), int(b)) for a, b in zip(sp, ep)] == want


@pytest.mark.parametrize("bits", [0, 64])
def test_peak_memory(O, pkg, ctx, bits):
    """the documented bounds (pfpgpu.h): the index (1 + sigma/128 + sigma/8192 + 0.140625) B/row + 6 w/run + 8 KiB; the build
    adds at most 0.140625 B/row and 4 w/run, and the library's scratch (4 MiB here); everything goes back at close()"""
    text = O.gen_fasta(250_000, 4, 0.002, 7)
    got = ctx.bigbwt(text, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    with pkg.Context(0) as c:          # (a context of its own: its peak is the index's alone)
        c.set_index_bits(bits)
        import torch
        keep = [torch.from_numpy(np.asarray(x).copy()).cuda() for x in (got["bwt"], got["ssa"], got["esa"])]
        torch.cuda.synchronize()
        base = c.mem_stats()
        assert base["live"] == 0
        fm = c.fm_index_dev(keep[0].data_ptr(), keep[0].numel(), keep[1].data_ptr(), keep[1].numel(), keep[2].data_ptr(), keep[2].numel())
        inf = fm.info()
        n1, r, wb = inf["n"] + 1, inf["runs"], inf["row_bits"] // 8
        pats = patterns_for(text, 5)[:100]
        fm.count(pats, toehold=True)
        fm.locate(pats[5:], max_occ=100)
        st = c.mem_stats()
        sigma = inf["sigma"]
        index = n1 * (1 + sigma / 128 + sigma / 8192 + 0.140625) + 6 * r * wb + 8192
        assert inf["device_bytes"] <= index, (inf, index)
        bound = index + n1 * 0.140625 + 4 * r * wb + (4 << 20)
        assert st["peak"] <= bound, (st, inf, bound)
        fm.close()
        assert c.mem_stats()["live"] == 0


def _fullsize(pkg, ctx, synth, name, need_gb):
    import torch
    free, _ = torch.cuda.mem_get_info(torch.device("cuda", 0))
    if free < need_gb * (1 << 30):
        pytest.skip(f"needs about {need_gb} GB of free device memory")
    ctx.pool_trim()
    text = synth.workload_text_torch(torch.device("cuda", 0), name)
    torch.cuda.empty_cache()
    n = text.numel()
    bwt = torch.empty(n + 17, dtype=torch.uint8, device=text.device)
    used, outs = ctx.bigbwt_formats_dev(text.data_ptr(), n, bwt.data_ptr(), 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    assert used == n
    return text, bwt, outs


@pytest.mark.parametrize("name,need_gb,npat,m,brute", [("c3", 40, 100_000, 32, 64), ("huge_s", 200, 4000, 24, 8)])
def test_fullsize(pkg, ctx, synth, name, need_gb, npat, m, brute):
    """configs[2] and the 12.6 GB collection (u64 rows, SA values above 2^32), both -s -e: sampled and mutated patterns"""
    import torch
    text, bwt, outs = _fullsize(pkg, ctx, synth, name, need_gb)
    dev = text.device
    n = text.numel()
    try:
        (ssa, ssa_b), (esa, esa_b) = outs["ssa"], outs["esa"]
        with pkg.Context(0) as c:
            torch.cuda.synchronize()           # (the library works on a stream of its own: torch's writes must be done)
            fm = c.fm_index_dev(bwt.data_ptr(), n + 1, ssa, ssa_b, esa, esa_b)
            for p, _ in outs.values():
                ctx.dev_free(p)
            outs = {}
            inf = fm.info()
            assert inf["n"] == n and inf["row_bits"] == (64 if n + 1 >= 2**32 else 32)
            g = torch.Generator(device="cpu").manual_seed(5)
            start = torch.randint(0, n - m, (npat,), generator=g).to(dev)
            P = text[start[:, None] + torch.arange(m, device=dev)[None, :]]
            mut = torch.rand(npat, generator=g).to(dev) < 0.1
            col = torch.randint(0, m, (npat,), generator=g).to(dev)
            rows = torch.arange(npat, device=dev)
            P[rows[mut], col[mut]] = torch.where(P[rows[mut], col[mut]] == ord("A"), ord("C"), ord("A")).to(torch.uint8)
            pat = P.reshape(-1).contiguous()
            off = torch.arange(0, npat * m + 1, m, dtype=torch.int64, device=dev)
            sp, ep, first = (torch.zeros(npat, dtype=torch.int64, device=dev) for _ in range(3))
            torch.cuda.synchronize()
            fm.count_dev(pat.data_ptr(), off.data_ptr(), npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr())
            out_off = torch.zeros(npat + 1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            fm.locate_dev(npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr(), 0, out_off.data_ptr())
            total = int(out_off[-1])
            pos = torch.zeros(total + 1, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            fm.locate_dev(npat, sp.data_ptr(), ep.data_ptr(), first.data_ptr(), 0, out_off.data_ptr(), pos.data_ptr())
            pos = pos[:total]
            cnt = ep - sp
            assert torch.equal(out_off[1:] - out_off[:-1], cnt)
            assert bool((cnt[~mut] >= 1).all())
            owner = torch.repeat_interleave(torch.arange(npat, device=dev), cnt)
            # every located position matches the text, and the sampled position is among its pattern's
            assert bool((pos <= n - m).all())
            assert torch.equal(text[pos[:, None] + torch.arange(m, device=dev)[None, :]], P[owner])
            hit = torch.zeros(npat, dtype=torch.bool, device=dev)
            hit[owner[pos == start[owner]]] = True
            assert bool(hit[~mut].all())
            # distinct within each pattern
            key = owner * (n + 1) + pos
            assert torch.unique(key).numel() == total
            # the toehold is the first located position
            has = cnt > 0
            assert torch.equal(first[has], pos[out_off[:-1][has]])
            # counts against a brute-force scan of the whole text
            for k in range(brute):
                pk = P[k]
                hitm = text[:n - m + 1] == pk[0]
                for j in range(1, m):
                    hitm &= text[j:n - m + 1 + j] == pk[j]
                found = sum(int(hitm[i:i + (1 << 28)].sum()) for i in range(0, hitm.numel(), 1 << 28))
                assert found == int(cnt[k]), k
            fm.close()
            assert c.mem_stats()["live"] == 0
    finally:
        for p, _ in outs.values():
            ctx.dev_free(p)
        del text, bwt
        ctx.pool_trim()
        torch.cuda.empty_cache()
