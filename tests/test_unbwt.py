"""Inverting and checking a BWT on the GPU (csrc/unbwt.hip): pfp_unbwt / pfp_unbwt_dev / pfp_check_bwt_dev.

The conventions (include/pfpgpu.h): a .bwt of n+1 bytes holds exactly one 0; .sa = SA[1..n] as 5-byte ints; .ssa / .esa =
pairs <j, SA[j]> of the run starts / ends.  n+1 bytes are a BWT iff they hold one 0 and LF is a single cycle."""
import time

import numpy as np
import pytest

from textgen import make_text

pytestmark = pytest.mark.gpu


def dev(a):
    """numpy bytes -> a CUDA uint8 tensor (16 spare bytes, so that an empty array still has a pointer)"""
    import torch
    t = torch.zeros(len(a) + 16, dtype=torch.uint8, device="cuda")
    if len(a):
        t[:len(a)] = torch.from_numpy(np.array(a, dtype=np.uint8))
    return t


def check(ctx, bwt, text=None, sa=None, ssa=None, esa=None):
    keep = [dev(bwt)] + [dev(x) if x is not None else None for x in (text, sa, ssa, esa)]
    p = [k.data_ptr() if k is not None else None for k in keep]
    return ctx.check_bwt_dev(p[0], len(bwt), p[1], p[2], p[3], len(ssa) if ssa is not None else 0, p[4], len(esa) if esa is not None else 0)


def clean(r):
    assert all(r[k] is None for k in ("text_mismatch", "sa_mismatch", "ssa_mismatch", "esa_mismatch")), r


def small_texts(O):
    yield "fasta", O.gen_fasta(60000, 4, 0.002, 5)
    yield "short", np.frombuffer(b"GATTACA", dtype=np.uint8)
    rng = np.random.default_rng(7)
    yield "all_bytes", np.concatenate([np.arange(3, 256, dtype=np.uint8), rng.integers(3, 256, 100_000, dtype=np.uint8)])
    yield "dna", rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 300_000)


@pytest.mark.parametrize("which", ["fasta", "short", "all_bytes", "dna"])
def test_round_trip(O, wctx, which):
    text = dict(small_texts(O))[which]
    bwt = wctx.bigbwt(text, 10, 100, 0)["bwt"] if len(text) > 1000 else O.simplebwt(text)      # (the chain needs 2 phrases)
    assert np.array_equal(wctx.unbwt(bwt), text)


def quirk_is_not_a_bwt(pkg, ctx, c, bwt):
    """where the first window triggers, the reference (and so this builder) emits 0x02 where the 0 belongs -
    the output is not a BWT, and the check says so"""
    if np.count_nonzero(bwt == 0) == 1:
        return False
    assert not c["bwt_equals_simplebwt"]
    with pytest.raises(pkg.PfpError) as e:
        ctx.unbwt(bwt)
    assert e.value.code == -6 and "bytes 0" in str(e.value)
    return True


@pytest.mark.parametrize("idx", range(15))
def test_round_trip_golden_texts(golden, O, pkg, wctx, idx):
    c = golden[idx]
    text = make_text(c["spec"], O)
    bwt = wctx.bigbwt(text, c["w"], c["p"], 0)["bwt"]
    if quirk_is_not_a_bwt(pkg, wctx, c, bwt):
        return
    got = wctx.unbwt(bwt)
    assert len(got) == len(bwt) - 1 and np.array_equal(got, text[:len(got)])      # (special_byte: the chain stops at a byte <= 2)


def test_edge_cases(wctx):
    assert len(wctx.unbwt(b"\x00")) == 0                                     # n = 0: the empty text
    assert bytes(wctx.unbwt(b"A\x00")) == b"A"
    run = 1 << 20                                                           # a^n: BWT = a^n . 0
    assert np.array_equal(wctx.unbwt(b"a" * run + b"\x00"), np.full(run, ord("a"), dtype=np.uint8))
    t = np.arange(3, 256, dtype=np.uint8)                                  # distinct ascending bytes: BWT = T[n-1], 0, T[0..n-2]
    bwt = np.concatenate([[t[-1], 0], t[:-1]]).astype(np.uint8)
    assert np.array_equal(wctx.unbwt(bwt), t)


@pytest.mark.parametrize("n1", [(8 << 20) + 1, (12 << 20) + 2])
def test_transfer_sizes_that_split_unevenly(ctx, n1):
    """a host <-> device copy is cut into whole 4 KiB pages for a few threads; a size that leaves a remainder of a byte or two
    over the threads (8 MiB + 1 over two, 12 MiB + 2 and 12 MiB + 1 over three) must arrive whole"""
    import torch
    n = n1 - 1                                                              # T = a^(n-1) b: BWT = b, 0, a^(n-1) - its last byte is not 0
    bwt = np.full(n1, ord("a"), dtype=np.uint8)
    bwt[0], bwt[1] = ord("b"), 0
    text = ctx.unbwt(bwt)                                                   # n1 bytes in, n out
    assert len(text) == n and text[-1] == ord("b") and (text[:-1] == ord("a")).all()
    src = torch.randint(0, 256, (n1,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                                # (the library copies on its own stream)
    assert np.array_equal(ctx.fetch_dev(src.data_ptr(), n1), src.cpu().numpy())


def test_unbwt_dev(O, ctx):
    import torch
    text = O.gen_fasta(60000, 4, 0.002, 5)
    bwt = ctx.bigbwt(text, 10, 100, 0)["bwt"]
    d_bwt = dev(bwt)
    out = torch.full((len(text) + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    ctx.unbwt_dev(d_bwt.data_ptr() + 0, len(bwt), out.data_ptr() + 3)          # (an unaligned destination)
    got = out.cpu().numpy()
    assert np.array_equal(got[3:3 + len(text)], text)
    assert (got[:3] == 0xEE).all() and (got[3 + len(text):] == 0xEE).all()    # nothing written outside


@pytest.mark.parametrize("idx", range(15))
def test_golden_outputs_check_clean(golden, O, pkg, wctx, idx):
    """the library's .bwt / .sa / .ssa / .esa of every golden case check clean against the text; ssa_runs / esa_runs are
    the reference's pair counts"""
    c = golden[idx]
    text = make_text(c["spec"], O)
    full = wctx.bigbwt(text, c["w"], c["p"], pkg.FLAG_SA)
    samp = wctx.bigbwt(text, c["w"], c["p"], pkg.FLAG_SSA | pkg.FLAG_ESA)
    n = len(full["bwt"]) - 1
    if quirk_is_not_a_bwt(pkg, wctx, c, full["bwt"]):
        return
    r = check(wctx, full["bwt"], text[:n], full["sa"], samp["ssa"], samp["esa"])
    assert r["n"] == n
    clean(r)
    assert r["ssa_runs"] == c["runs"]["6"]["ssa_len"] // 10 and r["esa_runs"] == c["runs"]["6"]["esa_len"] // 10


@pytest.fixture(scope="module")
def case200k(O, pkg, ctx):
    text = O.gen_fasta(50000, 4, 0.002, 11)
    assert 190_000 < len(text) < 220_000
    full = ctx.bigbwt(text, 10, 100, pkg.FLAG_SA)
    samp = ctx.bigbwt(text, 10, 100, pkg.FLAG_SSA | pkg.FLAG_ESA)
    return text, full["bwt"].copy(), full["sa"].copy(), samp["ssa"].copy(), samp["esa"].copy()


def test_exact_mismatch_reporting(pkg, wctx, case200k):
    text, bwt, sa, ssa, esa = case200k
    n = len(text)
    r = check(wctx, bwt, text, sa, ssa, esa)
    clean(r)
    runs_s, runs_e = r["ssa_runs"], r["esa_runs"]
    assert runs_s == len(ssa) // 10 and runs_e == len(esa) // 10
    # one .sa entry (j = k) changed
    for k in (1, 777, n // 2, n):
        bad = pkg.unpack5(sa)
        bad[k - 1] ^= 1
        assert check(wctx, bwt, text, pkg.pack5(bad))["sa_mismatch"] == k
    # two entries: the smaller index is reported
    bad = pkg.unpack5(sa)
    bad[n - 5] += 3; bad[100] += 1
    assert check(wctx, bwt, sa=pkg.pack5(bad))["sa_mismatch"] == 101
    # the SA value of .ssa pair i, the position of pair i
    pairs = pkg.unpack5(ssa).reshape(-1, 2)
    for i in (0, 5, runs_s // 3, runs_s - 1):
        bad = pairs.copy()
        bad[i, 1] += 1
        assert check(wctx, bwt, ssa=pkg.pack5(bad.reshape(-1)))["ssa_mismatch"] == i
    bad = pairs.copy()
    bad[7, 0] += 1
    assert check(wctx, bwt, ssa=pkg.pack5(bad.reshape(-1)))["ssa_mismatch"] == 7
    # .esa: the last pair dropped, one pair too many
    r = check(wctx, bwt, esa=esa[:-10])
    assert r["esa_mismatch"] == runs_e - 1 and r["esa_runs"] == runs_e
    assert check(wctx, bwt, esa=np.concatenate([esa, esa[-10:]]))["esa_mismatch"] == runs_e
    assert check(wctx, bwt, ssa=ssa[:-3])["ssa_mismatch"] == runs_s - 1
    # the text with byte p flipped
    for p in (0, 1, 15, 16, 4097, n // 3, n - 1):
        t = text.copy()
        t[p] ^= 0x20
        assert check(wctx, bwt, t)["text_mismatch"] == p
    t = text.copy()
    t[n - 3] ^= 1; t[n // 2] ^= 1
    assert check(wctx, bwt, t)["text_mismatch"] == n // 2


def test_not_a_bwt(pkg, wctx, case200k):
    text, bwt, *_ = case200k
    for bad in (b"a\x00ab", b"ab\x00\x00c", b"abcab", b"", b"\x00\x00"):
        with pytest.raises(pkg.PfpError) as e:
            wctx.unbwt(bad)
        assert e.value.code == -6, bad
    with pytest.raises(pkg.PfpError) as e:
        check(wctx, np.frombuffer(b"a\x00ab", dtype=np.uint8))
    assert e.value.code == -6 and "cycle" in str(e.value)
    with pytest.raises(pkg.PfpError) as e:
        wctx.unbwt(bwt[bwt != 0])
    assert e.value.code == -6 and "0" in str(e.value)
    # two unequal bytes of a valid BWT swapped: never "all clean"
    rng = np.random.default_rng(3)
    for _ in range(12):
        i, j = rng.integers(0, len(bwt), 2)
        if bwt[i] == bwt[j]:
            continue
        b = bwt.copy()
        b[i], b[j] = b[j], b[i]
        try:
            r = check(wctx, b, text)
        except pkg.PfpError as e:
            assert e.code == -6
            continue
        assert r["text_mismatch"] is not None


def test_random_bytes_never_hang(pkg, ctx):
    """arbitrary 1 MB inputs with one 0: a permutation of several cycles, or (rarely) a BWT of something; either way the
    call returns promptly"""
    rng = np.random.default_rng(5)
    for alpha in (2, 4, 256):
        b = (rng.integers(0, min(alpha, 253), 1 << 20) + 3).astype(np.uint8)
        b[int(rng.integers(0, len(b)))] = 0
        t0 = time.time()
        try:
            ctx.unbwt(b)
        except pkg.PfpError as e:
            assert e.code == -6
        assert time.time() - t0 < 30


@pytest.mark.parametrize("bits", [0, 64])
def test_check_peak_memory(pkg, case200k, bits):
    """a fresh context's device memory stays under 10 bytes per BWT byte (the inputs are the caller's) and is all handed
    back; a failing call leaves nothing allocated either"""
    text, bwt, sa, ssa, esa = case200k
    with pkg.Context(0) as c:
        c.set_index_bits(bits)
        clean(check(c, bwt, text, sa, ssa, esa))
        st = c.mem_stats()
        assert st["live"] == 0 and 0 < st["peak"] <= 10 * len(bwt), st
        with pytest.raises(pkg.PfpError):
            c.unbwt(np.frombuffer(b"a\x00ab", dtype=np.uint8))
        assert c.mem_stats()["live"] == 0


def _fullsize(pkg, ctx, synth, golden_full, name, need_gb):
    import torch
    if name not in golden_full:
        pytest.skip("no reference digest committed for this workload")
    free, _ = torch.cuda.mem_get_info(torch.device("cuda", 0))
    if free < need_gb * (1 << 30):
        pytest.skip(f"needs about {need_gb} GB of free device memory")
    g = golden_full[name]
    ctx.pool_trim()
    text = synth.workload_text_torch(torch.device("cuda", 0), name)
    torch.cuda.empty_cache()
    n = text.numel()
    bwt = torch.empty(n + 17, dtype=torch.uint8, device=text.device)
    used, outs = ctx.bigbwt_formats_dev(text.data_ptr(), n, bwt.data_ptr(), g["w"], g["p"], g["flags"])
    assert used == n
    return g, text, bwt, outs


@pytest.mark.parametrize("name,need_gb", [("c3", 40), ("huge_s", 230)])
def test_fullsize_check(pkg, ctx, synth, golden_full, name, need_gb):
    """configs[2] (-s -e) and the 12.6 GB north-star output (-s; n+1 > 2^32: the 8-byte layout) check clean against the text,
    within 10 bytes of library memory per BWT byte; the warm 12.6 GB check takes at most 2 s (twice the measured time)"""
    import torch
    g, text, bwt, outs = _fullsize(pkg, ctx, synth, golden_full, name, need_gb)
    n = text.numel()
    try:
        ssa, ssa_b = outs.get("ssa", (None, 0))
        esa, esa_b = outs.get("esa", (None, 0))
        ctx.pool_trim()
        times = []
        with pkg.Context(0) as c:          # (a context of its own: its peak is the check's alone)
            for _ in range(2):
                r = c.check_bwt_dev(bwt.data_ptr(), n + 1, text.data_ptr(), None, ssa, ssa_b, esa, esa_b)
                times.append(r["ms"])
                clean(r)
                assert r["n"] == n and r["ssa_runs"] == ssa_b // 10 and r["esa_runs"] == esa_b // 10
            st = c.mem_stats()
        assert st["peak"] <= 10 * (n + 1), st
        if name == "huge_s":
            assert n + 1 > 2**32 and min(times) <= 2000, times      # measured: 911 ms (profiles/unbwt_time.json)
    finally:
        for p, _ in outs.values():
            ctx.dev_free(p)
        del text, bwt
        ctx.pool_trim()
        torch.cuda.empty_cache()
