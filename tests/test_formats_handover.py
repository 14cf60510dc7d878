"""GPU: pfp_bigbwt_formats_dev hands the caller the pool blocks its outputs were written into (csrc/chain.hip: emit_outputs, hand_out)
instead of copies of them: the bytes are those of the host path, the pool reaches a steady state in which no call goes to the
driver, and an output without pairs is still a pointer pfp_dev_free takes."""
import numpy as np
import pytest

from textgen import make_text

pytestmark = pytest.mark.gpu

FLAGS = [1, 2, 4, 6, 7]


def formats_dev(ctx, text, w, p, flags):
    """-> (n_used, bwt bytes, {name: bytes}) through the device entry point; every output block is given back"""
    import torch
    d_text = torch.from_numpy(np.array(text, dtype=np.uint8)).cuda()
    d_bwt = torch.empty(len(text) + 1 + 16, dtype=torch.uint8, device="cuda")
    used, outs = ctx.bigbwt_formats_dev(d_text.data_ptr(), len(text), d_bwt.data_ptr(), w, p, flags)
    got = {}
    for key, (ptr, nbytes) in outs.items():
        assert ptr
        got[key] = ctx.fetch_dev(ptr, nbytes)
        ctx.dev_free(ptr)
    return used, d_bwt[: used + 1].cpu().numpy(), got


@pytest.fixture(scope="module")
def texts(O, golden):
    c = {x["name"]: x for x in golden}["gen_small"]
    small = make_text(c["spec"], O)
    coll = O.gen_fasta(50000, 6, 0.002, 17)[:300000]
    assert len(coll) == 300000
    return {"gen_small": (small, c["w"], c["p"]), "collection": (coll, 10, 100)}


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", ["gen_small", "collection"])
def test_bytes_equal_the_host_path(pkg, ctx, texts, name, flags):
    """.sa (-S), .ssa, .esa and both: byte for byte what pfp_bigbwt returns in host memory; -S together with -s / -e is refused by
    both entry points alike (bigbwt:59-61)"""
    text, w, p = texts[name]
    if flags == 7:
        with pytest.raises(Exception) as host_err:
            ctx.bigbwt(text, w, p, flags)
        with pytest.raises(Exception) as dev_err:
            formats_dev(ctx, text, w, p, flags)
        assert type(host_err.value) is type(dev_err.value) and str(host_err.value) == str(dev_err.value)
        return
    want = ctx.bigbwt(text, w, p, flags)
    used, bwt, got = formats_dev(ctx, text, w, p, flags)
    assert used == len(text) and np.array_equal(bwt, want["bwt"])
    names = [k for k, bit in (("sa", 1), ("ssa", 2), ("esa", 4)) if flags & bit]
    assert sorted(got) == sorted(names)
    for k in names:
        assert got[k].dtype == np.uint8 and np.array_equal(got[k], np.asarray(want[k]).view(np.uint8).reshape(-1)), (name, flags, k)
        assert len(got[k]) == (5 * len(text) if k == "sa" else 10 * (len(got[k]) // 10)) and len(got[k]) > 0


def test_pool_is_steady(pkg, ctx, texts):
    """five calls in a row, each after the previous outputs went back with pfp_dev_free: after two warm-up calls no request of the
    chain reaches the driver - the blocks handed out come back into the pool where the next call finds them"""
    import torch
    text, w, p = texts["collection"]
    d_text = torch.from_numpy(np.ascontiguousarray(text)).cuda()
    d_bwt = torch.empty(len(text) + 1 + 16, dtype=torch.uint8, device="cuda")
    for flags in (6, 1):
        outs, counts, first = {}, [], None
        for _ in range(5):
            for ptr, _nb in outs.values():
                ctx.dev_free(ptr)
            used, outs = ctx.bigbwt_formats_dev(d_text.data_ptr(), len(text), d_bwt.data_ptr(), w, p, flags)
            counts.append(ctx.pool_counters()["driver_allocs"])
            sizes = {k: nb for k, (_ptr, nb) in outs.items()}
            first = first or sizes
            assert used == len(text) and sizes == first
        for ptr, _nb in outs.values():
            ctx.dev_free(ptr)
        assert counts[1] == counts[2] == counts[3] == counts[4], (flags, counts)


@pytest.mark.parametrize("flags", [1, 2, 4, 6])
def test_one_byte_text(pkg, ctx, golden, flags):
    """a text of one byte has a parse of one phrase, which the chain refuses as the reference does (bwtparse.c:244): both entry
    points refuse it alike, and the device one leaves no block behind; the shortest texts that do have a parse (the golden
    known-answer texts of 29 and 27 bytes) come back as pointers with the host path's bytes behind them"""
    text = np.frombuffer(b"A", dtype=np.uint8)
    live = ctx.mem_stats()["live"]
    with pytest.raises(pkg.PfpError) as host_err:
        ctx.bigbwt(text, 10, 100, flags)
    with pytest.raises(pkg.PfpError) as dev_err:
        formats_dev(ctx, text, 10, 100, flags)
    assert str(host_err.value) == str(dev_err.value) and "fewer than 2 phrases" in str(dev_err.value)
    assert ctx.mem_stats()["live"] == live
    for name in ("kat1", "kat_q1"):
        c = {x["name"]: x for x in golden}[name]
        text = make_text(c["spec"])
        want = ctx.bigbwt(text, c["w"], c["p"], flags)
        used, bwt, got = formats_dev(ctx, text, c["w"], c["p"], flags)
        assert used == len(text) < 30 and np.array_equal(bwt, want["bwt"])
        assert sorted(got) == sorted(k for k, bit in (("sa", 1), ("ssa", 2), ("esa", 4)) if flags & bit)
        for k, v in got.items():
            assert np.array_equal(v, np.asarray(want[k]).view(np.uint8).reshape(-1))
