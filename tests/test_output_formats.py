"""GPU: csrc/runsample.hip slice by slice - pfp_pack5_dev, pfp_sample_runs_dev, the sparse d_sa of pfp_bigbwt_dev, the two producers of
.ssa / .esa, and the ranks' pieces of them where a slice ends inside a run - against tests/formats_reference.py (which
tests/test_formats_reference.py holds against the oracle).  Every comparison is exact equality of bytes or integers; every output
buffer has a guard band on either side and is compared whole, so a byte written outside the result fails the test.
tests/README.md ("Tests of the output formats, slice by slice") has the tables."""
import importlib

import numpy as np
import pytest
import torch

import formats_cases as FC
import formats_reference as FR
from textgen import make_text

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xEE
EINVAL, ELIMIT = -1, -5
SENTINEL = -1          # all 64 bits set: no SA value (they are below 2^40)


def dev(a):
    """a host array as a device tensor, complete before the library's own stream may look at it"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def filled(count, value, dtype):
    t = torch.full((count,), value, dtype=dtype, device="cuda")
    torch.cuda.synchronize()          # (torch fills on its stream, the library writes on its own)
    return t


def dev_bytes(a, before, after, shift=1):
    """the bytes on the device between GUARD + shift copies of `before` and GUARD copies of `after`: (tensor, address of a[0])"""
    t = dev(np.concatenate([np.full(GUARD + shift, before, np.uint8), np.asarray(a, dtype=np.uint8), np.full(GUARD, after, np.uint8)]))
    return t, t.data_ptr() + GUARD + shift


def dev_u64(v):
    """the values on the device at an address that is 8 and not 16 bytes aligned (as d_sa + 1 is), between spare entries of all ones"""
    ones = np.full(9, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    t = dev(np.concatenate([ones, np.asarray(v, dtype=np.uint64), ones[:8]]).view(np.int64))
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 72


def guarded(nbytes, shift=0):
    """an output buffer of FILL bytes: (tensor, address of the result's first byte, check(want))"""
    t = filled(GUARD + shift + nbytes + GUARD, FILL, torch.uint8)

    def check(want):
        want = np.asarray(want, dtype=np.uint8)
        assert len(want) == nbytes
        whole = np.concatenate([np.full(GUARD + shift, FILL, np.uint8), want, np.full(GUARD, FILL, np.uint8)])
        got = t.cpu().numpy()
        bad = np.flatnonzero(got != whole)
        assert len(bad) == 0, "first wrong byte at %d of a result of %d bytes (guards of %d, %d)" % (bad[0] - GUARD - shift, nbytes, GUARD + shift, GUARD)
    return t, t.data_ptr() + GUARD + shift, check


# ---------------------------------------------------------------------------------------- pfp_pack5_dev
@pytest.mark.parametrize("count", FC.PACK_COUNTS)
def test_pack5_at_every_count_and_output_alignment(ctx, count):
    """count values from an address that is 8-byte aligned only, to 0, 1, 5 and 15 bytes past a 16-byte boundary: 5 * count bytes change,
    bits 40..63 of the input do not matter"""
    for kind in ("low", "high", "ones"):
        v = FC.pack_values(count, kind)
        want = FR.pack5(v)
        src, src_ptr = dev_u64(v)
        for off in FC.PACK_OUT_OFFSETS:
            out, out_ptr, check = guarded(5 * count, 16 + off)
            assert (out_ptr - off) % 16 == 0
            ctx.pack5_dev(src_ptr, count, out_ptr)
            check(want)
    if count == 17:      # every 16-byte chunk of this one ends up at b0 mod 5 = 0..4 with a full and a partial store; high bits masked off
        assert np.array_equal(FR.pack5(FC.pack_values(17, "high")), FR.pack5(FC.pack_values(17, "low")))


def test_pack5_of_nothing_writes_nothing(ctx):
    src, src_ptr = dev_u64(FC.pack_values(4, "ones"))
    out, out_ptr, check = guarded(0)
    ctx.pack5_dev(src_ptr, 0, out_ptr)
    check(np.zeros(0, np.uint8))
    ctx.pack5_dev(0, 0, 0)


# ---------------------------------------------------------------------------------------- pfp_sample_runs_dev, dense SA
def sample(ctx, bwt_ptr, sa_ptr, count, pos_base, left, right, run_end, want, shift=0):
    """the count-only call and the placing call into a guarded buffer; both must give what `want` (bytes) holds"""
    assert len(want) % 10 == 0
    k = len(want) // 10
    assert ctx.sample_runs_dev(bwt_ptr, None, count, pos_base, left, right, run_end) == k
    out, out_ptr, check = guarded(10 * k, shift)
    assert ctx.sample_runs_dev(bwt_ptr, sa_ptr, count, pos_base, left, right, run_end, out_ptr, k) == k
    check(want)
    return k


@pytest.mark.parametrize("run_end", [False, True], ids=["ssa", "esa"])
@pytest.mark.parametrize("name", FC.ARRAYS)
def test_whole_array_without_neighbours(ctx, name, run_end):
    """-1 / -1 over the whole array at an odd address, at three position bases (the last one ends at 2^40 exactly).  The bytes stored
    around the array repeat its edge bytes: a kernel that looked at memory where it is told -1 would miss the edge's pair."""
    a, v = FC.array(name), FC.sa_values(name)
    n = len(a)
    bwt, bwt_ptr = dev_bytes(a, a[0], a[-1])
    assert bwt_ptr % 2 == 1
    sa, sa_ptr = dev_u64(v)
    for kind in FC.POS_BASES:
        base = FC.pos_base(kind, n)
        want = FR.run_pairs(a, v, 0, n, -1, -1, run_end, base)
        k = sample(ctx, bwt_ptr, sa_ptr, n, base, -1, -1, run_end, want, shift=3)
        assert k >= 1 and (name != "alternating" or k == n) and (name != "constant" or k == 1)


@pytest.mark.parametrize("run_end", [False, True], ids=["ssa", "esa"])
@pytest.mark.parametrize("name", FC.SLICED)
def test_slices_with_true_neighbours_add_up(ctx, name, run_end):
    """slices of 1, 2, 15, 16, 17, 31, 33, 0, 4095, 4096, 4097 positions and cuts around a run start and inside a run; each slice with the
    bytes next to it and pos_base = lo; piece by piece = the reference's, back to back = the whole array's"""
    a, v, cuts = FC.array(name), FC.sa_values(name), FC.cut_list(name)
    for shift in (0, 1):          # even and odd addresses for every slice
        bwt, bwt_ptr = dev_bytes(a, 0, 0, shift)
        sa, sa_ptr = dev_u64(v)
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            left, right = FR.true_neighbours(a, lo, hi)
            want = FR.run_pairs(a, v, lo, hi, left, right, run_end, lo)
            sample(ctx, bwt_ptr + lo, sa_ptr + 8 * lo, hi - lo, lo, left, right, run_end, want)
            parts.append(want)
        assert np.array_equal(np.concatenate(parts), FR.run_pairs(a, v, 0, len(a), -1, -1, run_end, 0))


@pytest.mark.parametrize("run_end", [False, True], ids=["ssa", "esa"])
def test_slice_with_runs_at_its_chunk_and_tile_edges(ctx, run_end):
    """the array whose runs begin and end at 15, 16, 17, 4095, 4096, 4097 and 8192 as a slice of a larger one, at an odd offset"""
    big, v, lo, hi = FC.embedded("edges")
    bwt, bwt_ptr = dev_bytes(big, 0, 0, 0)
    sa, sa_ptr = dev_u64(v)
    assert (bwt_ptr + lo) % 2 == 1
    left, right = FR.true_neighbours(big, lo, hi)
    for kind in FC.POS_BASES:
        base = FC.pos_base(kind, hi - lo)
        sample(ctx, bwt_ptr + lo, sa_ptr + 8 * lo, hi - lo, base, left, right, run_end, FR.run_pairs(big, v, lo, hi, left, right, run_end, base))
    for cut in FC.EDGE_POINTS:          # ... and cut at each of those points: a run's first position opens the right-hand slice
        parts = []
        for x, y in ((lo, lo + cut), (lo + cut, hi)):
            l, r = FR.true_neighbours(big, x, y)
            parts.append(FR.run_pairs(big, v, x, y, l, r, run_end, x - lo))
            sample(ctx, bwt_ptr + x, sa_ptr + 8 * x, y - x, x - lo, l, r, run_end, parts[-1])
        assert np.array_equal(np.concatenate(parts), FR.run_pairs(big, v, lo, hi, left, right, run_end, 0))


def _other(b):
    return (int(b) + 1) % 256


@pytest.mark.parametrize("run_end", [False, True], ids=["ssa", "esa"])
@pytest.mark.parametrize("length", [1, 2, 15, 16, 17, 31, 32, 33, 48, 4096, 4097])
def test_neighbour_arguments_win_over_memory(ctx, length, run_end):
    """the slice inside a larger buffer, the bytes stored before and after it equal to its edge bytes or different from them, the
    arguments the other way round, or -1: the pairs follow the arguments.  (The reference sees the slice and the arguments only.)  A load
    that reached one byte outside [0, count) would take the stored byte for the argument."""
    for name in ("constant", "random_runs"):
        a = FC.array(name)[100: 100 + length]
        v = FC.sa_values(name)[100: 100 + length]
        sa, sa_ptr = dev_u64(v)
        first, last = int(a[0]), int(a[-1])
        for mem_l, mem_r in ((first, last), (_other(first), _other(last))):
            bwt, bwt_ptr = dev_bytes(a, mem_l, mem_r, 1)
            for left in (-1, first, _other(first)):
                for right in (-1, last, _other(last)):
                    want = FR.run_pairs(a, v, 0, length, left, right, run_end, 500)
                    sample(ctx, bwt_ptr, sa_ptr, length, 500, left, right, run_end, want)


@pytest.mark.parametrize("length", [1, 16, 100, 5000])
def test_slice_inside_one_run(ctx, length):
    """equal neighbours on both sides: no pair in either file; -1 on one side: exactly one pair, the edge's, in that side's file"""
    a, v = FC.array("constant"), FC.sa_values("constant")
    g = int(a[0])
    lo = 1001
    bwt, bwt_ptr = dev_bytes(a, g, g)
    sa, sa_ptr = dev_u64(v)
    none = np.zeros(0, np.uint8)
    first = FR.pack5(np.array([lo, v[lo]], dtype=np.uint64))
    last = FR.pack5(np.array([lo + length - 1, v[lo + length - 1]], dtype=np.uint64))
    for left, right, ssa, esa in ((g, g, none, none), (-1, g, first, none), (g, -1, none, last)):
        for run_end, want in ((False, ssa), (True, esa)):
            assert np.array_equal(FR.run_pairs(a, v, lo, lo + length, left, right, run_end, lo), want)
            sample(ctx, bwt_ptr + lo, sa_ptr + 8 * lo, length, lo, left, right, run_end, want)


def test_empty_slice(ctx):
    a, v = FC.array("random_runs"), FC.sa_values("random_runs")
    bwt, bwt_ptr = dev_bytes(a, 0, 0)
    sa, sa_ptr = dev_u64(v)
    for run_end in (False, True):
        for left, right in ((-1, -1), (int(a[4]), int(a[5])), (-1, int(a[5]))):
            sample(ctx, bwt_ptr + 5, sa_ptr + 40, 0, 5, left, right, run_end, np.zeros(0, np.uint8))
        assert ctx.sample_runs_dev(0, None, 0) == 0


def test_refusals_leave_the_context_usable(pkg, ctx):
    """PFP_ELIMIT for an output buffer one pair too small and for positions beyond 5 bytes; PFP_EINVAL for a neighbour that is no byte and
    for an output without SA values; the buffer untouched, and a good call answered after each"""
    a, v = FC.array("random_runs"), FC.sa_values("random_runs")
    n = len(a)
    bwt, bwt_ptr = dev_bytes(a, 0, 0)
    sa, sa_ptr = dev_u64(v)
    want = FR.run_pairs(a, v, 0, n, -1, -1, False, 0)
    k = len(want) // 10

    def refused(code, *args):
        out, out_ptr, check = guarded(10 * k)
        with pytest.raises(pkg.PfpError) as ei:
            ctx.sample_runs_dev(*[out_ptr if x == "out" else x for x in args])
        assert ei.value.code == code, str(ei.value)
        check(np.full(10 * k, FILL, np.uint8))
        sample(ctx, bwt_ptr, sa_ptr, n, 0, -1, -1, False, want)

    refused(ELIMIT, bwt_ptr, sa_ptr, n, 0, -1, -1, False, "out", k - 1)
    top = (1 << 40) - n
    sample(ctx, bwt_ptr, sa_ptr, n, top, -1, -1, True, FR.run_pairs(a, v, 0, n, -1, -1, True, top))          # ends at 2^40: accepted
    refused(ELIMIT, bwt_ptr, sa_ptr, n, top + 1, -1, -1, False, "out", k)
    refused(ELIMIT, bwt_ptr, None, n, top + 1, -1, -1, False)
    for left, right in ((256, -1), (-2, -1), (-1, 256), (-1, -2)):
        refused(EINVAL, bwt_ptr, sa_ptr, n, 0, left, right, False, "out", k)
    refused(EINVAL, bwt_ptr, None, n, 0, -1, -1, False, "out", k)


# ---------------------------------------------------------------------------------------- the chain's sparse d_sa, both producers
CHAIN_TEXTS = ("repeat_w6", "gen_small", "n_run", "copies400")
_chain = {}


def chain_case(name, O, golden):
    """(text, w, p, bwt, SA of every BWT position, .ssa bytes, .esa bytes) by the oracle, computed once"""
    if name not in _chain:
        if name == "copies400":
            import merge_cases
            c = merge_cases.CASES[name]
            text, w, p = merge_cases.text_of(O, name), c["w"], c["p"]
        else:
            c = {x["name"]: x for x in golden}[name]
            text, w, p = make_text(c["spec"], O), c["w"], c["p"]
            assert len(text) < 100000
        sampled = O.bigbwt(text, w, p, O.FLAG_SSA | O.FLAG_ESA)
        sa = np.concatenate([[len(text)], O.bigbwt(text, w, p, O.FLAG_SA)["sa"]]).astype(np.uint64)
        _chain[name] = (text, w, p, sampled["bwt"], sa, O.pack5(sampled["ssa"].reshape(-1)), O.pack5(sampled["esa"].reshape(-1)))
    return _chain[name]


def _trace_names(ctx):
    return {r["name"] for r in ctx.kernel_trace()}


@pytest.mark.parametrize("flags", [2, 4, 6], ids=["s", "e", "s_e"])
@pytest.mark.parametrize("name", CHAIN_TEXTS)
def test_sparse_sa_of_the_chain_and_both_producers(request, pkg, O, golden, wctx, name, flags):
    """pfp_bigbwt_dev with -s / -e into a caller's d_sa full of a sentinel: the entries at the run boundaries are the oracle's SA values,
    every other entry is still the sentinel; pfp_sample_runs_dev on that d_bwt / d_sa (run_count_kernel, run_place_kernel) gives the
    oracle's files, and so does pfp_bigbwt_formats_dev from the merge's run maps (bitmap_place_kernel): the same bytes"""
    ctx = wctx
    text, w, p, want_bwt, want_sa, ssa, esa = chain_case(name, O, golden)
    n = len(text)
    assert np.array_equal(FR.run_pairs(want_bwt, want_sa, 0, n + 1, -1, -1, False, 0), ssa)          # (the reference, on this text too)
    assert np.array_equal(FR.run_pairs(want_bwt, want_sa, 0, n + 1, -1, -1, True, 0), esa)
    files = [(key, run_end, want) for key, flag, run_end, want in (("ssa", pkg.FLAG_SSA, False, ssa), ("esa", pkg.FLAG_ESA, True, esa)) if flags & flag]
    d_text = dev(text)
    d_bwt, bwt_ptr, _ = guarded(n + 1 + 16)          # (GUARD is a multiple of 16: the chain wants d_bwt 16-byte aligned)
    d_sa = filled(n + 1, SENTINEL, torch.int64)
    try:
        assert ctx.bigbwt_dev(d_text.data_ptr(), n, bwt_ptr, d_sa.data_ptr(), w, p, flags) == n
        assert ctx.stats()["index_bits"] == request.node.callspec.params["wctx"]
        assert np.array_equal(d_bwt[GUARD: GUARD + n + 1].cpu().numpy(), want_bwt)
        assert (d_bwt[:GUARD] == FILL).all() and (d_bwt[GUARD + n + 1 + 16:] == FILL).all()
        got_sa = d_sa.cpu().numpy().view(np.uint64)
        mask = FR.boundary_mask(want_bwt)
        assert 2 <= mask.sum() < n + 1
        assert np.array_equal(got_sa[mask], want_sa[mask]), "an entry at a run boundary is not the oracle's SA value"
        untouched = got_sa[~mask] == np.uint64(0xFFFFFFFFFFFFFFFF)
        assert untouched.all(), "%d entries that are no run boundary were written, the first at %d" % (
            (~untouched).sum(), np.flatnonzero(~mask)[np.flatnonzero(~untouched)[0]])
        ctx.set_kernel_trace(True)
        by_pass = {}
        for key, run_end, want in files:
            k = len(want) // 10
            assert ctx.sample_runs_dev(bwt_ptr, None, n + 1, 0, -1, -1, run_end) == k
            out, out_ptr, check = guarded(10 * k)
            assert ctx.sample_runs_dev(bwt_ptr, d_sa.data_ptr(), n + 1, 0, -1, -1, run_end, out_ptr, k) == k
            check(want)
            by_pass[key] = out[GUARD: GUARD + 10 * k].cpu().numpy()
        names = _trace_names(ctx)
        assert {"pfp::run_count_kernel", "pfp::run_place_kernel"} <= names and "pfp::bitmap_place_kernel" not in names
        # the other producer: the merge's run maps, no pass over the BWT
        d_bwt2, bwt2_ptr, _ = guarded(n + 1 + 16)
        ctx.set_kernel_trace(True)
        used, outs = ctx.bigbwt_formats_dev(d_text.data_ptr(), n, bwt2_ptr, w, p, flags)
        names = _trace_names(ctx)
        got = {}
        for key, (ptr, nbytes) in outs.items():
            got[key] = ctx.fetch_dev(ptr, nbytes)
            ctx.dev_free(ptr)
        assert used == n and np.array_equal(d_bwt2[GUARD: GUARD + n + 1].cpu().numpy(), want_bwt)
        assert "pfp::bitmap_place_kernel" in names and "pfp::run_count_kernel" not in names and "pfp::run_place_kernel" not in names
        assert set(got) == {key for key, _, _ in files}
        for key, run_end, want in files:
            assert np.array_equal(got[key], want), key
            assert np.array_equal(got[key], by_pass[key]), key
    finally:
        ctx.set_kernel_trace(False)


# ---------------------------------------------------------------------------------------- the ranks' pieces, slices that end inside a run
@pytest.mark.parametrize("width", [32, 64], ids=["idx32", "idx64"])
@pytest.mark.parametrize("R", [4, 6])
def test_ranks_whose_slices_end_inside_a_run(pkg, O, R, width):
    """-s -e over R virtual ranks on a text whose BWT has one run longer than two slices: some slice's first position is no run start
    after all (bitmap_place_kernel's drop_first), some slice's last position no run end (drop_pos), and a slice wholly inside the run
    has one boundary in either map, drops it and returns no pair.  Every rank's pieces = the reference's for its [lo, hi) under its
    true neighbours; back to back = the oracle's files; the offsets tile."""
    from test_distributed import _pieces
    d = importlib.import_module("bigbwt_amd.dist")
    c = FC.dist_case(O, R)
    text, cuts = c["text"], c["cuts"]
    n = len(text)
    flags = pkg.FLAG_SSA | pkg.FLAG_ESA
    want = O.bigbwt(text, c["w"], c["p"], flags)
    bwt = want["bwt"]
    sa = np.concatenate([[n], O.bigbwt(text, c["w"], c["p"], O.FLAG_SA)["sa"]]).astype(np.uint64)
    a, b = FC.longest_run(bwt)
    ctxs = [pkg.Context(0) for _ in range(R)]
    try:
        for x in ctxs:
            x.set_index_bits(64 if width == 64 else 0)
            x.set_window_hash(False)
        shards = [dev(text[cuts[r]:cuts[r + 1]].copy()) for r in range(R)]
        res = d.simulate(ctxs, shards, c["w"], c["p"], flags, halo=c["halo"])
        assert {r["stats"]["glob"]["index_bits"] for r in res} == {width}
        assert res[0]["lo"] == 0 and res[-1]["hi"] == n + 1 and all(res[k]["hi"] == res[k + 1]["lo"] for k in range(R - 1))
        assert np.array_equal(np.concatenate([r["bwt"].cpu().numpy() for r in res]), bwt)
        # the slices the ranks really got: a cut strictly inside the run, a slice wholly inside it
        assert any(a < r["lo"] < b for r in res[1:])
        assert any(a < r["lo"] and r["hi"] < b for r in res)
        for key, run_end in (("ssa", False), ("esa", True)):
            off = 0
            for rank, r in enumerate(res):
                lo, hi = r["lo"], r["hi"]
                left, right = FR.true_neighbours(bwt, lo, hi)
                piece = FR.run_pairs(bwt, sa, lo, hi, left, right, run_end, lo)
                got = r[key].cpu().numpy()
                assert len(got) == len(piece), (key, rank, len(got) // 10, len(piece) // 10)
                assert np.array_equal(got, piece), (key, rank)
                assert r[key + "_off"] == off, (key, rank)
                off += len(piece)
            assert np.array_equal(_pieces(res, key), O.pack5(want[key].reshape(-1))), key
            assert res[0]["sampled_total"][key] == len(want[key])
        assert any(r["ssa"].numel() == 0 and r["esa"].numel() == 0 for r in res)          # the rank inside the run: no pair in either file
    finally:
        for x in ctxs:
            x.close()
