"""Seed extension on the GPU (csrc/fmextend.hip): FmIndex.extend / extend_dev / align / align_dev.

Definitions (include/pfpgpu.h, "Extending seeds"): a candidate (p, delta) gives the window lo = clamp(delta - k), hi = clamp(delta +
m + k); the result is (d*, s, e) with e the smallest end that attains d* = min Levenshtein(P, T[s..e)) and s the largest start for
that e, or (0xFF, UINT64_MAX, UINT64_MAX) where d* > k.  Every expected value comes from the unbanded numpy reference
(extend_reference.py, itself checked against a brute force in test_extend_reference.py); the alignments of a pattern are the
reference's composite over the MEMs that the already tested FmIndex.mems lists.

Texts: approx_reference.make_text: `copies`, `dna`, `ab` (a^3000 b a^2000: many ties in e and s) and `GATTACA` (windows clipped at
both ends, m > n).  Patterns: substrings with 0..k planted substitutions, insertions and deletions, also at the first and the last
byte, of the lengths at the edges of 16-byte loads and 64-bit words; random strings, a byte 0, an absent byte; one pattern of 5000
bytes with 20 edits at k = 32.  Diagonals: around the planted one by 0, 1, k and k + 1, left of the text by more than m + k, at and
past its end, and across its end."""
import ctypes as C
import functools

import numpy as np
import pytest

import approx_reference as R
import extend_reference as E
from extend_reference import planted

pytestmark = pytest.mark.gpu

EINVAL, ELIMIT = -1, -5
TEXTS = ("copies", "dna", "ab", "GATTACA")
BUDGETS = (0, 1, 2, 8, 32)
LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 128, 129, 300)
CASES = [(name, k) for name in TEXTS for k in BUDGETS]


@functools.lru_cache(maxsize=None)
def text_of(name):
    return R.make_text(name)


def samples(pkg, bwt, sa):
    """.ssa / .esa bytes from the BWT and SA[0..n]: <j, SA[j]> of the run starts / ends"""
    b = np.asarray(bwt)
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    ends = np.flatnonzero(np.concatenate([b[1:] != b[:-1], [True]]))
    pk = lambda rows: pkg.pack5(np.stack([rows, sa[rows]], axis=1).reshape(-1).astype(np.uint64))
    return pk(starts), pk(ends)


_parts = {}


def index_of(O, pkg, ctx, name):
    """an index with text over one of TEXTS (the BWT and the samples are computed once)"""
    if name not in _parts:
        text = text_of(name)
        bwt = O.simplebwt(text)
        _parts[name] = (bwt,) + samples(pkg, bwt, R.full_sa(O, text))
    bwt, ssa, esa = _parts[name]
    return ctx.fm_index_ms(bwt, ssa, esa, text_of(name))


@functools.lru_cache(maxsize=None)
def case(name, k):
    """(patterns, cand_pat, cand_diag, planted): planted = [(candidate, edits)] for the candidates on their pattern's own diagonal"""
    text = text_of(name)
    tb, n = text.tobytes(), len(text)
    rng = np.random.default_rng(1000 * TEXTS.index(name) + k)
    alphabet = sorted(set(tb))
    absent = min(c for c in range(1, 256) if c not in alphabet)
    pats, cp, cd, own = [], [], [], []

    def add(pat, diags, at=None, edits=0):
        for dg in diags:
            if at is not None and dg == at:
                own.append((len(cp), edits))
            cp.append(len(pats))
            cd.append(int(dg))
        pats.append(pat)

    def around(i, m):
        return [i + j for j in (-k - 1, -k, -1, 0, 1, k, k + 1)] + [-(m + k) - 5, n, n + 7, n - m // 2]

    for m in LENGTHS:
        m0 = min(m, n)
        starts = {0, n - m0, int(rng.integers(0, n - m0 + 1))}
        if name == "ab":
            starts |= {3000 - m0 // 2, 3001 - min(m0, 3001)}
        for q, i in enumerate(sorted(starts)):
            for edits in sorted({0, min(1, k), min(2, k), k}):
                pat = planted(rng, tb[i:i + m0], edits, alphabet, at_ends=(q + edits) % 2 == 0)
                add(pat, around(i, len(pat)) if edits in (0, k) else [i, i - k, i + k + 1], at=i, edits=edits)
    if name == "dna" and k == 32:
        i = 7000
        pat = planted(rng, tb[i:i + 5000], 20, alphabet, at_ends=True)
        add(pat, [i, i - 33, i + 32], at=i, edits=20)
    for m in (5, 40, 200):
        add(bytes(rng.choice(alphabet, m).astype(np.uint8)), [0, n // 2, n - m, n - 1])
    mid = tb[n // 2:n // 2 + 40]
    add(b"\x00", [0, 3, n])
    add(mid[:9] + b"\x00" + mid[10:], [n // 2, n // 2 + 1])
    add(bytes([absent]), [0, n - 1])
    add(mid[:20] + bytes([absent]) + mid[20:], [n // 2, n // 2 - k])
    add(tb[:64], [0, -1, -k, 1])
    if n < 100:
        add(tb + tb, [0, -n, 3])                            # m > n
    add(tb[-64:], [n - min(n, 64), n - min(n, 64) + k, n - min(n, 64) - 1])
    return pats, np.array(cp, dtype=np.uint32), np.array(cd, dtype=np.int64), own


@functools.lru_cache(maxsize=None)
def expected(name, k):
    """the reference's (dist, start, end) of case(name, k), computed once and shared"""
    pats, cp, cd, _ = case(name, k)
    return E.extend(text_of(name), pats, cp.tolist(), cd.tolist(), k)


def same(got, want, what, names=("dist", "start", "end")):
    for g, w, nm in zip(got, want, names):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, nm, np.flatnonzero(g != w)[:8] if g.shape == w.shape else (g.shape, w.shape))


@pytest.mark.parametrize("name,k", CASES)
def test_extend(O, pkg, wctx, name, k):
    pats, cp, cd, _ = case(name, k)
    with index_of(O, pkg, wctx, name) as fm:
        same(fm.extend(pats, cp, cd, k), expected(name, k), (name, k))


def test_the_cases_are_not_vacuous():
    """asserted on the reference's own output: the reference alone must satisfy these"""
    kinds = set()
    for name, k in CASES:
        text = text_of(name)
        n = len(text)
        pats, cp, cd, own = case(name, k)
        dist, start, end = expected(name, k)
        for c, edits in own:
            assert edits <= k and int(dist[c]) <= edits, (name, k, c, edits, int(dist[c]))
        for c in range(len(cp)):
            m, d = len(pats[cp[c]]), int(dist[c])
            if d == 0xFF:
                kinds.add("none")
                continue
            span = int(end[c]) - int(start[c])
            kinds.add("exact" if d == 0 else "shorter" if span < m else "longer" if span > m else "same")
            if int(cd[c]) - k < 0:
                kinds.add("lo clipped")
            if int(cd[c]) + m + k > n:
                kinds.add("hi clipped")
            if name == "ab" and m:
                lo, hi = E.window(n, m, int(cd[c]), k)
                row = E.last_row(np.frombuffer(pats[cp[c]], dtype=np.uint8), text[lo:hi], True)
                if np.count_nonzero(row == d) > 1:
                    kinds.add("ties in e")
    assert kinds == {"none", "exact", "shorter", "longer", "same", "lo clipped", "hi clipped", "ties in e"}, kinds


@pytest.mark.parametrize("k", [0, 2, 8])
def test_batch_independence(O, pkg, ctx, k):
    """permuted, split in halves and duplicated: every candidate keeps its triple"""
    pats, cp, cd, _ = case("dna", k)
    want = expected("dna", k)
    order = np.random.default_rng(4).permutation(len(cp))
    half = len(cp) // 2
    with index_of(O, pkg, ctx, "dna") as fm:
        got = fm.extend(pats, cp[order], cd[order], k)
        same(got, [w[order] for w in want], "permuted")
        a, b = fm.extend(pats, cp[:half], cd[:half], k), fm.extend(pats, cp[half:], cd[half:], k)
        same([np.concatenate(x) for x in zip(a, b)], want, "halves")
        same(fm.extend(pats, np.repeat(cp, 3), np.repeat(cd, 3), k), [np.repeat(w, 3) for w in want], "duplicated")
        # the same candidates against a pattern list in another order
        back = np.arange(len(pats))[::-1]
        same(fm.extend([pats[i] for i in back], (len(pats) - 1 - cp).astype(np.uint32), cd, k), want, "patterns reversed")


def test_no_such_pattern_and_no_candidates(O, pkg, ctx):
    with index_of(O, pkg, ctx, "GATTACA") as fm:
        dist, start, end = fm.extend([b"GATT", b"ACA"], [0, 2, 1, 7, 2**32 - 1], [0, 0, 4, 0, 0], 1)
        assert dist.tolist() == [0, 0xFF, 0, 0xFF, 0xFF]
        assert start.tolist() == [0, 2**64 - 1, 4, 2**64 - 1, 2**64 - 1] and end.tolist() == [4, 2**64 - 1, 7, 2**64 - 1, 2**64 - 1]
        dist, start, end = fm.extend([b"GATT"], [], [], 1)
        assert len(dist) == len(start) == len(end) == 0 and dist.dtype == np.uint8 and start.dtype == np.uint64
        dist, start, end = fm.extend([], [0], [0], 1)
        assert dist.tolist() == [0xFF]
        big = np.iinfo(np.int64)
        dist, start, end = fm.extend([b"GA", b""], [0, 0, 1, 1], [big.min, big.max, big.min, big.max], 2)      # (no overflow at the ends of int64)
        assert (dist.tolist(), start.tolist(), end.tolist()) == ([2, 2, 0, 0], [0, 7, 0, 7], [0, 7, 0, 7])


def test_bad_arguments(O, pkg, ctx):
    usable = lambda fm: fm.extend([b"TTA"], [0], [3], 1)
    text = text_of("GATTACA")
    with index_of(O, pkg, ctx, "GATTACA") as fm:
        for k in (33, -1):
            with pytest.raises(pkg.PfpError) as e:
                fm.extend([b"GAT"], [0], [0], k)
            assert e.value.code == EINVAL
            with pytest.raises(pkg.PfpError) as e:
                fm.align([b"GAT"], k, 2)
            assert e.value.code == EINVAL
            assert [x.tolist() for x in usable(fm)] == [[0], [2], [5]]
        with pytest.raises(pkg.PfpError) as e:
            fm.align([b"GAT"], 1, 0)                        # min_seed = 0
        assert e.value.code == EINVAL
        with pytest.raises(pkg.PfpError) as e:
            fm.align([b"GAT"], 1, 2, thresholds=True)       # no thresholds were added
        assert e.value.code == EINVAL
        with pytest.raises(pkg.PfpError) as e:
            fm.extend([b"GAT", b"A" * 65536], [0], [0], 1)
        assert e.value.code == ELIMIT
        with pytest.raises(pkg.PfpError) as e:
            fm.align([b"GAT", b"A" * 65536], 1, 2)
        assert e.value.code == ELIMIT
        d, s, e_ = fm.extend([b"A" * 65535], [0], [0], 32)   # (the limit itself is served)
        assert d.tolist() == [0xFF]
        assert [x.tolist() for x in usable(fm)] == [[0], [2], [5]]
        pat = np.frombuffer(b"GATTACAGATTACA", dtype=np.uint8).copy()
        u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        for off in ([0, 7, 3], [5, 2, 9]):
            off = np.array(off, dtype=np.uint64)
            cp, cd = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int64)
            dist, start, end = np.full(1, 7, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
            rc = fm.lib.pfp_fm_extend(fm._h, pat.ctypes.data_as(C.POINTER(C.c_uint8)), u64(off), C.c_uint64(2),
                                      cp.ctypes.data_as(C.POINTER(C.c_uint32)), cd.ctypes.data_as(C.POINTER(C.c_int64)), C.c_uint64(1), C.c_int(1),
                                      dist.ctypes.data_as(C.POINTER(C.c_uint8)), u64(start), u64(end))
            assert rc == EINVAL and "decrease" in ctx.lib.pfp_last_error(ctx._h).decode() and dist[0] == 7
            aln_off = np.zeros(3, dtype=np.uint64)
            ps, pe, pd = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)()
            rc = fm.lib.pfp_fm_align(fm._h, pat.ctypes.data_as(C.POINTER(C.c_uint8)), u64(off), C.c_uint64(2), C.c_uint64(2), C.c_int(1),
                                     C.c_uint64(0), C.c_int(0), u64(aln_off), C.byref(ps), C.byref(pe), C.byref(pd))
            assert rc == EINVAL and not ps and not pe and not pd
        assert [x.tolist() for x in usable(fm)] == [[0], [2], [5]]
    bwt = O.simplebwt(text)
    with ctx.fm_index(bwt, *samples(pkg, bwt, R.full_sa(O, text))) as plain:      # an index without text
        for call in (lambda: plain.extend([b"GAT"], [0], [0], 1), lambda: plain.align([b"GAT"], 1, 2)):
            with pytest.raises(pkg.PfpError) as e:
                call()
            assert e.value.code == EINVAL
        assert [int(x[0]) for x in plain.count([b"TTA"])] == [7, 8]


def test_device_call(O, pkg, ctx):
    """torch tensors in, torch tensors out; what lies behind the outputs stays"""
    import torch
    k = 8
    pats, cp, cd, _ = case("copies", k)
    dev = torch.device("cuda", ctx.device)
    pat, off = pkg.pfp._patterns(pats)
    nc = len(cp)
    d_pat = torch.from_numpy(pat.copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_cp = torch.from_numpy(cp.view(np.int32).copy()).to(dev)
    d_cd = torch.from_numpy(cd.copy()).to(dev)
    d_dist = torch.full((nc + 16,), 0x5A, dtype=torch.uint8, device=dev)
    d_start, d_end = (torch.full((nc + 2,), -7, dtype=torch.int64, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    with index_of(O, pkg, ctx, "copies") as fm:
        fm.extend_dev(d_pat.data_ptr(), d_off.data_ptr(), len(pats), d_cp.data_ptr(), d_cd.data_ptr(), nc, k, d_dist.data_ptr(),
                      d_start.data_ptr(), d_end.data_ptr())
    got = d_dist[:nc].cpu().numpy(), d_start[:nc].cpu().numpy().view(np.uint64), d_end[:nc].cpu().numpy().view(np.uint64)
    same(got, expected("copies", k), "device")
    assert (d_dist[nc:] == 0x5A).all() and (d_start[nc:] == -7).all() and (d_end[nc:] == -7).all()


# ---------------------------------------------------------------- align
@functools.lru_cache(maxsize=None)
def reads(name):
    """reads of 40 to 300 bytes with 0 to 3 planted edits, a read that is an exact substring, and one without a seed"""
    text = text_of(name)
    tb, n = text.tobytes(), len(text)
    rng = np.random.default_rng(77 + TEXTS.index(name))
    alphabet = sorted(set(tb))
    out = []
    for q, m in enumerate((40, 40, 64, 100, 100, 150, 150, 150, 200, 300, 300, 41)):
        i = int(rng.integers(0, n - m + 1))
        out.append(planted(rng, tb[i:i + m], q % 4, alphabet, at_ends=q % 3 == 0))
    out.append(b"")
    out.append(bytes(rng.choice(alphabet, 7).astype(np.uint8)))
    return out


_memo = {}


def want_align(fm, name, pats, L, k, max_aln, thresholds):
    mem_off, mems = fm.mems(pats, L, thresholds=thresholds)
    return E.align(text_of(name), pats, mem_off, mems, k, max_aln, _memo.setdefault((name, k), {}))


ALN = ("aln_off", "start", "end", "dist")


@pytest.mark.parametrize("thresholds", [False, True], ids=["phoni", "thr"])
@pytest.mark.parametrize("name", ["copies", "dna"])
def test_align(O, pkg, ctx, name, thresholds):
    pats = reads(name)
    seen = 0
    with index_of(O, pkg, ctx, name) as fm:
        if thresholds:
            fm.add_thresholds()
        for L in (8, 20):
            for k in (0, 2, 8):
                for max_aln in (0, 1, 3):
                    got = fm.align(pats, k, L, max_aln, thresholds)
                    same(got, want_align(fm, name, pats, L, k, max_aln, thresholds), (name, L, k, max_aln, thresholds), ALN)
                    seen += len(got[1])
    assert seen > 100


def test_align_special_patterns(O, pkg, ctx):
    text = text_of("dna")
    tb = text.tobytes()
    i, m = 4321, 60
    read = tb[i:i + m]
    assert tb.count(read) == 1
    with index_of(O, pkg, ctx, "dna") as fm:
        off, start, end, dist = fm.align([read, b"ACGTACGTACGTACG", b"", read], 2, 20)
        assert off.tolist() == [0, 1, 1, 1, 2] and start.tolist() == [i, i] and end.tolist() == [i + m, i + m] and dist.tolist() == [0, 0]
        off, start, end, dist = fm.align([], 2, 20)
        assert off.tolist() == [0] and len(start) == len(end) == len(dist) == 0
        off, start, end, dist = fm.align([b"", b"\x00\x00"], 2, 1)
        assert off.tolist() == [0, 0, 0]


@pytest.mark.parametrize("thresholds", [False, True], ids=["phoni", "thr"])
def test_align_in_groups_and_resumed(O, pkg, ctx, monkeypatch, thresholds):
    """PFP_FM_SEQ_BUDGET=50: the host call takes its patterns in many groups; PFP_FM_MS_STEPS=7: the matching statistics resume"""
    pats = reads("copies") + reads("dna")
    with index_of(O, pkg, ctx, "copies") as fm:
        if thresholds:
            fm.add_thresholds()
        want = fm.align(pats, 2, 8, 3, thresholds)
        same(want, want_align(fm, "copies", pats, 8, 2, 3, thresholds), "usual", ALN)
        monkeypatch.setenv("PFP_FM_SEQ_BUDGET", "50")
        same(fm.align(pats, 2, 8, 3, thresholds), want, "groups", ALN)
        monkeypatch.setenv("PFP_FM_MS_STEPS", "7")
        same(fm.align(pats, 2, 8, 3, thresholds), want, "groups, resumed", ALN)
        monkeypatch.delenv("PFP_FM_SEQ_BUDGET")
        same(fm.align(pats, 2, 8, 3, thresholds), want, "resumed", ALN)


def test_align_device_call(O, pkg, ctx):
    import torch
    pats = reads("copies")
    k, L = 2, 8
    dev = torch.device("cuda", ctx.device)
    pat, off = pkg.pfp._patterns(pats)
    npat = len(pats)
    d_pat = torch.from_numpy(pat.copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_aoff = torch.zeros(npat + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    with index_of(O, pkg, ctx, "copies") as fm:
        want = want_align(fm, "copies", pats, L, k, 0, False)
        fm.align_dev(d_pat.data_ptr(), d_off.data_ptr(), npat, k, L, d_aoff.data_ptr())
        assert np.array_equal(d_aoff.cpu().numpy().view(np.uint64), want[0])
        A = int(d_aoff[-1])
        d_start, d_end = (torch.full((A + 2,), -7, dtype=torch.int64, device=dev) for _ in range(2))
        d_dist = torch.full((A + 16,), 0x5A, dtype=torch.uint8, device=dev)
        d_aoff.zero_()
        torch.cuda.synchronize()
        for some in ((d_start.data_ptr(), d_end.data_ptr(), None), (None, None, d_dist.data_ptr()), (d_start.data_ptr(), None, d_dist.data_ptr())):
            with pytest.raises(pkg.PfpError) as e:
                fm.align_dev(d_pat.data_ptr(), d_off.data_ptr(), npat, k, L, d_aoff.data_ptr(), *some)
            assert e.value.code == EINVAL
        fm.align_dev(d_pat.data_ptr(), d_off.data_ptr(), npat, k, L, d_aoff.data_ptr(), d_start.data_ptr(), d_end.data_ptr(), d_dist.data_ptr())
        got = (d_aoff.cpu().numpy().view(np.uint64), d_start[:A].cpu().numpy().view(np.uint64), d_end[:A].cpu().numpy().view(np.uint64),
               d_dist[:A].cpu().numpy())
        same(got, want, "device", ALN)
        assert (d_dist[A:] == 0x5A).all() and (d_start[A:] == -7).all() and (d_end[A:] == -7).all()
        d_aoff.zero_()
        torch.cuda.synchronize()
        fm.align_dev(d_pat.data_ptr(), d_off.data_ptr(), npat, k, L, d_aoff.data_ptr(), max_aln=1)
        assert np.array_equal(d_aoff.cpu().numpy().view(np.uint64), want_align(fm, "copies", pats, L, k, 1, False)[0])
