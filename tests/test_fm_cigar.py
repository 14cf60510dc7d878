"""Edit scripts on the GPU (csrc/fmcigar.hip): FmIndex.cigar / cigar_dev / align(cigar=True).

Definitions (include/pfpgpu.h, "Edit scripts"): alignment (p, s, e) gives dist = Levenshtein(P, T[s..e)) and the run-length encoded
script that rules 1-4 read backwards from (m, L); 0xFF and no runs where the span is not one of the text, the lengths differ by more
than k or the cost exceeds k.  Every expected value comes from the unbanded numpy reference (cigar_reference.py, itself checked
against a brute force in test_cigar_reference.py), exactly; every returned script also goes through the reference's validator.

Texts: approx_reference.make_text: `copies`, `dna`, `ab` (a^3000 b a^2000: ties between I and D placements around the b) and
`GATTACA` (m > n).  Budgets: the edges of every number of cells per lane.  Lengths: the edges of the 16-row packing.  Alignments:
what FmIndex.extend finds for patterns with 0..k planted edits (the script then costs d and has no D at either end), the same
spans moved or resized by 1 and k at either end (leading and trailing D and I runs), and the spans without a script."""
import ctypes as C
import functools

import numpy as np
import pytest

import approx_reference as R
import cigar_reference as G
import extend_reference as E
from extend_reference import planted

pytestmark = pytest.mark.gpu

EINVAL, ELIMIT = -1, -5
TEXTS = ("copies", "dna", "ab", "GATTACA")
BUDGETS = (0, 1, 7, 8, 15, 16, 23, 24, 32)
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 300)
CASES = [(name, k) for name in TEXTS for k in BUDGETS]
RES = ("dist", "cig_off", "cig")


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
    """(patterns, diagonals, extra): pattern q is extended along diagonals[q]; extra = [(pattern, s, e)], the spans given outright"""
    text = text_of(name)
    tb, n = text.tobytes(), len(text)
    rng = np.random.default_rng(3000 * TEXTS.index(name) + k)
    alphabet = sorted(set(tb))
    absent = min(c for c in range(1, 256) if c not in alphabet)
    pats, diags, extra = [], [], []
    for m in LENGTHS:
        m0 = min(m, n)
        starts = {0, n - m0, int(rng.integers(0, n - m0 + 1))}
        if name == "ab":
            starts |= {3000 - m0 // 2}
        for q, i in enumerate(sorted(starts)):
            for edits in sorted({0, min(1, k), k // 2, k}):
                pats.append(planted(rng, tb[i:i + m0], edits, alphabet, at_ends=(q + edits) % 2 == 0))
                diags.append(i)
            # k + 1 substitutions at distinct places: a span of cost k + 1 where no cheaper script exists
            if m0 > k:
                p = bytearray(tb[i:i + m0])
                for j in rng.choice(m0, k + 1, replace=False).tolist():
                    p[j] = int(rng.choice([c for c in alphabet if c != p[j]] or [absent]))
                extra.append((len(pats), i, i + m0))
                pats.append(bytes(p))
                diags.append(i)
    if name == "dna" and k == 32:
        pats.append(planted(rng, tb[7000:12000], 20, alphabet, at_ends=True))
        diags.append(7000)
    h = n // 2
    mid = tb[h:h + 40]
    w = len(mid)
    for pat in (mid[:9] + b"\x00" + mid[10:], mid[:20] + bytes([absent]) + mid[21:], b"\x00", bytes([absent])):
        extra.append((len(pats), h, h + len(pat)))          # a byte 0 and an absent byte: substitutions
        pats.append(pat)
        diags.append(h)
    extra += [(len(pats), 3, 3), (len(pats), 3, 3 + k), (len(pats), 0, 0), (len(pats), n, n), (len(pats), n - min(k, n), n)]      # the empty pattern
    pats.append(b"")
    diags.append(3)
    p0 = len(pats)
    pats.append(mid)
    diags.append(h)
    if n < 100:
        for more in (1, k, k + 1):                          # m > n
            extra.append((len(pats), 0, n))
            pats.append(tb + tb[:more])
            diags.append(0)
    # no script: the lengths differ by k + 1, s > e, e = n + 1, the ends of uint64, a pattern index = npat and the largest one
    extra += [(p0, h, h + w + k + 1), (p0, h + k + 1, h + w), (p0, h + 5, h + 4), (p0, n + 1 - w, n + 1), (p0, n + 1, n + 1), (p0, h, 2**64 - 1),
              (p0, 2**64 - 1, 2**64 - 1), (len(pats), h, h + w), (2**32 - 1, h, h + w)]
    return pats, np.array(diags, dtype=np.int64), extra


def alignments(name, k, ext):
    """(aln_pat, start, end, found): the extensions ext = (d, s, e) of case(name, k) - the first `found` alignments - then their
    spans moved and resized, then the case's extra spans"""
    n = len(text_of(name))
    pats, _, extra = case(name, k)
    d, s, e = (x.tolist() for x in ext)
    rows = [(q, s[q], e[q]) for q in range(len(pats)) if d[q] != 0xFF]
    found = len(rows)
    for q, s0, e0 in rows[:found]:
        for ds, de in ((1, 0), (-1, 0), (0, 1), (0, -1), (k, 0), (-k, 0), (0, k), (0, -k)):
            if s0 + ds >= 0 and e0 + de >= 0 and (ds, de) != (0, 0):
                rows.append((q, s0 + ds, e0 + de))      # (past n, or crossed: no script)
    rows += extra
    col = lambda i, dt: np.array([r[i] for r in rows], dtype=dt)
    return col(0, np.uint32), col(1, np.uint64), col(2, np.uint64), found


_memo = {}


def expected(name, k, pats, ap, st, en):
    return G.cigar(text_of(name), pats, ap.tolist(), st.tolist(), en.tolist(), k, _memo.setdefault((name, k), {}))


def same(got, want, what, names=RES):
    for g, w, nm in zip(got, want, names):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, nm, np.flatnonzero(g != w)[:8] if g.shape == w.shape else (g.shape, w.shape))


def check_scripts(name, pats, ap, st, en, got):
    """every script that came back replays against its pattern and its span"""
    tb = text_of(name).tobytes()
    dist, off, cig = got
    for a in range(len(ap)):
        runs = cig[int(off[a]):int(off[a + 1])]
        if dist[a] == 0xFF:
            assert len(runs) == 0, a
        else:
            G.validate(pats[ap[a]], tb[int(st[a]):int(en[a])], runs, int(dist[a]))


def run_case(O, pkg, ctx, name, k):
    """-> (patterns, the alignments, the extensions, what cigar returned)"""
    pats, diags, _ = case(name, k)
    with index_of(O, pkg, ctx, name) as fm:
        ext = fm.extend(pats, np.arange(len(pats), dtype=np.uint32), diags, k)
        aln = alignments(name, k, ext)
        return pats, aln, ext, fm.cigar(pats, aln[0], aln[1], aln[2], k)


@pytest.mark.parametrize("name,k", CASES)
def test_cigar(O, pkg, wctx, name, k):
    pats, (ap, st, en, found), ext, got = run_case(O, pkg, wctx, name, k)
    same(got, expected(name, k, pats, ap, st, en), (name, k))
    check_scripts(name, pats, ap, st, en, got)
    # what extend found: the script costs d, and has no D at either end (s is the largest start, e the smallest end)
    dist, off, cig = got
    d = ext[0][ext[0] != 0xFF]
    assert found == len(d) and found > 10 and np.array_equal(dist[:found], d), (name, k)
    for a in range(found):
        runs = cig[int(off[a]):int(off[a + 1])]
        assert len(runs) == 0 or (runs[0] & 15 != G.OP_D and runs[-1] & 15 != G.OP_D), (name, k, a, G.cigar_string(runs))
        assert len(runs) <= 2 * int(dist[a]) + 1


def test_the_cases_are_not_vacuous(O, pkg, ctx):
    """asserted on the reference's own output for the alignments of three cases"""
    kinds = set()
    for name, k in (("ab", 8), ("dna", 16), ("GATTACA", 1)):
        n = len(text_of(name))
        pats, (ap, st, en, found), _, _ = run_case(O, pkg, ctx, name, k)
        dist, off, cig = expected(name, k, pats, ap, st, en)
        for a in range(len(ap)):
            runs = [int(r) for r in cig[int(off[a]):int(off[a + 1])]]
            s, e = int(st[a]), int(en[a])
            if dist[a] == 0xFF:
                m = len(pats[ap[a]]) if ap[a] < len(pats) else None
                kinds.add("no pattern" if m is None else "s > e" if s > e else "e > n" if e > n else "lengths" if abs(e - s - m) > k else "cost")
                continue
            kinds |= {G.LETTER[r & 15] for r in runs}
            if runs:
                kinds |= {"leading " + G.LETTER[runs[0] & 15], "trailing " + G.LETTER[runs[-1] & 15]}
            else:
                kinds.add("empty")
            if len(runs) == 2 * int(dist[a]) + 1 and dist[a] >= 2:
                kinds.add("most runs")
            if s == 0:
                kinds.add("at 0")
            if e == n:
                kinds.add("at n")
            if len(pats[ap[a]]) > n:
                kinds.add("m > n")
    want = {"no pattern", "s > e", "e > n", "lengths", "cost", "=", "X", "I", "D", "empty", "most runs", "at 0", "at n", "m > n"}
    want |= {side + op for side in ("leading ", "trailing ") for op in "=XID"}
    assert kinds == want, (kinds ^ want)


@functools.lru_cache(maxsize=None)
def reads(name):
    """reads of 40 to 300 bytes with 0 to 3 planted edits, the empty read, and one without a seed"""
    tb = text_of(name).tobytes()
    rng = np.random.default_rng(177 + TEXTS.index(name))
    alphabet = sorted(set(tb))
    out = []
    for q, m in enumerate((40, 40, 64, 100, 100, 150, 150, 200, 300, 41)):
        i = int(rng.integers(0, len(tb) - m + 1))
        out.append(planted(rng, tb[i:i + m], q % 4, alphabet, at_ends=q % 3 == 0))
    return out + [b"", bytes(rng.choice(alphabet, 7).astype(np.uint8))]


@pytest.mark.parametrize("thresholds", [False, True], ids=["phoni", "thr"])
@pytest.mark.parametrize("name", ["copies", "dna"])
def test_align_with_cigar(O, pkg, ctx, name, thresholds):
    """align(cigar=True) = align and the reference's scripts of its triples"""
    pats = reads(name)
    seen = 0
    with index_of(O, pkg, ctx, name) as fm:
        if thresholds:
            fm.add_thresholds()
        for k in (0, 2, 8):
            plain = fm.align(pats, k, 12, 3, thresholds)
            got = fm.align(pats, k, 12, 3, thresholds, cigar=True)
            assert len(plain) == 4 and len(got) == 6
            same(got[:4], plain, (name, k), ("aln_off", "start", "end", "dist"))
            ap = np.repeat(np.arange(len(pats), dtype=np.uint32), np.diff(plain[0]).astype(np.int64))
            want = expected(name, k, pats, ap, plain[1], plain[2])
            assert np.array_equal(want[0], plain[3]), (name, k)
            same(got[4:], want[1:], (name, k), RES[1:])
            seen += len(ap)
    assert seen > 20


def test_device_call_and_offsets_only(O, pkg, ctx):
    """cigar = cigar_dev; the call without d_cig gives the same dist and cig_off; what lies behind the outputs stays"""
    import torch
    name, k = "copies", 8
    pats, (ap, st, en, _), _, want = run_case(O, pkg, ctx, name, k)
    dev = torch.device("cuda", ctx.device)
    pat, off = pkg.pfp._patterns(pats)
    na, total = len(ap), int(want[1][-1])
    up = lambda a, view: torch.from_numpy(a.view(view).copy()).to(dev)
    d_pat, d_off, d_ap, d_st, d_en = up(pat, np.uint8), up(off, np.int64), up(ap, np.int32), up(st, np.int64), up(en, np.int64)
    with index_of(O, pkg, ctx, name) as fm:
        for fill in (False, True):
            d_dist = torch.full((na + 16,), 0x5A, dtype=torch.uint8, device=dev)
            d_coff = torch.full((na + 3,), -7, dtype=torch.int64, device=dev)
            d_cig = torch.full((total + 5,), -9, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            fm.cigar_dev(d_pat.data_ptr(), d_off.data_ptr(), len(pats), d_ap.data_ptr(), d_st.data_ptr(), d_en.data_ptr(), na, k,
                         d_dist.data_ptr(), d_coff.data_ptr(), d_cig.data_ptr() if fill else None)
            got = d_dist[:na].cpu().numpy(), d_coff[:na + 1].cpu().numpy().view(np.uint64)
            same(got, want[:2], ("device", fill), RES[:2])
            assert (d_dist[na:] == 0x5A).all() and (d_coff[na + 1:] == -7).all() and (d_cig[total:] == -9).all()
            if fill:
                assert np.array_equal(d_cig[:total].cpu().numpy().view(np.uint32), want[2])
            else:
                assert (d_cig == -9).all()


def test_chunks_and_batch_independence(O, pkg, wctx, monkeypatch):
    """PFP_FM_CIGAR_SCRATCH at one 300-byte alignment's records: many launches, the same results; permuted and duplicated too"""
    name, k = "dna", 8                                      # 2 cells per lane: 4 * 2 * 304 bytes for 300 rows
    pats, (ap, st, en, _), _, want = run_case(O, pkg, wctx, name, k)

    def traced(fm, *args):
        wctx.set_kernel_trace(True)
        got = fm.cigar(*args)
        trace = wctx.kernel_trace()
        wctx.set_kernel_trace(False)
        return got, sum(r["launches"] for r in trace if r["name"] == "fm_cigar")
    with index_of(O, pkg, wctx, name) as fm:
        monkeypatch.delenv("PFP_FM_CIGAR_SCRATCH", raising=False)
        got, launches = traced(fm, pats, ap, st, en, k)
        same(got, want, "one launch")
        assert launches == 1
        monkeypatch.setenv("PFP_FM_CIGAR_SCRATCH", str(4 * 2 * 304))
        got, launches = traced(fm, pats, ap, st, en, k)
        same(got, want, "chunks")
        assert launches > 1
        order = np.random.default_rng(4).permutation(len(ap))
        got = fm.cigar(pats, ap[order], st[order], en[order], k)
        assert np.array_equal(got[0], want[0][order])
        runs_of = lambda r, a: r[2][int(r[1][a]):int(r[1][a + 1])].tolist()
        assert all(runs_of(got, j) == runs_of(want, a) for j, a in enumerate(order.tolist()))
        monkeypatch.delenv("PFP_FM_CIGAR_SCRATCH")
        twice = fm.cigar(pats, np.repeat(ap, 2), np.repeat(st, 2), np.repeat(en, 2), k)
        assert np.array_equal(twice[0], np.repeat(want[0], 2)) and all(runs_of(twice, 2 * a + 1) == runs_of(want, a) for a in range(len(ap)))


def test_bad_arguments_and_no_alignments(O, pkg, ctx):
    text = text_of("GATTACA")
    usable = lambda fm: [x.tolist() for x in fm.cigar([b"GATA"], [0], [0], [4], 1)]
    with index_of(O, pkg, ctx, "GATTACA") as fm:
        assert usable(fm) == [[1], [0, 2], [3 << 4 | 7, 1 << 4 | 8]]       # GATA against GATT
        for k in (33, -1):
            with pytest.raises(pkg.PfpError) as e:
                fm.cigar([b"GAT"], [0], [0], [3], k)
            assert e.value.code == EINVAL
        with pytest.raises(pkg.PfpError) as e:
            fm.cigar([b"GAT", b"A" * 65536], [0], [0], [3], 1)
        assert e.value.code == ELIMIT
        dist, off, cig = fm.cigar([b"A" * 65535], [0], [0], [7], 32)      # (the limit itself is served)
        assert dist.tolist() == [0xFF] and off.tolist() == [0, 0] and len(cig) == 0
        dist, off, cig = fm.cigar([b"GAT"], [], [], [], 1)
        assert len(dist) == 0 and off.tolist() == [0] and len(cig) == 0 and cig.dtype == np.uint32
        dist, off, cig = fm.cigar([], [0], [0], [0], 1)
        assert dist.tolist() == [0xFF] and off.tolist() == [0, 0]
        pat = np.frombuffer(b"GATTACAGATTACA", dtype=np.uint8).copy()
        u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
        bad_off = np.array([0, 7, 3], dtype=np.uint64)
        ap, st, en = np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint64), np.full(1, 7, dtype=np.uint64)
        dist, coff, pc = np.full(1, 7, dtype=np.uint8), np.zeros(2, dtype=np.uint64), C.POINTER(C.c_uint32)()
        rc = fm.lib.pfp_fm_cigar(fm._h, pat.ctypes.data_as(C.POINTER(C.c_uint8)), u64(bad_off), C.c_uint64(2),
                                 ap.ctypes.data_as(C.POINTER(C.c_uint32)), u64(st), u64(en), C.c_uint64(1), C.c_int(1),
                                 dist.ctypes.data_as(C.POINTER(C.c_uint8)), u64(coff), C.byref(pc))
        assert rc == EINVAL and "decrease" in ctx.lib.pfp_last_error(ctx._h).decode() and dist[0] == 7 and not pc
        assert usable(fm)[0] == [1]
    bwt = O.simplebwt(text)
    with ctx.fm_index(bwt, *samples(pkg, bwt, R.full_sa(O, text))) as plain:      # an index without text
        with pytest.raises(pkg.PfpError) as e:
            plain.cigar([b"GAT"], [0], [0], [3], 1)
        assert e.value.code == EINVAL


def test_cigar_string(pkg):
    assert pkg.cigar_string([]) == "*"
    assert pkg.cigar_string(np.array([57 << 4 | 7, 1 << 4 | 8, 20 << 4 | 7, 1 << 4 | 1, 72 << 4 | 7, 3 << 4 | 2], dtype=np.uint32)) == "57=1X20=1I72=3D"
