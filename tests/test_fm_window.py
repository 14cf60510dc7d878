"""Aligning in a window on the GPU (csrc/fmwindow.hip): FmIndex.window / window_dev.

Definitions (include/pfpgpu.h, "Aligning in a window"): a candidate (p, lo, hi) gives (d*, s, e) with d* the least
Levenshtein(P, T[s..e)) over lo <= s <= e <= hi, e the smallest end that attains it and s the largest start for that e, or (0xFF,
UINT64_MAX, UINT64_MAX) where d* > k or the window is not one of the text.  Every expected value comes from window_reference.py
(checked against a brute force, literals and extend_reference in test_window_reference.py) and every array is compared exactly, in
both index widths.

The kernel takes a window in tiles of 256 columns (64 where no window of the call has more than 63 bytes) that hand their last
column on, so the sweeps below - every width 0..2200 with the pattern at the window's right end, and every offset of a window of
3000 bytes - put an alignment's end, its start and its whole span on and across every seam (columns 256, 512, ...: at least eight
lie inside); the tile is below 2000 columns, so the sweeps are as wide as the issue sets them."""
import functools

import numpy as np
import pytest

import approx_reference as R
import extend_reference as E
import map_cases as K
import window_reference as W

pytestmark = pytest.mark.gpu

EINVAL, ELIMIT = -1, -5
NOPOS = 2**64 - 1


def samples(pkg, bwt, sa):
    """.ssa / .esa bytes from the BWT and SA[0..n]: <j, SA[j]> of the run starts / ends"""
    b = np.asarray(bwt)
    starts = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1]]))
    ends = np.flatnonzero(np.concatenate([b[1:] != b[:-1], [True]]))
    pk = lambda rows: pkg.pack5(np.stack([rows, sa[rows]], axis=1).reshape(-1).astype(np.uint64))
    return pk(starts), pk(ends)


_parts = {}


def index_of(O, pkg, ctx, name):
    """an index with text over one of the texts (the BWT and the samples are computed once)"""
    if name not in _parts:
        text = K.text_of(name)
        bwt = O.simplebwt(text)
        _parts[name] = (bwt,) + samples(pkg, bwt, R.full_sa(O, text))
    bwt, ssa, esa = _parts[name]
    return ctx.fm_index_ms(bwt, ssa, esa, K.text_of(name))


class Case:
    """patterns and candidates, collected one by one"""

    def __init__(self, name, k):
        self.name, self.k, self.pats, self.cp, self.lo, self.hi = name, k, [], [], [], []

    def add(self, pat, *windows):
        for lo, hi in windows:
            self.cp.append(len(self.pats))
            self.lo.append(lo)
            self.hi.append(hi)
        self.pats.append(bytes(pat))

    def arrays(self):
        return np.array(self.cp, dtype=np.uint32), np.array(self.lo, dtype=np.uint64), np.array(self.hi, dtype=np.uint64)


def width_sweep():
    """m = 20, k = 2: one candidate per width 0..2200, the pattern planted with 0..2 edits so that it ends with the window; every
    seventh width once more with the pattern at the window's left end"""
    tb = K.text_of("dna").tobytes()
    rng = np.random.default_rng(31)
    c = Case("dna", 2)
    lo = 5003
    for w in range(2201):
        c.add(E.planted(rng, tb[lo + w - 20:lo + w], w % 3, b"ACGT", at_ends=w % 2 == 0), (lo, lo + w))
        if w % 7 == 0:
            c.add(E.planted(rng, tb[lo:lo + 20], w % 3, b"ACGT", at_ends=w % 2 == 1), (lo, lo + w))
    return c


def position_sweep():
    """one window of 3000 bytes, m = 20, k = 2: one candidate per offset of the planted pattern"""
    tb = K.text_of("dna").tobytes()
    rng = np.random.default_rng(32)
    c = Case("dna", 2)
    lo = 4001
    for at in range(0, 3000 - 20 + 1):
        c.add(E.planted(rng, tb[lo + at:lo + at + 20], at % 3, b"ACGT", at_ends=at % 2 == 0), (lo, lo + 3000))
    return c


def seams():
    """m = 40, k = 3 around the first three seams of a window of 1000 bytes: an alignment crosses a seam at every one of its rows,
    the 16th and the 32nd included (the kernel looks at a tile's dead rows every 16 rows), with 0..4 edits before and after it"""
    tb = K.text_of("dna").tobytes()
    rng = np.random.default_rng(33)
    c = Case("dna", 3)
    lo = 9002
    for at in range(200, 780):
        c.add(E.planted(rng, tb[lo + at:lo + at + 40], at % 5, b"ACGT", at_ends=at % 2 == 0), (lo, lo + 1000))
    return c


def shapes(k):
    """m in {1, 15, 16, 17, 150} x window width in {m - k - 1, m - k, m, m + 2k, 600}: the pattern planted in the window with up to
    k edits, with k + 1 edits, and a random string"""
    tb = K.text_of("dna").tobytes()
    rng = np.random.default_rng(40 + k)
    c = Case("dna", k)
    for m in (1, 15, 16, 17, 150):
        for w in (m - k - 1, m - k, m, m + 2 * k, 600):
            w = max(w, 0)
            lo = int(rng.integers(1000, 15000))
            at = lo + max(w - m, 0) // 2
            for edits in sorted({0, min(k, 1), min(k, 3), k, k + 1}):
                c.add(E.planted(rng, tb[at:at + m], edits, b"ACGT", at_ends=edits % 2 == 0), (lo, lo + w))
            c.add(bytes(rng.choice(list(b"ACGT"), m).astype(np.uint8)), (lo, lo + w))
    return c


def density(k):
    """a^3000 b a^2000 with patterns a^m: every end and every start ties"""
    c = Case("ab", k)
    for m in (1, 15, 16, 17, 150, 300):
        c.add(b"a" * m, (0, 0), (7, 7 + max(m - 1, 0)), (7, 7 + m), (100, 700), (0, 3000), (2900, 3100), (3000, 3001), (3001, 5001),
              (3001 - m // 2, 3001 + m), (5001 - m, 5001))
        c.add(b"a" * (m // 2) + b"b" + b"a" * (m - m // 2), (0, 3000), (2000, 3400), (3001, 5001))
    return c


def clipping():
    """windows that end at n, start at 0, are empty at either end, and patterns that hang over either end"""
    tb = K.text_of("dna").tobytes()
    n = len(tb)
    c = Case("dna", 3)
    c.add(tb[-20:], (n - 300, n), (n - 20, n), (n - 19, n), (n, n), (n - 5000, n - 1), (n - 700, n - 1))
    c.add(tb[-18:] + b"GT", (n - 300, n), (n - 18, n))
    c.add(tb[:20], (0, 300), (0, 20), (1, 300), (0, 0), (0, 19))
    c.add(b"AC" + tb[:18], (0, 300), (0, 17))
    c.add(b"", (0, 0), (n, n), (5, 900))
    c.add(tb[9000:9040], (0, W.MAX_W), (n - W.MAX_W, n))
    return c


CASES = {"width sweep": width_sweep, "position sweep": position_sweep, "seams": seams, "clipping": clipping}
CASES.update({"shapes k=%d" % k: functools.partial(shapes, k) for k in (0, 1, 8, 32)})
CASES.update({"density k=%d" % k: functools.partial(density, k) for k in (0, 2)})


@functools.lru_cache(maxsize=None)
def case(which):
    return CASES[which]()


@functools.lru_cache(maxsize=None)
def expected(which):
    """the reference's (dist, start, end) of a case, computed once and shared"""
    c = case(which)
    return W.window(K.text_of(c.name), c.pats, c.cp, c.lo, c.hi, c.k)


def same(got, want, what, names=("dist", "start", "end")):
    for g, w, nm in zip(got, want, names):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, nm, np.flatnonzero(g != w)[:8] if g.shape == w.shape else (g.shape, w.shape))


@pytest.mark.parametrize("which", sorted(CASES))
def test_window(O, pkg, wctx, which):
    c = case(which)
    with index_of(O, pkg, wctx, c.name) as fm:
        same(fm.window(c.pats, *c.arrays(), c.k), expected(which), which)


def test_the_cases_are_not_vacuous():
    """asserted on the reference's own output: the reference alone must satisfy these"""
    c = case("width sweep")
    dist, start, end = expected("width sweep")
    cp, lo, hi = c.arrays()
    assert np.all(dist[hi - lo >= 22] <= 2) and set(dist.tolist()) == {0, 1, 2, 0xFF}
    for seam in range(256, 2200, 256):                      # an end at one of the columns seam - 1, seam, seam + 1 of every seam
        cols = (end[dist <= 2] - lo[dist <= 2]).tolist()
        assert len({seam - 1, seam, seam + 1} & set(cols)) >= 1, seam
    c = case("position sweep")
    dist, start, end = expected("position sweep")
    assert np.all(dist <= 2) and set(dist.tolist()) == {0, 1, 2}
    cols_s, cols_e = (start - np.uint64(4001)).tolist(), (end - np.uint64(4001)).tolist()
    for seam in range(256, 3000, 256):
        assert len({seam - 1, seam, seam + 1} & set(cols_e)) >= 1 and len({seam - 1, seam, seam + 1} & set(cols_s)) >= 1, seam
        assert any(s < seam - 5 and e > seam + 5 for s, e in zip(cols_s, cols_e)), seam
    kinds = set()
    for which in sorted(CASES):
        if not which.startswith(("shapes", "density", "clipping")):
            continue
        c = case(which)
        dist, start, end = expected(which)
        for i in range(len(dist)):
            m, d = len(c.pats[c.cp[i]]), int(dist[i])
            if d == 0xFF:
                kinds.add("none")
                continue
            span = int(end[i]) - int(start[i])
            kinds.add("exact" if d == 0 else "d = k" if d == c.k else "edits")
            kinds.add("shorter" if span < m else "longer" if span > m else "same")
            kinds |= {"empty span"} if span == 0 and m else set()
            kinds |= {"ends at n"} if int(end[i]) == 20000 and c.name == "dna" else set()
            kinds |= {"starts at 0"} if int(start[i]) == 0 and m else set()
            kinds |= {"k = 32"} if c.k == 32 and d > 8 else set()
            kinds |= {"widest"} if c.hi[i] - c.lo[i] == W.MAX_W else set()
    assert kinds == {"none", "exact", "d = k", "edits", "shorter", "longer", "same", "empty span", "ends at n", "starts at 0", "k = 32", "widest"}, kinds


def test_invalid_candidates_and_no_candidates(O, pkg, ctx):
    n = 20000
    tb = K.text_of("dna").tobytes()
    with index_of(O, pkg, ctx, "dna") as fm:
        pats = [tb[100:120], b""]
        cp = [0, 2, 2**32 - 1, 0, 0, 0, 1, 1, 1, 0]
        lo = [90, 90, 90, 131, n - 5, NOPOS, 7, 8, n + 1, 0]
        hi = [130, 130, 130, 130, n + 1, NOPOS, 7, 7, n + 1, 2**63]
        dist, start, end = fm.window(pats, cp, lo, hi, 1)
        assert dist.tolist() == [0, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0, 0xFF, 0xFF, 0xFF]
        assert start.tolist() == [100] + [NOPOS] * 5 + [7] + [NOPOS] * 3 and end.tolist() == [120] + [NOPOS] * 5 + [7] + [NOPOS] * 3
        same((dist, start, end), W.window(K.text_of("dna"), pats, [p if p < 2 else -1 for p in cp], lo, hi, 1), "invalid")
        dist, start, end = fm.window(pats, [], [], [], 1)
        assert len(dist) == len(start) == len(end) == 0 and dist.dtype == np.uint8 and start.dtype == np.uint64
        assert fm.window([], [0], [0], [10], 1)[0].tolist() == [0xFF]
        with pytest.raises(ValueError):
            fm.window(pats, [0, 0], [0], [10], 1)


def test_limits_and_bad_arguments(O, pkg, ctx):
    text = K.text_of("dna")
    tb = text.tobytes()
    usable = lambda fm: [x.tolist() for x in fm.window([tb[300:330]], [0], [0], [1000], 1)] == [[0], [300], [330]]
    assert pkg.pfp.FM_WINDOW_MAX_W == W.MAX_W == 16384
    with index_of(O, pkg, ctx, "dna") as fm:
        with pytest.raises(pkg.PfpError) as e:
            fm.window([tb[300:330]], [0, 0], [0, 100], [1000, 100 + W.MAX_W + 1], 1)
        assert e.value.code == ELIMIT and "PFP_FM_WINDOW_MAX_W" in str(e.value)
        assert fm.window([tb[300:330]], [0], [100], [100 + W.MAX_W], 1)[1].tolist() == [300]       # (the limit itself is served)
        for k in (33, -1):
            with pytest.raises(pkg.PfpError) as e:
                fm.window([tb[300:330]], [0], [0], [1000], k)
            assert e.value.code == EINVAL
        with pytest.raises(pkg.PfpError) as e:
            fm.window([b"GAT", b"A" * 65536], [0], [0], [10], 1)
        assert e.value.code == ELIMIT
        assert fm.window([b"A" * 65535], [0], [0], [W.MAX_W], 32)[0].tolist() == [0xFF]    # (the longest pattern fits no window)
        assert usable(fm)
    bwt = O.simplebwt(text)
    with ctx.fm_index(bwt, *samples(pkg, bwt, R.full_sa(O, text))) as plain:      # an index without text
        with pytest.raises(pkg.PfpError) as e:
            plain.window([b"GAT"], [0], [0], [10], 1)
        assert e.value.code == EINVAL


@pytest.mark.parametrize("name,k", [("dna", 0), ("dna", 2), ("copies", 8), ("ab", 8), ("dna", 32)])
def test_agrees_with_extend(O, pkg, wctx, name, k):
    """200 random diagonals: window on extend's own window equals FmIndex.extend"""
    tb = K.text_of(name).tobytes()
    n = len(tb)
    rng = np.random.default_rng(50 + k)
    pats, cd = [], []
    for q in range(200):
        m = int(rng.choice([1, 16, 40, 150]))
        i = int(rng.integers(0, n - m + 1))
        pats.append(E.planted(rng, tb[i:i + m], int(rng.integers(0, k + 2)), sorted(set(tb)), at_ends=q % 2 == 0))
        cd.append(int(rng.choice([i, i - k, i + k, i + k + 1, -3, n - m // 2])))
    win = [E.window(n, len(p), d, k) for p, d in zip(pats, cd)]
    cp = np.arange(200, dtype=np.uint32)
    with index_of(O, pkg, wctx, name) as fm:
        want = fm.extend(pats, cp, cd, k)
        same(fm.window(pats, cp, [w[0] for w in win], [w[1] for w in win], k), want, (name, k))
    assert 20 < np.count_nonzero(want[0] != 0xFF) < 200


def test_bounded_launches_and_order(O, pkg, wctx, monkeypatch):
    """PFP_FM_WINDOW_CELLS=4000 cuts the call into many pieces (most candidates of the sweep exceed it and go alone); a shuffled
    candidate list gives the shuffled results"""
    monkeypatch.delenv("PFP_FM_WINDOW_CELLS", raising=False)
    c = case("shapes k=8")
    cp, lo, hi = c.arrays()
    want = expected("shapes k=8")
    order = np.random.default_rng(6).permutation(len(cp))
    with index_of(O, pkg, wctx, "dna") as fm:
        same(fm.window(c.pats, cp[order], lo[order], hi[order], 8), [w[order] for w in want], "shuffled")
        back = np.arange(len(c.pats))[::-1]
        same(fm.window([c.pats[i] for i in back], (len(c.pats) - 1 - cp).astype(np.uint32), lo, hi, 8), want, "patterns reversed")
        monkeypatch.setenv("PFP_FM_WINDOW_CELLS", "4000")
        wctx.set_kernel_trace(True)
        got = fm.window(c.pats, cp, lo, hi, 8)
        trace = wctx.kernel_trace()
        wctx.set_kernel_trace(False)
        same(got, want, "pieces")
        assert sum(r["launches"] for r in trace if r["name"] == "fm_window") > 10
        same(fm.window(c.pats, cp[order], lo[order], hi[order], 8), [w[order] for w in want], "pieces, shuffled")
        ws = case("width sweep")
        monkeypatch.setenv("PFP_FM_WINDOW_CELLS", "400000")
        same(fm.window(ws.pats, *ws.arrays(), 2), expected("width sweep"), "pieces of the sweep")


def test_device_call(O, pkg, ctx):
    """torch tensors in, torch tensors out; what lies behind the outputs stays"""
    import torch
    c = case("shapes k=8")
    cp, lo, hi = c.arrays()
    dev = torch.device("cuda", ctx.device)
    pat, off = pkg.pfp._patterns(c.pats)
    nc = len(cp)
    up = lambda a, view: torch.from_numpy(a.view(view).copy()).to(dev)
    d_pat, d_off, d_cp, d_lo, d_hi = up(pat, np.uint8), up(off, np.int64), up(cp, np.int32), up(lo, np.int64), up(hi, np.int64)
    d_dist = torch.full((nc + 16,), 0x5A, dtype=torch.uint8, device=dev)
    d_start, d_end = (torch.full((nc + 2,), -7, dtype=torch.int64, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    with index_of(O, pkg, ctx, "dna") as fm:
        fm.window_dev(d_pat.data_ptr(), d_off.data_ptr(), len(c.pats), d_cp.data_ptr(), d_lo.data_ptr(), d_hi.data_ptr(), nc, 8,
                      d_dist.data_ptr(), d_start.data_ptr(), d_end.data_ptr())
    got = d_dist[:nc].cpu().numpy(), d_start[:nc].cpu().numpy().view(np.uint64), d_end[:nc].cpu().numpy().view(np.uint64)
    same(got, expected("shapes k=8"), "device")
    assert (d_dist[nc:] == 0x5A).all() and (d_start[nc:] == -7).all() and (d_end[nc:] == -7).all()
