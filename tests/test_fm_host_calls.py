"""The calls of FmIndex over host patterns (csrc/api_fm.hip) on the inputs of fm_host_cases.py: what a call returns does not
depend on how PFP_FM_SEQ_BUDGET cuts it into groups of patterns - 1: every pattern alone, 7: some groups, the repeated segment
alone - and equals what the *_dev methods, which never group, give for the same patterns on device arrays.  Mapping reads and
pairs run on the reads and the index their entry in fm_host_cases.CALLS names, under that entry's budgets."""
import numpy as np
import pytest

import fm_host_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm_of(O, pkg, ctx):
    """index name -> that index with thresholds, built when first asked for"""
    made = {}

    def get(index):
        if index not in made:
            made[index] = H.index_of(O, pkg, ctx, thresholds=True, index=index)
        return made[index]

    yield get
    for f in made.values():
        f.close()


@pytest.fixture(scope="module")
def fm(fm_of):
    return fm_of("text")


_plain = {}


def plain(fm, name):
    """the call without a budget, once (fm: the index the call's entry names)"""
    if name not in _plain:
        with H.Env({}):
            _plain[name] = H.CALLS[name].run(fm, list(H.INPUTS[H.CALLS[name].index]()))
    return _plain[name]


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, i, g.shape, w.shape)


def test_the_inputs_make_groups():
    """asserted on the inputs alone: a pattern with more hits than either budget, patterns without any, about 30 of them"""
    text, seg = H.text_and_segment()
    P = H.patterns()
    assert len(P) == 30 and b"" in P and b"A" in P and seg in P and all(len(p) <= 40 for p in P)
    assert sum(12 <= len(p) <= 40 for p in P) == 28
    assert text.tobytes().count(seg) == H.SEG_COPIES > 7 and len(H.seq_starts()) == H.NPARTS + 1
    assert sum(text.tobytes().count(p) == 0 for p in P if p) >= 5


def test_the_calls_name_their_offsets():
    """the fourteen calls of the first consolidation: offsets first (for ms the patterns' own), none from count and extend"""
    first, none = "locate approx approx_locate ms ms_thr mems mems_thr align align_thr locate_seqs doclist".split(), "count count_toehold extend".split()
    assert all(H.CALLS[n].offsets == (0,) for n in first) and all(H.CALLS[n].offsets == () for n in none)
    assert sorted(list(H.CALLS)[:14]) == sorted(first + none)


def test_the_cap_cuts(fm):
    """align_cap's max_aln = 2 is below what several patterns have: the capped call keeps the first two of each, in order"""
    with H.Env({}):
        off, start, end, dist = H.CALLS["align_cap"].run(fm, list(H.patterns()))
        uoff, ustart, uend, udist = fm.align(list(H.patterns()), H.K_CAP, H.CAP_SEED)
    per, uper = np.diff(off).astype(np.int64), np.diff(uoff).astype(np.int64)
    assert (uper > 2).sum() >= 2 and np.array_equal(per, np.minimum(uper, 2))
    keep = np.concatenate([np.arange(int(uoff[p]), int(uoff[p]) + int(per[p])) for p in range(len(per))]).astype(np.int64)
    same([start, end, dist], [ustart[keep], uend[keep], udist[keep]], "align_cap")


@pytest.mark.parametrize("name,budget", [(n, b) for b in H.BUDGETS + ("40", "9") for n in H.CALLS if b in H.CALLS[n].budgets])
def test_groups_do_not_change_the_answer(fm_of, name, budget):
    call = H.CALLS[name]
    f = fm_of(call.index)
    want = plain(f, name)
    with H.Env({"PFP_FM_SEQ_BUDGET": budget}):
        same(call.run(f, list(H.INPUTS[call.index]())), want, (name, budget))


@pytest.mark.parametrize("name", list(H.CALLS))
def test_no_patterns(fm_of, name):
    """offsets [0] in the arrays the call's entry names as offsets, and every other array empty"""
    call = H.CALLS[name]
    with H.Env({}):
        out = [np.asarray(a) for a in call.run(fm_of(call.index), [])]
    for i in call.offsets:
        assert out[i].tolist() == [0], (name, i)
    rest = [a for i, a in enumerate(out) if i not in call.offsets]
    assert rest and all(a.size == 0 for a in rest), (name, out)


# ---------------------------------------------------------------- the same from the *_dev methods
class Dev:
    """the patterns on the device, and device arrays that come back as numpy arrays of the library's types"""

    def __init__(self, pkg, ctx):
        import torch
        self.torch, self.dev = torch, torch.device("cuda", ctx.device)
        pat, off = pkg.pfp._patterns(list(H.patterns()))
        self.npat, self.bytes = len(off) - 1, int(off[-1])
        self.pat = torch.from_numpy(pat.copy()).to(self.dev)
        self.off = self.put(off)

    def put(self, a):
        a = np.ascontiguousarray(a)
        t = self.torch.from_numpy(a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]).copy()).to(self.dev)
        self.torch.cuda.synchronize()
        return t

    def new(self, n, dtype):
        t = self.torch.zeros(int(n) + 16, dtype={np.uint64: self.torch.int64, np.uint32: self.torch.int32, np.uint8: self.torch.uint8}[dtype],
                             device=self.dev)
        self.torch.cuda.synchronize()
        return t

    @staticmethod
    def get(t, n, dtype):
        return t[:int(n)].cpu().numpy().view(dtype)


@pytest.fixture(scope="module")
def dev(pkg, ctx):
    return Dev(pkg, ctx)


@pytest.fixture(scope="module")
def ranges(fm, dev):
    """count_dev: (sp, ep, first) on the device"""
    r = [dev.new(dev.npat, np.uint64) for _ in range(3)]
    fm.count_dev(dev.pat.data_ptr(), dev.off.data_ptr(), dev.npat, *(t.data_ptr() for t in r))
    return r


def test_count_from_device_calls(fm, dev, ranges):
    got = [dev.get(t, dev.npat, np.uint64) for t in ranges]
    same(got, plain(fm, "count_toehold"), "count_toehold")
    same(got[:2], plain(fm, "count"), "count")


def two_pass(dev, call, npat, outs):
    """call(d_off, *d_outs or Nones): offsets only, then with room for offsets[npat] of every output (dtype, per entry)"""
    d_off = dev.new(npat + 1, np.uint64)
    call(d_off.data_ptr(), *(None for _ in outs))
    off = dev.get(d_off, npat + 1, np.uint64)
    total = int(off[-1])
    d_outs = [dev.new(total * per, dt) for dt, per in outs]
    call(d_off.data_ptr(), *(t.data_ptr() for t in d_outs))
    return [dev.get(d_off, npat + 1, np.uint64)] + [dev.get(t, total * per, dt) for t, (dt, per) in zip(d_outs, outs)]


def test_locate_from_device_calls(fm, dev, ranges):
    sp, ep, first = (t.data_ptr() for t in ranges)
    off, pos = two_pass(dev, lambda o, p: fm.locate_dev(dev.npat, sp, ep, first, 0, o, p), dev.npat, [(np.uint64, 1)])
    same([off, pos] + [dev.get(t, dev.npat, np.uint64) for t in ranges[:2]], plain(fm, "locate"), "locate")


def test_approx_from_device_calls(fm, dev):
    pat, poff, k = dev.pat.data_ptr(), dev.off.data_ptr(), H.K_MISMATCH
    d_off = dev.new(dev.npat + 1, np.uint64)
    fm.approx_dev(pat, poff, dev.npat, k, d_off.data_ptr())
    hits = int(dev.get(d_off, dev.npat + 1, np.uint64)[-1])
    d_sp, d_ep, d_first, d_dist = (dev.new(hits, dt) for dt in (np.uint64, np.uint64, np.uint64, np.uint8))
    fm.approx_dev(pat, poff, dev.npat, k, d_off.data_ptr(), d_sp.data_ptr(), d_ep.data_ptr(), d_dist.data_ptr(), d_first.data_ptr())
    off, dist = dev.get(d_off, dev.npat + 1, np.uint64), dev.get(d_dist, hits, np.uint8)
    same([off] + [dev.get(t, hits, np.uint64) for t in (d_sp, d_ep)] + [dist, dev.get(d_first, hits, np.uint64)], plain(fm, "approx"), "approx")
    # approx_locate: the rows of every hit, hit by hit (locate_dev over the hits), each with its hit's mismatches
    hoff, hpos = two_pass(dev, lambda o, p: fm.locate_dev(hits, d_sp.data_ptr(), d_ep.data_ptr(), d_first.data_ptr(), 0, o, p), hits,
                          [(np.uint64, 1)])
    same([hoff[off.astype(np.int64)], hpos, np.repeat(dist, np.diff(hoff).astype(np.int64))], plain(fm, "approx_locate"), "approx_locate")


@pytest.mark.parametrize("thresholds", [False, True], ids=["phoni", "thr"])
def test_ms_and_mems_from_device_calls(fm, dev, thresholds):
    tag = "_thr" if thresholds else ""
    d_len, d_pos = dev.new(dev.bytes + 1, np.uint32), dev.new(dev.bytes + 1, np.uint64)
    fm.matching_statistics_dev(dev.pat.data_ptr(), dev.off.data_ptr(), dev.npat, d_len.data_ptr(), d_pos.data_ptr(), thresholds=thresholds)
    same([dev.get(dev.off, dev.npat + 1, np.uint64), dev.get(d_len, dev.bytes, np.uint32), dev.get(d_pos, dev.bytes, np.uint64)],
         plain(fm, "ms" + tag), "ms" + tag)
    off, mem = two_pass(dev, lambda o, m: fm.mems_dev(dev.off.data_ptr(), dev.npat, d_len.data_ptr(), d_pos.data_ptr(), H.MIN_MEM, o, m),
                        dev.npat, [(np.uint64, 3)])
    same([off, mem.reshape(-1, 3)], plain(fm, "mems" + tag), "mems" + tag)


def test_extend_from_device_calls(fm, dev):
    cp, cd = H.candidates()
    nc = len(cp)
    d_cp, d_cd = dev.put(cp), dev.put(cd)
    d_dist, d_start, d_end = dev.new(nc, np.uint8), dev.new(nc, np.uint64), dev.new(nc, np.uint64)
    fm.extend_dev(dev.pat.data_ptr(), dev.off.data_ptr(), dev.npat, d_cp.data_ptr(), d_cd.data_ptr(), nc, H.K_EDIT, d_dist.data_ptr(),
                  d_start.data_ptr(), d_end.data_ptr())
    same([dev.get(d_dist, nc, np.uint8), dev.get(d_start, nc, np.uint64), dev.get(d_end, nc, np.uint64)], plain(fm, "extend"), "extend")


@pytest.mark.parametrize("thresholds", [False, True], ids=["phoni", "thr"])
def test_align_from_device_calls(fm, dev, thresholds):
    got = two_pass(dev, lambda o, s, e, d: fm.align_dev(dev.pat.data_ptr(), dev.off.data_ptr(), dev.npat, H.K_EDIT, H.MIN_SEED, o, s, e, d,
                                                        thresholds=thresholds),
                   dev.npat, [(np.uint64, 1), (np.uint64, 1), (np.uint8, 1)])
    same(got, plain(fm, "align_thr" if thresholds else "align"), ("align", thresholds))


def test_sequence_calls_from_device_calls(fm, dev, ranges):
    sp, ep, first = (t.data_ptr() for t in ranges)
    rng = [dev.get(t, dev.npat, np.uint64) for t in ranges[:2]]
    # (locate_seqs_dev wants room for what locate_dev's offsets-only call reports: every row of every pattern here)
    rows = int((rng[1] - rng[0]).sum())
    d_off, d_seq, d_o = dev.new(dev.npat + 1, np.uint64), dev.new(rows, np.uint32), dev.new(rows, np.uint64)
    fm.locate_seqs_dev(dev.off.data_ptr(), dev.npat, sp, ep, first, 0, d_off.data_ptr(), d_seq.data_ptr(), d_o.data_ptr())
    off = dev.get(d_off, dev.npat + 1, np.uint64)
    kept = int(off[-1])
    same([off, dev.get(d_seq, kept, np.uint32), dev.get(d_o, kept, np.uint64)] + rng, plain(fm, "locate_seqs"), "locate_seqs")
    got = two_pass(dev, lambda o, d, c: fm.doclist_dev(dev.off.data_ptr(), dev.npat, sp, ep, first, o, d, c), dev.npat,
                   [(np.uint32, 1), (np.uint64, 1)])
    same(got, plain(fm, "doclist"), "doclist")
