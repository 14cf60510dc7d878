"""The whole words' chars written by inverted-list entry (word_chars_kernel) and the unit edges found from one ballot
(unit_edges_kernel), on inputs chosen for the seams of the two kernels: a whole-word run longer than an expand workgroup's
quota, units wider than a wave and than a workgroup, and output slices / slot ranges that cut through both.  Every case
runs BWT only, with the full SA and with the sampled SA files, in both index widths, against the CPU oracle."""
import numpy as np
import pytest

import merge_cases as mc

pytestmark = pytest.mark.gpu

EXPAND_QUOTA = 65536          # kExpandQuota (csrc/merge.hip)
WAVE, WORKGROUP = 64, 256     # lanes of unit_edges_kernel

# name -> (text(O), w, p)
INPUTS = {
    "long_word_run": (lambda O: np.frombuffer(b"ACGTTGCAAGCTTAGGCATCGA" * 70000, dtype=np.uint8).copy(), 4, 11),
    "units300": (lambda O: O.gen_fasta(3000, 300, 0.01, 7), 10, 100),
    "units130": (lambda O: O.gen_fasta(3000, 130, 0.01, 7), 10, 100),
}
_texts, _wants, _runs = {}, {}, {}


def text_of(O, name):
    if name not in _texts:
        _texts[name] = INPUTS[name][0](O)
    return _texts[name]


def want_of(O, name, flags):
    """the oracle's outputs, computed once per (input, flags)"""
    if (name, flags) not in _wants:
        _, w, p = INPUTS[name]
        _wants[name, flags] = O.bigbwt(text_of(O, name), w, p, flags)
    return _wants[name, flags]


def run_of(pkg, O, ctx, name, flags, width):
    """one traced call of the fused chain per (input, flags, width): its outputs and the names of the rows it opened"""
    key = (name, flags, width)
    if key not in _runs:
        _, w, p = INPUTS[name]
        ctx.set_index_bits(64 if width == 64 else 0)
        ctx.set_kernel_trace(True)
        try:
            got = ctx.bigbwt(text_of(O, name), w, p, flags)
            rows = {r["name"] for r in ctx.kernel_trace()}
        finally:
            ctx.set_kernel_trace(False)
            ctx.set_index_bits(0)
        _runs[key] = (got, rows)
    return _runs[key]


def check_outputs(pkg, got, want, flags):
    assert np.array_equal(got["bwt"], want["bwt"])
    if flags & pkg.FLAG_SA:
        assert np.array_equal(pkg.unpack5(got["sa"]), want["sa"])
    if flags & pkg.FLAG_SSA:
        assert np.array_equal(pkg.unpack5(got["ssa"]).reshape(-1, 2), want["ssa"])
    if flags & pkg.FLAG_ESA:
        assert np.array_equal(pkg.unpack5(got["esa"]).reshape(-1, 2), want["esa"])


def largest_units(O, name):
    """(largest group of words that share one suffix longer than w and agree on the char before it, largest such group
    whose members disagree), from the oracle's dictionary: the proper suffixes of every word, terminator included"""
    _, w, p = INPUTS[name]
    dict_ = O.parse(text_of(O, name), w, p)["dict"].tobytes()
    groups = {}
    start = 0
    for end in (i for i, b in enumerate(dict_) if b == 1):          # words end in 0x01 (EndOfWord)
        for i in range(start + 1, end - w):                          # proper suffixes longer than w
            groups.setdefault(dict_[i:end + 1], []).append(dict_[i - 1])
        start = end + 1
    same = max((len(v) for v in groups.values() if len(set(v)) == 1), default=0)
    mixed = max((len(v) for v in groups.values() if len(set(v)) > 1), default=0)
    return same, mixed


@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", mc.FLAG_SETS)
def test_whole_word_run_longer_than_the_expand_quota(O, pkg, ctx, flags, width):
    """four words, one of them with 70 000 occurrences: its whole-word run is longer than the 65 536 bytes an expand
    workgroup writes itself, so the zeros under it come from expand_kernel and expand_heavy_kernel both"""
    _, w, p = INPUTS["long_word_run"]
    occ = O.parse(text_of(O, "long_word_run"), w, p)["occ"]
    print("words", len(occ), "max occ", int(occ.max()))
    assert int(occ.max()) > EXPAND_QUOTA
    got, _ = run_of(pkg, O, ctx, "long_word_run", flags, width)
    check_outputs(pkg, got, want_of(O, "long_word_run", flags), flags)


@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", mc.FLAG_SETS)
def test_whole_word_chars_have_a_row_of_their_own(O, pkg, ctx, flags, width):
    """the witness: word_chars_kernel ran, whatever the outputs asked for"""
    _, rows = run_of(pkg, O, ctx, "long_word_run", flags, width)
    assert "pfp::word_chars_kernel" in rows and "pfp::expand_kernel" in rows


@pytest.fixture(scope="module")
def unit_sizes(O):
    return {name: largest_units(O, name) for name in ("units300", "units130")}


@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", mc.FLAG_SETS)
@pytest.mark.parametrize("name", ["units300", "units130"])
def test_units_wider_than_a_wave_and_a_workgroup(O, pkg, ctx, unit_sizes, name, flags, width):
    """300 copies: a unit of more than 256 slots - both extension loops run and the unit crosses a workgroup; 130 copies: wider
    than a wave, narrower than a workgroup"""
    same, mixed = unit_sizes[name]
    print(name, "largest unit with one char", same, "with mixed chars", mixed)
    if name == "units300":
        assert same > WORKGROUP and mixed > WORKGROUP
    else:
        assert WAVE < same <= WORKGROUP and WAVE < mixed <= WORKGROUP
    got, _ = run_of(pkg, O, ctx, name, flags, width)
    check_outputs(pkg, got, want_of(O, name, flags), flags)


def _pieces(res, key):
    off, parts = 0, []
    for r in res:
        assert r[key + "_off"] == off, (key, r[key + "_off"], off)
        parts.append(r[key].cpu().numpy())
        off += r[key].numel()
    return np.concatenate(parts)


@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", mc.FLAG_SETS)
@pytest.mark.parametrize("case", list(mc.DIST_CASES))
def test_slices_and_slot_ranges(O, pkg, case, flags, width):
    """the 300 copies through two virtual ranks, the suffix array replicated (every rank emits a slice of the output: whole-word
    runs and units are cut by out_lo / out_hi) or sharded by key range (words whose slot another rank holds)"""
    import importlib

    import torch
    d = importlib.import_module("bigbwt_amd.dist")
    name = "units300"
    _, w, p = INPUTS[name]
    text = text_of(O, name)
    want = want_of(O, name, flags)
    n = len(text)
    cuts = [0, n // 2 - 2, n]
    ctxs = [pkg.Context(0) for _ in range(2)]
    try:
        for c in ctxs:
            c.set_index_bits(64 if width == 64 else 0)
        shards = [torch.from_numpy(text[cuts[r]:cuts[r + 1]].copy()).cuda() for r in range(2)]
        res = d.simulate(ctxs, shards, w, p, flags, halo=8192, shard_sa=mc.DIST_CASES[case])
        assert res[0]["lo"] == 0 and res[0]["hi"] == res[1]["lo"] and res[1]["hi"] == n + 1
        assert np.array_equal(torch.cat([r["bwt"] for r in res]).cpu().numpy(), want["bwt"])
        if flags & pkg.FLAG_SA:
            assert np.array_equal(pkg.unpack5(_pieces(res, "sa5")), want["sa"])
        if flags & pkg.FLAG_SSA:
            assert np.array_equal(pkg.unpack5(_pieces(res, "ssa")).reshape(-1, 2), want["ssa"])
        if flags & pkg.FLAG_ESA:
            assert np.array_equal(pkg.unpack5(_pieces(res, "esa")).reshape(-1, 2), want["esa"])
    finally:
        for c in ctxs:
            c.close()
