"""CPU: tests/formats_reference.py against the oracle, so that the GPU tests of the output formats compare with a reference that is
not trusted on its own; slices of any cut list add up to the whole; and the inputs of tests/formats_cases.py hold the runs that
tests/README.md says they hold."""
import numpy as np
import pytest

import formats_cases as FC
import formats_reference as FR
from textgen import make_text


def small_golden(golden):
    return [c for c in golden if c["n"] <= 100000]


_files = {}


def _oracle_files(name, O, golden):
    """(bwt, SA of every BWT position, the oracle's -s -e result) of a golden text"""
    if name not in _files:
        c = {x["name"]: x for x in golden}[name]
        text = make_text(c["spec"], O)
        sampled = O.bigbwt(text, c["w"], c["p"], O.FLAG_SSA | O.FLAG_ESA)
        full = O.bigbwt(text, c["w"], c["p"], O.FLAG_SA)
        bwt = sampled["bwt"]
        assert np.array_equal(bwt, full["bwt"]) and len(full["sa"]) == len(bwt) - 1
        sa = np.concatenate([[len(bwt) - 1], full["sa"]]).astype(np.uint64)          # SA[0] = n is not in .sa
        _files[name] = (bwt, sa, sampled)
    return _files[name]


def test_whole_bwt_equals_the_oracle_on_the_golden_texts(golden, O):
    """run_pairs over the whole BWT with -1 / -1 = the oracle's .ssa / .esa, pack5 = the oracle's, on every golden text up to 100 KB"""
    seen = 0
    for c in small_golden(golden):
        bwt, sa, want = _oracle_files(c["name"], O, golden)
        for run_end, key in ((False, "ssa"), (True, "esa")):
            got = FR.run_pairs(bwt, sa, 0, len(bwt), -1, -1, run_end, 0)
            assert np.array_equal(got, O.pack5(want[key].reshape(-1))), (c["name"], key)
            assert FR.count_pairs(bwt, 0, len(bwt), -1, -1, run_end) == len(want[key])
        assert np.array_equal(FR.pack5(sa[1:]), O.pack5(sa[1:]))
        sampled = np.zeros(len(bwt), dtype=bool)
        sampled[want["ssa"][:, 0].astype(np.int64)] = True
        sampled[want["esa"][:, 0].astype(np.int64)] = True
        assert np.array_equal(FR.boundary_mask(bwt), sampled) and sampled[0] and sampled[-1]
        seen += 1
    assert seen >= 10


def test_pack5_by_hand(O):
    v = np.array([0, 1, 0x0102030405, (1 << 40) - 1, 1 << 40, 0xFFEEDDCCBBAA9988, (1 << 32) - 1, 1 << 32], dtype=np.uint64)
    want = bytes.fromhex("0000000000" "0100000000" "0504030201" "ffffffffff" "0000000000" "8899aabbcc" "ffffffff00" "0000000001")
    assert FR.pack5(v).tobytes() == want
    assert np.array_equal(FR.pack5(v), O.pack5(v)) and np.array_equal(FR.unpack5(FR.pack5(v)), v & np.uint64(FR.MASK40))
    assert FR.pack5([]).shape == (0,)
    for count in (1, 17, 4097):
        for kind in ("low", "high", "ones"):
            x = FC.pack_values(count, kind)
            assert np.array_equal(FR.pack5(x), O.pack5(x))


def test_run_pairs_by_hand():
    bwt = np.frombuffer(b"AABCCCA", dtype=np.uint8)
    sa = np.arange(100, 107, dtype=np.uint64)
    pairs = lambda *a: FR.unpack5(FR.run_pairs(bwt, sa, *a)).reshape(-1, 2).tolist()
    assert pairs(0, 7, -1, -1, False, 0) == [[0, 100], [2, 102], [3, 103], [6, 106]]
    assert pairs(0, 7, -1, -1, True, 0) == [[1, 101], [2, 102], [5, 105], [6, 106]]
    assert pairs(1, 5, ord("A"), ord("C"), False, 1) == [[2, 102], [3, 103]]
    assert pairs(1, 5, ord("A"), ord("C"), True, 1) == [[1, 101], [2, 102]]
    assert pairs(1, 5, ord("B"), ord("A"), False, 50) == [[50, 101], [51, 102], [52, 103]]
    assert pairs(1, 5, -1, -1, True, 50) == [[50, 101], [51, 102], [53, 104]]
    assert pairs(4, 5, ord("C"), ord("C"), False, 4) == [] and pairs(4, 5, ord("C"), ord("C"), True, 4) == []
    assert pairs(4, 5, -1, ord("C"), False, 4) == [[4, 104]] and pairs(4, 5, ord("C"), -1, True, 4) == [[4, 104]]
    assert pairs(3, 3, ord("B"), ord("C"), False, 3) == []
    assert pairs(0, 7, -1, -1, False, (1 << 40) - 7)[-1] == [(1 << 40) - 1, 106]
    assert FR.boundary_mask(bwt).tolist() == [True, True, True, True, False, True, True]


def _random_cuts(rng, n, k):
    cuts = sorted(int(x) for x in rng.integers(0, n + 1, size=k))
    return [0] + cuts + [n]          # (equal neighbours among them: empty slices)


def test_slices_add_up_to_the_whole(golden, O):
    """for any cut list, the slices' run_pairs under their true neighbours and pos_base = lo, back to back, are the whole's"""
    rng = np.random.default_rng(3)
    inputs = [(FC.array(name), FC.sa_values(name)) for name in FC.ARRAYS]
    inputs += [_oracle_files(name, O, golden)[:2] for name in ("kat1", "repeat_w6", "gen_small")]
    for bwt, sa in inputs:
        n = len(bwt)
        lists = [_random_cuts(rng, n, k) for k in (1, 2, 5, 40, 40)] + [list(range(n + 1)), [0, 0, n, n]]
        if n > 13000:
            lists.append([0] + [c for c in (1, 16, 17, 4096, 4097, 8192) if c < n] + [n])
        for run_end in (False, True):
            whole = FR.run_pairs(bwt, sa, 0, n, -1, -1, run_end, 0)
            for cuts in lists[: 5 if n > 20000 else None]:
                parts = FR.sliced_pairs(bwt, sa, cuts, run_end)
                assert np.array_equal(np.concatenate(parts), whole)
    for name in FC.SLICED:
        bwt, sa = FC.array(name), FC.sa_values(name)
        for run_end in (False, True):
            assert np.array_equal(np.concatenate(FR.sliced_pairs(bwt, sa, FC.cut_list(name), run_end)), FR.run_pairs(bwt, sa, 0, len(bwt), -1, -1, run_end, 0))


# ---------------------------------------------------------------------------------------- the inputs hold what they claim
def _runs(a):
    s = FC.run_starts(a)
    return s, np.diff(np.append(s, len(a)))


def test_arrays_hold_the_runs_they_claim():
    s, ln = _runs(FC.array("constant"))
    assert s.tolist() == [0] and ln[0] > 3 * FC.TILE
    a = FC.array("alternating")
    s, ln = _runs(a)
    assert len(s) == len(a) > 3 * FC.TILE and set(ln.tolist()) == {1}          # every position starts and ends a run: 4096 pairs a tile
    assert FR.count_pairs(a, 0, FC.TILE, -1, -1, True) == FC.TILE
    s, ln = _runs(FC.array("random_runs"))
    assert set(ln.tolist()) == set(range(1, 41)) and len(ln) == 800
    s, ln = _runs(FC.array("edges"))
    ends = set((s + ln - 1).tolist())
    assert set(FC.EDGE_POINTS) <= set(s.tolist()) and set(FC.EDGE_POINTS) <= ends          # a run begins, and a run ends, at each
    assert len(FC.array("edges")) > 2 * FC.TILE + FC.CHUNK
    a = FC.array("extremes").astype(np.int64)
    steps = set(zip(a[:-1].tolist(), a[1:].tolist()))
    assert {(0, 255), (255, 0), (0, 1), (254, 255), (255, 254), (1, 0)} <= steps
    for name in FC.ARRAYS:
        assert 1000 < len(FC.array(name)) < 100000
        # chunk and tile edges: boundaries on both sides of a multiple of 16 and of 4096 (but in the constant array, which has none)
        if name != "constant":
            m = FR.boundary_mask(FC.array(name))
            at = np.flatnonzero(m)
            assert (at % FC.CHUNK == 0).any() and (at % FC.CHUNK == FC.CHUNK - 1).any()
            if name in ("alternating", "edges"):
                assert (at % FC.TILE == 0)[1:].any() and (at % FC.TILE == FC.TILE - 1).any()


def test_sa_values_hold_the_special_values_at_boundaries():
    for name in FC.ARRAYS:
        a, v = FC.array(name), FC.sa_values(name)
        assert len(v) == len(a) and len(set(v.tolist())) >= len(v) - 8 and int(v.max()) <= FR.MASK40
        # the constant array has two boundaries, its ends: one special value in either file
        want = set(FC.SPECIAL_SA) if name != "constant" else {0, (1 << 32) - 1}
        assert want <= set(v[FR.boundary_mask(a)].tolist())
        if name != "constant":
            for run_end in (False, True):
                sampled = FR.unpack5(FR.run_pairs(a, v, 0, len(a), -1, -1, run_end, 0)).reshape(-1, 2)[:, 1]
                assert {(1 << 32) - 1, 1 << 32} & set(sampled.tolist()) and {0, (1 << 40) - 1} & set(sampled.tolist()), (name, run_end)
    assert FC.pos_base("top", 100) + 100 == 1 << 40 and FC.pos_base("small", 1) == 12345 and FC.pos_base("zero", 1) == 0


def test_cut_lists_cut_where_they_claim():
    lengths = None
    for name in FC.SLICED:
        cuts = FC.cut_list(name)
        lengths = [b - a for a, b in zip(cuts[:-1], cuts[1:])]
        assert lengths[: len(FC.SLICE_LENGTHS)] == list(FC.SLICE_LENGTHS) and cuts[-1] == len(FC.array(name))
        assert {1, 2, 15, 16, 17, 31, 33, 4095, 4096, 4097, 0} <= set(lengths)
        assert any(c % 2 == 1 for c in cuts) and any(c % 2 == 0 for c in cuts)
    a = FC.array("random_runs")
    cuts = FC.cut_list("random_runs")
    starts = set(FC.run_starts(a).tolist())
    tail = cuts[len(FC.SLICE_LENGTHS) + 1: -1]
    s = tail[1]
    assert tail[:3] == (s - 1, s, s + 1) and s in starts and s - 1 not in starts and s + 1 not in starts          # one before, on, one after
    mid = tail[3]
    assert all(x not in starts for x in range(mid - 2, mid + 4)) and tail[4] == mid + 1          # strictly inside a run: a slice of one position in it
    big, sa, lo, hi = FC.embedded("edges")
    assert lo % 2 == 1 and np.array_equal(big[lo:hi], FC.array("edges")) and np.array_equal(sa[lo:hi], FC.sa_values("edges"))
    assert lo > 300 and len(big) - hi > 300


def test_pack_cases_hold_what_they_claim():
    counts = FC.PACK_COUNTS
    assert {5 * c % 16 for c in counts if c <= 17} == set(range(16))          # every length of the last, partial 16-byte chunk (0: none)
    assert {(16 * q) % 5 for q in range(5)} == set(range(5))                    # ... and a count of 17 has chunks at every b0 mod 5
    assert {819, 820} <= set(counts) and 819 * 5 < 4096 <= 820 * 5              # one workgroup writes 4096 output bytes
    assert {255, 256, 257, 4095, 4096, 4097, 65537} <= set(counts)
    for kind in ("low", "high"):
        v = FC.pack_values(17, kind)
        assert (v & np.uint64(FR.MASK40) == 0).any() and (v & np.uint64(FR.MASK40) == FR.MASK40).any()
        assert ((v >> np.uint64(40)) != 0).all() == (kind == "high")
    assert np.array_equal(FC.pack_values(17, "high") & np.uint64(FR.MASK40), FC.pack_values(17, "low"))
    assert (FC.pack_values(5, "ones") == np.uint64(0xFFFFFFFFFFFFFFFF)).all()


@pytest.mark.parametrize("R", [4, 6])
def test_distributed_case_cuts_inside_its_long_run(O, R):
    """the text of the distributed test: the BWT has one run longer than two ranks' slices; with the equal slices of the replicated
    sort at least one cut falls strictly inside it and at least one rank's slice lies wholly inside it - that rank has no pair in
    either file"""
    import importlib
    import __graft_entry__ as entry
    entry.load_package()
    d = importlib.import_module("bigbwt_amd.dist")
    c = FC.dist_case(O, R)
    text = c["text"]
    assert len(text) < 100000 and len(c["cuts"]) == R + 1
    run_lo, run_hi = 3000, 3000 + FC.RUN          # the text's run holds no shard boundary: a shard inside it would hold no phrase end
    assert all(x <= run_lo or x >= run_hi for x in c["cuts"]) and len(set(text[run_lo:run_hi].tolist())) == 1
    bwt = O.bigbwt(text, c["w"], c["p"], 0)["bwt"]
    a, b = FC.longest_run(bwt)
    bounds = [d.slice_bounds(len(bwt), r, R) for r in range(R)]
    assert b - a > 2 * max(hi - lo for lo, hi in bounds)
    assert any(a < lo < b for lo, _ in bounds[1:])
    inside = [r for r, (lo, hi) in enumerate(bounds) if a < lo and hi < b]
    assert inside
    for r in inside:
        lo, hi = bounds[r]
        left, right = FR.true_neighbours(bwt, lo, hi)
        assert FR.count_pairs(bwt, lo, hi, left, right, False) == 0 and FR.count_pairs(bwt, lo, hi, left, right, True) == 0
