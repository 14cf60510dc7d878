"""CPU: the numpy restatement of the fused chain's scan (tests/scan_reference.py), which tests/test_scan_chain.py holds the
HIP kernels against, checked on its own - hand-computed values, the reference's Karp-Rabin hash through the oracle and the
known-answer test of SURVEY.md section 4, and the properties the chain relies on."""
import numpy as np

import scan_reference as R

FIRST_WINDOW_KINDS = [b"CGTTAATTAC", b"GTTAGGCAGA", b"GACGGTCCAG", b"ATCTTGGTCG"]      # w = 10, p = 100


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def test_window_hash_by_hand():
    # 65 * (0xB5 + 0x6B + 0xD3 + 0x97) = 65 * 650
    assert R.window_hashes(u8(b"AAAA"), 4).tolist() == [42250]
    # 65 * 181 + 67 * 107 + 71 * 211 + 84 * 151 = 11765 + 7169 + 14981 + 12684
    assert R.window_hashes(u8(b"ACGT"), 4).tolist() == [46599]
    # two windows of a five-byte text: entry j ends at position j + w - 1; the second is 67 * 181 + 71 * 107 + 84 * 211 + 65 * 151
    assert R.window_hashes(u8(b"ACGTA"), 4).tolist() == [46599, 12127 + 7597 + 17724 + 9815]
    # the widest window of the register path, all bytes 255: 255 * (sum of the first 17 multipliers)
    assert R.window_hashes(u8(b"\xff" * 17), 17).tolist() == [255 * int(R.FAST_MUL[:17].sum())] == [686205]
    # the trigger value: (h + seed) * 0x9E3779B1 mod 2^32
    assert int(R.trigger_values(np.uint64(42250), 0)) == (42250 * 0x9E3779B1) % (1 << 32) == 4019836394
    assert int(R.trigger_values(np.uint64(42250), 5)) == (42255 * 0x9E3779B1) % (1 << 32) == 112146015
    assert R.window_hashes(u8(b"ACG"), 4).size == 0


def test_thresholds():
    assert R.thresholds(100) == (89478485, 42949672, 1)          # 2^32 / 48 and 2^32 / 100: the candidate is p / 48
    assert R.thresholds(200) == (89478485, 21474836, 1)
    assert R.thresholds(1000) == (34359738, 4294967, 1)          # the candidate stops at 8
    assert R.thresholds(11) == (390451572, 390451572, 0)         # p <= 48: nothing denser than nominal to choose
    assert R.thresholds(100, 2.0) == (85899345, 85899345, 0) and R.thresholds(100, 0.5) == (21474836, 21474836, 0)
    assert R.thresholds(100, 1.3)[0] == 55834574
    assert R.thresholds(10, 64.0)[0] == 0xFFFFFFFF               # saturated


def test_karp_rabin_restatement(O, synth):
    assert R.kr_window_hashes(u8(b"GATT"), 4).tolist() == [1195463764] == [synth.kr_window_hash(b"GATT")]
    assert int(R.kr_window_hashes(u8(b"CCGA"), 4)[0]) % 11 == 6
    rng = np.random.default_rng(3)
    rnd = rng.integers(3, 256, size=30000, dtype=np.uint8)
    dna = O.gen_fasta(20000, 2, 0.001, 21)
    for text in (rnd, dna):
        for w, p in [(4, 11), (7, 10), (10, 100), (13, 64), (17, 37), (25, 33)]:
            assert np.array_equal(R.kr_cuts(text, w, p), O.scan(text, w, p)), (w, p)
    cut = dna.copy()
    cut[7777] = 2
    assert np.array_equal(R.kr_cuts(cut, 10, 100), O.scan(cut, 10, 100)) and R.usable_len(cut) == 7777
    # extra triggers: every window with one of the given hashes ends a phrase too
    h = R.kr_window_hashes(dna, 10)
    with_extra = R.kr_cuts(dna, 10, 100, extras=[int(h[500])])
    assert 509 in with_extra.tolist() and set(R.kr_cuts(dna, 10, 100).tolist()) <= set(with_extra.tolist())


def test_nominal_cuts_are_a_subset_of_dense_cuts(O):
    text = O.gen_fasta(50000, 2, 0.001, 7)
    for w in (4, 10, 17):
        for p in (100, 200):
            fthr, fnom, fauto = R.thresholds(p)
            assert fauto == 1 and fnom < fthr
            dense, nominal = R.fast_cuts(text, w, 3, fthr), R.fast_cuts(text, w, 3, fnom)
            assert 0 < len(nominal) < len(dense) and np.isin(nominal, dense).all()
            assert 0.7 * len(text) / p < len(nominal) < 1.3 * len(text) / p          # (the trigger's density is 1 / p)
            assert dense.min() >= w - 1 and dense.max() <= len(text) - 1


def test_seed_contract_on_the_four_first_window_kinds():
    """w = 10, p = 100: the reference's hash cuts the first window or not, seed 0 would cut it or not - the contract picks out
    one seed for each, rejects the seeds before it, and seed 0 is right only where nothing has to move"""
    fthr, fnom, _ = R.thresholds(100)
    kinds = set()
    for fw in FIRST_WINDOW_KINDS:
        ref = int(R.kr_window_hashes(u8(fw), 10)[0]) % 100 == 0
        zero = int(R.trigger_values(R.window_hashes(u8(fw), 10), 0)[0]) < fthr
        kinds.add((ref, zero))
        seed = 0
        while R.seed_contract_violations(fw, 10, 100, seed, fthr, fnom):
            seed += 1
        assert seed < 1000
        x = int(R.trigger_values(R.window_hashes(u8(fw), 10), seed)[0])
        assert (x < fnom) if ref else (x >= fthr)
        assert (seed == 0) == (not ref and not zero)
        later = seed + 1          # a later seed that satisfies clauses 1 and 2 is still refused: it is not the smallest
        while any("smallest" not in v for v in R.seed_contract_violations(fw, 10, 100, later, fthr, fnom)):
            later += 1
        assert any("smallest" in v for v in R.seed_contract_violations(fw, 10, 100, later, fthr, fnom))
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}


def test_seed_contract_knows_the_letter_runs():
    """runs of C at w = 7 would be cut into crumbs by seed 0 (p = 100): the contract refuses seed 0 for any text that does
    not begin with that run, and exempts the run that IS the first window and that the reference cuts"""
    fthr, fnom, _ = R.thresholds(100)
    assert any("run of 'C'" in v for v in R.seed_contract_violations(b"GATTACA", 7, 100, 0, fthr, fnom))
    assert any("run of 'C'" in v for v in R.seed_contract_violations(None, 7, 100, 0, fthr, fnom))


def test_density_rule():
    # the four inequalities, each the one that decides
    assert R.density_rule(3284, 370, 284, 100)[0]
    assert not R.density_rule(1000, 370, 284, 100)[0]          # sample too small
    assert not R.density_rule(2817, 55, 11, 100)[0]            # too few loci
    assert not R.density_rule(3000, 2000, 1600, 100)[0]        # more than half the contexts single: not a collection
    assert not R.density_rule(3000, 1100, 100, 100)[0]         # variants too light: 100 * 100 < 64 * 1000
    # byte-wise contexts: three cuts, two with equal contexts
    rng = np.random.default_rng(1)
    block = rng.integers(65, 91, size=200, dtype=np.uint8)
    text = np.concatenate([block, block, rng.integers(65, 91, size=200, dtype=np.uint8)])
    h = R.window_hashes(text, 10)
    ends = np.array([150, 350, 550])
    x = R.trigger_values(h[ends - 9], 0)
    got = R.density_choice(text, 10, 100, 0, (int(x.max()) + 1) * 16, ends)
    assert (got["sampled"], got["distinct"], got["singles"], got["dense"]) == (3, 2, 1, False)
    assert R.density_choice(text, 10, 100, 0, (int(x.max()) + 1) * 16, ends, min_end=200)["sampled"] == 2
    assert R.max_phrase_len(np.array([20, 50]), 100, 10) == 100 + 10 - (50 + 2 - 10) + 1
