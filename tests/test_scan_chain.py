"""GPU: stage 1a as the fused chain runs it (csrc/scan.hip: kr_scan_kernel<W, FAST = true> with its own window hash, the choice of
the phrase length, the Karp-Rabin fall-back, the giant-phrase splitter) and as a rank under a parse plan runs it, through
pfp_debug_scan_chain, against the numpy restatement of tests/scan_reference.py; and the exact Karp-Rabin scan (pfp_scan) against
the oracle at every window width, at the moduli that take another branch of make_kr_params, at the text lengths around a
16-byte chunk, a 4096-position chunk and a 64 KB tile, and with bytes <= 2.  Every comparison is exact: these are integers.
tests/README.md, "Tests of the scan, path by path", lists which case reaches which path."""
import contextlib

import numpy as np
import pytest

import scan_reference as R
from scan_reference import zero_hash_window

pytestmark = pytest.mark.gpu

WIDTHS = list(range(4, 18))


@contextlib.contextmanager
def settings(ctx, fast=True, density=0.0, max_phrase=0):
    try:
        ctx.set_window_hash(fast)
        ctx.set_parse_density(density)
        ctx.set_max_phrase(max_phrase)
        yield ctx
    finally:
        ctx.set_window_hash(True)
        ctx.set_parse_density(0.0)
        ctx.set_max_phrase(1 << 15)


@pytest.fixture(scope="module")
def rnd():
    """200 000 random bytes 3..255 with runs of 255 and of 3: three 64 KB tiles and a bit (look-back, tile seams)"""
    rng = np.random.default_rng(5)
    t = rng.integers(3, 256, size=200000, dtype=np.uint8)
    t[1000:1100] = 255
    t[5000:5100] = 3
    t[65530:65545] = 255          # across the first tile seam
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def dna(O):
    t = O.gen_fasta(66000, 3, 0.001, 21)[:200000].copy()
    assert len(t) == 200000
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def coll(O):
    """the 4.9 MB collection of test_phrase_length_follows_repetitiveness: 40 copies at 2 per mille"""
    t = O.gen_fasta(120000, 40, 0.002, 31)
    t.setflags(write=False)
    return t


def check_chain_scan(O, ctx, text, w, p, density=0.0, hashes=None, full_choice=False):
    """one run of the chain's scan under the context's settings (window hash on, `density` set by the caller) held against the
    reference: parameters, seed contract, the dense pass and its nominal flags, the fall-back, the final ends.  Returns the
    report."""
    text = np.asarray(text, dtype=np.uint8)
    rep = ctx.debug_scan_chain(text, w, p)
    n_used = R.usable_len(text)
    assert rep["n_used"] == n_used
    prefix = text[:n_used]
    fthr, fnom, fauto = R.thresholds(p, density)
    assert (rep["fthr_first"], rep["fthr_nom"], rep["fauto"]) == (fthr, fnom, fauto), (w, p, density)
    seed = rep["fseed"]
    assert R.seed_contract_violations(bytes(text[:w]) if len(text) >= w else None, w, p, seed, fthr, fnom) == [], (w, p, density, seed)
    h = hashes if hashes is not None else R.window_hashes(prefix, w)
    x = R.trigger_values(h, seed)
    dense = R._cuts(x < np.uint64(fthr), w)
    nominal = R._cuts(x < np.uint64(fnom), w)
    final, final_thr, want_density = dense, fthr, (density if density > 0 else 1.0)
    if fauto and len(dense):
        assert rep["chose"] == 1 and rep["dense_cuts"] == len(dense)
        assert np.array_equal(rep["dense_ends"], dense), (w, p)
        assert np.array_equal(rep["dense_ends"][rep["nominal"] != 0], nominal), (w, p)
        assert rep["n_nominal"] == len(nominal)
        assert rep["kept"] == rep["sampled"]          # no sample list overflowed
        if full_choice:
            ch = R.density_choice(prefix, w, p, seed, fnom, dense)
            assert (rep["sampled"], rep["distinct"], rep["singles"], rep["dense"]) == (ch["sampled"], ch["distinct"], ch["singles"], int(ch["dense"]))
        else:
            sampled = int((x < np.uint64(fnom // R.SAMPLE_SHIFT)).sum())
            assert rep["sampled"] == sampled
            assert sampled >= 1024 or rep["dense"] == 0
        if not rep["dense"]:
            final, final_thr = nominal, fnom
        else:
            want_density = float(np.float32(float(R.auto_density(p))))          # (pfp_stats keeps the density as a float)
    else:
        assert rep["chose"] == 0 and rep["dense_ends"] is None
    if len(final) == 0:          # the window hash cuts nowhere: the reference's own hash decides
        assert rep["kr_fallback"] == 1 and rep["fast"] == 0
        final, want_density = O.scan(prefix, w, p), 1.0
        assert np.array_equal(final, R.kr_cuts(prefix, w, p))
    else:
        assert rep["kr_fallback"] == 0 and rep["fast"] == 1 and rep["fthr"] == final_thr
    assert rep["n_ends"] == len(final) and np.array_equal(rep["ends"], final), (w, p, density, len(text))
    assert rep["parse_density"] == want_density
    assert rep["n_extra"] == 0
    return rep


# ---------------------------------------------------------------- every width, every tile position

@pytest.mark.parametrize("w", WIDTHS)
def test_window_hash_scan_every_width(O, ctx, rnd, dna, w):
    """kr_scan_kernel<w, true> for every instantiated width: 16 positions per lane cover every place of a window in its 32-byte
    register tile, three tiles the look-back; p = 11 (one threshold), 100 and 200 (dense candidate 100 / 48 and 200 / 48, the
    nominal flags of classify_ends_kernel against the same hash), pinned densities 1, 2 and 0.5"""
    for text in (rnd, dna):
        h = R.window_hashes(text, w)
        for p in (11, 100, 200):
            for density in (0.0, 1.0, 2.0, 0.5):
                with settings(ctx, density=density):
                    rep = check_chain_scan(O, ctx, text, w, p, density, hashes=h)
                assert rep["n_ends"] > 0.4 * len(text) / p * (density if density else 1.0)


# ---------------------------------------------------------------- lengths

LENGTHS = sorted({15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 65535, 65536, 65537, 131073})


@pytest.mark.parametrize("w", [4, 10, 17])
def test_window_hash_scan_lengths(O, ctx, rnd, dna, w):
    """text lengths around a 16-byte lane chunk, a 4096-position chunk and a 64 KB tile (the clipping masks of kr_mask16, the
    `interior` shortcut, the padded last tile); texts the window hash does not cut take the Karp-Rabin fall-back and get the
    reference's cuts, or none"""
    fell_back = none_at_all = 0
    for n in sorted(set(LENGTHS) | {w - 1, w, w + 1}):
        for text in (rnd[:n], dna[1000:1000 + n]):
            for p, density in ((11, 0.0), (100, 0.0), (100, 2.0)):
                with settings(ctx, density=density):
                    rep = check_chain_scan(O, ctx, text, w, p, density)
                fell_back += rep["kr_fallback"]
                none_at_all += rep["n_ends"] == 0
    assert fell_back >= 3 and none_at_all >= 3          # (n < w never cuts)


def test_window_hash_scan_many_tiles(O, ctx, coll):
    """4.9 MB: 75 tiles, more than the 64 one look-back step covers - whether a second step happens is a matter of timing, the
    ends must be right either way"""
    assert len(coll) > 64 * 65536
    with settings(ctx, density=1.0):
        rep = check_chain_scan(O, ctx, coll, 10, 100, 1.0)
    assert rep["n_ends"] > 40000


# ---------------------------------------------------------------- first window

def test_first_window_decides_like_the_reference(O, ctx, dna):
    """the text's first window must be cut exactly when the reference's hash cuts it, at either density; one text
    for each of: the reference silent / firing, seed 0 silent / firing (w = 10, p = 100)"""
    kinds = set()
    fthr, fnom, _ = R.thresholds(100)
    for head in (b"CGTTAATTAC", b"GTTAGGCAGA", b"GACGGTCCAG", b"ATCTTGGTCG"):
        fw = np.frombuffer(head, dtype=np.uint8)
        ref = int(R.kr_window_hashes(fw, 10)[0]) % 100 == 0
        zero = int(R.trigger_values(R.window_hashes(fw, 10), 0)[0]) < fthr
        kinds.add((ref, zero))
        text = np.concatenate([fw, dna[2000:42000]])
        for density in (0.0, 1.0, 2.0):
            with settings(ctx, density=density):
                rep = check_chain_scan(O, ctx, text, 10, 100, density)
            assert (9 in rep["ends"][:1].tolist()) == ref, (head, density)
            if density == 0.0:
                assert (9 in rep["dense_ends"][:1].tolist()) == ref
                assert (rep["fseed"] == 0) == (not ref and not zero)
    assert kinds == {(False, False), (False, True), (True, False), (True, True)}


# ---------------------------------------------------------------- letter runs

RUNS = [("C", 7, 100), ("C", 7, 200), ("c", 9, 100), ("c", 9, 200), ("t", 17, 100), ("t", 17, 200), ("A", 13, 32), ("T", 14, 32), ("G", 15, 32)]


@pytest.mark.parametrize("letter,w,p", RUNS)
def test_letter_runs_are_not_cut_into_crumbs(O, ctx, dna, letter, w, p):
    """runs of one DNA letter that seed 0 would cut at every position: the seed moves, the 50 KB run stays whole"""
    fthr, _, _ = R.thresholds(p)
    run = np.full(50000, ord(letter), dtype=np.uint8)
    assert int(R.trigger_values(R.window_hashes(run[:w], w), 0)[0]) < fthr          # (seed 0 would fire: that is the case)
    text = np.concatenate([dna[:30000], run, dna[30000:60000]])
    with settings(ctx):
        rep = check_chain_scan(O, ctx, text, w, p)
    assert rep["fseed"] != 0 and rep["kr_fallback"] == 0
    for ends in (rep["ends"], rep["dense_ends"]):
        if ends is not None:
            assert not ((ends >= 30000 + w - 1) & (ends < 80000)).any()


def test_a_run_that_is_the_first_window_may_be_cut(O, ctx, dna):
    """the exemption: where the text BEGINS with a run of one letter and the reference cuts that first window, the window hash
    has to cut it too - and with it every window of the run"""
    found = None
    for p in range(49, 400):
        for w in WIDTHS:
            for ch in R.DNA_LETTERS:
                if found is None and int(R.kr_window_hashes(np.full(w, ch, dtype=np.uint8), w)[0]) % p == 0:
                    found = (ch, w, p)
    assert found is not None
    ch, w, p = found
    text = np.concatenate([np.full(2000, ch, dtype=np.uint8), dna[:40000]])
    with settings(ctx):
        rep = check_chain_scan(O, ctx, text, w, p)
    assert np.array_equal(rep["ends"][:2000 - w + 1], np.arange(w - 1, 2000, dtype=np.uint64))


# ---------------------------------------------------------------- bytes <= 2

SPECIAL_OFFSETS = [0, 15, 16, 4095, 4096, 65535, 65536, 69999]


def special_byte_texts(base):
    """(text, position of the first byte <= 2): one such byte at the edges of a lane chunk, a 4096-position chunk, a tile and the
    text; two of them (the first wins); neighbours that borrow in the four-bytes-at-once test of bad_bytes4"""
    n = len(base)
    assert n == 70000
    k = 0
    for off in SPECIAL_OFFSETS:
        for val in (0, 1, 2):
            t = base.copy()
            t[off] = val
            yield t, off
        k += 1
    for first, second in ((4097, 4098), (100, 65536), (65535, 65536), (16, 31), (5000, 69999)):
        t = base.copy()
        t[first], t[second] = 2, 0
        yield t, first
    for nb in (3, 0x80, 0x81, 0x82, 0x83, 0xFF):
        for off in (1001, 1002, 4096, 65538):          # every place in a dword
            t = base.copy()
            t[off - 3:off + 4] = nb
            t[off] = k % 3
            k += 1
            yield t, off
        t = base.copy()          # the neighbours alone stop nothing
        t[1000:1008] = nb
        yield t, n


def test_window_hash_scan_stops_at_special_bytes(O, ctx, rnd, dna):
    """newscan.cpp:364 in the fused path: n_used is the position of the first byte <= 2, the ends are those of the prefix"""
    for base, w, p in ((rnd[:70000], 10, 11), (dna[:70000], 10, 100), (rnd[60000:130000], 17, 100), (dna[10000:80000], 4, 11)):
        for text, first in special_byte_texts(base):
            with settings(ctx):
                rep = check_chain_scan(O, ctx, text, w, p)
            assert rep["n_used"] == first


# ---------------------------------------------------------------- the density choice

def repeat_family_genome():
    """a single genome with repeat families: 2.4 MB of unique sequence, and 100 elements of 2 KB present four times each -
    loci in plenty, yet most sampled contexts are single"""
    rng = np.random.default_rng(77)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    fam = lut[rng.integers(0, 4, size=(100, 2000))]
    parts = []
    for k in range(400):
        parts.append(lut[rng.integers(0, 4, size=6000)])
        parts.append(fam[(k * 37) % 100])
    return np.concatenate(parts)


DENSITY_CASES = {
    "collection": (lambda O, coll: coll, True),
    "few_light_variants": (lambda O, coll: O.gen_fasta(60000, 64, 0.0001, 5), False),
    "small_sample": (lambda O, coll: O.gen_fasta(30000, 40, 0.002, 31), False),
    "single_genome": (lambda O, coll: O.gen_fasta(800000, 1, 0.0, 32), False),
    "repeat_families": (lambda O, coll: repeat_family_genome(), False),
}


@pytest.mark.parametrize("case", list(DENSITY_CASES))
def test_density_choice(O, ctx, coll, case):
    """classify_ends_kernel, the sort of the context hashes, count_distinct_kernel, sample_says_dense and keep_nominal_cuts
    against the rule restated on the contexts' BYTES, on inputs for which the reference decides by a factor of 1.25 or more"""
    make, want_dense = DENSITY_CASES[case]
    text = make(O, coll)
    with settings(ctx):
        rep = check_chain_scan(O, ctx, text, 10, 100, full_choice=True)
    dense, ratios = R.density_rule(rep["sampled"], rep["distinct"], rep["singles"], 100)
    print(case, len(text), rep["sampled"], rep["distinct"], rep["singles"], ratios)
    # the input's margin, in the reference's own figures (check_chain_scan has shown them equal to the kernels')
    if want_dense:
        assert min(ratios.values()) >= 1.25, ratios
    else:
        assert min(ratios.values()) <= 1 / 1.25, ratios
    assert dense == want_dense and rep["dense"] == int(want_dense)
    assert rep["parse_density"] == (float(np.float32(100 / 48)) if want_dense else 1.0)
    if case == "repeat_families":          # that input is there for ONE clause: the others hold
        assert ratios["collection"] <= 0.8 and ratios["sample"] >= 1.25 and ratios["loci"] >= 1.25
    if case == "single_genome":
        assert rep["singles"] == rep["distinct"] == rep["sampled"]


# ---------------------------------------------------------------- extra triggers

def extra_texts(O):
    rng = np.random.default_rng(9)
    unit = np.frombuffer(b"ACGGTCA", dtype=np.uint8)
    plain = O.gen_fasta(100000, 2, 0.001, 13)
    return {
        "n_block": (O.gen_fasta(100000, 2, 0.001, 11, n_blocks=[(30000, 20000)]), 40),
        "period7": (np.concatenate([plain[:60000], np.tile(unit, 3000), plain[60000:120000]]), 40),
        "neither": (plain, 40),
        "long_phrases": (plain, 200),          # phrases of 200 bytes on average: some exceed 700 by chance, and are split
    }


@pytest.mark.parametrize("fast", [True, False], ids=["window_hash", "karp_rabin"])
@pytest.mark.parametrize("max_phrase", [700, 3000])
def test_extra_triggers(O, ctx, max_phrase, fast):
    """giant_phrases_kernel, window_hash_kernel and propose_extra_triggers: whatever extra hashes the chain adds, they are
    hashes of windows of the text, never the first window's, at most 32, and the ends are the plain cuts plus every window
    with one of these hashes"""
    for name, (text, p) in extra_texts(O).items():
        w = 10
        with settings(ctx, fast=fast, max_phrase=max_phrase):
            rep = ctx.debug_scan_chain(text, w, p)
        assert rep["n_used"] == len(text) and rep["kr_fallback"] == 0 and rep["fast"] == int(fast)
        extras = rep["extra"]
        assert len(extras) == rep["n_extra"] <= 32 and len(set(extras)) == len(extras)
        if fast:
            # (automatic density: these texts are too small for a sample of 1024, the chain drops to the nominal threshold
            #  BEFORE it looks for giant phrases, and rescans with it)
            fthr, fnom, fauto = R.thresholds(p)
            assert (rep["fthr_first"], rep["fthr_nom"], rep["fauto"]) == (fthr, fnom, fauto)
            assert rep["chose"] == fauto and rep["dense"] == 0 and rep["sampled"] < 1024 and rep["fthr"] == fnom
            assert R.seed_contract_violations(bytes(text[:w]), w, p, rep["fseed"], fthr, fnom) == []
            hs = (R.window_hashes(text, w) + np.uint64(rep["fseed"])) & np.uint64(R.M32)
            plain_cuts = R.fast_cuts(text, w, rep["fseed"], fnom)
            want = R.fast_cuts(text, w, rep["fseed"], fnom, extras)
        else:
            hs = R.kr_window_hashes(text, w)
            plain_cuts = O.scan(text, w, p)
            want = R.kr_cuts(text, w, p, extras)
        assert np.isin(np.array(extras, dtype=np.uint64), hs).all(), name
        assert int(hs[0]) not in extras, name
        assert np.array_equal(rep["ends"], want), (name, max_phrase, fast)
        longest = R.max_phrase_len(plain_cuts, len(text), w)
        if name == "neither":
            assert longest <= max_phrase and extras == []
        if name == "period7" or (name == "n_block" and not fast):          # (the window hash happens to cut the N lines' line ends)
            assert longest > 3000
        if name == "long_phrases" and max_phrase == 700:
            assert longest > max_phrase and len(extras) >= 1          # (random sequence: no window of it recurs within 256 bytes)
            assert R.max_phrase_len(want, len(text), w) < longest or len(want) > len(plain_cuts)


# ---------------------------------------------------------------- one plan, one set of thresholds

def dense_sample(torch):
    """sorted context hashes that say "dense" for every p >= 50: 900 singles and 100 loci seen 12 times each"""
    v = np.concatenate([np.arange(1, 901, dtype=np.int64) * 1000, np.repeat(np.arange(1, 101, dtype=np.int64) * 1000 + 7, 12)])
    assert R.density_rule(len(v), 1000, 900, 50)[0]
    return torch.from_numpy(np.sort(v)).cuda()


@pytest.mark.parametrize("p,density", [(50, 0.0), (96, 0.0), (100, 0.0), (200, 0.0), (100, 1.3)])
def test_plan_and_single_gpu_chain_cut_alike(O, ctx, dna, p, density):
    """the multi-GPU chain's parse plan (pfp_dist_parse_plan, pfp_dist_decide_density, params_from_plan) yields the seed and
    the 32-bit thresholds of the single-GPU chain under the same settings - settled dense or not - and the same ends"""
    import torch
    w = 10
    text = np.concatenate([dna] * 5)[:1000000] if p == 100 and density == 0.0 else dna[:50000]
    with settings(ctx, density=density):
        single = check_chain_scan(O, ctx, text, w, p, density)
        plan, first_hash = ctx.dist_parse_plan(bytes(text[:32]), w, p, ranks=1)
        assert first_hash == int(R.window_hashes(text[:w], w)[0]) + single["fseed"]
        if density == 0.0:
            assert plan[3] == 1 and single["chose"] == 1
            smp = dense_sample(torch)
            settled = {True: ctx.dist_decide_density(smp.data_ptr(), smp.numel(), p, plan), False: ctx.dist_decide_density(0, 0, p, plan)}
        else:
            assert plan[3] == 0
            settled = {False: plan}
        for dense, pl in settled.items():
            assert pl[3] == 0
            got = ctx.debug_scan_chain(text, w, p, plan=pl)
            want_thr = single["fthr_first"] if (dense or density > 0) else single["fthr_nom"]
            assert (got["fseed"], got["fthr"], got["fthr_nom"]) == (single["fseed"], want_thr, single["fthr_nom"]), (p, density, dense)
            if density == 0.0:
                want = single["dense_ends"] if dense else single["dense_ends"][single["nominal"] != 0]
            else:
                want = single["ends"]
            assert np.array_equal(got["ends"], want) and got["n_used"] == len(text)
            if bool(single["dense"]) == dense:
                assert np.array_equal(got["ends"], single["ends"])


def test_plan_sample_counts_cuts_after_the_halo(O, ctx, coll):
    """pfp_dist_propose_triggers2 while the plan's density is a candidate: the shard's sample holds the sampled cuts at or after
    the halo, and no others"""
    import torch
    w, p, halo = 10, 100, 200000
    text = coll[300000:1500000]
    with settings(ctx):
        plan, _ = ctx.dist_parse_plan(bytes(coll[:32]), w, p, ranks=2)
        assert plan[0] == 1 and plan[3] == 1
        fthr, fnom, _ = R.thresholds(p)
        d_text = torch.from_numpy(text.copy()).cuda()
        d_smp = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
        _, n_sample = ctx.dist_propose_triggers2(d_text.data_ptr(), len(text), halo, w, p, plan, d_smp.data_ptr(), d_smp.numel())
        torch.cuda.synchronize()
    x = R.trigger_values(R.window_hashes(text, w), plan[1])
    ends = np.flatnonzero(x < np.uint64(fnom // R.SAMPLE_SHIFT)) + (w - 1)
    assert n_sample == int((ends >= halo).sum()) and 0 < n_sample < len(ends)
    got = d_smp[:n_sample].cpu().numpy().view(np.uint64)
    assert (np.diff(got.astype(np.float64)) >= 0).all() and (d_smp[n_sample:] == 0).all()


# ---------------------------------------------------------------- the exact (Karp-Rabin) scan: pfp_scan against the oracle

KR_MODULI = [10, 11, 64, 1 << 20, (1 << 31) - 1, 1 << 31, (1 << 32) + 1]


@pytest.mark.parametrize("w", WIDTHS + [18, 25])
def test_exact_scan_every_width_and_modulus(O, ctx, rnd, w):
    """kr_scan_kernel<w, false> for every instantiated width and the generic kernel beyond (18, 25), bytes 3..255; even moduli
    with a large power of two, and p >= 2^31, where only a window whose hash is 0 is cut: such windows are planted at a lane's
    first and last position and across a tile seam"""
    text = rnd.copy()
    planted = []
    if w <= 7:
        z = zero_hash_window(w)
        for end in (31, 4096, 65536 + 2, 150015):
            text[end - w + 1:end + 1] = z
            planted.append(end)
    for p in KR_MODULI:
        ends, used = ctx.scan(text, w, p)
        want = O.scan(text, w, p)
        assert used == len(text) and np.array_equal(ends, want), (w, p)
        assert np.array_equal(want, R.kr_cuts(text, w, p))
        if p >= (1 << 31) - 1:
            assert want.tolist() == planted
        if p <= 64:
            assert len(want) > 0.5 * len(text) / p


@pytest.mark.parametrize("w", [4, 10, 17, 18])
def test_exact_scan_lengths_and_special_bytes(O, ctx, rnd, dna, w):
    """pfp_scan at the lengths and with the bytes <= 2 of the fused path's tests"""
    for n in sorted(set(LENGTHS) | {w - 1, w, w + 1}):
        for text in (rnd[:n], dna[1000:1000 + n]):
            ends, used = ctx.scan(text, w, 11)
            assert used == n and np.array_equal(ends, O.scan(text, w, 11)), (w, n)
    for base, p in ((rnd[:70000], 11), (dna[:70000], 100)):
        for text, first in special_byte_texts(base):
            ends, used = ctx.scan(text, w, p)
            assert used == first and np.array_equal(ends, O.scan(text, w, p)), (w, p, first)
