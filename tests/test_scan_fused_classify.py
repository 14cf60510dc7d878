"""GPU: the fused chain's first pass with automatic density, which classifies its cuts where it finds them (csrc/scan.hip:
kr_scan_kernel<W, true, true> writes the nominal flags and lists the sampled cuts, sample_context_kernel hashes their contexts,
count_distinct_kernel counts per workgroup), through pfp_debug_scan_chain against the numpy restatement of tests/scan_reference.py.
The inputs are the smallest on which that code can go wrong: cuts beside a tile edge, more cuts than the first pass has room for,
a special byte (both retries must start clean), a sample larger than its lists, the shortest texts.  Every comparison is exact."""
import contextlib
import os

import numpy as np
import pytest

import scan_reference as R

pytestmark = pytest.mark.gpu

WIDTHS = [4, 10, 17]
P = 100
TILE = 16 * 4096          # positions one workgroup of the scan kernel takes
SAMPLE_SLOTS = 1024       # kSampleSlots


@contextlib.contextmanager
def settings(ctx, density=0.0, max_phrase=0):
    try:
        ctx.set_window_hash(True)
        ctx.set_parse_density(density)
        ctx.set_max_phrase(max_phrase)
        yield ctx
    finally:
        ctx.set_window_hash(True)
        ctx.set_parse_density(0.0)
        ctx.set_max_phrase(1 << 15)


def expected_seed(text, w, p):
    """the seed the contract of scan_reference.seed_contract_violations fixes (its clause 3: the smallest that satisfies 1 and 2);
    None for a first window that no seed below 2^20 satisfies (the searches below pass such texts by)"""
    fthr, fnom, _ = R.thresholds(p)
    first = bytes(text[:w]) if len(text) >= w else None
    for top in (1 << 10, 1 << 20):
        seed = _smallest_seed(first, w, p, fthr, fnom, top)
        if seed is not None:
            break
    assert seed is None or R.seed_contract_violations(first, w, p, seed, fthr, fnom) == []
    return seed


def _smallest_seed(first, w, p, fthr, fnom, top):
    seeds = np.arange(top, dtype=np.uint64)
    ok = np.ones(len(seeds), dtype=bool)
    h_first = None
    if first is not None:
        fw = np.frombuffer(first, dtype=np.uint8)
        h_first = int(R.window_hashes(fw, w)[0])
        x = R.trigger_values(np.uint64(h_first), seeds)
        ok &= (x < np.uint64(fnom)) if int(R.kr_window_hashes(fw, w)[0]) % p == 0 else (x >= np.uint64(fthr))
    if p >= 32:
        for ch in R.DNA_LETTERS:
            hr = int(R.window_hashes(np.full(w, ch, dtype=np.uint8), w)[0])
            if hr != h_first:
                ok &= ~(R.trigger_values(np.uint64(hr), seeds) < np.uint64(fthr))
    return int(np.flatnonzero(ok)[0]) if ok.any() else None


def reference(text, w, p, seed):
    """what the first pass must find on the parsed prefix: (dense cuts, their nominal flags, the sampled cuts)"""
    prefix = text[:R.usable_len(text)]
    fthr, fnom, fauto = R.thresholds(p)
    assert fauto == 1
    x = R.trigger_values(R.window_hashes(prefix, w), seed)
    dense = R._cuts(x < np.uint64(fthr), w)
    xd = x[dense.astype(np.int64) - (w - 1)]
    return dense, xd < np.uint64(fnom), dense[xd < np.uint64(fnom // R.SAMPLE_SHIFT)]


def first_pass_capacity(n, p):
    """room for cuts in the first attempt of scan_text (n bytes, dense candidate)"""
    return min(n, int((n // p) * float(np.float32(float(R.auto_density(p))))) * 4 + 65536)


def sample_capacity(cap, n):
    """room for sampled cuts beside `cap` cuts: an eighth of them and 64 per slot, shared out among one list per 16 tiles"""
    scap = ((cap // 8 + SAMPLE_SLOTS - 1) // SAMPLE_SLOTS + 64) * SAMPLE_SLOTS
    nslots = min(SAMPLE_SLOTS, max(1, -(-n // TILE) // 16))
    return -(-scap // nslots) * nslots


def check(ctx, text, w, p=P, counts=True):
    """one run of the chain's scan with automatic density against the reference: the first pass's cuts, their flags, the sample's
    figures, the choice and the final ends.  Returns (report, sampled cuts of the reference)."""
    text = np.asarray(text, dtype=np.uint8)
    with settings(ctx):
        rep = ctx.debug_scan_chain(text, w, p)
    n_used = R.usable_len(text)
    assert rep["n_used"] == n_used
    prefix = text[:n_used]
    fthr, fnom, _ = R.thresholds(p)
    assert (rep["fthr_first"], rep["fthr_nom"], rep["fauto"]) == (fthr, fnom, 1)
    seed = rep["fseed"]
    assert seed == expected_seed(text, w, p)
    dense, nominal, smp = reference(text, w, p, seed)
    if len(dense) == 0:
        assert rep["chose"] == 0 and rep["dense_ends"] is None and rep["kr_fallback"] == 1 and rep["fast"] == 0
        assert np.array_equal(rep["ends"], R.kr_cuts(prefix, w, p)) and rep["parse_density"] == 1.0
        return rep, smp
    assert rep["chose"] == 1 and rep["dense_cuts"] == len(dense)
    assert np.array_equal(rep["dense_ends"], dense), (w, len(text))
    assert np.array_equal(rep["nominal"] != 0, nominal), (w, len(text))
    assert set(np.unique(rep["nominal"]).tolist()) <= {0, 1}
    assert rep["n_nominal"] == int(nominal.sum())
    assert rep["sampled"] == len(smp), (w, len(text))
    assert rep["kept"] <= rep["sampled"]
    if counts and (len(smp) == 0 or int(smp[0]) >= R.CONTEXT - 1):          # (else the first context starts before the text)
        assert rep["kept"] == rep["sampled"]
        ch = R.density_choice(prefix, w, p, seed, fnom, dense)
        assert (rep["sampled"], rep["distinct"], rep["singles"], rep["dense"]) == (ch["sampled"], ch["distinct"], ch["singles"], int(ch["dense"])), (w, len(text))
    final = dense if rep["dense"] else dense[nominal]
    if len(final) == 0:
        assert rep["kr_fallback"] == 1 and np.array_equal(rep["ends"], R.kr_cuts(prefix, w, p))
    else:
        assert rep["kr_fallback"] == 0 and rep["fthr"] == (fthr if rep["dense"] else fnom)
        assert rep["n_ends"] == len(final) and np.array_equal(rep["ends"], final), (w, len(text))
    return rep, smp


def make_bases(O):
    """per width, a collection as test_scan_chain's `coll`, smaller: 6 copies at 2 per mille - loci and singles both occur.  DNA
    for w = 10 and 17; DNA has 256 windows of 4 letters only, too few for any to be sampled, so w = 4 gets the same over bytes"""
    dna = O.gen_fasta(40000, 6, 0.002, 31)
    rng = np.random.default_rng(31)
    genome = rng.integers(3, 256, size=40000, dtype=np.uint8)
    copies = []
    for _ in range(6):
        c = genome.copy()
        at = rng.integers(0, len(c), size=80)
        c[at] = rng.integers(3, 256, size=80, dtype=np.uint8)
        copies.append(c)
    wide = np.concatenate(copies)
    for t in (dna, wide):
        assert len(t) >= 2 * TILE + 64 + 4000
        t.setflags(write=False)
    return {4: wide, 10: dna, 17: dna}


@pytest.fixture(scope="module")
def bases(O):
    return make_bases(O)


# ---------------------------------------------------------------- tile edges

# offset into `base` at which the text starts, per width: found by edge_offset_search below, so that a cut of the first pass lies
# within w of the edge between the first two tiles
EDGE_OFFSET = {4: 101, 10: 0, 17: 143}


def cut_near_edge(dense, w, edge=TILE):
    d = dense.astype(np.int64)
    return bool(((d >= edge - w) & (d < edge + w)).any())


def edge_offset_search(base, w):
    for off in range(4000):
        text = base[off:off + 2 * TILE + 64]
        seed = expected_seed(text, w, P)
        if seed is not None and cut_near_edge(reference(text, w, P, seed)[0], w):
            return off
    return None


@pytest.mark.parametrize("w", WIDTHS)
def test_cuts_beside_a_tile_edge(ctx, bases, w):
    """lengths 65536 k + delta: the last tile full, short by a window or a byte, longer by one, by w - 1 and by a lane's chunk;
    the tile's own cuts are classified by the workgroup that found them, from the first of the tile to the last"""
    off, base = EDGE_OFFSET[w], bases[w]
    some_sample = both_kinds = 0
    for k in (1, 2):
        for delta in (-w, -1, 0, 1, w - 1, 16):
            text = base[off:off + TILE * k + delta]
            rep, smp = check(ctx, text, w)
            if TILE * k + delta > TILE + w:
                assert cut_near_edge(rep["dense_ends"], w), (w, k, delta)
            some_sample += len(smp) > 0
            both_kinds += rep["singles"] > 0 and rep["distinct"] > rep["singles"]
    assert some_sample >= 6 and both_kinds >= 1


# ---------------------------------------------------------------- more cuts than the first pass has room for

PERIOD_SEED = {4: 71, 10: 200, 17: 76}          # found by period_search below
HEAD = 200000


def periodic_text(base, w, seed, n=3000000):
    """200 KB of the collection (an ordinary sample: loci and singles), then a random period of 20 letters to the end"""
    unit = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=20)]
    return np.concatenate([base[:HEAD], np.tile(unit, (n - HEAD) // 20 + 1)])[:n]


def period_search(base, w):
    """the first rng seed whose period, under the seed the head's first window fixes, has three or more cutting windows - and
    none of them sampled, so that the sample still fits its lists on the second attempt"""
    s = expected_seed(base, w, P)
    fthr, fnom, _ = R.thresholds(P)
    for seed in range(1, 20000):
        unit = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=20)]
        x = R.trigger_values(R.window_hashes(np.tile(unit, 3)[:20 + w - 1], w), s)
        if (x < np.uint64(fthr)).sum() >= 3 and not (x < np.uint64(fnom // R.SAMPLE_SHIFT)).any():
            return seed
    return None


@pytest.mark.parametrize("w", WIDTHS)
def test_more_cuts_than_room_starts_clean(ctx, bases, w):
    """a text with more cuts than min(n, 4 n density / p + 65536): the first attempt is abandoned with its flags, lists and
    counters, and the report of the second equals the reference's"""
    text = periodic_text(bases[w], w, PERIOD_SEED[w])
    dense, _, smp = reference(text, w, P, expected_seed(text, w, P))
    assert len(dense) > first_pass_capacity(len(text), P)          # (the condition the period was searched for)
    assert 0 < len(smp) < 4096
    rep, _ = check(ctx, text, w)
    assert rep["distinct"] > rep["singles"] > 0


# ---------------------------------------------------------------- a special byte

@pytest.mark.parametrize("w", WIDTHS)
def test_special_byte_leaves_the_prefix_alone(ctx, bases, w):
    """a byte <= 2 in the middle of 200 KB: the pass over the whole text is abandoned, flags and sample are the prefix's"""
    base = bases[w]
    for at, val in ((100000, 0), (TILE, 2), (TILE + 5, 1)):
        text = base[:200000].copy()
        text[at] = val
        rep, smp = check(ctx, text, w)
        assert rep["n_used"] == at and len(smp) > 0
        whole = reference(base[:200000], w, P, rep["fseed"])[2]
        assert len(whole) > len(smp)          # (the abandoned pass had counted more)


# ---------------------------------------------------------------- a sample that does not fit

CROWD_SEED = {4: 199, 10: 76, 17: 314}          # found by crowd_search below
CROWD_N = 2000000


def crowd_text(w, seed, n=CROWD_N):
    """a period of 12 letters (w = 4: of 12 bytes, as in make_bases) to the end"""
    rng = np.random.default_rng(seed)
    unit = rng.integers(3, 256, size=12, dtype=np.uint8) if w == 4 else np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=12)]
    return np.tile(unit, n // 12 + 1)[:n]


def crowd_search(w):
    """the first rng seed whose period of 12 letters has cutting windows, all of them sampled"""
    fthr, fnom, _ = R.thresholds(P)
    for seed in range(1, 200000):
        text = crowd_text(w, seed, 12 + w - 1 + 64)
        s = expected_seed(text, w, P)
        if s is None:
            continue
        x = R.trigger_values(R.window_hashes(text[:12 + w - 1], w), s)
        cut = x < np.uint64(fthr)
        if cut.any() and np.array_equal(cut, x < np.uint64(fnom // R.SAMPLE_SHIFT)):
            return seed
    return None


@pytest.mark.parametrize("w", WIDTHS)
def test_sample_larger_than_its_lists(pkg, w):
    """every cut sampled, 31 tiles, one list: every sampled cut is counted, no more are kept than there is room for, and under the
    checking pool (PFP_POOL_DEBUG: exact blocks between canary bands) nothing is written beside the lists"""
    text = crowd_text(w, CROWD_SEED[w])
    dense, nominal, smp = reference(text, w, P, expected_seed(text, w, P))
    assert len(dense) <= first_pass_capacity(len(text), P)          # (one attempt)
    room = sample_capacity(first_pass_capacity(len(text), P), len(text))
    assert len(smp) == len(dense) > room          # (the condition the period was searched for)
    old = os.environ.get("PFP_POOL_DEBUG")
    os.environ["PFP_POOL_DEBUG"] = "1"
    try:
        own = pkg.Context(0)
    finally:
        if old is None:
            del os.environ["PFP_POOL_DEBUG"]
        else:
            os.environ["PFP_POOL_DEBUG"] = old
    try:
        rep, _ = check(own, text, w, counts=False)
        own.debug_check()
    finally:
        own.close()
    assert rep["sampled"] == len(smp) and rep["kept"] <= room and rep["kept"] < rep["sampled"]
    assert rep["kept"] >= 65536          # (what the lists hold is kept)


# ---------------------------------------------------------------- the shortest texts, no cut, a cut in the first window

@pytest.mark.parametrize("w", WIDTHS)
def test_shortest_texts_and_no_cut(ctx, bases, w):
    fell_back, base = 0, bases[w]
    for n in (w - 1, w, w + 1):
        rep, _ = check(ctx, base[1000:1000 + n], w)
        fell_back += rep["kr_fallback"]
    run = np.full(5000, ord("A"), dtype=np.uint8)          # (a run of one letter is not cut: the seed's contract)
    if int(R.kr_window_hashes(run[:w], w)[0]) % P:          # (unless the reference cuts its first window)
        rep, _ = check(ctx, run, w)
        assert rep["chose"] == 0 and rep["dense_ends"] is None
        fell_back += rep["kr_fallback"]
    assert fell_back >= 3


@pytest.mark.parametrize("w", WIDTHS)
def test_cut_in_the_first_window(ctx, bases, w):
    """a text whose first window the reference cuts: the first cut of the first pass is w - 1, inside the nominal threshold"""
    rng = np.random.default_rng(1234 + w)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for _ in range(100000):
        head = lut[rng.integers(0, 4, size=w)]
        if int(R.kr_window_hashes(head, w)[0]) % P == 0 and expected_seed(head, w, P) is not None:
            break
    else:
        raise AssertionError("no window with a reference hash of 0 mod p")
    text = np.concatenate([head, bases[w][2000:72000]])
    rep, _ = check(ctx, text, w)
    assert rep["dense_ends"][0] == w - 1 and rep["nominal"][0] == 1 and rep["ends"][0] == w - 1


# ---------------------------------------------------------------- count_distinct_kernel through sample_says_dense

def mixed(ns, singles, loci):
    """ns sorted values: `singles` values once (the smallest), `loci` values that share the rest (each twice or more)"""
    rest = ns - singles
    assert loci >= 1 and rest >= 2 * loci
    reps = np.full(loci, rest // loci, dtype=np.int64)
    reps[: rest % loci] += 1
    v = np.concatenate([np.arange(1, singles + 1, dtype=np.int64), np.repeat(np.arange(1, loci + 1, dtype=np.int64) * 7 + (1 << 40), reps)])
    assert len(v) == ns
    return v


def decide_cases():
    for ns in (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 100000):
        yield "equal", np.full(ns, 12345, dtype=np.int64)
        yield "distinct", np.arange(1, ns + 1, dtype=np.int64) * 3
        if ns >= 2047:
            # at either side of every clause of the rule (p = 100): loci >= 64, 2 singles <= ns, singles p >= 64 loci; the
            # workgroups' shares of 2048 values end inside runs, so a head counted twice or missed there changes the decision
            half = ns // 2
            yield "loci_64", mixed(ns, half - 100, 64)
            yield "loci_63", mixed(ns, half - 100, 63)
            yield "singles_half", mixed(ns, half, 64)
            yield "singles_half_plus_1", mixed(ns, half + 1, 64)
            yield "variants_enough", mixed(ns, 64, 100)
            yield "variants_one_short", mixed(ns, 63, 100)


def test_sample_says_dense_counts(ctx, bases):
    """pfp_dist_decide_density (sort, count_distinct_kernel, the rule) on sorted arrays of the sizes around a wave, a workgroup and
    a workgroup's share of 2048 values, all equal, all distinct and mixed: the decision numpy.unique's counts give"""
    import torch
    w = 10
    seen = set()
    with settings(ctx):
        plan, _ = ctx.dist_parse_plan(bytes(bases[w][:32]), w, P, ranks=1)
        assert plan[3] == 1
        for name, v in decide_cases():
            _, cnt = np.unique(v, return_counts=True)
            want, _ = R.density_rule(len(v), len(cnt), int((cnt == 1).sum()), P)
            d = torch.from_numpy(v).cuda()
            got = ctx.dist_decide_density(d.data_ptr(), d.numel(), P, plan)
            dens = np.array([got[2]], dtype=np.uint64).view(np.float64)[0]
            assert got[3] == 0 and (dens > 1.0) == want, (name, len(v))
            seen.add((name, want))
    assert ("loci_64", True) in seen and ("loci_63", False) in seen and ("singles_half", True) in seen
    assert ("singles_half_plus_1", False) in seen and ("variants_enough", True) in seen and ("variants_one_short", False) in seen
