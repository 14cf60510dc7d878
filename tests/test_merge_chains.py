"""The two kernels of the merge whose chains of dependent loads were cut (csrc/merge.hip): unit_edges_kernel, which now asks
for everything a slot's index addresses in one round trip and hands the word of the boundary map to its store, and phase A
of hard_groups_kernel, which reads the classifier's record of a fallback group instead of walking the group's members.

Every case drives the fused chain with BWT only, the full SA and the sampled SA files, in both index widths, and compares
every output with the CPU oracle.  What a case is named for is computed from the oracle's dictionary - `layout` lays the
merge's units out as the merge does: slots in suffix order, offsets from the occurrence counts - and asserted before the
outputs are looked at; what the GPU says about its path (`Context.stats()`, the kernel trace) must agree with it."""
import os

import numpy as np
import pytest

import merge_cases as mc

pytestmark = pytest.mark.gpu

BWT_ONLY, DENSE, SPARSE = mc.FLAG_SETS
EOW = 1                                          # the terminator of a dictionary word
HARD_RANK, HARD_MEM, HARD_SORT_MIN, HARD_LDS = 512, 256, 512, 1024      # kHardRank, kHardMem, kHardSortMin, kHardLds
OFF_TILE = 2048                                  # slots per offset tile (tbase[])


# ---------------------------------------------------------------- the merge's units, from the oracle's dictionary

def layout(O, text, w, p):
    """{units, n_out, n_slots, last_emits}: every group of equal suffixes longer than w (terminator included) in suffix
    order, with its members' (preceding char, occurrences), its first slot and its first output position"""
    ps = O.parse(text, w, p)
    d, occ = ps["dict"].tobytes(), ps["occ"]
    groups, short = {}, []
    start = wd = 0
    while start < len(d):
        end = d.find(b"\x01", start)
        if end < 0:
            break
        for i in range(start, end + 1):
            if end - i > w:
                groups.setdefault(d[i:end + 1], []).append((EOW if i == start else d[i - 1], int(occ[wd])))
            else:
                short.append(d[i:end + 1])
        start, wd = end + 1, wd + 1
    assert wd == len(occ)
    n_slots = len(d)                             # one slot per dictionary byte; the bytes after the last word sort first
    order = sorted([(s, None) for s in short] + [(s, m) for s, m in groups.items()], key=lambda x: x[0])
    slot, base, units = len(d) - start, 0, []
    for s, mem in order:
        if mem is None:
            slot += 1
            continue
        per = {}
        for c, o in mem:
            per[c] = per.get(c, 0) + o
        units.append(dict(s=s, k=len(mem), E=sum(per.values()), base=base, slot=slot, per=per, mem=mem))
        slot += len(mem)
        base += units[-1]["E"]
    assert slot == n_slots
    return dict(units=units, n_out=base, n_slots=n_slots, last_emits=order[-1][1] is not None and EOW not in units[-1]["per"])


def kind(u):
    """'word' (a whole word), 'fill' (one preceding char), or what hard_classify_kernel makes of a hard group: 'minor'
    (majority fill + minority placement) or 'fallback' (every occurrence ranked)"""
    if len(u["per"]) == 1:
        return "word" if EOW in u["per"] else "fill"
    E, k, maj = u["E"], u["k"], max(u["per"].values())
    mc_ = next(c for c in u["per"] if u["per"][c] == maj)
    minor = E - maj
    mm_max = max(o for c, o in u["mem"] if c != mc_)
    # (a tie for the majority: every candidate leaves minor * 4 > E or the same minor, and mm_max matters only above 1024)
    return "fallback" if len(u["per"]) > 4 or minor * 4 > E or mm_max > 1024 or minor * k > 16 * E + 4096 else "minor"


def route(u):
    """where hard_groups_kernel sends a group: ranked in its LDS tables, sorted by one wave, or queued for the device-wide path"""
    if u["E"] <= HARD_SORT_MIN:
        return "lds" if u["k"] <= HARD_MEM else "big"
    return "sort" if u["E"] <= HARD_LDS else "big"


def loci_text(ncopies, L, loci, seed, alleles=b"ACGT", linked=False):
    """ncopies copies of one random ACGT sequence of L bases; copy c carries alleles[(c // len(alleles)**j) % len(alleles)]
    at loci[j] (linked: j = 0 at every locus)"""
    rng = np.random.default_rng(seed)
    copies = np.tile(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)], (ncopies, 1))
    na = len(alleles)
    for j, pos in enumerate(loci):
        copies[:, pos] = np.frombuffer(alleles, dtype=np.uint8)[(np.arange(ncopies) // na ** (0 if linked else j)) % na]
    return copies.reshape(-1).copy()


# name -> (text(O), w, p).  The seeds, loci and copy numbers were found by search on the CPU (layout alone); the tests assert
# what they were chosen for:
#   e512 / e513   a locus whose groups are the text's only hard groups of 513 .. 1024 occurrences
#   k256 / k257   five adjacent loci, copy c carrying the digits of c in base 4: the loci change the phrase boundaries of some
#                 copies, so the words that share the suffix after the last locus are counted, not computed - 379 copies make
#                 256 distinct words, the 380th makes one more
#   sliced_groups the middle of its BWT, no multiple of 64, lies inside a fallback group
M_LOCI = [20, 21, 22, 23, 24]
INPUTS = {
    "k2": (lambda O: loci_text(100, 300, [150], 5, alleles=b"AC"), 4, 11),
    "e512": (lambda O: loci_text(512, 120, [35], 0), 4, 11),
    "e513": (lambda O: loci_text(513, 120, [35], 0), 4, 11),
    "k256": (lambda O: loci_text(379, 200, M_LOCI, 0), 4, 11),
    "k257": (lambda O: loci_text(380, 200, M_LOCI, 0), 4, 11),
    # a locus every ten bases, the same allele at all of them in one copy: nearly every phrase of a copy carries one
    "small_groups": (lambda O: loci_text(100, 2400, list(range(7, 2393, 10)), 11, linked=True), 4, 11),
    "sliced_groups": (lambda O: loci_text(100, 600, list(range(7, 593, 10)), 11, linked=True), 4, 11),
    "tiles": (lambda O: O.gen_fasta(3000, 130, 0.01, 7), 10, 100),
}
for _drop in range(16):
    INPUTS["tail%d" % _drop] = (lambda O, n=_drop: text_of(O, "tiles")[:len(text_of(O, "tiles")) - n].copy(), 10, 100)

_texts, _layouts, _wants, _runs = {}, {}, {}, {}


def new_context(pkg, **env):
    """a context that parses with the reference's window hash (PFP_WINDOW_HASH=kr, read when a context is made): the chain's
    own faster hash picks other phrase boundaries - the same BWT from another dictionary, and `layout` would describe
    the wrong one"""
    env = dict(env, PFP_WINDOW_HASH="kr")
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.Context(0)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx(pkg):
    """(overrides the session's context for this file; the pool check of conftest.py looks at the one named ctx)"""
    c = new_context(pkg)
    yield c
    c.close()


def text_of(O, name):
    if name not in _texts:
        _texts[name] = INPUTS[name][0](O)
    return _texts[name]


def layout_of(O, name):
    if name not in _layouts:
        _, w, p = INPUTS[name]
        _layouts[name] = layout(O, text_of(O, name), w, p)
    return _layouts[name]


def want_of(O, name, flags):
    """the oracle's outputs, computed once per (input, flags)"""
    if (name, flags) not in _wants:
        _, w, p = INPUTS[name]
        _wants[name, flags] = O.bigbwt(text_of(O, name), w, p, flags)
    return _wants[name, flags]


def run_of(O, ctx, name, flags, width):
    """one traced call of the fused chain per (input, flags, width): outputs, {row: launches}, the merge's statistics"""
    key = (name, flags, width)
    if key not in _runs:
        _, w, p = INPUTS[name]
        ctx.set_index_bits(64 if width == 64 else 0)
        ctx.set_kernel_trace(True)
        try:
            got = ctx.bigbwt(text_of(O, name), w, p, flags)
            rows = mc.merge_rows(ctx.kernel_trace())
            st = ctx.stats()
        finally:
            ctx.set_kernel_trace(False)
            ctx.set_index_bits(0)
        _runs[key] = (got, rows, {k: st[k] for k in mc.MERGE_STATS + ("dict_size",)})
    return _runs[key]


def check_outputs(pkg, got, want, flags):
    assert np.array_equal(got["bwt"], want["bwt"])
    if flags & pkg.FLAG_SA:
        assert np.array_equal(pkg.unpack5(got["sa"]), want["sa"])
    if flags & pkg.FLAG_SSA:
        assert np.array_equal(pkg.unpack5(got["ssa"]).reshape(-1, 2), want["ssa"])
    if flags & pkg.FLAG_ESA:
        assert np.array_equal(pkg.unpack5(got["esa"]).reshape(-1, 2), want["esa"])


def check_layout(O, name):
    """the layout is the merge's: it covers the BWT, and every fill unit's range holds its one char"""
    lay = layout_of(O, name)
    bwt = want_of(O, name, 0)["bwt"]
    assert lay["n_out"] == len(bwt) == len(text_of(O, name)) + 1
    for u in lay["units"]:
        if kind(u) == "fill":
            c = next(iter(u["per"]))
            assert (bwt[u["base"]:u["base"] + u["E"]] == (0 if c == 2 else c)).all()
    return lay


def check_path(lay, rows, st, flags):
    """what the GPU reports against what the layout predicts.  Dense SA classifies nothing: every group of several words is
    hard and phase A walks its members; the other two classify, and the fallback groups go through their records"""
    units = lay["units"]
    assert st["dict_size"] == lay["n_slots"]
    if flags == DENSE:
        hard = [u for u in units if u["k"] > 1]
        assert "pfp::hard_classify_kernel" not in rows and st["hard_minor_groups"] == 0
    else:
        hard = [u for u in units if kind(u) == "fallback"]
        assert rows.get("pfp::hard_classify_kernel") == 1
        assert st["hard_minor_groups"] == sum(kind(u) == "minor" for u in units)
    assert rows.get("pfp::hard_groups_kernel", 0) == (0 if not hard else 2 if flags == SPARSE else 1)
    assert st["hard_groups"] - st["hard_minor_groups"] == len(hard)
    assert st["hard_big_groups"] == sum(route(u) == "big" for u in hard)
    assert ("pfp::hard_sort_kernel" in rows) == any(route(u) == "sort" for u in hard)
    assert ("pfp::unit_edges_kernel" in rows) == (flags == SPARSE)
    return hard


def run_and_check(O, pkg, ctx, name, flags, width):
    lay = check_layout(O, name)
    got, rows, st = run_of(O, ctx, name, flags, width)
    hard = check_path(lay, rows, st, flags)
    check_outputs(pkg, got, want_of(O, name, flags), flags)
    return lay, hard, rows, st


CASES = [(f, w) for f in mc.FLAG_SETS for w in mc.WIDTHS]
case_ids = ["flags%d-idx%d" % c for c in CASES]


# ---------------------------------------------------------------- hard groups, fallback path

@pytest.mark.parametrize("flags,width", CASES, ids=case_ids)
def test_fallback_group_of_two_members(O, pkg, ctx, flags, width):
    """a locus that is A in half of the copies and C in the other half: the suffixes after it are groups of k = 2 members
    with no dominating char"""
    lay, hard, _, _ = run_and_check(O, pkg, ctx, "k2", flags, width)
    fb = [u for u in lay["units"] if kind(u) == "fallback"]
    assert any(u["k"] == 2 and u["E"] == 100 and sorted(u["per"].values()) == [50, 50] for u in fb)


@pytest.mark.parametrize("flags,width", CASES, ids=case_ids)
@pytest.mark.parametrize("name,E", [("e512", 512), ("e513", 513)])
def test_fallback_group_at_the_lds_ranking_limit(O, pkg, ctx, name, E, flags, width):
    """k = 4 members (a quarter of the copies each) of E = 512 occurrences: ranked in the LDS tables; 513: sorted by one
    wave.  No other hard group of the text lies in 513 .. 1024, so the row of hard_sort_kernel is the witness (check_path)"""
    lay, hard, rows, _ = run_and_check(O, pkg, ctx, name, flags, width)
    fb = [u for u in lay["units"] if kind(u) == "fallback"]
    assert any(u["k"] == 4 and u["E"] == E for u in fb)
    if flags != DENSE:
        assert ("pfp::hard_sort_kernel" in rows) == (E == 513)
        assert all(route(u) != "sort" or u["E"] == 513 for u in fb)


@pytest.mark.parametrize("flags,width", CASES, ids=case_ids)
@pytest.mark.parametrize("name,k", [("k256", 256), ("k257", 257)])
def test_fallback_group_at_the_member_limit(O, pkg, ctx, name, k, flags, width):
    """256 distinct words share the suffix after the last of five loci - the member table is full; one more copy, one more
    word: 257, and the group leaves the LDS tables for the device-wide queue although its 380 occurrences would fit"""
    lay, hard, _, st = run_and_check(O, pkg, ctx, name, flags, width)
    top = max((u for u in lay["units"] if kind(u) == "fallback"), key=lambda u: u["k"])
    assert top["k"] == k and top["E"] == k + 123 and route(top) == ("lds" if k == 256 else "big")
    assert top in hard
    if flags != DENSE:      # (with the full SA the fills of several words are hard groups as well, larger ones among them)
        assert st["hard_big_groups"] == (k == 257)


def batches_with_a_second_round(fb, gpb):
    """batches of gpb consecutive groups of which the LDS tables do not hold all live ones at once"""
    n = 0
    for b in range(0, len(fb), gpb):
        live = [u for u in fb[b:b + gpb] if route(u) == "lds"]
        n += sum(u["k"] for u in live) > HARD_MEM or sum(u["E"] for u in live) > HARD_RANK
    return n


@pytest.mark.parametrize("flags,width", CASES, ids=case_ids)
def test_batches_that_take_a_second_round(O, pkg, ctx, flags, width):
    """several hundred groups of 4 members and 100 occurrences: eight of them (a batch of a list this short) are 800
    occurrences, more than the 512 the tables rank at once"""
    import torch
    lay, hard, _, _ = run_and_check(O, pkg, ctx, "small_groups", flags, width)
    gpb, n_cu = 64, torch.cuda.get_device_properties(0).multi_processor_count
    while gpb > 8 and len(hard) // gpb < n_cu * 32:
        gpb >>= 1
    print("groups", len(hard), "per batch", gpb, "batches with a second round", batches_with_a_second_round(hard, gpb))
    assert len(hard) >= 200 and batches_with_a_second_round(hard, gpb) >= 10


@pytest.mark.parametrize("flags,width", CASES, ids=case_ids)
def test_classifier_records_equal_the_walk(O, pkg, flags, width):
    """PFP_DEBUG=1: the merge walks every fallback group's members as phase A did and fails the call when a record differs
    (member count, first output position, occurrences); on every text of this file, in a context of its own"""
    with new_context(pkg, PFP_DEBUG="1") as dctx:
        dctx.set_index_bits(64 if width == 64 else 0)
        for name in ("k2", "e512", "e513", "k256", "k257", "small_groups", "sliced_groups", "tiles"):
            _, w, p = INPUTS[name]
            dctx.set_kernel_trace(True)
            got = dctx.bigbwt(text_of(O, name), w, p, flags)
            rows = mc.merge_rows(dctx.kernel_trace())
            dctx.set_kernel_trace(False)
            assert ("pfp::hard_classify_kernel" in rows) == (flags != DENSE) and "pfp::hard_groups_kernel" in rows, name
            assert np.array_equal(got["bwt"], want_of(O, name, 0)["bwt"]), name


# ---------------------------------------------------------------- output slices (two virtual ranks on one device)

def _pieces(res, key):
    off, parts = 0, []
    for r in res:
        assert r[key + "_off"] == off, (key, r[key + "_off"], off)
        parts.append(r[key].cpu().numpy())
        off += r[key].numel()
    return np.concatenate(parts)


def run_sliced(O, pkg, name, flags, width):
    """the text through two ranks that each emit one half of the BWT; returns (slice boundary, per-rank statistics)"""
    import importlib

    import torch
    d = importlib.import_module("bigbwt_amd.dist")
    _, w, p = INPUTS[name]
    text, want = text_of(O, name), want_of(O, name, flags)
    n = len(text)
    cuts = [0, n // 2 - 2, n]
    ctxs = [new_context(pkg) for _ in range(2)]
    try:
        for c in ctxs:
            c.set_index_bits(64 if width == 64 else 0)
        shards = [torch.from_numpy(text[cuts[r]:cuts[r + 1]].copy()).cuda() for r in range(2)]
        res = d.simulate(ctxs, shards, w, p, flags, halo=8192, shard_sa=False)
        stats = [c.stats() for c in ctxs]
        assert res[0]["lo"] == 0 and res[0]["hi"] == res[1]["lo"] and res[1]["hi"] == n + 1
        assert np.array_equal(torch.cat([r["bwt"] for r in res]).cpu().numpy(), want["bwt"])
        if flags & pkg.FLAG_SA:
            assert np.array_equal(pkg.unpack5(_pieces(res, "sa5")), want["sa"])
        if flags & pkg.FLAG_SSA:
            assert np.array_equal(pkg.unpack5(_pieces(res, "ssa")).reshape(-1, 2), want["ssa"])
        if flags & pkg.FLAG_ESA:
            assert np.array_equal(pkg.unpack5(_pieces(res, "esa")).reshape(-1, 2), want["esa"])
        return res[1]["lo"], stats
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("flags,width", CASES, ids=case_ids)
def test_fallback_group_cut_by_a_slice_boundary(O, pkg, flags, width):
    """the middle of the BWT, where the second rank's slice begins, lies inside a fallback group: both ranks rank the group
    and each writes its part - and both count it"""
    lay = check_layout(O, "sliced_groups")
    cut, stats = run_sliced(O, pkg, "sliced_groups", flags, width)
    fb = [u for u in lay["units"] if kind(u) == "fallback"]
    assert cut % 64 != 0 and any(u["base"] < cut < u["base"] + u["E"] for u in fb)
    if flags != DENSE:
        assert sum(s["hard_groups"] - s["hard_minor_groups"] for s in stats) == len(fb) + 1


# ---------------------------------------------------------------- unit edges

def boundary_bits(bwt, lo, hi):
    """positions of [lo, hi) that start or end a run of the BWT, the slice's two ends always (run_bitmap_kernel)"""
    b = bwt[lo:hi]
    m = np.zeros(hi - lo, dtype=bool)
    m[0] = m[-1] = True
    m[1:] |= b[1:] != b[:-1]
    m[:-1] |= b[1:] != b[:-1]
    return m


def edge_seams(lay, bwt, lo, hi):
    """what the units of the slice [lo, hi) that unit_edges_kernel samples (fill and hard units, not whole words) meet in the
    boundary map: first and last position in one word / in two words, and the bit positions of the edges that are stored"""
    m = boundary_bits(bwt, lo, hi)
    same = two = 0
    bits = set()
    for u in lay["units"]:
        if kind(u) == "word":
            continue
        f, l = u["base"], u["base"] + u["E"] - 1
        if lo <= f and l < hi:
            same += (f - lo) >> 6 == (l - lo) >> 6 and f != l
            two += (f - lo) >> 6 != (l - lo) >> 6
        for x in (f, l):
            if lo <= x < hi and m[x - lo]:
                bits.add((x - lo) & 63)
    return same, two, bits


@pytest.mark.parametrize("flags,width", CASES, ids=case_ids)
def test_unit_edges_in_the_words_of_the_boundary_map(O, pkg, ctx, flags, width):
    """130 copies of 3000 bases, whole and as two slices of which the second begins at a position that is no multiple of
    64: units whose two edges share a word of the map and units whose edges lie in two, stored edges at bit 0 and bit 63"""
    lay, _, _, st = run_and_check(O, pkg, ctx, "tiles", flags, width)
    bwt = want_of(O, "tiles", 0)["bwt"]
    n_out = lay["n_out"]
    same, two, bits = edge_seams(lay, bwt, 0, n_out)
    assert same > 0 and two > 0 and {0, 63} <= bits
    cut, _ = run_sliced(O, pkg, "tiles", flags, width)
    assert cut % 64 != 0
    for lo, hi in ((0, cut), (cut, n_out)):
        same, two, bits = edge_seams(lay, bwt, lo, hi)
        assert same > 0 and two > 0 and {0, 63} <= bits
    # a unit cut by the slice boundary: each rank asks for the edge it holds
    assert any(u["base"] < cut < u["base"] + u["E"] for u in lay["units"] if kind(u) != "word")


def test_units_across_offset_tiles(O, pkg, ctx):
    """more than 2048 slots: a last member t whose t + 1 opens the next offset tile reads two different tbase[] entries, and
    a wave whose look-ahead slot lies in the next tile"""
    lay = check_layout(O, "tiles")
    assert lay["n_slots"] > 2 * OFF_TILE
    ends = {u["slot"] + u["k"] for u in lay["units"] if kind(u) != "word"}
    seams = [t for t in range(OFF_TILE, lay["n_slots"], OFF_TILE) if t in ends]
    print("slots", lay["n_slots"], "units that end at a tile seam", seams)
    assert seams
    for flags, width in CASES:
        run_and_check(O, pkg, ctx, "tiles", flags, width)


def last_slot(O, text, w, p):
    """(number of slots, the largest suffix of the dictionary emits as a unit - longer than w and no whole word); layout()
    says the same and more, at ten times the cost"""
    d = O.parse(text, w, p)["dict"].tobytes()
    best, best_whole, start = b"", False, 0
    while True:
        end = d.find(b"\x01", start)
        if end < 0:
            break
        i = max(range(start, end + 1), key=lambda j: d[j:end + 1])
        if d[i:end + 1] > best:
            best, best_whole = d[i:end + 1], i == start
        start = end + 1
    return len(d), len(best) - 1 > w and not best_whole


_tail0 = []


@pytest.mark.parametrize("drop", range(16))
def test_last_slot_in_every_lane(O, pkg, ctx, drop):
    """the same collection with 0 .. 15 trailing bases dropped: the number of slots N takes 16 consecutive values (N mod 64,
    N mod 256), and the largest suffix of the dictionary emits - the last unit ends at slot N - 1, whose loc[t + 1] and
    tbase[(t + 1) >> 11] are the padding's"""
    name = "tail%d" % drop
    _, w, p = INPUTS[name]
    if not _tail0:
        _tail0.append(last_slot(O, text_of(O, "tail0"), w, p)[0])
    n_slots, emits = last_slot(O, text_of(O, name), w, p)
    print("slots", n_slots, "mod 64", n_slots % 64, "mod 256", n_slots % 256)
    assert emits and n_slots == _tail0[0] - drop
    for flags, width in CASES:
        got, rows, st = run_of(O, ctx, name, flags, width)
        assert st["dict_size"] == n_slots
        assert ("pfp::unit_edges_kernel" in rows) == (flags == SPARSE)
        check_outputs(pkg, got, want_of(O, name, flags), flags)
