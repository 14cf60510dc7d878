"""Every path of the merge (csrc/merge.hip, `Merge<I>::run`) with a witness that it ran: per path one case whose kernel trace
holds the row only that path opens, and one whose trace does not.  The outputs of the same inputs are checked against the
references in test_gpu_parity.py; tests/README.md has the table, merge_cases.py the inputs."""
import pytest

import merge_cases as mc

pytestmark = pytest.mark.gpu

BWT_ONLY, DENSE, SPARSE = mc.FLAG_SETS
GOLDEN = "golden_gen_small"      # 61 KB, about 600 phrases: no group can reach the 513 occurrences of the sorted / queued paths
FROM_KEYS = "golden_tiny_dna_w4"
MID_GROUPS = "copies400"


@pytest.fixture(scope="module")
def launches(pkg, O):
    """launches(case, flags, width=32) -> {row: launches} of one traced call, run once per module"""
    cache = {}

    def get(case, flags, width=32):
        key = (case, flags, width)
        if key not in cache:
            cache[key] = mc.run_case(pkg, O, case, flags, width)["launches"]
        return cache[key]
    return get


def has(trace, *rows):
    return [r for r in rows if trace.get("pfp::" + r, 0) < 1]


def lacks(trace, *rows):
    return [r for r in rows if trace.get("pfp::" + r, 0) > 0]


@pytest.mark.parametrize("width", mc.WIDTHS)
def test_records_gathered_per_position_or_computed_per_slot(launches, width):
    """RecordSource::Gathered (pprec16_kernel writes a record per dictionary position) against RecordSource::PerSlot; with SA
    values everywhere the sort keys never carry the records, so the switch alone decides"""
    gathered = launches(GOLDEN + "/direct0", DENSE, width)
    per_slot = launches(GOLDEN + "/direct1", DENSE, width)
    assert not has(gathered, "pprec16_kernel", "slot_records_kernel") and not lacks(gathered, "slot_payload_kernel")
    assert not has(per_slot, "slot_records_kernel") and not lacks(per_slot, "pprec16_kernel", "slot_payload_kernel")


@pytest.mark.parametrize("width", mc.WIDTHS)
def test_records_from_the_sort_keys(launches, width):
    """RecordSource::SortKeys: the first-round keys carried the records (not -S, key of 39 + 1 bits, pair sort) and fewer than a
    fifth of the slots were re-ordered afterwards.  300 random bytes: no two suffixes agree in the 19 characters a key holds
    unless they are equal to their ends, so the first round settles everything.  Three copies of a genome: the variants of a
    phrase tie with it in the first round - more than half of the slots - and the records are gathered instead."""
    for flags in (BWT_ONLY, SPARSE):
        from_keys = launches(FROM_KEYS, flags, width)
        assert not has(from_keys, "slot_payload_kernel", "slot_loc_kernel", "group_flags_kernel"), flags
        assert not lacks(from_keys, "pprec16_kernel", "slot_records_kernel"), flags
        reordered = launches(GOLDEN, flags, width)
        assert not lacks(reordered, "slot_payload_kernel", "slot_loc_kernel", "group_flags_kernel"), flags
        assert not has(reordered, "slot_records_kernel"), flags
    dense = launches(FROM_KEYS, DENSE, width)
    assert not lacks(dense, "slot_payload_kernel", "slot_loc_kernel", "group_flags_kernel") and not has(dense, "slot_records_kernel")


@pytest.mark.parametrize("width", mc.WIDTHS)
def test_majority_fill_and_minority_placement(launches, width):
    """hard groups are classified, and the minority occurrences of those with a dominating char placed (a word of ~1200
    occurrences and its mutated copy, the N right before the common suffix), unless every SA value is wanted"""
    for flags in (BWT_ONLY, SPARSE):
        assert not has(launches("copies1200", flags, width), "hard_classify_kernel", "hard_minor_fill_kernel", "hard_minor_kernel"), flags
    assert not lacks(launches("copies1200", DENSE, width), "hard_classify_kernel", "hard_minor_fill_kernel", "hard_minor_kernel")


@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", mc.FLAG_SETS)
def test_groups_sorted_by_one_wave(launches, flags, width):
    """a hard group of kHardSortMin + 1 .. kHardLds occurrences is queued for hard_sort_kernel: two words of ~400 occurrences
    each that share a suffix.  With 1200 copies every such group has more than 1024, and a text of 600 phrases has none"""
    assert not has(launches(MID_GROUPS, flags, width), "hard_sort_kernel")
    assert not lacks(launches("copies1200", flags, width), "hard_sort_kernel")
    assert not lacks(launches(GOLDEN, flags, width), "hard_sort_kernel")


@pytest.mark.parametrize("width", mc.WIDTHS)
@pytest.mark.parametrize("flags", mc.FLAG_SETS)
def test_large_groups_sorted_device_wide_or_ranked_per_occurrence(launches, flags, width):
    """groups of more than kHardLds occurrences: one device-wide sort per chunk - or, beyond the budget, hard_big_kernel"""
    sort_rows = [r for r in launches("copies1200", flags, width) if r.endswith(mc.MERGE_SORT_TAG)]
    assert sort_rows and not has(launches("copies1200", flags, width), "big_keys_kernel", "big_place_kernel")
    assert not lacks(launches("copies1200", flags, width), "hard_big_kernel")
    ranked = launches("copies1200/budget100", flags, width)
    assert not has(ranked, "hard_big_kernel") and not lacks(ranked, "big_keys_kernel", "big_place_kernel")
    assert not [r for r in ranked if r.endswith(mc.MERGE_SORT_TAG)]
    assert not lacks(launches(GOLDEN, flags, width), "big_keys_kernel", "big_place_kernel", "hard_big_kernel", "hard_sort_kernel")


@pytest.mark.parametrize("width", mc.WIDTHS)
def test_queue_overflow_redoes_the_lds_pass(launches, width):
    """PFP_BIG_CAP=2: the queue of large groups overflows and hard_groups_kernel runs again with one that fits"""
    assert launches("copies1200/cap2", BWT_ONLY, width)["pfp::hard_groups_kernel"] >= 2
    assert launches("copies1200", BWT_ONLY, width)["pfp::hard_groups_kernel"] == 1


@pytest.mark.parametrize("width", mc.WIDTHS)
def test_second_round_only_for_sampled_sa(launches, width):
    """run boundaries, whole-word SA values and unit edges: the second round of -s / -e"""
    for case in (GOLDEN, "copies1200"):
        assert not has(launches(case, SPARSE, width), "run_bitmap_kernel", "word_sa_kernel", "unit_edges_kernel"), case
        for flags in (BWT_ONLY, DENSE):
            assert not lacks(launches(case, flags, width), "run_bitmap_kernel", "word_sa_kernel", "unit_edges_kernel"), (case, flags)


def test_groups_sorted_by_one_wave_match_the_oracle(O, pkg, wctx):
    """the input that reaches hard_sort_kernel is used by no parity test: every output against the oracle"""
    import numpy as np
    text = mc.text_of(O, MID_GROUPS)
    c = mc.CASES[MID_GROUPS]
    for flags, oflags in ((0, 0), (pkg.FLAG_SA, O.FLAG_SA), (pkg.FLAG_SSA | pkg.FLAG_ESA, O.FLAG_SSA | O.FLAG_ESA)):
        got = wctx.bigbwt(text, c["w"], c["p"], flags)
        want = O.bigbwt(text, c["w"], c["p"], oflags)
        assert np.array_equal(got["bwt"], want["bwt"]), flags
        if flags & pkg.FLAG_SA:
            assert np.array_equal(pkg.unpack5(got["sa"]), want["sa"])
        if flags & pkg.FLAG_SSA:
            assert np.array_equal(pkg.unpack5(got["ssa"]).reshape(-1, 2), want["ssa"])
            assert np.array_equal(pkg.unpack5(got["esa"]).reshape(-1, 2), want["esa"])
