"""No GPU: every input of parse_keys_cases.py has the property its name claims, in plain numpy - so that a GPU case that passes
has passed on the path it was built for."""
import numpy as np
import pytest

import parse_keys_cases as K


@pytest.mark.parametrize("name", [n for n in K.FIRST_ROUND if n not in ("below_merge_switch", "above_merge_switch", "tuned_sort")])
def test_first_round_strings_are_what_their_names_say(name):
    build, layout, pair_at = K.FIRST_ROUND[name]
    s = build()
    assert s.dtype == np.uint32 and s[-1] == 0 and (len(s) == 1 or s[:-1].min() >= 1), "ends in its only 0"
    pairs = K.equal_pairs(s)
    if pair_at is None:
        assert len(pairs) == 0, "run-free"
    else:
        assert pairs.tolist() == [pair_at], "exactly the one equal pair"
    width = 64 - 2 * K.bits_for(int(s.max()))
    if layout == "plain":
        assert width < K.RUN_BITS_MIN
    else:
        assert width >= K.RUN_BITS_MIN
        assert (layout == "two symbols") == (pair_at is None)
    if name.startswith("top_"):
        assert int(s.max()) == {"top_2^29-1": (1 << 29) - 1, "top_2^29": 1 << 29}[name]
        assert width == {"top_2^29-1": 6, "top_2^29": 4}[name]


def test_the_sizes_of_the_first_round_strings():
    sizes = sorted(len(K.FIRST_ROUND["free_%d" % n][0]()) for n in K.SMALL_SIZES)
    assert sizes == [2, 3, 64, 65, 257, 70_001]
    # (the three long strings are built once, here: length, largest symbol and run-freeness)
    for name, n in (("below_merge_switch", K.MERGE_SWITCH - 3), ("above_merge_switch", K.MERGE_SWITCH + 5), ("tuned_sort", K.TUNED_MIN + 1000)):
        s = K.FIRST_ROUND[name][0]()
        assert len(s) == n and int(s.max()) == 3000 and len(K.equal_pairs(s)) == 0 and s[-1] == 0 and s[:-1].min() >= 1
    assert K.MERGE_SWITCH - 3 < (1 << 20) < K.MERGE_SWITCH + 5 and K.TUNED_MIN + 1000 > 6 * (1 << 20)
    pairs = {n: [k for k in K.FIRST_ROUND if k.startswith("pair_%d_" % n)] for n in K.SMALL_SIZES}
    assert pairs[2] == [] and len(pairs[3]) == 1 and all(len(pairs[n]) == 3 for n in (64, 65, 257, 70_001))


@pytest.fixture(scope="module")
def rounds():
    out = {}
    for name, build in K.PIVOT.items():
        parse, last, occ = build()
        assert len(parse) == len(last) and parse[0] == 1 and (parse[1:] >= 2).all()
        out[name] = K.first_pivot_round(parse, occ)
    return out


def test_pivot_lists_are_long_enough_for_a_pivot_round(rounds):
    for name, r in rounds.items():
        m = len(r["pos"])
        if name in K.MEMBERS:
            assert m == K.MEMBERS[name], name
        assert (m >= K.PIVOT_MIN) == (name != "members_63"), name
        assert m >= 2 * len(np.unique(r["grp"])), name


def test_private_variants_end_every_walk_at_a_rare_symbol(rounds):
    r = rounds["private"]
    other = r["lcp"] >= 0
    assert other.sum() > 40 * 150
    # most members leave the pivot at their own variant, dist[i + 2] symbols on; none walks for cap symbols
    assert (r["lcp"][other] == r["dv"][other]).sum() > other.sum() // 2 and (r["lcp"] < K.CAP).all()


def test_shared_variant_members_differ_before_their_own_distance(rounds):
    r = rounds["shared_variant"]
    early = (r["lcp"] >= 0) & (r["lcp"] < r["dv"])
    assert early.sum() >= 30, "members whose first difference from the pivot lies before their next rare symbol"


def test_long_common_prefixes(rounds):
    assert (rounds["long_equal_batch"]["lcp"] > 4 * K.BATCH).sum() >= 100, "more than one batch"
    assert (rounds["long_equal_batch"]["lcp"] < K.CAP).all()
    assert (rounds["long_equal_cap"]["lcp"] == K.CAP).sum() >= 100, "equal to the pivot for cap symbols"


def test_tail_members_compare_across_the_end_of_the_string(rounds):
    r = rounds["tail"]
    other = r["lcp"] >= 0
    far = np.maximum(r["pos"], r["piv"]) + 2 + 4 * (r["lcp"] // 4)
    assert (other & (far + 4 > r["N"])).sum() >= 1, "the step that finds the difference cannot load 16 bytes of both strings"


def test_groups_straddle_wave_and_workgroup_edges(rounds):
    for name, edges in (("members_64", ()), ("members_65", (64,)), ("members_257", (64, 256))):
        g = rounds[name]["grp"]
        for e in edges:
            assert g[e - 1] == g[e], (name, e)
    g = rounds["members_64"]["grp"]
    assert len(g) == 64 and g[62] == g[63], "the last group ends with the wave"


def test_one_wave_mixes_short_and_long_distances(rounds):
    r = rounds["mixed_wave"]
    dv = r["dv"]
    waves = [dv[a:a + 64] for a in range(0, len(dv), 64)]
    assert any((w == 1).any() and (w > 4 * K.BATCH).any() for w in waves)
