"""No GPU: every input of first_round_cases.py has the property its name claims, in plain numpy - so that a GPU case that passes
has passed on the history it was built for."""
import json
import os

import numpy as np
import pytest

import first_round_cases as F
import parse_keys_cases as K
from textgen import make_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(F.STRINGS))
def test_strings_end_in_their_only_zero(name):
    s = F.STRINGS[name]()
    n = int(name.split("_")[1])
    assert s.dtype == np.uint32 and len(s) == n and s[-1] == 0 and (n == 1 or s[:-1].min() >= 1)


@pytest.mark.parametrize("n", F.SIZES)
def test_distinct_strings_leave_only_singletons(n):
    s = F.distinct(n)
    assert len(K.equal_pairs(s)) == 0
    _, head = F.first_round_groups(s)
    assert np.array_equal(head, np.arange(n)) and F.unresolved(head) == 0


@pytest.mark.parametrize("n", F.SIZES)
def test_constant_strings_are_one_group_from_slot_two_on(n):
    s = F.constant(n)
    assert n < 2 or 64 - 2 * K.bits_for(int(s.max())) < K.RUN_BITS_MIN, "the plain layout: two whole symbols"
    order, head = F.first_round_groups(s)
    if n >= 4:
        assert order[0] == n - 1 and order[1] == n - 2 and np.array_equal(order[2:], np.arange(n - 2))
        assert (head[2:] == 2).all() and F.unresolved(head) == n - 2
    else:
        assert F.unresolved(head) == 0


def test_the_long_constant_string_carries_a_head_across_whole_tiles():
    _, head = F.first_round_groups(F.constant(1500))
    heads_per_tile = [len(np.unique(head[t:t + F.TILE])) for t in range(0, 1500, F.TILE)]
    # tiles 1 .. 5 hold no head of their own: their group starts in tile 0, more than 512 slots before the last of them
    assert heads_per_tile[1:] == [1] * 5 and (head[F.TILE:] == 2).all() and (head == 2).sum() > 512


@pytest.mark.parametrize("n", (257, 511, 512, 513, 1500))
def test_periodic_and_fibonacci_groups_straddle_tile_edges(n):
    for build in (F.periodic, F.fibonacci):
        _, head = F.first_round_groups(build(n))
        edge = np.arange(F.TILE, n, F.TILE)
        assert (head[edge] < edge).any(), "a group whose head lies in an earlier tile"
        assert 0 < F.unresolved(head) and len(np.unique(head)) >= 3


@pytest.mark.parametrize("n", (255, 256, 257))
def test_groups_end_at_and_around_the_first_tile_edge(n):
    # (the last slot of the string is the last slot of a group that began before it)
    _, head = F.first_round_groups(F.periodic(n))
    assert head[n - 1] < n - 1


def test_fibonacci_takes_the_run_layout():
    s = F.fibonacci(513)
    assert len(K.equal_pairs(s)) > 0 and 64 - 2 * K.bits_for(int(s.max())) >= K.RUN_BITS_MIN


def test_far_variants_stay_equal_to_their_pivot_beyond_cap_and_beyond_the_finisher():
    parse, last, occ = F.far_variants()
    r = K.first_pivot_round(parse, occ)
    m = len(r["pos"])
    assert m >= K.PIVOT_MIN and (r["lcp"] == K.CAP).sum() * 4 > m, "more than a quarter of the members"
    body = parse[1:]
    # (the finisher compares whole suffixes: the first members of two copies agree for longer than it reads)
    assert np.array_equal(body[:2900], body[3000:5900]) and 2900 > F.FINISH_CMP


def _dict_of(O, text, w, p):
    return O.parse(text, w, p)["dict"].tobytes()


def test_directed_texts_hold_the_groups_they_are_named_for(O):
    sizes = {}
    for name, (spec, w, p) in F.TEXTS.items():
        sizes[name] = int(F.prefix_classes(_dict_of(O, make_text(spec, O), w, p), w).max())
    # 257 slots or more: the group crosses at least one edge of a 256-slot tile wherever it lies; more than 512: at least two
    assert F.TILE < sizes["run_400"] <= 2 * F.TILE, sizes
    assert sizes["run_700"] > 2 * F.TILE, sizes


def test_the_resolved_text_has_no_two_suffixes_alike_for_twelve_bytes(O):
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as fh:
        c = [c for c in json.load(fh) if c["name"] == F.RESOLVED][0]
    counts = F.prefix_classes(_dict_of(O, make_text(c["spec"], O), c["w"], c["p"]), c["w"], 12)
    assert len(counts) > 0 and counts.max() == 1
