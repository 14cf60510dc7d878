"""The linear suffix-array checker of tests/sacheck.py, pinned on the CPU: it accepts the oracle's arrays for the three
kinds of input (byte text, integer text, gsacak collection) at the sizes the GPU tests use it for, rejects a swap of two
neighbours, a duplicated entry and a wrong tie between separators, and on tiny strings accepts exactly one of all
permutations - the sorted one."""
import itertools

import numpy as np
import pytest

import sorter_cases as sc
from sacheck import assert_sa, sa_error

BANANA = np.frombuffer(b"banana\x01anaba\x01anan\x01\x00", dtype=np.uint8)      # gsa/README.md:76-104


def brute_sa(s, kind):
    """suffixes sorted as Python lists; the k-th separator of a collection becomes a symbol of its own below every letter"""
    s = [int(x) for x in s]
    if kind == "gsa":
        nsep = s.count(1)
        k, t = 0, []
        for x in s:
            if x == 1:
                k += 1
                t.append(k)
            else:
                t.append(x + nsep if x else 0)
        s = t
    return np.array(sorted(range(len(s)), key=lambda i: s[i:]), dtype=np.uint32)


def test_checker_accepts_exactly_the_sorted_permutation():
    rng = np.random.default_rng(1)
    for kind in ("bytes", "int", "gsa"):
        for _ in range(6):
            if kind == "gsa":
                s = np.concatenate([rng.integers(2, 4, size=4), [1, 0]]).astype(np.uint8)
                s[int(rng.integers(1, 3))] = 1      # two strings, or one empty one: separators tie
            else:
                s = np.concatenate([rng.integers(1, 3, size=5), [0]]).astype(np.uint8 if kind == "bytes" else np.uint32)
            want = brute_sa(s, kind)
            passing = [p for p in itertools.permutations(range(len(s))) if sa_error(s, np.array(p, dtype=np.uint32), kind) is None]
            assert passing == [tuple(want.tolist())], (kind, s.tolist())


def test_checker_on_the_trivial_sizes(O):
    for s in ([0], [5, 0], [5, 5, 0]):
        s8 = np.array(s, dtype=np.uint8)
        assert_sa(s8, O.sacak(s8), "bytes")
        assert_sa(np.array(s, dtype=np.uint32), O.sacak_int(np.array(s, dtype=np.uint32)), "int")
    assert sa_error(np.array([5, 0], np.uint8), np.array([0, 1], np.uint32), "bytes") is not None
    assert sa_error(np.array([5, 5], np.uint8), np.array([1, 0], np.uint32), "bytes") is not None      # no final 0


def mutations(s, sa, kind):
    """(what, array) - arrays the checker must reject"""
    n = len(sa)
    for i in (0, n // 3, n - 2):
        bad = sa.copy()
        bad[i], bad[i + 1] = sa[i + 1], sa[i]
        yield f"slots {i} and {i + 1} swapped", bad
    bad = sa.copy()
    bad[n // 2] = sa[n // 2 + 1]
    yield "a duplicated entry", bad
    bad = sa.copy()
    bad[n // 2] = n
    yield "an entry outside the string", bad
    yield "a shorter array", sa[:-1]
    if kind == "gsa":
        # slot 0 is the final 0, slots 1.. are the separators in position order: swap two of them
        nsep = int((s == 1).sum())
        assert nsep >= 2 and (s[sa[1:1 + nsep]] == 1).all()
        for i in (1, nsep - 1):
            bad = sa.copy()
            bad[i], bad[i + 1] = sa[i + 1], sa[i]
            yield f"separators at slots {i}, {i + 1} tied the wrong way", bad


@pytest.mark.parametrize("what", ["banana", "dictionary_1.8MB", "fibonacci_2M", "integers_1.5M"])
def test_checker_accepts_the_oracle_and_rejects_mutations(O, what):
    if what == "banana":
        s, kind = BANANA, "gsa"
    elif what == "dictionary_1.8MB":
        s, kind = sc.CASES["fam_segmented"]["build"](), "gsa"
    elif what == "fibonacci_2M":
        s, kind = sc.byte_text("fibonacci", 2_000_000), "bytes"
    else:
        s, kind = sc.CASES["int_copies"]["build"](), "int"
    sa = {"gsa": lambda: O.gsacak(s, want_lcp=False)[0], "bytes": lambda: O.sacak(s), "int": lambda: O.sacak_int(s)}[kind]()
    assert_sa(s, sa, kind, what)
    assert_sa(s, sa.astype(np.uint64), kind, what)      # the 64-bit entry points return the same array in wider entries
    for desc, bad in mutations(s, sa, kind):
        assert sa_error(s, bad, kind) is not None, f"{what}: the checker accepted {desc}"
