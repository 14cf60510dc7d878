"""CPU: chain_reference.py, the plain-Python statement of include/pfpgpu.h, "Chaining anchors", checked on its own - the worked
example of the header with its f, parents and chains as literals, the tie rules on hand-made sets, and properties of the peel on
random anchor sets.  The GPU tests (test_fm_chain.py) compare the library with it."""
import numpy as np

import chain_cases as C
import chain_reference as R
import map_cases as K

WORKED = [(0, 30, 1000), (31, 25, 1031), (60, 40, 1062), (101, 30, 1103), (10, 22, 5000), (40, 35, 5030)]


def test_worked_example():
    f, parent = R.programme(WORKED, None, 20000, 5000, 500)
    assert f == [30, 55, 94, 124, 22, 57]
    assert parent == [None, 0, 1, 2, None, 4]
    chains = R.chains_of(WORKED, None, 20000, 5000, 500, 20)
    fields = [tuple(c[k] for k in ("score", "n", "qs", "qe", "ts", "te", "match")) for c in chains]
    assert fields == [(124, 4, 0, 131, 1000, 1133, 125), (57, 2, 10, 75, 5000, 5065, 57)]
    got = R.chain_arrays([chains])
    assert [a.dtype for a in got] == [np.uint64, np.uint32, np.uint32, np.uint32, np.uint32, np.uint64, np.uint64, np.uint32]
    assert got[0].tolist() == [0, 2] and got[1].tolist() == [124, 57]


def test_the_rules_on_hand_made_sets():
    sets = C.chain_sets()
    starts = K.starts_of(C.CHAIN_TEXT, C.CHAIN_TABLE)
    run = lambda name, k=0: R.programme(sets[name][0][k], starts, 20000, *sets[name][1:3])
    f, parent = run("H back", 0)                            # the one predecessor lies exactly H back
    assert parent[-1] == 0 and len(parent) - 1 == R.H and f[-1] == 41
    f, parent = run("H back", 1)                            # H + 1 back: ignored
    assert parent[-1] is None and f[-1] == 20
    assert run("dq = 0, dt = 0", 0)[1] == [None, None] and run("dq = 0, dt = 0", 1)[1] == [None, None]
    f, parent = run("two equal predecessors")
    assert f == [20, 20, 40] and parent == [None, None, 1]
    a = sets["two equal predecessors"][0][0]
    assert R.programme([a[0], a[2]], starts, 20000, 5000, 500)[0] == [20, 40]       # the earlier one gives the same value
    assert run("f + gain = len") == ([10, 20], [None, None])
    assert run("negative gain")[0][:2] == [50, 30] and run("negative gain")[1][1] == 0
    f, parent = run("shared parent, S")
    assert f == [50, 70, 69] and parent == [None, 0, 0]
    kept, dropped, stopped = R.peel(sets["shared parent, S"][0][0], f, parent, 19)
    assert [(c["score"], c["n"]) for c in kept] == [(70, 2), (19, 1)] and stopped == 1 and not dropped
    kept, dropped, _ = R.peel(sets["shared parent, S"][0][0], f, parent, 20)
    assert [c["score"] for c in kept] == [70] and [c["score"] for c in dropped] == [19]
    assert run("two records")[1] == [None, None, None, 2] or run("two records")[1][2] is None      # no parent across the border
    assert [run("G", k)[1][1] for k in range(3)] == [0, None, 0] and [run("B", k)[1][1] for k in range(2)] == [0, None]
    for name, (anchor_sets, *_rest) in sets.items():
        assert all(R.sorted_strictly(a) for a in anchor_sets), name


def test_properties_on_random_anchor_sets():
    rng = np.random.default_rng(3)
    for trial in range(30):
        anc = C.random_set(rng, int(rng.integers(0, 200)))
        G, B, S = (int(rng.choice(v)) for v in ((50, 300, 5000), (5, 40, 500), (1, 10, 40)))
        f, parent = R.programme(anc, None, 20000, G, B)
        assert all(1 <= fx <= i + l for fx, (i, l, _) in zip(f, anc))
        assert all(p is None or 1 <= x - p <= R.H for x, p in enumerate(parent))
        kept, dropped, _ = R.peel(anc, f, parent, S)
        seen = [a for c in kept + dropped for a in c["anchors"]]
        assert sorted(seen) == list(range(len(anc)))        # disjoint, and the kept and dropped chains' sizes sum to A
        for c in kept + dropped:
            qe = [anc[a][0] + anc[a][1] for a in c["anchors"]]
            te = [anc[a][2] + anc[a][1] for a in c["anchors"]]
            assert all(x < y for x, y in zip(qe, qe[1:])) and all(x < y for x, y in zip(te, te[1:]))
            assert c["score"] <= c["match"] and c["n"] == len(c["anchors"])
            assert c["qs"] < c["qe"] and c["ts"] < c["te"]
        assert all(c["score"] >= S for c in kept) and all(c["score"] < S for c in dropped)


def test_anchors_by_brute_force():
    tb = b"ACGTACGTTTGACCA"
    assert R.ms_lengths(tb, b"ACGTT") == [5, 4, 3, 2, 1] and R.ms_lengths(tb, b"GAGA\x00C") == [2, 1, 2, 1, 0, 1]
    anc, skipped, dropped = R.anchors_of(tb, None, b"CGTAXACGT", 3, 2)
    assert anc == [(5, 4, 0), (0, 4, 1), (5, 4, 4)] and (skipped, dropped) == (0, 0)
    assert R.anchors_of(tb, None, b"CGTAXACGT", 3, 1) == ([(0, 4, 1)], 1, 0)             # ACGT occurs twice: skipped
    assert R.anchors_of(tb, np.array([0, 3, 15]), b"CGTAXACGT", 3, 2) == ([(5, 4, 4)], 0, 2)     # two cross the border at 3


def test_strand_merge_and_mapq():
    assert [R.mapq_of(s) for s in ([], [7], [100, 100], [100, 50], [100, 1], [3, 2])] == [0, 60, 0, 30, 59, 20]
    tb = K.text_of("dna").tobytes()
    starts = K.starts_of("dna", "records")
    read = R.revcomp(tb[13000:13600]) + tb[2000:2300]
    res = R.map_long(tb, starts, [read, b""], 12, 500, 5000, 500, 40, max_sec=3)
    assert [a.dtype for a in res] == [np.uint64, np.uint8, np.uint64, np.uint8, np.uint32, np.uint64, np.uint64, np.uint64] + [np.uint32] * 5
    assert len(res) == len(R.NAMES) and res[0].tolist() == [0, 2, 2] and res[2].tolist() == [2, 0]
    (mapq, _, rows), (mapq_empty, _, none) = R.per_read(res)
    # strand 1 first (600 bytes of record 4 = [12345, 20000), the read's first 600 bytes as given), then strand 0 (300 bytes of
    # record 2 = [1, 5000), the read's last 300); a MEM may run a few bytes further by chance
    (st1, q1, off1, ts1, te1, qs1, qe1, s1, n1, m1), (st2, q2, off2, ts2, te2, qs2, qe2, s2, n2, m2) = rows
    assert (st1, q1, qs1) == (1, 4, 0) and ts1 <= 13000 and 13600 <= te1 <= 13610 and off1 == ts1 - 12345 and 600 <= qe1 <= 610
    assert (st2, q2, qe2) == (0, 2, 900) and 1990 <= ts2 <= 2000 and te2 == 2300 and off2 == ts2 - 1 and 590 <= qs2 <= 600
    assert 600 <= s1 <= 610 and 300 <= s2 <= 310 and mapq == 60 * (s1 - s2) // s1 and 25 <= mapq <= 35
    assert (mapq_empty, none) == (0, [])
