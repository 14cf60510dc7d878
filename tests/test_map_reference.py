"""CPU: the reference of the read-mapping tests (map_reference.py) checked against itself and against literals.

  MD: T[s..e) rebuilt from the strand's pattern, the script and the MD string alone equals the text's span - for random (pattern,
  span) pairs and for the shapes that go wrong first: adjacent mismatches, a deletion followed by a mismatch, D .. I .. D.
  Shadowing: the definition over all pairs equals the sorted-window method on random interval sets, tandem sets included.
  MAPQ and the SAM formatter against literals.
  The sanity condition of test_fm_map.py on `dna`, confirmed here with the CPU references alone (ms_reference for the MEMs,
  extend_reference.align for the alignments, map_reference for the hits) for the generator seed map_cases.SANITY_SEED."""
import re

import numpy as np

import approx_reference as R
import cigar_reference as G
import extend_reference as E
import map_cases as K
import map_reference as M
import ms_reference as MS


def check_md(text, pat, s, e, k):
    d, runs = G.script(text, pat, s, e, k)
    assert d != G.NONE
    md = M.md_of(text, runs, s)
    assert M.rebuild_span(pat, runs, md) == bytes(bytearray(text[s:e].tolist())), (pat, s, e, G.cigar_string(runs), md)
    return G.cigar_string(runs), md


def test_md_rebuilds_the_span_random():
    rng = np.random.default_rng(11)
    seen = set()
    for alphabet in (b"ACGT", b"ab", b"0123^A"):           # (digits and ^ as text bytes: the walk tells them from the counts)
        text = np.frombuffer(bytes(rng.choice(list(alphabet), 3000).astype(np.uint8)), dtype=np.uint8)
        for q in range(60):
            L = int(rng.integers(0, 120))
            s = int(rng.integers(0, len(text) - L + 1))
            pat = E.planted(rng, text[s:s + L].tobytes(), q % 7, sorted(set(alphabet)), at_ends=q % 2 == 0)
            k = 7 + abs(len(pat) - L)
            cs, _ = check_md(text, pat, s, s + L, k)
            seen |= set(re.findall(r"[=XID]", cs))
    assert seen == set("=XID")


def test_md_shapes():
    t = np.frombuffer(b"ACGTACGTAC" + b"GGTTGACCAT" + b"CATCATGATC" + b"AAGTGTCTGT" + b"TTTTTTTTTT", dtype=np.uint8)
    tb = t.tobytes()
    # adjacent mismatches
    cs, md = check_md(t, tb[:4] + b"TA" + tb[6:20], 0, 20, 4)
    assert cs == "4=2X14=" and md == b"4A0C14"
    # a mismatch at either end
    cs, md = check_md(t, b"C" + tb[1:19] + b"A", 0, 20, 4)
    assert cs == "1X18=1X" and md == b"0A18T0"
    # a deletion followed by a mismatch
    cs, md = check_md(t, tb[:10] + b"A" + tb[13:30], 0, 30, 4)
    assert cs == "10=2D1X17=" and md == b"10^GG0T17"
    # D .. I .. D
    pat = tb[:10] + tb[12:25] + b"CC" + tb[25:30] + tb[32:50]
    cs, md = check_md(t, pat, 0, 50, 8)
    assert re.sub(r"\d+|=", "", cs) == "DID" and md == b"10^GG18^AA18", (cs, md)
    # nothing but insertions, the empty span, the empty pattern
    assert check_md(t, b"ACGT", 3, 3, 4) == ("4I", b"0")
    assert check_md(t, b"", 3, 3, 0) == ("*", b"0")
    assert check_md(t, b"", 3, 5, 2) == ("2D", b"0^TA0")


def random_candidates(rng, m, k, count, spread, tandem):
    out = []
    for q in range(count):
        s = 10 + (q * int(rng.integers(1, 4)) if tandem else int(rng.integers(0, spread)))
        out.append((int(rng.integers(0, k + 1)), int(rng.integers(0, 2)), s, s + m + int(rng.integers(-k, k + 1))))
    return out


def test_shadowing_by_pairs_equals_the_sorted_window():
    rng = np.random.default_rng(5)
    nonempty = 0
    for trial in range(300):
        m, k = int(rng.integers(1, 60)), int(rng.integers(0, 9))
        starts = [0, 0, 40, 41, 200, 100000] if trial % 3 else [0, 100000]
        cands = random_candidates(rng, m, k, int(rng.integers(0, 40)), int(rng.integers(1, 400)), trial % 4 == 0)
        cands += cands[:3]                                  # (the same triple twice: neither copy is below the other)
        a, b = M.hits_of(starts, cands), M.hits_by_window(starts, cands, m, k)
        assert a == b, (trial, cands)
        nonempty += bool(a)
        for h in a:
            assert M.is_inside(starts, h[2], h[3])
    assert nonempty > 200
    # not transitive: (0, 10..20) shadows (1, 15..30), which still shadows (2, 25..40)
    assert M.hits_of([0, 100], [(0, 0, 10, 20), (1, 0, 15, 30), (2, 0, 25, 40)]) == [(0, 0, 10, 20)]
    # a read that equals its own reverse complement: the second copy goes
    assert M.hits_of([0, 100], [(0, 0, 10, 50), (0, 1, 10, 50)]) == [(0, 0, 10, 50)]
    # empty spans and spans over a boundary are no candidates at all: they shadow nothing
    assert M.hits_of([0, 30, 100], [(0, 0, 25, 35), (0, 0, 28, 28), (1, 0, 26, 30)]) == [(1, 0, 26, 30)]


def test_mapq_table():
    table = {(): 0, (0,): 60, (3,): 60, (0, 0): 0, (2, 2, 5): 0, (0, 1): 10, (1, 2, 2): 10, (0, 3): 30, (0, 6): 60, (0, 7): 60, (1, 9, 9): 60,
             (4, 5, 4): 0, (0, 2, 1): 10}
    for dists, want in table.items():
        assert M.mapq_of(list(dists)) == want, dists


def test_sam_lines():
    names, starts = [b"chrA", b"empty", b"chr:B"], [0, 100, 100, 250]
    assert M.sam_header(names, starts) == b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrA\tLN:100\n@SQ\tSN:chr:B\tLN:150\n@PG\tID:bwtsearch\n"
    reads = [b"ACGTTGCA", b"GGGG", b"AACC"]
    u64 = lambda *a: np.array(a, dtype=np.uint64)
    u8 = lambda *a: np.array(a, dtype=np.uint8)
    cig = np.array([8 << 4 | 7, 2 << 4 | 7, 1 << 4 | 8, 1 << 4 | 7, 1 << 4 | 7, 1 << 4 | 2, 2 << 4 | 7, 1 << 4 | 1, 1 << 4 | 7], dtype=np.uint32)
    md = np.frombuffer(b"8" + b"2T1" + b"1^G2", dtype=np.uint8)
    res = (u64(0, 1, 1, 3), u8(60, 0, 10), u64(1, 0, 3), u8(0, 1, 0), np.array([0, 2, 2], dtype=np.uint32), u64(4, 0, 149), u64(4, 100, 249), u8(0, 1, 2),
           u64(0, 1, 4, 9), cig, u64(0, 1, 4, 8), md)
    want = (b"r1\t0\tchrA\t5\t60\t8=\t*\t0\t0\tACGTTGCA\t*\tNM:i:0\tMD:Z:8\tNH:i:1\n"
            b"r2\t4\t*\t0\t0\t*\t*\t0\t0\tGGGG\t*\n"
            b"r3\t16\tchr:B\t1\t10\t2=1X1=\t*\t0\t0\tGGTT\t*\tNM:i:1\tMD:Z:2T1\tNH:i:3\n"
            b"r3\t256\tchr:B\t150\t0\t1=1D2=1I1=\t*\t0\t0\tAACC\t*\tNM:i:2\tMD:Z:1^G2\tNH:i:3\n")
    assert M.sam_lines(names, [b"r1", b"r2", b"r3"], reads, res) == want


def test_reverse_complement_and_inside():
    assert M.revcomp(b"ACGTNacgtn-") == b"-nacgtNACGT" and M.revcomp(b"") == b""
    assert M.interleaved([b"AAC", "G"]) == [b"AAC", b"GTT", b"G", b"C"]
    starts = [0, 0, 5, 5, 6, 10]
    assert [M.seq_of(starts, x) for x in (0, 4, 5, 6, 9)] == [1, 1, 3, 4, 4]
    assert M.is_inside(starts, 0, 5) and not M.is_inside(starts, 0, 6) and M.is_inside(starts, 5, 6) and not M.is_inside(starts, 5, 7)
    assert not M.is_inside(starts, 3, 3) and M.is_inside(starts, 6, 10)


def test_the_sanity_condition_holds_for_the_reference_alone(O):
    """every read of map_cases.sanity_reads has, by the CPU references alone, a primary on the planted strand that overlaps the
    planted span, with MAPQ 60; and no seed string of at least 20 bytes repeats in `dna`"""
    text = K.text_of("dna")
    tb = text.tobytes()
    sa = R.full_sa(O, text)
    starts = K.starts_of("dna", "records")
    planted = K.sanity_reads()
    reads = [r for r, _, _ in planted]
    pats = M.interleaved(reads)
    mem_off, mems = [0], []
    for pat in pats:
        for i, ln in MS.mems_from_lengths(MS.ms_lengths(tb, sa, pat), 20):
            pos = tb.find(pat[i:i + ln])
            assert pos >= 0 and tb.find(pat[i:i + ln], pos + 1) < 0, "a seed string repeats: pick another generator seed"
            mems.append((i, ln, pos))
        mem_off.append(len(mems))
    aln = E.align(text, pats, mem_off, np.array(mems, dtype=np.uint64).reshape(-1, 3), 8)
    res = M.per_read(M.map_reads(text, starts, reads, aln, 8))
    assert len(res) == 16
    for (mq, nh, hits), (_, strand, i) in zip(res, planted):
        assert nh >= 1 and mq == 60, (mq, nh, i)
        h = hits[0]
        end = h[3] + sum(int(r) >> 4 for r in h[5] if int(r) & 15 != G.OP_I)         # (every run but I consumes text)
        assert h[0] == strand and max(h[3], i) < min(end, i + 100), (h, strand, i)
