"""`bin/bwtsearch --sam K --paired` and `-2 FILE` (host/bwtsearch.c) end to end, on the collection of test_fm_map_cli.py: read
pairs from an interleaved line file, from two line files, and from FASTQ files whose names end in /1 and /2.  stdout must equal,
byte for byte, what pair_reference.sam_lines_paired formats from pair_reference.map_pairs - which starts from FmIndex.map_reads
and window_reference.  Also the usage errors, and `--sam` without `--paired`, which must print what it printed before."""
import numpy as np
import pytest

import map_reference as M
import pair_cases as PC
import pair_reference as P
import window_reference as W
from extend_reference import planted
from test_fm_seqs_cli import BIGBWT, BWTSEARCH, make_fasta, run

pytestmark = pytest.mark.gpu

K, SEED, LO, HI, C = 8, 14, 100, 400, 4


@pytest.fixture(scope="module")
def built(ctx, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs_cli")
    raw, names, seqs = make_fasta()
    f = d / "c.fa"
    f.write_bytes(raw)
    out = run([BIGBWT, "-f", "--seqs", "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    tb = b"".join(seqs)
    text = np.frombuffer(tb, dtype=np.uint8)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    rng = np.random.default_rng(41)
    pairs = []
    for q, (F, m) in enumerate(((300, 60), (250, 50), (380, 80), (401, 60), (150, 40), (300, 100))):
        i = int(starts[3 * q + 1]) + int(rng.integers(0, 200))
        a, b = PC.ends(tb, i, F, m)
        a, b = planted(rng, a, q % 3, b"ACGT", q % 2 == 0), planted(rng, b, (q + 1) % 3, b"ACGT", q % 2 == 1)
        pairs.append((b, a) if q % 2 else (a, b))
    a, b = PC.ends(tb, int(starts[20]) + 100, 320, 60, 40)
    pairs += [(a, PC.every_tenth(b)), (PC.every_tenth(b), a), (tb[900:960], b"N" * 30), (b"", b"ACGTACGTAC" * 3), (b"NNNNNNNNNNNNNNNNNNNNNN", b""),
              (tb[int(starts[5]) - 80:int(starts[5]) - 20], M.revcomp(tb[int(starts[5]) + 100:int(starts[5]) + 160]))]
    reads = [r for p in pairs for r in p]
    pats = M.interleaved(reads)
    with ctx.fm_index_ms_files(str(f), text) as fm:
        assert fm.set_sequences_file(str(f) + ".seqs") == names
        res = fm.map_reads(reads, K, SEED, C - 1)
        single = M.map_reads(text, starts, reads, fm.align(pats, K, SEED), K, 0)
    want = P.map_pairs(text, starts, reads, res, lambda r, strand, lo, hi: W.window_one(text, pats[2 * r + strand], lo, hi, K), K, LO, HI, C)
    per = P.per_pair_read(want)
    assert {x[0] for x in per} == {0, 1} and {x[2] for x in per} == {0, 1} and any(x[3] for x in per) and {x[6] for x in per} == {0, 1}
    return dict(dir=d, base=f, names=names, starts=starts, reads=reads, want=want, single=single)


def sam(b, qnames):
    return M.sam_header(b["names"], b["starts"]) + P.sam_lines_paired(b["names"], qnames, b["reads"], b["want"])


ARGS = ["--sam", K, "--seed", SEED, "--ins", "%d:%d" % (LO, HI), "--anchors", C]


def test_line_files(built):
    b = built
    reads = b["reads"]
    both, one, two = (b["dir"] / x for x in ("both.txt", "one.txt", "two.txt"))
    both.write_bytes(b"\n".join(reads) + b"\n")
    one.write_bytes(b"\n".join(reads[0::2]) + b"\n")
    two.write_bytes(b"\n".join(reads[1::2]))              # (the last line has no end)
    for env in ({}, {"PFP_FM_BATCH": "3"}, {"PFP_FM_BATCH": "2"}):
        out = run([BWTSEARCH] + ARGS + ["--paired", both, b["base"]], env=env)
        assert out.returncode == 0, out.stderr
        assert out.stdout == sam(b, [b"%d" % (r + 1) for r in range(len(reads))]), env       # a read's name: its line number
    out = run([BWTSEARCH] + ARGS + ["-2", two, one, b["base"]], env={"PFP_FM_BATCH": "5"})
    assert out.returncode == 0, out.stderr
    assert out.stdout == sam(b, [b"%d" % (r // 2 + 1) for r in range(len(reads))])
    lines = out.stdout.split(b"\n")
    assert sum(not x.startswith(b"@") for x in lines[:-1]) == len(reads) and any(x.endswith(b"\tYR:i:1") for x in lines)


def test_fastq_names(built):
    """@p3/1 and @p3/2 become p3; a pair whose names do not end so keeps mate 1's name for both"""
    b = built
    reads = b["reads"]
    keep = [q for q in range(len(reads) // 2) if reads[2 * q] and reads[2 * q + 1]]        # (FASTQ holds no empty read)
    name = lambda q, t: (b"p%d/%d" % (q, t + 1)) if q % 3 else (b"p%d.%s" % (q, b"ab"[t:t + 1]))
    fq = [b"".join(b"@%s lane 1\n%s\n+\n%s\n" % (name(q, t), reads[2 * q + t], b"I" * len(reads[2 * q + t])) for q in keep) for t in (0, 1)]
    qnames = [b"-"] * len(reads)
    for q in keep:
        qnames[2 * q], qnames[2 * q + 1] = name(q, 0), name(q, 1)
    lines = P.sam_lines_paired(b["names"], qnames, reads, b["want"]).split(b"\n")[:-1]
    want = M.sam_header(b["names"], b["starts"]) + b"".join(x + b"\n" for x in lines if not x.startswith(b"-\t"))
    assert b"\np1\t" in want and b"\np3.a\t" in want and b"p1/1" not in want
    one, two, both = (b["dir"] / x for x in ("one.fq", "two.fq", "both.fq"))
    one.write_bytes(fq[0])
    two.write_bytes(fq[1])
    both.write_bytes(b"".join(b"@%s\n%s\n+\n%s\n" % (name(q, t), reads[2 * q + t], b"I" * len(reads[2 * q + t])) for q in keep for t in (0, 1)))
    out = run([BWTSEARCH] + ARGS + ["-2", two, one, b["base"]])
    assert out.returncode == 0 and out.stdout == want, out.stderr
    out = run([BWTSEARCH] + ARGS + ["--paired", both, b["base"]], env={"PFP_FM_BATCH": "4"})
    assert out.returncode == 0 and out.stdout == want, out.stderr


def test_usage_errors(built):
    b = built
    one, odd = b["dir"] / "u1.txt", b["dir"] / "u3.txt"
    one.write_bytes(b"ACGT\nACGT\n")
    odd.write_bytes(b"ACGT\nACGT\nACGT\n")
    for more in (["--paired", "--secondary", 2], ["-2", one, "--secondary", 1], ["--ins", "0:500", "--paired", "--secondary", 1]):
        out = run([BWTSEARCH, "--sam", K] + more + [one, b["base"]])
        assert out.returncode == 2 and b"--secondary" in out.stderr and not out.stdout.startswith(b"@HD"), more
    for args in (["--paired"], ["-2", one], ["--ins", "0:500"], ["--anchors", 4], ["--align", 2, "--paired"]):
        out = run([BWTSEARCH] + args + [one, b["base"]])
        assert out.returncode == 2 and b"need --sam" in out.stderr, args
    for args in (["--ins", "500:100"], ["--ins", "100"], ["--ins", "0:16385"], ["--ins", "-1:5"], ["--anchors", 0], ["--anchors", 65], ["--anchors", "x"]):
        out = run([BWTSEARCH, "--sam", K, "--paired"] + args + [one, b["base"]])
        assert out.returncode == 2 and b"usage" in out.stdout, args
    out = run([BWTSEARCH, "--sam", K, "--ins", "0:500", one, b["base"]])
    assert out.returncode == 2 and b"--paired" in out.stderr
    out = run([BWTSEARCH, "--sam", K, "-2", odd, one, b["base"]])
    assert out.returncode == 1 and b"holds 2 reads" in out.stderr and b"holds 3:" in out.stderr and b"@HD" not in out.stdout
    out = run([BWTSEARCH, "--sam", K, "--paired", odd, b["base"]])
    assert out.returncode == 1 and b"even number" in out.stderr and b"@HD" not in out.stdout
    help_ = run([BWTSEARCH, "-h"])
    assert help_.returncode == 0 and all(x in help_.stdout for x in (b"--paired", b"-2 FILE", b"--ins MIN:MAX", b"--anchors C", b"YR:i:1"))


def test_single_end_output_is_unchanged(built):
    """--sam without --paired on the same reads: what map_reference.sam_lines formats, as in test_fm_map_cli.py"""
    b = built
    reads = b["reads"]
    pf = b["dir"] / "single.txt"
    pf.write_bytes(b"\n".join(reads) + b"\n")
    out = run([BWTSEARCH, "--sam", K, "--seed", SEED, pf, b["base"]], env={"PFP_FM_BATCH": "5"})
    assert out.returncode == 0, out.stderr
    numbers = [b"%d" % (i + 1) for i in range(len(reads))]
    assert out.stdout == M.sam_header(b["names"], b["starts"]) + M.sam_lines(b["names"], numbers, reads, b["single"])
