"""`bin/bwtsearch --sam K` (host/bwtsearch.c) end to end: `bigbwt -f --seqs -s -e` on a multi-record FASTA (test_fm_seqs_cli.py's),
then reads from a line file, a FASTA (plain and gzip-compressed) and a FASTQ.  stdout must equal, byte for byte, what
map_reference.py formats - header, flags, 1-based POS, NM / MD / NH, secondary lines, unmapped lines - from the alignments
FmIndex.align lists for the reads and their reverse complements."""
import gzip
import shutil

import numpy as np
import pytest

import map_reference as M
from extend_reference import planted
from test_fm_seqs_cli import BIGBWT, BWTSEARCH, make_fasta, run

pytestmark = pytest.mark.gpu

K, SEED = 3, 14


@pytest.fixture(scope="module")
def built(ctx, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("map_cli")
    raw, names, seqs = make_fasta()
    assert not synth.first_window_triggers(b"".join(seqs)[:10], 10, 100)
    f = d / "c.fa"
    f.write_bytes(raw)
    out = run([BIGBWT, "-f", "--seqs", "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    tb = b"".join(seqs)
    text = np.frombuffer(tb, dtype=np.uint8)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    rng = np.random.default_rng(31)
    reads = []
    for q, m in enumerate((40, 60, 100, 100, 150, 150, 35, 80)):
        i = int(rng.integers(0, len(tb) - m + 1))
        r = planted(rng, tb[i:i + m], q % 4, sorted(set(tb)), at_ends=q % 3 == 0)
        reads.append(M.revcomp(r) if q % 2 else r)
    b = int(starts[3])
    reads += [tb[b - 1:b + 59], tb[b - 30:b + 30], b"", b"ACGT" * 10, b"NNNNNNNNNNNNNNNNNNNNNNNN", tb[5:9]]
    with ctx.fm_index_ms_files(str(f), text) as fm:
        assert fm.set_sequences_file(str(f) + ".seqs") == names
        fm.add_thresholds()
        want = {}
        for thresholds in (False, True):
            aln = fm.align(M.interleaved(reads), K, SEED, 0, thresholds)
            for max_sec in (0, 2):
                want[(thresholds, max_sec)] = M.map_reads(text, starts, reads, aln, K, max_sec)
    nh = want[(False, 2)][2]
    assert (nh == 0).any() and (nh > 1).any() and set(want[(False, 2)][3].tolist()) == {0, 1}
    return dict(dir=d, base=f, names=names, starts=starts, reads=reads, want=want)


def sam(b, qnames, reads, key):
    return M.sam_header(b["names"], b["starts"]) + M.sam_lines(b["names"], qnames, reads, b["want"][key])


def test_line_file(built):
    b = built
    reads = b["reads"]
    pf = b["dir"] / "reads.txt"
    pf.write_bytes(b"\n".join(reads) + b"\n")
    numbers = [b"%d" % (i + 1) for i in range(len(reads))]
    for thresholds, max_sec, env in ((False, 0, {}), (False, 2, {"PFP_FM_BATCH": "3"}), (True, 2, {"PFP_FM_BATCH": "1"}), (True, 0, {})):
        args = ["--sam", K, "--seed", SEED] + (["--secondary", max_sec] if max_sec else []) + (["--thresholds"] if thresholds else [])
        out = run([BWTSEARCH] + args + [pf, b["base"]], env=env)
        assert out.returncode == 0, out.stderr
        assert out.stdout == sam(b, numbers, reads, (thresholds, max_sec)), (thresholds, max_sec)
    lines = out.stdout.split(b"\n")
    assert lines[0] == b"@HD\tVN:1.6\tSO:unsorted" and sum(x.startswith(b"@SQ") for x in lines) == 39      # (one record is empty)
    assert b"11\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*" in lines                   # the empty line: unmapped, SEQ *


def fasta_of(reads, fastq):
    """the reads as records r0, r1, ... with a description behind the name; lower case in every third (the reader upper-cases)"""
    raw, names = b"", []
    for i, r in enumerate(reads):
        names.append(b"r%d" % i)
        body = r.lower() if i % 3 == 1 else r
        if fastq:
            raw += b"@r%d lane 1\n%s\n+\n%s\n" % (i, body, b"I" * len(r))
        else:
            raw += b">r%d some words\n" % i + b"".join(body[j:j + 50] + b"\n" for j in range(0, len(body), 50))
    return raw, names


def test_fasta_gzip_and_fastq(built):
    b = built
    every = b["reads"]
    for fastq in (False, True):
        keep = [i for i, r in enumerate(every) if r or not fastq]       # (the FASTQ file leaves the empty read out)
        raw, names = fasta_of([every[i] for i in keep], fastq)
        # the reference's lines of all reads, the kept ones under their record names; every read's answer is its own
        qnames = [b"-"] * len(every)
        for i, nm in zip(keep, names):
            qnames[i] = nm
        lines = M.sam_lines(b["names"], qnames, every, b["want"][(False, 2)]).split(b"\n")[:-1]
        want = M.sam_header(b["names"], b["starts"]) + b"".join(x + b"\n" for x in lines if not x.startswith(b"-\t"))
        pf = b["dir"] / ("reads.fq" if fastq else "reads.fa")
        pf.write_bytes(raw)
        out = run([BWTSEARCH, "--sam", K, "--seed", SEED, "--secondary", 2, pf, b["base"]], env={"PFP_FM_BATCH": "4"})
        assert out.returncode == 0, out.stderr
        assert out.stdout == want, fastq
        if not fastq:
            gz = b["dir"] / "reads.fa.gz"
            gz.write_bytes(gzip.compress(raw))
            again = run([BWTSEARCH, "--sam", K, "--seed", SEED, "--secondary", 2, gz, b["base"]])
            assert again.returncode == 0 and again.stdout == want


def test_refused_combinations_and_a_missing_table(built, tmp_path):
    b = built
    pf = b["dir"] / "reads.txt"
    pf.write_bytes(b"ACGT\n")
    for more in (["-l"], ["-k", 1], ["-m", 3], ["--ms"], ["--mems", 5], ["--docs"], ["--align", 2], ["--cigar"], ["--rc"]):
        out = run([BWTSEARCH, "--sam", K] + more + [pf, b["base"]])
        assert out.returncode != 0 and b"--sam does not combine" in out.stderr and not out.stdout.startswith(b"@HD"), more
    for args in (["--secondary", 2], ["--sam", 33], ["--sam", "x"], ["--sam", K, "--secondary", "-1"]):
        out = run([BWTSEARCH] + args + [pf, b["base"]])
        assert out.returncode == 2 and b"usage" in out.stdout, args
    g = tmp_path / "g"
    for ext in (".bwt", ".ssa", ".esa"):
        shutil.copy(str(b["base"]) + ext, str(g) + ext)
    out = run([BWTSEARCH, "--sam", K, pf, g])
    assert out.returncode == 1 and b"bigbwt -f --seqs" in out.stderr and b"g.seqs" in out.stderr and b"@HD" not in out.stdout
    out = run([BWTSEARCH, "--sam", K, "--seqs=" + str(b["base"]) + ".seqs", pf, g])
    assert out.returncode == 0 and out.stdout.startswith(b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:rec0\tLN:700\n")
    assert out.stdout.endswith(b"@PG\tID:bwtsearch\n1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n")
    help_ = run([BWTSEARCH, "-h"])
    assert help_.returncode == 0 and b"--sam" in help_.stdout and b"--secondary" in help_.stdout and b"qualities" in help_.stdout
