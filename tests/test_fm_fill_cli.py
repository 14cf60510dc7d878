"""`bin/bwtsearch --paf --cigar [--fill F]` (host/bwtsearch.c) end to end: `bigbwt -f --seqs -s -e` on a multi-record FASTA
(test_fm_seqs_cli.py's), then long reads from a line file.  Every line is parsed back against fill_reference.py's answer for the same
reads - the alignment in plain Python - and the whole output must equal fill_reference.paf_lines' formatting; `--paf` alone must
print what test_fm_chain_cli.py expects of it, byte for byte."""
import re

import numpy as np
import pytest

import chain_reference as R
import fill_reference as F
from chain_cases import with_substitutions
from map_reference import revcomp
from test_fm_seqs_cli import BIGBWT, BWTSEARCH, make_fasta, run

pytestmark = pytest.mark.gpu

SEED, OCC, GAP, BAND, SCORE = 15, 40, 300, 50, 30
ARGS = ["--paf", "--seed", SEED, "--max-occ", OCC, "--gap", GAP, "--band", BAND, "--min-score", SCORE]


@pytest.fixture(scope="module")
def built(ctx, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("fill_cli")
    raw, names, seqs = make_fasta()
    assert not synth.first_window_triggers(b"".join(seqs)[:10], 10, 100)
    f = d / "c.fa"
    f.write_bytes(raw)
    out = run([BIGBWT, "-f", "--seqs", "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    tb = b"".join(seqs)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    at = lambda k, i, m: tb[int(starts[k]) + i:int(starts[k]) + i + m]
    noisy = with_substitutions(at(3, 250, 120), 7, 6)                   # no seed of 15 bytes in it: one gap of 17 substitutions
    reads = [with_substitutions(at(3, 50, 500), 40), revcomp(with_substitutions(at(20, 0, 600), 33)), at(3, 100, 150) + noisy + at(3, 370, 150),
             revcomp(at(8, 100, 200) + b"GATTACAGATTACA" + at(8, 300, 50) + at(8, 360, 200)), b"", b"N" * 300, at(5, 0, 690)]
    want = {(table, max_sec, fill): F.map_long_aln(tb, starts if table else None, reads, SEED, OCC, GAP, BAND, SCORE, max_sec, fill)
            for table, max_sec, fill in ((True, 1, 500), (True, 2, 500), (False, 1, 500), (True, 1, 3))}
    assert want[(True, 1, 3)][16].any() and not want[(True, 1, 500)][16].any() and set(want[(True, 2, 500)][3].tolist()) == {0, 1}
    assert int(want[(True, 1, 500)][15].max()) >= 17
    return dict(dir=d, base=f, names=names, starts=starts, reads=reads, want=want, n=len(tb), text=np.frombuffer(tb, dtype=np.uint8))


def lines_of(b, qnames, table, max_sec, secondary, fill=500):
    names = [nm.decode() for nm in b["names"]] if table else None
    lines = F.paf_lines(names, b["starts"], b["n"], "c.fa", qnames, b["reads"], b["want"][(table, max_sec, fill)], secondary)
    return "".join(x + "\n" for x in lines).encode()


def check_lines(b, stdout, table, max_sec, secondary, fill=500):
    """every line parsed back: the columns against the reference's arrays, the script against the line's own coordinates"""
    res = b["want"][(table, max_sec, fill)]
    hit_off = [int(x) for x in res[0]]
    lines = [x.split("\t") for x in stdout.decode().split("\n")[:-1]]
    at = 0
    for p in range(len(b["reads"])):
        for h in range(hit_off[p], min(hit_off[p + 1], hit_off[p] + 1 + secondary)):
            ln = lines[at]
            at += 1
            strand, off, ts, te, qs, qe, aqs, ats, nm, unf = (int(res[k][h]) for k in (3, 5, 6, 7, 8, 9, 13, 14, 15, 16))
            assert ln[0] == str(p + 1) and ln[4] == "+-"[strand]
            assert (int(ln[2]), int(ln[3])) == ((qs, aqs) if strand else (aqs, qe)) and (int(ln[7]), int(ln[8])) == (off + ats - ts, off + te - ts)
            tags = dict(t.split(":", 1) for t in ln[12:])
            ops = [(int(n), o) for n, o in re.findall(r"(\d+)([=XID])", tags["cg"][2:])]
            assert "".join("%d%s" % x for x in ops) == tags["cg"][2:]
            assert int(ln[3]) - int(ln[2]) == sum(n for n, o in ops if o in "=XI") and int(ln[8]) - int(ln[7]) == sum(n for n, o in ops if o in "=XD")
            assert int(ln[9]) == sum(n for n, o in ops if o == "=") and int(ln[10]) == sum(n for n, o in ops)
            assert tags["NM"] == "i:%d" % nm == "i:%d" % sum(n for n, o in ops if o != "=")
            assert ("uf" in tags) == (unf > 0) and (not unf or tags["uf"] == "i:%d" % unf)
            assert list(tags)[-2 - (unf > 0):] == ["NM"] + (["uf"] if unf else []) + ["cg"]
    assert at == len(lines)


def test_cigar_lines(built):
    b = built
    pf = b["dir"] / "reads.txt"
    pf.write_bytes(b"\n".join(b["reads"]) + b"\n")
    numbers = [str(i + 1) for i in range(len(b["reads"]))]
    for table, secondary, fill, env in ((True, 0, 500, {}), (True, 2, 500, {"PFP_FM_BATCH": "2"}), (False, 0, 500, {"PFP_FM_BATCH": "1"}),
                                        (True, 0, 3, {})):
        args = ARGS + ["--cigar"] + (["--fill", fill] if fill != 500 else []) + (["--secondary", secondary] if secondary else []) + \
            (["--seqs"] if table else [])
        out = run([BWTSEARCH] + args + [pf, b["base"]], env=env)
        assert out.returncode == 0, out.stderr
        check_lines(b, out.stdout, table, max(secondary, 1), secondary, fill)
        assert out.stdout == lines_of(b, numbers, table, max(secondary, 1), secondary, fill), (table, secondary, fill)
    out = run([BWTSEARCH] + ARGS + ["--cigar", "--fill", 500, "--seqs", pf, b["base"]])                    # the default, spelled out
    assert out.returncode == 0 and out.stdout == lines_of(b, numbers, True, 1, 0)


def test_paf_alone_is_unchanged(built):
    """without --cigar: the lines test_fm_chain_cli.py expects (chain_reference.paf_lines over the reference's map_long)"""
    b = built
    pf = b["dir"] / "reads.txt"
    pf.write_bytes(b"\n".join(b["reads"]) + b"\n")
    numbers = [str(i + 1) for i in range(len(b["reads"]))]
    names = [nm.decode() for nm in b["names"]]
    for secondary in (0, 2):
        out = run([BWTSEARCH] + ARGS + (["--secondary", secondary] if secondary else []) + ["--seqs", pf, b["base"]])
        assert out.returncode == 0, out.stderr
        want = R.paf_lines(names, b["starts"], b["n"], "c.fa", numbers, b["reads"], b["want"][(True, max(secondary, 1), 500)][:13], secondary)
        assert out.stdout == "".join(x + "\n" for x in want).encode()
        assert b"cg:Z:" not in out.stdout and b"NM:i:" not in out.stdout


def test_fill_refusals(built):
    b = built
    pf = b["dir"] / "one.txt"
    pf.write_bytes(b"ACGT\n")
    for args in (["--paf", "--fill", 10], ["--cigar", "--fill", 10], ["--fill", 10], ["--align", 2, "--cigar", "--fill", 10],
                 ["--paf", "--cigar", "--fill", 4097], ["--paf", "--cigar", "--fill", -1], ["--paf", "--cigar", "--fill", "x"],
                 ["--paf", "--cigar", "--fill", ""]):
        out = run([BWTSEARCH] + args + [pf, b["base"]])
        assert out.returncode == 2 and not out.stdout.startswith(b"1\t"), args
    out = run([BWTSEARCH, "--paf", "--fill", 10, pf, b["base"]])
    assert b"--fill needs --paf --cigar" in out.stderr
    for more in (["-l"], ["--sam", 3], ["--align", 2], ["--rc"]):              # every other --paf refusal stays
        out = run([BWTSEARCH, "--paf", "--cigar"] + more + [pf, b["base"]])
        assert out.returncode in (1, 2) and b"\tcg:Z:" not in out.stdout, more
    for fill in (0, 4096):
        out = run([BWTSEARCH, "--paf", "--cigar", "--fill", fill, pf, b["base"]])          # a read shorter than the seed: no line
        assert out.returncode == 0 and out.stdout == b"", fill
