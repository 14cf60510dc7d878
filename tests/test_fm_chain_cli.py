"""`bin/bwtsearch --paf` (host/bwtsearch.c) end to end: `bigbwt -f --seqs -s -e` on a multi-record FASTA (test_fm_seqs_cli.py's),
then long reads from a line file and a FASTA.  Every line is parsed back and compared with what FmIndex.map_long returns for the
same reads (that call has its own tests: test_fm_chain.py); the whole output must equal chain_reference.paf_lines' formatting."""
import numpy as np
import pytest

import chain_reference as R
from chain_cases import with_substitutions
from map_reference import revcomp
from test_fm_seqs_cli import BIGBWT, BWTSEARCH, make_fasta, run

pytestmark = pytest.mark.gpu

SEED, OCC, GAP, BAND, SCORE = 15, 40, 300, 50, 30
ARGS = ["--paf", "--seed", SEED, "--max-occ", OCC, "--gap", GAP, "--band", BAND, "--min-score", SCORE]


@pytest.fixture(scope="module")
def built(ctx, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("chain_cli")
    raw, names, seqs = make_fasta()
    assert not synth.first_window_triggers(b"".join(seqs)[:10], 10, 100)
    f = d / "c.fa"
    f.write_bytes(raw)
    out = run([BIGBWT, "-f", "--seqs", "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    tb = b"".join(seqs)
    text = np.frombuffer(tb, dtype=np.uint8)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    at = lambda k, i, m: tb[int(starts[k]) + i:int(starts[k]) + i + m]
    reads = [with_substitutions(at(3, 50, 500), 40), revcomp(with_substitutions(at(20, 0, 600), 33)), at(8, 100, 250) + at(30, 300, 200),
             at(5, 0, 690), b"", b"ACGT" * 50, b"N" * 300, at(17, 200, 14), at(2, 650, 40) + at(3, 0, 40)]
    with ctx.fm_index_ms_files(str(f), text) as fm:
        want = {}
        for table in (False, True):
            if table:
                assert fm.set_sequences_file(str(f) + ".seqs") == names
            for max_sec in (1, 2):
                want[(table, max_sec)] = fm.map_long(reads, SEED, OCC, GAP, BAND, SCORE, max_sec)
    nc = want[(True, 2)][2]
    assert (nc == 0).any() and (nc > 2).any() and set(want[(True, 2)][3].tolist()) == {0, 1}
    return dict(dir=d, base=f, names=names, starts=starts, reads=reads, want=want, n=len(tb))


def paf(b, qnames, table, max_sec, secondary):
    names = [nm.decode() for nm in b["names"]] if table else None
    lines = R.paf_lines(names, b["starts"], b["n"], "c.fa", qnames, b["reads"], b["want"][(table, max_sec)], secondary)
    return "".join(x + "\n" for x in lines).encode()


def check_lines(b, stdout, table, secondary):
    """every line parsed back against map_long's arrays"""
    res = R.per_read(b["want"][(table, max(secondary, 1))])
    lines = [x.split("\t") for x in stdout.decode().split("\n")[:-1]]
    at = 0
    for p, (mq, nc, rows) in enumerate(res):
        for r, (strand, q, off, ts, te, qs, qe, score, cn, match) in enumerate(rows[:1 + secondary]):
            ln = lines[at]
            at += 1
            assert ln[0] == str(p + 1) and int(ln[1]) == len(b["reads"][p]) and (int(ln[2]), int(ln[3])) == (qs, qe) and ln[4] == "+-"[strand]
            if table:
                assert ln[5] == b["names"][q].decode() and int(ln[6]) == int(b["starts"][q + 1] - b["starts"][q])
            else:
                assert ln[5] == "c.fa" and int(ln[6]) == b["n"] and q == 0 and off == ts
            assert (int(ln[7]), int(ln[8])) == (off, off + te - ts) and int(ln[9]) == match and int(ln[10]) == max(qe - qs, te - ts)
            assert int(ln[11]) == (0 if r else mq) and 0 <= int(ln[11]) <= 60
            tags = dict(t.split(":", 1) for t in ln[12:])
            assert tags["tp"] == ("A:S" if r else "A:P") and tags["cm"] == "i:%d" % cn and tags["s1"] == "i:%d" % score
            assert ("s2" in tags) == (r == 0 and nc > 1) and (r or nc < 2 or tags["s2"] == "i:%d" % rows[1][7])
    assert at == len(lines)


def test_line_file(built):
    b = built
    pf = b["dir"] / "reads.txt"
    pf.write_bytes(b"\n".join(b["reads"]) + b"\n")
    numbers = [str(i + 1) for i in range(len(b["reads"]))]
    for table, secondary, env in ((True, 0, {}), (True, 2, {"PFP_FM_BATCH": "2"}), (False, 0, {"PFP_FM_BATCH": "1"}), (False, 2, {})):
        args = ARGS + (["--secondary", secondary] if secondary else []) + (["--seqs"] if table else [])
        out = run([BWTSEARCH] + args + [pf, b["base"]], env=env)
        assert out.returncode == 0, out.stderr
        check_lines(b, out.stdout, table, secondary)
        assert out.stdout == paf(b, numbers, table, max(secondary, 1), secondary), (table, secondary)
    first = [x.split(b"\t")[0] for x in out.stdout.split(b"\n")[:-1]]
    assert b"5" not in first and b"7" not in first           # the empty read and the N's: no chain, no line
    assert sum(x == b"1" for x in first) == 3                # --secondary 2: the primary and two more


def test_fasta_with_thresholds(built):
    b = built
    keep = [i for i, r in enumerate(b["reads"]) if r]
    raw = b"".join(b">r%d words\n%s\n" % (i, b["reads"][i].lower() if i % 2 else b["reads"][i]) for i in keep)
    pf = b["dir"] / "reads.fa"
    pf.write_bytes(raw)
    out = run([BWTSEARCH] + ARGS + ["--secondary", 2, "--thresholds", "--seqs=" + str(b["base"]) + ".seqs", pf, b["base"]])
    assert out.returncode == 0, out.stderr
    qnames = ["r%d" % i for i in range(len(b["reads"]))]
    assert out.stdout == paf(b, qnames, True, 2, 2)


def test_refused_combinations(built):
    b = built
    pf = b["dir"] / "one.txt"
    pf.write_bytes(b"ACGT\n")
    out = run([BWTSEARCH, "--paf", "--sam", 3, pf, b["base"]])
    assert out.returncode == 1 and b"usage" in out.stdout and b"--paf" in out.stdout
    for more in (["-l"], ["-k", 1], ["-m", 3], ["--ms"], ["--mems", 5], ["--docs"], ["--align", 2], ["--rc"]):
        out = run([BWTSEARCH, "--paf"] + more + [pf, b["base"]])
        assert out.returncode == 2 and b"--paf does not combine" in out.stderr and not out.stdout, more
    for args in (["--gap", 5], ["--paf", "--max-occ", 0], ["--paf", "--max-occ", 65537], ["--paf", "--gap", 0], ["--paf", "--band", "x"],
                 ["--paf", "--min-score", 0], ["--paf", "--seed", 0]):
        out = run([BWTSEARCH] + args + [pf, b["base"]])
        assert out.returncode == 2, args
    out = run([BWTSEARCH, "--paf", pf, b["base"]])          # a read shorter than the seed: no line
    assert out.returncode == 0 and out.stdout == b""
