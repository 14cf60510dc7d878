"""`bigbwt -f --seqs` and `bwtsearch --seqs / --docs / --rc` end to end on a multi-FASTA, every output line against
tests/seq_reference.py (occurrences by bytes.find, put in row order by the oracle's suffix array)."""
import os
import subprocess

import numpy as np
import pytest

import seq_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "big-bwt_amd")
BIGBWT = os.path.join(PKG, "bigbwt")
BWTSEARCH = os.path.join(PKG, "bin", "bwtsearch")


def run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([str(c) for c in cmd], capture_output=True, timeout=timeout, env=e)


def make_fasta():
    """40 records of one mutated genome: lower case in some, CRLF in some, one empty record, a name with a ':'.  (The seed: the
    text's first window must not be a trigger - SURVEY 2.2-Q1, the builder then writes, as the reference does, bytes that are not a
    BWT, which no index accepts; `built` asserts it.)"""
    rng = np.random.default_rng(22)
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 700)
    raw, names, seqs = b"", [], []
    for k in range(40):
        g = genome.copy()
        hit = rng.random(len(g)) < 0.01
        g[hit] = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(hit.sum()))
        s = g[: 700 - 3 * k].tobytes()
        name = b"chr:%d" % k if k == 7 else b"rec%d" % k
        if k == 11:
            s = b""
        body = s.lower() if k % 5 == 2 else s
        eol = b"\r\n" if k % 4 == 1 else b"\n"
        raw += b">" + name + b" sample %d" % k + eol + b"".join(body[i:i + 60] + eol for i in range(0, len(body), 60))
        names.append(name)
        seqs.append(s)
    return raw, names, seqs


@pytest.fixture(scope="module")
def built(O, synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("seqs_cli")
    raw, names, seqs = make_fasta()
    assert not synth.first_window_triggers(b"".join(seqs)[:10], 10, 100)
    f = d / "c.fa"
    f.write_bytes(raw)
    text = b"".join(seqs)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    rng = np.random.default_rng(4)
    pats = [b"", b"A", b"ACGT", b"ZZZ", text[:30]]
    for b in starts[1:8]:                         # cut from the text across a border
        b = int(b)
        pats += [text[b - 4:b + 4], text[b - 1:b + 1], text[b - 12:b]]
    for m in (6, 15, 40):
        for _ in range(8):
            i = int(rng.integers(0, len(text) - m))
            pats.append(text[i:i + m])
    pats += [R.reverse_complement(p) for p in pats[-6:]]
    pf = d / "pats"
    pf.write_bytes(b"\n".join(pats) + b"\n")
    sa = np.concatenate([[len(text)], O.sacak(np.frombuffer(text, dtype=np.uint8))]).astype(np.int64)
    rank = np.zeros(len(text) + 1, dtype=np.int64)
    rank[sa] = np.arange(len(sa))
    return dict(dir=d, fasta=f, names=names, seqs=seqs, text=text, starts=starts, pats=pats, patfile=pf, rank=rank)


def rows_in_suffix_order(b, pat):
    """the positions of pat in row order: by the rank of the suffixes that start there"""
    occ = R.occurrences_find(b["text"], pat)
    return occ[np.argsort(b["rank"][occ.astype(np.int64)])]


def want_locate(b, pats, max_occ=0):
    out = []
    for p in pats:
        rows = rows_in_suffix_order(b, p)
        seq, off = R.locate_seqs(b["starts"], rows, len(p), max_occ)
        out.append("%d\t%s" % (len(rows), " ".join("%s:%d" % (b["names"][s].decode(), o) for s, o in zip(seq, off))))
    return out


def want_docs(b, pats):
    out = []
    for p in pats:
        docs, cnt = R.doclist(b["starts"], R.occurrences_find(b["text"], p), len(p))
        out.append("%d\t%s" % (len(docs), " ".join("%s:%d" % (b["names"][d].decode(), c) for d, c in zip(docs, cnt))))
    return out


def test_seqs_needs_fasta_mode(tmp_path):
    f = tmp_path / "x"
    f.write_bytes(b"ACGT" * 100)
    out = run([BIGBWT, "--seqs", f])
    assert out.returncode == 2 and b"usage" in out.stdout
    assert not os.path.exists(str(f) + ".seqs") and not os.path.exists(str(f) + ".bwt")
    out = run([BIGBWT, "-h"])
    assert out.returncode == 0 and b"--seqs" in out.stdout
    out = run([BWTSEARCH, "-h"])
    assert out.returncode == 0 and b"--seqs" in out.stdout and b"--docs" in out.stdout and b"--rc" in out.stdout and b"span" in out.stdout
    for args in (["--docs", "-l", "p", "b"], ["--docs", "-m", "3", "p", "b"], ["--ms", "--seqs", "p", "b"], ["--mems", "3", "--docs", "p", "b"]):
        out = run([BWTSEARCH] + args)
        assert out.returncode == 2 and b"usage" in out.stdout, args


@pytest.mark.gpu
def test_build_and_search(built):
    b = built
    f, pf, pats = b["fasta"], b["patfile"], b["pats"]
    # without --seqs: no table, and the same .bwt as with it
    out = run([BIGBWT, "-f", "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    assert not os.path.exists(str(f) + ".seqs")
    bwt0 = open(str(f) + ".bwt", "rb").read()
    out = run([BIGBWT, "-f", "-s", "-e", "--seqs", f])
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(str(f) + ".bwt", "rb").read() == bwt0 and len(bwt0) == len(b["text"]) + 1
    want = [b"%s\t%d\t%d" % (nm, st, len(s)) for nm, st, s in zip(b["names"], b["starts"], b["seqs"])]
    assert open(str(f) + ".seqs", "rb").read().split(b"\n") == want + [b""]
    assert want[7].startswith(b"chr:7\t") and want[11].endswith(b"\t0")
    # the reference has something to say: hits inside a sequence, and occurrences that span a border
    kept = sum(int(R.keep(b["starts"], R.occurrences_find(b["text"], p), len(p)).sum()) for p in pats)
    total = sum(len(R.occurrences_find(b["text"], p)) for p in pats) - 1           # (position n of the empty pattern)
    assert kept >= 1 and total - kept >= 1

    for env in ({}, {"PFP_FM_BATCH": "4"}, {"PFP_FM_SEQ_BUDGET": "50"}):
        out = run([BWTSEARCH, "-l", "--seqs", pf, f], env=env)
        assert out.returncode == 0, out.stderr
        assert out.stdout.decode().splitlines() == want_locate(b, pats), env
    out = run([BWTSEARCH, "-l", "--seqs", "-m", "3", pf, f])
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == want_locate(b, pats, 3)
    for env in ({}, {"PFP_FM_BATCH": "5"}):
        out = run([BWTSEARCH, "--docs", pf, f], env=env)
        assert out.returncode == 0, out.stderr
        assert out.stdout.decode().splitlines() == want_docs(b, pats), env
    # the offset is what follows the last ':'
    line = [ln for ln in want_locate(b, pats) if "chr:7:" in ln][0]
    hit = [h for h in line.split("\t")[1].split(" ") if h.startswith("chr:7:")][0]
    assert hit.rsplit(":", 1)[0] == "chr:7" and hit.rsplit(":", 1)[1].isdigit()

    # --rc: every line as given, then its reverse complement
    both = [q for p in pats for q in (p, R.reverse_complement(p))]
    out = run([BWTSEARCH, "--rc", pf, f])
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == [str(len(R.occurrences_find(b["text"], q))) for q in both]
    out = run([BWTSEARCH, "--rc", "-l", "--seqs", pf, f], env={"PFP_FM_BATCH": "3"})
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == want_locate(b, both)
    out = run([BWTSEARCH, "--rc", "--docs", pf, f])
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == want_docs(b, both)
    out = run([BWTSEARCH, "--rc", "-l", pf, f])                 # plain locate: positions in the concatenation
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == ["%d\t%s" % (len(r), " ".join(str(int(x)) for x in r))
                                                for r in (rows_in_suffix_order(b, q) for q in both)]
    # an explicit table file
    alt = b["dir"] / "alt.seqs"
    alt.write_bytes(b"all\t0\t%d\n" % len(b["text"]))
    out = run([BWTSEARCH, "--docs", "--seqs=" + str(alt), pf, f])
    assert out.returncode == 0, out.stderr
    lines = out.stdout.decode().splitlines()
    assert lines[1] == "1\tall:%d" % b["text"].count(b"A") and lines[3] == "0\t"


@pytest.mark.gpu
def test_exit_codes(built, tmp_path):
    b = built
    f, pf = b["fasta"], b["patfile"]
    if not os.path.exists(str(f) + ".bwt"):
        assert run([BIGBWT, "-f", "-s", "-e", "--seqs", f]).returncode == 0
    g = tmp_path / "g"
    for ext in (".bwt", ".ssa", ".esa"):
        (tmp_path / ("g" + ext)).write_bytes(open(str(f) + ext, "rb").read())
    for args in (["--docs"], ["-l", "--seqs"], ["--seqs"]):             # no g.seqs
        out = run([BWTSEARCH] + args + [pf, g])
        assert out.returncode == 1 and b"g.seqs" in out.stderr, args
    out = run([BWTSEARCH, "--docs", "--seqs=" + str(tmp_path / "nothing"), pf, g])
    assert out.returncode == 1 and b"nothing" in out.stderr
    n = len(b["text"])
    (tmp_path / "g.seqs").write_bytes(b"a\t0\t100\nb\t100\n")          # malformed
    out = run([BWTSEARCH, "--docs", pf, g])
    assert out.returncode == 1 and b"line 2" in out.stderr
    (tmp_path / "g.seqs").write_bytes(b"a\t0\t100\nb\t101\t%d\n" % (n - 101))
    out = run([BWTSEARCH, "-l", "--seqs", pf, g])
    assert out.returncode == 1 and b"line 2" in out.stderr
    (tmp_path / "g.seqs").write_bytes(b"a\t0\t100\nb\t100\t%d\n" % (n - 99))      # a table of another length
    out = run([BWTSEARCH, "--docs", pf, g])
    assert out.returncode == 1 and b"sum to" in out.stderr
    (tmp_path / "g.seqs").write_bytes(b"a\t0\t100\nb\t100\t%d\n" % (n - 100))
    out = run([BWTSEARCH, "--docs", pf, g])
    assert out.returncode == 0, out.stderr
    out = run([BWTSEARCH, pf, g])                                       # the plain modes never look for a table
    assert out.returncode == 0
