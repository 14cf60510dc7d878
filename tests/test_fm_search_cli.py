"""`bin/bwtsearch` (host/bwtsearch.c): count / locate the lines of a pattern file through basename.bwt (.ssa / .esa)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "big-bwt_amd")
BIGBWT = os.path.join(PKG, "bigbwt")
BWTSEARCH = os.path.join(PKG, "bin", "bwtsearch")


def run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([str(c) for c in cmd], capture_output=True, timeout=timeout, env=e)


def test_usage_and_exit_codes(tmp_path):
    assert os.access(BWTSEARCH, os.X_OK)
    out = run([BWTSEARCH, "-h"])
    assert out.returncode == 0 and b"usage" in out.stdout and b"-l" in out.stdout
    for args in ([], [tmp_path / "p"], ["-m"], ["-m", "x", "p", "b"], ["-m", "-3", "p", "b"], ["-q", "p", "b"], ["p", "b", "c"]):
        out = run([BWTSEARCH] + args)
        assert out.returncode == 2 and b"usage" in out.stdout, args


@pytest.fixture(scope="module")
def built(O, tmp_path_factory):
    d = tmp_path_factory.mktemp("cli")
    text = O.gen_fasta(100_000, 4, 0.002, 9)
    f = d / "t"
    f.write_bytes(text.tobytes())
    out = run([BIGBWT, "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    rng = np.random.default_rng(1)
    tb = text.tobytes()
    pats = [b"", b"A", b"ACGT", tb[:20], b"ZZZ", b"A\x00C", b"A\rC", tb[-7:], b"\xff\xfe"]
    for m in (5, 12, 40, 200):
        for _ in range(6):
            i = int(rng.integers(0, len(tb) - m))
            pats.append(tb[i:i + m])
    pats = [p.replace(b"\n", b"N") for p in pats]          # (a line holds no newline)
    pats.append(b"A")                                       # the last line occurs: its final '\n' must not become part of it
    pf = d / "pats"
    pf.write_bytes(b"\n".join(pats) + b"\n")
    return text, f, pf, pats


@pytest.mark.gpu
def test_cli_matches_the_api(pkg, ctx, built):
    text, f, pf, pats = built
    with ctx.fm_index_files(str(f), pkg.FLAG_SSA | pkg.FLAG_ESA) as fm:
        off, pos, sp, ep = fm.locate(pats, max_occ=5, ranges=True)
        offa, posa = fm.locate(pats)
    cnt = (ep - sp).astype(np.int64)
    out = run([BWTSEARCH, pf, f])
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == [str(c) for c in cnt]
    for env in ({}, {"PFP_FM_BATCH": "4"}):
        out = run([BWTSEARCH, "-l", pf, f], env=env)
        assert out.returncode == 0, out.stderr
        want = ["%d\t%s" % (cnt[k], " ".join(str(int(x)) for x in posa[offa[k]:offa[k + 1]])) for k in range(len(pats))]
        assert out.stdout.decode().splitlines() == want
    out = run([BWTSEARCH, "-l", "-m", "5", pf, f], env={"PFP_FM_BATCH": "3"})
    assert out.returncode == 0, out.stderr
    want = ["%d\t%s" % (cnt[k], " ".join(str(int(x)) for x in pos[off[k]:off[k + 1]])) for k in range(len(pats))]
    assert out.stdout.decode().splitlines() == want
    assert cnt[-1] > 0 and out.stdout.decode().splitlines()[-1].startswith("%d\t" % cnt[-1])
    # with and without a final newline, the last line is the same pattern; an empty line in between is the empty pattern
    for body in (b"ACGT\nA", b"ACGT\nA\n"):
        p2 = pf.parent / "p2"
        p2.write_bytes(body)
        out = run([BWTSEARCH, p2, f])
        assert out.returncode == 0 and out.stdout.decode().splitlines() == [str(cnt[2]), str(cnt[1])], body
    p2.write_bytes(b"ACGT\n\nA\n")
    out = run([BWTSEARCH, p2, f])
    assert out.returncode == 0 and out.stdout.decode().splitlines() == [str(cnt[2]), str(cnt[0]), str(cnt[1])]


@pytest.mark.gpu
def test_cli_missing_files(built, tmp_path):
    text, f, pf, pats = built
    g = tmp_path / "g"
    for ext in (".bwt", ".ssa"):
        (tmp_path / ("g" + ext)).write_bytes(open(str(f) + ext, "rb").read())
    out = run([BWTSEARCH, pf, g])                          # count needs the .bwt only
    assert out.returncode == 0
    out = run([BWTSEARCH, "-l", pf, g])
    assert out.returncode == 1 and b"g.esa" in out.stderr
    out = run([BWTSEARCH, pf, tmp_path / "nothing"])
    assert out.returncode == 1
    (tmp_path / "bad.bwt").write_bytes(b"ab\x00\x00c")
    out = run([BWTSEARCH, pf, tmp_path / "bad"])
    assert out.returncode == 1 and b"not a BWT" in out.stderr
