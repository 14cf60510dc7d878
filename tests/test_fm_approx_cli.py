"""`bin/bwtsearch -k K` (host/bwtsearch.c): the lines of a pattern file with at most K substitutions, counted or located.  The
expected lines are formatted from the brute-force reference (approx_reference.py)."""
import os
import subprocess

import pytest

import approx_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "big-bwt_amd")
BIGBWT = os.path.join(PKG, "bigbwt")
BWTSEARCH = os.path.join(PKG, "bin", "bwtsearch")
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([str(c) for c in cmd], capture_output=True, timeout=timeout, env=e)


@pytest.fixture(scope="module")
def built(O, tmp_path_factory):
    d = tmp_path_factory.mktemp("approx_cli")
    text, pats = R.case("copies")
    f = d / "t"
    f.write_bytes(text.tobytes())
    out = run([BIGBWT, "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    pats = [p for p in pats if len(p) <= 64 and b"\n" not in p] + [text.tobytes()]
    pf = d / "pats"
    pf.write_bytes(b"\n".join(pats) + b"\n")
    return R.reference(O, "copies"), f, pf, pats


def count_line(ref, p, k):
    hits = ref.hits(p, k)
    by = [sum(len(h[4]) for h in hits if h[3] == d) for d in range(k + 1)]
    return "%d\t%s" % (sum(by), " ".join(str(c) for c in by))


def locate_line(ref, p, k, max_occ):
    rows = [(int(x), h[3]) for h in ref.hits(p, k) for x in h[4]]
    shown = rows[:max_occ] if max_occ else rows
    return "%d\t%s" % (len(rows), " ".join("%d:%d" % r for r in shown))


def test_count_and_locate_lines(built):
    ref, f, pf, pats = built
    for env in ({}, {"PFP_FM_BATCH": "5"}):
        out = run([BWTSEARCH, "-k", "2", pf, f], env=env)
        assert out.returncode == 0, out.stderr
        assert out.stdout.decode().splitlines() == [count_line(ref, p, 2) for p in pats]
        out = run([BWTSEARCH, "-l", "-k", "1", "-m", "3", pf, f], env=env)
        assert out.returncode == 0, out.stderr
        assert out.stdout.decode().splitlines() == [locate_line(ref, p, 1, 3) for p in pats]
    out = run([BWTSEARCH, "-k", "0", "-l", pf, f])
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == [locate_line(ref, p, 0, 0) for p in pats]


def test_reverse_complement(built):
    ref, f, pf, pats = built
    out = run([BWTSEARCH, "--rc", "-k", "1", pf, f])
    assert out.returncode == 0, out.stderr
    want = []
    for p in pats:
        want += [count_line(ref, p, 1), count_line(ref, p.translate(_RC)[::-1], 1)]
    assert out.stdout.decode().splitlines() == want and len(want) == 2 * len(pats)


def test_usage_errors_and_missing_files(built, tmp_path):
    ref, f, pf, pats = built
    for args in (["-k", "4"], ["-k", "-1"], ["-k", "x"], ["-k", "1", "--ms"], ["-k", "1", "--mems", "3"], ["-k", "1", "--docs"],
                 ["-k", "1", "-l", "--seqs"]):
        out = run([BWTSEARCH] + args + [pf, f])
        assert out.returncode == 2 and b"usage" in out.stdout, args
    out = run([BWTSEARCH, "-h"])
    assert out.returncode == 0 and b"-k K" in out.stdout
    g = tmp_path / "g"
    for ext in (".bwt", ".esa"):
        (tmp_path / ("g" + ext)).write_bytes(open(str(f) + ext, "rb").read())
    out = run([BWTSEARCH, "-k", "1", pf, g])              # counting needs the .bwt only
    assert out.returncode == 0 and out.stdout.decode().splitlines() == [count_line(ref, p, 1) for p in pats]
    out = run([BWTSEARCH, "-l", "-k", "1", pf, g])
    assert out.returncode == 1 and b"g.ssa" in out.stderr
