"""`bin/bwtsearch --align K --cigar` (host/bwtsearch.c): seed-and-extend with edit scripts over the lines of a pattern file.  The
expected lines are formatted from the MEMs FmIndex.mems lists, the numpy reference's composite (extend_reference.py) and the
reference's scripts of its triples (cigar_reference.py).  The text and the patterns are test_fm_extend_cli.py's."""
import os
import subprocess

import pytest

import approx_reference as R
import cigar_reference as G
import extend_reference as E
from extend_reference import planted

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "big-bwt_amd")
BIGBWT = os.path.join(PKG, "bigbwt")
BWTSEARCH = os.path.join(PKG, "bin", "bwtsearch")
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
K, SEED = 2, 12


def run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([str(c) for c in cmd], capture_output=True, timeout=timeout, env=e)


@pytest.fixture(scope="module")
def built(ctx, tmp_path_factory):
    import numpy as np
    d = tmp_path_factory.mktemp("cigar_cli")
    text = R.make_text("copies")
    tb = text.tobytes()
    f = d / "t"
    f.write_bytes(tb)
    out = run([BIGBWT, "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    rng = np.random.default_rng(9)
    pats = []
    for q, m in enumerate((30, 40, 64, 100, 150, 150, 200, 41, 11)):
        i = int(rng.integers(0, len(tb) - m + 1))
        pats.append(planted(rng, tb[i:i + m], q % 3, sorted(set(tb)), at_ends=q % 2 == 0))
    pats += [b"", b"ACGT", tb[100:160]]
    pf = d / "pats"
    pf.write_bytes(b"\n".join(pats) + b"\n")
    with ctx.fm_index_ms_files(str(f), text) as fm:
        fm.add_thresholds()
        memo, scripts = {}, {}

        def lines(ps, thresholds, cap, cigar=True):
            mem_off, mems = fm.mems(ps, SEED, thresholds=thresholds)
            off, start, end, dist = E.align(text, ps, mem_off, mems, K, 0, memo)
            out = []
            for p in range(len(ps)):
                rows = range(int(off[p]), int(off[p + 1]))
                shown = list(rows)[:cap] if cap else rows
                items = []
                for j in shown:
                    items.append("%d:%d:%d" % (start[j], end[j], dist[j]))
                    if cigar:
                        key = (ps[p], int(start[j]), int(end[j]))
                        if key not in scripts:
                            scripts[key] = G.script(text, *key, K)
                        d_, runs = scripts[key]
                        assert d_ == dist[j]
                        items[-1] += ":" + G.cigar_string(runs)
                out.append("%d\t%s" % (len(rows), " ".join(items)))
            return out
        both = [q for p in pats for q in (p, p.translate(_RC)[::-1])]
        want = {(t, cap): lines(pats, t, cap) for t in (False, True) for cap in (0, 1)}
        want["rc"] = lines(both, False, 0)
        want["plain"] = lines(pats, False, 0, cigar=False)
    assert sum(int(x.split("\t")[0]) for x in want[(False, 0)]) >= 8
    assert any(op in line for line in want[(False, 0)] for op in "XID") and any("=" in line for line in want[(False, 0)])
    return f, pf, want


def test_cigar_lines(built):
    f, pf, want = built
    for env in ({}, {"PFP_FM_BATCH": "5"}):
        out = run([BWTSEARCH, "--align", K, "--seed", SEED, "--cigar", pf, f], env=env)
        assert out.returncode == 0, out.stderr
        assert out.stdout.decode().splitlines() == want[(False, 0)]
        out = run([BWTSEARCH, "--align", K, "--seed", SEED, "--cigar", "-m", "1", pf, f], env=env)
        assert out.returncode == 0, out.stderr
        assert out.stdout.decode().splitlines() == want[(False, 1)]
    out = run([BWTSEARCH, "--cigar", "--align", K, "--seed", SEED, "--thresholds", "--text", f, pf, f])
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == want[(True, 0)]
    out = run([BWTSEARCH, "--align", K, "--seed", SEED, "--thresholds", "--cigar", "-m", "1", pf, f])
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == want[(True, 1)]


def test_reverse_complement(built):
    f, pf, want = built
    out = run([BWTSEARCH, "--rc", "--align", K, "--seed", SEED, "--cigar", pf, f])
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == want["rc"]


def test_without_cigar_the_lines_stay(built):
    f, pf, want = built
    out = run([BWTSEARCH, "--align", K, "--seed", SEED, pf, f])
    assert out.returncode == 0, out.stderr
    assert out.stdout.decode().splitlines() == want["plain"]


def test_usage_errors(built):
    f, pf, want = built
    for args in (["--cigar"], ["--cigar", "-l"], ["--cigar", "--mems", "3"], ["--cigar", "--ms"], ["--cigar", "-k", "1"], ["--cigar", "--seed", "12"],
                 ["--cigar=1", "--align", "2"]):
        out = run([BWTSEARCH] + args + [pf, f])
        assert out.returncode == 2 and b"usage" in out.stdout, args
    out = run([BWTSEARCH, "-h"])
    assert out.returncode == 0 and b"--cigar" in out.stdout and b"start:end:d:CIGAR" in out.stdout
