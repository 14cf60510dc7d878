"""`bin/unbwt --thresholds [--lcp]` (host/unbwt.c) and `bin/bwtsearch --ms | --mems L --thresholds` (host/bwtsearch.c)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "big-bwt_amd")
BIGBWT = os.path.join(PKG, "bigbwt")
BWTSEARCH = os.path.join(PKG, "bin", "bwtsearch")
UNBWT = os.path.join(PKG, "bin", "unbwt")

pytestmark = pytest.mark.gpu


def run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([str(c) for c in cmd], capture_output=True, timeout=timeout, env=e)


@pytest.fixture(scope="module")
def built(O, tmp_path_factory):
    d = tmp_path_factory.mktemp("lcpcli")
    text = O.gen_fasta(100_000, 4, 0.002, 9)
    f = d / "t"
    f.write_bytes(text.tobytes())
    out = run([BIGBWT, "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    rng = np.random.default_rng(1)
    tb = text.tobytes()
    pats = [b"A", b"", b"ACGT", tb[:20], b"ZZZ", b"AC#GT", tb[-7:]]
    for m in (5, 12, 40, 200):
        for _ in range(4):
            i = int(rng.integers(0, len(tb) - m))
            s = bytearray(tb[i:i + m])
            pats.append(bytes(s))
            s[m // 2] = ord("#")
            pats.append(bytes(s))
    pats.append(tb[100:300] + tb[5000:5200])
    pats = [p.replace(b"\n", b"N") for p in pats]          # (a line holds no newline)
    pf = d / "pats"
    pf.write_bytes(b"\n".join(pats) + b"\n")
    return text, f, pf, pats


def lens(stdout):
    """the len column of --ms: per line the lengths, positions dropped"""
    return [[tok.split(":")[0] for tok in line.split(" ")] if line else [] for line in stdout.decode().split("\n")[:-1]]


def test_unbwt_thresholds_and_search(pkg, ctx, built):
    text, f, pf, pats = built
    n = len(text)
    rd = lambda ext: open(str(f) + ext, "rb").read()
    want = ctx.lcp(rd(".bwt"), rd(".ssa"), rd(".esa"), text)
    plain = run([BWTSEARCH, "--ms", pf, f])
    assert plain.returncode == 0, plain.stderr
    # no .thr_pos yet: bwtsearch computes the thresholds itself
    assert not os.path.exists(str(f) + ".thr_pos")
    first = run([BWTSEARCH, "--ms", "--thresholds", pf, f])
    assert first.returncode == 0, first.stderr
    assert lens(first.stdout) == lens(plain.stdout) and len(lens(plain.stdout)) == len(pats)
    for extra in ([], ["--text", f]):
        for ext in (".thr_pos", ".lcp"):
            if os.path.exists(str(f) + ext):
                os.remove(str(f) + ext)
        out = run([UNBWT, "--thresholds"] + extra + [f])
        assert out.returncode == 0, out.stderr
        assert not os.path.exists(str(f) + ".lcp")
        assert np.array_equal(pkg.unpack5(rd(".thr_pos")), want["thr"])
        out = run([UNBWT, "--thresholds", "--lcp"] + extra + [f])
        assert out.returncode == 0, out.stderr
        assert len(rd(".lcp")) == 5 * (n + 1) and np.array_equal(pkg.unpack5(rd(".lcp")), want["lcp"])
        assert np.array_equal(pkg.unpack5(rd(".thr_pos")), want["thr"])
    # with the file: the same output, positions included
    for extra in ([], ["--text", f]):
        for env in ({}, {"PFP_FM_BATCH": "3"}):
            out = run([BWTSEARCH, "--ms", "--thresholds"] + extra + [pf, f], env=env)
            assert out.returncode == 0, out.stderr
            assert out.stdout == first.stdout
    a = run([BWTSEARCH, "--mems", "8", pf, f])
    b = run([BWTSEARCH, "--mems", "8", "--thresholds", pf, f])
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    strip = lambda o: [[t.rsplit(":", 1)[0] for t in line.split("\t")[1].split(" ") if t] for line in o.decode().split("\n")[:-1]]
    assert strip(a.stdout) == strip(b.stdout)
    # a .thr_pos of another BWT is refused
    open(str(f) + ".thr_pos", "ab").write(b"\0" * 5)
    out = run([BWTSEARCH, "--ms", "--thresholds", pf, f])
    assert out.returncode == 1 and b"thr_pos" in out.stderr
    os.remove(str(f) + ".thr_pos")


def test_usage_errors(built):
    text, f, pf, pats = built
    out = run([UNBWT, "-h"])
    assert out.returncode == 0 and b"--thresholds" in out.stdout and b"--lcp" in out.stdout and b"--text" in out.stdout
    for args in (["--lcp", f], ["--text", f, f], ["--thresholds", "--check", f, f], ["--thresholds", "-o", "x", f], ["--thresholds"],
                 ["--thresholds", f, f], ["--thresholds", "--text"]):
        out = run([UNBWT] + args)
        assert out.returncode == 2 and b"usage" in out.stdout, args
    out = run([BWTSEARCH, "-h"])
    assert out.returncode == 0 and b"--thresholds" in out.stdout
    for args in (["--thresholds"], ["--thresholds", "-l"], ["--thresholds", "-m", "3"]):
        out = run([BWTSEARCH] + args + [pf, f])
        assert out.returncode == 2 and b"usage" in out.stdout, args


def test_input_errors(built, tmp_path):
    text, f, pf, pats = built
    out = run([UNBWT, "--thresholds", "--text", tmp_path / "nothing", f])
    assert out.returncode == 1 and b"nothing" in out.stderr
    (tmp_path / "short").write_bytes(text.tobytes()[:-1])
    out = run([UNBWT, "--thresholds", "--text", tmp_path / "short", f])
    assert out.returncode == 1 and b"short" in out.stderr and str(len(text)).encode() in out.stderr
    for ext in (".bwt", ".ssa"):
        (tmp_path / ("g" + ext)).write_bytes(open(str(f) + ext, "rb").read())
    out = run([UNBWT, "--thresholds", tmp_path / "g"])
    assert out.returncode == 1 and b"g.esa" in out.stderr
