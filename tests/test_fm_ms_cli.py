"""`bin/bwtsearch --ms` / `--mems L` (host/bwtsearch.c): matching statistics and maximal exact matches of the lines of a pattern file."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "big-bwt_amd")
BIGBWT = os.path.join(PKG, "bigbwt")
BWTSEARCH = os.path.join(PKG, "bin", "bwtsearch")

pytestmark = pytest.mark.gpu


def run(cmd, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([str(c) for c in cmd], capture_output=True, timeout=timeout, env=e)


@pytest.fixture(scope="module")
def built(O, tmp_path_factory):
    d = tmp_path_factory.mktemp("mscli")
    text = O.gen_fasta(100_000, 4, 0.002, 9)
    f = d / "t"
    f.write_bytes(text.tobytes())
    out = run([BIGBWT, "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    rng = np.random.default_rng(1)
    tb = text.tobytes()
    pats = [b"A", b"", b"ACGT", tb[:20], b"ZZZ", b"A\x00C", b"AC#GT", tb[-7:], b"\xff\xfe"]
    for m in (5, 12, 40, 200):
        for _ in range(4):
            i = int(rng.integers(0, len(tb) - m))
            s = bytearray(tb[i:i + m])
            pats.append(bytes(s))
            s[m // 2] = ord("#")
            pats.append(bytes(s))
    pats = [p.replace(b"\n", b"N") for p in pats]          # (a line holds no newline)
    pf = d / "pats"
    pf.write_bytes(b"\n".join(pats) + b"\n")
    return text, f, pf, pats


def ms_lines(pats, off, ln, pos):
    return [" ".join("%d:%d" % (ln[j], pos[j]) if ln[j] else "0:-" for j in range(int(off[k]), int(off[k + 1]))) for k in range(len(pats))]


def mem_lines(pats, mem_off, mems):
    return ["%d\t%s" % (mem_off[k + 1] - mem_off[k], " ".join("%d:%d:%d" % tuple(int(x) for x in r) for r in mems[int(mem_off[k]):int(mem_off[k + 1])]))
            for k in range(len(pats))]


def test_cli_matches_the_api(pkg, ctx, built):
    text, f, pf, pats = built
    with ctx.fm_index_ms_files(str(f), text) as fm:
        want_ms = ms_lines(pats, *fm.matching_statistics(pats))
        want_mems = mem_lines(pats, *fm.mems(pats, 8))
    assert want_ms[1] == "" and "0:-" in want_ms[4] and want_mems[1] == "0\t"
    for extra in ([], ["--text", f]):
        for env in ({}, {"PFP_FM_BATCH": "3"}):
            out = run([BWTSEARCH, "--ms"] + extra + [pf, f], env=env)
            assert out.returncode == 0, out.stderr
            assert out.stdout.decode().split("\n")[:-1] == want_ms
            out = run([BWTSEARCH, "--mems", "8"] + extra + [pf, f], env=env)
            assert out.returncode == 0, out.stderr
            assert out.stdout.decode().split("\n")[:-1] == want_mems


def test_cli_usage_errors(built):
    text, f, pf, pats = built
    out = run([BWTSEARCH, "-h"])
    assert out.returncode == 0 and b"-l" in out.stdout and b"--ms" in out.stdout and b"--mems" in out.stdout and b"--text" in out.stdout
    for args in (["--ms", "-l"], ["--ms", "--mems", "3"], ["--mems", "3", "-l"], ["--ms", "-m", "4"], ["--mems", "3", "-m", "4"],
                 ["--mems", "0"], ["--mems", "x"], ["--mems", "-2"], ["--mems"], ["--text", f], ["--text", f, "-l"]):
        out = run([BWTSEARCH] + args + [pf, f])
        assert out.returncode == 2 and b"usage" in out.stdout, args


def test_cli_input_errors(built, tmp_path):
    text, f, pf, pats = built
    n = len(text)
    out = run([BWTSEARCH, "--ms", "--text", tmp_path / "nothing", pf, f])
    assert out.returncode == 1 and b"nothing" in out.stderr
    for name, body in (("short", text.tobytes()[:-1]), ("long", text.tobytes() + b"A")):
        (tmp_path / name).write_bytes(body)
        out = run([BWTSEARCH, "--mems", "4", "--text", tmp_path / name, pf, f])
        assert out.returncode == 1 and name.encode() in out.stderr, out.stderr
        assert str(len(body)).encode() in out.stderr and str(n).encode() in out.stderr
    for ext in (".bwt", ".ssa"):
        (tmp_path / ("g" + ext)).write_bytes(open(str(f) + ext, "rb").read())
    out = run([BWTSEARCH, "--ms", pf, tmp_path / "g"])
    assert out.returncode == 1 and b"g.esa" in out.stderr
