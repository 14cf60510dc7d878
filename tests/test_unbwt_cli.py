"""`bigbwt --verify` and `bin/unbwt` (host/unbwt.c): inverting a .bwt and checking written outputs against their text."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "big-bwt_amd")
BIGBWT = os.path.join(PKG, "bigbwt")
UNBWT = os.path.join(PKG, "bin", "unbwt")
REF = os.path.join(ROOT, "oracle", "_ref")


def run(cmd, timeout=300):
    return subprocess.run([str(c) for c in cmd], capture_output=True, text=True, timeout=timeout)


def test_bigbwt_help_lists_verify():
    out = run([BIGBWT, "-h"])
    assert out.returncode == 0 and "--verify" in out.stdout


def test_unbwt_usage():
    assert os.access(UNBWT, os.X_OK)
    out = run([UNBWT])
    assert out.returncode != 0 and "usage" in out.stdout
    out = run([UNBWT, "-h"])
    assert out.returncode == 0 and "--check" in out.stdout


def test_verify_is_a_usage_error_with_parsing(tmp_path):
    f = tmp_path / "t"
    f.write_bytes(b"ACGT" * 100)
    for mode in ("--parsing", "--compress"):
        out = run([BIGBWT, "--verify", mode, f])
        assert out.returncode == 2 and "--verify" in out.stdout
        assert not os.path.exists(str(f) + ".dicz")


@pytest.fixture(scope="module")
def text1m(O):
    t = O.gen_fasta(250_000, 4, 0.002, 7)
    assert 0.9e6 < len(t) < 1.1e6
    return t


@pytest.mark.gpu
def test_bigbwt_verify(tmp_path, text1m):
    f = tmp_path / "t"
    f.write_bytes(text1m.tobytes())
    out = run([BIGBWT, "-s", "-e", "--verify", f])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "==== Checking outputs by inverting the BWT. Command: pfp_check_bwt_files(%s)" % f in out.stdout
    for line in ("BWT inverts to the input", "SSA ok", "ESA ok"):
        assert line in out.stdout.splitlines(), out.stdout
    assert "SA  ok" not in out.stdout
    out = run([BIGBWT, "-S", "--verify", f])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "BWT inverts to the input" in out.stdout and "SA  ok" in out.stdout.splitlines()


@pytest.mark.gpu
def test_bigbwt_verify_fasta_and_two_ranks(tmp_path, text1m, monkeypatch):
    """-f: the check runs on the filtered text; -G 2 (rank threads over one device here): the files the chain wrote"""
    f = tmp_path / "t.fa"
    seq = text1m[(text1m != ord(">")) & (text1m != 10)]
    body = b"\n".join(seq[i:i + 60].tobytes() for i in range(0, len(seq), 60))
    f.write_bytes(b">one\n" + body + b"\n")
    out = run([BIGBWT, "-f", "-s", "--verify", f])
    assert out.returncode == 0 and "BWT inverts to the input" in out.stdout and "SSA ok" in out.stdout, out.stdout + out.stderr
    g = tmp_path / "t"
    g.write_bytes(text1m.tobytes())
    monkeypatch.setenv("PFP_MULTI_LOOPBACK", "1")
    out = run([BIGBWT, "-G", "2", "-s", "-e", "--verify", g])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "BWT inverts to the input" in out.stdout and "SSA ok" in out.stdout and "ESA ok" in out.stdout


@pytest.mark.gpu
def test_unbwt_check_finds_a_corrupted_ssa(pkg, tmp_path, text1m):
    f = tmp_path / "t"
    f.write_bytes(text1m.tobytes())
    assert run([BIGBWT, "-s", "-e", f]).returncode == 0
    out = run([UNBWT, "--check", f, "-s", "-e", f])
    assert out.returncode == 0 and "SSA ok" in out.stdout and "ESA ok" in out.stdout, out.stdout + out.stderr
    ssa = bytearray(open(str(f) + ".ssa", "rb").read())
    i = len(ssa) // 10 // 2
    ssa[10 * i + 5] ^= 1                                  # the SA value of pair i
    open(str(f) + ".ssa", "wb").write(bytes(ssa))
    out = run([UNBWT, "--check", f, "-s", "-e", f])
    assert out.returncode == 1
    assert "SSA differs at entry %d" % i in out.stdout.splitlines() and "ESA ok" in out.stdout, out.stdout
    # a text that differs, and a .bwt that is not one
    t = bytearray(text1m.tobytes())
    t[12345] ^= 0x20
    (tmp_path / "u").write_bytes(bytes(t))
    out = run([UNBWT, "--check", tmp_path / "u", f])
    assert out.returncode == 1 and "BWT differs from the input at text position 12345" in out.stdout, out.stdout
    (tmp_path / "bad.bwt").write_bytes(b"a\x00ab")
    out = run([UNBWT, tmp_path / "bad"])
    assert out.returncode == 1 and "cycle" in out.stderr
    out = run([UNBWT, "--check", f, tmp_path / "bad"])
    assert out.returncode == 1 and "cycle" in out.stdout


@pytest.mark.gpu
def test_unbwt_rebuilds_the_input(tmp_path, text1m):
    f = tmp_path / "t"
    f.write_bytes(text1m.tobytes())
    assert run([BIGBWT, f]).returncode == 0
    out = run([UNBWT, f])
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(str(f) + ".out", "rb").read() == text1m.tobytes()
    o = tmp_path / "elsewhere.txt"
    assert run([UNBWT, "-o", o, f]).returncode == 0
    assert o.read_bytes() == text1m.tobytes()


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "pfbwtNT.x")), reason="oracle/_ref not built")
def test_unbwt_checks_the_reference_outputs(tmp_path, text1m):
    """the .bwt / .ssa / .esa the real reference writes for the same text check clean"""
    f = tmp_path / "r"
    f.write_bytes(text1m.tobytes())
    for cmd in ([os.path.join(REF, "newscanNT.x"), f, "-w", "10", "-p", "100", "-s"], [os.path.join(REF, "bwtparse"), f, "-s"],
                [os.path.join(REF, "pfbwtNT.x"), "-w", "10", f, "-s", "-e"]):
        out = run(cmd, timeout=600)
        assert out.returncode == 0, out.stdout + out.stderr
    out = run([UNBWT, "--check", f, "-s", "-e", f])
    assert out.returncode == 0, out.stdout + out.stderr
    assert "BWT inverts to the input" in out.stdout and "SSA ok" in out.stdout and "ESA ok" in out.stdout
