"""The sequence table of `bigbwt -f --seqs` (host/fasta.c: pfp_fasta_text_seqs; host/seqs.c: the .seqs writer and parser), through
libpfphost.so, on the CPU: the table tiles the text the reader returns for every golden case and byte soup, the named edge cases
give the names and lengths written out here, and the parser refuses every malformed form with the line's number."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "golden_fasta.json")) as fh:
    _G = json.load(fh)
CASES, SOUPS = _G["cases"], _G["soups"]


class Seqs(C.Structure):
    _fields_ = [("nseq", C.c_uint64), ("cap", C.c_uint64), ("start", C.POINTER(C.c_uint64)), ("name", C.POINTER(C.c_char_p))]


@pytest.fixture(scope="module")
def lib():
    h = C.CDLL(os.path.join(ROOT, "big-bwt_amd", "libpfphost.so"))
    h.pfp_fasta_text.restype = C.c_size_t
    h.pfp_fasta_text.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p]
    h.pfp_fasta_text_seqs.restype = C.c_size_t
    h.pfp_fasta_text_seqs.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(Seqs)]
    h.pfp_seqs_init.argtypes = h.pfp_seqs_free.argtypes = [C.POINTER(Seqs)]
    h.pfp_seqs_init.restype = h.pfp_seqs_free.restype = None
    h.pfp_seqs_add.argtypes = [C.POINTER(Seqs), C.c_char_p, C.c_size_t, C.c_uint64]
    h.pfp_seqs_write.argtypes = [C.c_char_p, C.POINTER(Seqs)]
    h.pfp_seqs_read.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(Seqs), C.c_char_p, C.c_size_t]
    return h


def table(lib, raw):
    """(text, names, starts) of raw as the reader and its table give them"""
    out = C.create_string_buffer(max(len(raw), 1))
    t = Seqs()
    lib.pfp_seqs_init(C.byref(t))
    n = lib.pfp_fasta_text_seqs(raw, len(raw), out, C.byref(t))
    assert n != 2**64 - 1
    names = [t.name[k] for k in range(t.nseq)]
    starts = [int(t.start[k]) for k in range(t.nseq + 1)] if t.nseq else [0]
    lib.pfp_seqs_free(C.byref(t))
    return out.raw[:n], names, starts


def plain(raw):
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def check_tiles(starts, n):
    assert starts[0] == 0 and starts[-1] == n
    assert all(a <= b for a, b in zip(starts, starts[1:]))


@pytest.mark.parametrize("c", CASES, ids=["%s-w%d" % (c["name"], c["w"]) for c in CASES])
def test_table_tiles_the_golden_text(lib, c):
    text, names, starts = table(lib, plain(bytes.fromhex(c["raw_hex"])))
    assert text == bytes.fromhex(c["text_hex"])
    check_tiles(starts, len(c["text_hex"]) // 2)
    assert len(names) == len(starts) - 1


def test_table_tiles_the_golden_soups(lib):
    for raw_hex, text_hex in SOUPS:
        raw = bytes.fromhex(raw_hex)
        text, names, starts = table(lib, raw)
        assert text == bytes.fromhex(text_hex), raw
        check_tiles(starts, len(text_hex) // 2)


# name -> (names, lengths), read off tests/golden/make_golden_fasta.py
NAMED = {
    "two_records": ([b"chr1", b"chr2"], [150, 97]),
    "lowercase_and_crlf": ([b"r1", b"r2"], [61, 50]),
    "junk_blank_lines_no_final_newline": ([b"s1", b"empty_record", b"s2"], [70, 0, 97]),
    "fastq_four_line": ([b"read1", b"read2"], [80, 60]),
    "fastq_multi_line": ([b"m1", b"m2"], [100, 50]),
    "fastq_truncated_quality": ([b"t1"], [60]),              # t2's quality is short: the record is not delivered and has no line
    "stops_at_special_byte": ([b"x", b"y"], [50, 20]),        # y is cut at the byte 2; z is never read
    "gzip_three_copies": ([b"copy0", b"copy1", b"copy2"], [3000, 2999, 2998]),
}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_cases(lib, name):
    c = [c for c in CASES if c["name"] == name][0]
    text, names, starts = table(lib, plain(bytes.fromhex(c["raw_hex"])))
    want_names, want_lens = NAMED[name]
    assert names == want_names
    assert [b - a for a, b in zip(starts, starts[1:])] == want_lens
    assert text == bytes.fromhex(c["text_hex"])
    if name == "lowercase_and_crlf":
        assert text == text.upper() and b"\r" not in text


def test_no_header_at_all(lib):
    for raw in (b"", b"ACGT\nACGT\n", b"\n\n"):
        text, names, starts = table(lib, raw)
        assert text == b"" and names == [] and starts == [0]


def test_header_chars_inside_lines_and_empty_names(lib):
    text, names, starts = table(lib, b">\nAC\n> x\nG\n>id:1|a>b\nT>T\n")
    assert names == [b"", b"", b"id:1|a>b"] and text == b"ACGT>T" and starts == [0, 2, 3, 6]


def test_total_equals_reader_on_random_soups(lib):
    """byte soups of the characters that steer the reader: the table's total is what pfp_fasta_text returns"""
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b">@+\n\n\r \tacgtACGTN\x02", dtype=np.uint8)
    seen_records = 0
    for trial in range(600):
        raw = alphabet[rng.integers(0, alphabet.size, size=int(rng.integers(0, 120)))].tobytes()
        out = C.create_string_buffer(max(len(raw), 1))
        n = lib.pfp_fasta_text(raw, len(raw), out)
        text, names, starts = table(lib, raw)
        assert text == out.raw[:n], raw
        check_tiles(starts, n)
        seen_records += len(names)
    assert seen_records > 300


def write_table(lib, path, names, lens):
    t = Seqs()
    lib.pfp_seqs_init(C.byref(t))
    for nm, ln in zip(names, lens):
        assert lib.pfp_seqs_add(C.byref(t), nm, len(nm), ln) == 0
    assert lib.pfp_seqs_write(str(path).encode(), C.byref(t)) == 0
    lib.pfp_seqs_free(C.byref(t))


def read_table(lib, path, n):
    t, err = Seqs(), C.create_string_buffer(1024)
    rc = lib.pfp_seqs_read(str(path).encode(), n, C.byref(t), err, len(err))
    if rc:
        return rc, err.value.decode()
    got = ([t.name[k] for k in range(t.nseq)], [int(t.start[k]) for k in range(t.nseq + 1)] if t.nseq else [0])
    lib.pfp_seqs_free(C.byref(t))
    return 0, got


def test_round_trip(lib, tmp_path):
    names = [b"chr1", b"id:with:colons", b"", b"empty", b"x" * 300] + [b"s%d" % k for k in range(200)]
    lens = [5, 0, 7, 0, 2**33] + list(range(200))
    f = tmp_path / "t.seqs"
    write_table(lib, f, names, lens)
    lines = f.read_bytes().split(b"\n")
    assert lines[0] == b"chr1\t0\t5" and lines[1] == b"id:with:colons\t5\t0" and lines[-1] == b""
    rc, got = read_table(lib, f, sum(lens))
    assert rc == 0
    assert got[0] == names and got[1] == np.concatenate([[0], np.cumsum(lens)]).tolist()
    f.write_bytes(f.read_bytes()[:-1])                       # a last line without its newline is a line
    rc, got2 = read_table(lib, f, sum(lens))
    assert rc == 0 and got2 == got
    f.write_bytes(b"")
    assert read_table(lib, f, 0) == (0, ([], [0]))


@pytest.mark.parametrize("body,n,line,word", [
    (b"a\t0\t4\nb\t4\n", 8, 2, "three fields"),                 # two fields
    (b"a\t0\t4\n\nb\t4\t4\n", 8, 2, "three fields"),            # an empty line
    (b"a\t0\t4\tx\n", 4, 1, "three fields"),                    # four fields
    (b"a\t0\t4\nb\t4\t-4\n", 8, 2, "three fields"),             # not a number
    (b"a b\t0\n", 4, 1, "three fields"),                        # blanks are not tabs
    (b"a\t0\t4\nb\t5\t4\n", 9, 2, "start 5"),                   # start is not the running sum
    (b"a\t1\t4\n", 5, 1, "start 1"),                            # the first start is not 0
    (b"a\t0\t4\nb\t4\t4\n", 9, 2, "sum to 8"),                  # the total is not n
    (b"a\t0\t4\nb\t4\t4\n", 7, 2, "sum to 8"),
])
def test_parser_rejects_malformed_tables(lib, tmp_path, body, n, line, word):
    f = tmp_path / "bad.seqs"
    f.write_bytes(body)
    rc, msg = read_table(lib, f, n)
    assert rc == -2 and ("line %d" % line) in msg and word in msg, msg


def test_parser_missing_file(lib, tmp_path):
    rc, msg = read_table(lib, tmp_path / "nothing.seqs", 0)
    assert rc == -1 and "nothing.seqs" in msg


def test_python_reader_uses_the_same_parser(pkg, lib, tmp_path):
    f = tmp_path / "t.seqs"
    write_table(lib, f, [b"a", b"b:1"], [3, 4])
    names, starts = pkg.read_seqs_file(str(f), 7)
    assert names == [b"a", b"b:1"] and starts.tolist() == [0, 3, 7]
    with pytest.raises(pkg.PfpError) as e:
        pkg.read_seqs_file(str(f), 8)
    assert "line 2" in str(e.value)


def test_reverse_complement(pkg):
    import seq_reference as R
    pats = [b"", b"A", b"ACGTacgtNn-", bytes(range(1, 256)), "GATTACA"]
    got = pkg.reverse_complement(pats)
    assert got == [R.reverse_complement(p.encode() if isinstance(p, str) else p) for p in pats]
    assert got[2] == b"-nNacgtACGT" and got[4] == b"TGTAATC"
