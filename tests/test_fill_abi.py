"""The entry points of "Aligning chains" at the C boundary: declared in include/pfpgpu.h, described in the binding's table
(abi.SIGNATURES) and exported by the built library."""
import ctypes

from test_abi_and_host import declared_symbols

ENTRY_POINTS = ("pfp_fm_fill_dev", "pfp_fm_fill", "pfp_fm_chain_align_dev", "pfp_fm_chain_align", "pfp_fm_map_long_aln_dev", "pfp_fm_map_long_aln")


def test_the_header_declares_them():
    names = declared_symbols()
    assert [s for s in ENTRY_POINTS if s not in names] == []


def test_the_binding_describes_them(pkg):
    table = pkg.abi.SIGNATURES
    assert [s for s in ENTRY_POINTS if s not in table] == []
    # what the calls add to their models: pfp_fm_cigar's shape with two offsets per side, and max_fill with the scripts' outputs
    assert len(table["pfp_fm_fill"][1]) == len(table["pfp_fm_cigar"][1]) + 2
    assert len(table["pfp_fm_map_long_aln"][1]) == len(table["pfp_fm_map_long"][1]) + 7
    assert len(table["pfp_fm_map_long_aln_dev"][1]) == len(table["pfp_fm_map_long_dev"][1]) + 7
    assert len(table["pfp_fm_chain_align_dev"][1]) == len(table["pfp_fm_chain_dev"][1]) + 3 + 8
    assert all(table[s][0] is ctypes.c_int for s in ENTRY_POINTS)


def test_the_library_exports_them(pkg):
    lib = pkg.load_library()
    assert [s for s in ENTRY_POINTS if not hasattr(lib, s)] == []
    for s in ENTRY_POINTS:
        assert getattr(lib, s).argtypes is not None and len(getattr(lib, s).argtypes) == len(pkg.abi.SIGNATURES[s][1])
