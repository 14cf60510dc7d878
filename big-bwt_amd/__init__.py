"""big-bwt_amd: MI355X-native prefix-free-parsing BWT builder (HIP kernels behind a C ABI).

The directory name carries a hyphen (it mirrors the reference's name), so import it through
`__graft_entry__.load_package()` / `tests/conftest.py`, which register it as `bigbwt_amd`.
"""
from .pfp import (Context, PfpError, FLAG_SA, FLAG_SSA, FLAG_ESA, SYMBOLS, LIB_PATH, load_library,  # noqa: F401
                  pack5, unpack5, reverse_complement, read_seqs_file, cigar_string, md_string,
                  FM_EXTEND_MAX_K, FM_EXTEND_MAX_M, FM_WINDOW_MAX_W, FM_PAIR_MAX_ANCHORS, PAIR_NAMES, FM_CHAIN_PRED, LONG_NAMES,
                  FM_FILL_MAX_F, FM_FILL_MAX_LEN, CHAIN_ALN_NAMES, LONG_ALN_NAMES)
