"""The C ABI of libpfpgpu.so as ctypes sees it: the structures of include/pfpgpu.h and one line per function it declares.
pfp.load_library() gives every function of SIGNATURES its restype and argtypes, so a call passes plain values - ints, bools,
numpy arrays, device addresses, None - and ctypes converts each at the width the header states (with no argtypes a bare int
goes out as a C int: an address or a byte count above 2^32 arrives cut).  A new function of the header needs its line here
before it can be called; tests/test_abi_and_host.py compares the table with the header."""
import ctypes as C

import numpy as np


class _ParseResult(C.Structure):
    _fields_ = [("n_used", C.c_uint64), ("dict", C.POINTER(C.c_uint8)), ("dict_size", C.c_uint64),
                ("occ", C.POINTER(C.c_uint32)), ("n_words", C.c_uint64),
                ("parse", C.POINTER(C.c_uint32)), ("n_phrases", C.c_uint64),
                ("last", C.POINTER(C.c_uint8)), ("sai", C.POINTER(C.c_uint8))]


class _BwtResult(C.Structure):
    _fields_ = [("bwt", C.POINTER(C.c_uint8)), ("bwt_size", C.c_uint64),
                ("sa", C.POINTER(C.c_uint8)), ("sa_bytes", C.c_uint64),
                ("ssa", C.POINTER(C.c_uint8)), ("ssa_bytes", C.c_uint64),
                ("esa", C.POINTER(C.c_uint8)), ("esa_bytes", C.c_uint64)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_uint64), ("total_ms", C.c_double), ("algo_bytes", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n", "n_phrases", "n_words", "dict_size", "sa_rounds_dict", "sa_rounds_parse", "hard_groups",
                                          "hard_chars", "hard_big_groups", "hard_max_chars", "hard_max_members", "hash_reseeds",
                                          "extra_triggers", "index_bits", "hard_minor_groups", "hard_minor_chars")] + \
               [(k, C.c_double) for k in ("ms_scan", "ms_phrases", "ms_sa_dict", "ms_sa_parse", "ms_merge", "ms_total", "parse_density")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ScanReport(C.Structure):
    _fields_ = [("n_used", C.c_uint64), ("n_ends", C.c_uint64)] + \
               [(k, C.c_uint32) for k in ("fast", "fthr", "fseed", "fthr_nom", "fauto", "fthr_first", "n_extra", "reserved")] + \
               [("extra", C.c_uint32 * 32), ("density", C.c_double), ("parse_density", C.c_double)] + \
               [(k, C.c_uint64) for k in ("chose", "dense", "kr_fallback", "dense_cuts", "n_nominal", "sampled", "kept", "distinct", "singles")]


class MultiStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n", "n_words", "n_phrases", "dict_size", "index_bits", "ranks", "sa_shares", "parse_shares")] + \
               [("ms_chain", C.c_double), ("ms_total", C.c_double), ("parse_density", C.c_double)]


class CheckResult(C.Structure):
    _fields_ = [("n", C.c_uint64), ("text_mismatch", C.c_uint64), ("sa_mismatch", C.c_uint64), ("ssa_runs", C.c_uint64),
                ("esa_runs", C.c_uint64), ("ssa_mismatch", C.c_uint64), ("esa_mismatch", C.c_uint64), ("ms", C.c_double)]

    def as_dict(self):
        """mismatch fields are None where the output is correct or was not checked (UINT64_MAX in the C struct)"""
        d = {k: getattr(self, k) for k, _ in self._fields_}
        for k in ("text_mismatch", "sa_mismatch", "ssa_mismatch", "esa_mismatch"):
            d[k] = None if d[k] == 2**64 - 1 else int(d[k])
        return d


class _FmInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("runs", C.c_uint64), ("sigma", C.c_uint32), ("row_bits", C.c_uint32), ("device_bytes", C.c_uint64),
                ("has_samples", C.c_int), ("has_thresholds", C.c_int), ("nseq", C.c_uint64)]


class TypedPtr:
    """The argument class of a `T *` parameter (`const T *`, `T name[4]`).  It takes None (NULL), a C-contiguous numpy array of
    exactly T's dtype (any other array is a TypeError, which ctypes reports as ArgumentError), an int (an address: the _dev
    entry points declare their device pointers with the element type too), and whatever POINTER(T) takes: a typed pointer, a
    ctypes array, byref of a scalar."""

    def __init__(self, ctype):
        self.ctype, self.ptr, self.dtype = ctype, C.POINTER(ctype), np.dtype(ctype)

    def from_param(self, a):
        if a is None:
            return None
        if isinstance(a, int):
            return C.c_void_p(a)
        if isinstance(a, np.ndarray):
            if a.dtype != self.dtype or not a.flags.c_contiguous:
                raise TypeError(f"a C-contiguous {self.dtype} array is wanted, not {a.dtype}{'' if a.flags.c_contiguous else ' in strides'}")
            return a.ctypes.data_as(self.ptr)
        return self.ptr.from_param(a)


i32, u32, u64, f64, vp, cs = C.c_int, C.c_uint32, C.c_uint64, C.c_double, C.c_void_p, C.c_char_p
pint, p8, p32, p64, pi32, pi64 = (TypedPtr(t) for t in (C.c_int, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int32, C.c_int64))
pp8, pp32, pp64, pvp = (C.POINTER(t) for t in (C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p))
ptr = C.POINTER

# name: (restype, argtypes), in the header's order.  vp: pfp_ctx *, pfp_fm *, void *; pvp: pfp_ctx **, pfp_fm **, void *[];
# cs: const char *, char *; p8 .. pi64: TypedPtr; pp8 .. pp64: T ** results
SIGNATURES = {
    "pfp_device_count": (i32, []),
    "pfp_ctx_create": (i32, [pvp, i32]),
    "pfp_ctx_destroy": (None, [vp]),
    "pfp_last_error": (cs, [vp]),
    "pfp_strerror": (cs, [i32]),
    "pfp_version": (cs, []),
    "pfp_ctx_stream": (vp, [vp]),
    "pfp_free": (None, [vp]),
    "pfp_debug_check": (i32, [vp]),
    "pfp_pool_trim": (None, [vp]),
    "pfp_get_mem_stats": (i32, [vp, p64]),
    "pfp_get_pool_counters": (i32, [vp, p64]),
    "pfp_scan": (i32, [vp, p8, u64, i32, u64, pp64, p64, p64]),
    "pfp_parse": (i32, [vp, p8, u64, i32, u64, i32, ptr(_ParseResult)]),
    "pfp_parse_result_free": (None, [ptr(_ParseResult)]),
    "pfp_sacak_int": (i32, [vp, p32, p32, u64, u64]),
    "pfp_sacak": (i32, [vp, p8, p32, u64]),
    "pfp_gsacak": (i32, [vp, p8, p32, u64]),
    "pfp_gsacak_lcp_da": (i32, [vp, p8, p32, pi32, pi32, u64]),
    "pfp_gsacak_lcp_da64": (i32, [vp, p8, p64, pi64, pi64, u64]),
    "pfp_sacak_int64": (i32, [vp, p32, p64, u64, u64]),
    "pfp_sacak64": (i32, [vp, p8, p64, u64]),
    "pfp_gsacak64": (i32, [vp, p8, p64, u64]),
    "pfp_bwtparse": (i32, [vp, p32, u64, p8, p8, p32, u64, p32, p8, p8]),
    "pfp_merge": (i32, [vp, p8, u64, p32, u64, p32, p8, p8, u64, i32, i32, ptr(_BwtResult)]),
    "pfp_bwt_result_free": (None, [ptr(_BwtResult)]),
    "pfp_bigbwt": (i32, [vp, p8, u64, i32, u64, i32, ptr(_BwtResult)]),
    "pfp_bigbwt_files": (i32, [vp, p8, u64, i32, u64, i32, cs, p64]),
    "pfp_bigbwt_fd": (i32, [vp, i32, u64, u64, i32, u64, i32, cs, p64]),
    "pfp_bigbwt_dev": (i32, [vp, vp, u64, i32, u64, i32, vp, vp, p64]),
    "pfp_pack5_dev": (i32, [vp, vp, u64, vp]),
    "pfp_pwrite_dev": (i32, [vp, cs, u64, vp, u64]),
    "pfp_sample_runs_dev": (i32, [vp, vp, vp, u64, u64, i32, i32, i32, vp, u64, p64]),
    "pfp_bigbwt_formats_dev": (i32, [vp, vp, u64, i32, u64, i32, vp, pvp, p64, p64]),
    "pfp_dev_free": (None, [vp, vp]),
    "pfp_memcpy_d2h": (i32, [vp, vp, vp, u64]),
    "pfp_get_stats": (i32, [vp, ptr(Stats)]),
    "pfp_set_profiling": (None, [vp, i32]),
    "pfp_set_kernel_trace": (None, [vp, i32]),
    "pfp_get_kernel_trace": (i32, [vp, ptr(KernelStat), i32]),
    "pfp_debug_lib_sort": (i32, [vp, i32, vp, vp, u64, i32, i32, p32, p32, u64]),
    "pfp_debug_scan_chain": (i32, [vp, p8, u64, i32, u64, p64, p32, u32, pp64, pp64, pp8, ptr(ScanReport)]),
    "pfp_set_max_phrase": (None, [vp, u64]),
    "pfp_set_window_hash": (None, [vp, i32]),
    "pfp_set_parse_density": (i32, [vp, f64]),
    "pfp_set_index_bits": (i32, [vp, i32]),
    "pfp_dist_propose_triggers": (i32, [vp, vp, u64, i32, u64, p32, p32]),
    "pfp_dist_local_parse": (i32, [vp, vp, u64, u64, i32, u64, i32, i32, u64, i32, p32, u32, p64]),
    "pfp_dist_parse_plan": (i32, [vp, p8, u64, i32, u64, u32, p64, p64]),
    "pfp_dist_propose_triggers2": (i32, [vp, vp, u64, u64, i32, u64, p64, p32, p32, vp, u64, p64]),
    "pfp_dist_decide_density": (i32, [vp, vp, u64, u64, p64]),
    "pfp_dist_local_parse2": (i32, [vp, vp, u64, u64, i32, u64, i32, i32, u64, i32, p64, p32, u32, p64]),
    "pfp_dist_export_local": (i32, [vp, vp, vp, vp, vp]),
    "pfp_dist_global": (i32, [vp, vp, u64, vp, u64, u64, vp, p64]),
    "pfp_dist_global_sort": (i32, [vp, vp, u64, vp, u64, u32, u32, vp, p64]),
    "pfp_dist_global_finish": (i32, [vp, vp, u32, u64, vp]),
    "pfp_dist_partition_words": (i32, [vp, u32, p64]),
    "pfp_dist_export_partition": (i32, [vp, vp, vp]),
    "pfp_dist_owner_dedup": (i32, [vp, vp, u64, vp, u64, vp, p64]),
    "pfp_dist_export_owned": (i32, [vp, vp, vp]),
    "pfp_dist_global_sort_distinct": (i32, [vp, vp, u64, vp, u64, vp, u32, u32, vp, p64]),
    "pfp_dist_parse_sort": (i32, [vp, vp, u64, u32, u32, vp, p64]),
    "pfp_dist_set_parse_sa": (i32, [vp, vp, u64]),
    "pfp_dist_merge": (i32, [vp, vp, u64, vp, vp, i32, u64, u64, u64, vp, vp]),
    "pfp_dist_sample_runs": (i32, [vp, i32, i32, vp, u64, p64]),
    "pfp_dist_release": (None, [vp]),
    "pfp_bigbwt_files_multi": (i32, [i32, pint, p8, u64, i32, u64, i32, u64, cs, ptr(MultiStats), cs, u64]),
    "pfp_multi_rccl_selftest": (i32, [i32, cs, u64]),
    "pfp_multi_rccl_selftest2": (i32, [i32, i32, cs, u64]),
    "pfp_unbwt_dev": (i32, [vp, vp, u64, vp]),
    "pfp_unbwt": (i32, [vp, p8, u64, p8]),
    "pfp_check_bwt_dev": (i32, [vp, vp, u64, vp, vp, vp, u64, vp, u64, ptr(CheckResult)]),
    "pfp_check_bwt_files": (i32, [vp, cs, p8, i32, u64, u64, i32, ptr(CheckResult)]),
    "pfp_fm_build_dev": (i32, [vp, vp, u64, vp, u64, vp, u64, pvp]),
    "pfp_fm_build_files": (i32, [vp, cs, i32, pvp]),
    "pfp_fm_count_dev": (i32, [vp, vp, p64, u64, p64, p64, p64]),
    "pfp_fm_locate_dev": (i32, [vp, u64, p64, p64, p64, u64, p64, p64]),
    "pfp_fm_count": (i32, [vp, p8, p64, u64, p64, p64, p64]),
    "pfp_fm_locate": (i32, [vp, p8, p64, u64, u64, p64, p64, p64, pp64]),
    "pfp_fm_info": (i32, [vp, ptr(_FmInfo)]),
    "pfp_fm_free": (None, [vp]),
    "pfp_fm_approx_dev": (i32, [vp, vp, p64, u64, i32, p64, p64, p64, p64, p8]),
    "pfp_fm_approx": (i32, [vp, p8, p64, u64, i32, p64, pp64, pp64, pp64, pp8]),
    "pfp_fm_approx_locate": (i32, [vp, p8, p64, u64, i32, u64, p64, pp64, pp8]),
    "pfp_fm_approx_stats": (i32, [vp, p64]),
    "pfp_fm_extend_dev": (i32, [vp, vp, p64, u64, p32, pi64, u64, i32, p8, p64, p64]),
    "pfp_fm_extend": (i32, [vp, p8, p64, u64, p32, pi64, u64, i32, p8, p64, p64]),
    "pfp_fm_align_dev": (i32, [vp, vp, p64, u64, u64, i32, u64, i32, p64, p64, p64, p8]),
    "pfp_fm_align": (i32, [vp, p8, p64, u64, u64, i32, u64, i32, p64, pp64, pp64, pp8]),
    "pfp_fm_window_dev": (i32, [vp, vp, p64, u64, p32, p64, p64, u64, i32, p8, p64, p64]),
    "pfp_fm_window": (i32, [vp, p8, p64, u64, p32, p64, p64, u64, i32, p8, p64, p64]),
    "pfp_fm_cigar_dev": (i32, [vp, vp, p64, u64, p32, p64, p64, u64, i32, p8, p64, p32]),
    "pfp_fm_cigar": (i32, [vp, p8, p64, u64, p32, p64, p64, u64, i32, p8, p64, pp32]),
    "pfp_fm_map_dev": (i32, [vp, vp, p64, u64, u64, i32, u64, i32, p64, p8, p64, p8, p32, p64, p64, p8, p64, pp32, p64, pp8]),
    "pfp_fm_map": (i32, [vp, p8, p64, u64, u64, i32, u64, i32, p64, p8, p64, pp8, pp32, pp64, pp64, pp8, pp64, pp32, pp64, pp8]),
    "pfp_fm_map_pairs_dev": (i32, [vp, vp, p64, u64, u64, i32, i32, u64, u64, u64, p8, p64, p8, p8, p8, p64, p8, p32, p64, p64, p8, pi64,
                                   p64, pp32, p64, pp8]),
    "pfp_fm_map_pairs": (i32, [vp, p8, p64, u64, u64, i32, i32, u64, u64, u64, p8, p64, p8, p8, p8, p64, p8, p32, p64, p64, p8, pi64,
                               p64, pp32, p64, pp8]),
    "pfp_fm_anchors_dev": (i32, [vp, vp, p64, u64, u64, u64, i32, p64, p64, p32]),
    "pfp_fm_anchors": (i32, [vp, p8, p64, u64, u64, u64, i32, p64, pp64, p32]),
    "pfp_fm_chain_dev": (i32, [vp, p64, p64, u64, u64, u64, u64, u64, p64, p32, p32, p32, p32, p64, p64, p32]),
    "pfp_fm_chain": (i32, [vp, p64, p64, u64, u64, u64, u64, u64, p64, pp32, pp32, pp32, pp32, pp64, pp64, pp32]),
    "pfp_fm_map_long_dev": (i32, [vp, vp, p64, u64, u64, u64, u64, u64, u64, u64, i32, p64, p8, p64, p8, p32, p64, p64, p64, p32, p32, p32,
                                  p32, p32]),
    "pfp_fm_map_long": (i32, [vp, p8, p64, u64, u64, u64, u64, u64, u64, u64, i32, p64, p8, p64, pp8, pp32, pp64, pp64, pp64, pp32, pp32,
                              pp32, pp32, pp32]),
    "pfp_fm_fill_dev": (i32, [vp, vp, p64, u64, p32, p64, p64, p64, p64, u64, u64, p32, p64, p32]),
    "pfp_fm_fill": (i32, [vp, p8, p64, u64, p32, p64, p64, p64, p64, u64, u64, p32, p64, pp32]),
    "pfp_fm_chain_align_dev": (i32, [vp, vp, p64, u64, p64, p64, u64, u64, u64, u64, u64, p64, p32, p32, p32, p32, p64, p64, p32, p32, p64, p32,
                                     p32, p64, p32, p64, p32]),
    "pfp_fm_chain_align": (i32, [vp, p8, p64, u64, p64, p64, u64, u64, u64, u64, u64, p64, pp32, pp32, pp32, pp32, pp64, pp64, pp32, pp32, pp64,
                                 pp32, pp32, pp64, pp32, pp64, pp32]),
    "pfp_fm_map_long_aln_dev": (i32, [vp, vp, p64, u64, u64, u64, u64, u64, u64, u64, i32, u64, p64, p8, p64, p8, p32, p64, p64, p64, p32, p32,
                                      p32, p32, p32, p32, p64, p32, p32, p64, p32]),
    "pfp_fm_map_long_aln": (i32, [vp, p8, p64, u64, u64, u64, u64, u64, u64, u64, i32, u64, p64, p8, p64, pp8, pp32, pp64, pp64, pp64, pp32,
                                  pp32, pp32, pp32, pp32, pp32, pp64, pp32, pp32, pp64, pp32]),
    "pfp_fm_fill_stats": (i32, [vp, p64]),
    "pfp_fm_build_ms_dev": (i32, [vp, vp, u64, vp, u64, vp, u64, vp, pvp]),
    "pfp_fm_build_ms_files": (i32, [vp, cs, p8, i32, u64, u64, pvp]),
    "pfp_fm_ms_dev": (i32, [vp, vp, p64, u64, p32, p64]),
    "pfp_fm_mems_dev": (i32, [vp, p64, u64, p32, p64, u64, p64, p64]),
    "pfp_fm_ms_stats": (i32, [vp, p64]),
    "pfp_fm_ms": (i32, [vp, p8, p64, u64, p32, p64]),
    "pfp_fm_mems": (i32, [vp, p8, p64, u64, u64, p64, pp64]),
    "pfp_lcp_dev": (i32, [vp, vp, u64, vp, u64, vp, u64, vp, p64, p64, p64]),
    "pfp_lcp_files": (i32, [vp, cs, p8, i32, u64, u64, i32]),
    "pfp_fm_thresholds_dev": (i32, [vp, vp, u64]),
    "pfp_fm_thresholds_files": (i32, [vp, cs]),
    "pfp_fm_ms_thr_dev": (i32, [vp, vp, p64, u64, p32, p64]),
    "pfp_fm_ms_thr": (i32, [vp, p8, p64, u64, p32, p64]),
    "pfp_fm_mems_thr": (i32, [vp, p8, p64, u64, u64, p64, pp64]),
    "pfp_fm_set_seqs": (i32, [vp, p64, u64]),
    "pfp_fm_seqmap_dev": (i32, [vp, p64, u64, p32, p64]),
    "pfp_fm_locate_seqs_dev": (i32, [vp, p64, u64, p64, p64, p64, u64, p64, p32, p64]),
    "pfp_fm_doclist_dev": (i32, [vp, p64, u64, p64, p64, p64, p64, p32, p64]),
    "pfp_fm_locate_seqs": (i32, [vp, p8, p64, u64, u64, p64, p64, p64, pp32, pp64]),
    "pfp_fm_doclist": (i32, [vp, p8, p64, u64, p64, pp32, pp64]),
    "pfp_stage_text_dev": (i32, [vp, vp, u64, i32]),
    "pfp_scan_staged": (i32, [vp, u64, p64]),
    "pfp_scan_k1_enqueue": (i32, [vp, u64]),
}

