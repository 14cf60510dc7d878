"""Host-side mirror of the reference's stage interface over the C ABI of libpfpgpu.so.

The reference (alshai/Big-BWT) is three executables glued by files; this module exposes the
same three stages plus the whole chain as functions over numpy arrays that hold the reference's
file formats byte for byte:

    parse()     == newscanNT.x / pscan.x      (newscan.cpp:569-650)
    bwtparse()  == bwtparse                   (bwtparse.c:212-322)
    merge()     == pfbwtNT.x / pfbwt.x        (pfbwt.cpp:320-418)
    bigbwt()    == bigbwt -w W -p M [-S|-s|-e] (bigbwt:69-156)
    sacak_int() / sacak() / gsacak()  == gsa/gsacak.h:78-105

Everything computes in hand-written HIP kernels on the MI355X; there is no CPU fallback: the
import succeeds without a GPU (so that symbol checks can run), but creating a Context does not.
abi.py declares the signature of every function of the library; the calls below pass plain values.
"""
import ctypes as C
import os

import numpy as np

from .abi import SIGNATURES, CheckResult, KernelStat, MultiStats, ScanReport, Stats, _BwtResult, _FmInfo, _ParseResult  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libpfpgpu.so")

FLAG_SA, FLAG_SSA, FLAG_ESA = 1, 2, 4

ERRORS = {0: "PFP_OK", -1: "PFP_EINVAL", -2: "PFP_ENODEV", -3: "PFP_EHIP", -4: "PFP_ECOLLISION",
          -5: "PFP_ELIMIT", -6: "PFP_EFORMAT", -7: "PFP_ENOMEM", -8: "PFP_ESHORT"}

SYMBOLS = list(SIGNATURES)      # every symbol include/pfpgpu.h declares

FM_APPROX_MAX_K = 3
FM_EXTEND_MAX_K, FM_EXTEND_MAX_M = 32, 65535
FM_WINDOW_MAX_W = 16384
FM_PAIR_MAX_ANCHORS = 64
# the arrays FmIndex.map_pairs returns, in order: the first two per pair, the next ten per read, then the reads' scripts and MD strings
PAIR_NAMES = ("proper", "npairs", "mapped", "rescued", "mapq", "nhits", "strand", "seq", "off", "start", "dist", "tlen", "cig_off", "cig",
              "md_off", "md")
FM_CHAIN_PRED = 64
# the arrays FmIndex.map_long returns, in order: the first three per read, the others per returned chain
LONG_NAMES = ("hit_off", "mapq", "nchains", "strand", "seq", "off", "ts", "te", "qs", "qe", "score", "n", "match")
FM_FILL_MAX_F, FM_FILL_MAX_LEN = 4096, 65535
# the arrays FmIndex.chain_align returns, in order: chain()'s, then per chain where its script begins, its edits, its unfilled gaps,
# the scripts and the members
CHAIN_ALN_NAMES = ("chain_off", "score", "n", "qs", "qe", "ts", "te", "match", "aqs", "ats", "nm", "unfilled", "cig_off", "cig", "mem_off", "mem")
# the arrays FmIndex.map_long_aln returns, in order: map_long()'s, then per returned chain the same but the members
LONG_ALN_NAMES = LONG_NAMES + ("aqs", "ats", "nm", "unfilled", "cig_off", "cig")
CIGAR_OPS = {1: "I", 2: "D", 7: "=", 8: "X"}    # the BAM codes of the operations an edit script holds

LCP_LCP, LCP_THR = 1, 2


class PfpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class _Seqs(C.Structure):
    """pfp_seqs of host/seqs.h (libpfphost.so)"""
    _fields_ = [("nseq", C.c_uint64), ("cap", C.c_uint64), ("start", C.POINTER(C.c_uint64)), ("name", C.POINTER(C.c_char_p))]


_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def reverse_complement(patterns):
    """each pattern reversed with A<->T, C<->G, a<->t, c<->g swapped; every other byte stays as it is (DNA reads: the other strand)"""
    return [(p.encode() if isinstance(p, str) else bytes(p)).translate(_RC)[::-1] for p in patterns]


def read_seqs_file(path, n):
    """(names, starts) of a .seqs file (host/seqs.h) whose lengths must sum to n; the parser is the one bwtsearch uses"""
    host = C.CDLL(os.path.join(HERE, "libpfphost.so"))
    host.pfp_seqs_read.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(_Seqs), C.c_char_p, C.c_size_t]
    host.pfp_seqs_free.argtypes = [C.POINTER(_Seqs)]
    host.pfp_seqs_free.restype = None
    t, err = _Seqs(), C.create_string_buffer(1024)
    rc = host.pfp_seqs_read(os.fsencode(path), n, C.byref(t), err, len(err))
    if rc:
        raise PfpError(-1 if rc == -1 else -6, err.value.decode(errors="replace"))
    try:
        names = [t.name[k] for k in range(t.nseq)]
        starts = np.ctypeslib.as_array(t.start, shape=(t.nseq + 1,)).astype(np.uint64) if t.nseq else np.zeros(1, dtype=np.uint64)
    finally:
        host.pfp_seqs_free(C.byref(t))
    return names, starts


def cigar_string(runs):
    """the runs of one edit script (uint32: length << 4 | op) as text, e.g. "57=1X20=1I72="; "*" for no runs"""
    return "".join("%d%s" % (int(r) >> 4, CIGAR_OPS[int(r) & 15]) for r in runs) or "*"


def md_string(md, md_off, i):
    """the MD string of hit i of FmIndex.map_reads, as bytes: matched lengths in decimal, a text byte per substitution, ^ and the
    text bytes of a deletion, e.g. b"57T20^AC72" (text bytes are kept as they are)"""
    return bytes(md[int(md_off[i]):int(md_off[i + 1])])


def _patterns(patterns):
    """a list of bytes / str (UTF-8) / uint8 arrays -> (concatenated uint8 bytes, npat+1 uint64 offsets)"""
    parts = [p.encode() if isinstance(p, str) else bytes(np.asarray(p, dtype=np.uint8)) if isinstance(p, np.ndarray) else bytes(p)
             for p in patterns]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([len(x) for x in parts], dtype=np.uint64)
    return np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8), off


def _addr(p):
    """the address a pointer holds; None for NULL"""
    return C.cast(p, C.c_void_p).value


class _Closing:
    """a handle of the library: the end of a with block and collection both close() it"""

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FmIndex(_Closing):
    """Count and locate over a BWT and its run samples (pfp_fm, csrc/fmsearch.hip; the r-index of Gagie, Navarro and Prezza).
    Made by Context.fm_index / fm_index_files; holds device memory of its context until close()."""

    def __init__(self, ctx, handle):
        self.ctx, self.lib, self._h = ctx, ctx.lib, handle

    def close(self):
        """hand the device memory back to the context (a context closed before leaves nothing to hand back)"""
        if self._h and self.ctx._h:
            self.lib.pfp_fm_free(self._h)
        self._h = C.c_void_p()

    @staticmethod
    def _host_patterns(patterns):
        """-> (npat, the npat+1 offsets, the three leading arguments of a call over host patterns)"""
        pat, off = _patterns(patterns)
        npat = len(off) - 1
        return npat, off, (pat, off, npat)

    def _take_free(self, ptr, n, dtype):
        """a copy of the n entries of a result array of the library, which goes back to it (pfp_free takes NULL)"""
        out = _take(ptr, n, dtype)
        self.lib.pfp_free(ptr)
        return out

    def info(self):
        r = _FmInfo()
        self.ctx._check(self.lib.pfp_fm_info(self._h, C.byref(r)))
        return {k: int(getattr(r, k)) for k, _ in r._fields_}

    def count(self, patterns, toehold=False):
        """-> (sp, ep) uint64 arrays, the row range [sp, ep) of each pattern; toehold=True: (sp, ep, SA[sp]) (needs samples)"""
        npat, _, args = self._host_patterns(patterns)
        sp, ep = np.zeros(npat, dtype=np.uint64), np.zeros(npat, dtype=np.uint64)
        first = np.zeros(npat, dtype=np.uint64) if toehold else None
        self.ctx._check(self.lib.pfp_fm_count(self._h, *args, sp, ep, first))
        return (sp, ep, first) if toehold else (sp, ep)

    def locate(self, patterns, max_occ=0, ranges=False):
        """-> (offsets, positions): pattern p's positions, in row order, are positions[offsets[p]:offsets[p+1]], at most max_occ
        of them (0: all); ranges=True: (offsets, positions, sp, ep)"""
        npat, _, args = self._host_patterns(patterns)
        sp, ep = np.zeros(npat, dtype=np.uint64), np.zeros(npat, dtype=np.uint64)
        out_off = np.zeros(npat + 1, dtype=np.uint64)
        pos = C.POINTER(C.c_uint64)()
        self.ctx._check(self.lib.pfp_fm_locate(self._h, *args, max_occ, sp, ep, out_off, C.byref(pos)))
        positions = self._take_free(pos, out_off[-1], np.uint64)
        return (out_off, positions, sp, ep) if ranges else (out_off, positions)

    def approx(self, patterns, k, toehold=False):
        """the hits of every pattern with at most k substitutions (pfpgpu.h, "Approximate search"; k in 0..FM_APPROX_MAX_K)
        -> (hit_off, sp, ep, dist): pattern p's hits, by increasing sp, are the row ranges [sp[i], ep[i]) with dist[i] (uint8)
        mismatches for i in hit_off[p]:hit_off[p+1]; toehold=True: (hit_off, sp, ep, dist, SA[sp]) (needs samples)"""
        npat, _, args = self._host_patterns(patterns)
        hit_off = np.zeros(npat + 1, dtype=np.uint64)
        sp, ep, first = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        dist = C.POINTER(C.c_uint8)()
        self.ctx._check(self.lib.pfp_fm_approx(self._h, *args, k, hit_off, C.byref(sp), C.byref(ep),
                                               C.byref(first) if toehold else None, C.byref(dist)))
        total = hit_off[-1]
        out = hit_off, self._take_free(sp, total, np.uint64), self._take_free(ep, total, np.uint64), self._take_free(dist, total, np.uint8)
        return out + (self._take_free(first, total, np.uint64),) if toehold else out

    def approx_locate(self, patterns, k, max_occ=0):
        """-> (off, pos, dist): the positions of pattern p's occurrences with at most k substitutions are pos[off[p]:off[p+1]],
        hits by increasing sp and rows in row order inside a hit, each with its number of mismatches in dist (uint8); at most
        max_occ per pattern (0: all).  Needs samples."""
        npat, _, args = self._host_patterns(patterns)
        out_off = np.zeros(npat + 1, dtype=np.uint64)
        pos, dist = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)()
        self.ctx._check(self.lib.pfp_fm_approx_locate(self._h, *args, k, max_occ, out_off, C.byref(pos), C.byref(dist)))
        return out_off, self._take_free(pos, out_off[-1], np.uint64), self._take_free(dist, out_off[-1], np.uint8)

    def approx_dev(self, d_pat, d_pat_off, npat, k, d_hit_off, d_sp=None, d_ep=None, d_dist=None, d_first=None):
        """device pointers: pattern bytes, npat+1 uint64 offsets -> npat+1 uint64 d_hit_off; d_sp / d_ep (uint64) and d_dist
        (uint8), room for d_hit_off[npat] each, get the hits (all three None: offsets only), d_first their toeholds"""
        self.ctx._check(self.lib.pfp_fm_approx_dev(self._h, d_pat, d_pat_off, npat, k, d_hit_off, d_sp, d_ep, d_first, d_dist))

    def approx_stats(self):
        """{launches, pairs, hits} of the approximate searches since the last look; pairs (LF pairs of the walks) are collected
        only under PFP_FM_MS_STATS=1"""
        out = (C.c_uint64 * 3)()
        self.ctx._check(self.lib.pfp_fm_approx_stats(self._h, out))
        return dict(launches=int(out[0]), pairs=int(out[1]), hits=int(out[2]))

    def extend(self, patterns, cand_pat, cand_diag, k):
        """the best alignment of a whole pattern near a diagonal under unit-cost edit distance (pfpgpu.h, "Extending seeds"; k in
        0..FM_EXTEND_MAX_K, an index with text).  Candidate i is pattern cand_pat[i] with pattern byte 0 at text position
        cand_diag[i] (signed) -> (dist, start, end): dist[i] (uint8) edits align the pattern to T[start[i]:end[i]); 0xFF and
        2^64 - 1 twice where nothing within k edits lies in the window"""
        _, _, args = self._host_patterns(patterns)
        cp = np.ascontiguousarray(cand_pat, dtype=np.uint32)
        cd = np.ascontiguousarray(cand_diag, dtype=np.int64)
        if cp.shape != cd.shape or cp.ndim != 1:
            raise ValueError("cand_pat and cand_diag: two 1-D arrays of one length")
        nc = len(cp)
        dist, start, end = np.zeros(nc, dtype=np.uint8), np.zeros(nc, dtype=np.uint64), np.zeros(nc, dtype=np.uint64)
        self.ctx._check(self.lib.pfp_fm_extend(self._h, *args, cp, cd, nc, k, dist, start, end))
        return dist, start, end

    def extend_dev(self, d_pat, d_pat_off, npat, d_cand_pat, d_cand_diag, ncand, k, d_dist, d_start, d_end):
        """device pointers: pattern bytes, npat+1 uint64 offsets, ncand uint32 pattern indices and int64 diagonals -> ncand uint8
        d_dist and uint64 d_start / d_end"""
        self.ctx._check(self.lib.pfp_fm_extend_dev(self._h, d_pat, d_pat_off, npat, d_cand_pat, d_cand_diag, ncand, k, d_dist, d_start, d_end))

    def window(self, patterns, cand_pat, lo, hi, k):
        """the best alignment of a whole pattern anywhere in a window of the text under unit-cost edit distance (pfpgpu.h,
        "Aligning in a window"; k in 0..FM_EXTEND_MAX_K, an index with text, windows of at most FM_WINDOW_MAX_W bytes).  Candidate i
        is pattern cand_pat[i] against T[lo[i]:hi[i]) -> (dist, start, end): dist[i] (uint8) edits align the pattern to
        T[start[i]:end[i]), the shortest span that ends first among the best; 0xFF and 2^64 - 1 twice where nothing within k edits
        lies in the window, or the window is not one of the text"""
        _, _, args = self._host_patterns(patterns)
        cp = np.ascontiguousarray(cand_pat, dtype=np.uint32)
        lo, hi = np.ascontiguousarray(lo, dtype=np.uint64), np.ascontiguousarray(hi, dtype=np.uint64)
        if not (cp.shape == lo.shape == hi.shape) or cp.ndim != 1:
            raise ValueError("cand_pat, lo and hi: three 1-D arrays of one length")
        nc = len(cp)
        dist, start, end = np.zeros(nc, dtype=np.uint8), np.zeros(nc, dtype=np.uint64), np.zeros(nc, dtype=np.uint64)
        self.ctx._check(self.lib.pfp_fm_window(self._h, *args, cp, lo, hi, nc, k, dist, start, end))
        return dist, start, end

    def window_dev(self, d_pat, d_pat_off, npat, d_cand_pat, d_lo, d_hi, ncand, k, d_dist, d_start, d_end):
        """device pointers: pattern bytes, npat+1 uint64 offsets, ncand uint32 pattern indices and uint64 window starts and ends ->
        ncand uint8 d_dist and uint64 d_start / d_end"""
        self.ctx._check(self.lib.pfp_fm_window_dev(self._h, d_pat, d_pat_off, npat, d_cand_pat, d_lo, d_hi, ncand, k, d_dist, d_start, d_end))

    def align(self, patterns, k, min_seed, max_aln=0, thresholds=False, cigar=False):
        """seed-and-extend: every maximal exact match of at least min_seed bytes (as mems lists them; thresholds as there) is
        extended along its diagonal with at most k edits -> (aln_off, start, end, dist): pattern p's distinct alignments are
        T[start[i]:end[i]) with dist[i] (uint8) edits for i in aln_off[p]:aln_off[p+1], ordered by (dist, start, end), at most
        max_aln of them (0: all).  A heuristic: a MEM carries one position of its string.  cigar=True: (aln_off, start, end,
        dist, cig_off, cig), the alignments' edit scripts as cigar() returns them"""
        npat, _, args = self._host_patterns(patterns)
        aln_off = np.zeros(npat + 1, dtype=np.uint64)
        start, end, dist = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)()
        self.ctx._check(self.lib.pfp_fm_align(self._h, *args, min_seed, k, max_aln, bool(thresholds), aln_off, C.byref(start), C.byref(end),
                                              C.byref(dist)))
        total = aln_off[-1]
        out = aln_off, self._take_free(start, total, np.uint64), self._take_free(end, total, np.uint64), self._take_free(dist, total, np.uint8)
        if not cigar:
            return out
        aln_pat = np.repeat(np.arange(npat, dtype=np.uint32), np.diff(aln_off).astype(np.int64))
        return out + self.cigar(patterns, aln_pat, out[1], out[2], k)[1:]

    def cigar(self, patterns, aln_pat, start, end, k):
        """the edit scripts of alignments that extend or align found, or of any spans (pfpgpu.h, "Edit scripts"; k as there).
        Alignment i is pattern aln_pat[i] against T[start[i]:end[i]) -> (dist, cig_off, cig): dist[i] (uint8) edits, and the runs
        cig[cig_off[i]:cig_off[i+1]] (uint32: length << 4 | op; cigar_string writes them out); 0xFF and no runs where the span
        is not one of the text or the pattern is more than k edits from it"""
        _, _, args = self._host_patterns(patterns)
        ap = np.ascontiguousarray(aln_pat, dtype=np.uint32)
        st, en = np.ascontiguousarray(start, dtype=np.uint64), np.ascontiguousarray(end, dtype=np.uint64)
        if not (ap.shape == st.shape == en.shape) or ap.ndim != 1:
            raise ValueError("aln_pat, start and end: three 1-D arrays of one length")
        na = len(ap)
        dist, cig_off = np.zeros(na, dtype=np.uint8), np.zeros(na + 1, dtype=np.uint64)
        cig = C.POINTER(C.c_uint32)()
        self.ctx._check(self.lib.pfp_fm_cigar(self._h, *args, ap, st, en, na, k, dist, cig_off, C.byref(cig)))
        return dist, cig_off, self._take_free(cig, cig_off[-1], np.uint32)

    def cigar_dev(self, d_pat, d_pat_off, npat, d_aln_pat, d_start, d_end, naln, k, d_dist, d_cig_off, d_cig=None):
        """device pointers: pattern bytes, npat+1 uint64 offsets, naln uint32 pattern indices and uint64 starts and ends -> naln
        uint8 d_dist and naln+1 uint64 d_cig_off; d_cig (uint32, room for d_cig_off[naln]) gets the runs (None: offsets only)"""
        self.ctx._check(self.lib.pfp_fm_cigar_dev(self._h, d_pat, d_pat_off, npat, d_aln_pat, d_start, d_end, naln, k, d_dist, d_cig_off, d_cig))

    def align_dev(self, d_pat, d_pat_off, npat, k, min_seed, d_aln_off, d_start=None, d_end=None, d_dist=None, max_aln=0, thresholds=False):
        """device pointers: pattern bytes, npat+1 uint64 offsets -> npat+1 uint64 d_aln_off; d_start / d_end (uint64) and d_dist
        (uint8), room for d_aln_off[npat] each, get the alignments (all three None: offsets only)"""
        self.ctx._check(self.lib.pfp_fm_align_dev(self._h, d_pat, d_pat_off, npat, min_seed, k, max_aln, bool(thresholds), d_aln_off,
                                                  d_start, d_end, d_dist))

    def map_reads(self, patterns, k, min_seed, max_sec=0, thresholds=False):
        """one answer per read over a collection (pfpgpu.h, "Mapping reads"; an index with text and a sequence table): both
        strands through seed-and-extend, the alignments inside one record, one hit per locus, ordered by (dist, strand, start, end)
        -> (hit_off, mapq, nhits, strand, seq, off, start, dist, cig_off, cig, md_off, md): read p has nhits[p] hits and mapping
        quality mapq[p] (uint8; a choice, not a probability); the first 1 + max_sec of them are i in hit_off[p]:hit_off[p+1], the
        first the primary: strand[i] (uint8; 1: the reverse complement aligns), record seq[i] (uint32) at offset off[i], text
        position start[i], dist[i] (uint8) edits, the runs cig[cig_off[i]:cig_off[i+1]] as cigar() gives them and the MD string
        md[md_off[i]:md_off[i+1]] (uint8; md_string reads it)"""
        npat, _, args = self._host_patterns(patterns)
        hit_off, mapq, nhits = np.zeros(npat + 1, dtype=np.uint64), np.zeros(npat, dtype=np.uint8), np.zeros(npat, dtype=np.uint64)
        u8, u32, u64 = C.c_uint8, C.c_uint32, C.c_uint64
        strand, seq, off, start, dist, cig_off, cig, md_off, md = (C.POINTER(t)() for t in (u8, u32, u64, u64, u8, u64, u32, u64, u8))
        self.ctx._check(self.lib.pfp_fm_map(self._h, *args, min_seed, k, max_sec, bool(thresholds), hit_off, mapq, nhits,
                                            C.byref(strand), C.byref(seq), C.byref(off), C.byref(start),
                                            C.byref(dist), C.byref(cig_off), C.byref(cig), C.byref(md_off), C.byref(md)))
        H = int(hit_off[-1])
        t = self._take_free
        co, mo = t(cig_off, H + 1, np.uint64), t(md_off, H + 1, np.uint64)
        return (hit_off, mapq, nhits, t(strand, H, np.uint8), t(seq, H, np.uint32), t(off, H, np.uint64), t(start, H, np.uint64),
                t(dist, H, np.uint8), co, t(cig, co[-1], np.uint32), mo, t(md, mo[-1], np.uint8))

    def map_reads_dev(self, d_pat, d_pat_off, npat, k, min_seed, d_hit_off, d_mapq, d_nhits, d_strand=None, d_seq=None, d_off=None,
                      d_start=None, d_dist=None, d_cig_off=None, d_md_off=None, max_sec=0, thresholds=False):
        """device pointers: read bytes, npat+1 uint64 offsets -> npat+1 uint64 d_hit_off, npat uint8 d_mapq and uint64 d_nhits.
        The per-hit outputs all None: those only.  Otherwise d_strand (uint8), d_seq (uint32), d_off, d_start (uint64) and d_dist
        (uint8) with room for d_hit_off[npat] entries and d_cig_off, d_md_off (uint64) for one more are filled, and the call
        returns (d_cig, d_md): the addresses of the runs (uint32) and the MD bytes, device buffers of the library that go back
        with Context.dev_free (None where there is no hit)"""
        per_hit = (d_strand, d_seq, d_off, d_start, d_dist, d_cig_off, d_md_off)
        fill = any(x for x in per_hit)
        d_cig, d_md = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        self.ctx._check(self.lib.pfp_fm_map_dev(self._h, d_pat, d_pat_off, npat, min_seed, k, max_sec, bool(thresholds), d_hit_off,
                                                d_mapq, d_nhits, d_strand, d_seq, d_off, d_start, d_dist,
                                                d_cig_off, C.byref(d_cig) if fill else None, d_md_off,
                                                C.byref(d_md) if fill else None))
        return (_addr(d_cig), _addr(d_md)) if fill else None

    def map_pairs(self, patterns, k, min_seed, min_ins, max_ins, anchors=8, thresholds=False):
        """read pairs over a collection (pfpgpu.h, "Mapping read pairs"): patterns 2q and 2q + 1 are mates 1 and 2 of pair q,
        forward/reverse.  The first `anchors` hits of both mates (as map_reads orders them) are combined into proper pairs - same
        record, opposite strands, min_ins <= insert <= max_ins - and an anchor without a proper partner has its mate looked for
        in the window it points at (window()).  -> the arrays PAIR_NAMES names: proper (uint8) and npairs (uint64) per pair;
        mapped, rescued, mapq (uint8), nhits (uint64), strand (uint8), seq (uint32), off, start (uint64), dist (uint8) and tlen
        (int64) per read; cig_off, cig, md_off, md: read r's runs are cig[cig_off[r]:cig_off[r+1]], its MD string
        md[md_off[r]:md_off[r+1]].  In a proper pair a read reports its member of the primary pair and the pair MAPQ, otherwise
        its own first hit and MAPQ; an unmapped read has seq 2^32 - 1, off = start = 2^64 - 1, dist 0xFF, no runs, no MD"""
        npat, _, args = self._host_patterns(patterns)
        z = lambda count, dt: np.zeros(count, dtype=dt)
        proper, npairs = z(npat // 2, np.uint8), z(npat // 2, np.uint64)
        mapped, rescued, mapq, nhits, strand = z(npat, np.uint8), z(npat, np.uint8), z(npat, np.uint8), z(npat, np.uint64), z(npat, np.uint8)
        seq, off, start, dist, tlen = z(npat, np.uint32), z(npat, np.uint64), z(npat, np.uint64), z(npat, np.uint8), z(npat, np.int64)
        cig_off, md_off = z(npat + 1, np.uint64), z(npat + 1, np.uint64)
        cig, md = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        self.ctx._check(self.lib.pfp_fm_map_pairs(self._h, *args, min_seed, k, bool(thresholds), min_ins, max_ins, anchors, proper, npairs,
                                                  mapped, rescued, mapq, nhits, strand, seq, off, start, dist, tlen, cig_off, C.byref(cig),
                                                  md_off, C.byref(md)))
        return (proper, npairs, mapped, rescued, mapq, nhits, strand, seq, off, start, dist, tlen, cig_off,
                self._take_free(cig, cig_off[-1], np.uint32), md_off, self._take_free(md, md_off[-1], np.uint8))

    def map_pairs_dev(self, d_pat, d_pat_off, npat, k, min_seed, min_ins, max_ins, d_proper, d_npairs, d_mapped, d_rescued, d_mapq, d_nhits,
                      d_strand, d_seq, d_off, d_start, d_dist, d_tlen, d_cig_off, d_md_off, anchors=8, thresholds=False):
        """device pointers: read bytes, npat+1 uint64 offsets -> npat/2 uint8 d_proper and uint64 d_npairs; npat uint8 d_mapped,
        d_rescued, d_mapq, d_strand, d_dist, uint64 d_nhits, d_off, d_start, uint32 d_seq, int64 d_tlen; npat+1 uint64 d_cig_off and
        d_md_off.  Returns (d_cig, d_md): the addresses of the runs (uint32) and the MD bytes, device buffers of the library that
        go back with Context.dev_free (None where there is nothing)"""
        d_cig, d_md = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint8)()
        self.ctx._check(self.lib.pfp_fm_map_pairs_dev(self._h, d_pat, d_pat_off, npat, min_seed, k, bool(thresholds), min_ins, max_ins,
                                                      anchors, d_proper, d_npairs, d_mapped, d_rescued, d_mapq, d_nhits, d_strand, d_seq,
                                                      d_off, d_start, d_dist, d_tlen, d_cig_off, C.byref(d_cig), d_md_off, C.byref(d_md)))
        return _addr(d_cig), _addr(d_md)

    def anchors(self, patterns, min_seed, max_occ=500, thresholds=False):
        """every occurrence of every maximal exact match of at least min_seed bytes (pfpgpu.h, "Chaining anchors", 1; an index with
        text) -> (anc_off, anc, skipped): pattern p's anchors are the rows anc[anc_off[p]:anc_off[p+1]] of a (k, 3) uint64 array,
        each (i, len, t): P[i:i+len] = T[t:t+len], by increasing (t + len, i + len).  A MEM with more than max_occ occurrences is
        left out and counted in skipped[p] (uint32); with a sequence table set, so is an occurrence that crosses a record border
        (uncounted).  max_occ = 500 is a choice."""
        npat, _, args = self._host_patterns(patterns)
        anc_off, skipped = np.zeros(npat + 1, dtype=np.uint64), np.zeros(npat, dtype=np.uint32)
        out = C.POINTER(C.c_uint64)()
        self.ctx._check(self.lib.pfp_fm_anchors(self._h, *args, min_seed, max_occ, bool(thresholds), anc_off, C.byref(out), skipped))
        return anc_off, self._take_free(out, 3 * int(anc_off[-1]), np.uint64).reshape(-1, 3), skipped

    def anchors_dev(self, d_pat, d_pat_off, npat, min_seed, d_anc_off, d_anc=None, d_skipped=None, max_occ=500, thresholds=False):
        """device pointers: pattern bytes, npat+1 uint64 offsets -> npat+1 uint64 d_anc_off; d_anc (room for 3 * d_anc_off[npat]
        uint64) gets the triples (None: offsets only), d_skipped (npat uint32, may be None) the skipped MEMs"""
        self.ctx._check(self.lib.pfp_fm_anchors_dev(self._h, d_pat, d_pat_off, npat, min_seed, max_occ, bool(thresholds), d_anc_off, d_anc,
                                                    d_skipped))

    def chain(self, anc_off, anc, max_gap=5000, band=500, min_score=40, max_chains=0):
        """the chains of every pattern's anchors (pfpgpu.h, "Chaining anchors", 2): anc_off / anc as anchors() gives them, or any
        anchors in strictly increasing (t + len, i + len) order per pattern -> (chain_off, score, n, qs, qe, ts, te, match): pattern
        p's chains, by (score descending, te, qe), at most max_chains (0: all), are i in chain_off[p]:chain_off[p+1]: n[i]
        anchors spanning P[qs[i]:qe[i]] and T[ts[i]:te[i]], match[i] bytes in seeds (uint32 but ts, te: uint64).  Two anchors
        chain when they lie at most max_gap apart on either side and at most band off each other's diagonal; a chain scoring
        below min_score is dropped.  The defaults are choices."""
        off = _arr(np.asarray(anc_off), np.uint64)
        a = _arr(np.asarray(anc).reshape(-1), np.uint64)
        npat = len(off) - 1
        if npat < 0 or len(a) % 3:
            raise ValueError("anc_off: npat + 1 offsets; anc: three values per anchor")
        chain_off = np.zeros(npat + 1, dtype=np.uint64)
        u32, u64 = C.c_uint32, C.c_uint64
        score, n, qs, qe, ts, te, match = (C.POINTER(t)() for t in (u32, u32, u32, u32, u64, u64, u32))
        self.ctx._check(self.lib.pfp_fm_chain(self._h, off, a, npat, max_gap, band, min_score, max_chains, chain_off, C.byref(score),
                                              C.byref(n), C.byref(qs), C.byref(qe), C.byref(ts), C.byref(te), C.byref(match)))
        t, total = self._take_free, int(chain_off[-1])
        return (chain_off, t(score, total, np.uint32), t(n, total, np.uint32), t(qs, total, np.uint32), t(qe, total, np.uint32),
                t(ts, total, np.uint64), t(te, total, np.uint64), t(match, total, np.uint32))

    def chain_dev(self, d_anc_off, d_anc, npat, d_chain_off, d_score=None, d_n=None, d_qs=None, d_qe=None, d_ts=None, d_te=None, d_match=None,
                  max_gap=5000, band=500, min_score=40, max_chains=0):
        """device pointers: npat+1 uint64 anchor offsets and the triples -> npat+1 uint64 d_chain_off; the seven arrays behind it
        (uint32 but d_ts, d_te: uint64; room for d_chain_off[npat] each) get the chains (all None: offsets only)"""
        self.ctx._check(self.lib.pfp_fm_chain_dev(self._h, d_anc_off, d_anc, npat, max_gap, band, min_score, max_chains, d_chain_off, d_score,
                                                  d_n, d_qs, d_qe, d_ts, d_te, d_match))

    def map_long(self, patterns, min_seed, max_occ=500, max_gap=5000, band=500, min_score=40, max_sec=0, thresholds=False):
        """where long reads lie (pfpgpu.h, "Chaining anchors", 3): both strands of every read through anchors() and chain(), their
        chains merged by (score descending, strand, te, qe) -> the arrays LONG_NAMES names: read p has nchains[p] chains (uint64)
        and mapping quality mapq[p] (uint8; 0 without a chain, 60 with one, else min(60, 60 (s1 - s2) / s1): a choice); the first
        1 + max_sec are i in hit_off[p]:hit_off[p+1], the first the primary: strand[i] (uint8), record seq[i] (uint32; 0 without
        a table) at offset off[i], T[ts[i]:te[i]], the read's bytes qs[i]:qe[i] as given, score[i], n[i] anchors, match[i] bytes
        in seeds.  The defaults are choices."""
        npat, _, args = self._host_patterns(patterns)
        hit_off, mapq, nchains = np.zeros(npat + 1, dtype=np.uint64), np.zeros(npat, dtype=np.uint8), np.zeros(npat, dtype=np.uint64)
        u8, u32, u64 = C.c_uint8, C.c_uint32, C.c_uint64
        kinds = (u8, u32, u64, u64, u64, u32, u32, u32, u32, u32)
        ptrs = [C.POINTER(t)() for t in kinds]
        self.ctx._check(self.lib.pfp_fm_map_long(self._h, *args, min_seed, max_occ, max_gap, band, min_score, max_sec, bool(thresholds), hit_off,
                                                 mapq, nchains, *(C.byref(q) for q in ptrs)))
        H = int(hit_off[-1])
        return (hit_off, mapq, nchains) + tuple(self._take_free(q, H, np.dtype(t)) for q, t in zip(ptrs, kinds))

    def map_long_dev(self, d_pat, d_pat_off, npat, min_seed, d_hit_off, d_mapq, d_nchains, d_strand=None, d_seq=None, d_off=None, d_ts=None,
                     d_te=None, d_qs=None, d_qe=None, d_score=None, d_n=None, d_match=None, max_occ=500, max_gap=5000, band=500, min_score=40,
                     max_sec=0, thresholds=False):
        """device pointers: read bytes, npat+1 uint64 offsets -> npat+1 uint64 d_hit_off, npat uint8 d_mapq and uint64 d_nchains; the
        ten per-chain outputs (LONG_NAMES[3:]; room for d_hit_off[npat] each) all None: those three only"""
        self.ctx._check(self.lib.pfp_fm_map_long_dev(self._h, d_pat, d_pat_off, npat, min_seed, max_occ, max_gap, band, min_score, max_sec,
                                                     bool(thresholds), d_hit_off, d_mapq, d_nchains, d_strand, d_seq, d_off, d_ts, d_te, d_qs,
                                                     d_qe, d_score, d_n, d_match))

    def fill(self, patterns, seg_pat, q0, q1, t0, t1, max_fill):
        """the global alignment of stretches of patterns against stretches of the text (pfpgpu.h, "Aligning chains", 1): segment i
        is pattern seg_pat[i]'s bytes q0[i]:q1[i] against T[t0[i]:t1[i]] -> (dist, cig_off, cig): dist[i] (uint32) edits, at most
        max_fill (0 .. FM_FILL_MAX_F), and the runs cig[cig_off[i]:cig_off[i+1]] as cigar() gives them; 0xFFFFFFFF and no runs
        where the segment is not one of the pattern and the text, a side is longer than FM_FILL_MAX_LEN, or the two are more than
        max_fill edits apart"""
        _, _, args = self._host_patterns(patterns)
        sp = np.ascontiguousarray(seg_pat, dtype=np.uint32)
        cols = [np.ascontiguousarray(a, dtype=np.uint64) for a in (q0, q1, t0, t1)]
        if sp.ndim != 1 or any(a.shape != sp.shape for a in cols):
            raise ValueError("seg_pat, q0, q1, t0 and t1: five 1-D arrays of one length")
        ns = len(sp)
        dist, cig_off = np.zeros(ns, dtype=np.uint32), np.zeros(ns + 1, dtype=np.uint64)
        cig = C.POINTER(C.c_uint32)()
        self.ctx._check(self.lib.pfp_fm_fill(self._h, *args, sp, *cols, ns, max_fill, dist, cig_off, C.byref(cig)))
        return dist, cig_off, self._take_free(cig, cig_off[-1], np.uint32)

    def fill_dev(self, d_pat, d_pat_off, npat, d_seg_pat, d_q0, d_q1, d_t0, d_t1, nseg, max_fill, d_dist, d_cig_off, d_cig=None):
        """device pointers: pattern bytes, npat+1 uint64 offsets, nseg uint32 pattern indices and four uint64 arrays -> nseg uint32
        d_dist and nseg+1 uint64 d_cig_off; d_cig (uint32, room for d_cig_off[nseg]) gets the runs (None: offsets only)"""
        self.ctx._check(self.lib.pfp_fm_fill_dev(self._h, d_pat, d_pat_off, npat, d_seg_pat, d_q0, d_q1, d_t0, d_t1, nseg, max_fill, d_dist,
                                                 d_cig_off, d_cig))

    def fill_stats(self):
        """what the gap passes counted since the last call, under PFP_FM_MS_STATS=1 only: gaps, trivial gaps, and per band width
        (16, 32, 64, 256, 1024, 4160 cells) the gaps that went through a pass and the cells of those passes"""
        out = np.zeros(14, dtype=np.uint64)
        self.ctx._check(self.lib.pfp_fm_fill_stats(self._h, out))
        return {"gaps": int(out[0]), "trivial": int(out[1]), "widths": (16, 32, 64, 256, 1024, 4160),
                "passes": [int(v) for v in out[2:8]], "cells": [int(v) for v in out[8:14]]}

    def chain_align(self, patterns, anc_off, anc, max_gap=5000, band=500, min_score=40, max_chains=0, max_fill=500):
        """chain() and the edit script of every chain (pfpgpu.h, "Aligning chains", 2) -> the arrays CHAIN_ALN_NAMES names: chain()'s
        eight, then per chain i aqs[i] (uint32) and ats[i] (uint64), where its first anchor begins; nm[i] edits; unfilled[i] gaps
        that are more than max_fill edits and stand in the script as an insertion and a deletion; the runs
        cig[cig_off[i]:cig_off[i+1]], which align P[aqs[i]:qe[i]] to T[ats[i]:te[i]]; and its anchors mem[mem_off[i]:mem_off[i+1]]
        (uint32), in increasing order, as indices among the pattern's.  max_fill = 500 = the default band is a choice."""
        _, _, args = self._host_patterns(patterns)
        off = _arr(np.asarray(anc_off), np.uint64)
        a = _arr(np.asarray(anc).reshape(-1), np.uint64)
        npat = len(off) - 1
        if npat != args[2] or len(a) % 3:
            raise ValueError("anc_off: one offset more than the patterns; anc: three values per anchor")
        chain_off = np.zeros(npat + 1, dtype=np.uint64)
        u32, u64 = C.c_uint32, C.c_uint64
        kinds = (u32, u32, u32, u32, u64, u64, u32, u32, u64, u32, u32, u64, u32, u64, u32)
        ptrs = [C.POINTER(t)() for t in kinds]
        self.ctx._check(self.lib.pfp_fm_chain_align(self._h, *args, off, a, max_gap, band, min_score, max_chains, max_fill, chain_off,
                                                    *(C.byref(q) for q in ptrs)))
        total = int(chain_off[-1])
        out = [self._take_free(q, total, np.dtype(t)) for q, t in zip(ptrs[:11], kinds)]
        cig_off = self._take_free(ptrs[11], total + 1, np.uint64)
        cig = self._take_free(ptrs[12], cig_off[-1], np.uint32)
        mem_off = self._take_free(ptrs[13], total + 1, np.uint64)
        return (chain_off,) + tuple(out) + (cig_off, cig, mem_off, self._take_free(ptrs[14], mem_off[-1], np.uint32))

    def chain_align_dev(self, d_pat, d_pat_off, npat, d_anc_off, d_anc, d_chain_off, d_score=None, d_n=None, d_qs=None, d_qe=None, d_ts=None,
                        d_te=None, d_match=None, d_aqs=None, d_ats=None, d_nm=None, d_unfilled=None, d_cig_off=None, d_cig=None, d_mem_off=None,
                        d_mem=None, max_gap=5000, band=500, min_score=40, max_chains=0, max_fill=500):
        """device pointers: patterns, anchors as in chain_dev -> npat+1 uint64 d_chain_off; everything behind it None: offsets only;
        else the seven fields, d_aqs, d_ats, d_nm, d_unfilled (room for d_chain_off[npat]) and d_cig_off (one more) are required,
        d_cig (room for d_cig_off[last]), d_mem_off and d_mem may be None"""
        self.ctx._check(self.lib.pfp_fm_chain_align_dev(self._h, d_pat, d_pat_off, npat, d_anc_off, d_anc, max_gap, band, min_score, max_chains,
                                                        max_fill, d_chain_off, d_score, d_n, d_qs, d_qe, d_ts, d_te, d_match, d_aqs, d_ats, d_nm,
                                                        d_unfilled, d_cig_off, d_cig, d_mem_off, d_mem))

    def map_long_aln(self, patterns, min_seed, max_occ=500, max_gap=5000, band=500, min_score=40, max_sec=0, thresholds=False, max_fill=500):
        """map_long() and the edit script of every returned chain (pfpgpu.h, "Aligning chains", 3) -> the arrays LONG_ALN_NAMES
        names: map_long()'s thirteen, unchanged, then per returned chain i aqs[i], ats[i], nm[i], unfilled[i] and the runs
        cig[cig_off[i]:cig_off[i+1]] as chain_align gives them for the strand's pattern: the script reads along the text.  aqs is
        in the read as given: the script covers its bytes aqs[i]:qe[i] on strand 0 and qs[i]:aqs[i] on strand 1."""
        npat, _, args = self._host_patterns(patterns)
        hit_off, mapq, nchains = np.zeros(npat + 1, dtype=np.uint64), np.zeros(npat, dtype=np.uint8), np.zeros(npat, dtype=np.uint64)
        u8, u32, u64 = C.c_uint8, C.c_uint32, C.c_uint64
        kinds = (u8, u32, u64, u64, u64, u32, u32, u32, u32, u32, u32, u64, u32, u32, u64, u32)
        ptrs = [C.POINTER(t)() for t in kinds]
        self.ctx._check(self.lib.pfp_fm_map_long_aln(self._h, *args, min_seed, max_occ, max_gap, band, min_score, max_sec, bool(thresholds),
                                                     max_fill, hit_off, mapq, nchains, *(C.byref(q) for q in ptrs)))
        H = int(hit_off[-1])
        out = [self._take_free(q, H, np.dtype(t)) for q, t in zip(ptrs[:14], kinds)]
        cig_off = self._take_free(ptrs[14], H + 1, np.uint64)
        return (hit_off, mapq, nchains) + tuple(out) + (cig_off, self._take_free(ptrs[15], cig_off[-1], np.uint32))

    def map_long_aln_dev(self, d_pat, d_pat_off, npat, min_seed, d_hit_off, d_mapq, d_nchains, d_strand=None, d_seq=None, d_off=None, d_ts=None,
                         d_te=None, d_qs=None, d_qe=None, d_score=None, d_n=None, d_match=None, d_aqs=None, d_ats=None, d_nm=None,
                         d_unfilled=None, d_cig_off=None, d_cig=None, max_occ=500, max_gap=5000, band=500, min_score=40, max_sec=0,
                         thresholds=False, max_fill=500):
        """device pointers as in map_long_dev; behind its ten per-chain outputs d_aqs, d_ats, d_nm, d_unfilled (room for
        d_hit_off[npat]) and d_cig_off (one more), required with them; d_cig (room for d_cig_off[last]) may be None"""
        self.ctx._check(self.lib.pfp_fm_map_long_aln_dev(self._h, d_pat, d_pat_off, npat, min_seed, max_occ, max_gap, band, min_score, max_sec,
                                                         bool(thresholds), max_fill, d_hit_off, d_mapq, d_nchains, d_strand, d_seq, d_off, d_ts,
                                                         d_te, d_qs, d_qe, d_score, d_n, d_match, d_aqs, d_ats, d_nm, d_unfilled, d_cig_off,
                                                         d_cig))

    def set_sequences(self, starts):
        """give the index the sequence table of its collection (pfpgpu.h, "Sequences of a collection"): nseq + 1 starts, the
        first 0, non-decreasing, the last n; a second call replaces the table"""
        st = _arr(np.asarray(starts), np.uint64)
        self.ctx._check(self.lib.pfp_fm_set_seqs(self._h, st, max(len(st), 1) - 1))
        return self

    def set_sequences_file(self, path):
        """the same from a .seqs file (bigbwt -f --seqs writes it; host/seqs.h); -> the names (bytes), in table order"""
        names, starts = read_seqs_file(path, self.info()["n"])
        self.set_sequences(starts)
        return names

    def seqmap(self, positions):
        """-> (seq uint32, off uint64) of text positions; (2**32 - 1, 2**64 - 1) for a position >= n"""
        import torch
        pos = _arr(np.asarray(positions), np.uint64)
        dev = torch.device("cuda", self.ctx.device)
        d_pos = torch.from_numpy(pos.view(np.int64).copy()).to(dev)
        d_seq = torch.zeros(len(pos), dtype=torch.int32, device=dev)
        d_off = torch.zeros(len(pos), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        self.seqmap_dev(d_pos.data_ptr(), len(pos), d_seq.data_ptr(), d_off.data_ptr())
        return d_seq.cpu().numpy().view(np.uint32), d_off.cpu().numpy().view(np.uint64)

    def locate_seqs(self, patterns, max_occ=0, ranges=False):
        """-> (off, seq, offset): the hits of pattern p that lie inside one sequence, among the at most max_occ rows locate() would
        list (0: all), in row order, are (seq[i], offset[i]) for i in off[p]:off[p+1]; ranges=True: (off, seq, offset, sp, ep)"""
        npat, _, args = self._host_patterns(patterns)
        sp, ep = np.zeros(npat, dtype=np.uint64), np.zeros(npat, dtype=np.uint64)
        out_off = np.zeros(npat + 1, dtype=np.uint64)
        seq, off = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)()
        self.ctx._check(self.lib.pfp_fm_locate_seqs(self._h, *args, max_occ, sp, ep, out_off, C.byref(seq), C.byref(off)))
        seqs, offs = self._take_free(seq, out_off[-1], np.uint32), self._take_free(off, out_off[-1], np.uint64)
        return (out_off, seqs, offs, sp, ep) if ranges else (out_off, seqs, offs)

    def doclist(self, patterns):
        """-> (off, doc, cnt): the distinct sequences that hold a hit of pattern p inside one sequence are doc[off[p]:off[p+1]]
        (uint32, ascending) and cnt (uint64) their numbers of such hits; every occurrence counts"""
        npat, _, args = self._host_patterns(patterns)
        doc_off = np.zeros(npat + 1, dtype=np.uint64)
        doc, cnt = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint64)()
        self.ctx._check(self.lib.pfp_fm_doclist(self._h, *args, doc_off, C.byref(doc), C.byref(cnt)))
        return doc_off, self._take_free(doc, doc_off[-1], np.uint32), self._take_free(cnt, doc_off[-1], np.uint64)

    def seqmap_dev(self, d_pos, count, d_seq=None, d_off=None):
        """device pointers: count uint64 positions -> uint32 d_seq / uint64 d_off (either may be None)"""
        self.ctx._check(self.lib.pfp_fm_seqmap_dev(self._h, d_pos, count, d_seq, d_off))

    def locate_seqs_dev(self, d_pat_off, npat, d_sp, d_ep, d_first, max_occ, d_out_off, d_seq=None, d_off=None):
        """device pointers from count_dev -> npat+1 offsets of the kept hits; d_seq (uint32) / d_off (uint64), each with room for
        what locate_dev's offsets-only call reports, get them (both None: offsets only)"""
        self.ctx._check(self.lib.pfp_fm_locate_seqs_dev(self._h, d_pat_off, npat, d_sp, d_ep, d_first, max_occ, d_out_off, d_seq, d_off))

    def doclist_dev(self, d_pat_off, npat, d_sp, d_ep, d_first, d_doc_off, d_doc=None, d_cnt=None):
        """device pointers from count_dev -> npat+1 offsets of the documents; d_doc (uint32) / d_cnt (uint64), room for
        offsets[npat] each, get them (both None: offsets only)"""
        self.ctx._check(self.lib.pfp_fm_doclist_dev(self._h, d_pat_off, npat, d_sp, d_ep, d_first, d_doc_off, d_doc, d_cnt))

    def add_thresholds(self, thr=None):
        """give the index its thresholds (pfpgpu.h, "The LCP array and thresholds"): thr=None computes them on the GPU, else the
        bytes of a .thr_pos file (5 per run), or a path base whose base.thr_pos is read"""
        if thr is None:
            self.ctx._check(self.lib.pfp_fm_thresholds_dev(self._h, None, 0))
        elif isinstance(thr, (str, os.PathLike)):
            self.ctx._check(self.lib.pfp_fm_thresholds_files(self._h, os.fsencode(thr)))
        else:
            import torch
            d_thr5, nbytes, keep = self.ctx._upload_padded(thr)
            torch.cuda.synchronize()
            self.ctx._check(self.lib.pfp_fm_thresholds_dev(self._h, d_thr5, nbytes))
        return self

    def add_thresholds_dev(self, d_thr5, nbytes):
        """the same from a device image of a .thr_pos file (5 bytes per run)"""
        self.ctx._check(self.lib.pfp_fm_thresholds_dev(self._h, d_thr5, nbytes))
        return self

    def matching_statistics(self, patterns, thresholds=False):
        """-> (off, len, pos): for byte i of pattern p, len[off[p] + i] (uint32) is the length of the longest prefix of
        patterns[p][i:] that occurs in the text and pos[off[p] + i] (uint64) one place where it occurs (2**64 - 1 where the
        length is 0).  Needs an index with text (Context.fm_index_ms*).  thresholds=True: the two passes with thresholds
        (add_thresholds first): the same len, pos by their own rule."""
        _, off, args = self._host_patterns(patterns)
        total = int(off[-1])
        ln, pos = np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.uint64)
        call = self.lib.pfp_fm_ms_thr if thresholds else self.lib.pfp_fm_ms
        self.ctx._check(call(self._h, *args, ln, pos))
        return off, ln, pos

    def mems(self, patterns, min_len=1, thresholds=False):
        """-> (mem_off, mems): the maximal exact matches of pattern p of at least min_len bytes are the rows
        mems[mem_off[p]:mem_off[p+1]] of a (k, 3) uint64 array, each (i, len, pos), by increasing i; thresholds as in
        matching_statistics"""
        npat, _, args = self._host_patterns(patterns)
        mem_off = np.zeros(npat + 1, dtype=np.uint64)
        out = C.POINTER(C.c_uint64)()
        call = self.lib.pfp_fm_mems_thr if thresholds else self.lib.pfp_fm_mems
        self.ctx._check(call(self._h, *args, min_len, mem_off, C.byref(out)))
        return mem_off, self._take_free(out, 3 * int(mem_off[-1]), np.uint64).reshape(-1, 3)

    def ms_stats(self):
        """{launches, jumps, matched} of the matching-statistics calls (and add_thresholds) since the last look; jumps (steps
        that took step 3) and matched (bytes the extensions matched) are collected only under PFP_FM_MS_STATS=1"""
        out = (C.c_uint64 * 3)()
        self.ctx._check(self.lib.pfp_fm_ms_stats(self._h, out))
        return dict(launches=int(out[0]), jumps=int(out[1]), matched=int(out[2]))

    def matching_statistics_dev(self, d_pat, d_pat_off, npat, d_len, d_pos=None, thresholds=False):
        """device pointers: pattern bytes, npat+1 uint64 offsets -> uint32 d_len / uint64 d_pos, entry t for pattern byte d_pat[t]"""
        call = self.lib.pfp_fm_ms_thr_dev if thresholds else self.lib.pfp_fm_ms_dev
        self.ctx._check(call(self._h, d_pat, d_pat_off, npat, d_len, d_pos))

    def mems_dev(self, d_pat_off, npat, d_len, d_pos, min_len, d_mem_off, d_mem=None):
        """device pointers from matching_statistics_dev -> npat+1 offsets; d_mem (room for 3 * offsets[npat] uint64) gets the
        triples (None: offsets only)"""
        self.ctx._check(self.lib.pfp_fm_mems_dev(self._h, d_pat_off, npat, d_len, d_pos, min_len, d_mem_off, d_mem))

    def count_dev(self, d_pat, d_pat_off, npat, d_sp, d_ep, d_first=None):
        """device pointers: pattern bytes, npat+1 uint64 offsets -> npat uint64 sp / ep (and SA[sp] where d_first is given)"""
        self.ctx._check(self.lib.pfp_fm_count_dev(self._h, d_pat, d_pat_off, npat, d_sp, d_ep, d_first))

    def locate_dev(self, npat, d_sp, d_ep, d_first, max_occ, d_out_off, d_pos=None):
        """device pointers from count_dev -> npat+1 offsets; d_pos (room for offsets[npat]) gets the positions (None: offsets only)"""
        self.ctx._check(self.lib.pfp_fm_locate_dev(self._h, npat, d_sp, d_ep, d_first, max_occ, d_out_off, d_pos))


_lib = None


def load_library():
    """dlopen libpfpgpu.so (built in-tree by __graft_entry__.build / csrc/Makefile) and give its functions the signatures of abi.py."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                              f"(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        # PyTorch wheels bundle their own HIP runtime (torch/lib/libamdhip64.so, soname
        # libamdhip64.so.7).  Two HIP runtimes in one process cannot both own the GPU, so when
        # torch is installed it is imported FIRST: libpfpgpu.so's DT_NEEDED libamdhip64.so.7 then
        # binds to the runtime torch already loaded and both share devices, streams and memory.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(lib, name):
                raise ImportError(f"{LIB_PATH} does not export {name}, which include/pfpgpu.h declares")
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
    return _lib


def _arr(a, dtype):
    if isinstance(a, (bytes, bytearray, memoryview)):
        a = np.frombuffer(a, dtype=np.uint8)
    a = np.ascontiguousarray(a)
    if a.dtype != dtype:
        a = a.astype(dtype) if dtype != np.uint8 or a.dtype.itemsize == 1 else a.view(np.uint8)
    return a


def _take(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(int(n),)).astype(dtype, copy=True)


def _adopt(lib, ptr, n):
    """a malloc'ed result buffer of the library as a numpy array WITHOUT copying it (a copy of a 0.8 GB .bwt costs more
    than its trip across PCIe); the buffer is handed to pfp_free when the array is collected"""
    if n == 0 or not ptr:
        return np.zeros(0, dtype=np.uint8)
    import weakref
    arr = np.ctypeslib.as_array(ptr, shape=(int(n),))
    weakref.finalize(arr, lib.pfp_free, _addr(ptr))
    return arr


def _text_nul(text):
    """-> (the text's bytes and one NUL: never a NULL pointer, for an empty text neither; the text's length)"""
    t = _arr(text, np.uint8)
    return np.concatenate([t, np.zeros(1, dtype=np.uint8)]), len(t)


def _sort_info(info):
    """out_info of pfp_dist_global_sort / pfp_dist_global_sort_distinct"""
    return dict(words=int(info[0]), dict_bytes=int(info[1]), rounds=int(info[2]), complete=bool(info[3]), slots=int(info[4]),
                slot_base=int(info[5]), emits=int(info[6]), index_bits=int(info[7]))


def _local_sizes(sizes):
    """out_sizes of pfp_dist_local_parse / pfp_dist_local_parse2"""
    return dict(dict_bytes=int(sizes[0]), words=int(sizes[1]), phrases=int(sizes[2]), last_trigger=int(sizes[3]))


def unpack5(b):
    """5-byte little-endian ints (utils.c:112-129) -> u64 array"""
    b = np.frombuffer(bytes(b), dtype=np.uint8).reshape(-1, 5)
    out = np.zeros((len(b), 8), dtype=np.uint8)
    out[:, :5] = b
    return out.view(np.uint64).reshape(-1)


def pack5(v):
    v = np.ascontiguousarray(v, dtype=np.uint64).reshape(-1)
    return v.view(np.uint8).reshape(-1, 8)[:, :5].copy().reshape(-1)


class Context(_Closing):
    """One HIP stream + memory pool on one GPU (pfp_ctx)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self._h = C.c_void_p()
        rc = self.lib.pfp_ctx_create(C.byref(self._h), device)
        if rc:
            raise PfpError(rc, "pfp_ctx_create failed: " + self.lib.pfp_strerror(rc).decode() +
                           " (the HIP path is mandatory; no CPU fallback exists)")
        self.device = device

    def close(self):
        if self._h:
            self.lib.pfp_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def _check(self, rc):
        if rc:
            raise PfpError(rc, self.lib.pfp_last_error(self._h).decode(errors="replace"))

    def _upload_padded(self, a):
        """host bytes -> (address, length, t): t, a zeroed uint8 torch tensor of length + 16 bytes on the context's device, begins
        with them; (None, 0, None) for None.  torch fills t on its own stream: torch.cuda.synchronize before the library reads it."""
        if a is None:
            return None, 0, None
        import torch
        b = _arr(a, np.uint8)
        t = torch.zeros(len(b) + 16, dtype=torch.uint8, device=torch.device("cuda", self.device))
        if len(b):
            t[:len(b)] = torch.from_numpy(b.copy())
        return t.data_ptr(), len(b), t

    @property
    def stream(self):
        return self.lib.pfp_ctx_stream(self._h)

    def debug_check(self):
        """PFP_POOL_DEBUG=1: raise if a canary band of any released device block was damaged"""
        self._check(self.lib.pfp_debug_check(self._h))

    def pool_trim(self):
        self.lib.pfp_pool_trim(self._h)

    def mem_stats(self):
        out = (C.c_uint64 * 4)()
        self._check(self.lib.pfp_get_mem_stats(self._h, out))
        return dict(held=int(out[0]), peak=int(out[1]), live=int(out[2]), debug_blocks=int(out[3]))

    def pool_counters(self):
        out = (C.c_uint64 * 2)()
        self._check(self.lib.pfp_get_pool_counters(self._h, out))
        return dict(driver_allocs=int(out[0]), trims=int(out[1]))

    def set_profiling(self, on=True):
        self.lib.pfp_set_profiling(self._h, bool(on))

    def set_kernel_trace(self, on=True):
        """start (and clear) / stop per-kernel HIP-event timing on the ctx stream"""
        self.lib.pfp_set_kernel_trace(self._h, bool(on))

    def kernel_trace(self):
        """rows {name, launches, total_ms, algo_bytes} accumulated since set_kernel_trace(True)"""
        n = self.lib.pfp_get_kernel_trace(self._h, None, 0)
        if n <= 0:
            return []
        arr = (KernelStat * n)()
        self.lib.pfp_get_kernel_trace(self._h, arr, n)
        return [dict(name=r.name.decode(), launches=int(r.launches), total_ms=float(r.total_ms), algo_bytes=int(r.algo_bytes))
                for r in arr]

    def set_max_phrase(self, max_phrase):
        """fused chain: split phrases longer than this with extra trigger windows (0 = reference parse)"""
        self.lib.pfp_set_max_phrase(self._h, max_phrase)

    def set_window_hash(self, fast):
        """fused chain: cut the text by the cheap window hash (True, default) or by the reference's Karp-Rabin hash (False)"""
        self.lib.pfp_set_window_hash(self._h, bool(fast))

    LIB_SORT_KINDS = {"pairs_u64_u32": (0, np.uint64, np.uint32), "pairs_u64_u64": (1, np.uint64, np.uint64), "keys_db": (2, np.uint64, None),
                      "keys_raw": (3, np.uint64, None), "seg_u32_u32": (4, np.uint32, np.uint32), "seg_u32_u64": (5, np.uint32, np.uint64),
                      "seg_u64_u32": (6, np.uint64, np.uint32), "inclusive_max_u32": (7, np.uint32, None),
                      "exclusive_sum_u32_u64": (8, np.uint32, np.uint64), "select_index": (9, np.uint8, np.uint32)}

    def debug_lib_sort(self, kind, keys, vals=None, begin_bit=0, end_bit=64, seg_begin=None, seg_end=None):
        """the library sorts / scans / selection behind prims.hip's wrappers on numpy arrays, in place (pfpgpu.h: pfp_debug_lib_sort);
        select_index wants n + 1 values (the count comes back in the last one)"""
        code, kt, vt = self.LIB_SORT_KINDS[kind]
        n = len(keys)
        assert keys.dtype == kt and keys.flags.c_contiguous
        assert (vals is None and vt is None) or (vals.dtype == vt and vals.flags.c_contiguous and len(vals) == n + (code == 9))
        nseg = 0
        if seg_begin is not None:
            assert seg_begin.dtype == np.uint32 and seg_end.dtype == np.uint32 and len(seg_begin) == len(seg_end)
            assert seg_begin.flags.c_contiguous and seg_end.flags.c_contiguous
            nseg = len(seg_begin)
        self._check(self.lib.pfp_debug_lib_sort(self._h, code, keys.ctypes.data, vals.ctypes.data if vals is not None else None, n,
                                                begin_bit, end_bit, seg_begin if nseg else None, seg_end if nseg else None, nseg))

    def debug_scan_chain(self, text, w=10, p=100, plan=None, extra=()):
        """stage 1a as the fused chain runs it under the context's settings - or, with a settled plan, as a rank of the multi-GPU
        chain runs it - and what it did (pfpgpu.h: pfp_debug_scan_chain): a dict of the report's fields plus `ends`, `extra` and,
        where a density choice was made, `dense_ends` and `nominal` (else None)"""
        t = _arr(text, np.uint8)
        ends, dends, nom = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint8)()
        rep = ScanReport()
        pl = (C.c_uint64 * 4)(*plan) if plan is not None else None
        ex = np.ascontiguousarray(np.array(list(extra), dtype=np.uint32))
        rc = self.lib.pfp_debug_scan_chain(self._h, t, len(t), w, p, pl, ex if len(ex) else None, len(ex),
                                           C.byref(ends), C.byref(dends), C.byref(nom), C.byref(rep))
        try:
            self._check(rc)
            out = {k: getattr(rep, k) for k, _ in ScanReport._fields_ if k not in ("extra", "reserved")}
            out["extra"] = [int(rep.extra[q]) for q in range(rep.n_extra)]
            out["ends"] = _take(ends, rep.n_ends, np.uint64)
            out["dense_ends"] = _take(dends, rep.dense_cuts, np.uint64) if dends else None
            out["nominal"] = _take(nom, rep.dense_cuts, np.uint8) if nom else None
        finally:
            self.lib.pfp_free(ends)
            self.lib.pfp_free(dends)
            self.lib.pfp_free(nom)
        return out

    def set_parse_density(self, density):
        """fused chain, opt-in: the window hash cuts with probability density / p (outputs unchanged, see pfpgpu.h)"""
        self._check(self.lib.pfp_set_parse_density(self._h, density))

    def set_index_bits(self, bits):
        """0: index width by size (32 bits below 4 GiB), 64: always the wide build (bigbwt:109-151)"""
        self._check(self.lib.pfp_set_index_bits(self._h, bits))

    def stats(self):
        st = Stats()
        self._check(self.lib.pfp_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    # -- stage 1a: newscan.cpp:168-202, 363-377
    def scan(self, text, w=10, p=100):
        t = _arr(text, np.uint8)
        ends = C.POINTER(C.c_uint64)()
        ne, used = C.c_uint64(), C.c_uint64()
        self._check(self.lib.pfp_scan(self._h, t, len(t), w, p, C.byref(ends), C.byref(ne), C.byref(used)))
        out = _take(ends, ne.value, np.uint64)
        self.lib.pfp_free(ends)
        return out, used.value

    # -- stage 1: newscan.cpp main
    def parse(self, text, w=10, p=100, want_sai=False):
        t = _arr(text, np.uint8)
        r = _ParseResult()
        self._check(self.lib.pfp_parse(self._h, t, len(t), w, p, bool(want_sai), C.byref(r)))
        out = dict(n_used=int(r.n_used), dict=_take(r.dict, r.dict_size, np.uint8), occ=_take(r.occ, r.n_words, np.uint32),
                   parse=_take(r.parse, r.n_phrases, np.uint32), last=_take(r.last, r.n_phrases, np.uint8),
                   sai=_take(r.sai, 5 * r.n_phrases, np.uint8) if want_sai else None)
        self.lib.pfp_parse_result_free(C.byref(r))
        return out

    # -- gsa/gsacak.h, and its -DM64 build (the names that end in 64): 64-bit SA entries
    def _suffix_array(self, name, s, s_dtype, sa_dtype, *k):
        s = _arr(s, s_dtype)
        sa = np.zeros(len(s), dtype=sa_dtype)
        self._check(getattr(self.lib, name)(self._h, s, sa, len(s), *k))
        return sa

    def sacak_int(self, s, k=0):
        return self._suffix_array("pfp_sacak_int", s, np.uint32, np.uint32, k)

    def sacak(self, s):
        return self._suffix_array("pfp_sacak", s, np.uint8, np.uint32)

    def gsacak(self, s):
        return self._suffix_array("pfp_gsacak", s, np.uint8, np.uint32)

    def sacak_int64(self, s, k=0):
        return self._suffix_array("pfp_sacak_int64", s, np.uint32, np.uint64, k)

    def sacak64(self, s):
        return self._suffix_array("pfp_sacak64", s, np.uint8, np.uint64)

    def gsacak64(self, s):
        return self._suffix_array("pfp_gsacak64", s, np.uint8, np.uint64)

    def gsacak_lcp_da(self, s, wide=False):
        """gsacak(s, SA, LCP, DA, n) with all three outputs (gsa/gsacak.h:96-105)"""
        s = _arr(s, np.uint8)
        it, ut, fn = (np.int64, np.uint64, self.lib.pfp_gsacak_lcp_da64) if wide else (np.int32, np.uint32, self.lib.pfp_gsacak_lcp_da)
        sa = np.zeros(len(s), dtype=ut); lcp = np.zeros(len(s), dtype=it); da = np.zeros(len(s), dtype=it)
        self._check(fn(self._h, s, sa, lcp, da, len(s)))
        return sa, lcp, da

    # -- stage 2: bwtparse.c main
    def bwtparse(self, parse, last, occ, sai=None):
        parse = _arr(parse, np.uint32); last = _arr(last, np.uint8); occ = _arr(occ, np.uint32)
        P = len(parse)
        ilist = np.zeros(P + 1, dtype=np.uint32)
        bwlast = np.zeros(P + 1, dtype=np.uint8)
        bwsai = np.zeros(5 * (P + 1), dtype=np.uint8) if sai is not None else None
        sai_a = _arr(sai, np.uint8) if sai is not None else None
        self._check(self.lib.pfp_bwtparse(self._h, parse, P, last, sai_a, occ, len(occ), ilist, bwlast, bwsai))
        return ilist, bwlast, bwsai

    def _bwt_result(self, r):
        return dict(bwt=_adopt(self.lib, r.bwt, r.bwt_size), sa=_adopt(self.lib, r.sa, r.sa_bytes),
                    ssa=_adopt(self.lib, r.ssa, r.ssa_bytes), esa=_adopt(self.lib, r.esa, r.esa_bytes))

    # -- stage 3: pfbwt.cpp main
    def merge(self, dict_, occ, ilist, bwlast, bwsai=None, w=10, flags=0):
        d = _arr(dict_, np.uint8); occ = _arr(occ, np.uint32); ilist = _arr(ilist, np.uint32); bwlast = _arr(bwlast, np.uint8)
        bs = _arr(bwsai, np.uint8) if bwsai is not None else None
        r = _BwtResult()
        self._check(self.lib.pfp_merge(self._h, d, len(d), occ, len(occ), ilist, bwlast, bs, len(ilist), w, flags, C.byref(r)))
        return self._bwt_result(r)

    # -- bigbwt chain, host buffers
    def bigbwt(self, text, w=10, p=100, flags=0):
        t = _arr(text, np.uint8)
        r = _BwtResult()
        self._check(self.lib.pfp_bigbwt(self._h, t, len(t), w, p, flags, C.byref(r)))
        return self._bwt_result(r)

    def bigbwt_files(self, text, base, w=10, p=100, flags=0):
        """host text in, <base>.bwt/.sa/.ssa/.esa out (streamed from HBM); returns the sizes written"""
        t = _arr(text, np.uint8)
        sizes = (C.c_uint64 * 4)()
        self._check(self.lib.pfp_bigbwt_files(self._h, t, len(t), w, p, flags, os.fsencode(base), sizes))
        return dict(bwt=int(sizes[0]), sa=int(sizes[1]), ssa=int(sizes[2]), esa=int(sizes[3]))

    # -- bigbwt chain, device-resident (raw device pointers, e.g. torch tensor.data_ptr())
    def bigbwt_dev(self, d_text_ptr, n, d_bwt_ptr, d_sa_ptr=None, w=10, p=100, flags=0):
        used = C.c_uint64()
        self._check(self.lib.pfp_bigbwt_dev(self._h, d_text_ptr, n, w, p, flags, d_bwt_ptr, d_sa_ptr, C.byref(used)))
        return used.value

    def bigbwt_formats_dev(self, d_text_ptr, n, d_bwt_ptr, w=10, p=100, flags=0):
        """device text in, .bwt into d_bwt, .sa/.ssa/.esa as library-owned device buffers: -> (n_used, {name: (ptr, bytes)});
        release every ptr with dev_free"""
        used, outs, sizes = C.c_uint64(), (C.c_void_p * 3)(), (C.c_uint64 * 3)()
        self._check(self.lib.pfp_bigbwt_formats_dev(self._h, d_text_ptr, n, w, p, flags, d_bwt_ptr, outs, sizes, C.byref(used)))
        return used.value, {k: (outs[i], int(sizes[i])) for i, k in enumerate(("sa", "ssa", "esa")) if outs[i]}

    def fetch_dev(self, d_ptr, nbytes):
        """device bytes (a buffer the library handed out) -> numpy uint8 array"""
        out = np.empty(int(nbytes), dtype=np.uint8)
        self._check(self.lib.pfp_memcpy_d2h(self._h, out.ctypes.data, d_ptr, nbytes))
        return out

    def dev_free(self, d_ptr):
        self.lib.pfp_dev_free(self._h, d_ptr)

    def pack5_dev(self, d_vals_ptr, count, d_out5_ptr):
        """count u64 device values -> 5-byte LE ints in device memory (utils.c:112-129)"""
        self._check(self.lib.pfp_pack5_dev(self._h, d_vals_ptr, count, d_out5_ptr))

    def sample_runs_dev(self, d_bwt_ptr, d_sa_ptr, count, pos_base=0, left=-1, right=-1, run_end=False, d_out10_ptr=None, cap_pairs=0):
        """.ssa / .esa pairs of a BWT slice in device memory (pfbwt.cpp:605-676); returns the number of pairs"""
        k = C.c_uint64()
        self._check(self.lib.pfp_sample_runs_dev(self._h, d_bwt_ptr, d_sa_ptr, count, pos_base, left, right, bool(run_end),
                                                 d_out10_ptr, cap_pairs, C.byref(k)))
        return k.value

    def pwrite_dev(self, path, file_offset, d_src_ptr, nbytes):
        """device bytes -> file at an offset (pfthreads.hpp:369-376 pattern), through pinned staging buffers"""
        self._check(self.lib.pfp_pwrite_dev(self._h, os.fsencode(path), file_offset, d_src_ptr, nbytes))

    # -- inverting / checking a BWT (the reference's readme: "check the correctness of the BWT by ... inverting it")
    def unbwt(self, bwt):
        """host .bwt bytes (n+1, one 0) -> the text (numpy uint8, n bytes); PfpError(PFP_EFORMAT) if they are not a BWT"""
        b = _arr(bwt, np.uint8)
        out = np.empty(max(len(b) - 1, 0), dtype=np.uint8)
        self._check(self.lib.pfp_unbwt(self._h, b if len(b) else None, len(b), out if len(out) else None))
        return out

    def unbwt_dev(self, d_bwt_ptr, n_plus_1, d_text_ptr):
        """device .bwt (n_plus_1 bytes) -> device text (n_plus_1 - 1 bytes)"""
        self._check(self.lib.pfp_unbwt_dev(self._h, d_bwt_ptr, n_plus_1, d_text_ptr))

    def check_bwt_dev(self, d_bwt_ptr, n_plus_1, d_text_ptr=None, d_sa5_ptr=None, d_ssa10_ptr=None, ssa_bytes=0, d_esa10_ptr=None, esa_bytes=0):
        """invert a device .bwt and compare with whatever is given (device pointers): -> dict of pfp_check_result"""
        r = CheckResult()
        self._check(self.lib.pfp_check_bwt_dev(self._h, d_bwt_ptr, n_plus_1, d_text_ptr, d_sa5_ptr, d_ssa10_ptr, ssa_bytes, d_esa10_ptr,
                                               esa_bytes, C.byref(r)))
        return r.as_dict()

    def check_bwt_files(self, base, text, flags=0):
        """<base>.bwt (and .sa / .ssa / .esa as flags ask) against a host text: -> dict of pfp_check_result"""
        t = _arr(text, np.uint8)
        r = CheckResult()
        self._check(self.lib.pfp_check_bwt_files(self._h, os.fsencode(base), t if len(t) else None, -1, 0, len(t), flags, C.byref(r)))
        return r.as_dict()

    # -- searching a BWT (csrc/fmsearch.hip): count and locate, pfpgpu.h states the definitions
    def fm_index(self, bwt, ssa=None, esa=None):
        """an FmIndex over host .bwt bytes and, for locate, the .ssa / .esa bytes (bigbwt -s -e); the index keeps its own copy"""
        import torch
        up = [self._upload_padded(a) for a in (bwt, ssa, esa)]
        torch.cuda.synchronize(torch.device("cuda", self.device))
        return self.fm_index_dev(*up[0][:2], *up[1][:2], *up[2][:2])

    def fm_index_dev(self, d_bwt, n_plus_1, d_ssa10=None, ssa_bytes=0, d_esa10=None, esa_bytes=0):
        """an FmIndex over device buffers (copied: the caller may free them afterwards)"""
        h = C.c_void_p()
        self._check(self.lib.pfp_fm_build_dev(self._h, d_bwt, n_plus_1, d_ssa10, ssa_bytes, d_esa10, esa_bytes, C.byref(h)))
        return FmIndex(self, h)

    def fm_index_files(self, base, flags=0):
        """an FmIndex over <base>.bwt and, when flags holds FLAG_SSA | FLAG_ESA, <base>.ssa / .esa"""
        h = C.c_void_p()
        self._check(self.lib.pfp_fm_build_files(self._h, os.fsencode(base), flags, C.byref(h)))
        return FmIndex(self, h)

    # -- matching statistics and MEMs: an index that also keeps the text and the run-end values
    def fm_index_ms(self, bwt, ssa, esa, text=None):
        """an FmIndex for matching_statistics / mems over host .bwt, .ssa and .esa bytes; text=None: the text is inverted from
        the BWT on the GPU, else a numpy array / bytes of len(bwt) - 1 bytes"""
        import torch
        if ssa is None or esa is None:
            raise PfpError(-1, "matching statistics need the run samples: .ssa and .esa (bigbwt -s -e writes them)")
        up = [self._upload_padded(a) for a in (bwt, ssa, esa, text)]
        self._text_fits(text, up)
        torch.cuda.synchronize(torch.device("cuda", self.device))
        return self.fm_index_ms_dev(*up[0][:2], *up[1][:2], *up[2][:2], up[3][0])

    @staticmethod
    def _text_fits(text, up):
        """up: the uploads of (bwt, ssa, esa, text)"""
        if text is not None and up[3][1] + 1 != up[0][1]:
            raise PfpError(-1, f"the text holds {up[3][1]} bytes; the BWT holds {up[0][1]} rows, so its text holds {max(up[0][1], 1) - 1}")

    def fm_index_ms_dev(self, d_bwt, n_plus_1, d_ssa10, ssa_bytes, d_esa10, esa_bytes, d_text=None):
        """the same over device buffers (copied); d_text: n_plus_1 - 1 device bytes, None: inverted"""
        h = C.c_void_p()
        self._check(self.lib.pfp_fm_build_ms_dev(self._h, d_bwt, n_plus_1, d_ssa10, ssa_bytes, d_esa10, esa_bytes, d_text, C.byref(h)))
        return FmIndex(self, h)

    def fm_index_ms_files(self, base, text=None):
        """the same over <base>.bwt / .ssa / .esa; text=None: inverted"""
        h = C.c_void_p()
        buf, n = _text_nul(text) if text is not None else (None, 0)
        self._check(self.lib.pfp_fm_build_ms_files(self._h, os.fsencode(base), buf, -1, 0, n, C.byref(h)))
        return FmIndex(self, h)

    # -- the LCP array and thresholds (csrc/lcp.hip; pfpgpu.h states the definitions)
    def lcp(self, bwt, ssa, esa, text=None, want=("lcp", "thr")):
        """host .bwt / .ssa / .esa bytes (text=None: inverted) -> dict with "lcp" (n + 1 uint64) and / or "thr" (one uint64 per run)"""
        import torch
        dev = torch.device("cuda", self.device)
        up = [self._upload_padded(a) for a in (bwt, ssa, esa, text)]
        if ssa is None or esa is None:
            raise PfpError(-1, "the LCP array needs the run samples: .ssa and .esa (bigbwt -s -e writes them)")
        self._text_fits(text, up)
        n1 = up[0][1]
        args = (*up[0][:2], *up[1][:2], *up[2][:2], up[3][0])
        runs = up[1][1] // 10          # (a .ssa of another size is refused before anything is written)
        d_lcp = torch.zeros(n1 + 1, dtype=torch.int64, device=dev) if "lcp" in want else None
        d_thr = torch.zeros(runs + 1, dtype=torch.int64, device=dev) if "thr" in want else None
        torch.cuda.synchronize(dev)
        runs = self.lcp_dev(*args, d_lcp=d_lcp.data_ptr() if d_lcp is not None else None, d_thr=d_thr.data_ptr() if d_thr is not None else None)
        out = {}
        if d_lcp is not None:
            out["lcp"] = d_lcp[:n1].cpu().numpy().view(np.uint64)
        if d_thr is not None:
            out["thr"] = d_thr[:runs].cpu().numpy().view(np.uint64)
        return out

    def lcp_dev(self, d_bwt, n_plus_1, d_ssa10, ssa_bytes, d_esa10, esa_bytes, d_text=None, d_lcp=None, d_thr=None):
        """device pointers; d_lcp: room for n_plus_1 uint64, d_thr: one uint64 per run; -> the number of runs (both None: only that)"""
        runs = C.c_uint64()
        self._check(self.lib.pfp_lcp_dev(self._h, d_bwt, n_plus_1, d_ssa10, ssa_bytes, d_esa10, esa_bytes, d_text, d_lcp, d_thr, C.byref(runs)))
        return int(runs.value)

    def lcp_files(self, base, text=None, want=("lcp", "thr")):
        """<base>.bwt / .ssa / .esa (text=None: inverted) -> <base>.lcp and / or <base>.thr_pos, 5-byte ints"""
        what = (LCP_LCP if "lcp" in want else 0) | (LCP_THR if "thr" in want else 0)
        buf, n = _text_nul(text) if text is not None else (None, 0)
        self._check(self.lib.pfp_lcp_files(self._h, os.fsencode(base), buf, -1, 0, n, what))

    # -- multi-GPU chain, one rank's share (device pointers; collectives are the caller's: dist.py)
    def dist_propose_triggers(self, d_text_ptr, n, w, p):
        hashes, cnt = (C.c_uint32 * 8)(), C.c_uint32()
        self._check(self.lib.pfp_dist_propose_triggers(self._h, d_text_ptr, n, w, p, hashes, C.byref(cnt)))
        return [int(hashes[i]) for i in range(cnt.value)]

    def dist_local_parse(self, d_text_ptr, n, halo_len, w, p, is_first, is_last, global_offset, want_sai, extra=()):
        sizes, ex = (C.c_uint64 * 4)(), (C.c_uint32 * max(1, len(extra)))(*extra)
        self._check(self.lib.pfp_dist_local_parse(self._h, d_text_ptr, n, halo_len, w, p, int(is_first), int(is_last), global_offset,
                                                  int(want_sai), ex, len(extra), sizes))
        return _local_sizes(sizes)

    def dist_parse_plan(self, first_bytes, w, p, ranks=1):
        """rank 0: (plan, first_hash) from the text's first bytes (pfp_dist_parse_plan); plan = four 64-bit integers"""
        fb = np.ascontiguousarray(np.frombuffer(bytes(first_bytes), dtype=np.uint8))
        plan, fh = (C.c_uint64 * 4)(), C.c_uint64()
        self._check(self.lib.pfp_dist_parse_plan(self._h, fb if len(fb) else None, len(fb), w, p, ranks, plan, C.byref(fh)))
        return [int(x) for x in plan], int(fh.value)

    def dist_propose_triggers2(self, d_text_ptr, n, halo_len, w, p, plan, d_sample_ptr, sample_cap):
        hashes, cnt, ns = (C.c_uint32 * 8)(), C.c_uint32(), C.c_uint64()
        pl = (C.c_uint64 * 4)(*plan)
        self._check(self.lib.pfp_dist_propose_triggers2(self._h, d_text_ptr, n, halo_len, w, p, pl, hashes, C.byref(cnt),
                                                        d_sample_ptr if sample_cap else None, sample_cap, C.byref(ns)))
        return [int(hashes[i]) for i in range(cnt.value)], int(ns.value)

    def dist_decide_density(self, d_samples_ptr, count, p, plan):
        pl = (C.c_uint64 * 4)(*plan)
        self._check(self.lib.pfp_dist_decide_density(self._h, d_samples_ptr if count else None, count, p, pl))
        return [int(x) for x in pl]

    def dist_local_parse2(self, d_text_ptr, n, halo_len, w, p, is_first, is_last, global_offset, want_sai, plan, extra=()):
        sizes, ex, pl = (C.c_uint64 * 4)(), (C.c_uint32 * max(1, len(extra)))(*extra), (C.c_uint64 * 4)(*plan)
        self._check(self.lib.pfp_dist_local_parse2(self._h, d_text_ptr, n, halo_len, w, p, int(is_first), int(is_last), global_offset,
                                                   int(want_sai), pl, ex, len(extra), sizes))
        return _local_sizes(sizes)

    def dist_export_local(self, d_dict=None, d_occ=None, d_last=None, d_sai=None):
        self._check(self.lib.pfp_dist_export_local(self._h, d_dict, d_occ, d_last, d_sai))

    def dist_global(self, d_union, union_bytes, d_union_occ, n_union, my_word_base, d_sym_out):
        info = (C.c_uint64 * 3)()
        self._check(self.lib.pfp_dist_global(self._h, d_union, union_bytes, d_union_occ, n_union, my_word_base, d_sym_out, info))
        return dict(words=int(info[0]), dict_bytes=int(info[1]), rounds=int(info[2]))

    def dist_global_sort(self, d_union, union_bytes, d_union_occ, n_union, part, parts, d_wslot_out):
        info = (C.c_uint64 * 8)()
        self._check(self.lib.pfp_dist_global_sort(self._h, d_union, union_bytes, d_union_occ, n_union, part, parts, d_wslot_out, info))
        return _sort_info(info)

    def dist_partition_words(self, parts):
        """-> [(words, bytes)] this rank sends to every owner (hash-partitioned dedup)"""
        cnt = (C.c_uint64 * (2 * parts))()
        self._check(self.lib.pfp_dist_partition_words(self._h, parts, cnt))
        return [(int(cnt[2 * o]), int(cnt[2 * o + 1])) for o in range(parts)]

    def dist_export_partition(self, d_bytes, d_occ):
        self._check(self.lib.pfp_dist_export_partition(self._h, d_bytes, d_occ))

    def dist_owner_dedup(self, d_bytes, nbytes, d_occ, n_words, d_pid_out):
        out = (C.c_uint64 * 2)()
        self._check(self.lib.pfp_dist_owner_dedup(self._h, d_bytes, nbytes, d_occ, n_words, d_pid_out, out))
        return int(out[0]), int(out[1])

    def dist_export_owned(self, d_bytes, d_occ):
        self._check(self.lib.pfp_dist_export_owned(self._h, d_bytes, d_occ))

    def dist_global_sort_distinct(self, d_dict, dict_bytes, d_occ, n_words, d_gid_sent, part, parts, d_wslot_out):
        info = (C.c_uint64 * 8)()
        self._check(self.lib.pfp_dist_global_sort_distinct(self._h, d_dict, dict_bytes, d_occ, n_words, d_gid_sent, part, parts,
                                                           d_wslot_out, info))
        return _sort_info(info)

    def dist_global_finish(self, d_wslot_all, parts, my_word_base, d_sym_out):
        self._check(self.lib.pfp_dist_global_finish(self._h, d_wslot_all, parts, my_word_base, d_sym_out))

    def dist_parse_sort(self, d_sym, P, part, parts, d_sa_out):
        info = (C.c_uint64 * 4)()
        self._check(self.lib.pfp_dist_parse_sort(self._h, d_sym, P, part, parts, d_sa_out, info))
        return dict(entries=int(info[0]), slot_base=int(info[1]), complete=bool(info[2]), rounds=int(info[3]))

    def dist_set_parse_sa(self, d_sa, count):
        self._check(self.lib.pfp_dist_set_parse_sa(self._h, d_sa if count else None, count))

    def dist_merge(self, d_sym, P, d_last, d_sai, flags, n_total, out_lo, out_hi, d_bwt_slice, d_sa_slice=None):
        self._check(self.lib.pfp_dist_merge(self._h, d_sym, P, d_last, d_sai, flags, n_total, out_lo, out_hi, d_bwt_slice, d_sa_slice))

    def dist_sample_runs(self, run_end, drop_edge, d_out10_ptr=None, cap_pairs=0):
        """.ssa / .esa pairs of the slice the last dist_merge emitted (-s / -e without an SA slice), from its run maps;
        returns the number of pairs (count only without an output pointer)"""
        k = C.c_uint64()
        self._check(self.lib.pfp_dist_sample_runs(self._h, bool(run_end), bool(drop_edge), d_out10_ptr, cap_pairs, C.byref(k)))
        return k.value

    def dist_release(self):
        self.lib.pfp_dist_release(self._h)

    def stage_text_dev(self, d_text_ptr, n, w=10):
        self._check(self.lib.pfp_stage_text_dev(self._h, d_text_ptr, n, w))

    def scan_staged(self, p=100):
        ne = C.c_uint64()
        self._check(self.lib.pfp_scan_staged(self._h, p, C.byref(ne)))
        return ne.value

    def scan_k1_enqueue(self, p=100):
        self._check(self.lib.pfp_scan_k1_enqueue(self._h, p))


def bigbwt_files_multi(text, base, devices, w=10, p=100, flags=0, halo=0):
    """pfp_bigbwt_files_multi: one BWT on len(devices) GPUs from this process (csrc/multi.hip); returns its statistics"""
    lib = load_library()
    text = _arr(text, np.uint8)
    st, err = MultiStats(), C.create_string_buffer(1024)
    devs = (C.c_int * len(devices))(*devices)
    rc = lib.pfp_bigbwt_files_multi(len(devices), devs, text, len(text), w, p, flags, halo, str(base).encode(), C.byref(st), err, len(err))
    if rc != 0:
        raise PfpError(rc, err.value.decode(errors="replace"))
    return {k: getattr(st, k) for k, _ in MultiStats._fields_}


def multi_rccl_selftest(device=0, inject_failure=False):
    """pfp_multi_rccl_selftest2: the native multi-GPU host's RCCL transport over one device (raises PfpError with its message);
    inject_failure: also the error path - a failure inside an open group, the communicators aborted"""
    lib = load_library()
    err = C.create_string_buffer(1024)
    rc = lib.pfp_multi_rccl_selftest2(device, bool(inject_failure), err, len(err))
    if rc:
        raise PfpError(rc, err.value.decode(errors="replace"))
