/* pfpgpu.h -- C ABI of libpfpgpu.so: MI355X (gfx950) prefix-free-parsing BWT builder.
 *
 * This is the drop-in boundary for the parse -> SA -> BWT hot path of alshai/Big-BWT.
 * The reference has no FFI; its stages are three executables glued by files, and the only
 * in-process ABI on the path is gsa/gsacak.h.  Each entry point below names the reference
 * interface it replaces (file:line under the reference tree).  Plain pointers and sizes only:
 * no C++/torch types cross this boundary.
 *
 * Conventions
 *   - every function returns PFP_OK (0) or a negative PFP_E* code; nothing calls exit()
 *     (the reference die()s: utils.c:12-16); pfp_last_error(ctx) gives a message.
 *   - "host" entry points take/return caller-owned host buffers in the reference's on-disk
 *     byte formats; "_dev" entry points take device pointers (hipMalloc'ed
 *     or torch CUDA tensors' data_ptr) and leave results in device memory.
 *   - one pfp_ctx per host thread / GPU; a ctx owns one HIP stream and a device memory pool.
 *   - all compute runs in HIP kernels on the ctx's device; there is no CPU fallback: if no
 *     GPU is usable pfp_ctx_create fails with PFP_ENODEV.
 */
#ifndef PFPGPU_H
#define PFPGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFP_OK 0
#define PFP_EINVAL (-1)     /* bad argument (w<4, p<10: newscan.cpp:537-544; -S with -s/-e: bigbwt:59-61) */
#define PFP_ENODEV (-2)     /* no usable HIP device */
#define PFP_EHIP (-3)       /* HIP runtime error */
#define PFP_ECOLLISION (-4) /* phrase-hash collision survived all reseeds (newscan.cpp:282-286) */
#define PFP_ELIMIT (-5)     /* size limit: parse > 2^32-2 words (bwtparse.c:93), dict >= 2^32-2 bytes */
#define PFP_EFORMAT (-6)    /* inconsistent stage inputs (pfbwt.cpp:498-512 style checks) */
#define PFP_ENOMEM (-7)
#define PFP_ESHORT (-8)     /* text shorter than the window / empty parse (bwtparse.c:244) */

/* output selection, same meaning as bigbwt -S / -s / -e (bigbwt:41-43) */
#define PFP_FLAG_SA 1
#define PFP_FLAG_SSA 2
#define PFP_FLAG_ESA 4

typedef struct pfp_ctx pfp_ctx;

/* number of HIP devices this process can see (0 without a GPU); `bigbwt -G 0` takes all of them */
int pfp_device_count(void);
int pfp_ctx_create(pfp_ctx **ctx, int device);
void pfp_ctx_destroy(pfp_ctx *ctx);
const char *pfp_last_error(const pfp_ctx *ctx);
const char *pfp_strerror(int code);
/* library / kernel build identification ("pfpgpu <ver> gfx950 ...") */
const char *pfp_version(void);
/* HIP stream the ctx launches on (hipStream_t), for callers that time with events */
void *pfp_ctx_stream(pfp_ctx *ctx);
void pfp_free(void *host_ptr);     /* frees host buffers returned by this library */
/* PFP_POOL_DEBUG=1 in the environment of pfp_ctx_create: every device block of the context gets an exact-size
 * allocation of its own with canary bands on both sides and a poison-filled body; bands are verified when a
 * block is released.  pfp_debug_check returns PFP_EHIP (message in pfp_last_error) once a band was damaged. */
int pfp_debug_check(pfp_ctx *ctx);
/* returns the context's cached (currently unused) device blocks to the driver */
void pfp_pool_trim(pfp_ctx *ctx);
/* out = {bytes held from the driver, peak of the bytes in use, bytes in use now, blocks handed out in debug mode};
 * "in use" counts what the holders asked for (a recycled block can be larger than the request: that shows in out[0]) */
int pfp_get_mem_stats(const pfp_ctx *ctx, uint64_t out[4]);
/* out = {allocations that reached the driver (hipMalloc) since the context was made, times a failed one made the
 * pool hand its cached blocks back}: a steady-state call adds nothing to either */
int pfp_get_pool_counters(const pfp_ctx *ctx, uint64_t out[2]);

/* ------------------------------------------------------------------------------------
 * Stage 1a: rolling Karp-Rabin window scan + phrase-boundary compaction.
 * Replaces KR_window::addchar + the trigger test of process_file (newscan.cpp:168-202,
 * 363-377; pscan.hpp:44-108).  ends[k] = text position of the last byte of phrase k, for
 * every trigger position (the final phrase, which ends in the w Dollars, is not listed).
 * *n_used = bytes actually parsed: parsing stops at the first byte <= 2 (newscan.cpp:364).
 * ------------------------------------------------------------------------------------ */
int pfp_scan(pfp_ctx *ctx, const uint8_t *text, uint64_t n, int w, uint64_t p,
             uint64_t **ends, uint64_t *n_ends, uint64_t *n_used);

/* ------------------------------------------------------------------------------------
 * Stage 1: the whole parser (newscanNT.x / pscan.x main: newscan.cpp:569-650).
 * Outputs are the reference's files as byte-exact buffers (library-allocated, pfp_free):
 *   dict  (.dict)  sorted phrases, each + 0x01, final 0x00      occ (.occ) u32[d]
 *   parse (.parse) u32[P] 1-based ranks                         last (.last) u8[P]
 *   sai   (.sai)   5-byte LE ints [P], only when want_sai
 * ------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t n_used;
  uint8_t *dict;   uint64_t dict_size;
  uint32_t *occ;   uint64_t n_words;      /* d */
  uint32_t *parse; uint64_t n_phrases;    /* P */
  uint8_t *last;
  uint8_t *sai;                           /* 5*P bytes or NULL */
} pfp_parse_result;
int pfp_parse(pfp_ctx *ctx, const uint8_t *text, uint64_t n, int w, uint64_t p, int want_sai,
              pfp_parse_result *out);
void pfp_parse_result_free(pfp_parse_result *r);

/* ------------------------------------------------------------------------------------
 * Suffix sorting, drop-in for gsa/gsacak.h:78-105 (32-bit build, uint_t = uint32_t).
 *   pfp_sacak_int  == sacak_int(s,SA,n,k)   s[n-1]==0 unique smallest   (bwtparse.c:167)
 *   pfp_sacak      == sacak(s,SA,n)                                      (simplebwt.c:77)
 *   pfp_gsacak     == gsacak(s,SA,LCP,DA,n) with LCP==DA==NULL: separators (byte 1) ordered
 *                     by position, s[n-1]==0                             (pfbwt.cpp:495)
 * Return 0 on success (the reference returns the recursion depth, callers only test >=0).
 * ------------------------------------------------------------------------------------ */
int pfp_sacak_int(pfp_ctx *ctx, const uint32_t *s, uint32_t *SA, uint64_t n, uint64_t k);
int pfp_sacak(pfp_ctx *ctx, const uint8_t *s, uint32_t *SA, uint64_t n);
int pfp_gsacak(pfp_ctx *ctx, const uint8_t *s, uint32_t *SA, uint64_t n);
/* The same for the reference's -DM64 build (gsa/gsacak.h:42-60: uint_t = uint64_t, int_text stays 32 bits), which
 * bigbwt selects for parses / dictionaries / texts beyond the 32-bit limits (bigbwt:109-151, 177-194): 64-bit SA
 * entries, n up to 2^40.  Inside the library the index width follows the input size in every entry point
 * (32-bit positions below 4 GiB, 64-bit above; PFP_FORCE_IDX64=1 in the environment forces the wide build). */
/* gsacak with its optional outputs (gsa/gsacak.h:96-105; either may be NULL): LCP[i] = common prefix of the
 * suffixes SA[i-1], SA[i] with separators and the final 0 ending the count, LCP[0] = 0; DA[i] = index of the
 * string suffix SA[i] starts in (gsa/README.md:76-104).  The reference's pfbwt passes DA = NULL and uses LCP only
 * for its "same suffix as the entry before" test (pfbwt.cpp:204-209), which pfp_merge answers from rank equality. */
int pfp_gsacak_lcp_da(pfp_ctx *ctx, const uint8_t *s, uint32_t *SA, int32_t *LCP, int32_t *DA, uint64_t n);
int pfp_gsacak_lcp_da64(pfp_ctx *ctx, const uint8_t *s, uint64_t *SA, int64_t *LCP, int64_t *DA, uint64_t n);
int pfp_sacak_int64(pfp_ctx *ctx, const uint32_t *s, uint64_t *SA, uint64_t n, uint64_t k);
int pfp_sacak64(pfp_ctx *ctx, const uint8_t *s, uint64_t *SA, uint64_t n);
int pfp_gsacak64(pfp_ctx *ctx, const uint8_t *s, uint64_t *SA, uint64_t n);

/* ------------------------------------------------------------------------------------
 * Stage 2: bwtparse main (bwtparse.c:212-322): SA of the parse, BWT(P), inverted lists and
 * the permuted last / sai arrays.  Caller-allocated outputs: ilist u32[P+1],
 * bwlast u8[P+1], bwsai 5*(P+1) bytes (only when sai != NULL).
 * ------------------------------------------------------------------------------------ */
int pfp_bwtparse(pfp_ctx *ctx, const uint32_t *parse, uint64_t P, const uint8_t *last,
                 const uint8_t *sai /*5P bytes or NULL*/, const uint32_t *occ, uint64_t n_words,
                 uint32_t *ilist, uint8_t *bwlast, uint8_t *bwsai);

/* ------------------------------------------------------------------------------------
 * Stage 3: pfbwt main (pfbwt.cpp:320-418 -> bwt() :109-242, pfthreads.hpp:403-518).
 * n_plus_1 = ilist length = P+1.  Outputs library-allocated (pfp_free):
 *   bwt (.bwt) n+1 bytes; sa (.sa) 5n bytes; ssa/esa (.ssa/.esa) 10 bytes per pair.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  uint8_t *bwt; uint64_t bwt_size;
  uint8_t *sa;  uint64_t sa_bytes;
  uint8_t *ssa; uint64_t ssa_bytes;
  uint8_t *esa; uint64_t esa_bytes;
} pfp_bwt_result;
int pfp_merge(pfp_ctx *ctx, const uint8_t *dict, uint64_t dict_size, const uint32_t *occ,
              uint64_t n_words, const uint32_t *ilist, const uint8_t *bwlast,
              const uint8_t *bwsai /*5(P+1) bytes or NULL*/, uint64_t n_plus_1, int w, int flags,
              pfp_bwt_result *out);
void pfp_bwt_result_free(pfp_bwt_result *r);

/* ------------------------------------------------------------------------------------
 * The whole chain in one call, as `bigbwt -w W -p M [-S|-s|-e] file` runs it (bigbwt:69-156),
 * with every intermediate kept in HBM (no files).  Host text in, host results out.
 * ------------------------------------------------------------------------------------ */
int pfp_bigbwt(pfp_ctx *ctx, const uint8_t *text, uint64_t n, int w, uint64_t p, int flags,
               pfp_bwt_result *out);

/* File to files: like pfp_bigbwt, but the outputs are streamed from HBM into <base>.bwt and, as the flags ask,
 * <base>.sa / .ssa / .esa (created or truncated) instead of being returned: what the `bigbwt` driver calls.  `text`
 * may be an mmap of the input file: it is read once, front to back, in chunks.  out_bytes (may be NULL) = the sizes
 * written {bwt, sa, ssa, esa}.
 * An output of 64 MB or more whose file lies in a memory file system (tmpfs: /dev/shm) is not staged through pinned buffers and
 * pwrite(): the file is created at its final size, mapped, its pages allocated and registered with the runtime by a helper
 * thread beside the text input and the chain, and the result copied from HBM straight into them (.bwt and .sa, whose sizes n
 * fixes, from the start of the call; .ssa / .esa once their run count is known).  Consequences a caller can see: those files
 * exist (zero-filled) while the call runs, and are removed again if it fails; PFP_MAP_OUTPUT=0 in the environment keeps every
 * output on the pwrite path (the reference writes with fwrite / pwrite: pfbwt.cpp:145-223, pfthreads.hpp:369-376). */
int pfp_bigbwt_files(pfp_ctx *ctx, const uint8_t *text, uint64_t n, int w, uint64_t p, int flags,
                     const char *base, uint64_t out_bytes[4]);
/* The same with the text taken from bytes [file_offset, file_offset + n) of an open file descriptor instead of a host buffer:
 * a few threads pread() straight into the pinned staging buffers (an mmap'ed input costs a page fault per 4 KB: 2 GB/s for a
 * 12.6 GB file in /dev/shm, where this reads at the rate of the PCIe link).  What host/bigbwt.c calls for a plain input file
 * (the reference's parsers read theirs with fread / getc: newscan.cpp:355-377). */
int pfp_bigbwt_fd(pfp_ctx *ctx, int fd, uint64_t file_offset, uint64_t n, int w, uint64_t p, int flags, const char *out_base,
                  uint64_t out_bytes[4]);

/* Device-resident variant: d_text is a device pointer to n bytes; d_bwt must hold n+1 bytes.
 * Optional device outputs (may be NULL unless the flag is set):
 *   d_sa   u64[n+1]  SA value per BWT position (d_sa[0] = n), flags & (SA|SSA|ESA).  With PFP_FLAG_SA every entry is
 *                    written.  With only PFP_FLAG_SSA / PFP_FLAG_ESA the entries at the run boundaries of the BWT -
 *                    positions j with BWT[j] != BWT[j-1] or BWT[j] != BWT[j+1], j = 0 and j = n, i.e. every entry
 *                    the .ssa/.esa files hold (pfbwt.cpp:605-676) - are written and the rest is left untouched.
 * Run-sampled / packed outputs are derived from d_bwt/d_sa by pfp_pack5_dev / pfp_sample_runs_dev below.
 * *n_used returns the parsed length; bwt length is *n_used + 1. */
int pfp_bigbwt_dev(pfp_ctx *ctx, const void *d_text, uint64_t n, int w, uint64_t p, int flags,
                   void *d_bwt, void *d_sa, uint64_t *n_used);

/* Reference file formats from device-resident results (device pointers in and out):
 *   pfp_pack5_dev       : count u64 values -> 5-byte little-endian ints (utils.c:112-129; `.sa`, pfbwt.cpp:159-160:
 *                         pass d_sa + 1 and count = n, SA[0] = n is not written)
 *   pfp_sample_runs_dev : the `.ssa` (run_end = 0: positions j with BWT[j] != BWT[j-1], incl. j = 0; pfbwt.cpp:169-174,
 *                         184-189, 605-676) or `.esa` (run_end = 1: BWT[j] != BWT[j+1], incl. j = n; pfbwt.cpp:175-179,
 *                         225-229) pairs <j, SA[j]>, 5 + 5 bytes each, of the BWT slice [pos_base, pos_base + count):
 *                         d_bwt / d_sa point at the slice's first element; left_byte / right_byte = the BWT byte just
 *                         before / after the slice (a rank's halo from its neighbours), -1 at the ends of
 *                         the whole BWT.  *n_pairs = boundaries in the slice; d_out10 == NULL only counts; more pairs
 *                         than cap_pairs -> PFP_ELIMIT (with *n_pairs set).  Concatenating the slices' outputs in
 *                         order gives the reference's file. */
int pfp_pack5_dev(pfp_ctx *ctx, const void *d_vals_u64, uint64_t count, void *d_out5);
/* writes nbytes of device memory into `path` at file_offset (file created if missing, never truncated), streamed
 * through pinned staging buffers: how a rank of the multi-GPU chain stores its slice of .bwt/.sa/.ssa/.esa -
 * the reference's threads pwrite() their ranges the same way (pfthreads.hpp:369-376) */
int pfp_pwrite_dev(pfp_ctx *ctx, const char *path, uint64_t file_offset, const void *d_src, uint64_t nbytes);
int pfp_sample_runs_dev(pfp_ctx *ctx, const void *d_bwt, const void *d_sa, uint64_t count, uint64_t pos_base,
                        int left_byte, int right_byte, int run_end, void *d_out10, uint64_t cap_pairs,
                        uint64_t *n_pairs);

/* Device-resident chain that hands back the reference's SA-derived FILES instead of SA values: d_out[0] = .sa
 * bytes (PFP_FLAG_SA), d_out[1] = .ssa, d_out[2] = .esa - device buffers allocated by the library, released with
 * pfp_dev_free; out_bytes their sizes; entries for flags not set stay NULL / 0.  The SA values live inside the call
 * only (-S: 8 bytes per text byte, allocated after the suffix sorter has returned its scratch; -s / -e: 8 bytes per
 * run boundary of the BWT), so a >= 10 GB input with -s fits one GPU.  d_bwt as in pfp_bigbwt_dev.  The buffers are
 * blocks of the context's memory pool: pfp_dev_free hands them back for reuse by later calls on the context, so the
 * caller must have finished reading them (or have read them on the context's stream) before it frees them; they are
 * released with the context at the latest. */
int pfp_bigbwt_formats_dev(pfp_ctx *ctx, const void *d_text, uint64_t n, int w, uint64_t p, int flags, void *d_bwt,
                           void *d_out[3], uint64_t out_bytes[3], uint64_t *n_used);
void pfp_dev_free(pfp_ctx *ctx, void *d_ptr);
/* device -> host copy through the context's pinned staging buffers (for buffers the library handed out) */
int pfp_memcpy_d2h(pfp_ctx *ctx, void *host_dst, const void *d_src, uint64_t nbytes);

/* per-call statistics of the most recent pfp_bigbwt / pfp_bigbwt_dev / pfp_parse on this ctx */
typedef struct {
  uint64_t n, n_phrases, n_words, dict_size;
  uint64_t sa_rounds_dict, sa_rounds_parse;
  uint64_t hard_groups, hard_chars;
  uint64_t hard_big_groups, hard_max_chars, hard_max_members;
  uint64_t hash_reseeds;
  uint64_t extra_triggers;   /* window hashes added by the fused chain to split giant phrases */
  uint64_t index_bits;       /* 32 or 64: width of dictionary positions / suffix-array slots used (bigbwt:130-151) */
  uint64_t hard_minor_groups, hard_minor_chars; /* hard groups done by majority fill; occurrences ranked for them */
  double ms_scan, ms_phrases, ms_sa_dict, ms_sa_parse, ms_merge, ms_total; /* host wall, synced */
  double parse_density;      /* fused chain: the text was cut with probability parse_density / p (pfp_set_parse_density) */
} pfp_stats;
int pfp_get_stats(const pfp_ctx *ctx, pfp_stats *st);
/* when set (default 0) every pipeline phase is bracketed by a stream sync so ms_* are filled */
void pfp_set_profiling(pfp_ctx *ctx, int on);
/* Per-kernel device times measured with HIP events on the ctx stream.  pfp_set_kernel_trace(ctx,1)
 * clears the table and starts recording; pfp_get_kernel_trace synchronises, resolves the events
 * and returns the number of rows (rows beyond cap are counted, not written).  algo_bytes is the
 * sum over the launches of the kernel's algorithmic bytes (DESIGN.md "kernels"). */
typedef struct { char name[64]; uint64_t launches; double total_ms; uint64_t algo_bytes; } pfp_kernel_stat;
void pfp_set_kernel_trace(pfp_ctx *ctx, int on);
int pfp_get_kernel_trace(pfp_ctx *ctx, pfp_kernel_stat *out, int cap);

/* Fused chain only (pfp_bigbwt / pfp_bigbwt_dev): phrases longer than max_phrase bytes are split
 * by adding a few extra trigger windows taken from inside them (default 32768; 0 = parse exactly
 * as the reference does).  The .bwt/.sa/.ssa/.esa outputs do not depend on the parse
 * (SURVEY.md 2.2-Q11); pfp_scan / pfp_parse always use the reference's trigger set. */
/* Diagnostic (tests): the library sorts as the suffix sorter reaches them - through the wrappers of csrc/prims.hip, with their size
 * thresholds, tuned configurations and work-arounds - on caller data, in place.  kind: 0 sort_pairs_db (u64 keys, u32 vals),
 * 1 sort_pairs_db (u64, u64), 2 sort_keys_db (u64; vals unused), 3 sort_keys_raw (u64; vals unused), 4 segsort_pairs_u32 (u32 keys,
 * u32 vals), 5 segsort_pairs_u32 (u32 keys, u64 vals), 6 segsort_pairs_u64_u32 (u64 keys, u32 vals); all stable on key bits
 * [begin_bit, end_bit), the segmented ones inside each [seg_begin[k], seg_end[k]) of nseg segments (elements outside every segment
 * stay as they were).  7 inclusive_max_u32 (keys: u32, in place), 8 exclusive_sum_u32_u64 (keys: u32 in, vals: u64 out),
 * 9 select_index (keys: n flag bytes, vals: n + 1 u32 - the indices of the non-zero flags, their count in vals[n]). */
int pfp_debug_lib_sort(pfp_ctx *ctx, int kind, void *keys, void *vals, uint64_t n, int begin_bit, int end_bit,
                       const uint32_t *seg_begin, const uint32_t *seg_end, uint64_t nseg);
/* Diagnostic (tests): stage 1a exactly as the fused chain runs it on a host text - the window hash or Karp-Rabin, the choice of
 * the phrase length, the Karp-Rabin fall-back of a text the window hash does not cut, the extra triggers that split giant phrases -
 * under the context's current settings (pfp_set_window_hash, pfp_set_parse_density, pfp_set_max_phrase), with a report of what
 * it did.  With plan != NULL (a settled plan of pfp_dist_parse_plan) the text is scanned as a rank of the multi-GPU chain scans
 * its shard instead: the plan's parameters plus the n_extra given extra hashes, one pass.  ends (library-allocated, pfp_free):
 * rep->n_ends final phrase ends.  dense_ends / nominal (optional, NULL to skip; library-allocated; NULL when no choice was made):
 * the rep->dense_cuts cuts of the first, dense pass and for each whether it lies inside the nominal threshold. */
typedef struct {
  uint64_t n_used, n_ends;
  uint32_t fast, fthr;                   /* the last pass: window hash (1) or Karp-Rabin (0), the threshold it cut at */
  uint32_t fseed, fthr_nom;              /* the first pass (all passes but a Karp-Rabin fall-back): the seed, the nominal threshold, */
  uint32_t fauto, fthr_first;            /* whether its density was a candidate, the threshold it cut at */
  uint32_t n_extra, reserved;            /* extra trigger hashes of the last pass (seeded window hashes, or Karp-Rabin hashes) */
  uint32_t extra[32];
  double density;                        /* the density the first pass cut at (x nominal) */
  double parse_density;                  /* pfp_stats.parse_density as the chain would report it */
  uint64_t chose, dense, kr_fallback;    /* a density choice was made; it kept the dense cuts; the window hash made no cut: Karp-Rabin */
  uint64_t dense_cuts, n_nominal;        /* the choice: cuts of the dense pass, those inside the nominal threshold, */
  uint64_t sampled, kept;                /* sampled cuts counted, sampled cuts that found room on the sample lists, */
  uint64_t distinct, singles;            /* distinct 64-byte contexts among the kept ones, contexts seen once */
} pfp_scan_report;
int pfp_debug_scan_chain(pfp_ctx *ctx, const uint8_t *text, uint64_t n, int w, uint64_t p, const uint64_t *plan,
                         const uint32_t *extra_hashes, uint32_t n_extra, uint64_t **ends, uint64_t **dense_ends, uint8_t **nominal,
                         pfp_scan_report *rep);
void pfp_set_max_phrase(pfp_ctx *ctx, uint64_t max_phrase);
/* Fused chain only: which function of the last w bytes cuts the text.  fast != 0 (default): a multiply-add hash of the window,
 * a third of the arithmetic of the reference's `KR_window` (newscan.cpp:168-202: mod 1999999973, then mod p) with the same 1 / p
 * density; 0 (or PFP_WINDOW_HASH=kr in the environment at pfp_ctx_create): Karp-Rabin as in the reference.  The outputs do not
 * depend on the choice (quirk Q1 is reproduced either way); pfp_scan / pfp_parse / the stage executables
 * always cut exactly where the reference does.  With fast == 0 and max_phrase == 0 the fused chain parses like the reference. */
void pfp_set_window_hash(pfp_ctx *ctx, int fast);
/* Fused chain with the window hash only: cut with probability density / p instead of 1 / p.  The outputs do not depend on it; the
 * work does - for c copies at mutation rate r the dictionary grows with the phrase length (about G (1 + c r L) bytes) while the
 * parse shrinks (n / L phrases), so a collection of many near-identical copies is processed faster, and in half the memory, with
 * shorter phrases (density 2 = what -p p/2 would parse like), and a single genome is not.  density = 0 (default; PFP_PARSE_DENSITY
 * in the environment at pfp_ctx_create sets another): the chain decides between 1 and p / 48 (phrases of ~48 bytes) itself - one
 * scan at the higher density, a content-defined sample of the cuts, all cuts kept if the sampled 64-byte contexts show more
 * variants than loci (weighted by the phrase length), else the cuts beyond 1 / p dropped again (scan.hip: choose_parse_density).  density = 1 pins what -p says; the staged entry points and the stage
 * executables always parse exactly like the reference.  pfp_stats.parse_density tells what a call used; `bigbwt --density D`. */
int pfp_set_parse_density(pfp_ctx *ctx, double density);
/* Index width of dictionary positions and suffix-array slots: 0 = by size (32 bits below 4 GiB of dictionary /
 * text, 64 above: the reference's choice between its 32-bit and -DM64 executables, bigbwt:109-151), 64 = always
 * the wide build (what PFP_FORCE_IDX64=1 in the environment sets at pfp_ctx_create), 32 = the narrow build wherever its positions
 * fit.  By size means: narrow below 2^31 bytes of dictionary, wide from 2^32 - 16 on, and in between the wide build where ~96 bytes
 * of device memory per dictionary byte are free (it keeps the sorter's pivot rounds there; the narrow build has no spare bit in a
 * position for them), else the narrow one.  Outputs are identical. */
int pfp_set_index_bits(pfp_ctx *ctx, int bits);

/* ------------------------------------------------------------------------------------
 * Multi-GPU chain, one rank's share (the reference's analogue is the byte-range
 * threading of pscan.hpp:114-165 and the output-range threading of pfthreads.hpp:456-493).
 * The caller (big-bwt_amd/dist.py, torch.distributed over RCCL) shards the text, moves the
 * halos and runs the allgathers between the steps; all pointers are device pointers.
 *   pfp_dist_propose_triggers: window hashes (<= 8) that would split this shard's giant phrases
 *       (pfp_set_max_phrase); the caller allgathers them, every rank passes the union as
 *       extra_hashes so that all ranks parse with one trigger set (outputs do not depend on it)
 *   pfp_dist_local_parse : d_text = halo (the last halo_len bytes of the previous shard; 0 for the
 *       first rank) followed by this rank's shard, n bytes in all; global_offset = position of the
 *       shard's first byte in the whole text.  Owns the phrases that end inside the shard.  want_sai = the output
 *       flags of the run (PFP_FLAG_*; 0 = BWT only: no sa info is kept).
 *       out_sizes = {local dict bytes, local words, local phrases, local position of last trigger}
 *   pfp_dist_export_local: copies the local dictionary (words + 0x01), its occ (u32), last (u8)
 *       and sai (u64) into caller buffers (any may be NULL)
 *   pfp_dist_global      : d_union = the ranks' local dictionaries back to back, d_union_occ their
 *       occ; my_word_base = index of this rank's first word in the union.  Builds the global
 *       dictionary and writes this rank's parse as global 1-based ranks (u32[local phrases]).
 *       out_info = {global words, global dict bytes, doubling rounds}
 *   pfp_dist_global_sort / pfp_dist_global_finish: the same in two steps, with the suffix array of
 *       the global dictionary sharded by key range (the reference shards the same array by index
 *       range across threads, pfthreads.hpp:171-176): share `part` of `parts` sorts the suffixes
 *       whose first-round key falls in its part of the key space (splitters from a deterministic
 *       sample, identical on all ranks, no exchange) and holds one contiguous range of SA(D).
 *       d_wslot_out (u64[n_union], the first out_info[0] used): 1 + SA(D) slot of every global
 *       word's first suffix if this share holds it, else 0.  out_info = {global words, global
 *       dict bytes, sorting rounds, complete (0/1), slots held, first slot, BWT positions the held
 *       slots emit, index width used (32 / 64)}.  complete == 0: some group could not be settled without other shares'
 *       ranks - every rank must then redo the step with parts = 1 (the replicated sort).
 *       The caller allgathers d_wslot_out (and complete / emit counts) and passes all `parts`
 *       arrays, out_info[0] entries each, back to back to pfp_dist_global_finish, which ranks the
 *       words and writes this rank's parse.  parts = 1 needs no exchange (= pfp_dist_global).
 *   pfp_dist_merge       : d_sym/d_last/d_sai = the whole parse in text order (all ranks);
 *       n_total = text length; emits BWT positions [out_lo,out_hi) into d_bwt_slice (u8) and, with
 *       flags, SA values into d_sa_slice (u64).  After a sharded sort [out_lo,out_hi) must be the
 *       range the held slots emit: out_lo = sum of the emit counts of the lower shares.
 * ------------------------------------------------------------------------------------ */
int pfp_dist_propose_triggers(pfp_ctx *ctx, const void *d_text, uint64_t n, int w, uint64_t p,
                              uint32_t out_hashes[8], uint32_t *n_hashes);
int pfp_dist_local_parse(pfp_ctx *ctx, const void *d_text, uint64_t n, uint64_t halo_len, int w, uint64_t p,
                         int is_first, int is_last, uint64_t global_offset, int want_sai,
                         const uint32_t *extra_hashes, uint32_t n_extra, uint64_t out_sizes[4]);
/* Round 4: the multi-GPU chain under a PARSE PLAN - the window hash and the phrase length by repetitiveness of the fused chain
 * (pfp_set_window_hash, pfp_set_parse_density), agreed between the ranks.  plan[4]: [0] 0 = the reference's Karp-Rabin hash (what
 * the two calls above cut by), 1 = the window hash, 2 = the window hash at a pinned density (pfp_set_parse_density > 0, or more
 * than two ranks); [1] its seed; [2] the density (the bits of a double: cuts with probability density / p - the very double the
 * single-GPU chain computes its thresholds from, so both chains cut at the same 32-bit thresholds); [3] 1 while that density is
 * a candidate the ranks still have to decide on.
 *   pfp_dist_parse_plan        rank 0, from the text's first bytes (host): the plan every rank gets, and the first window's hash
 *                              under it (banned as an extra trigger: SURVEY.md 2.2-Q1).  The density is a candidate (p / 48) on one
 *                              or two ranks and nominal beyond: every rank reads the whole parse, only the dictionary is shared
 *   pfp_dist_propose_triggers2 with plan[3] set: this rank's sample of its cuts (sorted 64-bit context hashes of the cuts at or
 *                              after halo_len, at most sample_cap, in d_sample) and no proposals
 *   -- the hosts all-gather the samples --
 *   pfp_dist_decide_density    on every rank, the same gathered samples: settles plan[2] (the candidate, or 1) and clears plan[3]
 *   pfp_dist_propose_triggers2 under the settled plan: as pfp_dist_propose_triggers (the proposals are made at the density the parse
 *                              will have: a window of a periodic stretch can cut at the candidate density and not at the nominal one)
 *   pfp_dist_local_parse2      as pfp_dist_local_parse, under the settled plan (extra_hashes are hashes under the plan) */
int pfp_dist_parse_plan(pfp_ctx *ctx, const uint8_t *first_bytes, uint64_t n_bytes, int w, uint64_t p, uint32_t ranks, uint64_t plan[4],
                        uint64_t *first_hash);
int pfp_dist_propose_triggers2(pfp_ctx *ctx, const void *d_text, uint64_t n, uint64_t halo_len, int w, uint64_t p, const uint64_t plan[4],
                               uint32_t out_hashes[8], uint32_t *n_hashes, void *d_sample, uint64_t sample_cap, uint64_t *n_sample);
int pfp_dist_decide_density(pfp_ctx *ctx, const void *d_samples, uint64_t count, uint64_t p, uint64_t plan[4]);
int pfp_dist_local_parse2(pfp_ctx *ctx, const void *d_text, uint64_t n, uint64_t halo_len, int w, uint64_t p,
                          int is_first, int is_last, uint64_t global_offset, int want_sai, const uint64_t plan[4],
                          const uint32_t *extra_hashes, uint32_t n_extra, uint64_t out_sizes[4]);
int pfp_dist_export_local(pfp_ctx *ctx, void *d_dict, void *d_occ, void *d_last, void *d_sai);
int pfp_dist_global(pfp_ctx *ctx, const void *d_union, uint64_t union_bytes, const void *d_union_occ,
                    uint64_t n_union, uint64_t my_word_base, void *d_sym_out, uint64_t out_info[3]);
int pfp_dist_global_sort(pfp_ctx *ctx, const void *d_union, uint64_t union_bytes, const void *d_union_occ,
                         uint64_t n_union, uint32_t part, uint32_t parts, void *d_wslot_out, uint64_t out_info[8]);
int pfp_dist_global_finish(pfp_ctx *ctx, const void *d_wslot_all, uint32_t parts, uint64_t my_word_base,
                           void *d_sym_out);
/* Hash-partitioned deduplication (the exchange SURVEY.md 8e calls A; the reference's threaded parser shards its
 * maps by `hash % (3 N)`, pscan.cpp:137-205): every distinct word is owned by the rank its identity hash points
 * at, so the union of the local dictionaries is deduplicated in `parts` disjoint pieces and only distinct words
 * are gathered.  Between the calls the caller runs an all-to-all of (words, occ), an all-to-all of the answers
 * and an allgatherv of the owners' distinct words (dist.py):
 *   pfp_dist_partition_words      : counts[2*o], counts[2*o+1] = words / bytes (one 0x01 per word included) this
 *                                   rank sends to owner o
 *   pfp_dist_export_partition     : the local words (each + 0x01) and their occ, grouped by owner, owner 0 first
 *   pfp_dist_owner_dedup          : d_bytes/d_occ = what all ranks sent to this owner, back to back in rank order;
 *                                   d_pid_out[u] = index of received word u among this owner's distinct words;
 *                                   out = {distinct words, their bytes}
 *   pfp_dist_export_owned         : the owner's distinct words (each + 0x01) and their summed occ
 *   pfp_dist_global_sort_distinct : as pfp_dist_global_sort, on the gathered owner pieces (owner 0 first, no
 *                                   further dedup); d_gid_sent[k] = global id (owner base + pid answer) of the k-th
 *                                   word this rank exported; pfp_dist_global_finish then needs no my_word_base */
int pfp_dist_partition_words(pfp_ctx *ctx, uint32_t parts, uint64_t *counts);
int pfp_dist_export_partition(pfp_ctx *ctx, void *d_bytes, void *d_occ);
int pfp_dist_owner_dedup(pfp_ctx *ctx, const void *d_bytes, uint64_t nbytes, const void *d_occ, uint64_t n_words,
                         void *d_pid_out, uint64_t out[2]);
int pfp_dist_export_owned(pfp_ctx *ctx, void *d_bytes, void *d_occ);
int pfp_dist_global_sort_distinct(pfp_ctx *ctx, const void *d_dict, uint64_t dict_bytes, const void *d_occ, uint64_t n_words,
                                  const void *d_gid_sent, uint32_t part, uint32_t parts, void *d_wslot_out,
                                  uint64_t out_info[8]);
/* The suffix array of the (replicated) parse in shares, like the dictionary's: pfp_dist_parse_sort sorts the suffixes of the whole
 * parse d_sym (u32[P], all ranks') whose first-round key lies in share `part` of `parts` into d_sa_out (u32, room for P + 1) -
 * out_info = {entries, first slot, complete, rounds}; complete = 0: only a doubling round could go on (then, or if any rank says so,
 * nobody sets anything and pfp_dist_merge sorts the whole parse itself as bwtparse.c does).  The caller all-gathers the shares in
 * rank order (they are consecutive ranges of the array) and hands the P + 1 entries to pfp_dist_set_parse_sa before
 * pfp_dist_merge, which uses them once. */
int pfp_dist_parse_sort(pfp_ctx *ctx, const void *d_sym, uint64_t P, uint32_t part, uint32_t parts, void *d_sa_out, uint64_t out_info[4]);
int pfp_dist_set_parse_sa(pfp_ctx *ctx, const void *d_sa, uint64_t count);
int pfp_dist_merge(pfp_ctx *ctx, const void *d_sym, uint64_t P, const void *d_last, const void *d_sai, int flags,
                   uint64_t n_total, uint64_t out_lo, uint64_t out_hi, void *d_bwt_slice, void *d_sa_slice);
/* After pfp_dist_merge with PFP_FLAG_SSA / PFP_FLAG_ESA and d_sa_slice == NULL (the SA values then stay inside: 8 bytes
 * per run boundary of the slice instead of 8 per position): the slice's pieces of .ssa (run_end == 0) / .esa
 * (run_end != 0) as 10-byte pairs <global position, SA value> (pfbwt.cpp:605-676), written from the run maps the merge
 * left - no pass over the BWT bytes.  drop_edge: the slice's first (.ssa) / last (.esa) position is not a run start /
 * end after all, because the neighbouring slice's adjacent byte is the same (the caller has exchanged those bytes).
 * d_out10 == NULL: count only. */
int pfp_dist_sample_runs(pfp_ctx *ctx, int run_end, int drop_edge, void *d_out10, uint64_t cap_pairs, uint64_t *n_pairs);
void pfp_dist_release(pfp_ctx *ctx);

/* ------------------------------------------------------------------------------------
 * One BWT on n_dev GPUs of one node, from one process (csrc/multi.hip): a host thread and a context per device run
 * the chain above and meet in RCCL collectives over xGMI (grouped ncclSend / ncclRecv of the ranks' pieces; librccl is
 * loaded on the first call).  The reference's analogue is its threaded build, `bigbwt -t N`: pscan.cpp / pscan.hpp:114-165
 * (byte ranges of the input, hash-sharded dictionary) and pfthreads.hpp:171-176, 369-376, 456-493 (the suffix array sharded
 * by range, output ranges written with pwrite).  text = the whole input in host memory (rank r reads bytes
 * [n r / n_dev, n (r+1) / n_dev)); halo = bytes of a range its right neighbour also reads, must cover the longest phrase
 * (0 = 1 MiB); outputs out_base.bwt / .sa / .ssa / .esa as pfp_bigbwt_files writes them.  A failure on any rank ends all
 * ranks; its text goes to errbuf.  Bytes <= 2 in the text are an error here (PFP_EFORMAT), not the end of the input.
 * PFP_MULTI_LOOPBACK=1 (tests on a one-GPU box): the ranks share the devices given, modulo the visible ones, and exchange
 * through device copies instead of RCCL. */
typedef struct {
  uint64_t n, n_words, n_phrases, dict_size, index_bits;
  uint64_t ranks, sa_shares;      /* sa_shares = 1: a key range could not finish alone, every rank sorted the whole dictionary */
  uint64_t parse_shares;          /* ranks when the parse's suffix array was sorted in key ranges too, 1 when every rank sorted all of it */
  double ms_chain, ms_total;      /* rank 0: upload to finished device outputs; + files */
  double parse_density;           /* the plan's settled density (1 under the Karp-Rabin plan) */
} pfp_multi_stats;
int pfp_bigbwt_files_multi(int n_dev, const int *devices, const uint8_t *text, uint64_t n, int w, uint64_t p, int flags,
                           uint64_t halo, const char *out_base, pfp_multi_stats *stats, char *errbuf, uint64_t errbuf_len);

/* The RCCL transport of pfp_bigbwt_files_multi on ONE device (tests on a one-GPU box): librccl resolved with dlopen, a communicator
 * from ncclCommInitAll over `device`, every exchange shape of the chain as a self send / recv inside a group, and the one-collective
 * all-gather; returns PFP_OK when every byte came back. */
int pfp_multi_rccl_selftest(int device, char *errbuf, uint64_t errbuf_len);
/* the same, then (inject_failure != 0) an exchange that fails between ncclGroupStart and ncclGroupEnd with a send already queued:
 * the group is closed on the way out and every communicator aborted (ncclCommAbort), as a failing rank of the chain does; PFP_OK =
 * it failed as intended and came back */
int pfp_multi_rccl_selftest2(int device, int inject_failure, char *errbuf, uint64_t errbuf_len);

/* ------------------------------------------------------------------------------------
 * Inverting and checking a BWT (csrc/unbwt.hip).  The reference has no inverter; its readme asks users of large inputs to
 * "check the correctness of the BWT by some other means (for example inverting it)" (readme.md, and the Description of the
 * bigbwt script), and its only whole-output check is `bigbwt -c` (bigbwt:177-194: a whole-text suffix array).  These take
 * O(n) work and about 4 (below 2^32 rows) or 8 bytes of device memory per BWT byte, plus 0.14 per .ssa / .esa checked.
 * Conventions for a text T of n bytes: the .bwt holds n+1 bytes with exactly one 0; row j has SA[j] and BWT[j] = T[SA[j]-1]
 * (0 where SA[j] = 0), SA[0] = n.  .sa holds SA[1..n] as 5-byte little-endian ints; .ssa the pairs <j, SA[j]> of the run
 * starts (j = 0 or BWT[j] != BWT[j-1]), .esa those of the run ends (j = n or BWT[j] != BWT[j+1]), 5 + 5 bytes each.
 * Validity: n+1 bytes are a BWT iff they hold exactly one 0 and LF(j) = C[BWT[j]] + #{i < j : BWT[i] = BWT[j]} is ONE cycle
 * through all n+1 rows; anything else returns PFP_EFORMAT (pfp_last_error names the rule).  A mismatch against the text or
 * the SA files is not an error: the call returns PFP_OK with the fields below set.  n+1 > 2^40 -> PFP_ELIMIT (the .sa
 * format's limit).  PFP_FORCE_IDX64=1 / pfp_set_index_bits(ctx, 64) selects the 8-byte layout at any size.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  uint64_t n;                           /* text length the BWT encodes (n_plus_1 - 1) */
  uint64_t text_mismatch;               /* smallest text position where the inverse differs from the given text (a text of another
                                           length: at most the shorter length); UINT64_MAX = equal or not checked */
  uint64_t sa_mismatch;                 /* smallest j in 1..n whose .sa entry != SA[j], or the first index past a short / long file */
  uint64_t ssa_runs, esa_runs;          /* run starts / ends of the BWT = the pairs a correct .ssa / .esa holds (0 if not checked) */
  uint64_t ssa_mismatch, esa_mismatch;  /* smallest pair index that is wrong, missing or extra; UINT64_MAX = correct or not checked */
  double ms;                            /* host wall time of the call */
} pfp_check_result;
/* d_bwt: n_plus_1 device bytes -> d_text: n device bytes (may be NULL when n = 0) */
int pfp_unbwt_dev(pfp_ctx *ctx, const void *d_bwt, uint64_t n_plus_1, void *d_text);
/* the same with host buffers (text: n_plus_1 - 1 bytes) */
int pfp_unbwt(pfp_ctx *ctx, const uint8_t *bwt, uint64_t n_plus_1, uint8_t *text);
/* device pointers; every input but d_bwt may be NULL (not checked): d_text n bytes, d_sa5 5n bytes, d_ssa10 / d_esa10 of
 * ssa_bytes / esa_bytes.  out is filled on PFP_OK. */
int pfp_check_bwt_dev(pfp_ctx *ctx, const void *d_bwt, uint64_t n_plus_1, const void *d_text, const void *d_sa5, const void *d_ssa10,
                      uint64_t ssa_bytes, const void *d_esa10, uint64_t esa_bytes, pfp_check_result *out);
/* what `bigbwt --verify` and `unbwt --check` call: reads <base>.bwt and, as flags ask (PFP_FLAG_SA / SSA / ESA), <base>.sa /
 * .ssa / .esa through the pinned staging buffers; the text (n bytes) comes from host memory, or (text == NULL) from bytes
 * [text_offset, text_offset + n) of the open file text_fd.  A requested file that cannot be read -> PFP_EINVAL. */
int pfp_check_bwt_files(pfp_ctx *ctx, const char *base, const uint8_t *text, int text_fd, uint64_t text_offset, uint64_t n, int flags,
                        pfp_check_result *out);

/* ------------------------------------------------------------------------------------
 * Searching a BWT: pattern count and locate over a .bwt and its run samples (csrc/fmsearch.hip).  The reference has no
 * counterpart: the method is the r-index of Gagie, Navarro and Prezza, "Optimal-time text indexing in BWT-runs bounded
 * space" (SODA 2018): backward search that keeps one SA value of the range (the toehold), and phi^-1, a predecessor search
 * over the run-end samples, for the other SA values of the range.  The conventions are unbwt's (above): the text T has n bytes,
 * the .bwt n+1 bytes with exactly one 0, row j has SA[j] with SA[0] = n, .ssa / .esa hold the pairs <j, SA[j]> of the run
 * starts / ends as 5-byte little-endian ints.
 * For a pattern P of m bytes:
 *   occurrences: the positions i in [0, n-m] with T[i..i+m) = P.  The empty pattern has the n+1 occurrences 0..n (all rows);
 *     a pattern that holds byte 0, or is longer than n, has none.
 *   count: the half-open row range [sp, ep) of the suffixes that start with P; the count is ep - sp; sp = ep = 0 when it is 0.
 *     With samples, count also gives the toehold first = SA[sp] (UINT64_MAX when the count is 0).
 *   locate: SA[sp], SA[sp+1], ... in row order (the suffixes' lexicographic order), at most max_occ per pattern (0: all).
 * Patterns come as concatenated bytes plus npat+1 offsets (pattern p = pat[off[p] .. off[p+1])).  Every row, position and
 * offset crosses the ABI as uint64; inside the index rows and SA values are u32 below 2^32 rows and u64 above (or when
 * PFP_FORCE_IDX64=1 / pfp_set_index_bits(ctx, 64) forces the wide layout).
 * Checked at build: the .bwt holds exactly one 0 (else PFP_EFORMAT, unbwt's first rule); .ssa and .esa hold 10 r bytes for the
 * r runs of the .bwt and pair i names the i-th run start / end (else PFP_EFORMAT).  Not checked: the SA values of the pairs,
 * which need the inversion (`unbwt --check TEXT -s -e`, pfp_check_bwt_files); wrong values give wrong positions, never a read
 * outside the index.  Nor that LF is one cycle: bytes that are not a BWT but hold one 0 give answers for no text.
 * Device memory of the index (pfp_fm_info's device_bytes), with sigma = distinct bytes other than 0 and w = 4 bytes below
 * 2^32 rows, 8 above: at most (1 + sigma/128 + sigma/8192) bytes per row for count (BWT bytes, u16 block and u64 superblock
 * counters), with samples plus 0.140625 bytes per row (run-start bitmap and directory) and 6 w per run, plus below 8 KiB.  The
 * build peaks at the index plus at most 0.140625 bytes per row and 4 w per run, plus the scratch of the library sort and scans.
 * Locate takes 24 bytes per segment (a run start inside a range, plus one per pattern) and 32 per pattern on top of the
 * caller's buffers.
 * ------------------------------------------------------------------------------------ */
typedef struct pfp_fm pfp_fm;
typedef struct {
  uint64_t n;              /* text length (rows - 1) */
  uint64_t runs;           /* runs of the BWT (0 for an index without samples) */
  uint32_t sigma;          /* distinct bytes other than 0 */
  uint32_t row_bits;       /* 32 or 64: width of rows and SA values inside the index */
  uint64_t device_bytes;   /* device memory the index holds */
  int has_samples;         /* 1: built with .ssa / .esa (locate works) */
  int has_thresholds;      /* 1: pfp_fm_thresholds_* gave it thresholds (pfp_fm_ms_thr* work) */
  uint64_t nseq;           /* sequences of the table pfp_fm_set_seqs gave it (0: none) */
} pfp_fm_info_t;
/* an index over n_plus_1 device bytes; d_ssa10 / d_esa10 (ssa_bytes / esa_bytes) both NULL: count only.  The index copies
 * what it keeps: the caller may free its buffers afterwards.  *out is set on PFP_OK only (nothing stays allocated otherwise). */
int pfp_fm_build_dev(pfp_ctx *ctx, const void *d_bwt, uint64_t n_plus_1, const void *d_ssa10, uint64_t ssa_bytes, const void *d_esa10,
                     uint64_t esa_bytes, pfp_fm **out);
/* reads <base>.bwt and, when flags holds PFP_FLAG_SSA | PFP_FLAG_ESA, <base>.ssa and <base>.esa (a file that cannot be read:
 * PFP_EINVAL naming it; one of the two flags alone: PFP_EINVAL) */
int pfp_fm_build_files(pfp_ctx *ctx, const char *base, int flags, pfp_fm **out);
/* device pointers: d_pat_off npat+1 non-decreasing offsets into d_pat (pattern bytes are read from d_pat[d_pat_off[0]] to
 * d_pat[d_pat_off[npat]]; a pair of decreasing offsets counts as no occurrence); d_sp / d_ep / d_first npat entries each.
 * d_first may be NULL; it needs samples otherwise (PFP_EINVAL). */
int pfp_fm_count_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t *d_sp, uint64_t *d_ep,
                     uint64_t *d_first);
/* device pointers, from pfp_fm_count_dev: d_out_off (npat+1) gets the exclusive sums of min(ep - sp, max_occ) (max_occ = 0: no
 * cap), so d_out_off[npat] is the total; d_pos (room for that total) gets pattern p's positions at d_out_off[p] ..
 * d_out_off[p+1] in row order.  d_pos NULL: the offsets only.  An index without samples: PFP_EINVAL naming the files. */
int pfp_fm_locate_dev(pfp_fm *fm, uint64_t npat, const uint64_t *d_sp, const uint64_t *d_ep, const uint64_t *d_first, uint64_t max_occ,
                      uint64_t *d_out_off, uint64_t *d_pos);
/* host buffers: pat / pat_off as above (offsets that decrease: PFP_EINVAL); sp, ep (npat each) and first (NULL ok) are filled */
int pfp_fm_count(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t *sp, uint64_t *ep, uint64_t *first);
/* both phases with host buffers: sp / ep (NULL ok) get the ranges, out_off (npat+1) the offsets, *pos a malloc'ed array of
 * out_off[npat] positions (pfp_free; NULL when there are none) */
int pfp_fm_locate(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t max_occ, uint64_t *sp, uint64_t *ep,
                  uint64_t *out_off, uint64_t **pos);
int pfp_fm_info(const pfp_fm *fm, pfp_fm_info_t *out);
/* releases the index's device memory to its context (call before pfp_ctx_destroy); NULL is a no-op.  Errors of the calls that
 * take an index are reported through its context's pfp_last_error. */
void pfp_fm_free(pfp_fm *fm);

/* ------------------------------------------------------------------------------------
 * Approximate search: the occurrences of a pattern with at most k substitutions, over the same index (csrc/fmapprox.hip).  The
 * reference has no counterpart: the method is backtracking over the BWT, a depth-first walk that spends one of k mismatches
 * where it steps with a byte other than the pattern's.  Conventions as in "Searching a BWT": the text T has n bytes, rows run
 * 0..n with SA[0] = n, symbols are the bytes other than 0 that T holds.
 * For a pattern P of m bytes and a budget k in 0..PFP_FM_APPROX_MAX_K:
 *   occurrence: a position i in [0, n-m] with Hamming(T[i..i+m), P) <= k.  A pattern byte that is 0, or that T does not hold,
 *     can never match: it costs one mismatch wherever the window lies.  m > n gives no occurrence.
 *   hit: a distinct string S of m bytes that occurs in T with d = Hamming(S, P) <= k, reported as (sp, ep, first, d): [sp, ep)
 *     is the non-empty row range of the suffixes that start with S, first = SA[sp] as pfp_fm_count_dev gives it.
 *   order of hits: the hits of one pattern have disjoint ranges and are listed by increasing sp, the lexicographic order of the
 *     strings S: the answer depends on the inputs only, not on the walk, the batch or the launch budget.
 *   special cases: the empty pattern has the one hit (0, n+1, n, 0); with k = 0 the result is exactly pfp_fm_count's, one hit or
 *     none; with m <= k every string of m bytes that occurs in T is a hit.
 *   locating: the positions of a pattern are the SA values of its hits' rows, hits in hit order and rows in row order inside a
 *     hit, so the whole list is in increasing row order; each position carries its hit's d.  max_occ (0: all) caps the rows per
 *     PATTERN: it keeps the first max_occ rows in that order.
 * PFP_FM_APPROX_MAX_K is a choice, not a measurement: the record a bounded launch leaves holds k + 1 frames, and the walk's work
 * grows roughly as (m sigma)^k.  k outside 0..PFP_FM_APPROX_MAX_K: PFP_EINVAL.
 * Device memory on top of the caller's buffers: 176 bytes per pattern (the record) and 8 per pattern for the counts; filling
 * takes 25 bytes per hit for the hits in walk order (17 without toeholds), 16 for the sort's keys and values, 8 per pattern
 * for its segment bounds, plus the library sort's scratch.  2^32 - 1 or more hits in one call: PFP_ELIMIT (the segmented
 * sort's segment bounds are u32).
 * ------------------------------------------------------------------------------------ */
#define PFP_FM_APPROX_MAX_K 3
/* device pointers, patterns as in pfp_fm_count_dev.  d_hit_off (npat+1) gets the exclusive sums of the hit counts.  d_sp, d_ep
 * and d_dist all NULL: the offsets only; otherwise all three are required, with room for d_hit_off[npat] entries, and pattern
 * p's hits lie at d_hit_off[p] .. d_hit_off[p+1].  d_first may be NULL; it needs samples otherwise (PFP_EINVAL).  A hit is a
 * "pattern" for pfp_fm_locate_dev: the H = d_hit_off[npat] triples (sp, ep, first) as its npat list every hit's positions. */
int pfp_fm_approx_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, int k, uint64_t *d_hit_off, uint64_t *d_sp,
                      uint64_t *d_ep, uint64_t *d_first, uint8_t *d_dist);
/* host buffers (offsets that decrease: PFP_EINVAL): hit_off (npat+1) is filled; *sp, *ep, *dist and, where first is not NULL,
 * *first are malloc'ed arrays of hit_off[npat] entries (pfp_free; NULL when there are none).  The patterns go through in
 * consecutive groups of at most PFP_SEQ_BUDGET hits (a pattern with more goes alone; PFP_FM_SEQ_BUDGET=K lowers it). */
int pfp_fm_approx(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, uint64_t *hit_off, uint64_t **sp,
                  uint64_t **ep, uint64_t **first, uint8_t **dist);
/* host buffers: out_off (npat+1), *pos and *dist malloc'ed arrays of out_off[npat] positions and their distances, in the order
 * of "locating" above.  Needs samples.  The groups also hold at most PFP_SEQ_BUDGET positions (a pattern with more goes alone). */
int pfp_fm_approx_locate(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, uint64_t max_occ,
                         uint64_t *out_off, uint64_t **pos, uint8_t **dist);
/* {launches, LF pairs, hits filled} of the approximate searches since the last call, which it resets; the LF pairs are
 * collected only under PFP_FM_MS_STATS=1 (measurement: tools/approx_time.py) */
int pfp_fm_approx_stats(pfp_fm *fm, uint64_t out[3]);

/* ------------------------------------------------------------------------------------
 * Extending seeds: edit-distance alignment of a whole pattern to the text near a diagonal, and the seed-and-extend call that takes
 * a pattern's MEMs as its diagonals (csrc/fmextend.hip).  The reference has no counterpart: the method is the banded form of
 * Sellers' dynamic programme (Sellers, "The theory and computation of evolutionary distances: pattern recognition", 1980; the band
 * is Ukkonen's, "Algorithms for approximate string matching", 1985) under unit costs.  Conventions as in "Searching a BWT"; the
 * index is one built with text (pfp_fm_build_ms_*), an index without text: PFP_EINVAL.  The text T has n bytes.
 * For a pattern P of m bytes and a budget k in 0..PFP_FM_EXTEND_MAX_K:
 *   candidate: a pair (p, delta) of a pattern index and a signed 64-bit diagonal, the text position that pattern byte 0 would have.
 *     A MEM (i, len, pos) of pattern p gives delta = pos - i.  delta may be negative, or >= n.
 *   window, in signed arithmetic: lo = min(max(delta - k, 0), n), hi = min(max(delta + m + k, 0), n).
 *   d(s, e) = Levenshtein(P, T[s..e)) for lo <= s <= e <= hi: a substitution, an insertion and a deletion cost 1 each.  A pattern
 *     byte that is 0, or that T does not hold, equals no text byte.  d* = the minimum over all such pairs (s, e).
 *   result (d, s, e): if d* > k there is no alignment: d = 0xFF and s = e = UINT64_MAX.  Otherwise d = d*, e is the smallest e with
 *     min over s of d(s, e) = d*, and s the largest s with d(s, e) = d*: the shortest span that ends first.  The empty pattern
 *     gives (0, lo, lo).  The result is a function of (P, T, delta, k) alone - not of the batch, the launch shape or the schedule.
 *   A candidate whose pattern index is >= npat, or whose pattern's offsets decrease, gets "no alignment".  Nothing is read outside
 *     the index or the pattern buffer.
 *   alignments of a pattern (the composite call): the MEMs of P of at least min_seed bytes, by PHONI or by thresholds, exactly as
 *     pfp_fm_mems / pfp_fm_mems_thr list them, each give the candidate delta = pos - i.  The alignments of P are the distinct
 *     triples (s, e, d) with d <= k among the results, ordered by (d, s, e); with max_aln > 0 only the first max_aln per pattern
 *     are kept.  min_seed = 0: PFP_EINVAL.  A MEM carries ONE position of its string, so this is a heuristic, as in every
 *     seed-and-extend mapper: a better alignment elsewhere in T - at another occurrence of a seed, or where no seed of min_seed
 *     bytes survives the edits - can be missed.
 * PFP_FM_EXTEND_MAX_K and PFP_FM_EXTEND_MAX_M are choices, not measurements: the band holds 5k + 1 diagonals, which at k = 32 is
 * 11 cells per lane of a group of 16, and a span of at most m + 2k bytes is packed in 17 bits of a sort key.  k outside
 * 0..PFP_FM_EXTEND_MAX_K: PFP_EINVAL.  A pattern of the call longer than PFP_FM_EXTEND_MAX_M: PFP_ELIMIT.
 * Bounds: every loop of the kernel is bounded by m and k: a candidate costs at most two passes of m rows over a band of 16
 * ceil((5k + 1) / 16) cells, about 2 m (5k + 1) cell updates, 2.1e7 at the limits.  So a launch is not cut into bounded pieces and
 * no record is kept (PFP_FM_MS_STEPS bounds the matching statistics of the composite call as it bounds pfp_fm_ms*).
 * Device memory on top of the caller's buffers: pfp_fm_extend_dev takes 8 bytes.  pfp_fm_align_dev takes 12 bytes per pattern
 * byte (the matching statistics) and 16 per pattern; per seed (MEM) 24 for the triples, then - those released - 44 for the
 * diagonals, their sort and the scan; per distinct diagonal 12 for the candidate and 17 for its result, then 32 for the keys,
 * their sort and the scan, plus the library sort's scratch.  2^32 - 1 or more seeds in one call: PFP_ELIMIT (the segmented
 * sort's segment bounds are u32).
 * ------------------------------------------------------------------------------------ */
#define PFP_FM_EXTEND_MAX_K 32
#define PFP_FM_EXTEND_MAX_M 65535
/* device pointers, patterns as in pfp_fm_count_dev.  Candidate i is (d_cand_pat[i], d_cand_diag[i]); d_dist (uint8), d_start and
 * d_end (ncand entries each) get its result. */
int pfp_fm_extend_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_cand_pat,
                      const int64_t *d_cand_diag, uint64_t ncand, int k, uint8_t *d_dist, uint64_t *d_start, uint64_t *d_end);
/* the same with host buffers (offsets that decrease: PFP_EINVAL) */
int pfp_fm_extend(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat,
                  const int64_t *cand_diag, uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end);
/* device pointers.  thresholds != 0: the seeds are pfp_fm_mems_thr's (an index without thresholds: PFP_EINVAL), else pfp_fm_mems's.
 * d_aln_off (npat+1) gets the exclusive sums of the patterns' numbers of alignments.  d_start, d_end and d_dist all NULL: the offsets
 * only; otherwise all three are required (PFP_EINVAL), with room for d_aln_off[npat] entries, and pattern p's alignments lie at
 * d_aln_off[p] .. d_aln_off[p+1]. */
int pfp_fm_align_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln,
                     int thresholds, uint64_t *d_aln_off, uint64_t *d_start, uint64_t *d_end, uint8_t *d_dist);
/* host buffers (offsets that decrease: PFP_EINVAL): aln_off (npat+1) is filled; *start, *end and *dist are malloc'ed arrays of
 * aln_off[npat] entries (pfp_free; NULL when there are none).  The matching statistics are computed for the whole call; the
 * patterns then go through in consecutive groups of at most PFP_SEQ_BUDGET seeds (a pattern with more goes alone;
 * PFP_FM_SEQ_BUDGET=K lowers it). */
int pfp_fm_align(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln,
                 int thresholds, uint64_t *aln_off, uint64_t **start, uint64_t **end, uint8_t **dist);

/* ------------------------------------------------------------------------------------
 * Aligning in a window: the best edit-distance alignment of a whole pattern anywhere in a given window of the text
 * (csrc/fmwindow.hip).  pfp_fm_extend looks within k columns of one diagonal, so it cannot look through a window as wide as the
 * insert size of a read pair; this call can, and it also realigns a read inside a known region.  The reference has no
 * counterpart: the method is Sellers' dynamic programme with a free start (Sellers, 1980, as in "Extending seeds"), unbanded.
 * Conventions, the byte-0 rule, the unit costs and k in 0..PFP_FM_EXTEND_MAX_K are as in "Extending seeds"; the index is one built
 * with text.  The text T has n bytes.
 *   candidate: a triple (p, lo, hi) of a pattern index and an unsigned window T[lo..hi) of the text.
 *   d(s, e) = Levenshtein(P, T[s..e)) for lo <= s <= e <= hi; d* = the minimum over all such pairs (s, e).
 *   result (d, s, e): if d* > k there is no alignment: d = 0xFF and s = e = UINT64_MAX.  Otherwise d = d*, e is the smallest e with
 *     min over s of d(s, e) = d*, and s the largest s with d(s, e) = d*: the shortest span that ends first, the tie rule of
 *     pfp_fm_extend.  The empty pattern gives (0, lo, lo).  For a candidate (p, delta) of pfp_fm_extend, the window
 *     lo = clamp(delta - k), hi = clamp(delta + m + k) gives that call's result.
 *   "No alignment" is also the result where p >= npat, the pattern's offsets decrease, lo > hi, or hi > n.
 *   The result is a function of (P, T, lo, hi, k) alone - not of the batch, the launch shape, the tiling or the pieces of the launch.
 * k outside 0..PFP_FM_EXTEND_MAX_K or an index without text: PFP_EINVAL.  A pattern of the call longer than PFP_FM_EXTEND_MAX_M:
 * PFP_ELIMIT.  A window with lo <= hi <= n of more than PFP_FM_WINDOW_MAX_W bytes: PFP_ELIMIT.  PFP_FM_WINDOW_MAX_W is a choice,
 * not a measurement: 16 times a usual insert size, and a column index that fits 16 bits.  Nothing is read outside T[lo..hi) or
 * outside the pattern's offsets.
 * Bounds: a candidate costs about m (hi - lo) cell updates, 1.07e9 at the limits, and up to m (2k + 1) more for its start.  A call
 * goes through in consecutive pieces of at most 2^34 cell updates (PFP_FM_WINDOW_CELLS in the source: a choice, not a
 * measurement; the environment variable PFP_FM_WINDOW_CELLS=N, read per call, lowers it); a candidate with more goes alone.
 * Device memory on top of the caller's buffers: 32 bytes per candidate and 48 for the plan (cell counts, scratch sizes and their
 * sums), and during a piece m + 1 bytes for each of its candidates whose window holds 256 bytes or more (the column that a tile
 * of 256 columns hands to the next): at most 1/128 byte per cell of the piece, 134 MB at 2^34 cells.
 * ------------------------------------------------------------------------------------ */
#define PFP_FM_WINDOW_MAX_W 16384
/* device pointers, patterns as in pfp_fm_count_dev.  Candidate i is (d_cand_pat[i], d_lo[i], d_hi[i]); d_dist (uint8), d_start and
 * d_end (ncand entries each) get its result. */
int pfp_fm_window_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_cand_pat,
                      const uint64_t *d_lo, const uint64_t *d_hi, uint64_t ncand, int k, uint8_t *d_dist, uint64_t *d_start, uint64_t *d_end);
/* the same with host buffers (offsets that decrease: PFP_EINVAL) */
int pfp_fm_window(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat, const uint64_t *lo,
                  const uint64_t *hi, uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end);

/* ------------------------------------------------------------------------------------
 * Edit scripts (CIGAR): which edits align a pattern to a span of the text that pfp_fm_extend* or pfp_fm_align* found - or to any
 * other span (csrc/fmcigar.hip).  A separate call: one more banded pass over exactly P against T[s..e), which records the
 * operation of every cell, and a walk back along the records (Ukkonen's band again; the traceback is Needleman and Wunsch's).
 * The reference has no counterpart.  Conventions and the index as in "Extending seeds".
 * For a pattern P of m bytes, a span 0 <= s <= e <= n of T with L = e - s, and a budget k in 0..PFP_FM_EXTEND_MAX_K:
 *   D[i][j] = Levenshtein(P[0..i), T[s..s+j)) with unit costs; as in "Extending seeds", a pattern byte 0 equals no text byte.
 *   operations, with the BAM codes: I = 1, D = 2, '=' = 7, X = 8.  '=' is a pattern byte that equals its text byte, X a
 *     substitution, I a pattern byte with no text byte, D a text byte with no pattern byte.
 *   the script of (P, s, e) is read backwards from (i, j) = (m, L) with c = D[i][j], until (0, 0):
 *     1. i > 0, j > 0 and P[i-1] = T[s+j-1] (and not byte 0): '=', go to (i-1, j-1);
 *     2. else i > 0, j > 0 and D[i-1][j-1] = c - 1: X, go to (i-1, j-1);
 *     3. else i > 0 and D[i-1][j] = c - 1: I, go to (i-1, j);
 *     4. else: D, go to (i, j-1).
 *     Listed from the pattern's first byte this is the optimal script whose reversed operation string is the smallest under
 *     '=' < X < I < D (tests/test_cigar_reference.py checks that against a brute force over all scripts).
 *   The script is returned run-length encoded, one uint32 per run: length << 4 | op.  A script of cost d has at most 2d + 1 runs,
 *     and the bound is attained.
 *   result: dist = D[m][L] and the runs - a function of (P, T, s, e, k) alone, not of the batch, the chunks or the schedule.
 *   no script: dist = 0xFF and no runs, where the pattern index is >= npat, the pattern's offsets decrease, s > e, e > n,
 *     |L - m| > k, or D[m][L] > k.  The empty pattern with s = e gives dist = 0 and no runs.
 *   For a result (d, s, e) of pfp_fm_extend* or pfp_fm_align* at the same k: dist = d, and the script neither begins nor ends
 *     with D, because s is the largest start and e the smallest end.
 * k outside 0..PFP_FM_EXTEND_MAX_K or an index without text: PFP_EINVAL.  A pattern of the call longer than PFP_FM_EXTEND_MAX_M:
 * PFP_ELIMIT.  Nothing is read outside T[s..e) or the pattern's offsets.
 * Bounds: every cell of an optimal path has |j - i| <= D[i][j] <= k, so the band is the 2k + 1 diagonals -k..k: an alignment
 * costs m rows over a band of 16 ceil((2k + 1) / 16) cells and a walk of at most m + L steps by one lane.
 * Device memory on top of the caller's buffers: 4 (2k + 1) bytes per alignment for its runs and 24 for the counts and the plan;
 * the records of the pass take 4 ceil((2k + 1) / 16) bytes per pattern byte (5 above k = 23; whole blocks of 16 rows: 1.3 MB at
 * the limits) and live only during a launch: alignments go through in consecutive chunks whose records fit 1 GiB - a choice,
 * not a measurement; PFP_FM_CIGAR_SCRATCH=BYTES, read per call, lowers it - and one that needs more goes alone.  So the peak is
 * min(1 GiB, all records) + 4 (2k + 1) naln + 24 naln, or one alignment's 1.3 MB where that is more.
 * ------------------------------------------------------------------------------------ */
/* device pointers; alignment i is (d_aln_pat[i], d_start[i], d_end[i]).  d_dist (naln, uint8) and d_cig_off (naln + 1, exclusive
 * sums of the run counts) are filled; d_cig NULL: those only, else room for d_cig_off[naln] uint32 */
int pfp_fm_cigar_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_aln_pat,
                     const uint64_t *d_start, const uint64_t *d_end, uint64_t naln, int k, uint8_t *d_dist, uint64_t *d_cig_off,
                     uint32_t *d_cig);
/* host buffers (offsets that decrease: PFP_EINVAL); *cig is a malloc'ed array of cig_off[naln] entries (pfp_free; NULL when none) */
int pfp_fm_cigar(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *aln_pat,
                 const uint64_t *start, const uint64_t *end, uint64_t naln, int k, uint8_t *dist, uint64_t *cig_off, uint32_t **cig);

/* ------------------------------------------------------------------------------------
 * Mapping reads: one answer per read over a collection - where it maps, on which strand, how confidently, with its edit script
 * and its MD string (csrc/fmmap.hip).  The layer over "Extending seeds", "Edit scripts" and "Sequences of a collection" that a
 * read mapper needs; the reference has no counterpart.  Conventions as in those sections.  The index carries the text
 * (pfp_fm_build_ms_*) and a sequence table (pfp_fm_set_seqs): either one missing is PFP_EINVAL.  starts[0..nseq], seq(x) and
 * off(x) are as in "Sequences of a collection".  Arguments: k in 0..PFP_FM_EXTEND_MAX_K, min_seed >= 1, thresholds as in
 * pfp_fm_align, and max_sec, the cap on the secondary hits returned per read (0: none).
 * For a read P:
 *   strands: strand 0 is P, strand 1 is rc(P): P reversed with A<->T, C<->G, a<->t, c<->g swapped and every other byte as it is
 *     (what `bwtsearch --rc` searches).  The candidates of P are the alignments (s, e, d) that pfp_fm_align lists for P (strand
 *     0) and for rc(P) (strand 1) with the same min_seed, k and thresholds and max_aln = 0.
 *   inside: a candidate with s < e and e <= starts[seq(s) + 1]: its whole span lies in one record.  All others are discarded -
 *     the empty spans that appear when m <= k included.
 *   key: (d, strand, s, e), compared in that order.
 *   shadowed: an inside candidate a for which some inside candidate b of the same read - on either strand, shadowed itself or
 *     not - has key(b) < key(a) and max(s_a, s_b) < min(e_a, e_b): b is better and their spans intersect.  This folds the
 *     neighbouring triples of one locus, and the second copy of a read that equals its own reverse complement, into one hit.  It
 *     is NOT the greedy, transitive rule (a shadowed b would no longer shadow): this one is decided per candidate from its
 *     neighbours alone, whatever the order they are looked at.
 *   hits: the inside candidates that are not shadowed, in key order.  nhits is their number, the first is the primary.  At most
 *     1 + max_sec of them are returned; nhits stays the full number.
 *   MAPQ: a choice, as every mapper's is, not a calibrated probability.  With d1 the primary's distance: 0 if another hit has
 *     distance d1; 60 if the primary is the only hit; otherwise min(60, 10 (d2 - d1)) with d2 the smallest distance above d1
 *     among the hits.  A read without hits (unmapped): 0.  It says how far the next best place found is - and seed-and-extend
 *     finds only places a seed leads to.
 *   per returned hit: strand (uint8); seq (uint32) and off (uint64, 0-based in the record) of s; start = s (uint64, in the
 *     text); dist = d (uint8); the edit script of the strand's pattern against T[s..e) exactly as pfp_fm_cigar returns it
 *     (length << 4 | op); and the MD string.
 *   MD: walk the script from the pattern's first byte with a text cursor j = s and a counter run = 0.  A '=' run of length L:
 *     run += L, j += L.  An X run: for each of its bytes emit run in decimal (a 0 included), emit T[j], run = 0, j += 1.  An I
 *     run: nothing.  A D run of length L: emit run, '^', T[j..j+L), run = 0, j += L.  At the end emit run.  Text bytes are emitted
 *     as they are.  (So T[s..e) can be rebuilt from the strand's pattern, the script and the MD string alone.)
 *   An empty read has no hits.  The result is a function of (P, index, table, arguments) alone - not of the batch, its order,
 *   the groups of the host call, the chunks of the edit scripts or the launch shape.
 * Errors follow pfp_fm_align and pfp_fm_cigar: k out of range or min_seed = 0: PFP_EINVAL; thresholds asked of an index without
 * them: PFP_EINVAL; a read longer than PFP_FM_EXTEND_MAX_M: PFP_ELIMIT; 2^32 - 1 or more candidates in one call: PFP_ELIMIT.
 * Bounds: on top of pfp_fm_align and pfp_fm_cigar, a candidate costs one predecessor search in the table's directory, two places
 * in the library's segmented sort (by s, then by key) and one scan of its neighbours: a span holds at most m + k bytes, so the
 * scan looks left while s_b > s_a - (m + k) and right while s_b < e_a, and visits only the candidates of its read that start
 * within m + 2k bytes of it.  A returned hit costs one walk over its at most 2k + 1 runs and 2k text bytes, twice.
 * Device memory on top of the caller's buffers and of what pfp_fm_align_dev (on 2 npat patterns) and pfp_fm_cigar_dev (on the
 * returned hits) take: 2 bytes per read byte and 32 per read for the two strands and their offsets; 17 per candidate for the
 * triples and 32 for the keys, their sorts and the reads' numbers, plus the library sort's scratch; 16 per read for the segments
 * and counts; per returned hit 21 for the plan of the scripts and the MD lengths, plus the scripts and the MD strings themselves.
 * ------------------------------------------------------------------------------------ */
/* device pointers, reads as patterns in pfp_fm_count_dev.  d_hit_off (npat + 1) gets the exclusive sums of the numbers of hits
 * returned, d_mapq (uint8) and d_nhits (uint64) npat entries each.  The nine outputs behind them all NULL: those three only;
 * otherwise all nine are required (PFP_EINVAL).  d_strand, d_seq, d_off, d_start and d_dist need room for d_hit_off[npat] entries -
 * which the offsets-only call reports, and npat (1 + max_sec) bounds - and d_cig_off, d_md_off for one more: read p's hits lie at
 * d_hit_off[p] .. d_hit_off[p+1], hit h's runs at (*d_cig)[d_cig_off[h] .. d_cig_off[h+1]), its MD string at (*d_md)[d_md_off[h] ..
 * d_md_off[h+1]) (no terminator).  The runs and the MD bytes are sized inside the call: *d_cig and *d_md are device buffers the
 * LIBRARY allocates, blocks of the context's pool as pfp_bigbwt_formats_dev hands out; the caller releases each with pfp_dev_free
 * (NULL where there is no hit). */
int pfp_fm_map_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_sec,
                   int thresholds, uint64_t *d_hit_off, uint8_t *d_mapq, uint64_t *d_nhits, uint8_t *d_strand, uint32_t *d_seq, uint64_t *d_off,
                   uint64_t *d_start, uint8_t *d_dist, uint64_t *d_cig_off, uint32_t **d_cig, uint64_t *d_md_off, uint8_t **d_md);
/* host buffers (offsets that decrease: PFP_EINVAL): hit_off (npat + 1), mapq and nhits (npat each) are filled; *strand, *seq, *off,
 * *start and *dist are malloc'ed arrays of hit_off[npat] entries, *cig_off and *md_off of hit_off[npat] + 1, *cig of the runs and
 * *md of the MD bytes (pfp_free each; NULL for an array without entries).  The matching statistics of both strands are computed
 * for the whole call; the reads then go through in consecutive groups of at most PFP_SEQ_BUDGET seeds, both strands counted (a read
 * with more goes alone; PFP_FM_SEQ_BUDGET=K lowers it). */
int pfp_fm_map(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_sec, int thresholds,
               uint64_t *hit_off, uint8_t *mapq, uint64_t *nhits, uint8_t **strand, uint32_t **seq, uint64_t **off, uint64_t **start,
               uint8_t **dist, uint64_t **cig_off, uint32_t **cig, uint64_t **md_off, uint8_t **md);

/* ------------------------------------------------------------------------------------
 * Mapping read pairs: reads 2q and 2q + 1 of a call are mates 1 and 2 of pair q (csrc/fmpair.hip).  The layer over "Mapping
 * reads" and "Aligning in a window" that paired short reads need: the mates' hits are combined into proper pairs, a mate
 * whose seeds did not survive its edits is looked for where its partner says it must be, and the mapping quality takes the
 * mate into account.  The reference has no counterpart.  The orientation is forward/reverse (FR: the mates face each other, as
 * Illumina paired-end libraries give them) ONLY; other orientations are out of scope.  Arguments: those of pfp_fm_map without
 * max_sec, plus the insert bounds min_ins <= max_ins <= PFP_FM_WINDOW_MAX_W and anchors = C in 1..PFP_FM_PAIR_MAX_ANCHORS (64: a
 * choice); a violation of those bounds or an odd npat: PFP_EINVAL.  The other errors are pfp_fm_map's.
 *   anchors(r): the first min(nhits, C) hits of read r, exactly as "Mapping reads" defines and orders hits.  Each is (d, strand,
 *     s, e), inside record seq(s) = [b0, b1).
 *   proper(a, b), a of mate 1 and b of mate 2: same record, different strands, and with f the strand-0 one and r the strand-1
 *     one: s_f <= s_r, e_f <= e_r and min_ins <= e_r - s_f <= max_ins.
 *   rescue(a), for an anchor a of read r, only when no anchor of the mate is proper with a: the mate's strand 1 - strand(a)
 *     pattern is aligned in a window as "Aligning in a window" defines, with the same k.  strand(a) = 0: lo = s_a, hi =
 *     min(s_a + max_ins, b1).  strand(a) = 1: hi = e_a, lo = max(e_a - min(e_a, max_ins), b0).  A result with s < e is a rescued
 *     alignment (d, 1 - strand(a), s, e); it is inside by construction.
 *   pairs of q, as distinct (a, b) values: the proper (a, b) over anchors(2q) x anchors(2q + 1); the proper (a, rescue(a)); the
 *     proper (rescue(b), b).  A rescued alignment pairs only with the anchor that produced it.
 *   pair key: (d_a + d_b, key(a), key(b)) with key as in "Mapping reads"; the primary pair is the smallest.
 *   same locus: a pair (a', b') with the primary's strands where a' intersects a and b' intersects b is at the primary's locus.
 *     npairs = 1 + the number of pairs not at the primary's locus; D2 = the smallest sum d_a + d_b among those, D1 the primary's.
 *   pair MAPQ, a choice like the single-end rule: 60 if npairs = 1; 0 if D2 = D1; otherwise min(60, 10 (D2 - D1)).
 *   per pair: proper (uint8: the pair has pairs) and npairs (uint64; 0 when not proper).
 *   per read (2 npair entries, no offsets array): mapped, rescued (uint8), mapq (uint8), nhits (uint64, the single-end number),
 *     strand, seq, off, start, dist as in "Mapping reads", tlen (int64), the edit script as pfp_fm_cigar returns it and the MD
 *     string.  In a proper pair the read's alignment is its member of the primary pair, rescued says that it is a rescued
 *     alignment, and mapq is the pair MAPQ.  Otherwise it is the read's single-end primary with its single-end MAPQ.  A read
 *     without a hit that is in no proper pair: mapped = 0, seq = 0xFFFFFFFF, off = start = UINT64_MAX, dist = 0xFF, no runs, an
 *     empty MD.
 *   tlen: when both mates are mapped in one record, max(e) - min(s): positive for the mate with the smaller s, mate 1 on a tie,
 *     and negated for the other.  Otherwise 0.
 *   The result is a function of (the pair, index, table, arguments) alone - not of the batch, its order, the groups of the host
 *   call or the pieces of any launch.
 * Bounds: per pair at most 2C rescues, each a window of at most max_ins bytes, and two walks over at most C^2 + 2C pairs.
 * Device memory on top of pfp_fm_map_dev's (with max_sec = C - 1, without its per-hit outputs): 16 C bytes per read for the
 * flags and their sums, 37 per rescue plus what pfp_fm_window_dev takes, 12 per read for the reported alignments, and the scripts.
 * ------------------------------------------------------------------------------------ */
#define PFP_FM_PAIR_MAX_ANCHORS 64
/* device pointers, reads as patterns in pfp_fm_count_dev.  d_proper (uint8) and d_npairs (uint64): npat / 2 entries; d_mapped,
 * d_rescued, d_mapq, d_strand, d_dist (uint8), d_nhits, d_off, d_start (uint64), d_seq (uint32) and d_tlen (int64): npat entries;
 * d_cig_off and d_md_off: npat + 1.  Read r's runs lie at (*d_cig)[d_cig_off[r] .. d_cig_off[r+1]), its MD string at
 * (*d_md)[d_md_off[r] .. d_md_off[r+1]).  *d_cig and *d_md are device buffers the LIBRARY allocates, as in pfp_fm_map_dev; the
 * caller releases each with pfp_dev_free (NULL where there is nothing). */
int pfp_fm_map_pairs_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, int k, int thresholds,
                         uint64_t min_ins, uint64_t max_ins, uint64_t anchors, uint8_t *d_proper, uint64_t *d_npairs, uint8_t *d_mapped,
                         uint8_t *d_rescued, uint8_t *d_mapq, uint64_t *d_nhits, uint8_t *d_strand, uint32_t *d_seq, uint64_t *d_off,
                         uint64_t *d_start, uint8_t *d_dist, int64_t *d_tlen, uint64_t *d_cig_off, uint32_t **d_cig, uint64_t *d_md_off,
                         uint8_t **d_md);
/* host buffers of the same sizes (offsets that decrease: PFP_EINVAL); *cig and *md are malloc'ed (pfp_free; NULL when empty).  The
 * matching statistics of both strands are computed for the whole call; WHOLE pairs then go through in consecutive groups of at
 * most PFP_SEQ_BUDGET seeds, both strands of both mates counted (a pair with more goes alone; PFP_FM_SEQ_BUDGET=K lowers it). */
int pfp_fm_map_pairs(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, int thresholds,
                     uint64_t min_ins, uint64_t max_ins, uint64_t anchors, uint8_t *proper, uint64_t *npairs, uint8_t *mapped, uint8_t *rescued,
                     uint8_t *mapq, uint64_t *nhits, uint8_t *strand, uint32_t *seq, uint64_t *off, uint64_t *start, uint8_t *dist, int64_t *tlen,
                     uint64_t *cig_off, uint32_t **cig, uint64_t *md_off, uint8_t **md);

/* ------------------------------------------------------------------------------------
 * Chaining anchors: where a long read lies (csrc/fmchain.hip).  "Extending seeds" aligns a whole read within k <= 32 edits of one
 * seed's diagonal; a read of 10 kb carries hundreds of edits, and every one of its seeds finds the right place all the same.
 * The first step of every long-read mapper is to chain the seeds and report the chain; base-level alignment of a chain (a band in
 * the hundreds) is "Aligning chains" below, which takes a chain's anchors.  The reference has no
 * counterpart; the method is seed chaining as in Li, "Minimap2: pairwise alignment for nucleotide sequences" (Bioinformatics
 * 2018), section 2.1, over MEM anchors instead of minimizers, in integer arithmetic.  Conventions as in "Searching a BWT" and
 * "Matching statistics".  The index is one built with text and samples (pfp_fm_build_ms_*); otherwise PFP_EINVAL, as for
 * pfp_fm_mems*.  Three layers, each usable on its own, each a function of its inputs alone - not of the batch, the launch shape,
 * the budget or the schedule.
 *
 * 1. Anchors: every occurrence of every MEM.  Arguments: min_seed >= 1, 1 <= max_occ <= 65536, thresholds.  For a pattern P:
 *   MEMs: its MEMs (i, len) of at least min_seed bytes are exactly those pfp_fm_mems lists (thresholds != 0: pfp_fm_mems_thr; the
 *     lengths are the same either way, so the anchors do not depend on thresholds).  A MEM carries ONE position of its string;
 *     in a collection of near-identical copies the positions of neighbouring MEMs lie in different copies, so a chain needs all.
 *   row range: [sp, ep) of P[i .. i+len) as pfp_fm_count defines it.  ep - sp > max_occ: the MEM is skipped (a repeat filter); the
 *     number of skipped MEMs per pattern is an output.
 *   anchors: otherwise every t = SA[r], sp <= r < ep, gives an anchor (i, len, t).
 *   record borders: with a sequence table set (pfp_fm_set_seqs), an anchor whose bytes [t, t+len) do not lie inside one record is
 *     dropped (it does count towards ep - sp).
 *   order: a pattern's anchors are listed by increasing (t + len, i + len).  The order is strict: two MEMs of a pattern never end
 *     at the same pattern byte, and the occurrences of one MEM differ in t.
 *   2^32 - 1 or more occurrences to look at in one device call: PFP_ELIMIT.
 *
 * 2. Chains.  Inputs: anc_off and anc as layer 1 gives them, or any anchors of the caller's.  A pattern's anchors that are not in
 * strictly increasing (t + len, i + len) order, an anchor with len = 0 or with i + len >= 2^32, offsets that decrease: PFP_EINVAL.
 * Arguments: max_gap G and band B, both in 1 .. 2^31 - 1; min_score S >= 1; max_chains (0: all).  H = PFP_FM_CHAIN_PRED = 64
 * predecessors are looked at: a choice (one wavefront), not a measurement.  For the anchors a_0 .. a_{A-1} of a pattern, in the
 * given order, write qe_x = i_x + len_x, te_x = t_x + len_x, rec_x = the record that holds t_x (no table: the whole text is
 * record 0).
 *   predecessors: j is a predecessor of x iff x - H <= j < x, rec_j = rec_x, dq = qe_x - qe_j >= 1, dt = te_x - te_j >= 1,
 *     dq <= G, dt <= G and g = |dt - dq| <= B.
 *   gain(j, x) = min(dq, dt, len_x) - cost(g), cost(g) = (g + 3) >> 2: signed, it can be negative.  The first term is the number
 *     of new bytes the anchor adds; a quarter per byte of gap is a choice.
 *   score: f_x = max(len_x, max over predecessors j of f_j + gain(j, x)).
 *   parent_x: the predecessor that attains that maximum, provided f_j + gain(j, x) > len_x strictly; among equal values the
 *     largest j.  Otherwise x has no parent.  (1 <= f_x <= qe_x < 2^32.)
 *   peel: visit the pattern's anchors by (f descending, index ascending).  For each unvisited x walk y = x, parent_x, ... while y
 *     exists and is unvisited, marking each visited.  The anchors walked are a chain with score = f_x - f_y, y the visited anchor
 *     the walk stopped at, or f_x if the walk ran out of parents.  The chain is kept iff score >= S; its anchors stay visited
 *     either way.
 *   fields of a chain: score; n, its number of anchors; qs = the least i of its anchors and qe = qe_x; ts = the least t of its
 *     anchors and te = te_x; match: along the chain in increasing order, len of the first anchor plus min(dq, dt, len) of each
 *     later one against the one before it - the gain without its cost.
 *   order of output: a pattern's chains by (score descending, te, qe): strict, because end anchors differ.  Only the first
 *     max_chains are kept.
 *   Example: anchors (0,30,1000) (31,25,1031) (60,40,1062) (101,30,1103) (10,22,5000) (40,35,5030), G = 5000, B = 500, S = 20: f =
 *     30, 55, 94, 124, 22, 57; parents -, 0, 1, 2, -, 4 (anchor 2: dq = 44, dt = 46, g = 2, 55 + 40 - 1 = 94); chains (score 124,
 *     n 4, q 0..131, t 1000..1133, match 125) and (57, 2, 10..75, 5000..5065, 57).
 *
 * 3. Mapping long reads.  Strand 0 of a read is the read, strand 1 its reverse complement: exactly the bytes pfp_fm_map searches.
 * Both go through layer 1 (min_seed, max_occ, thresholds) and layer 2 (G, B, S, max_chains = 0).  The read's chains are those of
 * both strands by (score descending, strand, te, qe); nchains is their number, the first is the primary, and up to max_sec
 * further ones are returned behind it.
 *   MAPQ: a choice, as the other MAPQs here are: 0 for a read without a chain, 60 for a read with one, otherwise
 *     min(60, 60 (s1 - s2) / s1) in integer division over the scores of the first two.
 *   per returned chain: strand (uint8); seq (uint32, the record of ts; 0 without a table) and off (ts minus the record's start);
 *     ts, te; qs, qe in coordinates of the read AS GIVEN (strand 1: m - qe and m - qs of the strand's pattern); score, n, match.
 *
 * Bounds: the programme is sequential along a pattern's anchors and parallel over the H predecessors: one wave per pattern, 64
 * evaluations and one wave-wide maximum per anchor.  Both the programme and the peel are bounded, resumable launches: a launch
 * advances a pattern by at most PFP_FM_CHAIN_STEPS anchors (the peel: visits and steps of its walks); the default 65536 is a
 * choice, the environment variable of the same name lowers it, is read per call and is never below 1.  The programme resumes by
 * reloading f and the fields of the previous H anchors, the peel from its place in the sorted order and its current walk.  A
 * pattern has up to m * max_occ anchors; no launch is bounded by that.  The peel is O(A) per pattern, one lane each.
 * Device memory on top of the caller's buffers.  Anchors: what pfp_fm_ms_dev's outputs take (12 bytes per pattern byte) and 32 per
 * pattern; 80 bytes per MEM (its triple, its span, its row range, toehold, clipped end and offset); per occurrence 8 for its
 * position and 32 for its end, keys and order, plus what pfp_fm_locate_dev and the library's segmented sort take; 24 per anchor
 * for the triples, which the call sizes itself.  Chains: 58 bytes per anchor (f, parent, visited flag, the sort's keys and values,
 * the fields of the chain it may end, the order of output) plus the sort's scratch, 56 per pattern (segments, counts, the
 * programme's and the peel's records); 36 bytes per chain.  Long reads: 2 bytes per read byte and 32 per read for the strands,
 * the anchors and chains of 2 npat patterns as above, and 60 per chain of either strand for its fields, key and order.
 * ------------------------------------------------------------------------------------ */
#define PFP_FM_CHAIN_PRED 64
/* device pointers, patterns as in pfp_fm_count_dev.  d_anc_off (npat + 1) gets the exclusive sums of the numbers of anchors;
 * d_anc, room for 3 * d_anc_off[npat] uint64 - which a call with d_anc == NULL reports - gets {i, len, t} per anchor (NULL: offsets
 * only); d_skipped (uint32 per pattern, may be NULL) the MEMs the repeat filter skipped. */
int pfp_fm_anchors_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                       int thresholds, uint64_t *d_anc_off, uint64_t *d_anc, uint32_t *d_skipped);
/* host buffers (offsets that decrease: PFP_EINVAL): anc_off (npat + 1) and skipped (npat, may be NULL) are filled; *anc is a
 * malloc'ed array of 3 * anc_off[npat] entries (pfp_free; NULL when none).  The matching statistics are computed for the whole
 * call; the patterns then go through in consecutive groups of at most PFP_SEQ_BUDGET MEMs, as in pfp_fm_align (a pattern with
 * more goes alone; PFP_FM_SEQ_BUDGET=K lowers it). */
int pfp_fm_anchors(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ, int thresholds,
                   uint64_t *anc_off, uint64_t **anc, uint32_t *skipped);
/* device pointers: pattern p's anchors are the triples d_anc[3 * d_anc_off[p] .. 3 * d_anc_off[p+1]).  d_chain_off (npat + 1) gets
 * the exclusive sums of the numbers of chains.  The seven arrays behind it all NULL: offsets only; otherwise all are required
 * (PFP_EINVAL), with room for d_chain_off[npat] entries each: score, n, qs, qe and match as uint32, ts and te as uint64. */
int pfp_fm_chain_dev(pfp_fm *fm, const uint64_t *d_anc_off, const uint64_t *d_anc, uint64_t npat, uint64_t max_gap, uint64_t band,
                     uint64_t min_score, uint64_t max_chains, uint64_t *d_chain_off, uint32_t *d_score, uint32_t *d_n, uint32_t *d_qs,
                     uint32_t *d_qe, uint64_t *d_ts, uint64_t *d_te, uint32_t *d_match);
/* host buffers: chain_off (npat + 1) is filled; *score, *n, *qs, *qe, *ts, *te and *match are malloc'ed arrays of chain_off[npat]
 * entries (pfp_free each; NULL when there is no chain). */
int pfp_fm_chain(pfp_fm *fm, const uint64_t *anc_off, const uint64_t *anc, uint64_t npat, uint64_t max_gap, uint64_t band, uint64_t min_score,
                 uint64_t max_chains, uint64_t *chain_off, uint32_t **score, uint32_t **n, uint32_t **qs, uint32_t **qe, uint64_t **ts,
                 uint64_t **te, uint32_t **match);
/* device pointers, reads as patterns in pfp_fm_count_dev.  d_hit_off (npat + 1) gets the exclusive sums of the numbers of chains
 * returned, d_mapq (uint8) and d_nchains (uint64) npat entries each.  The ten outputs behind them all NULL: those three only;
 * otherwise all ten are required (PFP_EINVAL), with room for d_hit_off[npat] entries - which the first kind of call reports, and
 * npat (1 + max_sec) bounds. */
int pfp_fm_map_long_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                        uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_sec, int thresholds, uint64_t *d_hit_off,
                        uint8_t *d_mapq, uint64_t *d_nchains, uint8_t *d_strand, uint32_t *d_seq, uint64_t *d_off, uint64_t *d_ts,
                        uint64_t *d_te, uint32_t *d_qs, uint32_t *d_qe, uint32_t *d_score, uint32_t *d_n, uint32_t *d_match);
/* host buffers (offsets that decrease: PFP_EINVAL): hit_off (npat + 1), mapq and nchains (npat each) are filled; the ten arrays
 * behind them are malloc'ed, hit_off[npat] entries each (pfp_free each; NULL when there is none).  The matching statistics of
 * both strands are computed for the whole call; the reads then go through in consecutive groups of at most PFP_SEQ_BUDGET MEMs,
 * both strands counted (a read with more goes alone; PFP_FM_SEQ_BUDGET=K lowers it). */
int pfp_fm_map_long(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                    uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_sec, int thresholds, uint64_t *hit_off, uint8_t *mapq,
                    uint64_t *nchains, uint8_t **strand, uint32_t **seq, uint64_t **off, uint64_t **ts, uint64_t **te, uint32_t **qs,
                    uint32_t **qe, uint32_t **score, uint32_t **n, uint32_t **match);

/* ------------------------------------------------------------------------------------
 * Aligning chains: how a long read aligns where its chain lies, base by base (csrc/fmfill.hip).  "Chaining anchors" says where a
 * read lies; the anchors of a chain are exact matches already, so what is left is the stretch between two consecutive anchors: a
 * global edit-distance alignment of up to G bytes, up to B off the diagonal - more edits than the k <= 32 of "Edit scripts", in a
 * band that is neither symmetric nor narrow.  The reference has no counterpart; the band is Ukkonen's, the operations, the tie
 * rules and the run format are those of "Edit scripts".  Conventions and the index as in "Chaining anchors".  Three layers, each
 * usable on its own, each a function of its inputs alone - not of the batch, the chunks, the scratch, the slack schedule or the
 * launch bounds.  Everything below is a choice unless it says "derived".
 *
 * 1. Filling one gap.  A segment is (p, q0, q1, t0, t1); the argument max_fill F is in 0 .. PFP_FM_FILL_MAX_F = 4096 (a choice:
 * cell values stay within 16 bits and a band within one wave's registers).  It aligns P_p[q0 .. q1) against T[t0 .. t1)
 * globally; a = q1 - q0, b = t1 - t0.
 *   no script: dist = 0xFFFFFFFF and no runs where p >= npat, q0 > q1, q1 > m_p, t0 > t1, t1 > n, a or b above PFP_FM_FILL_MAX_LEN
 *     = 65535, |a - b| > F (derived: the distance is at least |a - b|), or the Levenshtein distance D of the two strings (unit
 *     costs; a pattern byte 0 equals nothing, as everywhere else) is above F.
 *   otherwise dist = D (uint32) and the script is the one rules 1-4 of "Edit scripts" choose on the full, unbanded matrix of the
 *     two strings, walking back from (a, b): runs of length << 4 | op with the BAM codes 7, 8, 1, 2, listed from the pattern's
 *     first byte.  a = b = 0 gives dist = 0 and the empty script.
 *   Derived: where both apply (q0 = 0, q1 = m_p, D <= k <= 32) the runs equal what pfp_fm_cigar gives for (p, t0, t1) at k.
 *   F out of range or an index without text: PFP_EINVAL.  Pattern offsets that decrease: PFP_EINVAL.
 *
 * 2. Aligning a chain.  Inputs: patterns, anchors as pfp_fm_chain takes them (its refusals hold), G, B, S, max_chains, and F.
 * The chains, their order and their seven fields are exactly pfp_fm_chain's.  Per chain in addition:
 *   members: the anchors the peel's walk listed for the chain, written in increasing order c_0 .. c_{n-1}, as indices inside the
 *     pattern's segment of anchors (uint32): mem[mem_off[c] .. mem_off[c+1]).
 *   trimming: c_0 is kept whole.  For r >= 1 let o = max(0, qe_{r-1} - i_r, te_{r-1} - t_r); anchor r becomes (i_r + o, len_r - o,
 *     t_r + o): it begins where the one before it has ended on both sides.  Derived: o <= len_r - 1, so every trimmed anchor
 *     keeps at least one byte - qe_{r-1} - i_r = len_r - dq and te_{r-1} - t_r = len_r - dt, and a predecessor has dq, dt >= 1.
 *     An anchor's ends qe_r, te_r do not move, so trimming needs no order.
 *   gaps: gap r >= 1 is the segment P[qe_{r-1} .. i_r + o) against T[te_{r-1} .. t_r + o).  Derived: the two lengths are dq - (len_r
 *     - o) and dt - (len_r - o), so |a - b| = |dt - dq| <= B and a, b < G.  A gap with a = b = 0 adds nothing; a gap that has a
 *     script under layer 1 at F adds that script; any other gap is UNFILLED: it adds a I then b D (a length 0 is left out) and
 *     counts in `unfilled`.
 *   the script of a chain: len_0 '=', then for r = 1 .. n-1 gap r's runs and len_r - o '='; neighbouring runs of one operation are
 *     merged.  It aligns P[aqs .. qe) to T[ats .. te) with aqs = i_0 and ats = t_0, the FIRST MEMBER'S.  These are not always the
 *     chain's qs and ts, which are minima over the members.  In a chain that the programme walks from an anchor without a parent
 *     they are (derived: f_j <= qe_j - i_0 along it, so a later anchor that begins before i_0 is longer than any f_j + gain and
 *     takes no parent; the same for t): the pair (0,20,1000) (5,100,930), which would differ, does not chain - dq = 85, dt = 10,
 *     g = 75, 20 + 10 - 19 = 11 <= 100 - and gives two chains of one anchor.  A chain that the peel cuts off at a visited anchor
 *     can differ.  Example, G = 5000, B = 10, S = 1: anchors (0,50,1000) (60,30,1058) (60,20,1070) (55,40,1066) (95,50,1093) have f =
 *     50, 79, 67, 81, 129 and parents -, 0, 0, 2, 1.  The peel takes 4, 1, 0 (score 129), then 3, 2 and stops at the visited 0: the
 *     chain (60,20,1070) (55,40,1066) with score 31, qs = 55, ts = 1066, but aqs = 60, ats = 1070.  Its second anchor is trimmed by o
 *     = max(0, 80 - 55, 1090 - 1066) = 25 to (80,15,1091); gap 1 is P[80 .. 80) against T[1090 .. 1091); the script is 20= 1D 15=,
 *     nm = 1, and it aligns P[60 .. 95) to T[1070 .. 1106).
 *   nm: the sum of the script's X, I and D lengths.  Derived: nm = the sum of the filled gaps' dist plus a + b of the unfilled.
 *
 * 3. Long reads: pfp_fm_map_long's arguments plus F; its outputs unchanged and bit-equal; per RETURNED chain (1 + max_sec per
 * read; no other chain is aligned) aqs, ats, nm, unfilled and the script.  The script reads along the strand's pattern, that is
 * along the text, as SAM's does.  aqs is the strand's aqs turned into the read AS GIVEN as pfp_fm_map_long turns qs: strand 0:
 * aqs; strand 1: m - aqs.  So the script covers the read's bytes [aqs, qe) on strand 0 and [qs, aqs) on strand 1 (qs, qe: this
 * call's outputs; on strand 1 qs = m - qe of the strand's pattern is exact and the turned value is the stretch's END).
 *
 * Bounds: a gap costs a rows over a band of at most F + 2 cells per round, at most five rounds (slack 8, 32, 128, 512, 2048, cut
 * where the band proves D > F or holds the whole matrix), and a walk of at most a + b steps by one lane; gaps with a = 0, b = 0
 * or a = b = 1 cost one lane a few loads.  The members' walk is a bounded, resumable launch under PFP_FM_CHAIN_STEPS.
 * Device memory on top of the caller's buffers and of what pfp_fm_chain_dev / pfp_fm_map_long_dev take: 4 bytes per member and 57
 * per gap (a member has one: its segment, its trimmed length, dist, run count, slot address, round and bucket) plus 32 per gap
 * during a round for the plan; the runs of a band-filled gap wait in a slot of 4 min(2 min(F, |a - b| + 2e + 1) + 1, a + b)
 * bytes; the records of a pass take a / 16 (rounded up) times the band's width (16, 32, 64, 256, 1024 or 4160 cells) times 4
 * bytes - 68 MB for the largest legal gap - and live only during a launch: a round's gaps go through in consecutive chunks whose
 * records fit 1 GiB (a choice, not a measurement; PFP_FM_FILL_SCRATCH=BYTES, read per call, lowers it), and one that needs more
 * goes alone.
 * ------------------------------------------------------------------------------------ */
#define PFP_FM_FILL_MAX_F 4096
#define PFP_FM_FILL_MAX_LEN 65535
/* device pointers, patterns as in pfp_fm_count_dev; segment i is (d_seg_pat[i], d_q0[i], d_q1[i], d_t0[i], d_t1[i]).  d_dist (nseg,
 * uint32) and d_cig_off (nseg + 1, exclusive sums of the run counts) are filled; d_cig NULL: those only, else room for
 * d_cig_off[nseg] uint32 */
int pfp_fm_fill_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_seg_pat, const uint64_t *d_q0,
                    const uint64_t *d_q1, const uint64_t *d_t0, const uint64_t *d_t1, uint64_t nseg, uint64_t max_fill, uint32_t *d_dist,
                    uint64_t *d_cig_off, uint32_t *d_cig);
/* host buffers; *cig is a malloc'ed array of cig_off[nseg] entries (pfp_free; NULL when none) */
int pfp_fm_fill(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *seg_pat, const uint64_t *q0,
                const uint64_t *q1, const uint64_t *t0, const uint64_t *t1, uint64_t nseg, uint64_t max_fill, uint32_t *dist, uint64_t *cig_off,
                uint32_t **cig);
/* device pointers: patterns as in pfp_fm_count_dev; anchors, G, B, S, max_chains and the seven fields as in pfp_fm_chain_dev.  Everything behind
 * d_chain_off NULL: the chains' offsets only.  Otherwise the seven fields, d_aqs, d_nm, d_unfilled (uint32), d_ats (uint64) and
 * d_cig_off (d_chain_off[npat] + 1 entries) are required; d_cig NULL: no runs, else room for d_cig_off[last] uint32; d_mem_off
 * (d_chain_off[npat] + 1) and d_mem (uint32, room for the sum of the chains' n) may each be NULL. */
int pfp_fm_chain_align_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint64_t *d_anc_off,
                           const uint64_t *d_anc, uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_chains, uint64_t max_fill,
                           uint64_t *d_chain_off, uint32_t *d_score, uint32_t *d_n, uint32_t *d_qs, uint32_t *d_qe, uint64_t *d_ts, uint64_t *d_te,
                           uint32_t *d_match, uint32_t *d_aqs, uint64_t *d_ats, uint32_t *d_nm, uint32_t *d_unfilled, uint64_t *d_cig_off,
                           uint32_t *d_cig, uint64_t *d_mem_off, uint32_t *d_mem);
/* host buffers: chain_off (npat + 1) is filled; the arrays behind it are malloc'ed (pfp_free each; NULL when there is none):
 * chain_off[npat] entries each, *cig_off and *mem_off one more, *cig (*cig_off)[last] and *mem (*mem_off)[last]; mem_off and mem
 * may be NULL */
int pfp_fm_chain_align(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint64_t *anc_off, const uint64_t *anc,
                       uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_chains, uint64_t max_fill, uint64_t *chain_off,
                       uint32_t **score, uint32_t **n, uint32_t **qs, uint32_t **qe, uint64_t **ts, uint64_t **te, uint32_t **match,
                       uint32_t **aqs, uint64_t **ats, uint32_t **nm, uint32_t **unfilled, uint64_t **cig_off, uint32_t **cig,
                       uint64_t **mem_off, uint32_t **mem);
/* pfp_fm_map_long_dev's arguments with max_fill behind thresholds, and behind its outputs: d_aqs, d_nm, d_unfilled (uint32), d_ats
 * (uint64), d_hit_off[npat] entries each, and d_cig_off (one more); required whenever the ten are given, and NULL with them.
 * d_cig NULL: no runs, else room for d_cig_off[last] uint32 */
int pfp_fm_map_long_aln_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                            uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_sec, int thresholds, uint64_t max_fill,
                            uint64_t *d_hit_off, uint8_t *d_mapq, uint64_t *d_nchains, uint8_t *d_strand, uint32_t *d_seq, uint64_t *d_off,
                            uint64_t *d_ts, uint64_t *d_te, uint32_t *d_qs, uint32_t *d_qe, uint32_t *d_score, uint32_t *d_n, uint32_t *d_match,
                            uint32_t *d_aqs, uint64_t *d_ats, uint32_t *d_nm, uint32_t *d_unfilled, uint64_t *d_cig_off, uint32_t *d_cig);
/* host buffers, grouped as pfp_fm_map_long groups the reads; *aqs, *ats, *nm, *unfilled: hit_off[npat] entries, *cig_off one more,
 * *cig (*cig_off)[last] (malloc'ed; pfp_free each) */
int pfp_fm_map_long_aln(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                        uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_sec, int thresholds, uint64_t max_fill,
                        uint64_t *hit_off, uint8_t *mapq, uint64_t *nchains, uint8_t **strand, uint32_t **seq, uint64_t **off, uint64_t **ts,
                        uint64_t **te, uint32_t **qs, uint32_t **qe, uint32_t **score, uint32_t **n, uint32_t **match, uint32_t **aqs,
                        uint64_t **ats, uint32_t **nm, uint32_t **unfilled, uint64_t **cig_off, uint32_t **cig);
/* measurement (tools/fill_time.py; counted only under PFP_FM_MS_STATS=1): gaps, trivial gaps, then for each of the six band
 * widths the gaps that went through a pass of it and the cells of those passes; the counters are reset */
int pfp_fm_fill_stats(pfp_fm *fm, uint64_t out[14]);

/* ------------------------------------------------------------------------------------
 * Matching statistics and maximal exact matches over the same index (csrc/fmsearch.hip).  The reference has no counterpart:
 * the method is PHONI (Boucher, Gagie, I, Koppl, Langmead, Manzini, Navarro, Pacheco, Rossi, "PHONI: Streamed Matching
 * Statistics with Multi-Genome References", DCC 2021), which refines Bannai, Gagie, I, "Refining the r-index" (2020): backward
 * steps over the BWT, and where the BWT byte differs a jump to the nearest row above or below that carries the wanted byte - a run
 * end or a run start, so its SA value is a sample - chosen by a longest-common-extension query on the text.
 * Conventions as in "Searching a BWT".  For a pattern P of m bytes and every i in [0, m):
 *   len[i] = the largest l <= m - i such that P[i .. i+l) occurs in T.  It is 0 where P[i] is byte 0 or a byte T does not hold.
 *   pos[i] = a text position with T[pos[i] .. pos[i]+len[i]) = P[i .. i+len[i]); UINT64_MAX where len[i] = 0.  Several positions
 *     can qualify; which one is returned is fixed by the algorithm below, so it depends on the inputs only - not on the batch,
 *     the launch budget or the schedule.
 *   a MEM of P is a triple (i, len[i], pos[i]) with len[i] >= min_len (>= 1) and (i = 0 or len[i-1] <= len[i]).  (len[i-1] <=
 *     len[i] + 1 always holds; the match at i extends to the left exactly when len[i-1] = len[i] + 1.  It cannot extend to the
 *     right by the definition of len.)  The MEMs of a pattern are listed by increasing i.
 * Algorithm, per pattern, right to left, state (q, pos, l) with SA[q] = pos and T[pos .. pos+l) = P[i+1 .. i+1+l); start with
 * q = 0, pos = n, l = 0.  For i = m-1 .. 0, c = P[i]:
 *   1. c is byte 0 or a byte T does not hold: l = 0, len[i] = 0, (q, pos) stay.
 *   2. BWT[q] = c: q = LF(q), pos -= 1, l += 1.
 *   3. otherwise q_p = the last row before q and q_s = the first row after q whose BWT byte is c (a run end and a run start);
 *      l_p = min(l, LCE(SA[q_p], pos)), l_s = min(l, LCE(SA[q_s], pos)), a side that does not exist loses; take q_p if l_p >= l_s,
 *      else q_s; with the chosen row x: q = LF(x), pos = SA[x] - 1, l = l_x + 1.  When l = 0 no text is read.
 *   4. len[i] = l, pos[i] = pos.
 * A pattern that mismatches at every step compares O(m^2) bytes; the work of one kernel launch is bounded per pattern and the
 * library launches until every pattern is done (PFP_FM_MS_STEPS=K in the environment, read per call, lowers that bound: tests).
 * len is 32 bits: the two arrays have one entry per pattern BYTE; a single pattern of 2^32 - 1 bytes or more is PFP_ELIMIT.
 * Not checked: that the text given is the BWT's (wrong text or wrong SA values give wrong answers, never a read outside the
 * index).  Device memory: an index with text holds at most (n + 256) bytes and w bytes per run more than the plain index with
 * samples; a query takes 32 bytes per pattern on top of the caller's buffers; building by inversion peaks at the index plus what
 * pfp_unbwt_dev needs (its 4 / 8 bytes per row are transient).  pfp_fm_count* / pfp_fm_locate* work on such an index as on a
 * plain one.  pfp_fm_ms* / pfp_fm_mems* on an index without text: PFP_EINVAL.
 * ------------------------------------------------------------------------------------ */
/* as pfp_fm_build_dev with both sample files (required: PFP_EINVAL otherwise), plus the text: d_text = n_plus_1 - 1 device bytes,
 * or NULL: the library inverts d_bwt itself (bytes that are not one LF cycle: PFP_EFORMAT).  The index copies what it keeps. */
int pfp_fm_build_ms_dev(pfp_ctx *ctx, const void *d_bwt, uint64_t n_plus_1, const void *d_ssa10, uint64_t ssa_bytes,
                        const void *d_esa10, uint64_t esa_bytes, const void *d_text, pfp_fm **out);
/* reads <base>.bwt / .ssa / .esa; the text as in pfp_check_bwt_files (host pointer, or bytes [text_offset, text_offset + n) of
 * text_fd), or text == NULL and text_fd < 0: inverted.  n != rows - 1 -> PFP_EINVAL naming both numbers. */
int pfp_fm_build_ms_files(pfp_ctx *ctx, const char *base, const uint8_t *text, int text_fd, uint64_t text_offset, uint64_t n,
                          pfp_fm **out);
/* d_len (uint32) and d_pos (uint64, may be NULL) run parallel to d_pat: entry t belongs to pattern byte d_pat[t],
 * d_pat_off[0] <= t < d_pat_off[npat]; entries outside that range are not touched.  A pair of decreasing offsets: no pattern. */
int pfp_fm_ms_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint32_t *d_len, uint64_t *d_pos);
/* from pfp_fm_ms_dev's outputs: d_mem_off (npat + 1) = exclusive sums of the patterns' MEM counts; d_mem (NULL: offsets only)
 * = 3 uint64 per MEM {i, len, pos}, i counted from the pattern's first byte.  min_len = 0: PFP_EINVAL. */
int pfp_fm_mems_dev(pfp_fm *fm, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_len, const uint64_t *d_pos,
                    uint64_t min_len, uint64_t *d_mem_off, uint64_t *d_mem);
/* measurement: out = {kernel launches of the matching-statistics calls, steps that took step 3, bytes their extensions matched}
 * since the index was built or this was last called; the last two are collected only while PFP_FM_MS_STATS=1 is in the
 * environment (two atomic additions per pattern and launch) */
int pfp_fm_ms_stats(pfp_fm *fm, uint64_t out[3]);
/* host buffers; len / pos hold pat_off[npat] - pat_off[0] entries (pos NULL ok); offsets that decrease: PFP_EINVAL */
int pfp_fm_ms(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos);
/* mem_off (npat + 1) and *mems, a malloc'ed array of 3 mem_off[npat] uint64 (pfp_free; NULL when there are none) */
int pfp_fm_mems(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_len, uint64_t *mem_off,
                uint64_t **mems);

/* ------------------------------------------------------------------------------------
 * The LCP array and thresholds of a BWT, and matching statistics in two passes with thresholds (csrc/lcp.hip).  The reference
 * has no counterpart.  Sources: Karkkainen, Manzini, Puglisi, "Permuted longest-common-prefix array" (CPM 2009); Bannai, Gagie,
 * I, "Refining the r-index" (2020); Rossi, Oliva, Langmead, Gagie, Boucher, "MONI: a pangenomic index for finding maximal exact
 * matches" (2022).  Conventions as in "Inverting and checking a BWT": rows j = 0..n, SA[0] = n.
 *   LCP[0] = 0; for j >= 1, LCP[j] = the length of the common prefix of T[SA[j-1]..n) and T[SA[j]..n).  So LCP[1] = 0.
 *   Runs k = 0..r-1 of the BWT have start row s_k, end row e_k and byte c_k; prev(k) = the largest k' < k with c_k' = c_k.
 *   thr[k] = 0 if prev(k) does not exist; otherwise the SMALLEST row t in (e_prev(k), s_k] with LCP[t] = min LCP(e_prev(k), s_k].
 *     (The range holds at least run k-1 and s_k.)
 *   Irreducible values: row j starts a run exactly when LCP[j] is irreducible.  Then SA[j] is an .ssa value, SA[j-1] the .esa
 *     value of the run before, and LCP[j] their longest common extension on the text.  In text order PLCP[i] = PLCP[i0] - (i - i0)
 *     with i0 the largest run-start SA value <= i (position 0 always is one: the byte before it is the 0), and LCP[j] =
 *     PLCP[SA[j]]: r extensions and one pass that knows SA[j] at every row (the inverter's walk) give the whole array.
 * Matching statistics with thresholds, per pattern P of m bytes; len and pos mean what they mean in "Matching statistics".
 *   Pass 1, for i = m-1 .. 0, state (q, pos) starting from (0, n), c = P[i]:
 *     1. c is byte 0 or a byte T does not hold: pos[i] = none, the state stays.
 *     2. BWT[q] = c: q = LF(q), pos -= 1.
 *     3. otherwise q_p and q_s as in PHONI's step 3.  Only one exists: take it.  Else, with k the run q_s starts: take q_p if
 *        q < thr[k], else q_s.  With the chosen row x: q = LF(x), pos = SA[x] - 1.
 *     4. pos[i] = pos.
 *   Pass 2, for i = 0 .. m-1, starting with l = 0: pos[i] none: l = 0.  Otherwise l = max(l - 1, 0), then l grows while
 *     i + l < m, pos[i] + l < n and P[i+l] = T[pos[i]+l].  len[i] = l; pos[i] becomes UINT64_MAX where len[i] = 0.
 *   len equals what pfp_fm_ms* gives.  pos may differ from PHONI's where several positions qualify; it is fixed by the rules
 *   above, so it depends on the inputs only - not on the batch, the launch budget or the schedule.  Pass 1 reads no text; pass 2
 *   matches at most m bytes of a pattern of m bytes, whatever the input (PHONI compares O(m^2) in the worst case).
 * Work per launch is bounded in every kernel and unfinished work resumes from a small record, as in pfp_fm_ms*: an irreducible
 * value can be as long as the text (a^n has one of n - 1 bytes).  PFP_FM_MS_STEPS=K lowers these bounds too.
 * Files: <base>.lcp holds n + 1 and <base>.thr_pos r values as 5-byte little-endian ints, like .sa.  This is the project's own
 * format; MONI's pfp-thresholds is believed to write .thr_pos in the same layout, which has not been checked.
 * Not checked: the SA values of the samples and that the text is the BWT's (pfp_check_bwt_files checks both); wrong ones, or wrong
 * thresholds, give wrong answers, never a read outside the index.
 * Device memory, with w = 4 bytes below 2^32 rows, 8 above: the index keeps w bytes per run more.  Computing LCP or thresholds
 * peaks at the index with text plus 3 w bytes per row (PLCP, LCP and the walk's LF, all transient) plus 0.1875 bytes per row
 * (the LF build's histograms) plus at most 16 + 7.75 w bytes per run, plus the scratch of a library scan and of a library sort
 * of the runs; pfp_lcp_files adds 5 bytes per row and / or per run for the file images.
 * ------------------------------------------------------------------------------------ */
#define PFP_LCP_LCP 1
#define PFP_LCP_THR 2
/* device pointers as in pfp_fm_build_ms_dev (d_text NULL: inverted); d_lcp (n_plus_1 uint64) and d_thr (runs uint64) may each be
 * NULL; *runs (NULL ok) gets r, so a call with both NULL tells the size d_thr needs.  Nothing stays allocated. */
int pfp_lcp_dev(pfp_ctx *ctx, const void *d_bwt, uint64_t n_plus_1, const void *d_ssa10, uint64_t ssa_bytes, const void *d_esa10,
                uint64_t esa_bytes, const void *d_text, uint64_t *d_lcp, uint64_t *d_thr, uint64_t *runs);
/* reads <base>.bwt / .ssa / .esa, the text as in pfp_fm_build_ms_files; writes <base>.lcp (what & PFP_LCP_LCP) and / or
 * <base>.thr_pos (what & PFP_LCP_THR) */
int pfp_lcp_files(pfp_ctx *ctx, const char *base, const uint8_t *text, int text_fd, uint64_t text_offset, uint64_t n, int what);
/* gives an index built by pfp_fm_build_ms_* its thresholds: from d_thr5 (device image of a .thr_pos, bytes != 5 r: PFP_EFORMAT;
 * values above the rows count as the row count), or d_thr5 NULL: computed from the index.  An index without text: PFP_EINVAL. */
int pfp_fm_thresholds_dev(pfp_fm *fm, const void *d_thr5, uint64_t bytes);
/* the same from <base>.thr_pos (a file that cannot be read: PFP_EINVAL naming it) */
int pfp_fm_thresholds_files(pfp_fm *fm, const char *base);
/* pfp_fm_ms_dev / pfp_fm_ms / pfp_fm_mems by the two passes above; an index without thresholds: PFP_EINVAL.  pfp_fm_mems_dev
 * works on the outputs of pfp_fm_ms_thr_dev unchanged.  pfp_fm_ms_stats counts their launches (and those that compute
 * thresholds) and, under PFP_FM_MS_STATS=1, the steps of pass 1 that jumped and the bytes pass 2 matched. */
int pfp_fm_ms_thr_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint32_t *d_len, uint64_t *d_pos);
int pfp_fm_ms_thr(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos);
int pfp_fm_mems_thr(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_len, uint64_t *mem_off,
                    uint64_t **mems);

/* ------------------------------------------------------------------------------------
 * Sequences of a collection: locate that stays inside one sequence, positions as (sequence, offset), and document listing
 * (csrc/seqmap.hip).  The reference has no counterpart.  `bigbwt -f` concatenates the records of a FASTA / FASTQ file with no
 * separator, so the index alone cannot tell a match inside a record from one that begins in the tail of a record and ends in
 * the head of the next; `bigbwt -f --seqs` also writes the table these calls need (host/seqs.h: the <base>.seqs format).
 * Conventions as in "Searching a BWT".  A table is nseq + 1 values starts[0..nseq] with starts[0] = 0, starts[k] <= starts[k+1]
 * and starts[nseq] = n: sequence k is T[starts[k] .. starts[k+1]), and it may be empty.
 *   seq(x), for a text position x < n: the one k with starts[k] <= x < starts[k+1] - never an empty sequence; off(x) = x - starts[k].
 *     For x >= n (SA[0] = n, and UINT64_MAX, the "none" of matching statistics): seq = UINT32_MAX, off = UINT64_MAX.
 *   kept: an occurrence x of a pattern of m bytes is kept when x < n and x + m <= starts[seq(x) + 1]: it lies inside one sequence.
 *     The empty pattern keeps every x < n.
 *   locate with sequences: the positions pfp_fm_locate_dev lists for the same arguments (row order, at most max_occ ROWS per
 *     pattern, 0: all) that are kept, still in row order, as (seq, off).  The cap applies before the filter.
 *   document listing: per pattern the distinct seq(x) over ALL its kept occurrences (no cap), by increasing sequence number, each
 *     with its number of kept occurrences.  The results depend on the inputs only - not on the batch or the schedule.
 * Checked by pfp_fm_set_seqs: the three rules above and nseq in [1, 2^32 - 2] (else PFP_EINVAL naming the first bad entry).  Not
 * checked: that the table is the one the text was built with - another table of the same total gives answers for that table.
 * Every other call of this section on an index without a table: PFP_EINVAL.
 * Method.  seq(x) is a predecessor search, done as phi^-1 does it: a directory over text positions with about one start per
 * bucket, then a binary search among the bucket's starts.  Locate with sequences: the plain locate, one lane per position for
 * seq(x) and the test, a library scan of the flags, a scatter.  Document listing, on the kept hits: with at most 4096 sequences one
 * workgroup per 32768 hits of a pattern counts them in an LDS histogram (a pattern with more hits is split, its pieces meet in
 * a counter row in device memory) and the non-zero counters are written in order; with more sequences each pattern's
 * sequence numbers are sorted by the library's segmented sort and run-length encoded.  Work per launch is bounded in every
 * kernel (PFP_FM_MS_STEPS=K lowers the hits per workgroup to K: tests).
 * Device memory, with w = 4 bytes below 2^32 rows, 8 above: the index keeps at most (w + 8) (nseq + 1) + 16 bytes for the table
 * and its directory (in pfp_fm_info's device_bytes).  With U = the positions plain locate lists for the same arguments (what its
 * offsets-only call reports) and K <= U the kept ones: pfp_fm_locate_seqs_dev takes 20 U bytes and 8 per pattern on top of
 * what pfp_fm_locate_dev takes and of the caller's buffers; pfp_fm_doclist_dev takes that and 4 K + 8 per pattern, then - the
 * 20 U released - at most 16 K + 8 bytes per document listed + 16 per pattern (sort regime) or 5 K + 48 per pattern (histogram
 * regime: 4 K, and 8 nseq per pattern of more than 32768 kept hits), plus the scratch of the library's scans and sort.  2^32 - 1
 * or more kept hits in one call of the sort regime: PFP_ELIMIT.
 * The host-buffer calls bound this: they hold at most PFP_SEQ_BUDGET = 2^26 located positions on the device at once (at most 32
 * bytes each with their own output buffers, 2.1 GB, plus locate's 24 per segment) and take the patterns of a call in consecutive
 * groups under that budget; a pattern with more positions goes alone.  The sizes come from the offsets-only locate, so no
 * pattern is located twice.  On top of that they keep 40 bytes per pattern of the call on the device.  PFP_FM_SEQ_BUDGET=K in the
 * environment, read per call, lowers the budget (tests).
 * ------------------------------------------------------------------------------------ */
#define PFP_SEQ_BUDGET (1ull << 26)
/* starts: nseq + 1 host values.  The index copies them (as u32 below 2^32 rows, u64 above) and builds the directory; a second
 * call replaces the table. */
int pfp_fm_set_seqs(pfp_fm *fm, const uint64_t *starts, uint64_t nseq);
/* device pointers: d_seq (uint32) and d_off (uint64) get seq(x) and off(x) of the count positions d_pos; either may be NULL.  Any
 * positions do: locate's, those of matching statistics, or the third column of MEM triples gathered by the caller. */
int pfp_fm_seqmap_dev(pfp_fm *fm, const uint64_t *d_pos, uint64_t count, uint32_t *d_seq, uint64_t *d_off);
/* device pointers; d_pat_off / npat / d_sp / d_ep / d_first / max_occ as pfp_fm_count_dev gave and pfp_fm_locate_dev takes them
 * (only the patterns' lengths are read from d_pat_off).  d_out_off (npat + 1): exclusive sums of the kept counts, so
 * d_out_off[npat] is the number kept.  d_seq (uint32) / d_off (uint64): pattern p's kept hits at d_out_off[p] .. d_out_off[p+1];
 * both need room for the UNFILTERED total, which is what the offsets-only call of pfp_fm_locate_dev reports - one pass is
 * then enough.  Both NULL: the offsets only; one NULL: PFP_EINVAL. */
int pfp_fm_locate_seqs_dev(pfp_fm *fm, const uint64_t *d_pat_off, uint64_t npat, const uint64_t *d_sp, const uint64_t *d_ep,
                           const uint64_t *d_first, uint64_t max_occ, uint64_t *d_out_off, uint32_t *d_seq, uint64_t *d_off);
/* device pointers as above.  d_doc_off (npat + 1): exclusive sums of the patterns' document counts; d_doc (uint32) / d_cnt
 * (uint64), room for d_doc_off[npat] each: the documents and their hit counts.  Both NULL: the offsets only. */
int pfp_fm_doclist_dev(pfp_fm *fm, const uint64_t *d_pat_off, uint64_t npat, const uint64_t *d_sp, const uint64_t *d_ep,
                       const uint64_t *d_first, uint64_t *d_doc_off, uint32_t *d_doc, uint64_t *d_cnt);
/* count, locate and filter with host buffers: sp / ep (NULL ok) get the row ranges, out_off (npat + 1) the offsets of the kept
 * hits, *seq / *off malloc'ed arrays of out_off[npat] entries (pfp_free; NULL when there are none) */
int pfp_fm_locate_seqs(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t max_occ, uint64_t *sp,
                       uint64_t *ep, uint64_t *out_off, uint32_t **seq, uint64_t **off);
/* the same for document listing: doc_off (npat + 1), *doc / *cnt malloc'ed arrays of doc_off[npat] entries */
int pfp_fm_doclist(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t *doc_off, uint32_t **doc,
                   uint64_t **cnt);

/* ---- micro entry points used by bench.py's roofline leg and by the parity tests ---- */
/* copy a device-resident text into the ctx's padded staging buffer (T' = Dollar.T.Dollar^w) */
int pfp_stage_text_dev(pfp_ctx *ctx, const void *d_text, uint64_t n, int w);
/* run only stage 1a (K1 window-hash + trigger mask, block-count scan, K2 compaction) on the
 * staged text; all work is enqueued on pfp_ctx_stream(ctx) and finished on return. */
int pfp_scan_staged(pfp_ctx *ctx, uint64_t p, uint64_t *n_ends);
/* enqueue only K1 (the window-hash kernel, n + n/8 bytes of traffic) - no sync, for event timing */
int pfp_scan_k1_enqueue(pfp_ctx *ctx, uint64_t p);

#ifdef __cplusplus
}
#endif
#endif
