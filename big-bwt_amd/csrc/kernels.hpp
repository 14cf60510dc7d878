// kernels.hpp -- declarations shared by the pipeline translation units.
#pragma once
#include "common.hpp"
#include "wordview.hpp"

namespace pfp {

// ---------------------------------------------------------------- text staging
// T' = Dollar . T . Dollar^w lives in HBM with a zeroed 64-byte front pad so that T[0] is
// 16-byte aligned, T'[x] = tprime()[x], and short unaligned over-reads stay inside the buffer.
struct StagedText {
  static constexpr size_t kFront = 64, kBack = 128;
  DBuf<uint8_t> buf;
  uint64_t n = 0;
  int w = 0;
  const uint8_t *tbase() const { return buf.p + kFront; }        // T[i]
  const uint8_t *tprime() const { return buf.p + kFront - 1; }   // T'[x]
  void stage(pfp_ctx *c, const void *src, bool src_on_device, uint64_t n_, int w_);
  void stage_fd(pfp_ctx *c, int fd, uint64_t file_off, uint64_t n_, int w_);      // host text read from an open file (parallel pread)
  void restage_tail(pfp_ctx *c, uint64_t new_n, int w_) const;    // Dollars at [new_n,new_n+w), zeros after
};

// ---------------------------------------------------------------- stage 1a (scan.hip)
struct KRParams {
  static constexpr uint32_t kMaxExtra = 32;
  uint32_t negpw, pinv, pshift, plimit;
  float fdens = 1.0f;                          // the density the scan cuts at (x nominal)
  uint32_t fthr_nom = 0, fauto = 0;            // nominal threshold (density 1 / p); fauto: the chain chooses between fthr_nom and fthr = twice that
  uint32_t fast = 0, fseed = 0, fthr = 0;      // fused chain only (round 4): the cheap window hash of scan.hip instead of Karp-Rabin
  uint32_t nextra;            // extra trigger hashes (fused chain only), 0 in the reference-exact scan
  uint64_t bloom;             // bit (h & 63) set for every extra hash
  uint32_t extra[kMaxExtra];
};
KRParams make_kr_params(int w, uint64_t p);
KRParams make_fast_params(pfp_ctx *c, const StagedText &tx, uint64_t n, int w, uint64_t p);
KRParams make_fast_params_host(const uint8_t *first_window, int w, uint64_t p, double density_setting, double *density_used);
KRParams params_from_plan(int w, uint64_t p, const uint64_t plan[4]);      // a rank's parameters under a parse plan (pfp_dist_parse_plan)
// phrase length by repetitiveness (scan.hip): the pieces the single-GPU chain runs in one go and the multi-GPU chain with an
// all-gather of the ranks' samples in between
struct CutSample { DBuf<uint8_t> nominal; DBuf<uint64_t> hashes; uint64_t ns = 0, counted = 0; };      // counted: sampled cuts, ns: those that found room
void classify_cuts(pfp_ctx *c, const StagedText &tx, int w, const DBuf<uint64_t> &d_ends, uint64_t ne, const KRParams &kp, uint64_t min_end,
                   CutSample &out);
bool sample_says_dense(pfp_ctx *c, const uint64_t *d_sorted, uint64_t ns, uint64_t p, uint64_t counts[2] = nullptr);
uint64_t keep_nominal_cuts(pfp_ctx *c, DBuf<uint64_t> &d_ends, uint64_t ne, const DBuf<uint8_t> &nominal);
uint32_t window_hash_host(const uint8_t *win, int w, uint32_t seed);      // the seeded window hash of scan.hip, on the host
void scan_flags(pfp_ctx *c, const uint8_t *tbase, uint64_t n, int w, uint64_t p, uint16_t *flags16,
                uint32_t *block_counts, unsigned long long *first_bad, const KRParams *kp_override = nullptr);
// classify (the window hash's first pass with automatic density): the settled pass also fills it, as classify_cuts(min_end = 0) would
uint64_t scan_text(pfp_ctx *c, const StagedText &tx, uint64_t n, int w, uint64_t p, DBuf<uint64_t> &d_ends,
                   uint64_t *n_used, const KRParams *kp_override = nullptr, CutSample *classify = nullptr);
uint32_t propose_extra_triggers(pfp_ctx *c, const StagedText &tx, uint64_t n_used, int w, uint64_t max_phrase,
                                const DBuf<uint64_t> &d_ends, uint64_t ne, KRParams &kp);
// what scan_text_adaptive did, for the diagnostic entry point pfp_debug_scan_chain (host memory only; the chain passes none)
struct ScanReport {
  KRParams first{}, kp{};       // the parameters of the first pass and of the last one
  bool chose = false, dense = false, kr_fallback = false;      // a density choice was made / it kept the dense cuts / no cut: Karp-Rabin
  uint64_t sampled = 0, kept = 0, distinct = 0, singles = 0;   // the choice's sample: cuts counted, cuts that found room, contexts
  std::vector<uint64_t> dense_ends;                            // the first pass's cuts and their "inside the nominal threshold" flags
  std::vector<uint8_t> nominal;
};
// fused chain: reference triggers plus a few extra window hashes that split phrases longer than max_phrase
uint64_t scan_text_adaptive(pfp_ctx *c, const StagedText &tx, uint64_t n, int w, uint64_t p, uint64_t max_phrase,
                            DBuf<uint64_t> &d_ends, uint64_t *n_used, uint32_t *n_extra, ScanReport *rep = nullptr);

// ---------------------------------------------------------------- stage 1b (phrase.hip)
// Distinct phrases (the dictionary), most frequent first (ties: first occurrence), plus the parse as word ids.
struct Dictionary {
  uint64_t P = 0;          // # phrases
  uint64_t d = 0;          // # distinct words
  uint64_t dsize = 0;      // bytes of dict incl. one 0x01 per word and the final 0x00
  DBuf<uint8_t> bytes;     // D (padded with zeros: +64 front is not needed, +64 back)
  DBuf<uint64_t> woff;     // [d+1] start of word j in bytes; woff[d] = dsize-1
  DBuf<uint32_t> wlen;     // [d]
  DBuf<uint32_t> wocc;     // [d]
  DBuf<uint32_t> pid;      // [P] word id of phrase k (empty when built from a .dict file)
  DBuf<uint8_t> last;      // [P] .last
  DBuf<uint64_t> sai;      // [P] .sai values
  uint64_t reseeds = 0;
};
void build_dictionary(pfp_ctx *c, const StagedText &tx, uint64_t n, int w, const DBuf<uint64_t> &ends, uint64_t n_ends,
                      bool want_sai, Dictionary &D);
// multi-GPU: a shard owns phrases [k0,k0+P) of its local scan; sai values are shifted by sai_base
void build_dictionary_shard(pfp_ctx *c, const StagedText &tx, uint64_t n, int w, const DBuf<uint64_t> &ends,
                            uint64_t n_ends, uint64_t k0, uint64_t P, bool want_sai, uint64_t sai_base, Dictionary &D);
// multi-GPU: dictionary of a union of word lists; D.pid[u] = id of union word u, occ = sum of weights
void build_dictionary_words(pfp_ctx *c, const uint8_t *bytes, const uint64_t *wstart, const uint32_t *wlen, uint64_t U,
                            const uint32_t *weight, uint64_t total_bytes, Dictionary &D);
// identity hash of every word of a list (same function the dedup sorts by)
void reorder_dictionary_by_occ(pfp_ctx *c, Dictionary &D, DBuf<uint32_t> &perm);      // words by descending occurrence; perm[old] = new
void hash_word_list(pfp_ctx *c, const uint8_t *bytes, const uint64_t *wstart, const uint32_t *wlen, uint64_t U, uint64_t seed,
                    uint64_t *d_hash);

// ---------------------------------------------------------------- suffix sorting (sufsort.hip)
// Index width.  Positions inside the dictionary and slots of its suffix array are `I` = uint32_t while the
// dictionary is shorter than 4 GiB and uint64_t beyond (the reference makes the same switch between its
// 32-bit and -DM64 builds, bigbwt:109-151, gsa/gsacak.h:42-60).  Everything that indexes the parse (P <=
// 2^32-2, bwtparse.c:93), words (d < 2^32) or a distance inside one word stays 32 bits wide in both builds.
template <class I> struct IdxTraits;
template <> struct IdxTraits<uint32_t> { using DKey = uint64_t; static constexpr uint32_t kNone = 0xFFFFFFFFu; static constexpr uint32_t kTop = 0x80000000u; };
template <> struct IdxTraits<uint64_t> { using DKey = unsigned __int128; static constexpr uint64_t kNone = ~0ull; static constexpr uint64_t kTop = 1ull << 63; };
// true when a dictionary of dsize bytes needs (or PFP_FORCE_IDX64 asks for) the wide build
// (the reference goes to its 64-bit build at 2^31 - 4 already, bigbwt:130; unsigned 32-bit positions reach twice as far, and
// the wide build needs 8 bytes where this one needs 4)
inline bool use_wide_index(const pfp_ctx *c, uint64_t dsize) { return c->force_wide || dsize >= 0xFFFFFFF0ull; }
// Dictionaries of 2^31 .. 2^32 bytes on one GPU (round 4): 32-bit positions still fit, but not with the sorter's "settled" flag in
// their top bit - the narrow build then has doubling rounds only (2.0 s for a 2.4 GB dictionary of 3 % variants); the wide build
// keeps its pivot rounds (1.25 s) at ~96 bytes of device memory per dictionary byte.  Width by cost: wide where that much memory
// is there (free on the device + cached in the pool), narrow otherwise.  profiles/r04_dictionary_2_to_4_gib.json
inline bool prefer_wide_index(const pfp_ctx *c, uint64_t dsize) {
  if (use_wide_index(c, dsize)) return true;
  if (dsize < (1ull << 31) || c->force_narrow) return false;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
  const uint64_t avail = (uint64_t)free_b + (c->pool.total_bytes - c->pool.live_bytes);
  return avail >= dsize * 100ull;
}

template <class I>
struct SuffixOrderT {
  double rep_hint = 0;   // set by the caller before sort_dict_suffixes: text bytes per dictionary byte (>= 2: a repetitive collection)
  uint64_t N = 0;        // slots held here: all NP suffixes, or (key-range sharded sort) one contiguous range of SA(D), or (sort_dict_suffixes
                         // with a minimum length) the suffixes that emit something, numbered among themselves
  uint64_t NP = 0;       // positions of the sorted string
  uint64_t slot_base = 0;        // range mode: SA(D) slot of local slot 0
  uint64_t range_emits = 0;      // range mode: BWT positions the range emits (when a count source was given)
  uint64_t klo = 0, khi = ~0ull; // range mode: first-round keys in [klo, khi) (khi == ~0: no upper bound)
  bool range = false, complete = true;   // range mode stops (complete = false) where it would need other ranks' ranks
  DBuf<I> sa;            // [N] suffix start positions in sorted order (ties: position order)
  DBuf<I> grp;           // [N] grp[t] = first sa slot of slot t's group (equal strings share it)
  DBuf<I> rank;          // [NP] rank[i] = grp[slot of i]; kNone where the sorter never needed it (see RankView); not allocated
                         // where no round ever read it (then: wordrank; plain mode: nothing - sa and grp are the result)
  DBuf<I> wordrank;      // [d+1] rank of word j's whole-word suffix where a round after the first settled it, else kNone
  uint64_t rounds = 0;
  // Dictionary mode keeps the sorted first-round keys: the rank of a suffix that the first round
  // already settled is the lower bound of its packed key among them, found on demand instead of
  // being scattered to rank[] for all N positions (the scatter was 9 ms of 56 at N = 260 M).
  DBuf<uint64_t> skeys;  // [N] packed keys of the first round in sorted order
  DBuf<I> tab;           // [T] kNone - (first slot whose key has top bits >= T-1-r), r reversed bucket
  DBuf<uint32_t> lut;    // [256] byte -> (alphabetic code << 6) | code length
  const uint8_t *bytes = nullptr;
  int kbits = 0, shift = 0;   // kbits code bits per key (+ 1 flag bit)
  uint32_t T = 0;
  I finbit = 0;          // dictionary mode: rank[] values carry this bit once their suffix is settled (0: N too large for a spare bit)
  // When the first-round keys leave 16 bits free, every key carries its suffix's merge record {preceding
  // char, count code} there (SlotPayloadSrc): it arrives at the suffix's slot with the sort, and the merge
  // reads it from skeys instead of gathering 2 bytes per slot at random (4.9 ms of 38 at N = 260 M).
  // refined[t] != 0: slot t was re-ordered after the first round, its record has to be fetched.
  int paybits = 0;
  uint64_t keymask = ~0ull;
  DBuf<uint8_t> refined;
  uint64_t n_refined = 0;
};
using SuffixOrder = SuffixOrderT<uint32_t>;
using SuffixOrder64 = SuffixOrderT<uint64_t>;
// what a merge record is made from: the word of a position (WordView), the words' occurrence counts, the window
struct SlotPayloadSrc { WordView wv; const uint32_t *wocc; int w; };
// device-side view for rank lookups (sufsort.hip: rank_at)
template <class I>
struct RankViewT {
  const I *rank; const uint64_t *skeys; const I *tab; const uint32_t *lut; const uint8_t *bytes;
  uint64_t N; int kbits, shift; uint32_t T; I finbit; uint64_t keymask;
  const I *wordrank;      // gather_ranks over the word starts: see SuffixOrderT::wordrank
};
template <class I> RankViewT<I> rank_view(const SuffixOrderT<I> &so);
// out[k] = rank of the suffix starting at pos[k]
template <class I> void gather_ranks(pfp_ctx *c, const SuffixOrderT<I> &so, const uint64_t *d_pos, uint64_t count, I *d_out);
// Suffixes of the dictionary as 0x01-terminated strings (gsacak semantics); wv answers where the
// word of a position ends (the final 0x00 is its own word).
// min_len > 0 (and PFP_DROP_SHORT unset or != 0, read per call): only the suffixes LONGER than min_len bytes (terminator not
// counted) are sorted - the merge's window w: a suffix of at most w bytes emits nothing (pfbwt.cpp:151), nor does the final
// 0x00.  out.N < out.NP then, sa / grp / skeys and every rank number the kept suffixes alone.  A dictionary with a word of at
// most min_len bytes, or one whose sort needs a doubling round (ranks of arbitrary positions), is sorted whole as with 0.
template <class I>
void sort_dict_suffixes(pfp_ctx *c, const uint8_t *bytes, uint64_t N, const WordView &wv, SuffixOrderT<I> &out,
                        const SlotPayloadSrc *pay = nullptr, int min_len = 0);
// multi-GPU: rank `part` of `parts` sorts the suffixes whose first-round key lies in its share of the key
// space (splitters from a deterministic key sample: every rank derives the same ones, no exchange);
// groups never straddle shares, and pivot rounds compare strings, not ranks, so a share is finished
// without its neighbours.  out.complete == false: a group was left that only doubling could settle.
template <class I>
void sort_dict_suffixes_range(pfp_ctx *c, const uint8_t *bytes, uint64_t N, const WordView &wv, uint32_t part,
                              uint32_t parts, SuffixOrderT<I> &out, const SlotPayloadSrc *pay = nullptr,
                              const SlotPayloadSrc *count = nullptr);
// range mode: out[j] = 1 + SA(D) slot of the whole-word suffix of word j if it belongs to this share, else 0 (count = d)
template <class I>
void gather_slots_range(pfp_ctx *c, const SuffixOrderT<I> &so, const WordView &wv, uint64_t count, uint64_t *d_out);
// plain suffix array of an integer string with unique smallest last symbol (sacak_int)
// max_sym: largest symbol value (spare key bits then describe runs of equal symbols)
// one rank's share of the same suffix array (the suffixes whose first-round key lies in share `part` of `parts`): out.N slots from
// out.slot_base on, out.complete = false where only a doubling round could go on
void sort_int_suffixes_range(pfp_ctx *c, const uint32_t *sym, uint64_t N, uint32_t max_sym, const uint32_t *occ, uint32_t n_sym,
                             uint32_t part, uint32_t parts, SuffixOrder &out);
// occ (optional, n_sym entries): occ[x - 1] = occurrences of symbol x - lets the sorter pick its pivots (the parse of a collection)
void sort_int_suffixes(pfp_ctx *c, const uint32_t *sym, uint64_t N, SuffixOrder &out, uint32_t max_sym = 0xFFFFFFFFu,
                       const uint32_t *occ = nullptr, uint32_t n_sym = 0);
// plain suffix array of a byte string with s[N-1]==0 unique smallest (sacak)
template <class I> void sort_byte_suffixes(pfp_ctx *c, const uint8_t *bytes, uint64_t N, SuffixOrderT<I> &out);

// ---------------------------------------------------------------- the dictionary index and the words' ranks (dictindex.hip)
struct DictIndex {        // word lookup over the dictionary (wordview.hpp): |D| / 16 + 8 d bytes, no per-position array
  DBuf<uint32_t> blk_word;   // [dsize / 64 + 1] word containing position 64 b
  DBuf<uint64_t> wend;       // [d+1] terminator position of word j (wend[d] = dsize-1)
  DBuf<uint32_t> lexrank;    // [d] 0-based lexicographic rank of word j
  DBuf<uint64_t> wslot_lex;  // [d] SA(D) slot (global) of the whole-word suffix of the word of lexicographic rank q
};
void build_dict_index(pfp_ctx *c, const Dictionary &D, DictIndex &ix);      // needs D.woff / D.wlen
inline WordView word_view(const Dictionary &D, const DictIndex &ix) {
  return WordView{D.bytes.p, ix.blk_word.p, ix.wend.p, (uint32_t)D.d, D.dsize};
}
// D.bytes/D.dsize given (words + 0x01, final 0x00): fills D.d, D.woff, D.wlen; at most max_words words expected
void word_table_from_bytes(pfp_ctx *c, Dictionary &D, uint64_t max_words);
template <class I> void compute_lexrank(pfp_ctx *c, const Dictionary &D, SuffixOrderT<I> &so, DictIndex &ix);
// d_wslot_all: `parts` arrays of d entries (u64), 1 + SA(D) slot of every word's first suffix or 0
void compute_lexrank_from_slots(pfp_ctx *c, const Dictionary &D, const uint64_t *d_wslot_all, uint32_t parts, DictIndex &ix);
template <class I> uint64_t count_slot_outputs(pfp_ctx *c, const Dictionary &D, const DictIndex &ix, const SuffixOrderT<I> &so, int w);

// ---------------------------------------------------------------- stage 2 (parsebwt.hip)
struct ParseBWT {         // outputs of bwtparse.c in HBM
  uint64_t P = 0;
  DBuf<uint32_t> ilist;    // [P+1]
  DBuf<uint8_t> bwlast;    // [P+1]
  DBuf<uint64_t> bwsai;    // [P+1] (only with SA flags)
  // [P+1] the sorted symbols of the inverted-list sort: iword[0] = the EOS symbol, iword[e + 1] = 1-based lexicographic rank of
  // the word inverted-list entry e belongs to.  Live until the merge ends; empty where the lists came from a file (the merge
  // then derives it from the words' counts)
  DBuf<uint32_t> iword;
  uint64_t rounds = 0;
};
// parse symbols are 1-based lexicographic ranks; occ_lex[r] = occurrences of rank r
// sa_given (optional): the suffix array of the parse + its end symbol, P + 1 entries, computed elsewhere
void parse_bwt(pfp_ctx *c, const uint32_t *parse_sym, uint64_t P, const uint8_t *last, const uint64_t *sai,
               const uint32_t *occ_lex, uint64_t d, ParseBWT &out, const uint32_t *sa_given = nullptr);

// ---------------------------------------------------------------- stage 3 (merge.hip)
struct BwtOutputs {
  uint64_t n_out = 0;      // n+1
  uint8_t *d_bwt = nullptr;    // [n+1] device, caller-provided
  uint64_t *d_sa = nullptr;    // [n+1] device, caller-provided when flags != 0
  uint64_t hard_groups = 0, hard_chars = 0, hard_big_groups = 0, hard_max_chars = 0, hard_max_members = 0;
  uint64_t hard_minor_groups = 0, hard_minor_chars = 0;   // groups handled by majority fill; occurrences ranked for them
  // -s / -e without -S (sparse SA): the run boundaries of the emitted BWT slice - bit r of bmap = position r starts or ends
  // a run, bpre[k] = boundaries before bit 64 k, n_bound of them in all.  With d_sa == nullptr the SA values live in
  // sa_c[rank of the position among the boundaries] (16 bytes per run instead of 8 per text byte); with d_sa given they
  // are stored there, at boundary positions only.
  DBuf<uint64_t> bmap, bpre, sa_c;
  uint64_t n_bound = 0;
  // ... and, when the emitted slice is the whole BWT, where runs start / end (the .ssa / .esa positions) with their
  // prefix counts: the sampled files are then written from the bitmaps alone, without another pass over the BWT bytes
  DBuf<uint64_t> smap, spre, emap, epre;
  uint64_t n_starts = 0, n_ends = 0;
  uint64_t slice_n = 0;        // positions the maps cover (the emitted slice; a slice's two edge positions count as boundaries)
};
// where the SA value of BWT position i (relative to the slice the arrays describe) is found
struct SaView {
  const uint64_t *dense = nullptr;                       // dense[i], or
  const uint64_t *bmap = nullptr, *bpre = nullptr, *sa_c = nullptr;      // sa_c[rank of i among the set bits of bmap]
  // whole BWT only: run starts / ends as bitmaps with prefix counts (null: find them in the BWT bytes)
  const uint64_t *smap = nullptr, *spre = nullptr, *emap = nullptr, *epre = nullptr;
  uint64_t n_starts = 0, n_ends = 0, n_words = 0;
};
inline SaView sa_view(const BwtOutputs &o) {
  SaView v;
  if (o.sa_c.p) {
    v.bmap = o.bmap.p; v.bpre = o.bpre.p; v.sa_c = o.sa_c.p;
    v.smap = o.smap.p; v.spre = o.spre.p; v.emap = o.emap.p; v.epre = o.epre.p;
    v.n_starts = o.n_starts; v.n_ends = o.n_ends; v.n_words = ((o.slice_n ? o.slice_n : o.n_out) + 63) / 64;
  } else v.dense = o.d_sa;
  return v;
}
// what merge_bwt is asked for: the window, the outputs (PFP_FLAG_*), the number of positions the slots must emit (0: not
// checked), and which part of the BWT this call emits into out.d_bwt[0..) / out.d_sa[0..)
struct MergeOpts {
  int w = 0, flags = 0;
  uint64_t expect_n_out = 0;
  uint64_t out_lo = 0, out_hi = ~0ull;          // positions [out_lo, out_hi) of the order's output are emitted
  uint64_t pos_base = 0, n_out_global = 0;      // global position of the order's first output; global n + 1 (0: what the order emits)
  // a whole suffix order, everything it emits
  static MergeOpts whole(int w, int flags, uint64_t expect_n_out) { MergeOpts o; o.w = w; o.flags = flags; o.expect_n_out = expect_n_out; return o; }
  // multi-GPU, replicated sort: a whole suffix order, positions [out_lo, out_hi) of it
  static MergeOpts slice(int w, int flags, uint64_t expect_n_out, uint64_t out_lo, uint64_t out_hi) {
    MergeOpts o = whole(w, flags, expect_n_out); o.out_lo = out_lo; o.out_hi = out_hi; return o;
  }
  // multi-GPU, sort sharded by key range: the held slots are one contiguous range of SA(D); all they emit, expect_n_out positions
  // that start at position pos_base of the n_out_global of the whole BWT
  static MergeOpts slot_range(int w, int flags, uint64_t expect_n_out, uint64_t pos_base, uint64_t n_out_global) {
    MergeOpts o = whole(w, flags, expect_n_out); o.pos_base = pos_base; o.n_out_global = n_out_global; return o;
  }
};
template <class I>
void merge_bwt(pfp_ctx *c, const Dictionary &D, const DictIndex &ix, const SuffixOrderT<I> &so, const ParseBWT &pb,
               const uint32_t *occ_lex, const MergeOpts &o, BwtOutputs &out);

// ---------------------------------------------------------------- 5-byte packing and run sampling of finished device outputs (runsample.hip)
void pack5_dev(pfp_ctx *c, const uint64_t *vals, uint64_t cnt, uint8_t *out5);
void unpack5_dev(pfp_ctx *c, const uint8_t *in5, uint64_t cnt, uint64_t *vals);
// pairs (pos,sa) packed as 10 bytes each; returns pair count; out buffer allocated inside
uint64_t sample_runs_dev(pfp_ctx *c, const uint8_t *bwt, const SaView &sa, uint64_t n_out, bool run_end,
                         DBuf<uint8_t> &out10);
// the same for a slice whose maps a merge left (multi-GPU): pairs of the run starts (ends) at slice position r as
// <pos_base + r, SA value>; drop_edge: the slice's first (last) position is NOT a run start (end) after all - its
// neighbour in the adjacent slice carries the same byte.  out10 == nullptr: count only.
uint64_t sample_runs_maps(pfp_ctx *c, const SaView &sa, uint64_t slice_n, bool run_end, bool drop_edge, uint64_t pos_base, uint8_t *out10);
// the same in two steps over a slice of the BWT (multi-GPU): count the boundaries, then place the pairs.
// left / right = the BWT byte just before / after the slice, -1 at the ends of the whole BWT.
struct RunSampler {
  pfp_ctx *c; const uint8_t *bwt; uint64_t cnt; int left, right; bool run_end;
  uint64_t ntile = 0, pairs = 0;
  DBuf<uint32_t> tile_cnt; DBuf<uint64_t> tile_off;
  RunSampler(pfp_ctx *c, const uint8_t *bwt, uint64_t cnt, int left, int right, bool run_end);   // counts (one sync)
  void place(const SaView &sa, uint64_t pos_base, uint8_t *out10);                                 // SA value i belongs to bwt[i]
};


// ---------------------------------------------------------------- inverting / checking a BWT (unbwt.hip)
// Device pointers.  out != NULL: write the text (n = n1 - 1 bytes) there; else text != NULL: compare with text_len bytes.
// sa5 / ssa10 / esa10 (each may be NULL): the files to check.  Not a BWT -> Error(PFP_EFORMAT).
struct BwtCheckArgs {
  const uint8_t *bwt = nullptr; uint64_t n1 = 0;
  uint8_t *out = nullptr;
  const uint8_t *text = nullptr; uint64_t text_len = 0;
  const uint8_t *sa5 = nullptr; uint64_t sa_bytes = 0;
  const uint8_t *ssa10 = nullptr; uint64_t ssa_bytes = 0;
  const uint8_t *esa10 = nullptr; uint64_t esa_bytes = 0;
};
void invert_bwt(pfp_ctx *c, const BwtCheckArgs &in, pfp_check_result *res);
// bitmap of the run starts (which = 0: j = 0 or BWT[j] != BWT[j-1]) or run ends (which = 1) of a BWT, with a popcount
// directory: dir[b] = set bits before row 512 b (cdiv(n1, 512) + 1 entries); bit_rank (devutil.hpp) reads them
struct RunIndex {
  DBuf<uint64_t> bits, dir;
  uint64_t runs = 0;
  void build(pfp_ctx *c, const uint8_t *bwt, uint64_t n1, int which);
};

// ---------------------------------------------------------------- searching a BWT (fmsearch.hip)
// Count and locate over a .bwt and its run samples (the r-index of Gagie, Navarro and Prezza); see fmsearch.hip and pfpgpu.h.
// Everything the searches read is owned here (the build copies what it needs from the caller's buffers).
struct FmIndex {
  pfp_ctx *c = nullptr;
  uint64_t n1 = 0, runs = 0;
  int sigma = 0;                         // distinct bytes other than 0 (dense codes 0..sigma-1 in byte order)
  bool wide = false, samples = false;    // wide: rows and SA values as u64 (else u32)
  DBuf<uint8_t> bwt;                     // the BWT, zero-padded to whole 256-row blocks (one block more than n1 >> 8)
  DBuf<uint8_t> codes;                   // [256] byte -> code (0xFF: absent, and byte 0), [256 + k] code -> byte
  DBuf<uint16_t> blk;                    // [block * sigma + k] occurrences of code k in the blocks of its superblock before it
  DBuf<uint64_t> sbc;                    // [superblock * sigma + k] C[byte] + occurrences before the superblock
  RunIndex rs;                           // run starts (samples only)
  DBuf<uint8_t> rs_row, rs_sa;           // [runs] of I: row and SA value of run start i
  DBuf<uint8_t> phi_key, phi_val, phi_dir;  // [runs - 1] of I: SA[e_i] sorted, SA[s_{i+1}]; [nbk + 1] first key of each bucket
  uint64_t nphi = 0, nbk = 0;
  int shift = 0;                         // bucket of text position x: x >> shift
  bool has_text = false;                 // built by fm_build_ms: the two arrays below exist (matching statistics read them)
  DBuf<uint8_t> text;                    // the text, n1 - 1 bytes and 16 bytes of zero padding (whole 16-byte loads stay in bounds)
  DBuf<uint8_t> re_sa;                   // [runs] of I: SA value of run end i
  uint64_t ms_stats[3] = {0, 0, 0};      // fm_ms launches; with PFP_FM_MS_STATS=1 also steps that jumped and bytes their LCEs matched
  uint64_t fill_stats[14] = {};          // with PFP_FM_MS_STATS=1 (fmfill.hip): gaps, trivial ones, then per width gaps that went through a pass and their cells
  uint64_t apx_stats[3] = {0, 0, 0};     // fm_approx launches and hits filled; with PFP_FM_MS_STATS=1 also (in [1]) LF pairs
  bool has_thr = false;                  // fm_lcp (keep) or fm_load_thresholds filled the array below
  DBuf<uint8_t> thr;                     // [runs] of I: the threshold row of run k (lcp.hip)
  uint64_t nseq = 0;                     // sequences of the collection (seqmap.hip); 0: no table was set
  DBuf<uint8_t> seq_start;               // [nseq + 1] of I: first text position of sequence k; seq_start[nseq] = n
  DBuf<uint32_t> seq_dir;                // [seq_nbk + 1] first k with seq_start[k] >= b << seq_shift (about one start per bucket)
  uint64_t seq_nbk = 0;
  int seq_shift = 0;
  uint64_t device_bytes() const;
};
uint64_t fm_bwt_bytes(uint64_t n1);      // f.bwt's size: n1 bytes and the zero padding
// bwt == f.bwt.p (filled with n1 bytes, fm_bwt_bytes(n1) allocated): the index adopts it instead of copying
void fm_build(pfp_ctx *c, FmIndex &f, const uint8_t *bwt, uint64_t n1, const uint8_t *ssa10, uint64_t ssa_bytes, const uint8_t *esa10,
              uint64_t esa_bytes);
// the same (samples required) plus what matching statistics need: the SA value of every run end and the text.  text == NULL:
// inverted from the BWT (invert_bwt: not one LF cycle -> PFP_EFORMAT); text == f.text.p (n1 + 15 bytes allocated): adopted
void fm_build_ms(pfp_ctx *c, FmIndex &f, const uint8_t *bwt, uint64_t n1, const uint8_t *ssa10, uint64_t ssa_bytes, const uint8_t *esa10,
                 uint64_t esa_bytes, const uint8_t *text);
// matching statistics (PHONI; pfpgpu.h states the definitions): len / pos run parallel to pat, pos may be NULL
void fm_ms(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos);
// maximal exact matches from fm_ms's outputs: mem_off[0..npat] exclusive sums of the counts; mem == NULL: only those
void fm_mems(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint32_t *len, const uint64_t *pos, uint64_t min_len,
             uint64_t *mem_off, uint64_t *mem);
// the triples alone, at offsets a call above gave for the same patterns
void fm_mem_triples(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint32_t *len, const uint64_t *pos, uint64_t min_len,
                    const uint64_t *mem_off, uint64_t *mem);
// the LCP array and thresholds of an index with text (lcp.hip; pfpgpu.h states the definitions).  Device outputs, each may be
// NULL: lcp64 n1 values, thr64 runs values, lcp5 / thr5 the same as 5-byte ints; keep: the index keeps the thresholds (fm_ms_thr)
struct LcpOut {
  uint64_t *lcp64 = nullptr, *thr64 = nullptr;
  uint8_t *lcp5 = nullptr, *thr5 = nullptr;
  bool keep = false;
};
void fm_lcp(FmIndex &f, const LcpOut &o);
// thresholds from a .thr_pos image (5 bytes per run; another size -> PFP_EFORMAT)
void fm_load_thresholds(FmIndex &f, const uint8_t *thr5, uint64_t bytes);
// matching statistics in two passes with thresholds: fm_ms's arguments and lengths; an index without thresholds -> PFP_EINVAL
void fm_ms_thr(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos);
// lcp[j] = plcp[SA[j]] for every row j through the inverter's splitter walk (unbwt.hip): plcp in text order, n1 entries each
template <class I> void lcp_by_rows(pfp_ctx *c, const uint8_t *bwt, uint64_t n1, const I *plcp, I *lcp);
// device pointers; first may be NULL (needs samples otherwise)
void fm_count(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t *sp, uint64_t *ep, uint64_t *first);
// the same kernel over strings that lie anywhere in pat: string j is pat[begin[j] .. end[j]) (end == NULL: begin[j + 1])
void fm_count_spans(FmIndex &f, const uint8_t *pat, const uint64_t *begin, const uint64_t *end, uint64_t npat, uint64_t *sp, uint64_t *ep,
                    uint64_t *first);
// out_off[0..npat] (device): exclusive sums of min(ep - sp, max_occ); pos == NULL: only those
void fm_locate(FmIndex &f, uint64_t npat, const uint64_t *sp, const uint64_t *ep, const uint64_t *first, uint64_t max_occ,
               uint64_t *out_off, uint64_t *pos);
// the sequences of a collection (seqmap.hip; pfpgpu.h states the definitions).  starts: nseq + 1 host values; replaces a table
// set before.  The calls below need a table (PFP_EINVAL otherwise)
void fm_set_seqs(FmIndex &f, const uint64_t *starts, uint64_t nseq);
// seq[i] (u32) / off[i] (u64) of pos[i]; either output may be NULL
void fm_seqmap(FmIndex &f, const uint64_t *pos, uint64_t count, uint32_t *seq, uint64_t *off);
// fm_locate's positions that lie inside one sequence, in row order: out_off[0..npat] exclusive sums of the kept counts; seq / off
// (room for the unfiltered total, both or neither) get the kept hits
void fm_locate_seqs(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint64_t *sp, const uint64_t *ep, const uint64_t *first,
                    uint64_t max_occ, uint64_t *out_off, uint32_t *seq, uint64_t *off);
// per pattern the distinct sequences of its kept hits, ascending, with their numbers of hits: doc_off[0..npat], and doc / cnt in the
// caller's device buffers (both NULL: the offsets only) or, where own_doc / own_cnt are given, in buffers allocated once the total is
// known (a caller that cannot size them without listing twice)
struct DocOut {
  uint32_t *doc = nullptr; uint64_t *cnt = nullptr;
  DBuf<uint32_t> *own_doc = nullptr; DBuf<uint64_t> *own_cnt = nullptr;
};
void fm_doclist(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint64_t *sp, const uint64_t *ep, const uint64_t *first,
                uint64_t *doc_off, DocOut &o);
// k-mismatch search (fmapprox.hip; pfpgpu.h, "Approximate search", states the definitions).  Device pointers.  k outside 0 ..
// PFP_FM_APPROX_MAX_K, or a toehold asked of an index without samples -> PFP_EINVAL
void fm_approx_check(const FmIndex &f, int k, bool toehold);
// cnt[p] = hits of pattern p, cnt[npat] = 0 (npat + 1 entries)
void fm_approx_count(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, uint64_t *cnt);
// the H = hit_off[npat] hits, pattern p's at hit_off[p] .. hit_off[p+1] by increasing sp (hit_off: the exclusive sums of
// fm_approx_count's counts); first may be NULL
void fm_approx_fill(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, const uint64_t *hit_off, uint64_t H,
                    uint64_t *sp, uint64_t *ep, uint64_t *first, uint8_t *dist);
// both: hit_off[0..npat] is written; sp == NULL: only that
void fm_approx(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, uint64_t *hit_off, uint64_t *sp, uint64_t *ep,
               uint64_t *first, uint8_t *dist);
// locating fm_approx_fill's hits, at most max_occ rows per pattern (0: all): cep[h] = hit h's ep clipped to the rows its pattern
// keeps (allocated here), out_off[0..npat] the exclusive sums of the positions per pattern
void fm_approx_clip(FmIndex &f, uint64_t npat, const uint64_t *hit_off, uint64_t H, const uint64_t *sp, const uint64_t *ep, const uint64_t *first,
                    uint64_t max_occ, uint64_t *out_off, DBuf<uint64_t> &cep);
// the positions of H hits (a whole call's, or those of consecutive patterns) in hit order, rows in row order, each with its hit's
// distance; pos / pdist are allocated here once their number, which is returned, is known
uint64_t fm_approx_positions(FmIndex &f, uint64_t H, const uint64_t *sp, const uint64_t *cep, const uint64_t *first, const uint8_t *dist,
                             DBuf<uint64_t> &pos, DBuf<uint8_t> &pdist);

// extending seeds (fmextend.hip; pfpgpu.h, "Extending seeds", states the definitions).  Device pointers.  k outside 0 ..
// PFP_FM_EXTEND_MAX_K or an index without text -> PFP_EINVAL; a pattern longer than PFP_FM_EXTEND_MAX_M -> PFP_ELIMIT
void fm_extend_check(const FmIndex &f, int k);
// fm_extend_check, then what seeding asks: min_seed = 0, or thresholds wanted of an index without them -> PFP_EINVAL
void fm_align_check(const FmIndex &f, int k, uint64_t min_seed, bool thresholds);
// candidate i = (cand_pat[i], cand_diag[i]) -> (dist[i], start[i], end[i]); 0xFF and UINT64_MAX twice where nothing aligns
void fm_extend(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat, const int64_t *cand_diag,
               uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end);
// a pattern of the call longer than PFP_FM_EXTEND_MAX_M -> PFP_ELIMIT (one pass over the offsets, one scalar read back)
void fm_extend_check_patterns(FmIndex &f, const uint64_t *pat_off, uint64_t npat);
// what fm_align_seeds leaves for fm_align_write: the C candidates' sorted keys, the flags of the kept ones and their exclusive sums
struct AlnKeys {
  DBuf<uint64_t> skey, flag, idx;
  uint64_t C = 0, total = 0;               // total: the alignments kept, which is what the outputs must hold
};
// the alignments of every pattern from its matching statistics (len / pos as fm_ms or fm_ms_thr gave them) and its MEM offsets
// (mem_off[0..npat] as fm_mems gave them for the same patterns, M = mem_off[npat]): aln_off[0..npat] the exclusive sums of their
// numbers, at most max_aln per pattern (0: all).  The callers have checked the patterns' lengths (fm_extend_check_patterns)
void fm_align_seeds(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln,
                    const uint32_t *len, const uint64_t *pos, const uint64_t *mem_off, uint64_t M, uint64_t *aln_off, AlnKeys &out);
// the kept alignments, each pattern's ordered by (d, start, end): room for keys.total entries each
void fm_align_write(FmIndex &f, const AlnKeys &keys, uint64_t *start, uint64_t *end, uint8_t *dist);
// matching statistics (thresholds: by fm_ms_thr), MEMs and fm_align_seeds: the checks of fm_align and everything but the writing
void fm_align_keys(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln, bool thresholds,
                   uint64_t *aln_off, AlnKeys &keys);
// fm_align_keys and, where start is given, fm_align_write
void fm_align(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln, bool thresholds,
              uint64_t *aln_off, uint64_t *start, uint64_t *end, uint8_t *dist);

// aligning in a window (fmwindow.hip; pfpgpu.h, "Aligning in a window", states the definitions).  Device pointers; the checks are
// fm_extend's, and a window lo <= hi <= n of more than PFP_FM_WINDOW_MAX_W bytes -> PFP_ELIMIT.
// candidate i = (cand_pat[i], lo[i], hi[i]) -> (dist[i], start[i], end[i]); 0xFF and UINT64_MAX twice where nothing aligns
void fm_window(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat, const uint64_t *lo,
               const uint64_t *hi, uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end);

// edit scripts (fmcigar.hip; pfpgpu.h, "Edit scripts", states the definitions).  Device pointers; the checks are fm_extend's.
// what fm_cigar_runs leaves for fm_cigar_write: every alignment's runs, last first, in a slot of S = 2k + 1 words
struct CigRuns {
  DBuf<uint32_t> slot;
  uint64_t naln = 0, S = 0, total = 0;     // total: the runs of all alignments, which is what the output must hold
};
// alignment i = (aln_pat[i], start[i], end[i]) -> dist[i] (0xFF: no script) and cig_off[0..naln], the exclusive sums of the run counts
void fm_cigar_runs(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *aln_pat, const uint64_t *start,
                   const uint64_t *end, uint64_t naln, int k, uint8_t *dist, uint64_t *cig_off, CigRuns &out);
// the runs in order, alignment i's at cig_off[i] .. cig_off[i + 1]: room for runs.total entries
void fm_cigar_write(FmIndex &f, const CigRuns &runs, const uint64_t *cig_off, uint32_t *cig);
// fm_cigar_runs and, where cig is given, fm_cigar_write
void fm_cigar(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *aln_pat, const uint64_t *start,
              const uint64_t *end, uint64_t naln, int k, uint8_t *dist, uint64_t *cig_off, uint32_t *cig);

// mapping reads (fmmap.hip; pfpgpu.h, "Mapping reads", states the definitions).  Device pointers.  An index without text or
// without a sequence table -> PFP_EINVAL
void fm_map_check(const FmIndex &f, int k, uint64_t min_seed, bool thresholds);
// the 2 npat patterns of a call's reads: pattern 2p = read p, 2p + 1 = its reverse complement; off holds 2 npat + 1 offsets into
// pat, which has 16 bytes of padding behind the last pattern
struct MapReads {
  DBuf<uint8_t> pat;
  DBuf<uint64_t> off;
};
// (any_length: reads that go through no band - fmchain.hip - skip fm_extend_check_patterns)
void fm_map_strands(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, MapReads &out, bool any_length = false);
// the candidates of some patterns, as fm_align gives them: aln_off (one entry more than the patterns) and the A = aln_off[last]
// triples start / end / dist.  The triples serve fm_map_select alone: its callers drop them before they fill or pair
struct MapCands {
  DBuf<uint64_t> aln_off, start, end;
  DBuf<uint8_t> dist;
  uint64_t A = 0;
  void drop_triples() { start.release(); end.release(); dist.release(); }
};
// the candidates of npat2 patterns, every alignment kept: fm_align_keys, then the triples, then a wait (the keys are gone after it)
void fm_map_cands(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t npat2, uint64_t min_seed, int k, bool thresholds, MapCands &out);
// the same from what fm_align_seeds takes (a group of a call whose matching statistics stand, and the group's MEM offsets).
// held: the caller keeps the keys and waits for the stream itself before they go
void fm_map_cands_ms(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln,
                     const uint32_t *len, const uint64_t *pos, const uint64_t *mem_off, uint64_t M, MapCands &out, AlnKeys *held = nullptr);
// what fm_map_select leaves for fm_map_fill: the candidates' keys (d, strand, s, e - s), sorted inside every read's segment with
// the hits first, and the number of hits returned
struct MapSel {
  DBuf<uint64_t> key;
  uint64_t H = 0;
};
// from the candidates of the 2 npat patterns: inside, shadowing, order and cap -> hit_off[0 .. npat], mapq[npat], nhits[npat]
void fm_map_select(FmIndex &f, const uint64_t *pat2_off, uint64_t npat, int k, uint64_t max_sec, const MapCands &cd, uint64_t *hit_off, uint8_t *mapq,
                   uint64_t *nhits, MapSel &sel);
// the sel.H returned hits: strand, seq, off, start, dist (room for sel.H each), cig_off / md_off (sel.H + 1 each); cig and md are
// allocated here once their sizes are known
void fm_map_fill(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t npat, int k, const uint64_t *aln_off, const uint64_t *hit_off,
                 const MapSel &sel, uint8_t *strand, uint32_t *seq, uint64_t *off, uint64_t *start, uint8_t *dist, uint64_t *cig_off,
                 DBuf<uint32_t> &cig, uint64_t *md_off, DBuf<uint8_t> &md);
// the part of fm_map_fill that works from an explicit list: the scripts and the MD strings of the H alignments (aln_pat[h] among
// the npat2 patterns of pat2, start[h], end[h]); cig_off / md_off (H + 1 each), cig and md are allocated here.  An entry that is
// no alignment (aln_pat[h] >= npat2) gets no runs and an empty MD
void fm_map_scripts(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t npat2, int k, const uint32_t *aln_pat, const uint64_t *start,
                    const uint64_t *end, uint64_t H, uint64_t *cig_off, DBuf<uint32_t> &cig, uint64_t *md_off, DBuf<uint8_t> &md);
// all of it over device patterns: fm_map_strands, fm_map_cands, fm_map_select and, where strand is given, fm_map_fill
void fm_map(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_sec, bool thresholds,
            uint64_t *hit_off, uint8_t *mapq, uint64_t *nhits, uint8_t *strand, uint32_t *seq, uint64_t *off, uint64_t *start, uint8_t *dist,
            uint64_t *cig_off, DBuf<uint32_t> &cig, uint64_t *md_off, DBuf<uint8_t> &md);

// chaining anchors (fmchain.hip; pfpgpu.h, "Chaining anchors", states the definitions).  Device pointers.  An index without text
// or samples, min_seed = 0, max_occ outside 1 .. 65536, thresholds wanted of an index without them -> PFP_EINVAL
void fm_anchors_check(const FmIndex &f, uint64_t min_seed, uint64_t max_occ, bool thresholds);
// the anchors of npat patterns whose matching statistics stand (len / pos as fm_ms or fm_ms_thr gave them; mem_off[0..npat] as
// fm_mems gave them for the same patterns, counted from the first, M = mem_off[npat]): anc_off[0..npat] and, sized here, the
// triples; skipped (npat, may be NULL).  2^32 - 1 or more occurrences -> PFP_ELIMIT.  Returns the number of anchors
uint64_t fm_anchors_ms(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                       const uint32_t *len, const uint64_t *pos, const uint64_t *mem_off, uint64_t M, uint64_t *anc_off, DBuf<uint64_t> &anc,
                       uint32_t *skipped);
// matching statistics (thresholds: by fm_ms_thr), MEMs and fm_anchors_ms
uint64_t fm_anchors(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ, bool thresholds,
                    uint64_t *anc_off, DBuf<uint64_t> &anc, uint32_t *skipped);
// G or B outside 1 .. 2^31 - 1, S = 0 -> PFP_EINVAL
void fm_chain_check(const FmIndex &f, uint64_t max_gap, uint64_t band, uint64_t min_score);
// what fm_chains_run leaves for fm_chains_write: per anchor that ends a kept chain its fields, and the kept chains' end anchors
// in the order of output inside every pattern's segment
struct ChainSel {
  DBuf<uint32_t> score, n, qs, match, order, sb;
  DBuf<uint8_t> par;        // how many anchors back every anchor's parent lies (fmfill.hip walks a chain's members along them)
  DBuf<uint64_t> ts;
  uint64_t total = 0;
};
// the programme and the peel over npat patterns' anchors (anc_off as the caller gave it: offsets that decrease, anchors out of
// order, len = 0 or i + len >= 2^32 -> PFP_EINVAL): chain_off[0..npat], at most max_chains per pattern (0: all)
void fm_chains_run(FmIndex &f, const uint64_t *anc_off, const uint64_t *anc, uint64_t npat, uint64_t max_gap, uint64_t band, uint64_t min_score,
                   uint64_t max_chains, uint64_t *chain_off, ChainSel &sel);
struct ChainOut {
  uint32_t *score, *n, *qs, *qe;
  uint64_t *ts, *te;
  uint32_t *match;
};
void fm_chains_write(FmIndex &f, const uint64_t *anc, uint64_t npat, const uint64_t *chain_off, const ChainSel &sel, const ChainOut &out);
// what fm_map_long_select leaves for fm_map_long_fill: both strands' patterns, their chains and the reads' order of them
struct LongSel {
  MapReads rd;
  ChainSel cs;              // keep: what the programme and the peel left stays here (fm_map_long_align reads it), else it goes at once
  bool keep = false;
  DBuf<uint64_t> chain_off, ts, te;
  DBuf<uint32_t> score, n, qs, qe, match, order;
  uint64_t H = 0;
};
struct LongOut {
  uint8_t *strand;
  uint32_t *seq;
  uint64_t *off, *ts, *te;
  uint32_t *qs, *qe, *score, *n, *match;
};
// the chains of npat reads from their 2 npat strands' anchors (anc_off2, anc; pat2_off = fm_map_strands' offsets, moved into
// sel.rd by the caller or given): hit_off[0..npat], mapq and nchains
void fm_map_long_select(FmIndex &f, const uint64_t *anc_off2, const uint64_t *anc, uint64_t npat, uint64_t max_gap, uint64_t band,
                        uint64_t min_score, uint64_t max_sec, uint64_t *hit_off, uint8_t *mapq, uint64_t *nchains, LongSel &sel);
void fm_map_long_fill(FmIndex &f, const uint64_t *pat2_off, uint64_t npat, const uint64_t *hit_off, const LongSel &sel, const LongOut &out);
struct LongAln;     // (below, with fmfill.hip's)
// all of it over device patterns; out == NULL: hit_off, mapq and nchains only.  aln: the scripts of the returned chains as well
void fm_map_long(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ, uint64_t max_gap,
                 uint64_t band, uint64_t min_score, uint64_t max_sec, bool thresholds, uint64_t *hit_off, uint8_t *mapq, uint64_t *nchains,
                 const LongOut *out, const LongAln *aln = nullptr);
// aligning chains (fmfill.hip; pfpgpu.h, "Aligning chains", states the definitions).  Device pointers.  max_fill above
// PFP_FM_FILL_MAX_F or an index without text -> PFP_EINVAL
void fm_fill_check(const FmIndex &f, uint64_t max_fill);
// device pattern offsets that decrease -> PFP_EINVAL
void fm_fill_check_patterns(FmIndex &f, const uint64_t *pat_off, uint64_t npat);
// segment g = (pat[g], q0[g], q1[g], t0[g], t1[g])
struct FillSegs {
  const uint32_t *pat;
  const uint64_t *q0, *q1, *t0, *t1;
};
// what the gap passes leave for the passes that place runs: per gap its number of runs and where they wait, last first (0: none
// are stored - a trivial gap's one run is derived); pool holds them until this goes
struct FillRuns {
  DBuf<uint64_t> cnt, rptr;
  std::vector<DBuf<uint32_t>> pool;
  uint64_t total = 0;       // the runs of all segments (fm_fill_runs)
};
// the gap passes alone: dist[g] (0xFFFFFFFF: no script) and out
void fm_fill_gaps(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const FillSegs &sg, uint64_t ngap, uint64_t max_fill,
                  uint32_t *dist, FillRuns &out);
// pattern offsets that decrease -> PFP_EINVAL; dist and cig_off[0..nseg], the exclusive sums of the run counts
void fm_fill_runs(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const FillSegs &sg, uint64_t nseg, uint64_t max_fill,
                  uint32_t *dist, uint64_t *cig_off, FillRuns &out);
// the runs in order, segment g's at cig_off[g] .. cig_off[g + 1]: room for runs.total entries
void fm_fill_write(FmIndex &f, const FillSegs &sg, uint64_t nseg, const uint32_t *dist, const FillRuns &runs, const uint64_t *cig_off, uint32_t *cig);
// fm_fill_runs and, where cig is given, fm_fill_write
void fm_fill(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const FillSegs &sg, uint64_t nseg, uint64_t max_fill,
             uint32_t *dist, uint64_t *cig_off, uint32_t *cig);
// what fm_chain_align_runs leaves for fm_chain_align_write (and for a caller that wants the members): the aligned chains' members
// (mem_off, mem: indices inside the pattern's anchors), and per member its gap (seg_pat, seg64 = q0, q1, t0, t1, dist, runs) and
// the bytes its trimmed anchor keeps
struct ChainAln {
  uint64_t nal = 0, M = 0, total = 0;      // total: the runs of all scripts, which is what the output must hold
  DBuf<uint64_t> mem_off, seg64;
  DBuf<uint32_t> mem, seg_pat, keep, dist;
  FillRuns runs;
};
struct AlnOut {
  uint32_t *aqs = nullptr;
  uint64_t *ats = nullptr;
  uint32_t *nm = nullptr, *unfilled = nullptr;
};
// the scripts of nal chains of those fm_chains_run left in cs (chain_off: its offsets): chain list[k] (NULL: k), k < nal.  out gets
// nal entries each, cig_off[0..nal] the exclusive sums of the run counts.  turn: the patterns are the strands of reads
// (fm_map_strands) and aqs of an odd pattern is turned into the read as given
void fm_chain_align_runs(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint64_t *anc_off, const uint64_t *anc,
                         const uint64_t *chain_off, const ChainSel &cs, const uint32_t *list, uint64_t nal, uint64_t max_fill, bool turn,
                         const AlnOut &out, uint64_t *cig_off, ChainAln &st);
void fm_chain_align_write(FmIndex &f, const ChainAln &st, const uint64_t *cig_off, uint32_t *cig);
// the scripts of the sel.H chains that fm_map_long_select returns (sel.keep was set): out and cig_off as above, H entries
void fm_map_long_align(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t npat, const uint64_t *anc_off2, const uint64_t *anc,
                       const uint64_t *hit_off, const LongSel &sel, uint64_t max_fill, const AlnOut &out, uint64_t *cig_off, ChainAln &st);
// what pfp_fm_map_long_aln adds to fm_map_long: out and cig_off get hit_off[npat] (+ 1) entries; cig NULL: those only
struct LongAln {
  uint64_t max_fill;
  AlnOut out;
  uint64_t *cig_off;
  uint32_t *cig;
};
// mapping read pairs (fmpair.hip; pfpgpu.h, "Mapping read pairs", states the definitions).  Device pointers.  fm_map_check's
// errors; an odd number of reads, min_ins > max_ins, max_ins > PFP_FM_WINDOW_MAX_W or anchors outside 1 ..
// PFP_FM_PAIR_MAX_ANCHORS -> PFP_EINVAL
void fm_pair_check(const FmIndex &f, uint64_t npat, int k, uint64_t min_seed, bool thresholds, uint64_t min_ins, uint64_t max_ins, uint64_t anchors);
// where a call's results go: proper and npairs per pair (nread / 2), the rest per read (nread; cig_off and md_off nread + 1)
struct PairOut {
  uint8_t *proper; uint64_t *npairs;
  uint8_t *mapped, *rescued, *mapq, *strand; uint32_t *seq; uint64_t *off, *start; uint8_t *dist; int64_t *tlen;
  uint64_t *cig_off, *md_off;
};
// from the hits of the nread reads as fm_map_select left them with max_sec = C - 1 (aln_off, hit_off, smapq = the single-end MAPQ,
// sel; pat2 / pat2_off = fm_map_strands' 2 nread patterns): need, rescue, reduce and the scripts; cig and md are allocated here
void fm_pair(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t nread, int k, uint64_t min_ins, uint64_t max_ins, uint64_t C,
             const uint64_t *aln_off, const uint64_t *hit_off, const uint8_t *smapq, const MapSel &sel, const PairOut &out, DBuf<uint32_t> &cig,
             DBuf<uint8_t> &md);
// all of it over device patterns: fm_pair_check, fm_map_strands, fm_map_cands, fm_map_select and fm_pair; nhits[npat]
void fm_map_pairs(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, bool thresholds, uint64_t min_ins,
                  uint64_t max_ins, uint64_t anchors, uint64_t *nhits, const PairOut &out, DBuf<uint32_t> &cig, DBuf<uint8_t> &md);

// ---------------------------------------------------------------- PFP_DEBUG=1 (validate.hip)
void validate_scan(pfp_ctx *c, const DBuf<uint64_t> &ends, uint64_t n_ends, uint64_t n, int w);
void validate_dictionary(pfp_ctx *c, const Dictionary &D, int w);
void validate_index(pfp_ctx *c, const Dictionary &D, const DictIndex &ix);
template <class I> void validate_suffix_order(pfp_ctx *c, const uint8_t *bytes, SuffixOrderT<I> &so, bool dict_mode, const char *what);
void validate_int_sa(pfp_ctx *c, const uint32_t *sym, const SuffixOrder &so);
void validate_lexrank(pfp_ctx *c, const Dictionary &D, const DictIndex &ix);
void validate_parse_bwt(pfp_ctx *c, const ParseBWT &pb);

}  // namespace pfp
