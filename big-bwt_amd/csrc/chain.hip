// chain.hip -- the fused parse -> SA -> BWT chain: every intermediate stays in HBM (bigbwt:69-156: newscan -> bwtparse -> pfbwt).
// The pfp_bigbwt* family over host buffers, device pointers and files, and the output formats of device-resident results.
#include "chain.hpp"

using namespace pfp;

namespace pfp {

// occ in lexicographic order and the parse as 1-based lexicographic ranks (newscan.cpp:436,456)
__global__ void occ_lex_kernel(uint32_t d, const uint32_t *__restrict__ lexrank, const uint32_t *__restrict__ wocc,
                               uint32_t *__restrict__ occ_lex, uint32_t *__restrict__ word_at_rank) {
  uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j >= d) return;
  uint32_t r = lexrank[j];
  occ_lex[r] = wocc[j];
  if (word_at_rank) word_at_rank[r] = j;
}
__global__ void parse_sym_kernel(uint64_t P, const uint32_t *__restrict__ pid, const uint32_t *__restrict__ lexrank,
                                 uint32_t *__restrict__ sym) {
  uint64_t k = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (k < P) sym[k] = lexrank[pid[k]] + 1;
}
// .dict in lexicographic order (newscan.cpp:406-438): 8 lanes per word, 16-byte pieces
__global__ __launch_bounds__(256) void dict_permute_kernel(uint32_t d, const uint32_t *__restrict__ word_at_rank,
                                                           const uint64_t *__restrict__ woff,
                                                           const uint32_t *__restrict__ wlen,
                                                           const uint8_t *__restrict__ src,
                                                           const uint64_t *__restrict__ doff, uint8_t *__restrict__ dst) {
  uint64_t t = (uint64_t)BID * 256 + threadIdx.x;
  uint64_t r = t >> 3;
  int l8 = (int)(t & 7);
  if (r >= d) return;
  uint32_t j = word_at_rank[r];
  uint64_t len = (uint64_t)wlen[j] + 1;   // with terminator
  const uint8_t *s = src + woff[j];
  uint8_t *o = dst + doff[r];
  for (uint64_t off = (uint64_t)l8 * 16; off < len; off += 128) {
    if (off + 16 <= len) st16u(o + off, ld16u(s + off));
    else for (uint64_t b = off; b < len; b++) o[b] = s[b];
  }
}
void occ_in_lex_order(pfp_ctx *c, uint32_t d, const uint32_t *lexrank, const uint32_t *wocc, uint32_t *occ_lex, uint32_t *word_at_rank) {
  hipLaunchKernelGGL(occ_lex_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, lexrank, wocc, occ_lex, word_at_rank);
}
void permute_dictionary(pfp_ctx *c, uint32_t d, const uint32_t *order, const uint64_t *woff, const uint32_t *wlen, const uint8_t *src,
                        const uint64_t *doff, uint8_t *dst) {
  hipLaunchKernelGGL(dict_permute_kernel, gdim(cdiv((uint64_t)d * 8, TB)), gdim(TB), 0, c->stream, d, order, woff, wlen, src, doff, dst);
}

void run_parse(pfp_ctx *c, Chain &ch, uint64_t n, int w, uint64_t p, bool want_sai, bool exact_reference_parse, bool dense_sa) {
  pfp_stats &st = c->stats;
  {
    PhaseTimer t(c, &st.ms_scan);
    uint32_t n_extra = 0;
    // the staged entry points parse exactly as the reference does (newscan.cpp:168-202, 363-377); the fused chain cuts by
    // its own window hash (pfp_set_window_hash) and splits giant phrases with extra triggers (pfp_set_max_phrase)
    st.parse_density = 1.0;
    if (exact_reference_parse || (!c->max_phrase && !c->fast_triggers)) ch.n_ends = scan_text(c, ch.tx, n, w, p, ch.ends, &ch.n_used);
    else ch.n_ends = scan_text_adaptive(c, ch.tx, n, w, p, c->max_phrase, ch.ends, &ch.n_used, &n_extra);
    st.extra_triggers = n_extra;
    if (c->debug) validate_scan(c, ch.ends, ch.n_ends, ch.n_used, w);
  }
  {
    PhaseTimer t(c, &st.ms_phrases);
    build_dictionary(c, ch.tx, ch.n_used, w, ch.ends, ch.n_ends, want_sai, ch.D);
    if (c->debug) validate_dictionary(c, ch.D, w);
    build_dict_index(c, ch.D, ch.ix);
    if (c->debug) validate_index(c, ch.D, ch.ix);
    // the text and its phrase ends have done their part: dictionary, parse, last and sai are all there is from here on
    ch.tx.buf.release();
    ch.ends.release();
  }
  {
    PhaseTimer t(c, &st.ms_sa_dict);
    // BWT only: the merge records ride in the spare bits of the first-round keys (SuffixOrder::paybits)
    const WordView wv = word_view(ch.D, ch.ix);
    const SlotPayloadSrc pay{wv, ch.D.wocc.p, w};
    ch.ord.wide = prefer_wide_index(c, ch.D.dsize);      // 32- or 64-bit dictionary positions (bigbwt:130-151)
    with_width(ch.ord.wide, [&](auto tag) {
      using I = decltype(tag);
      auto &so = ch.ord.get<I>();
      so.rep_hint = (double)ch.n_used / (double)std::max<uint64_t>(ch.D.dsize, 1);
      // (w: the suffixes of at most w bytes emit nothing - they are not sorted, so.N < dsize, and every slot number from
      //  here on - lexrank's, ix.wslot_lex, the merge's - counts the sorted ones alone)
      sort_dict_suffixes<I>(c, ch.D.bytes.p, ch.D.dsize, wv, so, dense_sa ? nullptr : &pay, w);
      if (c->debug) validate_suffix_order<I>(c, ch.D.bytes.p, so, true, "dict SA");
      compute_lexrank<I>(c, ch.D, so, ch.ix);
      if (!c->debug) { so.rank.release(); so.tab.release(); }      // the merge reads sa / grp / skeys only
    });
    if (c->debug) validate_lexrank(c, ch.D, ch.ix);
    const uint32_t d = (uint32_t)ch.D.d;
    ch.occ_lex.alloc(c, d); ch.word_at_rank.alloc(c, d);
    occ_in_lex_order(c, d, ch.ix.lexrank.p, ch.D.wocc.p, ch.occ_lex.p, ch.word_at_rank.p);
    ch.sym.alloc(c, ch.D.P);
    hipLaunchKernelGGL(parse_sym_kernel, gdim(cdiv(ch.D.P, TB)), gdim(TB), 0, c->stream, ch.D.P, ch.D.pid.p,
                       ch.ix.lexrank.p, ch.sym.p);
    PFP_HIP(hipGetLastError());
  }
  st.n = ch.n_used; st.n_phrases = ch.D.P; st.n_words = ch.D.d; st.dict_size = ch.D.dsize;
  st.sa_rounds_dict = ch.ord.rounds(); st.hash_reseeds = ch.D.reseeds; st.index_bits = ch.ord.wide ? 64 : 32;
}

// d_sa == nullptr with SA flags: the SA values live in buffers of the chain, allocated when the suffix sorter has
// given its scratch back - all of them for -S (ch.sa_own), those at the run boundaries of the BWT for -s / -e
// (ch.out.sa_c); the caller never sees them, only what is sampled / packed from them
static void run_chain_dev(pfp_ctx *c, Chain &ch, uint64_t n, int w, uint64_t p, int flags, uint8_t *d_bwt,
                          uint64_t *d_sa, uint64_t *n_used) {
  pfp_stats &st = c->stats;
  st = pfp_stats{};
  auto t0 = std::chrono::steady_clock::now();
  run_parse(c, ch, n, w, p, flags != 0, false, (flags & PFP_FLAG_SA) != 0);
  {
    PhaseTimer t(c, &st.ms_sa_parse);
    parse_bwt(c, ch.sym.p, ch.D.P, ch.D.last.p, flags ? ch.D.sai.p : nullptr, ch.occ_lex.p, ch.D.d, ch.pb);
    st.sa_rounds_parse = ch.pb.rounds;
    if (c->debug) validate_parse_bwt(c, ch.pb);
  }
  {
    PhaseTimer t(c, &st.ms_merge);
    BwtOutputs &bo = ch.out;
    if ((flags & PFP_FLAG_SA) && !d_sa) { ch.sa_own.alloc(c, ch.n_used + 1); d_sa = ch.sa_own.p; }
    bo.d_bwt = d_bwt; bo.d_sa = d_sa;
    with_width(ch.ord.wide, [&](auto tag) {
      using I = decltype(tag);
      merge_bwt<I>(c, ch.D, ch.ix, ch.ord.get<I>(), ch.pb, ch.occ_lex.p, MergeOpts::whole(w, flags, ch.n_used + 1), bo);
    });
    st.hard_groups = bo.hard_groups; st.hard_chars = bo.hard_chars;
    st.hard_big_groups = bo.hard_big_groups; st.hard_max_chars = bo.hard_max_chars; st.hard_max_members = bo.hard_max_members;
    st.hard_minor_groups = bo.hard_minor_groups; st.hard_minor_chars = bo.hard_minor_chars;
  }
  sync(c);
  st.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *n_used = ch.n_used;
}

// the reference's output files from the device results of a finished chain, produced one after the other into
// `sink(name, device pointer, bytes, buffer)` (host buffers of a pfp_bwt_result, files, or device blocks for the caller);
// buffer: the pool block that was filled for this output alone - a sink may take it over (hand_out) - or nullptr for the BWT
template <class Sink>
static void emit_outputs(pfp_ctx *c, const uint8_t *d_bwt, const SaView &d_sa, uint64_t n_out, int flags, Sink &&sink) {
  sink("bwt", d_bwt, n_out, nullptr);
  if (flags & PFP_FLAG_SA) {                       // .sa: n entries, SA[0]=n omitted (pfbwt.cpp:158-162)
    uint64_t cnt = n_out - 1;
    DBuf<uint8_t> packed(c, cnt * 5 + 16);
    PFP_REQUIRE(d_sa.dense, PFP_EINVAL, "full SA output without the SA values");
    pack5_dev(c, d_sa.dense + 1, cnt, packed.p);
    sink("sa", packed.p, cnt * 5, &packed);
    sync(c);
  }
  if (flags & PFP_FLAG_SSA) {
    DBuf<uint8_t> pairs;
    uint64_t k = sample_runs_dev(c, d_bwt, d_sa, n_out, false, pairs);
    sink("ssa", pairs.p, k * 10, &pairs);
    sync(c);
  }
  if (flags & PFP_FLAG_ESA) {
    DBuf<uint8_t> pairs;
    uint64_t k = sample_runs_dev(c, d_bwt, d_sa, n_out, true, pairs);
    sink("esa", pairs.p, k * 10, &pairs);
    sync(c);
  }
  sync(c);
}
void fetch_outputs(pfp_ctx *c, const uint8_t *d_bwt, const SaView &d_sa, uint64_t n_out, int flags, pfp_bwt_result *out) {
  emit_outputs(c, d_bwt, d_sa, n_out, flags, [&](const char *name, const uint8_t *d, uint64_t bytes, DBuf<uint8_t> *) {
    uint8_t *h = fetch_bytes(c, d, bytes);
    if (name[0] == 'b') { out->bwt = h; out->bwt_size = bytes; }
    else if (name[0] == 's' && name[1] == 'a') { out->sa = h; out->sa_bytes = bytes; }
    else if (name[0] == 's') { out->ssa = h; out->ssa_bytes = bytes; }
    else { out->esa = h; out->esa_bytes = bytes; }
  });
}

}  // namespace pfp

// PFP_TRACE_HOST: where the time of the host boundary goes
static bool trace_host() { static const bool on = getenv("PFP_TRACE_HOST") != nullptr; return on; }
static std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
static double ms(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// file to files: the host text (an mmap of the input works) is streamed in, the outputs are streamed from HBM
// straight into <base>.bwt / .sa / .ssa / .esa - no host copy of any output is held
template <class Stage>
static int bigbwt_to_files(pfp_ctx *c, uint64_t n, int w, uint64_t p, int flags, const char *base, uint64_t out_bytes[4], Stage &&stage) {
  PFP_TRY_DEV(c)
  check_args(w, p, flags);
  const auto t0 = now();
  join_background(c);
  // the two outputs whose sizes the text's length fixes get their files now: their pages are made ready beside the input and the chain
  MappedOut m_bwt, m_sa;
  // (measured: holding the registrations back until the text is in, or starting only then, moves the helper's 1.6-1.9 s for
  //  12.6 GB behind the chain instead of beside the input - same total; profiles/r04_cli_probe_hold.txt)
  const bool map_bwt = m_bwt.start(c, std::string(base) + ".bwt", n + 1);
  const bool map_sa = (flags & PFP_FLAG_SA) && n && m_sa.start(c, std::string(base) + ".sa", n * 5);
  Chain ch;
  stage(ch.tx);
  if (trace_host()) sync(c);
  const auto t1 = now();
  DBuf<uint8_t> d_bwt(c, n + 1 + 16);
  uint64_t used = 0;
  run_chain_dev(c, ch, n, w, p, flags, d_bwt.p, nullptr, &used);
  const auto t2 = now();
  uint64_t sizes[4] = {0, 0, 0, 0};
  int n_mapped = 0;
  emit_outputs(c, d_bwt.p, sa_view(ch.out), used + 1, flags, [&](const char *name, const uint8_t *d, uint64_t bytes, DBuf<uint8_t> *) {
    sizes[name[0] == 'b' ? 0 : (name[1] == 'a' ? 1 : (name[0] == 's' ? 2 : 3))] = bytes;
    if (trace_host()) fprintf(stderr, "[pfp]   %.1f ms after the chain: .%s (%.2f GB) is on the device\n", ms(t2, now()), name, bytes / 1e9);
    MappedOut *mo = name[0] == 'b' ? (map_bwt ? &m_bwt : nullptr) : (name[0] == 's' && name[1] == 'a' && name[2] == 0 ? (map_sa ? &m_sa : nullptr) : nullptr);
    MappedOut late;      // .ssa / .esa (and an .sa that could not start early): their sizes are only known now - the helper works while the copies follow it
    if (!mo && late.start(c, std::string(base) + "." + name, bytes)) mo = &late;
    if (mo && mo->active() && bytes <= mo->bytes) {
      if (mo->write(c, d, bytes)) {
        n_mapped++;
        if (mo != &m_bwt) mo->finish(c, bytes);      // (its device buffer goes back to the pool when this returns; the BWT's lives to the end)
        return;
      }
      mo->abandon(false);
    } else if (mo && mo->active()) mo->abandon(false);
    write_dev_file(c, std::string(base) + "." + name, 0, d, bytes, true);
  });
  if (trace_host()) fprintf(stderr, "[pfp]   %.1f ms after the chain: the other files are written\n", ms(t2, now()));
  if (m_bwt.active()) m_bwt.finish(c, sizes[0]);
  if (m_sa.active()) m_sa.abandon(true);
  if (trace_host())
    fprintf(stderr, "[pfp] file to files: text in %.1f ms, chain %.1f ms (first call: the pool is cold), files out %.1f ms%s\n", ms(t0, t1), ms(t1, t2),
            ms(t2, now()), n_mapped ? (std::string(" (") + std::to_string(n_mapped) + " of them straight into the files' mapped pages)").c_str() : "");
  if (out_bytes) memcpy(out_bytes, sizes, sizeof sizes);
  return PFP_OK;
  PFP_CATCH(c)
}

extern "C" {

// ---------------------------------------------------------------- output formats of device-resident results
int pfp_pack5_dev(pfp_ctx *c, const void *d_vals, uint64_t count, void *d_out5) {
  if (!c || ((!d_vals || !d_out5) && count)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  pack5_dev(c, (const uint64_t *)d_vals, count, (uint8_t *)d_out5);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_sample_runs_dev(pfp_ctx *c, const void *d_bwt, const void *d_sa, uint64_t count, uint64_t pos_base, int left_byte,
                        int right_byte, int run_end, void *d_out10, uint64_t cap_pairs, uint64_t *n_pairs) {
  if (!c || !n_pairs || (count && !d_bwt) || (d_out10 && count && !d_sa)) return PFP_EINVAL;
  *n_pairs = 0;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(left_byte >= -1 && left_byte <= 255 && right_byte >= -1 && right_byte <= 255, PFP_EINVAL, "neighbour bytes are -1 or 0..255");
  PFP_REQUIRE(pos_base + count <= (1ull << 40), PFP_ELIMIT, "positions do not fit 5 bytes");
  RunSampler rs(c, (const uint8_t *)d_bwt, count, left_byte, right_byte, run_end != 0);
  *n_pairs = rs.pairs;
  if (!d_out10) return PFP_OK;                  // count only
  PFP_REQUIRE(rs.pairs <= cap_pairs, PFP_ELIMIT, "output buffer holds " + std::to_string(cap_pairs) + " pairs, the slice has " +
                                                     std::to_string(rs.pairs) + " run boundaries");
  SaView sv;
  sv.dense = (const uint64_t *)d_sa;
  rs.place(sv, pos_base, (uint8_t *)d_out10);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

// pfthreads.hpp:369-376: every worker pwrite()s its range of the output file at its offset
int pfp_pwrite_dev(pfp_ctx *c, const char *path, uint64_t file_offset, const void *d_src, uint64_t nbytes) {
  if (!c || !path || (!d_src && nbytes)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  write_dev_file(c, path, file_offset, (const uint8_t *)d_src, nbytes, false);
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- whole chain
int pfp_bigbwt_dev(pfp_ctx *c, const void *d_text, uint64_t n, int w, uint64_t p, int flags, void *d_bwt, void *d_sa,
                   uint64_t *n_used) {
  if (!c || (!d_text && n) || !d_bwt || (flags && !d_sa)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  check_args(w, p, flags);
  PFP_REQUIRE(((uintptr_t)d_bwt & 15) == 0, PFP_EINVAL, "d_bwt must be 16-byte aligned");
  Chain ch;
  ch.tx.stage(c, d_text, true, n, w);
  uint64_t used = 0;
  run_chain_dev(c, ch, n, w, p, flags, (uint8_t *)d_bwt, (uint64_t *)d_sa, &used);
  if (n_used) *n_used = used;
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_bigbwt(pfp_ctx *c, const uint8_t *text, uint64_t n, int w, uint64_t p, int flags, pfp_bwt_result *out) {
  if (!c || (!text && n) || !out) return PFP_EINVAL;
  memset(out, 0, sizeof *out);
  PFP_TRY_DEV(c)
  check_args(w, p, flags);
  const auto t0 = now();
  Chain ch;
  ch.tx.stage(c, text, false, n, w);
  if (trace_host()) sync(c);
  const auto t1 = now();
  DBuf<uint8_t> d_bwt(c, n + 1 + 16);
  uint64_t used = 0;
  run_chain_dev(c, ch, n, w, p, flags, d_bwt.p, nullptr, &used);
  const auto t2 = now();
  fetch_outputs(c, d_bwt.p, sa_view(ch.out), used + 1, flags, out);
  if (trace_host())
    fprintf(stderr, "[pfp] host boundary: text in %.1f ms, chain %.1f ms, outputs out %.1f ms (%.2f GB in, %.2f GB out)\n", ms(t0, t1), ms(t1, t2),
            ms(t2, now()), n / 1e9, (out->bwt_size + out->sa_bytes + out->ssa_bytes + out->esa_bytes) / 1e9);
  return PFP_OK;
  PFP_CATCH(c)
}

// Device-resident chain whose SA-derived outputs are the reference's files, not SA values: .sa (PFP_FLAG_SA, 5-byte
// ints), .ssa / .esa (10-byte pairs) as device buffers of the library (pfp_dev_free).  The SA values themselves stay
// inside (allocated after the suffix sorter has returned its scratch): the 8 bytes per text byte a d_sa array takes
// are what keeps a 12.6 GB input with -s from fitting one GPU next to the sorter.
int pfp_bigbwt_formats_dev(pfp_ctx *c, const void *d_text, uint64_t n, int w, uint64_t p, int flags, void *d_bwt,
                           void *d_out[3], uint64_t out_bytes[3], uint64_t *n_used) {
  if (!c || (!d_text && n) || !d_bwt || !d_out || !out_bytes) return PFP_EINVAL;
  for (int k = 0; k < 3; k++) { d_out[k] = nullptr; out_bytes[k] = 0; }
  PFP_TRY_DEV(c)
  check_args(w, p, flags);
  PFP_REQUIRE(((uintptr_t)d_bwt & 15) == 0, PFP_EINVAL, "d_bwt must be 16-byte aligned");
  Chain ch;
  ch.tx.stage(c, d_text, true, n, w);
  uint64_t used = 0;
  run_chain_dev(c, ch, n, w, p, flags, (uint8_t *)d_bwt, nullptr, &used);
  if (n_used) *n_used = used;
  emit_outputs(c, (const uint8_t *)d_bwt, sa_view(ch.out), used + 1, flags, [&](const char *name, const uint8_t *, uint64_t bytes, DBuf<uint8_t> *buf) {
    if (name[0] == 'b') return;
    const int k = name[1] == 'a' ? 0 : (name[0] == 's' ? 1 : 2);
    // the block the output was written into goes to the caller as it is (a block of the context's pool, handed back by
    // pfp_dev_free: steady-state calls do not reach the driver); never null, an empty output included
    d_out[k] = hand_out(*buf); out_bytes[k] = bytes;
  });
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_bigbwt_files(pfp_ctx *c, const uint8_t *text, uint64_t n, int w, uint64_t p, int flags, const char *base,
                     uint64_t out_bytes[4]) {
  if (!c || (!text && n) || !base) return PFP_EINVAL;
  return bigbwt_to_files(c, n, w, p, flags, base, out_bytes, [&](StagedText &tx) { tx.stage(c, text, false, n, w); });
}
// the same with the text read from bytes [file_offset, file_offset + n) of an open file (parallel pread into the pinned
// staging buffers: what the C driver uses for a plain input file)
int pfp_bigbwt_fd(pfp_ctx *c, int fd, uint64_t file_offset, uint64_t n, int w, uint64_t p, int flags, const char *base,
                  uint64_t out_bytes[4]) {
  if (!c || fd < 0 || !base) return PFP_EINVAL;
  return bigbwt_to_files(c, n, w, p, flags, base, out_bytes, [&](StagedText &tx) { tx.stage_fd(c, fd, file_offset, n, w); });
}

}  // extern "C"
