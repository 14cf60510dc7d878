// api_stages.hip -- the reference's stage executables and gsa/gsacak.h over host buffers that hold its files byte for byte:
// pfp_scan, pfp_parse, pfp_bwtparse, pfp_merge, pfp_sacak* / pfp_gsacak* (with gsacak's optional LCP and DA arrays).
#include "chain.hpp"

using namespace pfp;

namespace pfp {

__global__ void sorted_len1_kernel(uint32_t d, const uint32_t *__restrict__ word_at_rank,
                                   const uint32_t *__restrict__ wlen, uint32_t *__restrict__ len1) {
  uint32_t r = BID * blockDim.x + threadIdx.x;
  if (r == 0) len1[d] = 0;
  if (r < d) len1[r] = wlen[word_at_rank[r]] + 1;
}

// narrowing / widening copy of an index array to the host (the staged gsacak.h entry points fix their SA width)
template <class A, class B>
__global__ void convert_kernel(const A *__restrict__ in, uint64_t n, B *__restrict__ out) {
  uint64_t i = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (B)in[i];
}
template <class A, class B>
static void fetch_converted(pfp_ctx *c, const A *d_in, uint64_t n, B *h_out) {
  if constexpr (sizeof(A) == sizeof(B)) {
    d2h(c, (A *)h_out, d_in, n);
    sync(c);
  } else {
    DBuf<B> tmp(c, n);
    hipLaunchKernelGGL((convert_kernel<A, B>), gdim(cdiv(n, TB)), gdim(TB), 0, c->stream, d_in, n, tmp.p);
    PFP_HIP(hipGetLastError());
    d2h(c, h_out, tmp.p, n);
    sync(c);
  }
}

}  // namespace pfp

// suffix array of an integer string ending in a unique 0 (symbols < k; k = 0: not stated) into a host array of OUT-wide entries
template <class OUT>
static void sacak_int_any(pfp_ctx *c, const uint32_t *s, OUT *SA, uint64_t n, uint64_t k) {
  PFP_REQUIRE(n >= 1, PFP_EINVAL, "empty string");
  PFP_REQUIRE(s[n - 1] == 0, PFP_EFORMAT, "sacak_int: last symbol must be 0");
  DBuf<uint32_t> ds(c, n);
  h2d(c, ds.p, s, n);
  SuffixOrder so;
  sort_int_suffixes(c, ds.p, n, so, k ? (uint32_t)std::min<uint64_t>(k - 1, 0xFFFFFFFFull) : 0xFFFFFFFFu);
  fetch_converted<uint32_t, OUT>(c, so.sa.p, n, SA);
}
// suffix array of a byte string ending in a unique 0 into a host array of OUT-wide entries
template <class OUT>
static void sacak_any(pfp_ctx *c, const uint8_t *s, OUT *SA, uint64_t n) {
  PFP_REQUIRE(n >= 1, PFP_EINVAL, "empty string");
  PFP_REQUIRE(s[n - 1] == 0, PFP_EFORMAT, "sacak: last symbol must be 0");
  PFP_REQUIRE(sizeof(OUT) == 8 || n < 0xFFFFFFF0ull, PFP_ELIMIT, "text of 4 GiB or more needs the 64-bit entry point (simplebwt64)");
  DBuf<uint8_t> ds(c, n + 64);
  h2d(c, ds.p, s, n);
  PFP_HIP(hipMemsetAsync(ds.p + n, 0, 64, c->stream));
  with_width(use_wide_index(c, n), [&](auto tag) {
    using I = decltype(tag);
    SuffixOrderT<I> so;
    sort_byte_suffixes<I>(c, ds.p, n, so);
    fetch_converted<I, OUT>(c, so.sa.p, n, SA);
  });
}

// dictionary given as bytes: fill D.{bytes,dsize,d,woff,wlen} and the index
static void dictionary_from_host(pfp_ctx *c, const uint8_t *s, uint64_t n, Dictionary &D, DictIndex &ix) {
  PFP_REQUIRE(n >= 2 && s[n - 1] == kEndOfDict && s[n - 2] == kEndOfWord, PFP_EFORMAT,
              "dictionary must end with 0x01 0x00 (pfbwt.cpp:498-503)");
  D.dsize = n;
  D.bytes.alloc(c, n + 64);
  h2d(c, D.bytes.p, s, n);
  PFP_HIP(hipMemsetAsync(D.bytes.p + n, 0, 64, c->stream));
  word_table_from_bytes(c, D, n);
  build_dict_index(c, D, ix);
}

// gsacak's optional outputs (gsa/gsacak.h:78-105): LCP[i] = length of the common prefix of the suffixes SA[i-1] and
// SA[i], where a separator (1) or the final 0 ends the count (gsa/README.md:76-104); DA[i] = index of the string
// the suffix SA[i] starts in.
// Pass 1: one thread per slot compares its two suffixes 8 bytes at a time, for at most kLcpCap bytes; a pair still equal
// there is flagged.  Pass 2 (only if something was flagged - long exact repeats: an 18 Mb run of N inside one string has
// 18 M pairs with a mean common prefix of 9 MB, which one thread per pair would never finish): the flagged slots in TEXT
// order, 1024 of them per wave.  Neighbours in text order inherit (Kasai et al.: lcp(phi(b+1), b+1) >= lcp(phi(b), b) - 1;
// separators rank as distinct smallest symbols, gsacak.c:2493, so the lemma holds for a collection), the compare itself
// is the whole wave's: 64 lanes x 16 bytes per step, a ballot finds the first difference or end.
constexpr uint32_t kLcpCap = 2048;
constexpr uint32_t kLcpChunk = 1024;
template <class I, class L>
__global__ void lcp_da_kernel(const uint8_t *__restrict__ s, uint64_t n, const I *__restrict__ sa, WordView wv,
                              L *__restrict__ lcp, L *__restrict__ da, uint8_t *__restrict__ longf) {
  const uint64_t t = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint64_t b = sa[t];
  if (da) da[t] = (L)word_of(wv, b);
  if (!lcp) return;
  longf[t] = 0;
  if (t == 0) { lcp[0] = 0; return; }
  const uint64_t a = sa[t - 1];
  uint64_t l = 0;
  for (; l < kLcpCap; l += 8) {
    const uint64_t x = ld8u(s + a + l), y = ld8u(s + b + l);
    const uint64_t end = lt2_flags64(x);
    const uint64_t diff = x ^ y;
    if (diff | end) {
      const int fd = diff ? (__builtin_ctzll(diff) >> 3) : 8, fe = end ? (__builtin_ctzll(end) >> 3) : 8;
      lcp[t] = (L)(l + (fd < fe ? fd : fe));
      return;
    }
  }
  longf[t] = 1;      // equal for kLcpCap bytes: pass 2
}
template <class I>
__global__ void lcp_long_pos_kernel(uint64_t m, const uint64_t *__restrict__ slot, const I *__restrict__ sa, uint64_t *__restrict__ pos) {
  const uint64_t j = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (j < m) pos[j] = sa[slot[j]];
}
// one wave per kLcpChunk flagged pairs (sorted by text position b; slot[j] = their suffix-array slot)
template <class I, class L>
__global__ __launch_bounds__(64) void lcp_long_kernel(const uint8_t *__restrict__ s, uint64_t n, const I *__restrict__ sa, uint64_t m,
                                                      const uint64_t *__restrict__ pos, const uint64_t *__restrict__ slot, L *__restrict__ lcp) {
  const uint64_t j0 = (uint64_t)BID * kLcpChunk;
  if (j0 >= m) return;
  const uint64_t j1 = j0 + kLcpChunk < m ? j0 + kLcpChunk : m;
  const int lane = threadIdx.x;
  uint64_t prev_b = ~0ull, prev_l = 0;
  for (uint64_t j = j0; j < j1; j++) {
    const uint64_t b = pos[j], t = slot[j], a = sa[t - 1];      // (slot 0 is never flagged)
    uint64_t l = kLcpCap;
    if (prev_b + 1 == b && prev_l > (uint64_t)kLcpCap + 1) l = prev_l - 1;
    for (;;) {
      const uint64_t off = l + (uint64_t)lane * 16;
      // (the buffer is padded with 64 zero bytes past n: a lane that would read beyond them sees an end instead)
      const bool in = a + off + 16 <= n + 64 && b + off + 16 <= n + 64;
      uint4 x = make_uint4(0u, 0u, 0u, 0u), y = x;
      if (in) { x = ld16u(s + a + off); y = ld16u(s + b + off); }
      const uint32_t xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
      int ev = 16;
#pragma unroll
      for (int q = 3; q >= 0; q--) {
        const uint32_t end = lt2_flags32(xs[q]), diff = xs[q] ^ ys[q];
        if (diff | end) {
          const int fd = diff ? (__builtin_ctz(diff) >> 3) : 4, fe = end ? (__builtin_ctz(end) >> 3) : 4;
          ev = 4 * q + (fd < fe ? fd : fe);
        }
      }
      const unsigned long long hit = __ballot(ev < 16);
      if (hit) {
        const int first = __ffsll((long long)hit) - 1;
        l += (uint64_t)first * 16 + (uint64_t)__shfl(ev, first, 64);
        break;
      }
      l += 1024;
    }
    if (lane == 0) lcp[t] = (L)l;
    prev_b = b; prev_l = l;
  }
}
template <class I, class L>
static void lcp_da_device(pfp_ctx *c, const uint8_t *bytes, uint64_t n, const I *sa, const WordView &wv, L *d_lcp, L *d_da) {
  DBuf<uint8_t> longf(c, d_lcp ? n + 16 : 16);
  if (d_lcp) PFP_HIP(hipMemsetAsync(longf.p + n, 0, 16, c->stream));
  hipLaunchKernelGGL((lcp_da_kernel<I, L>), gdim(cdiv(n, TB)), gdim(TB), 0, c->stream, bytes, n, sa, wv, d_lcp, d_da, longf.p);
  PFP_HIP(hipGetLastError());
  if (!d_lcp) return;
  const uint64_t m = count_flags(c, longf.p, n);
  if (!m) return;
  DBuf<uint64_t> slot(c, m), slot2(c, m), pos(c, m), pos2(c, m), cnt(c, 1);
  select_index<uint64_t>(c, longf.p, slot.p, cnt.p, n);
  hipLaunchKernelGGL(lcp_long_pos_kernel<I>, gdim(cdiv(m, TB)), gdim(TB), 0, c->stream, m, slot.p, sa, pos.p);
  sort_pairs_db(c, pos, pos2, slot, slot2, m, 0, bits_for(n));
  hipLaunchKernelGGL((lcp_long_kernel<I, L>), gdim((unsigned)cdiv64(m, kLcpChunk)), gdim(64), 0, c->stream, bytes, n, sa, m, pos.p, slot.p, d_lcp);
  PFP_HIP(hipGetLastError());
}
template <class OUT, class L>
static void gsacak_any(pfp_ctx *c, const uint8_t *s, OUT *SA, uint64_t n, L *LCP = nullptr, L *DA = nullptr) {
  PFP_REQUIRE(sizeof(OUT) == 8 || n < 0xFFFFFFF0ull, PFP_ELIMIT, "collection of 4 GiB or more needs the 64-bit entry point (gsacak.h -DM64)");
  Dictionary D; DictIndex ix;
  dictionary_from_host(c, s, n, D, ix);
  with_width(use_wide_index(c, n), [&](auto tag) {
    using I = decltype(tag);
    SuffixOrderT<I> so;
    sort_dict_suffixes<I>(c, D.bytes.p, n, word_view(D, ix), so);
    fetch_converted<I, OUT>(c, so.sa.p, n, SA);
    if (LCP || DA) {
      DBuf<L> dl(c, LCP ? n : 1), dd(c, DA ? n : 1);
      lcp_da_device<I, L>(c, D.bytes.p, n, so.sa.p, word_view(D, ix), LCP ? dl.p : (L *)nullptr, DA ? dd.p : (L *)nullptr);
      if (LCP) d2h(c, LCP, dl.p, n);
      if (DA) d2h(c, DA, dd.p, n);
      sync(c);
    }
  });
}

extern "C" {

// ---------------------------------------------------------------- stage 1a
int pfp_scan(pfp_ctx *c, const uint8_t *text, uint64_t n, int w, uint64_t p, uint64_t **ends, uint64_t *n_ends,
             uint64_t *n_used) {
  if (!c || (!text && n) || !ends || !n_ends) return PFP_EINVAL;
  *ends = nullptr; *n_ends = 0;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(w >= 1 && w <= 4096 && p >= 1, PFP_EINVAL, "bad window or modulus");
  StagedText tx;
  tx.stage(c, text, false, n, w);
  DBuf<uint64_t> d_ends;
  uint64_t used = n;
  uint64_t k = scan_text(c, tx, n, w, p, d_ends, &used);
  uint64_t *h = host_alloc<uint64_t>(k);
  if (k) d2h(c, h, d_ends.p, k);
  sync(c);
  *ends = h; *n_ends = k;
  if (n_used) *n_used = used;
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- stage 1
int pfp_parse(pfp_ctx *c, const uint8_t *text, uint64_t n, int w, uint64_t p, int want_sai, pfp_parse_result *out) {
  if (!c || (!text && n) || !out) return PFP_EINVAL;
  memset(out, 0, sizeof *out);
  PFP_TRY_DEV(c)
  check_args(w, p, 0);
  c->stats = pfp_stats{};
  Chain ch;
  ch.tx.stage(c, text, false, n, w);
  run_parse(c, ch, n, w, p, want_sai != 0, true, true);      // the staged parser's outputs do not depend on the key payload
  const uint32_t d = (uint32_t)ch.D.d;
  const uint64_t P = ch.D.P;
  // .dict in lexicographic order
  DBuf<uint32_t> len1(c, (size_t)d + 1);
  DBuf<uint64_t> doff(c, (size_t)d + 1);
  hipLaunchKernelGGL(sorted_len1_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, ch.word_at_rank.p, ch.D.wlen.p,
                     len1.p);
  exclusive_sum_u32_u64(c, len1.p, doff.p, (size_t)d + 1);
  DBuf<uint8_t> sdict(c, ch.D.dsize + 64);
  PFP_HIP(hipMemsetAsync(sdict.p + ch.D.dsize - 1, 0, 1, c->stream));
  permute_dictionary(c, d, ch.word_at_rank.p, ch.D.woff.p, ch.D.wlen.p, ch.D.bytes.p, doff.p, sdict.p);
  PFP_HIP(hipGetLastError());
  out->n_used = ch.n_used;
  out->dict_size = ch.D.dsize; out->n_words = d; out->n_phrases = P;
  out->dict = host_alloc<uint8_t>(ch.D.dsize);
  out->occ = host_alloc<uint32_t>(d);
  out->parse = host_alloc<uint32_t>(P);
  out->last = host_alloc<uint8_t>(P);
  d2h(c, out->dict, sdict.p, ch.D.dsize);
  d2h(c, out->occ, ch.occ_lex.p, d);
  d2h(c, out->parse, ch.sym.p, P);
  d2h(c, out->last, ch.D.last.p, P);
  if (want_sai) {
    DBuf<uint8_t> packed(c, P * 5);
    pack5_dev(c, ch.D.sai.p, P, packed.p);
    out->sai = host_alloc<uint8_t>(P * 5);
    d2h(c, out->sai, packed.p, P * 5);
    sync(c);
  }
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- suffix sorting
int pfp_sacak_int(pfp_ctx *c, const uint32_t *s, uint32_t *SA, uint64_t n, uint64_t k) {
  if (!c || !s || !SA) return PFP_EINVAL;   // gsacak.c:2498 returns -1 on NULL
  PFP_TRY_DEV(c)
  sacak_int_any<uint32_t>(c, s, SA, n, k);
  return PFP_OK;
  PFP_CATCH(c)
}
int pfp_sacak_int64(pfp_ctx *c, const uint32_t *s, uint64_t *SA, uint64_t n, uint64_t k) {
  if (!c || !s || !SA) return PFP_EINVAL;   // -DM64: uint_t SA entries, int_text stays 32 bits (gsacak.h:42-60)
  PFP_TRY_DEV(c)
  sacak_int_any<uint64_t>(c, s, SA, n, k);
  return PFP_OK;
  PFP_CATCH(c)
}
int pfp_sacak(pfp_ctx *c, const uint8_t *s, uint32_t *SA, uint64_t n) {
  if (!c || !s || !SA) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  sacak_any<uint32_t>(c, s, SA, n);
  return PFP_OK;
  PFP_CATCH(c)
}
int pfp_sacak64(pfp_ctx *c, const uint8_t *s, uint64_t *SA, uint64_t n) {
  if (!c || !s || !SA) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  sacak_any<uint64_t>(c, s, SA, n);
  return PFP_OK;
  PFP_CATCH(c)
}
int pfp_gsacak(pfp_ctx *c, const uint8_t *s, uint32_t *SA, uint64_t n) {
  if (!c || !s || !SA) return PFP_EINVAL;   // gsacak.c:2503
  PFP_TRY_DEV(c)
  gsacak_any<uint32_t, int32_t>(c, s, SA, n);
  return PFP_OK;
  PFP_CATCH(c)
}
int pfp_gsacak64(pfp_ctx *c, const uint8_t *s, uint64_t *SA, uint64_t n) {
  if (!c || !s || !SA) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  gsacak_any<uint64_t, int64_t>(c, s, SA, n);
  return PFP_OK;
  PFP_CATCH(c)
}
int pfp_gsacak_lcp_da(pfp_ctx *c, const uint8_t *s, uint32_t *SA, int32_t *LCP, int32_t *DA, uint64_t n) {
  if (!c || !s || !SA) return PFP_EINVAL;   // gsacak.c:2503; LCP and DA are optional like there
  PFP_TRY_DEV(c)
  gsacak_any<uint32_t, int32_t>(c, s, SA, n, LCP, DA);
  return PFP_OK;
  PFP_CATCH(c)
}
int pfp_gsacak_lcp_da64(pfp_ctx *c, const uint8_t *s, uint64_t *SA, int64_t *LCP, int64_t *DA, uint64_t n) {
  if (!c || !s || !SA) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  gsacak_any<uint64_t, int64_t>(c, s, SA, n, LCP, DA);
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- stage 2
int pfp_bwtparse(pfp_ctx *c, const uint32_t *parse, uint64_t P, const uint8_t *last, const uint8_t *sai,
                 const uint32_t *occ, uint64_t n_words, uint32_t *ilist, uint8_t *bwlast, uint8_t *bwsai) {
  if (!c || !parse || !last || !occ || !ilist || !bwlast || (sai && !bwsai)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(P >= 2, PFP_ESHORT, "parse has fewer than 2 phrases (bwtparse.c:244)");
  PFP_REQUIRE(P <= 0xFFFFFFFEull, PFP_ELIMIT, "Input containing more than 2^32-2 phrases (bwtparse.c:93)");
  DBuf<uint32_t> dparse(c, P), docc(c, n_words);
  DBuf<uint8_t> dlast(c, P);
  DBuf<uint64_t> dsai;
  h2d(c, dparse.p, parse, P); h2d(c, dlast.p, last, P); h2d(c, docc.p, occ, n_words);
  if (sai) {
    DBuf<uint8_t> packed(c, P * 5);
    h2d(c, packed.p, sai, P * 5);
    dsai.alloc(c, P);
    unpack5_dev(c, packed.p, P, dsai.p);
    sync(c);
  }
  ParseBWT pb;
  parse_bwt(c, dparse.p, P, dlast.p, sai ? dsai.p : nullptr, docc.p, n_words, pb);
  d2h(c, ilist, pb.ilist.p, P + 1);
  d2h(c, bwlast, pb.bwlast.p, P + 1);
  if (sai) {
    DBuf<uint8_t> packed(c, (P + 1) * 5);
    pack5_dev(c, pb.bwsai.p, P + 1, packed.p);
    d2h(c, bwsai, packed.p, (P + 1) * 5);
    sync(c);
  }
  sync(c);
  PFP_REQUIRE(ilist[0] == 1, PFP_EFORMAT, "ilist[0] != 1 (bwtparse.c:305): parse does not start with the smallest word");
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- stage 3
int pfp_merge(pfp_ctx *c, const uint8_t *dict, uint64_t dict_size, const uint32_t *occ, uint64_t n_words,
              const uint32_t *ilist, const uint8_t *bwlast, const uint8_t *bwsai, uint64_t n_plus_1, int w, int flags,
              pfp_bwt_result *out) {
  if (!c || !dict || !occ || !ilist || !bwlast || !out) return PFP_EINVAL;
  memset(out, 0, sizeof *out);
  PFP_TRY_DEV(c)
  check_args(w, 10, flags);
  PFP_REQUIRE(!flags || bwsai, PFP_EINVAL, "SA output requested but no bwsai given");
  PFP_REQUIRE(dict_size > 1 + (uint64_t)w, PFP_EFORMAT, "invalid dictionary file (pfbwt.cpp:332)");
  PFP_REQUIRE(ilist[0] == 1, PFP_EFORMAT, "ilist[0] != 1 (pfbwt.cpp:377)");
  PFP_REQUIRE(dict[0] == kDollar, PFP_EFORMAT, "dictionary must start with Dollar (pfbwt.cpp:125)");
  Dictionary D; DictIndex ix; DictOrder ord;
  dictionary_from_host(c, dict, dict_size, D, ix);
  PFP_REQUIRE(D.d == n_words, PFP_EFORMAT, "occ entries != dictionary words (pfbwt.cpp:357)");
  // expected output size: every suffix longer than w of every word, once per occurrence
  uint64_t expect = 0, tot_occ = 0;
  {
    uint64_t s = 0, j = 0;
    for (uint64_t i = 0; i < dict_size; i++) {
      // (a word's bytes are all above the terminators: the word lookup and the sorter count words by the bytes below 2)
      PFP_REQUIRE(dict[i] >= kDollar || dict[i] == kEndOfWord || i + 1 == dict_size, PFP_EFORMAT,
                  "invalid dictionary file: byte 0x00 inside a word at offset " + std::to_string(i));
      if (dict[i] == kEndOfWord) {
        uint64_t len = i - s;
        if (len > (uint64_t)w) expect += (len - (uint64_t)w) * occ[j];
        tot_occ += occ[j];
        j++; s = i + 1;
      }
    }
  }
  PFP_REQUIRE(tot_occ + 1 == n_plus_1, PFP_EFORMAT, "sum(occ)+1 != parse size (pfbwt.cpp:397)");
  D.wocc.alloc(c, D.d);
  h2d(c, D.wocc.p, occ, D.d);
  if (c->debug) validate_index(c, D, ix);
  const WordView wv = word_view(D, ix);
  const SlotPayloadSrc pay{wv, D.wocc.p, w};
  ord.wide = use_wide_index(c, D.dsize);      // pfbwt[NT].x or pfbwt[NT]64.x (bigbwt:130-151)
  with_width(ord.wide, [&](auto tag) {
    using I = decltype(tag);
    auto &so = ord.get<I>();
    sort_dict_suffixes<I>(c, D.bytes.p, D.dsize, wv, so, (flags & PFP_FLAG_SA) ? nullptr : &pay, w);      // (only the suffixes longer than w: chain.hip)
    if (c->debug) validate_suffix_order<I>(c, D.bytes.p, so, true, "dict SA");
    compute_lexrank<I>(c, D, so, ix);
  });
  if (c->debug) validate_lexrank(c, D, ix);
  DBuf<uint32_t> occ_lex(c, D.d);
  occ_in_lex_order(c, (uint32_t)D.d, ix.lexrank.p, D.wocc.p, occ_lex.p, nullptr);
  ParseBWT pb;
  pb.P = n_plus_1 - 1;
  pb.ilist.alloc(c, n_plus_1); pb.bwlast.alloc(c, n_plus_1);
  h2d(c, pb.ilist.p, ilist, n_plus_1); h2d(c, pb.bwlast.p, bwlast, n_plus_1);
  if (flags) {
    DBuf<uint8_t> packed(c, n_plus_1 * 5);
    h2d(c, packed.p, bwsai, n_plus_1 * 5);
    pb.bwsai.alloc(c, n_plus_1);
    unpack5_dev(c, packed.p, n_plus_1, pb.bwsai.p);
    sync(c);
  }
  DBuf<uint8_t> d_bwt(c, expect + 16);
  DBuf<uint64_t> d_sa;
  if (flags & PFP_FLAG_SA) d_sa.alloc(c, expect + 1);      // -s / -e: the merge keeps the values at the run boundaries (bo.sa_c)
  BwtOutputs bo;
  bo.d_bwt = d_bwt.p; bo.d_sa = d_sa.p;
  with_width(ord.wide, [&](auto tag) {
    using I = decltype(tag);
    merge_bwt<I>(c, D, ix, ord.get<I>(), pb, occ_lex.p, MergeOpts::whole(w, flags, expect), bo);
  });
  c->stats.hard_groups = bo.hard_groups; c->stats.hard_chars = bo.hard_chars;
  fetch_outputs(c, d_bwt.p, sa_view(bo), expect, flags, out);
  return PFP_OK;
  PFP_CATCH(c)
}

}  // extern "C"
