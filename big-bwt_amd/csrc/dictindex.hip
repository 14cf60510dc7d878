// dictindex.hip -- what the later stages ask about the dictionary: the word lookup over its bytes (DictIndex, wordview.hpp),
// the word table of a dictionary given as bytes, the lexicographic rank of every word (newscan.cpp:622-636) and the
// number of BWT positions a set of suffix-array slots emits.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include <algorithm>

namespace pfp {

static constexpr int TB = 256;

// Word lookup over the dictionary (wordview.hpp): terminators per 64-byte line, scanned, and the word ends from the
// word table.  |D| / 16 + 8 d bytes instead of the 8 bytes per dictionary byte of pos_word[] / slen[] (rounds 1-2).
__global__ __launch_bounds__(256) void line_terms_kernel(const uint8_t *__restrict__ b, uint64_t N, uint64_t nlines, uint32_t *__restrict__ cnt) {
  const uint64_t ln = (uint64_t)BID * 256 + threadIdx.x;
  if (ln > nlines) return;
  if (ln == nlines) { cnt[ln] = 0; return; }
  const uint64_t b0 = ln * 64;
  const uint32_t nb = N - b0 >= 64 ? 64u : (uint32_t)(N - b0);      // (the padding behind the dictionary is zero, but keep the count exact)
  const uint4 *line = reinterpret_cast<const uint4 *>(b + b0);
  uint32_t n = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) if (nb > 16u * q) n += count_term_bytes16(line[q], nb - 16u * q < 16u ? nb - 16u * q : 16u);
  cnt[ln] = n;
}
__global__ void word_ends_kernel(uint32_t d, const uint64_t *__restrict__ woff, const uint32_t *__restrict__ wlen, uint64_t dsize,
                                 uint64_t *__restrict__ wend) {
  const uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j > d) return;
  wend[j] = j == d ? dsize - 1 : woff[j] + wlen[j];      // the word's 0x01; the final 0x00 is its own word
}

void build_dict_index(pfp_ctx *c, const Dictionary &D, DictIndex &ix) {
  const uint64_t N = D.dsize;
  PFP_REQUIRE(D.woff.p && D.wlen.p, PFP_EINVAL, "dictionary without a word table");
  PFP_REQUIRE(((uintptr_t)D.bytes.p & 63) == 0, PFP_EINVAL, "dictionary bytes must be 64-byte aligned");
  const uint64_t nlines = cdiv64(N, 64);
  DBuf<uint32_t> cnt(c, nlines + 1);
  ix.blk_word.alloc(c, nlines + 1);
  ix.wend.alloc(c, D.d + 1);
  KScope ks(c, "pfp::line_terms_kernel", N + nlines * 12 + D.d * 20);
  hipLaunchKernelGGL(line_terms_kernel, gdim(cdiv(nlines + 1, TB)), gdim(TB), 0, c->stream, D.bytes.p, N, nlines, cnt.p);
  exclusive_sum_u32(c, cnt.p, ix.blk_word.p, nlines + 1);
  hipLaunchKernelGGL(word_ends_kernel, gdim(cdiv((uint64_t)D.d + 1, TB)), gdim(TB), 0, c->stream, (uint32_t)D.d, D.woff.p, D.wlen.p, N, ix.wend.p);
  PFP_HIP(hipGetLastError());
}

// word table of a dictionary given as bytes (words + 0x01, closed by 0x00): terminator positions by
// compaction of the 0x01 bytes, then starts and lengths
__global__ void words_from_ends_kernel(uint32_t d, const uint64_t *__restrict__ ends, uint64_t dsize, uint64_t *__restrict__ woff,
                                       uint32_t *__restrict__ wlen) {
  uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j == 0) woff[d] = dsize - 1;
  if (j >= d) return;
  const uint64_t s0 = j ? (uint64_t)ends[j - 1] + 1 : 0;
  woff[j] = s0;
  wlen[j] = (uint32_t)(ends[j] - s0);
}
void word_table_from_bytes(pfp_ctx *c, Dictionary &D, uint64_t max_words) {
  DBuf<uint64_t> ends(c, max_words + 1), cnt(c, 1);
  select_byte_index<uint64_t>(c, D.bytes.p, kEndOfWord, ends.p, cnt.p, D.dsize);
  D.d = read_scalar(c, cnt.p);
  PFP_REQUIRE(D.d <= max_words, PFP_EFORMAT, "more words in the dictionary bytes than announced");
  D.woff.alloc(c, D.d + 1); D.wlen.alloc(c, std::max<uint64_t>(D.d, 1));
  if (D.d)
    hipLaunchKernelGGL(words_from_ends_kernel, gdim(cdiv(D.d, TB)), gdim(TB), 0, c->stream, (uint32_t)D.d, ends.p, D.dsize, D.woff.p,
                       D.wlen.p);
  PFP_HIP(hipGetLastError());
}

// Lexicographic rank of every word.  A whole word is a singleton group in SA(D) (the parse is
// prefix free), so rank[start of word] is its slot: sorting the d words by that slot gives the
// order std::sort produces in the reference (newscan.cpp:622-636) without touching all N slots.
__global__ void iota_u32_kernel(uint32_t d, uint32_t *__restrict__ val) {
  uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j < d) val[j] = j;
}
__global__ void lexrank_from_order_kernel(uint32_t d, const uint32_t *__restrict__ word_sorted, uint32_t *__restrict__ lexrank) {
  uint32_t r = BID * blockDim.x + threadIdx.x;
  if (r < d) lexrank[word_sorted[r]] = r;
}

// multi-GPU: every share of the suffix array reported 1 + slot for the words it holds, 0 for the others
__global__ void combine_word_slots_kernel(uint32_t d, uint32_t parts, const uint64_t *__restrict__ wslot_all,
                                          uint64_t *__restrict__ key, uint32_t *__restrict__ missing) {
  uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j >= d) return;
  uint64_t v = 0;
  for (uint32_t r = 0; r < parts; r++) { const uint64_t x = wslot_all[(uint64_t)r * d + j]; v = x > v ? x : v; }
  if (v == 0) atomicAdd(missing, 1u);
  key[j] = v - 1;
}
void compute_lexrank_from_slots(pfp_ctx *c, const Dictionary &D, const uint64_t *d_wslot_all, uint32_t parts, DictIndex &ix) {
  const uint32_t d = (uint32_t)D.d;
  ix.lexrank.alloc(c, d);
  DBuf<uint64_t> key(c, d), keyo(c, d);
  DBuf<uint32_t> val(c, d), valo(c, d), missing(c, 1);
  missing.zero();
  hipLaunchKernelGGL(combine_word_slots_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, parts, d_wslot_all, key.p, missing.p);
  PFP_REQUIRE(read_scalar(c, missing.p) == 0, PFP_EFORMAT, "a dictionary word was claimed by no share of the suffix array");
  hipLaunchKernelGGL(iota_u32_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, val.p);
  sort_pairs_u64_u32(c, key.p, keyo.p, val.p, valo.p, d, 0, bits_for(D.dsize));
  hipLaunchKernelGGL(lexrank_from_order_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, valo.p, ix.lexrank.p);
  PFP_HIP(hipGetLastError());
  ix.wslot_lex = std::move(keyo);      // the slots in ascending order = in the words' lexicographic order
}

// number of BWT positions the slots of `so` emit (sum of the occurrence counts of their words)
template <class I>
__global__ __launch_bounds__(256) void slot_output_count_kernel(uint64_t n, const I *__restrict__ sa, WordView wv,
                                                                const uint32_t *__restrict__ wocc, uint32_t d, int w,
                                                                unsigned long long *__restrict__ total) {
  __shared__ unsigned long long ws[4];
  unsigned long long cnt = 0;
  for (uint64_t t = (uint64_t)BID * 256 + threadIdx.x; t < n; t += (uint64_t)GDIM * 256) {
    const I i = sa[t];
    const uint32_t wd = word_of(wv, i);
    if (wd < d && wv.wend[wd] - i > (uint64_t)w) cnt += wocc[wd];
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) { const unsigned long long t2 = ws[0] + ws[1] + ws[2] + ws[3]; if (t2) atomicAdd(total, t2); }
}
template <class I>
uint64_t count_slot_outputs(pfp_ctx *c, const Dictionary &D, const DictIndex &ix, const SuffixOrderT<I> &so, int w) {
  DBuf<unsigned long long> total(c, 1);
  total.zero();
  if (so.N)
    hipLaunchKernelGGL(slot_output_count_kernel<I>, gdim((int)std::min<uint64_t>(cdiv64(so.N, 256), (uint64_t)c->n_cu * 16)), gdim(256),
                       0, c->stream, so.N, so.sa.p, word_view(D, ix), D.wocc.p, (uint32_t)D.d, w, total.p);
  PFP_HIP(hipGetLastError());
  PFP_HIP(hipMemcpyAsync(c->h_scalars, total.p, 8, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  return c->h_scalars[0];
}
template uint64_t count_slot_outputs<uint32_t>(pfp_ctx *, const Dictionary &, const DictIndex &, const SuffixOrderT<uint32_t> &, int);
template uint64_t count_slot_outputs<uint64_t>(pfp_ctx *, const Dictionary &, const DictIndex &, const SuffixOrderT<uint64_t> &, int);

template <class I>
__global__ void widen_kernel(uint32_t n, const I *__restrict__ in, uint64_t *__restrict__ out) {
  uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j < n) out[j] = (uint64_t)in[j];
}
template <class I>
void compute_lexrank(pfp_ctx *c, const Dictionary &D, SuffixOrderT<I> &so, DictIndex &ix) {
  const uint32_t d = (uint32_t)D.d;
  ix.lexrank.alloc(c, d);
  DBuf<I> key(c, d), keyo(c, d);
  DBuf<uint32_t> val(c, d), valo(c, d);
  gather_ranks<I>(c, so, D.woff.p, d, key.p);
  hipLaunchKernelGGL(iota_u32_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, val.p);
  sort_pairs<I, uint32_t>(c, key.p, keyo.p, val.p, valo.p, d, 0, bits_for(D.dsize));
  hipLaunchKernelGGL(lexrank_from_order_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, valo.p, ix.lexrank.p);
  ix.wslot_lex.alloc(c, d);
  hipLaunchKernelGGL((widen_kernel<I>), gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, keyo.p, ix.wslot_lex.p);
  PFP_HIP(hipGetLastError());
}
template void compute_lexrank<uint32_t>(pfp_ctx *, const Dictionary &, SuffixOrderT<uint32_t> &, DictIndex &);
template void compute_lexrank<uint64_t>(pfp_ctx *, const Dictionary &, SuffixOrderT<uint64_t> &, DictIndex &);

}  // namespace pfp
