// seqmap.hip -- the sequences of a collection over an FmIndex: text position -> (sequence, offset), locate that keeps the hits inside
// one sequence, and document listing.  The reference has no counterpart; include/pfpgpu.h, "Sequences of a collection", states the
// definitions (starts[0..nseq], seq(x), kept).
//
//   seq(x).  A predecessor search over the starts, solved as fmsearch.hip solves phi^-1: a bucket directory over text positions
//   (bucket_dir_k, about one start per bucket), then a binary search among the bucket's starts.  The search is for the FIRST start
//   above x, so the equal starts of empty sequences resolve to the sequence that holds x.
//   Locate with sequences.  fm_locate's positions -> one lane per position: its pattern (a binary search over the unfiltered
//   offsets, as fm_expand does), seq(x) and the test x + m <= starts[seq + 1], the sequence or "dropped" in a u32 -> a library scan
//   counts the kept ones before every position -> a scatter writes (seq, off) in row order; pattern p's offset is the count at its
//   first unfiltered position.
//   Document listing, on the kept hits' sequence numbers (compacted as above, all rows).  Up to kDocLds sequences: the hits of a
//   pattern are cut into chunks of kDocChunk; a workgroup counts a chunk in an LDS histogram; a pattern of one chunk is finished by
//   that workgroup (the non-zero counters, in order: a block-wide scan per 256 counters), a pattern of several adds its non-zero
//   counters to a row in device memory that a workgroup of a second kernel finishes the same way - so a pattern with a million hits
//   is counted by many workgroups.  Two passes (count the documents, a library scan, write them): the histograms are rebuilt for
//   the second.  More sequences: the library's segmented sort inside each pattern's range, run heads (a new value or a new pattern),
//   a library scan of the heads, and the heads' positions give the counts.  Integer sums only: the same answers in any schedule.
// Bounds: a lane does one search of at most log2 of a bucket's starts; a workgroup reads at most kDocChunk hits and nseq counters.
// Values read from positions are tested against n before they index anything; sequence numbers are clamped to the table.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"

namespace pfp {

namespace {

constexpr uint64_t kDocLds = 4096;          // sequences whose counters (u64) fit in LDS: 32 KiB per workgroup, five workgroups per CU
constexpr uint64_t kDocChunk = 32768;       // hits a workgroup counts

template <class I>
__global__ void __launch_bounds__(kTB) seq_map_k(SeqArgs<I> s, const uint64_t *__restrict__ pos, uint64_t count, uint32_t *__restrict__ seq,
                                                 uint64_t *__restrict__ off) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i >= count) return;
  const uint64_t x = pos[i];
  uint32_t k = kNoSeq;
  uint64_t o = ~0ull;
  if (x < s.n) { k = seq_of(s, x); o = x - (uint64_t)s.start[k]; }
  if (seq) seq[i] = k;
  if (off) off[i] = o;
}

// one lane per located position i < U: tmp[i] = its sequence if the hit is kept, else kNoSeq; tmp[U] = kNoSeq (the scan's last entry)
template <class I>
__global__ void __launch_bounds__(kTB) seq_flag_k(SeqArgs<I> s, const uint64_t *__restrict__ pat_off, uint64_t npat, const uint64_t *__restrict__ uoff,
                                                  const uint64_t *__restrict__ pos, uint64_t U, uint32_t *__restrict__ tmp) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i > U) return;
  uint32_t k = kNoSeq;
  const uint64_t x = i < U ? pos[i] : ~0ull;
  if (x < s.n) {
    const uint64_t p = last_le(uoff, npat, i);          // the position's pattern
    const uint64_t o0 = pat_off[p], o1 = pat_off[p + 1], m = o1 > o0 ? o1 - o0 : 0;
    const uint32_t q = seq_of(s, x);
    if (m <= (uint64_t)s.start[q + 1] - x) k = q;       // x + m <= starts[q + 1], without the sum
  }
  tmp[i] = k;
}

// the kept hits to their slots, in row order
template <class I>
__global__ void __launch_bounds__(kTB) seq_scatter_k(SeqArgs<I> s, const uint64_t *__restrict__ pos, uint64_t U, const uint32_t *__restrict__ tmp,
                                                     const uint64_t *__restrict__ slot, uint32_t *__restrict__ seq, uint64_t *__restrict__ off) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i >= U) return;
  const uint32_t k = tmp[i];
  if (k == kNoSeq) return;
  const uint64_t j = slot[i];
  seq[j] = k;
  if (off) off[j] = pos[i] - (uint64_t)s.start[k];
}

// ---------------------------------------------------------------- document listing: the histogram regime
// per pattern (entry npat: 0): the chunks of its kept hits, and whether it needs a row (more than one chunk)
__global__ void __launch_bounds__(kTB) doc_plan_k(const uint64_t *__restrict__ hoff, uint64_t npat, uint64_t chunk, uint64_t *__restrict__ nchunk,
                                                  uint64_t *__restrict__ isrow) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p > npat) return;
  const uint64_t c = p < npat ? hoff[p + 1] - hoff[p] : 0, k = (c + chunk - 1) / chunk;
  nchunk[p] = k;
  isrow[p] = k > 1;
}
__global__ void __launch_bounds__(kTB) doc_rowpat_k(const uint64_t *__restrict__ isrow, const uint64_t *__restrict__ row_of, uint64_t npat,
                                                    uint64_t *__restrict__ rowpat) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p < npat && isrow[p]) rowpat[row_of[p]] = p;
}

// the whole workgroup: the non-zero counters among ctr[0 .. nseq) in order.  EMIT: written from slot base on; else *ndoc = their number
template <bool EMIT>
__device__ __forceinline__ void doc_tail(const unsigned long long *ctr, uint64_t nseq, uint64_t *ndoc, uint64_t base, uint32_t *__restrict__ doc,
                                         uint64_t *__restrict__ cnt, uint32_t *wsum) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint64_t run = 0;
  for (uint64_t t0 = 0; t0 < nseq; t0 += kTB) {         // (t0 and run are the same in every lane)
    const uint64_t t = t0 + threadIdx.x;
    const unsigned long long c = t < nseq ? ctr[t] : 0;
    const uint32_t f = c != 0, incl = wave_incl_sum(f);
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kTB / 64; w++) {
      if (w < wv) before += wsum[w];
      total += wsum[w];
    }
    if (EMIT && f) {
      const uint64_t j = base + run + before + incl - 1;
      doc[j] = (uint32_t)t;
      cnt[j] = c;
    }
    run += total;
    __syncthreads();
  }
  if (!EMIT && threadIdx.x == 0) *ndoc = run;
}

// one workgroup per chunk of a pattern's kept hits (sq: their sequence numbers, all below nseq <= kDocLds)
template <bool EMIT>
__global__ void __launch_bounds__(kTB) doc_hist_k(const uint32_t *__restrict__ sq, const uint64_t *__restrict__ hoff, uint64_t npat,
                                                  const uint64_t *__restrict__ chunk_off, uint64_t C, uint64_t chunk, uint64_t nseq,
                                                  const uint64_t *__restrict__ row_of, unsigned long long *__restrict__ rows, uint64_t *__restrict__ ndoc,
                                                  const uint64_t *__restrict__ doc_off, uint32_t *__restrict__ doc, uint64_t *__restrict__ cnt) {
  __shared__ unsigned long long h[kDocLds];
  __shared__ uint32_t wsum[kTB / 64];
  const uint64_t b = BID;
  if (b >= C) return;                                   // (the whole workgroup)
  const uint64_t p = last_le(chunk_off, npat, b);       // the last pattern with chunk_off[p] <= b: it has a chunk b
  const uint64_t k = b - chunk_off[p], nchunks = chunk_off[p + 1] - chunk_off[p];
  if (EMIT && nchunks > 1) return;                      // (written from its row)
  const uint64_t i0 = hoff[p] + k * chunk, end = hoff[p + 1], i1 = i0 + chunk < end ? i0 + chunk : end;
  for (uint64_t t = threadIdx.x; t < nseq; t += kTB) h[t] = 0;
  __syncthreads();
  for (uint64_t i = i0 + threadIdx.x; i < i1; i += kTB) {
    const uint32_t s = sq[i];
    if (s < nseq) atomicAdd(&h[s], 1ull);
  }
  __syncthreads();
  if (nchunks > 1) {
    unsigned long long *row = rows + row_of[p] * nseq;
    for (uint64_t t = threadIdx.x; t < nseq; t += kTB)
      if (h[t]) atomicAdd(&row[t], h[t]);
    return;
  }
  doc_tail<EMIT>(h, nseq, &ndoc[p], EMIT ? doc_off[p] : 0, doc, cnt, wsum);
}

// one workgroup per pattern of several chunks: its row
template <bool EMIT>
__global__ void __launch_bounds__(kTB) doc_rows_k(const unsigned long long *__restrict__ rows, const uint64_t *__restrict__ rowpat, uint64_t R, uint64_t nseq,
                                                  uint64_t *__restrict__ ndoc, const uint64_t *__restrict__ doc_off, uint32_t *__restrict__ doc,
                                                  uint64_t *__restrict__ cnt) {
  __shared__ uint32_t wsum[kTB / 64];
  const uint64_t r = BID;
  if (r >= R) return;
  const uint64_t p = rowpat[r];
  doc_tail<EMIT>(rows + r * nseq, nseq, &ndoc[p], EMIT ? doc_off[p] : 0, doc, cnt, wsum);
}

// ---------------------------------------------------------------- document listing: the sort regime
__global__ void __launch_bounds__(kTB) doc_heads_k(const uint32_t *__restrict__ sorted, uint64_t K, uint32_t *__restrict__ head) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i >= 1 && i < K && sorted[i] != sorted[i - 1]) head[i] = 1;
}
// run j starts at hp[j]; hp[D] = K
__global__ void __launch_bounds__(kTB) doc_runs_k(const uint32_t *__restrict__ sorted, uint64_t K, const uint32_t *__restrict__ head,
                                                  const uint64_t *__restrict__ hs, uint32_t *__restrict__ doc, uint64_t *__restrict__ hp) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i > K) return;
  if (i == K) { hp[hs[K]] = K; return; }
  if (!head[i]) return;
  const uint64_t j = hs[i];
  doc[j] = sorted[i];
  hp[j] = i;
}
__global__ void __launch_bounds__(kTB) doc_cnt_k(const uint64_t *__restrict__ hp, uint64_t D, uint64_t *__restrict__ cnt) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j < D) cnt[j] = hp[j + 1] - hp[j];
}

// ---------------------------------------------------------------- host side
// fm_locate's positions with what the filter found: tmp[i] = sequence or kNoSeq, slot[i] = kept before i (U + 1 entries each)
struct Kept {
  DBuf<uint64_t> uoff, pos, slot;
  DBuf<uint32_t> tmp;
  uint64_t U = 0;
};

// out_off[0..npat] (device): exclusive sums of the kept counts
template <class I>
void keep_hits(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint64_t *sp, const uint64_t *ep, const uint64_t *first,
               uint64_t max_occ, uint64_t *out_off, Kept &k) {
  pfp_ctx *c = f.c;
  k.uoff.alloc(c, npat + 1);
  fm_locate(f, npat, sp, ep, first, max_occ, k.uoff.p, nullptr);
  const uint64_t U = k.U = read_scalar(c, k.uoff.p + npat);
  if (!U) {
    PFP_HIP(hipMemsetAsync(out_off, 0, (npat + 1) * sizeof(uint64_t), c->stream));
    return;
  }
  k.pos.alloc(c, U);
  fm_locate(f, npat, sp, ep, first, max_occ, k.uoff.p, k.pos.p);
  k.tmp.alloc(c, U + 1);
  k.slot.alloc(c, U + 1);
  {
    KScope ks(c, "seq_flag", U * 20);
    seq_flag_k<I><<<gdim(cdiv(U + 1, kTB)), kTB, 0, c->stream>>>(seq_args<I>(f), pat_off, npat, k.uoff.p, k.pos.p, U, k.tmp.p);
    PFP_HIP(hipGetLastError());
  }
  exclusive_count_ne_u32(c, k.tmp.p, kNoSeq, k.slot.p, U + 1);
  gather_off_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(k.uoff.p, npat, k.slot.p, U, out_off);
  PFP_HIP(hipGetLastError());
}

template <class I>
void scatter_hits(FmIndex &f, const Kept &k, uint32_t *seq, uint64_t *off) {
  if (!k.U) return;
  pfp_ctx *c = f.c;
  KScope ks(c, "seq_scatter", k.U * 12 + k.U * (off ? 20 : 4));
  seq_scatter_k<I><<<gdim(cdiv(k.U, kTB)), kTB, 0, c->stream>>>(seq_args<I>(f), k.pos.p, k.U, k.tmp.p, k.slot.p, seq, off);
  PFP_HIP(hipGetLastError());
}

void require_seqs(const FmIndex &f) {
  PFP_REQUIRE(f.nseq, PFP_EINVAL, "this index has no sequence table: give it one with pfp_fm_set_seqs (bigbwt -f --seqs writes it)");
}

// the outputs once their number D is known: the caller's buffers, or buffers allocated here
void doc_out_ready(pfp_ctx *c, DocOut &o, uint64_t D) {
  if (!o.own_doc) return;
  o.own_doc->alloc(c, D);
  o.own_cnt->alloc(c, D);
  o.doc = o.own_doc->p; o.cnt = o.own_cnt->p;
}

// sq: the K kept hits' sequence numbers, pattern p's at hoff[p] .. hoff[p+1]
void doc_hist(FmIndex &f, const uint32_t *sq, const uint64_t *hoff, uint64_t npat, uint64_t *doc_off, DocOut &o) {
  pfp_ctx *c = f.c;
  const uint64_t chunk = budget_from_env(kDocChunk), nseq = f.nseq;   // (tests: a small bound splits the patterns of small inputs)
  DBuf<uint64_t> nchunk(c, npat + 1), isrow(c, npat + 1), chunk_off(c, npat + 1), row_of(c, npat + 1), ndoc(c, npat + 1);
  doc_plan_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(hoff, npat, chunk, nchunk.p, isrow.p);
  PFP_HIP(hipGetLastError());
  exclusive_sum_u64(c, nchunk.p, chunk_off.p, npat + 1);
  exclusive_sum_u64(c, isrow.p, row_of.p, npat + 1);
  nchunk.release();
  const uint64_t C = read_scalar(c, chunk_off.p + npat), R = read_scalar(c, row_of.p + npat);
  DBuf<unsigned long long> rows(c, R * nseq);
  DBuf<uint64_t> rowpat(c, R);
  if (R) {
    rows.zero();
    doc_rowpat_k<<<gdim(cdiv(npat, kTB)), kTB, 0, c->stream>>>(isrow.p, row_of.p, npat, rowpat.p);
    PFP_HIP(hipGetLastError());
  }
  ndoc.zero();
  if (C) {
    KScope ks(c, "doc_hist", C * nseq * 8);
    doc_hist_k<false><<<gdim(C), kTB, 0, c->stream>>>(sq, hoff, npat, chunk_off.p, C, chunk, nseq, row_of.p, rows.p, ndoc.p, nullptr, nullptr, nullptr);
    PFP_HIP(hipGetLastError());
    if (R) {
      doc_rows_k<false><<<gdim(R), kTB, 0, c->stream>>>(rows.p, rowpat.p, R, nseq, ndoc.p, nullptr, nullptr, nullptr);
      PFP_HIP(hipGetLastError());
    }
  }
  exclusive_sum_u64(c, ndoc.p, doc_off, npat + 1);
  if (o.own_doc) doc_out_ready(c, o, read_scalar(c, doc_off + npat));
  uint32_t *doc = o.doc;
  uint64_t *cnt = o.cnt;
  if (!doc || !C) return;
  KScope ks(c, "doc_hist", C * nseq * 8);
  doc_hist_k<true><<<gdim(C), kTB, 0, c->stream>>>(sq, hoff, npat, chunk_off.p, C, chunk, nseq, row_of.p, rows.p, ndoc.p, doc_off, doc, cnt);
  PFP_HIP(hipGetLastError());
  if (R) {
    doc_rows_k<true><<<gdim(R), kTB, 0, c->stream>>>(rows.p, rowpat.p, R, nseq, ndoc.p, doc_off, doc, cnt);
    PFP_HIP(hipGetLastError());
  }
}

void doc_sort(FmIndex &f, DBuf<uint32_t> &sq, uint64_t K, const uint64_t *hoff, uint64_t npat, uint64_t *doc_off, DocOut &o) {
  pfp_ctx *c = f.c;
  PFP_REQUIRE(K < 0xFFFFFFFFull, PFP_ELIMIT, "document listing over more than 4096 sequences sorts the kept hits of a call in segments: " +
                                                 std::to_string(K) + " of them, the limit is 2^32 - 2 (fewer patterns per call)");
  DBuf<uint32_t> sorted(c, K), sb(c, npat), se(c, npat), head(c, K + 1);
  head.zero();
  seg_bounds_k<uint32_t><<<gdim(cdiv(npat, kTB)), kTB, 0, c->stream>>>(hoff, npat, nullptr, sb.p, se.p, head.p, nullptr, 0);   // (head: a first hit starts a run)
  PFP_HIP(hipGetLastError());
  segsort_keys_u32(c, sq.p, sorted.p, K, npat, sb.p, se.p, 0, bits_for(f.nseq - 1));
  sq.release(); sb.release(); se.release();
  doc_heads_k<<<gdim(cdiv(K, kTB)), kTB, 0, c->stream>>>(sorted.p, K, head.p);
  PFP_HIP(hipGetLastError());
  DBuf<uint64_t> hs(c, K + 1);
  exclusive_sum_u32_u64(c, head.p, hs.p, K + 1);
  gather_off_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(hoff, npat, hs.p, K, doc_off);
  PFP_HIP(hipGetLastError());
  if (!o.doc && !o.own_doc) return;
  const uint64_t D = read_scalar(c, hs.p + K);
  doc_out_ready(c, o, D);
  uint32_t *doc = o.doc;
  uint64_t *cnt = o.cnt;
  DBuf<uint64_t> hp(c, D + 1);
  KScope ks(c, "doc_runs", K * 16 + D * 28);
  doc_runs_k<<<gdim(cdiv(K + 1, kTB)), kTB, 0, c->stream>>>(sorted.p, K, head.p, hs.p, doc, hp.p);
  PFP_HIP(hipGetLastError());
  doc_cnt_k<<<gdim(cdiv(D, kTB)), kTB, 0, c->stream>>>(hp.p, D, cnt);
  PFP_HIP(hipGetLastError());
}

template <class I>
void doclist_t(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint64_t *sp, const uint64_t *ep, const uint64_t *first,
               uint64_t *doc_off, DocOut &o) {
  pfp_ctx *c = f.c;
  DBuf<uint64_t> hoff(c, npat + 1);
  DBuf<uint32_t> sq;
  uint64_t K = 0;
  {
    Kept k;
    keep_hits<I>(f, pat_off, npat, sp, ep, first, 0, hoff.p, k);
    if (k.U) K = read_scalar(c, hoff.p + npat);
    sq.alloc(c, K);
    if (K) scatter_hits<I>(f, k, sq.p, nullptr);
  }                                                     // (the positions and the scan go back before the second stage allocates)
  if (!K) {
    PFP_HIP(hipMemsetAsync(doc_off, 0, (npat + 1) * sizeof(uint64_t), c->stream));
    doc_out_ready(c, o, 0);
    return;
  }
  if (f.nseq <= kDocLds) doc_hist(f, sq.p, hoff.p, npat, doc_off, o);
  else doc_sort(f, sq, K, hoff.p, npat, doc_off, o);
}

template <class I>
void set_seqs_t(FmIndex &f, const uint64_t *starts, uint64_t nseq) {
  pfp_ctx *c = f.c;
  const uint64_t n = f.n1 - 1;
  std::vector<I> h(nseq + 1);
  for (uint64_t k = 0; k <= nseq; k++) h[k] = (I)starts[k];
  DBuf<uint8_t> d_start(c, (nseq + 1) * sizeof(I));
  h2d(c, as<I>(d_start), h.data(), nseq + 1);
  // about one start per bucket
  const int shift = std::max(0, bits_for(f.n1) - bits_for(nseq + 1));
  const uint64_t nbk = (n >> shift) + 1;
  DBuf<uint32_t> d_dir(c, nbk + 1);
  {
    KScope ks(c, "seq_dir", (nbk + 1) * 4 * 8);
    bucket_dir_k<I, uint32_t><<<gdim(cdiv(nbk + 1, kTB)), kTB, 0, c->stream>>>(as<I>(d_start), nseq + 1, nbk, shift, d_dir.p);
    PFP_HIP(hipGetLastError());
  }
  sync(c);                                              // (h is read until here; a failure above leaves the old table in place)
  f.seq_start = std::move(d_start);
  f.seq_dir = std::move(d_dir);
  f.nseq = nseq; f.seq_nbk = nbk; f.seq_shift = shift;
}

}  // namespace

void fm_set_seqs(FmIndex &f, const uint64_t *starts, uint64_t nseq) {
  const uint64_t n = f.n1 - 1;
  PFP_REQUIRE(starts, PFP_EINVAL, "no sequence table");
  PFP_REQUIRE(nseq >= 1 && nseq < 0xFFFFFFFFull, PFP_EINVAL, "a sequence table holds 1 .. 2^32 - 2 sequences, not " + std::to_string(nseq));
  PFP_REQUIRE(starts[0] == 0, PFP_EINVAL, "sequence table entry 0 is " + std::to_string(starts[0]) + ": the first sequence starts at 0");
  for (uint64_t k = 1; k <= nseq; k++)
    PFP_REQUIRE(starts[k] >= starts[k - 1], PFP_EINVAL, "sequence table entry " + std::to_string(k) + " is " + std::to_string(starts[k]) +
                                                            ", below entry " + std::to_string(k - 1) + ": the starts do not decrease");
  PFP_REQUIRE(starts[nseq] == n, PFP_EINVAL, "sequence table entry " + std::to_string(nseq) + " (the last) is " + std::to_string(starts[nseq]) +
                                                 ": it is the text's length, " + std::to_string(n));
  by_width(f, [&](auto w) { set_seqs_t<decltype(w)>(f, starts, nseq); });
}

void fm_seqmap(FmIndex &f, const uint64_t *pos, uint64_t count, uint32_t *seq, uint64_t *off) {
  pfp_ctx *c = f.c;
  require_seqs(f);
  if (!count || (!seq && !off)) return;
  KScope ks(c, "seq_map", count * 20);
  by_width(f, [&](auto w) { seq_map_k<decltype(w)><<<gdim(cdiv(count, kTB)), kTB, 0, c->stream>>>(seq_args<decltype(w)>(f), pos, count, seq, off); });
  PFP_HIP(hipGetLastError());
}

void fm_locate_seqs(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint64_t *sp, const uint64_t *ep, const uint64_t *first,
                    uint64_t max_occ, uint64_t *out_off, uint32_t *seq, uint64_t *off) {
  require_seqs(f);
  PFP_REQUIRE(!seq == !off, PFP_EINVAL, "the kept hits come as a pair: sequences and offsets, or neither");
  if (!npat) {
    PFP_HIP(hipMemsetAsync(out_off, 0, sizeof(uint64_t), f.c->stream));
    return;
  }
  Kept k;
  by_width(f, [&](auto w) {
    keep_hits<decltype(w)>(f, pat_off, npat, sp, ep, first, max_occ, out_off, k);
    if (seq) scatter_hits<decltype(w)>(f, k, seq, off);
  });
}

void fm_doclist(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint64_t *sp, const uint64_t *ep, const uint64_t *first,
                uint64_t *doc_off, DocOut &o) {
  require_seqs(f);
  PFP_REQUIRE(!o.doc == !o.cnt, PFP_EINVAL, "the documents come as a pair: sequences and counts, or neither");
  if (!npat) {
    PFP_HIP(hipMemsetAsync(doc_off, 0, sizeof(uint64_t), f.c->stream));
    doc_out_ready(f.c, o, 0);
    return;
  }
  by_width(f, [&](auto w) { doclist_t<decltype(w)>(f, pat_off, npat, sp, ep, first, doc_off, o); });
}

}  // namespace pfp
