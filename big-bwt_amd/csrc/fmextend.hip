// fmextend.hip -- seed-and-extend over an FmIndex with text: the best alignment of a whole pattern to the text near a diagonal under
// unit-cost edit distance, and the composite that takes a pattern's MEMs as its diagonals.  The reference has no counterpart;
// include/pfpgpu.h, "Extending seeds", states the definitions (candidate, window, result, alignments of a pattern).
//
//   The band.  Cell (i, j) of the DP is pattern prefix i against a text span that ends at j.  An alignment of cost <= k that starts
//   at s >= lo and ends at e <= hi has s <= e - m + k, and its path leaves the diagonal j - i = s by at most k: every cell of it
//   lies on the diagonals lo - k .. hi - m + 2k, at most 5k + 1 of them because hi - lo <= m + 2k.  Cells off the band count as
//   "more than k"; inside it every value <= k is exact, larger ones are only known to be larger.  Values are capped at k + 1.
//   The layout.  One group of 16 lanes per candidate, CPL consecutive diagonals per lane (16 CPL >= 5k + 1: CPL is a template
//   parameter chosen from k, so a lane's cells and its text bytes stay in registers), one pattern row per step.  Cell c of row i is
//   column x = i + c, where column x is text position org + (x - k) and the columns k .. L + k are the window.  A row takes the
//   diagonal and the vertical move from the row above (the neighbour lane's first cell comes by one shuffle), then the horizontal
//   moves inside the row: a min-plus scan, inside the lane first and then across the group.  A lane's text bytes slide by one
//   column per row; the byte that enters at the band's right edge and the row's pattern byte were read 16 rows at a time, one per
//   lane.  A column outside the window is never read: its cells hold k + 1 below the window, and above it they feed only one another.
//   Two passes.  Forward with a free start: row 0 is 0 across the window, and the last row gives d* and the smallest e.  Backward
//   from e with a fixed end: the reversed pattern against the reversed T[lo .. e), row 0 is the column number, band -k .. k, and the
//   first column of the last row that holds d* is the largest s.  A row that is k + 1 everywhere ends the candidate (checked every
//   16 rows).  k = 0 is a compare of 16 bytes per lane and step.
//   The composite.  fm_ms / fm_ms_thr -> fm_mems -> one candidate per MEM (pattern by binary search, diagonal pos - i) -> the
//   library's segmented sort of the diagonals inside every pattern, a scan over "differs from its predecessor", a scatter: the
//   distinct diagonals -> fm_extend -> keys d : s : e - s (6 + 40 + 17 bits, all ones for "no alignment") -> the same sort, scan
//   and scatter over the keys, with the cap of max_aln per pattern in between.
//   The pass itself (band_pass) is in fmband.hpp: fmwindow.hip takes its starts from the backward form.
// Bounds: every loop is bounded by m, k or a directory's size; text is read at positions lo .. hi - 1 only and patterns inside
// their offsets; outputs are written at the candidate's own index, or below the total the scan gave.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"
#include "fmband.hpp"

namespace pfp {

namespace {

constexpr int64_t kDiagMax = 1ll << 62;                 // diagonals are clamped to +-2^62: far outside any text, and sums stay in range
constexpr uint64_t kDiagBias = 1ull << 17;              // a MEM's diagonal is > -2^16: biased, it is a sort key

__device__ __forceinline__ uint64_t clamp_pos(int64_t x, uint64_t n) { return x < 0 ? 0 : ((uint64_t)x > n ? n : (uint64_t)x); }

// what a candidate is about: its pattern and diagonal, or ok = false (no such pattern, decreasing offsets, a pattern too long)
struct ExtCand { uint64_t o0; int m; int64_t diag; bool ok; };
__device__ __forceinline__ ExtCand ext_cand(const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ cand_pat,
                                            const int64_t *__restrict__ cand_diag, uint64_t ci) {
  ExtCand r{0, 0, 0, false};
  const uint64_t p = cand_pat[ci];
  if (p >= npat) return r;
  const uint64_t o0 = off[p], o1 = off[p + 1];
  if (o1 < o0 || o1 - o0 > PFP_FM_EXTEND_MAX_M) return r;
  int64_t d = cand_diag[ci];
  d = d < -kDiagMax ? -kDiagMax : (d > kDiagMax ? kDiagMax : d);
  return ExtCand{o0, (int)(o1 - o0), d, true};
}

// one group of 16 lanes per candidate, 1 <= k <= PFP_FM_EXTEND_MAX_K, 16 CPL >= 5k + 1
template <int CPL>
__global__ void __launch_bounds__(kTB) fm_extend_k(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ pat,
                                                   const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ cand_pat,
                                                   const int64_t *__restrict__ cand_diag, uint64_t ncand, int k, uint8_t *__restrict__ dist,
                                                   uint64_t *__restrict__ start, uint64_t *__restrict__ end) {
  const int gl = threadIdx.x & 15, base = gl * CPL;
  const uint64_t ci = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (ci >= ncand) return;                              // (whole groups leave together: the shuffles stay inside groups)
  const ExtCand cd = ext_cand(off, npat, cand_pat, cand_diag, ci);
  uint64_t d = kExtNone, s = kExtNoPos, e = kExtNoPos;
  if (cd.ok) {                                          // (every lane of the group holds the same state)
    const int m = cd.m;
    const uint64_t lo = clamp_pos(cd.diag - k, n), hi = clamp_pos(cd.diag + m + k, n);
    const int L = (int)(hi - lo);                       // (<= m + 2k)
    int cur[CPL];
    if (L + k >= m && band_pass<CPL, false>(text, pat + cd.o0, m, lo, L, k, gl, cur)) {
      uint64_t best = ~0ull;                            // the smallest value of the last row inside the window, at its first column
#pragma unroll
      for (int q = 0; q < CPL; q++) {
        const int x = m + base + q;
        if (x >= k && x <= L + k && cur[q] <= k) best = min(best, (uint64_t)cur[q] << 32 | (uint32_t)x);
      }
      best = gmin16(best);
      if (best != ~0ull) {
        const int dstar = (int)(best >> 32);
        const uint64_t ee = lo + (uint64_t)((int)(uint32_t)best - k);
        const int L2 = (int)(ee - lo);
        band_pass<CPL, true>(text, pat + cd.o0, m, ee, L2, k, gl, cur);
        uint64_t first = ~0ull;                         // the first column of the last row that holds d*: the shortest span
#pragma unroll
        for (int q = 0; q < CPL; q++) {
          const int x = m + base + q;
          if (x >= k && x <= L2 + k && cur[q] == dstar) first = min(first, (uint64_t)x);
        }
        first = gmin16(first);
        if (first != ~0ull) { d = (uint64_t)dstar; e = ee; s = ee - (first - (uint64_t)k); }
      }
    }
  }
  if (gl == 0) { dist[ci] = (uint8_t)d; start[ci] = s; end[ci] = e; }
}

// k = 0: the pattern at its diagonal or nothing.  One group per candidate, 16 bytes per lane and step
__global__ void __launch_bounds__(kTB) fm_extend0_k(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ pat,
                                                    const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ cand_pat,
                                                    const int64_t *__restrict__ cand_diag, uint64_t ncand, uint8_t *__restrict__ dist,
                                                    uint64_t *__restrict__ start, uint64_t *__restrict__ end) {
  const int gl = threadIdx.x & 15;
  const uint64_t ci = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (ci >= ncand) return;
  const ExtCand cd = ext_cand(off, npat, cand_pat, cand_diag, ci);
  uint64_t d = kExtNone, s = kExtNoPos, e = kExtNoPos;
  if (cd.ok) {
    const uint64_t m = (uint64_t)cd.m, lo = clamp_pos(cd.diag, n), hi = clamp_pos(cd.diag + cd.m, n);
    if (hi - lo == m) {                                 // (with m > 0: the window is not clipped, lo is the diagonal)
      const uint8_t *P = pat + cd.o0, *T = text + lo;
      uint64_t bad = 0;
      for (uint64_t t = 16 * (uint64_t)gl; t < m; t += 256) {
        if (t + 16 <= m) {
          const uint4 a = ld16u(P + t), b = ld16u(T + t);
          bad |= (a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w) | zero_bytes(a.x) | zero_bytes(a.y) | zero_bytes(a.z) | zero_bytes(a.w);
        } else {
          for (uint64_t u = t; u < m; u++) bad |= (uint64_t)(P[u] != T[u] || !P[u]);
        }
      }
      if (!gsum16(bad != 0)) { d = 0; s = lo; e = hi; }
    }
  }
  if (gl == 0) { dist[ci] = (uint8_t)d; start[ci] = s; end[ci] = e; }
}

// ctr[0] += patterns longer than PFP_FM_EXTEND_MAX_M
__global__ void __launch_bounds__(kTB) ext_long_k(const uint64_t *__restrict__ off, uint64_t npat, unsigned long long *__restrict__ ctr) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p < npat && off[p + 1] > off[p] && off[p + 1] - off[p] > PFP_FM_EXTEND_MAX_M) atomicAdd(ctr, 1ull);
}

// one candidate per MEM: its pattern (mem_off: the exclusive sums of the patterns' MEM counts) and its diagonal pos - i, biased
__global__ void __launch_bounds__(kTB) aln_cand_k(uint64_t M, const uint64_t *__restrict__ mem_off, uint64_t npat, const uint64_t *__restrict__ mem,
                                                  uint32_t *__restrict__ cpat, uint64_t *__restrict__ key) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j >= M) return;
  cpat[j] = (uint32_t)last_le(mem_off, npat, j);
  key[j] = mem[3 * j + 2] - mem[3 * j] + kDiagBias;
}

// flag[j] = entry j of the sorted keys is the first of its value in its pattern, and not `none`; flag[count] = 0
__global__ void __launch_bounds__(kTB) aln_mark_k(uint64_t count, const uint64_t *__restrict__ key, const uint32_t *__restrict__ cpat, uint64_t none,
                                                  uint64_t *__restrict__ flag) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j > count) return;
  flag[j] = j < count && key[j] != none && (j == 0 || cpat[j] != cpat[j - 1] || key[j] != key[j - 1]);
}

// the distinct candidates: entry idx[j] of the outputs for every flagged j
__global__ void __launch_bounds__(kTB) aln_uniq_k(uint64_t M, const uint64_t *__restrict__ flag, const uint64_t *__restrict__ idx,
                                                  const uint64_t *__restrict__ key, const uint32_t *__restrict__ cpat, uint64_t C,
                                                  uint32_t *__restrict__ upat, int64_t *__restrict__ udiag) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j >= M || !flag[j] || idx[j] >= C) return;
  upat[idx[j]] = cpat[j];
  udiag[idx[j]] = (int64_t)(key[j] - kDiagBias);
}

// key[c] = d : s : e - s in 6 + 40 + 17 bits, all ones for "no alignment"
__global__ void __launch_bounds__(kTB) aln_key_k(uint64_t C, const uint8_t *__restrict__ dist, const uint64_t *__restrict__ start,
                                                 const uint64_t *__restrict__ end, uint64_t *__restrict__ key) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j >= C) return;
  const uint64_t d = dist[j], s = start[j], span = end[j] - start[j];
  // (a result always fits: s <= n < 2^40, the limit of the 5-byte formats that fm_build enforces, and span <= m + 2k < 2^17 by
  // PFP_FM_EXTEND_MAX_M and PFP_FM_EXTEND_MAX_K; the two tests only keep a value that broke these from spilling into d's bits)
  key[j] = d <= PFP_FM_EXTEND_MAX_K && s < (1ull << 40) && span < (1ull << 17) ? d << 57 | s << 17 | span : ~0ull;
}

// the cap: a flagged entry stays when fewer than max_aln flagged entries of its pattern precede it (idx: exclusive sums of flag)
__global__ void __launch_bounds__(kTB) aln_cap_k(uint64_t C, const uint64_t *__restrict__ idx, const uint32_t *__restrict__ cpat,
                                                 const uint32_t *__restrict__ sb, uint64_t npat, uint64_t max_aln, uint64_t *__restrict__ flag) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j >= C || !flag[j]) return;
  const uint64_t p = cpat[j], b = p < npat ? sb[p] : 0;
  if (idx[j] - idx[b < C ? b : C] >= max_aln) flag[j] = 0;
}

// aln_off[p] = kept entries before pattern p's first, p = 0 .. npat.  (Not gather_off_k: the place comes from the sort's 32-bit
// bounds, which have no entry npat.)
__global__ void __launch_bounds__(kTB) aln_off_k(uint64_t npat, const uint32_t *__restrict__ sb, uint64_t C, const uint64_t *__restrict__ idx,
                                                 uint64_t *__restrict__ aln_off) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p > npat) return;
  const uint64_t b = p < npat ? sb[p] : C;
  aln_off[p] = idx[b < C ? b : C];
}

__global__ void __launch_bounds__(kTB) aln_out_k(uint64_t C, const uint64_t *__restrict__ flag, const uint64_t *__restrict__ idx,
                                                 const uint64_t *__restrict__ key, uint64_t A, uint64_t *__restrict__ start, uint64_t *__restrict__ end,
                                                 uint8_t *__restrict__ dist) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j >= C || !flag[j] || idx[j] >= A) return;
  const uint64_t s = key[j] >> 17 & ((1ull << 40) - 1);
  start[idx[j]] = s;
  end[idx[j]] = s + (key[j] & ((1ull << 17) - 1));
  dist[idx[j]] = (uint8_t)(key[j] >> 57);
}

// sorts the `count` keys inside every pattern's segment and flags the first entry of every distinct key other than `none`: skey,
// flag and idx (its exclusive sums, count + 1 entries each) are allocated here.  cpat[j] = the pattern of entry j, before and after
void sort_and_mark(pfp_ctx *c, const uint64_t *key, const uint32_t *cpat, uint64_t count, uint64_t npat, const uint32_t *sb, const uint32_t *se,
                   int bits, uint64_t none, DBuf<uint64_t> &skey, DBuf<uint64_t> &flag, DBuf<uint64_t> &idx) {
  skey.alloc(c, count);
  flag.alloc(c, count + 1);
  idx.alloc(c, count + 1);
  {
    DBuf<uint32_t> spat(c, count);                      // (the values travel inside their segments: they come out as they went in)
    segsort_pairs_u64_u32(c, key, skey.p, cpat, spat.p, count, npat, sb, se, 0, bits);
  }
  aln_mark_k<<<gdim(cdiv(count + 1, kTB)), kTB, 0, c->stream>>>(count, skey.p, cpat, none, flag.p);
  PFP_HIP(hipGetLastError());
  exclusive_sum_u64(c, flag.p, idx.p, count + 1);
}

template <int CPL>
void launch_extend(pfp_ctx *c, const uint8_t *text, uint64_t n, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat,
                   const int64_t *cand_diag, uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end) {
  fm_extend_k<CPL><<<gdim(cdiv(ncand, kTB / 16)), kTB, 0, c->stream>>>(text, n, pat, pat_off, npat, cand_pat, cand_diag, ncand, k, dist, start, end);
}

}  // namespace

void fm_extend_check(const FmIndex &f, int k) {
  PFP_REQUIRE(k >= 0 && k <= PFP_FM_EXTEND_MAX_K, PFP_EINVAL, "k = " + std::to_string(k) + ": the edit budget is 0 .. " +
                                                                   std::to_string(PFP_FM_EXTEND_MAX_K) + " (PFP_FM_EXTEND_MAX_K)");
  PFP_REQUIRE(f.has_text, PFP_EINVAL, "extending seeds needs the text: build the index with pfp_fm_build_ms_dev / pfp_fm_build_ms_files");
}

void fm_align_check(const FmIndex &f, int k, uint64_t min_seed, bool thresholds) {
  fm_extend_check(f, k);
  PFP_REQUIRE(min_seed >= 1, PFP_EINVAL, "min_seed = 0: a seed is a maximal exact match of at least 1 byte");
  PFP_REQUIRE(!thresholds || f.has_thr, PFP_EINVAL, "this index has no thresholds: add them with pfp_fm_thresholds_dev / pfp_fm_thresholds_files");
}

void fm_extend_check_patterns(FmIndex &f, const uint64_t *pat_off, uint64_t npat) {
  pfp_ctx *c = f.c;
  if (!npat) return;
  DBuf<uint64_t> ctr(c, 1);
  ctr.zero();
  ext_long_k<<<gdim(cdiv(npat, kTB)), kTB, 0, c->stream>>>(pat_off, npat, (unsigned long long *)ctr.p);
  PFP_HIP(hipGetLastError());
  const uint64_t bad = read_scalar(c, ctr.p);
  PFP_REQUIRE(!bad, PFP_ELIMIT, std::to_string(bad) + " patterns of more than " + std::to_string(PFP_FM_EXTEND_MAX_M) +
                                    " bytes (PFP_FM_EXTEND_MAX_M): the band's columns are counted in 32 bits and a span in 17");
}

// the launch alone: the callers have checked k, the index and the patterns' lengths
static void extend_launch(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat, const int64_t *cand_diag,
                          uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end) {
  pfp_ctx *c = f.c;
  if (!ncand) return;
  const uint8_t *text = f.text.p;
  const uint64_t n = f.n1 - 1;
  KScope ks(c, "fm_extend", 0);
  if (k == 0)
    fm_extend0_k<<<gdim(cdiv(ncand, kTB / 16)), kTB, 0, c->stream>>>(text, n, pat, pat_off, npat, cand_pat, cand_diag, ncand, dist, start, end);
  else if (5 * k + 1 <= 16) launch_extend<1>(c, text, n, pat, pat_off, npat, cand_pat, cand_diag, ncand, k, dist, start, end);
  else if (5 * k + 1 <= 32) launch_extend<2>(c, text, n, pat, pat_off, npat, cand_pat, cand_diag, ncand, k, dist, start, end);
  else if (5 * k + 1 <= 48) launch_extend<3>(c, text, n, pat, pat_off, npat, cand_pat, cand_diag, ncand, k, dist, start, end);
  else if (5 * k + 1 <= 96) launch_extend<6>(c, text, n, pat, pat_off, npat, cand_pat, cand_diag, ncand, k, dist, start, end);
  else launch_extend<11>(c, text, n, pat, pat_off, npat, cand_pat, cand_diag, ncand, k, dist, start, end);
  PFP_HIP(hipGetLastError());
}

void fm_extend(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat, const int64_t *cand_diag,
               uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end) {
  fm_extend_check(f, k);
  fm_extend_check_patterns(f, pat_off, npat);
  extend_launch(f, pat, pat_off, npat, cand_pat, cand_diag, ncand, k, dist, start, end);
}

void fm_align_seeds(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln,
                    const uint32_t *len, const uint64_t *pos, const uint64_t *mem_off, uint64_t M, uint64_t *aln_off, AlnKeys &out) {
  pfp_ctx *c = f.c;
  fm_align_check(f, k, min_seed, false);
  require_sortable(M, "seeds");
  out.C = out.total = 0;
  if (!M || !npat) {
    PFP_HIP(hipMemsetAsync(aln_off, 0, (npat + 1) * sizeof(uint64_t), c->stream));
    sync(c);
    return;
  }
  // the distinct diagonals of every pattern
  DBuf<uint32_t> sb(c, npat), se(c, npat), upat;
  DBuf<int64_t> udiag;
  uint64_t C = 0;
  {
    DBuf<uint64_t> mem(c, 3 * M), key(c, M), skey, flag, idx;
    DBuf<uint32_t> cpat(c, M);
    fm_mem_triples(f, pat_off, npat, len, pos, min_seed, mem_off, mem.p);
    KScope ks(c, "fm_align_seeds", 0);
    aln_cand_k<<<gdim(cdiv(M, kTB)), kTB, 0, c->stream>>>(M, mem_off, npat, mem.p, cpat.p, key.p);
    PFP_HIP(hipGetLastError());
    mem.release();
    seg_bounds_k<uint32_t><<<gdim(cdiv(npat, kTB)), kTB, 0, c->stream>>>(mem_off, npat, nullptr, sb.p, se.p, nullptr, nullptr, 0);
    PFP_HIP(hipGetLastError());
    sort_and_mark(c, key.p, cpat.p, M, npat, sb.p, se.p, bits_for(f.n1 + 2 * kDiagBias), ~0ull, skey, flag, idx);
    C = read_scalar(c, idx.p + M);
    upat.alloc(c, C);
    udiag.alloc(c, C);
    aln_uniq_k<<<gdim(cdiv(M, kTB)), kTB, 0, c->stream>>>(M, flag.p, idx.p, skey.p, cpat.p, C, upat.p, udiag.p);
    PFP_HIP(hipGetLastError());
    seg_bounds_k<uint32_t><<<gdim(cdiv(npat, kTB)), kTB, 0, c->stream>>>(mem_off, npat, idx.p, sb.p, se.p, nullptr, nullptr, 0);
    PFP_HIP(hipGetLastError());
    sync(c);                                            // (the seeds' arrays go back when this block ends)
  }
  DBuf<uint64_t> key(c, C), c_start(c, C), c_end(c, C);
  DBuf<uint8_t> c_dist(c, C);
  extend_launch(f, pat, pat_off, npat, upat.p, udiag.p, C, k, c_dist.p, c_start.p, c_end.p);
  KScope ks(c, "fm_align_sort", 0);
  aln_key_k<<<gdim(cdiv(C, kTB)), kTB, 0, c->stream>>>(C, c_dist.p, c_start.p, c_end.p, key.p);
  PFP_HIP(hipGetLastError());
  c_start.release(); c_end.release(); c_dist.release();
  sort_and_mark(c, key.p, upat.p, C, npat, sb.p, se.p, 64, ~0ull, out.skey, out.flag, out.idx);
  if (max_aln) {
    aln_cap_k<<<gdim(cdiv(C, kTB)), kTB, 0, c->stream>>>(C, out.idx.p, upat.p, sb.p, npat, max_aln, out.flag.p);
    PFP_HIP(hipGetLastError());
    exclusive_sum_u64(c, out.flag.p, out.idx.p, C + 1);
  }
  aln_off_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(npat, sb.p, C, out.idx.p, aln_off);
  PFP_HIP(hipGetLastError());
  out.C = C;
  out.total = read_scalar(c, out.idx.p + C);            // (syncs: the candidates' arrays go back when this returns)
}

void fm_align_write(FmIndex &f, const AlnKeys &keys, uint64_t *start, uint64_t *end, uint8_t *dist) {
  pfp_ctx *c = f.c;
  if (!keys.total) return;
  KScope ks(c, "fm_align_sort", 0);
  aln_out_k<<<gdim(cdiv(keys.C, kTB)), kTB, 0, c->stream>>>(keys.C, keys.flag.p, keys.idx.p, keys.skey.p, keys.total, start, end, dist);
  PFP_HIP(hipGetLastError());
}

void fm_align_keys(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln, bool thresholds,
                   uint64_t *aln_off, AlnKeys &keys) {
  pfp_ctx *c = f.c;
  fm_align_check(f, k, min_seed, thresholds);
  fm_extend_check_patterns(f, pat_off, npat);
  const uint64_t bytes = npat ? read_scalar(c, pat_off + npat) : 0;
  DBuf<uint32_t> len(c, bytes + 1);
  DBuf<uint64_t> pos(c, bytes + 1), mem_off(c, npat + 1);
  if (thresholds) fm_ms_thr(f, pat, pat_off, npat, len.p, pos.p);
  else fm_ms(f, pat, pat_off, npat, len.p, pos.p);
  fm_mems(f, pat_off, npat, len.p, pos.p, min_seed, mem_off.p, nullptr);
  const uint64_t M = read_scalar(c, mem_off.p + npat);
  fm_align_seeds(f, pat, pat_off, npat, min_seed, k, max_aln, len.p, pos.p, mem_off.p, M, aln_off, keys);
}

void fm_align(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln, bool thresholds,
              uint64_t *aln_off, uint64_t *start, uint64_t *end, uint8_t *dist) {
  AlnKeys keys;
  fm_align_keys(f, pat, pat_off, npat, min_seed, k, max_aln, thresholds, aln_off, keys);
  if (start) fm_align_write(f, keys, start, end, dist);
  sync(f.c);                                            // (the keys go back when this returns)
}

}  // namespace pfp
