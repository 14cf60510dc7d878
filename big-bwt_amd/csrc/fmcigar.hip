// fmcigar.hip -- the edit script (CIGAR) of alignments that fm_extend / fm_align found: one more banded pass over exactly P against
// T[s .. e), which records the operation every cell takes, and a walk back along the records.  The reference has no counterpart;
// include/pfpgpu.h, "Edit scripts", states the definitions (operations, the script of (P, s, e), the result, "no script").
//
//   The band.  Cell (i, j) of the DP is pattern prefix i against T[s .. s + j).  Every cell of an optimal path of cost <= k has
//   |j - i| <= D[i][j] <= k: the band is the diagonals j - i = -k .. k.  Cell c of row i is column j = i + c - k.  Cells off the
//   band or with j < 0 count as "more than k"; inside the band every value <= k is exact.  Values are capped at k + 1.
//   The layout is fmextend.hip's: one group of 16 lanes per alignment, CPL consecutive cells per lane (16 CPL >= 2k + 1: the cells
//   past 2k are further diagonals to the right, which hold k + 1), one pattern row per step, the row's horizontal moves by a
//   min-plus scan.  Row 0 is the column number.  Cells right of column L feed only one another and never read text.
//   The records.  For every cell the row loop keeps 2 bits: the operation that rules 1-4 of the definition choose there (0 '=',
//   1 'X', 2 'I', 3 'D').  16 rows make one uint32 per cell: word (i - 1) / 16 * 16 CPL + c holds row i of cell c at bits
//   2 ((i - 1) % 16).  A lane stores its CPL words every 16 rows: 4 CPL m bytes per alignment, in whole blocks of 16 rows.
//   The walk.  Lane 0 of the group goes from (m, L) to (0, 0): '=' and 'X' keep the cell, 'I' moves one cell up the band, 'D' one
//   cell down in the same row; at i = 0 the rest is one D run, at j = 0 one I run.  The '=' of one word that follow one another
//   are one step (the leading zero bits of the word say how many).  Runs come out last first, into the
//   alignment's slot of 2k + 1 words; a scan over the run counts and cig_place_k put them in order.
//   k = 0 needs no band: a compare of 16 bytes per lane and step, and the script is m '=' or nothing.
//   The scratch for the records is bounded (kCigarScratch): alignments go through in consecutive chunks whose records fit.
// Bounds: every loop is bounded by m, L or k; text is read at s .. e - 1 only and patterns inside their offsets; records are
// written inside the alignment's own words, whose number cig_words gives to the kernel that sizes them and to the one that fills
// them; the walk takes at most m + L steps, reads only words the pass wrote, and writes at most 2k + 1 runs.
#include <vector>
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"
#include "fmband.hpp"

namespace pfp {

namespace {

constexpr uint8_t kCigNone = 0xFF;
constexpr uint64_t kCigarScratch = 1ull << 30;          // bytes of records per launch: a choice (0.8 million reads of 150 bytes at k = 8)

// what an alignment is about: its pattern and its span, or ok = false (no such pattern, decreasing offsets, a pattern too long,
// s > e, e > n, or lengths that differ by more than k)
struct CigAln { uint64_t o0, s; int m, L; bool ok; };
__device__ __forceinline__ CigAln cig_aln(const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ aln_pat,
                                          const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t n, int k, uint64_t ai) {
  CigAln r{0, 0, 0, 0, false};
  const uint64_t p = aln_pat[ai];
  if (p >= npat) return r;
  const uint64_t o0 = off[p], o1 = off[p + 1];
  if (o1 < o0 || o1 - o0 > PFP_FM_EXTEND_MAX_M) return r;
  const uint64_t s = start[ai], e = end[ai], m = o1 - o0;
  if (s > e || e > n) return r;
  const uint64_t L = e - s;
  if (L > m + (uint64_t)k || m > L + (uint64_t)k) return r;
  return CigAln{o0, s, (int)m, (int)L, true};
}

// need[ai] = the words of alignment ai's records (0: it has no script), ai < naln; need[naln] = 0
__global__ void __launch_bounds__(kTB) cig_need_k(const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ aln_pat,
                                                  const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t naln, uint64_t n,
                                                  int k, uint64_t W, uint64_t *__restrict__ need) {
  const uint64_t ai = BID * kTB + threadIdx.x;
  if (ai > naln) return;
  uint64_t w = 0;
  if (ai < naln) {
    const CigAln a = cig_aln(off, npat, aln_pat, start, end, n, k, ai);
    if (a.ok) w = cig_words((uint64_t)a.m, W);
  }
  need[ai] = w;
}

// the m rows of the band (see the head of the file): T = the span's first byte, P = the pattern's.  cur = the last row's cells,
// cell q of this lane is c = gl CPL + q; ops gets the records.  false: a whole row exceeded k (the records stop there)
template <int CPL>
__device__ __forceinline__ bool cig_forward(const uint8_t *__restrict__ T, const uint8_t *__restrict__ P, int m, int L, int k, int gl,
                                            int (&cur)[CPL], uint32_t *ops) {
  const int inf = k + 1, base = gl * CPL;
  // the text byte of column x = j + k (columns outside 1 .. L are not read; no cell that counts uses them)
  auto fetch = [&](int x) -> int {
    if (x <= k || x > L + k) return 0;
    return T[x - k - 1];
  };
  // the horizontal moves of one row: v[c] = min over c' <= c of v[c'] + (c - c'), capped
  auto scan = [&](int (&v)[CPL]) {
#pragma unroll
    for (int q = 1; q < CPL; q++) v[q] = min(v[q], v[q - 1] + 1);
    const int z = gscan16(v[CPL - 1] - base - (CPL - 1), gl, [](int x, int y) { return min(x, y); });
    int carry = __shfl_up(z, 1, 16);                    // the lanes before this one
    carry = gl ? carry + base : (1 << 20);
#pragma unroll
    for (int q = 0; q < CPL; q++) v[q] = min(min(v[q], carry + q), inf);
  };
  int tb[CPL];
#pragma unroll
  for (int q = 0; q < CPL; q++) {
    const int x = base + q;
    cur[q] = x == k ? 0 : inf;                          // row 0: cell c is column c - k, and its value is the column number
    tb[q] = fetch(1 + x);
  }
  scan(cur);
  for (int i0 = 0; i0 < m; i0 += 16) {
    // this lane's share of the block's bytes: the pattern byte of row i0 + 1 + gl (0x100 for a byte 0: it equals nothing) and the
    // text byte that enters the band's right edge after that row
    const int row = i0 + 1 + gl;
    int mine = 0x100;
    if (row <= m) {
      const int b = P[row - 1];
      mine = (b ? b : 0x100) | fetch(row + 16 * CPL) << 16;
    }
    const int rows = min(16, m - i0);
    uint32_t w[CPL];
#pragma unroll
    for (int q = 0; q < CPL; q++) w[q] = 0;
    for (int r = 0; r < rows; r++) {
      const int both = __shfl(mine, r, 16), pb = both & 0xFFFF;
      const int next = __shfl_down(cur[0] | tb[0] << 8, 1, 16);       // the neighbour's first cell and its text byte
      const int up = gl == 15 ? inf : (next & 0xFF);
      int v[CPL];
#pragma unroll
      for (int q = 0; q < CPL; q++) v[q] = min(cur[q] + (tb[q] != pb), (q + 1 < CPL ? cur[q + 1] : up) + 1);
      scan(v);
#pragma unroll
      for (int q = 0; q < CPL; q++) {                   // rules 1-4 (a cell above k may record anything: no optimal path visits it)
        const int above = q + 1 < CPL ? cur[q + 1] : up;
        const uint32_t op = tb[q] == pb ? 0u : cur[q] == v[q] - 1 ? 1u : above == v[q] - 1 ? 2u : 3u;
        w[q] |= op << (2 * r);
      }
#pragma unroll
      for (int q = 0; q < CPL; q++) cur[q] = v[q];
#pragma unroll
      for (int q = 0; q + 1 < CPL; q++) tb[q] = tb[q + 1];
      tb[CPL - 1] = gl == 15 ? both >> 16 : next >> 8;
    }
#pragma unroll
    for (int q = 0; q < CPL; q++) ops[(uint64_t)(i0 >> 4) * (16 * CPL) + base + q] = w[q];
    int low = cur[0];
#pragma unroll
    for (int q = 1; q < CPL; q++) low = min(low, cur[q]);
    if (gmin16((uint64_t)low) >= (uint64_t)inf) return false;
  }
  return true;
}

// one group of 16 lanes per alignment a0 <= ai < a1, 1 <= k <= PFP_FM_EXTEND_MAX_K, 16 CPL >= 2k + 1.  soff = the exclusive sums
// of the alignments' words, sbase = soff[a0]: scratch holds the words of this launch's alignments.  slot: 2k + 1 words each
template <int CPL>
__global__ void __launch_bounds__(kTB) fm_cigar_k(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ pat,
                                                  const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ aln_pat,
                                                  const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t a0, uint64_t a1,
                                                  int k, const uint64_t *__restrict__ soff, uint64_t sbase, uint32_t *scratch,
                                                  uint8_t *__restrict__ dist, uint64_t *__restrict__ cnt, uint32_t *__restrict__ slot) {
  const int gl = threadIdx.x & 15;
  const uint64_t ai = a0 + BID * (kTB / 16) + (threadIdx.x >> 4);
  if (ai >= a1) return;                                 // (whole groups leave together: the shuffles stay inside groups)
  const CigAln a = cig_aln(off, npat, aln_pat, start, end, n, k, ai);
  uint64_t d = kCigNone;
  uint32_t runs = 0;
  if (a.ok) {                                           // (every lane of the group holds the same state)
    uint32_t *ops = scratch + (soff[ai] - sbase);
    int cur[CPL];
    if (cig_forward<CPL>(text + a.s, pat + a.o0, a.m, a.L, k, gl, cur, ops)) {
      const int c = a.L - a.m + k;                      // (m, L) is cell c of the last row, 0 <= c <= 2k
      uint64_t v = ~0ull;
#pragma unroll
      for (int q = 0; q < CPL; q++)
        if (gl * CPL + q == c) v = (uint64_t)cur[q];
      v = gmin16(v);
      if (v <= (uint64_t)k) {
        d = v;
        // the group's records, written by 16 lanes of this wave, are read by one: a fence of the block's scope orders them (a
        // device-wide one would write the L2's dirty lines - these records - back first); no other group shares their 128-byte lines
        __threadfence_block();
        if (gl == 0) runs = cig_walk(ops, 16 * CPL, a.m, a.L, c, slot + ai * (uint64_t)(2 * k + 1), (uint32_t)(2 * k + 1));
      }
    }
  }
  if (gl == 0) { dist[ai] = (uint8_t)d; cnt[ai] = runs; }
}

// k = 0: the pattern at its span or nothing.  One group per alignment, 16 bytes per lane and step; slot: 1 word each
__global__ void __launch_bounds__(kTB) fm_cigar0_k(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ pat,
                                                   const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ aln_pat,
                                                   const uint64_t *__restrict__ start, const uint64_t *__restrict__ end, uint64_t naln,
                                                   uint8_t *__restrict__ dist, uint64_t *__restrict__ cnt, uint32_t *__restrict__ slot) {
  const int gl = threadIdx.x & 15;
  const uint64_t ai = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (ai >= naln) return;
  const CigAln a = cig_aln(off, npat, aln_pat, start, end, n, 0, ai);
  uint64_t d = kCigNone;
  uint32_t runs = 0;
  if (a.ok) {                                           // (L = m)
    const uint64_t m = (uint64_t)a.m;
    const uint8_t *P = pat + a.o0, *T = text + a.s;
    uint64_t bad = 0;
    for (uint64_t t = 16 * (uint64_t)gl; t < m; t += 256) {
      if (t + 16 <= m) {
        const uint4 x = ld16u(P + t), y = ld16u(T + t);
        bad |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w) | zero_bytes(x.x) | zero_bytes(x.y) | zero_bytes(x.z) | zero_bytes(x.w);
      } else {
        for (uint64_t u = t; u < m; u++) bad |= (uint64_t)(P[u] != T[u] || !P[u]);
      }
    }
    if (!gsum16(bad != 0)) {
      d = 0;
      if (m) { runs = 1; if (gl == 0) slot[ai] = (uint32_t)m << 4 | kOpEq; }
    }
  }
  if (gl == 0) { dist[ai] = (uint8_t)d; cnt[ai] = runs; }
}

// cig[cig_off[ai] + r] = run r of alignment ai, which its slot of S words holds last first
__global__ void __launch_bounds__(kTB) cig_place_k(uint64_t naln, uint64_t S, const uint32_t *__restrict__ slot, const uint64_t *__restrict__ cig_off,
                                                   uint64_t total, uint32_t *__restrict__ cig) {
  const uint64_t t = BID * kTB + threadIdx.x, ai = t / S, r = t % S;
  if (ai >= naln) return;
  const uint64_t o = cig_off[ai], runs = cig_off[ai + 1] - o;
  if (r < runs && runs <= S && o + r < total) cig[o + r] = slot[ai * S + (runs - 1 - r)];
}

// PFP_FM_CIGAR_SCRATCH=BYTES: a bound below kCigarScratch (tests: a small one cuts a small call into chunks)
uint64_t cigar_scratch_from_env() {
  uint64_t bytes = kCigarScratch;
  if (const char *e = getenv("PFP_FM_CIGAR_SCRATCH")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < bytes) bytes = v;
  }
  return bytes;
}

template <int CPL>
void launch_cigar(pfp_ctx *c, const uint8_t *text, uint64_t n, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *aln_pat,
                  const uint64_t *start, const uint64_t *end, uint64_t a0, uint64_t a1, int k, const uint64_t *soff, uint64_t sbase,
                  uint32_t *scratch, uint8_t *dist, uint64_t *cnt, uint32_t *slot) {
  fm_cigar_k<CPL><<<gdim(cdiv(a1 - a0, kTB / 16)), kTB, 0, c->stream>>>(text, n, pat, pat_off, npat, aln_pat, start, end, a0, a1, k, soff, sbase,
                                                                        scratch, dist, cnt, slot);
}

}  // namespace

void fm_cigar_runs(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *aln_pat, const uint64_t *start,
                   const uint64_t *end, uint64_t naln, int k, uint8_t *dist, uint64_t *cig_off, CigRuns &out) {
  pfp_ctx *c = f.c;
  fm_extend_check(f, k);
  fm_extend_check_patterns(f, pat_off, npat);
  out.naln = naln; out.S = 2 * (uint64_t)k + 1; out.total = 0;
  if (!naln) {
    PFP_HIP(hipMemsetAsync(cig_off, 0, sizeof(uint64_t), c->stream));
    sync(c);
    return;
  }
  const uint8_t *text = f.text.p;
  const uint64_t n = f.n1 - 1;
  out.slot.alloc(c, naln * out.S);
  DBuf<uint64_t> cnt;
  alloc_counts(c, cnt, naln);
  if (k == 0) {
    KScope ks(c, "fm_cigar", 0);
    fm_cigar0_k<<<gdim(cdiv(naln, kTB / 16)), kTB, 0, c->stream>>>(text, n, pat, pat_off, npat, aln_pat, start, end, naln, dist, cnt.p, out.slot.p);
    PFP_HIP(hipGetLastError());
  } else {
    const int cpl = 2 * k + 1 <= 16 ? 1 : 2 * k + 1 <= 32 ? 2 : 2 * k + 1 <= 48 ? 3 : 5;
    // the words of every alignment's records and their exclusive sums
    DBuf<uint64_t> need(c, naln + 1), soff(c, naln + 1);
    {
      KScope ks(c, "fm_cigar_plan", 0);
      cig_need_k<<<gdim(cdiv(naln + 1, kTB)), kTB, 0, c->stream>>>(pat_off, npat, aln_pat, start, end, naln, n, k, 16 * (uint64_t)cpl, need.p);
      PFP_HIP(hipGetLastError());
      exclusive_sum_u64(c, need.p, soff.p, naln + 1);
    }
    const uint64_t all = read_scalar(c, soff.p + naln), budget = cigar_scratch_from_env() / sizeof(uint32_t);
    std::vector<uint64_t> h;                            // the sums on the host, where one launch cannot hold all the records
    if (all > budget) {
      h.resize(naln + 1);
      d2h(c, h.data(), soff.p, naln + 1);
      sync(c);
    }
    // consecutive alignments whose records fit the budget; one that needs more goes alone
    for (uint64_t a0 = 0, a1; a0 < naln; a0 = a1) {
      a1 = naln;
      if (!h.empty())
        for (a1 = a0 + 1; a1 < naln && h[a1 + 1] - h[a0] <= budget;) a1++;
      const uint64_t sbase = h.empty() ? 0 : h[a0], words = h.empty() ? all : h[a1] - h[a0];
      DBuf<uint32_t> scratch(c, words);                 // (goes back to the pool in stream order)
      KScope ks(c, "fm_cigar", 0);
      if (cpl == 1) launch_cigar<1>(c, text, n, pat, pat_off, npat, aln_pat, start, end, a0, a1, k, soff.p, sbase, scratch.p, dist, cnt.p, out.slot.p);
      else if (cpl == 2) launch_cigar<2>(c, text, n, pat, pat_off, npat, aln_pat, start, end, a0, a1, k, soff.p, sbase, scratch.p, dist, cnt.p, out.slot.p);
      else if (cpl == 3) launch_cigar<3>(c, text, n, pat, pat_off, npat, aln_pat, start, end, a0, a1, k, soff.p, sbase, scratch.p, dist, cnt.p, out.slot.p);
      else launch_cigar<5>(c, text, n, pat, pat_off, npat, aln_pat, start, end, a0, a1, k, soff.p, sbase, scratch.p, dist, cnt.p, out.slot.p);
      PFP_HIP(hipGetLastError());
    }
  }
  exclusive_sum_u64(c, cnt.p, cig_off, naln + 1);
  out.total = read_scalar(c, cig_off + naln);           // (syncs: the counts and the sums go back when this returns)
}

void fm_cigar_write(FmIndex &f, const CigRuns &runs, const uint64_t *cig_off, uint32_t *cig) {
  pfp_ctx *c = f.c;
  if (!runs.total) return;
  KScope ks(c, "fm_cigar_place", 0);
  cig_place_k<<<gdim(cdiv(runs.naln * runs.S, kTB)), kTB, 0, c->stream>>>(runs.naln, runs.S, runs.slot.p, cig_off, runs.total, cig);
  PFP_HIP(hipGetLastError());
}

void fm_cigar(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *aln_pat, const uint64_t *start,
              const uint64_t *end, uint64_t naln, int k, uint8_t *dist, uint64_t *cig_off, uint32_t *cig) {
  CigRuns runs;
  fm_cigar_runs(f, pat, pat_off, npat, aln_pat, start, end, naln, k, dist, cig_off, runs);
  if (cig) fm_cigar_write(f, runs, cig_off, cig);
  sync(f.c);                                            // (the slots go back when this returns)
}

}  // namespace pfp
