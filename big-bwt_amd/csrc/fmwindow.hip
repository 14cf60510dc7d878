// fmwindow.hip -- the best alignment of a whole pattern anywhere in a window T[lo..hi) of the text of an FmIndex, under unit-cost
// edit distance: what pairing reads needs (a mate lies within an insert size of its partner) and what realigns a read inside a
// known region.  The reference has no counterpart; include/pfpgpu.h, "Aligning in a window", states the definitions.
//
//   The programme is Sellers' with a free start: cell (i, j) is pattern prefix i against a text span that ends at lo + j, columns
//   j = 0 .. W = hi - lo, row 0 is 0 across the window, and the last row gives d* and the smallest end e.  Values are capped at
//   k + 1: every move adds a cost >= 0, so a capped cell is exact where it is <= k and k + 1 where the true value is larger.
//   The layout.  One group of 16 lanes per candidate, CPL consecutive columns per lane (a template parameter: a lane's cells and
//   its text bytes stay in registers), one pattern row per step.  The window does not slide, unlike fmextend.hip's band: a lane's
//   text bytes are read once per tile.  A row takes the vertical move from the row above, the diagonal move from the left
//   neighbour's last cell of the row above (one shuffle), then the horizontal moves: the min-plus scan that band_pass uses
//   (row_scan, fmband.hpp), inside the lane first and then across the group.  The row's pattern byte was read 16 rows at a time,
//   one per lane.
//   Tiles.  A window wider than 16 CPL columns goes through in tiles of 16 CPL columns, left to right, by the same group.  The
//   tiles do NOT overlap: a tile hands its last column to the next one - D[i][c - 1] for every row i, one byte each, written 16
//   rows at a time into m + 1 bytes of scratch - and the next tile's first column takes its diagonal and its horizontal move from
//   those bytes (read 16 rows at a time, in the same loads as the pattern bytes).  So every cell of the window is computed once
//   and from exactly the cells the recurrence names: the result is that of the untiled programme whatever 16 CPL is, and the
//   minimum of (d, e) over the tiles' last rows is the window's.  (The alternative - overlapping tiles that step by their width
//   minus m + k, each complete in itself - needs no scratch but computes a share of (m + k) / (16 CPL) of the cells twice and
//   cannot serve m + k >= 16 CPL; it was not built.)
//   Dead rows.  Once a tile's row is k + 1 everywhere and the column handed in is k + 1 from that row on (that row included: its
//   cell is the next row's diagonal), the rest of the tile is k + 1: the tile ends (checked every 16 rows).  A tile records the last row at which the column it hands on was <= k; rows
//   after it are taken as k + 1 and are neither written nor read.
//   The start.  A second kernel runs fmextend.hip's backward pass (band_pass<CPL, true>, fmband.hpp) from e over the band
//   -k .. k: an alignment of cost <= k with a fixed end leaves its diagonal by at most k and spans at most m + k bytes, so the
//   first column of the last row that holds d* is the largest s, exactly as in fm_extend_k.  k = 0: s = e - m.
//   Row scan or bit vector: the row scan was built, because every part of it was already proven in fmextend.hip.  Myers' bit-vector
//   form would meet the same definition; which of the two is faster on this chip has not been measured.
//   Bounded launches.  A candidate costs m (hi - lo) cell updates; a call goes through in consecutive pieces of at most
//   kWindowCells cells (PFP_FM_WINDOW_CELLS lowers it), a candidate with more goes alone.
// Bounds: text is read at positions lo .. hi - 1 only, for candidates with lo <= hi <= n, and patterns inside their offsets; the
// scratch of candidate ci is col[0 .. m] at coff[ci] - cbase, inside the piece's buffer by the sums that sized it; outputs are
// written at the candidate's own index.  Every loop is bounded by m, W / (16 CPL) or k.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"
#include "fmband.hpp"

namespace pfp {

namespace {

constexpr uint64_t kWindowCells = 1ull << 34;           // cell updates per launch: a choice, not a measurement
constexpr int kWinWide = 16;                            // columns per lane of the wide kernel: tiles of 256 columns
constexpr int kWinNarrow = 4;                           // and of the narrow one, for calls whose widest window fits one tile of 64

// what a candidate is about: its pattern and its window of W = hi - lo bytes at lo, or ok = false ("no alignment": no such
// pattern, decreasing offsets, a pattern too long, lo > hi, hi > n, a window too wide, or m - k > W: no span can hold the pattern)
struct WinCand { uint64_t o0, lo; int m, W; bool ok; };
__device__ __forceinline__ WinCand win_cand(const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ cand_pat,
                                            const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, uint64_t n, int k, uint64_t ci) {
  WinCand r{0, 0, 0, 0, false};
  const uint64_t p = cand_pat[ci];
  if (p >= npat) return r;
  const uint64_t o0 = off[p], o1 = off[p + 1], l = lo[ci], h = hi[ci];
  if (o1 < o0 || o1 - o0 > PFP_FM_EXTEND_MAX_M || l > h || h > n || h - l > PFP_FM_WINDOW_MAX_W) return r;
  if (o1 - o0 > h - l + (uint64_t)k) return r;
  return WinCand{o0, l, (int)(o1 - o0), (int)(h - l), true};
}

// the plan: cells[ci] = m W, need[ci] = the bytes of the column that candidate ci's tiles hand on (0 where one tile of `tile`
// columns holds the window), cells[ncand] = need[ncand] = 0; ctr[0] += windows lo <= hi <= n wider than PFP_FM_WINDOW_MAX_W,
// ctr[1] = the widest window of a candidate that is served
__global__ void __launch_bounds__(kTB) win_plan_k(const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ cand_pat,
                                                  const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, uint64_t ncand, uint64_t n, int k,
                                                  uint64_t tile, uint64_t *__restrict__ cells, uint64_t *__restrict__ need,
                                                  unsigned long long *__restrict__ ctr) {
  const uint64_t ci = BID * kTB + threadIdx.x;
  if (ci > ncand) return;
  uint64_t c = 0, b = 0;
  if (ci < ncand) {
    if (lo[ci] <= hi[ci] && hi[ci] <= n && hi[ci] - lo[ci] > PFP_FM_WINDOW_MAX_W) atomicAdd(&ctr[0], 1ull);
    const WinCand cd = win_cand(off, npat, cand_pat, lo, hi, n, k, ci);
    if (cd.ok && cd.m) {
      c = (uint64_t)cd.m * (uint64_t)cd.W;
      if ((uint64_t)cd.W + 1 > tile) b = (uint64_t)cd.m + 1;
      atomicMax(&ctr[1], (unsigned long long)cd.W);
    }
  }
  cells[ci] = c;
  need[ci] = b;
}

// the forward pass: one group of 16 lanes per candidate a0 <= ci < a1, 0 <= k <= PFP_FM_EXTEND_MAX_K -> dist[ci] = d* and
// end[ci] = the smallest e, or "no alignment".  coff = the exclusive sums of win_plan_k's need, cbase = coff[a0], col = the
// piece's scratch
template <int CPL>
__global__ void __launch_bounds__(kTB) fm_window_k(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ pat,
                                                   const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ cand_pat,
                                                   const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, uint64_t a0, uint64_t a1, int k,
                                                   const uint64_t *__restrict__ coff, uint64_t cbase, uint8_t *__restrict__ colbuf,
                                                   uint8_t *__restrict__ dist, uint64_t *__restrict__ end) {
  constexpr int TW = 16 * CPL;
  const int gl = threadIdx.x & 15, base = gl * CPL, inf = k + 1;
  const uint64_t ci = a0 + BID * (kTB / 16) + (threadIdx.x >> 4);
  if (ci >= a1) return;                                 // (whole groups leave together: the shuffles stay inside groups)
  const WinCand cd = win_cand(off, npat, cand_pat, lo, hi, n, k, ci);
  uint64_t d = kExtNone, e = kExtNoPos;
  if (cd.ok && cd.m == 0) { d = 0; e = cd.lo; }
  else if (cd.ok) {                                     // (every lane of the group holds the same state)
    const int m = cd.m, W = cd.W;
    const uint8_t *P = pat + cd.o0, *T = text + cd.lo;
    uint8_t *col = colbuf + (coff[ci] - cbase);         // (used only where W + 1 > TW: then win_plan_k gave it m + 1 bytes)
    uint64_t best = ~0ull;                              // the smallest value of the last row inside the window, at its first column
    int prev_alive = 0;                                 // the last row at which the column handed in is <= k
    for (int c0 = 0; c0 <= W; c0 += TW) {
      const bool more = c0 + TW <= W;                   // another tile follows: this one hands its last column on
      int cur[CPL], tb[CPL];
#pragma unroll
      for (int q = 0; q < CPL; q++) {
        const int j = c0 + base + q;                    // column j ends at T[j]: it carries text byte T[j - 1]
        cur[q] = j <= W ? 0 : inf;
        tb[q] = j >= 1 && j <= W ? T[j - 1] : 0x200;    // (0x200 equals no pattern byte: a column past the window feeds only such columns)
      }
      int diag_in = c0 ? 0 : inf;                       // D[i - 1][c0 - 1] of the row to come: row 0 is 0, left of column 0 lies nothing
      int alive = 0;
      bool reached = true;
      for (int i0 = 0; i0 < m; i0 += 16) {
        // this lane's share of the block: the pattern byte of row i0 + 1 + gl (0x100 for a byte 0: it equals nothing) and the
        // cell D[row][c0 - 1] that the tile before handed on
        const int row = i0 + 1 + gl;
        int mine = 0x100 | inf << 16;
        if (row <= m) {
          const int b = P[row - 1];
          mine = (b ? b : 0x100) | (c0 && row <= prev_alive ? (int)col[row] : inf) << 16;
        }
        int keep = inf;
        const int rows = min(16, m - i0);
        for (int r = 0; r < rows; r++) {
          const int both = __shfl(mine, r, 16), pb = both & 0xFFFF, hin = both >> 16;
          int left = __shfl_up(cur[CPL - 1], 1, 16);    // the left neighbour's last cell of the row above
          if (gl == 0) left = diag_in;
          int v[CPL];
          v[0] = min(left + (tb[0] != pb), cur[0] + 1);
#pragma unroll
          for (int q = 1; q < CPL; q++) v[q] = min(cur[q - 1] + (tb[q] != pb), cur[q] + 1);
          if (gl == 0) v[0] = min(v[0], hin + 1);       // the horizontal move out of the tile before
          row_scan<CPL>(v, gl, inf);
#pragma unroll
          for (int q = 0; q < CPL; q++) cur[q] = v[q];
          diag_in = hin;
          if (more) {
            const int out = __shfl(cur[CPL - 1], 15, 16);
            if (gl == r) keep = out;
            if (out <= k) alive = i0 + 1 + r;
          }
        }
        if (more && row <= m) col[row] = (uint8_t)keep;
        int low = cur[0];
#pragma unroll
        for (int q = 1; q < CPL; q++) low = min(low, cur[q]);
        // (>: the handed-in cell of the block's last row is the next row's diagonal, so it must be k + 1 as well)
        if (gmin16((uint64_t)low) >= (uint64_t)inf && i0 + 16 > prev_alive) { reached = false; break; }
      }
      if (reached) {
#pragma unroll
        for (int q = 0; q < CPL; q++) {
          const int j = c0 + base + q;
          if (j <= W && cur[q] <= k) best = min(best, (uint64_t)cur[q] << 32 | (uint32_t)j);
        }
      }
      prev_alive = alive;
    }
    best = gmin16(best);
    if (best != ~0ull) { d = best >> 32; e = cd.lo + (uint32_t)best; }
  }
  if (gl == 0) { dist[ci] = (uint8_t)d; end[ci] = e; }
}

// the start: one group per candidate that fm_window_k gave (d, e), 16 CPL >= 2k + 1 -> start[ci] = the largest s with
// d(s, e) = d, by the backward pass from e over T[max(lo, e - (m + k)) .. e)
template <int CPL>
__global__ void __launch_bounds__(kTB) fm_window_start_k(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ pat,
                                                         const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ cand_pat,
                                                         const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, uint64_t ncand, int k,
                                                         uint8_t *__restrict__ dist, uint64_t *__restrict__ start, uint64_t *__restrict__ end) {
  const int gl = threadIdx.x & 15, base = gl * CPL;
  const uint64_t ci = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (ci >= ncand) return;
  const int dstar = dist[ci];
  uint64_t s = kExtNoPos;
  if (dstar != kExtNone) {
    const WinCand cd = win_cand(off, npat, cand_pat, lo, hi, n, k, ci);     // (ok: fm_window_k found an alignment)
    const uint64_t e = end[ci];
    const int m = cd.m;
    if (k == 0 || m == 0) s = e - (uint64_t)m;          // (an exact match spans m bytes)
    else {
      const int L2 = (int)min(e - cd.lo, (uint64_t)(m + k));
      int cur[CPL];
      uint64_t first = ~0ull;                           // the first column of the last row that holds d*: the shortest span
      if (band_pass<CPL, true>(text, pat + cd.o0, m, e, L2, k, gl, cur)) {
#pragma unroll
        for (int q = 0; q < CPL; q++) {
          const int x = m + base + q;
          if (x >= k && x <= L2 + k && cur[q] == dstar) first = min(first, (uint64_t)x);
        }
      }
      first = gmin16(first);
      if (first != ~0ull) s = e - (first - (uint64_t)k);
    }
  }
  if (gl == 0) {
    start[ci] = s;
    if (s == kExtNoPos) { dist[ci] = kExtNone; end[ci] = kExtNoPos; }
  }
}

// PFP_FM_WINDOW_CELLS=N: a bound below kWindowCells (tests: a small one cuts a small call into pieces)
uint64_t window_cells_from_env() {
  uint64_t cells = kWindowCells;
  if (const char *e = getenv("PFP_FM_WINDOW_CELLS")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < cells) cells = v;
  }
  return cells;
}

template <int CPL>
void launch_window_start(pfp_ctx *c, const uint8_t *text, uint64_t n, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat,
                         const uint32_t *cand_pat, const uint64_t *lo, const uint64_t *hi, uint64_t ncand, int k, uint8_t *dist, uint64_t *start,
                         uint64_t *end) {
  fm_window_start_k<CPL><<<gdim(cdiv(ncand, kTB / 16)), kTB, 0, c->stream>>>(text, n, pat, pat_off, npat, cand_pat, lo, hi, ncand, k, dist, start, end);
}

}  // namespace

void fm_window(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat, const uint64_t *lo,
               const uint64_t *hi, uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end) {
  pfp_ctx *c = f.c;
  fm_extend_check(f, k);
  fm_extend_check_patterns(f, pat_off, npat);
  if (!ncand) return;
  const uint8_t *text = f.text.p;
  const uint64_t n = f.n1 - 1;
  // the plan: every candidate's cells and scratch, their exclusive sums, the windows too wide and the widest one
  DBuf<uint64_t> cells(c, ncand + 1), need(c, ncand + 1), eoff(c, ncand + 1), coff(c, ncand + 1), ctr(c, 2);
  uint64_t h[2];
  {
    KScope ks(c, "fm_window_plan", 0);
    ctr.zero();
    win_plan_k<<<gdim(cdiv(ncand + 1, kTB)), kTB, 0, c->stream>>>(pat_off, npat, cand_pat, lo, hi, ncand, n, k, 16 * (uint64_t)kWinWide, cells.p,
                                                                  need.p, (unsigned long long *)ctr.p);
    PFP_HIP(hipGetLastError());
    d2h(c, h, ctr.p, 2);
    sync(c);
    PFP_REQUIRE(!h[0], PFP_ELIMIT, std::to_string(h[0]) + " windows of more than " + std::to_string(PFP_FM_WINDOW_MAX_W) +
                                       " bytes (PFP_FM_WINDOW_MAX_W)");
    exclusive_sum_u64(c, cells.p, eoff.p, ncand + 1);
    exclusive_sum_u64(c, need.p, coff.p, ncand + 1);
  }
  const bool narrow = h[1] + 1 <= 16 * (uint64_t)kWinNarrow;        // (then every window is one tile and nothing is handed on)
  const uint64_t all = read_scalar(c, eoff.p + ncand), budget = window_cells_from_env();
  std::vector<uint64_t> he, hc;                         // the sums on the host, where one launch may not hold all the cells
  if (all > budget) {
    he.resize(ncand + 1);
    hc.resize(ncand + 1);
    d2h(c, he.data(), eoff.p, ncand + 1);
    d2h(c, hc.data(), coff.p, ncand + 1);
    sync(c);
  }
  const uint64_t all_col = he.empty() ? read_scalar(c, coff.p + ncand) : hc[ncand];
  // consecutive candidates whose cells fit the budget; one that needs more goes alone
  for (uint64_t a0 = 0, a1; a0 < ncand; a0 = a1) {
    a1 = ncand;
    if (!he.empty())
      for (a1 = a0 + 1; a1 < ncand && he[a1 + 1] - he[a0] <= budget;) a1++;
    const uint64_t cbase = he.empty() ? 0 : hc[a0], bytes = he.empty() ? all_col : hc[a1] - hc[a0];
    DBuf<uint8_t> col(c, bytes);                        // (goes back to the pool in stream order)
    KScope ks(c, "fm_window", 0);
    const auto grid = gdim(cdiv(a1 - a0, kTB / 16));
    if (narrow)
      fm_window_k<kWinNarrow><<<grid, kTB, 0, c->stream>>>(text, n, pat, pat_off, npat, cand_pat, lo, hi, a0, a1, k, coff.p, cbase, col.p, dist, end);
    else
      fm_window_k<kWinWide><<<grid, kTB, 0, c->stream>>>(text, n, pat, pat_off, npat, cand_pat, lo, hi, a0, a1, k, coff.p, cbase, col.p, dist, end);
    PFP_HIP(hipGetLastError());
  }
  {
    KScope ks(c, "fm_window_start", 0);
    if (2 * k + 1 <= 16) launch_window_start<1>(c, text, n, pat, pat_off, npat, cand_pat, lo, hi, ncand, k, dist, start, end);
    else if (2 * k + 1 <= 32) launch_window_start<2>(c, text, n, pat, pat_off, npat, cand_pat, lo, hi, ncand, k, dist, start, end);
    else if (2 * k + 1 <= 48) launch_window_start<3>(c, text, n, pat, pat_off, npat, cand_pat, lo, hi, ncand, k, dist, start, end);
    else launch_window_start<5>(c, text, n, pat, pat_off, npat, cand_pat, lo, hi, ncand, k, dist, start, end);
    PFP_HIP(hipGetLastError());
  }
  sync(c);                                              // (the plan's arrays go back when this returns)
}

}  // namespace pfp
