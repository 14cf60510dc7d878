// fmband.hpp -- what the banded files share.  The banded pass of fmextend.hip and fmwindow.hip: m rows of Sellers' dynamic programme over a band of 16 CPL
// diagonals, by one group of 16 lanes, forwards with a free start or backwards with a fixed end.  fmextend.hip's head states the
// band and the layout; both files take an alignment's start from the backward form.  And the walk back along the records of a
// pass that kept them, which fmcigar.hip and fmfill.hip share.
#pragma once
#include "fmdev.hpp"

namespace pfp {

namespace {

constexpr uint8_t kExtNone = 0xFF;
constexpr uint64_t kExtNoPos = ~0ull;

// the horizontal moves of one row held by a group of 16 lanes, CPL consecutive cells per lane (gl = this lane's place): v[c] = min
// over c' <= c of v[c'] + (c - c'), capped at inf.  Inside the lane first, then across the group
template <int CPL>
__device__ __forceinline__ void row_scan(int (&v)[CPL], int gl, int inf) {
  const int base = gl * CPL;
#pragma unroll
  for (int q = 1; q < CPL; q++) v[q] = min(v[q], v[q - 1] + 1);
  // the last cells of this lane and those before it, as seen from column 0
  const int z = gscan16(v[CPL - 1] - base - (CPL - 1), gl, [](int x, int y) { return min(x, y); });
  int carry = __shfl_up(z, 1, 16);                      // the lanes before this one
  carry = gl ? carry + base : (1 << 20);
#pragma unroll
  for (int q = 0; q < CPL; q++) v[q] = min(min(v[q], carry + q), inf);
}

// one pass over the m rows of the band (see the head of fmextend.hip).  P = the pattern's first byte; the window is L columns wide and
// column x > k carries text byte org + (x - k) - 1 (forward) or org - (x - k) (BACK: the text read leftwards from org, the pattern
// from its end).  cur = the last row's cells, cell q of this lane is column m + gl CPL + q.  false: a whole row exceeded k
template <int CPL, bool BACK>
__device__ __forceinline__ bool band_pass(const uint8_t *__restrict__ text, const uint8_t *__restrict__ P, int m, uint64_t org, int L, int k,
                                          int gl, int (&cur)[CPL]) {
  const int inf = k + 1, base = gl * CPL;
  auto fetch = [&](int x) -> int {                      // (columns outside the window are not read; no cell that counts uses them)
    if (x <= k || x > L + k) return 0;
    return BACK ? text[org - (uint64_t)(x - k)] : text[org + (uint64_t)(x - k) - 1];
  };
  auto scan = [&](int (&v)[CPL]) { row_scan<CPL>(v, gl, inf); };
  int tb[CPL];
#pragma unroll
  for (int q = 0; q < CPL; q++) {
    const int x = base + q;
    cur[q] = BACK ? (x == k ? 0 : inf) : (x >= k && x <= L + k ? 0 : inf);
    tb[q] = fetch(1 + x);
  }
  scan(cur);
  for (int i0 = 0; i0 < m; i0 += 16) {
    // this lane's share of the block's bytes: the pattern byte of row i0 + 1 + gl (0x100 for a byte 0: it equals nothing) and the
    // text byte that enters the band's right edge after that row
    const int row = i0 + 1 + gl;
    int mine = 0x100;
    if (row <= m) {
      const int b = BACK ? P[m - row] : P[row - 1];
      mine = (b ? b : 0x100) | fetch(row + 16 * CPL) << 16;
    }
    const int rows = min(16, m - i0);
    for (int r = 0; r < rows; r++) {
      const int both = __shfl(mine, r, 16), pb = both & 0xFFFF;
      const int next = __shfl_down(cur[0] | tb[0] << 8, 1, 16);       // the neighbour's first cell and its text byte
      const int up = gl == 15 ? inf : (next & 0xFF);
      int v[CPL];
#pragma unroll
      for (int q = 0; q < CPL; q++) v[q] = min(cur[q] + (tb[q] != pb), (q + 1 < CPL ? cur[q + 1] : up) + 1);
      scan(v);
#pragma unroll
      for (int q = 0; q < CPL; q++) cur[q] = v[q];
#pragma unroll
      for (int q = 0; q + 1 < CPL; q++) tb[q] = tb[q + 1];
      tb[CPL - 1] = gl == 15 ? both >> 16 : next >> 8;
    }
    int low = cur[0];
#pragma unroll
    for (int q = 1; q < CPL; q++) low = min(low, cur[q]);
    if (gmin16((uint64_t)low) >= (uint64_t)inf) return false;
  }
  return true;
}

// ---------------------------------------------------------------- the walk back along a pass's records (fmcigar.hip, fmfill.hip)
// the records: 2 bits per cell, the operation rules 1-4 of "Edit scripts" choose there (0 '=', 1 'X', 2 'I', 3 'D'); word
// (i - 1) / 16 * W + c holds row i of cell c of a band of W cells at bits 2 ((i - 1) % 16)
constexpr uint32_t kOpI = 1, kOpD = 2, kOpEq = 7, kOpX = 8;     // the BAM codes

// the uint32 words that hold the records of m rows of a band of W cells: whole blocks of 16 rows, and whole 128 bytes
__host__ __device__ __forceinline__ uint64_t cig_words(uint64_t m, uint64_t W) { return ((m + 15) / 16 * W + 31) & ~31ull; }

// one lane walks from (m, L), which is cell c of the last row, to (0, 0) along the records of a band of W cells; the runs go into
// slot last first (at most cap of them are written) -> their number
__device__ __forceinline__ uint32_t cig_walk(const uint32_t *ops, int W, int m, int L, int c, uint32_t *__restrict__ slot, uint32_t cap) {
  int i = m, j = L;
  uint32_t runs = 0, op = 0, len = 0;                   // the run that is open (op 0: none yet)
  auto emit = [&](uint32_t o, uint32_t count) {
    if (o == op) { len += count; return; }
    if (len) {
      if (runs < cap) slot[runs] = len << 4 | op;
      runs++;
    }
    op = o; len = count;
  };
  uint64_t at = ~0ull;                                  // the word that `word` holds: '=' and 'X' stay in it for 16 rows
  uint32_t word = 0;
  while (i > 0 && j > 0 && (unsigned)c < (unsigned)W) {
    const uint64_t idx = (uint64_t)((i - 1) >> 4) * W + c;
    if (idx != at) { word = ops[idx]; at = idx; }
    const int r = (i - 1) & 15;
    const uint32_t top = word << (2 * (15 - r));        // row i's record in the two highest bits, the rows below it behind
    const int eq = min(min(top ? __clz((int)top) >> 1 : 16, r + 1), j);       // the '=' from row i down, inside this word
    if (eq) { emit(kOpEq, (uint32_t)eq); i -= eq; j -= eq; continue; }
    const uint32_t code = top >> 30;
    if (code <= 1) { emit(kOpX, 1); i--; j--; }
    else if (code == 2) { emit(kOpI, 1); i--; c++; }
    else { emit(kOpD, 1); j--; c--; }
  }
  if (i > 0) emit(kOpI, (uint32_t)i);
  else if (j > 0) emit(kOpD, (uint32_t)j);
  emit(0, 0);                                           // closes the open run
  return runs;
}

}  // namespace

}  // namespace pfp
