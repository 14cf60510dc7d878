// fmband.hpp -- the banded pass that fmextend.hip and fmwindow.hip share: m rows of Sellers' dynamic programme over a band of 16 CPL
// diagonals, by one group of 16 lanes, forwards with a free start or backwards with a fixed end.  fmextend.hip's head states the
// band and the layout; both files take an alignment's start from the backward form.
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

}  // namespace

}  // namespace pfp
