// fmfill.hip -- aligning chains base by base: the global edit-distance alignment, with its edit script, of the stretch between two
// consecutive anchors of a chain (a gap), and the passes that stitch anchors and gaps into the script of a chain.  The reference has
// no counterpart; the band is Ukkonen's ("Algorithms for approximate string matching", Information and Control 1985), the records
// and the walk are fmcigar.hip's.  include/pfpgpu.h, "Aligning chains", states the definitions (segments, "no script", members,
// trimming, gaps, the script of a chain, the strand turn).
//
//   The band.  A gap is a = q1 - q0 pattern bytes against b = t1 - t0 text bytes; cell (i, j) of the DP is pattern prefix i against
//   text prefix j, on diagonal j - i.  (0, 0) lies on diagonal 0 and (a, b) on diagonal b - a.  With lo = min(0, b - a) and hi =
//   max(0, b - a), the band at slack e is the diagonals lo - e .. hi + e; cells outside it count as "too many".
//   Exactness.  A path from (0, 0) to (a, b) that reaches diagonal hi + e + 1 has made at least e + 1 steps to the right of the
//   diagonals it must visit anyway (0 .. b - a or b - a .. 0) and has to undo each of them: at least e + 1 D beyond max(0, b - a) and
//   e + 1 I beyond max(0, a - b), so it costs at least |b - a| + 2e + 2; the same on the other side.  The banded value D' is the
//   cheapest path inside the band, so D' >= D always, and D' <= |b - a| + 2e + 1 means no path that leaves the band is cheaper:
//   D' = D, and every optimal path lies inside the band.  So a banded result D' <= min(F, |b - a| + 2e + 1) is exact.  If the result
//   is above that and |b - a| + 2e + 1 >= F, then D > F (were D <= F, every optimal path would lie inside the band and D' = D).
//   A band that holds more diagonals than lo - e .. hi + e keeps all of this: its values lie between D and the narrower band's.
//   The schedule.  e = 8, 32, 128, 512, 2048 (round 0 .. 4), cut at lim = min(ceil((F - |b - a|) / 2), max(a, b)): at the first,
//   |b - a| + 2e + 1 >= F, at the second the band is the whole matrix (and D <= max(a, b) <= |b - a| + 2e + 1).  A round that reaches
//   lim is a gap's last: its result is exact or D > F.  So at most five rounds, and a band of at most F + 2 cells.  The schedule is a
//   choice; the results do not depend on it.
//   The same script as the full matrix.  The walk starts at (a, b), whose banded value is exact, and visits only cells on optimal
//   paths: rule 1 moves along a match, which an optimal path through the cell can always take, and rules 2-4 move to a neighbour
//   whose value is one less.  Every cell of an optimal path lies inside the band and its banded value is exact (the prefix of an
//   optimal path is optimal and inside the band).  At such a cell with value c, a neighbour whose true value is c - 1 lies on an
//   optimal path too, so its banded value is c - 1; any other neighbour's banded value is at least its true value >= c, so the
//   rules do not choose it.  The rules therefore choose on the band what they choose on the full matrix - which is why the tests
//   may compare with an unbanded reference.
//   The layout is fmcigar.hip's with the width as a template: a group of GW lanes per gap, CPL consecutive cells per lane, one
//   pattern row per step, the row's horizontal moves by the min-plus scan of fmband.hpp's row_scan, over GW lanes.  Cell c of row i
//   is column j = i + c - sh, sh = e - lo.  Cell values are at most F + 1 <= 4097: 16 bits, and a lane hands its first cell and its
//   text byte to its left neighbour in one 32-bit shuffle.  Six widths: 16, 32 and 64 cells by groups of 16 lanes; 256, 1024 and
//   4160 cells by a whole wave, whose lanes loop over their share of the band (4, 16 or 65 cells each).  The gaps of a round are
//   bucketed by the width they need, one launch per bucket that is not empty.  No LDS, no cross-lane operation wider than the group.
//   Trivial gaps - a = 0 or b = 0 (one run), a = b = 1 ('=' or X) - are settled by one lane each in the classifying pass: on real
//   reads most gaps are a lone substitution between two MEMs.  Their runs are not stored; the passes that place runs derive them.
//   The records of a launch are bounded (kFillScratch; PFP_FM_FILL_SCRATCH lowers it): a round's gaps go through in consecutive
//   chunks whose records fit, and one that needs more goes alone.  The runs of a gap come out last first into a slot of min(2 cap +
//   1, a + b) words (cap = min(F, |b - a| + 2e + 1) bounds the cost that round accepts); the slots of a chunk are one buffer, which
//   lives until the runs are placed.
//   Members and stitching.  A lane per aligned chain walks n parents back from the chain's last anchor (bounded, resumable: n has
//   no bound but the pattern's anchors); a lane per member trims its anchor against the one before and writes the gap; the gaps go
//   through the passes above; a lane per chain counts its runs, merging neighbours of one operation at the seams, the library
//   scan gives the offsets, and the same lane writes them.
// Bounds: every loop is bounded by a, b, F or a chain's n; text is read at t0 .. t1 - 1 only and patterns at q0 .. q1 - 1 inside
// their offsets; records are written inside the gap's own words, whose number cig_words gives to the kernel that sizes them and to
// the one that fills them; the walk takes at most a + b steps, reads only words the pass wrote, and writes at most the slot's runs;
// a member index read from a parent stays inside its pattern's segment.
#include <vector>
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"
#include "fmband.hpp"

namespace pfp {

namespace {

constexpr uint32_t kFillNone = 0xFFFFFFFFu;
constexpr uint64_t kFillScratch = 1ull << 30;           // bytes of records per launch: a choice, as kCigarScratch
constexpr uint8_t kSettled = 0xFF;
constexpr int kFillBuckets = 6;
const char *const kFillName[kFillBuckets] = {"fm_fill_16", "fm_fill_32", "fm_fill_64", "fm_fill_256", "fm_fill_1024", "fm_fill_4160"};  // the trace's rows
constexpr uint64_t kChainSteps = 65536;                 // members per chain and launch of the walk: fmchain.hip's default

__host__ __device__ __forceinline__ int fill_width(int bk) {
  return bk == 0 ? 16 : bk == 1 ? 32 : bk == 2 ? 64 : bk == 3 ? 256 : bk == 4 ? 1024 : 4160;
}

// PFP_FM_FILL_SCRATCH=BYTES: a bound below kFillScratch (tests: a small one cuts a small call into chunks)
uint64_t fill_scratch_from_env() {
  uint64_t bytes = kFillScratch;
  if (const char *e = getenv("PFP_FM_FILL_SCRATCH")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < bytes) bytes = v;
  }
  return bytes;
}
// PFP_FM_CHAIN_STEPS, as fmchain.hip reads it
uint64_t member_steps_from_env() {
  uint64_t steps = kChainSteps;
  if (const char *e = getenv("PFP_FM_CHAIN_STEPS")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < steps) steps = v;
  }
  return steps;
}

// what a gap is about: its bytes, or ok = false (see "no script" in the definitions, but for the distance)
struct FillGap { uint64_t po, to; int a, b; bool ok; };
__device__ __forceinline__ FillGap fill_gap(const uint64_t *__restrict__ off, uint64_t npat, const FillSegs &sg, uint64_t n, uint64_t F, uint64_t g) {
  FillGap r{0, 0, 0, 0, false};
  const uint64_t p = sg.pat[g];
  if (p >= npat) return r;
  const uint64_t o0 = off[p], o1 = off[p + 1];
  if (o1 < o0) return r;
  const uint64_t q0 = sg.q0[g], q1 = sg.q1[g], t0 = sg.t0[g], t1 = sg.t1[g];
  if (q0 > q1 || q1 > o1 - o0 || t0 > t1 || t1 > n) return r;
  const uint64_t a = q1 - q0, b = t1 - t0;
  if (a > PFP_FM_FILL_MAX_LEN || b > PFP_FM_FILL_MAX_LEN || (a > b ? a - b : b - a) > F) return r;
  return FillGap{o0 + q0, t0, (int)a, (int)b, true};
}

// the band of a gap in a round (see the head of the file): slack e, W = its cells, cap = the largest cost the round accepts
struct FillBand { int e, W, cap, bk; bool last; };
__device__ __forceinline__ FillBand fill_band(int a, int b, int F, int round) {
  const int d = a > b ? a - b : b - a, lim = min((F - d + 1) >> 1, max(a, b));
  int e = round < 5 ? 8 << (2 * round) : lim;
  const bool last = e >= lim;
  if (last) e = lim;
  const int W = d + 2 * e + 1;
  int bk = 0;
  while (bk + 1 < kFillBuckets && fill_width(bk) < W) bk++;
  return FillBand{e, W, min(F, W), bk, last};
}
__device__ __forceinline__ uint32_t fill_slot(const FillBand &bd, int a, int b) { return (uint32_t)min(2 * bd.cap + 1, a + b); }

// one lane per gap: no script, a trivial gap, or round 0
__global__ void __launch_bounds__(kTB) fill_classify_k(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ pat,
                                                       const uint64_t *__restrict__ off, uint64_t npat, FillSegs sg, uint64_t ngap, uint64_t F,
                                                       uint8_t *__restrict__ rnd, uint32_t *__restrict__ dist, uint64_t *__restrict__ cnt,
                                                       uint64_t *__restrict__ rptr, unsigned long long *__restrict__ ctr) {
  const uint64_t g = BID * kTB + threadIdx.x;
  if (g >= ngap) return;
  const FillGap x = fill_gap(off, npat, sg, n, F, g);
  uint32_t d = kFillNone, runs = 0;
  uint8_t r = kSettled;
  if (x.ok) {
    if (!x.a || !x.b) { d = (uint32_t)(x.a + x.b); runs = d != 0; }     // (|a - b| <= F holds)
    else if (x.a == 1 && x.b == 1) {
      const uint32_t diff = pat[x.po] != text[x.to] || !pat[x.po];
      if (diff <= F) { d = diff; runs = 1; }
    } else r = 0;
    if (ctr && r == kSettled) atomicAdd(&ctr[0], 1ull);                 // (measurement: the trivial gaps)
  }
  rnd[g] = r; dist[g] = d; cnt[g] = runs; rptr[g] = 0;
}

// one lane per gap (entry ngap: zeros): the record words and the slot of a gap that is pending in this round, and its bucket.
// ctr[bucket] += its gaps; stats (measurement): ctr[8 + bucket] += the cells of their passes
__global__ void __launch_bounds__(kTB) fill_plan_k(const uint64_t *__restrict__ off, uint64_t npat, FillSegs sg, uint64_t ngap, uint64_t n, uint64_t F,
                                                   int round, const uint8_t *__restrict__ rnd, uint8_t *__restrict__ bkt,
                                                   uint64_t *__restrict__ need, uint64_t *__restrict__ bnd, int stats, unsigned long long *__restrict__ ctr) {
  const uint64_t g = BID * kTB + threadIdx.x;
  if (g > ngap) return;
  uint64_t w = 0, s = 0;
  uint8_t bk = kSettled;
  if (g < ngap && rnd[g] == (uint8_t)round) {
    const FillGap x = fill_gap(off, npat, sg, n, F, g);
    if (x.ok) {
      const FillBand bd = fill_band(x.a, x.b, (int)F, round);
      bk = (uint8_t)bd.bk;
      w = cig_words((uint64_t)x.a, (uint64_t)fill_width(bd.bk));
      s = fill_slot(bd, x.a, x.b);
      if (stats) atomicAdd(&ctr[8 + bd.bk], (unsigned long long)x.a * (unsigned long long)fill_width(bd.bk));
    }
  }
  for (int k = 0; k < kFillBuckets; k++) {              // one atomic per wave and bucket
    const uint64_t m = __ballot(bk == (uint8_t)k);
    if (m && (int)(threadIdx.x & 63) == __ffsll((unsigned long long)m) - 1) atomicAdd(&ctr[k], (unsigned long long)__popcll(m));
  }
  if (g < ngap) bkt[g] = bk;
  need[g] = w; bnd[g] = s;
}

template <int GW, class T, class Op>
__device__ __forceinline__ T gscan(T v, int gl, Op op) {
#pragma unroll
  for (int d = 1; d < GW; d <<= 1) {
    const T o = __shfl_up(v, d, GW);
    if (gl >= d) v = op(v, o);
  }
  return v;
}
template <int GW>
__device__ __forceinline__ uint64_t gmin(uint64_t v) {
#pragma unroll
  for (int d = 1; d < GW; d <<= 1) { const uint64_t o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
  return v;
}

// the m rows of the band (see the head of the file; cig_forward of fmcigar.hip with the group's width, the shift and the cap as
// arguments): T = the gap's first text byte, P = its first pattern byte.  cur = the last row's cells, cell q of this lane is
// c = gl CPL + q; ops gets the records.  false: a whole row reached inf (the records stop there)
template <int GW, int CPL>
__device__ __forceinline__ bool fill_forward(const uint8_t *__restrict__ T, const uint8_t *__restrict__ P, int m, int L, int sh, int inf, int gl,
                                             int (&cur)[CPL], uint32_t *ops) {
  const int base = gl * CPL;
  // the text byte of column x = j + sh (columns outside 1 .. L are not read; no cell that counts uses them)
  auto fetch = [&](int x) -> int {
    if (x <= sh || x > L + sh) return 0;
    return T[x - sh - 1];
  };
  // the horizontal moves of one row: v[c] = min over c' <= c of v[c'] + (c - c'), capped
  auto scan = [&](int (&v)[CPL]) {
#pragma unroll
    for (int q = 1; q < CPL; q++) v[q] = min(v[q], v[q - 1] + 1);
    const int z = gscan<GW>(v[CPL - 1] - base - (CPL - 1), gl, [](int x, int y) { return min(x, y); });
    int carry = __shfl_up(z, 1, GW);                    // the lanes before this one
    carry = gl ? carry + base : (1 << 20);
#pragma unroll
    for (int q = 0; q < CPL; q++) v[q] = min(min(v[q], carry + q), inf);
  };
  int tb[CPL];
#pragma unroll
  for (int q = 0; q < CPL; q++) {
    const int x = base + q;
    cur[q] = x == sh ? 0 : inf;                         // row 0: cell c is column c - sh, and its value is the column number
    tb[q] = fetch(1 + x);
  }
  scan(cur);
  for (int i0 = 0; i0 < m; i0 += 16) {
    // the first 16 lanes' share of the block's bytes: the pattern byte of row i0 + 1 + gl (0x100 for a byte 0: it equals nothing)
    // and the text byte that enters the band's right edge after that row
    const int row = i0 + 1 + gl;
    int mine = 0x100;
    if (gl < 16 && row <= m) {
      const int b = P[row - 1];
      mine = (b ? b : 0x100) | fetch(row + GW * CPL) << 16;
    }
    const int rows = min(16, m - i0);
    uint32_t w[CPL];
#pragma unroll
    for (int q = 0; q < CPL; q++) w[q] = 0;
    for (int r = 0; r < rows; r++) {
      const int both = __shfl(mine, r, GW), pb = both & 0xFFFF;
      const int next = __shfl_down(cur[0] | tb[0] << 16, 1, GW);       // the neighbour's first cell and its text byte
      const int up = gl == GW - 1 ? inf : (next & 0xFFFF);
      int v[CPL];
#pragma unroll
      for (int q = 0; q < CPL; q++) v[q] = min(cur[q] + (tb[q] != pb), (q + 1 < CPL ? cur[q + 1] : up) + 1);
      scan(v);
#pragma unroll
      for (int q = 0; q < CPL; q++) {                   // rules 1-4 (a cell at inf may record anything: no optimal path visits it)
        const int above = q + 1 < CPL ? cur[q + 1] : up;
        const uint32_t op = tb[q] == pb ? 0u : cur[q] == v[q] - 1 ? 1u : above == v[q] - 1 ? 2u : 3u;
        w[q] |= op << (2 * r);
      }
#pragma unroll
      for (int q = 0; q < CPL; q++) cur[q] = v[q];
#pragma unroll
      for (int q = 0; q + 1 < CPL; q++) tb[q] = tb[q + 1];
      tb[CPL - 1] = gl == GW - 1 ? both >> 16 : next >> 16;
    }
#pragma unroll
    for (int q = 0; q < CPL; q++) ops[(uint64_t)(i0 >> 4) * (GW * CPL) + base + q] = w[q];
    int low = cur[0];
#pragma unroll
    for (int q = 1; q < CPL; q++) low = min(low, cur[q]);
    if (gmin<GW>((uint64_t)low) >= (uint64_t)inf) return false;
  }
  return true;
}

// what a launch of the gap kernel works on: the gaps g0 <= g < g1 whose bucket is bk; soff / boff = the exclusive sums of the
// record words and of the slots, sbase / bbase = their values at g0: scratch and pool hold this launch's
struct FillLaunch {
  uint64_t g0, g1;
  int F, round, bk;
  const uint8_t *bkt;
  const uint64_t *soff, *boff;
  uint64_t sbase, bbase;
  uint32_t *scratch, *pool;
};

// one group of GW lanes per gap, GW CPL = fill_width(bk).  A gap whose result is exact gets dist, cnt and rptr (its runs, last
// first); one whose last round this was and whose result is not gets "no script"; any other goes to the next round
template <int GW, int CPL>
__global__ void __launch_bounds__(kTB) fm_fill_k(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ pat,
                                                 const uint64_t *__restrict__ off, uint64_t npat, FillSegs sg, FillLaunch la, uint8_t *__restrict__ rnd,
                                                 uint32_t *__restrict__ dist, uint64_t *__restrict__ cnt, uint64_t *__restrict__ rptr) {
  const int gl = threadIdx.x & (GW - 1);
  const uint64_t g = la.g0 + BID * (kTB / GW) + threadIdx.x / GW;
  if (g >= la.g1 || la.bkt[g] != (uint8_t)la.bk) return;        // (whole groups leave together: the shuffles stay inside groups)
  const FillGap x = fill_gap(off, npat, sg, n, (uint64_t)la.F, g);
  if (!x.ok) return;                                    // (the plan gave it a bucket: it is)
  const FillBand bd = fill_band(x.a, x.b, la.F, la.round);
  uint32_t *ops = la.scratch + (la.soff[g] - la.sbase);
  const int sh = bd.e - min(0, x.b - x.a), c = x.b - x.a + sh;          // (a, b) is cell c of the last row, c = hi + e < W
  int cur[CPL];
  uint64_t v = ~0ull;
  if (fill_forward<GW, CPL>(text + x.to, pat + x.po, x.a, x.b, sh, bd.cap + 1, gl, cur, ops)) {
#pragma unroll
    for (int q = 0; q < CPL; q++)
      if (gl * CPL + q == c) v = (uint64_t)cur[q];
    v = gmin<GW>(v);
  }
  if (v <= (uint64_t)bd.cap) {
    // the group's records, written by the lanes of this wave, are read by one: a fence of the block's scope orders them (as in
    // fmcigar.hip; no other group shares their 128-byte lines)
    __threadfence_block();
    if (gl == 0) {
      uint32_t *slot = la.pool + (la.boff[g] - la.bbase);
      cnt[g] = cig_walk(ops, GW * CPL, x.a, x.b, c, slot, fill_slot(bd, x.a, x.b));
      dist[g] = (uint32_t)v; rptr[g] = (uint64_t)slot; rnd[g] = kSettled;
    }
  } else if (gl == 0) {
    if (bd.last) { dist[g] = kFillNone; cnt[g] = 0; rnd[g] = kSettled; }
    else rnd[g] = (uint8_t)(la.round + 1);
  }
}

// what the passes that place runs read of the gaps
struct GapRuns {
  FillSegs sg;
  const uint32_t *dist;
  const uint64_t *cnt, *rptr;
};
// run r < cnt[g] of gap g, counted from the pattern's first byte: from its slot, or derived (a trivial gap has one)
__device__ __forceinline__ uint32_t gap_run(const GapRuns &gr, uint64_t g, uint64_t r) {
  if (gr.rptr[g]) return ((const uint32_t *)gr.rptr[g])[gr.cnt[g] - 1 - r];
  const uint32_t a = (uint32_t)(gr.sg.q1[g] - gr.sg.q0[g]), b = (uint32_t)(gr.sg.t1[g] - gr.sg.t0[g]);
  return !a ? b << 4 | kOpD : !b ? a << 4 | kOpI : 1u << 4 | (gr.dist[g] ? kOpX : kOpEq);
}

// cig[t] = the run of the segment that holds place t of the offsets
__global__ void __launch_bounds__(kTB) fill_place_k(GapRuns gr, uint64_t nseg, const uint64_t *__restrict__ cig_off, uint64_t total,
                                                    uint32_t *__restrict__ cig) {
  const uint64_t t = BID * kTB + threadIdx.x;
  if (t >= total) return;
  const uint64_t g = last_le(cig_off, nseg, t);          // (segments without runs share their offset with the next: the last one holds t)
  if (t - cig_off[g] < gr.cnt[g]) cig[t] = gap_run(gr, g, t - cig_off[g]);
}

// h[0] += offsets that decrease
__global__ void __launch_bounds__(kTB) fill_offsets_k(const uint64_t *__restrict__ off, uint64_t npat, unsigned long long *__restrict__ h) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p < npat && off[p] > off[p + 1]) atomicAdd(&h[0], 1ull);
}

template <int GW, int CPL>
void launch_fill(pfp_ctx *c, const uint8_t *text, uint64_t n, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const FillSegs &sg,
                 const FillLaunch &la, uint8_t *rnd, uint32_t *dist, uint64_t *cnt, uint64_t *rptr) {
  static_assert(GW == 16 || GW == 64, "a group is 16 lanes or a wave");
  fm_fill_k<GW, CPL><<<gdim(cdiv(la.g1 - la.g0, kTB / GW)), kTB, 0, c->stream>>>(text, n, pat, pat_off, npat, sg, la, rnd, dist, cnt, rptr);
}

// ---------------------------------------------------------------- members, trimming, stitching
struct Anchor { uint64_t i, len, t; };
__device__ __forceinline__ Anchor anchor_at(const uint64_t *__restrict__ anc, uint64_t a) { return Anchor{anc[3 * a], anc[3 * a + 1], anc[3 * a + 2]}; }

// one lane per aligned chain k (entry nal: cnt = 0): chain list[k] (NULL: k) of the call's, its pattern, its last anchor and its n
__global__ void __launch_bounds__(kTB) aln_heads_k(const uint32_t *__restrict__ list, uint64_t nal, const uint64_t *__restrict__ chain_off,
                                                   uint64_t npat, uint64_t C, const uint32_t *__restrict__ sb, const uint32_t *__restrict__ order,
                                                   uint64_t A, const uint32_t *__restrict__ cn, uint32_t *__restrict__ cpat,
                                                   uint32_t *__restrict__ last, uint64_t *__restrict__ cnt) {
  const uint64_t k = BID * kTB + threadIdx.x;
  if (k > nal) return;
  if (k == nal) { cnt[k] = 0; return; }
  const uint64_t c = list ? list[k] : k;
  uint64_t p = 0, x = A;
  if (c < C) {
    p = last_le(chain_off, npat, c);
    const uint64_t slot = sb[p] + (c - chain_off[p]);
    if (slot < A) x = order[slot];
  }
  cpat[k] = (uint32_t)p; last[k] = (uint32_t)(x < A ? x : 0);
  cnt[k] = x < A ? cn[x] : 0;
}

// one lane per aligned chain, at most `steps` members per launch: mem[mem_off[k] + r] = member r as an index inside its pattern's
// anchors.  rec[k] = {the anchor the walk stands at, the members left}.  ctr[0] += chains left unfinished
__global__ void __launch_bounds__(kTB) aln_members_k(uint64_t nal, const uint64_t *__restrict__ mem_off, const uint32_t *__restrict__ cpat,
                                                     const uint32_t *__restrict__ last, const uint64_t *__restrict__ anc_off,
                                                     const uint8_t *__restrict__ par, uint64_t steps, int first, uint2 *__restrict__ rec,
                                                     uint32_t *__restrict__ mem, unsigned long long *__restrict__ ctr) {
  const uint64_t k = BID * kTB + threadIdx.x;
  if (k >= nal) return;
  const uint64_t o = mem_off[k], b = anc_off[cpat[k]];
  uint2 r = first ? make_uint2(last[k], (uint32_t)(mem_off[k + 1] - o)) : rec[k];
  for (uint64_t work = 0; work < steps && r.y; work++) {
    r.y--;
    mem[o + r.y] = (uint32_t)(r.x - b);
    const uint32_t d = par[r.x];
    if (r.y && d && (uint64_t)r.x >= b + d) r.x -= d;   // (the peel counted n anchors along these parents)
  }
  rec[k] = r;
  if (r.y) atomicAdd(&ctr[0], 1ull);
}

// one lane per member slot s < M: the trimmed length of its anchor and the gap before it (member 0: an empty one)
__global__ void __launch_bounds__(kTB) aln_gaps_k(uint64_t nal, uint64_t M, const uint64_t *__restrict__ mem_off, const uint32_t *__restrict__ cpat,
                                                  const uint32_t *__restrict__ mem, const uint64_t *__restrict__ anc_off,
                                                  const uint64_t *__restrict__ anc, uint32_t *__restrict__ seg_pat, uint64_t *__restrict__ q0,
                                                  uint64_t *__restrict__ q1, uint64_t *__restrict__ t0, uint64_t *__restrict__ t1,
                                                  uint32_t *__restrict__ keep) {
  const uint64_t s = BID * kTB + threadIdx.x;
  if (s >= M) return;
  const uint64_t k = last_le(mem_off, nal, s), p = cpat[k], b = anc_off[p];
  const Anchor x = anchor_at(anc, b + mem[s]);
  seg_pat[s] = (uint32_t)p;
  if (s == mem_off[k]) { q0[s] = q1[s] = x.i; t0[s] = t1[s] = x.t; keep[s] = (uint32_t)x.len; return; }
  const Anchor y = anchor_at(anc, b + mem[s - 1]);
  const uint64_t qe = y.i + y.len, te = y.t + y.len;
  uint64_t o = 0;                                       // o <= len - 1: dq, dt >= 1
  if (qe > x.i) o = qe - x.i;
  if (te > x.t && te - x.t > o) o = te - x.t;
  if (o >= x.len) o = x.len - 1;                        // (anchors that no programme chained: keep the derivation's bound)
  q0[s] = qe; q1[s] = x.i + o; t0[s] = te; t1[s] = x.t + o; keep[s] = (uint32_t)(x.len - o);
  if (q1[s] < qe) q1[s] = qe;
  if (t1[s] < te) t1[s] = te;
}

// one lane per aligned chain: its script from its members' gaps and trimmed lengths, neighbouring runs of one operation merged.
// WRITE = false: cnt[k] = its runs, and aqs, ats, nm, unfilled (turn: the pattern offsets; an odd pattern is a read's strand 1 and
// aqs is turned into the read as given).  WRITE = true: the runs at cig_off[k]
template <bool WRITE>
__global__ void __launch_bounds__(kTB) aln_stitch_k(uint64_t nal, const uint64_t *__restrict__ mem_off, GapRuns gr, const uint32_t *__restrict__ keep,
                                                    const uint64_t *__restrict__ turn, uint64_t *__restrict__ cnt, AlnOut out,
                                                    const uint64_t *__restrict__ cig_off, uint64_t total, uint32_t *__restrict__ cig) {
  const uint64_t k = BID * kTB + threadIdx.x;
  if (k >= nal) return;
  const uint64_t s0 = mem_off[k], s1 = mem_off[k + 1];
  uint64_t runs = 0, at = WRITE ? cig_off[k] : 0;
  uint32_t op = 0, len = 0, nm = 0, unfilled = 0;       // the run that is open (op 0: none yet)
  auto emit = [&](uint32_t o, uint32_t count) {
    if (o == op) { len += count; return; }
    if (len) {
      if (WRITE && at + runs < total) cig[at + runs] = len << 4 | op;
      if (op != kOpEq) nm += len;
      runs++;
    }
    op = o; len = count;
  };
  for (uint64_t s = s0; s < s1; s++) {
    const uint32_t a = (uint32_t)(gr.sg.q1[s] - gr.sg.q0[s]), b = (uint32_t)(gr.sg.t1[s] - gr.sg.t0[s]);
    if (a | b) {
      if (gr.dist[s] != kFillNone) {
        for (uint64_t r = 0; r < gr.cnt[s]; r++) { const uint32_t w = gap_run(gr, s, r); emit(w & 15, w >> 4); }
      } else {
        unfilled++;
        if (a) emit(kOpI, a);
        if (b) emit(kOpD, b);
      }
    }
    emit(kOpEq, keep[s]);
  }
  emit(0, 0);                                           // closes the open run
  if (WRITE) return;
  cnt[k] = runs;
  uint32_t aqs = 0;
  uint64_t ats = 0;
  if (s1 > s0) {
    aqs = (uint32_t)gr.sg.q0[s0]; ats = gr.sg.t0[s0];
    const uint64_t p = gr.sg.pat[s0];
    if (turn && (p & 1)) aqs = (uint32_t)(turn[p + 1] - turn[p]) - aqs;
  }
  out.aqs[k] = aqs; out.ats[k] = ats; out.nm[k] = nm; out.unfilled[k] = unfilled;
}

// list[h] = the chain, among those of the 2 npat strands, that read r returns as its (h - hit_off[r])-th
__global__ void __launch_bounds__(kTB) long_list_k(const uint64_t *__restrict__ hit_off, uint64_t npat, uint64_t H,
                                                   const uint64_t *__restrict__ chain_off, const uint32_t *__restrict__ order, uint64_t C,
                                                   uint32_t *__restrict__ list) {
  const uint64_t h = BID * kTB + threadIdx.x;
  if (h >= H) return;
  const uint64_t r = last_le(hit_off, npat, h), slot = chain_off[2 * r] + (h - hit_off[r]);
  list[h] = slot < C ? order[slot] : (uint32_t)C;
}

}  // namespace

void fm_fill_check(const FmIndex &f, uint64_t max_fill) {
  require_text(f, "gaps");
  PFP_REQUIRE(max_fill <= PFP_FM_FILL_MAX_F, PFP_EINVAL, "max_fill = " + std::to_string(max_fill) + ": the edits of a gap are 0 .. " +
                                                          std::to_string(PFP_FM_FILL_MAX_F) + " (PFP_FM_FILL_MAX_F)");
}

void fm_fill_check_patterns(FmIndex &f, const uint64_t *pat_off, uint64_t npat) {
  pfp_ctx *c = f.c;
  if (!npat) return;
  DBuf<uint64_t> ctr(c, 1);
  ctr.zero();
  fill_offsets_k<<<gdim(cdiv(npat, kTB)), kTB, 0, c->stream>>>(pat_off, npat, (unsigned long long *)ctr.p);
  PFP_HIP(hipGetLastError());
  const uint64_t bad = read_scalar(c, ctr.p);
  PFP_REQUIRE(!bad, PFP_EINVAL, std::to_string(bad) + " pattern offsets decrease");
}

void fm_fill_gaps(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const FillSegs &sg, uint64_t ngap, uint64_t max_fill,
                  uint32_t *dist, FillRuns &out) {
  pfp_ctx *c = f.c;
  fm_fill_check(f, max_fill);
  out.total = 0;
  out.pool.clear();
  alloc_counts(c, out.cnt, ngap);
  out.rptr.alloc(c, ngap);
  if (!ngap) return;
  const uint8_t *text = f.text.p;
  const uint64_t n = f.n1 - 1, budget = std::max<uint64_t>(fill_scratch_from_env() / sizeof(uint32_t), 1);
  const int F = (int)max_fill;
  DBuf<uint8_t> rnd(c, ngap), bkt(c, ngap);
  DBuf<uint64_t> need(c, ngap + 1), bnd(c, ngap + 1), soff(c, ngap + 1), boff(c, ngap + 1), ctr(c, 16);
  const int stats = stats_from_env();
  ctr.zero();
  {
    KScope ks(c, "fm_fill_plan", 0);
    fill_classify_k<<<gdim(cdiv(ngap, kTB)), kTB, 0, c->stream>>>(text, n, pat, pat_off, npat, sg, ngap, max_fill, rnd.p, dist, out.cnt.p, out.rptr.p,
                                                                 stats ? (unsigned long long *)ctr.p : nullptr);
    PFP_HIP(hipGetLastError());
  }
  if (stats) {
    f.fill_stats[0] += ngap;
    f.fill_stats[1] += read_scalar(c, ctr.p);
  }
  std::vector<uint64_t> hs, hb;                          // the sums on the host, where one launch cannot hold all the records
  for (int round = 0; round < 8; round++) {             // (a gap's last round is at most round 4)
    uint64_t h[16], pending = 0;
    ctr.zero();
    {
      KScope ks(c, "fm_fill_plan", 0);
      fill_plan_k<<<gdim(cdiv(ngap + 1, kTB)), kTB, 0, c->stream>>>(pat_off, npat, sg, ngap, n, max_fill, round, rnd.p, bkt.p, need.p, bnd.p,
                                                                   stats, (unsigned long long *)ctr.p);
      PFP_HIP(hipGetLastError());
    }
    d2h(c, h, ctr.p, 16);
    sync(c);
    for (int bk = 0; bk < kFillBuckets; bk++) {
      pending += h[bk];
      if (stats) { f.fill_stats[2 + bk] += h[bk]; f.fill_stats[8 + bk] += h[8 + bk]; }
    }
    if (!pending) break;
    exclusive_sum_u64(c, need.p, soff.p, ngap + 1);
    exclusive_sum_u64(c, bnd.p, boff.p, ngap + 1);
    const uint64_t all = read_scalar(c, soff.p + ngap), slots = read_scalar(c, boff.p + ngap);
    const bool cut = all > budget;
    if (cut) {
      hs.resize(ngap + 1); hb.resize(ngap + 1);
      d2h(c, hs.data(), soff.p, ngap + 1);
      d2h(c, hb.data(), boff.p, ngap + 1);
      sync(c);
    }
    // consecutive gaps whose records fit the budget; one that needs more goes alone
    for (uint64_t g0 = 0, g1; g0 < ngap; g0 = g1) {
      g1 = ngap;
      if (cut)
        for (g1 = g0 + 1; g1 < ngap && hs[g1 + 1] - hs[g0] <= budget;) g1++;
      const uint64_t sbase = cut ? hs[g0] : 0, words = cut ? hs[g1] - hs[g0] : all;
      const uint64_t bbase = cut ? hb[g0] : 0, room = cut ? hb[g1] - hb[g0] : slots;
      if (!words) continue;                             // (nothing pending among them)
      DBuf<uint32_t> scratch(c, words);                 // (goes back to the pool in stream order)
      out.pool.emplace_back(c, room);
      for (int bk = 0; bk < kFillBuckets; bk++) {
        if (!h[bk]) continue;
        const FillLaunch la{g0, g1, F, round, bk, bkt.p, soff.p, boff.p, sbase, bbase, scratch.p, out.pool.back().p};
        KScope ks(c, kFillName[bk], 0);
        if (bk == 0) launch_fill<16, 1>(c, text, n, pat, pat_off, npat, sg, la, rnd.p, dist, out.cnt.p, out.rptr.p);
        else if (bk == 1) launch_fill<16, 2>(c, text, n, pat, pat_off, npat, sg, la, rnd.p, dist, out.cnt.p, out.rptr.p);
        else if (bk == 2) launch_fill<16, 4>(c, text, n, pat, pat_off, npat, sg, la, rnd.p, dist, out.cnt.p, out.rptr.p);
        else if (bk == 3) launch_fill<64, 4>(c, text, n, pat, pat_off, npat, sg, la, rnd.p, dist, out.cnt.p, out.rptr.p);
        else if (bk == 4) launch_fill<64, 16>(c, text, n, pat, pat_off, npat, sg, la, rnd.p, dist, out.cnt.p, out.rptr.p);
        else launch_fill<64, 65>(c, text, n, pat, pat_off, npat, sg, la, rnd.p, dist, out.cnt.p, out.rptr.p);
        PFP_HIP(hipGetLastError());
      }
    }
  }
  sync(c);                                              // (the plan goes back when this returns)
}

void fm_fill_runs(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const FillSegs &sg, uint64_t nseg, uint64_t max_fill,
                  uint32_t *dist, uint64_t *cig_off, FillRuns &out) {
  pfp_ctx *c = f.c;
  fm_fill_check(f, max_fill);
  fm_fill_check_patterns(f, pat_off, npat);
  fm_fill_gaps(f, pat, pat_off, npat, sg, nseg, max_fill, dist, out);
  exclusive_sum_u64(c, out.cnt.p, cig_off, nseg + 1);
  out.total = read_scalar(c, cig_off + nseg);
}

void fm_fill_write(FmIndex &f, const FillSegs &sg, uint64_t nseg, const uint32_t *dist, const FillRuns &runs, const uint64_t *cig_off, uint32_t *cig) {
  pfp_ctx *c = f.c;
  if (!runs.total) return;
  KScope ks(c, "fm_fill_place", 0);
  fill_place_k<<<gdim(cdiv(runs.total, kTB)), kTB, 0, c->stream>>>(GapRuns{sg, dist, runs.cnt.p, runs.rptr.p}, nseg, cig_off, runs.total, cig);
  PFP_HIP(hipGetLastError());
}

void fm_fill(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const FillSegs &sg, uint64_t nseg, uint64_t max_fill,
             uint32_t *dist, uint64_t *cig_off, uint32_t *cig) {
  FillRuns runs;
  fm_fill_runs(f, pat, pat_off, npat, sg, nseg, max_fill, dist, cig_off, runs);
  if (cig) fm_fill_write(f, sg, nseg, dist, runs, cig_off, cig);
  sync(f.c);                                            // (the slots go back when this returns)
}

void fm_chain_align_runs(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint64_t *anc_off, const uint64_t *anc,
                         const uint64_t *chain_off, const ChainSel &cs, const uint32_t *list, uint64_t nal, uint64_t max_fill, bool turn,
                         const AlnOut &out, uint64_t *cig_off, ChainAln &st) {
  pfp_ctx *c = f.c;
  fm_fill_check(f, max_fill);
  st.nal = nal; st.M = st.total = 0;
  st.mem_off.alloc(c, nal + 1);
  if (!nal) {
    PFP_HIP(hipMemsetAsync(st.mem_off.p, 0, sizeof(uint64_t), c->stream));
    PFP_HIP(hipMemsetAsync(cig_off, 0, sizeof(uint64_t), c->stream));
    sync(c);
    return;
  }
  const uint64_t A = cs.order.n;
  DBuf<uint32_t> cpat(c, nal), last(c, nal);
  DBuf<uint64_t> cnt(c, nal + 1), ctr(c, 4);
  {
    KScope ks(c, "fm_aln_members", 0);
    aln_heads_k<<<gdim(cdiv(nal + 1, kTB)), kTB, 0, c->stream>>>(list, nal, chain_off, npat, cs.total, cs.sb.p, cs.order.p, A, cs.n.p, cpat.p, last.p,
                                                                cnt.p);
    PFP_HIP(hipGetLastError());
    exclusive_sum_u64(c, cnt.p, st.mem_off.p, nal + 1);
  }
  const uint64_t M = st.M = read_scalar(c, st.mem_off.p + nal);
  st.mem.alloc(c, M); st.seg_pat.alloc(c, M); st.keep.alloc(c, M); st.dist.alloc(c, M); st.seg64.alloc(c, 4 * M);
  {
    DBuf<uint2> rec(c, nal);
    const uint64_t steps = member_steps_from_env();
    bounded_launches(c, "fm_aln_members", ctr, [&](int first, unsigned long long *d_ctr) {
      aln_members_k<<<gdim(cdiv(nal, kTB)), kTB, 0, c->stream>>>(nal, st.mem_off.p, cpat.p, last.p, anc_off, cs.par.p, steps, first, rec.p, st.mem.p,
                                                                d_ctr);
    }, [](const uint64_t *) {});
  }
  uint64_t *q0 = st.seg64.p, *q1 = q0 + M, *t0 = q1 + M, *t1 = t0 + M;
  const FillSegs sg{st.seg_pat.p, q0, q1, t0, t1};
  if (M) {
    KScope ks(c, "fm_aln_gaps", 0);
    aln_gaps_k<<<gdim(cdiv(M, kTB)), kTB, 0, c->stream>>>(nal, M, st.mem_off.p, cpat.p, st.mem.p, anc_off, anc, st.seg_pat.p, q0, q1, t0, t1, st.keep.p);
    PFP_HIP(hipGetLastError());
  }
  fm_fill_gaps(f, pat, pat_off, npat, sg, M, max_fill, st.dist.p, st.runs);
  {
    KScope ks(c, "fm_aln_stitch", 0);
    aln_stitch_k<false><<<gdim(cdiv(nal, kTB)), kTB, 0, c->stream>>>(nal, st.mem_off.p, GapRuns{sg, st.dist.p, st.runs.cnt.p, st.runs.rptr.p}, st.keep.p,
                                                                    turn ? pat_off : nullptr, cnt.p, out, nullptr, 0, nullptr);
    PFP_HIP(hipGetLastError());
    exclusive_sum_u64(c, cnt.p, cig_off, nal + 1);
  }
  st.total = read_scalar(c, cig_off + nal);             // (syncs: the heads and the counts go back when this returns)
}

void fm_chain_align_write(FmIndex &f, const ChainAln &st, const uint64_t *cig_off, uint32_t *cig) {
  pfp_ctx *c = f.c;
  if (!st.total) return;
  const uint64_t M = st.M;
  uint64_t *q0 = st.seg64.p;
  const FillSegs sg{st.seg_pat.p, q0, q0 + M, q0 + 2 * M, q0 + 3 * M};
  KScope ks(c, "fm_aln_stitch", 0);
  aln_stitch_k<true><<<gdim(cdiv(st.nal, kTB)), kTB, 0, c->stream>>>(st.nal, st.mem_off.p, GapRuns{sg, st.dist.p, st.runs.cnt.p, st.runs.rptr.p},
                                                                    st.keep.p, nullptr, nullptr, AlnOut{}, cig_off, st.total, cig);
  PFP_HIP(hipGetLastError());
}

void fm_map_long_align(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t npat, const uint64_t *anc_off2, const uint64_t *anc,
                       const uint64_t *hit_off, const LongSel &sel, uint64_t max_fill, const AlnOut &out, uint64_t *cig_off, ChainAln &st) {
  pfp_ctx *c = f.c;
  DBuf<uint32_t> list(c, sel.H);
  if (sel.H) {
    KScope ks(c, "fm_aln_members", 0);
    long_list_k<<<gdim(cdiv(sel.H, kTB)), kTB, 0, c->stream>>>(hit_off, npat, sel.H, sel.chain_off.p, sel.order.p, sel.score.n, list.p);
    PFP_HIP(hipGetLastError());
  }
  fm_chain_align_runs(f, pat2, pat2_off, 2 * npat, anc_off2, anc, sel.chain_off.p, sel.cs, list.p, sel.H, max_fill, true, out, cig_off, st);
}

}  // namespace pfp
