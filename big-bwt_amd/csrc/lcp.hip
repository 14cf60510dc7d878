// lcp.hip -- the LCP array of a BWT, its thresholds, and matching statistics with thresholds over an FmIndex with text.  The
// reference has no counterpart; the sources are Karkkainen, Manzini, Puglisi, "Permuted longest-common-prefix array" (CPM 2009)
// for the irreducible values, Bannai, Gagie, I, "Refining the r-index" (2020) for thresholds and Rossi, Oliva, Langmead, Gagie,
// Boucher, "MONI: a pangenomic index for finding maximal exact matches" (2022) for the two passes.  Conventions and the
// definitions: include/pfpgpu.h, "The LCP array and thresholds".
//
//   1. Irreducible values.  Row j starts a run exactly when LCP[j] is irreducible; then SA[j] and SA[j-1] are samples of the
//      index (rs_sa[k], re_sa[k-1]) and LCP[j] is their longest common extension on the text.  First launch: one group of 16
//      lanes per run compares at most kIrrGroup KiB (lce16).  A run that uses its budget up goes on a list; the following
//      launches give every listed run a whole block (16 KiB per iteration, at most kIrrBlock iterations per launch) and resume
//      from the bytes matched so far, until the list is empty.
//   2. PLCP in text order.  PLCP[i] + i = PLCP[i0] + i0 for the largest run-start SA value i0 <= i, and PLCP[i] + i never
//      decreases, so: scatter irr[k] + rs_sa[k] to position rs_sa[k], a library running maximum, subtract i.
//   3. LCP[j] = PLCP[SA[j]]: the inverter's splitter walk (unbwt.hip, lcp_by_rows) knows SA[j] at every row.
//   4. Thresholds.  Per run the minimum of LCP and the smallest row that has it (two passes of atomicMin, one per run and wave);
//      a sparse table over blocks of 32 runs answers "leftmost minimum over runs (p, k)" with at most 64 run values and two
//      table entries read; prev(k) comes from one stable library sort of the run numbers by their byte.
//   5. Matching statistics.  Pass 1 walks a pattern right to left with one rank per step and writes pos; it reads no text.
//      Pass 2 walks left to right and extends on the text from max(len[i-1] - 1, 0): at most m bytes matched per pattern.
// Bounds: every loop is bounded by a launch's budget, a directory's size or the pattern length; run numbers are clamped below
// runs and positions to [0, n] before they index anything; thresholds are only ever compared.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"

namespace pfp {

namespace {

constexpr uint64_t kIrrGroup = 16;          // iterations of 1024 bytes a group of 16 lanes gives a run (the first launch)
constexpr uint64_t kIrrBlock = 4096;        // iterations of kBlockBytes a block gives a listed run per launch
constexpr uint64_t kBlockBytes = 16384;     // 256 threads x 4 rows x 16 bytes
constexpr int kRmqLog = 5;                  // runs per block of the range-minimum table
constexpr uint64_t kRmq = 1ull << kRmqLog;

__device__ __forceinline__ void atomic_min_u64(uint64_t *p, uint64_t v) { atomicMin((unsigned long long *)p, (unsigned long long)v); }

// ---------------------------------------------------------------- 1. irreducible values
// one group of 16 lanes per run: irr[k] = LCE(SA[s_k], SA[e_{k-1}]), at most budget KiB of it; a run that needs more is listed
template <class I>
__global__ void __launch_bounds__(kTB) lcp_irr_group(const uint8_t *__restrict__ text, uint64_t n, const I *__restrict__ rs_sa,
                                                     const I *__restrict__ re_sa, uint64_t runs, uint64_t budget, uint64_t *__restrict__ irr,
                                                     I *__restrict__ todo, unsigned long long *__restrict__ ctr) {
  const int gl = threadIdx.x & 15;
  const uint64_t k = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (k >= runs) return;                               // (whole groups leave together: the shuffles stay inside groups)
  uint64_t v = 0;
  bool more = false;
  if (k) {
    uint64_t x = rs_sa[k], y = re_sa[k - 1], work = 0;
    if (x > n) x = n;
    if (y > n) y = n;
    const uint64_t room = n - (x > y ? x : y), cap = budget * 1024;
    v = lce16(text, n, x, y, cap, gl, work);
    more = v >= cap && cap < room;
  }
  if (gl == 0) {
    irr[k] = v;
    if (more) todo[atomicAdd(&ctr[0], 1ull)] = (I)k;
  }
}

// one block per listed run: resumes at irr[k] bytes, at most budget iterations of kBlockBytes; ctr[1] += runs left unfinished
template <class I>
__global__ void __launch_bounds__(kTB) lcp_irr_block(const uint8_t *__restrict__ text, uint64_t n, const I *__restrict__ rs_sa,
                                                     const I *__restrict__ re_sa, uint64_t runs, uint64_t budget, uint64_t *__restrict__ irr,
                                                     I *__restrict__ todo, uint64_t listed, unsigned long long *__restrict__ ctr) {
  __shared__ uint64_t wmin[kTB / 64];
  if (BID >= listed) return;
  const uint64_t k = todo[BID];
  if (k == 0 || k >= runs) return;                     // (~0: finished in an earlier launch; uniform per block)
  uint64_t x = rs_sa[k], y = re_sa[k - 1];
  if (x > n) x = n;
  if (y > n) y = n;
  const uint64_t room = n - (x > y ? x : y);
  uint64_t done = irr[k];
  if (done > room) done = room;
  const uint64_t cap = room - done < budget * kBlockBytes ? room : done + budget * kBlockBytes;
  uint64_t res = cap;
  for (uint64_t base = done; base < cap; base += kBlockBytes) {     // (base and cap are the same in all threads)
    uint4 u[4], v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint64_t o = base + 4096 * j + 16 * (uint64_t)threadIdx.x;
      u[j] = v[j] = make_uint4(0, 0, 0, 0);
      if (o < cap) { u[j] = ld16u(text + x + o); v[j] = ld16u(text + y + o); }      // (below text + n + 16: the copy's padding)
    }
    uint64_t mine = first_diff_rows<4096>(u, v, base + 16 * (uint64_t)threadIdx.x, cap);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint64_t o = __shfl_xor(mine, d, 64); mine = o < mine ? o : mine; }
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = mine;
    __syncthreads();
    uint64_t m = wmin[0];
#pragma unroll
    for (int i = 1; i < kTB / 64; i++) m = wmin[i] < m ? wmin[i] : m;
    __syncthreads();
    if (m < cap) { res = m; break; }
  }
  if (threadIdx.x == 0) {
    irr[k] = res;
    if (res < cap || cap >= room) todo[BID] = ~(I)0;
    else atomicAdd(&ctr[1], 1ull);
  }
}

// ---------------------------------------------------------------- 2. PLCP in text order
// key[SA[s_k]] = irr[k] + SA[s_k] (key zeroed before; distinct runs have distinct SA values)
template <class I>
__global__ void __launch_bounds__(kTB) lcp_scatter(const I *__restrict__ rs_sa, const uint64_t *__restrict__ irr, uint64_t runs, uint64_t n,
                                                   I *__restrict__ key) {
  const uint64_t k = BID * kTB + threadIdx.x;
  if (k >= runs) return;
  uint64_t x = rs_sa[k];
  if (x > n) x = n;
  const uint64_t v = irr[k] + x;
  key[x] = (I)(v > n ? n : v);
}
// in place: the running maximum of the keys -> PLCP[i] = max - i (0 where no run start lies at or before i: wrong samples only)
template <class I>
__global__ void __launch_bounds__(kTB) lcp_plcp(I *__restrict__ key, uint64_t n1) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i >= n1) return;
  const uint64_t v = key[i];
  key[i] = (I)(v > i ? v - i : 0);
}

// ---------------------------------------------------------------- 4. thresholds
// pass 0: runmin[k] = min of LCP over run k; pass 1: runarg[k] = the smallest row of run k whose LCP is runmin[k].  One lane per
// row; lanes of one run are neighbours, so a wave reduces by run with shuffles and its last lane of each run does the atomic.
template <class I>
__global__ void __launch_bounds__(kTB) lcp_runmin(const I *__restrict__ lcp, uint64_t n1, const uint64_t *__restrict__ rbits,
                                                  const uint64_t *__restrict__ rdir, uint64_t runs, int pass, uint64_t *__restrict__ runmin,
                                                  uint64_t *__restrict__ runarg) {
  const uint64_t j = BID * kTB + threadIdx.x;
  const int lane = threadIdx.x & 63;
  uint64_t k = ~0ull, v = ~0ull;
  if (j < n1) {
    k = j + 1 < n1 ? bit_rank(rbits, rdir, j + 1) : runs;          // run starts in [0, j]: row j lies in run k - 1
    k = k ? k - 1 : 0;
    if (k >= runs) k = runs - 1;
    v = lcp[j];
    if (pass) v = v == runmin[k] ? j : ~0ull;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t ov = __shfl_up(v, d, 64), ok = __shfl_up(k, d, 64);
    if (lane >= d && ok == k && ov < v) v = ov;
  }
  const uint64_t nk = __shfl_down(k, 1, 64);
  if (j < n1 && (lane == 63 || nk != k) && v != ~0ull) atomic_min_u64(pass ? &runarg[k] : &runmin[k], v);
}

// the leftmost run of [lo, hi] (inclusive, lo <= hi < runs) with the smallest runmin, scanning
__device__ __forceinline__ uint64_t scan_min(const uint64_t *__restrict__ runmin, uint64_t lo, uint64_t hi) {
  uint64_t best = lo, bv = runmin[lo];
  for (uint64_t k = lo + 1; k <= hi; k++) {
    const uint64_t v = runmin[k];
    if (v < bv) { bv = v; best = k; }
  }
  return best;
}
// level 0 of the table: tab[b] = the leftmost minimum of block b
template <class I>
__global__ void __launch_bounds__(kTB) lcp_rmq0(const uint64_t *__restrict__ runmin, uint64_t runs, uint64_t nb, I *__restrict__ tab) {
  const uint64_t b = BID * kTB + threadIdx.x;
  if (b >= nb) return;
  const uint64_t lo = b << kRmqLog, hi = lo + kRmq - 1 < runs - 1 ? lo + kRmq - 1 : runs - 1;
  tab[b] = (I)scan_min(runmin, lo, hi);
}
// level l from level l - 1: blocks [b, b + 2^l) = [b, b + 2^(l-1)) and [b + 2^(l-1), b + 2^l); the left half wins a tie
template <class I>
__global__ void __launch_bounds__(kTB) lcp_rmq_up(const uint64_t *__restrict__ runmin, uint64_t nb, uint64_t half, const I *__restrict__ below,
                                                  I *__restrict__ tab) {
  const uint64_t b = BID * kTB + threadIdx.x;
  if (b + 2 * half > nb) return;
  const uint64_t x = below[b], y = below[b + half];
  tab[b] = (I)(runmin[x] <= runmin[y] ? x : y);
}

// sorted position i of (byte, run): thr of run k = sv[i]; its prev is sv[i - 1] where the bytes agree
template <class I>
__global__ void __launch_bounds__(kTB) lcp_thr(const I *__restrict__ sk, const I *__restrict__ sv, uint64_t runs, const uint64_t *__restrict__ runmin,
                                               const uint64_t *__restrict__ runarg, const I *__restrict__ tab, uint64_t nb,
                                               const I *__restrict__ rs_row, const I *__restrict__ lcp, uint64_t n1, I *__restrict__ thr,
                                               uint64_t *__restrict__ thr64) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i >= runs) return;
  uint64_t k = sv[i];
  if (k >= runs) k = runs - 1;
  uint64_t t = 0;
  if (i && sk[i - 1] == sk[i]) {
    uint64_t p = sv[i - 1];
    if (p + 2 <= k) {                                  // (always: neighbouring runs differ in their byte)
      const uint64_t lo = p + 1, hi = k - 1, bl = lo >> kRmqLog, bh = hi >> kRmqLog;
      uint64_t best;
      if (bl == bh) {
        best = scan_min(runmin, lo, hi);
      } else {
        best = scan_min(runmin, lo, ((bl + 1) << kRmqLog) - 1);
        if (bl + 1 < bh) {                             // whole blocks bl + 1 .. bh - 1: two table entries cover them
          const uint64_t cnt = bh - bl - 1;
          const int l = 63 - __clzll((long long)cnt);
          uint64_t x = tab[(uint64_t)l * nb + bl + 1], y = tab[(uint64_t)l * nb + bh - (1ull << l)];
          if (x >= runs) x = runs - 1;
          if (y >= runs) y = runs - 1;
          const uint64_t mid = runmin[x] <= runmin[y] ? x : y;
          if (runmin[mid] < runmin[best]) best = mid;
        }
        const uint64_t last = scan_min(runmin, bh << kRmqLog, hi);
        if (runmin[last] < runmin[best]) best = last;
      }
      uint64_t row = rs_row[k];
      if (row >= n1) row = n1 - 1;
      t = (uint64_t)lcp[row] < runmin[best] ? row : runarg[best];
    }
  }
  if (thr) thr[k] = (I)t;
  if (thr64) thr64[k] = t;
}

// the run bytes as sort keys, the run numbers as values
template <class I>
__global__ void __launch_bounds__(kTB) lcp_runbytes(const uint8_t *__restrict__ bwt, const I *__restrict__ rs_row, uint64_t runs, uint64_t n1,
                                                    I *__restrict__ key, I *__restrict__ val) {
  const uint64_t k = BID * kTB + threadIdx.x;
  if (k >= runs) return;
  uint64_t row = rs_row[k];
  if (row >= n1) row = n1 - 1;
  key[k] = (I)bwt[row];
  val[k] = (I)k;
}

template <class I>
__global__ void __launch_bounds__(kTB) lcp_widen(const I *__restrict__ in, uint64_t cnt, uint64_t *__restrict__ out) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i < cnt) out[i] = in[i];
}
// thr[k] = the k-th 5-byte value of a .thr_pos file, clamped to the rows
template <class I>
__global__ void __launch_bounds__(kTB) lcp_thr_load(const uint8_t *__restrict__ thr5, uint64_t runs, uint64_t n1, I *__restrict__ thr) {
  const uint64_t k = BID * kTB + threadIdx.x;
  if (k >= runs) return;
  const uint64_t v = ld5(thr5, 5 * k, 5 * runs);
  thr[k] = (I)(v > n1 ? n1 : v);
}

// I values -> 5-byte ints, through a chunk of u64 (pack5_dev reads those)
template <class I>
void pack5_from(pfp_ctx *c, const I *in, uint64_t cnt, uint8_t *out5) {
  const uint64_t chunk = 16ull << 20;                   // (a multiple of 16: every chunk's bytes start on a 16-byte stride of out5)
  DBuf<uint64_t> tmp(c, std::min(cnt, chunk));
  for (uint64_t at = 0; at < cnt; at += chunk) {
    const uint64_t k = std::min(chunk, cnt - at);
    lcp_widen<I><<<gdim(cdiv(k, kTB)), kTB, 0, c->stream>>>(in + at, k, tmp.p);
    PFP_HIP(hipGetLastError());
    pack5_dev(c, tmp.p, k, out5 + 5 * at);
  }
}

template <class I>
void lcp_t(FmIndex &f, const LcpOut &o) {
  pfp_ctx *c = f.c;
  const uint64_t n1 = f.n1, n = n1 - 1, r = f.runs;
  const I *rs_sa = as<I>(f.rs_sa), *re_sa = as<I>(f.re_sa), *rs_row = as<I>(f.rs_row);
  // 1. irreducible values
  DBuf<uint64_t> irr(c, r);
  {
    DBuf<I> todo(c, r);
    DBuf<uint64_t> ctr(c, 2);
    ctr.zero();
    {
      KScope ks(c, "lcp_irr_group", 0);
      lcp_irr_group<I><<<gdim(cdiv(r, kTB / 16)), kTB, 0, c->stream>>>(f.text.p, n, rs_sa, re_sa, r, budget_from_env(kIrrGroup), irr.p, todo.p,
                                                                      (unsigned long long *)ctr.p);
      PFP_HIP(hipGetLastError());
    }
    f.ms_stats[0] += 1;
    const uint64_t listed = read_scalar(c, ctr.p);
    const uint64_t budget = budget_from_env(kIrrBlock);
    // (not bounded_launches: no launch at all where nothing is listed, only ctr[1] is zeroed, and the count comes by read_scalar)
    for (uint64_t left = listed; left;) {               // every launch matches at least kBlockBytes more of every listed run
      PFP_HIP(hipMemsetAsync(ctr.p + 1, 0, 8, c->stream));
      {
        KScope ks(c, "lcp_irr_block", 0);
        lcp_irr_block<I><<<gdim(listed), kTB, 0, c->stream>>>(f.text.p, n, rs_sa, re_sa, r, budget, irr.p, todo.p, listed,
                                                              (unsigned long long *)ctr.p);
        PFP_HIP(hipGetLastError());
      }
      f.ms_stats[0] += 1;
      left = read_scalar(c, ctr.p + 1);
    }
  }
  // 2. PLCP in text order, 3. LCP by rows
  DBuf<I> lcp(c, n1);                                   // (first the keys of the running maximum, then the array by rows)
  {
    DBuf<I> plcp(c, n1);
    lcp.zero();
    {
      KScope ks(c, "lcp_plcp", r * (8 + 2 * sizeof(I)) + 4 * n1 * sizeof(I));
      lcp_scatter<I><<<gdim(cdiv(r, kTB)), kTB, 0, c->stream>>>(rs_sa, irr.p, r, n, lcp.p);
      PFP_HIP(hipGetLastError());
      inclusive_max<I>(c, lcp.p, plcp.p, n1);
      lcp_plcp<I><<<gdim(cdiv(n1, kTB)), kTB, 0, c->stream>>>(plcp.p, n1);
      PFP_HIP(hipGetLastError());
    }
    lcp_by_rows<I>(c, f.bwt.p, n1, plcp.p, lcp.p);
  }
  irr.release();
  if (o.lcp64) {
    lcp_widen<I><<<gdim(cdiv(n1, kTB)), kTB, 0, c->stream>>>(lcp.p, n1, o.lcp64);
    PFP_HIP(hipGetLastError());
  }
  if (o.lcp5) pack5_from<I>(c, lcp.p, n1, o.lcp5);
  if (!o.thr64 && !o.thr5 && !o.keep) return;
  // 4. thresholds
  DBuf<uint8_t> thr(c, r * sizeof(I));
  {
    DBuf<uint64_t> runmin(c, r), runarg(c, r);
    PFP_HIP(hipMemsetAsync(runmin.p, 0xFF, r * 8, c->stream));
    PFP_HIP(hipMemsetAsync(runarg.p, 0xFF, r * 8, c->stream));
    {
      KScope ks(c, "lcp_runmin", 2 * n1 * (sizeof(I) + 0.140625));
      for (int pass = 0; pass < 2; pass++) {
        lcp_runmin<I><<<gdim(cdiv(n1, kTB)), kTB, 0, c->stream>>>(lcp.p, n1, f.rs.bits.p, f.rs.dir.p, r, pass, runmin.p, runarg.p);
        PFP_HIP(hipGetLastError());
      }
    }
    const uint64_t nb = cdiv(r, kRmq);
    const int levels = bits_for(nb);                    // level l exists while 2^l <= nb
    DBuf<I> tab(c, (uint64_t)levels * nb);
    {
      KScope ks(c, "lcp_rmq", r * 8 + (uint64_t)levels * nb * 3 * sizeof(I));
      lcp_rmq0<I><<<gdim(cdiv(nb, kTB)), kTB, 0, c->stream>>>(runmin.p, r, nb, tab.p);
      PFP_HIP(hipGetLastError());
      for (int l = 1; l < levels && (2ull << (l - 1)) <= nb; l++) {
        lcp_rmq_up<I><<<gdim(cdiv(nb, kTB)), kTB, 0, c->stream>>>(runmin.p, nb, 1ull << (l - 1), tab.p + (uint64_t)(l - 1) * nb, tab.p + (uint64_t)l * nb);
        PFP_HIP(hipGetLastError());
      }
    }
    DBuf<I> key(c, r), val(c, r), sk(c, r), sv(c, r);
    lcp_runbytes<I><<<gdim(cdiv(r, kTB)), kTB, 0, c->stream>>>(f.bwt.p, rs_row, r, n1, key.p, val.p);
    PFP_HIP(hipGetLastError());
    {
      SortTag tag("runs by byte");
      sort_pairs<I, I>(c, key.p, sk.p, val.p, sv.p, r, 0, 8);
    }
    key.release(); val.release();
    DBuf<uint64_t> thr64;
    if (!o.thr64 && o.thr5) thr64.alloc(c, r);
    uint64_t *t64 = o.thr64 ? o.thr64 : thr64.p;
    {
      KScope ks(c, "lcp_thr", r * (4 * sizeof(I) + 16 + 8));
      lcp_thr<I><<<gdim(cdiv(r, kTB)), kTB, 0, c->stream>>>(sk.p, sv.p, r, runmin.p, runarg.p, tab.p, nb, rs_row, lcp.p, n1, as<I>(thr), t64);
      PFP_HIP(hipGetLastError());
    }
    if (o.thr5) pack5_dev(c, t64, r, o.thr5);
    sync(c);
  }
  if (o.keep) { f.thr = std::move(thr); f.has_thr = true; }
}

// ---------------------------------------------------------------- 5. matching statistics with thresholds
// at most 15 bytes of p, the first in the lowest byte: never reads p[cnt] (patterns carry no padding)
__device__ __forceinline__ uint4 ld_tail(const uint8_t *__restrict__ p, int cnt) {
  uint64_t lo = 0, hi = 0;
  for (int i = 0; i < cnt && i < 8; i++) lo |= (uint64_t)p[i] << (8 * i);
  for (int i = 8; i < cnt && i < 16; i++) hi |= (uint64_t)p[i] << (8 * (i - 8));
  return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
// the common prefix of p[0 .. cap) and t[0 .. cap): lce16 with one side a pattern.  Reads of t stay below t + cap + 16
__device__ __forceinline__ uint64_t lce16_pat(const uint8_t *__restrict__ p, const uint8_t *__restrict__ t, uint64_t cap, int gl, uint64_t &work) {
  for (uint64_t done = 0; done < cap; done += 1024) {   // (done and cap are the same in all 16 lanes)
    uint4 u[4], v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint64_t o = done + 256 * j + 16 * (uint64_t)gl;
      u[j] = v[j] = make_uint4(0, 0, 0, 0);
      if (o < cap) {
        v[j] = ld16u(t + o);
        if (cap - o >= 16) u[j] = ld16u(p + o);
        else { u[j] = ld_tail(p + o, (int)(cap - o)); v[j] = keep_bytes16(v[j], (int)(cap - o)); }
      }
    }
    work++;
    const uint64_t m = first_diff_1024(u, v, done, cap, gl);
    if (m < cap) return m;
  }
  return cap;
}

// pass 1, one group of 16 lanes per pattern, right to left: pos_out[t] = the position the state holds after byte t (2^64 - 1:
// none).  Records and counters as fm_ms_k: ctr[0] += unfinished, ctr[1] += refused, stats: ctr[2] += steps that jumped
template <class I>
__global__ void __launch_bounds__(kTB) fm_ms_thr1(FmArgs<I> a, const I *__restrict__ re_sa, const I *__restrict__ thr, const uint8_t *__restrict__ pat,
                                                  const uint64_t *__restrict__ off, uint64_t npat, MsRec *__restrict__ rec, int first, uint64_t budget,
                                                  uint64_t *__restrict__ pos_out, unsigned long long *__restrict__ ctr, int stats) {
  __shared__ uint8_t code[256];
  PatGroup g;
  if (!pat_group(code, a.codes, off, npat, g)) return;
  const int gl = g.gl;
  const uint64_t p = g.p, o0 = g.o0, o1 = g.o1;
  MsRec s = ms_start(first, rec + p, o0, o1, a.n1 - 1, ctr, gl);
  uint64_t work = 0, jumps = 0;
  while (s.t > o0 && work < budget) {
    s.t--;
    work++;
    const uint32_t c = pat[s.t], k = code[c];
    uint64_t out = ~0ull;
    if (k != kAbsent) {
      const uint32_t c4 = c * 0x01010101u;
      const uint64_t target = lf_at(a, s.q, c4, k, gl);
      if (a.bwt[s.q] == c) {
        s.q = target; s.pos -= 1;
        out = s.pos;
      } else {
        const MsNeighbours nb = ms_neighbours(a, s.q, target, c4, k, gl);
        if (nb.qp != ~0ull || nb.qs != ~0ull) {        // (no c at all: only for a directory that is not this BWT's; the state stays)
          uint64_t rs = 0;
          bool up = nb.qs == ~0ull;
          if (!up) {
            rs = run_starting_at(a, nb.qs);
            up = nb.qp != ~0ull && s.q < (uint64_t)thr[rs];
          }
          if (up) {
            s.q = target - 1; s.pos = (uint64_t)re_sa[run_ending_at(a, nb.qp)] - 1;
          } else {
            s.q = target; s.pos = (uint64_t)a.rs_sa[rs] - 1;
          }
          out = s.pos;
          jumps++;
        }
      }
    }
    if (gl == 0) pos_out[s.t] = out;
  }
  if (gl == 0) {
    rec[p] = s;
    if (s.t > o0) atomicAdd(&ctr[0], 1ull);
    if (stats) atomicAdd(&ctr[2], (unsigned long long)jumps);
  }
}

// pass 2, left to right: the record holds t = the byte in hand, l = the bytes matched at it so far, q = 1 while its extension is
// under way (a launch's budget ran out inside it).  stats: ctr[3] += bytes matched
__global__ void __launch_bounds__(kTB) fm_ms_thr2(const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ pat,
                                                  const uint64_t *__restrict__ off, uint64_t npat, MsRec *__restrict__ rec, int first, uint64_t budget,
                                                  uint32_t *__restrict__ len_out, uint64_t *__restrict__ pos, unsigned long long *__restrict__ ctr,
                                                  int stats) {
  const int gl = threadIdx.x & 15;
  const uint64_t p = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (p >= npat) return;
  const uint64_t o0 = off[p], o1 = off[p + 1], end = o1 > o0 ? o1 : o0;
  MsRec s = first ? MsRec{o0, 0, 0, 0} : rec[p];
  uint64_t work = 0, matched = 0;
  while (s.t < end && work < budget) {
    const uint64_t ps = pos[s.t];
    if (!s.q) {
      work++;
      s.l = ps == ~0ull || !s.l ? 0 : s.l - 1;
      s.q = 1;
    }
    bool paused = false;
    if (ps != ~0ull) {
      const uint64_t x = ps > n ? n : ps;
      const uint64_t cap = n - x < end - s.t ? n - x : end - s.t;
      if (s.l > cap) s.l = cap;                         // (only for positions that are not this text's)
      if (s.l < cap) {
        const uint64_t lim = cap - s.l, allowed = (budget > work ? budget - work : 1) * 1024;
        const uint64_t want = lim < allowed ? lim : allowed;
        const uint64_t got = lce16_pat(pat + s.t + s.l, text + x + s.l, want, gl, work);
        s.l += got;
        matched += got;
        paused = got == want && want < lim;
      }
    }
    if (paused) break;                                  // (the extension goes on in the next launch)
    if (gl == 0) {
      len_out[s.t] = (uint32_t)s.l;
      if (!s.l) pos[s.t] = ~0ull;
    }
    s.t++;
    s.q = 0;
  }
  if (gl == 0) {
    rec[p] = s;
    if (s.t < end) atomicAdd(&ctr[0], 1ull);
    if (stats) atomicAdd(&ctr[3], (unsigned long long)matched);
  }
}

template <class I>
void ms_thr_t(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos) {
  pfp_ctx *c = f.c;
  const uint64_t budget = budget_from_env(kMsWork);
  const FmArgs<I> a = args_of<I>(f);
  DBuf<MsRec> rec(c, npat);
  DBuf<uint64_t> ctr(c, 4), own;
  if (!pos) {                                           // (pass 2 reads what pass 1 wrote)
    own.alloc(c, read_scalar(c, pat_off + npat) + 1);
    pos = own.p;
  }
  const int stats = stats_from_env();
  const auto counted = [&](const uint64_t *h) { ms_launch_counted(f, h); };
  bounded_launches(c, "fm_ms_thr1", ctr, [&](int first, unsigned long long *d_ctr) {
    fm_ms_thr1<I><<<gdim(cdiv(npat, kTB / 16)), kTB, 0, c->stream>>>(a, as<I>(f.re_sa), as<I>(f.thr), pat, pat_off, npat, rec.p, first, budget, pos,
                                                                     d_ctr, stats);
  }, counted);
  bounded_launches(c, "fm_ms_thr2", ctr, [&](int first, unsigned long long *d_ctr) {      // (a unit of its work: a step, or 1024 bytes)
    fm_ms_thr2<<<gdim(cdiv(npat, kTB / 16)), kTB, 0, c->stream>>>(f.text.p, f.n1 - 1, pat, pat_off, npat, rec.p, first, budget, len, pos, d_ctr, stats);
  }, counted);
}

}  // namespace

void fm_lcp(FmIndex &f, const LcpOut &o) {
  require_text(f, "the LCP array and thresholds");
  by_width(f, [&](auto w) { lcp_t<decltype(w)>(f, o); });
  sync(f.c);
}

void fm_load_thresholds(FmIndex &f, const uint8_t *thr5, uint64_t bytes) {
  pfp_ctx *c = f.c;
  require_text(f, "thresholds");
  const uint64_t r = f.runs;
  PFP_REQUIRE(bytes == 5 * r, PFP_EFORMAT, ".thr_pos holds " + std::to_string(bytes) + " bytes; the BWT has " + std::to_string(r) +
                                               " runs, so its .thr_pos holds " + std::to_string(5 * r));
  DBuf<uint8_t> thr(c, r * (f.wide ? 8 : 4));
  by_width(f, [&](auto w) { lcp_thr_load<decltype(w)><<<gdim(cdiv(r, kTB)), kTB, 0, c->stream>>>(thr5, r, f.n1, as<decltype(w)>(thr)); });
  PFP_HIP(hipGetLastError());
  sync(c);
  f.thr = std::move(thr);
  f.has_thr = true;
}

void fm_ms_thr(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos) {
  require_text(f, "matching statistics");
  PFP_REQUIRE(f.has_thr, PFP_EINVAL, "this index has no thresholds: add them with pfp_fm_thresholds_dev / pfp_fm_thresholds_files");
  if (!npat) return;
  by_width(f, [&](auto w) { ms_thr_t<decltype(w)>(f, pat, pat_off, npat, len, pos); });
}

}  // namespace pfp
