// fmdev.hpp -- the toolkit of the files over an FmIndex (fmsearch.hip, fmapprox.hip, fmextend.hip, fmcigar.hip, fmfill.hip, fmmap.hip, lcp.hip, seqmap.hip).  Device side:
// the index as kernel arguments, rank and select by groups of 16 lanes, the start of a group-per-pattern kernel, the steps the walks
// share (toehold, matching-statistics start and neighbours), the 1024-byte compare, and the tiny kernels every segmented sort needs.
// Host side: the environment's budget and stats switch, the index width as a type, the requirement checks, and the one loop that
// repeats a bounded launch until nothing is left unfinished.
#pragma once
#include "kernels.hpp"
#include "devutil.hpp"
#include <cstdlib>
#include <string>

namespace pfp {

namespace {

constexpr int kTB = 256;
constexpr int kBlkLog = 8;                  // 256 rows per rank block
constexpr int kSbLog = 16;                  // 65536 rows per superblock: in-superblock counts fit u16
constexpr int kBlkPerSb = 1 << (kSbLog - kBlkLog);
constexpr uint8_t kAbsent = 0xFF;

template <class I>
struct FmArgs {
  const uint8_t *bwt; uint64_t n1;
  const uint8_t *codes;
  const uint16_t *blk; const uint64_t *sbc; int sigma;
  const uint64_t *rbits, *rdir; uint64_t runs;
  const I *rs_row, *rs_sa;
  const I *key, *val, *dir; uint64_t nphi, nbk; int shift;
};

__device__ __forceinline__ uint64_t gsum16(uint64_t v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
  return v;
}
__device__ __forceinline__ uint64_t gmin16(uint64_t v) {
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) { const uint64_t o = __shfl_xor(v, d, 64); v = o < v ? o : v; }
  return v;
}
// inclusive scan over the group's 16 lanes (gl = this lane's place in it), by any associative op; gscan16_incl: the sum
template <class T, class Op>
__device__ __forceinline__ T gscan16(T v, int gl, Op op) {
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) {
    const T o = __shfl_up(v, d, 16);
    if (gl >= d) v = op(v, o);
  }
  return v;
}
__device__ __forceinline__ uint32_t gscan16_incl(uint32_t v, int gl) {
  return gscan16(v, gl, [](uint32_t x, uint32_t y) { return x + y; });
}
// bit 7 of each byte of w set where that byte equals the byte replicated in c4
__device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t c4) {
  const uint32_t x = w ^ c4;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// bit 7 of a byte of w set where that byte is 0
__device__ __forceinline__ uint32_t zero_bytes(uint32_t w) { return (w - 0x01010101u) & ~w & 0x80808080u; }

// C[c] + rank_c(i) for 0 <= i <= n1; gl = this lane's place in its group of 16 (all 16 call it with the same arguments)
template <class I>
__device__ __forceinline__ uint64_t lf_at(const FmArgs<I> &a, uint64_t i, uint32_t c4, uint32_t k, int gl) {
  const uint64_t blk = i >> kBlkLog;
  const uint64_t base = a.sbc[(i >> kSbLog) * a.sigma + k] + a.blk[blk * a.sigma + k];
  const uint4 v = ld16u(a.bwt + (blk << kBlkLog) + 16 * gl);
  const int keep = (int)(i & 255) - 16 * gl;           // bytes of this lane's 16 that lie before row i
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t cnt = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int kq = keep - 4 * q;
    const uint32_t m = kq >= 4 ? 0x80808080u : kq <= 0 ? 0u : (0x80808080u & ((1u << (8 * kq)) - 1u));
    cnt += __popc(eq_bytes(w[q], c4) & m);
  }
  return base + gsum16(cnt);
}

// the row j in [sp, ep) of the c with C[c] + rank_c(j) = target (the first c there); ~0 if there is none
template <class I>
__device__ __forceinline__ uint64_t select_first(const FmArgs<I> &a, uint64_t sp, uint64_t ep, uint64_t target, uint32_t c4, uint32_t k, int gl) {
  uint64_t lo = sp >> kBlkLog, hi = (ep - 1) >> kBlkLog;        // the last block whose start has lf <= target
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    const uint64_t r = a.sbc[(mid >> (kSbLog - kBlkLog)) * a.sigma + k] + a.blk[mid * a.sigma + k];
    if (r <= target) lo = mid;
    else hi = mid - 1;
  }
  const uint64_t want = target - (a.sbc[(lo >> (kSbLog - kBlkLog)) * a.sigma + k] + a.blk[lo * a.sigma + k]);
  const uint4 v = ld16u(a.bwt + (lo << kBlkLog) + 16 * gl);
  const uint32_t e[4] = {eq_bytes(v.x, c4), eq_bytes(v.y, c4), eq_bytes(v.z, c4), eq_bytes(v.w, c4)};
  const uint32_t mine = __popc(e[0]) + __popc(e[1]) + __popc(e[2]) + __popc(e[3]);
  const uint32_t incl = gscan16_incl(mine, gl);
  uint64_t j = ~0ull;
  const uint64_t excl = incl - mine;
  if (want >= excl && want < incl) {
    uint32_t left = (uint32_t)(want - excl);
    for (int q = 0; q < 4; q++) {
      uint32_t m = e[q];
      const uint32_t pc = __popc(m);
      if (left < pc) {
        for (uint32_t t = 0; t < left; t++) m &= m - 1;
        j = (lo << kBlkLog) + 16 * gl + 4 * q + (__ffs(m) - 1) / 8;
        break;
      }
      left -= pc;
    }
  }
  j = gmin16(j);
  return j >= sp && j < ep ? j : ~0ull;
}

// the bucket directory of a predecessor search over sorted keys: dir[b] = first index of a key >= b << shift (b = 0..nbk).  A
// search for x then starts in [dir[x >> shift], dir[(x >> shift) + 1]): about one key with the shift its callers choose
template <class K, class D>
__global__ void __launch_bounds__(kTB) bucket_dir_k(const K *__restrict__ key, uint64_t nkeys, uint64_t nbk, int shift, D *__restrict__ dir) {
  const uint64_t b = BID * kTB + threadIdx.x;
  if (b > nbk) return;
  const uint64_t x = b << shift;
  uint64_t lo = 0, hi = nkeys;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)key[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  dir[b] = (D)lo;
}

// the last index i in [0, count) with off[i] <= x (off[0] <= x; count >= 1)
__device__ __forceinline__ uint64_t last_le(const uint64_t *__restrict__ off, uint64_t count, uint64_t x) {
  uint64_t lo = 0, hi = count - 1;
  while (lo < hi) {
    const uint64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

constexpr uint64_t kMsWork = 16384;         // units of work per pattern and launch: one per step, one per 1024 bytes compared
                                            // (matching statistics), one per iteration of the approximate walk (fmapprox.hip)
struct MsRec { uint64_t t, q, pos, l; };    // the next byte to read is pat[t - 1]; SA[q] = pos; l bytes matched to the right of it

// one step of a compare: u[j], v[j] = this lane's 16 bytes of either side at byte `at` + ROW j, j = 0..3 (equal words where a side
// was not read).  The first byte at which the sides differ among this lane's, capped at cap
template <int ROW>
__device__ __forceinline__ uint64_t first_diff_rows(const uint4 (&u)[4], const uint4 (&v)[4], uint64_t at, uint64_t cap) {
  uint64_t mine = cap;                                  // no difference below cap among this lane's bytes
#pragma unroll
  for (int j = 3; j >= 0; j--) {
    const uint32_t w[4] = {u[j].x ^ v[j].x, u[j].y ^ v[j].y, u[j].z ^ v[j].z, u[j].w ^ v[j].w};
#pragma unroll
    for (int q = 3; q >= 0; q--)
      if (w[q]) mine = at + ROW * j + 4 * q + (__ffs(w[q]) - 1) / 8;
  }
  return mine > cap ? cap : mine;
}
// the same for a group of 16 lanes that compares 1024 bytes from `done` on, four rows of 256: the group's first difference, or cap
__device__ __forceinline__ uint64_t first_diff_1024(const uint4 (&u)[4], const uint4 (&v)[4], uint64_t done, uint64_t cap, int gl) {
  return gmin16(first_diff_rows<256>(u, v, done + 16 * (uint64_t)gl, cap));
}

// the common prefix of T[x ..) and T[y ..), at most cap bytes and never past the end of the text (x, y are clamped to n); the
// group compares 1024 bytes per iteration, 16 bytes per lane and row, all eight loads in flight together (a short cap leaves the
// later rows out).  Reads stay below text + n + 16: the padding of the index's copy.
__device__ __forceinline__ uint64_t lce16(const uint8_t *__restrict__ text, uint64_t n, uint64_t x, uint64_t y, uint64_t cap, int gl, uint64_t &work) {
  if (x > n) x = n;
  if (y > n) y = n;
  const uint64_t room = n - (x > y ? x : y);
  if (cap > room) cap = room;
  for (uint64_t done = 0; done < cap; done += 1024) {   // (done and cap are the same in all 16 lanes)
    uint4 u[4], v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint64_t o = done + 256 * j + 16 * (uint64_t)gl;
      u[j] = v[j] = make_uint4(0, 0, 0, 0);
      if (o < cap) { u[j] = ld16u(text + x + o); v[j] = ld16u(text + y + o); }
    }
    work++;
    const uint64_t m = first_diff_1024(u, v, done, cap, gl);
    if (m < cap) return m;
  }
  return cap;
}

// ---------------------------------------------------------------- kernels with one group of 16 lanes per pattern
// their start: the code table into LDS (code[256], every thread of the block), this lane's place in its group, the group's pattern
// and its offsets: off[p] .. off[p + 1], or off[p] .. end[p] where the ends are given apart (strings that lie anywhere in the
// buffer: fm_count_spans).  false: no such pattern (whole groups leave together: the shuffles stay inside groups)
struct PatGroup { int gl; uint64_t p, o0, o1; };
__device__ __forceinline__ bool pat_group(uint8_t *code, const uint8_t *__restrict__ codes, const uint64_t *__restrict__ off, uint64_t npat,
                                          PatGroup &g, const uint64_t *__restrict__ end = nullptr) {
  code[threadIdx.x] = codes[threadIdx.x];
  __syncthreads();
  g.gl = threadIdx.x & 15;
  g.p = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (g.p >= npat) return false;
  g.o0 = off[g.p]; g.o1 = end ? end[g.p] : off[g.p + 1];
  return true;
}

// where a right-to-left walk of matching statistics stands: at (m, 0, n, 0) in a first launch, else at its record.  A pattern of
// 2^32 - 1 bytes or more is refused (its lengths would not fit 32 bits): it starts finished, and ctr[1] counts it
__device__ __forceinline__ MsRec ms_start(int first, const MsRec *__restrict__ rec, uint64_t o0, uint64_t o1, uint64_t n,
                                          unsigned long long *__restrict__ ctr, int gl) {
  if (!first) return *rec;
  MsRec s{o1 > o0 ? o1 : o0, 0, n, 0};                  // (decreasing offsets: no pattern)
  if (o1 > o0 && o1 - o0 >= 0xFFFFFFFFull) {
    s.t = o0;
    if (gl == 0) atomicAdd(&ctr[1], 1ull);
  }
  return s;
}

// the toehold SA[sp'] after a backward step by byte c (code k) from [sp, ep) with toehold `first`, nsp = LF(sp, c) and a range that
// stays non-empty: first - 1 if BWT[sp] = c, else SA[j] - 1 for the first c in the range, a run start (2^64 - 1: wrong samples only)
template <class I>
__device__ __forceinline__ uint64_t toehold_step(const FmArgs<I> &a, uint64_t sp, uint64_t ep, uint64_t nsp, uint64_t first, uint32_t c,
                                                 uint32_t c4, uint32_t k, int gl) {
  if (a.bwt[sp] == c) return first - 1;
  const uint64_t j = select_first(a, sp, ep, nsp, c4, k, gl);
  const uint64_t q = j < a.n1 ? bit_rank(a.rbits, a.rdir, j) : a.runs;
  return q < a.runs ? (uint64_t)a.rs_sa[q] - 1 : ~0ull;
}

// BWT[q] != c, target = LF(q, c): the last c before row q (it ends a run) and the first after it (it starts one), 2^64 - 1 for a
// side that does not exist; and, for the side a caller goes to, its run number clamped below runs: both SA values are samples
struct MsNeighbours { uint64_t qp, qs; };
template <class I>
__device__ __forceinline__ MsNeighbours ms_neighbours(const FmArgs<I> &a, uint64_t q, uint64_t target, uint32_t c4, uint32_t k, int gl) {
  return MsNeighbours{q ? select_first(a, 0, q, target - 1, c4, k, gl) : ~0ull,
                      q + 1 < a.n1 ? select_first(a, q + 1, a.n1, target, c4, k, gl) : ~0ull};
}
template <class I>
__device__ __forceinline__ uint64_t run_ending_at(const FmArgs<I> &a, uint64_t qp) {
  uint64_t r = bit_rank(a.rbits, a.rdir, qp + 1);       // run starts in [0, qp]: qp lies in run r - 1
  r = r ? r - 1 : 0;
  return r >= a.runs ? a.runs - 1 : r;
}
template <class I>
__device__ __forceinline__ uint64_t run_starting_at(const FmArgs<I> &a, uint64_t qs) {
  const uint64_t r = bit_rank(a.rbits, a.rdir, qs);
  return r >= a.runs ? a.runs - 1 : r;
}

// ---------------------------------------------------------------- the tiny kernels around a segmented sort
// (templates over the element, as bucket_dir_k: only a file that launches one holds a copy of it)
// segment p of a sort = the entries of pattern p: sb[p], se[p] = off[p], off[p + 1], or at[off[..]] (at NULL: the offsets
// themselves).  head (may be NULL): head[sb[p]] = 1 for a segment that is not empty; val[i] = i for i < nval (the sort's values)
template <class B>
__global__ void __launch_bounds__(kTB) seg_bounds_k(const uint64_t *__restrict__ off, uint64_t npat, const uint64_t *__restrict__ at,
                                                    B *__restrict__ sb, B *__restrict__ se, B *__restrict__ head, B *__restrict__ val, uint64_t nval) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i < npat) {
    const uint64_t b = at ? at[off[i]] : off[i], e = at ? at[off[i + 1]] : off[i + 1];
    sb[i] = (B)b; se[i] = (B)e;
    if (head && e > b) head[b] = 1;
  }
  if (i < nval) val[i] = (B)i;
}
// out[p] = sums[at[p]], p = 0..npat: what was counted before pattern p's first entry (sums has last + 1 entries; at is clamped)
template <class T>
__global__ void __launch_bounds__(kTB) gather_off_k(const uint64_t *__restrict__ at, uint64_t npat, const T *__restrict__ sums, uint64_t last,
                                                    T *__restrict__ out) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p > npat) return;
  const uint64_t h = at[p];
  out[p] = sums[h < last ? h : last];
}

// ---------------------------------------------------------------- the sequences of a collection (seqmap.hip, fmmap.hip)
// the table as kernel arguments: start[0 .. nseq] and its bucket directory over text positions
constexpr uint32_t kNoSeq = 0xFFFFFFFFu;
template <class I>
struct SeqArgs {
  const I *start; const uint32_t *dir; uint64_t nseq, n; int shift;
};
// the sequence that holds text position x < n: the first start above x, searched in x's bucket, is the next sequence's
template <class I>
__device__ __forceinline__ uint32_t seq_of(const SeqArgs<I> &s, uint64_t x) {
  const uint64_t b = x >> s.shift;
  uint64_t lo = s.dir[b], hi = s.dir[b + 1];            // starts [lo, hi) lie in the bucket; those before lo are <= x
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)s.start[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  if (lo < 1) lo = 1;                                   // (starts[0] = 0 <= x < n = starts[nseq]: checked when the table was set)
  if (lo > s.nseq) lo = s.nseq;
  return (uint32_t)(lo - 1);
}

// ---------------------------------------------------------------- host side
// the index's arrays "of I" (DBuf<uint8_t>: their element is u32 or u64 by f.wide) as I
template <class I>
I *as(const DBuf<uint8_t> &b) { return (I *)b.p; }
// fn(uint32_t{}) or fn(uint64_t{}): the index's width as the type of fn's argument
template <class F>
void by_width(const FmIndex &f, F &&fn) {
  if (f.wide) fn(uint64_t{});
  else fn(uint32_t{});
}

template <class I>
FmArgs<I> args_of(const FmIndex &f) {
  FmArgs<I> a{};
  a.bwt = f.bwt.p; a.n1 = f.n1; a.codes = f.codes.p;
  a.blk = f.blk.p; a.sbc = f.sbc.p; a.sigma = f.sigma;
  if (f.samples) {
    a.rbits = f.rs.bits.p; a.rdir = f.rs.dir.p; a.runs = f.runs;
    a.rs_row = as<I>(f.rs_row); a.rs_sa = as<I>(f.rs_sa);
    a.key = as<I>(f.phi_key); a.val = as<I>(f.phi_val); a.dir = as<I>(f.phi_dir);
    a.nphi = f.nphi; a.nbk = f.nbk; a.shift = f.shift;
  }
  return a;
}

template <class I>
SeqArgs<I> seq_args(const FmIndex &f) {
  return SeqArgs<I>{as<I>(f.seq_start), f.seq_dir.p, f.nseq, f.n1 - 1, f.seq_shift};
}

// PFP_FM_MS_STEPS: a bound below the default (tests: a small one reaches the resume paths with small inputs)
inline uint64_t budget_from_env(uint64_t budget) {
  if (const char *e = getenv("PFP_FM_MS_STEPS")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < budget) budget = v;
  }
  return budget;
}
// PFP_FM_MS_STATS (measurement: tools/ms_time.py and approx_time.py read the sums through pfp_fm_ms_stats / pfp_fm_approx_stats)
inline int stats_from_env() {
  const char *se = getenv("PFP_FM_MS_STATS");
  return se && *se && *se != '0';
}

inline void require_text(const FmIndex &f, const char *what) {
  PFP_REQUIRE(f.has_text, PFP_EINVAL, std::string(what) + " need the text and the run-end values: build the index with pfp_fm_build_ms_dev / "
                                      "pfp_fm_build_ms_files");
}
inline void require_samples(const FmIndex &f) {
  PFP_REQUIRE(f.samples, PFP_EINVAL, "locate needs the run samples: this index was built without .ssa / .esa (bigbwt -s -e writes them)");
}
inline void require_toehold(const FmIndex &f, bool toehold) {
  PFP_REQUIRE(!toehold || f.samples, PFP_EINVAL, "the toehold SA[sp] needs the run samples: this index was built without .ssa / .esa");
}
// `count` entries (noun: "hits", "seeds") go through the segmented sort in one call
inline void require_sortable(uint64_t count, const char *noun) {
  PFP_REQUIRE(count < 0xFFFFFFFFull, PFP_ELIMIT, std::to_string(count) + " " + noun + " in one call: the limit is 2^32 - 2 (the segmented sort's "
                                                 "bounds are 32 bits; fewer patterns per call)");
}

// A bounded launch gives every pattern a budget of work and leaves the unfinished ones in records; this repeats it until none is
// left.  Per launch: zero the counters, launch(first, ctr) under a scope `name`, read the counters back, hand them to each(h) -
// which adds them to its stats and raises its errors - and stop when h[0], the patterns left unfinished, is 0.  At most 4 counters
template <class Launch, class Each>
void bounded_launches(pfp_ctx *c, const char *name, DBuf<uint64_t> &ctr, Launch &&launch, Each &&each) {
  uint64_t h[4];
  for (int first = 1;; first = 0) {                     // every launch finishes at least one unit of work of every unfinished pattern
    ctr.zero();
    {
      KScope ks(c, name, 0);
      launch(first, (unsigned long long *)ctr.p);
      PFP_HIP(hipGetLastError());
    }
    d2h(c, h, ctr.p, ctr.n);
    sync(c);
    each(h);
    if (!h[0]) break;
  }
}
// what a launch of matching statistics counted (fm_ms, fm_ms_thr): h[1] patterns refused, h[2] jumps, h[3] bytes matched
inline void ms_launch_counted(FmIndex &f, const uint64_t *h) {
  f.ms_stats[0] += 1; f.ms_stats[1] += h[2]; f.ms_stats[2] += h[3];
  PFP_REQUIRE(!h[1], PFP_ELIMIT, std::to_string(h[1]) + " patterns of 2^32 - 1 bytes or more: the lengths of matching statistics are 32 bits");
}

}  // namespace

}  // namespace pfp
