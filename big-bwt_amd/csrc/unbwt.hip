// unbwt.hip -- inverting a BWT and checking it (and its .sa / .ssa / .esa) against the text: the check the reference's readme
// asks users of large inputs to make "by some other means (for example inverting it)".  O(n) work and memory, no suffix sort.
//
// A .bwt of n+1 bytes with one 0 has rows j = 0..n; LF(j) = C[BWT[j]] + #{i < j : BWT[i] = BWT[j]}.  The walk r_0 = 0,
// r_{k+1} = LF(r_k) visits the row of suffix n-k at step k (SA[r_k] = n - k) and reads the text backwards:
// T[n-1-k] = BWT[r_k] = F[r_{k+1}].  The bytes are a BWT iff they hold exactly one 0 and LF is one cycle of all n+1 rows.
//
//   1. LF in one streaming build: per-wave-tile byte histograms, one scan of the [256 x tile] counts in symbol-major order,
//      then a second pass ranks equal bytes stably inside each tile (eight ballots per 64 rows, running counts in LDS).
//      LF is u32 below 2^32 rows and u64 above (or when the context is forced wide).  BWT bytes are not kept: BWT[r] =
//      F[LF(r)], a search of the 257-entry C table in LDS.
//   2. List ranking by splitters: the rows are cut into blocks of kSpl, each with one splitter at a hashed offset (row 0 is the
//      first block's), so a row's splitter test needs no memory read and a splitter's id is its block.  One lane per splitter
//      walks LF to the next splitter (next id, segment length); pointer jumping over the splitters gives each one its distance
//      to the end of the cycle through row 0.  That cycle has n+1 rows or the input is not a BWT.
//   3. One lane per splitter re-walks its segment from its now-known step k0: writes T (16-byte words buffered in registers,
//      only the segments' ends with byte stores), or compares with T, .sa (sa5[r-1] == n-k) and .ssa / .esa (the pair index of
//      a run boundary is its rank in a bitmap of run starts / ends with a popcount directory).  Mismatches meet in atomicMin,
//      so the smallest wrong index is reported whatever the schedule.
// Every walk is bounded by n+1 steps: no input makes a kernel spin.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"

namespace pfp {

namespace {

constexpr int kTB = 256;                    // threads per block of the tile kernels (four waves, one tile each)
constexpr uint64_t kTile = 16384;           // rows per wave tile of the LF build
constexpr int kSplLog = 9;                  // one splitter per 512 rows
constexpr uint64_t kSpl = 1ull << kSplLog;
constexpr uint32_t kNil = 0xFFFFFFFFu;

// offset of block s's splitter inside its block (block 0: row 0)
__device__ __forceinline__ uint64_t spl_row(uint64_t s, uint64_t n1) {
  if (s == 0) return 0;
  const uint64_t base = s << kSplLog, len = n1 - base < kSpl ? n1 - base : kSpl;
  const uint64_t h = fmix64(s * 0x9E3779B97F4A7C15ull + 0x5851F42D4C957F2Dull);
  return base + (len == kSpl ? (h & (kSpl - 1)) : h % len);
}
__device__ __forceinline__ bool is_spl(uint64_t r, uint64_t n1) { return spl_row(r >> kSplLog, n1) == r; }

// F[i] = the byte of row i of the sorted column: the largest c with C[c] <= i
__device__ __forceinline__ uint32_t f_of(const uint64_t *sC, uint64_t i) {
  uint32_t lo = 0;
#pragma unroll
  for (uint32_t step = 128; step; step >>= 1)
    if (sC[lo + step] <= i) lo += step;
  return lo;
}

__device__ __forceinline__ void atomic_min_u64(uint64_t *p, uint64_t v) { atomicMin((unsigned long long *)p, (unsigned long long)v); }

// ---------------------------------------------------------------- 1. LF
// cnt[c * nt + t] = occurrences of byte c in wave tile t
__global__ void __launch_bounds__(kTB) unbwt_hist(const uint8_t *__restrict__ bwt, uint64_t n1, uint64_t nt, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t h[kTB / 64][256];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = lane; i < 256; i += 64) h[wv][i] = 0;
  __syncthreads();
  const uint64_t t = BID * (kTB / 64) + wv;
  if (t < nt) {
    const uint64_t lo = t * kTile, hi = lo + kTile < n1 ? lo + kTile : n1;
    for (uint64_t b = lo + 16 * (uint64_t)lane; b < hi; b += 1024) {
      if (b + 16 <= hi) {
        const uint4 v = ld16u(bwt + b);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 16; q++) atomicAdd(&h[wv][(w[q >> 2] >> (8 * (q & 3))) & 255], 1u);
      } else {
        for (uint64_t x = b; x < hi; x++) atomicAdd(&h[wv][bwt[x]], 1u);
      }
    }
  }
  __syncthreads();
  if (t < nt)
    for (int i = lane; i < 256; i += 64) cnt[(uint64_t)i * nt + t] = h[wv][i];
}

// C[c] = base[c * nt] (first row of byte c in F), C[256] = n1
__global__ void unbwt_ctab(const uint64_t *__restrict__ base, uint64_t nt, uint64_t n1, uint64_t *__restrict__ C) {
  const int c = threadIdx.x;
  C[c] = base[(uint64_t)c * nt];
  if (c == 0) C[256] = n1;
}

// LF[r] = base[BWT[r] * nt + tile] + rank of row r among the rows of its tile with the same byte
template <class I>
__global__ void __launch_bounds__(kTB) unbwt_rank(const uint8_t *__restrict__ bwt, uint64_t n1, uint64_t nt, const uint64_t *__restrict__ base,
                                                  I *__restrict__ lf) {
  __shared__ uint64_t run[kTB / 64][256];
  __shared__ __attribute__((aligned(16))) uint8_t stage[kTB / 64][1024];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t t = BID * (kTB / 64) + wv;
  if (t >= nt) return;                                  // (no block-wide barrier below: every wave works alone)
  for (int i = lane; i < 256; i += 64) run[wv][i] = base[(uint64_t)i * nt + t];
  const uint64_t lo = t * kTile, hi = lo + kTile < n1 ? lo + kTile : n1;
  const uint64_t below = (1ull << lane) - 1;
  for (uint64_t b = lo; b < hi; b += 1024) {
    const uint64_t x = b + 16 * (uint64_t)lane;
    if (x + 16 <= hi) {
      *reinterpret_cast<uint4 *>(&stage[wv][16 * lane]) = ld16u(bwt + x);
    } else {
      for (int q = 0; q < 16; q++) stage[wv][16 * lane + q] = x + q < hi ? bwt[x + q] : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int k = 0; k < 16; k++) {
      const uint64_t r = b + 64 * k + lane;
      const bool ok = r < hi;
      const uint32_t c = stage[wv][64 * k + lane];
      uint64_t m = __ballot(ok);
#pragma unroll
      for (int bit = 0; bit < 8; bit++) {
        const uint64_t bal = __ballot((c >> bit) & 1);
        m &= ((c >> bit) & 1) ? bal : ~bal;
      }
      const uint64_t mine = run[wv][c];
      if (ok) lf[r] = (I)(mine + __popcll(m & below));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (ok && (m >> lane) == 1) run[wv][c] = mine + __popcll(m);      // the highest lane of the group moves the count on
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

// ---------------------------------------------------------------- 2. list ranking by splitters
// one lane per splitter: walk LF to the next splitter; seg = rows of the segment, nxt = next splitter (kNil: back at row 0)
template <class I>
__global__ void __launch_bounds__(kTB) unbwt_walk1(const I *__restrict__ lf, uint64_t n1, uint64_t m, uint32_t *__restrict__ nxt,
                                                   uint64_t *__restrict__ seg) {
  const uint64_t s = BID * kTB + threadIdx.x;
  if (s >= m) return;
  uint64_t r = lf[spl_row(s, n1)], len = 1;
  while (!is_spl(r, n1) && len <= n1) { r = lf[r]; len++; }      // (LF is a permutation: a splitter comes within n1 steps)
  const uint64_t id = r >> kSplLog;
  nxt[s] = id == 0 ? kNil : (uint32_t)id;
  seg[s] = len;
}

// Wyllie's pointer jumping: dist[s] = rows from splitter s to the end of the chain (the row before row 0)
__global__ void __launch_bounds__(kTB) unbwt_jump(uint64_t m, const uint32_t *__restrict__ nin, const uint64_t *__restrict__ din,
                                                  uint32_t *__restrict__ nout, uint64_t *__restrict__ dout) {
  const uint64_t s = BID * kTB + threadIdx.x;
  if (s >= m) return;
  const uint32_t q = nin[s];
  if (q == kNil) { nout[s] = kNil; dout[s] = din[s]; return; }
  nout[s] = nin[q];
  dout[s] = din[s] + din[q];
}

// ---------------------------------------------------------------- run-boundary bitmaps with a popcount directory
// bits[w] bit i: row 64 w + i starts (which = 0) / ends (which = 1) a run; sbc[b] = set bits of the 512-row superblock b
__global__ void __launch_bounds__(512) unbwt_runbits(const uint8_t *__restrict__ bwt, uint64_t n1, int which, uint64_t *__restrict__ bits,
                                                     uint32_t *__restrict__ sbc) {
  __shared__ uint32_t part[8];
  if (BID * 512 >= n1) return;                          // (the last row of a 2-D grid; uniform per block)
  const uint64_t r = BID * 512 + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  bool f = false;
  if (r < n1) {
    const uint8_t b = bwt[r];
    f = which == 0 ? (r == 0 || bwt[r - 1] != b) : (r + 1 == n1 || bwt[r + 1] != b);
  }
  const uint64_t word = __ballot(f);
  if (lane == 0) {
    if (r < n1) bits[r >> 6] = word;
    part[wv] = __popcll(word);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int i = 0; i < 8; i++) s += part[i];
    sbc[BID] = s;
  }
}

struct PairFile { const uint8_t *p; uint64_t bytes, pairs; const uint64_t *bits, *dir; };

__device__ __forceinline__ void check_pair(const PairFile &f, uint64_t r, uint64_t sa, uint64_t *mm) {
  if (!((f.bits[r >> 6] >> (r & 63)) & 1)) return;
  const uint64_t i = bit_rank(f.bits, f.dir, r);
  if (i >= f.pairs) return;                                       // (a short file is reported from the counts)
  const uint64_t j = ld5(f.p, 10 * i, f.bytes), v = ld5(f.p, 10 * i + 5, f.bytes);
  if (j != r || v != sa) atomic_min_u64(mm, i);
}

struct Walk2Args {
  uint64_t n1, m;
  const uint64_t *C;
  const uint64_t *seg, *dist;
  uint8_t *out;                      // decode: T (n bytes)
  const uint8_t *text; uint64_t text_len;   // check: the text
  const uint8_t *sa5; uint64_t sa_bytes, sa_q;
  PairFile ssa, esa;
  uint64_t *mm;                      // {text, sa, ssa, esa} smallest mismatch
};

__device__ __forceinline__ uint32_t byte_of(uint64_t lo, uint64_t hi, int i) { return (uint32_t)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 255); }

// the cnt bytes at text positions [p, p + cnt) held in (lo, hi), lowest position in the lowest byte
__device__ __forceinline__ void flush(const Walk2Args &a, uint64_t p, int cnt, uint64_t lo, uint64_t hi) {
  if (a.out) {
    if (cnt == 16) {
      *reinterpret_cast<uint4 *>(a.out + p) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    } else {
      for (int i = 0; i < cnt; i++) a.out[p + i] = (uint8_t)byte_of(lo, hi, i);
    }
  } else if (a.text) {
    if (cnt == 16 && p + 16 <= a.text_len) {
      const uint4 v = *reinterpret_cast<const uint4 *>(a.text + p);
      const uint64_t x0 = lo ^ ((uint64_t)v.y << 32 | v.x), x1 = hi ^ ((uint64_t)v.w << 32 | v.z);
      if (x0 | x1) atomic_min_u64(&a.mm[0], p + (x0 ? __builtin_ctzll(x0) >> 3 : 8 + (__builtin_ctzll(x1) >> 3)));
    } else {
      for (int i = 0; i < cnt; i++)
        if (p + i < a.text_len && a.text[p + i] != byte_of(lo, hi, i)) { atomic_min_u64(&a.mm[0], p + i); break; }
    }
  }
}

// one lane per splitter: re-walk the segment from step k0 = n1 - dist
template <class I>
__global__ void __launch_bounds__(kTB) unbwt_walk2(const I *__restrict__ lf, Walk2Args a) {
  __shared__ uint64_t sC[257];
  for (int i = threadIdx.x; i < 257; i += kTB) sC[i] = a.C[i];
  __syncthreads();
  const uint64_t s = BID * kTB + threadIdx.x;
  if (s >= a.m) return;
  const uint64_t n = a.n1 - 1, len = a.seg[s];
  uint64_t k = a.n1 - a.dist[s];
  uint64_t r = spl_row(s, a.n1), rn = lf[r];
  const bool bytes = a.out || a.text;
  const uintptr_t abase = (uintptr_t)(a.out ? a.out : a.text);
  uint64_t blo = 0, bhi = 0;
  int cnt = 0;
  for (uint64_t st = 0; st < len; st++, k++) {
    const uint64_t rnn = st + 1 < len ? (uint64_t)lf[rn] : 0;       // the next load is in flight during this row's work
    if (bytes && k < n) {
      const uint64_t p = n - 1 - k;
      bhi = (bhi << 8) | (blo >> 56);
      blo = (blo << 8) | f_of(sC, rn);
      cnt++;
      if (((abase + p) & 15) == 0 || st + 1 == len || k + 1 == n) { flush(a, p, cnt, blo, bhi); cnt = 0; }
    }
    if (a.sa5 && r >= 1 && r - 1 < a.sa_q && ld5(a.sa5, 5 * (r - 1), a.sa_bytes) != n - k) atomic_min_u64(&a.mm[1], r);
    if (a.ssa.p) check_pair(a.ssa, r, n - k, &a.mm[2]);
    if (a.esa.p) check_pair(a.esa, r, n - k, &a.mm[3]);
    r = rn; rn = rnn;
  }
}

// one lane per splitter, the same walk with SA[r] = n - k in hand: lcp[r] = plcp[SA[r]] (plcp in text order, n1 entries)
template <class I>
__global__ void __launch_bounds__(kTB) unbwt_walk_lcp(const I *__restrict__ lf, uint64_t n1, uint64_t m, const uint64_t *__restrict__ seg,
                                                      const uint64_t *__restrict__ dist, const I *__restrict__ plcp, I *__restrict__ lcp) {
  const uint64_t s = BID * kTB + threadIdx.x;
  if (s >= m) return;
  const uint64_t n = n1 - 1, len = seg[s];
  uint64_t k = n1 - dist[s];
  uint64_t r = spl_row(s, n1), rn = lf[r];
  for (uint64_t st = 0; st < len; st++, k++) {
    const uint64_t rnn = st + 1 < len ? (uint64_t)lf[rn] : 0;       // the next load is in flight during this row's work
    if (k <= n && r < n1) lcp[r] = plcp[n - k];
    r = rn; rn = rnn;
  }
}

}  // namespace

// .ssa / .esa bitmap, directory and run count (kernels.hpp)
void RunIndex::build(pfp_ctx *c, const uint8_t *bwt, uint64_t n1, int which) {
    const uint64_t nsb = cdiv(n1, 512);
    bits.alloc(c, nsb * 8);
    DBuf<uint32_t> sbc(c, nsb + 1);
    dir.alloc(c, nsb + 1);
    PFP_HIP(hipMemsetAsync(sbc.p + nsb, 0, sizeof(uint32_t), c->stream));
    {
      KScope ks(c, which ? "unbwt_runbits [esa]" : "unbwt_runbits [ssa]", n1 + n1 / 8);
      unbwt_runbits<<<gdim(nsb), 512, 0, c->stream>>>(bwt, n1, which, bits.p, sbc.p);
      PFP_HIP(hipGetLastError());
    }
    exclusive_sum_u32_u64(c, sbc.p, dir.p, nsb + 1);
    runs = read_scalar(c, dir.p + nsb);
}

namespace {

// LF and, by list ranking, every splitter's segment length and distance to the end of the cycle: what the second walk starts
// from (invert_t: decode / check; lcp_by_rows: the gather through SA)
template <class I>
struct LfRanks {
  DBuf<I> lf;
  DBuf<uint64_t> C, seg, dist;
  uint64_t m = 0;
};

template <class I>
void lf_ranks(pfp_ctx *c, const uint8_t *bwt, uint64_t n1, LfRanks<I> &w) {
  const uint64_t nt = cdiv(n1, kTile), m = w.m = cdiv(n1, kSpl);
  w.lf.alloc(c, n1);
  DBuf<uint32_t> cnt(c, 256 * nt);
  DBuf<uint64_t> base(c, 256 * nt);
  w.C.alloc(c, 257);
  {
    KScope ks(c, "unbwt_hist", n1 + 256 * nt * 4);
    unbwt_hist<<<gdim(cdiv(nt, kTB / 64)), kTB, 0, c->stream>>>(bwt, n1, nt, cnt.p);
    PFP_HIP(hipGetLastError());
  }
  exclusive_sum_u32_u64(c, cnt.p, base.p, 256 * nt);
  unbwt_ctab<<<1, 256, 0, c->stream>>>(base.p, nt, n1, w.C.p);
  PFP_HIP(hipGetLastError());
  uint64_t hC[257];
  d2h(c, hC, w.C.p, 257);
  sync(c);
  const uint64_t zeros = hC[1] - hC[0];
  PFP_REQUIRE(zeros == 1, PFP_EFORMAT, "not a BWT: " + std::to_string(zeros) + " bytes 0 among " + std::to_string(n1) + " (a BWT holds exactly one)");
  {
    KScope ks(c, "unbwt_rank", n1 + n1 * sizeof(I) + 256 * nt * 8);
    unbwt_rank<I><<<gdim(cdiv(nt, kTB / 64)), kTB, 0, c->stream>>>(bwt, n1, nt, base.p, w.lf.p);
    PFP_HIP(hipGetLastError());
  }
  cnt.release(); base.release();

  DBuf<uint32_t> nxt(c, m), nxt2(c, m);
  DBuf<uint64_t> dist2(c, m);
  w.seg.alloc(c, m); w.dist.alloc(c, m);
  {
    KScope ks(c, "unbwt_walk1", n1 * sizeof(I) + m * 12);
    unbwt_walk1<I><<<gdim(cdiv(m, kTB)), kTB, 0, c->stream>>>(w.lf.p, n1, m, nxt.p, w.seg.p);
    PFP_HIP(hipGetLastError());
  }
  PFP_HIP(hipMemcpyAsync(w.dist.p, w.seg.p, m * 8, hipMemcpyDeviceToDevice, c->stream));
  {
    const int rounds = m > 1 ? bits_for(m - 1) : 0;      // ceil(log2 m) launches, each reads 2 x 12 and writes 12 bytes per splitter
    KScope ks(c, "unbwt_jump", (uint64_t)rounds * m * 36);
    for (int round = 0; round < rounds; round++) {
      unbwt_jump<<<gdim(cdiv(m, kTB)), kTB, 0, c->stream>>>(m, nxt.p, w.dist.p, nxt2.p, dist2.p);
      PFP_HIP(hipGetLastError());
      std::swap(nxt, nxt2); std::swap(w.dist, dist2);
    }
  }
  nxt2.release(); dist2.release();
  const uint64_t cyc = read_scalar(c, w.dist.p);
  PFP_REQUIRE(cyc == n1, PFP_EFORMAT, "not a BWT: the LF mapping has more than one cycle (the cycle through row 0 has " + std::to_string(cyc) +
                                          " of " + std::to_string(n1) + " rows)");
}

template <class I>
void invert_t(pfp_ctx *c, const BwtCheckArgs &in, pfp_check_result *res) {
  const uint64_t n1 = in.n1, n = n1 - 1;
  LfRanks<I> w;
  lf_ranks<I>(c, in.bwt, n1, w);
  const uint64_t m = w.m;
  DBuf<I> &lf = w.lf;
  {
    RunIndex rs, re;
    Walk2Args a{};
    a.n1 = n1; a.m = m; a.C = w.C.p; a.seg = w.seg.p; a.dist = w.dist.p;
    a.out = in.out;
    a.text = in.text; a.text_len = in.text_len;
    DBuf<uint64_t> mm(c, 4);
    PFP_HIP(hipMemsetAsync(mm.p, 0xFF, 32, c->stream));
    a.mm = mm.p;
    if (in.sa5) { a.sa5 = in.sa5; a.sa_bytes = in.sa_bytes; a.sa_q = std::min<uint64_t>(in.sa_bytes / 5, n); }
    if (in.ssa10) {
      rs.build(c, in.bwt, n1, 0);
      a.ssa = PairFile{in.ssa10, in.ssa_bytes, in.ssa_bytes / 10, rs.bits.p, rs.dir.p};
      res->ssa_runs = rs.runs;
    }
    if (in.esa10) {
      re.build(c, in.bwt, n1, 1);
      a.esa = PairFile{in.esa10, in.esa_bytes, in.esa_bytes / 10, re.bits.p, re.dir.p};
      res->esa_runs = re.runs;
    }
    {
      const uint64_t per_row = sizeof(I) + (a.out || a.text ? 1 : 0) + (a.sa5 ? 5 : 0);
      KScope ks(c, in.out ? "unbwt_walk2 [decode]" : "unbwt_walk2 [check]", n1 * per_row + m * 16);
      unbwt_walk2<I><<<gdim(cdiv(m, kTB)), kTB, 0, c->stream>>>(lf.p, a);
      PFP_HIP(hipGetLastError());
    }
    uint64_t h[4];
    d2h(c, h, mm.p, 4);
    sync(c);
    // lengths: a text of another length differs where the shorter one ends, a short / long .sa at the first entry it lacks or
    // has too many, a short / long .ssa / .esa at the first pair it lacks or has too many
    if (in.text && in.text_len != n) h[0] = std::min(h[0], std::min(in.text_len, n));
    if (in.sa5 && (in.sa_bytes % 5 || in.sa_bytes / 5 != n)) h[1] = std::min(h[1], std::min(in.sa_bytes / 5, n) + 1);
    if (in.ssa10 && (in.ssa_bytes % 10 || in.ssa_bytes / 10 != rs.runs)) h[2] = std::min(h[2], std::min(in.ssa_bytes / 10, rs.runs));
    if (in.esa10 && (in.esa_bytes % 10 || in.esa_bytes / 10 != re.runs)) h[3] = std::min(h[3], std::min(in.esa_bytes / 10, re.runs));
    res->text_mismatch = in.text ? h[0] : UINT64_MAX;
    res->sa_mismatch = in.sa5 ? h[1] : UINT64_MAX;
    res->ssa_mismatch = in.ssa10 ? h[2] : UINT64_MAX;
    res->esa_mismatch = in.esa10 ? h[3] : UINT64_MAX;
  }
}

}  // namespace

template <class I>
void lcp_by_rows(pfp_ctx *c, const uint8_t *bwt, uint64_t n1, const I *plcp, I *lcp) {
  LfRanks<I> w;
  lf_ranks<I>(c, bwt, n1, w);
  KScope ks(c, "unbwt_walk_lcp", n1 * 3 * sizeof(I) + w.m * 16);
  unbwt_walk_lcp<I><<<gdim(cdiv(w.m, kTB)), kTB, 0, c->stream>>>(w.lf.p, n1, w.m, w.seg.p, w.dist.p, plcp, lcp);
  PFP_HIP(hipGetLastError());
}
template void lcp_by_rows<uint32_t>(pfp_ctx *, const uint8_t *, uint64_t, const uint32_t *, uint32_t *);
template void lcp_by_rows<uint64_t>(pfp_ctx *, const uint8_t *, uint64_t, const uint64_t *, uint64_t *);

void invert_bwt(pfp_ctx *c, const BwtCheckArgs &in, pfp_check_result *res) {
  const auto t0 = std::chrono::steady_clock::now();
  memset(res, 0, sizeof *res);
  res->text_mismatch = res->sa_mismatch = res->ssa_mismatch = res->esa_mismatch = UINT64_MAX;
  PFP_REQUIRE(in.n1 >= 1, PFP_EFORMAT, "not a BWT: no byte 0 (an empty input)");
  PFP_REQUIRE(in.n1 <= (1ull << 40), PFP_ELIMIT, "a BWT of more than 2^40 bytes (the limit of the 5-byte .sa format)");
  PFP_REQUIRE(in.bwt, PFP_EINVAL, "no BWT");
  if (c->force_wide || in.n1 >= (1ull << 32)) invert_t<uint64_t>(c, in, res);
  else invert_t<uint32_t>(c, in, res);
  res->n = in.n1 - 1;
  res->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace pfp
