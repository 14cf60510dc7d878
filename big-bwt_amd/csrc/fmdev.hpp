// fmdev.hpp -- what the kernels over an FmIndex share (fmsearch.hip, fmapprox.hip, fmextend.hip, lcp.hip, seqmap.hip): the index as kernel arguments, rank and select
// by groups of 16 lanes, the longest common extension on the text, and the record a bounded launch leaves behind.
#pragma once
#include "kernels.hpp"
#include "devutil.hpp"

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
// bit 7 of each byte of w set where that byte equals the byte replicated in c4
__device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t c4) {
  const uint32_t x = w ^ c4;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

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
  uint32_t incl = mine;                                            // inclusive sum over the group's lanes
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 16);
    if (gl >= d) incl += o;
  }
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

// the common prefix of T[x ..) and T[y ..), at most cap bytes and never past the end of the text (x, y are clamped to n); the
// group compares 1024 bytes per iteration: four rows of 256, 16 bytes per lane, all eight loads in flight together (a short
// cap leaves the later rows out).  Reads stay below text + n + 16: the padding of the index's copy.
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
    uint64_t mine = cap;                                // no difference below cap among this lane's bytes
#pragma unroll
    for (int j = 3; j >= 0; j--) {
      const uint64_t o = done + 256 * j + 16 * (uint64_t)gl;
      const uint32_t w[4] = {u[j].x ^ v[j].x, u[j].y ^ v[j].y, u[j].z ^ v[j].z, u[j].w ^ v[j].w};
#pragma unroll
      for (int q = 3; q >= 0; q--)
        if (w[q]) mine = o + 4 * q + (__ffs(w[q]) - 1) / 8;
    }
    if (mine > cap) mine = cap;
    work++;
    const uint64_t m = gmin16(mine);
    if (m < cap) return m;
  }
  return cap;
}

template <class I>
FmArgs<I> args_of(const FmIndex &f) {
  FmArgs<I> a{};
  a.bwt = f.bwt.p; a.n1 = f.n1; a.codes = f.codes.p;
  a.blk = f.blk.p; a.sbc = f.sbc.p; a.sigma = f.sigma;
  if (f.samples) {
    a.rbits = f.rs.bits.p; a.rdir = f.rs.dir.p; a.runs = f.runs;
    a.rs_row = (const I *)f.rs_row.p; a.rs_sa = (const I *)f.rs_sa.p;
    a.key = (const I *)f.phi_key.p; a.val = (const I *)f.phi_val.p; a.dir = (const I *)f.phi_dir.p;
    a.nphi = f.nphi; a.nbk = f.nbk; a.shift = f.shift;
  }
  return a;
}

}  // namespace

}  // namespace pfp
