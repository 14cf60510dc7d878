// runsample.hip -- finished device outputs on their way to the files: 5-byte packing (.sa, and the pairs of .ssa / .esa)
// and the sampling of the suffix array at the run boundaries of the BWT.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"

namespace pfp {

static constexpr int TB = 256;

// utils.c:112-129: low 5 bytes, little endian.  One thread per 16 OUTPUT bytes (3.2 values): it reads the
// (up to) four values its chunk overlaps - neighbouring lanes read overlapping, consecutive values - lays
// their 5-byte fields end to end and cuts its 16 bytes out; every store is one aligned-size 16-byte store.
__global__ __launch_bounds__(256) void pack5_kernel(const uint64_t *__restrict__ v, uint64_t cnt, uint8_t *__restrict__ out) {
  const uint64_t q = (uint64_t)BID * 256 + threadIdx.x;
  const uint64_t total = cnt * 5, b0 = q * 16;
  if (b0 >= total) return;
  const uint64_t v0 = b0 / 5;
  const uint32_t s = (uint32_t)(b0 - v0 * 5) * 8;
  const uint64_t M = 0xFFFFFFFFFFull;
  const uint64_t a = v[v0] & M, b = v0 + 1 < cnt ? v[v0 + 1] & M : 0, c2 = v0 + 2 < cnt ? v[v0 + 2] & M : 0,
                 d = v0 + 3 < cnt ? v[v0 + 3] & M : 0;
  const uint64_t lo = a | (b << 40), mid = (b >> 24) | (c2 << 16) | (d << 56), hi = d >> 8;
  const uint64_t olo = s ? (lo >> s) | (mid << (64 - s)) : lo, ohi = s ? (mid >> s) | (hi << (64 - s)) : mid;
  if (b0 + 16 <= total) st16u(out + b0, make_uint4((uint32_t)olo, (uint32_t)(olo >> 32), (uint32_t)ohi, (uint32_t)(ohi >> 32)));
  else
    for (uint64_t k = 0; b0 + k < total; k++) out[b0 + k] = (uint8_t)((k < 8 ? olo >> (8 * k) : ohi >> (8 * (k - 8))) & 0xff);
}
__global__ void unpack5_kernel(const uint8_t *__restrict__ in, uint64_t cnt, uint64_t *__restrict__ v) {
  uint64_t i = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const uint8_t *p = in + 5 * i;
  uint64_t x = 0;
#pragma unroll
  for (int b = 0; b < 5; b++) x |= (uint64_t)p[b] << (8 * b);
  v[i] = x;
}
void pack5_dev(pfp_ctx *c, const uint64_t *vals, uint64_t cnt, uint8_t *out5) {
  if (!cnt) return;
  KScope ks(c, "pfp::pack5_kernel", cnt * 13);
  hipLaunchKernelGGL(pack5_kernel, gdim((unsigned)cdiv64(cdiv64(cnt * 5, 16), TB)), gdim(TB), 0, c->stream, vals, cnt, out5);
  PFP_HIP(hipGetLastError());
}
void unpack5_dev(pfp_ctx *c, const uint8_t *in5, uint64_t cnt, uint64_t *vals) {
  if (!cnt) return;
  hipLaunchKernelGGL(unpack5_kernel, gdim(cdiv(cnt, TB)), gdim(TB), 0, c->stream, in5, cnt, vals);
  PFP_HIP(hipGetLastError());
}

// .ssa / .esa pairs of the whole BWT from the bitmaps: one thread per word of the start (end) map, the SA value of a
// set bit from its rank among all boundaries
__global__ __launch_bounds__(256) void bitmap_place_kernel(const uint64_t *__restrict__ map, const uint64_t *__restrict__ pre,
                                                           const uint64_t *__restrict__ bmap, const uint64_t *__restrict__ bpre,
                                                           const uint64_t *__restrict__ sa_c, uint64_t nw, uint8_t *__restrict__ out10,
                                                           uint64_t pos_base, int drop_first, uint64_t drop_pos) {
  const uint64_t w = (uint64_t)BID * 256 + threadIdx.x;
  if (w >= nw) return;
  uint64_t m = map[w];
  uint64_t o = pre[w];
  // a slice's edge that is no boundary after all (multi-GPU): position 0 leaves the list and every later pair moves
  // up by one; drop_pos (the slice's last position, or ~0) just leaves
  if (drop_first) { if (w == 0) m &= ~1ull; else o -= 1; }
  if ((drop_pos >> 6) == w) m &= ~(1ull << (drop_pos & 63));
  if (!m) return;
  const uint64_t all = bmap[w], rb = bpre[w];
  while (m) {
    const int b = __builtin_ctzll(m);
    m &= m - 1;
    const uint64_t x = pos_base + w * 64 + b, v = sa_c[rb + (uint64_t)__popcll(all & ((1ull << b) - 1ull))];
    uint8_t *dst = out10 + 10 * o++;
    reinterpret_cast<U64u *>(dst)->v = (x & 0xFFFFFFFFFFull) | (v << 40);       // 5 bytes of x, 3 low bytes of v
    reinterpret_cast<U16u *>(dst + 8)->v = (uint16_t)(v >> 24);                  // bytes 3, 4 of v
  }
}

// run boundaries: .ssa = <j,SA[j]> for BWT[j] != BWT[j-1] incl. j=0 (pfbwt.cpp:169-174,184-189);
//                 .esa = <j,SA[j]> for BWT[j] != BWT[j+1] incl. j=n (pfbwt.cpp:175-179,225-229)
// Two streaming passes over the BWT bytes of a slice [pos_base, pos_base+cnt) (16 positions per thread from
// one unaligned 16-byte load, the neighbour byte shifted in): boundaries counted per tile of 4096
// positions, tile offsets scanned, then every thread places its pairs <position, SA value> as 10 bytes.
// left / right: the BWT byte just outside the slice, or -1 at the ends of the whole BWT (then the
// edge position is a boundary by definition).
constexpr int kRunTile = 4096;
__global__ __launch_bounds__(256) void run_count_kernel(const uint8_t *__restrict__ bwt, uint64_t cnt, int left, int right,
                                                        int run_end, uint32_t *__restrict__ tile_cnt) {
  __shared__ uint32_t ws[4];
  if ((uint64_t)BID * kRunTile >= cnt) return;      // a workgroup of the padded last grid row
  const uint64_t base = (uint64_t)BID * kRunTile + (uint64_t)threadIdx.x * 16;
  uint32_t m[4];
  run_mask16(bwt, base, cnt, left, right, run_end, m);
  uint32_t c = __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[BID] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ __launch_bounds__(256) void run_place_kernel(const uint8_t *__restrict__ bwt, SaView sa,
                                                        uint64_t cnt, uint64_t pos_base, int left, int right, int run_end,
                                                        const uint64_t *__restrict__ tile_off, uint8_t *__restrict__ out10) {
  __shared__ uint32_t ws[4];
  if ((uint64_t)BID * kRunTile >= cnt) return;      // a workgroup of the padded last grid row
  const uint64_t base = (uint64_t)BID * kRunTile + (uint64_t)threadIdx.x * 16;
  uint32_t m[4];
  run_mask16(bwt, base, cnt, left, right, run_end, m);
  const uint32_t c = __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
  uint32_t inc = c;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  if (!c) return;
  uint64_t o = tile_off[BID] + inc - c;
  for (int q = 0; q < wv; q++) o += ws[q];
#pragma unroll
  for (int k = 0; k < 16; k++)
    if ((m[k >> 2] >> (8 * (k & 3))) & 1u) {
      const uint64_t x = pos_base + base + k, r = base + k;
      uint64_t v;
      if (sa.dense) v = sa.dense[r];
      else { const uint64_t wv = sa.bmap[r >> 6]; v = sa.sa_c[sa.bpre[r >> 6] + (uint64_t)__popcll(wv & ((1ull << (r & 63)) - 1ull))]; }
      uint8_t *dst = out10 + 10 * o;
      reinterpret_cast<U64u *>(dst)->v = (x & 0xFFFFFFFFFFull) | (v << 40);       // 5 bytes of x, 3 low bytes of v
      reinterpret_cast<U16u *>(dst + 8)->v = (uint16_t)(v >> 24);                  // bytes 3, 4 of v
      o++;
    }
}

RunSampler::RunSampler(pfp_ctx *c_, const uint8_t *bwt_, uint64_t cnt_, int left_, int right_, bool run_end_)
    : c(c_), bwt(bwt_), cnt(cnt_), left(left_), right(right_), run_end(run_end_) {
  ntile = cdiv64(cnt, kRunTile);
  alloc_counts(c, tile_cnt, ntile);
  tile_off.alloc(c, ntile + 1);
  if (ntile) {
    KScope ks(c, "pfp::run_count_kernel", cnt);
    hipLaunchKernelGGL(run_count_kernel, gdim((unsigned)ntile), gdim(256), 0, c->stream, bwt, cnt, left, right, run_end ? 1 : 0,
                       tile_cnt.p);
  }
  exclusive_sum_u32_u64(c, tile_cnt.p, tile_off.p, ntile + 1);
  PFP_HIP(hipGetLastError());
  pairs = read_scalar(c, tile_off.p + ntile);
}
void RunSampler::place(const SaView &sa, uint64_t pos_base, uint8_t *out10) {
  if (!ntile || !pairs) return;
  KScope ks(c, "pfp::run_place_kernel", cnt + pairs * 18);
  hipLaunchKernelGGL(run_place_kernel, gdim((unsigned)ntile), gdim(256), 0, c->stream, bwt, sa, cnt, pos_base, left, right,
                     run_end ? 1 : 0, tile_off.p, out10);
  PFP_HIP(hipGetLastError());
}

uint64_t sample_runs_dev(pfp_ctx *c, const uint8_t *bwt, const SaView &sa, uint64_t n_out, bool run_end,
                         DBuf<uint8_t> &out10) {
  const uint64_t *map = run_end ? sa.emap : sa.smap;
  if (map && sa.sa_c) {      // the merge left the run starts / ends as bitmaps
    const uint64_t pairs = run_end ? sa.n_ends : sa.n_starts;
    out10.alloc(c, pairs * 10 + 16);
    if (sa.n_words) {
      KScope ks(c, "pfp::bitmap_place_kernel", sa.n_words * 24 + pairs * 18);
      hipLaunchKernelGGL(bitmap_place_kernel, gdim(cdiv(sa.n_words, 256)), gdim(256), 0, c->stream, map, run_end ? sa.epre : sa.spre, sa.bmap,
                         sa.bpre, sa.sa_c, sa.n_words, out10.p, (uint64_t)0, 0, ~0ull);
      PFP_HIP(hipGetLastError());
    }
    return pairs;
  }
  RunSampler rs(c, bwt, n_out, -1, -1, run_end);
  out10.alloc(c, rs.pairs * 10 + 16);
  rs.place(sa, 0, out10.p);
  return rs.pairs;
}

uint64_t sample_runs_maps(pfp_ctx *c, const SaView &sa, uint64_t slice_n, bool run_end, bool drop_edge, uint64_t pos_base, uint8_t *out10) {
  const uint64_t *map = run_end ? sa.emap : sa.smap;
  PFP_REQUIRE(map && sa.sa_c, PFP_EINVAL, "no run maps: the merge was not run for a sampled SA without an SA array");
  const uint64_t all = run_end ? sa.n_ends : sa.n_starts;
  const uint64_t pairs = all - ((drop_edge && all) ? 1 : 0);
  if (!out10 || !pairs || !sa.n_words) return pairs;
  KScope ks(c, "pfp::bitmap_place_kernel", sa.n_words * 24 + pairs * 18);
  hipLaunchKernelGGL(bitmap_place_kernel, gdim(cdiv(sa.n_words, 256)), gdim(256), 0, c->stream, map, run_end ? sa.epre : sa.spre, sa.bmap,
                     sa.bpre, sa.sa_c, sa.n_words, out10, pos_base, (drop_edge && !run_end) ? 1 : 0,
                     (drop_edge && run_end && slice_n) ? slice_n - 1 : ~0ull);
  PFP_HIP(hipGetLastError());
  return pairs;
}

}  // namespace pfp
