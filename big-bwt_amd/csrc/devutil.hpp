// devutil.hpp -- small device-side helpers (unaligned vector access, sub-wave reductions).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace pfp {

// gfx950 runs with unaligned-access mode on: a dwordx4 global load/store may start at any byte.
struct __attribute__((packed, aligned(1))) U128u { uint32_t x, y, z, w; };
struct __attribute__((packed, aligned(1))) U64u { uint64_t v; };
struct __attribute__((packed, aligned(1))) U16u { uint16_t v; };

__device__ __forceinline__ uint4 ld16u(const uint8_t *p) {
  U128u v = *reinterpret_cast<const U128u *>(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st16u(uint8_t *p, uint4 v) {
  U128u u{v.x, v.y, v.z, v.w};
  *reinterpret_cast<U128u *>(p) = u;
}
__device__ __forceinline__ uint64_t ld8u(const uint8_t *p) { return reinterpret_cast<const U64u *>(p)->v; }

// Terminated strings (dictionary words: bytes >= 2, ended by one < 2).  Bit 7 of every byte of x that is below 2; lowest flag exact.
__device__ __forceinline__ uint32_t lt2_flags32(uint32_t x) { return (x - 0x02020202u) & ~x & 0x80808080u; }
__device__ __forceinline__ uint64_t lt2_flags64(uint64_t x) { return (x - 0x0202020202020202ull) & ~x & 0x8080808080808080ull; }
// One 8-byte step of comparing two terminated strings that are equal so far, x and y their next 8 bytes (little-endian):
// -1 / +1 = x's string is the smaller / larger, 0 = the same string (both end before they differ), kCmpOn = neither yet.
constexpr int kCmpOn = 2;
__device__ __forceinline__ int cmp_term8(uint64_t x, uint64_t y) {
  const uint64_t diff = x ^ y, term = lt2_flags64(x);
  if (!(diff | term)) return kCmpOn;
  const int fd = diff ? (__builtin_ctzll(diff) >> 3) : 8, ft = term ? (__builtin_ctzll(term) >> 3) : 8;
  if (ft < fd) return 0;                                    // both end before they differ: the same string
  const uint32_t bx = (uint32_t)(x >> (8 * fd)) & 0xffu, by = (uint32_t)(y >> (8 * fd)) & 0xffu;
  return bx < by ? -1 : 1;
}

// zero the bytes at index >= keep (0..16) of a little-endian 16-byte register block
__device__ __forceinline__ uint4 keep_bytes16(uint4 v, int keep) {
  uint32_t r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    int k = keep - 4 * i;
    r[i] = k >= 4 ? r[i] : (k <= 0 ? 0u : (r[i] & ((1u << (8 * k)) - 1u)));
  }
  return make_uint4(r[0], r[1], r[2], r[3]);
}

__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
  return k;
}

// sum / or over the 2^LG lanes of an aligned lane group (LG = 2 or 3)
template <int LG>
__device__ __forceinline__ uint64_t group_sum(uint64_t v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64);
  if (LG > 2) v += __shfl_xor(v, 4, 64);
  return v;
}
template <int LG>
__device__ __forceinline__ uint32_t group_or(uint32_t v) {
  v |= __shfl_xor(v, 1, 64); v |= __shfl_xor(v, 2, 64);
  if (LG > 2) v |= __shfl_xor(v, 4, 64);
  return v;
}

// inclusive prefix sum over the 64 lanes of a wave with DPP moves only (row_shr 1 / 2 / 4 / 8 inside the rows of 16 lanes, then
// the two row broadcasts gfx9 keeps for exactly this): six v_add with a DPP operand instead of six ds_bpermute round trips
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);      // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);      // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);      // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);      // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
  return v;
}

// minimum / maximum over the 64 lanes of a wave (all of them active), the same in every lane: the same six DPP steps - a lane
// without a source keeps the identity - leave the result in lane 63
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
  const int id = -1;      // 0xFFFFFFFF
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x111, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x112, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x114, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x118, 0xf, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x142, 0xa, 0xf, false));
  v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)v, 0x143, 0xc, 0xf, false));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// 16 flag bytes -> four words with bit 0 of every byte set where the flag is non-zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) {
  x |= x >> 4; x |= x >> 2; x |= x >> 1;
  return x & 0x01010101u;
}
__device__ __forceinline__ void load_flags16(const uint8_t *__restrict__ flags, uint64_t base, uint64_t n, uint32_t w[4]) {
  if (base + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4 *>(flags + base);
    w[0] = nonzero_bytes(v.x); w[1] = nonzero_bytes(v.y); w[2] = nonzero_bytes(v.z); w[3] = nonzero_bytes(v.w);
  } else {
    w[0] = w[1] = w[2] = w[3] = 0;
    for (int k = 0; k < 16; k++) if (base + k < n && flags[base + k]) w[k >> 2] |= 1u << (8 * (k & 3));
  }
}
// which of the 16 positions from `base` on of a BWT slice of cnt bytes start a run (run_end = 0: differ from the byte before) or
// end one (run_end = 1: differ from the byte after), as flag bytes like load_flags16; left / right: the byte just outside the
// slice, or -1 (then the edge position counts)
__device__ __forceinline__ void run_mask16(const uint8_t *__restrict__ bwt, uint64_t base, uint64_t cnt, int left, int right,
                                           int run_end, uint32_t m[4]) {
  m[0] = m[1] = m[2] = m[3] = 0;
  if (base >= cnt) return;
  if (base + 17 <= cnt && base >= 1) {          // interior: both neighbours of all 16 positions are inside the slice
    const uint4 x = ld16u(bwt + base);
    const uint4 y = run_end ? ld16u(bwt + base + 1) : ld16u(bwt + base - 1);
    m[0] = nonzero_bytes(x.x ^ y.x); m[1] = nonzero_bytes(x.y ^ y.y); m[2] = nonzero_bytes(x.z ^ y.z); m[3] = nonzero_bytes(x.w ^ y.w);
    return;
  }
  for (int k = 0; k < 16; k++) {
    const uint64_t i = base + k;
    if (i >= cnt) break;
    const int b = bwt[i];
    int nb;
    if (run_end) nb = i + 1 < cnt ? (int)bwt[i + 1] : right;
    else nb = i ? (int)bwt[i - 1] : left;
    if (nb < 0 || nb != b) m[k >> 2] |= 1u << (8 * (k & 3));
  }
}
// rank in a bitmap with a popcount directory of 512-bit superblocks: set bits of bits[] before bit r (bits[r >> 6] must exist)
__device__ __forceinline__ uint64_t bit_rank(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ dir, uint64_t r) {
  const uint64_t wi = r >> 6;
  uint64_t k = dir[r >> 9];
  for (uint64_t w = (r >> 9) << 3; w < wi; w++) k += __popcll(bits[w]);
  return k + __popcll(bits[wi] & ((1ull << (r & 63)) - 1));
}

// the 5-byte little-endian integer at byte off of a buffer of `bytes` bytes (the .sa / .ssa / .esa format)
__device__ __forceinline__ uint64_t ld5(const uint8_t *p, uint64_t off, uint64_t bytes) {
  if (off + 8 <= bytes) return ld8u(p + off) & 0xFFFFFFFFFFull;
  uint64_t v = 0;
  for (int i = 4; i >= 0; i--) v = (v << 8) | p[off + i];
  return v;
}
}  // namespace pfp
