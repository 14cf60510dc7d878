// fmhit.hpp -- the keys of the alignments of a read (fmmap.hip, fmpair.hip): the place key that orders a read's alignments by their
// start, and the hit key that is the order of the definition, (d, strand, s, e); include/pfpgpu.h, "Mapping reads".
#pragma once
#include "fmdev.hpp"

namespace pfp {

namespace {

constexpr uint64_t kNone = ~0ull;           // the key of an alignment that is not a hit (no key equals it: d <= 32)
constexpr int kSpanBits = 17, kPosBits = 40;

struct MapAln { uint64_t s, span; uint32_t d, strand; };
// the place key: the first sort orders a read's alignments by s
__device__ __forceinline__ uint64_t place_key(const MapAln &a) { return a.s << 24 | a.span << 7 | (uint64_t)a.d << 1 | a.strand; }
__device__ __forceinline__ MapAln from_place(uint64_t k) {
  return MapAln{k >> 24, k >> 7 & ((1ull << kSpanBits) - 1), (uint32_t)(k >> 1 & 63), (uint32_t)(k & 1)};
}
// the hit key: (d, strand, s, e) in the order of the definition
__device__ __forceinline__ uint64_t hit_key(const MapAln &a) { return (uint64_t)a.d << 58 | (uint64_t)a.strand << 57 | a.s << kSpanBits | a.span; }
__device__ __forceinline__ MapAln from_hit(uint64_t k) {
  return MapAln{k >> kSpanBits & ((1ull << kPosBits) - 1), k & ((1ull << kSpanBits) - 1), (uint32_t)(k >> 58), (uint32_t)(k >> 57 & 1)};
}

}  // namespace

}  // namespace pfp
