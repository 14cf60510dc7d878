// merge.hip -- stage 3: the final BWT / SA from the suffix order of the dictionary and the BWT of the parse.
//
// Replaces bwt() (pfbwt.cpp:109-242), its
// writers fwrite_chars_same_suffix{,_sa,_ssa} (pfbwt.cpp:520-676) and the threaded variant
// (pfthreads.hpp:83-518).  The reference walks SA(D) serially and fputc()s each char; here
// the walk is a data-parallel decomposition (the same one pfthreads.hpp:456-493 uses for its
// thread ranges): every dictionary suffix longer than w contributes occ(word) output chars,
// an exclusive scan of those counts fixes every output offset, and then
//   * fill entries are expanded output-centrically (each thread owns 16 consecutive BWT
//     bytes, finds its SA(D) slot by binary search and walks forward), the occurrences of
//     whole words are written one lane per inverted-list entry,
//   * groups of equal suffixes whose members disagree (or any multi-word group when SA values
//     are requested) are merged by rank computation over the members' inverted lists - the
//     data-parallel form of the reference's heap merge (pfbwt.cpp:537-556).
// The kernels come first; the host side (struct Merge: one member function per step, run() is the list) closes the file.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include <algorithm>
#include <cstdlib>

namespace pfp {

static constexpr int TB = 256;
constexpr int kOffTileLog = 11;      // slots per offset tile (= one expand workgroup): 2048

// ------------------------------------------------------------------ stage 3: the kernels

template <class I> struct alignas(16) Idx8 { I v[8]; };
// The same per-slot outputs when the records travelled in the top 16 bits of the first-round keys
// (SuffixOrder::paybits): a streaming read of skeys; only slots that later rounds re-ordered
// (refined[t]) fetch their record, and a count code of 255 its word's count.
template <class I>
__global__ __launch_bounds__(256) void slot_payload_kernel(uint64_t N, const I *__restrict__ sa,
                                                           const uint64_t *__restrict__ skeys,
                                                           const uint8_t *__restrict__ refined, const uint8_t *__restrict__ b,
                                                           WordView wv,
                                                           const uint32_t *__restrict__ wocc, uint32_t d, int w,
                                                           uint32_t *__restrict__ cnt, uint8_t *__restrict__ pc) {
  if ((uint64_t)BID * 2048 >= N) return;      // a workgroup of the padded last grid row
  uint64_t t0 = ((uint64_t)BID * 256 + threadIdx.x) * 8;
  uint32_t c8[8], p8[8];
  const int nk = t0 >= N ? 0 : ((N - t0) >= 8 ? 8 : (int)(N - t0));
  uint64_t rf = 0;
  if (refined) rf = nk == 8 ? *reinterpret_cast<const uint64_t *>(refined + t0) : ~0ull;      // tail: take the slow path
#pragma unroll
  for (int k = 0; k < 8; k++) {
    uint32_t rec = 0;
    if (k < nk) {
      rec = (uint32_t)(skeys[t0 + k] >> 48);
      if ((rf >> (8 * k)) & 0xffu) {
        const I i = sa[t0 + k];
        const uint32_t wd = word_of(wv, i);
        rec = 0;
        if (wd < d && wv.wend[wd] - i > (uint64_t)w) {
          const uint32_t occ = wocc[wd];
          rec = (i == 0 ? (uint32_t)kEndOfWord : (uint32_t)b[i - 1]) | ((occ < 255u ? occ : 255u) << 8);
        }
      }
    }
    p8[k] = rec & 0xffu; c8[k] = rec >> 8;
  }
#pragma unroll
  for (int k = 0; k < 8; k++) if (c8[k] == 255u) c8[k] = wocc[word_of(wv, sa[t0 + k])];
  if (nk == 8) {
    *reinterpret_cast<uint4 *>(cnt + t0) = make_uint4(c8[0], c8[1], c8[2], c8[3]);
    *reinterpret_cast<uint4 *>(cnt + t0 + 4) = make_uint4(c8[4], c8[5], c8[6], c8[7]);
    *reinterpret_cast<uint2 *>(pc + t0) = make_uint2(p8[0] | (p8[1] << 8) | (p8[2] << 16) | (p8[3] << 24),
                                                     p8[4] | (p8[5] << 8) | (p8[6] << 16) | (p8[7] << 24));
  } else {
    for (int k = 0; k < nk; k++) { cnt[t0 + k] = c8[k]; pc[t0 + k] = (uint8_t)p8[k]; }
  }
}
// ------------------------------------------------------------------ one gather per slot (BWT only / sparse SA)
//
// Random reads from HBM run at ~54 G accesses/s on this GPU whatever the element size up to 16 bytes (tools/microbench/
// gather.hip; only tables of <= 4 MB, one XCD's L2, are faster), so the merge makes exactly ONE random access per
// SA(D) slot and lets it carry everything any later kernel wants to know about the slot's suffix: a 16-byte record
// per dictionary POSITION, written by a streaming pass, gathered once per slot, and laid down again as per-SLOT
// arrays that every later kernel reads coalesced.  (Before: a 2-byte record per slot, then pos_word[sa[t]] ->
// wrec[...] per member in unit_edges_kernel and per (occurrence, member) in hard_minor_kernel: 2-3 dependent random
// sectors each, 9.5x / 34x the algorithmic bytes by the PMC counters of round 2.)
//   occ   occurrences of the position's word, 0 = the suffix emits nothing (<= w long, pfbwt.cpp:151; final 0x00)
//   first / last   smallest / largest BWT(P) position of the word's inverted list (ilist[ist], ilist[ist + occ - 1])
//   pcsl  low byte: preceding char, 1 (EndOfWord) = the suffix is a whole word (pfbwt.cpp:153);
//         bits 8..31: suffix length = distance to the word's terminator, capped at kSlCap (then: slen[] has it)
struct alignas(16) PosRec { uint32_t occ, first, last, pcsl; };
constexpr uint32_t kSlCap = 0xFFFFFFu;
// 256 positions per workgroup: the word of the block's first position is one table read (blocks start at multiples of
// 64), the words of the others follow from the terminators before them in the block (ballots); consecutive positions
// share their word's record.  dense_ist: full SA output wants the start of the word's inverted list where the sparse
// modes want its smallest position (field `first`).
// Positions [pos0, pos1), out[i - pos0] (pos0 a multiple of 256).
__global__ __launch_bounds__(256) void pprec16_kernel(WordView wv, int w, const uint4 *__restrict__ wrec /* WordRec as two uint4 */,
                                                      int dense_ist, uint64_t pos0, uint64_t pos1, PosRec *__restrict__ out) {
  __shared__ uint32_t wt[4];
  const uint64_t i = pos0 + (uint64_t)BID * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wvi = threadIdx.x >> 6;
  const uint32_t ch = i < wv.NP ? (uint32_t)wv.bytes[i] : 0u;
  const unsigned long long tm = __ballot(ch == (uint32_t)kEndOfWord);
  if (lane == 0) wt[wvi] = (uint32_t)__popcll(tm);
  __syncthreads();
  if (i >= pos1) return;
  uint32_t wd = wv.blk_word[(pos0 >> 6) + (uint64_t)BID * 4] + (uint32_t)__popcll(tm & ((1ull << lane) - 1ull));
  for (int q = 0; q < wvi; q++) wd += wt[q];
  PosRec r{0u, 0u, 0u, 0u};
  if (wd < wv.d) {
    const uint64_t sl = wv.wend[wd] - i;
    if (sl > (uint64_t)w) {
      const uint4 wr = wrec[2 * (uint64_t)wd];      // {ist, occ, first, last}
      const uint32_t pc = (i == 0) ? (uint32_t)kEndOfWord : (uint32_t)wv.bytes[i - 1];
      r = PosRec{wr.y, dense_ist ? wr.x : wr.z, wr.w, pc | ((sl < kSlCap ? (uint32_t)sl : kSlCap) << 8)};
    }
  }
  *reinterpret_cast<uint4 *>(out + (i - pos0)) = make_uint4(r.occ, r.first, r.last, r.pcsl);
}
// the same record for ONE position, computed where it is wanted: the position's 64-byte line of the dictionary (word
// lookup + preceding char) and its word's 32-byte record - two random sectors instead of one, and no 16 bytes per
// dictionary position.  A share of the suffix array (multi-GPU: N slots of NP positions, N << NP) and a dictionary whose
// records would not fit take this form.
__device__ __forceinline__ uint4 posrec_at(const WordView &wv, int w, const uint4 *__restrict__ wrec, int dense_ist, uint64_t i) {
  const uint32_t wd = word_of(wv, i);
  if (wd >= wv.d) return make_uint4(0u, 0u, 0u, 0u);
  const uint4 wr = wrec[2 * (uint64_t)wd], we = wrec[2 * (uint64_t)wd + 1];      // {ist, occ, first, last} {terminator position, -}
  const uint64_t sl = ((uint64_t)we.x | ((uint64_t)we.y << 32)) - i;
  if (sl <= (uint64_t)w) return make_uint4(0u, 0u, 0u, 0u);
  const uint32_t pc = (i == 0) ? (uint32_t)kEndOfWord : (uint32_t)wv.bytes[i - 1];
  return make_uint4(wr.y, dense_ist ? wr.x : wr.z, wr.w, pc | ((sl < kSlCap ? (uint32_t)sl : kSlCap) << 8));
}

// Per tile of 2048 slots (256 threads x 8 consecutive slots): gather the records, exclusive scan of the counts inside
// the tile (loc[], tile total -> tsum[]), preceding chars, and the hard-group flags: a slot
// whose preceding char differs from that of the slot before it IN THE SAME GROUP marks the group's head (members of a
// group are contiguous, so "not all chars equal" is seen at some adjacent pair; pfbwt.cpp:524-536).  Replaces
// slot_gather + slot_loc + group_flags: cnt[] (4 B per slot written and read again) is gone, pc[] is not re-read.
template <class I>
__global__ __launch_bounds__(256) void slot_records_kernel(uint64_t N, const I *__restrict__ sa, const I *__restrict__ grp,
                                                           const PosRec *__restrict__ prec, uint32_t *__restrict__ loc,
                                                           uint8_t *__restrict__ pc, uint32_t *__restrict__ sfirst,
                                                           uint32_t *__restrict__ slast, uint32_t *__restrict__ ssl,
                                                           uint64_t *__restrict__ tsum, uint32_t *__restrict__ overflow,
                                                           uint8_t *__restrict__ hard, int any_multi_is_hard, WordView view, int w,
                                                           const uint4 *__restrict__ wrec, int dense_ist) {
  // prec == null: no per-position records - every slot computes its own (posrec_at)
  __shared__ uint64_t ws[4];
  __shared__ uint32_t lpc[256];
  __shared__ I lgrp[256];
  if (((uint64_t)BID << kOffTileLog) > N) return;      // tiles 0 .. N >> 11 exist (a workgroup of the padded last grid row)
  const uint64_t t0 = ((uint64_t)BID << kOffTileLog) + (uint64_t)threadIdx.x * 8;
  const int nk = t0 >= N ? 0 : ((N - t0) >= 8 ? 8 : (int)(N - t0));
  I idx[8], g8[8];
  if (nk == 8) {
    const Idx8<I> v8 = *reinterpret_cast<const Idx8<I> *>(sa + t0), w8 = *reinterpret_cast<const Idx8<I> *>(grp + t0);
#pragma unroll
    for (int k = 0; k < 8; k++) { idx[k] = v8.v[k]; g8[k] = w8.v[k]; }
  } else {
    for (int k = 0; k < 8; k++) { idx[k] = k < nk ? sa[t0 + k] : (I)0; g8[k] = k < nk ? grp[t0 + k] : IdxTraits<I>::kNone; }
  }
  uint4 r8[8];
#pragma unroll
  for (int k = 0; k < 8; k++)
    r8[k] = k >= nk ? make_uint4(0u, 0u, 0u, 0u)
                    : (prec ? *reinterpret_cast<const uint4 *>(prec + (uint64_t)idx[k]) : posrec_at(view, w, wrec, dense_ist, (uint64_t)idx[k]));
  // the slot before this thread's first one: the previous thread's last slot, or (first thread) the last slot of the tile before
  uint32_t p8[8];
#pragma unroll
  for (int k = 0; k < 8; k++) p8[k] = r8[k].w & 0xffu;
  lpc[threadIdx.x] = p8[7]; lgrp[threadIdx.x] = g8[7];
  uint32_t prev_pc = 0; I prev_g = IdxTraits<I>::kNone;
  if (threadIdx.x == 0 && t0 > 0 && nk) {
    prev_pc = (prec ? prec[(uint64_t)sa[t0 - 1]].pcsl : posrec_at(view, w, wrec, dense_ist, (uint64_t)sa[t0 - 1]).w) & 0xffu;
    prev_g = grp[t0 - 1];
  }
  // counts: exclusive scan inside the tile
  uint64_t own = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) own += r8[k].x;
  uint64_t inc = own;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) { const uint64_t u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  if (threadIdx.x > 0) { prev_pc = lpc[threadIdx.x - 1]; prev_g = lgrp[threadIdx.x - 1]; }
  uint64_t run = inc - own;
  for (int q = 0; q < wv; q++) run += ws[q];
  uint32_t o8[8];
#pragma unroll
  for (int k = 0; k < 8; k++) { o8[k] = (uint32_t)run; run += r8[k].x; }
  // (loc[] is padded to whole tiles: the slots past N get the running total, slot N's is what slot_off(N) reads)
  *reinterpret_cast<uint4 *>(loc + t0) = make_uint4(o8[0], o8[1], o8[2], o8[3]);
  *reinterpret_cast<uint4 *>(loc + t0 + 4) = make_uint4(o8[4], o8[5], o8[6], o8[7]);
  if (threadIdx.x == 255) {
    tsum[BID] = run;
    if (run >> 32) atomicOr(overflow, 1u);      // a tile's offsets would not fit 32 bits
  }
  if (nk == 8) {
    *reinterpret_cast<uint2 *>(pc + t0) = make_uint2(p8[0] | (p8[1] << 8) | (p8[2] << 16) | (p8[3] << 24),
                                                     p8[4] | (p8[5] << 8) | (p8[6] << 16) | (p8[7] << 24));
    if (sfirst) {
      *reinterpret_cast<uint4 *>(sfirst + t0) = make_uint4(r8[0].y, r8[1].y, r8[2].y, r8[3].y);
      *reinterpret_cast<uint4 *>(sfirst + t0 + 4) = make_uint4(r8[4].y, r8[5].y, r8[6].y, r8[7].y);
    }
    if (slast) {
      *reinterpret_cast<uint4 *>(slast + t0) = make_uint4(r8[0].z, r8[1].z, r8[2].z, r8[3].z);
      *reinterpret_cast<uint4 *>(slast + t0 + 4) = make_uint4(r8[4].z, r8[5].z, r8[6].z, r8[7].z);
    }
    if (ssl) {
      *reinterpret_cast<uint4 *>(ssl + t0) = make_uint4(r8[0].w >> 8, r8[1].w >> 8, r8[2].w >> 8, r8[3].w >> 8);
      *reinterpret_cast<uint4 *>(ssl + t0 + 4) = make_uint4(r8[4].w >> 8, r8[5].w >> 8, r8[6].w >> 8, r8[7].w >> 8);
    }
  } else {
    for (int k = 0; k < nk; k++) {
      pc[t0 + k] = (uint8_t)p8[k];
      if (sfirst) sfirst[t0 + k] = r8[k].y;
      if (slast) slast[t0 + k] = r8[k].z;
      if (ssl) ssl[t0 + k] = r8[k].w >> 8;
    }
  }
  // hard groups: a differing char next to a member of the same group
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (k < nk && p8[k] != 0 && g8[k] == prev_g && (any_multi_is_hard || p8[k] != prev_pc)) hard[g8[k]] = 1;      // (SA output: any group of several words, pfbwt.cpp:568, 612)
    prev_pc = p8[k]; prev_g = g8[k];
  }
}

// a group is "hard" when its members disagree on the preceding char (pfbwt.cpp:524-536), or, with
// SA output, whenever it has more than one member (pfbwt.cpp:568, 612)
template <class I>
__global__ void group_flags_kernel(uint64_t N, const I *__restrict__ grp, const uint8_t *__restrict__ pc,
                                   int any_multi_is_hard, uint8_t *__restrict__ hard) {
  uint64_t t = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (t >= N || pc[t] == 0) return;
  I g = grp[t];
  if (g == t) return;
  if (any_multi_is_hard || pc[t] != pc[g]) hard[g] = 1;
}

enum : uint8_t { CLS_NONE = 0, CLS_FILL = 1, CLS_FULL = 2, CLS_HARD = 3 };
// SA values asked for: none (BWT only), every position (-S), or only where the sampled SA files can look:
// at run boundaries of the BWT (-s / -e)
enum : int { SA_NONE = 0, SA_DENSE = 1, SA_SPARSE = 2 };

// per word: start of its inverted list, number of occurrences, smallest / largest BWT(P) position, end - one 32-byte record,
// one memory sector for everything a hard-group or unit-edge kernel wants to know about a member's word
struct alignas(32) WordRec { uint32_t ist, occ, first, last; uint64_t wend, pad; };      // wend: position of the word's terminator
__global__ void wistart_kernel(uint32_t d, const uint32_t *__restrict__ lexrank, const uint32_t *__restrict__ istart_lex,
                               const uint32_t *__restrict__ wocc, const uint32_t *__restrict__ ilist,
                               const uint64_t *__restrict__ wend, uint32_t *__restrict__ wistart, WordRec *__restrict__ wrec) {
  uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j >= d) return;
  const uint32_t st = istart_lex[lexrank[j]] + 1;   // +1: ilist[0] is the EOS symbol (pfbwt.cpp:389)
  wistart[j] = st;
  if (wrec) { const uint32_t oc = wocc[j]; wrec[j] = WordRec{st, oc, ilist[st], ilist[st + oc - 1], wend[j], 0}; }
}

// sparse SA: what the BWT round leaves of a ranked occurrence of a fallback group for the SA round - its BWT(P) position
// and suffix length; the entry's index says where it landed (staging offset of the group + rank inside the group)
struct alignas(8) RankedOcc { uint32_t pos, sl; };
constexpr uint32_t kUnwritten = 0xFFFFFFFFu;      // both fields of an entry nobody wrote (PFP_DEBUG fills the staging with 0xFF)

template <class I>
struct MergeArgsT {
  uint64_t N, n_out; uint32_t d; int w; int want_sa;
  uint64_t pos_base, n_out_global;   // global BWT position of local position 0; global n+1 (== n_out unless the slots are one rank's range)
  uint64_t out_lo, out_hi;   // this call emits BWT positions [out_lo,out_hi) only (multi-GPU slices); bwt/out_sa are indexed by global position
  const I *sa, *grp;
  WordView wv;               // word / suffix length of a dictionary position where no per-slot copy exists
  const uint32_t *ist, *wistart;
  const WordRec *wrec;
  // per-slot copies of the gathered position records (slot_records_kernel; null: look the word up through sa / pos_word):
  // smallest / largest BWT(P) position of the slot's word, suffix length (kSlCap = look it up in slen[])
  const uint32_t *sfirst, *slast, *ssl;
  const uint8_t *pc, *hard, *gmaj;     // gmaj[g]: majority char of hard group g when the minority path places the rest (else 0)
  const uint64_t *tbase; const uint32_t *loc;    // output offset of slot t = tbase[t >> 11] + loc[t] (slot_off)
  const uint32_t *ilist; const uint8_t *bwlast; const uint64_t *bwsai;
  // whole words, one lane per inverted-list entry e (word_chars_kernel, word_sa_kernel): iword[e + 1] - 1 = q, the
  // lexicographic rank of the entry's word, whose list starts at istart_lex[q] + 1 and whose whole-word slot is wslot_lex[q]
  // (a global slot: local slot + slot_base)
  const uint32_t *istart_lex, *iword; const uint64_t *wslot_lex; uint64_t slot_base;
  uint8_t *bwt; uint64_t *out_sa;
  // what a launch writes: BWT chars (bit 0), SA values (bit 1).  Dense SA does both at once; sparse SA needs the finished
  // BWT to know where values are looked at, so its kernels run twice.
  int pass;
  // sparse SA: bit (x - out_lo) of bmap is set where position x starts or ends a run of the BWT (the two ends of the
  // slice always count); bpre[k] = boundaries before bit 64 k.  SA values go to sa_c[rank of x among the boundaries]
  // (the caller keeps no SA array), or to out_sa[x] - only where the bit is set.
  const uint64_t *bmap, *bpre;
  uint64_t *sa_c;
  // sparse SA with replay: where the kernels that rank a fallback group's occurrences leave them (null: the SA round
  // ranks them again) - entry soff[h] + r is the occurrence of rank r of the group whose head is the h-th of the fallback list
  RankedOcc *ranked; const uint64_t *soff;
};
enum : int { PASS_BWT = 1, PASS_SA = 2 };
template <class I>
__device__ __forceinline__ void sa_put(const MergeArgsT<I> &a, uint64_t x, uint64_t v) {
  if (x < a.out_lo || x >= a.out_hi) return;
  if (!a.bmap) { a.out_sa[x] = v; return; }
  const uint64_t r = x - a.out_lo, wv = a.bmap[r >> 6];
  if (!((wv >> (r & 63)) & 1ull)) return;
  if (a.sa_c) a.sa_c[a.bpre[r >> 6] + (uint64_t)__popcll(wv & ((1ull << (r & 63)) - 1ull))] = v;
  else a.out_sa[x] = v;
}
// sa_put for a caller that has looked at x itself: x lies in the slice and its bit is set in `word`, the word of the
// boundary map that holds it, `pre` that word's bpre[] entry (both unused without a map) - the map is not read again
template <class I>
__device__ __forceinline__ void sa_put_at(const MergeArgsT<I> &a, uint64_t x, uint64_t word, uint64_t pre, uint64_t v) {
  if (a.bmap && a.sa_c) a.sa_c[pre + (uint64_t)__popcll(word & ((1ull << ((x - a.out_lo) & 63)) - 1ull))] = v;
  else a.out_sa[x] = v;
}
template <class I>
__device__ __forceinline__ bool sa_wanted(const MergeArgsT<I> &a, uint64_t x) {      // would sa_put(x) store anything?
  if (x < a.out_lo || x >= a.out_hi) return false;
  if (!a.bmap) return true;
  const uint64_t r = x - a.out_lo;
  return (a.bmap[r >> 6] >> (r & 63)) & 1ull;
}
// SA round of the replay: the occurrence that the BWT round ranked to output position o and staged at ranked[idx].  The
// boundary bit of o is looked at first; the entry and bwsai[] are read only where a value is stored.  `unwritten`
// (PFP_DEBUG, else null): every entry of the slice is read and one that nobody wrote is counted
template <class I>
__device__ __forceinline__ void sa_replay(const MergeArgsT<I> &a, uint64_t idx, uint64_t o, unsigned long long *unwritten) {
  if (o < a.out_lo || o >= a.out_hi) return;
  const uint64_t r = o - a.out_lo, word = a.bmap[r >> 6];
  const bool at = (word >> (r & 63)) & 1ull;
  if (!at && !unwritten) return;
  const RankedOcc e = a.ranked[idx];
  if (unwritten && e.pos == kUnwritten && e.sl == kUnwritten) { atomicAdd(unwritten, 1ull); return; }
  if (at) sa_put_at(a, o, word, a.bpre[r >> 6], a.bwsai[e.pos] - (uint64_t)e.sl);
}
// Exclusive prefix of the per-slot counts, kept as a 64-bit base per 2048 slots (= one expand workgroup) and a
// 32-bit offset inside the tile: 4 bytes per slot to write and read instead of 8, and the N-long scan
// becomes one streaming tile kernel plus a scan over N/2048 sums.
template <class I>
__device__ __forceinline__ uint64_t slot_off(const MergeArgsT<I> &a, uint64_t t) { return a.tbase[t >> kOffTileLog] + a.loc[t]; }


__device__ __forceinline__ uint8_t fix_char(uint8_t ch) { return ch == kDollar ? 0 : ch; }  // pfbwt.cpp:126
// start of slot t's word in ilist: stored per slot when SA values are wanted, looked up otherwise
// (BWT only needs it for hard groups)
template <class I>
__device__ __forceinline__ uint32_t slot_ist(const MergeArgsT<I> &a, uint64_t t) {
  return a.ist ? a.ist[t] : a.wistart[word_of(a.wv, a.sa[t])];
}

// what the hard-group / unit-edge kernels ask about the word of slot t: from the per-slot arrays when the slot records
// were gathered (one coalesced read), else through sa -> pos_word -> the word's record (three dependent random reads)
template <class I>
__device__ __forceinline__ uint32_t slot_first(const MergeArgsT<I> &a, uint64_t t) { return a.sfirst ? a.sfirst[t] : a.wrec[word_of(a.wv, a.sa[t])].first; }
template <class I>
__device__ __forceinline__ uint32_t slot_last(const MergeArgsT<I> &a, uint64_t t) { return a.slast ? a.slast[t] : a.wrec[word_of(a.wv, a.sa[t])].last; }
template <class I>
__device__ __forceinline__ uint64_t slot_slen(const MergeArgsT<I> &a, uint64_t t) {
  if (a.ssl) { const uint32_t v = a.ssl[t]; if (v != kSlCap) return v; }
  return slen_of(a.wv, a.sa[t]);
}

// Expansion.  One workgroup owns kSlots consecutive SA(D) slots, i.e. one contiguous range of
// the output; slot offsets, classes and chars are staged in LDS and every thread then produces 16
// consecutive BWT bytes per iteration (binary search in LDS for the first one, forward walk for
// the rest) and stores them with one 16-byte store.
//   fill entry      : the preceding char, occ times                       (pfbwt.cpp:527-533)
//   full-word entry : bwlast[ilist[..]] per occurrence                    (pfbwt.cpp:153-197): zeros here, the chars
//                     come from word_chars_kernel, one lane per occurrence - in the 16-byte walk every such byte was
//                     two dependent random loads on which the other 63 lanes of the wave waited
//   hard entry     : each occurrence is ranked among all occurrences of all members of its group
//                     by BWT(P) position - own index + lower_bound in every other member's
//                     inverted list - and written to that slot of the group's range: the
//                     data-parallel form of the reference's heap merge (pfbwt.cpp:537-556).
constexpr int kHardLds = 1024;   // occurrences of a group one wave sorts in LDS (hard_sort_kernel)
constexpr int kHardRank = 512;   // occurrences of one batch ranked in LDS (hard_groups_kernel): larger groups are sorted anyway,
                                 // and 7.6 KB of tables per wave instead of 10 let five workgroups share a CU instead of three
constexpr int kHardMem = 256;    // members of one batch
constexpr int kHardSortMin = 512;   // a group with more occurrences than this (and <= kHardLds) is sorted, not ranked all-pairs
constexpr int kSlots = 2048;
constexpr uint64_t kExpandQuota = 1u << 16;   // output bytes one workgroup expands before the rest is shared

// kDense: SA values everywhere (-S) - expand_sa_1 then asks for a slot's class and, for a whole word, the start of its
// inverted list; the chars alone need neither (12 KB of LDS per workgroup less)
template <bool kDense>
struct ExpandLds {
  uint32_t loff[kSlots + 1];      // offsets inside the tile fit 32 bits (slot_loc_kernel checks)
  uint8_t lch[kSlots];            // the byte the slot's range is filled with (0: written by a later kernel)
  uint8_t lcls[kDense ? kSlots : 1];
  uint32_t lfist[kDense ? kSlots : 1];      // whole-word slots: start of the word's inverted list
};

template <class I, bool kDense>
__device__ __forceinline__ void expand_stage(const MergeArgsT<I> &a, ExpandLds<kDense> &L, uint64_t t0, int ns, uint64_t base) {
  for (int s = threadIdx.x; s <= ns; s += 256) L.loff[s] = (uint32_t)(slot_off(a, t0 + s) - base);
  for (int s = threadIdx.x; s < ns; s += 256) {
    const uint64_t t = t0 + s;
    const uint8_t pc = a.pc[t];
    uint8_t cls = pc == 0 ? CLS_NONE : (pc == kEndOfWord ? CLS_FULL : CLS_FILL);
    uint8_t ch = 0;      // whole words: every occurrence has a char of its own (word_chars_kernel)
    if (cls == CLS_FILL) {
      ch = fix_char(pc);
      const I g = a.grp[t];
      if (a.hard[g]) {
        cls = CLS_HARD;
        ch = a.gmaj ? a.gmaj[g] : 0;      // the group's majority char (its other occurrences are placed by hard_minor_kernel), or 0:
      }                                   // every position of the group is written by the hard-group kernels that run after this one
    }
    L.lch[s] = ch;
    if constexpr (kDense) {
      L.lcls[s] = cls;
      if (cls == CLS_FULL) L.lfist[s] = a.ist[t];
    }
  }
  __syncthreads();
}

// 16 output bytes starting at block-relative offset x0 (< Ltot)
template <class I, bool kDense>
__device__ __forceinline__ void expand_16(const MergeArgsT<I> &a, const ExpandLds<kDense> &L, int ns, uint64_t base, uint64_t x0,
                                          uint64_t Ltot) {
  if (base + x0 + 16 <= a.out_lo || base + x0 >= a.out_hi) return;     // outside this rank's slice
  int lo = 0, hi = ns;                    // loff[lo] <= x0 < loff[hi]
  while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (L.loff[mid] <= x0) lo = mid; else hi = mid; }
  int s = lo;
  uint64_t nxt = L.loff[s + 1];
  const int nb = (Ltot - x0) >= 16 ? 16 : (int)(Ltot - x0);
  uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    if (k < nb) {
      const uint64_t x = x0 + k;
      while (x >= nxt) { s++; nxt = L.loff[s + 1]; }
      const uint32_t sh = (uint32_t)L.lch[s] << (8 * (k & 3));
      if (k < 4) r0 |= sh; else if (k < 8) r1 |= sh; else if (k < 12) r2 |= sh; else r3 |= sh;
    }
  }
  uint8_t *dst = a.bwt + base + x0;
  if (nb == 16 && base + x0 >= a.out_lo && base + x0 + 16 <= a.out_hi) st16u(dst, make_uint4(r0, r1, r2, r3));
  else {
    const uint32_t rr[4] = {r0, r1, r2, r3};
#pragma unroll
    for (int k = 0; k < 16; k++)
      if (k < nb && base + x0 + k >= a.out_lo && base + x0 + k < a.out_hi) dst[k] = (uint8_t)(rr[k >> 2] >> (8 * (k & 3)));
  }
}

// SA value of block-relative output position x (fill and full-word entries; hard groups write their
// own).  One lane per position, so that the 8-byte stores of a wave are 512 contiguous bytes - the
// 16-positions-per-thread layout of expand_16 would put every lane's store in a different 128-byte line.
template <class I>
__device__ __forceinline__ void expand_sa_1(const MergeArgsT<I> &a, const ExpandLds<true> &L, uint64_t t0, int ns, uint64_t base,
                                            uint64_t x) {
  if (base + x < a.out_lo || base + x >= a.out_hi) return;
  int lo = 0, hi = ns;                    // loff[lo] <= x < loff[hi]
  while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (L.loff[mid] <= x) lo = mid; else hi = mid; }
  const uint8_t cl = L.lcls[lo];
  if (cl != CLS_FULL && cl != CLS_FILL) return;
  if (!sa_wanted(a, base + x)) return;
  const uint64_t pos = a.ilist[(cl == CLS_FULL ? L.lfist[lo] : slot_ist(a, t0 + lo)) + (uint32_t)(x - L.loff[lo])];
  sa_put(a, base + x, (cl == CLS_FULL && a.pos_base + base + x == 0) ? a.n_out_global - 1 : a.bwsai[pos] - slot_slen(a, t0 + lo));
}

// Sparse SA mode (-s / -e without -S): SA values are only looked at where a run of the BWT starts or ends.
//   * a whole word's occurrences carry unrelated chars (bwlast): all their SA values are written, P positions in
//     all - word_sa_kernel;
//   * a slot, or a group of slots, whose chars all agree fills its range with one char: only the first and
//     the last position of that range can be run boundaries - unit_edges_kernel;
//   * hard groups: the two ends (unit_edges_kernel) and what the hard-group kernels find inside.
template <class I, bool kDense>
__global__ __launch_bounds__(256) void expand_kernel(MergeArgsT<I> a, uint32_t *__restrict__ heavy, uint32_t *__restrict__ nheavy,
                                                     uint32_t heavy_cap) {
  __shared__ ExpandLds<kDense> L;
  const uint64_t t0 = (uint64_t)BID * kSlots;
  if (t0 >= a.N) return;      // a workgroup of the padded last grid row
  const int ns = (a.N - t0) >= (uint64_t)kSlots ? kSlots : (int)(a.N - t0);
  const uint64_t base = slot_off(a, t0);
  expand_stage(a, L, t0, ns, base);
  const uint64_t Ltot = L.loff[ns];
  if (base + Ltot <= a.out_lo || base >= a.out_hi) return;
  // a block whose slots emit more than the quota (a word with hundreds of thousands of
  // occurrences) finishes only its first quota here; expand_heavy_kernel shares the rest
  const uint64_t mine = Ltot <= kExpandQuota ? Ltot : kExpandQuota;
  if (Ltot > kExpandQuota && threadIdx.x == 0) { uint32_t i = atomicAdd(nheavy, 1u); if (i < heavy_cap) heavy[i] = BID; }
  for (uint64_t x0 = (uint64_t)threadIdx.x * 16; x0 < mine; x0 += 256 * 16) expand_16(a, L, ns, base, x0, Ltot);
  if constexpr (kDense)
    for (uint64_t x = threadIdx.x; x < mine; x += 256) expand_sa_1(a, L, t0, ns, base, x);
}

template <class I, bool kDense>
__global__ __launch_bounds__(256) void expand_heavy_kernel(MergeArgsT<I> a, const uint32_t *__restrict__ heavy, uint32_t nheavy) {
  __shared__ ExpandLds<kDense> L;
  for (uint32_t q = 0; q < nheavy; q++) {
    const uint64_t t0 = (uint64_t)heavy[q] * kSlots;
    const int ns = (a.N - t0) >= (uint64_t)kSlots ? kSlots : (int)(a.N - t0);
    const uint64_t base = slot_off(a, t0);
    __syncthreads();
    expand_stage(a, L, t0, ns, base);
    const uint64_t Ltot = L.loff[ns];
    for (uint64_t x0 = kExpandQuota + ((uint64_t)BID * 256 + threadIdx.x) * 16; x0 < Ltot; x0 += (uint64_t)GDIM * 256 * 16)
      expand_16(a, L, ns, base, x0, Ltot);
    if constexpr (kDense)
      for (uint64_t x = kExpandQuota + (uint64_t)BID * 256 + threadIdx.x; x < Ltot; x += (uint64_t)GDIM * 256)
        expand_sa_1(a, L, t0, ns, base, x);
  }
}

// Whole words, one lane per occurrence e of the inverted lists laid end to end (iword[e + 1], ilist[e + 1]: read coalesced).
// The entry's word is the one of lexicographic rank q = iword[e + 1] - 1 (the sorted symbols of the inverted-list sort), the
// word's slot is wslot_lex[q], the output position that slot's offset plus the occurrence's index in its list; lanes of one
// word read the same q-indexed entries.  false: the word's slot belongs to another rank's range (multi-GPU).
template <class I>
__device__ __forceinline__ bool word_entry(const MergeArgsT<I> &a, uint64_t e, uint64_t &t, uint64_t &x) {
  const uint32_t q = a.iword[e + 1] - 1u;
  const uint64_t gs = a.wslot_lex[q];
  if (gs < a.slot_base || gs - a.slot_base >= a.N) return false;
  t = gs - a.slot_base;
  x = slot_off(a, t) + (e - (uint64_t)a.istart_lex[q]);
  return true;
}
// the chars: every occurrence of a whole word carries its own (bwlast of its BWT(P) position; pfbwt.cpp:153-197) - written
// over the zeros expand_kernel left there
template <class I>
__global__ __launch_bounds__(256) void word_chars_kernel(MergeArgsT<I> a, uint64_t P) {
  const uint64_t e = (uint64_t)BID * 256 + threadIdx.x;
  if (e >= P) return;
  uint64_t t, x;
  if (!word_entry(a, e, t, x) || x < a.out_lo || x >= a.out_hi) return;
  a.bwt[x] = a.bwlast[a.ilist[e + 1]];       // +1: ilist[0] is the EOS symbol (pfbwt.cpp:389)
}
// Sparse SA mode: any of the P positions the whole words emit can be a run boundary (unrelated chars).
// (Staging every tile of expand_kernel again would find a dozen whole words in each.)
template <class I>
__global__ __launch_bounds__(256) void word_sa_kernel(MergeArgsT<I> a, uint64_t P) {
  const uint64_t e = (uint64_t)BID * 256 + threadIdx.x;
  if (e >= P) return;
  uint64_t t, x;
  if (!word_entry(a, e, t, x) || !sa_wanted(a, x)) return;
  const uint64_t pos = a.ilist[e + 1];
  sa_put(a, x, a.pos_base + x == 0 ? a.n_out_global - 1 : a.bwsai[pos] - slot_slen(a, t));
}
// iword[] where the parse stage did not leave it (inverted lists read from a file): entry e belongs to the word of rank q
// with istart_lex[q] <= e < istart_lex[q + 1]
__global__ void iword_kernel(uint64_t P, uint32_t d, const uint32_t *__restrict__ istart_lex, uint32_t *__restrict__ iword) {
  const uint64_t e = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (e > P) return;
  if (e == P) { iword[0] = 0; return; }
  uint32_t lo = 0, hi = d;
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if ((uint64_t)istart_lex[mid] <= e) lo = mid; else hi = mid; }
  iword[e + 1] = lo + 1;
}

// Sparse SA mode.  A *unit* is a slot that emits, or a group of slots of equal suffixes (several words share the
// suffix): its output range is one fill char c (unknown for hard groups), so a run of the BWT can start only at
// the unit's first position - when the unit before ends in a different char - and end only at its last position.
// The first position belongs to the smallest BWT(P) position over the members' inverted lists, the last one to the
// largest (WordRec::first / last per word): O(members) per unit instead of merging the lists (pfbwt.cpp:605-676 walks a
// heap through all of them).  One lane per slot: whether the two positions can be sampled from the boundary bitmap of
// the finished BWT, "needed" flags spread over a unit's lanes, segmented min / max by shuffles; the part of a unit that
// lies outside the wave is fetched by all 64 lanes together.
// A unit is a contiguous run of lanes, so everything a lane asks about its unit follows from one ballot: cont (the unit
// goes on in the next slot).  Lanes l and l + o belong to one unit when no cont bit in [l, l + o) is clear; only mn and
// mx travel through the shuffles (before: the group and the unit flag with them at every step, 70 ds_bpermute per wave).
__device__ __forceinline__ uint32_t lane_read(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ uint64_t lane_read(uint64_t v, int l) {
  return (uint64_t)lane_read((uint32_t)v, l) | ((uint64_t)lane_read((uint32_t)(v >> 32), l) << 32);
}
template <class I>
__global__ __launch_bounds__(256) void unit_edges_kernel(MergeArgsT<I> a) {
  const uint64_t t = (uint64_t)BID * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const uint64_t wbase = t - lane;
  const bool in = t < a.N;
  // ---- round trip 1: everything that is addressed by t alone, asked for by every lane with a slot (streams that are read
  // anyway: most units are one slot, which is head and last member at once).  What keeps each load inside its allocation:
  //   pc[t + 1], grp[t + 1] : t + 1 <= N, and pc and grp have N + 8 entries (their values at N are never used: `t + 1 < N` below)
  //   loc[t + 1]            : loc is padded to whole offset tiles, ntile * 2048 > N entries (slot N's is the tile's running total)
  //   tbase[(t + 1) >> 11]  : (t + 1) >> 11 <= N >> 11 = ntile - 1, and tbase has ntile + 1 entries
  uint32_t ch = 0, ch_n = 0, loc_t = 0, loc_n = 0;
  uint64_t tb_t = 0, tb_n = 0;
  I g = 0, g_n = 0;
  if (in) {
    ch = a.pc[t]; g = a.grp[t];
    loc_t = a.loc[t]; loc_n = a.loc[t + 1];
    tb_t = a.tbase[t >> kOffTileLog]; tb_n = a.tbase[(t + 1) >> kOffTileLog];
    if (lane == 63) { ch_n = a.pc[t + 1]; g_n = a.grp[t + 1]; }       // the next wave's first slot
  }
  const bool unit = ch != 0 && ch != kEndOfWord;        // lanes that belong to a fill / hard unit (whole words: word_sa_kernel)
  if (!unit) g = 0;
  const unsigned long long um = __ballot(unit);
  // same unit as the next slot?
  const I g_next = __shfl_down(g, 1, 64);
  const bool unit_next = (um >> ((lane + 1) & 63)) & 1ull;
  bool cont;                                       // the unit goes on in slot t + 1
  if (lane < 63) cont = unit && unit_next && g_next == g;
  else cont = unit && t + 1 < a.N && ch_n != 0 && ch_n != kEndOfWord && g_n == g;
  const unsigned long long cm = __ballot(cont);
  const bool head = unit && (uint64_t)g == t;
  const bool last = unit && !cont;
  // ---- round trip 2: is the unit's first / last position one the sampled files can look at?  The word of the boundary map
  // and its prefix count together - the store at the end needs both, and their index is known as soon as the offset is
  const uint64_t o_first = tb_t + loc_t, o_last = tb_n + loc_n - 1;       // (slot_off(t), slot_off(t + 1) - 1: a unit lane emits)
  const bool ask_first = head && o_first >= a.out_lo && o_first < a.out_hi;
  const bool ask_last = last && o_last >= a.out_lo && o_last < a.out_hi;
  uint64_t w_first = ~0ull, w_last = ~0ull, p_first = 0, p_last = 0;      // (no map: every position of the slice is wanted)
  if (a.bmap) {
    if (ask_first) { const uint64_t k = (o_first - a.out_lo) >> 6; w_first = a.bmap[k]; p_first = a.bpre[k]; }
    if (ask_last) { const uint64_t k = (o_last - a.out_lo) >> 6; w_last = a.bmap[k]; p_last = a.bpre[k]; }
  }
  const bool need_first = ask_first && ((w_first >> ((o_first - a.out_lo) & 63)) & 1ull);
  const bool need_last = ask_last && ((w_last >> ((o_last - a.out_lo) & 63)) & 1ull);
  // spread the two flags over the lanes of the unit that lie in this wave
  const bool head_here = unit && (uint64_t)g >= wbase;
  const int hl = head_here ? (int)((uint64_t)g - wbase) : lane;
  const unsigned long long lm = __ballot(last) >> lane;      // (the first `last` lane at or after a unit lane is its own unit's)
  const int ll = lm ? lane + (__ffsll((long long)lm) - 1) : lane;
  const bool nf = head_here && ((__ballot(need_first) >> hl) & 1ull);
  const bool nlz = unit && lm != 0 && ((__ballot(need_last) >> ll) & 1ull);
  uint32_t mn = 0xFFFFFFFFu, mx = 0;
  uint64_t mysl = 0;      // length of the (common) suffix: distance to the word's terminator
  if (nf || nlz) {
    if (nf) mn = slot_first(a, t);
    if (nlz) mx = slot_last(a, t);
    if (need_first || need_last) mysl = slot_slen(a, t);      // (equal suffixes: the same for every member; only the edge lanes store)
  }
  // segmented reductions: min towards the first lane of the unit, max towards its last lane.  Bit l of r: lanes l .. l + o
  // are one unit (lane 63's cont bit speaks of the next wave); no bit left = no unit of the wave is longer than o
  const bool do_min = __ballot(nf) != 0, do_max = __ballot(nlz) != 0;
  unsigned long long r = cm & ~(1ull << 63);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    if (!r) break;
    if (do_min) {
      const uint32_t v = __shfl_down(mn, o, 64);
      if (((r >> lane) & 1ull) && v < mn) mn = v;
    }
    if (do_max) {
      const uint32_t v = __shfl_up(mx, o, 64);
      if (lane >= o && ((r >> (lane - o)) & 1ull) && v > mx) mx = v;
    }
    r &= r >> o;
  }
  // At most one unit leaves the wave through lane 63 (its head is here and wants the minimum over ALL its members) and at
  // most one enters through lane 0 (its last member is here and wants the maximum): the members outside the wave are
  // fetched by all 64 lanes together, 64 at a time (one lane walking them was a chain of 3 dependent gathers per member,
  // hundreds of members long for the word families of a 1000-copy collection).
  const I g63 = lane_read(g, 63);
  const bool cont63 = (cm >> 63) & 1ull;
  const unsigned long long fwd = __ballot(need_first && cont63 && g63 == g);       // the head lane of the unit that goes on
  if (fwd) {
    uint32_t ext = 0xFFFFFFFFu;
    for (uint64_t m0 = wbase + 64;; m0 += 64) {
      const uint64_t m = m0 + lane;
      const bool mine = m < a.N && a.grp[m] == g63;       // (members are contiguous; a slot of the group emits)
      uint32_t f = 0xFFFFFFFFu;
      if (mine) f = slot_first(a, m);
      f = wave_min(f);
      ext = f < ext ? f : ext;
      if (__ballot(mine) != ~0ull) break;
    }
    if ((fwd >> lane) & 1ull) mn = ext < mn ? ext : mn;
  }
  const uint64_t g0 = lane_read(g, 0);
  const unsigned long long bwd = __ballot(need_last && (uint64_t)g < wbase);        // the last lane of the unit that came in
  if (bwd && (um & 1ull)) {
    uint32_t ext = 0;
    for (uint64_t m0 = g0; m0 < wbase; m0 += 64) {
      const uint64_t m = m0 + lane;
      uint32_t l = 0;
      if (m < wbase) l = slot_last(a, m);
      l = wave_max(l);
      ext = l > ext ? l : ext;
    }
    if ((bwd >> lane) & 1ull) mx = ext > mx ? ext : mx;
  }
  // ---- round trip 4 (3 was sfirst / slast / ssl): the two values, stored through the map word and prefix of round trip 2
  uint64_t v_first = 0, v_last = 0;
  if (need_first) v_first = a.bwsai[mn];
  if (need_last) v_last = a.bwsai[mx];
  if (need_first) sa_put_at(a, o_first, w_first, p_first, v_first - mysl);
  if (need_last) sa_put_at(a, o_last, w_last, p_last, v_last - mysl);
}

// Boundaries of the runs of the BWT slice [out_lo, out_hi): bit r of the map = position out_lo + r starts a run
// (differs from the byte before) or ends one (differs from the byte after); the slice's own first and last position
// always count - their neighbours belong to another rank.
__device__ __forceinline__ uint32_t pack_byte_flags(uint32_t m) {      // flags at bits 0, 8, 16, 24 -> bits 0..3
  return (m & 1u) | ((m >> 7) & 2u) | ((m >> 14) & 4u) | ((m >> 21) & 8u);
}
// one lane per 16 positions (one 16-byte load and its two shifted neighbours), four lanes make one word of the map;
// smap / emap (optional): the starts and the ends on their own, with their counts per word
__global__ __launch_bounds__(256) void run_bitmap_kernel(const uint8_t *__restrict__ bwt, uint64_t cnt, uint64_t *__restrict__ bmap,
                                                         uint32_t *__restrict__ wcnt, uint64_t *__restrict__ smap,
                                                         uint32_t *__restrict__ scnt, uint64_t *__restrict__ emap,
                                                         uint32_t *__restrict__ ecnt) {
  const uint64_t ch = (uint64_t)BID * 256 + threadIdx.x;
  const uint64_t base = ch * 16;
  uint32_t ms[4], me[4];
  run_mask16(bwt, base, cnt, -1, -1, 0, ms);
  run_mask16(bwt, base, cnt, -1, -1, 1, me);
  uint32_t bs = 0, be = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) { bs |= pack_byte_flags(ms[q]) << (4 * q); be |= pack_byte_flags(me[q]) << (4 * q); }
  uint64_t vs = (uint64_t)bs << (16 * (threadIdx.x & 3)), ve = (uint64_t)be << (16 * (threadIdx.x & 3));
  vs |= __shfl_xor(vs, 1, 64); vs |= __shfl_xor(vs, 2, 64);
  ve |= __shfl_xor(ve, 1, 64); ve |= __shfl_xor(ve, 2, 64);
  if ((threadIdx.x & 3) == 0 && base < cnt) {
    const uint64_t w = ch >> 2;
    bmap[w] = vs | ve; wcnt[w] = (uint32_t)__popcll(vs | ve);
    if (smap) { smap[w] = vs; scnt[w] = (uint32_t)__popcll(vs); }
    if (emap) { emap[w] = ve; ecnt[w] = (uint32_t)__popcll(ve); }
  }
}
__global__ void count_unset_kernel(const uint64_t *__restrict__ v, uint64_t n, unsigned long long *__restrict__ total) {
  const uint64_t i = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (i < n && v[i] == ~0ull) atomicAdd(total, 1ull);
}
// Hard groups, BWT-only and sparse-SA modes: majority fill + minority placement.  The members of a group of equal
// suffixes whose preceding chars disagree are, in a collection of similar sequences, one or a few words with most of
// the occurrences and one char (the base phrase and the variants that differ elsewhere) plus a handful of
// occurrences with another char (the variants that differ right here).  The occurrences of the majority char need no
// ranks: whatever their order, they write the same byte.  So the group's range is filled with the majority char (by
// expand_kernel, through gmaj[]) and only the minority occurrences are ranked - own index + lower_bound in every other
// member's inverted list, straight from global memory - and written over the fill.  In sparse SA mode a minority
// occurrence also gives the SA values of its two neighbours in the merged order (predecessor / successor of its
// BWT(P) position over all lists): those and the group's two ends are the only places a run can start or end.
// Groups where no char dominates and that fit the LDS kernels keep the old path (fallback list).
struct HardGroupInfo { uint64_t g; uint64_t E; uint32_t k; uint32_t minor; };
// member m (of k) of the hard group at head slot g does not carry the majority char; roff: index of its first occurrence among
// all minority occurrences (where hard_minor_kernel keeps its record for the SA round - no counter to contend for)
// base / ist / occ / sl / ch: the group's first output position and the member's own inverted list, char and suffix length, looked up
// once where the list is laid out (eight lanes per group) instead of at the head of every ranking wave's chain of dependent loads
struct MinorMember { uint64_t g; uint32_t k, m; uint64_t roff; uint64_t base; uint32_t ist, occ; uint32_t sl; uint32_t ch; };
// sparse SA: what the second pass needs of a placed minority occurrence - its output position, its BWT(P) position
// and those of its neighbours in the merged order (flags bit 0 / 1: there is a predecessor / successor), suffix length
struct MinorRec { uint64_t o; uint32_t pos, pred, succ, flags, sl, pad; };
// (One thread per group.  Eight lanes per group - members strided over the lanes, tables merged by a butterfly - was
//  tried in round 3 and ran twice as long, 10 -> 20 ms on 1024 copies: most groups have a handful of members, and the
//  chain of dependent loads that finds a group's extent is the same for eight lanes as for one.)
template <class I>
__global__ __launch_bounds__(256) void hard_classify_kernel(MergeArgsT<I> a, const I *__restrict__ heads, uint64_t nH,
                                                            uint8_t *__restrict__ gmaj, HardGroupInfo *__restrict__ info,
                                                            uint32_t *__restrict__ minor_cnt, uint8_t *__restrict__ fallback,
                                                            unsigned long long *__restrict__ chars_total, uint32_t *__restrict__ minor_members) {
  const uint64_t h = (uint64_t)BID * 256 + threadIdx.x;
  unsigned long long mychars = 0, myk = 0;
  if (h < nH) {
  const uint64_t g = heads[h];
  // members are the slots g .. g+k-1 (grp == g): gallop, then bisect
  uint64_t lo = 1, hi = 2;                   // offset lo is inside (a hard group has two members), hi will be outside
  while (g + hi < a.N && a.grp[g + hi] == (I)g) { lo = hi; hi *= 2; }
  if (g + hi > a.N) hi = a.N - g;            // slot N counts as outside
  while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.grp[g + mid] == (I)g) lo = mid; else hi = mid; }
  const uint64_t k = hi;                     // first offset outside = number of members
  const uint64_t base = slot_off(a, g);
  const uint64_t E = slot_off(a, g + k) - base;
  // occurrences per distinct char (up to 4 kept; more distinct chars: fallback)
  uint32_t c0 = 0x100, c1 = 0x100, c2 = 0x100, c3 = 0x100;
  uint64_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
  bool many = false;
  uint64_t prev = base;
  for (uint64_t m = 0; m < k; m++) {
    const uint64_t nxt = slot_off(a, g + m + 1);
    const uint64_t occ = nxt - prev;
    prev = nxt;
    const uint32_t c = fix_char(a.pc[g + m]);
    if (c == c0 || c0 == 0x100) { c0 = c; n0 += occ; }
    else if (c == c1 || c1 == 0x100) { c1 = c; n1 += occ; }
    else if (c == c2 || c2 == 0x100) { c2 = c; n2 += occ; }
    else if (c == c3 || c3 == 0x100) { c3 = c; n3 += occ; }
    else many = true;
  }
  uint32_t mc = c0; uint64_t mnn = n0;
  if (n1 > mnn) { mc = c1; mnn = n1; }
  if (n2 > mnn) { mc = c2; mnn = n2; }
  if (n3 > mnn) { mc = c3; mnn = n3; }
  const uint64_t minor = E - mnn;
  uint32_t mm = 0;                               // members that do not carry the majority char, and the longest of their lists
  uint64_t mm_max = 0;
  prev = base;
  for (uint64_t m = 0; m < k; m++) {
    const uint64_t nxt = slot_off(a, g + m + 1);
    if ((uint32_t)fix_char(a.pc[g + m]) != mc) { mm++; mm_max = nxt - prev > mm_max ? nxt - prev : mm_max; }
    prev = nxt;
  }
  // fallback (the kernels that rank every occurrence): no dominating char, a long minority list (its occurrences
  // would be ranked one after the other), too many distinct chars
  // ... or a minority that is cheap per occurrence but meets too many members: every minority occurrence is ranked against every
  // member of the group (hard_minor_kernel: minor x k list checks), which is nothing for a phrase and its variants and quadratic
  // for the words of a satellite array - 17 K near-identical monomers, 2 % of them with another preceding char: 0.02 k^2 = 6 M
  // checks per group where ranking all k occurrences by sorting costs k log k (round 4, the c2r workload: 200 ms -> 3 ms)
  const bool fb = many || minor * 4 > E || mm_max > 1024 || minor * k > 16 * E + 4096;
  const bool in_slice = !(base + E <= a.out_lo || base >= a.out_hi);
  fallback[h] = (fb && in_slice) ? 1 : 0;
  gmaj[g] = fb ? 0 : (uint8_t)mc;
  minor_cnt[h] = (fb || !in_slice) ? 0u : (uint32_t)minor;
  minor_members[h] = (fb || !in_slice) ? 0u : mm;
  info[h] = HardGroupInfo{g, E, (uint32_t)k, (uint32_t)(fb ? 0 : minor)};
  if (!fb && in_slice) { mychars = E; myk = k; }
  }
  for (int o = 32; o > 0; o >>= 1) { mychars += __shfl_down(mychars, o, 64); myk += __shfl_down(myk, o, 64); }      // "Hard bwt chars" (pfbwt.cpp:231-233) of these groups
  if ((threadIdx.x & 63) == 0 && mychars) { atomicAdd(chars_total, mychars); atomicAdd(chars_total + 1, myk); }      // [1]: members, for the lane choice of hard_minor_kernel
}

// the minority members of all groups, laid end to end (offsets = prefix sums of their count per group); eight lanes per
// group, eight members per step, order and record offsets from prefix sums over the lanes
template <class I>
__global__ __launch_bounds__(256) void hard_minor_fill_kernel(MergeArgsT<I> a, const HardGroupInfo *__restrict__ info, uint64_t nH,
                                                              const uint64_t *__restrict__ mm_off, const uint64_t *__restrict__ minor_off,
                                                              const uint8_t *__restrict__ gmaj, MinorMember *__restrict__ out) {
  const uint64_t tq = (uint64_t)BID * 256 + threadIdx.x;
  const uint64_t h = tq >> 3;
  const int l8 = (int)(tq & 7);
  if (h >= nH) return;
  uint64_t o = mm_off[h];
  if (mm_off[h + 1] == o) return;
  const HardGroupInfo gi = info[h];
  const uint32_t maj = gmaj[gi.g];
  uint64_t r = minor_off[h];
  const uint64_t gbase = slot_off(a, gi.g);
  for (uint32_t m0 = 0; m0 < gi.k; m0 += 8) {
    const uint32_t m = m0 + (uint32_t)l8;
    const bool is_minor = m < gi.k && (uint32_t)fix_char(a.pc[gi.g + m]) != maj;
    uint32_t cnt = is_minor ? 1u : 0u;
    uint64_t oc = is_minor ? slot_off(a, gi.g + m + 1) - slot_off(a, gi.g + m) : 0ull;
    const uint32_t own_c = cnt; const uint64_t own_o = oc;
#pragma unroll
    for (int d2 = 1; d2 < 8; d2 <<= 1) {
      const uint32_t vc = __shfl_up(cnt, d2, 8); const uint64_t vo = __shfl_up(oc, d2, 8);
      if (l8 >= d2) { cnt += vc; oc += vo; }
    }
    if (is_minor) {
      const uint64_t myi = a.sa[gi.g + m];
      const WordRec wr = a.wrec[word_of(a.wv, myi)];
      out[o + cnt - own_c] = MinorMember{gi.g, gi.k, m, r + oc - own_o, gbase, wr.ist, wr.occ, (uint32_t)(wr.wend - myi),
                                         (uint32_t)fix_char(a.pc[gi.g + m])};
    }
    o += __shfl(cnt, 7, 8); r += __shfl(oc, 7, 8);
  }
}
// LPM lanes per minority member (8, or the whole wave where groups have many members - the word families of a
// collection of hundreds of copies): its occurrences (usually one) are ranked one after the other - own index +
// lower_bound in every other member's inverted list, the group's members shared among the lanes - rank, predecessor
// and successor combined by shuffles.  What a member's list looks like from outside (smallest / largest position,
// length) comes from the per-slot arrays, LPM consecutive slots per load.
template <class I, int LPM>
__global__ __launch_bounds__(256) void hard_minor_kernel(MergeArgsT<I> a, const MinorMember *__restrict__ mem, uint64_t total,
                                                         MinorRec *__restrict__ recs) {
  constexpr int PER = 256 / LPM;             // members per workgroup and round
  const int ll = threadIdx.x & (LPM - 1);
  const uint64_t rounds = (total + GDIM * PER - 1) / (GDIM * PER);      // every lane runs the same number of rounds (shuffles inside)
  for (uint64_t it = 0; it < rounds; it++) {
    const uint64_t q = (it * GDIM + BID) * PER + (threadIdx.x / LPM);
    const bool live = q < total;
    MinorMember mmv{0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (live) mmv = mem[q];
    const uint64_t g = mmv.g;
    const uint32_t k = mmv.k, me = mmv.m;
    const uint32_t my_occ = mmv.occ, my_ist = mmv.ist;
    const uint64_t base = mmv.base, sl = mmv.sl;          // (equal suffixes: the same length for every member)
    const uint8_t mych = (uint8_t)mmv.ch;
    // longest occurrence count among the members of the wave decides the trip count (shuffles inside the loop)
    uint32_t trips = my_occ;
#pragma unroll
    for (int o = LPM; o < 64; o <<= 1) { const uint32_t v = __shfl_xor(trips, o, 64); trips = v > trips ? v : trips; }
    for (uint32_t j = 0; j < trips; j++) {
      const bool act = live && j < my_occ;
      uint64_t r = 0;
      uint32_t pos = 0, pred = 0, succ = 0xFFFFFFFFu, has_pred = 0, has_succ = 0;
      if (act) {
        pos = a.ilist[my_ist + j];
        for (uint32_t m = (uint32_t)ll; m < k; m += LPM) {
          uint32_t lb, pv = 0, sv = 0;
          bool hp = false, hs = false;
          if (m == me) {
            lb = j;
            if (a.want_sa) {
              if (j > 0) { pv = a.ilist[my_ist + j - 1]; hp = true; }
              if (j + 1 < my_occ) { sv = a.ilist[my_ist + j + 1]; hs = true; }
            }
          } else {
            // a list that lies wholly on one side of pos (a variant that occurs once: always) needs no look inside;
            // only a list that straddles pos is looked up and bisected
            const uint32_t mfirst = slot_first(a, g + m), mlast = slot_last(a, g + m);
            if (pos < mfirst) { lb = 0; sv = mfirst; hs = true; }
            else if (pos > mlast) { lb = (uint32_t)(slot_off(a, g + m + 1) - slot_off(a, g + m)); pv = mlast; hp = true; }
            else {
              const WordRec wr = a.wrec[word_of(a.wv, a.sa[g + m])];
              const uint32_t *lst = a.ilist + wr.ist;
              uint32_t l2 = 1, h2 = wr.occ - 1;          // # entries < pos: lst[0] < pos < lst[occ - 1]
              while (l2 < h2) { const uint32_t mid = (l2 + h2) >> 1; if (lst[mid] < pos) l2 = mid + 1; else h2 = mid; }
              lb = l2;
              if (a.want_sa) { pv = lst[lb - 1]; hp = true; sv = lst[lb]; hs = true; }
            }
          }
          r += lb;
          if (hp && (!has_pred || pv > pred)) { pred = pv; has_pred = 1; }
          if (hs && (!has_succ || sv < succ)) { succ = sv; has_succ = 1; }
        }
      }
#pragma unroll
      for (int o = 1; o < LPM; o <<= 1) {
        r += __shfl_xor(r, o, 64);
        const uint32_t op = __shfl_xor(pred, o, 64), ohp = __shfl_xor(has_pred, o, 64);
        const uint32_t os = __shfl_xor(succ, o, 64), ohs = __shfl_xor(has_succ, o, 64);
        if (ohp && (!has_pred || op > pred)) { pred = op; has_pred = 1; }
        if (ohs && (!has_succ || os < succ)) { succ = os; has_succ = 1; }
      }
      if (!act || ll != 0) continue;
      const uint64_t o = base + r;
      if (o >= a.out_lo && o < a.out_hi) a.bwt[o] = mych;
      if (a.want_sa)       // (also when the occurrence lies just outside this rank's slice: its neighbours may be inside)
        recs[mmv.roff + j] = MinorRec{o, pos, pred, succ, has_pred | (has_succ << 1), (uint32_t)sl, 0u};
    }
  }
}

template <class I>
__global__ void hard_minor_sa_kernel(MergeArgsT<I> a, const MinorRec *__restrict__ recs, uint64_t n) {
  const uint64_t q = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const MinorRec r = recs[q];
  sa_put(a, r.o, a.bwsai[r.pos] - (uint64_t)r.sl);
  if ((r.flags & 1u) && r.o >= 1) sa_put(a, r.o - 1, a.bwsai[r.pred] - (uint64_t)r.sl);
  if (r.flags & 2u) sa_put(a, r.o + 1, a.bwsai[r.succ] - (uint64_t)r.sl);
}

// Hard groups.  hard[] is 1 exactly at the head slot of every hard group; the heads are compacted
// into a list and every wave takes 64 of them at a time, one per lane.  A single group is a chain
// of dependent loads (members, offsets, inverted-list starts, positions), so the work of a batch
// is laid out flat and every phase runs with all lanes busy on independent loads:
//   A  lane = group      : member count, output base, number of occurrences E
//   B  lane = member     : offset of its occurrences, inverted-list start, char, suffix length
//   C  lane = occurrence : its BWT(P) position from the inverted list  -> LDS
//   D  lane = occurrence : rank among the E positions of its own group -> output slot
// Every occurrence (member, j) must land at the rank of its BWT(P) position among all occurrences
// of the group - the reference pops a heap (pfbwt.cpp:537-556).  Ranking is all-pairs over the
// group's LDS segment, or, when the group is a few long sorted lists, own index + lower_bound in
// each other member's segment.  Groups that do not fit the LDS tables are queued for
// hard_big_kernel.  (One group at a time per wave took 7.7 us per group, 22 ms at 8.8 M groups.)
// (head: the index of the group's head in the list - soff[head] is where its ranked occurrences are staged for the SA round's
//  replay: an exclusive sum of E over the list, which does not depend on the order in which the waves' atomics fill the queues.
//  32 bits: a list of 2^32 heads or more is not replayed)
struct BigGroup { uint64_t g; uint64_t E; uint32_t k; uint32_t head; };
// What phase A of hard_groups_kernel wants of a fallback group - head slot, first output position, occurrences, members -
// as hard_classify_kernel found it (one 32-byte record next to fb_heads[], same order).  The classifier counts the members
// by grp alone (gallop and bisection over grp[g + x] == g), phase A's own walk by grp and pc != 0; for the head of a hard group
// the two agree: pc[t] == 0 says that slot t's suffix is no longer than w (or lies past the last word) and emits nothing
// (pprec16_kernel, posrec_at), the members of a group are equal strings up to and including the terminator, hence equally
// long, and a head is flagged only by a member with pc != 0 (slot_records_kernel, group_flags_kernel) - so every member of a
// flagged group has pc != 0 and the walk ends where grp changes, or at slot N, as the classifier does.  Neither E nor base
// depends on anything but k and the offsets.  PFP_DEBUG=1 checks it on every record (fb_records_check_kernel).
struct alignas(16) FallbackRec { uint64_t g, base, E; uint32_t k, pad; };
template <class I>
__global__ void fb_records_kernel(MergeArgsT<I> a, uint64_t n, const I *__restrict__ fidx, const HardGroupInfo *__restrict__ info,
                                  I *__restrict__ fb_heads, FallbackRec *__restrict__ recs, uint64_t *__restrict__ fb_E /* sparse SA, else null */) {
  const uint64_t i = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const HardGroupInfo gi = info[fidx[i]];
  fb_heads[i] = (I)gi.g;
  recs[i] = FallbackRec{gi.g, slot_off(a, gi.g), gi.E, gi.k, 0u};
  if (fb_E) fb_E[i] = gi.E;      // summed to the groups' staging offsets (MergeArgsT::soff)
}
template <class I>
__global__ void fb_records_check_kernel(MergeArgsT<I> a, uint64_t n, const FallbackRec *__restrict__ recs,
                                        unsigned long long *__restrict__ bad) {
  const uint64_t i = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const FallbackRec r = recs[i];
  uint64_t kk = 0;
  while (r.g + kk < a.N && a.grp[r.g + kk] == (I)r.g && a.pc[r.g + kk] != 0) kk++;
  if (kk != r.k || slot_off(a, r.g) != r.base || slot_off(a, r.g + kk) - r.base != r.E) atomicAdd(bad, 1ull);
}
struct HardLds {
  uint32_t lpos[kHardRank];
  uint8_t lq[kHardRank];
  uint32_t lmoff[kHardMem + 1], lmist[kHardMem], lmsl[kHardMem];
  uint8_t lmch[kHardMem], lmg[kHardMem];
  uint64_t gbase[64], ghead[64], gsoff[64];      // gsoff: the group's staging offset (sparse SA with replay)
  uint16_t geoff[65], gk0[65];                   // (<= kHardRank, <= kHardMem: 16 bits, so that gsoff[] leaves five workgroups on a CU)
};
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const uint32_t x = __shfl_xor(v, o, 64); v = x > v ? x : v; }
  return v;
}
// kReplay (sparse SA, second round): phase A as ever, then no tables and no ranking - entry soff + r of a group that the
// BWT round ranked here is the occurrence at output position base + r (sa_replay); S[] is not touched
template <class I, bool kReplay>
__global__ __launch_bounds__(256) void hard_groups_kernel(MergeArgsT<I> a, const I *__restrict__ heads,
                                                          const FallbackRec *__restrict__ recs /* null: phase A walks */,
                                                          const uint64_t *__restrict__ nheads_p,
                                                          unsigned long long *__restrict__ stats /* null: SA round, the queues stand */,
                                                          BigGroup *__restrict__ big, uint32_t big_cap,
                                                          BigGroup *__restrict__ mid, uint32_t mid_cap, int gpb,
                                                          unsigned long long *__restrict__ unwritten /* replay with PFP_DEBUG, else null */) {
  __shared__ HardLds S[4];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  HardLds &L = S[wv];
  const uint64_t nH = *nheads_p;
  // gpb groups per wave and batch: 64 when there are groups enough to keep every wave of the chip busy, fewer
  // otherwise - a batch is one long chain of dependent phases, so the chip wants many of them in flight
  const uint64_t nbatch = (nH + gpb - 1) / gpb;
  unsigned long long my_chars = 0, my_groups = 0;
  for (uint64_t b = BID * 4 + wv; b < nbatch; b += GDIM * 4) {
    // ---- A: one group per lane
    const uint64_t hidx = b * gpb + lane;
    uint64_t g = 0, base = 0, so = 0;
    uint32_t k = 0, E = 0;
    bool live = false;
    if (lane < gpb && hidx < nH) {
      uint32_t kk = 0;
      uint64_t Eg;
      if (a.ranked) so = a.soff[hidx];
      if (recs) {      // the classifier's record: one load (FallbackRec has the proof that it is what the walk finds)
        const FallbackRec r = recs[hidx];
        g = r.g; kk = r.k; base = r.base; Eg = r.E;
      } else {         // dense SA, every head unclassified: walk the members
        g = heads[hidx];
        while (g + kk < a.N && a.grp[g + kk] == (I)g && a.pc[g + kk] != 0) kk++;
        base = slot_off(a, g);
        Eg = slot_off(a, g + kk) - base;
      }
      if (kk && !(base + Eg <= a.out_lo || base >= a.out_hi)) {      // inside this rank's slice
        my_chars += Eg; my_groups += 1;
        const bool sorted_path = Eg > (uint64_t)kHardSortMin;
        if (Eg <= (uint64_t)kHardRank && kk <= (uint32_t)kHardMem && !sorted_path) { live = true; k = kk; E = (uint32_t)Eg; }
        else if (stats && Eg <= (uint64_t)kHardLds && sorted_path) {      // one wave sorts it in LDS: hard_sort_kernel
          const unsigned long long idx = atomicAdd(&stats[3], 1ull);
          if (idx < mid_cap) mid[idx] = BigGroup{g, Eg, kk, (uint32_t)hidx};
        } else if (stats) {     // too large for the LDS tables: hard_big_kernel (whole grid, one thread per occurrence)
          const unsigned long long idx = atomicAdd(&stats[2], 1ull);
          if (idx < big_cap) big[idx] = BigGroup{g, Eg, kk, (uint32_t)hidx};
        }
      }
    }
    if constexpr (kReplay) {
      // the batch's ranked occurrences flat over the lanes: which group holds occurrence e, by bisection over the lanes'
      // running sums of E (six shuffles; every lane takes part in each)
      uint32_t pE = live ? E : 0u;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const uint32_t vE = __shfl_up(pE, o, 64); if (lane >= o) pE += vE; }
      const uint32_t Eb = __shfl(pE, 63, 64);
      for (uint32_t e0 = 0; e0 < Eb; e0 += 64) {
        const uint32_t e = e0 + lane;
        int lo = 0, hi = 63;                         // the first lane whose sum exceeds e lies in [lo, hi] (e < Eb)
#pragma unroll
        for (int s = 0; s < 6; s++) {
          const int mdl = (lo + hi) >> 1;
          if (__shfl(pE, mdl, 64) > e) hi = mdl; else lo = mdl + 1;
        }
        lo &= 63;                                    // (e >= Eb: any lane, nothing is done)
        const uint32_t r = e - (__shfl(pE, lo, 64) - __shfl(E, lo, 64));
        const uint64_t gb = __shfl(base, lo, 64), gs = __shfl(so, lo, 64);
        if (e < Eb) sa_replay(a, gs + r, gb + r, unwritten);
      }
      continue;
    }
    unsigned long long todo = __ballot(live);
    while (todo) {
      // the longest prefix of the remaining groups whose members and occurrences fit the tables
      const bool mine = (todo >> lane) & 1ull;
      uint32_t pk = mine ? k : 0u, pE = mine ? E : 0u;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t vk = __shfl_up(pk, o, 64), vE = __shfl_up(pE, o, 64);
        if (lane >= o) { pk += vk; pE += vE; }
      }
      const bool fit = mine && pk <= (uint32_t)kHardMem && pE <= (uint32_t)kHardRank;
      const unsigned long long take = __ballot(fit);       // never empty: a single live group fits
      todo &= ~take;
      const int nG = __popcll(take);
      const int lastl = 63 - __clzll((long long)take);
      const uint32_t M = __shfl(pk, lastl, 64), Eb = __shfl(pE, lastl, 64);
      if (fit) {
        const int gi = __popcll(take & ((1ull << lane) - 1ull));
        L.ghead[gi] = g; L.gbase[gi] = base; L.gsoff[gi] = so; L.geoff[gi] = (uint16_t)(pE - E); L.gk0[gi] = (uint16_t)(pk - k);
      }
      if (lane == 0) { L.geoff[nG] = (uint16_t)Eb; L.gk0[nG] = (uint16_t)M; }
      wave_lds_sync();
      // ---- B: one member per lane
      for (uint32_t q = lane; q < M; q += 64) {
        int lo = 0, hi = nG;                       // gk0[lo] <= q < gk0[hi]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (L.gk0[mid] <= q) lo = mid; else hi = mid; }
        const uint64_t t = L.ghead[lo] + (q - L.gk0[lo]);
        L.lmoff[q] = L.geoff[lo] + (uint32_t)(slot_off(a, t) - L.gbase[lo]);
        L.lmist[q] = slot_ist(a, t);
        uint32_t sl = 0;
        if (a.want_sa) sl = (uint32_t)slot_slen(a, t);
        L.lmsl[q] = sl;
        L.lmch[q] = fix_char(a.pc[t]);
        L.lmg[q] = (uint8_t)lo;
      }
      if (lane == 0) L.lmoff[M] = Eb;
      wave_lds_sync();
      // ---- C: one occurrence per lane, independent inverted-list gathers
      for (uint32_t e = lane; e < Eb; e += 64) {
        uint32_t lo = 0, hi = M;                   // lmoff[lo] <= e < lmoff[hi]
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (L.lmoff[mid] <= e) lo = mid; else hi = mid; }
        L.lpos[e] = a.ilist[L.lmist[lo] + (e - L.lmoff[lo])];
        L.lq[e] = (uint8_t)lo;
      }
      wave_lds_sync();
      // ---- D: rank inside the own group's segment
      for (uint32_t e = lane; e < Eb; e += 64) {
        const uint32_t q = L.lq[e], gi = L.lmg[q];
        const uint32_t s0 = L.geoff[gi], s1 = L.geoff[gi + 1], k0 = L.gk0[gi], k1 = L.gk0[gi + 1];
        const uint32_t Eg = s1 - s0, kg = k1 - k0;
        const uint32_t pos = L.lpos[e];
        uint32_t lg = 1;
        while ((kg << lg) < Eg) lg++;
        const bool by_search = (uint64_t)kg * (lg + 1) * 3 < Eg;
        uint32_t r = 0;
        if (!by_search) {
          for (uint32_t x = s0; x < s1; x++) r += L.lpos[x] < pos;
        } else {
          for (uint32_t m2 = k0; m2 < k1; m2++) {
            uint32_t l2 = L.lmoff[m2], h2 = L.lmoff[m2 + 1];       // # entries < pos in member m2's segment
            const uint32_t b2 = l2;
            while (l2 < h2) { const uint32_t mid = (l2 + h2) >> 1; if (L.lpos[mid] < pos) l2 = mid + 1; else h2 = mid; }
            r += l2 - b2;
          }
        }
        const uint64_t o = L.gbase[gi] + r;
        if (o >= a.out_lo && o < a.out_hi) {
          if (a.pass & PASS_BWT) a.bwt[o] = L.lmch[q];
          if (a.ranked) a.ranked[L.gsoff[gi] + r] = RankedOcc{pos, L.lmsl[q]};
          if (a.want_sa && (a.pass & PASS_SA) && sa_wanted(a, o)) sa_put(a, o, a.bwsai[pos] - (uint64_t)L.lmsl[q]);
        }
      }
      wave_lds_sync();
    }
  }
  // statistics (pfbwt.cpp:231-233 "Hard bwt chars")
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { my_chars += __shfl_down(my_chars, o, 64); my_groups += __shfl_down(my_groups, o, 64); }
  if (stats && lane == 0 && (my_chars | my_groups)) { atomicAdd(&stats[0], my_chars); atomicAdd(&stats[1], my_groups); }
}

// Groups of 513..1024 occurrences (a word family of a collection of hundreds of copies): ranking every
// occurrence against all others costs E^2 LDS reads; one wave sorts the group's positions with a bitonic
// network instead (E log^2 E / 2 exchanges; 12.6 GB / 1024 copies: 374 -> ~250 ms).  Kept out of
// hard_groups_kernel so that its 10 KB of sort buffers per wave do not halve that kernel's occupancy
// (they did: 11 -> 20 ms on the 64-copy workload).  The member search is by position here (a member table
// would not fit for k > 256): every occurrence finds its member by bisection over the slots' offsets.
template <class I>
__global__ __launch_bounds__(256) void hard_sort_kernel(MergeArgsT<I> a, const BigGroup *__restrict__ mid, uint32_t nmid) {
  __shared__ uint64_t skey[4][kHardLds];       // (position << 16 | occurrence index)
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint64_t *K = skey[wv];
  for (uint32_t qi = BID * 4 + wv; qi < nmid; qi += GDIM * 4) {
    const uint64_t g = mid[qi].g;
    const uint32_t E = (uint32_t)mid[qi].E, k = mid[qi].k;
    const uint64_t base = slot_off(a, g);
    uint32_t n = 64;
    while (n < E) n <<= 1;
    for (uint32_t e = lane; e < n; e += 64) {
      uint64_t key = ~0ull;
      if (e < E) {
        uint32_t lo = 0, hi = k;                 // member holding occurrence e: off[g+lo] - base <= e
        while (hi - lo > 1) { const uint32_t mdl = (lo + hi) >> 1; if (slot_off(a, g + mdl) - base <= e) lo = mdl; else hi = mdl; }
        const uint32_t pos = a.ilist[slot_ist(a, g + lo) + (e - (uint32_t)(slot_off(a, g + lo) - base))];
        key = ((uint64_t)pos << 16) | e;
      }
      K[e] = key;
    }
    wave_lds_sync();
    for (uint32_t k2 = 2; k2 <= n; k2 <<= 1)
      for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
        for (uint32_t i = lane; i < (n >> 1); i += 64) {
          const uint32_t x = ((i & ~(j - 1)) << 1) | (i & (j - 1)), y = x | j;
          const uint64_t kx = K[x], ky = K[y];
          if ((kx > ky) == ((x & k2) == 0)) { K[x] = ky; K[y] = kx; }
        }
        wave_lds_sync();
      }
    for (uint32_t r = lane; r < E; r += 64) {
      const uint64_t key = K[r];
      const uint32_t pos = (uint32_t)(key >> 16), e = (uint32_t)(key & 0xffffu);
      const uint64_t o = base + r;
      if (o < a.out_lo || o >= a.out_hi) continue;
      uint32_t lo = 0, hi = k;
      while (hi - lo > 1) { const uint32_t mdl = (lo + hi) >> 1; if (slot_off(a, g + mdl) - base <= e) lo = mdl; else hi = mdl; }
      const uint64_t t = g + lo;
      if (a.pass & PASS_BWT) a.bwt[o] = fix_char(a.pc[t]);
      if (a.ranked) a.ranked[a.soff[mid[qi].head] + r] = RankedOcc{pos, (uint32_t)slot_slen(a, t)};
      if (a.want_sa && (a.pass & PASS_SA) && sa_wanted(a, o)) sa_put(a, o, a.bwsai[pos] - slot_slen(a, t));
    }
    wave_lds_sync();
  }
}

// large hard groups: one thread per occurrence, rank = own index + lower_bound in every other
// member's inverted list
template <class I>
__global__ __launch_bounds__(256) void hard_big_kernel(MergeArgsT<I> a, const BigGroup *__restrict__ big, uint32_t nbig,
                                                       const uint64_t *__restrict__ estart, uint64_t total) {
  const uint64_t e0 = estart[0];              // (the queue's offsets are absolute: this launch may start in its middle)
  for (uint64_t gi = (uint64_t)BID * 256 + threadIdx.x; gi < total; gi += (uint64_t)GDIM * 256) {
    const uint64_t ge = e0 + gi;
    uint32_t lo = 0, hi = nbig;               // estart[lo] <= ge < estart[hi]
    while (hi - lo > 1) { uint32_t mid = (lo + hi) >> 1; if (estart[mid] <= ge) lo = mid; else hi = mid; }
    const uint64_t g = big[lo].g, e = ge - estart[lo];
    const uint32_t k = big[lo].k;
    const uint64_t base = slot_off(a, g);
    uint32_t ml = 0, mh = k;                  // member holding occurrence e
    while (mh - ml > 1) { uint32_t mid = (ml + mh) >> 1; if (slot_off(a, g + mid) - base <= e) ml = mid; else mh = mid; }
    const uint64_t t = g + ml;
    const uint32_t j = (uint32_t)(e - (slot_off(a, t) - base));
    const uint32_t pos = a.ilist[slot_ist(a, t) + j];
    uint64_t r = j;
    for (uint64_t t2 = g; t2 < g + k; t2++) {
      if (t2 == t) continue;
      const uint32_t *lst = a.ilist + slot_ist(a, t2);
      uint32_t l2 = 0, h2 = (uint32_t)(slot_off(a, t2 + 1) - slot_off(a, t2));      // # entries < pos
      while (l2 < h2) { uint32_t mid = (l2 + h2) >> 1; if (lst[mid] < pos) l2 = mid + 1; else h2 = mid; }
      r += l2;
    }
    if (base + r >= a.out_lo && base + r < a.out_hi) {
      if (a.pass & PASS_BWT) a.bwt[base + r] = fix_char(a.pc[t]);
      if (a.ranked) a.ranked[a.soff[big[lo].head] + r] = RankedOcc{pos, (uint32_t)slot_slen(a, t)};
      if (a.want_sa && (a.pass & PASS_SA) && sa_wanted(a, base + r)) sa_put(a, base + r, a.bwsai[pos] - slot_slen(a, t));
    }
  }
}

// Large hard groups, the usual way: the occurrences of a chunk of queued groups become keys (group, BWT(P) position)
// with the member's slot as value, one device-wide radix sort merges every group's lists at once (the reference pops a
// heap, pfbwt.cpp:537-556), and position i of a group's sorted range is its i-th output.  Ranking every occurrence
// against every member's list (hard_big_kernel) is E k log(E / k) dependent loads; on 1024 copies of a genome with
// repeats - k words of ~1000 occurrences each - that was the longest kernel of the chain.
template <class I>
__global__ __launch_bounds__(256) void big_keys_kernel(MergeArgsT<I> a, const BigGroup *__restrict__ big, uint32_t q0, uint32_t q1,
                                                       const uint64_t *__restrict__ estart, uint64_t cnt,
                                                       uint64_t *__restrict__ keys, uint64_t *__restrict__ vals) {
  const uint64_t i = (uint64_t)BID * 256 + threadIdx.x;
  if (i >= cnt) return;
  const uint64_t ge = estart[q0] + i;
  uint32_t lo = q0, hi = q1;                // estart[lo] <= ge < estart[hi]
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (estart[mid] <= ge) lo = mid; else hi = mid; }
  const uint64_t g = big[lo].g, e = ge - estart[lo];
  const uint32_t k = big[lo].k;
  const uint64_t base = slot_off(a, g);
  uint32_t ml = 0, mh = k;                  // member holding occurrence e
  while (mh - ml > 1) { const uint32_t mid = (ml + mh) >> 1; if (slot_off(a, g + mid) - base <= e) ml = mid; else mh = mid; }
  const uint64_t t = g + ml;
  const uint32_t j = (uint32_t)(e - (slot_off(a, t) - base));
  keys[i] = ((uint64_t)(lo - q0) << 32) | a.ilist[slot_ist(a, t) + j];
  vals[i] = t;
}
template <class I>
__global__ __launch_bounds__(256) void big_place_kernel(MergeArgsT<I> a, const BigGroup *__restrict__ big, uint32_t q0,
                                                        const uint64_t *__restrict__ estart, uint64_t cnt,
                                                        const uint64_t *__restrict__ keys, const uint64_t *__restrict__ vals) {
  const uint64_t i = (uint64_t)BID * 256 + threadIdx.x;
  if (i >= cnt) return;
  const uint64_t key = keys[i], t = vals[i];
  const uint32_t lo = q0 + (uint32_t)(key >> 32), pos = (uint32_t)key;
  const uint64_t r = estart[q0] + i - estart[lo], o = slot_off(a, big[lo].g) + r;
  if (o < a.out_lo || o >= a.out_hi) return;
  if (a.pass & PASS_BWT) a.bwt[o] = fix_char(a.pc[t]);
  if (a.ranked) a.ranked[a.soff[big[lo].head] + r] = RankedOcc{pos, (uint32_t)slot_slen(a, t)};
  if (a.want_sa && (a.pass & PASS_SA) && sa_wanted(a, o)) sa_put(a, o, a.bwsai[pos] - slot_slen(a, t));
}

// Sparse SA, second round, the queued groups: nothing is ranked or sorted again - hard_sort_kernel, big_place_kernel and
// hard_big_kernel staged every occurrence at its rank.  The mid queue has no estart[] and groups of 513 .. 1024 occurrences:
// one wave per group; the big queue one lane per occurrence over estart[] (absolute from the queue's start), as
// big_keys_kernel walks it.
template <class I>
__global__ __launch_bounds__(256) void hard_replay_kernel(MergeArgsT<I> a, const BigGroup *__restrict__ mid, uint32_t nmid,
                                                          const BigGroup *__restrict__ big, uint32_t nbig,
                                                          const uint64_t *__restrict__ estart, uint64_t total,
                                                          unsigned long long *__restrict__ unwritten /* PFP_DEBUG, else null */) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint64_t qi = BID * 4 + wv; qi < nmid; qi += GDIM * 4) {
    const BigGroup q = mid[qi];
    const uint64_t base = slot_off(a, q.g), so = a.soff[q.head];
    for (uint32_t r = lane; r < (uint32_t)q.E; r += 64) sa_replay(a, so + r, base + r, unwritten);
  }
  for (uint64_t ge = BID * 256 + threadIdx.x; ge < total; ge += GDIM * 256) {
    uint32_t lo = 0, hi = nbig;               // estart[lo] <= ge < estart[hi]
    while (hi - lo > 1) { const uint32_t mdl = (lo + hi) >> 1; if (estart[mdl] <= ge) lo = mdl; else hi = mdl; }
    const uint64_t r = ge - estart[lo];
    sa_replay(a, a.soff[big[lo].head] + r, slot_off(a, big[lo].g) + r, unwritten);
  }
}

// loc[t] = sum of cnt over the slots of t's tile before t; tsum[tile] = the tile's total.  256 threads x 8 slots.
__global__ __launch_bounds__(256) void slot_loc_kernel(const uint32_t *__restrict__ cnt, uint64_t N, uint32_t *__restrict__ loc,
                                                       uint64_t *__restrict__ tsum, uint32_t *__restrict__ overflow) {
  __shared__ uint64_t ws[4];
  if (((uint64_t)BID << kOffTileLog) > N) return;      // tiles 0 .. N >> 11 exist (a workgroup of the padded last grid row)
  const uint64_t t0 = ((uint64_t)BID << kOffTileLog) + (uint64_t)threadIdx.x * 8;
  uint32_t v[8];
  if (t0 + 8 <= N) {
    const uint4 x = *reinterpret_cast<const uint4 *>(cnt + t0), y = *reinterpret_cast<const uint4 *>(cnt + t0 + 4);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
  } else {
    for (int k = 0; k < 8; k++) v[k] = t0 + k < N ? cnt[t0 + k] : 0u;
  }
  uint64_t own = 0;
  for (int k = 0; k < 8; k++) own += v[k];
  uint64_t inc = own;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) { const uint64_t u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  uint64_t run = inc - own;
  for (int q = 0; q < wv; q++) run += ws[q];
  uint32_t o8[8];
  for (int k = 0; k < 8; k++) { o8[k] = (uint32_t)run; run += v[k]; }
  *reinterpret_cast<uint4 *>(loc + t0) = make_uint4(o8[0], o8[1], o8[2], o8[3]);
  *reinterpret_cast<uint4 *>(loc + t0 + 4) = make_uint4(o8[4], o8[5], o8[6], o8[7]);
  if (threadIdx.x == 255) {
    tsum[BID] = run;
    if (run >> 32) atomicOr(overflow, 1u);      // a tile's offsets would not fit 32 bits
  }
}

// ------------------------------------------------------------------ stage 3: the host side

// where a slot's record (occurrences, preceding char, first / last BWT(P) position, suffix length) comes from
enum class RecordSource {
  SortKeys,      // the sorter carried it in the spare bits of its first-round keys: already at the slot
  Gathered,      // one 16-byte record per dictionary position, written by a streaming pass, gathered once per slot
  PerSlot,       // every slot computes its record from the dictionary line and its word's entry
};

// the test switches of a call.  Read per call: the tests switch them inside one process
struct MergeSwitches {
  int prec_direct = -1;                  // PFP_PREC_DIRECT: 1 / 0 forces RecordSource::PerSlot / Gathered where the sort keys carry no record
  uint32_t big_cap = 0;                  // PFP_BIG_CAP: capacity of the queue of large hard groups (0: by size)
  uint64_t big_budget = 1ull << 27;      // PFP_BIG_BUDGET: occurrences of queued groups sorted at once
  int sa_replay = -1;                    // PFP_SA_REPLAY: 1 / 0 forces the SA round of the fallback groups to replay the staged ranks / to rank again
  uint64_t replay_budget = ~0ull;        // PFP_SA_REPLAY_BUDGET: bytes the staging may take where nothing is forced (unset: an eighth of the device)
  static MergeSwitches read() {
    MergeSwitches s;
    if (const char *e = getenv("PFP_SA_REPLAY")) s.sa_replay = atoi(e) != 0;
    if (const char *e = getenv("PFP_SA_REPLAY_BUDGET")) s.replay_budget = strtoull(e, nullptr, 10);
    if (const char *e = getenv("PFP_PREC_DIRECT")) s.prec_direct = atoi(e) != 0;
    if (const char *e = getenv("PFP_BIG_CAP")) { if (atoll(e) > 0) s.big_cap = (uint32_t)atoll(e); }
    if (const char *e = getenv("PFP_BIG_BUDGET")) s.big_budget = strtoull(e, nullptr, 10);
    return s;
  }
};

// the device's memory, from the pool's soft limit (seven tenths of it)
static uint64_t device_bytes(const pfp_ctx *c) { return c->pool.soft_limit ? c->pool.soft_limit / 7 * 10 : (64ull << 30); }

template <class I>
static RecordSource choose_record_source(pfp_ctx *c, uint64_t N, uint64_t NP, int sa_mode, const SuffixOrderT<I> &so, const MergeSwitches &sw) {
  // records already sit at their slots - unless most slots were re-ordered after the first round (a
  // dictionary of near-identical variants), where fetching each such record costs more than the gather
  if (sa_mode != SA_DENSE && so.paybits == 16 && so.skeys.p && so.n_refined * 5 < N) return RecordSource::SortKeys;
  // everything else: ONE 16-byte gather per slot (slot_records_kernel); full SA output included - its per-slot inverted-list
  // start travels in the record's `first` field.
  // 16 bytes per dictionary position, written by one streaming pass and gathered once per slot - unless the slots are a
  // small share of the positions (a rank's range of the multi-GPU chain: the pass over all NP positions is replicated
  // work, 14 GB of records for a 0.9 GB dictionary) or the records would take more than an eighth of the device
  // (a 30 GB dictionary: 480 GB): then every slot computes its record itself from the dictionary line and its word's
  // entry (posrec_at: two random sectors per slot instead of one).  PFP_PREC_DIRECT=1/0 forces the choice (tests).
  bool direct = N * 4 <= NP;
  if (NP * sizeof(PosRec) > device_bytes(c) / 8) direct = true;
  if (sw.prec_direct >= 0) direct = sw.prec_direct != 0;
  return direct ? RecordSource::PerSlot : RecordSource::Gathered;
}

// which heads the LDS kernels (hard_groups_kernel) work through, and where the list's length lives on the device
template <class I>
struct HeadList {
  const I *heads;
  const FallbackRec *recs;      // the classifier's record of every head of the list, or null (dense SA: nothing was classified)
  const uint64_t *n_dev;
  uint64_t n;
};

// The state of one merge_bwt call, and one member function per step of it (run() is the list).  The buffers are grouped by
// what they describe; every group lives to the end of the call, what is needed for a shorter time is a local of its step.
template <class I>
struct Merge {
  // ---- fixed when the call starts
  pfp_ctx *const c;
  const Dictionary &D;
  const DictIndex &ix;
  const SuffixOrderT<I> &so;
  const ParseBWT &pb;
  const uint32_t *const occ_lex;
  const MergeOpts o;
  BwtOutputs &out;
  // NP dictionary positions; N suffix-array slots held by `so` (all of them, or - multi-GPU, key-range
  // sharded sort - one contiguous range of SA(D) whose first output position is o.pos_base)
  const uint64_t NP, N;
  const uint32_t d;
  // SA values: none, all (-S), or only where the sampled files can look (-s / -e): run boundaries of the BWT
  const int sa_mode;
  const MergeSwitches sw;
  const RecordSource src;
  const WordView wv;
  const uint64_t ntile;         // offset tiles: covers slot index N (one past the last)
  const uint32_t nblk;          // expand workgroups
  // what one launch writes in the first round: chars and SA values together (dense), or chars first and - once the finished
  // BWT says where the sampled files can look - SA values in a second round of the same kernels (sparse)
  const int first_pass;

  MergeArgsT<I> a{};            // what the kernels get (its `pass` comes from with_pass)
  uint64_t n_out = 0;

  // ---- per word
  struct {
    DBuf<uint32_t> istart_lex, wistart;      // istart in lexicographic order (pfbwt.cpp:388-396), looked up per word
    DBuf<uint32_t> iword;                    // the word of every inverted-list entry, where the parse stage left none
    DBuf<WordRec> wrec;                      // list start, occurrences, smallest / largest BWT(P) position, terminator
  } word;
  // ---- per slot
  struct {
    DBuf<uint8_t> pc, hard;
    DBuf<uint32_t> loc, ovf;
    DBuf<uint64_t> tsum, tbase;
    DBuf<uint32_t> sfirst, slast, ssl;
  } slot;
  // ---- hard groups
  enum { kAllHeads = 0, kFallbackHeads = 1 };      // entries of hg.list_len
  struct {
    DBuf<unsigned long long> hstats;
    uint64_t n_heads = 0;
    uint32_t big_cap = 0, mid_cap = 0;
    DBuf<BigGroup> big, mid;      // queues of hard_groups_kernel: groups of more than 1024 / more than kHardSortMin occurrences
    DBuf<I> heads;
    DBuf<uint64_t> list_len;      // [kAllHeads] heads selected, [kFallbackHeads] fallback heads selected
    DBuf<unsigned long long> mstat;      // chars and members of the hard groups the minority path takes
    // BWT only / sparse SA: majority fill + minority placement
    DBuf<uint8_t> gmaj, fallback;
    DBuf<HardGroupInfo> ginfo;
    DBuf<uint32_t> minor_cnt, mm_cnt;
    DBuf<uint64_t> minor_off, mm_off;
    DBuf<MinorMember> mm_list;
    uint64_t n_mm = 0, sum_k = 0, n_minor = 0, n_staged = 0;
    DBuf<I> fb_heads;
    DBuf<FallbackRec> fb_recs;    // ... and what the classifier knows of each (phase A of hard_groups_kernel)
    DBuf<MinorRec> recs;          // sparse SA: what a minority occurrence found, for the second round
    DBuf<uint64_t> soff;          // sparse SA: occurrences of the fallback groups before each (and, last, of all): staging offsets
    DBuf<RankedOcc> ranked;       // ... and the staging itself, from the BWT round to the end of the SA round (empty: the SA round ranks again)
    int gpb = 64;                 // groups per wave batch of hard_groups_kernel
    uint32_t nmid = 0, nbig = 0;
    DBuf<uint64_t> estart;        // occurrences of the queued groups, laid end to end
    std::vector<uint64_t> es;     // ... and their host copy
  } hg;
  DBuf<uint32_t> heavy, nheavy;   // expand workgroups beyond their quota

  Merge(pfp_ctx *c_, const Dictionary &D_, const DictIndex &ix_, const SuffixOrderT<I> &so_, const ParseBWT &pb_, const uint32_t *occ_lex_,
        const MergeOpts &o_, BwtOutputs &out_)
      : c(c_), D(D_), ix(ix_), so(so_), pb(pb_), occ_lex(occ_lex_), o(o_), out(out_), NP(D_.dsize), N(so_.N), d((uint32_t)D_.d),
        sa_mode(!o_.flags ? SA_NONE : ((o_.flags & PFP_FLAG_SA) ? SA_DENSE : SA_SPARSE)), sw(MergeSwitches::read()),
        src(choose_record_source<I>(c_, N, NP, sa_mode, so_, sw)), wv(word_view(D_, ix_)), ntile((N >> kOffTileLog) + 1),
        nblk((uint32_t)cdiv64(N, kSlots)), first_pass(sa_mode == SA_SPARSE ? PASS_BWT : (PASS_BWT | PASS_SA)) {}

  MergeArgsT<I> with_pass(int pass) const { MergeArgsT<I> x = a; x.pass = pass; return x; }

  // ---- 1. word records
  void word_records() {
    word.istart_lex.alloc(c, d); word.wistart.alloc(c, d);
    exclusive_sum_u32(c, occ_lex, word.istart_lex.p, d);
    word.wrec.alloc(c, d);
    hipLaunchKernelGGL(wistart_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, ix.lexrank.p, word.istart_lex.p, D.wocc.p, pb.ilist.p,
                       ix.wend.p, word.wistart.p, word.wrec.p);
    if (!pb.iword.p) {
      word.iword.alloc(c, pb.P + 1);
      hipLaunchKernelGGL(iword_kernel, gdim(cdiv(pb.P + 1, TB)), gdim(TB), 0, c->stream, pb.P, d, word.istart_lex.p, word.iword.p);
    }
  }

  // ---- 2. slot tables: chars, hard flags, counts per tile, from wherever the records are (cnt: the from-keys counts)
  void alloc_slot_tables() {
    slot.pc.alloc(c, N + 8); slot.hard.alloc(c, N);
    slot.loc.alloc(c, ntile << kOffTileLog); slot.ovf.alloc(c, 1);
    alloc_counts(c, slot.tsum, ntile); slot.tbase.alloc(c, ntile + 1);
    slot.hard.zero();
    slot.ovf.zero();
  }
  void slot_tables_from_keys(DBuf<uint32_t> &cnt) {
    { KScope ks(c, "pfp::slot_payload_kernel", N * (8 + 1 + 5));
      hipLaunchKernelGGL(slot_payload_kernel<I>, gdim(cdiv(cdiv64(N, 8), 256)), gdim(256), 0, c->stream, N, so.sa.p, so.skeys.p,
                         so.refined.p, D.bytes.p, wv, D.wocc.p, d, o.w, cnt.p, slot.pc.p); }
    { KScope ks(c, "pfp::slot_loc_kernel", N * 8);
      hipLaunchKernelGGL(slot_loc_kernel, gdim((unsigned)ntile), gdim(256), 0, c->stream, cnt.p, N, slot.loc.p, slot.tsum.p, slot.ovf.p); }
    { KScope ks(c, "pfp::group_flags_kernel", N * 5);
      hipLaunchKernelGGL(group_flags_kernel<I>, gdim(cdiv(N, TB)), gdim(TB), 0, c->stream, N, so.grp.p, slot.pc.p, 0, slot.hard.p); }
  }
  void slot_tables_gathered() {
    const int dense = sa_mode == SA_DENSE ? 1 : 0;
    const uint64_t np256 = cdiv64(NP, 256) * 256;
    DBuf<PosRec> prec(c, np256);      // (16 bytes per dictionary position: gone when the slots have their copies)
    { KScope ks(c, "pfp::pprec16_kernel", NP * (1 + 16) + (uint64_t)d * 40);
      hipLaunchKernelGGL(pprec16_kernel, gdim(cdiv(np256, TB)), gdim(TB), 0, c->stream, wv, o.w, reinterpret_cast<const uint4 *>(word.wrec.p),
                         dense, (uint64_t)0, NP, prec.p); }
    slot_records(prec.p);
  }
  void slot_tables_per_slot() { slot_records(nullptr); }
  void slot_records(const PosRec *prec) {
    const int dense = sa_mode == SA_DENSE ? 1 : 0;
    // per-slot copies of what the unit-edge / minority kernels ask about a slot's word (read coalesced there); full SA:
    // the list start of every slot's word and its suffix length
    slot.sfirst.alloc(c, ntile << kOffTileLog);
    if (!dense) slot.slast.alloc(c, ntile << kOffTileLog);
    if (sa_mode != SA_NONE) slot.ssl.alloc(c, ntile << kOffTileLog);
    KScope ks(c, "pfp::slot_records_kernel", N * (2 * sizeof(I) + (prec ? 16 : 64 + 32) + 4 + 1 + 4 + (slot.slast.p ? 4 : 0) + (slot.ssl.p ? 4 : 0)));
    hipLaunchKernelGGL(slot_records_kernel<I>, gdim((unsigned)ntile), gdim(256), 0, c->stream, N, so.sa.p, so.grp.p, prec, slot.loc.p,
                       slot.pc.p, slot.sfirst.p, slot.slast.p, slot.ssl.p, slot.tsum.p, slot.ovf.p, slot.hard.p, dense, wv, o.w, reinterpret_cast<const uint4 *>(word.wrec.p), dense);
  }

  // ---- 3. offsets and totals
  void offsets_and_totals() {
    exclusive_sum_u64(c, slot.tsum.p, slot.tbase.p, ntile + 1);
    PFP_REQUIRE(read_scalar(c, slot.ovf.p) == 0, PFP_ELIMIT, "2048 consecutive suffix-array slots emit 2^32 or more BWT positions");
    n_out = read_scalar(c, slot.tbase.p + ntile);
    PFP_REQUIRE(o.expect_n_out == 0 || n_out == o.expect_n_out, PFP_EFORMAT,
                "merge: sum of occurrence counts (" + std::to_string(n_out) + ") != text length + 1 (" +
                    std::to_string(o.expect_n_out) + ")");
    out.n_out = n_out;
  }

  // ---- 4. what the kernels get
  void fill_args() {
    const bool dense = sa_mode == SA_DENSE;
    a.N = N; a.n_out = n_out; a.d = d; a.w = o.w; a.want_sa = sa_mode;
    a.pos_base = o.pos_base; a.n_out_global = o.n_out_global ? o.n_out_global : n_out;
    a.sa = so.sa.p; a.grp = so.grp.p; a.wv = wv;
    a.ist = dense ? slot.sfirst.p : nullptr;          // full SA: the record's `first` field held the list start
    a.wistart = word.wistart.p; a.wrec = word.wrec.p;
    a.sfirst = dense ? nullptr : slot.sfirst.p; a.slast = slot.slast.p; a.ssl = slot.ssl.p;
    a.pc = slot.pc.p; a.hard = slot.hard.p; a.tbase = slot.tbase.p; a.loc = slot.loc.p;
    a.ilist = pb.ilist.p; a.bwlast = pb.bwlast.p; a.bwsai = pb.bwsai.p;
    a.istart_lex = word.istart_lex.p; a.iword = pb.iword.p ? pb.iword.p : word.iword.p;
    a.wslot_lex = ix.wslot_lex.p; a.slot_base = so.slot_base;
    // the caller's buffers hold positions [out_lo, out_hi): rebase so that kernels index by global position
    a.out_lo = o.out_lo; a.out_hi = o.out_hi < n_out ? o.out_hi : n_out;
    a.bwt = out.d_bwt - o.out_lo; a.out_sa = out.d_sa ? out.d_sa - o.out_lo : nullptr;
  }

  // ---- 5. hard groups: their heads, and the queues the LDS kernels fill
  void find_hard_groups() {
    hg.hstats.alloc(c, 5);
    hg.hstats.zero();
    // hard[] marks exactly the heads of the hard groups (group_flags_kernel): count, then compact them once
    hg.n_heads = count_flags(c, slot.hard.p, N);
    // queue of the groups of more than 1024 occurrences: each emits more than 1024 positions and is a hard group; redone larger
    // if it overflows all the same (PFP_BIG_CAP: tests)
    hg.big_cap = sw.big_cap ? sw.big_cap : (uint32_t)std::min<uint64_t>({(uint64_t)1u << 20, hg.n_heads + 1, n_out / 1024 + 1});
    hg.big.alloc(c, hg.big_cap);
    // such a group emits > kHardSortMin positions
    hg.mid_cap = (uint32_t)std::min<uint64_t>(n_out / (kHardSortMin + 1) + 64, 0x7FFFFFFFull);
    hg.mid.alloc(c, hg.mid_cap);
    hg.heads.alloc(c, hg.n_heads + 1);
    hg.list_len.alloc(c, 2);
    select_index<I>(c, slot.hard.p, hg.heads.p, hg.list_len.p + kAllHeads, N);
    hg.mstat.alloc(c, 2);
    hg.mstat.zero();
  }

  // ---- 6. BWT only / sparse SA: majority fill + minority placement; groups it leaves (no dominating char) go to the LDS
  //         kernels - the list that is returned
  HeadList<I> classify() {
    const uint64_t n_heads = hg.n_heads;
    hg.gmaj.alloc(c, N); hg.fallback.alloc(c, n_heads); hg.ginfo.alloc(c, n_heads);
    alloc_counts(c, hg.minor_cnt, n_heads); hg.minor_off.alloc(c, n_heads + 1);
    alloc_counts(c, hg.mm_cnt, n_heads); hg.mm_off.alloc(c, n_heads + 1);
    a.gmaj = hg.gmaj.p;
    { KScope ks(c, "pfp::hard_classify_kernel", n_heads * 40);
      hipLaunchKernelGGL(hard_classify_kernel<I>, gdim(cdiv(n_heads, 256)), gdim(256), 0, c->stream, a, hg.heads.p, n_heads, hg.gmaj.p,
                         hg.ginfo.p, hg.minor_cnt.p, hg.fallback.p, hg.mstat.p, hg.mm_cnt.p); }
    exclusive_sum_u32_u64(c, hg.minor_cnt.p, hg.minor_off.p, n_heads + 1);
    exclusive_sum_u32_u64(c, hg.mm_cnt.p, hg.mm_off.p, n_heads + 1);
    hg.n_mm = read_scalar(c, hg.mm_off.p + n_heads);
    hg.sum_k = read_scalar(c, (const uint64_t *)hg.mstat.p + 1);
    if (hg.n_mm) {
      hg.mm_list.alloc(c, hg.n_mm);
      KScope ks(c, "pfp::hard_minor_fill_kernel", n_heads * 40 + hg.n_mm * 16);
      hipLaunchKernelGGL(hard_minor_fill_kernel<I>, gdim(cdiv(n_heads * 8, 256)), gdim(256), 0, c->stream, a, hg.ginfo.p, n_heads, hg.mm_off.p,
                         hg.minor_off.p, hg.gmaj.p, hg.mm_list.p);
    }
    const uint64_t n_fallback = count_flags(c, hg.fallback.p, n_heads);
    hg.n_minor = read_scalar(c, hg.minor_off.p + n_heads);
    hg.fb_heads.alloc(c, n_fallback + 1); hg.fb_recs.alloc(c, n_fallback + 1);
    {  // heads of the fallback groups = heads[] where fallback[] is set, and their records in the same gather
      DBuf<I> fidx(c, n_fallback + 1);
      DBuf<uint64_t> fb_E;      // sparse SA: occurrences of every fallback group, summed to its staging offset
      if (sa_mode == SA_SPARSE && n_fallback && sw.sa_replay != 0) { alloc_counts(c, fb_E, n_fallback); hg.soff.alloc(c, n_fallback + 1); }
      select_index<I>(c, hg.fallback.p, fidx.p, hg.list_len.p + kFallbackHeads, n_heads);
      if (n_fallback) hipLaunchKernelGGL(fb_records_kernel<I>, gdim(cdiv(n_fallback, 256)), gdim(256), 0, c->stream, a, n_fallback, fidx.p,
                                         hg.ginfo.p, hg.fb_heads.p, hg.fb_recs.p, fb_E.p);
      if (fb_E.p) exclusive_sum_u64(c, fb_E.p, hg.soff.p, n_fallback + 1);
      PFP_HIP(hipGetLastError());
      if (fb_E.p) hg.n_staged = read_scalar(c, hg.soff.p + n_fallback);      // (syncs, as the other branch)
      else sync(c);
    }
    if (c->debug && n_fallback) {      // the records are what phase A's walk would find (FallbackRec)
      DBuf<unsigned long long> bad(c, 1);
      bad.zero();
      hipLaunchKernelGGL(fb_records_check_kernel<I>, gdim(cdiv(n_fallback, 256)), gdim(256), 0, c->stream, a, n_fallback, hg.fb_recs.p, bad.p);
      const uint64_t nb = read_scalar(c, (const uint64_t *)bad.p);
      PFP_REQUIRE(nb == 0, PFP_EHIP, "merge: " + std::to_string(nb) + " fallback records differ from the walk over their group's members");
    }
    return HeadList<I>{hg.fb_heads.p, hg.fb_recs.p, hg.list_len.p + kFallbackHeads, n_fallback};
  }

  // ---- 7. expand: fill entries and the majority chars of the hard groups, then the whole words' chars occurrence by occurrence
  void expand() {
    const MergeArgsT<I> ap = with_pass(first_pass);
    const bool dense = sa_mode == SA_DENSE;
    heavy.alloc(c, nblk); nheavy.alloc(c, 1);
    nheavy.zero();
    // per slot: offset, char, group and its flag; per position the byte (dense: ilist entry, bwsai gather, 8-byte value)
    { KScope ks(c, "pfp::expand_kernel", N * (4 + 1 + sizeof(I) + 1) + n_out * (dense ? 17 : 1));
      if (dense) hipLaunchKernelGGL((expand_kernel<I, true>), gdim(nblk), gdim(256), 0, c->stream, ap, heavy.p, nheavy.p, nblk);
      else hipLaunchKernelGGL((expand_kernel<I, false>), gdim(nblk), gdim(256), 0, c->stream, ap, heavy.p, nheavy.p, nblk); }
    const uint32_t nh = read_scalar(c, nheavy.p);
    { KScope ks2(c, "pfp::expand_heavy_kernel", 0);   // bytes are accounted in expand_kernel's n_out term
      if (nh && dense) hipLaunchKernelGGL((expand_heavy_kernel<I, true>), gdim(c->n_cu * 4), gdim(256), 0, c->stream, ap, heavy.p, nh);
      else if (nh) hipLaunchKernelGGL((expand_heavy_kernel<I, false>), gdim(c->n_cu * 4), gdim(256), 0, c->stream, ap, heavy.p, nh); }
    if (pb.P) {      // per entry: its word's rank and BWT(P) position, the word's slot, list start and offset, one char in and out
      KScope ks(c, "pfp::word_chars_kernel", pb.P * (4 + 4 + 1 + 1) + (uint64_t)d * (8 + 4 + 12));
      hipLaunchKernelGGL(word_chars_kernel<I>, gdim(cdiv(pb.P, 256)), gdim(256), 0, c->stream, ap, pb.P);
    }
    PFP_HIP(hipGetLastError());
  }

  // ---- 8. minority occurrences, ranked against their group's lists and written over the fill
  void place_minority(const HeadList<I> &lds) {
    if (hg.n_mm) {
      const MergeArgsT<I> ap = with_pass(first_pass);
      if (sa_mode == SA_SPARSE) hg.recs.alloc(c, hg.n_minor + 1);
      KScope ks(c, "pfp::hard_minor_kernel", hg.n_minor * 64);
      // lanes per minority member: eight, or the wave where the groups average more than 32 members
      const uint64_t avg_k = hg.sum_k / std::max<uint64_t>(hg.n_heads - lds.n, 1);
      if (avg_k > 32)
        hipLaunchKernelGGL((hard_minor_kernel<I, 64>), gdim((unsigned)std::min<uint64_t>(cdiv64(hg.n_mm, 4), (uint64_t)c->n_cu * 64)), gdim(256), 0,
                           c->stream, ap, hg.mm_list.p, hg.n_mm, hg.recs.p);
      else
        hipLaunchKernelGGL((hard_minor_kernel<I, 8>), gdim((unsigned)std::min<uint64_t>(cdiv64(hg.n_mm, 32), (uint64_t)c->n_cu * 64)), gdim(256), 0,
                           c->stream, ap, hg.mm_list.p, hg.n_mm, hg.recs.p);
    }
    PFP_HIP(hipGetLastError());
  }

  // ---- 9. sparse SA: shall the kernels that rank the fallback groups' occurrences stage them (8 bytes each, hg.soff says
  //         where), so that the SA round replays the ranks instead of computing them again?  Yes, unless the staging would
  //         take more than the share of the device that choose_record_source allows the position records
  //         (PFP_SA_REPLAY_BUDGET: another share, tests); PFP_SA_REPLAY=1/0 forces the choice
  void stage_ranks() {
    if (!hg.n_staged) return;
    const uint64_t budget = sw.replay_budget != ~0ull ? sw.replay_budget : device_bytes(c) / 8;
    const bool replay = (sw.sa_replay >= 0 ? sw.sa_replay != 0 : hg.n_staged * sizeof(RankedOcc) <= budget) && hg.soff.n <= (1ull << 32);      // (BigGroup::head)
    if (!replay) { hg.soff.release(); return; }
    hg.ranked.alloc(c, hg.n_staged);
    if (c->debug) PFP_HIP(hipMemsetAsync(hg.ranked.p, 0xFF, hg.n_staged * sizeof(RankedOcc), c->stream));      // kUnwritten
    a.ranked = hg.ranked.p; a.soff = hg.soff.p;
  }

  // ---- 10. the groups of the list ranked in LDS; larger ones are queued (hg.mid, hg.big) - redone when the big queue overflows
  void rank_in_lds(const HeadList<I> &lds) {
    const MergeArgsT<I> ap = with_pass(first_pass);
    // groups per wave batch: down to 8 while that still leaves every wave of the launch a batch
    while (hg.gpb > 8 && lds.n / hg.gpb < (uint64_t)c->n_cu * 32) hg.gpb >>= 1;
    for (;;) {
      if (!lds.n) { PFP_HIP(hipMemsetAsync(hg.hstats.p, 0, 40, c->stream)); }
      else { KScope ks(c, "pfp::hard_groups_kernel", N * 5);
        hipLaunchKernelGGL((hard_groups_kernel<I, false>), gdim(c->n_cu * 8), gdim(256), 0, c->stream, ap, lds.heads, lds.recs, lds.n_dev,
                           hg.hstats.p, hg.big.p, hg.big_cap, hg.mid.p, hg.mid_cap, hg.gpb, (unsigned long long *)nullptr); }
      PFP_HIP(hipGetLastError());
      PFP_HIP(hipMemcpyAsync(c->h_scalars, hg.hstats.p, 40, hipMemcpyDeviceToHost, c->stream));
      sync(c);
      if (c->h_scalars[2] <= hg.big_cap) break;
      hg.big_cap = (uint32_t)std::min<uint64_t>(c->h_scalars[2], 0xFFFFFFFFull);   // rare: redo with a queue that fits
      hg.big.alloc(c, hg.big_cap);
      hg.hstats.zero();
    }
    out.hard_chars = c->h_scalars[0];
    out.hard_groups = c->h_scalars[1];
    out.hard_minor_groups = hg.n_heads - lds.n; out.hard_minor_chars = hg.n_minor;
    out.hard_big_groups = c->h_scalars[2]; out.hard_max_members = c->h_scalars[4];
    hg.nmid = (uint32_t)std::min<uint64_t>(c->h_scalars[3], hg.mid_cap);
    PFP_REQUIRE(c->h_scalars[3] <= hg.mid_cap, PFP_EHIP, "more sorted-path hard groups than the output can hold");
    hg.nbig = (uint32_t)c->h_scalars[2];
    out.hard_chars += read_scalar(c, (const uint64_t *)hg.mstat.p);      // all chars of hard groups, whichever path wrote them
    out.hard_groups += hg.n_heads - lds.n;
  }

  // ---- 11. occurrences of the queued groups, laid end to end
  void lay_out_queued() {
    const uint32_t nbig = hg.nbig;
    hg.es.assign(nbig + 1, 0);
    if (!nbig) return;
    std::vector<BigGroup> hb(nbig);
    PFP_HIP(hipMemcpyAsync(hb.data(), hg.big.p, nbig * sizeof(BigGroup), hipMemcpyDeviceToHost, c->stream));
    sync(c);
    for (uint32_t q = 0; q < nbig; q++) hg.es[q + 1] = hg.es[q] + hb[q].E;
    hg.estart.alloc(c, nbig + 1);
    PFP_HIP(hipMemcpyAsync(hg.estart.p, hg.es.data(), (nbig + 1) * 8, hipMemcpyHostToDevice, c->stream));
    sync(c);
  }

  // ---- 12. the queued groups: sorted in LDS (mid), merged by device-wide sorts or ranked occurrence by occurrence (big)
  void queued_groups(int pass) {
    const MergeArgsT<I> ap = with_pass(pass);
    const std::vector<uint64_t> &es = hg.es;
    if (hg.nmid) {
      KScope ks(c, "pfp::hard_sort_kernel", (uint64_t)hg.nmid * (kHardSortMin + 1) * (sa_mode ? 21 : 5));      // lower bound: ilist entry + char (+ SA) per occurrence
      hipLaunchKernelGGL(hard_sort_kernel<I>, gdim(c->n_cu * 4), gdim(256), 0, c->stream, ap, hg.mid.p, hg.nmid);
      PFP_HIP(hipGetLastError());
    }
    // queued groups in chunks of at most big_budget occurrences: keys, one sort, placement (a single group beyond the
    // budget is ranked occurrence by occurrence - its sort scratch is not worth the memory)
    // The sort's four buffers are drawn once, by the first chunk that is sorted (a call whose groups all exceed the budget draws
    // none), and sized by the budget (or by all queued occurrences, if fewer), not by the chunk.
    // The queue is filled with atomics, so its order - and with it where the chunks are cut, by a few thousand occurrences -
    // differs from call to call: a request per chunk came out a few KB larger than the blocks the pool had cached from the
    // call before every now and then, and the 12.6 GB workload went to the driver for a gigabyte in its steady state
    // (PFP_TRACE_POOL shows the requests).  The sum of the queue is the same in every order.
    const uint64_t max_cnt = std::min<uint64_t>(sw.big_budget, es[hg.nbig]);
    DBuf<uint64_t> bk, bka, bv, bva;
    for (uint32_t q0 = 0; q0 < hg.nbig;) {
      uint32_t q1 = q0 + 1;
      while (q1 < hg.nbig && es[q1 + 1] - es[q0] <= sw.big_budget) q1++;
      const uint64_t cnt = es[q1] - es[q0];
      if (cnt > sw.big_budget) {
        const int nb = (int)std::min<uint64_t>(cdiv64(cnt, 256), (uint64_t)c->n_cu * 32);
        KScope ks(c, "pfp::hard_big_kernel", cnt * (sa_mode ? 21 : 5));
        hipLaunchKernelGGL(hard_big_kernel<I>, gdim(nb), gdim(256), 0, c->stream, ap, hg.big.p + q0, q1 - q0, hg.estart.p + q0, cnt);
      } else {
        if (!bk.p) { bk.alloc(c, max_cnt); bka.alloc(c, max_cnt); bv.alloc(c, max_cnt); bva.alloc(c, max_cnt); }
        { KScope ks(c, "pfp::big_keys_kernel", cnt * 28);
          hipLaunchKernelGGL(big_keys_kernel<I>, gdim(cdiv(cnt, 256)), gdim(256), 0, c->stream, ap, hg.big.p, q0, q1, hg.estart.p, cnt, bk.p, bv.p); }
        { SortTag tag("large hard groups"); sort_pairs_db<uint64_t, uint64_t>(c, bk, bka, bv, bva, cnt, 0, 32 + bits_for(q1 - q0)); }
        { KScope ks(c, "pfp::big_place_kernel", cnt * (sa_mode ? 34 : 18));
          hipLaunchKernelGGL(big_place_kernel<I>, gdim(cdiv(cnt, 256)), gdim(256), 0, c->stream, ap, hg.big.p, q0, hg.estart.p, cnt, bk.p, bv.p); }
      }
      PFP_HIP(hipGetLastError());
      q0 = q1;
    }
  }

  // ---- 13. sparse SA, second round: where can the sampled files look?  The run boundaries of the finished BWT slice
  void mark_run_boundaries() {
    const uint64_t cnt_slice = a.out_hi > a.out_lo ? a.out_hi - a.out_lo : 0;
    const uint64_t nw = cdiv64(cnt_slice, 64);
    out.bmap.alloc(c, nw + 1); out.bpre.alloc(c, nw + 1);
    // ... and no SA array to write to: the sampled files come from bitmaps (a slice's two edge positions count as run
    // starts / ends here; the multi-GPU caller drops them again when the neighbour's halo byte says so)
    const bool want_s = !out.d_sa && (o.flags & PFP_FLAG_SSA), want_e = !out.d_sa && (o.flags & PFP_FLAG_ESA);
    out.slice_n = cnt_slice;
    {
      DBuf<uint32_t> wcnt, scnt, ecnt;      // boundaries per word of the maps
      alloc_counts(c, wcnt, nw);
      PFP_HIP(hipMemsetAsync(out.bmap.p + nw, 0, 8, c->stream));
      if (want_s) { out.smap.alloc(c, nw + 1); out.spre.alloc(c, nw + 1); alloc_counts(c, scnt, nw); }
      if (want_e) { out.emap.alloc(c, nw + 1); out.epre.alloc(c, nw + 1); alloc_counts(c, ecnt, nw); }
      if (nw) {
        KScope ks(c, "pfp::run_bitmap_kernel", cnt_slice + nw * (12 + (want_s ? 12 : 0) + (want_e ? 12 : 0)));
        hipLaunchKernelGGL(run_bitmap_kernel, gdim(cdiv(cdiv64(cnt_slice, 16), 256)), gdim(256), 0, c->stream, out.d_bwt, cnt_slice,
                           out.bmap.p, wcnt.p, out.smap.p, scnt.p, out.emap.p, ecnt.p);
      }
      exclusive_sum_u32_u64(c, wcnt.p, out.bpre.p, nw + 1);
      if (want_s) exclusive_sum_u32_u64(c, scnt.p, out.spre.p, nw + 1);
      if (want_e) exclusive_sum_u32_u64(c, ecnt.p, out.epre.p, nw + 1);
      out.n_bound = read_scalar(c, out.bpre.p + nw);
      if (want_s) out.n_starts = read_scalar(c, out.spre.p + nw);
      if (want_e) out.n_ends = read_scalar(c, out.epre.p + nw);
    }
    a.bmap = out.bmap.p; a.bpre = out.bpre.p;
    if (!out.d_sa) {      // the caller keeps no SA array: values go to their rank among the boundaries
      out.sa_c.alloc(c, out.n_bound + 1);
      if (c->debug) PFP_HIP(hipMemsetAsync(out.sa_c.p, 0xFF, (out.n_bound + 1) * 8, c->stream));
      a.sa_c = out.sa_c.p;
    }
  }

  // ---- 14. sparse SA, second round: SA values at the boundaries, class by class
  void sa_round(const HeadList<I> &lds) {
    const MergeArgsT<I> ap = with_pass(PASS_SA);
    // whole words: one lane per occurrence of the inverted lists (a parse without phrases emits nothing)
    if (pb.P) {      // per entry: its word's rank; at a boundary its BWT(P) position, the bwsai gather and the value
      KScope ks(c, "pfp::word_sa_kernel", pb.P * (4 + 1) + (uint64_t)d * (8 + 4 + 12) + out.n_bound * (4 + 8 + 8));
      hipLaunchKernelGGL(word_sa_kernel<I>, gdim(cdiv(pb.P, 256)), gdim(256), 0, c->stream, ap, pb.P);
    }
    { KScope ks(c, "pfp::unit_edges_kernel", N * (1 + sizeof(I) * 2 + 4));
      hipLaunchKernelGGL(unit_edges_kernel<I>, gdim(cdiv(N, 256)), gdim(256), 0, c->stream, ap); }
    if (hg.n_mm) {
      const uint64_t nr = hg.n_minor;      // one record per minority occurrence, at its precomputed index (MinorMember::roff)
      if (nr) hipLaunchKernelGGL(hard_minor_sa_kernel<I>, gdim(cdiv(nr, 256)), gdim(256), 0, c->stream, ap, hg.recs.p, nr);
    }
    if (lds.n && hg.ranked.p) replay_ranks(ap, lds);
    else if (lds.n) {      // the groups the LDS kernels ranked: the same ranks again, SA values this time (queues as they stand)
      { KScope ks(c, "pfp::hard_groups_kernel", N * 5);
        hipLaunchKernelGGL((hard_groups_kernel<I, false>), gdim(c->n_cu * 8), gdim(256), 0, c->stream, ap, lds.heads, lds.recs,
                           lds.n_dev, (unsigned long long *)nullptr, hg.big.p, 0u, hg.mid.p, 0u, hg.gpb, (unsigned long long *)nullptr); }
      PFP_HIP(hipGetLastError());
      queued_groups(PASS_SA);
      sync(c);
    }
    PFP_HIP(hipGetLastError());
  }
  // the fallback groups' share of the SA round when the BWT round staged their ranks: the groups ranked in LDS through
  // hard_groups_kernel's replay (a batch of gpb groups per wave, no LDS: four times the workgroups), the queued ones
  // through hard_replay_kernel - no inverted-list gather, no ranking, no sort
  void replay_ranks(const MergeArgsT<I> &ap, const HeadList<I> &lds) {
    DBuf<unsigned long long> unwritten;      // PFP_DEBUG: staged entries of the slice that nobody wrote
    if (c->debug) { unwritten.alloc(c, 1); unwritten.zero(); }
    // (bytes, a lower bound: the groups' records and the map's bits; entries and values are read at boundaries only)
    { KScope ks(c, "pfp::hard_groups_kernel", lds.n * 40 + hg.n_staged / 8);
      const uint64_t nwg = std::min<uint64_t>(cdiv64(cdiv64(lds.n, hg.gpb), 4), (uint64_t)c->n_cu * 32);
      hipLaunchKernelGGL((hard_groups_kernel<I, true>), gdim(nwg), gdim(256), 0, c->stream, ap, lds.heads, lds.recs, lds.n_dev,
                         (unsigned long long *)nullptr, hg.big.p, 0u, hg.mid.p, 0u, hg.gpb, unwritten.p); }
    const uint64_t nq = hg.es[hg.nbig];      // occurrences of the big queue
    if (hg.nmid || nq) {
      KScope ks(c, "pfp::hard_replay_kernel", ((uint64_t)hg.nmid + hg.nbig) * 32 + (nq + (uint64_t)hg.nmid * (kHardSortMin + 1)) / 8);
      const uint64_t nwg = std::min<uint64_t>(std::max<uint64_t>(cdiv64(hg.nmid, 4), cdiv64(nq, 256)), (uint64_t)c->n_cu * 32);
      hipLaunchKernelGGL(hard_replay_kernel<I>, gdim(nwg), gdim(256), 0, c->stream, ap, hg.mid.p, hg.nmid, hg.big.p, hg.nbig, hg.estart.p, nq,
                         unwritten.p);
    }
    PFP_HIP(hipGetLastError());
    if (c->debug) {
      const uint64_t u = read_scalar(c, (const uint64_t *)unwritten.p);
      PFP_REQUIRE(u == 0, PFP_EHIP, "sparse SA: the replay met " + std::to_string(u) + " staged occurrences that the BWT round did not write");
    }
  }

  // ---- 15. PFP_DEBUG: every boundary of the BWT must have received its value
  void check_boundaries_set() {
    if (!c->debug || !a.sa_c) return;
    DBuf<unsigned long long> unset(c, 1);
    unset.zero();
    // (a slice's own two edge positions are marked as boundaries whatever their neighbours in the other slices hold:
    //  when they lie inside a run of the whole BWT nobody owes them a value - and nobody will sample them)
    const uint64_t skip_lo = (a.pos_base + a.out_lo > 0) ? 1 : 0, skip_hi = (a.pos_base + a.out_hi < a.n_out_global) ? 1 : 0;
    if (out.n_bound > skip_lo + skip_hi)
      hipLaunchKernelGGL(count_unset_kernel, gdim(cdiv(out.n_bound, 256)), gdim(256), 0, c->stream, out.sa_c.p + skip_lo,
                         out.n_bound - skip_lo - skip_hi, unset.p);
    const uint64_t u = read_scalar(c, (const uint64_t *)unset.p);
    PFP_REQUIRE(u == 0, PFP_EHIP, "sparse SA: " + std::to_string(u) + " run boundaries of the BWT received no SA value");
  }

  void run() {
    PFP_REQUIRE(!o.flags || pb.bwsai.p, PFP_EINVAL, "SA output requested without sa info");
    // the whole words are written and sampled by inverted-list entry (every caller ranks the words - compute_lexrank or
    // compute_lexrank_from_slots - before it merges)
    PFP_REQUIRE(ix.wslot_lex.p, PFP_EINVAL, "merge: the dictionary index has no whole-word slots (compute_lexrank has not run)");
    word_records();
    {
      DBuf<uint32_t> cnt;      // from the sort keys: occurrences per slot, until the offsets are summed
      if (src == RecordSource::SortKeys) alloc_counts(c, cnt, N, 8);
      alloc_slot_tables();
      switch (src) {
        case RecordSource::SortKeys: slot_tables_from_keys(cnt); break;
        case RecordSource::Gathered: slot_tables_gathered(); break;
        case RecordSource::PerSlot: slot_tables_per_slot(); break;
      }
      offsets_and_totals();
    }
    fill_args();
    find_hard_groups();
    const HeadList<I> lds = sa_mode != SA_DENSE && hg.n_heads ? classify() : HeadList<I>{hg.heads.p, nullptr, hg.list_len.p + kAllHeads, hg.n_heads};
    expand();
    place_minority(lds);
    stage_ranks();
    rank_in_lds(lds);
    lay_out_queued();
    queued_groups(first_pass);
    if (sa_mode == SA_SPARSE) {
      mark_run_boundaries();
      sa_round(lds);
      check_boundaries_set();
    }
    sync(c);
  }
};

template <class I>
void merge_bwt(pfp_ctx *c, const Dictionary &D, const DictIndex &ix, const SuffixOrderT<I> &so, const ParseBWT &pb,
               const uint32_t *occ_lex, const MergeOpts &o, BwtOutputs &out) {
  Merge<I>(c, D, ix, so, pb, occ_lex, o, out).run();
}
template void merge_bwt<uint32_t>(pfp_ctx *, const Dictionary &, const DictIndex &, const SuffixOrderT<uint32_t> &, const ParseBWT &,
                                  const uint32_t *, const MergeOpts &, BwtOutputs &);
template void merge_bwt<uint64_t>(pfp_ctx *, const Dictionary &, const DictIndex &, const SuffixOrderT<uint64_t> &, const ParseBWT &,
                                  const uint32_t *, const MergeOpts &, BwtOutputs &);

}  // namespace pfp
