// fmchain.hip -- chaining anchors: every occurrence of every MEM of a pattern, the chaining programme over them, the peel that
// cuts its forest into chains, and the long-read layer that merges both strands' chains.  The reference has no counterpart; the
// method is seed chaining as in Li, "Minimap2: pairwise alignment for nucleotide sequences" (Bioinformatics 2018), section 2.1,
// over MEM anchors, in integer arithmetic.  include/pfpgpu.h, "Chaining anchors", states the definitions (anchors, predecessors,
// gain, score, parent, peel, the fields and the order of chains, the strand merge and MAPQ).
//
//   Anchors.  The MEM triples of the patterns (fmsearch.hip) give one string each, pat[begin .. end): fm_count_spans counts them
//   where they lie, a lane per MEM empties the ranges wider than max_occ and counts them as skipped, fm_locate lists the others'
//   rows, and a lane per occurrence applies the record test and leaves te = t + len (or a value above every te for a dropped
//   one).  A pattern's occurrences are one segment, MEM by MEM, so by increasing i + len already; the library's segmented sort
//   orders it by te with the slot in the key's low half, which makes every key distinct and the order (te, i + len) whatever the
//   sort does with equal keys.  32 bits of te go into a pass, so an index of 64-bit positions takes two.  A lane per pattern finds
//   where the dropped ones begin, the library scan of the counts is anc_off, a lane per slot writes the triples.
//   The programme.  One wave per pattern, four per workgroup.  The last 64 anchors are a ring, one per lane: lane x & 63 holds
//   qe, te, rec and f of anchor x in registers.  64 anchors are loaded at a time, one per lane; anchor x is broadcast from lane
//   x & 63 with v_readlane (x is wave-uniform), every lane evaluates the anchor it holds against it and leaves the key
//   (f_j + gain + 2^30) << 8 | 64 - (x - j), or 0 if j is no predecessor; one wave-wide maximum of the keys (six DPP steps on both
//   halves of the key: row_shr 1 / 2 / 4 / 8 and the two row broadcasts, as devutil.hpp's wave_max) is f_x, and its low bits the
//   parent: among equal values the largest j.  Lane x & 63 then takes anchor x into the ring.  No LDS, no atomics but the count
//   of unfinished patterns.  A launch advances a pattern by at most PFP_FM_CHAIN_STEPS anchors; it resumes by reloading the ring
//   from the anchors and f.
//   The peel.  The segmented sort orders a pattern's anchors by (~f, index).  One lane per pattern visits them and walks the
//   parents of every unvisited one; where a walk ends it leaves the chain's fields at the entry of the anchor it began at, the
//   chain's last, if the score reaches min_score.  A launch takes at most PFP_FM_CHAIN_STEPS visits and steps of a pattern; its place in the order and its walk
//   wait in a record.  Anchors are sorted by (te, qe), so the order of output (score descending, te, qe) is (~score, index of the
//   chain's last anchor): a third segmented sort, a count, the library scan, and a lane per chain that writes its fields.
//   Long reads.  Both strands of every read (fm_map_strands) go through all of the above; a read's chains are the segment
//   chain_off[2p] .. chain_off[2p + 2], strand 0's first and each strand's in order, so (score descending, strand, te, qe) is
//   (~score, index of the chain): a fourth segmented sort.  A lane per read counts and derives MAPQ, a lane per returned chain
//   looks up the record and turns strand 1's pattern coordinates into the read's.
// Bounds: every index read from an offset, a sorted value or a parent is used inside its own pattern's segment; the ring's
// parents point at most 64 anchors back and never before the pattern's first; text positions only ever become outputs or go
// through seq_of below n.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"

namespace pfp {

namespace {

static_assert(PFP_FM_CHAIN_PRED == 64, "the ring of predecessors is one wavefront");
constexpr uint64_t kChainSteps = 65536;     // anchors of a pattern per launch of the programme, visits and steps per launch of the peel
constexpr uint64_t kNoKey = ~0ull;
constexpr uint32_t kNoAnchor = 0xFFFFFFFFu;
constexpr int64_t kBias = 1ll << 30;        // f_j + gain > -2^29: cost(g) <= (2^31 + 2) / 4

// PFP_FM_CHAIN_STEPS: a bound below the default (tests: a small one reaches the resume paths with small inputs)
uint64_t chain_steps_from_env() {
  uint64_t steps = kChainSteps;
  if (const char *e = getenv("PFP_FM_CHAIN_STEPS")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < steps) steps = v;
  }
  return steps;
}

// ---------------------------------------------------------------- anchors
// one lane per MEM j < M of the npat patterns: its string lies at pat[begin[j] .. end[j])
__global__ void __launch_bounds__(kTB) anc_spans_k(const uint64_t *__restrict__ pat_off, uint64_t npat, const uint64_t *__restrict__ mem_off,
                                                   const uint64_t *__restrict__ mem, uint64_t M, uint64_t *__restrict__ begin,
                                                   uint64_t *__restrict__ end) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j >= M) return;
  const uint64_t p = last_le(mem_off, npat, j);         // (mem_off[0] = 0 <= j < mem_off[npat])
  const uint64_t b = pat_off[p] + mem[3 * j];
  begin[j] = b; end[j] = b + mem[3 * j + 1];
}

// one lane per MEM: a range of more than max_occ rows becomes empty and counts as skipped
__global__ void __launch_bounds__(kTB) anc_clip_k(const uint64_t *__restrict__ sp, const uint64_t *__restrict__ ep, uint64_t M, uint64_t max_occ,
                                                  const uint64_t *__restrict__ mem_off, uint64_t npat, uint64_t *__restrict__ cep,
                                                  uint32_t *__restrict__ skipped) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j >= M) return;
  const uint64_t s = sp[j], e = ep[j];
  const bool skip = e > s && e - s > max_occ;
  cep[j] = skip ? s : e;
  if (skip && skipped) atomicAdd(&skipped[last_le(mem_off, npat, j)], 1u);
}

// one lane per occurrence o < O: tek[o] = t + len if the anchor lies inside one record (the whole text without a table), else drop
template <class I>
__global__ void __launch_bounds__(kTB) anc_ends_k(SeqArgs<I> sq, int has_seq, const uint64_t *__restrict__ occ_off, uint64_t M,
                                                  const uint64_t *__restrict__ mem, const uint64_t *__restrict__ pos, uint64_t O, uint64_t drop,
                                                  uint64_t *__restrict__ tek) {
  const uint64_t o = BID * kTB + threadIdx.x;
  if (o >= O) return;
  const uint64_t j = last_le(occ_off, M, o), len = mem[3 * j + 1], t = pos[o];
  bool ok = t < sq.n && len <= sq.n - t;
  if (ok && has_seq) ok = t + len <= (uint64_t)sq.start[seq_of(sq, t) + 1];
  tek[o] = ok ? t + len : drop;
}

// one lane per slot s < O: key[s] = 32 bits of tek[src[s]] from bit `shift` on, above the slot
__global__ void __launch_bounds__(kTB) anc_key_k(const uint64_t *__restrict__ tek, const uint32_t *__restrict__ src, uint64_t O, int shift,
                                                 uint64_t *__restrict__ key) {
  const uint64_t s = BID * kTB + threadIdx.x;
  if (s >= O) return;
  key[s] = (((tek[src[s]] >> shift) & 0xFFFFFFFFull) << 32) | s;
}

// one lane per pattern (entry npat: 0): the slots of its segment before the first dropped occurrence
__global__ void __launch_bounds__(kTB) anc_count_k(const uint64_t *__restrict__ tek, const uint32_t *__restrict__ order, uint64_t O,
                                                   const uint32_t *__restrict__ sb, const uint32_t *__restrict__ se, uint64_t npat, uint64_t drop,
                                                   uint64_t *__restrict__ cnt) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p > npat) return;
  if (p == npat) { cnt[p] = 0; return; }
  uint64_t b = sb[p], e = se[p];
  if (e > O) e = O;
  if (b > e) b = e;
  uint64_t lo = b, hi = e;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (tek[order[mid]] != drop) lo = mid + 1;
    else hi = mid;
  }
  cnt[p] = lo - b;
}

// one lane per slot s < O of the sorted segments: a kept occurrence becomes anchor anc_off[p] + (s - its segment's start)
__global__ void __launch_bounds__(kTB) anc_write_k(const uint64_t *__restrict__ tek, const uint32_t *__restrict__ order, uint64_t O,
                                                   const uint64_t *__restrict__ seg_off, uint64_t npat, const uint64_t *__restrict__ occ_off,
                                                   uint64_t M, const uint64_t *__restrict__ mem, const uint64_t *__restrict__ pos, uint64_t drop,
                                                   const uint64_t *__restrict__ anc_off, uint64_t total, uint64_t *__restrict__ anc) {
  const uint64_t s = BID * kTB + threadIdx.x;
  if (s >= O) return;
  const uint64_t o = order[s];
  if (o >= O || tek[o] == drop) return;
  const uint64_t p = last_le(seg_off, npat, s), a = anc_off[p] + (s - seg_off[p]);
  if (a >= total) return;
  const uint64_t j = last_le(occ_off, M, o);
  anc[3 * a] = mem[3 * j]; anc[3 * a + 1] = mem[3 * j + 1]; anc[3 * a + 2] = pos[o];
}

// ---------------------------------------------------------------- checks of a caller's anchors
// h[0] += offsets that decrease; h[1] = anc_off[npat]
__global__ void __launch_bounds__(kTB) chain_offsets_k(const uint64_t *__restrict__ off, uint64_t npat, unsigned long long *__restrict__ h) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p >= npat) return;
  if (off[p] > off[p + 1]) atomicAdd(&h[0], 1ull);
  if (p + 1 == npat) h[1] = off[npat];
}

struct Anchor { uint64_t i, len, t; };
__device__ __forceinline__ Anchor anchor_at(const uint64_t *__restrict__ anc, uint64_t a) { return Anchor{anc[3 * a], anc[3 * a + 1], anc[3 * a + 2]}; }

// one lane per anchor a in [off[0], A): bad[0] = the smallest index of one that breaks a rule (len = 0, i + len >= 2^32, t + len
// wraps, or not above the anchor before it in its pattern by (t + len, i + len))
__global__ void __launch_bounds__(kTB) chain_check_k(const uint64_t *__restrict__ off, uint64_t npat, const uint64_t *__restrict__ anc, uint64_t A,
                                                     unsigned long long *__restrict__ bad) {
  const uint64_t a = BID * kTB + threadIdx.x;
  if (a >= A || a < off[0]) return;
  const Anchor x = anchor_at(anc, a);
  bool ok = x.len >= 1 && x.i < (1ull << 32) && x.len < (1ull << 32) && x.i + x.len < (1ull << 32) && x.t <= ~0ull - x.len;
  if (ok && a > off[last_le(off, npat, a)]) {
    const Anchor y = anchor_at(anc, a - 1);
    const uint64_t te = x.t + x.len, pe = y.t + y.len;  // (y passes or fails its own test)
    ok = pe < te || (pe == te && y.i + y.len < x.i + x.len);
  }
  if (!ok) atomicMin(&bad[0], (unsigned long long)a);
}

// ---------------------------------------------------------------- the programme
template <int CTRL, int ROWS>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {       // (a lane without a source gets 0, the identity of the maximum)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROWS, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROWS, 0xf, false);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }
// the maximum over the 64 lanes of a wave (all of them active), the same in every lane
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  v = max_u64(v, dpp_u64<0x111, 0xf>(v));               // row_shr:1
  v = max_u64(v, dpp_u64<0x112, 0xf>(v));               // row_shr:2
  v = max_u64(v, dpp_u64<0x114, 0xf>(v));               // row_shr:4
  v = max_u64(v, dpp_u64<0x118, 0xf>(v));               // row_shr:8
  v = max_u64(v, dpp_u64<0x142, 0xa>(v));               // row_bcast:15 into rows 1 and 3
  v = max_u64(v, dpp_u64<0x143, 0xc>(v));               // row_bcast:31 into rows 2 and 3
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int k) {     // (k is the same in every lane)
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k);
  return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint32_t readlane_u32(uint32_t v, int k) { return (uint32_t)__builtin_amdgcn_readlane((int)v, k); }

template <class I>
__device__ __forceinline__ uint32_t rec_of(const SeqArgs<I> &sq, int has_seq, uint64_t t) {
  if (!has_seq) return 0;
  return t < sq.n ? seq_of(sq, t) : kNoSeq;
}

// one wave per pattern; done[p] = its anchors that have their f and par (first: none).  f[a] = the score of anchor a, par[a] = how
// many anchors back its parent lies (1 .. 64; 0: none).  ctr[0] += patterns left unfinished
template <class I>
__global__ void __launch_bounds__(kTB) chain_dp_k(SeqArgs<I> sq, int has_seq, const uint64_t *__restrict__ anc_off, uint64_t npat,
                                                  const uint64_t *__restrict__ anc, uint64_t G, uint64_t B, uint64_t steps, int first,
                                                  uint64_t *__restrict__ done, uint32_t *__restrict__ f, uint8_t *__restrict__ par,
                                                  unsigned long long *__restrict__ ctr) {
  const int lane = threadIdx.x & 63;
  const uint64_t p = BID * (kTB / 64) + (threadIdx.x >> 6);
  if (p >= npat) return;                                // (whole waves leave: nothing below waits for another wave)
  const uint64_t b = anc_off[p], e = anc_off[p + 1], A = e > b ? e - b : 0;
  uint64_t x = first ? 0 : done[p];
  if (x >= A) {
    if (first && lane == 0) done[p] = A;
    return;
  }
  const uint64_t stop = A - x > steps ? x + steps : A;
  // the ring before anchor x: this lane holds the last anchor j < x with j = lane (mod 64); rf = 0: none (f >= 1)
  uint64_t rqe = 0, rte = 0;
  uint32_t rrec = 0, rf = 0;
  if (x > 0) {
    const uint64_t last = x - 1, back = (last - (uint64_t)lane) & 63;
    if (back <= last) {
      const Anchor y = anchor_at(anc, b + last - back);
      rqe = y.i + y.len; rte = y.t + y.len; rrec = rec_of(sq, has_seq, y.t); rf = f[b + last - back];
    }
  }
  while (x < stop) {
    const uint64_t base = x & ~63ull;
    uint64_t nqe = 0, nte = 0;                          // this lane's anchor of the 64 from base on
    uint32_t nrec = 0, nlen = 0;
    if (base + lane < A) {
      const Anchor y = anchor_at(anc, b + base + lane);
      nqe = y.i + y.len; nte = y.t + y.len; nrec = rec_of(sq, has_seq, y.t); nlen = (uint32_t)y.len;
    }
    const int k0 = (int)(x & 63), k1 = stop - base < 64 ? (int)(stop - base) : 64;
    uint32_t mypar = 0;
    for (int k = k0; k < k1; k++) {                     // anchor base + k against the ring; k is the same in every lane
      const uint64_t xqe = readlane_u64(nqe, k), xte = readlane_u64(nte, k);
      const uint32_t xrec = readlane_u32(nrec, k), xlen = readlane_u32(nlen, k);
      uint64_t key = 0;
      const uint64_t dq = xqe - rqe, dt = xte - rte;    // (a difference below 1 wraps and fails the test against G)
      if (rf && rrec == xrec && dq - 1 < G && dt - 1 < G) {
        const uint64_t g = dq > dt ? dq - dt : dt - dq;
        if (g <= B) {
          const uint64_t add = dq < dt ? (dq < xlen ? dq : xlen) : (dt < xlen ? dt : xlen);
          const int64_t cand = (int64_t)rf + (int64_t)add - (int64_t)((g + 3) >> 2);
          const int d = ((k - lane - 1) & 63) + 1;      // the held anchor lies d back
          key = (uint64_t)(cand + kBias) << 8 | (uint64_t)(64 - d);
        }
      }
      const uint64_t best = wave_max_u64(key);
      uint32_t fx = xlen, px = 0;
      if (best) {
        const int64_t cand = (int64_t)(best >> 8) - kBias;
        if (cand > (int64_t)xlen) { fx = (uint32_t)cand; px = 64 - (uint32_t)(best & 63); }
      }
      if (lane == k) { rqe = nqe; rte = nte; rrec = nrec; rf = fx; mypar = px; }
    }
    if (lane >= k0 && lane < k1) { f[b + base + lane] = rf; par[b + base + lane] = (uint8_t)mypar; }
    x = base + k1;
  }
  if (lane == 0) {
    done[p] = x;
    if (x < A) atomicAdd(&ctr[0], 1ull);
  }
}

// ---------------------------------------------------------------- the peel
// key[a] = ~f[a] above a: a pattern's anchors by (f descending, index)
__global__ void __launch_bounds__(kTB) peel_key_k(const uint32_t *__restrict__ f, uint64_t A, uint64_t *__restrict__ key) {
  const uint64_t a = BID * kTB + threadIdx.x;
  if (a >= A) return;
  key[a] = (uint64_t)(~f[a]) << 32 | a;
}

// where a pattern's peel stands: s = the next slot of its sorted segment; x = the anchor whose walk is under way (kNoAnchor:
// none), y = the anchor the walk visits next, and the walk's sums so far
struct PeelRec { uint64_t s, ts; uint32_t x, y, n, qs, match, pad; };

// one lane per pattern, at most `steps` visits and walk steps per launch.  An anchor that ends a kept chain gets score (>= 1; the
// array starts zeroed), n, qs, ts and match.  ctr[0] += patterns left unfinished
__global__ void __launch_bounds__(kTB) peel_k(const uint64_t *__restrict__ anc_off, uint64_t npat, const uint64_t *__restrict__ anc,
                                              const uint32_t *__restrict__ f, const uint8_t *__restrict__ par, const uint32_t *__restrict__ order,
                                              uint64_t S, uint64_t steps, int first, PeelRec *__restrict__ rec, uint8_t *__restrict__ visited,
                                              uint32_t *__restrict__ score, uint32_t *__restrict__ cn, uint32_t *__restrict__ cqs,
                                              uint64_t *__restrict__ cts, uint32_t *__restrict__ cmatch, unsigned long long *__restrict__ ctr) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p >= npat) return;
  const uint64_t b = anc_off[p], e0 = anc_off[p + 1], e = e0 > b ? e0 : b;
  PeelRec r = first ? PeelRec{b, 0, kNoAnchor, 0, 0, 0, 0, 0} : rec[p];
  for (uint64_t work = 0; work < steps; work++) {
    if (r.x == kNoAnchor) {
      if (r.s >= e) break;
      const uint32_t a = order[r.s++];
      if (a < b || a >= e || visited[a]) continue;      // (the sort keeps a segment's values inside it)
      r.x = r.y = a; r.n = 0; r.qs = 0xFFFFFFFFu; r.ts = ~0ull; r.match = 0;
      continue;
    }
    const uint32_t y = r.y, d = par[y];
    const Anchor ay = anchor_at(anc, y);
    visited[y] = 1;
    r.n++;
    if ((uint32_t)ay.i < r.qs) r.qs = (uint32_t)ay.i;
    if (ay.t < r.ts) r.ts = ay.t;
    const bool has = d && y >= b + d;                   // (the programme's parents lie inside the pattern)
    if (has && !visited[y - d]) {
      const Anchor az = anchor_at(anc, y - d);
      const uint64_t dq = ay.i + ay.len - (az.i + az.len), dt = ay.t + ay.len - (az.t + az.len);
      const uint64_t add = dq < dt ? (dq < ay.len ? dq : ay.len) : (dt < ay.len ? dt : ay.len);
      r.match += (uint32_t)add;
      r.y = y - d;
      continue;
    }
    r.match += (uint32_t)ay.len;
    // (the walk stopped at a visited anchor: the score is the difference, which a negative gain can take below 1)
    const int64_t sc = (int64_t)f[r.x] - (has ? (int64_t)f[y - d] : 0);
    if (sc >= 1 && (uint64_t)sc >= S) { score[r.x] = (uint32_t)sc; cn[r.x] = r.n; cqs[r.x] = r.qs; cts[r.x] = r.ts; cmatch[r.x] = r.match; }
    r.x = kNoAnchor;
  }
  rec[p] = r;
  if (r.x != kNoAnchor || r.s < e) atomicAdd(&ctr[0], 1ull);
}

// key[a] = ~score[a] above a for the last anchor of a kept chain, else kNoKey: a pattern's chains by (score descending, te, qe)
__global__ void __launch_bounds__(kTB) chain_key_k(const uint32_t *__restrict__ score, uint64_t A, uint64_t *__restrict__ key) {
  const uint64_t a = BID * kTB + threadIdx.x;
  if (a >= A) return;
  key[a] = !score[a] ? kNoKey : ((uint64_t)(~score[a]) << 32 | a);
}

// one lane per segment (entry nseg: 0) of sorted keys: the keys before the first kNoKey, at most cap of them (0: all)
__global__ void __launch_bounds__(kTB) front_count_k(const uint64_t *__restrict__ key, uint64_t A, const uint32_t *__restrict__ sb,
                                                     const uint32_t *__restrict__ se, uint64_t nseg, uint64_t cap, uint64_t *__restrict__ cnt) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p > nseg) return;
  if (p == nseg) { cnt[p] = 0; return; }
  uint64_t b = sb[p], e = se[p];
  if (e > A) e = A;
  if (b > e) b = e;
  uint64_t lo = b, hi = e;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (key[mid] != kNoKey) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t k = lo - b;
  cnt[p] = cap && k > cap ? cap : k;
}

// one lane per chain c < C: the (c - chain_off[p])-th of its pattern's sorted segment
__global__ void __launch_bounds__(kTB) chain_write_k(const uint64_t *__restrict__ chain_off, uint64_t npat, uint64_t C, const uint32_t *__restrict__ sb,
                                                     const uint32_t *__restrict__ order, uint64_t A, const uint64_t *__restrict__ anc,
                                                     const uint32_t *__restrict__ score, const uint32_t *__restrict__ cn,
                                                     const uint32_t *__restrict__ cqs, const uint64_t *__restrict__ cts,
                                                     const uint32_t *__restrict__ cmatch, ChainOut out) {
  const uint64_t c = BID * kTB + threadIdx.x;
  if (c >= C) return;
  const uint64_t p = last_le(chain_off, npat, c), slot = sb[p] + (c - chain_off[p]);
  const uint64_t x = slot < A ? order[slot] : A;
  if (x >= A) return;
  const Anchor a = anchor_at(anc, x);
  out.score[c] = score[x]; out.n[c] = cn[x]; out.qs[c] = cqs[x]; out.qe[c] = (uint32_t)(a.i + a.len);
  out.ts[c] = cts[x]; out.te[c] = a.t + a.len; out.match[c] = cmatch[x];
}

// ---------------------------------------------------------------- long reads
// sb[r], se[r] = the segment of read r among the chains of the 2 npat strands; key[c] = ~score[c] above c
__global__ void __launch_bounds__(kTB) long_keys_k(const uint64_t *__restrict__ chain_off, uint64_t npat, const uint32_t *__restrict__ score,
                                                   uint64_t C, uint32_t *__restrict__ sb, uint32_t *__restrict__ se, uint64_t *__restrict__ key,
                                                   uint32_t *__restrict__ val) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i < npat) { sb[i] = (uint32_t)chain_off[2 * i]; se[i] = (uint32_t)chain_off[2 * i + 2]; }
  if (i < C) { key[i] = (uint64_t)(~score[i]) << 32 | i; val[i] = (uint32_t)i; }
}

// one lane per read r (entry npat: cnt = 0) over the sorted segments: nchains, mapq, and what is returned
__global__ void __launch_bounds__(kTB) long_reads_k(const uint32_t *__restrict__ order, const uint32_t *__restrict__ score, uint64_t C,
                                                    const uint32_t *__restrict__ sb, const uint32_t *__restrict__ se, uint64_t npat, uint64_t max_sec,
                                                    uint64_t *__restrict__ nchains, uint8_t *__restrict__ mapq, uint64_t *__restrict__ cnt) {
  const uint64_t r = BID * kTB + threadIdx.x;
  if (r > npat) return;
  if (r == npat) { cnt[r] = 0; return; }
  uint64_t b = sb[r], e = se[r];
  if (e > C) e = C;
  if (b > e) b = e;
  const uint64_t nc = e - b;
  uint32_t q = 0;
  if (nc == 1) q = 60;
  else if (nc > 1) {
    const uint64_t s1 = score[order[b]], s2 = score[order[b + 1]];      // (s1 >= s2 >= 1: the order of the keys)
    q = (uint32_t)(60 * (s1 - s2) / s1);
    if (q > 60) q = 60;
  }
  nchains[r] = nc;
  mapq[r] = (uint8_t)q;
  cnt[r] = max_sec < nc ? max_sec + 1 : nc;
}

struct LongChains {
  const uint64_t *chain_off, *ts, *te;
  const uint32_t *score, *n, *qs, *qe, *match, *order;
};
// one lane per returned chain h < H: the (h - hit_off[r])-th of its read's sorted segment
template <class I>
__global__ void __launch_bounds__(kTB) long_hits_k(SeqArgs<I> sq, int has_seq, LongChains ch, uint64_t C, const uint64_t *__restrict__ pat2_off,
                                                   const uint64_t *__restrict__ hit_off, uint64_t npat, uint64_t H, LongOut out) {
  const uint64_t h = BID * kTB + threadIdx.x;
  if (h >= H) return;
  const uint64_t r = last_le(hit_off, npat, h), slot = ch.chain_off[2 * r] + (h - hit_off[r]);
  const uint64_t c = slot < C ? ch.order[slot] : C;
  if (c >= C) return;
  const uint32_t strand = c >= ch.chain_off[2 * r + 1];
  const uint64_t ts = ch.ts[c], m = pat2_off[2 * r + 1] - pat2_off[2 * r];
  uint32_t q = 0;
  uint64_t o = ts;
  if (has_seq) {
    q = kNoSeq; o = ~0ull;
    if (ts < sq.n) { q = seq_of(sq, ts); o = ts - (uint64_t)sq.start[q]; }
  }
  out.strand[h] = (uint8_t)strand; out.seq[h] = q; out.off[h] = o; out.ts[h] = ts; out.te[h] = ch.te[c];
  out.qs[h] = strand ? (uint32_t)(m - ch.qe[c]) : ch.qs[c];
  out.qe[h] = strand ? (uint32_t)(m - ch.qs[c]) : ch.qe[c];
  out.score[h] = ch.score[c]; out.n[h] = ch.n[c]; out.match[h] = ch.match[c];
}

}  // namespace

void fm_anchors_check(const FmIndex &f, uint64_t min_seed, uint64_t max_occ, bool thresholds) {
  require_text(f, "anchors");
  require_samples(f);
  PFP_REQUIRE(min_seed >= 1, PFP_EINVAL, "min_seed = 0: a seed is a maximal exact match of at least 1 byte");
  PFP_REQUIRE(max_occ >= 1 && max_occ <= 65536, PFP_EINVAL, "max_occ = " + std::to_string(max_occ) + ": the repeat filter takes 1 .. 65536");
  PFP_REQUIRE(!thresholds || f.has_thr, PFP_EINVAL, "this index has no thresholds: add them with pfp_fm_thresholds_dev / pfp_fm_thresholds_files");
}

void fm_chain_check(const FmIndex &f, uint64_t max_gap, uint64_t band, uint64_t min_score) {
  require_text(f, "chains");
  require_samples(f);
  PFP_REQUIRE(max_gap >= 1 && max_gap < (1ull << 31), PFP_EINVAL, "max_gap = " + std::to_string(max_gap) + ": 1 .. 2^31 - 1");
  PFP_REQUIRE(band >= 1 && band < (1ull << 31), PFP_EINVAL, "band = " + std::to_string(band) + ": 1 .. 2^31 - 1");
  PFP_REQUIRE(min_score >= 1, PFP_EINVAL, "min_score = 0: a chain scores at least 1");
}

uint64_t fm_anchors_ms(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                       const uint32_t *len, const uint64_t *pos, const uint64_t *mem_off, uint64_t M, uint64_t *anc_off, DBuf<uint64_t> &anc,
                       uint32_t *skipped) {
  pfp_ctx *c = f.c;
  if (skipped && npat) PFP_HIP(hipMemsetAsync(skipped, 0, npat * sizeof(uint32_t), c->stream));
  if (!npat || !M) {
    PFP_HIP(hipMemsetAsync(anc_off, 0, (npat + 1) * sizeof(uint64_t), c->stream));
    anc.alloc(c, 0);
    sync(c);
    return 0;
  }
  DBuf<uint64_t> mem(c, 3 * M), rng(c, 4 * M), occ_off(c, M + 1), spans(c, 2 * M);
  uint64_t *sp = rng.p, *ep = sp + M, *first = ep + M, *cep = first + M;
  fm_mem_triples(f, pat_off, npat, len, pos, min_seed, mem_off, mem.p);
  {
    KScope ks(c, "fm_anchor_spans", 0);
    anc_spans_k<<<gdim(cdiv(M, kTB)), kTB, 0, c->stream>>>(pat_off, npat, mem_off, mem.p, M, spans.p, spans.p + M);
    PFP_HIP(hipGetLastError());
  }
  fm_count_spans(f, pat, spans.p, spans.p + M, M, sp, ep, first);
  {
    KScope ks(c, "fm_anchor_spans", 0);
    anc_clip_k<<<gdim(cdiv(M, kTB)), kTB, 0, c->stream>>>(sp, ep, M, max_occ, mem_off, npat, cep, skipped);
    PFP_HIP(hipGetLastError());
  }
  uint64_t O = 0;
  {
    KScope ks(c, "fm_anchor_locate", 0);
    fm_locate(f, M, sp, cep, first, 0, occ_off.p, nullptr);
    O = read_scalar(c, occ_off.p + M);
  }
  require_sortable(O, "anchors");
  if (!O) {
    PFP_HIP(hipMemsetAsync(anc_off, 0, (npat + 1) * sizeof(uint64_t), c->stream));
    anc.alloc(c, 0);
    sync(c);
    return 0;
  }
  DBuf<uint64_t> occ(c, O), tek(c, O), key(c, O), skey(c, O), seg_off(c, npat + 1), cnt(c, npat + 1);
  DBuf<uint32_t> sb(c, npat), se(c, npat), val(c, O), order(c, O);
  {
    KScope ks(c, "fm_anchor_locate", 0);
    fm_locate(f, M, sp, cep, first, 0, occ_off.p, occ.p);
  }
  const uint64_t drop = f.wide ? 1ull << 40 : 0xFFFFFFFFull;    // above every t + len <= n: n < 2^40, and n < 2^32 - 1 in a narrow index
  {
    KScope ks(c, "fm_anchor_sort", 0);
    by_width(f, [&](auto w) {
      using I = decltype(w);
      anc_ends_k<I><<<gdim(cdiv(O, kTB)), kTB, 0, c->stream>>>(seq_args<I>(f), f.nseq != 0, occ_off.p, M, mem.p, occ.p, O, drop, tek.p);
    });
    PFP_HIP(hipGetLastError());
    seg_bounds_k<uint32_t><<<gdim(cdiv(std::max(npat, O), kTB)), kTB, 0, c->stream>>>(mem_off, npat, occ_off.p, sb.p, se.p, nullptr, val.p, O);
    PFP_HIP(hipGetLastError());
    gather_off_k<uint64_t><<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(mem_off, npat, occ_off.p, M, seg_off.p);
    PFP_HIP(hipGetLastError());
    for (int shift = 0; shift < (f.wide ? 64 : 32); shift += 32) {
      anc_key_k<<<gdim(cdiv(O, kTB)), kTB, 0, c->stream>>>(tek.p, val.p, O, shift, key.p);
      PFP_HIP(hipGetLastError());
      segsort_pairs_u64_u32(c, key.p, skey.p, val.p, order.p, O, npat, sb.p, se.p, 0, 64);
      std::swap(val, order);                            // (the next pass, and what follows, read the order in val)
    }
    anc_count_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(tek.p, val.p, O, sb.p, se.p, npat, drop, cnt.p);
    PFP_HIP(hipGetLastError());
    exclusive_sum_u64(c, cnt.p, anc_off, npat + 1);
  }
  const uint64_t total = read_scalar(c, anc_off + npat);
  anc.alloc(c, 3 * total);
  if (total) {
    KScope ks(c, "fm_anchor_sort", 0);
    anc_write_k<<<gdim(cdiv(O, kTB)), kTB, 0, c->stream>>>(tek.p, val.p, O, seg_off.p, npat, occ_off.p, M, mem.p, occ.p, drop, anc_off, total, anc.p);
    PFP_HIP(hipGetLastError());
  }
  sync(c);                                              // (the scratch goes back when this returns)
  return total;
}

uint64_t fm_anchors(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ, bool thresholds,
                    uint64_t *anc_off, DBuf<uint64_t> &anc, uint32_t *skipped) {
  pfp_ctx *c = f.c;
  fm_anchors_check(f, min_seed, max_occ, thresholds);
  if (!npat) return fm_anchors_ms(f, pat, pat_off, 0, min_seed, max_occ, nullptr, nullptr, nullptr, 0, anc_off, anc, skipped);
  const uint64_t bytes = read_scalar(c, pat_off + npat);
  DBuf<uint32_t> len(c, bytes + 1);
  DBuf<uint64_t> pos(c, bytes + 1), mem_off(c, npat + 1);
  (thresholds ? fm_ms_thr : fm_ms)(f, pat, pat_off, npat, len.p, pos.p);
  fm_mems(f, pat_off, npat, len.p, pos.p, min_seed, mem_off.p, nullptr);
  const uint64_t M = read_scalar(c, mem_off.p + npat);
  return fm_anchors_ms(f, pat, pat_off, npat, min_seed, max_occ, len.p, pos.p, mem_off.p, M, anc_off, anc, skipped);
}

void fm_chains_run(FmIndex &f, const uint64_t *anc_off, const uint64_t *anc, uint64_t npat, uint64_t max_gap, uint64_t band, uint64_t min_score,
                   uint64_t max_chains, uint64_t *chain_off, ChainSel &sel) {
  pfp_ctx *c = f.c;
  fm_chain_check(f, max_gap, band, min_score);
  sel.total = 0;
  if (!npat) {
    PFP_HIP(hipMemsetAsync(chain_off, 0, sizeof(uint64_t), c->stream));
    sync(c);
    return;
  }
  DBuf<uint64_t> ctr(c, 4);
  uint64_t h[4];
  ctr.zero();
  chain_offsets_k<<<gdim(cdiv(npat, kTB)), kTB, 0, c->stream>>>(anc_off, npat, (unsigned long long *)ctr.p);
  PFP_HIP(hipGetLastError());
  d2h(c, h, ctr.p, 4);
  sync(c);
  PFP_REQUIRE(!h[0], PFP_EINVAL, std::to_string(h[0]) + " anchor offsets decrease");
  const uint64_t A = h[1];
  require_sortable(A, "anchors");
  PFP_REQUIRE(!A || anc, PFP_EINVAL, "no anchors");
  if (A) {
    PFP_HIP(hipMemsetAsync(ctr.p, 0xFF, sizeof(uint64_t), c->stream));
    chain_check_k<<<gdim(cdiv(A, kTB)), kTB, 0, c->stream>>>(anc_off, npat, anc, A, (unsigned long long *)ctr.p);
    PFP_HIP(hipGetLastError());
    const uint64_t bad = read_scalar(c, ctr.p);
    PFP_REQUIRE(bad == ~0ull, PFP_EINVAL, "anchor " + std::to_string(bad) + ": an anchor has len >= 1 and i + len < 2^32, and a pattern's anchors "
                                          "strictly increase by (t + len, i + len)");
  }
  const uint64_t steps = chain_steps_from_env();
  DBuf<uint32_t> fs(c, A), se(c, npat), val(c, A), order(c, A);
  DBuf<uint8_t> visited(c, A);
  DBuf<uint8_t> &par = sel.par;
  par.alloc(c, A);
  DBuf<uint64_t> key(c, A), skey(c, A), cnt(c, npat + 1);
  sel.score.alloc(c, A); sel.n.alloc(c, A); sel.qs.alloc(c, A); sel.match.alloc(c, A); sel.ts.alloc(c, A);
  sel.order.alloc(c, A); sel.sb.alloc(c, npat);
  {
    DBuf<uint64_t> done(c, npat);
    by_width(f, [&](auto w) {
      using I = decltype(w);
      const SeqArgs<I> sq = seq_args<I>(f);
      bounded_launches(c, "fm_chain_dp", ctr, [&](int first, unsigned long long *d_ctr) {
        chain_dp_k<I><<<gdim(cdiv(npat, kTB / 64)), kTB, 0, c->stream>>>(sq, f.nseq != 0, anc_off, npat, anc, max_gap, band, steps, first, done.p, fs.p,
                                                                         par.p, d_ctr);
      }, [](const uint64_t *) {});
    });
  }
  {
    KScope ks(c, "fm_chain_sort", 0);
    seg_bounds_k<uint32_t><<<gdim(cdiv(std::max(npat, A), kTB)), kTB, 0, c->stream>>>(anc_off, npat, nullptr, sel.sb.p, se.p, nullptr, val.p, A);
    PFP_HIP(hipGetLastError());
    if (A) {
      peel_key_k<<<gdim(cdiv(A, kTB)), kTB, 0, c->stream>>>(fs.p, A, key.p);
      PFP_HIP(hipGetLastError());
      segsort_pairs_u64_u32(c, key.p, skey.p, val.p, order.p, A, npat, sel.sb.p, se.p, 0, 64);
    }
  }
  visited.zero();
  sel.score.zero();
  {
    DBuf<PeelRec> rec(c, npat);
    bounded_launches(c, "fm_chain_peel", ctr, [&](int first, unsigned long long *d_ctr) {
      peel_k<<<gdim(cdiv(npat, kTB)), kTB, 0, c->stream>>>(anc_off, npat, anc, fs.p, par.p, order.p, min_score, steps, first, rec.p, visited.p,
                                                           sel.score.p, sel.n.p, sel.qs.p, sel.ts.p, sel.match.p, d_ctr);
    }, [](const uint64_t *) {});
  }
  KScope ks(c, "fm_chain_sort", 0);
  if (A) {
    chain_key_k<<<gdim(cdiv(A, kTB)), kTB, 0, c->stream>>>(sel.score.p, A, key.p);
    PFP_HIP(hipGetLastError());
    segsort_pairs_u64_u32(c, key.p, skey.p, val.p, sel.order.p, A, npat, sel.sb.p, se.p, 0, 64);
  }
  front_count_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(skey.p, A, sel.sb.p, se.p, npat, max_chains, cnt.p);
  PFP_HIP(hipGetLastError());
  exclusive_sum_u64(c, cnt.p, chain_off, npat + 1);
  sel.total = read_scalar(c, chain_off + npat);         // (syncs: the scratch goes back when this returns)
}

void fm_chains_write(FmIndex &f, const uint64_t *anc, uint64_t npat, const uint64_t *chain_off, const ChainSel &sel, const ChainOut &out) {
  pfp_ctx *c = f.c;
  if (!sel.total) return;
  KScope ks(c, "fm_chain_write", 0);
  chain_write_k<<<gdim(cdiv(sel.total, kTB)), kTB, 0, c->stream>>>(chain_off, npat, sel.total, sel.sb.p, sel.order.p, sel.order.n, anc, sel.score.p,
                                                                   sel.n.p, sel.qs.p, sel.ts.p, sel.match.p, out);
  PFP_HIP(hipGetLastError());
}

void fm_map_long_select(FmIndex &f, const uint64_t *anc_off2, const uint64_t *anc, uint64_t npat, uint64_t max_gap, uint64_t band,
                        uint64_t min_score, uint64_t max_sec, uint64_t *hit_off, uint8_t *mapq, uint64_t *nchains, LongSel &sel) {
  pfp_ctx *c = f.c;
  sel.H = 0;
  if (!npat) {
    PFP_HIP(hipMemsetAsync(hit_off, 0, sizeof(uint64_t), c->stream));
    sync(c);
    return;
  }
  sel.chain_off.alloc(c, 2 * npat + 1);
  {
    ChainSel gone, &cs = sel.keep ? sel.cs : gone;
    fm_chains_run(f, anc_off2, anc, 2 * npat, max_gap, band, min_score, 0, sel.chain_off.p, cs);
    const uint64_t C = cs.total;
    require_sortable(C, "chains");
    sel.score.alloc(c, C); sel.n.alloc(c, C); sel.qs.alloc(c, C); sel.qe.alloc(c, C); sel.match.alloc(c, C);
    sel.ts.alloc(c, C); sel.te.alloc(c, C); sel.order.alloc(c, C);
    fm_chains_write(f, anc, 2 * npat, sel.chain_off.p, cs, ChainOut{sel.score.p, sel.n.p, sel.qs.p, sel.qe.p, sel.ts.p, sel.te.p, sel.match.p});
    sync(c);
  }
  const uint64_t C = sel.score.n;
  DBuf<uint32_t> sb(c, npat), se(c, npat), val(c, C);
  DBuf<uint64_t> key(c, C), skey(c, C), cnt(c, npat + 1);
  KScope ks(c, "fm_long_select", 0);
  long_keys_k<<<gdim(cdiv(std::max(npat, C), kTB)), kTB, 0, c->stream>>>(sel.chain_off.p, npat, sel.score.p, C, sb.p, se.p, key.p, val.p);
  PFP_HIP(hipGetLastError());
  segsort_pairs_u64_u32(c, key.p, skey.p, val.p, sel.order.p, C, npat, sb.p, se.p, 0, 64);
  long_reads_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(sel.order.p, sel.score.p, C, sb.p, se.p, npat, max_sec, nchains, mapq, cnt.p);
  PFP_HIP(hipGetLastError());
  exclusive_sum_u64(c, cnt.p, hit_off, npat + 1);
  sel.H = read_scalar(c, hit_off + npat);               // (syncs: the scratch of the sort goes back when this returns)
}

void fm_map_long_fill(FmIndex &f, const uint64_t *pat2_off, uint64_t npat, const uint64_t *hit_off, const LongSel &sel, const LongOut &out) {
  pfp_ctx *c = f.c;
  if (!sel.H) return;
  KScope ks(c, "fm_long_hits", 0);
  const LongChains ch{sel.chain_off.p, sel.ts.p, sel.te.p, sel.score.p, sel.n.p, sel.qs.p, sel.qe.p, sel.match.p, sel.order.p};
  by_width(f, [&](auto w) {
    using I = decltype(w);
    long_hits_k<I><<<gdim(cdiv(sel.H, kTB)), kTB, 0, c->stream>>>(seq_args<I>(f), f.nseq != 0, ch, sel.score.n, pat2_off, hit_off, npat, sel.H, out);
  });
  PFP_HIP(hipGetLastError());
}

void fm_map_long(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ, uint64_t max_gap,
                 uint64_t band, uint64_t min_score, uint64_t max_sec, bool thresholds, uint64_t *hit_off, uint8_t *mapq, uint64_t *nchains,
                 const LongOut *out, const LongAln *aln) {
  pfp_ctx *c = f.c;
  fm_anchors_check(f, min_seed, max_occ, thresholds);
  fm_chain_check(f, max_gap, band, min_score);
  if (aln) fm_fill_check(f, aln->max_fill);
  LongSel sel;
  sel.keep = aln != nullptr;
  fm_map_strands(f, pat, pat_off, npat, sel.rd, true);
  DBuf<uint64_t> anc_off(c, 2 * npat + 1), anc;
  fm_anchors(f, sel.rd.pat.p, sel.rd.off.p, 2 * npat, min_seed, max_occ, thresholds, anc_off.p, anc, nullptr);
  fm_map_long_select(f, anc_off.p, anc.p, npat, max_gap, band, min_score, max_sec, hit_off, mapq, nchains, sel);
  if (out) fm_map_long_fill(f, sel.rd.off.p, npat, hit_off, sel, *out);
  if (aln && npat) {
    ChainAln st;
    fm_map_long_align(f, sel.rd.pat.p, sel.rd.off.p, npat, anc_off.p, anc.p, hit_off, sel, aln->max_fill, aln->out, aln->cig_off, st);
    if (aln->cig) fm_chain_align_write(f, st, aln->cig_off, aln->cig);
    sync(c);                                            // (the gaps and their runs go back when this returns)
  } else if (aln) {
    PFP_HIP(hipMemsetAsync(aln->cig_off, 0, sizeof(uint64_t), c->stream));
  }
  sync(c);
}

}  // namespace pfp
