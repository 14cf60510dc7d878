// fmsearch.hip -- counting and locating patterns over a .bwt and its run samples (.ssa / .esa): the r-index of Gagie, Navarro
// and Prezza, "Optimal-time text indexing in BWT-runs bounded space" (SODA 2018), with the plain BWT bytes for rank.  The
// reference has no counterpart; the paper is the source.  Conventions: include/pfpgpu.h (rows j = 0..n, SA[0] = n).
//
//   Rank.  The symbols present (bytes other than 0) get dense codes.  The BWT is cut into 256-row blocks and 65536-row
//   superblocks; sbc[superblock][k] = C[c] + occurrences of c before the superblock (u64), blk[block][k] = occurrences before
//   the block inside its superblock (u16).  LF(i, c) = C[c] + rank_c(i) = sbc + blk + the c's among the first i & 255 bytes of
//   i's block, which a group of 16 lanes counts from one contiguous 256-byte read (16 bytes per lane, a SWAR compare, a masked
//   popcount and a group sum): "lanes per item matched to the item".
//   Count.  One group of 16 lanes per pattern runs backward search from [0, n+1): sp' = LF(sp, c), ep' = LF(ep, c), at most m
//   steps.  With samples it keeps the toehold SA[sp]: toehold - 1 if BWT[sp] = c, else SA[j] - 1 for the first c in [sp, ep),
//   a run start j (BWT[j-1] != c) found by a select (binary search over the block directory, then the 16 lanes of one block),
//   whose SA value is the run-start sample of rank j in the run-start bitmap.
//   Locate.  The run starts inside [sp, sp + cap) cut the range into segments whose first SA value is known (the toehold, or a
//   run-start sample); inside a segment SA[j+1] = phi^-1(SA[j]) = SA[s_{i+1}] + (SA[j] - SA[e_i]) with SA[e_i] the largest
//   run-end sample <= SA[j].  Plan (segments and positions per pattern) -> library scans -> expand (one lane per segment:
//   pattern by binary search, start row and value, output slot out_off[p] + row - sp) -> chains, one lane per segment, at
//   most kChainSteps steps per launch; the predecessor search reads a bucket directory over text positions, then at most
//   log2 of the bucket's keys.
//   Matching statistics (PHONI: Boucher, Gagie, I, Koppl, Langmead, Manzini, Navarro, Pacheco, Rossi, DCC 2021, after Bannai,
//   Gagie, I, "Refining the r-index", 2020).  An index built with the text also keeps SA[run end] by run number.  One group of
//   16 lanes per pattern walks it right to left with (q, pos, l), SA[q] = pos, T[pos .. pos+l) = P[i+1 .. i+1+l).  BWT[q] = c:
//   one LF.  Otherwise the c just before q ends a run and the c just after q starts one, so both SA values are samples; the
//   longer common extension with T[pos ..) wins (the predecessor on a tie), compared on the text 1024 bytes per group and
//   iteration.  A launch gives every pattern kMsWork units (one per step and per LCE iteration) and leaves (i, q, pos, l) in a
//   32-byte record; the host launches until no pattern is unfinished.  The answers depend on the inputs only.
//   MEMs.  (i, len[i], pos[i]) with len[i] >= min_len and (i = 0 or len[i-1] <= len[i]): counted per pattern by its group, a
//   library scan, then gathered in order of i.
// Bounds: every loop is bounded by the pattern length, a directory's size, kChainSteps or a launch's budget; values read from
// the samples or the text only ever become output values or are clamped before they index anything.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"

namespace pfp {

namespace {

constexpr int kHistBlocks = 16;             // rank blocks per wave of the directory build
constexpr uint64_t kChainSteps = 16384;     // phi^-1 steps per chain and launch

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void atomic_min_u64(uint64_t *p, uint64_t v) { atomicMin((unsigned long long *)p, (unsigned long long)v); }
__device__ __forceinline__ void atomic_max_u64(uint64_t *p, uint64_t v) { atomicMax((unsigned long long *)p, (unsigned long long)v); }

// ---------------------------------------------------------------- directory build
// hist[c] += occurrences of byte c (per-wave LDS histograms)
__global__ void __launch_bounds__(kTB) fm_bytehist(const uint8_t *__restrict__ bwt, uint64_t n1, unsigned long long *__restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t lo = BID * 16384, hi = lo + 16384 < n1 ? lo + 16384 : n1;
  for (uint64_t x = lo + 16 * (uint64_t)threadIdx.x; x < hi; x += 16 * kTB) {
    const uint4 v = ld16u(bwt + x);      // (the copy is padded: whole 16-byte words are in bounds)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 16; q++)
      if (x + q < hi) atomicAdd(&h[(w[q >> 2] >> (8 * (q & 3))) & 255], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// cnt[b * sigma + k] = occurrences of code k in rank block b; one wave per kHistBlocks blocks, 4 bytes per lane
__global__ void __launch_bounds__(kTB) fm_blockhist(const uint8_t *__restrict__ bwt, uint64_t n1, uint64_t nb, const uint8_t *__restrict__ codes,
                                                    int sigma, uint16_t *__restrict__ cnt) {
  __shared__ uint32_t h[kTB / 64][256];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t b0 = (BID * (kTB / 64) + wv) * kHistBlocks;
  if (b0 >= nb) return;                                 // (no block-wide barrier below: every wave works alone)
  const uint64_t b1 = b0 + kHistBlocks < nb ? b0 + kHistBlocks : nb;
  for (uint64_t b = b0; b < b1; b++) {
    for (int i = lane; i < 256; i += 64) h[wv][i] = 0;
    wave_sync();
    const uint64_t r = (b << kBlkLog) + 4 * (uint64_t)lane;
    const uint32_t w = *reinterpret_cast<const uint32_t *>(bwt + r);
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (r + q < n1) atomicAdd(&h[wv][(w >> (8 * q)) & 255], 1u);
    wave_sync();
    for (int k = lane; k < sigma; k += 64) cnt[b * sigma + k] = (uint16_t)h[wv][codes[256 + k]];
    wave_sync();
  }
}

// in place: cnt[b * sigma + k] -> occurrences of code k in the blocks of b's superblock before b; tot[k * ns + s] = the superblock's
__global__ void __launch_bounds__(kTB) fm_blockscan(uint16_t *__restrict__ cnt, uint64_t nb, uint64_t ns, int sigma, uint64_t *__restrict__ tot) {
  const uint64_t t = BID * kTB + threadIdx.x;
  if (t >= ns * sigma) return;
  const uint64_t s = t / sigma, k = t % sigma;
  const uint64_t b0 = s * kBlkPerSb, b1 = b0 + kBlkPerSb < nb ? b0 + kBlkPerSb : nb;
  uint32_t run = 0;
  for (uint64_t b = b0; b < b1; b++) {
    const uint32_t x = cnt[b * sigma + k];
    cnt[b * sigma + k] = (uint16_t)run;
    run += x;
  }
  tot[k * ns + s] = run;
}

// sbc[s * sigma + k] = base[k * ns + s] + 1: the symbol-major exclusive sum counts the bytes of smaller codes, + 1 for the 0
__global__ void __launch_bounds__(kTB) fm_sbc(const uint64_t *__restrict__ base, uint64_t ns, int sigma, uint64_t *__restrict__ sbc) {
  const uint64_t t = BID * kTB + threadIdx.x;
  if (t >= ns * sigma) return;
  const uint64_t s = t / sigma, k = t % sigma;
  sbc[t] = base[k * ns + s] + 1;
}

// ---------------------------------------------------------------- samples
// pair i of .ssa / .esa: its row must be the i-th run start / end (bit set, rank i); the smallest bad pair index meets in
// bad[0] / bad[1].  rs_row / rs_sa: the run starts; key / val: the phi^-1 table SA[e_i] -> SA[s_{i+1}], i < runs - 1;
// re_sa (may be NULL): SA[e_i]
template <class I>
__global__ void __launch_bounds__(kTB) fm_pairs(const uint8_t *__restrict__ ssa, const uint8_t *__restrict__ esa, uint64_t runs, uint64_t n1,
                                                const uint64_t *__restrict__ sbits, const uint64_t *__restrict__ sdir, const uint64_t *__restrict__ ebits,
                                                const uint64_t *__restrict__ edir, I *__restrict__ rs_row, I *__restrict__ rs_sa, I *__restrict__ key,
                                                I *__restrict__ val, I *__restrict__ re_sa, uint64_t *__restrict__ bad) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i >= runs) return;
  const uint64_t bytes = 10 * runs;
  const uint64_t js = ld5(ssa, 10 * i, bytes), vs = ld5(ssa, 10 * i + 5, bytes);
  const uint64_t je = ld5(esa, 10 * i, bytes), ve = ld5(esa, 10 * i + 5, bytes);
  if (js >= n1 || !((sbits[js >> 6] >> (js & 63)) & 1) || bit_rank(sbits, sdir, js) != i) atomic_min_u64(&bad[0], i);
  if (je >= n1 || !((ebits[je >> 6] >> (je & 63)) & 1) || bit_rank(ebits, edir, je) != i) atomic_min_u64(&bad[1], i);
  rs_row[i] = (I)js;
  rs_sa[i] = (I)vs;
  if (re_sa) re_sa[i] = (I)ve;                         // (an index with text: SA[run end] by run number)
  if (i + 1 < runs) {
    key[i] = (I)ve;
    val[i] = (I)ld5(ssa, 10 * (i + 1) + 5, bytes);
  }
}

// ---------------------------------------------------------------- searches
// one group of 16 lanes per pattern: pat[off[p] .. off[p + 1]), or pat[off[p] .. end[p]) where end is given
template <class I>
__global__ void __launch_bounds__(kTB) fm_count_k(FmArgs<I> a, const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off,
                                                  const uint64_t *__restrict__ end, uint64_t npat, uint64_t *__restrict__ sp_out,
                                                  uint64_t *__restrict__ ep_out, uint64_t *__restrict__ first_out) {
  __shared__ uint8_t code[256];
  PatGroup g;
  if (!pat_group(code, a.codes, off, npat, g, end)) return;
  const int gl = g.gl;
  const uint64_t p = g.p, o0 = g.o0, o1 = g.o1;
  uint64_t sp = 0, ep = o1 < o0 ? 0 : a.n1, first = a.n1 - 1;      // (decreasing offsets: no pattern, no occurrence)
  for (uint64_t t = o1; t > o0 && sp < ep;) {           // at most m = o1 - o0 steps
    t--;
    const uint32_t c = pat[t], k = code[c];
    if (k == kAbsent) { ep = sp; break; }               // (byte 0 has no code: a pattern holding it has no occurrence)
    const uint32_t c4 = c * 0x01010101u;
    const uint64_t nsp = lf_at(a, sp, c4, k, gl), nep = lf_at(a, ep, c4, k, gl);
    if (first_out && nep > nsp) first = toehold_step(a, sp, ep, nsp, first, c, c4, k, gl);
    sp = nsp; ep = nep;
  }
  if (ep <= sp) { sp = ep = 0; first = ~0ull; }
  if (gl == 0) {
    sp_out[p] = sp; ep_out[p] = ep;
    if (first_out) first_out[p] = first;
  }
}

// run starts in rows [0, x), 0 <= x <= n1
template <class I>
__device__ __forceinline__ uint64_t starts_before(const FmArgs<I> &a, uint64_t x) { return x >= a.n1 ? a.runs : bit_rank(a.rbits, a.rdir, x); }

// per pattern: positions cap = min(ep - sp, max_occ), segments 1 + run starts in (sp, sp + cap), q0 = rank of the first of them
template <class I>
__global__ void __launch_bounds__(kTB) fm_plan(FmArgs<I> a, uint64_t npat, const uint64_t *__restrict__ sp, const uint64_t *__restrict__ ep,
                                               uint64_t max_occ, uint64_t *__restrict__ npos, uint64_t *__restrict__ nseg, uint64_t *__restrict__ q0) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p > npat) return;
  uint64_t cap = 0, segs = 0, q = 0;
  if (p < npat) {
    const uint64_t s = sp[p], e = ep[p];
    cap = e <= a.n1 && s < e ? e - s : 0;
    if (max_occ && cap > max_occ) cap = max_occ;
    if (cap && nseg) {
      q = starts_before(a, s + 1);
      segs = 1 + starts_before(a, s + cap) - q;
    }
  }
  npos[p] = cap;                                       // (entry npat = 0: the exclusive sums end with the totals)
  if (nseg) { nseg[p] = segs; q0[p] = q; }
}

struct Seg { uint64_t x, slot, rem; };

// one lane per segment: its pattern (binary search over seg_off), start row and SA value, output slot and length
template <class I>
__global__ void __launch_bounds__(kTB) fm_expand(FmArgs<I> a, uint64_t npat, uint64_t S, const uint64_t *__restrict__ seg_off,
                                                 const uint64_t *__restrict__ nseg, const uint64_t *__restrict__ q0, const uint64_t *__restrict__ npos,
                                                 const uint64_t *__restrict__ out_off, const uint64_t *__restrict__ sp, const uint64_t *__restrict__ first,
                                                 Seg *__restrict__ seg, uint64_t *__restrict__ maxlen) {
  const uint64_t g = BID * kTB + threadIdx.x;
  if (g >= S) return;
  const uint64_t p = last_le(seg_off, npat, g), k = g - seg_off[p], s = sp[p];
  uint64_t row = s, x = first[p];
  if (k) { row = a.rs_row[q0[p] + k - 1]; x = a.rs_sa[q0[p] + k - 1]; }
  const uint64_t end = k + 1 < nseg[p] ? (uint64_t)a.rs_row[q0[p] + k] : s + npos[p];
  const uint64_t len = end > row ? end - row : 0;
  seg[g] = Seg{x, out_off[p] + (row - s), len};
  atomic_max_u64(maxlen, len);
}

// SA[j + 1] from x = SA[j] (j not the last row of a run): the largest key <= x, searched in x's bucket
template <class I>
__device__ __forceinline__ uint64_t phi_inv(const FmArgs<I> &a, uint64_t x) {
  uint64_t b = x >> a.shift;
  if (b >= a.nbk) b = a.nbk - 1;
  uint64_t lo = a.dir[b], hi = a.dir[b + 1];           // keys [lo, hi) are in the bucket; the answer is in [lo - 1, hi - 1]
  while (lo < hi) {                                    // first index in [lo, hi) with key > x
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)a.key[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t i = lo ? lo - 1 : 0;                  // (lo = 0: no key <= x, only for samples that are not this BWT's)
  return (uint64_t)a.val[i] + (x - (uint64_t)a.key[i]);
}

// one lane per segment, at most kChainSteps positions per launch; the state goes back for the next launch
template <class I>
__global__ void __launch_bounds__(kTB) fm_chain(FmArgs<I> a, uint64_t S, Seg *__restrict__ seg, uint64_t *__restrict__ pos) {
  const uint64_t g = BID * kTB + threadIdx.x;
  if (g >= S) return;
  Seg s = seg[g];
  if (!s.rem) return;
  const uint64_t steps = s.rem < kChainSteps ? s.rem : kChainSteps;
  for (uint64_t t = 0; t < steps; t++) {
    pos[s.slot++] = s.x;
    if (--s.rem) s.x = phi_inv(a, s.x);
  }
  seg[g] = s;
}

// ---------------------------------------------------------------- matching statistics and MEMs
// one group of 16 lanes per pattern; first: start from (m, 0, n, 0), else from the record.  ctr[0] += patterns left
// unfinished, ctr[1] += patterns of 2^32 - 1 bytes or more (refused: their lengths would not fit len); stats: ctr[2] += steps
// that jumped (step 3), ctr[3] += bytes their extensions matched
template <class I>
__global__ void __launch_bounds__(kTB) fm_ms_k(FmArgs<I> a, const uint8_t *__restrict__ text, const I *__restrict__ re_sa,
                                               const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
                                               MsRec *__restrict__ rec, int first, uint64_t budget, uint32_t *__restrict__ len_out,
                                               uint64_t *__restrict__ pos_out, unsigned long long *__restrict__ ctr, int stats) {
  __shared__ uint8_t code[256];
  PatGroup g;
  if (!pat_group(code, a.codes, off, npat, g)) return;
  const int gl = g.gl;
  const uint64_t p = g.p, o0 = g.o0, o1 = g.o1, n = a.n1 - 1;
  MsRec s = ms_start(first, rec + p, o0, o1, n, ctr, gl);
  uint64_t work = 0, jumps = 0, matched = 0;
  while (s.t > o0 && work < budget) {                   // at least one step per launch, at most budget + what the last one compares
    s.t--;
    work++;
    const uint32_t c = pat[s.t], k = code[c];
    uint64_t out = ~0ull;
    if (k == kAbsent) {                                 // byte 0 or a byte the text does not hold: nothing matches, (q, pos) stay
      s.l = 0;
    } else {
      const uint32_t c4 = c * 0x01010101u;
      const uint64_t target = lf_at(a, s.q, c4, k, gl); // C[c] + rank_c(q): the c's before q have LF values below it
      if (a.bwt[s.q] == c) {
        s.q = target; s.pos -= 1; s.l += 1;
      } else {
        const MsNeighbours nb = ms_neighbours(a, s.q, target, c4, k, gl);
        int64_t lp = -1, ls = -1;                        // (a side that does not exist loses)
        uint64_t sap = 0, sas = 0;
        if (nb.qp != ~0ull) {
          sap = (uint64_t)re_sa[run_ending_at(a, nb.qp)];
          lp = s.l ? (int64_t)lce16(text, n, sap, s.pos, s.l, gl, work) : 0;
        }
        if (nb.qs != ~0ull && lp < (int64_t)s.l) {     // (lp = l: the predecessor wins whatever the successor has)
          sas = (uint64_t)a.rs_sa[run_starting_at(a, nb.qs)];
          ls = s.l ? (int64_t)lce16(text, n, sas, s.pos, s.l, gl, work) : 0;
        }
        jumps++;
        matched += (lp > 0 ? (uint64_t)lp : 0) + (ls > 0 ? (uint64_t)ls : 0);
        if (lp < 0 && ls < 0) {                         // (no c at all: only for a directory that is not this BWT's)
          s.l = 0;
        } else if (lp >= ls) {
          s.q = target - 1; s.pos = sap - 1; s.l = (uint64_t)lp + 1;
        } else {
          s.q = target; s.pos = sas - 1; s.l = (uint64_t)ls + 1;
        }
      }
      if (s.l) out = s.pos;
    }
    if (gl == 0) {
      len_out[s.t] = (uint32_t)s.l;
      if (pos_out) pos_out[s.t] = out;
    }
  }
  if (gl == 0) {
    rec[p] = s;
    if (s.t > o0) atomicAdd(&ctr[0], 1ull);
    if (stats) { atomicAdd(&ctr[2], (unsigned long long)jumps); atomicAdd(&ctr[3], (unsigned long long)matched); }
  }
}

__device__ __forceinline__ bool is_mem(const uint32_t *__restrict__ len, uint64_t t, uint64_t o0, uint64_t min_len) {
  const uint32_t l = len[t];
  return (uint64_t)l >= min_len && (t == o0 || len[t - 1] <= l);
}

// cnt[p] = MEMs of pattern p (one group of 16 lanes per pattern; cnt[npat] = 0: the exclusive sums end with the total)
__global__ void __launch_bounds__(kTB) fm_mem_count(const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ len,
                                                    uint64_t min_len, uint64_t *__restrict__ cnt) {
  const int gl = threadIdx.x & 15;
  const uint64_t p = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (p > npat) return;
  uint64_t k = 0;
  if (p < npat) {
    const uint64_t o0 = off[p], o1 = off[p + 1];
    for (uint64_t t = o0 + gl; t < o1; t += 16) k += is_mem(len, t, o0, min_len);
  }
  k = gsum16(k);
  if (gl == 0) cnt[p] = k;
}

// mem[3 * (mem_off[p] + j)] = {i, len, pos} of pattern p's j-th MEM, by increasing i
__global__ void __launch_bounds__(kTB) fm_mem_gather(const uint64_t *__restrict__ off, uint64_t npat, const uint32_t *__restrict__ len,
                                                     const uint64_t *__restrict__ pos, uint64_t min_len, const uint64_t *__restrict__ mem_off,
                                                     uint64_t *__restrict__ mem) {
  const int gl = threadIdx.x & 15;
  const uint64_t p = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (p >= npat) return;
  const uint64_t o0 = off[p], o1 = off[p + 1];
  uint64_t slot = mem_off[p];
  for (uint64_t base = o0; base < o1; base += 16) {     // (base, o1 and slot are the same in all 16 lanes)
    const uint64_t t = base + gl;
    const uint32_t f = t < o1 && is_mem(len, t, o0, min_len);
    const uint32_t incl = gscan16_incl(f, gl);
    const uint64_t mine = slot + incl - f;
    if (f) {
      mem[3 * mine] = t - o0; mem[3 * mine + 1] = len[t]; mem[3 * mine + 2] = pos ? pos[t] : ~0ull;
    }
    slot += __shfl(incl, 15, 16);
  }
}

template <class I>
void build_samples(pfp_ctx *c, FmIndex &f, const uint8_t *ssa10, uint64_t ssa_bytes, const uint8_t *esa10, uint64_t esa_bytes) {
  const uint64_t n1 = f.n1;
  f.rs.build(c, f.bwt.p, n1, 0);
  const uint64_t r = f.runs = f.rs.runs;
  PFP_REQUIRE(ssa_bytes == 10 * r, PFP_EFORMAT, ".ssa holds " + std::to_string(ssa_bytes) + " bytes; the BWT has " + std::to_string(r) +
                                                    " runs, so its .ssa holds " + std::to_string(10 * r));
  PFP_REQUIRE(esa_bytes == 10 * r, PFP_EFORMAT, ".esa holds " + std::to_string(esa_bytes) + " bytes; the BWT has " + std::to_string(r) +
                                                    " runs, so its .esa holds " + std::to_string(10 * r));
  f.rs_row.alloc(c, r * sizeof(I));
  f.rs_sa.alloc(c, r * sizeof(I));
  if (f.has_text) f.re_sa.alloc(c, r * sizeof(I));
  f.nphi = r - 1;
  DBuf<I> key(c, r), val(c, r);
  {
    RunIndex re;
    re.build(c, f.bwt.p, n1, 1);
    DBuf<uint64_t> bad(c, 2);
    PFP_HIP(hipMemsetAsync(bad.p, 0xFF, 16, c->stream));
    {
      KScope ks(c, "fm_pairs", 20 * r + 4 * r * sizeof(I));
      fm_pairs<I><<<gdim(cdiv(r, kTB)), kTB, 0, c->stream>>>(ssa10, esa10, r, n1, f.rs.bits.p, f.rs.dir.p, re.bits.p, re.dir.p,
                                                              as<I>(f.rs_row), as<I>(f.rs_sa), key.p, val.p, as<I>(f.re_sa), bad.p);
      PFP_HIP(hipGetLastError());
    }
    uint64_t h[2];
    d2h(c, h, bad.p, 2);
    sync(c);
    PFP_REQUIRE(h[0] == ~0ull, PFP_EFORMAT, ".ssa pair " + std::to_string(h[0]) + " does not name run start " + std::to_string(h[0]) + " of the BWT");
    PFP_REQUIRE(h[1] == ~0ull, PFP_EFORMAT, ".esa pair " + std::to_string(h[1]) + " does not name run end " + std::to_string(h[1]) + " of the BWT");
  }
  const int kb = bits_for(n1);
  f.phi_key.alloc(c, std::max<uint64_t>(f.nphi, 1) * sizeof(I));
  f.phi_val.alloc(c, std::max<uint64_t>(f.nphi, 1) * sizeof(I));
  if (f.nphi) {
    SortTag tag("phi^-1 table");
    sort_pairs<I, I>(c, key.p, as<I>(f.phi_key), val.p, as<I>(f.phi_val), f.nphi, 0, kb);
  } else {                                              // (one run: the table is never read; one entry keeps the search in bounds)
    PFP_HIP(hipMemsetAsync(f.phi_key.p, 0, sizeof(I), c->stream));
    PFP_HIP(hipMemsetAsync(f.phi_val.p, 0, sizeof(I), c->stream));
  }
  key.release(); val.release();
  // about one key per bucket
  f.shift = std::max(0, kb - bits_for(std::max<uint64_t>(f.nphi, 1)));
  f.nbk = (n1 >> f.shift) + 1;
  f.phi_dir.alloc(c, (f.nbk + 1) * sizeof(I));
  {
    KScope ks(c, "fm_phidir", (f.nbk + 1) * sizeof(I) * 8);
    bucket_dir_k<I, I><<<gdim(cdiv(f.nbk + 1, kTB)), kTB, 0, c->stream>>>(as<I>(f.phi_key), f.nphi, f.nbk, f.shift, as<I>(f.phi_dir));
    PFP_HIP(hipGetLastError());
  }
  f.samples = true;
}

}  // namespace

uint64_t fm_bwt_bytes(uint64_t n1) { return ((n1 >> kBlkLog) + 1) << kBlkLog; }

uint64_t FmIndex::device_bytes() const {
  return bwt.bytes() + codes.bytes() + blk.bytes() + sbc.bytes() + rs.bits.bytes() + rs.dir.bytes() + rs_row.bytes() + rs_sa.bytes() +
         phi_key.bytes() + phi_val.bytes() + phi_dir.bytes() + text.bytes() + re_sa.bytes() + thr.bytes() + seq_start.bytes() +
         seq_dir.bytes();
}

void fm_build(pfp_ctx *c, FmIndex &f, const uint8_t *bwt, uint64_t n1, const uint8_t *ssa10, uint64_t ssa_bytes, const uint8_t *esa10,
              uint64_t esa_bytes) {
  PFP_REQUIRE(n1 >= 1, PFP_EFORMAT, "not a BWT: no byte 0 (an empty input)");
  PFP_REQUIRE(n1 <= (1ull << 40), PFP_ELIMIT, "a BWT of more than 2^40 bytes (the limit of the 5-byte .sa format)");
  PFP_REQUIRE(bwt, PFP_EINVAL, "no BWT");
  PFP_REQUIRE(!ssa10 == !esa10, PFP_EINVAL, "the run samples come as a pair: .ssa and .esa, or neither");
  f.c = c;
  f.n1 = n1;
  f.wide = c->force_wide || n1 >= (1ull << 32);
  const uint64_t nb = (n1 >> kBlkLog) + 1, ns = (nb + kBlkPerSb - 1) / kBlkPerSb;
  if (bwt != f.bwt.p) {                                 // (pfp_fm_build_files reads the file into f.bwt itself)
    f.bwt.alloc(c, fm_bwt_bytes(n1));
    PFP_HIP(hipMemcpyAsync(f.bwt.p, bwt, n1, hipMemcpyDeviceToDevice, c->stream));
  }
  PFP_HIP(hipMemsetAsync(f.bwt.p + n1, 0, fm_bwt_bytes(n1) - n1, c->stream));
  uint64_t hist[256];
  {
    DBuf<uint64_t> d_hist(c, 256);
    d_hist.zero();
    {
      KScope ks(c, "fm_bytehist", n1);
      fm_bytehist<<<gdim(cdiv(n1, 16384)), kTB, 0, c->stream>>>(f.bwt.p, n1, (unsigned long long *)d_hist.p);
      PFP_HIP(hipGetLastError());
    }
    d2h(c, hist, d_hist.p, 256);
    sync(c);
  }
  PFP_REQUIRE(hist[0] == 1, PFP_EFORMAT, "not a BWT: " + std::to_string(hist[0]) + " bytes 0 among " + std::to_string(n1) + " (a BWT holds exactly one)");
  uint8_t codes[512];
  memset(codes, kAbsent, 256);
  memset(codes + 256, 0, 256);
  int sigma = 0;
  for (int b = 1; b < 256; b++)
    if (hist[b]) { codes[b] = (uint8_t)sigma; codes[256 + sigma] = (uint8_t)b; sigma++; }
  f.sigma = sigma;
  f.codes.alloc(c, 512);
  h2d(c, f.codes.p, codes, 512);
  f.blk.alloc(c, nb * std::max(sigma, 1));
  f.sbc.alloc(c, ns * std::max(sigma, 1));
  if (sigma) {
    const uint64_t waves = cdiv(nb, kHistBlocks);
    {
      KScope ks(c, "fm_blockhist", n1 + nb * sigma * 2);
      fm_blockhist<<<gdim(cdiv(waves, kTB / 64)), kTB, 0, c->stream>>>(f.bwt.p, n1, nb, f.codes.p, sigma, f.blk.p);
      PFP_HIP(hipGetLastError());
    }
    DBuf<uint64_t> tot(c, ns * sigma), base(c, ns * sigma);
    {
      KScope ks(c, "fm_blockscan", nb * sigma * 4 + ns * sigma * 8);
      fm_blockscan<<<gdim(cdiv(ns * sigma, kTB)), kTB, 0, c->stream>>>(f.blk.p, nb, ns, sigma, tot.p);
      PFP_HIP(hipGetLastError());
    }
    exclusive_sum_u64(c, tot.p, base.p, ns * sigma);
    fm_sbc<<<gdim(cdiv(ns * sigma, kTB)), kTB, 0, c->stream>>>(base.p, ns, sigma, f.sbc.p);
    PFP_HIP(hipGetLastError());
  }
  if (ssa10) by_width(f, [&](auto w) { build_samples<decltype(w)>(c, f, ssa10, ssa_bytes, esa10, esa_bytes); });
  sync(c);
}

void fm_build_ms(pfp_ctx *c, FmIndex &f, const uint8_t *bwt, uint64_t n1, const uint8_t *ssa10, uint64_t ssa_bytes, const uint8_t *esa10,
                 uint64_t esa_bytes, const uint8_t *text) {
  PFP_REQUIRE(ssa10 && esa10, PFP_EINVAL, "matching statistics need the run samples: .ssa and .esa (bigbwt -s -e writes them)");
  f.has_text = true;                                    // (build_samples keeps SA[run end] by run number)
  fm_build(c, f, bwt, n1, ssa10, ssa_bytes, esa10, esa_bytes);
  const uint64_t n = n1 - 1;
  if (text != f.text.p || !text) {
    f.text.alloc(c, n + 16);
    if (text) {
      PFP_HIP(hipMemcpyAsync(f.text.p, text, n, hipMemcpyDeviceToDevice, c->stream));
    } else if (n) {
      BwtCheckArgs in;
      in.bwt = f.bwt.p; in.n1 = n1; in.out = f.text.p;
      pfp_check_result res;
      invert_bwt(c, in, &res);
    }
  }
  PFP_HIP(hipMemsetAsync(f.text.p + n, 0, 16, c->stream));
  sync(c);
}

template <class I>
static void ms_t(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos) {
  pfp_ctx *c = f.c;
  const uint64_t budget = budget_from_env(kMsWork);
  const int stats = stats_from_env();
  const FmArgs<I> a = args_of<I>(f);
  DBuf<MsRec> rec(c, npat);
  DBuf<uint64_t> ctr(c, 4);
  bounded_launches(c, "fm_ms", ctr, [&](int first, unsigned long long *d_ctr) {
    fm_ms_k<I><<<gdim(cdiv(npat, kTB / 16)), kTB, 0, c->stream>>>(a, f.text.p, as<I>(f.re_sa), pat, pat_off, npat, rec.p, first, budget, len, pos,
                                                                  d_ctr, stats);
  }, [&](const uint64_t *h) { ms_launch_counted(f, h); });
}

void fm_ms(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos) {
  require_text(f, "matching statistics");
  if (!npat) return;
  by_width(f, [&](auto w) { ms_t<decltype(w)>(f, pat, pat_off, npat, len, pos); });
}

void fm_mems(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint32_t *len, const uint64_t *pos, uint64_t min_len,
             uint64_t *mem_off, uint64_t *mem) {
  pfp_ctx *c = f.c;
  require_text(f, "maximal exact matches");
  PFP_REQUIRE(min_len >= 1, PFP_EINVAL, "min_len = 0: a maximal exact match is at least 1 byte long");
  KScope ks(c, "fm_mems", 0);
  {
    DBuf<uint64_t> cnt(c, npat + 1);
    fm_mem_count<<<gdim(cdiv(npat + 1, kTB / 16)), kTB, 0, c->stream>>>(pat_off, npat, len, min_len, cnt.p);
    PFP_HIP(hipGetLastError());
    exclusive_sum_u64(c, cnt.p, mem_off, npat + 1);
  }
  if (mem && npat) {
    fm_mem_gather<<<gdim(cdiv(npat, kTB / 16)), kTB, 0, c->stream>>>(pat_off, npat, len, pos, min_len, mem_off, mem);
    PFP_HIP(hipGetLastError());
  }
}

void fm_mem_triples(FmIndex &f, const uint64_t *pat_off, uint64_t npat, const uint32_t *len, const uint64_t *pos, uint64_t min_len,
                    const uint64_t *mem_off, uint64_t *mem) {
  pfp_ctx *c = f.c;
  require_text(f, "maximal exact matches");
  PFP_REQUIRE(min_len >= 1, PFP_EINVAL, "min_len = 0: a maximal exact match is at least 1 byte long");
  if (!npat) return;
  KScope ks(c, "fm_mems", 0);
  fm_mem_gather<<<gdim(cdiv(npat, kTB / 16)), kTB, 0, c->stream>>>(pat_off, npat, len, pos, min_len, mem_off, mem);
  PFP_HIP(hipGetLastError());
}

void fm_count_spans(FmIndex &f, const uint8_t *pat, const uint64_t *begin, const uint64_t *end, uint64_t npat, uint64_t *sp, uint64_t *ep,
                    uint64_t *first) {
  pfp_ctx *c = f.c;
  require_toehold(f, first != nullptr);
  if (!npat) return;
  KScope ks(c, "fm_count", 0);
  by_width(f, [&](auto w) {
    fm_count_k<decltype(w)><<<gdim(cdiv(npat, kTB / 16)), kTB, 0, c->stream>>>(args_of<decltype(w)>(f), pat, begin, end, npat, sp, ep, first);
  });
  PFP_HIP(hipGetLastError());
}

void fm_count(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t *sp, uint64_t *ep, uint64_t *first) {
  fm_count_spans(f, pat, pat_off, nullptr, npat, sp, ep, first);
}

template <class I>
static void locate_t(FmIndex &f, uint64_t npat, const uint64_t *sp, const uint64_t *ep, const uint64_t *first, uint64_t max_occ,
                     uint64_t *out_off, uint64_t *pos) {
  pfp_ctx *c = f.c;
  const FmArgs<I> a = args_of<I>(f);
  DBuf<uint64_t> npos(c, npat + 1), nseg, q0, seg_off;
  if (pos) { nseg.alloc(c, npat + 1); q0.alloc(c, npat + 1); seg_off.alloc(c, npat + 1); }
  fm_plan<I><<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(a, npat, sp, ep, max_occ, npos.p, pos ? nseg.p : nullptr, pos ? q0.p : nullptr);
  PFP_HIP(hipGetLastError());
  exclusive_sum_u64(c, npos.p, out_off, npat + 1);
  if (!pos || !npat) return;
  exclusive_sum_u64(c, nseg.p, seg_off.p, npat + 1);
  const uint64_t S = read_scalar(c, seg_off.p + npat);
  if (!S) return;
  DBuf<Seg> seg(c, S);
  DBuf<uint64_t> maxlen(c, 1);
  maxlen.zero();
  {
    KScope ks(c, "fm_expand", S * (24 + 8 * 6));
    fm_expand<I><<<gdim(cdiv(S, kTB)), kTB, 0, c->stream>>>(a, npat, S, seg_off.p, nseg.p, q0.p, npos.p, out_off, sp, first, seg.p, maxlen.p);
    PFP_HIP(hipGetLastError());
  }
  const uint64_t longest = read_scalar(c, maxlen.p);
  KScope ks(c, "fm_chain", 0);
  for (uint64_t done = 0; done < longest; done += kChainSteps) {
    fm_chain<I><<<gdim(cdiv(S, kTB)), kTB, 0, c->stream>>>(a, S, seg.p, pos);
    PFP_HIP(hipGetLastError());
  }
}

void fm_locate(FmIndex &f, uint64_t npat, const uint64_t *sp, const uint64_t *ep, const uint64_t *first, uint64_t max_occ,
               uint64_t *out_off, uint64_t *pos) {
  require_samples(f);
  PFP_REQUIRE(!pos || first, PFP_EINVAL, "locate needs the toehold SA[sp] of every pattern (count with first)");
  by_width(f, [&](auto w) { locate_t<decltype(w)>(f, npat, sp, ep, first, max_occ, out_off, pos); });
}

}  // namespace pfp
