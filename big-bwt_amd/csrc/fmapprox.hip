// fmapprox.hip -- k-mismatch search over an FmIndex: the distinct strings within Hamming distance k of a pattern that occur in
// the text, each as a row range, and their positions.  The reference has no counterpart; include/pfpgpu.h, "Approximate search",
// states the definitions (occurrence, hit, order of hits, locating).
//
//   The walk.  One group of 16 lanes per pattern (lf_at is a 16-lane operation) walks the backtracking tree depth first with an
//   explicit stack of at most k + 1 frames.  Frame d is the exact backward walk of a branch that has spent d mismatches: (t, sp,
//   ep, first, next code), standing before pattern byte t - 1.  At each position a frame with d < k first opens a child frame
//   for every symbol other than P[t-1] whose range stays non-empty, in code order; then it takes the exact step, which does not
//   exist for a byte 0 or a byte the text does not hold.  A step that reaches the pattern's left end with a non-empty range
//   emits a hit.  The toehold moves by count's rule (fm_count_k).  The top frame lives in registers, the frames below it in LDS.
//   Small ranges.  A range of at most 16 rows is read (one BWT byte per lane) and only the symbols among those bytes are tried:
//   every one of them has a non-empty range, a range of one row has one child, and an exact step whose byte is not among them
//   is not taken.  Larger ranges try every symbol.
//   Bounded launches.  A launch gives every pattern `budget` iterations (kMsWork; an iteration makes at most one LF pair) and
//   leaves the stack, its depth and the hits emitted so far in an ApxRec; the host launches until no pattern is unfinished.
//   The call.  A counting walk -> a library exclusive scan -> a second walk that writes the hits at their offsets in walk order
//   -> the library's segmented sort by sp inside every pattern (values: the hit's place) -> one gather.  k = 0 has at most one
//   hit per pattern and skips the sort.
//   Locating.  The hits' ep clipped to the first max_occ rows of the pattern (an exclusive sum of ep - sp) -> fm_locate over the
//   hits -> d per position and the per-pattern offsets.
// Bounds: every loop is bounded by m, sigma, k + 1, a directory's size or the budget; a hit is written only below its
// pattern's next offset; values read from the samples only become outputs.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"

namespace pfp {

namespace {

constexpr int kApxFrames = PFP_FM_APPROX_MAX_K + 1;
constexpr uint64_t kApxDone = ~0ull;
constexpr uint64_t kNoCode = ~0ull;

struct ApxFrame { uint64_t t, sp, ep, first, nc; };                 // nc: the next code to try as a mismatch (sigma: none left)
struct ApxRec { ApxFrame f[kApxFrames]; uint64_t depth, hits; };    // depth = kApxDone: the walk has ended

// one group of 16 lanes per pattern; first_launch: start from the root, else from the record.  Counting (o_sp NULL): cnt[p] =
// hits once the walk ends.  Filling: hit j of the walk goes to hit_off[p] + j.  ctr[0] += patterns left unfinished; stats:
// ctr[1] += LF pairs
template <class I>
__global__ void __launch_bounds__(kTB) fm_approx_k(FmArgs<I> a, const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
                                                   int kmax, ApxRec *__restrict__ rec, int first_launch, uint64_t budget,
                                                   const uint64_t *__restrict__ hit_off, uint64_t *__restrict__ cnt, uint64_t *__restrict__ o_sp,
                                                   uint64_t *__restrict__ o_ep, uint64_t *__restrict__ o_first, uint8_t *__restrict__ o_dist,
                                                   unsigned long long *__restrict__ ctr, int stats) {
  __shared__ uint8_t code[256], sym[256];
  __shared__ ApxFrame stack[kTB / 16][kApxFrames];
  sym[threadIdx.x] = a.codes[256 + threadIdx.x];       // (pat_group's barrier covers it)
  PatGroup pg;
  if (!pat_group(code, a.codes, off, npat, pg)) return;
  const int gl = pg.gl, g = threadIdx.x >> 4;
  const uint64_t p = pg.p, o0 = pg.o0, o1 = pg.o1, sigma = (uint64_t)a.sigma;
  const uint64_t slot0 = o_sp ? hit_off[p] : 0, slot1 = o_sp ? hit_off[p + 1] : 0;
  const bool toehold = o_first != nullptr;
  ApxFrame cur;
  uint64_t d = 0, hits = 0;
  bool done = false;
  // (every lane of the group holds the same state and writes the same values: a lane reads back from LDS what it wrote itself)
  auto emit = [&](const ApxFrame &f, uint64_t dist) {
    const uint64_t slot = slot0 + hits;
    if (gl == 0 && o_sp && slot < slot1) {
      o_sp[slot] = f.sp; o_ep[slot] = f.ep; o_dist[slot] = (uint8_t)dist;
      if (toehold) o_first[slot] = f.first;
    }
    hits++;
  };
  if (first_launch) {
    cur = ApxFrame{o1, 0, a.n1, a.n1 - 1, 0};
    if (o1 < o0) {                                      // (decreasing offsets: no pattern, no hit)
      done = true;
    } else if (o1 == o0) {
      emit(cur, 0);
      done = true;
    }
  } else {
    d = rec[p].depth;
    hits = rec[p].hits;
    if (d == kApxDone) return;
    if (d > (uint64_t)kmax) d = (uint64_t)kmax;
    for (uint64_t i = 0; i < d; i++) stack[g][i] = rec[p].f[i];
    cur = rec[p].f[d];
  }
  uint64_t work = 0, pairs = 0;
  while (!done && work < budget) {                      // an iteration: one LF pair, or a frame that ends without one
    work++;
    const uint32_t kp = code[pat[cur.t - 1]];           // (kAbsent: byte 0 or a byte the text does not hold; t > o0 here)
    const uint64_t rows = cur.ep - cur.sp;
    const bool small = rows <= 16;
    uint32_t mine = kAbsent;                            // the code of this lane's row of a small range
    if (small && (uint64_t)gl < rows) mine = code[a.bwt[cur.sp + gl]];
    uint64_t c = kNoCode;
    if (d < (uint64_t)kmax && cur.nc < sigma) {         // the next symbol for a mismatch at t - 1
      if (small) {
        c = gmin16(mine != kAbsent && mine >= cur.nc && mine != kp ? (uint64_t)mine : kNoCode);
      } else {
        c = cur.nc;
        if (c == kp) c++;
        if (c >= sigma) c = kNoCode;
      }
      cur.nc = c != kNoCode ? c + 1 : sigma;
    }
    const bool child = c != kNoCode;
    bool pop = false;
    if (!child) {                                       // the exact step
      bool exists = kp != kAbsent;
      if (exists && small) exists = gsum16(mine == kp) != 0;
      if (exists) c = kp;
      else pop = true;
    }
    if (!pop) {
      const uint32_t b = sym[c], c4 = b * 0x01010101u;
      const uint64_t nsp = lf_at(a, cur.sp, c4, (uint32_t)c, gl), nep = lf_at(a, cur.ep, c4, (uint32_t)c, gl);
      pairs++;
      if (nep > nsp) {
        const uint64_t first = toehold ? toehold_step(a, cur.sp, cur.ep, nsp, cur.first, b, c4, (uint32_t)c, gl) : 0;
        const ApxFrame nf{cur.t - 1, nsp, nep, first, 0};
        if (nf.t == o0) {
          emit(nf, d + child);
          pop = !child;
        } else if (child) {
          stack[g][d] = cur;
          d++;
          cur = nf;
        } else {
          cur = nf;
        }
      } else {
        pop = !child;
      }
    }
    if (pop) {
      if (d == 0) {
        done = true;
      } else {
        d--;
        cur = stack[g][d];
      }
    }
  }
  if (gl == 0) {
    rec[p].hits = hits;
    rec[p].depth = done ? kApxDone : d;
    if (!done) {
      for (uint64_t i = 0; i < d; i++) rec[p].f[i] = stack[g][i];
      rec[p].f[d] = cur;
      atomicAdd(&ctr[0], 1ull);
    } else if (cnt) {
      cnt[p] = hits;
    }
    if (stats) atomicAdd(&ctr[1], (unsigned long long)pairs);
  }
}

// the hits from walk order to sp order: place[i] = where hit i of the sorted order stood
__global__ void __launch_bounds__(kTB) apx_gather_k(uint64_t H, const uint32_t *__restrict__ place, const uint64_t *__restrict__ w_sp,
                                                    const uint64_t *__restrict__ w_ep, const uint64_t *__restrict__ w_first,
                                                    const uint8_t *__restrict__ w_dist, uint64_t *__restrict__ sp, uint64_t *__restrict__ ep,
                                                    uint64_t *__restrict__ first, uint8_t *__restrict__ dist) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i >= H) return;
  uint64_t j = place[i];
  if (j >= H) j = H - 1;
  sp[i] = w_sp[j]; ep[i] = w_ep[j]; dist[i] = w_dist[j];
  if (first) first[i] = w_first[j];
}

// rows[h] = ep - sp of hit h; rows[H] = 0 (the exclusive sums end with the total)
__global__ void __launch_bounds__(kTB) apx_rows_k(uint64_t H, const uint64_t *__restrict__ sp, const uint64_t *__restrict__ ep, uint64_t *__restrict__ rows) {
  const uint64_t h = BID * kTB + threadIdx.x;
  if (h > H) return;
  rows[h] = h < H && ep[h] > sp[h] ? ep[h] - sp[h] : 0;
}

// cep[h] = the end of hit h's rows among the first max_occ rows of its pattern (rsum: exclusive sums of the hits' rows)
__global__ void __launch_bounds__(kTB) apx_clip_k(uint64_t H, const uint64_t *__restrict__ hit_off, uint64_t npat, const uint64_t *__restrict__ rsum,
                                                  const uint64_t *__restrict__ sp, uint64_t max_occ, uint64_t *__restrict__ cep) {
  const uint64_t h = BID * kTB + threadIdx.x;
  if (h >= H) return;
  const uint64_t p = last_le(hit_off, npat, h);
  uint64_t first_hit = hit_off[p];
  if (first_hit > h) first_hit = h;
  const uint64_t before = rsum[h] - rsum[first_hit], rows = rsum[h + 1] - rsum[h];
  uint64_t keep = rows;
  if (max_occ) keep = before >= max_occ ? 0 : (rows < max_occ - before ? rows : max_occ - before);
  cep[h] = sp[h] + keep;
}

// pdist[i] = the distance of the hit that position i belongs to (loc_off: fm_locate's H + 1 offsets over the hits)
__global__ void __launch_bounds__(kTB) apx_pdist_k(uint64_t U, const uint64_t *__restrict__ loc_off, uint64_t H, const uint8_t *__restrict__ dist,
                                                   uint8_t *__restrict__ pdist) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i < U) pdist[i] = dist[last_le(loc_off, H, i)];
}

struct ApxOut { uint64_t *sp, *ep, *first; uint8_t *dist; };

// the walk of every pattern, launch after launch; fill: the hits go to o at hit_off, else cnt[p] = their number
template <class I>
void walk_t(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, const uint64_t *hit_off, uint64_t *cnt, const ApxOut &o) {
  pfp_ctx *c = f.c;
  const uint64_t budget = budget_from_env(kMsWork);
  const int stats = stats_from_env();
  const FmArgs<I> a = args_of<I>(f);
  DBuf<ApxRec> rec(c, npat);
  DBuf<uint64_t> ctr(c, 2);
  bounded_launches(c, "fm_approx", ctr, [&](int first, unsigned long long *d_ctr) {
    fm_approx_k<I><<<gdim(cdiv(npat, kTB / 16)), kTB, 0, c->stream>>>(a, pat, pat_off, npat, k, rec.p, first, budget, hit_off, cnt, o.sp, o.ep, o.first,
                                                                      o.dist, d_ctr, stats);
  }, [&](const uint64_t *h) { f.apx_stats[0] += 1; f.apx_stats[1] += h[1]; });
}

void walk(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, const uint64_t *hit_off, uint64_t *cnt, const ApxOut &o) {
  by_width(f, [&](auto w) { walk_t<decltype(w)>(f, pat, pat_off, npat, k, hit_off, cnt, o); });
}

}  // namespace

void fm_approx_check(const FmIndex &f, int k, bool toehold) {
  PFP_REQUIRE(k >= 0 && k <= PFP_FM_APPROX_MAX_K, PFP_EINVAL, "k = " + std::to_string(k) + ": the mismatch budget is 0 .. " +
                                                                   std::to_string(PFP_FM_APPROX_MAX_K) + " (PFP_FM_APPROX_MAX_K)");
  require_toehold(f, toehold);
}

void fm_approx_count(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, uint64_t *cnt) {
  fm_approx_check(f, k, false);
  PFP_HIP(hipMemsetAsync(cnt + npat, 0, sizeof(uint64_t), f.c->stream));
  if (npat) walk(f, pat, pat_off, npat, k, nullptr, cnt, ApxOut{nullptr, nullptr, nullptr, nullptr});
}

void fm_approx_fill(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, const uint64_t *hit_off, uint64_t H,
                    uint64_t *sp, uint64_t *ep, uint64_t *first, uint8_t *dist) {
  pfp_ctx *c = f.c;
  fm_approx_check(f, k, first != nullptr);
  require_sortable(H, "hits");
  f.apx_stats[2] += H;
  if (!H || !npat) return;
  if (k == 0) {                                         // (at most one hit per pattern: walk order is sp order)
    walk(f, pat, pat_off, npat, k, hit_off, nullptr, ApxOut{sp, ep, first, dist});
    return;
  }
  DBuf<uint64_t> w_sp(c, H), w_ep(c, H), w_first(c, first ? H : 0), sorted(c, H);
  DBuf<uint8_t> w_dist(c, H);
  walk(f, pat, pat_off, npat, k, hit_off, nullptr, ApxOut{w_sp.p, w_ep.p, first ? w_first.p : nullptr, w_dist.p});
  DBuf<uint32_t> sb(c, npat), se(c, npat), val(c, H), place(c, H);
  seg_bounds_k<uint32_t><<<gdim(cdiv(std::max(npat, H), kTB)), kTB, 0, c->stream>>>(hit_off, npat, nullptr, sb.p, se.p, nullptr, val.p, H);
  PFP_HIP(hipGetLastError());
  segsort_pairs_u64_u32(c, w_sp.p, sorted.p, val.p, place.p, H, npat, sb.p, se.p, 0, bits_for(f.n1));
  KScope ks(c, "fm_approx_gather", H * (4 + 2 * (first ? 25 : 17)));
  apx_gather_k<<<gdim(cdiv(H, kTB)), kTB, 0, c->stream>>>(H, place.p, w_sp.p, w_ep.p, first ? w_first.p : nullptr, w_dist.p, sp, ep, first, dist);
  PFP_HIP(hipGetLastError());
  sync(c);                                              // (the walk-order arrays go back when this returns)
}

void fm_approx(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, uint64_t *hit_off, uint64_t *sp, uint64_t *ep,
               uint64_t *first, uint8_t *dist) {
  pfp_ctx *c = f.c;
  fm_approx_check(f, k, first != nullptr);
  {
    DBuf<uint64_t> cnt(c, npat + 1);
    fm_approx_count(f, pat, pat_off, npat, k, cnt.p);
    exclusive_sum_u64(c, cnt.p, hit_off, npat + 1);
  }
  const uint64_t H = read_scalar(c, hit_off + npat);
  require_sortable(H, "hits");
  if (sp) fm_approx_fill(f, pat, pat_off, npat, k, hit_off, H, sp, ep, first, dist);
}

void fm_approx_clip(FmIndex &f, uint64_t npat, const uint64_t *hit_off, uint64_t H, const uint64_t *sp, const uint64_t *ep, const uint64_t *first,
                    uint64_t max_occ, uint64_t *out_off, DBuf<uint64_t> &cep) {
  pfp_ctx *c = f.c;
  require_samples(f);
  cep.alloc(c, H);
  if (!H || !npat) {
    PFP_HIP(hipMemsetAsync(out_off, 0, (npat + 1) * sizeof(uint64_t), c->stream));
    return;
  }
  DBuf<uint64_t> rows(c, H + 1), rsum(c, H + 1), loc_off(c, H + 1);
  apx_rows_k<<<gdim(cdiv(H + 1, kTB)), kTB, 0, c->stream>>>(H, sp, ep, rows.p);
  PFP_HIP(hipGetLastError());
  exclusive_sum_u64(c, rows.p, rsum.p, H + 1);
  apx_clip_k<<<gdim(cdiv(H, kTB)), kTB, 0, c->stream>>>(H, hit_off, npat, rsum.p, sp, max_occ, cep.p);
  PFP_HIP(hipGetLastError());
  fm_locate(f, H, sp, cep.p, first, 0, loc_off.p, nullptr);
  gather_off_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(hit_off, npat, loc_off.p, H, out_off);
  PFP_HIP(hipGetLastError());
  sync(c);                                              // (the sums go back when this returns)
}

uint64_t fm_approx_positions(FmIndex &f, uint64_t H, const uint64_t *sp, const uint64_t *cep, const uint64_t *first, const uint8_t *dist,
                             DBuf<uint64_t> &pos, DBuf<uint8_t> &pdist) {
  pfp_ctx *c = f.c;
  if (!H) return 0;
  DBuf<uint64_t> loc_off(c, H + 1);
  fm_locate(f, H, sp, cep, first, 0, loc_off.p, nullptr);
  const uint64_t U = read_scalar(c, loc_off.p + H);
  if (!U) return 0;
  pos.alloc(c, U);
  pdist.alloc(c, U);
  fm_locate(f, H, sp, cep, first, 0, loc_off.p, pos.p);
  {
    KScope ks(c, "fm_approx_pdist", U * 2 + H * 9);
    apx_pdist_k<<<gdim(cdiv(U, kTB)), kTB, 0, c->stream>>>(U, loc_off.p, H, dist, pdist.p);
    PFP_HIP(hipGetLastError());
  }
  sync(c);
  return U;
}

}  // namespace pfp
