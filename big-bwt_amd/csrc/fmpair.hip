// fmpair.hip -- mapping read pairs: the hits of both mates (fmmap.hip) are combined into proper pairs, a mate whose partner has no
// proper partner among its hits is looked for in the window its partner points at (fmwindow.hip), and every pair of reads gets
// its primary pair, the number of its pairs and a pair MAPQ.  The reference has no counterpart; include/pfpgpu.h, "Mapping read
// pairs", states the definitions (anchors, proper, rescue, pairs, pair key, same locus, pair MAPQ, TLEN).
//
//   Anchors.  fm_map_select with max_sec = C - 1 leaves the hits of read r at the front of its segment of sel.key, in hit order:
//   anchor t of read r is the key at aln_off[2r] + t, t < hit_off[r + 1] - hit_off[r].  Slot r C + t names it everywhere below.
//   Need.  One lane per slot: does any anchor of the mate make a proper pair with it?  If none does, the slot is flagged.
//   Compact.  The library scan of the flags numbers the rescues.
//   Windows.  One lane per flagged slot writes candidate (pattern 2 mate + (1 - strand), lo, hi), with seq_of for the record's
//   bounds; fm_window aligns them all in one call.
//   Reduce.  One lane per pair of reads enumerates its at most C^2 + 2C pairs twice: once for the smallest pair key, once more to
//   count the pairs that are not at the primary's locus and to find the smallest sum among them.  It then writes what both reads
//   report - their member of the primary pair, or their own first hit - and TLEN.
//   Scripts.  fm_map_scripts (fmmap.hip) gives the edit script and the MD string of every read's reported alignment.
// Bounds: a slot's anchor is read only for t below the read's returned hits, so inside its segment; rescue j is read only where
// the scan put a flagged slot; the loops run over C and C^2 entries.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"
#include "fmhit.hpp"

namespace pfp {

namespace {

struct PairArgs {
  const uint64_t *key;        // sel.key
  const uint64_t *aln_off;    // 2 nread + 1
  const uint64_t *hit_off;    // nread + 1
  uint64_t nread, C, min_ins, max_ins;
};

__device__ __forceinline__ uint64_t anchors_of(const PairArgs &g, uint64_t r) { return g.hit_off[r + 1] - g.hit_off[r]; }
__device__ __forceinline__ MapAln anchor(const PairArgs &g, uint64_t r, uint64_t t) { return from_hit(g.key[g.aln_off[2 * r] + t]); }

// proper(a, b): different strands, forward/reverse within the insert bounds, and one record (looked up last)
template <class I>
__device__ __forceinline__ bool pair_proper(const SeqArgs<I> &sq, const PairArgs &g, const MapAln &a, const MapAln &b) {
  if (a.strand == b.strand) return false;
  const MapAln &fw = a.strand ? b : a, &rv = a.strand ? a : b;
  const uint64_t ef = fw.s + fw.span, er = rv.s + rv.span;
  if (fw.s > rv.s || ef > er) return false;
  const uint64_t ins = er - fw.s;
  if (ins < g.min_ins || ins > g.max_ins) return false;
  return seq_of(sq, a.s) == seq_of(sq, b.s);
}

// one lane per slot (entry nread C: 0): flag = the slot holds an anchor that no anchor of the mate is proper with
template <class I>
__global__ void __launch_bounds__(kTB) pair_need_k(SeqArgs<I> sq, PairArgs g, uint64_t *__restrict__ flag) {
  const uint64_t x = BID * kTB + threadIdx.x;
  if (x > g.nread * g.C) return;
  uint64_t need = 0;
  const uint64_t r = x / g.C, t = x % g.C;
  if (r < g.nread && t < anchors_of(g, r)) {
    const MapAln a = anchor(g, r, t);
    const uint64_t mate = r ^ 1, cm = anchors_of(g, mate);
    need = 1;
    for (uint64_t u = 0; u < cm && need; u++) {
      const MapAln b = anchor(g, mate, u);
      if (r & 1 ? pair_proper(sq, g, b, a) : pair_proper(sq, g, a, b)) need = 0;
    }
  }
  flag[x] = need;
}

// one lane per flagged slot: rescue ridx[x] = (the mate's pattern on the other strand, the window the anchor points at)
template <class I>
__global__ void __launch_bounds__(kTB) pair_windows_k(SeqArgs<I> sq, PairArgs g, const uint64_t *__restrict__ flag, const uint64_t *__restrict__ ridx,
                                                      uint64_t R, uint32_t *__restrict__ cand_pat, uint64_t *__restrict__ lo, uint64_t *__restrict__ hi) {
  const uint64_t x = BID * kTB + threadIdx.x;
  if (x >= g.nread * g.C || !flag[x] || ridx[x] >= R) return;
  const uint64_t r = x / g.C, j = ridx[x];
  const MapAln a = anchor(g, r, x % g.C);
  const uint32_t q = seq_of(sq, a.s);
  const uint64_t b0 = sq.start[q], b1 = sq.start[q + 1], e = a.s + a.span;
  cand_pat[j] = (uint32_t)(2 * (r ^ 1) + (1 - a.strand));
  if (a.strand == 0) { lo[j] = a.s; hi[j] = min(a.s + g.max_ins, b1); }
  else { hi[j] = e; lo[j] = max(e - min(e, g.max_ins), b0); }
}

struct PairOutArgs {
  uint8_t *proper; uint64_t *npairs;
  uint8_t *mapped, *rescued, *mapq, *strand; uint32_t *seq; uint64_t *off, *start; uint8_t *dist; int64_t *tlen;
  uint32_t *aln_pat; uint64_t *end;        // for the scripts: pattern 2r + strand, or none
};

// one lane per pair of reads: the primary pair, npairs, the pair MAPQ, and what both reads report
template <class I>
__global__ void __launch_bounds__(kTB) pair_reduce_k(SeqArgs<I> sq, PairArgs g, const uint64_t *__restrict__ flag, const uint64_t *__restrict__ ridx,
                                                     uint64_t R, const uint8_t *__restrict__ rdist, const uint64_t *__restrict__ rstart,
                                                     const uint64_t *__restrict__ rend, const uint8_t *__restrict__ smapq, PairOutArgs o) {
  const uint64_t q = BID * kTB + threadIdx.x;
  if (2 * q + 1 >= g.nread) return;
  const uint64_t r1 = 2 * q, r2 = r1 + 1, c1 = anchors_of(g, r1), c2 = anchors_of(g, r2);
  // the rescued alignment of slot (r, t), on the strand opposite to its anchor's; false: none
  auto rescued = [&](uint64_t r, uint64_t t, const MapAln &a, MapAln &out) -> bool {
    const uint64_t x = r * g.C + t;
    if (!flag[x] || ridx[x] >= R) return false;
    const uint64_t j = ridx[x];
    if (rdist[j] > PFP_FM_EXTEND_MAX_K || rstart[j] >= rend[j] || rend[j] - rstart[j] >= (1ull << kSpanBits)) return false;
    out = MapAln{rstart[j], rend[j] - rstart[j], rdist[j], 1 - a.strand};
    return true;
  };
  // every pair of the two reads: fn(a, b, which) with which = 2 for two anchors, else the mate (0, 1) that was rescued
  auto each = [&](auto &&fn) {
    for (uint64_t ta = 0; ta < c1; ta++) {
      const MapAln a = anchor(g, r1, ta);
      for (uint64_t tb = 0; tb < c2; tb++) {
        const MapAln b = anchor(g, r2, tb);
        if (pair_proper(sq, g, a, b)) fn(a, b, 2);
      }
      MapAln b;
      if (rescued(r1, ta, a, b) && pair_proper(sq, g, a, b)) fn(a, b, 1);
    }
    for (uint64_t tb = 0; tb < c2; tb++) {
      const MapAln b = anchor(g, r2, tb);
      MapAln a;
      if (rescued(r2, tb, b, a) && pair_proper(sq, g, a, b)) fn(a, b, 0);
    }
  };
  bool any = false;
  MapAln pa{}, pb{};
  uint64_t ka = 0, kb = 0, d1 = 0;
  int which = 2;
  each([&](const MapAln &a, const MapAln &b, int w) {
    const uint64_t sum = a.d + b.d, xa = hit_key(a), xb = hit_key(b);
    if (!any || sum < d1 || (sum == d1 && (xa < ka || (xa == ka && xb < kb)))) { any = true; pa = a; pb = b; ka = xa; kb = xb; d1 = sum; which = w; }
  });
  uint64_t np = 0, d2 = ~0ull;
  if (any) {
    np = 1;
    auto meets = [](const MapAln &x, const MapAln &y) { return max(x.s, y.s) < min(x.s + x.span, y.s + y.span); };
    each([&](const MapAln &a, const MapAln &b, int) {
      if (hit_key(a) == ka && hit_key(b) == kb) return;                 // the primary itself
      if (a.strand == pa.strand && b.strand == pb.strand && meets(a, pa) && meets(b, pb)) return;       // the primary's locus
      np++;
      d2 = min(d2, (uint64_t)(a.d + b.d));
    });
  }
  const uint32_t pq = np == 1 ? 60u : d2 == d1 ? 0u : (uint32_t)min((uint64_t)60, 10 * (d2 - d1));
  o.proper[q] = any ? 1 : 0;
  o.npairs[q] = np;
  // what each read reports: (mapped, the alignment, rescued, mapq)
  MapAln al[2] = {pa, pb};
  bool mp[2] = {any, any};
  if (!any) {
    mp[0] = c1 > 0; mp[1] = c2 > 0;
    if (mp[0]) al[0] = anchor(g, r1, 0);
    if (mp[1]) al[1] = anchor(g, r2, 0);
  }
  uint32_t sqn[2] = {kNoSeq, kNoSeq};
  for (int t = 0; t < 2; t++)
    if (mp[t] && al[t].s < sq.n) sqn[t] = seq_of(sq, al[t].s);
  int64_t tl = 0;                                       // mate 1's TLEN; mate 2's is its negative
  if (mp[0] && mp[1] && sqn[0] == sqn[1] && sqn[0] != kNoSeq) {
    const uint64_t span = max(al[0].s + al[0].span, al[1].s + al[1].span) - min(al[0].s, al[1].s);
    tl = al[0].s <= al[1].s ? (int64_t)span : -(int64_t)span;
  }
  for (int t = 0; t < 2; t++) {
    const uint64_t r = r1 + t;
    const bool m = mp[t] && sqn[t] != kNoSeq;
    o.mapped[r] = m ? 1 : 0;
    o.rescued[r] = m && any && which == t ? 1 : 0;
    o.mapq[r] = any ? (uint8_t)pq : smapq[r];
    o.strand[r] = m ? (uint8_t)al[t].strand : 0;
    o.seq[r] = sqn[t];
    o.off[r] = m ? al[t].s - (uint64_t)sq.start[sqn[t]] : ~0ull;
    o.start[r] = m ? al[t].s : ~0ull;
    o.dist[r] = m ? (uint8_t)al[t].d : 0xFF;
    o.tlen[r] = t ? -tl : tl;
    o.aln_pat[r] = m ? (uint32_t)(2 * r + al[t].strand) : 0xFFFFFFFFu;
    o.end[r] = m ? al[t].s + al[t].span : ~0ull;
  }
}

}  // namespace

void fm_pair_check(const FmIndex &f, uint64_t npat, int k, uint64_t min_seed, bool thresholds, uint64_t min_ins, uint64_t max_ins, uint64_t anchors) {
  fm_map_check(f, k, min_seed, thresholds);
  PFP_REQUIRE(npat % 2 == 0, PFP_EINVAL, std::to_string(npat) + " reads: reads 2q and 2q + 1 are the mates of pair q, so their number is even");
  PFP_REQUIRE(min_ins <= max_ins && max_ins <= PFP_FM_WINDOW_MAX_W, PFP_EINVAL,
              "insert sizes " + std::to_string(min_ins) + " .. " + std::to_string(max_ins) + ": min_ins <= max_ins <= " +
                  std::to_string(PFP_FM_WINDOW_MAX_W) + " (PFP_FM_WINDOW_MAX_W)");
  PFP_REQUIRE(anchors >= 1 && anchors <= PFP_FM_PAIR_MAX_ANCHORS, PFP_EINVAL,
              "anchors = " + std::to_string(anchors) + ": 1 .. " + std::to_string(PFP_FM_PAIR_MAX_ANCHORS) + " (PFP_FM_PAIR_MAX_ANCHORS)");
}

void fm_pair(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t nread, int k, uint64_t min_ins, uint64_t max_ins, uint64_t C,
             const uint64_t *aln_off, const uint64_t *hit_off, const uint8_t *smapq, const MapSel &sel, const PairOut &out, DBuf<uint32_t> &cig,
             DBuf<uint8_t> &md) {
  pfp_ctx *c = f.c;
  if (!nread) {
    PFP_HIP(hipMemsetAsync(out.cig_off, 0, sizeof(uint64_t), c->stream));
    PFP_HIP(hipMemsetAsync(out.md_off, 0, sizeof(uint64_t), c->stream));
    sync(c);
    return;
  }
  const PairArgs g{sel.key.p, aln_off, hit_off, nread, C, min_ins, max_ins};
  const uint64_t slots = nread * C;
  DBuf<uint64_t> flag(c, slots + 1), ridx(c, slots + 1);
  {
    KScope ks(c, "fm_pair_need", 0);
    by_width(f, [&](auto w) {
      using I = decltype(w);
      pair_need_k<I><<<gdim(cdiv(slots + 1, kTB)), kTB, 0, c->stream>>>(seq_args<I>(f), g, flag.p);
    });
    PFP_HIP(hipGetLastError());
    exclusive_sum_u64(c, flag.p, ridx.p, slots + 1);
  }
  const uint64_t R = read_scalar(c, ridx.p + slots);    // the rescues
  DBuf<uint32_t> cand(c, R);
  DBuf<uint64_t> win(c, 2 * R), res(c, 2 * R);
  DBuf<uint8_t> rdist(c, R);
  if (R) {
    {
      KScope ks(c, "fm_pair_windows", 0);
      by_width(f, [&](auto w) {
        using I = decltype(w);
        pair_windows_k<I><<<gdim(cdiv(slots, kTB)), kTB, 0, c->stream>>>(seq_args<I>(f), g, flag.p, ridx.p, R, cand.p, win.p, win.p + R);
      });
      PFP_HIP(hipGetLastError());
    }
    fm_window(f, pat2, pat2_off, 2 * nread, cand.p, win.p, win.p + R, R, k, rdist.p, res.p, res.p + R);
  }
  DBuf<uint32_t> aln_pat(c, nread);
  DBuf<uint64_t> end(c, nread);
  {
    KScope ks(c, "fm_pair_reduce", 0);
    const PairOutArgs o{out.proper, out.npairs, out.mapped, out.rescued, out.mapq, out.strand, out.seq, out.off, out.start, out.dist, out.tlen,
                        aln_pat.p, end.p};
    by_width(f, [&](auto w) {
      using I = decltype(w);
      pair_reduce_k<I><<<gdim(cdiv(nread / 2, kTB)), kTB, 0, c->stream>>>(seq_args<I>(f), g, flag.p, ridx.p, R, rdist.p, res.p, res.p + R, smapq, o);
    });
    PFP_HIP(hipGetLastError());
  }
  fm_map_scripts(f, pat2, pat2_off, 2 * nread, k, aln_pat.p, out.start, end.p, nread, out.cig_off, cig, out.md_off, md);
}

void fm_map_pairs(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, bool thresholds, uint64_t min_ins,
                  uint64_t max_ins, uint64_t anchors, uint64_t *nhits, const PairOut &out, DBuf<uint32_t> &cig, DBuf<uint8_t> &md) {
  pfp_ctx *c = f.c;
  fm_pair_check(f, npat, k, min_seed, thresholds, min_ins, max_ins, anchors);
  MapReads rd;
  fm_map_strands(f, pat, pat_off, npat, rd);
  DBuf<uint64_t> hit_off(c, npat + 1);
  DBuf<uint8_t> smapq(c, npat);
  MapCands cd;
  fm_map_cands(f, rd.pat.p, rd.off.p, 2 * npat, min_seed, k, thresholds, cd);
  MapSel sel;
  fm_map_select(f, rd.off.p, npat, k, anchors - 1, cd, hit_off.p, smapq.p, nhits, sel);
  cd.drop_triples();
  fm_pair(f, rd.pat.p, rd.off.p, npat, k, min_ins, max_ins, anchors, cd.aln_off.p, hit_off.p, smapq.p, sel, out, cig, md);
  sync(c);
}

}  // namespace pfp
