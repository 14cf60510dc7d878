// fmmap.hip -- mapping reads to a collection: both strands through fm_align, then which alignments lie inside one record, which
// of them are one locus seen twice, their order, a mapping quality, and per returned hit its place, its edit script (fmcigar.hip)
// and its MD string.  The reference has no counterpart; include/pfpgpu.h, "Mapping reads", states the definitions (strands, inside,
// shadowing, hits, MAPQ, MD).
//
//   Strands.  map_strands_k writes the 2 npat patterns fm_align sees: 2p = read p, 2p + 1 = its reverse complement.  One group of
//   16 lanes per read, 16 bytes per lane and step: an unaligned 16-byte load, the four words swapped and byte-reversed (bswap: one
//   v_perm_b32 each), the complement as byte-parallel arithmetic on the words (A^T = 0x15, C^G = 0x04 under a mask of the bytes
//   that are one of the letters, either case), a 16-byte store.  A tail of less than 16 bytes goes byte by byte.
//   Inside.  One lane per alignment: its pattern by a binary search over aln_off (so its read and its strand), seq(s) through the
//   table's bucket directory (fmdev.hpp: seq_of) and the test e <= starts[seq + 1].  It leaves the place key s << 24 | (e - s) << 7
//   | d << 1 | strand (40 + 17 + 6 + 1 bits: the limits of fmextend.hip's key), or kNone for an alignment that is not inside.
//   Shadowing.  The alignments of read p, both strands, are the segment aln_off[2p] .. aln_off[2p + 2].  The library's segmented
//   sort orders every segment by the place key, so by s (kNone goes last).  A lane per alignment then looks left while
//   s_b + m + k > s_a and right while s_b < e_a: a span holds at most m + k bytes, so nothing beyond intersects.  It is shadowed when
//   one of those has a smaller hit key and intersects it.  Unshadowed: the hit key d << 58 | strand << 57 | s << 17 | (e - s).
//   Selection.  A second segmented sort, by the whole hit key: the hits of a read are now the front of its segment, in key order.
//   A lane per read finds where they end (a binary search for the first kNone), which is nhits, derives MAPQ from the first two
//   hits (sorted by d: the second hit's distance is d1 or the smallest above it), and counts min(nhits, 1 + max_sec); the library
//   scan of the counts is hit_off.
//   Filling.  A lane per returned hit unpacks its key and looks up (seq, off); fm_cigar_runs / fm_cigar_write give the scripts of
//   (pattern 2p + strand, s, e); the MD strings take two passes of one lane per hit over its runs, count and emit, with the
//   library scan of the lengths between them.
// Bounds: the shadow scan of an alignment visits the alignments of its read that start within m + k bytes before it or inside it;
// the MD walk visits at most 2k + 1 runs and 2k text bytes; every index read from a key or an offset is used inside its own
// segment only; text is read below n, patterns inside their offsets.
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "fmdev.hpp"
#include "fmhit.hpp"

namespace pfp {

namespace {

// len2[2p] = len2[2p + 1] = the bytes of read p (decreasing offsets: none); len2[2 npat] = 0
__global__ void __launch_bounds__(kTB) map_lens_k(const uint64_t *__restrict__ off, uint64_t npat, uint64_t *__restrict__ len2) {
  const uint64_t p = BID * kTB + threadIdx.x;
  if (p > npat) return;
  if (p == npat) { len2[2 * p] = 0; return; }
  const uint64_t o0 = off[p], o1 = off[p + 1], m = o1 > o0 ? o1 - o0 : 0;
  len2[2 * p] = m; len2[2 * p + 1] = m;
}

// the complement of every byte of w that is one of A C G T a c g t; the other bytes stay
__device__ __forceinline__ uint32_t comp4(uint32_t w) {
  const uint32_t l = w | 0x20202020u;                   // (a byte with bit 5 set equals a lower-case letter iff it was that letter in either case)
  const uint32_t at = (eq_bytes(l, 0x61616161u) | eq_bytes(l, 0x74747474u)) >> 7;
  const uint32_t cg = (eq_bytes(l, 0x63636363u) | eq_bytes(l, 0x67676767u)) >> 7;
  return w ^ (at * 0x15u) ^ (cg * 0x04u);               // 'A' ^ 'T' = 0x15, 'C' ^ 'G' = 0x04; at and cg hold 0 or 1 per byte
}
__device__ __forceinline__ uint32_t rc4(uint32_t w) { return __builtin_bswap32(comp4(w)); }

// one group of 16 lanes per read: out[off2[2p] ..) = the read, out[off2[2p + 1] ..) = its reverse complement
__global__ void __launch_bounds__(kTB) map_strands_k(const uint8_t *__restrict__ pat, const uint64_t *__restrict__ off, uint64_t npat,
                                                     const uint64_t *__restrict__ off2, uint8_t *__restrict__ out) {
  const int gl = threadIdx.x & 15;
  const uint64_t p = BID * (kTB / 16) + (threadIdx.x >> 4);
  if (p >= npat) return;
  const uint64_t o0 = off[p], m = off2[2 * p + 1] - off2[2 * p];
  const uint8_t *in = pat + o0;
  uint8_t *fw = out + off2[2 * p], *rv = out + off2[2 * p + 1];
  for (uint64_t t = 16 * (uint64_t)gl; t < m; t += 256) {
    if (t + 16 <= m) {
      st16u(fw + t, ld16u(in + t));
      const uint4 u = ld16u(in + (m - 16 - t));         // the 16 bytes that end where the reverse strand's byte t begins
      st16u(rv + t, make_uint4(rc4(u.w), rc4(u.z), rc4(u.y), rc4(u.x)));
    } else {
      for (uint64_t x = t; x < m; x++) {
        fw[x] = in[x];
        rv[x] = (uint8_t)comp4(in[m - 1 - x]);
      }
    }
  }
}

// sb[r], se[r] = the segment of read r among the alignments: aln_off[2r], aln_off[2r + 2]
__global__ void __launch_bounds__(kTB) map_bounds_k(const uint64_t *__restrict__ aln_off, uint64_t npat, uint32_t *__restrict__ sb,
                                                    uint32_t *__restrict__ se) {
  const uint64_t r = BID * kTB + threadIdx.x;
  if (r >= npat) return;
  sb[r] = (uint32_t)aln_off[2 * r]; se[r] = (uint32_t)aln_off[2 * r + 2];
}

// one lane per alignment j < A: its read, and its place key if it lies inside one record, else kNone
template <class I>
__global__ void __launch_bounds__(kTB) map_inside_k(SeqArgs<I> sq, const uint64_t *__restrict__ aln_off, uint64_t npat, const uint64_t *__restrict__ start,
                                                    const uint64_t *__restrict__ end, const uint8_t *__restrict__ dist, uint64_t A,
                                                    uint32_t *__restrict__ read, uint64_t *__restrict__ key) {
  const uint64_t j = BID * kTB + threadIdx.x;
  if (j >= A) return;
  const uint64_t p2 = last_le(aln_off, 2 * npat + 1, j);        // the alignment's pattern (j < aln_off[2 npat]: below 2 npat)
  const uint64_t s = start[j], e = end[j];
  const uint32_t d = dist[j];
  uint64_t k = kNone;
  if (s < e && e <= sq.n && d <= PFP_FM_EXTEND_MAX_K && e - s < (1ull << kSpanBits) && s < (1ull << kPosBits)) {
    const uint32_t q = seq_of(sq, s);
    if (e <= (uint64_t)sq.start[q + 1]) k = place_key(MapAln{s, e - s, d, (uint32_t)(p2 & 1)});
  }
  read[j] = (uint32_t)(p2 >> 1);
  key[j] = k;
}

// one lane per alignment i < A of the segments sorted by s: out[i] = its hit key if no alignment of its read with a smaller hit
// key intersects it, else kNone.  w = m + k bounds a span, so the scan to the left ends at the first start <= s - w
__global__ void __launch_bounds__(kTB) map_shadow_k(const uint64_t *__restrict__ key, const uint32_t *__restrict__ read, uint64_t A,
                                                    const uint32_t *__restrict__ sb, const uint32_t *__restrict__ se, uint64_t npat,
                                                    const uint64_t *__restrict__ off2, int k, uint64_t *__restrict__ out) {
  const uint64_t i = BID * kTB + threadIdx.x;
  if (i >= A) return;
  const uint64_t ka = key[i];
  uint64_t res = kNone;
  const uint64_t r = read[i];
  if (ka != kNone && r < npat) {
    const MapAln a = from_place(ka);
    const uint64_t mine = hit_key(a), ea = a.s + a.span, w = off2[2 * r + 1] - off2[2 * r] + (uint64_t)k;
    uint64_t b = sb[r], e = se[r];
    if (e > A) e = A;
    if (b > i) b = i;
    bool shadowed = false;
    for (uint64_t t = i; t > b && !shadowed;) {         // (every key before i in the segment is a place key: kNone sorts last)
      const MapAln o = from_place(key[--t]);
      if (o.s + w <= a.s) break;
      shadowed = o.s + o.span > a.s && hit_key(o) < mine;
    }
    for (uint64_t t = i + 1; t < e && !shadowed; t++) {
      const uint64_t kb = key[t];
      if (kb == kNone) break;
      const MapAln o = from_place(kb);
      if (o.s >= ea) break;
      shadowed = hit_key(o) < mine;                     // (a.s <= o.s < ea and the span is not empty: they intersect)
    }
    if (!shadowed) res = mine;
  }
  out[i] = res;
}

// one lane per read r (entry npat: cnt = 0) over the segments sorted by hit key: nhits, mapq, and what is returned
__global__ void __launch_bounds__(kTB) map_reads_k(const uint64_t *__restrict__ key, uint64_t A, const uint32_t *__restrict__ sb,
                                                   const uint32_t *__restrict__ se, uint64_t npat, uint64_t max_sec, uint64_t *__restrict__ nhits,
                                                   uint8_t *__restrict__ mapq, uint64_t *__restrict__ cnt) {
  const uint64_t r = BID * kTB + threadIdx.x;
  if (r > npat) return;
  if (r == npat) { cnt[r] = 0; return; }
  uint64_t b = sb[r], e = se[r];
  if (e > A) e = A;
  if (b > e) b = e;
  uint64_t lo = b, hi = e;                              // the first kNone of the segment
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (key[mid] != kNone) lo = mid + 1;
    else hi = mid;
  }
  const uint64_t nh = lo - b;
  uint32_t q = 0;
  if (nh == 1) q = 60;
  else if (nh > 1) {
    const uint32_t d1 = from_hit(key[b]).d, d2 = from_hit(key[b + 1]).d;      // (d2 >= d1: the order of the keys)
    q = d2 == d1 ? 0 : min(60u, 10u * (d2 - d1));
  }
  nhits[r] = nh;
  mapq[r] = (uint8_t)q;
  cnt[r] = max_sec < nh ? max_sec + 1 : nh;
}

// one lane per returned hit h < H: the t-th key of its read's segment, unpacked
template <class I>
__global__ void __launch_bounds__(kTB) map_hits_k(SeqArgs<I> sq, const uint64_t *__restrict__ key, uint64_t A, const uint64_t *__restrict__ aln_off,
                                                  const uint64_t *__restrict__ hit_off, uint64_t npat, uint64_t H, uint8_t *__restrict__ strand,
                                                  uint32_t *__restrict__ seq, uint64_t *__restrict__ off, uint64_t *__restrict__ start,
                                                  uint8_t *__restrict__ dist, uint32_t *__restrict__ aln_pat, uint64_t *__restrict__ end) {
  const uint64_t h = BID * kTB + threadIdx.x;
  if (h >= H) return;
  const uint64_t r = last_le(hit_off, npat + 1, h);     // (h < hit_off[npat]: below npat)
  const uint64_t i = aln_off[2 * r] + (h - hit_off[r]);
  MapAln a{0, 0, 0xFF, 0};
  uint32_t q = kNoSeq;
  uint64_t o = ~0ull;
  if (i < A && key[i] != kNone) {
    a = from_hit(key[i]);
    if (a.s < sq.n) { q = seq_of(sq, a.s); o = a.s - (uint64_t)sq.start[q]; }
  }
  strand[h] = (uint8_t)a.strand; seq[h] = q; off[h] = o; start[h] = a.s; dist[h] = (uint8_t)a.d;
  aln_pat[h] = (uint32_t)(2 * r + a.strand); end[h] = a.s + a.span;
}

// the MD string of hit h (pfpgpu.h, "Mapping reads", 7): EMIT writes it at md + md_off[h], else len[h] = its bytes (len[H] = 0)
template <bool EMIT>
__global__ void __launch_bounds__(kTB) map_md_k(const uint8_t *__restrict__ text, uint64_t n, const uint64_t *__restrict__ start, uint64_t H,
                                                const uint64_t *__restrict__ cig_off, const uint32_t *__restrict__ cig, uint64_t *__restrict__ len,
                                                const uint64_t *__restrict__ md_off, uint8_t *__restrict__ md) {
  const uint64_t h = BID * kTB + threadIdx.x;
  if (h > H) return;
  if (h == H) { if (!EMIT) len[h] = 0; return; }
  const uint64_t base = EMIT ? md_off[h] : 0, room = EMIT ? md_off[h + 1] - base : 0;
  if (cig_off[h] == cig_off[h + 1]) {                   // no script (a read without an alignment: fmpair.hip): no MD either
    if (!EMIT) len[h] = 0;
    return;
  }
  uint64_t at = 0, j = start[h], run = 0;
  auto put = [&](uint8_t b) {
    if (EMIT && at < room) md[base + at] = b;
    at++;
  };
  auto number = [&](uint64_t v) {
    char dg[20];
    int nd = 0;
    do { dg[nd++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (nd) put((uint8_t)dg[--nd]);
  };
  auto tbyte = [&](uint64_t x) -> uint8_t { return x < n ? text[x] : 0; };
  for (uint64_t c = cig_off[h], ce = cig_off[h + 1]; c < ce; c++) {
    const uint32_t w = cig[c], op = w & 15;
    const uint64_t L = w >> 4;
    if (op == 7) { run += L; j += L; }
    else if (op == 8) {
      for (uint64_t x = 0; x < L; x++) { number(run); put(tbyte(j)); run = 0; j++; }
    } else if (op == 2) {
      number(run); put('^');
      for (uint64_t x = 0; x < L; x++) put(tbyte(j + x));
      run = 0; j += L;
    }
  }
  number(run);
  if (!EMIT) len[h] = at;
}

}  // namespace

void fm_map_check(const FmIndex &f, int k, uint64_t min_seed, bool thresholds) {
  fm_extend_check(f, k);                                // (k and the text come before the table, min_seed and the thresholds behind it)
  PFP_REQUIRE(f.nseq, PFP_EINVAL, "this index has no sequence table: give it one with pfp_fm_set_seqs (bigbwt -f --seqs writes it)");
  fm_align_check(f, k, min_seed, thresholds);
}

void fm_map_strands(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, MapReads &out, bool any_length) {
  pfp_ctx *c = f.c;
  if (!any_length) fm_extend_check_patterns(f, pat_off, npat);      // (PFP_ELIMIT before anything is sized by a length)
  out.off.alloc(c, 2 * npat + 1);
  uint64_t bytes = 0;
  {
    DBuf<uint64_t> len2(c, 2 * npat + 1);
    KScope ks(c, "fm_map_strands", 0);
    map_lens_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(pat_off, npat, len2.p);
    PFP_HIP(hipGetLastError());
    exclusive_sum_u64(c, len2.p, out.off.p, 2 * npat + 1);
    bytes = read_scalar(c, out.off.p + 2 * npat);       // (syncs: the lengths go back)
  }
  out.pat.alloc(c, bytes + 16);
  PFP_HIP(hipMemsetAsync(out.pat.p + bytes, 0, 16, c->stream));
  if (!bytes) return;
  KScope ks(c, "fm_map_strands", 0);
  map_strands_k<<<gdim(cdiv(npat, kTB / 16)), kTB, 0, c->stream>>>(pat, pat_off, npat, out.off.p, out.pat.p);
  PFP_HIP(hipGetLastError());
}

// the end of both ways to the candidates: room for the kept alignments, the triples, and the wait that lets the keys go
static void cands_write(FmIndex &f, const AlnKeys &keys, bool wait, MapCands &out) {
  out.A = keys.total;
  out.start.alloc(f.c, out.A); out.end.alloc(f.c, out.A); out.dist.alloc(f.c, out.A);
  fm_align_write(f, keys, out.start.p, out.end.p, out.dist.p);
  if (wait) sync(f.c);
}

void fm_map_cands(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t npat2, uint64_t min_seed, int k, bool thresholds, MapCands &out) {
  out.aln_off.alloc(f.c, npat2 + 1);
  AlnKeys keys;
  fm_align_keys(f, pat2, pat2_off, npat2, min_seed, k, 0, thresholds, out.aln_off.p, keys);
  cands_write(f, keys, true, out);                      // (the keys go back when this returns)
}

void fm_map_cands_ms(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln,
                     const uint32_t *len, const uint64_t *pos, const uint64_t *mem_off, uint64_t M, MapCands &out, AlnKeys *held) {
  out.aln_off.alloc(f.c, npat + 1);
  AlnKeys own, &keys = held ? *held : own;
  fm_align_seeds(f, pat, pat_off, npat, min_seed, k, max_aln, len, pos, mem_off, M, out.aln_off.p, keys);
  cands_write(f, keys, !held, out);
}

void fm_map_select(FmIndex &f, const uint64_t *pat2_off, uint64_t npat, int k, uint64_t max_sec, const MapCands &cd, uint64_t *hit_off, uint8_t *mapq,
                   uint64_t *nhits, MapSel &sel) {
  pfp_ctx *c = f.c;
  const uint64_t A = cd.A;
  require_sortable(A, "alignments");
  sel.H = 0;
  if (!npat) {
    PFP_HIP(hipMemsetAsync(hit_off, 0, sizeof(uint64_t), c->stream));
    sync(c);
    return;
  }
  DBuf<uint32_t> sb(c, npat), se(c, npat), read(c, A), sread(c, A);
  DBuf<uint64_t> key(c, A), skey(c, A), cnt(c, npat + 1);
  sel.key.alloc(c, A);
  {
    KScope ks(c, "fm_map_inside", 0);
    map_bounds_k<<<gdim(cdiv(npat, kTB)), kTB, 0, c->stream>>>(cd.aln_off.p, npat, sb.p, se.p);
    PFP_HIP(hipGetLastError());
    if (A) {
      by_width(f, [&](auto w) {
        using I = decltype(w);
        map_inside_k<I><<<gdim(cdiv(A, kTB)), kTB, 0, c->stream>>>(seq_args<I>(f), cd.aln_off.p, npat, cd.start.p, cd.end.p, cd.dist.p, A, read.p,
                                                                   key.p);
      });
      PFP_HIP(hipGetLastError());
    }
  }
  if (A) {
    KScope ks(c, "fm_map_shadow", 0);
    segsort_pairs_u64_u32(c, key.p, skey.p, read.p, sread.p, A, npat, sb.p, se.p, 0, 64);
    map_shadow_k<<<gdim(cdiv(A, kTB)), kTB, 0, c->stream>>>(skey.p, read.p, A, sb.p, se.p, npat, pat2_off, k, key.p);
    PFP_HIP(hipGetLastError());
  }
  KScope ks(c, "fm_map_select", 0);
  if (A) segsort_pairs_u64_u32(c, key.p, sel.key.p, read.p, sread.p, A, npat, sb.p, se.p, 0, 64);
  map_reads_k<<<gdim(cdiv(npat + 1, kTB)), kTB, 0, c->stream>>>(sel.key.p, A, sb.p, se.p, npat, max_sec, nhits, mapq, cnt.p);
  PFP_HIP(hipGetLastError());
  exclusive_sum_u64(c, cnt.p, hit_off, npat + 1);
  sel.H = read_scalar(c, hit_off + npat);               // (syncs: the scratch of the sorts goes back when this returns)
}

void fm_map_fill(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t npat, int k, const uint64_t *aln_off, const uint64_t *hit_off,
                 const MapSel &sel, uint8_t *strand, uint32_t *seq, uint64_t *off, uint64_t *start, uint8_t *dist, uint64_t *cig_off,
                 DBuf<uint32_t> &cig, uint64_t *md_off, DBuf<uint8_t> &md) {
  pfp_ctx *c = f.c;
  const uint64_t H = sel.H;
  if (!H) {
    PFP_HIP(hipMemsetAsync(cig_off, 0, sizeof(uint64_t), c->stream));
    PFP_HIP(hipMemsetAsync(md_off, 0, sizeof(uint64_t), c->stream));
    sync(c);
    return;
  }
  DBuf<uint32_t> aln_pat(c, H);
  DBuf<uint64_t> end(c, H);
  {
    KScope ks(c, "fm_map_hits", 0);
    by_width(f, [&](auto w) {
      using I = decltype(w);
      map_hits_k<I><<<gdim(cdiv(H, kTB)), kTB, 0, c->stream>>>(seq_args<I>(f), sel.key.p, sel.key.n, aln_off, hit_off, npat, H, strand, seq, off, start,
                                                               dist, aln_pat.p, end.p);
    });
    PFP_HIP(hipGetLastError());
  }
  fm_map_scripts(f, pat2, pat2_off, 2 * npat, k, aln_pat.p, start, end.p, H, cig_off, cig, md_off, md);
}

void fm_map_scripts(FmIndex &f, const uint8_t *pat2, const uint64_t *pat2_off, uint64_t npat2, int k, const uint32_t *aln_pat, const uint64_t *start,
                    const uint64_t *end, uint64_t H, uint64_t *cig_off, DBuf<uint32_t> &cig, uint64_t *md_off, DBuf<uint8_t> &md) {
  pfp_ctx *c = f.c;
  DBuf<uint64_t> mdlen(c, H + 1);
  DBuf<uint8_t> cdist(c, H);
  CigRuns runs;
  fm_cigar_runs(f, pat2, pat2_off, npat2, aln_pat, start, end, H, k, cdist.p, cig_off, runs);
  cig.alloc(c, runs.total);
  fm_cigar_write(f, runs, cig_off, cig.p);
  const uint8_t *text = f.text.p;
  const uint64_t n = f.n1 - 1;
  uint64_t bytes = 0;
  {
    KScope ks(c, "fm_map_md", 0);
    map_md_k<false><<<gdim(cdiv(H + 1, kTB)), kTB, 0, c->stream>>>(text, n, start, H, cig_off, cig.p, mdlen.p, nullptr, nullptr);
    PFP_HIP(hipGetLastError());
    exclusive_sum_u64(c, mdlen.p, md_off, H + 1);
    bytes = read_scalar(c, md_off + H);
  }
  md.alloc(c, bytes);
  KScope ks(c, "fm_map_md", 0);
  map_md_k<true><<<gdim(cdiv(H + 1, kTB)), kTB, 0, c->stream>>>(text, n, start, H, cig_off, cig.p, nullptr, md_off, md.p);
  PFP_HIP(hipGetLastError());
  sync(c);                                              // (the runs' slots and the plan go back when this returns)
}

void fm_map(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_sec, bool thresholds,
            uint64_t *hit_off, uint8_t *mapq, uint64_t *nhits, uint8_t *strand, uint32_t *seq, uint64_t *off, uint64_t *start, uint8_t *dist,
            uint64_t *cig_off, DBuf<uint32_t> &cig, uint64_t *md_off, DBuf<uint8_t> &md) {
  fm_map_check(f, k, min_seed, thresholds);
  MapReads rd;
  fm_map_strands(f, pat, pat_off, npat, rd);
  MapCands cd;
  fm_map_cands(f, rd.pat.p, rd.off.p, 2 * npat, min_seed, k, thresholds, cd);
  MapSel sel;
  fm_map_select(f, rd.off.p, npat, k, max_sec, cd, hit_off, mapq, nhits, sel);
  cd.drop_triples();
  if (strand) fm_map_fill(f, rd.pat.p, rd.off.p, npat, k, cd.aln_off.p, hit_off, sel, strand, seq, off, start, dist, cig_off, cig, md_off, md);
  sync(f.c);
}

}  // namespace pfp
