// api_debug.hip -- micro and diagnostic entry points: a text staged once and scanned on its own (pfp_stage_text_dev,
// pfp_scan_staged, pfp_scan_k1_enqueue), the library sorts on caller data, the fused chain's scan with a
// report of what it did (pfp_debug_*).
#include "api.hpp"

using namespace pfp;

struct K1Scratch { DBuf<uint16_t> flags; DBuf<uint32_t> bcnt; DBuf<unsigned long long> fbad; uint64_t n = 0; };

void pfp::release_debug_state(pfp_ctx *c) {
  delete c->staged;
  delete c->k1scratch;
}

extern "C" {

int pfp_stage_text_dev(pfp_ctx *c, const void *d_text, uint64_t n, int w) {
  if (!c || (!d_text && n)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(w >= 1 && w <= 4096, PFP_EINVAL, "bad window");
  if (!c->staged) c->staged = new StagedText();
  c->staged->stage(c, d_text, true, n, w);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_scan_staged(pfp_ctx *c, uint64_t p, uint64_t *n_ends) {
  if (!c) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  StagedText *s = c->staged;
  PFP_REQUIRE(s && s->buf.p, PFP_EINVAL, "no staged text");
  DBuf<uint64_t> d_ends;
  uint64_t used = 0;
  uint64_t k = scan_text(c, *s, s->n, s->w, p, d_ends, &used);
  sync(c);
  if (n_ends) *n_ends = k;
  return PFP_OK;
  PFP_CATCH(c)
}

// diagnostic: the library sorts (and three scans / selections) exactly as the suffix sorter calls them - through the wrappers of
// prims.hip, with their size thresholds, configurations and work-arounds - on caller data (pfpgpu.h: pfp_debug_lib_sort)
int pfp_debug_lib_sort(pfp_ctx *c, int kind, void *keys, void *vals, uint64_t n, int begin_bit, int end_bit,
                       const uint32_t *seg_begin, const uint32_t *seg_end, uint64_t nseg) {
  if (!c || kind < 0 || kind > 9 || (n && !keys)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  if (!n) return PFP_OK;
  const bool seg = kind >= 4 && kind <= 6;
  PFP_REQUIRE(kind == 2 || kind == 3 || kind == 7 || vals, PFP_EINVAL, "pfp_debug_lib_sort: this kind needs vals");
  PFP_REQUIRE(!seg || (nseg && seg_begin && seg_end && n < 0xFFFFFFFFull), PFP_EINVAL, "pfp_debug_lib_sort: a segmented sort needs its segments");
  if (seg)
    for (uint64_t k = 0; k < nseg; k++)
      PFP_REQUIRE(seg_begin[k] <= seg_end[k] && seg_end[k] <= n, PFP_EINVAL, "pfp_debug_lib_sort: segment outside the array");
  DBuf<uint32_t> sb, se;
  if (seg) { sb.alloc(c, nseg); se.alloc(c, nseg); h2d(c, sb.p, seg_begin, nseg); h2d(c, se.p, seg_end, nseg); }
  auto pairs_db = [&](auto ktag, auto vtag) {
    using K = decltype(ktag); using V = decltype(vtag);
    DBuf<K> k(c, n), ka(c, n); DBuf<V> v(c, n), va(c, n);
    h2d(c, k.p, (const K *)keys, n); h2d(c, v.p, (const V *)vals, n);
    sort_pairs_db(c, k, ka, v, va, n, begin_bit, end_bit);
    d2h(c, (K *)keys, k.p, n); d2h(c, (V *)vals, v.p, n);
    sync(c);
  };
  // (a segmented sort leaves what lies outside every segment unwritten: the outputs start as copies of the inputs)
  auto seg_pairs = [&](auto ktag, auto vtag) {
    using K = decltype(ktag); using V = decltype(vtag);
    DBuf<K> k(c, n), ko(c, n); DBuf<V> v(c, n), vo(c, n);
    h2d(c, k.p, (const K *)keys, n); h2d(c, v.p, (const V *)vals, n);
    h2d(c, ko.p, (const K *)keys, n); h2d(c, vo.p, (const V *)vals, n);
    if constexpr (sizeof(K) == 4) segsort_pairs_u32<V>(c, k.p, ko.p, v.p, vo.p, n, nseg, sb.p, se.p, begin_bit, end_bit);
    else segsort_pairs_u64_u32(c, k.p, ko.p, v.p, vo.p, n, nseg, sb.p, se.p, begin_bit, end_bit);
    d2h(c, (K *)keys, ko.p, n); d2h(c, (V *)vals, vo.p, n);
    sync(c);
  };
  switch (kind) {
    case 0: pairs_db(uint64_t(), uint32_t()); break;
    case 1: pairs_db(uint64_t(), uint64_t()); break;
    case 2: {
      DBuf<uint64_t> k(c, n), ka(c, n);
      h2d(c, k.p, (const uint64_t *)keys, n);
      sort_keys_db(c, k, ka, n, begin_bit, end_bit);
      d2h(c, (uint64_t *)keys, k.p, n);
      sync(c);
    } break;
    case 3: {
      DBuf<uint64_t> k(c, n), ko(c, n);
      h2d(c, k.p, (const uint64_t *)keys, n);
      sort_keys_raw(c, k.p, ko.p, n, begin_bit, end_bit);
      d2h(c, (uint64_t *)keys, ko.p, n);
      sync(c);
    } break;
    case 4: seg_pairs(uint32_t(), uint32_t()); break;
    case 5: seg_pairs(uint32_t(), uint64_t()); break;
    case 6: seg_pairs(uint64_t(), uint32_t()); break;
    case 7: {
      DBuf<uint32_t> a(c, n), b(c, n);
      h2d(c, a.p, (const uint32_t *)keys, n);
      inclusive_max_u32(c, a.p, b.p, n);
      d2h(c, (uint32_t *)keys, b.p, n);
      sync(c);
    } break;
    case 8: {
      DBuf<uint32_t> a(c, n); DBuf<uint64_t> b(c, n);
      h2d(c, a.p, (const uint32_t *)keys, n);
      exclusive_sum_u32_u64(c, a.p, b.p, n);
      d2h(c, (uint64_t *)vals, b.p, n);
      sync(c);
    } break;
    default: {
      DBuf<uint8_t> f(c, n + 16); DBuf<uint32_t> o(c, n); DBuf<uint64_t> cnt(c, 1);
      PFP_REQUIRE(n < 0xFFFFFFFFull, PFP_ELIMIT, "pfp_debug_lib_sort: selection of 2^32 or more flags");
      h2d(c, f.p, (const uint8_t *)keys, n);
      PFP_HIP(hipMemsetAsync(f.p + n, 0, 16, c->stream));
      select_index<uint32_t>(c, f.p, o.p, cnt.p, n);
      const uint64_t got = read_scalar(c, cnt.p);
      PFP_REQUIRE(got <= n, PFP_EHIP, "pfp_debug_lib_sort: selection count beyond n");
      d2h(c, (uint32_t *)vals, o.p, got);
      sync(c);
      ((uint32_t *)vals)[n] = (uint32_t)got;
    } break;
  }
  return PFP_OK;
  PFP_CATCH(c)
}

// diagnostic: stage 1a as the fused chain runs it - scan_text_adaptive under the context's settings - or, with a plan, as a rank of
// the multi-GPU chain runs it (pfp_dist_local_parse2: params_from_plan, the given extra hashes, scan_text); see pfpgpu.h
int pfp_debug_scan_chain(pfp_ctx *c, const uint8_t *text, uint64_t n, int w, uint64_t p, const uint64_t *plan,
                         const uint32_t *extra_hashes, uint32_t n_extra, uint64_t **ends, uint64_t **dense_ends, uint8_t **nominal,
                         pfp_scan_report *rep) {
  if (!c || (!text && n) || !ends || !rep || (n_extra && !extra_hashes)) return PFP_EINVAL;
  *ends = nullptr;
  if (dense_ends) *dense_ends = nullptr;
  if (nominal) *nominal = nullptr;
  memset(rep, 0, sizeof *rep);
  PFP_TRY_DEV(c)
  check_args(w, p, 0);
  PFP_REQUIRE(n_extra <= KRParams::kMaxExtra, PFP_EINVAL, "too many extra trigger hashes");
  StagedText tx;
  tx.stage(c, text, false, n, w);
  DBuf<uint64_t> d_ends;
  uint64_t used = n, k = 0;
  ScanReport sr;
  if (plan) {
    KRParams kp = params_from_plan(w, p, plan);
    for (uint32_t q = 0; q < n_extra; q++) { kp.extra[kp.nextra++] = extra_hashes[q]; kp.bloom |= 1ull << (extra_hashes[q] & 63); }
    k = scan_text(c, tx, n, w, p, d_ends, &used, &kp);
    sr.first = sr.kp = kp;
    rep->parse_density = kp.fast ? (double)kp.fdens : 1.0;
  } else {
    uint32_t nx = 0;
    k = scan_text_adaptive(c, tx, n, w, p, c->max_phrase, d_ends, &used, &nx, &sr);
    rep->parse_density = c->stats.parse_density;
  }
  uint64_t *h = host_alloc<uint64_t>(k);
  if (k) d2h(c, h, d_ends.p, k);
  sync(c);
  *ends = h;
  const KRParams &kp = sr.kp;
  rep->n_used = used; rep->n_ends = k;
  // (seed and nominal threshold are the first pass's: only the Karp-Rabin fall-back, which has neither, ever replaces them)
  rep->fast = kp.fast; rep->fthr = kp.fthr; rep->fseed = sr.first.fseed; rep->fthr_nom = sr.first.fthr_nom;
  rep->fauto = sr.first.fauto; rep->fthr_first = sr.first.fthr; rep->density = (double)sr.first.fdens;
  rep->n_extra = kp.nextra;
  for (uint32_t q = 0; q < kp.nextra; q++) rep->extra[q] = kp.extra[q];
  rep->chose = sr.chose; rep->dense = sr.dense; rep->kr_fallback = sr.kr_fallback;
  rep->dense_cuts = sr.dense_ends.size();
  for (uint8_t f : sr.nominal) rep->n_nominal += f != 0;
  rep->sampled = sr.sampled; rep->kept = sr.kept; rep->distinct = sr.distinct; rep->singles = sr.singles;
  if (dense_ends && rep->dense_cuts) {
    *dense_ends = host_alloc<uint64_t>(rep->dense_cuts);
    memcpy(*dense_ends, sr.dense_ends.data(), rep->dense_cuts * 8);
  }
  if (nominal && rep->dense_cuts) {
    *nominal = host_alloc<uint8_t>(rep->dense_cuts);
    memcpy(*nominal, sr.nominal.data(), rep->dense_cuts);
  }
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_scan_k1_enqueue(pfp_ctx *c, uint64_t p) {
  if (!c) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  StagedText *s = c->staged;
  PFP_REQUIRE(s && s->buf.p, PFP_EINVAL, "no staged text");
  // scratch kept across calls so that the enqueue itself does no allocation
  if (!c->k1scratch) c->k1scratch = new K1Scratch();
  K1Scratch &sc = *c->k1scratch;
  uint64_t nchunks = cdiv64(s->n, 16);
  if (sc.n != s->n || !sc.flags.p) {
    sc.flags.alloc(c, nchunks + 1); sc.bcnt.alloc(c, cdiv64(nchunks, 256) + 1); sc.fbad.alloc(c, 1); sc.n = s->n;
  }
  scan_flags(c, s->tbase(), s->n, s->w, p, sc.flags.p, sc.bcnt.p, sc.fbad.p);
  return PFP_OK;
  PFP_CATCH(c)
}

}  // extern "C"
