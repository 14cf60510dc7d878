// api_fm.hip -- searching a BWT (fmsearch.hip; the r-index of Gagie, Navarro and Prezza, PHONI for matching statistics: no
// reference counterpart): struct pfp_fm and every pfp_fm_* call; the LCP array and thresholds (lcp.hip): pfp_lcp_*; the sequences
// of a collection (seqmap.hip); extending seeds (fmextend.hip).
#include <memory>
#include <vector>
#include "api.hpp"

using namespace pfp;

struct pfp_fm {
  pfp::FmIndex f;
};

// a malloc'ed result array that grows group by group
template <class T>
struct HostOut {
  T *p = nullptr;
  uint64_t n = 0;
  ~HostOut() { free(p); }
  // room for `more` entries behind the n held; returns where they go
  T *grow(uint64_t more) {
    T *q = (T *)realloc(p, (n + more ? n + more : 1) * sizeof(T));
    if (!q) throw Error(PFP_ENOMEM, "host malloc failed");
    p = q;
    return p + n;
  }
  T *release() { T *q = n ? p : nullptr; if (!n) free(p); p = nullptr; return q; }
};

// `count` device values behind the n held
template <class T>
static void apx_take(pfp_ctx *c, HostOut<T> &out, const T *d_src, uint64_t count) {
  if (!count) return;
  download(c, out.grow(count), (const uint8_t *)d_src, count * sizeof(T));
  sync(c);      // (the next download fills the same pinned buffers)
  out.n += count;
}

extern "C" {

// host patterns: the bytes to copy (pat_off[npat]), once the offsets are known to be non-decreasing (no kernel reads past them)
static uint64_t pattern_bytes(const uint8_t *pat, const uint64_t *pat_off, uint64_t npat) {
  if (!npat) return 0;
  for (uint64_t p = 0; p < npat; p++)
    PFP_REQUIRE(pat_off[p] <= pat_off[p + 1], PFP_EINVAL, "pattern offsets decrease at pattern " + std::to_string(p));
  PFP_REQUIRE(pat || !pat_off[npat], PFP_EINVAL, "no pattern bytes");
  return pat_off[npat];
}

int pfp_fm_build_dev(pfp_ctx *c, const void *d_bwt, uint64_t n_plus_1, const void *d_ssa10, uint64_t ssa_bytes, const void *d_esa10,
                     uint64_t esa_bytes, pfp_fm **out) {
  if (!c || !d_bwt || !out) return PFP_EINVAL;
  *out = nullptr;
  PFP_TRY_DEV(c)
  auto fm = std::make_unique<pfp_fm>();
  fm_build(c, fm->f, (const uint8_t *)d_bwt, n_plus_1, (const uint8_t *)d_ssa10, ssa_bytes, (const uint8_t *)d_esa10, esa_bytes);
  *out = fm.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_build_files(pfp_ctx *c, const char *base, int flags, pfp_fm **out) {
  if (!c || !base || !out) return PFP_EINVAL;
  *out = nullptr;
  PFP_TRY_DEV(c)
  const std::string b(base);
  const int samp = flags & (PFP_FLAG_SSA | PFP_FLAG_ESA);
  PFP_REQUIRE(samp == 0 || samp == (PFP_FLAG_SSA | PFP_FLAG_ESA), PFP_EINVAL, "the run samples come as a pair: .ssa and .esa, or neither");
  auto fm = std::make_unique<pfp_fm>();
  // (the index adopts the buffer the file is read into: it has the room fm_build wants behind the rows)
  const uint64_t n1 = file_to_dev(c, b + ".bwt", fm->f.bwt, [](uint64_t rows) { check_bwt_rows(rows); return fm_bwt_bytes(rows); });
  DBuf<uint8_t> d_ssa, d_esa;
  uint64_t ssa_bytes = 0, esa_bytes = 0;
  if (samp) {
    ssa_bytes = file_to_dev(c, b + ".ssa", d_ssa);
    esa_bytes = file_to_dev(c, b + ".esa", d_esa);
  }
  fm_build(c, fm->f, fm->f.bwt.p, n1, d_ssa.p, ssa_bytes, d_esa.p, esa_bytes);
  *out = fm.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_count_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t *d_sp, uint64_t *d_ep, uint64_t *d_first) {
  if (!fm || (npat && (!d_pat_off || !d_sp || !d_ep))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_count(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_sp, d_ep, d_first);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_locate_dev(pfp_fm *fm, uint64_t npat, const uint64_t *d_sp, const uint64_t *d_ep, const uint64_t *d_first, uint64_t max_occ,
                      uint64_t *d_out_off, uint64_t *d_pos) {
  if (!fm || !d_out_off || (npat && (!d_sp || !d_ep))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_locate(fm->f, npat, d_sp, d_ep, d_first, max_occ, d_out_off, d_pos);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_count(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t *sp, uint64_t *ep, uint64_t *first) {
  if (!fm || (npat && (!pat_off || !sp || !ep))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(!first || fm->f.samples, PFP_EINVAL, "the toehold SA[sp] needs the run samples: this index was built without .ssa / .esa");
  if (!npat) return PFP_OK;
  const uint64_t bytes = pattern_bytes(pat, pat_off, npat);
  DBuf<uint8_t> d_pat(c, bytes + 16);
  DBuf<uint64_t> d_off(c, npat + 1), d_out(c, 3 * npat);
  if (bytes) h2d(c, d_pat.p, pat, bytes);
  h2d(c, d_off.p, pat_off, npat + 1);
  fm_count(fm->f, d_pat.p, d_off.p, npat, d_out.p, d_out.p + npat, first ? d_out.p + 2 * npat : nullptr);
  d2h(c, sp, d_out.p, npat);
  d2h(c, ep, d_out.p + npat, npat);
  if (first) d2h(c, first, d_out.p + 2 * npat, npat);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_locate(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t max_occ, uint64_t *sp, uint64_t *ep,
                  uint64_t *out_off, uint64_t **pos) {
  if (!fm || !out_off || !pos || (npat && !pat_off)) return PFP_EINVAL;
  *pos = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(fm->f.samples, PFP_EINVAL, "locate needs the run samples: this index was built without .ssa / .esa (bigbwt -s -e writes them)");
  const uint64_t bytes = pattern_bytes(pat, pat_off, npat);
  DBuf<uint8_t> d_pat(c, bytes + 16);
  DBuf<uint64_t> d_off(c, npat + 1), d_rng(c, 3 * npat + 1), d_out_off(c, npat + 1);
  if (bytes) h2d(c, d_pat.p, pat, bytes);
  if (npat) h2d(c, d_off.p, pat_off, npat + 1);
  fm_count(fm->f, d_pat.p, d_off.p, npat, d_rng.p, d_rng.p + npat, d_rng.p + 2 * npat);
  d_pat.release();
  fm_locate(fm->f, npat, d_rng.p, d_rng.p + npat, d_rng.p + 2 * npat, max_occ, d_out_off.p, nullptr);
  d2h(c, out_off, d_out_off.p, npat + 1);
  if (sp) d2h(c, sp, d_rng.p, npat);
  if (ep) d2h(c, ep, d_rng.p + npat, npat);
  sync(c);
  const uint64_t total = out_off[npat];
  if (total) {
    DBuf<uint64_t> d_pos(c, total);
    fm_locate(fm->f, npat, d_rng.p, d_rng.p + npat, d_rng.p + 2 * npat, max_occ, d_out_off.p, d_pos.p);
    *pos = (uint64_t *)fetch_bytes(c, (const uint8_t *)d_pos.p, total * 8);
  }
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- approximate search (fmapprox.hip)
int pfp_fm_approx_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, int k, uint64_t *d_hit_off, uint64_t *d_sp,
                      uint64_t *d_ep, uint64_t *d_first, uint8_t *d_dist) {
  if (!fm || !d_hit_off || (npat && !d_pat_off)) return PFP_EINVAL;
  const bool fill = d_sp || d_ep || d_dist;
  if (fill && !(d_sp && d_ep && d_dist)) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_approx(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, k, d_hit_off, d_sp, d_ep, d_first, d_dist);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_approx_stats(pfp_fm *fm, uint64_t out[3]) {
  if (!fm || !out) return PFP_EINVAL;
  memcpy(out, fm->f.apx_stats, sizeof fm->f.apx_stats);
  memset(fm->f.apx_stats, 0, sizeof fm->f.apx_stats);
  return PFP_OK;
}

// host patterns on the device with their hit counts: cnt on the device (npat + 1), hcnt on the host
struct ApxCall {
  DBuf<uint8_t> pat;
  DBuf<uint64_t> off, cnt;
  std::vector<uint64_t> hcnt;
  uint64_t budget = PFP_SEQ_BUDGET;
  // the end of the group of consecutive entries that starts at p0: their sum stays within the budget, a larger entry goes alone
  uint64_t group_end(const std::vector<uint64_t> &per, uint64_t p0, uint64_t end) const {
    uint64_t p1 = p0 + 1, sum = per[p0];
    while (p1 < end && sum + per[p1] <= budget) sum += per[p1++];
    return p1;
  }
};
static void apx_call_begin(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, bool toehold, ApxCall &s) {
  pfp_ctx *c = fm->f.c;
  fm_approx_check(fm->f, k, toehold);
  if (const char *e = getenv("PFP_FM_SEQ_BUDGET")) {    // (tests: a small budget cuts a small call into groups)
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < s.budget) s.budget = v;
  }
  const uint64_t bytes = pattern_bytes(pat, pat_off, npat);
  s.pat.alloc(c, bytes + 16);
  s.off.alloc(c, npat + 1);
  s.cnt.alloc(c, npat + 1);
  s.hcnt.assign(npat + 1, 0);
  if (bytes) h2d(c, s.pat.p, pat, bytes);
  if (npat) h2d(c, s.off.p, pat_off, npat + 1);
  fm_approx_count(fm->f, s.pat.p, s.off.p, npat, k, s.cnt.p);
  d2h(c, s.hcnt.data(), s.cnt.p, npat + 1);
  sync(c);
}
// the hits of patterns [p0, p1) on the device
struct ApxHits {
  DBuf<uint64_t> hoff, sp, ep, first;
  DBuf<uint8_t> dist;
  uint64_t H = 0;
};
static void apx_group_hits(pfp_fm *fm, const ApxCall &s, uint64_t p0, uint64_t p1, int k, bool toehold, ApxHits &h) {
  pfp_ctx *c = fm->f.c;
  const uint64_t np = p1 - p0;
  h.H = 0;
  for (uint64_t p = p0; p < p1; p++) h.H += s.hcnt[p];
  h.hoff.alloc(c, np + 1);
  exclusive_sum_u64(c, s.cnt.p + p0, h.hoff.p, np + 1);   // (entry np of the input does not reach the sums)
  h.sp.alloc(c, h.H); h.ep.alloc(c, h.H); h.dist.alloc(c, h.H);
  if (toehold) h.first.alloc(c, h.H);
  fm_approx_fill(fm->f, s.pat.p, s.off.p + p0, np, k, h.hoff.p, h.H, h.sp.p, h.ep.p, toehold ? h.first.p : nullptr, h.dist.p);
}

int pfp_fm_approx(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, uint64_t *hit_off, uint64_t **sp,
                  uint64_t **ep, uint64_t **first, uint8_t **dist) {
  if (!fm || !hit_off || !sp || !ep || !dist || (npat && !pat_off)) return PFP_EINVAL;
  *sp = nullptr; *ep = nullptr; *dist = nullptr;
  if (first) *first = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  ApxCall s;
  apx_call_begin(fm, pat, pat_off, npat, k, first != nullptr, s);
  HostOut<uint64_t> h_sp, h_ep, h_first;
  HostOut<uint8_t> h_dist;
  hit_off[0] = 0;
  for (uint64_t p = 0; p < npat; p++) hit_off[p + 1] = hit_off[p] + s.hcnt[p];
  for (uint64_t p0 = 0, p1; p0 < npat; p0 = p1) {
    p1 = s.group_end(s.hcnt, p0, npat);
    ApxHits h;
    apx_group_hits(fm, s, p0, p1, k, first != nullptr, h);
    sync(c);
    apx_take(c, h_sp, h.sp.p, h.H);
    apx_take(c, h_ep, h.ep.p, h.H);
    apx_take(c, h_dist, h.dist.p, h.H);
    if (first) apx_take(c, h_first, h.first.p, h.H);
  }
  *sp = h_sp.release(); *ep = h_ep.release(); *dist = h_dist.release();
  if (first) *first = h_first.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_approx_locate(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, uint64_t max_occ, uint64_t *out_off,
                         uint64_t **pos, uint8_t **dist) {
  if (!fm || !out_off || !pos || !dist || (npat && !pat_off)) return PFP_EINVAL;
  *pos = nullptr; *dist = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(fm->f.samples, PFP_EINVAL, "locate needs the run samples: this index was built without .ssa / .esa (bigbwt -s -e writes them)");
  ApxCall s;
  apx_call_begin(fm, pat, pat_off, npat, k, true, s);
  HostOut<uint64_t> h_pos;
  HostOut<uint8_t> h_dist;
  std::vector<uint64_t> go, per, hbase;
  out_off[0] = 0;
  for (uint64_t p0 = 0, p1; p0 < npat; p0 = p1) {
    p1 = s.group_end(s.hcnt, p0, npat);
    const uint64_t np = p1 - p0;
    ApxHits h;
    apx_group_hits(fm, s, p0, p1, k, true, h);
    DBuf<uint64_t> d_go(c, np + 1), cep;
    fm_approx_clip(fm->f, np, h.hoff.p, h.H, h.sp.p, h.ep.p, h.first.p, max_occ, d_go.p, cep);
    go.resize(np + 1);
    d2h(c, go.data(), d_go.p, np + 1);
    sync(c);
    per.resize(np);
    hbase.assign(np + 1, 0);
    for (uint64_t i = 0; i < np; i++) {
      out_off[p0 + i + 1] = out_off[p0] + go[i + 1];
      per[i] = go[i + 1] - go[i];
      hbase[i + 1] = hbase[i] + s.hcnt[p0 + i];
    }
    // inside the group: consecutive patterns whose positions stay within the budget
    for (uint64_t q0 = 0, q1; q0 < np; q0 = q1) {
      q1 = s.group_end(per, q0, np);
      const uint64_t h0 = hbase[q0], nh = hbase[q1] - h0;
      DBuf<uint64_t> d_pos;
      DBuf<uint8_t> d_pd;
      const uint64_t U = fm_approx_positions(fm->f, nh, h.sp.p + h0, cep.p + h0, h.first.p + h0, h.dist.p + h0, d_pos, d_pd);
      if (U != go[q1] - go[q0]) throw Error(PFP_EHIP, "approximate locate: a group's positions do not add up");
      apx_take(c, h_pos, d_pos.p, U);
      apx_take(c, h_dist, d_pd.p, U);
    }
  }
  *pos = h_pos.release();
  *dist = h_dist.release();
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- matching statistics and MEMs (fmsearch.hip: PHONI)
int pfp_fm_build_ms_dev(pfp_ctx *c, const void *d_bwt, uint64_t n_plus_1, const void *d_ssa10, uint64_t ssa_bytes, const void *d_esa10,
                        uint64_t esa_bytes, const void *d_text, pfp_fm **out) {
  if (!c || !d_bwt || !out) return PFP_EINVAL;
  *out = nullptr;
  PFP_TRY_DEV(c)
  auto fm = std::make_unique<pfp_fm>();
  fm_build_ms(c, fm->f, (const uint8_t *)d_bwt, n_plus_1, (const uint8_t *)d_ssa10, ssa_bytes, (const uint8_t *)d_esa10, esa_bytes,
              (const uint8_t *)d_text);
  *out = fm.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_build_ms_files(pfp_ctx *c, const char *base, const uint8_t *text, int text_fd, uint64_t text_offset, uint64_t n, pfp_fm **out) {
  if (!c || !base || !out) return PFP_EINVAL;
  *out = nullptr;
  PFP_TRY_DEV(c)
  const std::string b(base);
  auto fm = std::make_unique<pfp_fm>();
  DBuf<uint8_t> d_bwt, d_ssa, d_esa;
  const uint64_t n1 = file_to_dev(c, b + ".bwt", d_bwt);
  check_bwt_rows(n1);
  const bool given = text || text_fd >= 0;
  PFP_REQUIRE(!given || n + 1 == n1, PFP_EINVAL, "the text holds " + std::to_string(n) + " bytes; " + b + ".bwt holds " + std::to_string(n1) +
                                                     " rows, so its text holds " + std::to_string(n1 ? n1 - 1 : 0));
  const uint64_t ssa_bytes = file_to_dev(c, b + ".ssa", d_ssa), esa_bytes = file_to_dev(c, b + ".esa", d_esa);
  if (given) {
    fm->f.text.alloc(c, n + 16);
    upload_text(c, fm->f.text.p, text, text_fd, text_offset, n);
    sync(c);
  }
  fm_build_ms(c, fm->f, d_bwt.p, n1, d_ssa.p, ssa_bytes, d_esa.p, esa_bytes, given ? fm->f.text.p : nullptr);
  *out = fm.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_ms_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint32_t *d_len, uint64_t *d_pos) {
  if (!fm || (npat && (!d_pat_off || !d_len))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_ms(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_len, d_pos);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_mems_dev(pfp_fm *fm, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_len, const uint64_t *d_pos, uint64_t min_len,
                    uint64_t *d_mem_off, uint64_t *d_mem) {
  if (!fm || !d_mem_off || (npat && (!d_pat_off || !d_len))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_mems(fm->f, d_pat_off, npat, d_len, d_pos, min_len, d_mem_off, d_mem);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

// host patterns -> device patterns, lengths and positions (entry t of the device arrays belongs to pattern byte t)
struct MsOnDevice {
  DBuf<uint8_t> pat; DBuf<uint64_t> off, pos; DBuf<uint32_t> len;
  uint64_t first = 0, total = 0;
};
static void ms_on_device(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, MsOnDevice &d, bool thr = false) {
  pfp_ctx *c = fm->f.c;
  const uint64_t bytes = pattern_bytes(pat, pat_off, npat);
  d.first = npat ? pat_off[0] : 0;
  d.total = bytes - d.first;
  d.pat.alloc(c, bytes + 16);
  d.off.alloc(c, npat + 1);
  d.len.alloc(c, bytes + 1);
  d.pos.alloc(c, bytes + 1);
  if (bytes) h2d(c, d.pat.p, pat, bytes);
  if (npat) h2d(c, d.off.p, pat_off, npat + 1);
  if (thr) fm_ms_thr(fm->f, d.pat.p, d.off.p, npat, d.len.p, d.pos.p);
  else fm_ms(fm->f, d.pat.p, d.off.p, npat, d.len.p, d.pos.p);
}

int pfp_fm_ms_stats(pfp_fm *fm, uint64_t out[3]) {
  if (!fm || !out) return PFP_EINVAL;
  memcpy(out, fm->f.ms_stats, sizeof fm->f.ms_stats);
  memset(fm->f.ms_stats, 0, sizeof fm->f.ms_stats);
  return PFP_OK;
}

static void require_thresholds(const pfp_fm *fm) {
  PFP_REQUIRE(fm->f.has_thr, PFP_EINVAL, "this index has no thresholds: add them with pfp_fm_thresholds_dev / pfp_fm_thresholds_files");
}

static int ms_host(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos, bool thr) {
  if (!fm || (npat && (!pat_off || !len))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(fm->f.has_text, PFP_EINVAL, "matching statistics need the text and the run-end values: build the index with pfp_fm_build_ms_dev / "
                                          "pfp_fm_build_ms_files");
  if (thr) require_thresholds(fm);
  if (!npat) return PFP_OK;
  MsOnDevice d;
  ms_on_device(fm, pat, pat_off, npat, d, thr);
  if (d.total) {
    download(c, len, (const uint8_t *)(d.len.p + d.first), d.total * 4);
    sync(c);      // (the next download fills the same pinned buffers)
    if (pos) download(c, pos, (const uint8_t *)(d.pos.p + d.first), d.total * 8);
  }
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_ms(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos) {
  return ms_host(fm, pat, pat_off, npat, len, pos, false);
}
int pfp_fm_ms_thr(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos) {
  return ms_host(fm, pat, pat_off, npat, len, pos, true);
}

static int mems_host(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_len, uint64_t *mem_off, uint64_t **mems,
                     bool thr) {
  if (!fm || !mem_off || !mems || (npat && !pat_off)) return PFP_EINVAL;
  *mems = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(fm->f.has_text, PFP_EINVAL, "maximal exact matches need the text and the run-end values: build the index with pfp_fm_build_ms_dev / "
                                          "pfp_fm_build_ms_files");
  if (thr) require_thresholds(fm);
  PFP_REQUIRE(min_len >= 1, PFP_EINVAL, "min_len = 0: a maximal exact match is at least 1 byte long");
  MsOnDevice d;
  ms_on_device(fm, pat, pat_off, npat, d, thr);
  d.pat.release();
  DBuf<uint64_t> d_mem_off(c, npat + 1);
  fm_mems(fm->f, d.off.p, npat, d.len.p, d.pos.p, min_len, d_mem_off.p, nullptr);
  d2h(c, mem_off, d_mem_off.p, npat + 1);
  sync(c);
  const uint64_t total = mem_off[npat];
  if (total) {
    DBuf<uint64_t> d_mem(c, 3 * total);
    fm_mems(fm->f, d.off.p, npat, d.len.p, d.pos.p, min_len, d_mem_off.p, d_mem.p);
    *mems = (uint64_t *)fetch_bytes(c, (const uint8_t *)d_mem.p, total * 24);
  }
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_mems(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_len, uint64_t *mem_off, uint64_t **mems) {
  return mems_host(fm, pat, pat_off, npat, min_len, mem_off, mems, false);
}
int pfp_fm_mems_thr(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_len, uint64_t *mem_off, uint64_t **mems) {
  return mems_host(fm, pat, pat_off, npat, min_len, mem_off, mems, true);
}

int pfp_fm_ms_thr_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint32_t *d_len, uint64_t *d_pos) {
  if (!fm || (npat && (!d_pat_off || !d_len))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_ms_thr(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_len, d_pos);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- the LCP array and thresholds (lcp.hip)
int pfp_fm_thresholds_dev(pfp_fm *fm, const void *d_thr5, uint64_t bytes) {
  if (!fm) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  if (d_thr5) {
    fm_load_thresholds(fm->f, (const uint8_t *)d_thr5, bytes);
  } else {
    LcpOut o;
    o.keep = true;
    fm_lcp(fm->f, o);
  }
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_thresholds_files(pfp_fm *fm, const char *base) {
  if (!fm || !base) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(fm->f.has_text, PFP_EINVAL, "thresholds need the text and the run-end values: build the index with pfp_fm_build_ms_dev / "
                                          "pfp_fm_build_ms_files");
  DBuf<uint8_t> d_thr;
  const uint64_t bytes = file_to_dev(c, std::string(base) + ".thr_pos", d_thr);
  fm_load_thresholds(fm->f, d_thr.p, bytes);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_lcp_dev(pfp_ctx *c, const void *d_bwt, uint64_t n_plus_1, const void *d_ssa10, uint64_t ssa_bytes, const void *d_esa10, uint64_t esa_bytes,
                const void *d_text, uint64_t *d_lcp, uint64_t *d_thr, uint64_t *runs) {
  if (!c || !d_bwt) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  FmIndex f;
  fm_build_ms(c, f, (const uint8_t *)d_bwt, n_plus_1, (const uint8_t *)d_ssa10, ssa_bytes, (const uint8_t *)d_esa10, esa_bytes,
              (const uint8_t *)d_text);
  if (runs) *runs = f.runs;
  LcpOut o;
  o.lcp64 = d_lcp; o.thr64 = d_thr;
  if (d_lcp || d_thr) fm_lcp(f, o);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_lcp_files(pfp_ctx *c, const char *base, const uint8_t *text, int text_fd, uint64_t text_offset, uint64_t n, int what) {
  if (!c || !base) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(what && !(what & ~(PFP_LCP_LCP | PFP_LCP_THR)), PFP_EINVAL, "what: PFP_LCP_LCP, PFP_LCP_THR or both");
  const std::string b(base);
  FmIndex f;
  {
    DBuf<uint8_t> d_bwt, d_ssa, d_esa;
    const uint64_t n1 = file_to_dev(c, b + ".bwt", d_bwt);
    check_bwt_rows(n1);
    const bool given = text || text_fd >= 0;
    PFP_REQUIRE(!given || n + 1 == n1, PFP_EINVAL, "the text holds " + std::to_string(n) + " bytes; " + b + ".bwt holds " + std::to_string(n1) +
                                                       " rows, so its text holds " + std::to_string(n1 ? n1 - 1 : 0));
    const uint64_t ssa_bytes = file_to_dev(c, b + ".ssa", d_ssa), esa_bytes = file_to_dev(c, b + ".esa", d_esa);
    if (given) {
      f.text.alloc(c, n + 16);
      upload_text(c, f.text.p, text, text_fd, text_offset, n);
      sync(c);
    }
    fm_build_ms(c, f, d_bwt.p, n1, d_ssa.p, ssa_bytes, d_esa.p, esa_bytes, given ? f.text.p : nullptr);
  }
  DBuf<uint8_t> lcp5, thr5;
  LcpOut o;
  if (what & PFP_LCP_LCP) { lcp5.alloc(c, 5 * f.n1 + 16); o.lcp5 = lcp5.p; }
  if (what & PFP_LCP_THR) { thr5.alloc(c, 5 * f.runs + 16); o.thr5 = thr5.p; }
  fm_lcp(f, o);
  if (o.lcp5) write_dev_file(c, b + ".lcp", 0, lcp5.p, 5 * f.n1, true);
  if (o.thr5) write_dev_file(c, b + ".thr_pos", 0, thr5.p, 5 * f.runs, true);
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- extending seeds (fmextend.hip)
int pfp_fm_extend_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_cand_pat,
                      const int64_t *d_cand_diag, uint64_t ncand, int k, uint8_t *d_dist, uint64_t *d_start, uint64_t *d_end) {
  if (!fm || (npat && !d_pat_off) || (ncand && (!d_cand_pat || !d_cand_diag || !d_dist || !d_start || !d_end))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_extend(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_cand_pat, d_cand_diag, ncand, k, d_dist, d_start, d_end);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_extend(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat, const int64_t *cand_diag,
                  uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end) {
  if (!fm || (npat && !pat_off) || (ncand && (!cand_pat || !cand_diag || !dist || !start || !end))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_extend_check(fm->f, k);
  const uint64_t bytes = pattern_bytes(pat, pat_off, npat);
  DBuf<uint8_t> d_pat(c, bytes + 16), d_dist(c, ncand);
  DBuf<uint64_t> d_off(c, npat + 1), d_out(c, 2 * ncand);
  DBuf<uint32_t> d_cp(c, ncand);
  DBuf<int64_t> d_cd(c, ncand);
  if (bytes) h2d(c, d_pat.p, pat, bytes);
  if (npat) h2d(c, d_off.p, pat_off, npat + 1);
  if (ncand) { h2d(c, d_cp.p, cand_pat, ncand); h2d(c, d_cd.p, cand_diag, ncand); }
  fm_extend(fm->f, d_pat.p, d_off.p, npat, d_cp.p, d_cd.p, ncand, k, d_dist.p, d_out.p, d_out.p + ncand);
  if (ncand) {
    d2h(c, dist, d_dist.p, ncand);
    d2h(c, start, d_out.p, ncand);
    d2h(c, end, d_out.p + ncand, ncand);
  }
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_align_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln,
                     int thresholds, uint64_t *d_aln_off, uint64_t *d_start, uint64_t *d_end, uint8_t *d_dist) {
  if (!fm || !d_aln_off || (npat && !d_pat_off)) return PFP_EINVAL;
  const bool fill = d_start || d_end || d_dist;
  if (fill && !(d_start && d_end && d_dist)) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_align(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, min_seed, k, max_aln, thresholds != 0, d_aln_off, d_start, d_end, d_dist);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_align(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln,
                 int thresholds, uint64_t *aln_off, uint64_t **start, uint64_t **end, uint8_t **dist) {
  if (!fm || !aln_off || !start || !end || !dist || (npat && !pat_off)) return PFP_EINVAL;
  *start = nullptr; *end = nullptr; *dist = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_extend_check(fm->f, k);
  PFP_REQUIRE(min_seed >= 1, PFP_EINVAL, "min_seed = 0: a seed is a maximal exact match of at least 1 byte");
  if (thresholds) require_thresholds(fm);
  ApxCall s;                                            // (its budget and its grouping)
  if (const char *e = getenv("PFP_FM_SEQ_BUDGET")) {    // (tests: a small budget cuts a small call into groups)
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < s.budget) s.budget = v;
  }
  pattern_bytes(pat, pat_off, npat);                    // (decreasing offsets: PFP_EINVAL before the lengths are looked at)
  for (uint64_t p = 0; p < npat; p++)                   // (before any work: fm_extend_check_patterns' rule, on the host's copy)
    PFP_REQUIRE(pat_off[p + 1] - pat_off[p] <= PFP_FM_EXTEND_MAX_M, PFP_ELIMIT,
                "pattern " + std::to_string(p) + " holds more than " + std::to_string(PFP_FM_EXTEND_MAX_M) + " bytes (PFP_FM_EXTEND_MAX_M)");
  MsOnDevice d;
  ms_on_device(fm, pat, pat_off, npat, d, thresholds != 0);
  aln_off[0] = 0;
  if (!npat) return PFP_OK;
  std::vector<uint64_t> moff(npat + 1), per(npat), goff, go;
  {
    DBuf<uint64_t> d_moff(c, npat + 1);
    fm_mems(fm->f, d.off.p, npat, d.len.p, d.pos.p, min_seed, d_moff.p, nullptr);
    d2h(c, moff.data(), d_moff.p, npat + 1);
    sync(c);
  }
  for (uint64_t p = 0; p < npat; p++) per[p] = moff[p + 1] - moff[p];
  HostOut<uint64_t> h_start, h_end;
  HostOut<uint8_t> h_dist;
  for (uint64_t p0 = 0, p1; p0 < npat; p0 = p1) {       // consecutive patterns whose seeds stay within the budget
    p1 = s.group_end(per, p0, npat);
    const uint64_t np = p1 - p0;
    goff.resize(np + 1);                                // the group's MEM offsets: the call's, counted from its first pattern
    for (uint64_t i = 0; i <= np; i++) goff[i] = moff[p0 + i] - moff[p0];
    DBuf<uint64_t> g_moff(c, np + 1), g_off(c, np + 1);
    h2d(c, g_moff.p, goff.data(), np + 1);
    AlnKeys keys;
    fm_align_seeds(fm->f, d.pat.p, d.off.p + p0, np, min_seed, k, max_aln, d.len.p, d.pos.p, g_moff.p, goff[np], g_off.p, keys);
    DBuf<uint64_t> g_start(c, keys.total), g_end(c, keys.total);
    DBuf<uint8_t> g_dist(c, keys.total);
    fm_align_write(fm->f, keys, g_start.p, g_end.p, g_dist.p);
    go.resize(np + 1);
    d2h(c, go.data(), g_off.p, np + 1);
    sync(c);
    for (uint64_t i = 0; i < np; i++) aln_off[p0 + i + 1] = aln_off[p0] + go[i + 1];
    apx_take(c, h_start, g_start.p, keys.total);
    apx_take(c, h_end, g_end.p, keys.total);
    apx_take(c, h_dist, g_dist.p, keys.total);
  }
  *start = h_start.release(); *end = h_end.release(); *dist = h_dist.release();
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- sequences of a collection (seqmap.hip)
int pfp_fm_set_seqs(pfp_fm *fm, const uint64_t *starts, uint64_t nseq) {
  if (!fm) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_set_seqs(fm->f, starts, nseq);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_seqmap_dev(pfp_fm *fm, const uint64_t *d_pos, uint64_t count, uint32_t *d_seq, uint64_t *d_off) {
  if (!fm || (count && !d_pos)) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_seqmap(fm->f, d_pos, count, d_seq, d_off);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_locate_seqs_dev(pfp_fm *fm, const uint64_t *d_pat_off, uint64_t npat, const uint64_t *d_sp, const uint64_t *d_ep,
                           const uint64_t *d_first, uint64_t max_occ, uint64_t *d_out_off, uint32_t *d_seq, uint64_t *d_off) {
  if (!fm || !d_out_off || (npat && (!d_pat_off || !d_sp || !d_ep))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_locate_seqs(fm->f, d_pat_off, npat, d_sp, d_ep, d_first, max_occ, d_out_off, d_seq, d_off);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_doclist_dev(pfp_fm *fm, const uint64_t *d_pat_off, uint64_t npat, const uint64_t *d_sp, const uint64_t *d_ep,
                       const uint64_t *d_first, uint64_t *d_doc_off, uint32_t *d_doc, uint64_t *d_cnt) {
  if (!fm || !d_doc_off || (npat && (!d_pat_off || !d_sp || !d_ep))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  DocOut o;
  o.doc = d_doc; o.cnt = d_cnt;
  fm_doclist(fm->f, d_pat_off, npat, d_sp, d_ep, d_first, d_doc_off, o);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

// host patterns counted on the device, and what plain locate would list for them: uoff = its npat + 1 offsets, on the host
struct SeqCall {
  DBuf<uint64_t> off, rng;
  std::vector<uint64_t> uoff;
  uint64_t budget = PFP_SEQ_BUDGET;
  // pattern p's entry of the ranges: which = 0 sp, 1 ep, 2 the toehold
  const uint64_t *range(uint64_t p, uint64_t npat, int which) const { return rng.p + which * npat + p; }
  // the end of the group of consecutive patterns that starts at p0: at most `budget` positions, a pattern with more goes alone
  uint64_t group_end(uint64_t p0, uint64_t npat) const {
    uint64_t p1 = p0 + 1;
    while (p1 < npat && uoff[p1 + 1] - uoff[p0] <= budget) p1++;
    return p1;
  }
};
static void seq_call_begin(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t max_occ, uint64_t *sp, uint64_t *ep,
                           SeqCall &s) {
  pfp_ctx *c = fm->f.c;
  PFP_REQUIRE(fm->f.samples, PFP_EINVAL, "locate needs the run samples: this index was built without .ssa / .esa (bigbwt -s -e writes them)");
  PFP_REQUIRE(fm->f.nseq, PFP_EINVAL, "this index has no sequence table: give it one with pfp_fm_set_seqs (bigbwt -f --seqs writes it)");
  if (const char *e = getenv("PFP_FM_SEQ_BUDGET")) {    // (tests: a small budget cuts a small call into groups)
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < s.budget) s.budget = v;
  }
  const uint64_t bytes = pattern_bytes(pat, pat_off, npat);
  DBuf<uint8_t> d_pat(c, bytes + 16);
  DBuf<uint64_t> d_uoff(c, npat + 1);
  s.off.alloc(c, npat + 1);
  s.rng.alloc(c, 3 * npat + 1);
  s.uoff.assign(npat + 1, 0);
  if (bytes) h2d(c, d_pat.p, pat, bytes);
  if (npat) h2d(c, s.off.p, pat_off, npat + 1);
  fm_count(fm->f, d_pat.p, s.off.p, npat, s.rng.p, s.rng.p + npat, s.rng.p + 2 * npat);
  fm_locate(fm->f, npat, s.rng.p, s.rng.p + npat, s.rng.p + 2 * npat, max_occ, d_uoff.p, nullptr);
  d2h(c, s.uoff.data(), d_uoff.p, npat + 1);
  if (sp) d2h(c, sp, s.rng.p, npat);
  if (ep) d2h(c, ep, s.rng.p + npat, npat);
  sync(c);
}
int pfp_fm_locate_seqs(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t max_occ, uint64_t *sp,
                       uint64_t *ep, uint64_t *out_off, uint32_t **seq, uint64_t **off) {
  if (!fm || !out_off || !seq || !off || (npat && !pat_off)) return PFP_EINVAL;
  *seq = nullptr; *off = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  SeqCall s;
  seq_call_begin(fm, pat, pat_off, npat, max_occ, sp, ep, s);
  HostOut<uint32_t> h_seq;
  HostOut<uint64_t> h_off;
  std::vector<uint64_t> go;
  out_off[0] = 0;
  for (uint64_t p0 = 0, p1; p0 < npat; p0 = p1) {
    p1 = s.group_end(p0, npat);
    const uint64_t k = p1 - p0, U = s.uoff[p1] - s.uoff[p0];
    DBuf<uint64_t> d_go(c, k + 1), d_o(c, U);
    DBuf<uint32_t> d_s(c, U);
    fm_locate_seqs(fm->f, s.off.p + p0, k, s.range(p0, npat, 0), s.range(p0, npat, 1), s.range(p0, npat, 2), max_occ, d_go.p, d_s.p, d_o.p);
    go.resize(k + 1);
    d2h(c, go.data(), d_go.p, k + 1);
    sync(c);
    for (uint64_t i = 1; i <= k; i++) out_off[p0 + i] = out_off[p0] + go[i];
    const uint64_t kept = go[k];
    if (kept) {
      download(c, h_seq.grow(kept), (const uint8_t *)d_s.p, kept * 4);
      sync(c);      // (the next download fills the same pinned buffers)
      download(c, h_off.grow(kept), (const uint8_t *)d_o.p, kept * 8);
      sync(c);
      h_seq.n += kept; h_off.n += kept;
    }
  }
  *seq = h_seq.release();
  *off = h_off.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_doclist(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t *doc_off, uint32_t **doc,
                   uint64_t **cnt) {
  if (!fm || !doc_off || !doc || !cnt || (npat && !pat_off)) return PFP_EINVAL;
  *doc = nullptr; *cnt = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  SeqCall s;
  seq_call_begin(fm, pat, pat_off, npat, 0, nullptr, nullptr, s);
  HostOut<uint32_t> h_doc;
  HostOut<uint64_t> h_cnt;
  std::vector<uint64_t> go;
  doc_off[0] = 0;
  for (uint64_t p0 = 0, p1; p0 < npat; p0 = p1) {
    p1 = s.group_end(p0, npat);
    const uint64_t k = p1 - p0;
    DBuf<uint64_t> d_go(c, k + 1), d_c;
    DBuf<uint32_t> d_d;
    DocOut o;
    o.own_doc = &d_d; o.own_cnt = &d_c;      // (sized inside, once the group's total is known: nothing is listed twice)
    fm_doclist(fm->f, s.off.p + p0, k, s.range(p0, npat, 0), s.range(p0, npat, 1), s.range(p0, npat, 2), d_go.p, o);
    go.resize(k + 1);
    d2h(c, go.data(), d_go.p, k + 1);
    sync(c);
    for (uint64_t i = 1; i <= k; i++) doc_off[p0 + i] = doc_off[p0] + go[i];
    const uint64_t docs = go[k];
    if (docs) {
      download(c, h_doc.grow(docs), (const uint8_t *)d_d.p, docs * 4);
      sync(c);
      download(c, h_cnt.grow(docs), (const uint8_t *)d_c.p, docs * 8);
      sync(c);
      h_doc.n += docs; h_cnt.n += docs;
    }
  }
  *doc = h_doc.release();
  *cnt = h_cnt.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_info(const pfp_fm *fm, pfp_fm_info_t *out) {
  if (!fm || !out) return PFP_EINVAL;
  memset(out, 0, sizeof *out);
  out->n = fm->f.n1 - 1;
  out->runs = fm->f.samples ? fm->f.runs : 0;
  out->sigma = (uint32_t)fm->f.sigma;
  out->row_bits = fm->f.wide ? 64 : 32;
  out->device_bytes = fm->f.device_bytes();
  out->has_samples = fm->f.samples ? 1 : 0;
  out->has_thresholds = fm->f.has_thr ? 1 : 0;
  out->nseq = fm->f.nseq;
  return PFP_OK;
}

void pfp_fm_free(pfp_fm *fm) {
  if (!fm) return;
  (void)hipSetDevice(fm->f.c->device);
  delete fm;
}

}  // extern "C"
