// api_fm.hip -- searching a BWT (fmsearch.hip; the r-index of Gagie, Navarro and Prezza, PHONI for matching statistics: no
// reference counterpart): struct pfp_fm and every pfp_fm_* call; the LCP array and thresholds (lcp.hip): pfp_lcp_*; the sequences
// of a collection (seqmap.hip); extending seeds (fmextend.hip), aligning in a window (fmwindow.hip), edit scripts (fmcigar.hip),
// mapping reads (fmmap.hip), chaining anchors (fmchain.hip) and aligning chains (fmfill.hip).
// What the calls over host arrays share is in the anonymous namespace below: one upload of the patterns (HostPatterns), one
// budget (seq_budget) and one rule that cuts a call into groups of patterns (group_end), one way to collect a group's results
// (HostOut::take / take_offsets, fetch_group_offsets).  align, map and map_pairs also share their beginning (seed_call_begin: the
// patterns the extension reads, their matching statistics and MEM counts) and their groups of candidates (seed_groups).
#include <algorithm>
#include <memory>
#include <utility>
#include <vector>
#include "api.hpp"

using namespace pfp;

struct pfp_fm {
  pfp::FmIndex f;
};

namespace {

// the body of an entry point over device pointers: body(), then a wait for the stream (api.hpp: between PFP_TRY_DEV and PFP_CATCH)
template <class F>
int dev_call(pfp_fm *fm, F &&body, bool wait = true) {
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  body();
  if (wait) sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

// the body of an entry point that makes an index: build(the new index's FmIndex); *out gets the index once it stands
template <class F>
int build_call(pfp_ctx *c, pfp_fm **out, F &&build) {
  *out = nullptr;
  PFP_TRY_DEV(c)
  auto fm = std::make_unique<pfp_fm>();
  build(fm->f);
  *out = fm.release();
  return PFP_OK;
  PFP_CATCH(c)
}

// host patterns: the bytes to copy (pat_off[npat]), once the offsets are known to be non-decreasing (no kernel reads past them)
uint64_t pattern_bytes(const uint8_t *pat, const uint64_t *pat_off, uint64_t npat) {
  if (!npat) return 0;
  for (uint64_t p = 0; p < npat; p++)
    PFP_REQUIRE(pat_off[p] <= pat_off[p + 1], PFP_EINVAL, "pattern offsets decrease at pattern " + std::to_string(p));
  PFP_REQUIRE(pat || !pat_off[npat], PFP_EINVAL, "no pattern bytes");
  return pat_off[npat];
}

// the device copy of a call's host patterns: pat (the bytes and 16 more) and off (npat + 1), filled by upload(), which checks
// the host arrays first (pattern_bytes).  pat can go before off does
struct HostPatterns {
  DBuf<uint8_t> pat;
  DBuf<uint64_t> off;
  uint64_t npat = 0, bytes = 0;
  void upload(pfp_ctx *c, const uint8_t *h_pat, const uint64_t *h_off, uint64_t n) {
    bytes = pattern_bytes(h_pat, h_off, n);
    npat = n;
    pat.alloc(c, bytes + 16);
    off.alloc(c, npat + 1);
    if (bytes) h2d(c, pat.p, h_pat, bytes);
    if (npat) h2d(c, off.p, h_off, npat + 1);
  }
};

// What one group of a call may hold: positions, hits or seeds (PFP_FM_SEQ_BUDGET lowers it: tests cut a small call into groups)
uint64_t seq_budget() {
  uint64_t budget = PFP_SEQ_BUDGET;
  if (const char *e = getenv("PFP_FM_SEQ_BUDGET")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= 1 && v < budget) budget = v;
  }
  return budget;
}
// The grouping rule of every call that works group by group.  off: exclusive sums of what each pattern brings.  The group that
// starts at p0 is the longest run of consecutive patterns before `end` whose total stays within the budget; a pattern that
// brings more goes alone.  -> the group's end
uint64_t group_end(const uint64_t *off, uint64_t p0, uint64_t end, uint64_t budget) {
  uint64_t p1 = p0 + 1;
  while (p1 < end && off[p1 + 1] - off[p0] <= budget) p1++;
  return p1;
}

// `count` offsets on the host, counted from where a group starts, go behind the call's: base is the call's offset of that start
void rebase_offsets(uint64_t *off, uint64_t count, uint64_t base) {
  for (uint64_t i = 0; i < count; i++) off[i] += base;
}

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
  // `count` device values behind the n held
  void take(pfp_ctx *c, const T *d_src, uint64_t count) {
    if (!count) return;
    download(c, grow(count), (const uint8_t *)d_src, count * sizeof(T));
    sync(c);      // (the next download fills the same pinned buffers)
    n += count;
  }
  // `count` device offsets, counted from where a group starts, behind the n >= 1 held: they go behind the last one held, which
  // is the call's offset of the group's start.  Returns what the group brought
  T take_offsets(pfp_ctx *c, const T *d_src, uint64_t count) {
    const T base = p[n - 1];
    take(c, d_src, count);
    rebase_offsets(p + n - count, count, base);
    return p[n - 1] - base;
  }
  T *release() { T *q = n ? p : nullptr; if (!n) free(p); p = nullptr; return q; }
};

// a group's np + 1 offsets, counted from its first pattern, come to the host (go) and go behind the call's: out[0] is the
// call's offset of the group's first pattern, out[1 .. np] are written
void fetch_group_offsets(pfp_ctx *c, const uint64_t *d_go, uint64_t np, std::vector<uint64_t> &go, uint64_t *out) {
  go.resize(np + 1);
  d2h(c, go.data(), d_go, np + 1);
  sync(c);
  for (uint64_t i = 1; i <= np; i++) out[i] = out[0] + go[i];
}

void require_samples(const pfp_fm *fm) {
  PFP_REQUIRE(fm->f.samples, PFP_EINVAL, "locate needs the run samples: this index was built without .ssa / .esa (bigbwt -s -e writes them)");
}
// what: "matching statistics need", ...
void require_text(const pfp_fm *fm, const char *what) {
  PFP_REQUIRE(fm->f.has_text, PFP_EINVAL, std::string(what) + " the text and the run-end values: build the index with pfp_fm_build_ms_dev / "
                                                              "pfp_fm_build_ms_files");
}
void require_thresholds(const pfp_fm *fm) {
  PFP_REQUIRE(fm->f.has_thr, PFP_EINVAL, "this index has no thresholds: add them with pfp_fm_thresholds_dev / pfp_fm_thresholds_files");
}

// f = an index with text from base.bwt / .ssa / .esa; the text: n bytes given in memory or in a file, else inverted from the BWT
void load_ms_index(pfp_ctx *c, const std::string &b, const uint8_t *text, int text_fd, uint64_t text_offset, uint64_t n, FmIndex &f) {
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

// ---------------------------------------------------------------- approximate search (fmapprox.hip)
// host patterns on the device with their hit counts: cnt on the device (npat + 1), hit_off their exclusive sums on the host
struct ApxCall {
  HostPatterns in;
  DBuf<uint64_t> cnt;
  std::vector<uint64_t> hit_off;
};
void apx_call_begin(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, bool toehold, ApxCall &s) {
  pfp_ctx *c = fm->f.c;
  fm_approx_check(fm->f, k, toehold);
  s.in.upload(c, pat, pat_off, npat);
  s.cnt.alloc(c, npat + 1);
  s.hit_off.assign(npat + 1, 0);
  fm_approx_count(fm->f, s.in.pat.p, s.in.off.p, npat, k, s.cnt.p);
  d2h(c, s.hit_off.data(), s.cnt.p, npat + 1);
  sync(c);
  uint64_t sum = 0;      // the counts become their sums (entry npat of the counts does not reach them)
  for (uint64_t p = 0; p <= npat; p++) { const uint64_t n = s.hit_off[p]; s.hit_off[p] = sum; sum += n; }
}
// the hits of patterns [p0, p1) on the device
struct ApxHits {
  DBuf<uint64_t> hoff, sp, ep, first;
  DBuf<uint8_t> dist;
  uint64_t H = 0;
};
void apx_group_hits(pfp_fm *fm, const ApxCall &s, uint64_t p0, uint64_t p1, int k, bool toehold, ApxHits &h) {
  pfp_ctx *c = fm->f.c;
  const uint64_t np = p1 - p0;
  h.H = s.hit_off[p1] - s.hit_off[p0];
  h.hoff.alloc(c, np + 1);
  exclusive_sum_u64(c, s.cnt.p + p0, h.hoff.p, np + 1);   // (entry np of the input does not reach the sums)
  h.sp.alloc(c, h.H); h.ep.alloc(c, h.H); h.dist.alloc(c, h.H);
  if (toehold) h.first.alloc(c, h.H);
  fm_approx_fill(fm->f, s.in.pat.p, s.in.off.p + p0, np, k, h.hoff.p, h.H, h.sp.p, h.ep.p, toehold ? h.first.p : nullptr, h.dist.p);
}

// ---------------------------------------------------------------- matching statistics and MEMs (fmsearch.hip: PHONI)
// host patterns -> device patterns (in.upload), lengths and positions (entry t of the device arrays belongs to pattern byte t)
struct MsOnDevice {
  HostPatterns in;
  DBuf<uint32_t> len;
  DBuf<uint64_t> pos;
  // the statistics of n device patterns whose offsets end at `bytes`: the upload, or what a caller has put in its place
  void stats(pfp_fm *fm, const uint8_t *pat, const uint64_t *off, uint64_t n, uint64_t bytes, bool thr) {
    len.alloc(fm->f.c, bytes + 1);
    pos.alloc(fm->f.c, bytes + 1);
    (thr ? fm_ms_thr : fm_ms)(fm->f, pat, off, n, len.p, pos.p);
  }
};

int ms_host(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos, bool thr) {
  if (!fm || (npat && (!pat_off || !len))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  require_text(fm, "matching statistics need");
  if (thr) require_thresholds(fm);
  if (!npat) return PFP_OK;
  MsOnDevice d;
  d.in.upload(c, pat, pat_off, npat);
  d.stats(fm, d.in.pat.p, d.in.off.p, npat, d.in.bytes, thr);
  const uint64_t first = pat_off[0], total = d.in.bytes - first;
  if (total) {
    download(c, len, (const uint8_t *)(d.len.p + first), total * 4);
    sync(c);      // (the next download fills the same pinned buffers)
    if (pos) download(c, pos, (const uint8_t *)(d.pos.p + first), total * 8);
  }
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int mems_host(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_len, uint64_t *mem_off, uint64_t **mems,
              bool thr) {
  if (!fm || !mem_off || !mems || (npat && !pat_off)) return PFP_EINVAL;
  *mems = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  require_text(fm, "maximal exact matches need");
  if (thr) require_thresholds(fm);
  PFP_REQUIRE(min_len >= 1, PFP_EINVAL, "min_len = 0: a maximal exact match is at least 1 byte long");
  MsOnDevice d;
  d.in.upload(c, pat, pat_off, npat);
  d.stats(fm, d.in.pat.p, d.in.off.p, npat, d.in.bytes, thr);
  d.in.pat.release();
  DBuf<uint64_t> d_mem_off(c, npat + 1);
  fm_mems(fm->f, d.in.off.p, npat, d.len.p, d.pos.p, min_len, d_mem_off.p, nullptr);
  d2h(c, mem_off, d_mem_off.p, npat + 1);
  sync(c);
  const uint64_t total = mem_off[npat];
  if (total) {
    DBuf<uint64_t> d_mem(c, 3 * total);
    fm_mems(fm->f, d.in.off.p, npat, d.len.p, d.pos.p, min_len, d_mem_off.p, d_mem.p);
    *mems = (uint64_t *)fetch_bytes(c, (const uint8_t *)d_mem.p, total * 24);
  }
  return PFP_OK;
  PFP_CATCH(c)
}

int ms_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint32_t *d_len, uint64_t *d_pos, bool thr) {
  if (!fm || (npat && (!d_pat_off || !d_len))) return PFP_EINVAL;
  return dev_call(fm, [&] { (thr ? fm_ms_thr : fm_ms)(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_len, d_pos); });
}

// ---------------------------------------------------------------- seed-and-extend (fmextend.hip, fmmap.hip, fmpair.hip)
// fm_extend_check_patterns' rule on the host's copy of the offsets, before any work; noun: what the caller calls a pattern
void require_extendable(const uint64_t *pat_off, uint64_t npat, const char *noun) {
  for (uint64_t p = 0; p < npat; p++)
    PFP_REQUIRE(pat_off[p + 1] - pat_off[p] <= PFP_FM_EXTEND_MAX_M, PFP_ELIMIT,
                std::string(noun) + " " + std::to_string(p) + " holds more than " + std::to_string(PFP_FM_EXTEND_MAX_M) + " bytes (PFP_FM_EXTEND_MAX_M)");
}

// MsOnDevice for the patterns the extension reads - pat / off, n of them: the upload itself, or both strands of every read (rd;
// n = 2 npat; the uploaded bytes go once the strands stand) - and moff, their n + 1 MEM offsets, on the host
struct SeedCall : MsOnDevice {
  MapReads rd;
  const uint8_t *pat = nullptr;
  const uint64_t *off = nullptr;
  uint64_t n = 0, min_seed = 0;
  int k = 0;
  std::vector<uint64_t> moff;
};
// the caller has checked k, min_seed and the thresholds; noun: require_extendable's (extendable = false: patterns of any length,
// for the callers that put them through no band).  Without patterns nothing but the upload
void seed_call_begin(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const char *noun, bool strands, uint64_t min_seed, int k,
                     bool thresholds, SeedCall &s, bool extendable = true) {
  FmIndex &f = fm->f;
  pfp_ctx *c = f.c;
  s.min_seed = min_seed; s.k = k;
  s.in.upload(c, pat, pat_off, npat);                   // (decreasing offsets: PFP_EINVAL before the lengths are looked at)
  if (extendable) require_extendable(pat_off, npat, noun);
  if (!npat) return;
  s.pat = s.in.pat.p; s.off = s.in.off.p; s.n = npat;
  uint64_t bytes = s.in.bytes;
  if (strands) {
    fm_map_strands(f, s.pat, s.off, npat, s.rd, !extendable);
    s.in.pat.release();
    s.pat = s.rd.pat.p; s.off = s.rd.off.p; s.n = 2 * npat;
    bytes = 2 * (pat_off[npat] - pat_off[0]);
  }
  s.stats(fm, s.pat, s.off, s.n, bytes, thresholds);
  s.moff.resize(s.n + 1);
  DBuf<uint64_t> d_moff(c, s.n + 1);
  fm_mems(f, s.off, s.n, s.len.p, s.pos.p, min_seed, d_moff.p, nullptr);
  d2h(c, s.moff.data(), d_moff.p, s.n + 1);
  sync(c);
}
// The groups of a seeded call: consecutive units of `unit` patterns (1: a pattern, 2: a read's strands, 4: a pair's) whose seeds
// stay within the budget (group_end); body(first pattern, patterns, their candidates: at most max_aln per pattern, 0: all) runs
// per group.  hold_keys: the keys live until the body, which fetches results and so waits for the stream, returns
template <class F>
void seed_groups(pfp_fm *fm, const SeedCall &s, uint64_t unit, uint64_t max_aln, bool hold_keys, F &&body) {
  pfp_ctx *c = fm->f.c;
  if (!s.n) return;
  const uint64_t budget = seq_budget(), nunit = s.n / unit;
  std::vector<uint64_t> uoff(nunit + 1), goff;
  for (uint64_t u = 0; u <= nunit; u++) uoff[u] = s.moff[unit * u];             // a unit brings the seeds of all its patterns
  for (uint64_t u0 = 0, u1; u0 < nunit; u0 = u1) {
    u1 = group_end(uoff.data(), u0, nunit, budget);
    const uint64_t p0 = unit * u0, np = unit * (u1 - u0);
    goff.resize(np + 1);                                // the group's MEM offsets: the call's, counted from its first pattern
    for (uint64_t i = 0; i <= np; i++) goff[i] = s.moff[p0 + i] - s.moff[p0];
    DBuf<uint64_t> g_moff(c, np + 1);
    h2d(c, g_moff.p, goff.data(), np + 1);
    AlnKeys keys;
    MapCands cd;
    fm_map_cands_ms(fm->f, s.pat, s.off + p0, np, s.min_seed, s.k, max_aln, s.len.p, s.pos.p, g_moff.p, goff[np], cd, hold_keys ? &keys : nullptr);
    body(p0, np, cd);
  }
}

// The groups of a call that lists anchors (fmchain.hip), cut as seed_groups cuts them: body(first pattern, patterns, their
// anchor offsets counted from the group's first, the triples, their number, the skipped MEMs per pattern) runs per group
template <class F>
void anchor_groups(pfp_fm *fm, const SeedCall &s, uint64_t unit, uint64_t max_occ, F &&body) {
  pfp_ctx *c = fm->f.c;
  if (!s.n) return;
  const uint64_t budget = seq_budget(), nunit = s.n / unit;
  std::vector<uint64_t> uoff(nunit + 1), goff;
  for (uint64_t u = 0; u <= nunit; u++) uoff[u] = s.moff[unit * u];
  for (uint64_t u0 = 0, u1; u0 < nunit; u0 = u1) {
    u1 = group_end(uoff.data(), u0, nunit, budget);
    const uint64_t p0 = unit * u0, np = unit * (u1 - u0);
    goff.resize(np + 1);
    for (uint64_t i = 0; i <= np; i++) goff[i] = s.moff[p0 + i] - s.moff[p0];
    DBuf<uint64_t> g_moff(c, np + 1), d_aoff(c, np + 1), d_anc;
    DBuf<uint32_t> d_skip(c, np);
    h2d(c, g_moff.p, goff.data(), np + 1);
    const uint64_t total = fm_anchors_ms(fm->f, s.pat, s.off + p0, np, s.min_seed, max_occ, s.len.p, s.pos.p, g_moff.p, goff[np], d_aoff.p, d_anc,
                                         d_skip.p);
    body(p0, np, d_aoff, d_anc, total, d_skip);
  }
}

// ---------------------------------------------------------------- sequences of a collection (seqmap.hip)
// host patterns counted on the device, and what plain locate would list for them: uoff = its npat + 1 offsets, on the host
struct SeqCall {
  HostPatterns in;      // (its bytes go once the patterns are counted; off stays for the groups)
  DBuf<uint64_t> rng;
  std::vector<uint64_t> uoff;
  // pattern p's entry of the ranges: which = 0 sp, 1 ep, 2 the toehold
  const uint64_t *range(uint64_t p, int which) const { return rng.p + which * in.npat + p; }
};
void seq_call_begin(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t max_occ, uint64_t *sp, uint64_t *ep,
                    SeqCall &s) {
  pfp_ctx *c = fm->f.c;
  require_samples(fm);
  PFP_REQUIRE(fm->f.nseq, PFP_EINVAL, "this index has no sequence table: give it one with pfp_fm_set_seqs (bigbwt -f --seqs writes it)");
  s.in.upload(c, pat, pat_off, npat);
  DBuf<uint64_t> d_uoff(c, npat + 1);
  s.rng.alloc(c, 3 * npat + 1);
  s.uoff.assign(npat + 1, 0);
  fm_count(fm->f, s.in.pat.p, s.in.off.p, npat, s.rng.p, s.rng.p + npat, s.rng.p + 2 * npat);
  fm_locate(fm->f, npat, s.rng.p, s.rng.p + npat, s.rng.p + 2 * npat, max_occ, d_uoff.p, nullptr);
  d2h(c, s.uoff.data(), d_uoff.p, npat + 1);
  if (sp) d2h(c, sp, s.rng.p, npat);
  if (ep) d2h(c, ep, s.rng.p + npat, npat);
  sync(c);
  s.in.pat.release();
}

}  // namespace

extern "C" {

int pfp_fm_build_dev(pfp_ctx *c, const void *d_bwt, uint64_t n_plus_1, const void *d_ssa10, uint64_t ssa_bytes, const void *d_esa10,
                     uint64_t esa_bytes, pfp_fm **out) {
  if (!c || !d_bwt || !out) return PFP_EINVAL;
  return build_call(c, out, [&](FmIndex &f) {
    fm_build(c, f, (const uint8_t *)d_bwt, n_plus_1, (const uint8_t *)d_ssa10, ssa_bytes, (const uint8_t *)d_esa10, esa_bytes);
  });
}

int pfp_fm_build_files(pfp_ctx *c, const char *base, int flags, pfp_fm **out) {
  if (!c || !base || !out) return PFP_EINVAL;
  return build_call(c, out, [&](FmIndex &f) {
    const std::string b(base);
    const int samp = flags & (PFP_FLAG_SSA | PFP_FLAG_ESA);
    PFP_REQUIRE(samp == 0 || samp == (PFP_FLAG_SSA | PFP_FLAG_ESA), PFP_EINVAL, "the run samples come as a pair: .ssa and .esa, or neither");
    // (the index adopts the buffer the file is read into: it has the room fm_build wants behind the rows)
    const uint64_t n1 = file_to_dev(c, b + ".bwt", f.bwt, [](uint64_t rows) { check_bwt_rows(rows); return fm_bwt_bytes(rows); });
    DBuf<uint8_t> d_ssa, d_esa;
    uint64_t ssa_bytes = 0, esa_bytes = 0;
    if (samp) {
      ssa_bytes = file_to_dev(c, b + ".ssa", d_ssa);
      esa_bytes = file_to_dev(c, b + ".esa", d_esa);
    }
    fm_build(c, f, f.bwt.p, n1, d_ssa.p, ssa_bytes, d_esa.p, esa_bytes);
  });
}

int pfp_fm_count_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t *d_sp, uint64_t *d_ep, uint64_t *d_first) {
  if (!fm || (npat && (!d_pat_off || !d_sp || !d_ep))) return PFP_EINVAL;
  return dev_call(fm, [&] { fm_count(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_sp, d_ep, d_first); });
}

int pfp_fm_locate_dev(pfp_fm *fm, uint64_t npat, const uint64_t *d_sp, const uint64_t *d_ep, const uint64_t *d_first, uint64_t max_occ,
                      uint64_t *d_out_off, uint64_t *d_pos) {
  if (!fm || !d_out_off || (npat && (!d_sp || !d_ep))) return PFP_EINVAL;
  return dev_call(fm, [&] { fm_locate(fm->f, npat, d_sp, d_ep, d_first, max_occ, d_out_off, d_pos); });
}

int pfp_fm_count(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t *sp, uint64_t *ep, uint64_t *first) {
  if (!fm || (npat && (!pat_off || !sp || !ep))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  PFP_REQUIRE(!first || fm->f.samples, PFP_EINVAL, "the toehold SA[sp] needs the run samples: this index was built without .ssa / .esa");
  if (!npat) return PFP_OK;
  HostPatterns in;
  in.upload(c, pat, pat_off, npat);
  DBuf<uint64_t> d_out(c, 3 * npat);
  fm_count(fm->f, in.pat.p, in.off.p, npat, d_out.p, d_out.p + npat, first ? d_out.p + 2 * npat : nullptr);
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
  require_samples(fm);
  HostPatterns in;
  in.upload(c, pat, pat_off, npat);
  DBuf<uint64_t> d_rng(c, 3 * npat + 1), d_out_off(c, npat + 1);
  fm_count(fm->f, in.pat.p, in.off.p, npat, d_rng.p, d_rng.p + npat, d_rng.p + 2 * npat);
  in.pat.release();
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
  return dev_call(fm, [&] { fm_approx(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, k, d_hit_off, d_sp, d_ep, d_first, d_dist); });
}

int pfp_fm_approx_stats(pfp_fm *fm, uint64_t out[3]) {
  if (!fm || !out) return PFP_EINVAL;
  memcpy(out, fm->f.apx_stats, sizeof fm->f.apx_stats);
  memset(fm->f.apx_stats, 0, sizeof fm->f.apx_stats);
  return PFP_OK;
}

int pfp_fm_approx(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, int k, uint64_t *hit_off, uint64_t **sp,
                  uint64_t **ep, uint64_t **first, uint8_t **dist) {
  if (!fm || !hit_off || !sp || !ep || !dist || (npat && !pat_off)) return PFP_EINVAL;
  *sp = nullptr; *ep = nullptr; *dist = nullptr;
  if (first) *first = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  const uint64_t budget = seq_budget();
  ApxCall s;
  apx_call_begin(fm, pat, pat_off, npat, k, first != nullptr, s);
  HostOut<uint64_t> h_sp, h_ep, h_first;
  HostOut<uint8_t> h_dist;
  std::copy(s.hit_off.begin(), s.hit_off.end(), hit_off);
  for (uint64_t p0 = 0, p1; p0 < npat; p0 = p1) {       // consecutive patterns whose hits stay within the budget (group_end)
    p1 = group_end(hit_off, p0, npat, budget);
    ApxHits h;
    apx_group_hits(fm, s, p0, p1, k, first != nullptr, h);
    sync(c);
    h_sp.take(c, h.sp.p, h.H);
    h_ep.take(c, h.ep.p, h.H);
    h_dist.take(c, h.dist.p, h.H);
    if (first) h_first.take(c, h.first.p, h.H);
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
  require_samples(fm);
  const uint64_t budget = seq_budget();
  ApxCall s;
  apx_call_begin(fm, pat, pat_off, npat, k, true, s);
  HostOut<uint64_t> h_pos;
  HostOut<uint8_t> h_dist;
  std::vector<uint64_t> go;
  out_off[0] = 0;
  for (uint64_t p0 = 0, p1; p0 < npat; p0 = p1) {       // consecutive patterns whose hits stay within the budget
    p1 = group_end(s.hit_off.data(), p0, npat, budget);
    const uint64_t np = p1 - p0;
    ApxHits h;
    apx_group_hits(fm, s, p0, p1, k, true, h);
    DBuf<uint64_t> d_go(c, np + 1), cep;
    fm_approx_clip(fm->f, np, h.hoff.p, h.H, h.sp.p, h.ep.p, h.first.p, max_occ, d_go.p, cep);
    fetch_group_offsets(c, d_go.p, np, go, out_off + p0);
    // inside the group: consecutive patterns whose positions stay within the budget
    for (uint64_t q0 = 0, q1; q0 < np; q0 = q1) {
      q1 = group_end(go.data(), q0, np, budget);
      const uint64_t h0 = s.hit_off[p0 + q0] - s.hit_off[p0], nh = s.hit_off[p0 + q1] - s.hit_off[p0 + q0];
      DBuf<uint64_t> d_pos;
      DBuf<uint8_t> d_pd;
      const uint64_t U = fm_approx_positions(fm->f, nh, h.sp.p + h0, cep.p + h0, h.first.p + h0, h.dist.p + h0, d_pos, d_pd);
      if (U != go[q1] - go[q0]) throw Error(PFP_EHIP, "approximate locate: a group's positions do not add up");
      h_pos.take(c, d_pos.p, U);
      h_dist.take(c, d_pd.p, U);
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
  return build_call(c, out, [&](FmIndex &f) {
    fm_build_ms(c, f, (const uint8_t *)d_bwt, n_plus_1, (const uint8_t *)d_ssa10, ssa_bytes, (const uint8_t *)d_esa10, esa_bytes,
                (const uint8_t *)d_text);
  });
}

int pfp_fm_build_ms_files(pfp_ctx *c, const char *base, const uint8_t *text, int text_fd, uint64_t text_offset, uint64_t n, pfp_fm **out) {
  if (!c || !base || !out) return PFP_EINVAL;
  return build_call(c, out, [&](FmIndex &f) { load_ms_index(c, base, text, text_fd, text_offset, n, f); });
}

int pfp_fm_ms_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint32_t *d_len, uint64_t *d_pos) {
  return ms_dev(fm, d_pat, d_pat_off, npat, d_len, d_pos, false);
}
int pfp_fm_ms_thr_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint32_t *d_len, uint64_t *d_pos) {
  return ms_dev(fm, d_pat, d_pat_off, npat, d_len, d_pos, true);
}

int pfp_fm_mems_dev(pfp_fm *fm, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_len, const uint64_t *d_pos, uint64_t min_len,
                    uint64_t *d_mem_off, uint64_t *d_mem) {
  if (!fm || !d_mem_off || (npat && (!d_pat_off || !d_len))) return PFP_EINVAL;
  return dev_call(fm, [&] { fm_mems(fm->f, d_pat_off, npat, d_len, d_pos, min_len, d_mem_off, d_mem); });
}

int pfp_fm_ms_stats(pfp_fm *fm, uint64_t out[3]) {
  if (!fm || !out) return PFP_EINVAL;
  memcpy(out, fm->f.ms_stats, sizeof fm->f.ms_stats);
  memset(fm->f.ms_stats, 0, sizeof fm->f.ms_stats);
  return PFP_OK;
}

int pfp_fm_ms(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos) {
  return ms_host(fm, pat, pat_off, npat, len, pos, false);
}
int pfp_fm_ms_thr(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint32_t *len, uint64_t *pos) {
  return ms_host(fm, pat, pat_off, npat, len, pos, true);
}

int pfp_fm_mems(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_len, uint64_t *mem_off, uint64_t **mems) {
  return mems_host(fm, pat, pat_off, npat, min_len, mem_off, mems, false);
}
int pfp_fm_mems_thr(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_len, uint64_t *mem_off, uint64_t **mems) {
  return mems_host(fm, pat, pat_off, npat, min_len, mem_off, mems, true);
}

// ---------------------------------------------------------------- the LCP array and thresholds (lcp.hip)
int pfp_fm_thresholds_dev(pfp_fm *fm, const void *d_thr5, uint64_t bytes) {
  if (!fm) return PFP_EINVAL;
  return dev_call(fm, [&] {
    if (d_thr5) {
      fm_load_thresholds(fm->f, (const uint8_t *)d_thr5, bytes);
    } else {
      LcpOut o;
      o.keep = true;
      fm_lcp(fm->f, o);
    }
  }, false);
}

int pfp_fm_thresholds_files(pfp_fm *fm, const char *base) {
  if (!fm || !base) return PFP_EINVAL;
  return dev_call(fm, [&] {
    require_text(fm, "thresholds need");
    DBuf<uint8_t> d_thr;
    const uint64_t bytes = file_to_dev(fm->f.c, std::string(base) + ".thr_pos", d_thr);
    fm_load_thresholds(fm->f, d_thr.p, bytes);
  }, false);
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
  load_ms_index(c, b, text, text_fd, text_offset, n, f);
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
  return dev_call(fm, [&] { fm_extend(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_cand_pat, d_cand_diag, ncand, k, d_dist, d_start, d_end); });
}

int pfp_fm_extend(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat, const int64_t *cand_diag,
                  uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end) {
  if (!fm || (npat && !pat_off) || (ncand && (!cand_pat || !cand_diag || !dist || !start || !end))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_extend_check(fm->f, k);
  HostPatterns in;
  in.upload(c, pat, pat_off, npat);
  DBuf<uint8_t> d_dist(c, ncand);
  DBuf<uint64_t> d_out(c, 2 * ncand);
  DBuf<uint32_t> d_cp(c, ncand);
  DBuf<int64_t> d_cd(c, ncand);
  if (ncand) { h2d(c, d_cp.p, cand_pat, ncand); h2d(c, d_cd.p, cand_diag, ncand); }
  fm_extend(fm->f, in.pat.p, in.off.p, npat, d_cp.p, d_cd.p, ncand, k, d_dist.p, d_out.p, d_out.p + ncand);
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
  return dev_call(fm, [&] {
    fm_align(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, min_seed, k, max_aln, thresholds != 0, d_aln_off, d_start, d_end, d_dist);
  });
}

int pfp_fm_align(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_aln,
                 int thresholds, uint64_t *aln_off, uint64_t **start, uint64_t **end, uint8_t **dist) {
  if (!fm || !aln_off || !start || !end || !dist || (npat && !pat_off)) return PFP_EINVAL;
  *start = nullptr; *end = nullptr; *dist = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_align_check(fm->f, k, min_seed, thresholds != 0);
  SeedCall s;
  seed_call_begin(fm, pat, pat_off, npat, "pattern", false, min_seed, k, thresholds != 0, s);
  HostOut<uint64_t> h_start, h_end;
  HostOut<uint8_t> h_dist;
  std::vector<uint64_t> go;
  aln_off[0] = 0;
  seed_groups(fm, s, 1, max_aln, true, [&](uint64_t p0, uint64_t np, MapCands &cd) {
    fetch_group_offsets(c, cd.aln_off.p, np, go, aln_off + p0);
    h_start.take(c, cd.start.p, cd.A); h_end.take(c, cd.end.p, cd.A); h_dist.take(c, cd.dist.p, cd.A);
  });
  *start = h_start.release(); *end = h_end.release(); *dist = h_dist.release();
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- aligning in a window (fmwindow.hip)
int pfp_fm_window_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_cand_pat, const uint64_t *d_lo,
                      const uint64_t *d_hi, uint64_t ncand, int k, uint8_t *d_dist, uint64_t *d_start, uint64_t *d_end) {
  if (!fm || (npat && !d_pat_off) || (ncand && (!d_cand_pat || !d_lo || !d_hi || !d_dist || !d_start || !d_end))) return PFP_EINVAL;
  return dev_call(fm, [&] { fm_window(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_cand_pat, d_lo, d_hi, ncand, k, d_dist, d_start, d_end); });
}

int pfp_fm_window(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *cand_pat, const uint64_t *lo,
                  const uint64_t *hi, uint64_t ncand, int k, uint8_t *dist, uint64_t *start, uint64_t *end) {
  if (!fm || (npat && !pat_off) || (ncand && (!cand_pat || !lo || !hi || !dist || !start || !end))) return PFP_EINVAL;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_extend_check(fm->f, k);
  HostPatterns in;
  in.upload(c, pat, pat_off, npat);
  DBuf<uint8_t> d_dist(c, ncand);
  DBuf<uint64_t> d_win(c, 2 * ncand), d_out(c, 2 * ncand);
  DBuf<uint32_t> d_cp(c, ncand);
  if (ncand) { h2d(c, d_cp.p, cand_pat, ncand); h2d(c, d_win.p, lo, ncand); h2d(c, d_win.p + ncand, hi, ncand); }
  fm_window(fm->f, in.pat.p, in.off.p, npat, d_cp.p, d_win.p, d_win.p + ncand, ncand, k, d_dist.p, d_out.p, d_out.p + ncand);
  if (ncand) {
    d2h(c, dist, d_dist.p, ncand);
    d2h(c, start, d_out.p, ncand);
    d2h(c, end, d_out.p + ncand, ncand);
  }
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- edit scripts (fmcigar.hip)
int pfp_fm_cigar_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_aln_pat,
                     const uint64_t *d_start, const uint64_t *d_end, uint64_t naln, int k, uint8_t *d_dist, uint64_t *d_cig_off,
                     uint32_t *d_cig) {
  if (!fm || !d_cig_off || (npat && !d_pat_off) || (naln && (!d_aln_pat || !d_start || !d_end || !d_dist))) return PFP_EINVAL;
  return dev_call(fm, [&] {
    fm_cigar(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_aln_pat, d_start, d_end, naln, k, d_dist, d_cig_off, d_cig);
  });
}

int pfp_fm_cigar(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *aln_pat, const uint64_t *start,
                 const uint64_t *end, uint64_t naln, int k, uint8_t *dist, uint64_t *cig_off, uint32_t **cig) {
  if (!fm || !cig_off || !cig || (npat && !pat_off) || (naln && (!aln_pat || !start || !end || !dist))) return PFP_EINVAL;
  *cig = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_extend_check(fm->f, k);
  HostPatterns in;
  in.upload(c, pat, pat_off, npat);
  DBuf<uint32_t> d_ap(c, naln);
  DBuf<uint64_t> d_span(c, 2 * naln), d_off(c, naln + 1);
  DBuf<uint8_t> d_dist(c, naln);
  if (naln) { h2d(c, d_ap.p, aln_pat, naln); h2d(c, d_span.p, start, naln); h2d(c, d_span.p + naln, end, naln); }
  CigRuns runs;                                         // (every script is computed once: the runs wait in their slots for their place)
  fm_cigar_runs(fm->f, in.pat.p, in.off.p, npat, d_ap.p, d_span.p, d_span.p + naln, naln, k, d_dist.p, d_off.p, runs);
  DBuf<uint32_t> d_cig(c, runs.total);
  fm_cigar_write(fm->f, runs, d_off.p, d_cig.p);
  if (naln) d2h(c, dist, d_dist.p, naln);
  d2h(c, cig_off, d_off.p, naln + 1);
  sync(c);
  HostOut<uint32_t> h_cig;
  h_cig.take(c, d_cig.p, runs.total);
  *cig = h_cig.release();
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- mapping reads (fmmap.hip)
int pfp_fm_map_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_sec,
                   int thresholds, uint64_t *d_hit_off, uint8_t *d_mapq, uint64_t *d_nhits, uint8_t *d_strand, uint32_t *d_seq, uint64_t *d_off,
                   uint64_t *d_start, uint8_t *d_dist, uint64_t *d_cig_off, uint32_t **d_cig, uint64_t *d_md_off, uint8_t **d_md) {
  if (!fm || !d_hit_off || (npat && (!d_pat_off || !d_mapq || !d_nhits))) return PFP_EINVAL;
  const bool fill = d_strand || d_seq || d_off || d_start || d_dist || d_cig_off || d_cig || d_md_off || d_md;
  if (fill && !(d_strand && d_seq && d_off && d_start && d_dist && d_cig_off && d_cig && d_md_off && d_md)) return PFP_EINVAL;
  if (fill) { *d_cig = nullptr; *d_md = nullptr; }
  return dev_call(fm, [&] {
    DBuf<uint32_t> cig;
    DBuf<uint8_t> md;
    fm_map(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, min_seed, k, max_sec, thresholds != 0, d_hit_off, d_mapq, d_nhits, d_strand, d_seq, d_off,
           d_start, d_dist, d_cig_off, cig, d_md_off, md);
    if (fill) { *d_cig = hand_out(cig); *d_md = hand_out(md); }
  });
}

int pfp_fm_map(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, uint64_t max_sec, int thresholds,
               uint64_t *hit_off, uint8_t *mapq, uint64_t *nhits, uint8_t **strand, uint32_t **seq, uint64_t **off, uint64_t **start,
               uint8_t **dist, uint64_t **cig_off, uint32_t **cig, uint64_t **md_off, uint8_t **md) {
  if (!fm || !hit_off || !strand || !seq || !off || !start || !dist || !cig_off || !cig || !md_off || !md ||
      (npat && (!pat_off || !mapq || !nhits)))
    return PFP_EINVAL;
  *strand = nullptr; *seq = nullptr; *off = nullptr; *start = nullptr; *dist = nullptr;
  *cig_off = nullptr; *cig = nullptr; *md_off = nullptr; *md = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  FmIndex &f = fm->f;
  fm_map_check(f, k, min_seed, thresholds != 0);
  SeedCall s;
  seed_call_begin(fm, pat, pat_off, npat, "read", true, min_seed, k, thresholds != 0, s);
  HostOut<uint8_t> h_strand, h_dist, h_md;
  HostOut<uint32_t> h_seq, h_cig;
  HostOut<uint64_t> h_off, h_start, h_cig_off, h_md_off;
  std::vector<uint64_t> go;
  hit_off[0] = 0;
  *h_cig_off.grow(1) = 0; h_cig_off.n = 1;
  *h_md_off.grow(1) = 0; h_md_off.n = 1;
  seed_groups(fm, s, 2, 0, false, [&](uint64_t p0, uint64_t np2, MapCands &cd) {
    const uint64_t r0 = p0 / 2, np = np2 / 2;           // the group's reads
    DBuf<uint64_t> d_hoff(c, np + 1), d_nh(c, np);
    DBuf<uint8_t> d_mapq(c, np);
    MapSel sel;
    fm_map_select(f, s.off + p0, np, k, max_sec, cd, d_hoff.p, d_mapq.p, d_nh.p, sel);
    cd.drop_triples();
    fetch_group_offsets(c, d_hoff.p, np, go, hit_off + r0);
    d2h(c, mapq + r0, d_mapq.p, np);
    d2h(c, nhits + r0, d_nh.p, np);
    sync(c);
    const uint64_t H = sel.H;
    DBuf<uint8_t> d_strand(c, H), d_dist(c, H), d_md;
    DBuf<uint32_t> d_seq(c, H), d_cig;
    DBuf<uint64_t> d_off(c, H), d_start(c, H), d_coff(c, H + 1), d_moff(c, H + 1);
    fm_map_fill(f, s.pat, s.off + p0, np, k, cd.aln_off.p, d_hoff.p, sel, d_strand.p, d_seq.p, d_off.p, d_start.p, d_dist.p, d_coff.p, d_cig, d_moff.p,
                d_md);
    h_strand.take(c, d_strand.p, H); h_seq.take(c, d_seq.p, H); h_off.take(c, d_off.p, H);
    h_start.take(c, d_start.p, H); h_dist.take(c, d_dist.p, H);
    const uint64_t runs = h_cig_off.take_offsets(c, d_coff.p + 1, H), md_bytes = h_md_off.take_offsets(c, d_moff.p + 1, H);
    h_cig.take(c, d_cig.p, runs);
    h_md.take(c, d_md.p, md_bytes);
  });
  *strand = h_strand.release(); *seq = h_seq.release(); *off = h_off.release(); *start = h_start.release(); *dist = h_dist.release();
  *cig_off = h_cig_off.release(); *cig = h_cig.release(); *md_off = h_md_off.release(); *md = h_md.release();
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- mapping read pairs (fmpair.hip)
int pfp_fm_map_pairs_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, int k, int thresholds,
                         uint64_t min_ins, uint64_t max_ins, uint64_t anchors, uint8_t *d_proper, uint64_t *d_npairs, uint8_t *d_mapped,
                         uint8_t *d_rescued, uint8_t *d_mapq, uint64_t *d_nhits, uint8_t *d_strand, uint32_t *d_seq, uint64_t *d_off,
                         uint64_t *d_start, uint8_t *d_dist, int64_t *d_tlen, uint64_t *d_cig_off, uint32_t **d_cig, uint64_t *d_md_off,
                         uint8_t **d_md) {
  if (!fm || !d_cig_off || !d_cig || !d_md_off || !d_md ||
      (npat && (!d_pat_off || !d_proper || !d_npairs || !d_mapped || !d_rescued || !d_mapq || !d_nhits || !d_strand || !d_seq || !d_off || !d_start ||
                !d_dist || !d_tlen)))
    return PFP_EINVAL;
  *d_cig = nullptr; *d_md = nullptr;
  return dev_call(fm, [&] {
    DBuf<uint32_t> cig;
    DBuf<uint8_t> md;
    const PairOut out{d_proper, d_npairs, d_mapped, d_rescued, d_mapq, d_strand, d_seq, d_off, d_start, d_dist, d_tlen, d_cig_off, d_md_off};
    fm_map_pairs(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, min_seed, k, thresholds != 0, min_ins, max_ins, anchors, d_nhits, out, cig, md);
    *d_cig = hand_out(cig); *d_md = hand_out(md);
  });
}

int pfp_fm_map_pairs(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, int k, int thresholds,
                     uint64_t min_ins, uint64_t max_ins, uint64_t anchors, uint8_t *proper, uint64_t *npairs, uint8_t *mapped, uint8_t *rescued,
                     uint8_t *mapq, uint64_t *nhits, uint8_t *strand, uint32_t *seq, uint64_t *off, uint64_t *start, uint8_t *dist, int64_t *tlen,
                     uint64_t *cig_off, uint32_t **cig, uint64_t *md_off, uint8_t **md) {
  if (!fm || !cig_off || !cig || !md_off || !md ||
      (npat && (!pat_off || !proper || !npairs || !mapped || !rescued || !mapq || !nhits || !strand || !seq || !off || !start || !dist || !tlen)))
    return PFP_EINVAL;
  *cig = nullptr; *md = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  FmIndex &f = fm->f;
  fm_pair_check(f, npat, k, min_seed, thresholds != 0, min_ins, max_ins, anchors);
  SeedCall s;
  seed_call_begin(fm, pat, pat_off, npat, "read", true, min_seed, k, thresholds != 0, s);
  HostOut<uint32_t> h_cig;
  HostOut<uint8_t> h_md;
  cig_off[0] = 0; md_off[0] = 0;
  seed_groups(fm, s, 4, 0, false, [&](uint64_t pat0, uint64_t np2, MapCands &cd) {      // groups of WHOLE pairs
    const uint64_t p0 = pat0 / 2, np = np2 / 2, q0 = p0 / 2;                            // the group's reads, its first pair
    // the group's results: nhits, off, start, tlen (np each) and npairs (np / 2); the single-end MAPQ, mapped, rescued, mapq,
    // strand, dist (np each) and proper (np / 2)
    DBuf<uint64_t> d_hoff(c, np + 1), d_u64(c, 4 * np + np / 2), d_coff(c, np + 1), d_mdoff(c, np + 1);
    DBuf<uint8_t> d_u8(c, 6 * np + np / 2), d_md;
    DBuf<uint32_t> d_seq(c, np), d_cig;
    uint64_t *d_nh = d_u64.p, *d_off = d_nh + np, *d_start = d_off + np, *d_tlen = d_start + np, *d_npairs = d_tlen + np;
    uint8_t *d_smapq = d_u8.p, *d_mapped = d_smapq + np, *d_resc = d_mapped + np, *d_mapq = d_resc + np, *d_strand = d_mapq + np,
            *d_dist = d_strand + np, *d_proper = d_dist + np;
    MapSel sel;
    fm_map_select(f, s.off + pat0, np, k, anchors - 1, cd, d_hoff.p, d_smapq, d_nh, sel);
    cd.drop_triples();
    const PairOut out{d_proper, d_npairs, d_mapped, d_resc, d_mapq, d_strand, d_seq.p, d_off, d_start, d_dist, (int64_t *)d_tlen, d_coff.p, d_mdoff.p};
    fm_pair(f, s.pat, s.off + pat0, np, k, min_ins, max_ins, anchors, cd.aln_off.p, d_hoff.p, d_smapq, sel, out, d_cig, d_md);
    d2h(c, proper + q0, d_proper, np / 2); d2h(c, npairs + q0, d_npairs, np / 2);
    d2h(c, mapped + p0, d_mapped, np); d2h(c, rescued + p0, d_resc, np); d2h(c, mapq + p0, d_mapq, np); d2h(c, nhits + p0, d_nh, np);
    d2h(c, strand + p0, d_strand, np); d2h(c, seq + p0, d_seq.p, np); d2h(c, off + p0, d_off, np); d2h(c, start + p0, d_start, np);
    d2h(c, dist + p0, d_dist, np); d2h(c, (uint64_t *)tlen + p0, d_tlen, np);
    // (one wait for all of the group's arrays, the two offset arrays among them, so not fetch_group_offsets, which waits per array)
    d2h(c, cig_off + p0 + 1, d_coff.p + 1, np); d2h(c, md_off + p0 + 1, d_mdoff.p + 1, np);
    sync(c);
    rebase_offsets(cig_off + p0 + 1, np, cig_off[p0]);
    rebase_offsets(md_off + p0 + 1, np, md_off[p0]);
    h_cig.take(c, d_cig.p, cig_off[p0 + np] - cig_off[p0]);
    h_md.take(c, d_md.p, md_off[p0 + np] - md_off[p0]);
  });
  *cig = h_cig.release(); *md = h_md.release();
  return PFP_OK;
  PFP_CATCH(c)
}

// ---------------------------------------------------------------- chaining anchors (fmchain.hip)
int pfp_fm_anchors_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                       int thresholds, uint64_t *d_anc_off, uint64_t *d_anc, uint32_t *d_skipped) {
  if (!fm || !d_anc_off || (npat && !d_pat_off)) return PFP_EINVAL;
  return dev_call(fm, [&] {
    pfp_ctx *c = fm->f.c;
    DBuf<uint64_t> anc;
    const uint64_t total = fm_anchors(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, min_seed, max_occ, thresholds != 0, d_anc_off, anc, d_skipped);
    if (d_anc && total) PFP_HIP(hipMemcpyAsync(d_anc, anc.p, 24 * total, hipMemcpyDeviceToDevice, c->stream));
    sync(c);                                            // (the triples go back when this returns)
  });
}

int pfp_fm_anchors(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ, int thresholds,
                   uint64_t *anc_off, uint64_t **anc, uint32_t *skipped) {
  if (!fm || !anc_off || !anc || (npat && !pat_off)) return PFP_EINVAL;
  *anc = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_anchors_check(fm->f, min_seed, max_occ, thresholds != 0);
  SeedCall s;
  seed_call_begin(fm, pat, pat_off, npat, "pattern", false, min_seed, 0, thresholds != 0, s, false);
  HostOut<uint64_t> h_anc;
  std::vector<uint64_t> go;
  anc_off[0] = 0;
  anchor_groups(fm, s, 1, max_occ, [&](uint64_t p0, uint64_t np, DBuf<uint64_t> &d_aoff, DBuf<uint64_t> &d_anc, uint64_t total, DBuf<uint32_t> &d_skip) {
    fetch_group_offsets(c, d_aoff.p, np, go, anc_off + p0);
    if (skipped) { d2h(c, skipped + p0, d_skip.p, np); sync(c); }
    h_anc.take(c, d_anc.p, 3 * total);
  });
  *anc = h_anc.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_chain_dev(pfp_fm *fm, const uint64_t *d_anc_off, const uint64_t *d_anc, uint64_t npat, uint64_t max_gap, uint64_t band,
                     uint64_t min_score, uint64_t max_chains, uint64_t *d_chain_off, uint32_t *d_score, uint32_t *d_n, uint32_t *d_qs,
                     uint32_t *d_qe, uint64_t *d_ts, uint64_t *d_te, uint32_t *d_match) {
  if (!fm || !d_chain_off || (npat && !d_anc_off)) return PFP_EINVAL;
  const bool fill = d_score || d_n || d_qs || d_qe || d_ts || d_te || d_match;
  if (fill && !(d_score && d_n && d_qs && d_qe && d_ts && d_te && d_match)) return PFP_EINVAL;
  return dev_call(fm, [&] {
    ChainSel sel;
    fm_chains_run(fm->f, d_anc_off, d_anc, npat, max_gap, band, min_score, max_chains, d_chain_off, sel);
    if (fill) fm_chains_write(fm->f, d_anc, npat, d_chain_off, sel, ChainOut{d_score, d_n, d_qs, d_qe, d_ts, d_te, d_match});
    sync(fm->f.c);                                      // (what the write reads goes back when this returns)
  });
}

int pfp_fm_chain(pfp_fm *fm, const uint64_t *anc_off, const uint64_t *anc, uint64_t npat, uint64_t max_gap, uint64_t band, uint64_t min_score,
                 uint64_t max_chains, uint64_t *chain_off, uint32_t **score, uint32_t **n, uint32_t **qs, uint32_t **qe, uint64_t **ts,
                 uint64_t **te, uint32_t **match) {
  if (!fm || !chain_off || !score || !n || !qs || !qe || !ts || !te || !match || (npat && !anc_off)) return PFP_EINVAL;
  *score = nullptr; *n = nullptr; *qs = nullptr; *qe = nullptr; *ts = nullptr; *te = nullptr; *match = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_chain_check(fm->f, max_gap, band, min_score);
  chain_off[0] = 0;
  if (!npat) return PFP_OK;
  for (uint64_t p = 0; p < npat; p++)
    PFP_REQUIRE(anc_off[p] <= anc_off[p + 1], PFP_EINVAL, "anchor offsets decrease at pattern " + std::to_string(p));
  const uint64_t A = anc_off[npat];
  PFP_REQUIRE(anc || !A, PFP_EINVAL, "no anchors");
  DBuf<uint64_t> d_aoff(c, npat + 1), d_anc(c, 3 * A), d_coff(c, npat + 1);
  h2d(c, d_aoff.p, anc_off, npat + 1);
  if (A) h2d(c, d_anc.p, anc, 3 * A);
  ChainSel sel;
  fm_chains_run(fm->f, d_aoff.p, d_anc.p, npat, max_gap, band, min_score, max_chains, d_coff.p, sel);
  const uint64_t C = sel.total;
  DBuf<uint32_t> d32(c, 5 * C);
  DBuf<uint64_t> d64(c, 2 * C);
  fm_chains_write(fm->f, d_anc.p, npat, d_coff.p, sel, ChainOut{d32.p, d32.p + C, d32.p + 2 * C, d32.p + 3 * C, d64.p, d64.p + C, d32.p + 4 * C});
  d2h(c, chain_off, d_coff.p, npat + 1);
  sync(c);
  HostOut<uint32_t> h_score, h_n, h_qs, h_qe, h_match;
  HostOut<uint64_t> h_ts, h_te;
  h_score.take(c, d32.p, C); h_n.take(c, d32.p + C, C); h_qs.take(c, d32.p + 2 * C, C); h_qe.take(c, d32.p + 3 * C, C);
  h_match.take(c, d32.p + 4 * C, C); h_ts.take(c, d64.p, C); h_te.take(c, d64.p + C, C);
  *score = h_score.release(); *n = h_n.release(); *qs = h_qs.release(); *qe = h_qe.release(); *ts = h_ts.release(); *te = h_te.release();
  *match = h_match.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_map_long_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                        uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_sec, int thresholds, uint64_t *d_hit_off,
                        uint8_t *d_mapq, uint64_t *d_nchains, uint8_t *d_strand, uint32_t *d_seq, uint64_t *d_off, uint64_t *d_ts,
                        uint64_t *d_te, uint32_t *d_qs, uint32_t *d_qe, uint32_t *d_score, uint32_t *d_n, uint32_t *d_match) {
  if (!fm || !d_hit_off || (npat && (!d_pat_off || !d_mapq || !d_nchains))) return PFP_EINVAL;
  const bool fill = d_strand || d_seq || d_off || d_ts || d_te || d_qs || d_qe || d_score || d_n || d_match;
  if (fill && !(d_strand && d_seq && d_off && d_ts && d_te && d_qs && d_qe && d_score && d_n && d_match)) return PFP_EINVAL;
  return dev_call(fm, [&] {
    const LongOut out{d_strand, d_seq, d_off, d_ts, d_te, d_qs, d_qe, d_score, d_n, d_match};
    fm_map_long(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, min_seed, max_occ, max_gap, band, min_score, max_sec, thresholds != 0, d_hit_off,
                d_mapq, d_nchains, fill ? &out : nullptr);
  });
}

// what pfp_fm_map_long_aln returns on top of pfp_fm_map_long
struct LongAlnHost {
  uint64_t max_fill;
  uint32_t **aqs;
  uint64_t **ats;
  uint32_t **nm, **unfilled;
  uint64_t **cig_off;
  uint32_t **cig;
};
// pfp_fm_map_long, and with aln pfp_fm_map_long_aln: one beginning, one grouping, the scripts of a group's returned chains behind its fields
static int map_long_host(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                         uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_sec, int thresholds, uint64_t *hit_off, uint8_t *mapq,
                         uint64_t *nchains, uint8_t **strand, uint32_t **seq, uint64_t **off, uint64_t **ts, uint64_t **te, uint32_t **qs,
                         uint32_t **qe, uint32_t **score, uint32_t **n, uint32_t **match, const LongAlnHost *aln) {
  if (!fm || !hit_off || !strand || !seq || !off || !ts || !te || !qs || !qe || !score || !n || !match ||
      (npat && (!pat_off || !mapq || !nchains)))
    return PFP_EINVAL;
  *strand = nullptr; *seq = nullptr; *off = nullptr; *ts = nullptr; *te = nullptr; *qs = nullptr; *qe = nullptr; *score = nullptr; *n = nullptr;
  *match = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  FmIndex &f = fm->f;
  fm_anchors_check(f, min_seed, max_occ, thresholds != 0);
  fm_chain_check(f, max_gap, band, min_score);
  if (aln) fm_fill_check(f, aln->max_fill);
  SeedCall s;
  seed_call_begin(fm, pat, pat_off, npat, "read", true, min_seed, 0, thresholds != 0, s, false);
  HostOut<uint8_t> h_strand;
  HostOut<uint32_t> h_seq, h_qs, h_qe, h_score, h_n, h_match, h_aqs, h_nm, h_unf, h_cig;
  HostOut<uint64_t> h_off, h_ts, h_te, h_ats, h_coff;
  if (aln) { *h_coff.grow(1) = 0; h_coff.n = 1; }
  std::vector<uint64_t> go;
  hit_off[0] = 0;
  anchor_groups(fm, s, 2, max_occ, [&](uint64_t p0, uint64_t np2, DBuf<uint64_t> &d_aoff, DBuf<uint64_t> &d_anc, uint64_t, DBuf<uint32_t> &) {
    const uint64_t r0 = p0 / 2, np = np2 / 2;           // the group's reads
    DBuf<uint64_t> d_hoff(c, np + 1), d_nc(c, np);
    DBuf<uint8_t> d_mapq(c, np);
    LongSel sel;
    sel.keep = aln != nullptr;
    fm_map_long_select(f, d_aoff.p, d_anc.p, np, max_gap, band, min_score, max_sec, d_hoff.p, d_mapq.p, d_nc.p, sel);
    fetch_group_offsets(c, d_hoff.p, np, go, hit_off + r0);
    d2h(c, mapq + r0, d_mapq.p, np);
    d2h(c, nchains + r0, d_nc.p, np);
    sync(c);
    const uint64_t H = sel.H;
    DBuf<uint8_t> d_strand(c, H);
    DBuf<uint32_t> d32(c, 6 * H);
    DBuf<uint64_t> d64(c, 3 * H);
    fm_map_long_fill(f, s.off + p0, np, d_hoff.p, sel,
                     LongOut{d_strand.p, d32.p, d64.p, d64.p + H, d64.p + 2 * H, d32.p + H, d32.p + 2 * H, d32.p + 3 * H, d32.p + 4 * H, d32.p + 5 * H});
    sync(c);
    h_strand.take(c, d_strand.p, H); h_seq.take(c, d32.p, H); h_off.take(c, d64.p, H); h_ts.take(c, d64.p + H, H); h_te.take(c, d64.p + 2 * H, H);
    h_qs.take(c, d32.p + H, H); h_qe.take(c, d32.p + 2 * H, H); h_score.take(c, d32.p + 3 * H, H); h_n.take(c, d32.p + 4 * H, H);
    h_match.take(c, d32.p + 5 * H, H);
    if (!aln) return;
    DBuf<uint32_t> a32(c, 3 * H), d_cig;
    DBuf<uint64_t> a64(c, H), d_coff(c, H + 1);
    ChainAln st;
    fm_map_long_align(f, s.pat, s.off + p0, np, d_aoff.p, d_anc.p, d_hoff.p, sel, aln->max_fill, AlnOut{a32.p, a64.p, a32.p + H, a32.p + 2 * H},
                      d_coff.p, st);
    d_cig.alloc(c, st.total);
    fm_chain_align_write(f, st, d_coff.p, d_cig.p);
    sync(c);
    h_aqs.take(c, a32.p, H); h_nm.take(c, a32.p + H, H); h_unf.take(c, a32.p + 2 * H, H); h_ats.take(c, a64.p, H);
    h_coff.take_offsets(c, d_coff.p + 1, H);
    h_cig.take(c, d_cig.p, st.total);
  });
  if (aln) {
    *aln->aqs = h_aqs.release(); *aln->ats = h_ats.release(); *aln->nm = h_nm.release(); *aln->unfilled = h_unf.release();
    *aln->cig_off = h_coff.release(); *aln->cig = h_cig.release();
  }
  *strand = h_strand.release(); *seq = h_seq.release(); *off = h_off.release(); *ts = h_ts.release(); *te = h_te.release();
  *qs = h_qs.release(); *qe = h_qe.release(); *score = h_score.release(); *n = h_n.release(); *match = h_match.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_map_long(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                    uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_sec, int thresholds, uint64_t *hit_off, uint8_t *mapq,
                    uint64_t *nchains, uint8_t **strand, uint32_t **seq, uint64_t **off, uint64_t **ts, uint64_t **te, uint32_t **qs,
                    uint32_t **qe, uint32_t **score, uint32_t **n, uint32_t **match) {
  return map_long_host(fm, pat, pat_off, npat, min_seed, max_occ, max_gap, band, min_score, max_sec, thresholds, hit_off, mapq, nchains, strand, seq,
                       off, ts, te, qs, qe, score, n, match, nullptr);
}

// ---------------------------------------------------------------- aligning chains (fmfill.hip)
int pfp_fm_fill_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint32_t *d_seg_pat, const uint64_t *d_q0,
                    const uint64_t *d_q1, const uint64_t *d_t0, const uint64_t *d_t1, uint64_t nseg, uint64_t max_fill, uint32_t *d_dist,
                    uint64_t *d_cig_off, uint32_t *d_cig) {
  if (!fm || !d_cig_off || (npat && !d_pat_off) || (nseg && (!d_seg_pat || !d_q0 || !d_q1 || !d_t0 || !d_t1 || !d_dist))) return PFP_EINVAL;
  return dev_call(fm, [&] {
    fm_fill(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, FillSegs{d_seg_pat, d_q0, d_q1, d_t0, d_t1}, nseg, max_fill, d_dist, d_cig_off, d_cig);
  });
}

int pfp_fm_fill(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint32_t *seg_pat, const uint64_t *q0,
                const uint64_t *q1, const uint64_t *t0, const uint64_t *t1, uint64_t nseg, uint64_t max_fill, uint32_t *dist, uint64_t *cig_off,
                uint32_t **cig) {
  if (!fm || !cig_off || !cig || (npat && !pat_off) || (nseg && (!seg_pat || !q0 || !q1 || !t0 || !t1 || !dist))) return PFP_EINVAL;
  *cig = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_fill_check(fm->f, max_fill);
  HostPatterns in;
  in.upload(c, pat, pat_off, npat);
  DBuf<uint32_t> d_sp(c, nseg), d_dist(c, nseg);
  DBuf<uint64_t> d_seg(c, 4 * nseg), d_off(c, nseg + 1);
  if (nseg) {
    h2d(c, d_sp.p, seg_pat, nseg);
    h2d(c, d_seg.p, q0, nseg); h2d(c, d_seg.p + nseg, q1, nseg); h2d(c, d_seg.p + 2 * nseg, t0, nseg); h2d(c, d_seg.p + 3 * nseg, t1, nseg);
  }
  const FillSegs sg{d_sp.p, d_seg.p, d_seg.p + nseg, d_seg.p + 2 * nseg, d_seg.p + 3 * nseg};
  FillRuns runs;                                        // (every script is computed once: the runs wait in their slots for their place)
  fm_fill_runs(fm->f, in.pat.p, in.off.p, npat, sg, nseg, max_fill, d_dist.p, d_off.p, runs);
  DBuf<uint32_t> d_cig(c, runs.total);
  fm_fill_write(fm->f, sg, nseg, d_dist.p, runs, d_off.p, d_cig.p);
  if (nseg) d2h(c, dist, d_dist.p, nseg);
  d2h(c, cig_off, d_off.p, nseg + 1);
  sync(c);
  HostOut<uint32_t> h_cig;
  h_cig.take(c, d_cig.p, runs.total);
  *cig = h_cig.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_fill_stats(pfp_fm *fm, uint64_t out[14]) {
  if (!fm || !out) return PFP_EINVAL;
  memcpy(out, fm->f.fill_stats, sizeof fm->f.fill_stats);
  memset(fm->f.fill_stats, 0, sizeof fm->f.fill_stats);
  return PFP_OK;
}

// the chains of device anchors and their scripts; what is the caller's: chain_off, out, al, cig_off; cig, mem_off and mem may be NULL
static void chain_align_on_device(FmIndex &f, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint64_t *anc_off, const uint64_t *anc,
                                  uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_chains, uint64_t max_fill, uint64_t *chain_off,
                                  const ChainOut &out, const AlnOut &al, uint64_t *cig_off, uint32_t *cig, uint64_t *mem_off, uint32_t *mem) {
  pfp_ctx *c = f.c;
  ChainSel sel;
  fm_chains_run(f, anc_off, anc, npat, max_gap, band, min_score, max_chains, chain_off, sel);
  fm_chains_write(f, anc, npat, chain_off, sel, out);
  ChainAln st;
  fm_chain_align_runs(f, pat, pat_off, npat, anc_off, anc, chain_off, sel, nullptr, sel.total, max_fill, false, al, cig_off, st);
  if (cig) fm_chain_align_write(f, st, cig_off, cig);
  if (mem_off) PFP_HIP(hipMemcpyAsync(mem_off, st.mem_off.p, (st.nal + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
  if (mem && st.M) PFP_HIP(hipMemcpyAsync(mem, st.mem.p, st.M * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  sync(c);                                              // (the members, the gaps and their runs go back when this returns)
}

int pfp_fm_chain_align_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, const uint64_t *d_anc_off,
                           const uint64_t *d_anc, uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_chains, uint64_t max_fill,
                           uint64_t *d_chain_off, uint32_t *d_score, uint32_t *d_n, uint32_t *d_qs, uint32_t *d_qe, uint64_t *d_ts, uint64_t *d_te,
                           uint32_t *d_match, uint32_t *d_aqs, uint64_t *d_ats, uint32_t *d_nm, uint32_t *d_unfilled, uint64_t *d_cig_off,
                           uint32_t *d_cig, uint64_t *d_mem_off, uint32_t *d_mem) {
  if (!fm || !d_chain_off || (npat && (!d_anc_off || !d_pat_off))) return PFP_EINVAL;
  const bool fill = d_score || d_n || d_qs || d_qe || d_ts || d_te || d_match || d_aqs || d_ats || d_nm || d_unfilled || d_cig_off || d_cig ||
                    d_mem_off || d_mem;
  if (fill && !(d_score && d_n && d_qs && d_qe && d_ts && d_te && d_match && d_aqs && d_ats && d_nm && d_unfilled && d_cig_off)) return PFP_EINVAL;
  return dev_call(fm, [&] {
    fm_fill_check(fm->f, max_fill);
    fm_fill_check_patterns(fm->f, d_pat_off, npat);
    if (!fill) {
      ChainSel sel;
      fm_chains_run(fm->f, d_anc_off, d_anc, npat, max_gap, band, min_score, max_chains, d_chain_off, sel);
      return;
    }
    chain_align_on_device(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, d_anc_off, d_anc, max_gap, band, min_score, max_chains, max_fill, d_chain_off,
                          ChainOut{d_score, d_n, d_qs, d_qe, d_ts, d_te, d_match}, AlnOut{d_aqs, d_ats, d_nm, d_unfilled}, d_cig_off, d_cig, d_mem_off,
                          d_mem);
  });
}

int pfp_fm_chain_align(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, const uint64_t *anc_off, const uint64_t *anc,
                       uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_chains, uint64_t max_fill, uint64_t *chain_off,
                       uint32_t **score, uint32_t **n, uint32_t **qs, uint32_t **qe, uint64_t **ts, uint64_t **te, uint32_t **match,
                       uint32_t **aqs, uint64_t **ats, uint32_t **nm, uint32_t **unfilled, uint64_t **cig_off, uint32_t **cig,
                       uint64_t **mem_off, uint32_t **mem) {
  if (!fm || !chain_off || !score || !n || !qs || !qe || !ts || !te || !match || !aqs || !ats || !nm || !unfilled || !cig_off || !cig ||
      (npat && (!anc_off || !pat_off)))
    return PFP_EINVAL;
  *score = nullptr; *n = nullptr; *qs = nullptr; *qe = nullptr; *ts = nullptr; *te = nullptr; *match = nullptr;
  *aqs = nullptr; *ats = nullptr; *nm = nullptr; *unfilled = nullptr; *cig_off = nullptr; *cig = nullptr;
  if (mem_off) *mem_off = nullptr;
  if (mem) *mem = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  fm_chain_check(fm->f, max_gap, band, min_score);
  fm_fill_check(fm->f, max_fill);
  chain_off[0] = 0;
  HostPatterns in;
  in.upload(c, pat, pat_off, npat);
  for (uint64_t p = 0; p < npat; p++)
    PFP_REQUIRE(anc_off[p] <= anc_off[p + 1], PFP_EINVAL, "anchor offsets decrease at pattern " + std::to_string(p));
  const uint64_t A = npat ? anc_off[npat] : 0;
  PFP_REQUIRE(anc || !A, PFP_EINVAL, "no anchors");
  DBuf<uint64_t> d_aoff(c, npat + 1), d_anc(c, 3 * A), d_coff(c, npat + 1);
  if (npat) h2d(c, d_aoff.p, anc_off, npat + 1);
  if (A) h2d(c, d_anc.p, anc, 3 * A);
  ChainSel sel;
  fm_chains_run(fm->f, d_aoff.p, d_anc.p, npat, max_gap, band, min_score, max_chains, d_coff.p, sel);
  const uint64_t C = sel.total;
  DBuf<uint32_t> d32(c, 8 * C), d_cig;
  DBuf<uint64_t> d64(c, 3 * C), d_goff(c, C + 1);
  fm_chains_write(fm->f, d_anc.p, npat, d_coff.p, sel, ChainOut{d32.p, d32.p + C, d32.p + 2 * C, d32.p + 3 * C, d64.p, d64.p + C, d32.p + 4 * C});
  ChainAln st;
  fm_chain_align_runs(fm->f, in.pat.p, in.off.p, npat, d_aoff.p, d_anc.p, d_coff.p, sel, nullptr, C, max_fill, false,
                      AlnOut{d32.p + 5 * C, d64.p + 2 * C, d32.p + 6 * C, d32.p + 7 * C}, d_goff.p, st);
  d_cig.alloc(c, st.total);
  fm_chain_align_write(fm->f, st, d_goff.p, d_cig.p);
  d2h(c, chain_off, d_coff.p, npat + 1);
  sync(c);
  HostOut<uint32_t> h_score, h_n, h_qs, h_qe, h_match, h_aqs, h_nm, h_unf, h_cig, h_mem;
  HostOut<uint64_t> h_ts, h_te, h_ats, h_goff, h_moff;
  h_score.take(c, d32.p, C); h_n.take(c, d32.p + C, C); h_qs.take(c, d32.p + 2 * C, C); h_qe.take(c, d32.p + 3 * C, C);
  h_match.take(c, d32.p + 4 * C, C); h_ts.take(c, d64.p, C); h_te.take(c, d64.p + C, C);
  h_aqs.take(c, d32.p + 5 * C, C); h_nm.take(c, d32.p + 6 * C, C); h_unf.take(c, d32.p + 7 * C, C); h_ats.take(c, d64.p + 2 * C, C);
  h_goff.take(c, d_goff.p, C + 1); h_cig.take(c, d_cig.p, st.total);
  if (mem_off) h_moff.take(c, st.mem_off.p, C + 1);
  if (mem) h_mem.take(c, st.mem.p, st.M);
  *score = h_score.release(); *n = h_n.release(); *qs = h_qs.release(); *qe = h_qe.release(); *ts = h_ts.release(); *te = h_te.release();
  *match = h_match.release(); *aqs = h_aqs.release(); *ats = h_ats.release(); *nm = h_nm.release(); *unfilled = h_unf.release();
  *cig_off = h_goff.release(); *cig = h_cig.release();
  if (mem_off) *mem_off = h_moff.release();
  if (mem) *mem = h_mem.release();
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_fm_map_long_aln_dev(pfp_fm *fm, const void *d_pat, const uint64_t *d_pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                            uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_sec, int thresholds, uint64_t max_fill,
                            uint64_t *d_hit_off, uint8_t *d_mapq, uint64_t *d_nchains, uint8_t *d_strand, uint32_t *d_seq, uint64_t *d_off,
                            uint64_t *d_ts, uint64_t *d_te, uint32_t *d_qs, uint32_t *d_qe, uint32_t *d_score, uint32_t *d_n, uint32_t *d_match,
                            uint32_t *d_aqs, uint64_t *d_ats, uint32_t *d_nm, uint32_t *d_unfilled, uint64_t *d_cig_off, uint32_t *d_cig) {
  if (!fm || !d_hit_off || (npat && (!d_pat_off || !d_mapq || !d_nchains))) return PFP_EINVAL;
  const bool fill = d_strand || d_seq || d_off || d_ts || d_te || d_qs || d_qe || d_score || d_n || d_match || d_aqs || d_ats || d_nm ||
                    d_unfilled || d_cig_off || d_cig;
  if (fill && !(d_strand && d_seq && d_off && d_ts && d_te && d_qs && d_qe && d_score && d_n && d_match && d_aqs && d_ats && d_nm && d_unfilled &&
                d_cig_off))
    return PFP_EINVAL;
  return dev_call(fm, [&] {
    fm_fill_check(fm->f, max_fill);
    const LongOut out{d_strand, d_seq, d_off, d_ts, d_te, d_qs, d_qe, d_score, d_n, d_match};
    const LongAln aln{max_fill, AlnOut{d_aqs, d_ats, d_nm, d_unfilled}, d_cig_off, d_cig};
    fm_map_long(fm->f, (const uint8_t *)d_pat, d_pat_off, npat, min_seed, max_occ, max_gap, band, min_score, max_sec, thresholds != 0, d_hit_off,
                d_mapq, d_nchains, fill ? &out : nullptr, fill ? &aln : nullptr);
  });
}

int pfp_fm_map_long_aln(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t min_seed, uint64_t max_occ,
                        uint64_t max_gap, uint64_t band, uint64_t min_score, uint64_t max_sec, int thresholds, uint64_t max_fill,
                        uint64_t *hit_off, uint8_t *mapq, uint64_t *nchains, uint8_t **strand, uint32_t **seq, uint64_t **off, uint64_t **ts,
                        uint64_t **te, uint32_t **qs, uint32_t **qe, uint32_t **score, uint32_t **n, uint32_t **match, uint32_t **aqs,
                        uint64_t **ats, uint32_t **nm, uint32_t **unfilled, uint64_t **cig_off, uint32_t **cig) {
  if (!aqs || !ats || !nm || !unfilled || !cig_off || !cig) return PFP_EINVAL;
  *aqs = nullptr; *ats = nullptr; *nm = nullptr; *unfilled = nullptr; *cig_off = nullptr; *cig = nullptr;
  const LongAlnHost aln{max_fill, aqs, ats, nm, unfilled, cig_off, cig};
  return map_long_host(fm, pat, pat_off, npat, min_seed, max_occ, max_gap, band, min_score, max_sec, thresholds, hit_off, mapq, nchains, strand, seq,
                       off, ts, te, qs, qe, score, n, match, &aln);
}

// ---------------------------------------------------------------- sequences of a collection (seqmap.hip)
int pfp_fm_set_seqs(pfp_fm *fm, const uint64_t *starts, uint64_t nseq) {
  if (!fm) return PFP_EINVAL;
  return dev_call(fm, [&] { fm_set_seqs(fm->f, starts, nseq); }, false);
}

int pfp_fm_seqmap_dev(pfp_fm *fm, const uint64_t *d_pos, uint64_t count, uint32_t *d_seq, uint64_t *d_off) {
  if (!fm || (count && !d_pos)) return PFP_EINVAL;
  return dev_call(fm, [&] { fm_seqmap(fm->f, d_pos, count, d_seq, d_off); });
}

int pfp_fm_locate_seqs_dev(pfp_fm *fm, const uint64_t *d_pat_off, uint64_t npat, const uint64_t *d_sp, const uint64_t *d_ep,
                           const uint64_t *d_first, uint64_t max_occ, uint64_t *d_out_off, uint32_t *d_seq, uint64_t *d_off) {
  if (!fm || !d_out_off || (npat && (!d_pat_off || !d_sp || !d_ep))) return PFP_EINVAL;
  return dev_call(fm, [&] { fm_locate_seqs(fm->f, d_pat_off, npat, d_sp, d_ep, d_first, max_occ, d_out_off, d_seq, d_off); });
}

int pfp_fm_doclist_dev(pfp_fm *fm, const uint64_t *d_pat_off, uint64_t npat, const uint64_t *d_sp, const uint64_t *d_ep,
                       const uint64_t *d_first, uint64_t *d_doc_off, uint32_t *d_doc, uint64_t *d_cnt) {
  if (!fm || !d_doc_off || (npat && (!d_pat_off || !d_sp || !d_ep))) return PFP_EINVAL;
  return dev_call(fm, [&] {
    DocOut o;
    o.doc = d_doc; o.cnt = d_cnt;
    fm_doclist(fm->f, d_pat_off, npat, d_sp, d_ep, d_first, d_doc_off, o);
  });
}

int pfp_fm_locate_seqs(pfp_fm *fm, const uint8_t *pat, const uint64_t *pat_off, uint64_t npat, uint64_t max_occ, uint64_t *sp,
                       uint64_t *ep, uint64_t *out_off, uint32_t **seq, uint64_t **off) {
  if (!fm || !out_off || !seq || !off || (npat && !pat_off)) return PFP_EINVAL;
  *seq = nullptr; *off = nullptr;
  pfp_ctx *c = fm->f.c;
  PFP_TRY_DEV(c)
  const uint64_t budget = seq_budget();
  SeqCall s;
  seq_call_begin(fm, pat, pat_off, npat, max_occ, sp, ep, s);
  HostOut<uint32_t> h_seq;
  HostOut<uint64_t> h_off;
  std::vector<uint64_t> go;
  out_off[0] = 0;
  for (uint64_t p0 = 0, p1; p0 < npat; p0 = p1) {       // consecutive patterns with at most `budget` positions to look at
    p1 = group_end(s.uoff.data(), p0, npat, budget);
    const uint64_t k = p1 - p0, U = s.uoff[p1] - s.uoff[p0];
    DBuf<uint64_t> d_go(c, k + 1), d_o(c, U);
    DBuf<uint32_t> d_s(c, U);
    fm_locate_seqs(fm->f, s.in.off.p + p0, k, s.range(p0, 0), s.range(p0, 1), s.range(p0, 2), max_occ, d_go.p, d_s.p, d_o.p);
    fetch_group_offsets(c, d_go.p, k, go, out_off + p0);
    h_seq.take(c, d_s.p, go[k]);
    h_off.take(c, d_o.p, go[k]);
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
  const uint64_t budget = seq_budget();
  SeqCall s;
  seq_call_begin(fm, pat, pat_off, npat, 0, nullptr, nullptr, s);
  HostOut<uint32_t> h_doc;
  HostOut<uint64_t> h_cnt;
  std::vector<uint64_t> go;
  doc_off[0] = 0;
  for (uint64_t p0 = 0, p1; p0 < npat; p0 = p1) {
    p1 = group_end(s.uoff.data(), p0, npat, budget);
    const uint64_t k = p1 - p0;
    DBuf<uint64_t> d_go(c, k + 1), d_c;
    DBuf<uint32_t> d_d;
    DocOut o;
    o.own_doc = &d_d; o.own_cnt = &d_c;      // (sized inside, once the group's total is known: nothing is listed twice)
    fm_doclist(fm->f, s.in.off.p + p0, k, s.range(p0, 0), s.range(p0, 1), s.range(p0, 2), d_go.p, o);
    fetch_group_offsets(c, d_go.p, k, go, doc_off + p0);
    h_doc.take(c, d_d.p, go[k]);
    h_cnt.take(c, d_c.p, go[k]);
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
