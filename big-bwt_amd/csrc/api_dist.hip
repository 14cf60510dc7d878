// api_dist.hip -- the multi-GPU chain, one rank's share: every pfp_dist_* call, the state a rank keeps between them, their kernels.
//
// the text is sharded over the ranks, phrases are independent units.  Every rank
//   1. pfp_dist_local_parse : scans (halo + its shard), owns the phrases that END inside the shard,
//                             deduplicates them locally                       [n/R bytes of work]
//   -- allgather of the local dictionaries (RCCL, done by the caller) --
//   2. pfp_dist_global      : deduplicates the union into the global dictionary, suffix-sorts it
//                             (replicated: O(|D|) << n for repetitive input), translates its own
//                             parse to global lexicographic ranks
//   -- allgather of parse symbols / last / sai --
//   3. pfp_dist_merge       : BWT of the parse (replicated) and the slice [lo,hi) of the final BWT/SA
// The collectives live in big-bwt_amd/dist.py (torch.distributed over RCCL/xGMI).
#include "chain.hpp"

using namespace pfp;

struct DistState {
  StagedText tx;
  DBuf<uint64_t> ends;
  uint64_t n_ends = 0, n_local = 0, k0 = 0, P_local = 0;
  int w = 0;
  Dictionary L;                 // local dictionary + local parse
  Dictionary G;                 // global dictionary (identical on every rank)
  DictIndex ix;
  DictOrder ord;
  DBuf<uint32_t> occ_lex;
  uint64_t local_total = 0;     // BWT positions the held slots emit
  BwtOutputs out;               // -s / -e without an SA slice: run maps and per-boundary SA values of the emitted slice
  uint64_t out_lo = 0;
  bool slice_empty = true;      // the last pfp_dist_merge emitted no position
  bool want_sai = false;
  int flags = 0;                // output flags announced at pfp_dist_local_parse (0: BWT only)
  // hash-partitioned dedup (pfp_dist_partition_words ...): local words in owner order, the words this rank owns,
  // and the global id of every local word once the owners have answered
  DBuf<uint32_t> part_order;    // [L.d] local word ids, grouped by owner
  Dictionary Own;               // distinct words of this rank's hash class (first-arrival order) with summed occ
  DBuf<uint32_t> gid_local;     // [L.d] global word id of local word j
  bool have_gid = false;
  DBuf<uint32_t> parse_sa;      // [P + 1] the parse's suffix array gathered from the ranks' shares (pfp_dist_set_parse_sa), used by the next merge
  uint64_t parse_sa_n = 0;
  uint64_t parse_share_rounds = 0;      // rounds of this rank's share sort (reported when the gathered array is used)
};
static DistState *dist_of(pfp_ctx *c) {
  if (!c->dist) c->dist = new DistState();
  return c->dist;
}

__global__ void count_below_kernel(const uint64_t *__restrict__ ends, uint64_t ne, uint64_t bound, uint64_t *out) {
  uint64_t lo = 0, hi = ne;                   // first index with ends[idx] >= bound
  while (lo < hi) { uint64_t mid = (lo + hi) >> 1; if (ends[mid] < bound) lo = mid + 1; else hi = mid; }
  out[0] = lo;
  out[1] = ne ? ends[ne - 1] : ~0ull;
}
__global__ void dist_sym_kernel(uint64_t P, const uint32_t *__restrict__ lpid, uint64_t word_base,
                                const uint32_t *__restrict__ gid_of_union, const uint32_t *__restrict__ lexrank,
                                uint32_t *__restrict__ sym) {
  uint64_t k = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (k < P) sym[k] = lexrank[gid_of_union[word_base + lpid[k]]] + 1;
}
// hash class of every local word: owner = (hash >> 20) % parts; per-owner word and byte counts
// (counts are summed per workgroup in LDS first: one atomic per workgroup and owner, not one per word - with few
// owners every word would hit the same two addresses)
__global__ __launch_bounds__(256) void word_owner_kernel(uint32_t d, const uint64_t *__restrict__ hash, const uint32_t *__restrict__ wlen,
                                                         uint32_t parts, uint32_t *__restrict__ owner, uint32_t *__restrict__ ids,
                                                         unsigned long long *__restrict__ counts) {
  __shared__ unsigned long long lc[2 * 64];
  const uint32_t np = parts < 64 ? parts : 64;      // owners beyond 64 (not a single-node case) go straight to global memory
  for (uint32_t q = threadIdx.x; q < 2 * np; q += 256) lc[q] = 0;
  __syncthreads();
  uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j < d) {
    const uint32_t o = (uint32_t)((hash[j] >> 20) % parts);
    owner[j] = o; ids[j] = j;
    unsigned long long *dst = o < np ? lc : counts;
    atomicAdd(&dst[2 * o], 1ull);
    atomicAdd(&dst[2 * o + 1], (unsigned long long)wlen[j] + 1);
  }
  __syncthreads();
  for (uint32_t q = threadIdx.x; q < 2 * np; q += 256) if (lc[q]) atomicAdd(&counts[q], lc[q]);
}
__global__ void gather_u32_kernel(uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ src, uint32_t *__restrict__ dst) {
  uint32_t i = BID * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[idx[i]];
}
__global__ void scatter_u32_kernel(uint32_t n, const uint32_t *__restrict__ idx, const uint32_t *__restrict__ src, uint32_t *__restrict__ dst) {
  uint32_t i = BID * blockDim.x + threadIdx.x;
  if (i < n) dst[idx[i]] = src[i];
}
__global__ void len1_of_kernel(uint32_t n, const uint32_t *__restrict__ order, const uint32_t *__restrict__ wlen, uint32_t *__restrict__ len1) {
  uint32_t i = BID * blockDim.x + threadIdx.x;
  if (i == 0) len1[n] = 0;
  if (i < n) len1[i] = wlen[order[i]] + 1;
}
__global__ void dist_sym_gid_kernel(uint64_t P, const uint32_t *__restrict__ lpid, const uint32_t *__restrict__ gid_local,
                                    const uint32_t *__restrict__ lexrank, uint32_t *__restrict__ sym) {
  uint64_t k = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (k < P) sym[k] = lexrank[gid_local[lpid[k]]] + 1;
}

__global__ __launch_bounds__(256) void sum_u32_kernel(const uint32_t *__restrict__ v, uint64_t n, unsigned long long *__restrict__ total) {
  unsigned long long s = 0;
  for (uint64_t i = (uint64_t)BID * 256 + threadIdx.x; i < n; i += (uint64_t)GDIM * 256) s += v[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}
template <class I>
__global__ void add_one_kernel(uint32_t n, const I *__restrict__ in, uint64_t *__restrict__ out) {
  uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j < n) out[j] = (uint64_t)in[j] + 1;
}

extern "C" {

// Extra trigger hashes this rank would add to split its giant phrases (<= 8, see scan.hip).  The
// caller allgathers the proposals and hands the union to every rank's pfp_dist_local_parse, so that
// all ranks scan with ONE trigger set.
int pfp_dist_propose_triggers(pfp_ctx *c, const void *d_text, uint64_t n, int w, uint64_t p, uint32_t out_hashes[8],
                              uint32_t *n_hashes) {
  if (!c || (!d_text && n) || !out_hashes || !n_hashes) return PFP_EINVAL;
  *n_hashes = 0;
  PFP_TRY_DEV(c)
  check_args(w, p, 0);
  if (!c->max_phrase) return PFP_OK;
  StagedText tx;
  tx.stage(c, d_text, true, n, w);
  DBuf<uint64_t> ends;
  uint64_t used = 0;
  KRParams kp = make_kr_params(w, p);
  uint64_t ne = scan_text(c, tx, n, w, p, ends, &used, &kp);
  propose_extra_triggers(c, tx, used, w, c->max_phrase, ends, ne, kp);
  for (uint32_t q = 0; q < kp.nextra && q < 8; q++) out_hashes[(*n_hashes)++] = kp.extra[q];
  return PFP_OK;
  PFP_CATCH(c)
}

// ---- the collection's parse plan (round 4): which hash cuts the text, with which seed, how densely
// plan[0] 0 = the reference's Karp-Rabin hash, 1 = the window hash of scan.hip, 2 = the same at a pinned density (no nominal
// threshold beside the scan's); plan[1] its seed; plan[2] the density (a double's bits, exactly the value the single-GPU chain
// computes its thresholds from: the text is cut with probability density / p); plan[3] 1 while the density is a candidate the
// ranks still have to decide on (scan.hip: params_from_plan)
// Rank 0 (which holds the text's first bytes) makes the plan; the hosts hand it to every rank.  first_hash: the hash of the text's
// first window under the plan (it must not become an extra trigger: SURVEY.md 2.2-Q1), ~0 when the text is shorter than a window.
int pfp_dist_parse_plan(pfp_ctx *c, const uint8_t *first_bytes, uint64_t n_bytes, int w, uint64_t p, uint32_t ranks, uint64_t plan[4],
                        uint64_t *first_hash) {
  if (!c || !plan || !first_hash || (!first_bytes && n_bytes)) return PFP_EINVAL;
  PFP_TRY(c)
  check_args(w, p, 0);
  const bool have = n_bytes >= (uint64_t)w;
  const double one = 1.0;
  *first_hash = ~0ull;
  if (!c->fast_triggers || w < 4 || w > 17) {
    plan[0] = 0; plan[1] = 0; memcpy(&plan[2], &one, 8); plan[3] = 0;
    if (have) { uint64_t h = 0; for (int k = 0; k < w; k++) h = (h * 256 + first_bytes[k]) % kPrime; *first_hash = h; }      // newscan.cpp:168-202
    return PFP_OK;
  }
  // (the dictionary's work is shared between the ranks, the parse's is not - every rank's merge reads the whole parse: shorter
  //  phrases pay on one or two ranks - 42.3 -> 35.8 and 51.1 -> 42.2 ms per rank - and no longer on eight, 71.9 -> 72.3; so the
  //  density is a candidate only there, and nominal beyond)
  const double setting = c->parse_density > 0 ? c->parse_density : (ranks > 2 ? 1.0 : 0.0);
  double dens = 1.0;
  const KRParams kp = make_fast_params_host(have ? first_bytes : nullptr, w, p, setting, &dens);
  plan[0] = setting > 0 ? 2 : 1; plan[1] = kp.fseed; memcpy(&plan[2], &dens, 8); plan[3] = kp.fauto;
  if (have) *first_hash = window_hash_host(first_bytes, w, kp.fseed);
  return PFP_OK;
  PFP_CATCH(c)
}
// pfp_dist_propose_triggers under a plan; while the plan's density is a candidate (plan[3]) also this rank's sample of the cuts
// at or after halo_len: at most sample_cap sorted context hashes in d_sample, *n_sample of them (the hosts all-gather the samples
// and every rank decides alike: pfp_dist_decide_density)
int pfp_dist_propose_triggers2(pfp_ctx *c, const void *d_text, uint64_t n, uint64_t halo_len, int w, uint64_t p, const uint64_t plan[4],
                               uint32_t out_hashes[8], uint32_t *n_hashes, void *d_sample, uint64_t sample_cap, uint64_t *n_sample) {
  if (!c || (!d_text && n) || !out_hashes || !n_hashes || !plan || !n_sample || (sample_cap && !d_sample)) return PFP_EINVAL;
  *n_hashes = 0; *n_sample = 0;
  PFP_TRY_DEV(c)
  check_args(w, p, 0);
  if (!c->max_phrase && !plan[3]) return PFP_OK;
  StagedText tx;
  tx.stage(c, d_text, true, n, w);
  DBuf<uint64_t> ends;
  uint64_t used = 0;
  KRParams kp = params_from_plan(w, p, plan);
  const uint64_t ne = scan_text(c, tx, n, w, p, ends, &used, &kp);
  // (proposals only under a SETTLED plan: a window of a periodic stretch may cut at the candidate density and not at the nominal
  //  one - the stretch then looks harmless here and is one giant phrase in the parse; the hosts call this twice while plan[3] is set:
  //  for the sample first, for the proposals after pfp_dist_decide_density)
  if (c->max_phrase && !plan[3]) {
    propose_extra_triggers(c, tx, used, w, c->max_phrase, ends, ne, kp);
    for (uint32_t q = 0; q < kp.nextra && q < 8; q++) out_hashes[(*n_hashes)++] = kp.extra[q];
  }
  if (plan[3] && kp.fast && ne) {
    CutSample cs;
    classify_cuts(c, tx, w, ends, ne, kp, halo_len, cs);
    const uint64_t take = std::min<uint64_t>(cs.ns, sample_cap);
    if (take) PFP_HIP(hipMemcpyAsync(d_sample, cs.hashes.p, take * 8, hipMemcpyDeviceToDevice, c->stream));
    sync(c);
    *n_sample = take;
  }
  return PFP_OK;
  PFP_CATCH(c)
}
// the ranks' samples, gathered: every rank sorts them and settles the plan's density the same way (candidate kept or 1)
int pfp_dist_decide_density(pfp_ctx *c, const void *d_samples, uint64_t count, uint64_t p, uint64_t plan[4]) {
  if (!c || !plan || (count && !d_samples)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  if (!plan[3]) return PFP_OK;
  bool dense = false;
  if (count >= 1024) {
    DBuf<uint64_t> sorted(c, count);
    sort_keys_raw(c, (const uint64_t *)d_samples, sorted.p, count, 0, 64);
    dense = sample_says_dense(c, sorted.p, count, p);
  }
  const double one = 1.0;
  if (!dense) memcpy(&plan[2], &one, 8);
  plan[3] = 0;
  return PFP_OK;
  PFP_CATCH(c)
}

static int dist_local_parse_impl(pfp_ctx *c, const void *d_text, uint64_t n, uint64_t halo_len, int w, uint64_t p, int is_first,
                                 int is_last, uint64_t global_offset, int want_sai, const uint64_t *plan, const uint32_t *extra_hashes,
                                 uint32_t n_extra, uint64_t out_sizes[4]) {
  if (!c || (!d_text && n) || !out_sizes || (n_extra && !extra_hashes)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  check_args(w, p, want_sai & 7);      // (callers pass the output flags here: -S with -s/-e is refused like bigbwt:59-61)
  PFP_REQUIRE(n_extra <= KRParams::kMaxExtra, PFP_EINVAL, "too many extra trigger hashes");
  PFP_REQUIRE(is_first ? halo_len == 0 : halo_len >= (uint64_t)w, PFP_EINVAL, "halo must hold at least one window");
  PFP_REQUIRE(halo_len <= n, PFP_EINVAL, "halo longer than the local text");
  DistState *ds = dist_of(c);
  *ds = DistState();
  ds->w = w; ds->n_local = n;
  pfp_stats &st = c->stats;
  st = pfp_stats{};
  ds->tx.stage(c, d_text, true, n, w);
  uint64_t used = 0;
  KRParams kp = params_from_plan(w, p, plan);                      // one trigger set on all ranks
  st.parse_density = kp.fast ? (double)kp.fdens : 1.0;
  for (uint32_t q = 0; q < n_extra; q++) { kp.extra[kp.nextra++] = extra_hashes[q]; kp.bloom |= 1ull << (extra_hashes[q] & 63); }
  { PhaseTimer t(c, &st.ms_scan);
    ds->n_ends = scan_text(c, ds->tx, n, w, p, ds->ends, &used, &kp); }
  PFP_REQUIRE(used == n, PFP_EFORMAT, "bytes <= 2 inside a text shard are not supported in the multi-GPU chain");
  DBuf<uint64_t> tmp(c, 2);
  hipLaunchKernelGGL(count_below_kernel, gdim(1), gdim(1), 0, c->stream, ds->ends.p, ds->n_ends, halo_len, tmp.p);
  PFP_HIP(hipMemcpyAsync(c->h_scalars, tmp.p, 16, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  ds->k0 = is_first ? 0 : c->h_scalars[0];
  const uint64_t last_end = c->h_scalars[1];
  PFP_REQUIRE(is_first || ds->k0 >= 1, PFP_ELIMIT, "no phrase boundary inside the halo: a phrase is longer than the halo");
  const uint64_t kend = is_last ? ds->n_ends + 1 : ds->n_ends;      // the partial tail phrase belongs to the next rank
  PFP_REQUIRE(kend > ds->k0, PFP_ESHORT, "text shard holds no complete phrase");
  ds->P_local = kend - ds->k0;
  // T' index x of the local text is global text position global_offset - halo_len + x - 1; sai = end position + 1
  const uint64_t sai_base = global_offset - halo_len;
  ds->want_sai = want_sai != 0;
  ds->flags = want_sai & 7;     // callers pass the output flags here (any non-zero value asks for sa info)
  { PhaseTimer t(c, &st.ms_phrases);
    build_dictionary_shard(c, ds->tx, n, w, ds->ends, ds->n_ends, ds->k0, ds->P_local, want_sai != 0, sai_base, ds->L); }
  st.n = n - halo_len; st.n_phrases = ds->P_local; st.extra_triggers = n_extra;
  out_sizes[0] = ds->L.dsize - 1;      // local dictionary bytes without the final 0x00
  out_sizes[1] = ds->L.d;
  out_sizes[2] = ds->P_local;
  out_sizes[3] = last_end;             // local position of the last trigger (the next rank's halo must reach it)
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_dist_local_parse(pfp_ctx *c, const void *d_text, uint64_t n, uint64_t halo_len, int w, uint64_t p, int is_first,
                         int is_last, uint64_t global_offset, int want_sai, const uint32_t *extra_hashes,
                         uint32_t n_extra, uint64_t out_sizes[4]) {
  return dist_local_parse_impl(c, d_text, n, halo_len, w, p, is_first, is_last, global_offset, want_sai, nullptr, extra_hashes, n_extra, out_sizes);
}
// the same under a (decided) parse plan
int pfp_dist_local_parse2(pfp_ctx *c, const void *d_text, uint64_t n, uint64_t halo_len, int w, uint64_t p, int is_first,
                          int is_last, uint64_t global_offset, int want_sai, const uint64_t plan[4], const uint32_t *extra_hashes,
                          uint32_t n_extra, uint64_t out_sizes[4]) {
  if (!plan || plan[3]) return PFP_EINVAL;
  return dist_local_parse_impl(c, d_text, n, halo_len, w, p, is_first, is_last, global_offset, want_sai, plan, extra_hashes, n_extra, out_sizes);
}

int pfp_dist_export_local(pfp_ctx *c, void *d_dict, void *d_occ, void *d_last, void *d_sai) {
  if (!c || !c->dist) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  if (d_dict) PFP_HIP(hipMemcpyAsync(d_dict, ds->L.bytes.p, ds->L.dsize - 1, hipMemcpyDeviceToDevice, c->stream));
  if (d_occ) PFP_HIP(hipMemcpyAsync(d_occ, ds->L.wocc.p, ds->L.d * 4, hipMemcpyDeviceToDevice, c->stream));
  if (d_last) PFP_HIP(hipMemcpyAsync(d_last, ds->L.last.p, ds->P_local, hipMemcpyDeviceToDevice, c->stream));
  if (d_sai) {
    PFP_REQUIRE(ds->L.sai.p, PFP_EINVAL, "sa info was not requested in pfp_dist_local_parse");
    PFP_HIP(hipMemcpyAsync(d_sai, ds->L.sai.p, ds->P_local * 8, hipMemcpyDeviceToDevice, c->stream));
  }
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

}  // extern "C"
// the global dictionary ds->G is in place: index it and sort its suffixes (replicated, or this rank's key range)
static void dist_sort_global(pfp_ctx *c, DistState *ds, uint32_t part, uint32_t parts, void *d_wslot_out, uint64_t out_info[8]) {
  PhaseTimer t_sa(c, &c->stats.ms_sa_dict);
  ds->ix = DictIndex();
  ds->ord = DictOrder();
  build_dict_index(c, ds->G, ds->ix);
  const uint32_t d = (uint32_t)ds->G.d;
  const WordView wv = word_view(ds->G, ds->ix);
  const SlotPayloadSrc pay{wv, ds->G.wocc.p, ds->w};
  const SlotPayloadSrc *payp = (ds->flags & PFP_FLAG_SA) ? nullptr : &pay;      // full SA: the merge gathers wider records itself
  // a share of a dictionary of 2^31 bytes or more takes the wide build: the 32-bit one has no spare bit for the settled flag
  // there, so no pivot rounds - and a share cannot run doubling rounds instead (they read other shares' ranks).  The share is
  // 1 / parts of the slots, so 8-byte indices are affordable where they would not be for the whole array.
  ds->ord.wide = use_wide_index(c, ds->G.dsize) || (parts > 1 && ds->G.dsize >= (1ull << 31));
  // phrases per distinct word = text bytes per dictionary byte, near enough (the same on every rank: the keys-only
  // first round of the sorter is chosen from it)
  double rep_hint = 0;
  {
    DBuf<unsigned long long> tot(c, 1);
    tot.zero();
    hipLaunchKernelGGL(sum_u32_kernel, gdim((int)std::min<uint64_t>(cdiv64(d, 256), 1024)), gdim(256), 0, c->stream, ds->G.wocc.p, (uint64_t)d, tot.p);
    rep_hint = (double)read_scalar(c, (const uint64_t *)tot.p) / (double)std::max<uint32_t>(d, 1);
  }
  uint64_t info_rounds = 0, info_complete = 1, info_N = 0, info_base = 0;
  with_width(ds->ord.wide, [&](auto tag) {
    using I = decltype(tag);
    auto &so = ds->ord.get<I>();
    so.rep_hint = rep_hint;
    if (parts == 1) {
      sort_dict_suffixes<I>(c, ds->G.bytes.p, ds->G.dsize, wv, so, payp);
      if (c->debug) validate_suffix_order<I>(c, ds->G.bytes.p, so, true, "global dict SA");
      DBuf<I> slots(c, d);
      gather_ranks<I>(c, so, ds->G.woff.p, d, slots.p);
      hipLaunchKernelGGL(add_one_kernel<I>, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, slots.p, (uint64_t *)d_wslot_out);
      ds->local_total = 0;
    } else {
      sort_dict_suffixes_range<I>(c, ds->G.bytes.p, ds->G.dsize, wv, part, parts, so, payp, &pay);
      gather_slots_range<I>(c, so, wv, d, (uint64_t *)d_wslot_out);
      ds->local_total = so.complete ? so.range_emits : 0;
      if (c->debug && so.complete)
        PFP_REQUIRE(count_slot_outputs<I>(c, ds->G, ds->ix, so, ds->w) == ds->local_total, PFP_EHIP,
                    "emit count by position differs from the count by slot");
    }
    info_rounds = so.rounds; info_complete = so.complete ? 1 : 0; info_N = so.N; info_base = so.slot_base;
  });
  PFP_HIP(hipGetLastError());
  sync(c);
  out_info[0] = ds->G.d; out_info[1] = ds->G.dsize; out_info[2] = info_rounds; out_info[3] = info_complete;
  out_info[4] = info_N; out_info[5] = info_base; out_info[6] = ds->local_total; out_info[7] = ds->ord.wide ? 64 : 32;
  c->stats.n_words = ds->G.d; c->stats.dict_size = ds->G.dsize; c->stats.sa_rounds_dict = info_rounds;
  c->stats.index_bits = ds->ord.wide ? 64 : 32;
}
extern "C" {

int pfp_dist_global_sort(pfp_ctx *c, const void *d_union, uint64_t union_bytes, const void *d_union_occ, uint64_t n_union,
                         uint32_t part, uint32_t parts, void *d_wslot_out, uint64_t out_info[8]) {
  if (!c || !c->dist || !d_union || !d_union_occ || !d_wslot_out || !out_info || parts < 1 || part >= parts) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  PFP_REQUIRE(n_union >= 1, PFP_EINVAL, "empty union");
  // the union is itself a (not sorted, not duplicate-free) dictionary: words + 0x01, closed by one 0x00
  Dictionary U;
  U.dsize = union_bytes + 1;
  U.bytes.alloc(c, U.dsize + 64);
  PFP_HIP(hipMemcpyAsync(U.bytes.p, d_union, union_bytes, hipMemcpyDeviceToDevice, c->stream));
  PFP_HIP(hipMemsetAsync(U.bytes.p + union_bytes, 0, 65, c->stream));
  word_table_from_bytes(c, U, n_union);           // only the word boundaries of the union are needed
  PFP_REQUIRE(U.d == n_union, PFP_EFORMAT, "the union holds a different number of words than occ entries");
  ds->G = Dictionary();
  ds->have_gid = false;
  build_dictionary_words(c, U.bytes.p, U.woff.p, U.wlen.p, n_union, (const uint32_t *)d_union_occ, union_bytes, ds->G);
  dist_sort_global(c, ds, part, parts, d_wslot_out, out_info);
  return PFP_OK;
  PFP_CATCH(c)
}

// ---- hash-partitioned dedup: every distinct word is owned by the rank its hash points at (SURVEY 8e exchange A; the
//      reference's threaded parser shards its maps by hash % (3 N) the same way, pscan.cpp:137-205)
int pfp_dist_partition_words(pfp_ctx *c, uint32_t parts, uint64_t *counts /* [2 * parts]: words, bytes (+1 per word) per owner */) {
  if (!c || !c->dist || !counts || parts < 1) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  const uint32_t d = (uint32_t)ds->L.d;
  PFP_REQUIRE(d >= 1, PFP_EINVAL, "pfp_dist_local_parse has not run");
  DBuf<uint64_t> hash(c, d);
  hash_word_list(c, ds->L.bytes.p, ds->L.woff.p, ds->L.wlen.p, d, 0x6A09E667F3BCC909ULL, hash.p);
  DBuf<uint32_t> owner(c, d), ownero(c, d), ids(c, d);
  DBuf<unsigned long long> cnt(c, 2 * (size_t)parts);
  cnt.zero();
  hipLaunchKernelGGL(word_owner_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, hash.p, ds->L.wlen.p, parts, owner.p, ids.p, cnt.p);
  ds->part_order.alloc(c, d);
  sort_pairs_u32_u32(c, owner.p, ownero.p, ids.p, ds->part_order.p, d, 0, bits_for(parts));      // stable: local order inside an owner
  PFP_HIP(hipGetLastError());
  PFP_HIP(hipMemcpyAsync(counts, cnt.p, 2 * (size_t)parts * 8, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_dist_export_partition(pfp_ctx *c, void *d_bytes, void *d_occ) {
  if (!c || !c->dist || !d_bytes || !d_occ) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  const uint32_t d = (uint32_t)ds->L.d;
  PFP_REQUIRE(ds->part_order.p, PFP_EINVAL, "pfp_dist_partition_words has not run");
  DBuf<uint32_t> len1(c, (size_t)d + 1);
  DBuf<uint64_t> doff(c, (size_t)d + 1);
  hipLaunchKernelGGL(len1_of_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, ds->part_order.p, ds->L.wlen.p, len1.p);
  exclusive_sum_u32_u64(c, len1.p, doff.p, (size_t)d + 1);
  permute_dictionary(c, d, ds->part_order.p, ds->L.woff.p, ds->L.wlen.p, ds->L.bytes.p, doff.p, (uint8_t *)d_bytes);
  hipLaunchKernelGGL(gather_u32_kernel, gdim(cdiv(d, TB)), gdim(TB), 0, c->stream, d, ds->part_order.p, ds->L.wocc.p, (uint32_t *)d_occ);
  PFP_HIP(hipGetLastError());
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_dist_owner_dedup(pfp_ctx *c, const void *d_bytes, uint64_t nbytes, const void *d_occ, uint64_t n_words, void *d_pid_out,
                         uint64_t out[2]) {
  if (!c || !c->dist || !out || (n_words && (!d_bytes || !d_occ || !d_pid_out))) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  ds->Own = Dictionary();
  out[0] = out[1] = 0;
  if (!n_words) return PFP_OK;                 // nobody sent a word of this hash class
  Dictionary U;
  U.dsize = nbytes + 1;
  U.bytes.alloc(c, U.dsize + 64);
  PFP_HIP(hipMemcpyAsync(U.bytes.p, d_bytes, nbytes, hipMemcpyDeviceToDevice, c->stream));
  PFP_HIP(hipMemsetAsync(U.bytes.p + nbytes, 0, 65, c->stream));
  word_table_from_bytes(c, U, n_words);
  PFP_REQUIRE(U.d == n_words, PFP_EFORMAT, "the received words do not match their occ entries");
  build_dictionary_words(c, U.bytes.p, U.woff.p, U.wlen.p, n_words, (const uint32_t *)d_occ, nbytes, ds->Own);
  PFP_HIP(hipMemcpyAsync(d_pid_out, ds->Own.pid.p, n_words * 4, hipMemcpyDeviceToDevice, c->stream));
  sync(c);
  out[0] = ds->Own.d; out[1] = ds->Own.dsize - 1;
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_dist_export_owned(pfp_ctx *c, void *d_bytes, void *d_occ) {
  if (!c || !c->dist) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  if (!ds->Own.d) return PFP_OK;
  PFP_REQUIRE(d_bytes && d_occ, PFP_EINVAL, "null output");
  PFP_HIP(hipMemcpyAsync(d_bytes, ds->Own.bytes.p, ds->Own.dsize - 1, hipMemcpyDeviceToDevice, c->stream));
  PFP_HIP(hipMemcpyAsync(d_occ, ds->Own.wocc.p, ds->Own.d * 4, hipMemcpyDeviceToDevice, c->stream));
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

// d_dict / d_occ: the owners' distinct words back to back (owner 0 first) = the global dictionary, duplicate free by
// construction; d_gid_sent: the global id of every local word in the order pfp_dist_export_partition sent them
int pfp_dist_global_sort_distinct(pfp_ctx *c, const void *d_dict, uint64_t dict_bytes, const void *d_occ, uint64_t n_words,
                                  const void *d_gid_sent, uint32_t part, uint32_t parts, void *d_wslot_out, uint64_t out_info[8]) {
  if (!c || !c->dist || !d_dict || !d_occ || !d_gid_sent || !d_wslot_out || !out_info || parts < 1 || part >= parts) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  PFP_REQUIRE(n_words >= 1 && n_words < 0xFFFFFFFFull, PFP_EINVAL, "bad word count");
  PFP_REQUIRE(ds->part_order.p, PFP_EINVAL, "pfp_dist_partition_words has not run");
  ds->G = Dictionary();
  ds->G.dsize = dict_bytes + 1;
  ds->G.bytes.alloc(c, ds->G.dsize + 64);
  PFP_HIP(hipMemcpyAsync(ds->G.bytes.p, d_dict, dict_bytes, hipMemcpyDeviceToDevice, c->stream));
  PFP_HIP(hipMemsetAsync(ds->G.bytes.p + dict_bytes, 0, 65, c->stream));
  word_table_from_bytes(c, ds->G, n_words);
  PFP_REQUIRE(ds->G.d == n_words, PFP_EFORMAT, "the global dictionary holds a different number of words than occ entries");
  ds->G.wocc.alloc(c, n_words);
  PFP_HIP(hipMemcpyAsync(ds->G.wocc.p, d_occ, n_words * 4, hipMemcpyDeviceToDevice, c->stream));
  const uint32_t dl = (uint32_t)ds->L.d;
  ds->gid_local.alloc(c, dl);
  static const bool by_occ = getenv("PFP_DIST_NO_OCC_ORDER") == nullptr;      // (diagnostic: the owners' order as it arrived)
  if (by_occ) {
    // most frequent words first: the pivots of the suffix sorter's pivot rounds become the words the variants deviate from
    DBuf<uint32_t> perm, gid(c, std::max<uint32_t>(dl, 1));
    { PhaseTimer t(c, &c->stats.ms_phrases); reorder_dictionary_by_occ(c, ds->G, perm); }
    hipLaunchKernelGGL(gather_u32_kernel, gdim(cdiv(dl, TB)), gdim(TB), 0, c->stream, dl, (const uint32_t *)d_gid_sent, perm.p, gid.p);
    hipLaunchKernelGGL(scatter_u32_kernel, gdim(cdiv(dl, TB)), gdim(TB), 0, c->stream, dl, ds->part_order.p, gid.p, ds->gid_local.p);
    sync(c);      // perm and gid are released on return
  } else
    hipLaunchKernelGGL(scatter_u32_kernel, gdim(cdiv(dl, TB)), gdim(TB), 0, c->stream, dl, ds->part_order.p, (const uint32_t *)d_gid_sent,
                       ds->gid_local.p);
  ds->have_gid = true;
  dist_sort_global(c, ds, part, parts, d_wslot_out, out_info);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_dist_global_finish(pfp_ctx *c, const void *d_wslot_all, uint32_t parts, uint64_t my_word_base, void *d_sym_out) {
  if (!c || !c->dist || !d_wslot_all || !d_sym_out || parts < 1) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  const uint32_t d = (uint32_t)ds->G.d;
  PFP_REQUIRE(d >= 1, PFP_EINVAL, "pfp_dist_global_sort has not run");
  compute_lexrank_from_slots(c, ds->G, (const uint64_t *)d_wslot_all, parts, ds->ix);
  if (c->debug) validate_lexrank(c, ds->G, ds->ix);
  ds->occ_lex.alloc(c, d);
  occ_in_lex_order(c, d, ds->ix.lexrank.p, ds->G.wocc.p, ds->occ_lex.p, nullptr);
  if (ds->have_gid)
    hipLaunchKernelGGL(dist_sym_gid_kernel, gdim(cdiv(ds->P_local, TB)), gdim(TB), 0, c->stream, ds->P_local, ds->L.pid.p,
                       ds->gid_local.p, ds->ix.lexrank.p, (uint32_t *)d_sym_out);
  else
    hipLaunchKernelGGL(dist_sym_kernel, gdim(cdiv(ds->P_local, TB)), gdim(TB), 0, c->stream, ds->P_local, ds->L.pid.p,
                       my_word_base, ds->G.pid.p, ds->ix.lexrank.p, (uint32_t *)d_sym_out);
  PFP_HIP(hipGetLastError());
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

// the two steps above on one rank holding the whole suffix array (no exchange in between)
int pfp_dist_global(pfp_ctx *c, const void *d_union, uint64_t union_bytes, const void *d_union_occ, uint64_t n_union,
                    uint64_t my_word_base, void *d_sym_out, uint64_t out_info[3]) {
  if (!c || !c->dist || !d_union || !d_union_occ || !d_sym_out || !out_info) return PFP_EINVAL;
  uint64_t info[8];
  uint64_t *wslot = nullptr;
  if (hipSetDevice(c->device) != hipSuccess || hipMalloc((void **)&wslot, (n_union ? n_union : 1) * 8) != hipSuccess) return PFP_ENOMEM;
  int rc = pfp_dist_global_sort(c, d_union, union_bytes, d_union_occ, n_union, 0, 1, wslot, info);
  if (rc == PFP_OK) rc = pfp_dist_global_finish(c, wslot, 1, my_word_base, d_sym_out);
  (void)hipFree(wslot);
  if (rc == PFP_OK) { out_info[0] = info[0]; out_info[1] = info[1]; out_info[2] = info[2]; }
  return rc;
}

int pfp_dist_parse_sort(pfp_ctx *c, const void *d_sym, uint64_t P, uint32_t part, uint32_t parts, void *d_sa_out, uint64_t out_info[4]) {
  if (!c || !c->dist || !d_sym || !d_sa_out || !out_info || parts < 1 || part >= parts) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  PFP_REQUIRE(ds->occ_lex.p && ds->G.d, PFP_EINVAL, "pfp_dist_global_finish has not run");
  PFP_REQUIRE(P >= 2, PFP_ESHORT, "parse has fewer than 2 phrases (bwtparse.c:244)");
  PhaseTimer t(c, &c->stats.ms_sa_parse);
  DBuf<uint32_t> sym(c, P + 1);      // the parse and its end symbol (bwtparse.c:212-230)
  PFP_HIP(hipMemcpyAsync(sym.p, d_sym, P * 4, hipMemcpyDeviceToDevice, c->stream));
  PFP_HIP(hipMemsetAsync(sym.p + P, 0, 4, c->stream));
  SuffixOrder so;
  sort_int_suffixes_range(c, sym.p, P + 1, (uint32_t)ds->G.d, ds->occ_lex.p, (uint32_t)ds->G.d, part, parts, so);
  if (so.complete && so.N) PFP_HIP(hipMemcpyAsync(d_sa_out, so.sa.p, so.N * 4, hipMemcpyDeviceToDevice, c->stream));
  sync(c);
  out_info[0] = so.N; out_info[1] = so.slot_base; out_info[2] = so.complete ? 1 : 0; out_info[3] = so.rounds;
  ds->parse_share_rounds = so.rounds;
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_dist_set_parse_sa(pfp_ctx *c, const void *d_sa, uint64_t count) {
  if (!c || !c->dist || (!d_sa && count)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  ds->parse_sa.release(); ds->parse_sa_n = 0;
  if (!count) return PFP_OK;
  ds->parse_sa.alloc(c, count);
  PFP_HIP(hipMemcpyAsync(ds->parse_sa.p, d_sa, count * 4, hipMemcpyDeviceToDevice, c->stream));
  sync(c);
  ds->parse_sa_n = count;
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_dist_merge(pfp_ctx *c, const void *d_sym, uint64_t P, const void *d_last, const void *d_sai, int flags,
                   uint64_t n_total, uint64_t out_lo, uint64_t out_hi, void *d_bwt_slice, void *d_sa_slice) {
  if (!c || !c->dist || !d_sym || !d_last || !d_bwt_slice || (flags && !d_sai) || ((flags & PFP_FLAG_SA) && !d_sa_slice)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  check_args(ds->w, 10, flags);
  PFP_REQUIRE(flags == ds->flags, PFP_EINVAL, "output flags differ from those announced at pfp_dist_local_parse");
  PFP_REQUIRE(out_lo <= out_hi && out_hi <= n_total + 1, PFP_EINVAL, "bad output slice");
  ParseBWT pb;
  { PhaseTimer t(c, &c->stats.ms_sa_parse);
    PFP_REQUIRE(!ds->parse_sa_n || ds->parse_sa_n == P + 1, PFP_EINVAL, "the gathered suffix array of the parse has " +
                std::to_string(ds->parse_sa_n) + " entries, the parse " + std::to_string(P) + " phrases");
    parse_bwt(c, (const uint32_t *)d_sym, P, (const uint8_t *)d_last, flags ? (const uint64_t *)d_sai : nullptr,
              ds->occ_lex.p, ds->G.d, pb, ds->parse_sa_n ? ds->parse_sa.p : nullptr);
    c->stats.sa_rounds_parse = ds->parse_sa_n ? ds->parse_share_rounds : pb.rounds;
    ds->parse_sa.release(); ds->parse_sa_n = 0; }
  if (c->debug) validate_parse_bwt(c, pb);
  ds->out = BwtOutputs();       // (-s / -e with d_sa_slice == NULL: what pfp_dist_sample_runs reads afterwards)
  ds->out_lo = out_lo;
  ds->slice_empty = out_hi == out_lo;
  BwtOutputs &bo = ds->out;
  bo.d_bwt = (uint8_t *)d_bwt_slice; bo.d_sa = (uint64_t *)d_sa_slice;
  bool empty_share = false;
  PhaseTimer t_merge(c, &c->stats.ms_merge);
  with_width(ds->ord.wide, [&](auto tag) {
    using I = decltype(tag);
    auto &so = ds->ord.get<I>();
    if (so.range) {
      // the held slots are one contiguous range of SA(D): they emit exactly [out_lo, out_hi)
      PFP_REQUIRE(so.complete, PFP_EINVAL, "this share of the suffix array is incomplete: redo pfp_dist_global_sort with parts = 1");
      PFP_REQUIRE(out_hi - out_lo == ds->local_total, PFP_EINVAL, "output range does not match this share's occurrence count");
      if (so.N == 0) { empty_share = true; return; }      // an empty share of the key space emits nothing
      merge_bwt<I>(c, ds->G, ds->ix, so, pb, ds->occ_lex.p, MergeOpts::slot_range(ds->w, flags, ds->local_total, out_lo, n_total + 1), bo);
    } else {
      merge_bwt<I>(c, ds->G, ds->ix, so, pb, ds->occ_lex.p, MergeOpts::slice(ds->w, flags, n_total + 1, out_lo, out_hi), bo);
    }
  });
  (void)empty_share;
  { pfp_stats &st = c->stats;
    st.hard_groups = bo.hard_groups; st.hard_chars = bo.hard_chars; st.hard_big_groups = bo.hard_big_groups;
    st.hard_max_members = bo.hard_max_members; st.hard_minor_groups = bo.hard_minor_groups; st.hard_minor_chars = bo.hard_minor_chars; }
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_dist_sample_runs(pfp_ctx *c, int run_end, int drop_edge, void *d_out10, uint64_t cap_pairs, uint64_t *n_pairs) {
  if (!c || !c->dist || !n_pairs) return PFP_EINVAL;
  *n_pairs = 0;
  PFP_TRY_DEV(c)
  DistState *ds = dist_of(c);
  PFP_REQUIRE((ds->flags & (PFP_FLAG_SSA | PFP_FLAG_ESA)) && !(ds->flags & PFP_FLAG_SA), PFP_EINVAL,
              "pfp_dist_sample_runs: the chain was not run with -s / -e");
  PFP_REQUIRE((run_end ? PFP_FLAG_ESA : PFP_FLAG_SSA) & ds->flags, PFP_EINVAL, "this sampled file was not asked for");
  if (ds->slice_empty) return PFP_OK;      // this rank's slice of the BWT holds no position
  PFP_REQUIRE(ds->out.slice_n && ds->out.sa_c.p, PFP_EINVAL, "the last pfp_dist_merge left no run maps (it must run before, with an SA-less slice)");
  const SaView sv = sa_view(ds->out);
  const uint64_t k = sample_runs_maps(c, sv, ds->out.slice_n, run_end != 0, drop_edge != 0, ds->out_lo, nullptr);
  *n_pairs = k;
  if (!d_out10) return PFP_OK;
  PFP_REQUIRE(k <= cap_pairs, PFP_ELIMIT, "output buffer holds " + std::to_string(cap_pairs) + " pairs, the slice has " + std::to_string(k));
  sample_runs_maps(c, sv, ds->out.slice_n, run_end != 0, drop_edge != 0, ds->out_lo, (uint8_t *)d_out10);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

void pfp_dist_release(pfp_ctx *c) {
  if (!c || !c->dist) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete c->dist;
  c->dist = nullptr;
}

}  // extern "C"
