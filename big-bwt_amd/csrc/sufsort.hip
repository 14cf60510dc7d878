// sufsort.hip -- GPU suffix sorting by prefix doubling on group-head ranks.
//
// Replaces the reference's serial induced sorting (gsa/gsacak.c: sacak_int :2497-2500 used by
// bwtparse.c:167; gsacak :2502-2522 used by pfbwt.cpp:495; sacak :2492-2495 used by
// simplebwt.c:77).  Induced sorting is one long left-to-right/right-to-left dependency chain
// (gsacak.c:262-289); by SURVEY.md 2.2-Q11 any correct sorter yields the same arrays, so the
// MI355X build sorts by prefix doubling: every round is a device-wide radix sort of the still
// unresolved suffixes keyed by (group head, rank of the suffix h positions on), O(log maxlen)
// rounds, all state resident in HBM.
//
// Dictionary mode compares 0x01-terminated strings: the key of a suffix never looks past its
// own word's terminator, a group whose whole string is already inside the sorted prefix is
// final, and equal strings keep one shared rank.  That rank equality *is* the "same suffix"
// test the reference derives from the LCP array (pfbwt.cpp:204-209), so no LCP array is built.
// Ties stay in position order (stable sorts), which reproduces gsacak's separator order
// (gsacak.c:1559-1561).
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include <algorithm>
#include <cmath>
#include <optional>
#include <vector>
#include <cstdio>
#include <cstdlib>

namespace pfp {

enum : int { MODE_DICT = 0, MODE_PLAIN = 1 };

struct SufGeom {
  int mode; uint64_t N; WordView wv;            // dictionary mode: where the word of a position ends
  const uint32_t *sym = nullptr;                // plain mode on an integer string (unique smallest last symbol): the string
  const uint32_t *dist = nullptr;               // ... and, where the caller knows the symbols' frequencies (the parse), the distance from every
                                                // position to the next RARE symbol at or after it: see the parse's pivot rounds below
};
// length of the suffix string starting at i, terminator included
__device__ __forceinline__ uint64_t suf_len(const SufGeom &g, uint64_t i) {
  if (g.mode == MODE_DICT) return slen_of(g.wv, i) + 1;
  return g.N - i;
}

// The environment switches of the sorters: diagnostics, and the paths the tests and measurements compare against.  Every entry
// point (sort_dict_suffixes, sort_byte_suffixes, sort_int_suffixes, the two *_range) reads them once per call with
// sorter_switches() and hands the value down; nothing else in this file looks at the environment.
constexpr uint32_t kPivCapMax = 8192;      // widest window of a dictionary pivot round (its order key: see kPivBits)
struct SorterSwitches {
  bool finflag;                  // PFP_NO_FINFLAG unset.  (tests: without it, the length-gather path)
  bool finisher;                 // PFP_NO_FINISHER unset: the comparison finisher may end the rounds
  bool small_seg;                // PFP_NO_SMALLSEG unset: small groups are placed directly in LDS
  bool trace_rounds;             // PFP_TRACE_ROUNDS set: a line on stderr per round and per decision of a sorter
  uint32_t pivot_cap;            // PFP_PIVOT_CAP: bytes compared per member in a dictionary pivot round (512; below 16: no pivot rounds)
  int keybits;                   // PFP_KEYBITS: width of the dictionary's first-round key, 8..63; 0 (unset) = the computed width
  uint64_t parse_pivot_min;      // PFP_PARSE_PIVOT_MIN: smallest list a parse pivot round is tried on (2^16; tests run it on small inputs; 0 = never)
  int keysonly;                  // PFP_KEYSONLY: keys-only first round of a dictionary: 1 always, 0 never, -1 (unset) = by the input
  // 0 = the path before it, which the tests compare with byte for byte; unset or anything else = on:
  bool plain_lazy_rank;          // PFP_PLAIN_LAZY_RANK: plain mode keeps no rank[] until a doubling round asks for it
  bool plain_tiles;              // PFP_PLAIN_TILES: plain mode's first round regroups by the dictionary's tile scheme (heads0 / write_back0)
  bool dict_fold;                // PFP_DICT_FOLD: dictionary first round: the tile counts come from write_back0, keep0 is the first round's keep[] itself
  bool drop_short;               // PFP_DROP_SHORT: a minimum suffix length is honoured (0: every position is sorted)
  bool ipivot_batch;             // PFP_IPIVOT_BATCH: the parse pivot round's key kernel issues kIntPivBatch load steps together (0: the one-step loop)
  bool parse_keybits;            // PFP_PARSE_KEYBITS: a parse without equal neighbours gets the two-symbol key (0: the run key)
};
static SorterSwitches sorter_switches() {
  auto set = [](const char *name) { return getenv(name) != nullptr; };
  auto unless_zero = [](const char *name) { const char *e = getenv(name); return !e || atoi(e) != 0; };
  auto number = [](const char *name, auto parse, auto unset) { const char *e = getenv(name); return e ? parse(e) : unset; };
  SorterSwitches s;
  s.finflag = !set("PFP_NO_FINFLAG");
  s.finisher = !set("PFP_NO_FINISHER");
  s.small_seg = !set("PFP_NO_SMALLSEG");
  s.trace_rounds = set("PFP_TRACE_ROUNDS");
  s.pivot_cap = std::min(number("PFP_PIVOT_CAP", [](const char *e) { return (uint32_t)atoll(e); }, 512u), kPivCapMax);
  s.keybits = number("PFP_KEYBITS", [](const char *e) { return std::max(8, std::min(63, atoi(e))); }, 0);
  s.parse_pivot_min = number("PFP_PARSE_PIVOT_MIN", [](const char *e) { const uint64_t v = strtoull(e, nullptr, 10); return v ? v : ~0ull; },
                             (uint64_t)1 << 16);
  s.keysonly = number("PFP_KEYSONLY", atoi, -1);
  s.plain_lazy_rank = unless_zero("PFP_PLAIN_LAZY_RANK");
  s.plain_tiles = unless_zero("PFP_PLAIN_TILES");
  s.dict_fold = unless_zero("PFP_DICT_FOLD");
  s.drop_short = unless_zero("PFP_DROP_SHORT");
  s.ipivot_batch = unless_zero("PFP_IPIVOT_BATCH");
  s.parse_keybits = unless_zero("PFP_PARSE_KEYBITS");
  return s;
}

// First-round keys.  The bytes that occur in the dictionary get an order-preserving prefix-free
// (alphabetic) code whose lengths follow their frequencies - A,C,G,T of a FASTA text cost 2-3 bits,
// header characters and other rare bytes a dozen - and the codes of the first characters of every
// suffix are concatenated into kbits (<= 63) bits, cut off where the bits run out; the last bit
// of the key tells whether the suffix's terminator lies inside.  Concatenated alphabetic codes
// compare like the strings they encode, so the first device-wide sort orders the suffixes by a
// prefix of 20-odd characters for DNA text with any number of rare symbols mixed in (a fixed
// width code gave 16 characters for <= 14 distinct bytes and 12 beyond that), and no suffix is
// covered by fewer than hmin = kbits / (longest code) characters.
// lut[b] = (code << 6) | length.
struct KeyCode {
  uint32_t lut[256];
  int kbits, hmin, maxlen;
};

__global__ __launch_bounds__(256) void byte_histogram_kernel(const uint8_t *__restrict__ s, uint64_t N,
                                                             unsigned long long *__restrict__ hist /*[256]*/) {
  __shared__ uint32_t h[4][256];
  for (int q = threadIdx.x; q < 1024; q += 256) (&h[0][0])[q] = 0;
  __syncthreads();
  uint32_t *mine = h[threadIdx.x >> 6];
  for (uint64_t i = ((uint64_t)BID * 256 + threadIdx.x) * 16; i < N; i += (uint64_t)GDIM * 256 * 16) {
    uint4 v = *reinterpret_cast<const uint4 *>(s + i);     // buffer is zero padded past N
    uint32_t w4[4] = {v.x, v.y, v.z, v.w};
    const int nb = (N - i) >= 16 ? 16 : (int)(N - i);
#pragma unroll
    for (int q = 0; q < 16; q++)
      if (q < nb) atomicAdd(&mine[(w4[q >> 2] >> (8 * (q & 3))) & 0xff], 1u);
  }
  __syncthreads();
  const uint32_t t = h[0][threadIdx.x] + h[1][threadIdx.x] + h[2][threadIdx.x] + h[3][threadIdx.x];
  if (t) atomicAdd(&hist[threadIdx.x], (unsigned long long)t);
}

// Alphabetic code by recursive weight-balanced splitting of the symbols in byte order (every split
// point minimises |left weight - right weight|): within 2 bits of the entropy bound, always a
// complete prefix-free order-preserving code.  Rare symbols are floored at 1/4096 of the total so
// that no code grows beyond ~14 bits.
static void balanced_code(const std::vector<uint64_t> &w, int lo, int hi, uint32_t code, int len, std::vector<uint32_t> &codes,
                          std::vector<int> &lens) {
  if (hi - lo == 1) { codes[lo] = code; lens[lo] = len; return; }
  uint64_t tot = 0;
  for (int k = lo; k < hi; k++) tot += w[k];
  uint64_t acc = 0, best = ~0ull;
  int cut = lo + 1;
  for (int k = lo; k + 1 < hi; k++) {
    acc += w[k];
    const uint64_t l = acc, r = tot - acc, diff = l > r ? l - r : r - l;
    if (diff < best) { best = diff; cut = k + 1; }
  }
  balanced_code(w, lo, cut, code << 1, len + 1, codes, lens);
  balanced_code(w, cut, hi, (code << 1) | 1u, len + 1, codes, lens);
}
static KeyCode make_key_code(const uint64_t hist[256], double rep_hint, const SorterSwitches &sw) {
  KeyCode kc{};
  std::vector<int> sym;
  for (int b2 = 0; b2 < 256; b2++) if (hist[b2] || b2 <= 1) sym.push_back(b2);       // 0x00 / 0x01 always coded
  uint64_t total = 0;
  for (int b2 : sym) total += hist[b2];
  const uint64_t floor_w = total / 4096 + 1;
  std::vector<uint64_t> w(sym.size());
  for (size_t k = 0; k < sym.size(); k++) w[k] = std::max<uint64_t>(hist[sym[k]], floor_w);
  std::vector<uint32_t> codes(sym.size());
  std::vector<int> lens(sym.size());
  if (sym.size() == 1) { codes[0] = 0; lens[0] = 1; }
  else balanced_code(w, 0, (int)sym.size(), 0u, 0, codes, lens);
  int maxlen = 1;
  for (int l : lens) maxlen = std::max(maxlen, l);
  if (maxlen > 24) {        // cannot happen with the weight floor; fixed width keeps the table format valid regardless
    const int bits = bits_for((uint64_t)sym.size() - 1);
    for (size_t k = 0; k < sym.size(); k++) { codes[k] = (uint32_t)k; lens[k] = bits; }
    maxlen = bits;
  }
  for (size_t k = 0; k < sym.size(); k++) kc.lut[sym[k]] = (codes[k] << 6) | (uint32_t)lens[k];
  // bytes that do not occur still need a valid entry (reads past the terminator are masked, not skipped)
  for (int b2 = 0; b2 < 256; b2++) if (!kc.lut[b2]) kc.lut[b2] = (uint32_t)maxlen;
  // Key width: every 8 bits less is one radix pass less over all N suffixes.  A key of kbits code bits
  // distinguishes about 2^(kbits * H / L) strings (H = order-0 entropy of the bytes, L = mean code
  // length); 2^8 times more than there are suffixes leaves well under 1 % of them tied by chance, and
  // the ties that remain - true repeats - are what the later rounds are for.  (253 MB FASTA: 47 bits,
  // 6 passes instead of 8, 2 M of 260 M suffixes tied after the first round: 48.3 -> 45.0 ms.)
  double H = 0, Lm = 0;
  for (size_t k = 0; k < sym.size(); k++) {
    if (!hist[sym[k]]) continue;
    const double pr = (double)hist[sym[k]] / (double)total;
    H -= pr * std::log2(pr); Lm += pr * lens[k];
  }
  // (a repetitive collection's dictionary holds about total / rep distinct contexts: the rest are family members no key width separates)
  const double need = std::log2(std::max((double)total / std::max(rep_hint, 1.0), 2.0)) + 6.0;
  kc.kbits = 63;
  for (int kb : {39, 47, 55}) if (Lm > 0 && kb * H / Lm >= need) { kc.kbits = kb; break; }
  if (sw.keybits) kc.kbits = sw.keybits;
  kc.hmin = std::max(1, std::min(32, kc.kbits / maxlen));
  kc.maxlen = maxlen;
  return kc;
}

// key of the suffix at i: codes of its first characters, most significant first, in kbits bits; then
// one bit "the terminator's code is inside".  `lut` may live in LDS (bulk kernel) or global memory.
__device__ __forceinline__ uint64_t packed_key_at(const uint8_t *__restrict__ s, uint64_t i, int kbits, const uint32_t *lut) {
  uint4 a = ld16u(s + i), b = ld16u(s + i + 16);
  const uint32_t w8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint64_t k = 0;
  int pos = kbits;
  uint32_t term = 0;
#pragma unroll
  for (int j = 0; j < 32; j++) {
    if ((j == 16 || j == 20 || j == 24 || j == 28) && !__any(pos > 0)) break;     // every active lane has filled its key
    if (pos > 0) {
      const uint32_t c = (w8[j >> 2] >> (8 * (j & 3))) & 0xff;
      const uint32_t e = lut[c];
      const int l = (int)(e & 63u);
      const uint64_t cd = e >> 6;
      if (pos >= l) {
        pos -= l;
        k |= cd << pos;
        if (c <= kEndOfWord) { term = 1; pos = 0; }
      } else {
        k |= cd >> (l - pos);
        pos = 0;
      }
    }
  }
  return (k << 1) | term;
}

// Rank of the suffix at j.  rank[j] holds it when some round after the first refined j's group;
// otherwise the first round settled j and its rank is the first slot holding j's packed key: the
// bucket table narrows the range to the slots that share the key's top bits, a binary search
// over the sorted keys finishes (a handful of sectors instead of one scattered write per suffix).
//
// `settled` (dictionary mode, finbit != 0): j's group will never be refined again - it is a
// singleton or a set of identical strings.  An unresolved tie whose continuations are settled is
// itself a set of identical strings (their sorted prefixes reach the terminator), which is how
// write_back retires groups without gathering the suffix length of every member every round.
template <class I>
__device__ __forceinline__ I rank_at(const RankViewT<I> &L, uint64_t j, bool &settled) {
  const I r = L.rank ? L.rank[j] : IdxTraits<I>::kNone;
  if (L.skeys == nullptr || r != IdxTraits<I>::kNone) { settled = (r & L.finbit) != 0; return r & ~L.finbit; }
  settled = true;
  const uint64_t k = packed_key_at(L.bytes, j, L.kbits, L.lut);
  const uint32_t b = (uint32_t)(k >> L.shift);
  I lo = IdxTraits<I>::kNone - L.tab[L.T - 1 - b];
  I hi = (b + 1 < L.T) ? IdxTraits<I>::kNone - L.tab[L.T - 2 - b] : (I)L.N;
  while (lo < hi) {
    const I mid = lo + ((hi - lo) >> 1);
    if ((L.skeys[mid] & L.keymask) < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// merge record of position i: low byte = preceding char (1 = whole word, pfbwt.cpp:153; 0 = emits
// nothing, <= w long, pfbwt.cpp:151), high byte = occurrences of its word, 255 = "255 or more"
__device__ __forceinline__ uint32_t slot_record(const uint8_t *__restrict__ b, uint64_t i, uint32_t wd, const SlotPayloadSrc &P) {
  if (!(wd < P.wv.d && P.wv.wend[wd] - i > (uint64_t)P.w)) return 0u;
  const uint32_t pc = (i == 0) ? kEndOfWord : b[i - 1];
  const uint32_t occ = P.wocc[wd];
  return pc | ((occ < 255u ? occ : 255u) << 8);
}
// The same keys for ALL positions, without walking 20-odd characters per suffix: a workgroup lays the
// codes of 256 consecutive characters down as one bit stream in LDS (bit offset = prefix sum of the code
// lengths), and the key of position t is the kbits bits that start at t's offset, cut at its word's
// terminator (endpos) and at 32 characters - exactly what packed_key_at assembles character by
// character (checked against it under PFP_DEBUG).  224 positions per workgroup, 32 characters of overlap.
constexpr int kKeyPos = 224;
struct KeyStreamLds { uint32_t off[257]; uint32_t bs[200]; uint32_t wsum[4]; unsigned long long tmask[4]; uint32_t wbase; };
// workgroup-cooperative: returns the key (code bits << 1 | terminator flag) of position B0 + threadIdx.x
// for threadIdx.x < kKeyPos and position < N; every thread of the workgroup must call it
// Where a position's word ends is read off the block's own characters (the first byte <= 1 at or after it, looked for
// over the 32 characters a key can cover): no per-position length array is read.
// word_out (optional, needs wv): the word of position B0 + threadIdx.x - the word of the block's first position (one count
// per block, see below) plus the terminators the ballots count before the lane.
// toterm_out (optional; written for the positions that get a key): characters up to and including the terminator, 33 = more than 32.
__device__ __forceinline__ uint64_t block_stream_key(KeyStreamLds &L, const uint8_t *__restrict__ s, uint64_t N,
                                                     const KeyCode &kp, uint64_t B0, const WordView *view = nullptr,
                                                     uint32_t *word_out = nullptr, uint32_t *toterm_out = nullptr) {
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint64_t pos = B0 + t;
  if (t < 200) L.bs[t] = 0;
  const uint32_t c = pos < N ? s[pos] : 0u;
  const uint32_t e = kp.lut[c];
  const uint32_t l = e & 63u, cd = e >> 6;
  uint32_t inc = l;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
  if (lane == 63) L.wsum[wv] = inc;
  const unsigned long long tmine = __ballot(c <= (uint32_t)kEndOfWord);      // terminators (0x01) and the final 0x00 / the padding behind it
  if (lane == 0) L.tmask[wv] = tmine;
  // (the word of B0 from the 64-byte line boundary that lies inside the tile: the count there minus the 0x01 bytes the
  //  first wave sees before it - one load that waits for nothing, where word_of(B0) is a count and then a line of bytes)
  if (word_out) {
    const unsigned long long t1 = __ballot(c == (uint32_t)kEndOfWord);
    if (t == 0) {
      const uint64_t line = (B0 >> 6) + 1;
      const uint32_t upto = (uint32_t)(line * 64 - B0);      // 1 .. 64 positions of the tile before that boundary
      L.wbase = B0 < N ? view->blk_word[line] - (uint32_t)__popcll(upto >= 64 ? t1 : (t1 & ((1ull << upto) - 1ull))) : 0u;
    }
  }
  __syncthreads();
  if (word_out) {
    uint32_t before = (uint32_t)__popcll(tmine & ((1ull << lane) - 1ull));
    for (int q = 0; q < wv; q++) before += (uint32_t)__popcll(L.tmask[q]);
    *word_out = L.wbase + before;
  }
  uint32_t base = 0;
  for (int q = 0; q < wv; q++) base += L.wsum[q];
  const uint32_t p = base + inc - l;            // bit offset of this character's code
  L.off[t] = p;
  if (t == 255) L.off[256] = p + l;
  {
    const uint32_t w = p >> 5, o = p & 31u;
    if (o + l <= 32) atomicOr(&L.bs[w], cd << (32 - o - l));
    else {
      const uint32_t r = o + l - 32;            // bits that spill into the next word
      atomicOr(&L.bs[w], cd >> r);
      atomicOr(&L.bs[w + 1], (cd & ((1u << r) - 1u)) << (32 - r));
    }
  }
  __syncthreads();
  if (t >= kKeyPos || pos >= N) return 0;
  // characters up to and including the terminator of this position's word (33 = "more than a key can cover")
  uint32_t toterm = 33u;
  {
    const unsigned long long m0 = tmine >> lane;
    if (m0) toterm = (uint32_t)__builtin_ctzll(m0) + 1u;
    else if (wv < 3) { const unsigned long long m1 = L.tmask[wv + 1]; if (m1) toterm = (uint32_t)(64 - lane) + (uint32_t)__builtin_ctzll(m1) + 1u; }
    if (toterm > 33u) toterm = 33u;
  }
  if (toterm_out) *toterm_out = toterm;
  const uint32_t nch = toterm < 32u ? toterm : 32u;
  const uint32_t avail = L.off[t + nch] - p;
  const uint32_t kb = (uint32_t)kp.kbits;
  const uint32_t take = avail < kb ? avail : kb;
  const uint32_t w = p >> 5, sh = p & 31u;
  const uint64_t hi = ((uint64_t)L.bs[w] << 32) | L.bs[w + 1];
  uint64_t x = hi << sh;
  if (sh) x |= (uint64_t)(L.bs[w + 2] >> (32 - sh));
  uint64_t k = x >> (64 - kb);
  if (take < kb) k &= ~((1ull << (kb - take)) - 1ull);
  const uint32_t term = (toterm <= 32u && L.off[t + toterm] - p <= kb) ? 1u : 0u;
  return (k << 1) | term;
}
// Suffixes that emit nothing in the merge: at most min_len bytes long (terminator not counted), and the final 0x00.  The
// first round can leave them out (sort_dict_suffixes with a minimum length).  Where every word is longer than min_len
// (short_words_kernel looks for others) each word has exactly min_len + 1 such positions, its last ones, so the kept
// position i of word j is the (i - (min_len + 1) j)-th kept position: init_keys_packed_kernel writes its key there - no
// count, no scan, no list of positions.  The word comes from the tile's ballots (block_stream_key's word_out), and so
// does the distance to the terminator while min_len + 1 characters fit into the 32 a tile looks ahead.
__device__ __forceinline__ bool suffix_kept(const WordView &v, uint32_t wd, uint64_t pos, int min_len) {
  return wd < v.d && v.wend[wd] - pos > (uint64_t)min_len;
}
// *found = 1 if some word has at most min_len bytes (found: a pinned host scalar the host cleared - no device buffer, no copy)
__global__ void short_words_kernel(WordView view, int min_len, unsigned long long *__restrict__ found) {
  const uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j >= view.d) return;
  const uint64_t start = j ? view.wend[j - 1] + 1 : 0;
  if (view.wend[j] - start <= (uint64_t)min_len) *found = 1ull;
}
// listed == 0: the key of every position, at the position's index.  Else (view, min_len): the keys of the `listed` kept
// positions, each at its index among the kept ones.
template <class I>
__global__ __launch_bounds__(256) void init_keys_packed_kernel(const uint8_t *__restrict__ s, uint64_t N, KeyCode kp,
                                                               SlotPayloadSrc P, int paybits, uint64_t *__restrict__ key,
                                                               I *__restrict__ val, int idx_bits, WordView view, int min_len,
                                                               uint64_t listed /* keys of the list, 0 = every position */) {
  __shared__ KeyStreamLds L;
  const uint64_t B0 = (uint64_t)BID * kKeyPos;
  uint32_t wd = 0, toterm = 0;
  uint64_t k = (paybits || listed) ? block_stream_key(L, s, N, kp, B0, &view, &wd, &toterm) : block_stream_key(L, s, N, kp, B0);
  const uint64_t pos = B0 + threadIdx.x;
  if (threadIdx.x >= kKeyPos || pos >= N) return;
  uint64_t at = pos;
  if (listed) {
    // (toterm - 1 = bytes before the terminator, exact up to 31; the final 0x00 ends at once)
    const bool keep = min_len < 32 ? toterm > (uint32_t)min_len + 1u : suffix_kept(view, wd, pos, min_len);
    if (!keep) return;
    at = pos - ((uint64_t)min_len + 1) * wd;
    // (never true: the host lists only a dictionary whose bytes below 2 are its d terminators and the final 0x00, and whose
    //  words are all longer than min_len - then the kept positions fill [0, listed) exactly.  Kept as the store's own bound)
    if (at >= listed) return;
  }
  if (idx_bits) { key[at] = (k << idx_bits) | pos; return; }      // keys-only sort: the position rides in the low bits
  if (paybits) k |= (uint64_t)slot_record(s, pos, wd, P) << 48;
  key[at] = k; val[at] = (I)pos;
}
// sorted (key << idx_bits | position) words -> the sorted keys and the sorted positions
template <class I>
__global__ void split_keys_kernel(const uint64_t *__restrict__ comb, uint64_t n, int idx_bits, uint64_t *__restrict__ key,
                                  I *__restrict__ val) {
  const uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= n) return;
  const uint64_t x = comb[a];
  key[a] = x >> idx_bits;
  val[a] = (I)(x & ((1ull << idx_bits) - 1ull));
}
// PFP_DEBUG: the bit-stream keys against the character-by-character ones
// (listed: the keys of the kept positions only, in position order - suffix_kept is asked again about every position named and
//  about the gap between neighbours, so a position dropped or kept wrongly counts as bad too)
template <class I>
__global__ void check_keys_kernel(const uint8_t *__restrict__ s, uint64_t n, KeyCode kp, const uint64_t *__restrict__ key,
                                  const I *__restrict__ val, uint64_t keymask, unsigned long long *__restrict__ bad, int idx_bits,
                                  int listed, WordView view, int min_len) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= n) return;
  uint64_t i = a;
  if (listed) {
    auto pos_at = [&](uint64_t q) { return idx_bits ? (key[q] & ((1ull << idx_bits) - 1ull)) : (uint64_t)val[q]; };
    i = pos_at(a);
    const uint64_t from = a ? pos_at(a - 1) + 1 : 0;
    bool ok = i < view.NP && from <= i && suffix_kept(view, word_of(view, i), i, min_len);
    for (uint64_t j = from; ok && j < i; j++) ok = !suffix_kept(view, word_of(view, j), j, min_len);
    if (ok && a + 1 == n) for (uint64_t j = i + 1; ok && j < view.NP; j++) ok = !suffix_kept(view, word_of(view, j), j, min_len);
    if (!ok) { atomicAdd(bad, 1ull); return; }
  }
  if (((key[a] >> idx_bits) & keymask) != packed_key_at(s, i, kp.kbits, kp.lut)) atomicAdd(bad, 1ull);
}
template <class I>
__global__ void init_keys_bytes_kernel(const uint8_t *__restrict__ s, uint64_t N, uint64_t *__restrict__ key,
                                       I *__restrict__ val) {
  uint64_t i = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (i >= N) return;
  key[i] = __builtin_bswap64(ld8u(s + i));         // buffer is zero padded past N
  val[i] = (I)i;
}
__global__ void init_keys_int_kernel(const uint32_t *__restrict__ s, uint64_t N, uint64_t *__restrict__ key,
                                     uint32_t *__restrict__ val) {
  uint64_t i = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (i >= N) return;
  uint64_t a = s[i], b = (i + 1 < N) ? s[i + 1] : 0;
  key[i] = (a << 32) | b; val[i] = (uint32_t)i;
}
// Integer strings (the parse): the first-round key holds two symbols and, where they are equal, how the
// run of that symbol ends.  Suffixes inside a run x^r y order by (y < x: shorter run first | y > x:
// longer run first), which plain doubling needs log2(r) rounds to find out - a parse of a text with
// a long N run holds a run of 300 k equal phrases (18 rounds; with the run key 8).
// out[0] = the largest symbol; out[1] != 0 where two neighbours are equal (s[i] == s[i+1], i + 1 < N): one pass answers both
__global__ __launch_bounds__(256) void max_u32_kernel(const uint32_t *__restrict__ s, uint64_t N, uint32_t *__restrict__ out) {
  uint32_t m = 0;
  bool pair = false;
  for (uint64_t i = (uint64_t)BID * 256 + threadIdx.x; i < N; i += (uint64_t)GDIM * 256) {
    const uint32_t x = s[i];
    m = x > m ? x : m;
    if (i + 1 < N && s[i + 1] == x) pair = true;
  }
  for (int o = 32; o > 0; o >>= 1) { const uint32_t v = __shfl_down(m, o, 64); m = v > m ? v : m; }
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
  if (__any(pair) && (threadIdx.x & 63) == 0) atomicOr(out + 1, 1u);
}
__global__ void run_marks_kernel(const uint32_t *__restrict__ s, uint32_t N, uint32_t *__restrict__ v) {
  uint32_t j = BID * blockDim.x + threadIdx.x;      // reversed index
  if (j >= N) return;
  const uint32_t i = N - 1 - j;
  v[j] = (i == N - 1 || s[i] != s[i + 1]) ? j : 0u;
}
__global__ void init_keys_int_run_kernel(const uint32_t *__restrict__ s, uint32_t N, const uint32_t *__restrict__ pm, int sb,
                                         uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
  uint32_t i = BID * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const uint64_t a = s[i], b = (i + 1 < N) ? s[i + 1] : 0;
  val[i] = i;
  // pm null: the string has no two equal neighbours, e would be 0 everywhere: the two symbols alone, right-aligned.  That is
  // the run key shifted right by 64 - 2 sb: order and equality of the keys are the same, the stable sort leaves ties in position
  // order either way, so the sorted permutation is the same - from a sort of 2 sb bits instead of 64
  if (!pm) { key[i] = (a << sb) | b; return; }
  const int eb = 64 - 2 * sb;
  uint64_t e = 0;
  if (b == a && i + 1 < N) {
    const uint32_t re = N - 1 - pm[N - 1 - i];              // last position of the run that holds i
    const uint64_t cap = (1ull << (eb - 1)) - 1;
    uint64_t r = (uint64_t)re - i + 1;
    if (r > cap) r = cap;
    const bool up = re + 1 < N && s[re + 1] > a;            // the run is followed by a larger symbol
    e = up ? ((1ull << (eb - 1)) | (cap - r)) : r;
  }
  key[i] = (a << (64 - sb)) | (b << (64 - 2 * sb)) | e;
}
template <class I>
__global__ void iota_kernel(I *p, uint64_t n) {
  uint64_t i = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (i < n) p[i] = (I)i;
}

// key of an unresolved suffix: (its group's head slot, 1 + rank of the suffix h further on).
// The suffix position and its group travel with the active list (active_place_kernel), so the only
// random access is rank[i+h].  In dictionary mode an unresolved suffix is always longer than the
// sorted prefix h (otherwise write_back would have retired it), so i+h stays inside its word.
template <class I>
__global__ void build_keys_kernel(SufGeom g, uint64_t m, uint64_t h, const I *__restrict__ act_i,
                                  const I *__restrict__ act_grp, RankViewT<I> L, int nb,
                                  typename IdxTraits<I>::DKey *__restrict__ key, I *__restrict__ val) {
  using K = typename IdxTraits<I>::DKey;
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const I i = act_i[a];
  const K grp = act_grp[a];
  bool settled = false;
  const uint64_t nxt = (g.mode == MODE_DICT || (uint64_t)i + h < g.N) ? (uint64_t)rank_at(L, (uint64_t)i + h, settled) + 1 : 0;
  key[a] = (grp << nb) | (K)nxt;
  val[a] = i | (settled ? L.finbit : (I)0);
}

// segmented variant of a doubling round: the unresolved suffixes are already grouped (the active
// list is in slot order), so only the 32-bit "next" key has to be sorted, inside every group
template <class I>
__global__ void group_starts_kernel(uint64_t m, const I *__restrict__ act_grp, uint8_t *__restrict__ gs) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a < m) gs[a] = (a == 0 || act_grp[a] != act_grp[a - 1]) ? 1 : 0;
}
__global__ void build_keys32_kernel(SufGeom g, uint64_t m, uint64_t h, const uint32_t *__restrict__ act_i,
                                    RankViewT<uint32_t> L, uint32_t *__restrict__ key, uint32_t *__restrict__ val) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const uint32_t i = act_i[a];
  bool settled = false;
  key[a] = (g.mode == MODE_DICT || (uint64_t)i + h < g.N) ? rank_at(L, (uint64_t)i + h, settled) + 1u : 0u;
  val[a] = i | (settled ? L.finbit : 0u);
}
// Small segments.  The unresolved suffixes of a dictionary of variants come in families of a handful of members
// (a phrase and the variants that agree with it over the first-round prefix): a device-wide radix sort of
// (group, order key) moves every element 7 times to reorder it inside a group of six.  Here every element
// finds its place directly: the group ids and keys of 256 list positions plus kSmallSeg on either side are
// staged in LDS, an element walks back to the start of its group and forward over its members, counting the
// keys that sort before its own (stable: equal keys keep their list order).  A group longer than kSmallSeg does
// not fit the window: the kernel then only raises *overflow and the caller sorts that round with the library.
// Also writes the group-start flags gs[] the head detection of the round reads.
// (Tried in round 3: the same kernel with a 2048-member window and 1024 positions per workgroup for the families of a
//  1000-copy collection, in place of the library's segmented sort.  Bit-exact, and 5x slower: 12.6 GB 58 -> 308 ms for these
//  sorts.  Counting is quadratic in the group size and the count loop is a chain of dependent LDS reads with four waves per
//  SIMD to hide them.  A real sort of whole groups in LDS - block radix, bitonic - was tried too: no faster than the library's
//  0.024 ns per element and round)
constexpr uint32_t kSmallSeg = 64;
template <class I, class KT>
__global__ __launch_bounds__(256) void seg_small_sort_kernel(uint64_t m, const I *__restrict__ act_grp,
                                                             const KT *__restrict__ key, const I *__restrict__ val,
                                                             uint8_t *__restrict__ gs, KT *__restrict__ keyo,
                                                             I *__restrict__ valo, uint32_t *__restrict__ overflow,
                                                             uint8_t *__restrict__ big) {
  constexpr int K = (int)kSmallSeg, W = 256 + 2 * K;
  __shared__ KT lkey[W];
  __shared__ I lgrp[W];
  const uint64_t B = (uint64_t)BID * 256;
  for (int idx = threadIdx.x; idx < W; idx += 256) {
    const uint64_t j = B + idx;                   // list position + K
    const bool ok = j >= (uint64_t)K && j - K < m;
    lkey[idx] = ok ? key[j - K] : (KT)0;
    lgrp[idx] = ok ? act_grp[j - K] : IdxTraits<I>::kNone;      // outside the list: no group
  }
  __syncthreads();
  const uint64_t a = B + threadIdx.x;
  if (a >= m) return;
  const int la = (int)threadIdx.x + K;
  const I g = lgrp[la];
  gs[a] = lgrp[la - 1] != g ? 1 : 0;
  // a group of more than K members: with `big` its elements are passed through in place and flagged (the caller
  // sorts just those), without it the round is the library's.  Groups are contiguous, so two probes tell: the
  // position K back, and - once the start is known - the position K past it.
  const KT ka = lkey[la];
  bool too_long = lgrp[la - K] == g;      // the group starts K or more positions back
  int ls = la;
  if (!too_long) {
    while (lgrp[ls - 1] == g) ls--;       // (stops within K - 1 steps)
    too_long = ls + K < W && lgrp[ls + K] == g;      // more than K members
  }
  if (too_long) {
    atomicOr(overflow, 1u);
    if (big) { big[a] = 1; keyo[a] = ka; valo[a] = val[a]; }
    return;
  }
  uint32_t r = 0;
  for (int j = ls; j < ls + K && lgrp[j] == g; j++) {
    const KT kj = lkey[j];
    r += (kj < ka || (kj == ka && j < la)) ? 1u : 0u;
  }
  if (big) big[a] = 0;
  const uint64_t s0 = a - (uint64_t)(la - ls);
  keyo[s0 + r] = ka;
  valo[s0 + r] = val[a];
}
// the elements of the groups seg_small_sort_kernel passed through: (group, key) words for one sort of just those,
// and the way back - the sorted side list has the groups in list order, so its j-th element belongs at idx[j]
template <class I>
__global__ void big_seg_gather_kernel(uint64_t nb, const I *__restrict__ idx, const I *__restrict__ act_grp, const uint32_t *__restrict__ keyo,
                                      const I *__restrict__ valo, uint64_t *__restrict__ k64, I *__restrict__ v) {
  const uint64_t j = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (j >= nb) return;
  const I a = idx[j];
  k64[j] = ((uint64_t)act_grp[a] << 32) | keyo[a];
  v[j] = valo[a];
}
template <class I>
__global__ void big_seg_scatter_kernel(uint64_t nb, const I *__restrict__ idx, const uint64_t *__restrict__ k64, const I *__restrict__ v,
                                       uint32_t *__restrict__ keyo, I *__restrict__ valo) {
  const uint64_t j = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (j >= nb) return;
  const I a = idx[j];
  keyo[a] = (uint32_t)k64[j];
  valo[a] = v[j];
}
__global__ void seg_end_kernel(uint32_t ng, uint32_t m, const uint32_t *__restrict__ seg_begin, uint32_t *__restrict__ seg_end,
                               uint32_t *__restrict__ maxlen) {
  uint32_t k = BID * blockDim.x + threadIdx.x;
  uint32_t len = 0;
  if (k < ng) { uint32_t e = (k + 1 < ng) ? seg_begin[k + 1] : m; seg_end[k] = e; len = e - seg_begin[k]; }
  for (int o = 32; o > 0; o >>= 1) { uint32_t v = __shfl_down(len, o, 64); len = v > len ? v : len; }
  if ((threadIdx.x & 63) == 0 && len) atomicMax(maxlen, len);
}
template <class I>
__global__ void heads32_kernel(uint64_t m, const uint8_t *__restrict__ gs, const uint32_t *__restrict__ key,
                               const I *__restrict__ aslot, uint8_t *__restrict__ hd, I *__restrict__ hv) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  bool h = gs[a] || key[a] != key[a - 1];
  hd[a] = h ? 1 : 0;
  hv[a] = h ? aslot[a] : (I)0;
}

// ---- pivot rounds for the suffixes of the PARSE of a collection of near-identical sequences.
// After the first round a group is one place of the genome in all its copies; two members agree until one of them meets a phrase
// that only its own copy has (a variant word: a rare symbol).  Comparing every member with the group's FIRST member only halves
// the group per round - that pivot has a variant of its own a few phrases on, and everybody who agrees with the consensus up to
// there ties at that position (round 2 tried it: 13 rounds instead of doubling's 8).  The frequencies of the symbols tell which
// member to compare with: the one whose next rare symbol is FARTHEST (dist[], one backward scan over the parse).  Every other
// member then leaves the pivot at its own variant - a different (offset, symbol) for each - and one round places 99 % of a
// group where doubling needs log2(offset) rounds (64 copies: 160 K unresolved -> 1.1 K after one round; first-member pivot: 81 K).
// Order key, as for the dictionary's pivot rounds: smaller than the pivot: ascending offset, then symbol; the pivot's class; greater:
// descending offset, then symbol - two 32-bit halves of a 64-bit key sorted inside every group.
constexpr uint32_t kIntPivCap = 1024;      // symbols compared per member and round
// 16-byte load steps a member issues together in the pivot round's key kernel.  (Measured on configs[2], 15.2 M members: 4 steps
// 0.69 ms at 54 VGPRs, 8 steps 0.80 ms at 86 VGPRs and five waves per SIMD, the one-step loop 0.85 ms)
// PFP_IPIVOT_BATCH=0 takes the one-step loop.
constexpr int kIntPivBatch = 4;
template <class I>
__global__ void ipivot_select_kernel(uint64_t m, uint64_t N, uint64_t h, const I *__restrict__ act_i, const I *__restrict__ act_grp,
                                     const uint32_t *__restrict__ dist, unsigned long long *__restrict__ best,
                                     uint32_t *__restrict__ dvs) {
  const uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  unsigned long long v = 0;
  uint64_t g = ~0ull;
  if (a < m) {
    const uint64_t i = act_i[a];
    g = act_grp[a];
    const uint32_t dv = i + h < N ? dist[i + h] : 0u;
    if (dvs) dvs[a] = dv;      // (coalesced; ipivot_keys_batch_kernel sizes its loads by it instead of gathering dist[] again)
    v = ((unsigned long long)dv << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)a);      // ties: the first member
  }
  // the members of a group are neighbours: maximum over the run of equal groups that ends at this lane, one atomic per run and wave
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(v, o, 64);
    const uint64_t ug = __shfl_up(g, o, 64);
    if (lane >= o && ug == g && u > v) v = u;
  }
  const uint64_t gn = __shfl_down(g, 1, 64);
  if (a < m && (lane == 63 || gn != g)) atomicMax(&best[g], v);
}
template <class I>
__global__ void ipivot_keys_kernel(uint64_t m, uint64_t N, uint64_t h, uint32_t cap, const uint32_t *__restrict__ sym,
                                   const I *__restrict__ act_i, const I *__restrict__ act_grp,
                                   const unsigned long long *__restrict__ best, uint64_t *__restrict__ key, I *__restrict__ val) {
  const uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const uint64_t i = act_i[a];
  const uint64_t piv = act_i[0xFFFFFFFFu - (uint32_t)(best[act_grp[a]] & 0xFFFFFFFFull)];
  uint64_t k = (uint64_t)(cap + 1) << 32;      // the pivot itself, and whoever equals it for cap symbols
  if (i != piv) {
    // four symbols a step (two unaligned 16-byte loads; round 4: one symbol a step was a chain of ~20 dependent 4-byte loads per
    // member - 52 ms of the 12.6 GB chain once the phrases got shorter); the last steps before the end of the string one by one
    bool done = false;
    for (uint32_t q = 0; q < cap && !done; q += 4) {
      const uint64_t pi = i + h + q, pp = piv + h + q;
      uint32_t x[4], y[4];
      if (pi + 4 <= N && pp + 4 <= N) {
        const uint4 X = ld16u(reinterpret_cast<const uint8_t *>(sym + pi)), Y = ld16u(reinterpret_cast<const uint8_t *>(sym + pp));
        if (X.x == Y.x && X.y == Y.y && X.z == Y.z && X.w == Y.w) continue;
        x[0] = X.x; x[1] = X.y; x[2] = X.z; x[3] = X.w; y[0] = Y.x; y[1] = Y.y; y[2] = Y.z; y[3] = Y.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) { x[j] = pi + j < N ? sym[pi + j] : 0u; y[j] = pp + j < N ? sym[pp + j] : 0u; }
      }
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (!done && q + j < cap && x[j] != y[j]) {
          const uint32_t qq = q + (uint32_t)j;
          k = ((uint64_t)(x[j] < y[j] ? qq : 2 * cap + 2 - qq) << 32) | x[j];
          done = true;
        }
    }
  }
  key[a] = k;
  val[a] = (I)i;
}
// The same key from loads that are issued together.  The loop above is a chain: every step's two loads wait for the compare of the
// step before, and a wave waits for its longest lane.  But a member leaves the pivot at its own variant, dvs[a] symbols on
// (ipivot_select_kernel has just read that distance), so the likely length of its walk is known before the first symbol is loaded:
// the lane issues the load pairs of the ceil(need / 4) steps that reach its variant, at most B of them, before the first compare,
// then compares in order.  The loads are predicated per lane: none reads past its own need, its batch or the end of the string.
// A lane still equal after its batch (a distance of more than 4 B symbols; beyond its own variant: the rest of cap) takes the next
// one.  Steps that would cross the end of the string go one by one, as above; the key is bit for bit the one of the loop above.
template <class I, int B>
__global__ __launch_bounds__(256) void ipivot_keys_batch_kernel(uint64_t m, uint64_t N, uint64_t h, uint32_t cap,
                                                                const uint32_t *__restrict__ sym, const I *__restrict__ act_i,
                                                                const I *__restrict__ act_grp, const unsigned long long *__restrict__ best,
                                                                const uint32_t *__restrict__ dvs, uint64_t *__restrict__ key,
                                                                I *__restrict__ val) {
  const uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const uint64_t i = act_i[a];
  const uint64_t piv = act_i[0xFFFFFFFFu - (uint32_t)(best[act_grp[a]] & 0xFFFFFFFFull)];
  uint64_t k = (uint64_t)(cap + 1) << 32;      // the pivot itself, and whoever equals it for cap symbols
  if (i != piv) {
    const uint32_t dv = dvs[a];
    const uint32_t need = dv < cap ? dv + 1 : cap;      // symbols up to and including the member's own variant
    bool done = false;
    uint32_t q = 0;
    auto differ = [&](uint32_t qq, uint32_t x, uint32_t y) {
      if (!done && qq < cap && x != y) {
        k = ((uint64_t)(x < y ? qq : 2 * cap + 2 - qq) << 32) | x;
        done = true;
      }
    };
    while (q < cap && !done) {
      const uint64_t pi = i + h + q, pp = piv + h + q;
      const uint64_t far = pi > pp ? pi : pp;
      const uint64_t room = far + 4 <= N ? (N - far) / 4 : 0;      // whole 16-byte steps that both strings still hold
      if (room == 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) differ(q + (uint32_t)j, pi + j < N ? sym[pi + j] : 0u, pp + j < N ? sym[pp + j] : 0u);
        q += 4;
        continue;
      }
      const uint32_t want = need > q ? need - q : cap - q;
      uint32_t steps = (want + 3) / 4;
      if (steps > (uint32_t)B) steps = B;
      if (steps > room) steps = (uint32_t)room;
      uint4 X[B], Y[B];
#pragma unroll
      for (int s = 0; s < B; s++)
        if ((uint32_t)s < steps) {
          X[s] = ld16u(reinterpret_cast<const uint8_t *>(sym + pi + 4 * s));
          Y[s] = ld16u(reinterpret_cast<const uint8_t *>(sym + pp + 4 * s));
        }
#pragma unroll
      for (int s = 0; s < B; s++)
        if ((uint32_t)s < steps && !done) {
          const uint32_t qs = q + 4 * (uint32_t)s;
          differ(qs, X[s].x, Y[s].x); differ(qs + 1, X[s].y, Y[s].y); differ(qs + 2, X[s].z, Y[s].z); differ(qs + 3, X[s].w, Y[s].w);
        }
      q += 4 * steps;
    }
  }
  key[a] = k;
  val[a] = (I)i;
}
template <class I>
__global__ void heads64seg_kernel(uint64_t m, const uint8_t *__restrict__ gs, const uint64_t *__restrict__ key,
                                  const I *__restrict__ aslot, uint8_t *__restrict__ hd, I *__restrict__ hv) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  bool h = gs[a] || key[a] != key[a - 1];
  hd[a] = h ? 1 : 0;
  hv[a] = h ? aslot[a] : (I)0;
}
// distance to the next rare symbol: marks over the reversed string (0 = common; else reversed index + 1), running maximum, difference
__global__ void rare_marks_kernel(const uint32_t *__restrict__ s, uint32_t N, const uint32_t *__restrict__ occ, uint32_t n_sym,
                                  uint32_t below, uint32_t *__restrict__ v) {
  uint32_t j = BID * blockDim.x + threadIdx.x;      // reversed index
  if (j >= N) return;
  const uint32_t x = s[N - 1 - j];
  const bool rare = x == 0 || x > n_sym || occ[x - 1] < below;
  v[j] = rare ? j + 1 : 0u;
}
__global__ void rare_dist_kernel(uint32_t N, const uint32_t *__restrict__ pm, uint32_t *__restrict__ dist) {
  uint32_t i = BID * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const uint32_t j = N - 1 - i, mk = pm[j];
  dist[i] = mk ? j + 1 - mk : 0xFFFFFFFFu;      // (the unique last symbol is rare: every position has one ahead)
}

// Compaction of the active list: kept suffixes and kept group heads counted per 256 list positions
// from 16-byte loads of the flag bytes, tiny scans over those sums, then one thread per list position
// places its (slot, suffix, group) triple (coalesced reads, consecutive writes).  Replaces an N-long
// inclusive scan into a 4-byte array and its re-read.
constexpr int kTile = 256;
__global__ __launch_bounds__(256) void active_count_kernel(const uint8_t *__restrict__ keep, const uint8_t *__restrict__ hd,
                                                           uint64_t m, uint32_t *__restrict__ tile_keep,
                                                           uint32_t *__restrict__ tile_heads) {
  // thread = 16 flags, 16 threads = one tile of 256
  const uint64_t t = (uint64_t)BID * 256 + threadIdx.x;
  const uint64_t base = t * 16;
  uint32_t k[4] = {0, 0, 0, 0}, h[4] = {0, 0, 0, 0};
  if (base < m) { load_flags16(keep, base, m, k); load_flags16(hd, base, m, h); }
  uint32_t ck = __popc(k[0]) + __popc(k[1]) + __popc(k[2]) + __popc(k[3]);
  uint32_t ch = __popc(k[0] & h[0]) + __popc(k[1] & h[1]) + __popc(k[2] & h[2]) + __popc(k[3] & h[3]);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) { ck += __shfl_down(ck, o, 16); ch += __shfl_down(ch, o, 16); }
  if ((threadIdx.x & 15) == 0 && base < m) { tile_keep[t >> 4] = ck; tile_heads[t >> 4] = ch; }
}
template <class I>
__global__ __launch_bounds__(256) void active_place_kernel(const uint8_t *__restrict__ keep, uint64_t m,
                                                           const uint32_t *__restrict__ tile_keep,
                                                           const I *__restrict__ tile_off,
                                                           const I *__restrict__ aslot, const I *__restrict__ val,
                                                           const I *__restrict__ newhead, I finbit,
                                                           I *__restrict__ aslot2, I *__restrict__ act_i,
                                                           I *__restrict__ act_grp) {
  __shared__ uint32_t ws[4];
  if ((uint64_t)BID * kTile >= m) return;      // a workgroup of the padded last grid row
  if (tile_keep[BID] == 0) return;       // nothing kept in these 256 positions (most tiles after the first round)
  const uint64_t a = (uint64_t)BID * kTile + threadIdx.x;
  const bool k = a < m && keep[a];
  const unsigned long long mask = __ballot(k);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) ws[wv] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (!k) return;
  I pos = tile_off[BID] + (I)__popcll(mask & ((1ull << lane) - 1ull));
  for (int q = 0; q < wv; q++) pos += ws[q];
  aslot2[pos] = aslot ? aslot[a] : (I)a; act_i[pos] = val[a] & ~finbit; act_grp[pos] = newhead[a];      // no list yet: slot == index
}

template <class I, class K>
__global__ void heads_kernel(uint64_t m, const K *__restrict__ key, const I *__restrict__ aslot,
                             uint8_t *__restrict__ hd, I *__restrict__ hv) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  bool h = (a == 0) || key[a] != key[a - 1];
  hd[a] = h ? 1 : 0;
  hv[a] = h ? aslot[a] : (I)0;
}

// First round of dictionary mode (slot == index): group heads, and the bucket table of the sorted
// keys for rank_at: the first slot of every occupied top-bits bucket marks its reversed entry.
// Per workgroup of 256 slots also the index of its last head (0 = none, slot 0 is always a head): a
// max-scan over those 4 bytes per 256 slots gives every workgroup of write_back0 its carry-in, and
// the head of each slot is found from the head flags with ballots - no N-long scan of head indices.
// Plain mode (DICT false: the first round of a parse or a byte text) takes the same kernel without the key mask, the bucket
// table.
template <class I, bool DICT>
__global__ __launch_bounds__(256) void heads0_kernel(uint64_t m, const uint64_t *__restrict__ key, uint64_t keymask, int shift,
                                                     uint32_t T, uint8_t *__restrict__ hd, I *__restrict__ tile_last,
                                                     I *__restrict__ tab) {
  __shared__ I wl[4];
  if ((uint64_t)BID * 256 >= m) return;      // a workgroup of the padded last grid row
  const uint64_t a = (uint64_t)BID * 256 + threadIdx.x;
  bool h = false;
  if (a < m) {
    if constexpr (DICT) {
      const uint64_t k = key[a] & keymask, kprev = a ? (key[a - 1] & keymask) : ~k;
      h = k != kprev;
      if (a == 0 || (k >> shift) != (kprev >> shift)) tab[T - 1 - (uint32_t)(k >> shift)] = IdxTraits<I>::kNone - (I)a;
    } else {
      h = a == 0 || key[a] != key[a - 1];
    }
    hd[a] = h ? 1 : 0;
  }
  const unsigned long long mask = __ballot(h);
  if ((threadIdx.x & 63) == 0)
    wl[threadIdx.x >> 6] = mask ? (I)(BID * 256ull + (threadIdx.x & ~63) + (63 - __clzll((long long)mask))) : (I)0;
  __syncthreads();
  if (threadIdx.x == 0) {
    I v = wl[0];
    for (int q = 1; q < 4; q++) v = wl[q] > v ? wl[q] : v;
    tile_last[BID] = v;
  }
}
template <class I>
__global__ void fill_kernel(I *p, uint64_t n, I v) {
  uint64_t i = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
// First round of dictionary mode: sa and grp are the sorted values / scanned heads themselves
// (streaming copies); rank[] is written only for the suffixes that stay unresolved.
// Plain mode (DICT false): no terminator flag in the key, nothing settles but a singleton, and rank[] - where there is one - gets
// every suffix, as no search over the sorted keys stands in for it there.
// tile_keep / tile_heads (not null): kept slots and kept group heads of these 256 slots, as active_count_kernel counts them.
template <class I, bool DICT>
__global__ __launch_bounds__(256) void write_back0_kernel(uint64_t m, const I *__restrict__ val,
                                                          const I *__restrict__ tile_scan,
                                                          const uint8_t *__restrict__ hd, const uint64_t *__restrict__ key0,
                                                          I *__restrict__ rank,
                                                          I *__restrict__ grp, uint8_t *__restrict__ keep, int write_ranks,
                                                          uint32_t *__restrict__ tile_keep, uint32_t *__restrict__ tile_heads) {
  __shared__ I wl[4];
  __shared__ uint32_t wk[4], wh[4];
  if ((uint64_t)BID * 256 >= m) return;      // a workgroup of the padded last grid row
  const uint64_t a = (uint64_t)BID * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  // all loads first: nothing below the barrier waits on memory except the carry-in
  const bool in = a < m;
  const bool h = in && hd[a];
  const bool hnext = in && (a + 1 == m || hd[a + 1]);
  const I i = in ? val[a] : (I)0;
  uint32_t flagbit = 0u;
  if constexpr (DICT) flagbit = in ? (uint32_t)(key0[a] & 1ull) : 0u;
  const I carry = BID ? tile_scan[BID - 1] : (I)0;
  const unsigned long long mask = __ballot(h);
  const I wbase = (I)(BID * 256ull + (threadIdx.x & ~63));
  const bool single = h && hnext;
  const bool fin = !single && flagbit;       // the terminator is inside the key: the tied strings are identical
  const bool k = in && !single && !fin;
  if (lane == 0) wl[wv] = mask ? wbase + (63 - __clzll((long long)mask)) : (I)0;
  if (tile_keep) {
    const unsigned long long km = __ballot(k), khm = __ballot(k && h);
    if (lane == 0) { wk[wv] = (uint32_t)__popcll(km); wh[wv] = (uint32_t)__popcll(khm); }
  }
  __syncthreads();
  if (tile_keep && threadIdx.x == 0) {
    tile_keep[BID] = wk[0] + wk[1] + wk[2] + wk[3];
    tile_heads[BID] = wh[0] + wh[1] + wh[2] + wh[3];
  }
  if (!in) return;
  // head of slot a: the last head flag at or before it - in its wave, else in an earlier wave of the
  // workgroup, else the carry-in (last head of all earlier workgroups)
  const unsigned long long upto = mask & (~0ull >> (63 - lane));
  I head;
  if (upto) head = wbase + (63 - __clzll((long long)upto));
  else {
    head = carry;
    for (int q = 0; q < wv; q++) head = wl[q] > head ? wl[q] : head;
  }
  grp[a] = head;       // sa[] is the sorted value array itself (moved into place by the host)
  if constexpr (DICT) {
    if (k && write_ranks) rank[i] = head;     // lazy mode: rank[] of an unresolved suffix is filled in when a doubling round asks
  } else {
    if (rank) rank[i] = head;
  }
  keep[a] = k ? 1 : 0;
}

// dense fallback after the first round: many suffixes stay unresolved, so most lookups would need
// the search; scatter the settled ranks once instead (the pre-lazy behaviour)
template <class I>
__global__ void scatter_settled_kernel(uint64_t N, const I *__restrict__ sa, const I *__restrict__ grp,
                                       const uint8_t *__restrict__ keep, I finbit, I *__restrict__ rank) {
  uint64_t t = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (t < N && !(keep && keep[t])) rank[sa[t]] = grp[t] | finbit;      // (keep null, plain mode's late rank[]: every slot)
}

// Pivot rounds.  The unresolved groups of a dictionary of near-identical phrases (a collection of
// variants) are families: most members are identical to each other up to the terminator or differ
// from each other at one position a few dozen bytes on.  Doubling needs log2(lcp) more rounds for
// them - each a device-wide sort plus a scattered rank update.  A pivot round instead compares
// every member directly with its group's first member P (= sa[head slot]), from the offset already
// known equal, 16 bytes per step, for at most `cap` bytes, and sorts by what it found:
//     smaller than P : (first difference at lcp, own byte there)   ascending lcp, then byte
//     identical to P up to the terminator
//     greater than P : descending lcp, then ascending byte
// Two members that differ from P at different offsets are thereby ordered against each other, two
// that differ at the same offset by their bytes; the same (side, lcp, byte) is a still unresolved
// tie.  A member still equal to P after cap bytes joins P's class unresolved (no settled bit) and
// vetoes the settling of that whole class (pivot_veto_kernel).  Order-key layout (kPivBits bits):
constexpr int kPivBits = 23;
constexpr uint32_t kPivEq = 1u << 21;      // (lcp < kPivCapMax, declared with SorterSwitches at the top, sits above the byte)
// (Tried in round 3: eight lanes per member, 128 contiguous bytes of the member's string per load instruction, the pivot's
//  bytes coalesced, ballot for the first differing chunk.  Same lines fetched, 3x fewer address-coalescer cycles - and 17 %
//  SLOWER (c3 6.8 -> 7.9 ms, 12.6 GB 107 -> 120 ms): the kernel is bound by the rate at which HBM serves random lines
//  (~54 G/s, tools/microbench/gather.hip; 112 M members x ~1.6 lines + their pivots' = 3.9 ms at that rate), not by
//  its instruction stream, and eight times the waves only add ballots.  One thread per member stays.
//  Also tried: 64 bytes per step instead of 32, the second half's loads in flight with the first's - c3 6.5 -> 7.1 ms,
//  12.6 GB 101 -> 102.5 ms: members that differ or end inside the first 32 bytes pay for a second line they do not need.)
template <class I>
__global__ void build_keys_pivot_kernel(const uint8_t *__restrict__ s, uint64_t m, uint64_t from, uint32_t cap,
                                        const I *__restrict__ act_i, const I *__restrict__ act_grp,
                                        const I *__restrict__ sa, I finbit, uint64_t *__restrict__ key,
                                        uint32_t *__restrict__ key32, I *__restrict__ val, int both = 0) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const I i = act_i[a], grp = act_grp[a];
  const I piv = sa[grp];
  uint32_t ok = kPivEq;
  I settled = finbit;
  if (i != piv) {
    settled = 0;
    const uint8_t *pa = s + i + from, *pp = s + piv + from;
    // skim 32 bytes per step until the strings differ or the member ends, then look inside that chunk
    uint32_t off = 0;
    uint4 xa0, xa1, xp0, xp1;
    bool hit = false;
    for (; off < cap; off += 32) {
      xa0 = ld16u(pa + off); xa1 = ld16u(pa + off + 16); xp0 = ld16u(pp + off); xp1 = ld16u(pp + off + 16);
      const uint32_t diff = (xa0.x ^ xp0.x) | (xa0.y ^ xp0.y) | (xa0.z ^ xp0.z) | (xa0.w ^ xp0.w) | (xa1.x ^ xp1.x) |
                            (xa1.y ^ xp1.y) | (xa1.z ^ xp1.z) | (xa1.w ^ xp1.w);
      const uint32_t term = lt2_flags32(xa0.x) | lt2_flags32(xa0.y) | lt2_flags32(xa0.z) | lt2_flags32(xa0.w) | lt2_flags32(xa1.x) |
                            lt2_flags32(xa1.y) | lt2_flags32(xa1.z) | lt2_flags32(xa1.w);
      if (diff | term) { hit = true; break; }
    }
    if (hit) {
      const uint64_t x[4] = {(uint64_t)xa0.x | ((uint64_t)xa0.y << 32), (uint64_t)xa0.z | ((uint64_t)xa0.w << 32),
                             (uint64_t)xa1.x | ((uint64_t)xa1.y << 32), (uint64_t)xa1.z | ((uint64_t)xa1.w << 32)};
      const uint64_t y[4] = {(uint64_t)xp0.x | ((uint64_t)xp0.y << 32), (uint64_t)xp0.z | ((uint64_t)xp0.w << 32),
                             (uint64_t)xp1.x | ((uint64_t)xp1.y << 32), (uint64_t)xp1.z | ((uint64_t)xp1.w << 32)};
      bool done = false;
#pragma unroll
      for (int q = 0; q < 4 && !done; q++) {
        const uint64_t tb = lt2_flags64(x[q]);
        if (x[q] == y[q]) { if (tb) { settled = finbit; done = true; } continue; }
        const int fd = __builtin_ctzll(x[q] ^ y[q]) >> 3;
        const int ft = tb ? (__builtin_ctzll(tb) >> 3) : 8;
        if (ft < fd) { settled = finbit; done = true; continue; }        // both end before they differ: identical
        const uint32_t bx = (uint32_t)(x[q] >> (8 * fd)) & 0xffu, by = (uint32_t)(y[q] >> (8 * fd)) & 0xffu;
        const uint32_t lcp = off + 8 * q + fd;
        ok = bx < by ? ((lcp << 8) | bx) : ((2u << 21) | ((kPivCapMax - 1 - lcp) << 8) | bx);
        if (bx <= kEndOfWord) settled = finbit;      // the member ends here: whoever shares this key is the same string
        done = true;
      }
    }
    // not done: still equal to P after cap bytes -> P's class, without the settled bit
  }
  if (key32) key32[a] = ok;                 // segmented sort: the group is the segment, only the order key is sorted
  if (!key32 || both) key[a] = ((uint64_t)grp << kPivBits) | ok;
  val[a] = i | settled;
}
template <class I>
__global__ void veto_clear_kernel(uint64_t m, const I *__restrict__ newhead, uint8_t *__restrict__ veto) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a < m) veto[newhead[a]] = 0;
}
// a member of P's class without the settled bit (equal to P for cap bytes, unknown beyond): nobody in
// that class may settle this round
template <class I>
__global__ void pivot_veto_kernel(uint64_t m, const uint64_t *__restrict__ key, const uint32_t *__restrict__ key32,
                                  const I *__restrict__ val, const I *__restrict__ newhead, I finbit,
                                  uint8_t *__restrict__ veto) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const uint32_t ok = key32 ? key32[a] : ((uint32_t)key[a] & ((1u << kPivBits) - 1));
  if (ok == kPivEq && !(val[a] & finbit)) veto[newhead[a]] = 1;
}

// write the refined order back and decide which suffixes stay unresolved.
// sorted_len = prefix length that is sorted after this round.
// Round 0 (key0 != nullptr) decides "whole string inside the sorted prefix" from the packed key
// itself (some field holds the terminator code 1): no gather.
template <class I, class K>
__global__ void write_back_kernel(SufGeom g, uint64_t m, uint64_t sorted_len, const I *__restrict__ aslot,
                                  const I *__restrict__ val, const I *__restrict__ newhead,
                                  const uint8_t *__restrict__ hd, I finbit, const K *__restrict__ prevkey,
                                  int prevshift, const I *__restrict__ prevgrp, const uint8_t *__restrict__ veto,
                                  const uint32_t *__restrict__ wstart_bits, I *__restrict__ sa,
                                  I *__restrict__ rank, I *__restrict__ wordrank, I *__restrict__ grp, uint8_t *__restrict__ keep) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const I iv = val[a], i = iv & ~finbit;
  const I slot = aslot[a];
  sa[slot] = i;
  grp[slot] = newhead[a];       // slot-side copy of the group head: the merge never gathers rank[]
  bool single = hd[a] && (a + 1 == m || hd[a + 1]);
  bool fin = false;
  if (!single && g.mode == MODE_DICT) {
    if (finbit) fin = (iv & finbit) != 0 && !(veto && veto[newhead[a]]);   // continuation settled / identical to the pivot
    else fin = suf_len(g, i) <= sorted_len;            // N >= 2^31: no spare bit, gather the length
  }
  const bool k = !single && !fin;
  // rank[i] already holds the old group head: a suffix that stays unresolved in a group that kept
  // its head needs no write - the scattered 4-byte store is the expensive access of this kernel
  const I old = prevkey ? (I)(prevkey[a] >> prevshift) : (prevgrp ? prevgrp[a] : ~newhead[a]);
  // Pivot rounds (lazy_bytes != null) do not read rank[], so the rank of a suffix that settles there is
  // written only if somebody will ask for it - the whole words, whose ranks order the dictionary
  // (compute_lexrank); every other settled rank is filled in by repair_ranks_kernel if a doubling
  // round follows after all.  One byte read replaces the scattered 4-byte store.
  bool wr = k ? old != newhead[a] : true;
  // (a whole word is a singleton group: only a suffix alone in its group can be one; which positions start a word is
  // read from a bitmap of N bits - it stays cache resident where the dictionary bytes would not)
  if (wstart_bits) wr = !k && single && ((wstart_bits[i >> 5] >> (i & 31)) & 1u);
  if (wr && rank) rank[i] = newhead[a] | (k ? (I)0 : finbit);
  else if (wr && wordrank && wstart_bits) wordrank[word_of(g.wv, i)] = newhead[a] | finbit;      // (a settled whole word: see `wr` above)
  keep[a] = k ? 1 : 0;
}

// ranks that pivot rounds left unwritten: every slot re-ordered after the first round that is not in
// the active list any more holds a settled suffix
// lazy ranks: the unresolved suffixes get theirs (= their group's head slot) from the active list
// bit i set: position i starts a word (i == 0 or the byte before it is a terminator)
__global__ __launch_bounds__(256) void word_start_bits_kernel(const uint8_t *__restrict__ s, uint64_t N, uint32_t *__restrict__ bits) {
  const uint64_t wi = (uint64_t)BID * 256 + threadIdx.x;      // 32 positions per thread
  const uint64_t p0 = wi * 32;
  if (p0 >= N) return;
  uint32_t m = 0;
  for (int k = 0; k < 32; k++) {
    const uint64_t i = p0 + k;
    if (i < N && (i == 0 || s[i - 1] == kEndOfWord)) m |= 1u << k;
  }
  bits[wi] = m;
}
template <class I>
__global__ void active_ranks_kernel(uint64_t m, const I *__restrict__ act_i, const I *__restrict__ act_grp, I *__restrict__ rank) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a < m) rank[act_i[a]] = act_grp[a];
}
template <class I>
__global__ void mark_slots_kernel(uint64_t m, const I *__restrict__ aslot, uint8_t *__restrict__ flag) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a < m) flag[aslot[a]] = 1;
}
template <class I>
__global__ void repair_ranks_kernel(uint64_t N, const uint8_t *__restrict__ refined, const uint8_t *__restrict__ active,
                                    const I *__restrict__ sa, const I *__restrict__ grp, I finbit,
                                    I *__restrict__ rank) {
  uint64_t t = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (t < N && refined[t] && !active[t]) rank[sa[t]] = grp[t] | finbit;
}

// The last few thousand suffixes.  A round costs a dozen launches and three host round trips however little is left,
// and the tail of a sort is many such rounds (-p 200: ten rounds for the last 40 K of 63 M suffixes).  Once at most
// kFinishMax suffixes are unresolved - in groups of at most kFinishGrp - every one of them is ranked inside its group by
// comparing the strings themselves (terminated words, or the integer string up to the first difference): lt = members
// that sort before it, eq = identical members before it in the list; nothing is written until no comparison ran past
// kFinishCmp bytes and no group was too long, so a refusal leaves the round machinery where it was.
constexpr uint64_t kFinishMax = 1u << 17;
constexpr int kFinishGrp = 64;
constexpr uint32_t kFinishCmp = 8192;
__device__ __forceinline__ int finish_cmp_dict(const uint8_t *__restrict__ s, uint64_t i, uint64_t j, uint32_t *ovf) {
  for (uint32_t k = 0; k < kFinishCmp; k += 8) {
    const int r = cmp_term8(ld8u(s + i + k), ld8u(s + j + k));
    if (r != kCmpOn) return r;
  }
  *ovf = 1;
  return 0;
}
__device__ __forceinline__ int finish_cmp_int(const uint32_t *__restrict__ sym, uint64_t i, uint64_t j, uint32_t *ovf) {
  for (uint32_t k = 0; k < kFinishCmp / 4; k++) {      // (the sentinel ends the shorter suffix with a difference)
    const uint32_t x = sym[i + k], y = sym[j + k];
    if (x != y) return x < y ? -1 : 1;
  }
  *ovf = 1;
  return 0;
}
template <class I>
__global__ void finish_rank_kernel(SufGeom g, const uint8_t *__restrict__ s, uint64_t m, const I *__restrict__ act_i,
                                   const I *__restrict__ act_grp, uint32_t *__restrict__ lt, uint32_t *__restrict__ eq,
                                   uint32_t *__restrict__ gstart, uint32_t *__restrict__ overflow) {
  // eight lanes per member, each comparing it with every eighth other member of its group (one lane per member was a chain of up
  // to 63 dependent string comparisons: 0.27 ms a launch for a few ten thousand members - the kernel's time is that chain's latency)
  const uint64_t t = (uint64_t)BID * blockDim.x + threadIdx.x;
  const uint64_t a = t >> 3;
  const int l8 = (int)(t & 7);
  if (a >= m) return;
  const I grp = act_grp[a];
  uint64_t gs = a, ge = a + 1;
  while (gs > 0 && a - gs < (uint64_t)kFinishGrp && act_grp[gs - 1] == grp) gs--;
  while (ge < m && ge - gs <= (uint64_t)kFinishGrp && act_grp[ge] == grp) ge++;
  if (ge - gs > (uint64_t)kFinishGrp || (gs > 0 && act_grp[gs - 1] == grp)) { if (l8 == 0) atomicOr(overflow, 1u); return; }
  const uint64_t ia = act_i[a];
  uint32_t nlt = 0, neq = 0, ovf = 0;
  for (uint64_t b = gs + (uint64_t)l8; b < ge; b += 8) {
    if (b == a) continue;
    if (*(volatile uint32_t *)overflow) break;      // somebody met a case for the rounds: no point in finishing the comparisons
    const uint64_t ib = act_i[b];
    const int cmp = g.mode == MODE_DICT ? finish_cmp_dict(s, ib, ia, &ovf) : finish_cmp_int(g.sym, ib, ia, &ovf);
    if (cmp < 0) nlt++;
    else if (cmp == 0 && b < a) neq++;
  }
  // (all eight lanes of a member arrive here together: everything above the loop is the same for them)
  uint32_t packed = nlt | (neq << 8) | (ovf << 16);      // <= 63 each
  packed += __shfl_xor(packed, 1, 64); packed += __shfl_xor(packed, 2, 64); packed += __shfl_xor(packed, 4, 64);
  if (l8 != 0) return;
  if (packed >> 16) atomicOr(overflow, 1u);
  lt[a] = packed & 0xffu; eq[a] = (packed >> 8) & 0xffu; gstart[a] = (uint32_t)gs;
}
template <class I>
__global__ void finish_write_kernel(SufGeom g, uint64_t m, const I *__restrict__ aslot, const I *__restrict__ act_i, const uint32_t *__restrict__ lt,
                                    const uint32_t *__restrict__ eq, const uint32_t *__restrict__ gstart, I finbit,
                                    I *__restrict__ sa, I *__restrict__ grp, I *__restrict__ rank, I *__restrict__ wordrank) {
  const uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const uint64_t gs = gstart[a];
  const I i = act_i[a], slot = aslot[gs + lt[a] + eq[a]], head = aslot[gs + lt[a]];
  sa[slot] = i;
  grp[slot] = head;            // identical strings share their group's first slot
  if (rank) rank[i] = head | finbit;
  else if (wordrank && ((uint64_t)i == 0 || g.wv.bytes[(uint64_t)i - 1] == kEndOfWord)) wordrank[word_of(g.wv, i)] = head | finbit;
}

// after the first round, pivot rounds are tried while the groups are families (average size up to
// kPivotAvg) and each one at least halves the unresolved set; at most SorterSwitches::pivot_cap bytes per comparison
constexpr uint32_t kPivotAvg = 1024u;

// the first round leaves more than N/kLazyRatio suffixes unresolved -> scatter all ranks after all
constexpr uint64_t kLazyRatio = 8ull;

// the library's segmented sort is tried from this average group size on
constexpr uint32_t kSegMinAvg = 24u;

template <class I>
RankViewT<I> rank_view(const SuffixOrderT<I> &so) {
  return RankViewT<I>{so.rank.p, so.skeys.p, so.tab.p, so.lut.p, so.bytes, so.N, so.kbits, so.shift, so.T, so.finbit, so.keymask, so.wordrank.p};
}
template RankViewT<uint32_t> rank_view(const SuffixOrderT<uint32_t> &);
template RankViewT<uint64_t> rank_view(const SuffixOrderT<uint64_t> &);

// what doubling() is asked for
struct DoublingOpts {
  explicit DoublingOpts(const SorterSwitches &sw_) : sw(sw_) {}
  const SorterSwitches sw;               // the entry point's switches, for the rounds
  int key_bits = 64;                     // width of the first-round keys
  bool dict = false;                     // dictionary mode: out.lut/bytes/kbits are set by the caller, ranks are lazy
  std::optional<uint64_t> list_len;      // list mode: key/val hold this many suffixes (in position order), not all g.N - the ones of this
                                         // rank's key range (a share), or
  bool whole_list = false;               // ... every suffix the caller wants sorted (the ones that emit: sort_dict_suffixes), in one piece
  int idx_bits = 0;                      // keys-only first round: the words are (key << idx_bits | position) and val is empty
};

// The sort that the regroup step finds: where its sorted keys are and what they mean.
enum class Round {
  FirstDict,            // first round of a dictionary: packed keys in keyo (heads0 / write_back0, which also start the lazy ranks)
  FirstPlain,           // first round of a parse or a byte text: keys in keyo, no groups before it (heads0 / write_back0 without the
                        // dictionary's key mask, bucket table and flag bit; PFP_PLAIN_TILES=0: the list path of the later rounds)
  DictPivotGlobal,      // dictionary pivot round ordered by one device-wide sort: (group, order key) in keyo
  DictPivotGrouped,     // ... ordered inside its groups: order keys in k32o
  ParsePivot,           // parse pivot round: 64-bit keys in keyo, ordered inside its groups
  DoublingGlobal,       // doubling round ordered device-wide: (group, continuation's rank) in keyo (dkeyo in the 64-bit index build)
  DoublingGrouped,      // ... ordered inside its groups: ranks in k32o
};

// The state of doubling()'s round loop, and one member function per step of it.
template <class I>
struct Rounds {
  using K = typename IdxTraits<I>::DKey;        // key of a doubling round: (group head, 1 + rank of the continuation)
  static constexpr bool kWide = sizeof(I) == 8;
  static constexpr int TB = 256;

  // ---- fixed when the loop starts
  pfp_ctx *const c;
  const SufGeom g;
  SuffixOrderT<I> &out;
  const DoublingOpts o;
  const uint64_t NP, N;         // positions of the string; suffixes sorted here (fewer in range mode)
  const bool lazy;
  // A list of suffixes (fewer than NP) never runs a doubling round - that would read ranks of suffixes outside the list: it
  // stops where one would be needed (out.complete = false).
  const bool list_mode;
  // A share of the suffix array (multi-GPU) also finds its whole words by looking at its own slots (gather_slots_range): no
  // rank per dictionary position is kept.  The list of all suffixes that emit keeps ranks as a whole sort does - slot numbers
  // among the listed suffixes, rank[] or wordrank[] and the search over skeys (rank_at) - so the words' ranks cost no pass.
  const bool range_mode;
  const int nb;                 // key of a later round = (group head << nb) | (1 + rank of the continuation)
  const bool plain_lazy, plain_tiles, dict_fold;      // (o.sw's switches, each in the mode it belongs to)
  bool lazy_active = false, late_rank = false;      // (see start_rounds)
  bool plain_late = false;      // plain mode without rank[] so far: the first doubling round fills it from the slots
  I *rank_p = nullptr, *wordrank_p = nullptr;

  // ---- the loop's variables
  Round kind;                   // the sort that was just run
  uint64_t m, h, m2 = 0, ngrp = 0;      // list length and sorted prefix of that sort; what its regrouping left unresolved, in how many groups
  uint32_t piv_cap = o.sw.pivot_cap;      // bytes compared per member in the next pivot round
  bool pivot_ok = true;         // dictionary pivot rounds still halve the unresolved set
  bool ipiv_ok = true;          // parse: the pivot round (farthest rare symbol) has not given up yet
  bool small_failed = false;    // a direct-placement attempt met a group longer than its window
  bool finisher_ok = true;      // the comparison finisher has not refused yet
  // freshness of rank[]
  bool rank_alloc = false;
  bool lazy_pending = false;    // dictionary mode: rank[] of the suffixes settled by the first round not scattered (yet)
  bool ranks_stale = false;     // pivot rounds skipped rank[] of settled suffixes that are not whole words
  bool active_stale = false;    // ... and the first round / pivot rounds skipped rank[] of the suffixes that stay unresolved

  // ---- buffers of the first round only
  DBuf<uint64_t> &key;          // (the caller's; with keyo/valo the ping-pong pairs of every device-wide sort)
  DBuf<I> &val;
  DBuf<I> tile_last, tile_scan;      // first round by tiles: last head per 256 slots, and its running maximum
  // ---- every round
  DBuf<uint64_t> keyo;
  DBuf<I> valo;
  DBuf<uint8_t> hd, keep;
  // active list (slot, suffix, group) of the unresolved suffixes and per-round scratch, list_cap elements each;
  // a first round by tiles (tiles_first) allocates them when it has told how many suffixes stay unresolved
  DBuf<I> aslot, aslot2, hv, newhead, act_i, act_grp;
  uint64_t list_cap = 0;
  DBuf<uint32_t> tile_keep, tile_heads;
  DBuf<I> tile_off, tile_hoff;
  // ---- dictionary mode, after the first round / on the first pivot round
  DBuf<uint8_t> keep0, veto;
  DBuf<uint32_t> wstart_bits;   // which positions start a word (their ranks order the dictionary)
  // ---- allocated on first use by the rounds ordered inside their groups
  DBuf<uint8_t> gs, bigf;
  DBuf<uint32_t> k32, k32o, segb, sege, nseg_d, ovf_d;
  DBuf<uint64_t> nsel_d;
  // ---- allocated on the first doubling round
  DBuf<K> dkey, dkeyo;          // wide build: 128-bit doubling keys (the 32-bit build keeps them in key/keyo)

  Rounds(pfp_ctx *c_, const SufGeom &g_, DBuf<uint64_t> &key_, DBuf<I> &val_, uint64_t h0, SuffixOrderT<I> &out_, const DoublingOpts &o_)
      : c(c_), g(g_), out(out_), o(o_), NP(g_.N), N(o_.list_len.value_or(g_.N)), lazy(o_.dict), list_mode(o_.list_len.has_value()),
        range_mode(o_.list_len.has_value() && !o_.whole_list),
        nb(bits_for(N)), plain_lazy(!o_.dict && o_.sw.plain_lazy_rank), plain_tiles(!o_.dict && o_.sw.plain_tiles),
        dict_fold(o_.dict && o_.sw.dict_fold), kind(o_.dict ? Round::FirstDict : Round::FirstPlain), m(N), h(h0), key(key_),
        val(val_) {}
  // the first round regroups by tiles (slot == index, no list yet): a dictionary always, plain mode by its switch
  bool tiles_first() const { return lazy || plain_tiles; }

  static uint64_t blocks(uint64_t n) { return cdiv(n, TB); }

  // ---- first round: one device-wide sort of all N (key, position) pairs, ping-ponging between the two buffer
  //      pairs (no third copy inside the library); afterwards keyo/valo hold the sorted pairs
  void first_round_sort() {
    keyo.alloc(c, N); valo.alloc(c, N);
    SortTag first_tag(g.mode == MODE_DICT ? "dictionary, first round" : "parse, first round");
    if (o.idx_bits) {
      // keys-only first round: the words are (key << idx_bits | position), 16 bytes per element and pass instead of 24;
      // the sort is stable on the key bits alone, so ties stay in position order; one streaming pass splits the result
      sort_keys_db(c, key, keyo, N, o.idx_bits, o.idx_bits + o.key_bits);
      KScope ks(c, "pfp::split_keys_kernel", N * (16 + sizeof(I)));
      hipLaunchKernelGGL(split_keys_kernel<I>, gdim(blocks(N)), gdim(TB), 0, c->stream, key.p, N, o.idx_bits, keyo.p, valo.p);
    } else {
      sort_pairs_db(c, key, keyo, val, valo, N, 0, o.key_bits);
      std::swap(key, keyo); std::swap(val, valo);
    }
  }

  void alloc_lists(uint64_t cap) {
    aslot.alloc(c, cap); aslot2.alloc(c, cap); hv.alloc(c, cap); newhead.alloc(c, cap); act_i.alloc(c, cap); act_grp.alloc(c, cap);
    list_cap = cap;
  }
  void alloc_rank() {
    out.rank.alloc(c, NP);
    if (lazy) PFP_HIP(hipMemsetAsync(out.rank.p, 0xff, NP * sizeof(I), c->stream));
    rank_p = out.rank.p; rank_alloc = true;
  }

  // what every later round works on, allocated once the first sort is done
  void start_rounds() {
    if (lazy) { key.release(); val.release(); }      // dictionary mode: later rounds sort the (much smaller) unresolved set
    // (allocated only now: while the first sort holds its four buffers - 32 bytes per suffix in the wide build - nothing else
    //  of that size is live: a 4.8 GB dictionary peaked at 206 GB with the group array next to them, 168 GB without)
    hd.alloc(c, N + 1); keep.alloc(c, N);
    out.grp.alloc(c, N + 8);
    if (!lazy) {
      if (!plain_tiles) {      // (by tiles: sa is the sorted value array, the lists come when the round has told their size)
        out.sa.alloc(c, N);
        alloc_lists(N);
        hipLaunchKernelGGL(iota_kernel<I>, gdim(blocks(N)), gdim(TB), 0, c->stream, aslot.p, N);
      }
    } else {
      const int tb = std::min(o.key_bits, std::max(8, std::min(24, bits_for(N) - 5)));
      out.shift = o.key_bits - tb;
      out.T = 1u << tb;
      out.tab.alloc(c, out.T);
      hipLaunchKernelGGL(fill_kernel<I>, gdim(blocks(out.T)), gdim(TB), 0, c->stream, out.tab.p, (uint64_t)out.T,
                         (I)(IdxTraits<I>::kNone - (I)N));
    }
    // (the flag rides in the top bit of a POSITION: it needs positions below 2^31 in the 32-bit build - all NP of them, also when
    //  only a share of N < 2^31 suffixes is sorted here)
    out.finbit = (g.mode == MODE_DICT && (kWide || NP < (1ull << 31)) && o.sw.finflag) ? IdxTraits<I>::kTop : (I)0;
    // lazy ranks are possible when pivot rounds (which never read rank[]) can follow the first round
    lazy_active = lazy && pivot_rounds_possible();
    // rank[] (one entry per dictionary position: 4 / 8 bytes each, 38 GB for a 4.8 GB dictionary in the wide build) exists
    // from the start only where a round may read it.  With lazy ranks nothing reads it before the first doubling round - and a
    // dictionary of word families never gets there - so it is allocated when (if) that round comes (late_rank); until then the
    // whole words, whose ranks order the dictionary, report to wordrank[d].  (PFP_DEBUG validates every rank: eager.)
    late_rank = !range_mode && lazy_active && !c->debug;
    // Plain mode: only a doubling round reads rank[], and the parse of a collection is settled by its pivot round and the
    // finisher; sa[] and grp[] are complete after every round there, so the round that asks fills rank[] from them in one pass
    plain_late = !lazy && !range_mode && plain_lazy && !c->debug;
    if (!range_mode && !late_rank && !plain_late) alloc_rank();
    if (late_rank) {
      out.wordrank.alloc(c, (uint64_t)g.wv.d + 1);
      PFP_HIP(hipMemsetAsync(out.wordrank.p, 0xff, ((uint64_t)g.wv.d + 1) * sizeof(I), c->stream));
      wordrank_p = out.wordrank.p;
    }
  }
  bool pivot_rounds_possible() const {
    return g.mode == MODE_DICT && out.finbit && o.sw.pivot_cap >= 16 && (uint64_t)nb + kPivBits <= 64;
  }

  // ---- regrouping: heads of the new groups -> slots, group ids, ranks -> compaction of what stays unresolved
  template <class KT>
  void heads(const KT *keys, int bytes) {
    KScope ks(c, "pfp::heads_kernel", m * bytes);
    hipLaunchKernelGGL((heads_kernel<I, KT>), gdim(blocks(m)), gdim(TB), 0, c->stream, m, keys, aslot.p, hd.p, hv.p);
  }
  void heads_k32() {
    KScope ks(c, "pfp::heads32_kernel", m * 14);
    hipLaunchKernelGGL(heads32_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, m, gs.p, k32o.p, aslot.p, hd.p, hv.p);
  }

  // tile counts of the kept slots and kept heads, written by the first round's write-back (compact() then launches no count)
  bool counts_from_write_back() const { return lazy ? dict_fold : plain_tiles; }
  void alloc_tile_counts() {
    if (!tile_keep.p) { tile_keep.alloc(c, cdiv64(N, kTile) + 1); tile_heads.alloc(c, cdiv64(N, kTile) + 1);
                        tile_off.alloc(c, cdiv64(N, kTile) + 1); tile_hoff.alloc(c, cdiv64(N, kTile) + 1); }
  }
  void first_dict_heads_and_write_back() {
    const bool counts = counts_from_write_back();
    if (counts) alloc_tile_counts();
    tile_last.alloc(c, cdiv64(m, 256)); tile_scan.alloc(c, cdiv64(m, 256));
    { KScope ks(c, "pfp::heads0_kernel", m * 13);
      hipLaunchKernelGGL((heads0_kernel<I, true>), gdim(blocks(m)), gdim(TB), 0, c->stream, m, keyo.p, out.keymask, out.shift, out.T,
                         hd.p, tile_last.p, out.tab.p); }
    inclusive_max<I>(c, out.tab.p, out.tab.p, out.T);
    inclusive_max<I>(c, tile_last.p, tile_scan.p, cdiv64(m, 256));
    { KScope ks(c, "pfp::write_back0_kernel", m * (4 + 4 + 1 + 8 + 4 + 1));
      hipLaunchKernelGGL((write_back0_kernel<I, true>), gdim(blocks(m)), gdim(TB), 0, c->stream, m, valo.p, tile_scan.p, hd.p, keyo.p,
                         rank_p, out.grp.p, keep.p, (lazy_active || range_mode) ? 0 : 1,
                         counts ? tile_keep.p : (uint32_t *)nullptr, counts ? tile_heads.p : (uint32_t *)nullptr); }
    if (lazy_active) active_stale = true;
    // the sorted keys and the sorted positions stay with the result; later rounds sort the (smaller) active set elsewhere
    out.skeys = std::move(keyo);
    out.sa = std::move(valo);
  }
  // plain mode by tiles: the same two kernels without what belongs to the dictionary's keys; the sorted keys stay in keyo
  void first_plain_heads_and_write_back() {
    alloc_tile_counts();
    tile_last.alloc(c, cdiv64(m, 256)); tile_scan.alloc(c, cdiv64(m, 256));
    { KScope ks(c, "pfp::heads0_kernel", m * 9);
      hipLaunchKernelGGL((heads0_kernel<I, false>), gdim(blocks(m)), gdim(TB), 0, c->stream, m, keyo.p, ~0ull, 0, 0u, hd.p, tile_last.p,
                         (I *)nullptr); }
    inclusive_max<I>(c, tile_last.p, tile_scan.p, cdiv64(m, 256));
    { KScope ks(c, "pfp::write_back0_kernel", m * (sizeof(I) + 1 + sizeof(I) + 1 + (rank_p ? sizeof(I) : 0)));
      hipLaunchKernelGGL((write_back0_kernel<I, false>), gdim(blocks(m)), gdim(TB), 0, c->stream, m, valo.p, tile_scan.p, hd.p,
                         (const uint64_t *)nullptr, rank_p, out.grp.p, keep.p, 0, tile_keep.p, tile_heads.p); }
    out.sa = std::move(valo);
  }

  // The one place that knows, per kind of round, which heads kernel reads which keys and what the write-back is told of the
  // element now at list position a: its previous group head - the high part of its device-wide sort key, or (a round ordered
  // inside its groups keeps every element in its segment) the group of list position a; the first round of plain mode has
  // neither: everything is written - and, after a pivot round, the vetoes and the word starts.
  void heads_and_write_back() {
    const uint64_t *keys = nullptr;      // (group head << keybits | ...) of a device-wide sort
    const K *dkeys = nullptr;            // ... of the wide build's doubling round
    const I *prevgrp = nullptr;
    const uint32_t *pivk32 = nullptr;
    bool pivot = false;
    switch (kind) {
      case Round::FirstDict: return first_dict_heads_and_write_back();
      case Round::FirstPlain:
        if (plain_tiles) return first_plain_heads_and_write_back();
        heads(keyo.p, 17);
        break;
      case Round::DictPivotGlobal: heads(keyo.p, 17); keys = keyo.p; pivot = true; break;
      case Round::DictPivotGrouped: heads_k32(); prevgrp = act_grp.p; pivk32 = k32o.p; pivot = true; break;
      case Round::ParsePivot: {
        KScope ks(c, "pfp::heads64seg_kernel", m * 18);
        hipLaunchKernelGGL(heads64seg_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, m, gs.p, keyo.p, aslot.p, hd.p, hv.p);
        prevgrp = act_grp.p;
      } break;
      case Round::DoublingGlobal:
        if constexpr (kWide) { heads(dkeyo.p, 25); dkeys = dkeyo.p; }
        else { heads(keyo.p, 17); keys = keyo.p; }
        break;
      case Round::DoublingGrouped: heads_k32(); prevgrp = act_grp.p; break;
    }
    inclusive_max<I>(c, hv.p, newhead.p, m);
    if (pivot) {
      if (!veto.p) veto.alloc(c, N);
      // only the entries of this round's groups are looked at: clear those (m bytes at most), not all N
      hipLaunchKernelGGL(veto_clear_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, m, newhead.p, veto.p);
      hipLaunchKernelGGL(pivot_veto_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, m, keyo.p, pivk32, valo.p, newhead.p, out.finbit, veto.p);
    }
    KScope ks(c, "pfp::write_back_kernel", m * (13 + 4 + 13));
    if (pivot && !wstart_bits.p) {
      wstart_bits.alloc(c, cdiv64(NP, 32));
      hipLaunchKernelGGL(word_start_bits_kernel, gdim(blocks(cdiv64(NP, 32))), gdim(TB), 0, c->stream, out.bytes, NP, wstart_bits.p);
    }
    const uint8_t *vetop = pivot ? veto.p : (const uint8_t *)nullptr;
    const uint32_t *lazyb = pivot ? wstart_bits.p : (const uint32_t *)nullptr;
    if (dkeys)
      hipLaunchKernelGGL((write_back_kernel<I, K>), gdim(blocks(m)), gdim(TB), 0, c->stream, g, m, h, aslot.p, valo.p, newhead.p, hd.p,
                         out.finbit, dkeys, nb, prevgrp, vetop, lazyb, out.sa.p, rank_p, wordrank_p, out.grp.p, keep.p);
    else
      hipLaunchKernelGGL((write_back_kernel<I, uint64_t>), gdim(blocks(m)), gdim(TB), 0, c->stream, g, m, h, aslot.p, valo.p, newhead.p,
                         hd.p, out.finbit, keys, pivot ? kPivBits : nb, prevgrp, vetop, lazyb, out.sa.p, rank_p, wordrank_p, out.grp.p, keep.p);
    if (pivot) { ranks_stale = true; active_stale = true; }
  }

  // kept suffixes / kept group heads per tile -> offsets -> placement into the next active list; sets m2 and ngrp
  void compact() {
    const bool round0 = kind == Round::FirstDict || (kind == Round::FirstPlain && plain_tiles);      // slot == index, no list yet
    const uint64_t ntile = cdiv64(m, kTile);
    alloc_tile_counts();
    auto read_counts = [&]() {
      sync(c);
      I t0, t1;
      memcpy(&t0, c->h_scalars, sizeof(I)); memcpy(&t1, c->h_scalars + 1, sizeof(I));
      m2 = t0; ngrp = t1;
    };
    {
      PFP_HIP(hipMemsetAsync(tile_keep.p + ntile, 0, 4, c->stream));
      PFP_HIP(hipMemsetAsync(tile_heads.p + ntile, 0, 4, c->stream));
      KScope ks(c, "pfp::active_place_kernel", m * 2 + 0);      // (+ active_count_kernel and the two tile scans)
      if (!(round0 && counts_from_write_back()))
        hipLaunchKernelGGL(active_count_kernel, gdim((unsigned)cdiv64(ntile, 16)), gdim(256), 0, c->stream, keep.p, hd.p, m,
                           tile_keep.p, tile_heads.p);
      exclusive_sum_u32_to<I>(c, tile_keep.p, tile_off.p, ntile + 1);
      exclusive_sum_u32_to<I>(c, tile_heads.p, tile_hoff.p, ntile + 1);
      PFP_HIP(hipMemcpyAsync(c->h_scalars, tile_off.p + ntile, sizeof(I), hipMemcpyDeviceToHost, c->stream));
      PFP_HIP(hipMemcpyAsync(c->h_scalars + 1, tile_hoff.p + ntile, sizeof(I), hipMemcpyDeviceToHost, c->stream));
      if (round0) {      // the lists are sized by what the first round left unresolved
        read_counts();
        if (m2) alloc_lists(m2);
      }
      if (!round0 || m2)
        hipLaunchKernelGGL(active_place_kernel<I>, gdim((unsigned)ntile), gdim(256), 0, c->stream, keep.p, m, tile_keep.p, tile_off.p,
                           round0 ? (const I *)nullptr : aslot.p, round0 ? out.sa.p : valo.p, round0 ? out.grp.p : newhead.p, out.finbit,
                           aslot2.p, act_i.p, act_grp.p);
      PFP_HIP(hipGetLastError());
    }
    if (!round0) read_counts();
  }

  // regroup what the last round sorted
  void regroup() {
    heads_and_write_back();
    compact();
    if (kind == Round::FirstDict && m2) {
      // whether the settled ranks get scattered after all is decided when (if) a doubling round
      // first needs them: pivot rounds read the strings, not rank[]
      lazy_pending = true;
      if (dict_fold) {      // the first round's keep[] itself; the list rounds flag list positions, m2 of them at most
        keep0 = std::move(keep);
        keep.alloc(c, m2);
      } else {
        keep0.alloc(c, N);
        PFP_HIP(hipMemcpyAsync(keep0.p, keep.p, N, hipMemcpyDeviceToDevice, c->stream));
      }
      out.n_refined = m2;
      if (out.paybits) {       // the merge wants to know which slots were re-ordered after this round
        out.refined.alloc(c, N + 16);
        PFP_HIP(hipMemcpyAsync(out.refined.p, keep0.p, N, hipMemcpyDeviceToDevice, c->stream));
        PFP_HIP(hipMemsetAsync(out.refined.p + N, 0, 16, c->stream));
      }
    }
    if (o.sw.trace_rounds) {
      const bool grouped = kind == Round::DictPivotGrouped || kind == Round::ParsePivot || kind == Round::DoublingGrouped;
      fprintf(stderr, "[pfp] doubling N=%llu round=%llu h=%llu m=%llu -> %llu unresolved in %llu groups%s\n", (unsigned long long)N,
              (unsigned long long)out.rounds, (unsigned long long)h, (unsigned long long)m, (unsigned long long)m2,
              (unsigned long long)ngrp, grouped ? " (seg)" : (kind == Round::DictPivotGlobal ? " (pivot)" : ""));
    }
  }

  // a pivot round that did not at least halve the unresolved set: what is left are members equal to
  // their pivot for the whole comparison window.  The window then grows fourfold (512 -> 2 K -> 8 K bytes) as long
  // as the bytes such a round may read - every member the full window - stay below 256 per dictionary byte; the
  // variants of long phrases settle there (-p 200: 3.3 M suffixes went through nine doubling rounds instead).
  // After the widest window the rest is doubling's business.
  void judge_pivot_round() {
    if (kind == Round::ParsePivot && m2 * 4 > m) ipiv_ok = false;      // a parse pivot round that left more than a quarter: doubling from here
    if ((kind == Round::DictPivotGlobal || kind == Round::DictPivotGrouped) && m2 * 2 > m) {
      const uint32_t next_cap = std::min<uint32_t>(piv_cap * 4, kPivCapMax - 16);
      if (piv_cap < kPivCapMax - 16 && piv_cap >= 16 && m2 * (uint64_t)next_cap < N * 128) piv_cap = next_cap;
      else pivot_ok = false;
    }
  }

  // the unresolved suffixes become the list of the next sort
  void next_list() {
    std::swap(aslot, aslot2);
    m = m2;
    if (m == 0) return;
    PFP_REQUIRE(h < 2 * NP, PFP_EHIP, "suffix sort failed to converge");
    if (!keyo.p || keyo.n < m) keyo.alloc(c, m);
    if (!key.p || key.n < m) key.alloc(c, m);
    if (!valo.p || valo.n < m) valo.alloc(c, m);
    if (!val.p || val.n < m) val.alloc(c, m);
  }

  // the comparison finisher (see finish_rank_kernel); false: not tried, or it refused and nothing was written
  bool try_finisher() {
    if (!(o.sw.finisher && finisher_ok && m <= kFinishMax && out.rounds >= 1 && (g.mode == MODE_DICT || (g.mode == MODE_PLAIN && g.sym))))
      return false;
    DBuf<uint32_t> flt(c, m), feq(c, m), fgs(c, m), fov(c, 1);
    fov.zero();
    KScope ks(c, "pfp::finish_rank_kernel", m * (sizeof(I) * 4 + 12));
    hipLaunchKernelGGL(finish_rank_kernel<I>, gdim(blocks(m * 8)), gdim(TB), 0, c->stream, g, out.bytes, m, act_i.p, act_grp.p, flt.p, feq.p,
                       fgs.p, fov.p);
    if (read_scalar(c, fov.p) != 0) {
      finisher_ok = false;      // a long group or a long common prefix: the rounds go on as they would have
      return false;
    }
    { KScope kw(c, "pfp::finish_write_kernel", m * (sizeof(I) * 5 + 12));
      hipLaunchKernelGGL(finish_write_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, g, m, aslot.p, act_i.p, flt.p, feq.p, fgs.p,
                         out.finbit, out.sa.p, out.grp.p, rank_p, wordrank_p); }
    PFP_HIP(hipGetLastError());
    if (o.sw.trace_rounds) fprintf(stderr, "[pfp] doubling N=%llu round=%llu: the last %llu suffixes ranked by comparison\n",
                                      (unsigned long long)N, (unsigned long long)out.rounds, (unsigned long long)m);
    out.rounds++;
    m = 0;
    return true;
  }

  // ---- ordering the keys of the (grouped) active list inside their groups.
  // Rounds after the first: the unresolved suffixes are already grouped, only the 32-bit "next"
  // key has to be ordered inside every group.  When the groups are many and of moderate size (a
  // dictionary of near-identical variants) a segmented sort moves 16 B per suffix instead of the
  // 7 x 24 B of a global 53-bit radix sort (big: 240 -> 126 ms of sorting).  rocPRIM's segmented
  // sort serialises a giant segment on one workgroup (the 300 k run of one symbol in a parse cost
  // 68 ms), and for tiny groups its bookkeeping eats the gain, so the choice is per round.

  // families of a handful of members: placed directly in LDS (after a group proved too long, only once the average is tiny)
  // (32-bit build: long families go to the side sort, so the average may be larger)
  bool small_groups() const {
    return o.sw.small_seg && ngrp && m / ngrp <= (kWide ? kSmallSeg / 4 : kSmallSeg / 2) && (!small_failed || m / ngrp <= 3);
  }
  // large families (a collection of hundreds of copies): the library's segmented sort is worth its set-up
  // (m < 2^32 - its offsets are 32-bit - always holds in the 32-bit index build)
  bool segmented_worthwhile() const { return ngrp && m >= (1u << 20) && m < 0xFFFFFFFFull && m / ngrp >= kSegMinAvg; }

  void seg_bufs() {
    if (!gs.p) { gs.alloc(c, list_cap + 1); k32.alloc(c, list_cap); k32o.alloc(c, list_cap); nseg_d.alloc(c, 2); nsel_d.alloc(c, 1); ovf_d.alloc(c, 1); }
  }
  // kin/val -> kout/valo, every group of the list sorted by its key; false: some group has more than kSmallSeg
  // members (nothing usable was written).
  // 32-bit keys in the 32-bit index build: the groups of more than kSmallSeg members are passed through in place, flagged, and
  // finished by ONE library sort of just their elements (a few long families no longer send the whole round to the library)
  template <class KT>
  bool place_small_groups(const KT *kin, KT *kout) {
    constexpr bool side = !kWide && sizeof(KT) == 4;
    seg_bufs();
    ovf_d.zero();
    if (side && (!bigf.p || bigf.n < m + 16)) bigf.alloc(c, list_cap + 16);
    { KScope ks(c, "pfp::seg_small_sort_kernel", m * (2 * sizeof(KT) + 3 * sizeof(I) + 1));
      hipLaunchKernelGGL((seg_small_sort_kernel<I, KT>), gdim(blocks(m)), gdim(TB), 0, c->stream, m, act_grp.p, kin, val.p, gs.p, kout,
                         valo.p, ovf_d.p, side ? bigf.p : (uint8_t *)nullptr); }
    if (read_scalar(c, ovf_d.p) == 0) return true;
    if (!side) return false;
    PFP_HIP(hipMemsetAsync(bigf.p + m, 0, 16, c->stream));      // (the flag reader looks at 16 bytes at a time)
    const uint64_t nbig = count_flags(c, bigf.p, m);
    if (nbig * 2 > m) return false;                // mostly long groups: the round is the library's after all
    DBuf<I> idx(c, nbig + 1), sv(c, nbig), sva(c, nbig);
    DBuf<uint64_t> sk(c, nbig), ska(c, nbig), cnt(c, 1);
    select_index<I>(c, bigf.p, idx.p, cnt.p, m);
    hipLaunchKernelGGL(big_seg_gather_kernel<I>, gdim(blocks(nbig)), gdim(TB), 0, c->stream, nbig, idx.p, act_grp.p, k32o.p, valo.p, sk.p, sv.p);
    sort_pairs_db(c, sk, ska, sv, sva, nbig, 0, 32 + nb);
    hipLaunchKernelGGL(big_seg_scatter_kernel<I>, gdim(blocks(nbig)), gdim(TB), 0, c->stream, nbig, idx.p, sk.p, sv.p, k32o.p, valo.p);
    PFP_HIP(hipGetLastError());
    return true;
  }
  // segments of the library's sort = groups of the list (segb/sege; the compaction that built the list counted its group heads - no
  // read-back of the selection's count); false: a group of more than 2^15 members, too long for it
  bool library_segments() {
    seg_bufs();
    if (!segb.p) { segb.alloc(c, list_cap + 1); sege.alloc(c, list_cap + 1); }
    hipLaunchKernelGGL(group_starts_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, m, act_grp.p, gs.p);
    select_index<uint32_t>(c, gs.p, segb.p, nsel_d.p, m);
    PFP_HIP(hipMemsetAsync(nseg_d.p + 1, 0, 4, c->stream));
    if (c->debug) PFP_REQUIRE(read_scalar(c, nsel_d.p) == ngrp, PFP_EHIP, "group count of the active list differs from the compaction's");
    hipLaunchKernelGGL(seg_end_kernel, gdim(blocks(ngrp)), gdim(TB), 0, c->stream, (uint32_t)ngrp, (uint32_t)m, segb.p, sege.p, nseg_d.p + 1);
    return read_scalar(c, nseg_d.p + 1) <= (1u << 15);
  }
  // the fallback: (group, key) pairs of the whole list through one device-wide sort, key/val -> keyo/valo
  void sort_device_wide(int bits) {
    sort_pairs_db(c, key, keyo, val, valo, m, 0, bits);
    std::swap(key, keyo); std::swap(val, valo);
  }

  // ---- the rounds.  A pivot round leaves the sorted prefix common to all groups at h: only a doubling round doubles it.
  bool dict_pivot_wanted() const { return pivot_ok && pivot_rounds_possible() && ngrp && m / ngrp <= kPivotAvg; }
  void dict_pivot_round() {
    // few suffixes left: the widest window at once.  (A compare reads only as far as the strings agree; the window bounds
    // the worst case, m x window bytes.  What is left after two rounds are mostly members of phrases longer than the
    // 512-byte window: without this they cost one round that settles nothing and quadruples the window, then another.)
    if (piv_cap >= 16 && piv_cap < kPivCapMax - 16 && out.rounds >= 2 && m * (uint64_t)(kPivCapMax - 16) < N * 128) piv_cap = kPivCapMax - 16;
    // a segmented sort of the 23-bit order key moves 16 B per suffix instead of 7 x 24 B
    bool small = small_groups();
    bool seg = !small && segmented_worthwhile() && library_segments();
    if (small) seg_bufs();
    // both key forms are written when the direct placement is tried: should a group prove too long, the
    // device-wide sort takes over with the 64-bit keys
    { KScope ks(c, "pfp::build_keys_pivot_kernel", m * (4 + 4 + 4 + 12 + 64));
      hipLaunchKernelGGL(build_keys_pivot_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, out.bytes, m, h, piv_cap, act_i.p,
                         act_grp.p, out.sa.p, out.finbit, key.p, (seg || small) ? k32.p : (uint32_t *)nullptr, val.p, small ? 1 : 0); }
    if (small && !place_small_groups(k32.p, k32o.p)) {
      small = false; small_failed = true;
      seg = segmented_worthwhile() && library_segments();
    }
    if (seg) segsort_pairs_u32<I>(c, k32.p, k32o.p, val.p, valo.p, m, (uint32_t)ngrp, segb.p, sege.p, 0, kPivBits);
    else if (!small) sort_device_wide(nb + kPivBits);
    kind = (small || seg) ? Round::DictPivotGrouped : Round::DictPivotGlobal;
    out.rounds++;
  }

  // the parse of a collection: a pivot round with the member whose next rare symbol is farthest (see ipivot_select_kernel)
  // (a share of the parse - range mode - has no doubling rounds to fall back on: it tries whatever the list's size)
  bool parse_pivot_wanted() const {
    return g.mode == MODE_PLAIN && g.dist && g.sym && ipiv_ok && ngrp && (range_mode || m >= o.sw.parse_pivot_min) && m < 0xFFFFFFFFull && m / ngrp >= 2;
  }
  // (32-bit index build only.)  There is no device-wide fallback: false, and no more parse pivot rounds, where neither way of
  // ordering the groups took them
  bool parse_pivot_round() {
    {
      DBuf<unsigned long long> best(c, N);
      best.zero();
      KScope ks(c, "pfp::ipivot_keys_kernel", m * (4 + 4 + 4 + 8 + 16 + 12 + 64));
      // the members' distances travel from one kernel to the other in hv[] (list_cap >= m entries of at least 4 bytes; nothing
      // of the list's scratch is live between next_list() and the heads of the coming sort)
      const bool batched = o.sw.ipivot_batch;
      uint32_t *dvs = batched ? reinterpret_cast<uint32_t *>(hv.p) : nullptr;
      hipLaunchKernelGGL(ipivot_select_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, m, NP, h, act_i.p, act_grp.p, g.dist, best.p, dvs);
      if (batched)
        hipLaunchKernelGGL((ipivot_keys_batch_kernel<I, kIntPivBatch>), gdim(blocks(m)), gdim(TB), 0, c->stream, m, NP, h, kIntPivCap, g.sym,
                           act_i.p, act_grp.p, best.p, dvs, key.p, val.p);
      else
        hipLaunchKernelGGL(ipivot_keys_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, m, NP, h, kIntPivCap, g.sym, act_i.p,
                           act_grp.p, best.p, key.p, val.p);
    }
    // small groups (pairs of copies with a common SNP): placed by counting in LDS, whatever PFP_NO_SMALLSEG says
    bool sorted = m / ngrp <= kSmallSeg / 2 && place_small_groups(key.p, keyo.p);
    if (!sorted && (m / ngrp >= 4 || range_mode) && library_segments()) {      // (a share has nothing else to fall back on)
      segsort_pairs_u64_u32(c, key.p, keyo.p, val.p, valo.p, m, (uint32_t)ngrp, segb.p, sege.p, 0, 32 + bits_for(2 * kIntPivCap + 3));
      sorted = true;
    }
    if (!sorted) { ipiv_ok = false; return false; }
    kind = Round::ParsePivot;
    out.rounds++;
    return true;
  }

  // a doubling round reads rank[] of arbitrary positions: whatever the first round and the pivot rounds left out is filled in
  void repair_ranks(uint64_t m_active, const I *aslot_list) {
    if (!ranks_stale) return;
    DBuf<uint8_t> act(c, N);
    act.zero();
    if (m_active) hipLaunchKernelGGL(mark_slots_kernel<I>, gdim(blocks(m_active)), gdim(TB), 0, c->stream, m_active, aslot_list, act.p);
    KScope ks(c, "pfp::repair_ranks_kernel", N * 6);
    hipLaunchKernelGGL(repair_ranks_kernel<I>, gdim(blocks(N)), gdim(TB), 0, c->stream, N, keep0.p, act.p, out.sa.p, out.grp.p,
                       out.finbit, out.rank.p);
    ranks_stale = false;
  }
  void prepare_ranks_for_doubling() {
    if (plain_late && !rank_alloc) {      // plain mode's first doubling round: every suffix gets its slot's group head
      alloc_rank();
      KScope ks(c, "pfp::scatter_settled_kernel", N * 3 * sizeof(I));
      hipLaunchKernelGGL(scatter_settled_kernel<I>, gdim(blocks(N)), gdim(TB), 0, c->stream, N, out.sa.p, out.grp.p, (const uint8_t *)nullptr,
                         (I)0, out.rank.p);
      // (the tests tell the three histories apart by this line - never, before any pivot round, after one; `round` is the
      //  doubling round that asks, as the round lines count them)
      if (o.sw.trace_rounds)
        fprintf(stderr, "[pfp] doubling N=%llu round=%llu: rank[] allocated late and filled from the slots\n", (unsigned long long)N,
                (unsigned long long)out.rounds + 1);
    }
    if (late_rank && !rank_alloc) {      // the first doubling round: rank[] is needed after all
      alloc_rank();
      ranks_stale = true;               // whatever pivot rounds settled (whole words included) is filled in from the slots
    }
    if (lazy_pending) {
      lazy_pending = false;
      if (m * kLazyRatio > N) {      // most lookups would need the search: scatter the settled ranks once
        KScope ks(c, "pfp::scatter_settled_kernel", N * (4 + 4 + 1 + 4));
        hipLaunchKernelGGL(scatter_settled_kernel<I>, gdim(blocks(N)), gdim(TB), 0, c->stream, N, out.sa.p, out.grp.p, keep0.p,
                           out.finbit, out.rank.p);
        if (!out.paybits) out.skeys.release();      // with payload the merge still reads the records from skeys
        out.tab.release();
      }
    }
    repair_ranks(m, aslot.p);
    if (active_stale) {
      hipLaunchKernelGGL(active_ranks_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, m, act_i.p, act_grp.p, out.rank.p);
      active_stale = false;
    }
  }

  void build_keys32(const RankViewT<I> &L) {
    KScope ks(c, "pfp::build_keys32_kernel", m * (4 + 4 + 8));
    hipLaunchKernelGGL(build_keys32_kernel, gdim(blocks(m)), gdim(TB), 0, c->stream, g, m, h, act_i.p, L, k32.p, val.p);
  }
  void doubling_round() {
    const RankViewT<I> L = rank_view(out);
    const int keybits = 2 * nb;
    kind = Round::DoublingGlobal;
    if constexpr (kWide) {
      if (!dkey.p || dkey.n < m) { dkey.alloc(c, m); dkeyo.alloc(c, m); }
      { KScope ks(c, "pfp::build_keys_kernel", m * (8 + 8 + 8 + 24));
        hipLaunchKernelGGL(build_keys_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, g, m, h, act_i.p, act_grp.p, L, nb, dkey.p, val.p); }
      sort_pairs_db(c, dkey, dkeyo, val, valo, m, 0, keybits);
      std::swap(dkey, dkeyo); std::swap(val, valo);
    } else {
      // the direct placement is decided on before any key is built, and k32 is built only where a sort inside the groups takes it
      if (small_groups()) {
        seg_bufs();
        build_keys32(L);
        if (place_small_groups(k32.p, k32o.p)) kind = Round::DoublingGrouped;
        else small_failed = true;
      }
      if (kind != Round::DoublingGrouped && segmented_worthwhile() && library_segments()) {
        build_keys32(L);
        segsort_pairs_u32<I>(c, k32.p, k32o.p, val.p, valo.p, m, (uint32_t)ngrp, segb.p, sege.p, 0, bits_for(N));
        kind = Round::DoublingGrouped;
      }
      if (kind != Round::DoublingGrouped) {
        { KScope ks(c, "pfp::build_keys_kernel", m * (4 + 4 + 4 + 12));
          hipLaunchKernelGGL(build_keys_kernel<I>, gdim(blocks(m)), gdim(TB), 0, c->stream, g, m, h, act_i.p, act_grp.p, L, nb, key.p, val.p); }
        sort_device_wide(keybits);
      }
    }
    h *= 2;
    out.rounds++;
  }

  // choose and run the next round; false: only a doubling round could go on, and this is a list of suffixes
  bool next_round() {
    if (dict_pivot_wanted()) { dict_pivot_round(); return true; }
    if constexpr (!kWide) {
      if (parse_pivot_wanted() && parse_pivot_round()) return true;
    }
    if (list_mode) { out.complete = false; return false; }     // doubling would read ranks of suffixes outside the list
    prepare_ranks_for_doubling();
    doubling_round();
    return true;
  }
};

template <class I>
static void doubling(pfp_ctx *c, SufGeom g, DBuf<uint64_t> &key, DBuf<I> &val, uint64_t h0, SuffixOrderT<I> &out, const DoublingOpts &o) {
  // precondition: key/val hold the initial (prefix key, position) pairs of the N suffixes to sort: all
  // g.N positions, or (range mode, o.list_len given) the ones of this rank's key range
  Rounds<I> r(c, g, key, val, h0, out, o);
  out.N = r.N; out.NP = r.NP; out.range = r.range_mode; out.complete = true;
  out.rounds = 0;
  if (r.N == 0) { out.sa.alloc(c, 1); out.grp.alloc(c, 8); out.rank.alloc(c, 1); return; }
  r.first_round_sort();
  SortTag later_tag(g.mode == MODE_DICT ? "dictionary, later rounds" : "parse, later rounds");
  r.start_rounds();
  for (;;) {
    r.regroup();
    r.judge_pivot_round();
    r.next_list();
    if (r.m == 0 || r.try_finisher() || !r.next_round()) break;
    r.tile_last.release(); r.tile_scan.release();      // (the first round's, kept until its successor is sorted)
  }
  // PFP_DEBUG validates the rank of every position: fill in what the pivot rounds left out
  if (c->debug && out.complete && !r.range_mode) r.repair_ranks(0, nullptr);
  if (r.rank_alloc) out.wordrank.release();      // every rank is in rank[]
}

template <class I>
__global__ void gather_ranks_kernel(RankViewT<I> L, uint64_t count, const uint64_t *__restrict__ pos, I *__restrict__ out) {
  uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  bool settled;
  if (a >= count) return;
  if (L.wordrank) {      // pos[] are the word starts, in word order: the whole words a later round settled reported here
    const I r = L.wordrank[a];
    if (r != IdxTraits<I>::kNone) { out[a] = r & ~L.finbit; return; }
  }
  out[a] = rank_at(L, pos[a], settled);
}
template <class I>
void gather_ranks(pfp_ctx *c, const SuffixOrderT<I> &so, const uint64_t *d_pos, uint64_t count, I *d_out) {
  if (!count) return;
  hipLaunchKernelGGL(gather_ranks_kernel<I>, gdim(cdiv(count, 256)), gdim(256), 0, c->stream, rank_view(so), count, d_pos, d_out);
  PFP_HIP(hipGetLastError());
}
template void gather_ranks<uint32_t>(pfp_ctx *, const SuffixOrderT<uint32_t> &, const uint64_t *, uint64_t, uint32_t *);
template void gather_ranks<uint64_t>(pfp_ctx *, const SuffixOrderT<uint64_t> &, const uint64_t *, uint64_t, uint64_t *);

// ---- whole-array entry points: first-round keys for all N positions, then doubling()

// low_counts (optional): how often the bytes 0x00 and 0x01 occur
static KeyCode dict_key_code(pfp_ctx *c, const uint8_t *bytes, uint64_t N, double rep_hint, const SorterSwitches &sw,
                             uint64_t *low_counts = nullptr) {
  DBuf<unsigned long long> hist(c, 256);
  hist.zero();
  hipLaunchKernelGGL(byte_histogram_kernel, gdim(std::min<uint64_t>(cdiv64(N, 4096), (uint64_t)c->n_cu * 8)), gdim(256), 0,
                     c->stream, bytes, N, hist.p);
  std::vector<uint64_t> hh(256);
  PFP_HIP(hipMemcpyAsync(hh.data(), hist.p, 2048, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  if (low_counts) { low_counts[0] = hh[0]; low_counts[1] = hh[1]; }
  return make_key_code(hh.data(), rep_hint, sw);
}

// keys-only first round (see sort_dict_suffixes): index bits of the combined word, 0 = sort (key, position) pairs;
// shortens kc's key to what is left of 64 bits
template <class I>
static int keysonly_bits(uint64_t N, double rep_hint, const SorterSwitches &sw, KeyCode &kc) {
  if (!(sizeof(I) == 4 && N >= 2 && (sw.keysonly == 1 || (sw.keysonly != 0 && rep_hint >= 2.0 && N >= (1u << 20))))) return 0;
  const int ib = bits_for(N - 1);
  int width = 64 - ib;                      // key bits incl. the terminator flag
  if (width > 3 * kKeysDigitBits && width % kKeysDigitBits <= 2) width -= width % kKeysDigitBits;       // a radix pass for one or two bits is a whole pass
  // (measured: 36 key bits on 129 M suffixes - first sort 7.8 -> 3.9 ms, same rounds after it; 31 key bits on 1.7 G
  //  suffixes leave three times as many unresolved after the first pivot round - the pair sort stays there)
  if (!(width - 1 >= 35 || sw.keysonly == 1)) return 0;
  if (kc.kbits > width - 1) { kc.kbits = std::max(8, width - 1); kc.hmin = std::max(1, std::min(32, kc.kbits / kc.maxlen)); }
  return ib;
}

template <class I>
static void require_dict_size(uint64_t N) {
  PFP_REQUIRE(N >= 1 && (sizeof(I) == 8 ? N < (1ull << 40) : N < 0xFFFFFFF0ull), PFP_ELIMIT,
              sizeof(I) == 8 ? "dictionary of 2^40 bytes or more" : "dictionary too large for 32-bit suffix indices");
}
static uint64_t dict_keymask(const KeyCode &kc) { return kc.kbits + 1 >= 64 ? ~0ull : ((1ull << (kc.kbits + 1)) - 1); }

// what follows the first-round keys of a dictionary, of all its positions or of a list of them (list_len): what the merge reads
// of the key code, then the rounds
template <class I>
static void dict_rounds(pfp_ctx *c, const SufGeom &g, const uint8_t *bytes, const KeyCode &kc, int idx_bits, std::optional<uint64_t> list_len,
                        DBuf<uint64_t> &key, DBuf<I> &val, SuffixOrderT<I> &out, const SorterSwitches &sw, bool whole_list = false) {
  out.keymask = dict_keymask(kc);
  out.lut.alloc(c, 256);
  PFP_HIP(hipMemcpyAsync(out.lut.p, kc.lut, 1024, hipMemcpyHostToDevice, c->stream));
  sync(c);      // kc may be a stack object of the caller
  out.bytes = bytes; out.kbits = kc.kbits;
  DoublingOpts o(sw);
  o.key_bits = kc.kbits + 1, o.dict = true, o.list_len = list_len, o.whole_list = whole_list, o.idx_bits = idx_bits;
  doubling<I>(c, g, key, val, (uint64_t)kc.hmin, out, o);
}

template <class I>
void sort_dict_suffixes(pfp_ctx *c, const uint8_t *bytes, uint64_t N, const WordView &wv, SuffixOrderT<I> &out,
                        const SlotPayloadSrc *pay, int min_len) {
  require_dict_size<I>(N);
  const SorterSwitches sw = sorter_switches();
  SufGeom g{MODE_DICT, N, wv};
  // Only the suffixes longer than min_len.  The placement of their keys (init_keys_packed_kernel) needs a dictionary in which
  // every word is longer than min_len - checked by short_words_kernel while the byte histogram is read back - and in which
  // the only bytes below 2 are the d terminators and the final 0x00 - read off that histogram: a parse makes no other, but
  // pfp_merge is handed a file whose bytes nobody looked at.  Then every word has exactly min_len + 1 positions that are not
  // kept, and the final 0x00 is one more.  Anything else is sorted whole.
  const uint64_t ntile = cdiv64(N, kKeyPos);
  const uint64_t dropped = (uint64_t)wv.d * ((uint64_t)min_len + 1) + 1;
  bool listed = min_len > 0 && wv.d >= 1 && dropped < N && sw.drop_short;
  unsigned long long *const short_found = reinterpret_cast<unsigned long long *>(c->h_scalars + 3);
  if (listed) {
    *short_found = 0;
    KScope ks(c, "pfp::short_words_kernel", (uint64_t)wv.d * 8);
    hipLaunchKernelGGL(short_words_kernel, gdim(cdiv((uint64_t)wv.d, 256)), gdim(256), 0, c->stream, wv, min_len, short_found);
  }
  uint64_t low_counts[2] = {0, 0};
  KeyCode kc = dict_key_code(c, bytes, N, out.rep_hint, sw, low_counts);      // (syncs)
  if (listed && (*short_found != 0 || low_counts[0] != 1 || low_counts[1] != (uint64_t)wv.d)) {
    listed = false;
    if (sw.trace_rounds)
      fprintf(stderr, "[pfp] dictionary with a word of at most %d bytes or a stray byte below 2: every position is sorted\n", min_len);
  }
  const uint64_t n = listed ? N - dropped : N;
  // Keys-only first round.  A dictionary of a repetitive collection (text / dictionary >= 2) is mostly families of
  // variants that no first-round key separates, whatever its width: the first round only has to bring the families
  // together.  Then the position fits into the same 64-bit word as a (shorter) key, the sort moves 16 bytes per
  // element and pass instead of 24 and makes 4-5 passes instead of 7, and the merge records in the key's spare bits
  // (which such an input hardly uses: most slots are re-ordered later) are given up.
  const int idx_bits = keysonly_bits<I>(N, out.rep_hint, sw, kc);      // (index bits hold a POSITION: by N also where fewer are sorted)
  DBuf<uint64_t> key(c, n);
  DBuf<I> val;
  if (!idx_bits) val.alloc(c, n);
  out.paybits = (pay && !idx_bits && kc.kbits + 1 <= 48) ? 16 : 0;
  { KScope ks(c, "pfp::init_keys_packed_kernel", N + n * (8 + (idx_bits ? 0 : sizeof(I)) + (out.paybits ? 9 : 0)));
    hipLaunchKernelGGL(init_keys_packed_kernel<I>, gdim((unsigned)ntile), gdim(256), 0, c->stream, bytes, N, kc,
                       pay ? *pay : SlotPayloadSrc{}, out.paybits, key.p, val.p, idx_bits, wv, min_len, listed ? n : (uint64_t)0); }
  if (c->debug) {
    DBuf<unsigned long long> bad(c, 1);
    bad.zero();
    hipLaunchKernelGGL(check_keys_kernel<I>, gdim(cdiv(n, 256)), gdim(256), 0, c->stream, bytes, n, kc, key.p, val.p, dict_keymask(kc), bad.p,
                       idx_bits, listed ? 1 : 0, wv, min_len);
    PFP_HIP(hipMemcpyAsync(c->h_scalars, bad.p, 8, hipMemcpyDeviceToHost, c->stream));
    sync(c);
    PFP_REQUIRE(c->h_scalars[0] == 0, PFP_EHIP, "bit-stream keys differ from packed_key_at at " + std::to_string(c->h_scalars[0]) + " positions");
  }
  if (!listed) { dict_rounds<I>(c, g, bytes, kc, idx_bits, std::nullopt, key, val, out, sw); return; }
  dict_rounds<I>(c, g, bytes, kc, idx_bits, n, key, val, out, sw, true);
  if (out.complete) return;
  // A group was left that only a doubling round settles, and that round reads the rank of positions that may not be listed:
  // the list's result is dropped and every position sorted, once.  (Deterministic and rare: a dictionary of a parse is
  // settled by the first round and pivot rounds.  The kernel trace shows it: short_words_kernel ran, and the first round twice.)
  if (sw.trace_rounds) fprintf(stderr, "[pfp] the sort of the %llu suffixes longer than %d bytes needs a doubling round: every position is sorted\n",
                                    (unsigned long long)n, min_len);
  key.release(); val.release();
  const double rep_hint = out.rep_hint;
  out = SuffixOrderT<I>{};
  out.rep_hint = rep_hint;
  sort_dict_suffixes<I>(c, bytes, N, wv, out, pay, 0);
}
template void sort_dict_suffixes<uint32_t>(pfp_ctx *, const uint8_t *, uint64_t, const WordView &, SuffixOrderT<uint32_t> &, const SlotPayloadSrc *, int);
template void sort_dict_suffixes<uint64_t>(pfp_ctx *, const uint8_t *, uint64_t, const WordView &, SuffixOrderT<uint64_t> &, const SlotPayloadSrc *, int);

// (Tried in round 3 and removed: "grouped order without sorting duplicates".  Equal suffixes of a dictionary of variants can be
//  read off the WORDS: sort the d words by their reversed strings, keep the longest common suffix lcs[r] of neighbours; the
//  suffix of length L of the word at rank r duplicates its left neighbour's iff lcs[r] >= L, so only one representative per
//  distinct string (71 M of 129 M suffixes on the 64-copy workload) is suffix-sorted - as a list - and every sorted
//  representative is expanded into its run of words.  Bit-exact on all goldens, half the peak memory (12.6 GB input: 165 ->
//  90 GB) - and slower: the dictionary sort went 20.0 -> 22.2 ms (64 copies) and 354 -> 434 ms (1024 copies).  The first
//  round shrinks (radix 3.8 -> 2.2 ms, pivot 6.8 -> 4.9 ms), but with the identical strings gone every remaining tie is a real
//  difference: 7 rounds instead of 5 (23 pivot launches instead of 7 on 1024 copies), and finding the runs and laying out
//  the slots costs 4.5 ms / 87 ms.  It would pay if the MERGE worked on the 71 M groups instead of 129 M slots (sums over
//  a run from prefix sums, "all chars equal" from a range minimum over lcs[]): DESIGN.md 7b.)

template <class I>
void sort_byte_suffixes(pfp_ctx *c, const uint8_t *bytes, uint64_t N, SuffixOrderT<I> &out) {
  PFP_REQUIRE(N >= 1 && (sizeof(I) == 8 ? N < (1ull << 40) : N < 0xFFFFFFF0ull), PFP_ELIMIT, "text too large for the suffix index width");
  SufGeom g{MODE_PLAIN, N, WordView{}};
  DBuf<uint64_t> key(c, N);
  DBuf<I> val(c, N);
  { KScope ks(c, "pfp::init_keys_bytes_kernel", N * (16 + sizeof(I)));
    hipLaunchKernelGGL(init_keys_bytes_kernel<I>, gdim(cdiv(N, 256)), gdim(256), 0, c->stream, bytes, N, key.p, val.p); }
  doubling<I>(c, g, key, val, 8, out, DoublingOpts(sorter_switches()));
}
template void sort_byte_suffixes<uint32_t>(pfp_ctx *, const uint8_t *, uint64_t, SuffixOrderT<uint32_t> &);
template void sort_byte_suffixes<uint64_t>(pfp_ctx *, const uint8_t *, uint64_t, SuffixOrderT<uint64_t> &);

// First-round keys of an integer string, for both integer sorters: the symbol-width check, g.dist for the pivot rounds where the
// caller wants it, key[] and val[] for all N positions.  The caller holds the IntKeys while it sorts and names the trace scopes
// that differ between the entry points, so that each one's rows stay its own (dist_scope null: none).  What the caller has
// allocated itself is not allocated here: each entry point keeps the order of its requests to the pool, which hands out its cached
// blocks by that order - the buffers of a sort lie where they lay when each sorter had its own setup.
struct IntKeys {
  DBuf<uint32_t> mx, dist, val;      // (mx: the largest symbol and the equal-neighbours flag; held with the rest, as it always has been: the pool's peak counts it)
  DBuf<uint64_t> key;
  int key_bits = 64;                 // the keys' width, for DoublingOpts::key_bits
};
// narrow_ok: the caller sorts the keys as doubling() does and reads them for order and equality only, so a string without equal
// neighbours may get the two-symbol key of 2 sb bits (init_keys_int_run_kernel) instead of the 64-bit run key.  PFP_PARSE_KEYBITS=0
// (tests and measurements switch it) keeps the run key.
static void int_first_keys(pfp_ctx *c, SufGeom &g, const uint32_t *sym, uint64_t N, uint32_t max_sym, const uint32_t *occ, uint32_t n_sym,
                           bool want_dist, const char *dist_scope, const char *plain_scope, uint64_t plain_bytes, bool narrow_ok,
                           const SorterSwitches &sw, IntKeys &k) {
  // the symbol width is measured, not taken on trust (max_sym is only an upper bound for the check)
  auto need = [&](auto &b) { if (!b.p) b.alloc(c, N); };
  k.mx.alloc(c, 2);
  k.mx.zero();
  hipLaunchKernelGGL(max_u32_kernel, gdim((int)std::min<uint64_t>(cdiv64(N, 256), 1024)), gdim(256), 0, c->stream, sym, N, k.mx.p);
  const uint64_t mx2 = read_scalar(c, reinterpret_cast<const uint64_t *>(k.mx.p));      // (one read-back for both words)
  const uint32_t real_max = (uint32_t)mx2;
  const bool has_pair = (mx2 >> 32) != 0;
  PFP_REQUIRE(real_max <= max_sym, PFP_EFORMAT, "integer string holds a symbol above its alphabet size");
  const int sb = bits_for(real_max);
  g.sym = sym;
  std::optional<KScope> ks;
  // occ[x - 1] = occurrences of symbol x (the parse: the words' counts): rare = fewer than the mean; dist[] for the pivot rounds
  if (want_dist) {
    if (dist_scope) ks.emplace(c, dist_scope, N * 24);      // (+ rare_marks_kernel and the running maximum between them)
    DBuf<uint32_t> mk(c, N), pm(c, N);
    need(k.dist);
    const uint32_t below = (uint32_t)std::max<uint64_t>(2, N / n_sym);
    hipLaunchKernelGGL(rare_marks_kernel, gdim(cdiv(N, 256)), gdim(256), 0, c->stream, sym, (uint32_t)N, occ, n_sym, below, mk.p);
    inclusive_max_u32(c, mk.p, pm.p, N);
    hipLaunchKernelGGL(rare_dist_kernel, gdim(cdiv(N, 256)), gdim(256), 0, c->stream, (uint32_t)N, pm.p, k.dist.p);
    g.dist = k.dist.p;
    ks.reset();
  }
  need(k.key);
  need(k.val);
  const char *layout = "plain";
  if (64 - 2 * sb >= 6) {
    if (narrow_ok && !has_pair && sw.parse_keybits) {
      // no run ends to find: no marks, no running maximum, no N-long temporaries; the same kernel under the same label
      ks.emplace(c, "pfp::init_keys_int_run_kernel", N * 16);
      hipLaunchKernelGGL(init_keys_int_run_kernel, gdim(cdiv(N, 256)), gdim(256), 0, c->stream, sym, (uint32_t)N, (const uint32_t *)nullptr, sb,
                         k.key.p, k.val.p);
      k.key_bits = 2 * sb;
      layout = "two symbols";
    } else {
      ks.emplace(c, "pfp::init_keys_int_run_kernel", N * 28);      // (+ run_marks_kernel and its running maximum)
      DBuf<uint32_t> v(c, N), pm(c, N);
      hipLaunchKernelGGL(run_marks_kernel, gdim(cdiv(N, 256)), gdim(256), 0, c->stream, sym, (uint32_t)N, v.p);
      inclusive_max_u32(c, v.p, pm.p, N);
      hipLaunchKernelGGL(init_keys_int_run_kernel, gdim(cdiv(N, 256)), gdim(256), 0, c->stream, sym, (uint32_t)N, pm.p, sb, k.key.p,
                         k.val.p);
      layout = "run";
    }
  } else {
    ks.emplace(c, plain_scope, plain_bytes);
    hipLaunchKernelGGL(init_keys_int_kernel, gdim(cdiv(N, 256)), gdim(256), 0, c->stream, sym, N, k.key.p, k.val.p);
  }
  // (the tests tell the layouts apart by this line)
  if (sw.trace_rounds)
    fprintf(stderr, "[pfp] integer first-round keys N=%llu sb=%d: %s layout, sorted bits [0, %d)\n", (unsigned long long)N, sb, layout, k.key_bits);
}

void sort_int_suffixes(pfp_ctx *c, const uint32_t *sym, uint64_t N, SuffixOrder &out, uint32_t max_sym, const uint32_t *occ,
                       uint32_t n_sym) {
  PFP_REQUIRE(N >= 1 && N < 0xFFFFFFF0ull, PFP_ELIMIT, "parse too large for 32-bit suffix indices");
  SufGeom g{MODE_PLAIN, N, WordView{}};
  const SorterSwitches sw = sorter_switches();
  IntKeys k;
  k.key.alloc(c, N);
  k.val.alloc(c, N);
  int_first_keys(c, g, sym, N, max_sym, occ, n_sym, occ && n_sym && N >= sw.parse_pivot_min, nullptr, "pfp::init_keys_int_kernel", N * (8 + 8 + 4), true,
                 sw, k);
  DoublingOpts o(sw);
  o.key_bits = k.key_bits;
  doubling<uint32_t>(c, g, k.key, k.val, 2, out, o);
}

// ---- one rank's share of a suffix array (multi-GPU chain): the suffixes of one key range out of `parts`.  First what the two share
// sorters have in common (share_splitters, select_share), then the dictionary's kernels and sorter with gather_slots_range, then the parse's.
// The splitters: every stride-th suffix's first-round key, sorted; the same on every rank.  `sample(stride, ns, key, val)`
// launches the caller's kernel, which writes the ns sample keys and val[k] = k.  Part q starts at the sample q ns / parts.
struct Splitters {
  std::vector<uint64_t> hs;          // the sample keys, ascending
  std::vector<uint32_t> hv;          // the sample each of them came from (where the caller asked for that)
  uint64_t klo = 0, khi = ~0ull;     // this part's keys: [klo, khi), no upper bound where khi_open
  int khi_open = 1;
};
template <class Sample>
static Splitters share_splitters(pfp_ctx *c, uint64_t N, uint32_t part, uint32_t parts, bool want_idx, Sample &&sample) {
  Splitters sp;
  sp.khi_open = part + 1 == parts ? 1 : 0;
  if (parts <= 1) return sp;
  const uint32_t ns = (uint32_t)std::min<uint64_t>(N, 1u << 16);
  DBuf<uint64_t> sk(c, ns), sko(c, ns);
  DBuf<uint32_t> sv(c, ns), svo(c, ns);
  sample(N / ns, ns, sk.p, sv.p);
  sort_pairs_u64_u32(c, sk.p, sko.p, sv.p, svo.p, ns, 0, 64);
  sp.hs.resize(ns);
  PFP_HIP(hipMemcpyAsync(sp.hs.data(), sko.p, (size_t)ns * 8, hipMemcpyDeviceToHost, c->stream));
  if (want_idx) {
    sp.hv.resize(ns);
    PFP_HIP(hipMemcpyAsync(sp.hv.data(), svo.p, (size_t)ns * 4, hipMemcpyDeviceToHost, c->stream));
  }
  sync(c);
  if (part > 0) sp.klo = sp.hs[(uint64_t)part * ns / parts];
  if (part + 1 < parts) sp.khi = sp.hs[(uint64_t)(part + 1) * ns / parts];
  return sp;
}

__global__ __launch_bounds__(256) void sum2_u64_kernel(const unsigned long long *__restrict__ a, const unsigned long long *__restrict__ b,
                                                       uint64_t n, unsigned long long *__restrict__ out) {
  __shared__ unsigned long long ws[2][4];
  unsigned long long x = 0, y = 0;
  for (uint64_t i = (uint64_t)BID * 256 + threadIdx.x; i < n; i += (uint64_t)GDIM * 256) { x += a[i]; y += b[i]; }
  for (int o = 32; o > 0; o >>= 1) { x += __shfl_down(x, o, 64); y += __shfl_down(y, o, 64); }
  if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = x; ws[1][threadIdx.x >> 6] = y; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(out, ws[0][0] + ws[0][1] + ws[0][2] + ws[0][3]);
    atomicAdd(out + 1, ws[1][0] + ws[1][1] + ws[1][2] + ws[1][3]);
  }
}
// the end of a flag pass: its per-tile sums added up, sums[0] += a[0..n), sums[1] += b[0..n).  The pass calls it itself, inside its
// own trace scope and while it holds the tile sums (the dictionary's go back to the pool before the flags are counted).
static void sum_tiles(pfp_ctx *c, const unsigned long long *a, const unsigned long long *b, uint64_t n, unsigned long long *sums) {
  hipLaunchKernelGGL(sum2_u64_kernel, gdim((int)std::min<uint64_t>(cdiv64(n, 256), 256)), gdim(256), 0, c->stream, a, b, n, sums);
}

// The share's positions.  `flag_pass(flag, sums)` is the caller's: it sets flag[i] = 1 for the positions of the share and 0 for the
// others, all N of them, has sum_tiles add the number of positions below the share into sums[0], and returns whether sums[1] then
// holds the number of BWT positions the share emits.  The caller holds the ShareList while it sorts.
template <class I>
struct ShareList {
  DBuf<I> idx;                       // the positions, ascending
  uint64_t n = 0, slot_base = 0, range_emits = 0;
  DBuf<unsigned long long> sums;     // the device scalars behind them: held until the sorter returns, as they always have been
  DBuf<uint64_t> cnt_d;              // (1 KiB that the pool's peak counts)
};
// flag_pad: bytes behind the N flags, zeroed.  Nothing reads them (flag_count_kernel and flag_place_kernel stop at N); the parse's
// sorter has always asked for 16, and N + 16 bytes are another request to the pool than N where N mod 512 is 0 or above 496.
template <class I, class FlagPass>
static void select_share(pfp_ctx *c, uint64_t N, size_t flag_pad, FlagPass &&flag_pass, ShareList<I> &sh) {
  DBuf<uint8_t> flag(c, N + flag_pad);
  if (flag_pad) PFP_HIP(hipMemsetAsync(flag.p + N, 0, flag_pad, c->stream));
  sh.sums.alloc(c, 2);
  sh.sums.zero();
  const bool counted = flag_pass(flag.p, sh.sums.p);
  sh.n = count_flags(c, flag.p, N);      // the share's size first: its index list is then exactly that long
  PFP_REQUIRE(sizeof(I) == 8 || sh.n < 0xFFFFFFF0ull, PFP_ELIMIT, "a share of the suffix array too large for 32-bit slots");
  sh.idx.alloc(c, std::max<uint64_t>(sh.n, 1));
  sh.cnt_d.alloc(c, 1);
  select_index<I>(c, flag.p, sh.idx.p, sh.cnt_d.p, N);
  PFP_HIP(hipMemcpyAsync(c->h_scalars + 1, sh.sums.p, 16, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  sh.slot_base = c->h_scalars[1];
  sh.range_emits = counted ? c->h_scalars[2] : 0;
}
template <class I>
static void set_share(SuffixOrderT<I> &out, const Splitters &sp, const ShareList<I> &sh) {
  out.slot_base = sh.slot_base; out.klo = sp.klo; out.khi = sp.khi_open ? ~0ull : sp.khi; out.range_emits = sh.range_emits;
}

// -- the dictionary's share
__global__ void sample_keys_kernel(const uint8_t *__restrict__ s, uint64_t N, uint64_t stride, uint32_t ns, KeyCode kp,
                                   uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
  __shared__ uint32_t lut[256];
  lut[threadIdx.x] = kp.lut[threadIdx.x];
  __syncthreads();
  const uint32_t k = BID * 256 + threadIdx.x;
  if (k >= ns) return;
  const uint64_t i = (uint64_t)k * stride;
  key[k] = i < N ? packed_key_at(s, i, kp.kbits, lut) : ~0ull;
  val[k] = k;
}
// The same selection without a key per position.  A share of the suffix array only has to be a contiguous range of the final
// order, and "is this suffix below that one" is a string comparison: the suffix at i against the suffix at a boundary position,
// 16 bytes at a time - decided at the first byte for three positions in four (DNA), never more than kRangeCmp bytes: a suffix that
// equals the boundary's that far goes to the upper side whichever way it would end (the suffixes that share 64 bytes with the
// boundary stand together in the order, so the cut just moves below them: still one cut, the same on both sides of it).
// Identical strings of different words (both reach their terminator) are a tie: upper side, never split.
// 8.7 -> ~2 ms for the 0.9 G positions of the 8-rank union dictionary (the key kernel codes every character of every position).
constexpr int kRangeCmp = 64;
__device__ __forceinline__ int cmp_suffix_boundary(const uint8_t *__restrict__ s, uint64_t i, uint64_t b) {
  if (i == b) return 0;
#pragma unroll 1
  for (int q = 0; q < kRangeCmp / 16; q++) {
    const uint4 x = ld16u(s + i + 16 * q), y = ld16u(s + b + 16 * q);
    int r = cmp_term8((uint64_t)x.x | ((uint64_t)x.y << 32), (uint64_t)y.x | ((uint64_t)y.y << 32));
    if (r == kCmpOn) r = cmp_term8((uint64_t)x.z | ((uint64_t)x.w << 32), (uint64_t)y.z | ((uint64_t)y.w << 32));
    if (r != kCmpOn) return r;
  }
  return 0;      // equal for kRangeCmp bytes: upper side
}
// the same with four consecutive positions per thread: their heads come out of five ALIGNED dwords (byte shifts) instead of four
// unaligned 16-byte loads and four byte loads, the four flags leave as one dword - the one-position form is bound by its byte-wide
// memory instructions, not by the compares.  1024 positions per workgroup.
// (cmp_words16: the first 16 bytes of both suffixes in registers, two 64-bit words each; the full compare only where they do not decide)
__device__ __forceinline__ int cmp_words16(uint64_t x0, uint64_t x1, uint64_t y0, uint64_t y1, const uint8_t *__restrict__ s, uint64_t i, uint64_t b) {
  int r = cmp_term8(x0, y0);
  if (r == kCmpOn) r = cmp_term8(x1, y1);
  return r != kCmpOn ? r : i == b ? 0 : cmp_suffix_boundary(s, i, b);      // (16 equal bytes: rare)
}
__global__ __launch_bounds__(256) void range_flags_cmp4_kernel(const uint8_t *__restrict__ s, uint64_t N, uint64_t b_lo, int has_lo,
                                                               uint64_t b_hi, int has_hi, SlotPayloadSrc count, int want_count,
                                                               uint8_t *__restrict__ flag, unsigned long long *__restrict__ tile_below,
                                                               unsigned long long *__restrict__ tile_emits) {
  __shared__ unsigned long long wsum[2][4];
  __shared__ uint32_t wt[4];
  const uint64_t B0 = (uint64_t)BID * 1024;
  if (B0 >= N) return;      // a workgroup of the padded last grid row
  const uint64_t p0 = B0 + (uint64_t)threadIdx.x * 4;
  const int lane = threadIdx.x & 63, wvi = threadIdx.x >> 6;
  // bytes [p0, p0 + 20): the dictionary is padded with 64 zero bytes, so the loads of the last positions stay inside it
  uint32_t d[5] = {0u, 0u, 0u, 0u, 0u};
  if (p0 < N) {
    const uint4 v = ld16u(s + p0);
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    d[4] = *reinterpret_cast<const uint32_t *>(s + p0 + 16);
  }
  const uint4 lo4 = has_lo ? ld16u(s + b_lo) : make_uint4(0u, 0u, 0u, 0u), hi4 = has_hi ? ld16u(s + b_hi) : make_uint4(0u, 0u, 0u, 0u);
  const uint64_t lo0 = (uint64_t)lo4.x | ((uint64_t)lo4.y << 32), lo1 = (uint64_t)lo4.z | ((uint64_t)lo4.w << 32);
  const uint64_t hi0 = (uint64_t)hi4.x | ((uint64_t)hi4.y << 32), hi1 = (uint64_t)hi4.z | ((uint64_t)hi4.w << 32);
  uint32_t tmask = 0, fl = 0, below = 0, minemask = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint64_t i = p0 + k;
    if (i >= N) break;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; j++) w[j] = k ? ((d[j] >> (8 * k)) | (d[j + 1] << (32 - 8 * k))) : d[j];
    const uint64_t x0 = (uint64_t)w[0] | ((uint64_t)w[1] << 32), x1 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    if ((w[0] & 0xffu) == (uint32_t)kEndOfWord) tmask |= 1u << k;
    const int cl = !has_lo ? 1 : cmp_words16(x0, x1, lo0, lo1, s, i, b_lo);
    if (cl < 0) below++;
    const bool mine = cl >= 0 && (!has_hi || cmp_words16(x0, x1, hi0, hi1, s, i, b_hi) < 0);
    if (mine) { fl |= 1u << (8 * k); minemask |= 1u << k; }
  }
  if (p0 + 4 <= N) *reinterpret_cast<uint32_t *>(flag + p0) = fl;
  else for (int k = 0; k < 4 && p0 + k < N; k++) flag[p0 + k] = (uint8_t)((fl >> (8 * k)) & 1u);
  // terminators before this thread's positions in the block (only the emit count of the share's own positions wants them)
  uint32_t tc = (uint32_t)__popc(tmask), inc = tc;
  for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
  if (lane == 63) wt[wvi] = inc;
  __syncthreads();
  unsigned long long emits = 0;
  if (minemask && want_count) {
    uint32_t before = inc - tc;
    for (int q = 0; q < wvi; q++) before += wt[q];
    const uint32_t wbase = count.wv.blk_word[B0 >> 6] + before;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if ((minemask >> k) & 1u) {
        const uint32_t wd = wbase + (uint32_t)__popc(tmask & ((1u << k) - 1u));
        if (wd < count.wv.d && count.wv.wend[wd] - (p0 + k) > (uint64_t)count.w) emits += count.wocc[wd];
      }
  }
  unsigned long long cnt = below;
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
  if (__ballot(emits != 0)) for (int o = 32; o > 0; o >>= 1) emits += __shfl_down(emits, o, 64);
  if (lane == 0) { wsum[0][wvi] = cnt; wsum[1][wvi] = emits; }
  __syncthreads();
  if (threadIdx.x == 0) {
    tile_below[BID] = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
    tile_emits[BID] = wsum[1][0] + wsum[1][1] + wsum[1][2] + wsum[1][3];
  }
}
template <class I>
__global__ __launch_bounds__(256) void init_keys_list_kernel(const uint8_t *__restrict__ s, uint64_t n, KeyCode kp,
                                                             const I *__restrict__ idx,
                                                             uint64_t *__restrict__ key, I *__restrict__ val, int idx_bits) {
  __shared__ uint32_t lut[256];
  lut[threadIdx.x] = kp.lut[threadIdx.x];
  __syncthreads();
  uint64_t a = (uint64_t)BID * 256 + threadIdx.x;
  if (a >= n) return;
  const I i = idx[a];
  const uint64_t k = packed_key_at(s, i, kp.kbits, lut);
  if (idx_bits) { key[a] = (k << idx_bits) | (uint64_t)i; return; }      // keys-only sort (the list is in position order)
  key[a] = k; val[a] = i;
}

template <class I>
void sort_dict_suffixes_range(pfp_ctx *c, const uint8_t *bytes, uint64_t N, const WordView &wv, uint32_t part,
                              uint32_t parts, SuffixOrderT<I> &out, const SlotPayloadSrc *pay, const SlotPayloadSrc *count) {
  require_dict_size<I>(N);
  PFP_REQUIRE(parts >= 1 && part < parts, PFP_EINVAL, "bad key-range share");
  const SorterSwitches sw = sorter_switches();
  SufGeom g{MODE_DICT, N, wv};
  KeyCode kc = dict_key_code(c, bytes, N, out.rep_hint, sw);
  const int idx_bits = keysonly_bits<I>(N, out.rep_hint, sw, kc);      // (before the splitters: every rank cuts the same keys)
  // splitters: every stride-th suffix's key, sorted; the same on every rank.  The share is cut by comparing every suffix with the
  // boundary SUFFIXES (range_flags_cmp4_kernel) - boundaries with distinct keys, so that they stand in the order they are used in
  // (the two earlier forms - a first-round key per position, one position per thread - went with round 4)
  const Splitters sp = share_splitters(c, N, part, parts, true, [&](uint64_t stride, uint32_t ns, uint64_t *sk, uint32_t *sv) {
    hipLaunchKernelGGL(sample_keys_kernel, gdim(cdiv(ns, 256)), gdim(256), 0, c->stream, bytes, N, stride, ns, kc, sk, sv);
  });
  // boundary of part q (q >= 1): the sample at q ns / parts - or the boundary before it, if that sample's key is no larger
  // (equal keys do not say which suffix is the smaller: such a part holds nothing)
  auto boundary = [&](uint32_t q, uint64_t &pos) {
    uint64_t prev_key = 0; bool have = false;
    for (uint32_t t = 1; t <= q; t++) {
      const uint64_t ns = sp.hs.size(), at = (uint64_t)t * ns / parts;
      if (!have || sp.hs[at] > prev_key) { pos = (uint64_t)sp.hv[at] * (N / ns); prev_key = sp.hs[at]; have = true; }
    }
    return have;
  };
  uint64_t b_lo = 0, b_hi = 0;
  const bool has_lo = part > 0 && boundary(part, b_lo), has_hi = part + 1 < parts && boundary(part + 1, b_hi);
  ShareList<I> sh;
  select_share<I>(c, N, 0, [&](uint8_t *flag, unsigned long long *sums) {
    const uint64_t nblk = cdiv64(N, 1024);
    DBuf<unsigned long long> tb(c, nblk), te(c, nblk);
    KScope ks(c, "pfp::range_flags_cmp4_kernel", N * 2);
    hipLaunchKernelGGL(range_flags_cmp4_kernel, gdim((unsigned)nblk), gdim(256), 0, c->stream, bytes, N, b_lo, has_lo ? 1 : 0, b_hi,
                       has_hi ? 1 : 0, count ? *count : SlotPayloadSrc{}, count ? 1 : 0, flag, tb.p, te.p);
    sum_tiles(c, tb.p, te.p, nblk, sums);
    return true;      // (zeros where no count was asked for)
  }, sh);
  // the suffixes of a LIST of positions (ascending) sorted among themselves: first-round keys position by position, then the
  // rounds of doubling() in its range mode (no rank per dictionary position; out.complete == false where only a doubling
  // round - ranks of suffixes outside the list - could go on).
  const uint64_t n = sh.n;
  DBuf<uint64_t> key(c, std::max<uint64_t>(n, 1));
  DBuf<I> val;
  if (!idx_bits) val.alloc(c, std::max<uint64_t>(n, 1));
  out.paybits = 0;
  if (n) {
    KScope ks(c, "pfp::init_keys_list_kernel", (uint64_t)n * 17);
    hipLaunchKernelGGL(init_keys_list_kernel<I>, gdim(cdiv(n, 256)), gdim(256), 0, c->stream, g.wv.bytes, n, kc, sh.idx.p, key.p, val.p, idx_bits);
  }
  sh.idx.release();
  dict_rounds<I>(c, g, g.wv.bytes, kc, idx_bits, n, key, val, out, sw);
  (void)pay;      // (no merge records in the keys of a share: its positions are a scattered list, every record would be a word lookup)
  set_share(out, sp, sh);
}
template void sort_dict_suffixes_range<uint32_t>(pfp_ctx *, const uint8_t *, uint64_t, const WordView &, uint32_t, uint32_t,
                                                 SuffixOrderT<uint32_t> &, const SlotPayloadSrc *, const SlotPayloadSrc *);
template void sort_dict_suffixes_range<uint64_t>(pfp_ctx *, const uint8_t *, uint64_t, const WordView &, uint32_t, uint32_t,
                                                 SuffixOrderT<uint64_t> &, const SlotPayloadSrc *, const SlotPayloadSrc *);

// range mode: out[word] = 1 + SA(D) slot of the word's whole-word suffix for the words whose suffix lies in this share (the others
// stay 0).  A share keeps no rank per position: it looks at its own slots - the suffix of slot t is a whole word iff the
// byte before it is a terminator - and asks the word lookup which word that is.
template <class I>
__global__ void word_slots_range_kernel(uint64_t N, const I *__restrict__ sa, WordView wv, uint64_t slot_base, uint64_t *__restrict__ out) {
  const uint64_t t = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (t >= N) return;
  const uint64_t i = sa[t];
  if (i != 0 && wv.bytes[i - 1] != kEndOfWord) return;
  const uint32_t wd = word_of(wv, i);
  if (wd < wv.d) out[wd] = slot_base + t + 1;
}
template <class I>
void gather_slots_range(pfp_ctx *c, const SuffixOrderT<I> &so, const WordView &wv, uint64_t count, uint64_t *d_out) {
  if (!count) return;
  PFP_HIP(hipMemsetAsync(d_out, 0, count * 8, c->stream));
  KScope ks(c, "pfp::word_slots_range_kernel", so.N * (sizeof(I) + 1) + count * 8);      // (one random byte per slot)
  if (so.N) hipLaunchKernelGGL(word_slots_range_kernel<I>, gdim(cdiv(so.N, 256)), gdim(256), 0, c->stream, so.N, so.sa.p, wv, so.slot_base, d_out);
  PFP_HIP(hipGetLastError());
}
template void gather_slots_range<uint32_t>(pfp_ctx *, const SuffixOrderT<uint32_t> &, const WordView &, uint64_t, uint64_t *);
template void gather_slots_range<uint64_t>(pfp_ctx *, const SuffixOrderT<uint64_t> &, const WordView &, uint64_t, uint64_t *);

// -- one rank's share of the parse's suffix array.  The parse is replicated, its suffix array was too; with the
// pivot round above a rank can sort the suffixes whose first-round key falls in its range without anybody's ranks, exactly as it
// sorts its share of the dictionary: the same keys for all N positions (a streaming pass), splitters from a deterministic sample
// (identical on every rank), the range's positions as a list, first sort + pivot round + comparison finisher on the list.
// out.complete = false where a doubling round would be needed (the caller then sorts the whole parse as before).
__global__ void sample_u64_kernel(const uint64_t *__restrict__ key, uint64_t stride, uint32_t ns, uint64_t *__restrict__ out, uint32_t *__restrict__ idx) {
  uint32_t j = BID * blockDim.x + threadIdx.x;
  if (j < ns) { out[j] = key[(uint64_t)j * stride]; idx[j] = j; }
}
__global__ __launch_bounds__(256) void range_flags_u64_kernel(const uint64_t *__restrict__ key, uint64_t N, uint64_t klo, uint64_t khi, int khi_open,
                                                              uint8_t *__restrict__ flag, unsigned long long *__restrict__ tile_below) {
  __shared__ unsigned long long ws[4];
  const uint64_t i = (uint64_t)BID * 256 + threadIdx.x;
  unsigned long long lt = 0;
  if (i < N) {
    const uint64_t k = key[i];
    flag[i] = (k >= klo && (khi_open || k < khi)) ? 1 : 0;
    lt = k < klo ? 1ull : 0ull;
  }
  for (int o = 32; o > 0; o >>= 1) lt += __shfl_down(lt, o, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = lt;
  __syncthreads();
  // (per-workgroup sums: an atomic per wave on one address serialises a million of them - 12 ms for 63 M keys)
  if (threadIdx.x == 0 && (uint64_t)BID * 256 < N) tile_below[BID] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ void gather_list_keys_kernel(uint64_t n, const uint32_t *__restrict__ idx, const uint64_t *__restrict__ key,
                                        uint64_t *__restrict__ lkey, uint32_t *__restrict__ lval) {
  const uint64_t a = (uint64_t)BID * blockDim.x + threadIdx.x;
  if (a < n) { const uint32_t i = idx[a]; lkey[a] = key[i]; lval[a] = i; }
}
void sort_int_suffixes_range(pfp_ctx *c, const uint32_t *sym, uint64_t N, uint32_t max_sym, const uint32_t *occ, uint32_t n_sym,
                             uint32_t part, uint32_t parts, SuffixOrder &out) {
  PFP_REQUIRE(N >= 1 && N < 0xFFFFFFF0ull, PFP_ELIMIT, "parse too large for 32-bit suffix indices");
  PFP_REQUIRE(parts >= 1 && part < parts && occ && n_sym, PFP_EINVAL, "bad share of the parse's suffix array");
  const SorterSwitches sw = sorter_switches();
  SufGeom g{MODE_PLAIN, N, WordView{}};
  IntKeys k;
  k.dist.alloc(c, N);
  int_first_keys(c, g, sym, N, max_sym, occ, n_sym, true, "pfp::rare_dist_kernel", "pfp::init_keys_int_run_kernel", N * 28, false, sw, k);
  // (narrow_ok false: the share keeps the 64-bit run key - its splitters and out.klo / out.khi are first-round keys that leave this
  //  function, and every rank and the caller must read them in one layout)
  k.val.release();      // unread: the list's values are gathered from the positions
  const Splitters sp = share_splitters(c, N, part, parts, false, [&](uint64_t stride, uint32_t ns, uint64_t *sk, uint32_t *sv) {
    hipLaunchKernelGGL(sample_u64_kernel, gdim(cdiv(ns, 256)), gdim(256), 0, c->stream, k.key.p, stride, ns, sk, sv);
  });
  std::optional<KScope> ks_sel;      // (ended before the list is sorted)
  ks_sel.emplace(c, "pfp::range_flags_u64_kernel", N * 10);      // (+ the flag count and the index selection)
  DBuf<unsigned long long> tb;       // (one sum per tile of 256 keys; held until the sorter returns, as it always has been)
  ShareList<uint32_t> sh;
  select_share<uint32_t>(c, N, 16, [&](uint8_t *flag, unsigned long long *sums) {
    const uint64_t nblk = cdiv64(N, 256);
    tb.alloc(c, nblk);
    hipLaunchKernelGGL(range_flags_u64_kernel, gdim(nblk), gdim(256), 0, c->stream, k.key.p, N, sp.klo, sp.khi, sp.khi_open, flag, tb.p);
    sum_tiles(c, tb.p, tb.p, nblk, sums);
    return false;
  }, sh);
  DBuf<uint64_t> lkey(c, std::max<uint64_t>(sh.n, 1));
  DBuf<uint32_t> lval(c, std::max<uint64_t>(sh.n, 1));
  if (sh.n) hipLaunchKernelGGL(gather_list_keys_kernel, gdim(cdiv(sh.n, 256)), gdim(256), 0, c->stream, sh.n, sh.idx.p, k.key.p, lkey.p, lval.p);
  PFP_HIP(hipGetLastError());
  k.key.release(); sh.idx.release();
  ks_sel.reset();
  DoublingOpts o(sw);
  o.list_len = sh.n;
  doubling<uint32_t>(c, g, lkey, lval, 2, out, o);
  set_share(out, sp, sh);
}

}  // namespace pfp

