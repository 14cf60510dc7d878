// api.hpp -- what the extern "C" files (api_*.hip, chain.hip) share: the entry guard, argument checks, the dictionary's suffix
// order in either index width.
#pragma once
#include <new>
#include "kernels.hpp"
#include "prims.hpp"
#include "devutil.hpp"
#include "hostio.hpp"

namespace pfp __attribute__((visibility("hidden"))) {

static constexpr int TB = 256;

// suffix order of the dictionary in the index width the dictionary's size asks for (use_wide_index)
struct DictOrder {
  bool wide = false;
  SuffixOrderT<uint32_t> so32;
  SuffixOrderT<uint64_t> so64;
  template <class I> SuffixOrderT<I> &get() {
    if constexpr (sizeof(I) == 8) return so64; else return so32;
  }
  uint64_t rounds() const { return wide ? so64.rounds : so32.rounds; }
};
// f(I{}) with I = uint64_t (wide) or uint32_t
template <class F> static void with_width(bool wide, F &&f) {
  if (wide) f(uint64_t{}); else f(uint32_t{});
}

inline void check_args(int w, uint64_t p, int flags) {
  PFP_REQUIRE(w >= 4, PFP_EINVAL, "Windows size must be at least 4 (newscan.cpp:537)");
  PFP_REQUIRE(w <= 4096, PFP_EINVAL, "window size above 4096 is not supported");
  PFP_REQUIRE(p >= 10, PFP_EINVAL, "Modulus must be at leas 10 (newscan.cpp:541)");
  PFP_REQUIRE(!((flags & PFP_FLAG_SA) && (flags & (PFP_FLAG_SSA | PFP_FLAG_ESA))), PFP_EINVAL,
              "You can either compute the full SA or a sample of it, not both (bigbwt:59-61)");
  PFP_REQUIRE((flags & ~7) == 0, PFP_EINVAL, "unknown flag bits");
}
inline void check_bwt_rows(uint64_t n_plus_1) {
  PFP_REQUIRE(n_plus_1 <= (1ull << 40), PFP_ELIMIT, "a BWT of more than 2^40 bytes (the limit of the 5-byte .sa format)");
}

void release_debug_state(pfp_ctx *c);      // api_debug.hip: what pfp_stage_text_dev and pfp_scan_k1_enqueue keep in the context

}  // namespace pfp

// Every entry point's body sits between PFP_TRY (or PFP_TRY_DEV, which also makes the context's device the current one) and
// PFP_CATCH: errors become the context's message and a return code.
#define PFP_TRY(ctx) try {                                                                \
  if ((ctx) && !(ctx)->pool.corrupt.empty()) throw ::pfp::Error(PFP_EHIP, (ctx)->pool.corrupt);
#define PFP_TRY_DEV(ctx) PFP_TRY(ctx) PFP_HIP(hipSetDevice((ctx)->device));
#define PFP_CATCH(ctx)                                                                    \
  }                                                                                       \
  catch (const pfp::Error &e) { if (ctx) (ctx)->err = e.what(); (void)hipGetLastError(); return e.code; } \
  catch (const std::bad_alloc &) { if (ctx) (ctx)->err = "host out of memory"; return PFP_ENOMEM; }   \
  catch (const std::exception &e) { if (ctx) (ctx)->err = e.what(); return PFP_EHIP; }
