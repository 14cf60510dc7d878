// chain.hpp -- the pieces of the fused chain (chain.hip) that the stage and multi-GPU entry points use as well.
#pragma once
#include "api.hpp"

namespace pfp __attribute__((visibility("hidden"))) {

struct Chain {
  StagedText tx;
  DBuf<uint64_t> ends;
  uint64_t n_ends = 0, n_used = 0;
  Dictionary D;
  DictIndex ix;
  DictOrder ord;
  DBuf<uint32_t> occ_lex, word_at_rank, sym;
  ParseBWT pb;
  DBuf<uint64_t> sa_own;      // every SA value (-S) when the caller keeps none (host / file entry points)
  BwtOutputs out;             // outputs of the merge; -s / -e with no caller array: SA values at the run boundaries only (out.sa_c)
};

// stage 1 on a staged text: scan, dictionary, dictionary suffix order, lexicographic ranks
void run_parse(pfp_ctx *c, Chain &ch, uint64_t n, int w, uint64_t p, bool want_sai, bool exact_reference_parse, bool dense_sa = false);
// the reference's output files from the device results of a finished chain, as host buffers
void fetch_outputs(pfp_ctx *c, const uint8_t *d_bwt, const SaView &d_sa, uint64_t n_out, int flags, pfp_bwt_result *out);
// occ_lex[lexrank[j]] = wocc[j] and (where asked for) word_at_rank[lexrank[j]] = j for the d words (newscan.cpp:436)
void occ_in_lex_order(pfp_ctx *c, uint32_t d, const uint32_t *lexrank, const uint32_t *wocc, uint32_t *occ_lex, uint32_t *word_at_rank);
// dst = the words order[0], order[1], ... of a dictionary with their terminators, word r at doff[r] (newscan.cpp:406-438)
void permute_dictionary(pfp_ctx *c, uint32_t d, const uint32_t *order, const uint64_t *woff, const uint32_t *wlen, const uint8_t *src,
                        const uint64_t *doff, uint8_t *dst);

}  // namespace pfp
