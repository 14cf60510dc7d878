// api_check.hip -- inverting a BWT and checking the output files against it (unbwt.hip): pfp_unbwt*, pfp_check_bwt*.
#include "api.hpp"

using namespace pfp;

extern "C" {

int pfp_unbwt_dev(pfp_ctx *c, const void *d_bwt, uint64_t n_plus_1, void *d_text) {
  if (!c || !d_bwt || (!d_text && n_plus_1 > 1)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  BwtCheckArgs a;
  a.bwt = (const uint8_t *)d_bwt; a.n1 = n_plus_1; a.out = (uint8_t *)d_text;
  pfp_check_result r;
  invert_bwt(c, a, &r);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_unbwt(pfp_ctx *c, const uint8_t *bwt, uint64_t n_plus_1, uint8_t *text) {
  if (!c || (!bwt && n_plus_1) || (!text && n_plus_1 > 1)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  check_bwt_rows(n_plus_1);
  DBuf<uint8_t> d_bwt(c, n_plus_1), d_text(c, n_plus_1);
  upload(c, d_bwt.p, bwt, n_plus_1);
  BwtCheckArgs a;
  a.bwt = d_bwt.p; a.n1 = n_plus_1; a.out = d_text.p;
  pfp_check_result r;
  invert_bwt(c, a, &r);
  if (n_plus_1 > 1) download(c, text, d_text.p, n_plus_1 - 1);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_check_bwt_dev(pfp_ctx *c, const void *d_bwt, uint64_t n_plus_1, const void *d_text, const void *d_sa5, const void *d_ssa10,
                      uint64_t ssa_bytes, const void *d_esa10, uint64_t esa_bytes, pfp_check_result *out) {
  if (!c || !d_bwt || !out) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  BwtCheckArgs a;
  const uint64_t n = n_plus_1 ? n_plus_1 - 1 : 0;
  a.bwt = (const uint8_t *)d_bwt; a.n1 = n_plus_1;
  a.text = (const uint8_t *)d_text; a.text_len = n;
  a.sa5 = (const uint8_t *)d_sa5; a.sa_bytes = 5 * n;
  a.ssa10 = (const uint8_t *)d_ssa10; a.ssa_bytes = ssa_bytes;
  a.esa10 = (const uint8_t *)d_esa10; a.esa_bytes = esa_bytes;
  invert_bwt(c, a, out);
  return PFP_OK;
  PFP_CATCH(c)
}

int pfp_check_bwt_files(pfp_ctx *c, const char *base, const uint8_t *text, int text_fd, uint64_t text_offset, uint64_t n, int flags,
                        pfp_check_result *out) {
  if (!c || !base || !out || (!text && text_fd < 0 && n)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  const auto t0 = std::chrono::steady_clock::now();
  const std::string b(base);
  DBuf<uint8_t> d_bwt, d_text, d_sa, d_ssa, d_esa;
  BwtCheckArgs a;
  a.n1 = file_to_dev(c, b + ".bwt", d_bwt);
  a.bwt = d_bwt.p;
  check_bwt_rows(a.n1);
  d_text.alloc(c, n + 16);
  upload_text(c, d_text.p, text, text_fd, text_offset, n);
  sync(c);      // (the next upload fills the same pinned buffers)
  a.text = d_text.p; a.text_len = n;
  if (flags & PFP_FLAG_SA) { a.sa_bytes = file_to_dev(c, b + ".sa", d_sa); a.sa5 = d_sa.p; }
  if (flags & PFP_FLAG_SSA) { a.ssa_bytes = file_to_dev(c, b + ".ssa", d_ssa); a.ssa10 = d_ssa.p; }
  if (flags & PFP_FLAG_ESA) { a.esa_bytes = file_to_dev(c, b + ".esa", d_esa); a.esa10 = d_esa.p; }
  sync(c);
  invert_bwt(c, a, out);
  out->ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return PFP_OK;
  PFP_CATCH(c)
}

}  // extern "C"
