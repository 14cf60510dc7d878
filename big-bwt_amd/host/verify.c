/* verify.c -- checking written outputs by inverting the BWT (pfp_check_bwt_files), shared by bigbwt --verify and unbwt --check */
#include <stdio.h>
#include "verify.h"

int pfp_print_check(const pfp_check_result *r, int flags) {
  int bad = 0;
  if (r->text_mismatch == UINT64_MAX) printf("BWT inverts to the input\n");
  else { printf("BWT differs from the input at text position %llu\n", (unsigned long long)r->text_mismatch); bad = 1; }
  const struct { int flag; const char *label; uint64_t mm; } rows[3] = {
      {PFP_FLAG_SA, "SA ", r->sa_mismatch}, {PFP_FLAG_SSA, "SSA", r->ssa_mismatch}, {PFP_FLAG_ESA, "ESA", r->esa_mismatch}};
  for (int k = 0; k < 3; k++) {
    if (!(flags & rows[k].flag)) continue;
    if (rows[k].mm == UINT64_MAX) printf("%s ok\n", rows[k].label);
    else { printf("%s differs at entry %llu\n", rows[k].label, (unsigned long long)rows[k].mm); bad = 1; }
  }
  return bad;
}

int pfp_verify_files(pfp_ctx *ctx, const char *base, const char *label, const uint8_t *text, int text_fd, uint64_t n, int flags) {
  printf("==== Checking outputs by inverting the BWT. Command: pfp_check_bwt_files(%s)\n", label);
  pfp_check_result r;
  const int rc = pfp_check_bwt_files(ctx, base, text, text_fd, 0, n, flags, &r);
  if (rc) {
    printf("%s.bwt: %s: %s\n", base, pfp_strerror(rc), pfp_last_error(ctx));
    return 1;
  }
  const int bad = pfp_print_check(&r, flags);
  printf("Check time: %.4f\n", r.ms / 1e3);
  return bad;
}
