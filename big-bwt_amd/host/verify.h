/* verify.h -- the report `bigbwt --verify` and `unbwt --check` print for pfp_check_bwt_files */
#ifndef PFP_VERIFY_H
#define PFP_VERIFY_H
#include "pfpgpu.h"
/* one line per output checked (flags: PFP_FLAG_SA / SSA / ESA); returns 1 if anything differs, else 0 */
int pfp_print_check(const pfp_check_result *r, int flags);
/* pfp_check_bwt_files with its heading and report; returns the exit status (0 clean, 1 different or not a BWT) */
int pfp_verify_files(pfp_ctx *ctx, const char *base, const char *label, const uint8_t *text, int text_fd, uint64_t n, int flags);
#endif
