/* unbwt.c -- invert a .bwt on the GPU, or check existing outputs against their text by inverting the BWT.
 *
 *   unbwt [-o outfile] basename                          <basename>.bwt -> the text, in <basename>.out (or outfile)
 *   unbwt --check TEXTFILE [-S] [-s] [-e] basename       <basename>.bwt (and .sa / .ssa / .esa) against TEXTFILE
 *   unbwt --thresholds [--lcp] [--text FILE] basename    <basename>.bwt / .ssa / .esa -> <basename>.thr_pos (and <basename>.lcp)
 *
 * The output name follows the reference's `unparse` (<basename>.out).  The reference's readme suggests checking large
 * outputs "by some other means (for example inverting it)"; --check does that for any .bwt / .sa / .ssa / .esa of the
 * reference's formats, whichever tool wrote them, and exits 1 on any difference.  A file that is not a BWT (not exactly
 * one byte 0, or an LF mapping of several cycles) is reported and exits 1.
 * --thresholds writes one threshold row per run of the BWT, --lcp with it the LCP array of all n + 1 rows, both as 5-byte
 * little-endian ints (the definitions: include/pfpgpu.h, "The LCP array and thresholds"); the text comes from FILE, or without
 * --text by inverting basename.bwt.
 */
#define _GNU_SOURCE
#include <fcntl.h>
#include <getopt.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include "pfpgpu.h"
#include "verify.h"

static void usage(const char *argv0) {
  printf("usage: %s [-h] [-o OUTFILE] basename\n"
         "       %s --check TEXTFILE [-S] [-s] [-e] basename\n"
         "       %s --thresholds [--lcp] [--text FILE] basename\n\n"
         "Inverts basename.bwt on the GPU (MI355X), or checks existing outputs against their text.\n\n"
         "  basename         reads basename.bwt (one byte 0; the bigbwt output format)\n"
         "  -o OUTFILE       write the text to OUTFILE (def. basename.out)\n"
         "  --check TEXTFILE compare the inverse with TEXTFILE instead of writing it; exit 1 on any difference\n"
         "  -S               with --check: also check basename.sa (full suffix array, 5-byte entries)\n"
         "  -s               with --check: also check basename.ssa (run starts)\n"
         "  -e               with --check: also check basename.esa (run ends)\n"
         "      --thresholds write basename.thr_pos: one threshold row per run; reads basename.bwt, .ssa and .esa\n"
         "      --lcp        with --thresholds: also write basename.lcp (the LCP array, n + 1 entries)\n"
         "      --text FILE  with --thresholds: the text (def. inverted from basename.bwt)\n"
         "      --device D   GPU to use (def. 0)\n",
         argv0, argv0, argv0);
}

int main(int argc, char **argv) {
  const char *outname = NULL, *textfile = NULL, *thrtext = NULL;
  int flags = 0, device = 0, thresholds = 0, lcp = 0;
  static struct option lo[] = {{"check", required_argument, 0, 1000}, {"device", required_argument, 0, 1001},
                               {"thresholds", no_argument, 0, 1002}, {"lcp", no_argument, 0, 1003}, {"text", required_argument, 0, 1004},
                               {"help", no_argument, 0, 'h'}, {0, 0, 0, 0}};
  int c;
  while ((c = getopt_long(argc, argv, "o:Sseh", lo, NULL)) != -1) {
    switch (c) {
      case 'o': outname = optarg; break;
      case 'S': flags |= PFP_FLAG_SA; break;
      case 's': flags |= PFP_FLAG_SSA; break;
      case 'e': flags |= PFP_FLAG_ESA; break;
      case 1000: textfile = optarg; break;
      case 1001: device = atoi(optarg); break;
      case 1002: thresholds = 1; break;
      case 1003: lcp = 1; break;
      case 1004: thrtext = optarg; break;
      case 'h': usage(argv[0]); return 0;
      default: usage(argv[0]); return 2;
    }
  }
  if (optind + 1 != argc || (flags && !textfile) || (outname && textfile)) { usage(argv[0]); return 2; }
  if (((lcp || thrtext) && !thresholds) || (thresholds && (textfile || outname))) { usage(argv[0]); return 2; }
  const char *base = argv[optind];

  pfp_ctx *ctx = NULL;
  int rc = pfp_ctx_create(&ctx, device);
  if (rc) {
    fprintf(stderr, "Cannot initialise the GPU (%s): this tool has no CPU path\n", pfp_strerror(rc));
    return 1;
  }
  int status = 0;
  if (thresholds) {
    int fd = -1;
    uint64_t n = 0;
    if (thrtext) {
      struct stat sb;
      fd = open(thrtext, O_RDONLY);
      if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        perror(thrtext);
        if (fd >= 0) close(fd);
        pfp_ctx_destroy(ctx);
        return 1;
      }
      n = (uint64_t)sb.st_size;
    }
    rc = pfp_lcp_files(ctx, base, NULL, fd, 0, n, PFP_LCP_THR | (lcp ? PFP_LCP_LCP : 0));
    if (fd >= 0) close(fd);
    if (rc) {
      if (thrtext) fprintf(stderr, "%s: ", thrtext);
      fprintf(stderr, "%s: %s: %s\n", base, pfp_strerror(rc), pfp_last_error(ctx));
      status = 1;
    }
  } else if (textfile) {
    const int fd = open(textfile, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) { perror(textfile); pfp_ctx_destroy(ctx); return 1; }
    status = pfp_verify_files(ctx, base, textfile, NULL, fd, (uint64_t)sb.st_size, flags);
    close(fd);
  } else {
    char inname[4096], defout[4096];
    snprintf(inname, sizeof inname, "%s.bwt", base);
    snprintf(defout, sizeof defout, "%s.out", base);
    if (!outname) outname = defout;
    const int fd = open(inname, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) { perror(inname); pfp_ctx_destroy(ctx); return 1; }
    const uint64_t n1 = (uint64_t)sb.st_size;
    const uint8_t *bwt = n1 ? mmap(NULL, n1, PROT_READ, MAP_PRIVATE, fd, 0) : NULL;
    if (bwt == MAP_FAILED) { perror("mmap"); pfp_ctx_destroy(ctx); return 1; }
    uint8_t *text = malloc(n1 > 1 ? n1 - 1 : 1);
    if (!text) { fprintf(stderr, "out of memory\n"); pfp_ctx_destroy(ctx); return 1; }
    rc = pfp_unbwt(ctx, bwt, n1, text);
    if (rc) {
      fprintf(stderr, "%s: %s: %s\n", inname, pfp_strerror(rc), pfp_last_error(ctx));
      status = 1;
    } else {
      const uint64_t n = n1 ? n1 - 1 : 0;
      FILE *f = fopen(outname, "wb");
      if (!f) { perror(outname); status = 1; }
      else {
        const size_t w = n ? fwrite(text, 1, n, f) : 0;
        if (fclose(f) != 0 || w != n) { fprintf(stderr, "Error writing %s\n", outname); status = 1; }
      }
    }
    free(text);
    if (n1) munmap((void *)bwt, n1);
    close(fd);
  }
  pfp_ctx_destroy(ctx);
  return status;
}
