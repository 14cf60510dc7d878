/* bwtsearch.c -- count (and locate) patterns in a text through its .bwt (and .ssa / .esa) on the GPU.
 *
 *   bwtsearch [-l] [-m MAXOCC] [--device D] PATTERNFILE basename
 *   bwtsearch --ms | --mems L [--thresholds] [--text FILE] [--device D] PATTERNFILE basename
 *   bwtsearch -l --seqs[=FILE] | --docs [--seqs=FILE] ... PATTERNFILE basename        (any mode: --rc)
 *   bwtsearch -k K [-l] [-m MAXOCC] [--device D] PATTERNFILE basename
 *   bwtsearch --align K [--seed L] [--cigar] [-m MAXALN] [--thresholds] [--text FILE] [--device D] PATTERNFILE basename
 *   bwtsearch --sam K [--seed L] [--secondary N] [--thresholds] [--text FILE] [--seqs=FILE] [--device D] READS basename
 *   bwtsearch --sam K --paired | -2 FILE [--ins MIN:MAX] [--anchors C] [--seed L] [--thresholds] ... READS basename
 *   bwtsearch --paf [--cigar [--fill F]] [--seed L] [--max-occ N] [--gap G] [--band B] [--min-score S] [--secondary N] [--thresholds] [--text FILE]
 *             [--seqs=FILE] [--device D] READS basename
 *
 * Patterns are the lines of PATTERNFILE, split at '\n' only, bytes kept as they are (a final '\n' ends the last line; it does
 * not start an empty one).  One output line per pattern: its count, or with -l `count<TAB>pos pos ...`, the positions in row
 * order (the lexicographic order of the suffixes), at most MAXOCC of them (0: all).  Count needs basename.bwt only; -l also
 * reads basename.ssa and basename.esa (bigbwt -s -e).  The definitions: include/pfpgpu.h, "Searching a BWT".
 * --ms prints the matching statistics of every pattern, `len:pos` for every byte of the line separated by one space, `0:-` where
 * the length is 0; --mems L its maximal exact matches of at least L bytes, `count<TAB>i:len:pos i:len:pos ...` (the definitions:
 * include/pfpgpu.h, "Matching statistics").  Both read basename.bwt, .ssa and .esa, and the text from FILE, or without --text by
 * inverting basename.bwt.  --thresholds computes them in two passes with thresholds (the same lengths; positions by that
 * algorithm's own rule): it reads basename.thr_pos if that file exists (unbwt --thresholds writes it) and computes the thresholds
 * otherwise.
 * --seqs[=FILE] loads the sequence table of a collection (seqs.h; FILE defaults to basename.seqs, which bigbwt -f --seqs writes).
 * With -l the line becomes `count<TAB>name:offset name:offset ...`: of the at most MAXOCC rows examined, the hits that lie inside
 * one sequence, each as its sequence's name and the offset in it (the offset is what follows the LAST ':': names may hold one).
 * count stays ep - sp, the rows - matches that span two sequences included.  --docs (implies --seqs) prints
 * `ndocs<TAB>name:hits name:hits ...`: the sequences that hold the pattern inside them, in table order, with their numbers of
 * hits; every occurrence counts.  --rc searches every line as given and then as its reverse complement (reversed, A<->T, C<->G,
 * a<->t, c<->g, other bytes as they are): two output lines per input line, in that order, in every mode.
 * -k K (0..3) searches with at most K substitutions (the definitions: include/pfpgpu.h, "Approximate search").  The line becomes
 * `total<TAB>c0 c1 .. cK`: the approximate occurrences, and how many of them have exactly 0, 1, .. K mismatches; with -l
 * `total<TAB>pos:d pos:d ...`: the positions with their mismatches, hits by increasing row range and rows in row order, at most
 * MAXOCC of them; total stays the number of occurrences.  Not with --ms, --mems, --docs or --seqs.
 * --align K (0..32) is seed-and-extend (the definitions: include/pfpgpu.h, "Extending seeds"): every maximal exact match of at
 * least L bytes (--seed, default 20: a choice) is extended along its diagonal with at most K edits (substitutions, insertions and
 * deletions).  The line becomes `count<TAB>start:end:d start:end:d ...`: the distinct alignments T[start..end) with their edit
 * distances, ordered by (d, start, end), at most MAXALN of them (0: all); count stays their number before the cap.  It reads the
 * files --mems reads and takes --text and --thresholds as --mems does.  Not with -l, -k, --ms, --mems, --docs or --seqs.
 * --cigar (with --align only) adds every alignment's edit script (the definitions: include/pfpgpu.h, "Edit scripts"): the items
 * become `start:end:d:CIGAR`, the runs as length and operation, `=` a match, `X` a substitution, `I` a pattern byte without a text
 * byte, `D` a text byte without a pattern byte, e.g. 57=1X20=1I72=; `*` for the empty script.
 * --sam K (0..32) maps reads to a collection and prints SAM (the definitions: include/pfpgpu.h, "Mapping reads"): both strands of
 * every read go through --align's seed-and-extend (--seed, --thresholds and --text as there), the alignments that lie inside one
 * record are kept, one per locus, and ordered by (edits, strand, position).  It needs the sequence table (--seqs=FILE, default
 * basename.seqs, which bigbwt -f --seqs writes).  READS: a file whose first byte is > or @ is FASTA / FASTQ, plain or
 * gzip-compressed, read as bigbwt -f reads it - names up to the first white space, bases upper-cased, qualities not kept (QUAL is
 * *); any other file holds one read per line, named by its 1-based line number.  Output: @HD VN:1.6 SO:unsorted, one @SQ SN:name
 * LN:length per record that is not empty, @PG ID:bwtsearch, then per read its primary line `QNAME FLAG RNAME POS MAPQ CIGAR * 0 0
 * SEQ * NM:i:edits MD:Z:... NH:i:hits` (tab-separated; FLAG 0, or 16 where the reverse complement aligns, and SEQ is then the
 * reverse complement; POS counts from 1 inside the record; CIGAR with = and X; MAPQ 0..60 is a choice, not a probability) and up
 * to N (--secondary, default 0) further hits with FLAG | 256 and MAPQ 0; a read without hits prints `QNAME 4 * 0 0 * * 0 0 SEQ *`.
 * Not with -l, -k, -m, --ms, --mems, --docs, --align, --cigar or --rc.
 * --paired (with --sam) maps read pairs, forward/reverse (the definitions: include/pfpgpu.h, "Mapping read pairs"): READS is
 * interleaved (mate 1, mate 2, ...); with -2 FILE, READS holds the mates 1 and FILE the mates 2 in the same order (-2 implies
 * --paired; a different number of reads, or an odd number in an interleaved file, is exit 1).  --ins MIN:MAX (default 0:1000, a
 * choice) bounds a proper pair's insert, from the forward mate's first byte to the reverse mate's last; --anchors C (1..64, default
 * 8, a choice) is how many hits of each mate are combined.  A mate without a proper partner among the hits is looked for within
 * MAX bytes of its partner (rescue).  One line per read, mate 1 then mate 2.  QNAME: a trailing /1 and /2 go when mate 1 ends in /1
 * and mate 2 in /2, otherwise mate 1's name serves both (a line file names a read by its line number in its own file).  FLAG = 1 +
 * 2 (proper pair) + 4 (unmapped) + 8 (mate unmapped) + 16 (own strand reversed) + 32 (mate's strand reversed) + 64 (mate 1) or 128
 * (mate 2).  RNEXT is = when the mate lies in the same record, its record's name otherwise, * when it is unmapped; PNEXT its POS or
 * 0; TLEN as the header defines it.  An unmapped read whose mate is mapped takes the mate's RNAME and POS, with RNEXT =, MAPQ 0
 * and CIGAR *.  In a proper pair MAPQ is the pair's and NH:i its number of pairs; otherwise they are the read's own.  A rescued
 * read carries YR:i:1.  None of --paired, -2, --ins, --anchors combines with --secondary, and all need --sam.
 * --paf maps long reads by chaining and prints PAF (the definitions: include/pfpgpu.h, "Chaining anchors"): both strands of every
 * read, every occurrence of every maximal exact match of at least L bytes (--seed, default 20) that occurs at most N times
 * (--max-occ, 1..65536, default 500), chained with gaps of at most G bytes (--gap, default 5000) and at most B bytes off the
 * diagonal (--band, default 500); chains that score below S (--min-score, default 40) are dropped.  All five defaults are
 * choices.  READS is read as --sam reads it; --text and --thresholds as --mems takes them.  One line per returned chain, none for
 * a read without one: `qname qlen qs qe strand tname tlen ts te match span mapq` (tab-separated; strand + or -; qs, qe in the read
 * as given; ts, te inside the record; match = the bytes in seeds; span = max(qe - qs, te - ts); MAPQ 0..60 is a choice) and the
 * tags tp:A:P (the best chain) or tp:A:S (up to N further ones, --secondary, default 0, with MAPQ 0), cm:i: the chain's anchors,
 * s1:i: its score and, on a primary line with a runner-up, s2:i: the runner-up's.  With --seqs[=FILE] tname and tlen are the
 * record's; without a table tname is basename's file name and tlen the text's length.  --paf combines with no other mode.
 * --paf --cigar aligns every printed chain base by base (include/pfpgpu.h, "Aligning chains"): the stretch between two anchors
 * by an edit-distance alignment of at most F edits (--fill, 0..4096, default 500 = the default band, a choice; needs both).  The
 * line's columns are then the alignment's: qs, qe and ts where the chain's first anchor begins (on strand - that moves qe), column
 * 10 the bytes in '=' runs, column 11 the sum of all run lengths; behind the tags above come NM:i:, uf:i: (the stretches that
 * take more than F edits and stand in the script as an insertion and a deletion; only where there are any; this program's own
 * tag) and cg:Z: with '=', X, I, D.  Without --cigar the output is what it was.
 * Large pattern files go through in batches of at most 2^20 patterns and 64 MiB (PFP_FM_BATCH=K: at most K patterns).
 * Exit codes: 0 done, 1 a file that cannot be read, is not a BWT or lacks a sample file, a sequence table that cannot be read, is
 * malformed or does not sum to the text's length, 2 a usage error.
 */
#define _GNU_SOURCE
#include <fcntl.h>
#include <getopt.h>
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include "pfpgpu.h"
#include "fasta.h"
#include "seqs.h"

static void usage(const char *argv0) {
  printf("usage: %s [-h] [-l] [-m MAXOCC] [--seqs[=FILE]] [--rc] [--device D] PATTERNFILE basename\n"
         "       %s --docs [--seqs=FILE] [--rc] [--device D] PATTERNFILE basename\n"
         "       %s --ms | --mems L [--thresholds] [--text FILE] [--rc] [--device D] PATTERNFILE basename\n"
         "       %s -k K [-l] [-m MAXOCC] [--rc] [--device D] PATTERNFILE basename\n"
         "       %s --align K [--seed L] [--cigar] [-m MAXALN] [--thresholds] [--text FILE] [--rc] [--device D] PATTERNFILE basename\n"
         "       %s --sam K [--seed L] [--secondary N] [--thresholds] [--text FILE] [--seqs=FILE] [--device D] READS basename\n"
         "       %s --sam K --paired | -2 FILE [--ins MIN:MAX] [--anchors C] [--seed L] [--thresholds] [--text FILE] [--seqs=FILE] READS basename\n"
         "       %s --paf [--cigar [--fill F]] [--seed L] [--max-occ N] [--gap G] [--band B] [--min-score S] [--secondary N] [--thresholds] [--text FILE] [--seqs=FILE] READS basename\n\n"
         "Counts, or with -l locates, the lines of PATTERNFILE in the text whose BWT is basename.bwt, on the GPU (MI355X).\n\n"
         "  PATTERNFILE   one pattern per line (split at \\n only, bytes kept as they are)\n"
         "  basename      reads basename.bwt; with -l also basename.ssa and basename.esa (bigbwt -s -e)\n"
         "  -l            print count<TAB>positions (in suffix order) instead of the count\n"
         "  -m MAXOCC     with -l: at most MAXOCC positions per pattern (def. 0 = all)\n"
         "  -k K          at most K substitutions (0..3): print total<TAB>c0 c1 .. cK, the occurrences and how many of them have\n"
         "                exactly 0, 1, .. K mismatches; with -l total<TAB>pos:d ... , at most MAXOCC positions with their\n"
         "                mismatches (not with --ms, --mems, --docs, --seqs)\n"
         "      --ms        print the matching statistics: len:pos for every byte of the line (0:- where nothing matches);\n"
         "                  reads basename.bwt, .ssa and .esa\n"
         "      --mems L    print count<TAB>i:len:pos ... : the maximal exact matches of at least L >= 1 bytes; reads the same files\n"
         "      --align K   seed-and-extend with at most K edits (0..32; substitutions, insertions, deletions): print\n"
         "                  count<TAB>start:end:d ... : the distinct alignments T[start..end) by (d, start, end), at most MAXALN (-m)\n"
         "                  of them; reads the files --mems reads (not with -l, -k, --ms, --mems, --docs, --seqs)\n"
         "      --seed L    with --align: the seeds are the maximal exact matches of at least L >= 1 bytes (def. 20, a choice)\n"
         "      --cigar     with --align: print count<TAB>start:end:d:CIGAR ... : every alignment with its edit script, runs of\n"
         "                  = (match), X (substitution), I (pattern byte alone), D (text byte alone); * for the empty script\n"
         "      --sam K     map the reads of READS to the records of a collection with at most K edits (0..32) and print SAM: both\n"
         "                  strands through --align's seed-and-extend (--seed, --thresholds, --text as there), the alignments inside\n"
         "                  one record, one per locus; per read the best hit (FLAG 0 / 16, POS from 1 in its record, MAPQ 0..60 - a\n"
         "                  choice, not a probability -, CIGAR with = and X, NM, MD, NH), `QNAME 4 * 0 0 * * 0 0 SEQ *` for a read\n"
         "                  without hits.  Needs the sequence table (--seqs=FILE, def. basename.seqs: bigbwt -f --seqs writes it).\n"
         "                  READS: first byte > or @: FASTA / FASTQ, plain or gzip, bases upper-cased, qualities not kept (QUAL is *);\n"
         "                  else one read per line, named by its line number (not with -l, -k, -m, --ms, --mems, --docs, --align,\n"
         "                  --cigar, --rc)\n"
         "      --secondary N with --sam: also print up to N further hits of a read, with FLAG | 256 and MAPQ 0 (def. 0)\n"
         "      --paired    with --sam: READS is interleaved read pairs (mate 1, mate 2, ...), forward/reverse: one line per read with the\n"
         "                  pair flags (1, 2 proper, 8 mate unmapped, 32 mate reversed, 64 / 128), RNEXT, PNEXT, TLEN, the pair's MAPQ\n"
         "                  and NH in a proper pair, YR:i:1 on a mate found by rescue; /1 and /2 are stripped from the names (not\n"
         "                  with --secondary)\n"
         "  -2 FILE         with --sam: READS holds the mates 1, FILE the mates 2, in the same order (implies --paired)\n"
         "      --ins MIN:MAX with --paired: a proper pair's insert, forward mate's first byte to reverse mate's last (def. 0:1000, a\n"
         "                  choice; MAX <= 16384); a mate without a proper partner is looked for within MAX bytes of its partner\n"
         "      --anchors C with --paired: the hits of each mate that are combined (1..64, def. 8, a choice)\n"
         "      --paf       map the long reads of READS (read as --sam reads it) by chaining and print PAF: both strands, every\n"
         "                  occurrence of every maximal exact match of at least L bytes (--seed, def. 20) chained; one line per chain,\n"
         "                  qname qlen qs qe strand tname tlen ts te match span mapq tp:A:P|S cm:i:anchors s1:i:score [s2:i:runner-up],\n"
         "                  none for a read without one; --secondary N prints up to N further chains (tp:A:S, MAPQ 0); with\n"
         "                  --seqs[=FILE] the target is the record, else the whole text under basename's name (no other mode)\n"
         "      --max-occ N with --paf: a match that occurs more than N times is left out (1..65536, def. 500, a choice)\n"
         "      --gap G     with --paf: two anchors chain when they end at most G bytes apart in the read and the text (def. 5000, a choice)\n"
         "      --band B    with --paf: ... and at most B bytes off each other's diagonal (def. 500, a choice)\n"
         "      --min-score S with --paf: a chain that scores below S is dropped (def. 40, a choice)\n"
         "      --cigar     with --paf: align every printed chain base by base: the line's coordinates are the alignment's, columns 10\n"
         "                  and 11 its matches and its length, and NM:i:, uf:i: (gaps left unfilled, if any) and cg:Z: (=, X, I, D) follow\n"
         "      --fill F    with --paf --cigar: the edits the stretch between two anchors may take (0..4096, def. 500 = the default\n"
         "                  band, a choice); a stretch that takes more stands in the script as an insertion and a deletion\n"
         "      --text FILE with --ms / --mems / --align / --sam / --paf: the text (def. inverted from basename.bwt)\n"
         "      --thresholds with --ms / --mems / --align / --sam / --paf: two passes with thresholds; reads basename.thr_pos if it exists, else computes it\n"
         "      --seqs[=FILE] load the sequence table FILE (def. basename.seqs; bigbwt -f --seqs writes it).  With -l print\n"
         "                  count<TAB>name:offset ... : the hits inside one sequence among the at most MAXOCC rows examined;\n"
         "                  count stays the number of rows, matches that span two sequences included\n"
         "      --docs      print ndocs<TAB>name:hits ... : the sequences that hold the pattern, in table order (implies --seqs;\n"
         "                  reads basename.ssa and .esa; every occurrence counts)\n"
         "      --rc        search every line as given, then its reverse complement (A<->T, C<->G): two output lines per line\n"
         "      --device D  GPU to use (def. 0)\n",
         argv0, argv0, argv0, argv0, argv0, argv0, argv0, argv0);
}

static int read_file(const char *path, uint8_t **out, uint64_t *len) {
  FILE *f = fopen(path, "rb");
  if (!f) return -1;
  uint64_t cap = 1 << 20, n = 0;
  uint8_t *b = malloc(cap);
  for (;;) {
    if (!b) { fclose(f); return -1; }
    const size_t got = fread(b + n, 1, cap - n, f);
    n += got;
    if (n < cap) break;
    cap *= 2;
    uint8_t *nb = realloc(b, cap);
    if (!nb) free(b);
    b = nb;
  }
  const int err = ferror(f);
  fclose(f);
  if (err) { free(b); return -1; }
  *out = b;
  *len = n;
  return 0;
}

/* out = the reverse complement of the len bytes at in */
static void revcomp(const uint8_t *in, uint64_t len, uint8_t *out) {
  static uint8_t map[256];
  if (!map['A']) {
    for (int i = 0; i < 256; i++) map[i] = (uint8_t)i;
    map['A'] = 'T'; map['T'] = 'A'; map['C'] = 'G'; map['G'] = 'C';
    map['a'] = 't'; map['t'] = 'a'; map['c'] = 'g'; map['g'] = 'c';
  }
  for (uint64_t i = 0; i < len; i++) out[i] = map[in[len - 1 - i]];
}

/* one batch of k patterns, the index, the options, and main's scratch arrays (room for k + 1 entries each; ep: k) */
typedef struct {
  pfp_ctx *ctx; pfp_fm *fm; const char *base; const pfp_seqs *tab;
  const uint8_t *pat; const uint64_t *off; uint64_t k, *oo, *sp, *ep;
  uint64_t maxocc, min_len, seed;
  int thresholds, locate, kmis, kedit, cigar;
  uint64_t min_ins, max_ins, anchors;
  uint64_t maxsec, first; char *const *qname;      /* --sam: the batch's first read, and the reads' names (NULL: their numbers) */
  uint64_t max_occ, gap, band, min_score, n; const char *tname;      /* --paf; n, tname: the text's length and name (no table) */
  uint64_t fill;                                                     /* --paf --cigar: the edits a gap between two anchors may take */
} batch_t;

static int fail(const char *what, int rc, pfp_ctx *ctx) {
  fprintf(stderr, "%s: %s: %s\n", what, pfp_strerror(rc), pfp_last_error(ctx));
  return 1;
}

/* the space between the items of a line: before every item j but the line's first */
static void sep(uint64_t j, uint64_t first) { if (j > first) putchar(' '); }

/* Every mode answers one batch, a line per pattern: 0, or 1 after the error went to stderr. */
static int mode_ms(const batch_t *b) {
  const uint64_t total = b->off[b->k];
  uint32_t *len = malloc((total + 1) * sizeof(uint32_t));
  uint64_t *pos = malloc((total + 1) * sizeof(uint64_t));
  int rc = 1;
  if (!len || !pos) fprintf(stderr, "out of memory\n");
  else if ((rc = (b->thresholds ? pfp_fm_ms_thr : pfp_fm_ms)(b->fm, b->pat, b->off, b->k, len, pos)) != 0) rc = fail(b->base, rc, b->ctx);
  for (uint64_t i = 0; !rc && i < b->k; i++) {
    for (uint64_t j = b->off[i]; j < b->off[i + 1]; j++) {
      sep(j, b->off[i]);
      if (len[j]) printf("%" PRIu32 ":%" PRIu64, len[j], pos[j]);
      else fputs("0:-", stdout);
    }
    putchar('\n');
  }
  free(len); free(pos);
  return rc;
}

static int mode_mems(const batch_t *b) {
  uint64_t *m = NULL, *oo = b->oo;
  const int rc = (b->thresholds ? pfp_fm_mems_thr : pfp_fm_mems)(b->fm, b->pat, b->off, b->k, b->min_len, oo, &m);
  if (rc) return fail(b->base, rc, b->ctx);
  for (uint64_t i = 0; i < b->k; i++) {
    printf("%" PRIu64 "\t", oo[i + 1] - oo[i]);
    for (uint64_t j = oo[i]; j < oo[i + 1]; j++) { sep(j, oo[i]); printf("%" PRIu64 ":%" PRIu64 ":%" PRIu64, m[3 * j], m[3 * j + 1], m[3 * j + 2]); }
    putchar('\n');
  }
  pfp_free(m);
  return 0;
}

/* --cigar: the edit scripts of a batch's alignments, alignment j = (its pattern by oo, as[j], ae[j]): *coff (their number + 1
 * offsets) and *cig (the runs); 0, or 1 after the error went to stderr */
static int align_scripts(const batch_t *b, const uint64_t *as, const uint64_t *ae, uint64_t **coff, uint32_t **cig) {
  const uint64_t *oo = b->oo, total = oo[b->k];
  uint32_t *ap = malloc((total + 1) * sizeof(uint32_t));
  uint8_t *cd = malloc(total + 1);
  *coff = malloc((total + 1) * sizeof(uint64_t));
  int rc = 1;
  if (!ap || !cd || !*coff) fprintf(stderr, "out of memory\n");
  else {
    for (uint64_t i = 0; i < b->k; i++)
      for (uint64_t j = oo[i]; j < oo[i + 1]; j++) ap[j] = (uint32_t)i;
    if ((rc = pfp_fm_cigar(b->fm, b->pat, b->off, b->k, ap, as, ae, total, b->kedit, cd, *coff, cig)) != 0) rc = fail(b->base, rc, b->ctx);
  }
  free(ap); free(cd);
  return rc;
}

static void print_script(const uint32_t *run, uint64_t nrun) {
  if (!nrun) putchar('*');
  for (uint64_t r = 0; r < nrun; r++) printf("%" PRIu32 "%c", run[r] >> 4, "MIDNSHP=X???????"[run[r] & 15]);
}

static int mode_align(const batch_t *b) {
  uint64_t *as = NULL, *ae = NULL, *oo = b->oo, *coff = NULL;
  uint8_t *ad = NULL;
  uint32_t *cig = NULL;
  int rc = pfp_fm_align(b->fm, b->pat, b->off, b->k, b->seed, b->kedit, 0, b->thresholds, oo, &as, &ae, &ad);
  if (rc) return fail(b->base, rc, b->ctx);
  if (b->cigar) rc = align_scripts(b, as, ae, &coff, &cig);
  for (uint64_t i = 0; !rc && i < b->k; i++) {
    const uint64_t cnt = oo[i + 1] - oo[i], shown = b->maxocc && b->maxocc < cnt ? b->maxocc : cnt;
    printf("%" PRIu64 "\t", cnt);
    for (uint64_t j = oo[i]; j < oo[i] + shown; j++) {
      sep(j, oo[i]);
      printf("%" PRIu64 ":%" PRIu64 ":%u", as[j], ae[j], (unsigned)ad[j]);
      if (b->cigar) { putchar(':'); print_script(cig + coff[j], coff[j + 1] - coff[j]); }
    }
    putchar('\n');
  }
  pfp_free(as); pfp_free(ae); pfp_free(ad); pfp_free(cig); free(coff);
  return rc;
}

/* --sam: the header, once */
static void sam_header(const pfp_seqs *tab) {
  puts("@HD\tVN:1.6\tSO:unsorted");
  for (uint64_t k = 0; k < tab->nseq; k++)
    if (tab->start[k + 1] > tab->start[k]) printf("@SQ\tSN:%s\tLN:%" PRIu64 "\n", tab->name[k], tab->start[k + 1] - tab->start[k]);
  puts("@PG\tID:bwtsearch");
}

/* --sam: one record per read and up to maxsec further hits (the definitions: include/pfpgpu.h, "Mapping reads") */
static int mode_sam(const batch_t *b) {
  uint64_t *oo = b->oo, *nhits = b->sp, *off = NULL, *start = NULL, *coff = NULL, *moff = NULL, longest = 0;
  uint8_t *strand = NULL, *dist = NULL, *md = NULL, *mapq = malloc(b->k + 1), *rc = NULL;
  uint32_t *seq = NULL, *cig = NULL;
  for (uint64_t i = 0; i < b->k; i++)
    if (b->off[i + 1] - b->off[i] > longest) longest = b->off[i + 1] - b->off[i];
  rc = malloc(longest + 1);
  int r = 1;
  if (!mapq || !rc) fprintf(stderr, "out of memory\n");
  else if ((r = pfp_fm_map(b->fm, b->pat, b->off, b->k, b->seed, b->kedit, b->maxsec, b->thresholds, oo, mapq, nhits, &strand, &seq, &off, &start,
                           &dist, &coff, &cig, &moff, &md)) != 0)
    r = fail(b->base, r, b->ctx);
  for (uint64_t i = 0; !r && i < b->k; i++) {
    const uint8_t *read = b->pat + b->off[i];
    const uint64_t m = b->off[i + 1] - b->off[i];
    char num[24];
    snprintf(num, sizeof num, "%" PRIu64, b->first + i + 1);
    const char *qn = b->qname ? b->qname[b->first + i] : num;
    if (oo[i + 1] == oo[i]) {
      printf("%s\t4\t*\t0\t0\t*\t*\t0\t0\t", qn);
      if (m) fwrite(read, 1, m, stdout); else putchar('*');
      fputs("\t*\n", stdout);
    }
    for (uint64_t j = oo[i]; j < oo[i + 1]; j++) {
      const int second = j > oo[i];
      printf("%s\t%d\t%s\t%" PRIu64 "\t%u\t", qn, (strand[j] ? 16 : 0) | (second ? 256 : 0), b->tab->name[seq[j]], off[j] + 1,
             second ? 0u : (unsigned)mapq[i]);
      print_script(cig + coff[j], coff[j + 1] - coff[j]);
      fputs("\t*\t0\t0\t", stdout);
      if (strand[j]) revcomp(read, m, rc);
      if (m) fwrite(strand[j] ? rc : read, 1, m, stdout); else putchar('*');
      printf("\t*\tNM:i:%u\tMD:Z:", (unsigned)dist[j]);
      fwrite(md + moff[j], 1, moff[j + 1] - moff[j], stdout);
      printf("\tNH:i:%" PRIu64 "\n", nhits[i]);
    }
  }
  pfp_free(strand); pfp_free(seq); pfp_free(off); pfp_free(start); pfp_free(dist); pfp_free(coff); pfp_free(cig); pfp_free(moff); pfp_free(md);
  free(mapq); free(rc);
  return r;
}

/* --paf: one line per returned chain (the definitions: include/pfpgpu.h, "Chaining anchors").  The runner-up is always asked for:
 * its score goes into the primary line.  --cigar: the chain's edit script ("Aligning chains") decides the line's coordinates - the
 * read's bytes [aqs, qe) on strand +, [qs, aqs) on strand -, the text from ats - the matches and the block length, and adds NM:i:,
 * uf:i: (the gaps left unfilled, where there are any) and cg:Z: */
static int mode_paf(const batch_t *b) {
  uint64_t *oo = b->oo, *nchains = b->sp, *off = NULL, *ts = NULL, *te = NULL, *ats = NULL, *coff = NULL;
  uint8_t *strand = NULL, *mapq = malloc(b->k + 1);
  uint32_t *seq = NULL, *qs = NULL, *qe = NULL, *score = NULL, *cn = NULL, *match = NULL, *aqs = NULL, *nm = NULL, *unf = NULL, *cig = NULL;
  int r = 1;
  if (!mapq) fprintf(stderr, "out of memory\n");
  else if (b->cigar) {
    if ((r = pfp_fm_map_long_aln(b->fm, b->pat, b->off, b->k, b->seed, b->max_occ, b->gap, b->band, b->min_score, b->maxsec ? b->maxsec : 1,
                                 b->thresholds, b->fill, oo, mapq, nchains, &strand, &seq, &off, &ts, &te, &qs, &qe, &score, &cn, &match, &aqs, &ats,
                                 &nm, &unf, &coff, &cig)) != 0)
      r = fail(b->base, r, b->ctx);
  } else if ((r = pfp_fm_map_long(b->fm, b->pat, b->off, b->k, b->seed, b->max_occ, b->gap, b->band, b->min_score, b->maxsec ? b->maxsec : 1,
                                b->thresholds, oo, mapq, nchains, &strand, &seq, &off, &ts, &te, &qs, &qe, &score, &cn, &match)) != 0)
    r = fail(b->base, r, b->ctx);
  for (uint64_t i = 0; !r && i < b->k; i++) {
    char num[24];
    snprintf(num, sizeof num, "%" PRIu64, b->first + i + 1);
    const char *qn = b->qname ? b->qname[b->first + i] : num;
    for (uint64_t j = oo[i]; j < oo[i + 1] && j - oo[i] <= b->maxsec; j++) {
      const int second = j > oo[i];
      const uint64_t qspan = qe[j] - qs[j], tspan = te[j] - ts[j];
      const uint64_t tlen = b->tab->nseq ? b->tab->start[seq[j] + 1] - b->tab->start[seq[j]] : b->n;
      uint64_t q0 = qs[j], q1 = qe[j], t0 = off[j], same = match[j], block = qspan > tspan ? qspan : tspan;
      if (b->cigar) {
        if (strand[j]) q1 = aqs[j];
        else q0 = aqs[j];
        t0 = off[j] + (ats[j] - ts[j]);
        same = block = 0;
        for (uint64_t x = coff[j]; x < coff[j + 1]; x++) {
          block += cig[x] >> 4;
          if ((cig[x] & 15) == 7) same += cig[x] >> 4;
        }
      }
      printf("%s\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%c\t%s\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%u",
             qn, b->off[i + 1] - b->off[i], q0, q1, strand[j] ? '-' : '+', b->tab->nseq ? b->tab->name[seq[j]] : b->tname, tlen, t0,
             off[j] + tspan, same, block, second ? 0u : (unsigned)mapq[i]);
      printf("\ttp:A:%c\tcm:i:%" PRIu32 "\ts1:i:%" PRIu32, second ? 'S' : 'P', cn[j], score[j]);
      if (!second && oo[i + 1] - oo[i] > 1) printf("\ts2:i:%" PRIu32, score[j + 1]);
      if (b->cigar) {
        printf("\tNM:i:%" PRIu32, nm[j]);
        if (unf[j]) printf("\tuf:i:%" PRIu32, unf[j]);
        fputs("\tcg:Z:", stdout);
        print_script(cig + coff[j], coff[j + 1] - coff[j]);
      }
      putchar('\n');
    }
  }
  pfp_free(strand); pfp_free(seq); pfp_free(off); pfp_free(ts); pfp_free(te); pfp_free(qs); pfp_free(qe); pfp_free(score); pfp_free(cn);
  pfp_free(match); pfp_free(aqs); pfp_free(ats); pfp_free(nm); pfp_free(unf); pfp_free(coff); pfp_free(cig);
  free(mapq);
  return r;
}

/* --sam --paired: one record per read (the definitions: include/pfpgpu.h, "Mapping read pairs"); b->k is even and b->qname names
 * every read */
static int mode_sam_paired(const batch_t *b) {
  const uint64_t k = b->k, np = k / 2;
  uint64_t longest = 0;
  for (uint64_t i = 0; i < k; i++)
    if (b->off[i + 1] - b->off[i] > longest) longest = b->off[i + 1] - b->off[i];
  uint64_t *u64 = malloc((6 * k + np + 2) * sizeof(uint64_t));          /* nhits, off, start, tlen (k each), npairs, coff, moff */
  uint8_t *u8 = malloc(5 * k + np + 1), *rc = malloc(longest + 1), *md = NULL;       /* mapped, rescued, mapq, strand, dist, proper */
  uint32_t *seq = malloc((k + 1) * sizeof(uint32_t)), *cig = NULL;
  int r = 1;
  if (!u64 || !u8 || !rc || !seq) { fprintf(stderr, "out of memory\n"); free(u64); free(u8); free(rc); free(seq); return 1; }
  uint64_t *nhits = u64, *off = nhits + k, *start = off + k, *npairs = start + k + k, *coff = npairs + np, *moff = coff + k + 1;
  int64_t *tlen = (int64_t *)(start + k);
  uint8_t *mapped = u8, *rescued = mapped + k, *mapq = rescued + k, *strand = mapq + k, *dist = strand + k, *proper = dist + k;
  if ((r = pfp_fm_map_pairs(b->fm, b->pat, b->off, k, b->seed, b->kedit, b->thresholds, b->min_ins, b->max_ins, b->anchors, proper, npairs, mapped,
                            rescued, mapq, nhits, strand, seq, off, start, dist, tlen, coff, &cig, moff, &md)) != 0)
    r = fail(b->base, r, b->ctx);
  for (uint64_t i = 0; !r && i < k; i++) {
    const uint64_t q = i / 2, o = i ^ 1, m = b->off[i + 1] - b->off[i];
    const uint8_t *read = b->pat + b->off[i];
    const char *n1 = b->qname[b->first + 2 * q], *n2 = b->qname[b->first + 2 * q + 1];
    size_t l1 = strlen(n1);
    const size_t l2 = strlen(n2);
    if (l1 >= 2 && l2 >= 2 && !strcmp(n1 + l1 - 2, "/1") && !strcmp(n2 + l2 - 2, "/2")) l1 -= 2;
    const int flag = 1 | (proper[q] ? 2 : 0) | (mapped[i] ? 0 : 4) | (mapped[o] ? 0 : 8) | (mapped[i] && strand[i] ? 16 : 0) |
                     (mapped[o] && strand[o] ? 32 : 0) | (i & 1 ? 128 : 64);
    const uint64_t w = mapped[i] ? i : o;               /* whose place the line shows */
    fwrite(n1, 1, l1, stdout);
    if (mapped[w]) printf("\t%d\t%s\t%" PRIu64, flag, b->tab->name[seq[w]], off[w] + 1);
    else printf("\t%d\t*\t0", flag);
    printf("\t%u\t", mapped[i] ? (unsigned)mapq[i] : 0u);
    if (mapped[i]) print_script(cig + coff[i], coff[i + 1] - coff[i]); else putchar('*');
    if (!mapped[o]) fputs("\t*\t0", stdout);
    else if (!mapped[i] || seq[o] == seq[i]) printf("\t=\t%" PRIu64, off[o] + 1);
    else printf("\t%s\t%" PRIu64, b->tab->name[seq[o]], off[o] + 1);
    printf("\t%" PRId64 "\t", tlen[i]);
    const int rev = mapped[i] && strand[i];
    if (rev) revcomp(read, m, rc);
    if (m) fwrite(rev ? rc : read, 1, m, stdout); else putchar('*');
    fputs("\t*", stdout);
    if (mapped[i]) {
      printf("\tNM:i:%u\tMD:Z:", (unsigned)dist[i]);
      fwrite(md + moff[i], 1, moff[i + 1] - moff[i], stdout);
      printf("\tNH:i:%" PRIu64, proper[q] ? npairs[q] : nhits[i]);
      if (rescued[i]) fputs("\tYR:i:1", stdout);
    }
    putchar('\n');
  }
  pfp_free(cig); pfp_free(md);
  free(u64); free(u8); free(rc); free(seq);
  return r;
}

/* the lines of a buffer: *lstart gets count + 1 entries, line k = [lstart[k], lstart[k + 1] - 1).  -> their number, or
 * UINT64_MAX when memory runs out */
static uint64_t split_lines(const uint8_t *p, uint64_t len, uint64_t **lstart) {
  uint64_t count = 0;
  for (uint64_t i = 0; i < len; i++) count += p[i] == '\n';
  if (len && p[len - 1] != '\n') count++;
  uint64_t *ls = malloc((count + 1) * sizeof(uint64_t));
  if (!ls) return UINT64_MAX;
  uint64_t k = 0, s = 0;
  for (uint64_t i = 0; i < len; i++)
    if (p[i] == '\n') { ls[k++] = s; s = i + 1; }
  if (k < count) ls[k++] = s;
  /* line k ends one byte before lstart[k + 1]: past the last line sits its '\n', or the end of a file without one */
  ls[count] = len && p[len - 1] == '\n' ? len : len + 1;
  *lstart = ls;
  return count;
}

static int reads_to_lines(uint8_t **buf, uint64_t *n, pfp_seqs *tab);

/* --sam: the reads of a file, plain or gzip-compressed, as lines (FASTA / FASTQ becomes one read per line and tab gets the names).
 * 0, or 1 after the error went to stderr */
static int load_reads(const char *path, uint8_t **buf, uint64_t *len, pfp_seqs *tab, int *named) {
  size_t n = 0;
  *buf = pfp_read_maybe_gz(path, &n);
  if (!*buf) { perror(path); return 1; }
  *len = n;
  *named = 0;
  if (n && ((*buf)[0] == '>' || (*buf)[0] == '@')) {
    if (reads_to_lines(buf, len, tab)) { fprintf(stderr, "out of memory\n"); return 1; }
    *named = 1;
  }
  return 0;
}

/* --sam with a FASTA / FASTQ file: *buf (n bytes, malloc'ed) becomes the reads one per line, as a line file holds them; tab gets
 * their names.  0, or -1 when memory runs out */
static int reads_to_lines(uint8_t **buf, uint64_t *n, pfp_seqs *tab) {
  uint8_t *text = malloc(*n + 1);
  if (!text) return -1;
  const size_t len = pfp_fasta_text_seqs(*buf, *n, text, tab);
  uint8_t *lines = len == (size_t)-1 ? NULL : malloc(len + tab->nseq + 1);
  if (!lines) { free(text); return -1; }
  uint64_t at = 0;
  for (uint64_t r = 0; r < tab->nseq; r++) {
    memcpy(lines + at, text + tab->start[r], tab->start[r + 1] - tab->start[r]);
    at += tab->start[r + 1] - tab->start[r];
    lines[at++] = '\n';
  }
  free(text); free(*buf);
  *buf = lines; *n = at;
  return 0;
}

/* -l, -l --seqs and --docs after their call: the lines count<TAB>[name:]value ..., count = ep - sp (rows) or the number of items,
 * the names by id (NULL: values alone); the arrays go back */
static int item_lines(const batch_t *b, int rc, int rows, uint32_t *id, uint64_t *val) {
  const uint64_t *oo = b->oo;
  if (rc) return fail(b->base, rc, b->ctx);
  for (uint64_t i = 0; i < b->k; i++) {
    printf("%" PRIu64 "\t", rows ? b->ep[i] - b->sp[i] : oo[i + 1] - oo[i]);
    for (uint64_t j = oo[i]; j < oo[i + 1]; j++) { sep(j, oo[i]); if (id) printf("%s:", b->tab->name[id[j]]); printf("%" PRIu64, val[j]); }
    putchar('\n');
  }
  pfp_free(id); pfp_free(val);
  return 0;
}
static int mode_docs(const batch_t *b) {
  uint32_t *doc = NULL;
  uint64_t *cnt = NULL;
  const int rc = pfp_fm_doclist(b->fm, b->pat, b->off, b->k, b->oo, &doc, &cnt);
  return item_lines(b, rc, 0, doc, cnt);
}
static int mode_locate_seqs(const batch_t *b) {
  uint32_t *sq = NULL;
  uint64_t *so = NULL;
  const int rc = pfp_fm_locate_seqs(b->fm, b->pat, b->off, b->k, b->maxocc, b->sp, b->ep, b->oo, &sq, &so);
  return item_lines(b, rc, 1, sq, so);
}
static int mode_locate(const batch_t *b) {
  uint64_t *pos = NULL;
  const int rc = pfp_fm_locate(b->fm, b->pat, b->off, b->k, b->maxocc, b->sp, b->ep, b->oo, &pos);
  return item_lines(b, rc, 1, NULL, pos);
}

/* -k K, and its -l form */
static int mode_approx(const batch_t *b) {
  uint64_t *hsp = NULL, *hep = NULL, *pos = NULL, *oo = b->oo, *po = b->sp;      /* (po: the positions' offsets) */
  uint8_t *hd = NULL, *pd = NULL;
  int rc = pfp_fm_approx(b->fm, b->pat, b->off, b->k, b->kmis, oo, &hsp, &hep, NULL, &hd);
  if (!rc && b->locate) rc = pfp_fm_approx_locate(b->fm, b->pat, b->off, b->k, b->kmis, b->maxocc, po, &pos, &pd);
  if (rc) rc = fail(b->base, rc, b->ctx);
  for (uint64_t i = 0; !rc && i < b->k; i++) {
    uint64_t by[PFP_FM_APPROX_MAX_K + 1] = {0}, total = 0;
    for (uint64_t j = oo[i]; j < oo[i + 1]; j++) {
      total += hep[j] - hsp[j];
      if (hd[j] <= PFP_FM_APPROX_MAX_K) by[hd[j]] += hep[j] - hsp[j];
    }
    printf("%" PRIu64 "\t", total);
    if (b->locate) for (uint64_t j = po[i]; j < po[i + 1]; j++) { sep(j, po[i]); printf("%" PRIu64 ":%u", pos[j], (unsigned)pd[j]); }
    else for (int d = 0; d <= b->kmis; d++) { sep(d, 0); printf("%" PRIu64, by[d]); }
    putchar('\n');
  }
  pfp_free(hsp); pfp_free(hep); pfp_free(hd); pfp_free(pos); pfp_free(pd);
  return rc;
}

static int mode_count(const batch_t *b) {
  const int rc = pfp_fm_count(b->fm, b->pat, b->off, b->k, b->sp, b->ep, NULL);
  if (rc) return fail(b->base, rc, b->ctx);
  for (uint64_t i = 0; i < b->k; i++) printf("%" PRIu64 "\n", b->ep[i] - b->sp[i]);
  return 0;
}

int main(int argc, char **argv) {
  int locate = 0, device = 0, ms = 0, mems = 0, have_m = 0, thresholds = 0, seqs = 0, docs = 0, rcomp = 0, approx = 0, kmis = 0, align = 0, kedit = 0, cigar = 0, sam = 0, have_sec = 0, paired = 0, have_pair_opt = 0, paf = 0, have_paf_opt = 0, have_fill = 0;
  const char *seqsfile = NULL, *mates2 = NULL;
  uint64_t min_ins = 0, max_ins = 1000, anchors = 8;
  pfp_seqs tab, rtab, rtab2;      /* the collection's table, and with --sam the names of a FASTA / FASTQ file's reads (-2: FILE's) */
  pfp_seqs_init(&tab);
  pfp_seqs_init(&rtab);
  pfp_seqs_init(&rtab2);
  uint64_t maxocc = 0, min_len = 0, seed = 20, have_seed = 0, maxsec = 0, paf_occ = 500, gap = 5000, band = 500, min_score = 40, fill = 500;
  const char *textfile = NULL;
  static struct option lo[] = {{"device", required_argument, 0, 1001}, {"ms", no_argument, 0, 1002}, {"mems", required_argument, 0, 1003},
                               {"text", required_argument, 0, 1004}, {"thresholds", no_argument, 0, 1005}, {"help", no_argument, 0, 'h'},
                               {"seqs", optional_argument, 0, 1006}, {"docs", no_argument, 0, 1007}, {"rc", no_argument, 0, 1008},
                               {"align", required_argument, 0, 1009}, {"seed", required_argument, 0, 1010},
                               {"cigar", no_argument, 0, 1011}, {"sam", required_argument, 0, 1012}, {"secondary", required_argument, 0, 1013},
                               {"paired", no_argument, 0, 1014}, {"ins", required_argument, 0, 1015}, {"anchors", required_argument, 0, 1016},
                               {"paf", no_argument, 0, 1017}, {"max-occ", required_argument, 0, 1018}, {"gap", required_argument, 0, 1019},
                               {"band", required_argument, 0, 1020}, {"min-score", required_argument, 0, 1021},
                               {"fill", required_argument, 0, 1022},
                               {0, 0, 0, 0}};
  int c;
  char *end;
  while ((c = getopt_long(argc, argv, "lm:k:h2:", lo, NULL)) != -1) {
    switch (c) {
      case 'l': locate = 1; break;
      case 'm':
        maxocc = strtoull(optarg, &end, 10);
        if (!*optarg || *end || optarg[0] == '-') { usage(argv[0]); return 2; }
        have_m = 1;
        break;
      case 'k': {
        const long v = strtol(optarg, &end, 10);
        if (!*optarg || *end || v < 0 || v > PFP_FM_APPROX_MAX_K) { usage(argv[0]); return 2; }
        approx = 1;
        kmis = (int)v;
      } break;
      case 1002: ms = 1; break;
      case 1003:
        min_len = strtoull(optarg, &end, 10);
        if (!*optarg || *end || optarg[0] == '-' || min_len < 1) { usage(argv[0]); return 2; }
        mems = 1;
        break;
      case 1004: textfile = optarg; break;
      case 1005: thresholds = 1; break;
      case 1006: seqs = 1; if (optarg) seqsfile = optarg; break;
      case 1007: docs = seqs = 1; break;
      case 1008: rcomp = 1; break;
      case 1009: {
        const long v = strtol(optarg, &end, 10);
        if (!*optarg || *end || v < 0 || v > PFP_FM_EXTEND_MAX_K) { usage(argv[0]); return 2; }
        align = 1;
        kedit = (int)v;
      } break;
      case 1010:
        seed = strtoull(optarg, &end, 10);
        if (!*optarg || *end || optarg[0] == '-' || seed < 1) { usage(argv[0]); return 2; }
        have_seed = 1;
        break;
      case 1011: cigar = 1; break;
      case 1012: {
        const long v = strtol(optarg, &end, 10);
        if (!*optarg || *end || v < 0 || v > PFP_FM_EXTEND_MAX_K) { usage(argv[0]); return 2; }
        sam = 1;
        kedit = (int)v;
      } break;
      case 1013:
        maxsec = strtoull(optarg, &end, 10);
        if (!*optarg || *end || optarg[0] == '-') { usage(argv[0]); return 2; }
        have_sec = 1;
        break;
      case 1014: paired = 1; break;
      case '2': mates2 = optarg; paired = 1; have_pair_opt = 1; break;
      case 1015: {
        min_ins = strtoull(optarg, &end, 10);
        if (!*optarg || optarg[0] == '-' || *end != ':' || !end[1] || end[1] == '-') { usage(argv[0]); return 2; }
        const char *second = end + 1;
        max_ins = strtoull(second, &end, 10);
        if (*end || min_ins > max_ins || max_ins > PFP_FM_WINDOW_MAX_W) { usage(argv[0]); return 2; }
        have_pair_opt = 1;
      } break;
      case 1016:
        anchors = strtoull(optarg, &end, 10);
        if (!*optarg || *end || optarg[0] == '-' || anchors < 1 || anchors > PFP_FM_PAIR_MAX_ANCHORS) { usage(argv[0]); return 2; }
        have_pair_opt = 1;
        break;
      case 1017: paf = 1; break;
      case 1018: case 1019: case 1020: case 1021: {
        const uint64_t v = strtoull(optarg, &end, 10);
        const uint64_t most = c == 1018 ? 65536 : c == 1021 ? UINT32_MAX : INT32_MAX;
        if (!*optarg || *end || optarg[0] == '-' || v < 1 || v > most) { usage(argv[0]); return 2; }
        *(c == 1018 ? &paf_occ : c == 1019 ? &gap : c == 1020 ? &band : &min_score) = v;
        have_paf_opt = 1;
      } break;
      case 1022:
        fill = strtoull(optarg, &end, 10);
        if (!*optarg || *end || optarg[0] == '-' || fill > PFP_FM_FILL_MAX_F) { usage(argv[0]); return 2; }
        have_fill = 1;
        break;
      case 1001:
        device = (int)strtol(optarg, &end, 10);
        if (!*optarg || *end) { usage(argv[0]); return 2; }
        break;
      case 'h': usage(argv[0]); return 0;
      default: usage(argv[0]); return 2;
    }
  }
  if (paf && sam) {      /* (two mappers' outputs on one stream) */
    usage(argv[0]);
    return 1;
  }
  if (paf && (locate || approx || have_m || ms || mems || docs || align || rcomp || paired || have_pair_opt)) {
    fprintf(stderr, "--paf does not combine with the other modes or with --rc (both strands are always searched)\n");
    return 2;
  }
  if (have_paf_opt && !paf) {
    fprintf(stderr, "--max-occ, --gap, --band and --min-score need --paf\n");
    return 2;
  }
  if (have_fill && !(paf && cigar)) {
    fprintf(stderr, "--fill needs --paf --cigar\n");
    return 2;
  }
  if (sam && (locate || approx || have_m || ms || mems || docs || align || cigar || rcomp)) {
    fprintf(stderr, "--sam does not combine with -l, -k, -m, --ms, --mems, --docs, --align, --cigar or --rc (both strands are always searched)\n");
    return 2;
  }
  if ((paired || have_pair_opt) && have_sec) {
    fprintf(stderr, "--paired, -2, --ins and --anchors do not combine with --secondary\n");
    return 2;
  }
  if ((paired || have_pair_opt) && !sam) {
    fprintf(stderr, "--paired, -2, --ins and --anchors need --sam\n");
    return 2;
  }
  if (have_pair_opt && !paired) {
    fprintf(stderr, "--ins and --anchors need --paired or -2 FILE\n");
    return 2;
  }
  if (optind + 2 != argc || ms + mems + locate + docs > 1 || ((ms || mems || docs) && have_m) ||
      ((textfile || thresholds) && !ms && !mems && !align && !sam && !paf) || ((ms || mems) && seqs) || (approx && (ms || mems || docs || seqs)) ||
      (align && (locate || approx || ms || mems || docs || seqs)) || (have_seed && !align && !sam && !paf) || (cigar && !align && !paf) ||
      (have_sec && !sam && !paf)) {
    usage(argv[0]);
    return 2;
  }
  if (sam) seqs = 1;
  const char *patfile = argv[optind], *base = argv[optind + 1];
  /* (everything `done` releases, before the first jump there) */
  uint8_t *pats = NULL, *buf = NULL, *big = NULL;
  uint64_t plen = 0, npat = 0, *lstart = NULL, *off = NULL, *oo = NULL, *sp = NULL, *ep = NULL;
  char *const *qname = NULL;
  char **pnames = NULL;      /* --paired: a name per read */
  uint64_t npnames = 0;
  pfp_ctx *ctx = NULL;
  pfp_fm *fm = NULL;
  int rc = 1;
  if (sam || paf) {      /* plain or gzip-compressed; FASTA / FASTQ becomes one read per line */
    int named = 0;
    if (load_reads(patfile, &pats, &plen, &rtab, &named)) goto done;
    if (named) qname = rtab.name;
  } else if (read_file(patfile, &pats, &plen)) { perror(patfile); goto done; }
  /* npat lines; line k = [lstart[k], lstart[k + 1] - 1) */
  if ((npat = split_lines(pats, plen, &lstart)) == UINT64_MAX) { npat = 0; fprintf(stderr, "out of memory\n"); goto done; }
  if (paired) {
    /* every read gets a name of its own (a line file: the read's line number in its file), and -2 FILE is woven in: the lines
     * become mate 1, mate 2, mate 1, ... */
    uint8_t *p2 = NULL, *woven = NULL;
    uint64_t len2 = 0, n2 = 0, *ls2 = NULL;
    int named2 = 0, bad = 0;
    if (mates2) {
      if (load_reads(mates2, &p2, &len2, &rtab2, &named2)) { free(p2); goto done; }
      if ((n2 = split_lines(p2, len2, &ls2)) == UINT64_MAX) { fprintf(stderr, "out of memory\n"); free(p2); goto done; }
      if (n2 != npat) {
        fprintf(stderr, "%s holds %" PRIu64 " reads and %s holds %" PRIu64 ": the mates 1 and the mates 2 of the same pairs, in the same order\n",
                patfile, npat, mates2, n2);
        free(p2); free(ls2); goto done;
      }
    } else if (npat & 1) {
      fprintf(stderr, "%s holds %" PRIu64 " reads: an interleaved file holds mate 1, mate 2, mate 1, ..., an even number\n", patfile, npat);
      goto done;
    }
    const uint64_t total = mates2 ? 2 * npat : npat;
    pnames = calloc(total + 1, sizeof(char *));
    npnames = total;
    if (mates2) woven = malloc(plen + len2 + 2 * npat + 2);
    if (!pnames || (mates2 && !woven)) bad = 1;
    uint64_t at = 0;
    for (uint64_t r = 0; !bad && r < total; r++) {
      const uint64_t i = mates2 ? r / 2 : r;            /* the read's line in its file */
      const int second = mates2 && (r & 1);
      char *const *src = second ? (named2 ? rtab2.name : NULL) : qname;
      char num[24];
      snprintf(num, sizeof num, "%" PRIu64, i + 1);
      if (!(pnames[r] = strdup(src ? src[i] : num))) bad = 1;
      if (mates2) {
        const uint8_t *from = second ? p2 : pats;
        const uint64_t *ls = second ? ls2 : lstart, ln = ls[i + 1] - 1 - ls[i];
        memcpy(woven + at, from + ls[i], ln);
        at += ln;
        woven[at++] = '\n';
      }
    }
    free(p2); free(ls2);
    if (bad) { fprintf(stderr, "out of memory\n"); free(woven); goto done; }
    if (mates2) {
      free(pats); free(lstart);
      pats = woven; plen = at; lstart = NULL;
      if ((npat = split_lines(pats, plen, &lstart)) == UINT64_MAX) { npat = 0; fprintf(stderr, "out of memory\n"); goto done; }
    }
    qname = pnames;
  }

  rc = pfp_ctx_create(&ctx, device);
  if (rc) { fprintf(stderr, "Cannot initialise the GPU (%s): this tool has no CPU path\n", pfp_strerror(rc)); rc = 1; goto done; }
  if (ms || mems || align || sam || paf) {
    int fd = -1;
    uint64_t n = 0;
    if (textfile) {
      struct stat sb;
      fd = open(textfile, O_RDONLY);
      if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        perror(textfile);
        if (fd >= 0) close(fd);
        rc = 1; goto done;
      }
      n = (uint64_t)sb.st_size;
    }
    rc = pfp_fm_build_ms_files(ctx, base, NULL, fd, 0, n, &fm);
    if (fd >= 0) close(fd);
    if (rc && textfile) fprintf(stderr, "%s: ", textfile);
    if (!rc && thresholds) {
      char thrname[4096];
      snprintf(thrname, sizeof thrname, "%s.thr_pos", base);
      rc = access(thrname, R_OK) == 0 ? pfp_fm_thresholds_files(fm, base) : pfp_fm_thresholds_dev(fm, NULL, 0);
    }
  } else {
    rc = pfp_fm_build_files(ctx, base, locate || docs ? (PFP_FLAG_SSA | PFP_FLAG_ESA) : 0, &fm);
  }
  if (rc) { rc = fail(base, rc, ctx); goto done; }

  if (seqs) {
    char name[4096 + 8], err[1024];
    pfp_fm_info_t inf;
    if (!seqsfile) { snprintf(name, sizeof name, "%s.seqs", base); seqsfile = name; }
    pfp_fm_info(fm, &inf);
    const int bad = pfp_seqs_read(seqsfile, inf.n, &tab, err, sizeof err);
    if (bad) {
      fprintf(stderr, "%s\n", err);
      if (sam && bad == -1) fprintf(stderr, "--sam needs the sequence table of the collection: bigbwt -f --seqs writes it\n");
      rc = 1; goto done;
    }
    if ((rc = pfp_fm_set_seqs(fm, tab.start, tab.nseq)) != 0) { rc = fail(seqsfile, rc, ctx); goto done; }
  }

  uint64_t batch = 1 << 20;
  const char *env = getenv("PFP_FM_BATCH");
  if (env && strtoull(env, NULL, 10) > 0) batch = strtoull(env, NULL, 10);
  if (paired && (batch & 1)) batch++;      /* whole pairs */
  const uint64_t max_bytes = 64ull << 20, mult = rcomp ? 2 : 1;      /* --rc: every line gives two patterns */
  off = malloc((mult * batch + 1) * sizeof(uint64_t)), oo = malloc((mult * batch + 1) * sizeof(uint64_t));
  sp = malloc((mult * batch + 1) * sizeof(uint64_t)), ep = malloc(mult * batch * sizeof(uint64_t));
  buf = malloc(mult * max_bytes + 1);
  if (!off || !oo || !sp || !ep || !buf) { fprintf(stderr, "out of memory\n"); rc = 1; goto done; }
  static char obuf[1 << 20];
  setvbuf(stdout, obuf, _IOFBF, sizeof obuf);
  if (sam) sam_header(&tab);
  pfp_fm_info_t info;
  pfp_fm_info(fm, &info);
  const char *tname = strrchr(base, '/') ? strrchr(base, '/') + 1 : base;
  int (*const mode)(const batch_t *) = paf ? mode_paf : paired ? mode_sam_paired : sam ? mode_sam : ms ? mode_ms : mems ? mode_mems : align ? mode_align : docs ? mode_docs : approx ? mode_approx
                                     : locate && seqs ? mode_locate_seqs : locate ? mode_locate : mode_count;
  for (uint64_t p0 = 0; p0 < npat;) {
    /* a batch: at most `batch` patterns and max_bytes bytes (a single longer line goes alone, from the file buffer) */
    uint64_t k = 0, bytes = 0;
    while (p0 + k < npat && k < batch) {
      const uint64_t len = lstart[p0 + k + 1] - 1 - lstart[p0 + k];
      if (k && bytes + len > max_bytes && !(paired && (k & 1))) break;       /* (--paired: never between the mates of a pair) */
      bytes += len;
      k++;
    }
    const uint8_t *pat = pats + lstart[p0];
    const uint64_t lines = k;
    if (bytes <= max_bytes || rcomp || paired) {
      /* the lines without their '\n' (--rc: each followed by its reverse complement) */
      uint8_t *dst = buf;
      if (bytes > max_bytes) {
        free(big);
        dst = big = malloc(2 * bytes + 1);
        if (!big) { fprintf(stderr, "out of memory\n"); rc = 1; goto done; }
      }
      off[0] = 0;
      k = 0;
      for (uint64_t i = 0; i < lines; i++) {
        const uint64_t len = lstart[p0 + i + 1] - 1 - lstart[p0 + i];
        memcpy(dst + off[k], pats + lstart[p0 + i], len);
        off[k + 1] = off[k] + len;
        k++;
        if (rcomp) {
          revcomp(pats + lstart[p0 + i], len, dst + off[k]);
          off[k + 1] = off[k] + len;
          k++;
        }
      }
      pat = dst;
    } else {
      off[0] = 0; off[1] = bytes;
    }
    const batch_t b = {ctx, fm, base, &tab, pat, off, k, oo, sp, ep, maxocc, min_len, seed, thresholds, locate, kmis, kedit, cigar, min_ins, max_ins, anchors, maxsec, p0, qname,
                       paf_occ, gap, band, min_score, info.n, tname, fill};
    if (mode(&b)) { rc = 1; goto done; }
    p0 += lines;
  }
  rc = 0;
done:
  if (fflush(stdout) != 0 && !rc) { fprintf(stderr, "Error writing the output\n"); rc = 1; }
  pfp_fm_free(fm);
  pfp_ctx_destroy(ctx);
  pfp_seqs_free(&tab);
  pfp_seqs_free(&rtab);
  pfp_seqs_free(&rtab2);
  for (uint64_t r = 0; pnames && r < npnames; r++) free(pnames[r]);
  free(pnames);
  free(off); free(oo); free(sp); free(ep); free(buf); free(big); free(pats); free(lstart);
  return rc;
}
