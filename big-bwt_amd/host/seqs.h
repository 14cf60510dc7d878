/* seqs.h -- the sequence table of a collection: where each record of the text `bigbwt -f` builds begins, and its name.
 * <base>.seqs is a text file, one line per record in input order: name<TAB>start<TAB>length\n.  start is the record's first
 * byte in the text, so start of line 1 is 0, every start is the sum of the lengths before it, and the lengths sum to the
 * text's length n; a record without bytes keeps its line with length 0.  The format is this project's own and can be written by
 * hand for a collection that did not come from FASTA.  Names hold no tab and no newline (kseq ends them at white space). */
#ifndef PFP_SEQS_H
#define PFP_SEQS_H
#include <stddef.h>
#include <stdint.h>
typedef struct {
  uint64_t nseq, cap;
  uint64_t *start;      /* nseq + 1 entries: start[k] of record k, start[nseq] = the total */
  char **name;          /* nseq strings */
} pfp_seqs;
void pfp_seqs_init(pfp_seqs *t);
void pfp_seqs_free(pfp_seqs *t);
/* appends a record of `length` bytes; 0, or -1 when memory runs out */
int pfp_seqs_add(pfp_seqs *t, const char *name, size_t name_len, uint64_t length);
/* 0, or -1 with errno set */
int pfp_seqs_write(const char *path, const pfp_seqs *t);
/* reads a table whose lengths must sum to n into t (initialised here).  0; -1: the file cannot be read (errno); -2: malformed -
 * a line without three fields, a start that is not the running sum, a total that is not n.  err gets a message naming the line. */
int pfp_seqs_read(const char *path, uint64_t n, pfp_seqs *t, char *err, size_t err_len);
#endif
