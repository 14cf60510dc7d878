/* seqs.c -- see seqs.h: the one writer and the one parser of <base>.seqs (bigbwt writes it, bwtsearch and the Python module read it). */
#include "seqs.h"
#include <errno.h>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void pfp_seqs_init(pfp_seqs *t) { memset(t, 0, sizeof *t); }

void pfp_seqs_free(pfp_seqs *t) {
  for (uint64_t k = 0; k < t->nseq; k++) free(t->name[k]);
  free(t->name);
  free(t->start);
  pfp_seqs_init(t);
}

int pfp_seqs_add(pfp_seqs *t, const char *name, size_t name_len, uint64_t length) {
  if (!t->start || t->nseq == t->cap) {
    const uint64_t cap = t->cap ? 2 * t->cap : 64;
    uint64_t *s = realloc(t->start, (cap + 1) * sizeof *s);
    if (!s) return -1;
    if (!t->start) s[0] = 0;
    t->start = s;
    char **nm = realloc(t->name, cap * sizeof *nm);
    if (!nm) return -1;
    t->name = nm;
    t->cap = cap;
  }
  char *copy = malloc(name_len + 1);
  if (!copy) return -1;
  memcpy(copy, name, name_len);
  copy[name_len] = 0;
  t->name[t->nseq] = copy;
  t->start[t->nseq + 1] = t->start[t->nseq] + length;
  t->nseq++;
  return 0;
}

int pfp_seqs_write(const char *path, const pfp_seqs *t) {
  FILE *f = fopen(path, "wb");
  if (!f) return -1;
  int bad = 0;
  for (uint64_t k = 0; k < t->nseq && !bad; k++)
    bad = fprintf(f, "%s\t%" PRIu64 "\t%" PRIu64 "\n", t->name[k], t->start[k], t->start[k + 1] - t->start[k]) < 0;
  if (fclose(f) != 0 || bad) { if (!errno) errno = EIO; return -1; }
  return 0;
}

/* a field of decimal digits, at least one and at most 19 (so it fits) */
static int field_u64(const char *s, const char *e, uint64_t *out) {
  if (s == e || e - s > 19) return -1;
  uint64_t v = 0;
  for (; s < e; s++) {
    if (*s < '0' || *s > '9') return -1;
    v = 10 * v + (uint64_t)(*s - '0');
  }
  *out = v;
  return 0;
}

int pfp_seqs_read(const char *path, uint64_t n, pfp_seqs *t, char *err, size_t err_len) {
  pfp_seqs_init(t);
  if (err_len) err[0] = 0;
  FILE *f = fopen(path, "rb");
  if (!f) { snprintf(err, err_len, "%s: %s", path, strerror(errno)); return -1; }
  char *buf = NULL;
  size_t len = 0, cap = 0;
  for (;;) {
    if (len == cap) {
      cap = cap ? 2 * cap : 1 << 16;
      char *nb = realloc(buf, cap);
      if (!nb) { free(buf); fclose(f); errno = ENOMEM; snprintf(err, err_len, "%s: out of memory", path); return -1; }
      buf = nb;
    }
    const size_t got = fread(buf + len, 1, cap - len, f);
    len += got;
    if (got == 0) break;
  }
  const int rerr = ferror(f);
  fclose(f);
  if (rerr) { free(buf); errno = EIO; snprintf(err, err_len, "%s: read error", path); return -1; }
  uint64_t line = 0;
  int rc = 0;
  for (size_t s = 0; s < len && !rc;) {
    const char *nl = memchr(buf + s, '\n', len - s);
    const char *e = nl ? nl : buf + len;      /* (a last line without its newline is a line) */
    line++;
    const char *t1 = memchr(buf + s, '\t', (size_t)(e - (buf + s)));
    const char *t2 = t1 ? memchr(t1 + 1, '\t', (size_t)(e - (t1 + 1))) : NULL;
    uint64_t start = 0, length = 0;
    if (!t2 || memchr(t2 + 1, '\t', (size_t)(e - (t2 + 1))) || field_u64(t1 + 1, t2, &start) || field_u64(t2 + 1, e, &length)) {
      snprintf(err, err_len, "%s: line %" PRIu64 " does not hold three fields name<TAB>start<TAB>length", path, line);
      rc = -2;
    } else if (start != (t->nseq ? t->start[t->nseq] : 0)) {
      snprintf(err, err_len, "%s: line %" PRIu64 ": start %" PRIu64 " is not the sum of the lengths before it, %" PRIu64, path, line, start,
               t->nseq ? t->start[t->nseq] : 0);
      rc = -2;
    } else if (pfp_seqs_add(t, buf + s, (size_t)(t1 - (buf + s)), length)) {
      snprintf(err, err_len, "%s: out of memory", path);
      errno = ENOMEM;
      rc = -1;
    }
    s = (size_t)(e - buf) + 1;
  }
  free(buf);
  const uint64_t total = t->nseq ? t->start[t->nseq] : 0;
  if (!rc && total != n) {
    snprintf(err, err_len, "%s: line %" PRIu64 " (the last): the lengths sum to %" PRIu64 ", the text holds %" PRIu64 " bytes", path, line, total, n);
    rc = -2;
  }
  if (rc) pfp_seqs_free(t);
  return rc;
}
