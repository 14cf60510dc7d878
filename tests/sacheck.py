"""Linear-time suffix-array checker in numpy: a second reference for the suffix sorters that shares no code with the
library or with the oracle (oracle/pfp_oracle.c sorts by prefix doubling).

The textbook check: `sa` is a permutation of 0..n-1, and for every pair of neighbours a = sa[i], b = sa[i+1]
  * s[a] <= s[b];
  * where the first symbols are equal and ordinary, the suffixes one position on are in order: rank[a+1] < rank[b+1];
  * where both are a separator of a gsacak collection (byte 1 after every string, one 0 after the last): a < b - gsacak orders
    equal suffixes by the index of their string (gsa/gsacak.h:78-105), which is position order.
By induction over the suffix length the correct array is the only one that passes.

kinds: "bytes" (sacak: bytes ending in a unique 0), "int" (sacak_int: uint32 symbols ending in a unique 0), "gsa" (gsacak).
"""
import numpy as np


def sa_error(s, sa, kind):
    """None if `sa` is the suffix array of `s`, else a one-line description of the first fault found."""
    assert kind in ("bytes", "int", "gsa")
    s = np.asarray(s)
    sa = np.asarray(sa)
    n = len(s)
    if len(sa) != n:
        return f"length {len(sa)} != {n}"
    if n == 0:
        return None
    if s[n - 1] != 0 or (n > 1 and int(s[:-1].min()) == 0):
        return "the string does not end in a unique 0"
    if kind == "gsa" and n > 1 and s[n - 2] != 1:
        return "the collection does not end in 1 0"
    sa64 = sa.astype(np.int64)
    if int(sa64.min()) < 0 or int(sa64.max()) >= n:
        return "an entry is outside 0..n-1"
    seen = np.zeros(n, dtype=bool)
    seen[sa64] = True
    if not seen.all():
        miss = int(np.flatnonzero(~seen)[0])
        return f"not a permutation: position {miss} is missing"
    if n == 1:
        return None
    rank = np.empty(n, dtype=np.int64)
    rank[sa64] = np.arange(n, dtype=np.int64)
    a, b = sa64[:-1], sa64[1:]
    ca, cb = s[a], s[b]
    bad = ca > cb
    eq = ca == cb
    # equal first symbols: neither suffix is the last position (its 0 is unique), so a + 1 and b + 1 exist
    if kind == "gsa":
        sep = eq & (ca == 1)
        bad |= sep & (a > b)
        eq &= ~sep
    ae, be = a[eq], b[eq]
    wrong = np.zeros(n - 1, dtype=bool)
    wrong[eq] = rank[ae + 1] > rank[be + 1]
    bad |= wrong
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        return f"slots {i}, {i + 1} (positions {int(a[i])}, {int(b[i])}) are out of order"
    return None


def assert_sa(s, sa, kind, what=""):
    err = sa_error(s, sa, kind)
    assert err is None, f"{what}: {err}" if what else err
