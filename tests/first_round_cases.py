"""Inputs for the tests of the sorters' first round by tiles of 256 slots (heads0_kernel / write_back0_kernel) and of plain
mode's late rank[], with plain numpy models that say which history an input reaches.  test_first_round_cases.py checks, without a
GPU, that every input is what its name claims; test_first_round_parse.py and test_first_round_dict.py run them on the GPU."""
import numpy as np

import parse_keys_cases as K

TILE = 256                       # slots per workgroup of the first round's two kernels (kTile)
SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 1500)
TOP_PLAIN = 1 << 29              # a symbol this large leaves no room for the run key: the key is the two whole symbols
FINISH_CMP = 2048                # symbols the comparison finisher reads before it refuses (kFinishCmp / 4)


# ------------------------------------------------------------------------------------------ integer strings (Context.sacak_int)
def distinct(n):
    """a permutation of 1 .. n - 1, then the 0: no pair of neighbours occurs twice, every first-round group is a singleton"""
    return np.concatenate([np.random.default_rng(n).permutation(n - 1) + 1, [0]]).astype(np.uint32)


def periodic(n):
    """1 2 3 1 2 3 ... 0: three groups of about n / 3 suffixes each"""
    return np.concatenate([np.arange(n - 1) % 3 + 1, [0]]).astype(np.uint32)


def constant(n):
    """A A A ... A 0 with A too large for the run key: all suffixes but the last two share the key (A, A) - one group from slot 2 on"""
    return np.concatenate([np.full(n - 1, TOP_PLAIN), [0]]).astype(np.uint32)


def fibonacci(n):
    """the Fibonacci word over {1, 2}, cut to n - 1 symbols, then the 0: equal neighbours (1 1), so the run key"""
    a, b = [1], [1, 2]
    while len(b) < n:
        a, b = b, b + a
    return np.asarray(b[:n - 1] + [0], dtype=np.uint32)


KINDS = {"distinct": distinct, "periodic": periodic, "constant": constant, "fibonacci": fibonacci}
STRINGS = {"%s_%d" % (kind, n): (lambda f=f, n=n: f(n)) for kind, f in KINDS.items() for n in SIZES}


def first_round_groups(s):
    """The first round of the integer sorter, in numpy: (order, head) - the suffixes in (key, position) order and head[t] = first
    slot of slot t's group.  The key is the pair of symbols and, for two equal symbols under the run layout, how the run ends
    (its remaining length and whether a larger symbol follows it); the plain layout (64 - 2 sb < 6) has the pair alone."""
    s = np.asarray(s, dtype=np.int64)
    N = len(s)
    nxt = np.concatenate([s[1:], [0]])
    run_layout = 64 - 2 * K.bits_for(int(s.max())) >= K.RUN_BITS_MIN
    r = np.zeros(N, dtype=np.int64)
    up = np.zeros(N, dtype=np.int64)
    if run_layout:
        end = N - 1                                  # last position of the run that holds i
        for i in range(N - 1, -1, -1):
            if i == N - 1 or s[i] != s[i + 1]:
                end = i
            if i + 1 < N and s[i] == s[i + 1]:
                r[i] = end - i + 1
                up[i] = 1 if end + 1 < N and s[end + 1] > s[i] else 0
    e = np.where(up == 1, (1 << 40) - r, r)          # (order inside a pair of equal symbols; only equality matters here)
    order = np.lexsort((np.arange(N), e, nxt, s))
    ks, kn, ke = s[order], nxt[order], e[order]
    is_head = np.concatenate([[True], (ks[1:] != ks[:-1]) | (kn[1:] != kn[:-1]) | (ke[1:] != ke[:-1])])
    head = np.maximum.accumulate(np.where(is_head, np.arange(N), 0))
    return order, head


def unresolved(head):
    """slots the first round leaves unresolved: the members of groups of two or more"""
    size = np.bincount(head, minlength=len(head))
    return int((size[head] >= 2).sum())


# ------------------------------------------------------------------------------------------ parses (Context.bwtparse with counts)
def far_variants():
    """three copies of 3000 symbols, each with one symbol of its own 50 symbols before its end: after the pivot round most members
    still equal their pivot for kIntPivCap symbols, and the finisher meets comparisons longer than it reads - doubling rounds follow
    a pivot round"""
    return K.copies_parse(K.perm_base(3000, 61), 3, {(k, 2950 + 7 * k): None for k in range(3)})


# ------------------------------------------------------------------------------------------ texts (the fused chain)
def _rand(seed, n, runs=()):
    return {"kind": "rand", "seed": seed, "n": n, "alphabet_hex": "41434754", "runs": [list(r) for r in runs]}


# name -> (spec for textgen.make_text, w, p)
TEXTS = {
    "run_400": (_rand("fr400", 20000, [(5000, 400, 0x4E)]), 10, 100),      # one group of 257 .. 512 slots
    "run_700": (_rand("fr700", 20000, [(9000, 700, 0x4E)]), 10, 100),      # one group of more than 512 slots
}
RESOLVED = "tiny_dna_w4"             # the golden whose dictionary the first round settles alone
PREFIX = 64                          # bytes no first-round key reaches beyond (63 key bits, at least one bit a byte)


def prefix_classes(dict_bytes, w, length=PREFIX):
    """sizes of the classes of kept dictionary suffixes (longer than w) that share their first `length` bytes with no terminator
    among them: each class lies inside one first-round group, in consecutive slots"""
    d = np.frombuffer(bytes(dict_bytes), dtype=np.uint8)
    ends = np.flatnonzero(d <= 1)
    nxt_end = ends[np.searchsorted(ends, np.arange(len(d)))]
    left = nxt_end - np.arange(len(d))               # bytes before the terminator
    at = np.flatnonzero((left >= length) & (left > w))
    if len(at) == 0:
        return np.zeros(0, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(d, length)[at]
    _, counts = np.unique(win, axis=0, return_counts=True)
    return counts
