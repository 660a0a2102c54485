"""Host model of the suffix-prefix overlaps of a string set (psacx_overlaps_*), from the definitions in include/psacx.h.  The result
is stated twice:

  by_bytes(text, off, min_len, whole)            all pairs by byte comparison: for every string j and every asked depth d,
                                                 T(j, d) = the positions whose suffix IS the first d bytes of string j, and
                                                 olb(j, d) = the number of suffixes below those bytes; a slot is (olb, olb + |T|)
                                                 where T is not empty and (0, 0) otherwise.
  by_walk(off, SA, ISA, LCP, min_len, whole)     the walk from ISA[o_j] towards the root over the oracle's arrays: a scalar
                                                 previous-smaller search in LCP per step, a bit test of the string end, a
                                                 linear scan for the end of the run.  The text is not read.

pairs_by_bytes lists the overlaps themselves as (target, pos, sid) and pairs_of_slots expands slots over SA into the same list.
Nothing here shares code with the library."""
import numpy as np


def _b(x):
    return x.tobytes() if isinstance(x, np.ndarray) else bytes(x)


def depths(L, min_len, whole):
    """the depths asked of a string of L bytes"""
    return range(max(1, min_len), (L if whole else L - 1) + 1)


def by_bytes(text, off, min_len, whole=False):
    """(lb, ub) as int64 arrays of n entries: slot o_j + d - 1 belongs to (j, d)."""
    s = _b(text)
    n, o = len(s), [int(x) for x in off]
    end = []
    for a, b in zip(o[:-1], o[1:]):
        end += [b] * (b - a)
    suf = [s[i:end[i]] for i in range(n)]
    order = sorted(suf)                                     # (a proper prefix is smaller: an end sorts below every character)
    count = {}
    for x in suf:
        count[x] = count.get(x, 0) + 1
    first = {}
    for r, x in enumerate(order):
        first.setdefault(x, r)                              # the number of suffixes below x, for an x that is one
    lb, ub = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for j in range(len(o) - 1):
        for d in depths(o[j + 1] - o[j], min_len, whole):
            X = s[o[j]:o[j] + d]
            if X in count:
                lb[o[j] + d - 1], ub[o[j] + d - 1] = first[X], first[X] + count[X]
    return lb, ub


def pairs_by_bytes(text, off, min_len, whole=False):
    """The overlaps as a sorted list of (slot, pos, sid): the suffix of string sid that starts at pos is the first d bytes of
    string j, with slot = o_j + d - 1.  Borders of j and whole strings that are prefixes of j are among them."""
    s = _b(text)
    n, o = len(s), [int(x) for x in off]
    m = len(o) - 1
    out = []
    for j in range(m):
        for d in depths(o[j + 1] - o[j], min_len, whole):
            X = s[o[j]:o[j] + d]
            for t in range(m):
                if o[t + 1] - o[t] >= d and s[o[t + 1] - d:o[t + 1]] == X:
                    out.append((o[j] + d - 1, o[t + 1] - d, t))
    return sorted(out)


def pairs_of_slots(off, SA, lb, ub):
    """(slot, pos, sid) of every SA entry inside a slot's interval, sorted"""
    o = np.asarray(off, np.int64)
    out = []
    for p in np.nonzero(np.asarray(ub) > np.asarray(lb))[0]:
        for x in range(int(lb[p]), int(ub[p])):
            pos = int(SA[x])
            out.append((int(p), pos, int(np.searchsorted(o, pos, side="right")) - 1))
    return sorted(out)


def by_walk(off, SA, ISA, LCP, min_len, whole=False, steps=None):
    """The slots by the walk of include/psacx.h ("suffix-prefix overlaps"); steps: a list that receives the steps per string."""
    o = [int(x) for x in off]
    n = o[-1]
    SA, LCP = [int(x) for x in SA], [int(x) for x in LCP]
    ends = set(o)
    lb, ub = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for j in range(len(o) - 1):
        L = o[j + 1] - o[j]
        r = int(ISA[o[j]])
        i, d, taken = r, (L if whole else L - 1), 0
        while d >= max(1, min_len):
            taken += 1
            if LCP[i] >= d:
                x = i - 1
                while x >= 0 and LCP[x] > d - 1:              # the previous value <= d - 1, one entry at a time
                    x -= 1
                if x < 0:
                    break
                i = x
            if SA[i] + d in ends:
                if d < L:
                    hi = r
                else:
                    hi = r + 1
                    while hi < n and LCP[hi] > d - 1:
                        hi += 1
                x = i + 1
                while x < hi and SA[x] + d in ends:
                    x += 1
                lb[o[j] + d - 1], ub[o[j] + d - 1] = i, x
            d = LCP[i]
        if steps is not None:
            steps.append(taken)
    return lb, ub


def cli_text(off, pairs):
    """What `overlaps --list` prints: "target source length" per (slot, pos, sid), in slot and SA order."""
    o = np.asarray(off, np.int64)
    out = []
    for p, pos, sid in pairs:
        j = int(np.searchsorted(o, p, side="right")) - 1
        out.append("%d %d %d\n" % (j, sid, p - int(o[j]) + 1))
    return "".join(out)


# ---------------------------------------------------------------------------------------------------------------
# string sets
# ---------------------------------------------------------------------------------------------------------------
def word_edges_set():
    """one letter, lengths 31, 32, 33 and 64: string ends at bits 31, 63, 96 and 160 = n"""
    return [b"a" * 31, b"a" * 32, b"a" * 33, b"a" * 64]


NAMED = {
    "abab": [b"abab", b"babab", b"ab", b"abab"],
    "unary": [b"aaaa", b"aaa", b"aa", b"a"],
    "single": [b"a"],
    "xxx": [b"x", b"x", b"x"],
    "word_edges": word_edges_set(),
    "copies300": [b"acgtacgt"] * 300,
    "borders": [b"abcab", b"cabca", b"abc", b"bcabc", b"c", b"abcabcab"],
}
SMALL = ["abab", "unary", "single", "xxx", "word_edges", "borders"]       # all pairs by bytes in no time


def reads(mutate=False):
    """512 reads of 64 bytes from 4096 random DNA; mutate: 2 % of their bytes substituted"""
    rng = np.random.RandomState(20)
    letters = np.frombuffer(b"ACGT", np.uint8)
    genome = rng.randint(0, 4, 4096)                        # as codes 0 .. 3
    starts = rng.randint(0, 4096 - 64 + 1, 512)
    out = [genome[s:s + 64].copy() for s in starts]
    if mutate:
        for x in out:
            hit = np.nonzero(rng.rand(64) < 0.02)[0]
            x[hit] = (x[hit] + rng.randint(1, 4, hit.size)) % 4          # another letter, never the same
    return [letters[x].tobytes() for x in out]


_sets = {}


def strings_of(name):
    if name == "reads":
        return reads()
    if name == "reads_mut":
        return reads(True)
    return NAMED[name]


def set_arrays(name):
    """(text, off, SA, ISA, LCP) of a named set, 64-bit, by the oracle"""
    if name not in _sets:
        import oracle_lib as O
        ref = O.construct_ss(strings_of(name), bits=64)
        _sets[name] = (np.asarray(ref["text"], np.uint8), np.asarray(ref["off"], np.uint64), ref["SA"], ref["ISA"], ref["LCP"])
    return _sets[name]


def min_lens(name):
    """1, 2 and the longest string's length"""
    return sorted(set([1, 2, max(len(x) for x in strings_of(name))]))


_slots = {}


def slots(name, min_len, whole):
    """by_walk over the oracle's arrays, computed once per case (the CPU test holds it to by_bytes)"""
    key = (name, min_len, bool(whole))
    if key not in _slots:
        text, off, SA, ISA, LCP = set_arrays(name)
        _slots[key] = by_walk(off, SA, ISA, LCP, min_len, whole)
    return _slots[key]
