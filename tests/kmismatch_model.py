"""Host model of the pattern search with mismatches (psacx_kmismatch_*; include/psacx.h: "pattern search with mismatches"), for
tests/test_kmismatch_model_cpu.py and tests/test_gpu_kmismatch*.py.

The result is stated twice:
  by_windows(text, off, SA, pats, e)   every window [t, t + m) of the text inside one string, by byte comparison: a hit iff at most e
                                       bytes differ.  The order comes afterwards: (pattern, first piece without a difference,
                                       ISA[t + b_i]).  Sizes up to a few thousand.
  by_pieces(text, off, SA, pats, e)    the pipeline of the header: the intervals of the pieces from locate_model / locate_gsa_model,
                                       every rank a candidate, tested where its window lies inside the text and one string, a hit
                                       iff d <= e and every earlier piece has a difference.  Also gives work = (candidates, tested).
A result is three int64 arrays (qid, tpos, dist) in the pinned order.  off is None for one text, else the m + 1 offsets of the set.
Nothing here shares code with the library."""
import json
import os

import numpy as np

import locate_gsa_model as G
import locate_model as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmismatch_named.json")


def pattern_buffer(pats):
    """(pat as uint8, poff as uint64 with q + 1 entries)"""
    pats = [bytes(P) for P in pats]
    poff = np.zeros(len(pats) + 1, np.uint64)
    poff[1:] = np.cumsum([len(P) for P in pats])
    return np.frombuffer(b"".join(pats), np.uint8).copy(), poff


def cuts(m, e):
    """b_i = floor(i m / (e + 1)) for i = 0 .. e + 1"""
    return [i * m // (e + 1) for i in range(e + 2)]


def ends_array(off, n):
    """end(p) for every text position, as int64 (n everywhere for one text)"""
    if off is None:
        return np.full(n, n, np.int64)
    o = np.asarray(off, np.int64)
    return np.repeat(o[1:], np.diff(o))


def _triples(rows):
    a = np.array(rows, np.int64).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def by_windows(text, off, SA, pats, e):
    t = np.asarray(text, np.uint8)
    n = int(t.size)
    end = ends_array(off, n)
    ISA = np.zeros(n, np.int64)
    ISA[np.asarray(SA, np.int64)] = np.arange(n)
    rows = []
    for j, P in enumerate(pats):
        P = np.frombuffer(bytes(P), np.uint8)
        m = int(P.size)
        if m < e + 1 or m > n:
            continue
        b = cuts(m, e)
        starts = np.arange(n - m + 1)
        starts = starts[starts + m <= end[starts]]
        if starts.size == 0:
            continue
        per_piece = np.zeros((starts.size, e + 1), np.int64)
        for i in range(e + 1):
            for x in range(b[i], b[i + 1]):
                per_piece[:, i] += t[starts + x] != P[x]
        d = per_piece.sum(axis=1)
        keep = d <= e
        first = np.argmax(per_piece[keep] == 0, axis=1)      # (d <= e over e + 1 pieces: one of them has no difference)
        found = [(int(i), int(ISA[s + b[int(i)]]), int(s), int(dd)) for i, s, dd in zip(first, starts[keep], d[keep])]
        rows += [(j, s, dd) for i, r, s, dd in sorted(found)]
    return _triples(rows)


def intervals(text, off, SA, pieces):
    """[lb, ub) of every piece by bisection (the same piece is searched once)"""
    s = np.asarray(text, np.uint8).tobytes()
    end = None if off is None else G.ends_of(off, len(s))
    seen = {}
    for P in pieces:
        if P not in seen:
            seen[P] = L.by_bisection(s, SA, P) if off is None else G.by_bisection(s, off, SA, P, end=end)
    return [seen[P] for P in pieces]


def by_pieces(text, off, SA, pats, e):
    """((qid, tpos, dist), (candidates, tested))"""
    t = np.asarray(text, np.uint8)
    n = int(t.size)
    sa = np.asarray(SA, np.int64)
    end = ends_array(off, n)
    pats = [bytes(P) for P in pats]
    long_enough = [j for j, P in enumerate(pats) if len(P) >= e + 1]
    pieces = [pats[j][b0:b1] for j in long_enough for b0, b1 in zip(cuts(len(pats[j]), e)[:-1], cuts(len(pats[j]), e)[1:])]
    iv = iter(intervals(t, off, sa, pieces))
    out, candidates, tested = [], 0, 0
    for j in long_enough:
        P = np.frombuffer(pats[j], np.uint8)
        m = int(P.size)
        b = cuts(m, e)
        for i in range(e + 1):
            lb, ub = next(iv)
            candidates += ub - lb
            s = sa[lb:ub]
            s = s[(s >= b[i]) & (s < n)]
            w = s - b[i]
            w = w[w + m <= n]
            w = w[w + m <= end[w]]
            tested += int(w.size)
            if w.size == 0:
                continue
            differ = t[w[:, None] + np.arange(m)[None, :]] != P[None, :]
            per_piece = np.add.reduceat(differ.astype(np.int64), b[:-1], axis=1)
            d = per_piece.sum(axis=1)
            keep = (d <= e) & np.all(per_piece[:, :i] > 0, axis=1)
            out.append(np.stack([np.full(int(keep.sum()), j, np.int64), w[keep], d[keep]], axis=1))
    rows = np.concatenate(out) if out else np.zeros((0, 3), np.int64)
    return (rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy()), (int(candidates), int(tested))


def true_hits(text, off, pats, e, got):
    """every reported triple is a hit by byte comparison with exactly that d (the totality clause)"""
    t = np.asarray(text, np.uint8)
    n = int(t.size)
    end = ends_array(off, n)
    for j, w, d in zip(*got):
        P = np.frombuffer(bytes(pats[int(j)]), np.uint8)
        m, w = int(P.size), int(w)
        if m < e + 1 or w < 0 or w + m > n or w + m > end[w] or int(np.sum(t[w:w + m] != P)) != int(d) or d > e:
            return False
    return True


# --------------------------------------------------------------------------------------------------------------- named examples
NAMED = {"mississippi": ([b"mississippi"], [b"issi", b"ssippx", b"m", b"", b"sip"]),
         "abcab_cab": ([b"abcab", b"cab"], [b"cab", b"abc", b"bc", b"cb", b"abcabc"])}


def named_arrays(name):
    """(text, off or None, SA, patterns) of a named example, SA from the definition"""
    import repeats_model as R
    strings, pats = NAMED[name]
    t, off, SA, _ = R.arrays_by_definition(strings)
    return t, (None if len(strings) == 1 else off), SA, pats


def named_results(name):
    t, off, SA, pats = named_arrays(name)
    out = {"SA": SA.tolist(), "patterns": [P.decode() for P in pats]}
    for e in (0, 1, 2):
        got, work = by_pieces(t, off, SA, pats, e)
        out["e%d" % e] = {"triples": [[int(a), int(b), int(c)] for a, b, c in zip(*got)], "work": list(work)}
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# --------------------------------------------------------------------------------------------------------------- the catalogue
def substituted(P, count, rng, alphabet):
    """P with `count` of its bytes replaced by other bytes of the alphabet (fewer where the alphabet has one letter)"""
    P = bytearray(P)
    for at in rng.choice(len(P), min(count, len(P)), replace=False):
        others = [int(c) for c in alphabet if int(c) != P[at]]
        if others:
            P[at] = others[int(rng.randint(0, len(others)))]
    return bytes(P)


REPETITIVE = ("a", "fib", "tandem7")
LENGTHS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 130)          # word masks, piece cuts, and the register / buffer switch at 32


SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097]
TEXTS = ["dna2", "dna4", "a", "fib", "tandem7", "bytes256"]
_cases = {}


def set_offsets(n):
    """the offsets of the set a text of n bytes is cut into: at odd places near the bitmap's word edges, then every 211 bytes"""
    cut = set(x for x in (1, 3, 7, 31, 33, 63, 65, 97, 129, (n // 2) | 1, n - 1) if 0 < x < n)
    cut |= set(range(341, n, 211))
    return np.array([0] + sorted(cut) + [n], np.int64)


class Case(object):
    """A text of the catalogue, as one text (off is None) or cut into a set, with the oracle's suffix array (int64)"""

    def __init__(self, kind, n, as_set, seed=1):
        import oracle_lib as O
        import repeats_model as R
        self.kind, self.n = kind, n
        self.text = np.ascontiguousarray(R.text_of(kind, n, seed), np.uint8)
        self.off = set_offsets(n) if as_set else None
        if as_set:
            ref = O.construct_ss(R.strings_of(self.text, self.off), bits=64, lcp=False)
        else:
            ref = O.construct(self.text, bits=64, lcp=False)
        self.SA = np.asarray(ref["SA"]).astype(np.int64)
        self._pats, self._results = {}, {}

    def patterns(self, e):
        if e not in self._pats:
            self._pats[e] = patterns_of(self.kind, self.text, e, off=self.off)
        return self._pats[e]

    def results(self, e, pats=None, key=None):
        """by_pieces of the case's own patterns (or of pats, memoised under key)"""
        k = (e, key)
        if k not in self._results:
            self._results[k] = by_pieces(self.text, self.off, self.SA, self.patterns(e) if pats is None else pats, e)
        return self._results[k]


def case(kind, n, as_set=False, seed=1):
    k = (kind, n, as_set, seed)
    if k not in _cases:
        _cases[k] = Case(kind, n, as_set, seed)
    return _cases[k]


def patterns_of(kind, text, e, seed=7, off=None):
    """The patterns of a text for e mismatches: pieces of the text of the LENGTHS, the same with 1 .. e + 1 bytes substituted, windows
    that start at 0 and end at n, the whole text, a pattern longer than it, an empty one, m = e and m = e + 1, and a byte the text
    lacks; for a set (off) a window that ends exactly at a string end and one that lies across it.  Repetitive texts get fewer and shorter ones: a piece of a^n owns about n candidates."""
    t = np.asarray(text, np.uint8)
    s, n = t.tobytes(), int(t.size)
    rng = np.random.RandomState(seed + n + 31 * e)
    present = np.zeros(256, bool)
    present[t] = True
    alphabet, absent = np.nonzero(present)[0], np.nonzero(~present)[0]
    few = kind in REPETITIVE
    lengths = (1, 9, 33) if few else LENGTHS
    out = [b""]
    for m in lengths:
        m = min(m, n)
        a = int(rng.randint(0, n - m + 1))
        out.append(s[a:a + m])
        for c in sorted(set([1, e + 1] if few else [1, max(1, e), e + 1])):
            out.append(substituted(s[a:a + m], c, rng, alphabet if alphabet.size > 1 or not absent.size else np.append(alphabet, absent[:1])))
    m = min(n, 12 if few else 40)
    out += [s[:m], s[n - m:], substituted(s[:m], 1, rng, alphabet), substituted(s[n - m:], 1, rng, alphabet)]
    out += [s, s + s[:1]]                                   # the whole text, and a pattern longer than it
    out += [s[:e], s[:min(n, e + 1)], b""]
    if absent.size:
        x = bytes([int(absent[0])])
        out += [x, s[:min(n, 5)] + x + s[:min(n, 5)]]
    if off is not None:                                     # a window that ends exactly at a string end, and one across it
        o = [int(v) for v in off]
        k = len(o) // 2
        if 0 < k < len(o) - 1:
            m = min(9, o[k] - o[k - 1])
            out += [s[o[k] - m:o[k]], s[max(0, o[k] - 4):o[k] + 4]]
    return out
