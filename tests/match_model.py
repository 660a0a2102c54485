"""Host model of the longest-match search (psacx_match_* and psacx_match_gsa_*), from the definitions in include/psacx.h
("longest match and matching statistics").  Texts, string sets and pattern catalogues are those of locate_model and
locate_gsa_model, imported, not copied.

For a query Q of m bytes, len(Q) is the largest d <= m such that Q[:d] is a prefix of some suffix, and [lb, ub) is the locate
interval of Q[:len].  The answer is stated twice:

  by_definition(text, Q, off=None)      the longest d with Q[:d] found by plain substring search (string by string for a set),
                                        then locate_model.by_definition / locate_gsa_model.by_definition of that prefix;
  by_bisection(text, SA, Q, off=None)   the insertion point of Q in the oracle's suffix array, the longer of the common prefixes
                                        with its two neighbours, then by_bisection of the prefix.

with_table states the rule by which a query uses the lookup table, queries_of expands a list of patterns into the queries of
either mode by a plain loop over buffer positions, and cli_text is what `locate --longest` prints.  Nothing here shares code
with the library."""
import numpy as np

import locate_model as L
import locate_gsa_model as G


def _b(x):
    return x.tobytes() if isinstance(x, np.ndarray) else bytes(x)


def common_prefix(a, b):
    d = 0
    while d < len(a) and d < len(b) and a[d] == b[d]:
        d += 1
    return d


def by_definition(text, Q, off=None):
    """(len, lb, ub) from the definition; off: the offsets of a string set."""
    s, Q = _b(text), _b(Q)
    strings = [s] if off is None else [s[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]
    d = len(Q)
    while d > 0 and not any(Q[:d] in x for x in strings):
        d -= 1
    iv = L.by_definition(s, Q[:d]) if off is None else G.by_definition(s, off, Q[:d])
    return d, iv[0], iv[1]


def by_bisection(text, SA, Q, off=None, end=None, lo=0, hi=None):
    """(len, lb, ub) over a suffix array (the oracle's), inside SA[lo:hi] (the whole array by default; a bucket of the table
    otherwise, whose neighbours outside share less than its own prefix).  end: locate_gsa_model.ends_of(off, n), where the caller
    has it."""
    s, Q = _b(text), _b(Q)
    n, m = len(s), len(Q)
    if off is not None and end is None:
        end = G.ends_of(off, n)
    hi = n if hi is None else hi

    def suffix(r):
        p = int(SA[r])
        return s[p:p + m] if end is None else s[p:min(end[p], p + m)]
    a, b = lo, hi
    while a < b:                                            # the insertion point: the first entry whose suffix, cut to m bytes, is >= Q
        mid = (a + b) // 2
        if suffix(mid) < Q:
            a = mid + 1
        else:
            b = mid
    d = 0
    if a > lo:
        d = max(d, common_prefix(suffix(a - 1), Q))
    if a < hi:
        d = max(d, common_prefix(suffix(a), Q))
    iv = L.by_bisection(s, SA, Q[:d], lo, hi) if off is None else G.by_bisection(s, off, SA, Q[:d], lo, hi, end=end)
    return d, iv[0], iv[1]


def with_table(text, SA, table, code, k, Q, off=None, end=None):
    """The answer by the table rule of include/psacx.h (for a correct table and SA): the longest prefix of at most min(m, k) bytes
    whose bucket is not empty comes from the table alone, a byte with code 0 bounds it, and only a query whose first k bytes
    occur, with m > k, is searched -- inside its bucket."""
    Q = _b(Q)
    m, n = len(Q), len(_b(text))
    B = int(code.max()) + 1
    j = min(m, k)
    for i in range(j):
        if int(code[Q[i]]) == 0:
            j = i
            break
    while j > 0:
        v = 0
        for c in Q[:j]:
            v = v * B + int(code[c])
        v *= B ** (k - j)
        w = v + B ** (k - j)
        if table[w] > table[v]:
            break
        j -= 1
    if j == 0:
        return 0, 0, n
    if j == k and m > k:
        return by_bisection(text, SA, Q, off=off, end=end, lo=int(table[v]), hi=int(table[v + 1]))
    return j, int(table[v]), int(table[w])


def queries_of(pats, suffixes=False, max_len=0):
    """The queries of a list of patterns, in result order: one per pattern, or with suffixes one per byte of the pattern buffer --
    slot p belongs to the pattern j with poff[j] <= p < poff[j + 1] and its query is pat[p : poff[j + 1]] -- each cut to max_len
    bytes where max_len > 0."""
    pats = [_b(P) for P in pats]
    if not suffixes:
        out = list(pats)
    else:
        buf = b"".join(pats)
        poff = [0]
        for P in pats:
            poff.append(poff[-1] + len(P))
        out = []
        for p in range(len(buf)):
            j = 0
            while not (poff[j] <= p < poff[j + 1]):
                j += 1
            out.append(buf[p:poff[j + 1]])
    return [Q[:max_len] for Q in out] if max_len else out


def cli_text(ln, lb, ub, occ=None, off=None):
    """What `locate --longest [--set] [--occ]` prints: "len lb ub" per query, then the occurrences as locate prints them."""
    out = []
    for i in range(len(lb)):
        line = "%d %d %d" % (ln[i], lb[i], ub[i])
        if occ is not None:
            for t in range(int(occ[0][i]), int(occ[0][i + 1])):
                line += " %d" % occ[1][t] if off is None else " %d:%d" % (occ[2][t], int(occ[1][t]) - int(off[int(occ[2][t])]))
        out.append(line + "\n")
    return "".join(out)


# ---------------------------------------------------------------------------------------------------------------
# expected answers, computed once per (text, mode) and shared by the tests
# ---------------------------------------------------------------------------------------------------------------
_memo = {}


def answers(key, queries, text, SA, off=None):
    """(len, lb, ub) as int64 arrays of a list of queries by bisection over the oracle's suffix array; memoised under key.  Equal
    queries are answered once."""
    if key not in _memo:
        end = None if off is None else G.ends_of(off, len(_b(text)))
        s = _b(text)
        seen = {}
        rows = []
        for Q in queries:
            if Q not in seen:
                seen[Q] = by_bisection(s, SA, Q, off=off, end=end)
            rows.append(seen[Q])
        _memo[key] = tuple(np.array([r[i] for r in rows], np.int64) for i in range(3))
    return _memo[key]


def expected(name, max_len=0):
    """(patterns, len, lb, ub) of a named text of locate_model on its whole pattern catalogue, one query per pattern."""
    pats = L.patterns_of(name)
    return (pats,) + answers(("plain", name, max_len), queries_of(pats, False, max_len), L.text_of(name), L.sa_of(name))


def expected_gsa(name, max_len=0):
    """The same for a named set of locate_gsa_model."""
    text, off, SA = G.arrays(name)
    pats = G.patterns_of(name)
    return (pats,) + answers(("set", name, max_len), queries_of(pats, False, max_len), text, SA, off)


PIECE_LENGTHS = (1, 7, 8, 9, 63, 64, 65, 130)
HEAD_LENGTHS = (1, 63, 64, 65, 63)


def pieces_of(text, seed=17, count=40):
    """The patterns of the suffix-mode tests: `count` pieces cut from the text, of lengths PIECE_LENGTHS in turn (shorter where the
    text is) after a head of 1, 63, 64, 65 and 63 bytes -- so that on a text of 65 or more bytes patterns end exactly at buffer
    positions 64 and 256, the edges of a wave and of a workgroup, while later ones straddle such edges -- two bytes substituted in each -- one with another byte of the text, one with a byte the text lacks (where it lacks
    one) -- and empty patterns at the front, in the middle and at the end."""
    t = np.asarray(text, np.uint8)
    s, n = t.tobytes(), int(t.size)
    rng = np.random.RandomState(seed)
    present = np.zeros(256, bool)
    present[t] = True
    alphabet = np.nonzero(present)[0]
    absent = [c for c in (0, 255, 66, 120) if not present[c]] or [int(c) for c in np.nonzero(~present)[0][:1]]
    out = [b""]
    for i in range(count):
        m = min((HEAD_LENGTHS + PIECE_LENGTHS * count)[i], n)
        p = int(rng.randint(0, n - m + 1))
        P = bytearray(s[p:p + m])
        P[int(rng.randint(0, m))] = int(alphabet[rng.randint(0, alphabet.size)])
        if absent:
            P[int(rng.randint(0, m))] = absent[i % len(absent)]
        out.append(bytes(P))
        if i == count // 2:
            out += [b"", b""]
    return out + [b""]
