"""Host model of the pattern search over string sets (psacx_string_ends_dev, psacx_lookup_table_gsa_dev_*, psacx_locate_gsa_*)
and of the occurrence lists (psacx_occurrences_dev_*), from the definitions in include/psacx.h, and the catalogue of string sets
and patterns the CPU and GPU tests share.

text[0..n) holds the m strings back to back, off their m + 1 offsets; end(p) is the offset at which the string holding p ends,
and suffix i is S[i..end(i)).  The interval of a pattern is stated twice, as in locate_model:

  by_definition(text, off, P)     lb = #{i : S[i..end(i)) < P}, ub = lb + #{i : P is a prefix of S[i..end(i))}, counted over all
                                  suffixes with Python's comparison of byte strings;
  by_bisection(text, off, SA, P)  two binary searches over the oracle's generalized suffix array.

The table is stated from key_k (table_by_definition), the rule by which a pattern uses it (with_table) restricts the bisection
to the pattern's bucket, the bitmap is stated bit by bit (ends_bitmap), and the occurrence lists by a plain loop (occurrences).
Nothing here shares code with the library."""
import numpy as np

import gst_model as GT
import locate_model as L
from locate_model import codes_of, key_space, smallest_k_above, table_ks, LENGTHS, MAX_KEYS  # noqa: F401  (for the tests)


def _b(x):
    return x.tobytes() if isinstance(x, np.ndarray) else bytes(x)


def ends_of(off, n):
    """end(p) for every position p in 0 .. n - 1, as a list."""
    off = [int(x) for x in off]
    out = []
    for a, b in zip(off[:-1], off[1:]):
        out += [b] * (b - a)
    assert len(out) == n
    return out


def ends_bitmap(off, n):
    """The (n >> 5) + 1 words of psacx_string_ends_dev: bit p = "a string starts at p, or p == n"."""
    bits = np.zeros((n >> 5) + 1, np.uint32)
    for p in off:
        bits[int(p) >> 5] |= np.uint32(1 << (int(p) & 31))
    return bits


def by_definition(text, off, P):
    s, P = _b(text), _b(P)
    m = len(P)
    end = ends_of(off, len(s))
    # (a suffix is cut to m + 1 bytes before it is compared, as in locate_model.by_definition)
    suf = [s[i:min(e, i + m + 1)] for i, e in enumerate(end)]
    lb = sum(1 for x in suf if x < P)
    return lb, lb + sum(1 for x in suf if x[:m] == P)


def occurrence_set(text, off, P):
    """The positions at which P occurs inside one string, ascending."""
    s, P = _b(text), _b(P)
    m = len(P)
    return [i for i, e in enumerate(ends_of(off, len(s))) if i + m <= e and s[i:i + m] == P]


def by_bisection(text, off, SA, P, lo=0, hi=None, end=None):
    """[lb, ub) inside SA[lo:hi] (the whole array by default).  end: ends_of(off, n), where the caller has it."""
    s, P = _b(text), _b(P)
    m = len(P)
    end = ends_of(off, len(s)) if end is None else end
    hi = len(s) if hi is None else hi
    a, b = lo, hi
    while a < b:                                            # first entry whose suffix, cut to m bytes, is >= P
        mid = (a + b) // 2
        p = int(SA[mid])
        if s[p:min(end[p], p + m)] < P:
            a = mid + 1
        else:
            b = mid
    lb, b = a, hi
    while a < b:                                            # first entry whose suffix, cut to m bytes, is > P
        mid = (a + b) // 2
        p = int(SA[mid])
        if s[p:min(end[p], p + m)] <= P:
            a = mid + 1
        else:
            b = mid
    return lb, a


def keys_by_definition(text, off, k):
    """key_k(i) = sum_j c_j B^(k-1-j), c_j = code(S[i+j]) if i + j < end(i), else 0 -- for every position, as int64."""
    t = np.asarray(text, np.uint8)
    n = int(t.size)
    code, sigma = codes_of(t)
    B = sigma + 1
    end = np.asarray(ends_of(off, n), np.int64)
    pos = np.arange(n, dtype=np.int64)
    padded = np.concatenate([code[t].astype(np.int64), np.zeros(k, np.int64)])
    keys = np.zeros(n, np.int64)
    for j in range(k):
        keys = keys * B + np.where(pos + j < end, padded[j:j + n], 0)
    return keys, B


def table_by_definition(text, off, k):
    """table[v] = #{i : key_k(i) < v} for v in [0, B^k]."""
    keys, B = keys_by_definition(text, off, k)
    table = np.zeros(B ** k + 1, np.int64)
    table[1:] = np.cumsum(np.bincount(keys, minlength=B ** k))
    return table


def with_table(text, off, SA, table, code, k, P, end=None):
    """The interval by the rule of include/psacx.h, 'Use of the table by a pattern' (for a correct table and SA)."""
    P = _b(P)
    m = len(P)
    B = int(code.max()) + 1
    j = min(m, k)
    cs = [int(code[c]) for c in P[:j]]
    if any(c == 0 for c in cs):
        return by_bisection(text, off, SA, P, end=end)
    v = 0
    for c in cs:
        v = v * B + c
    v *= B ** (k - j)
    w = v + B ** (k - j)
    if m <= k:
        return int(table[v]), int(table[w])
    return by_bisection(text, off, SA, P, int(table[v]), int(table[v + 1]), end=end)


def occurrences(SA, n, lb, ub, limit=0, off=None):
    """(start, pos, sid) of psacx_occurrences_dev_* by a plain loop; sid is None without offsets."""
    start, pos, sid = [0], [], []
    for a, b in zip(lb, ub):
        a, b = int(a), int(b)
        c = b - a if a <= b <= n else 0
        if limit and c > limit:
            c = limit
        for t in range(c):
            p = int(SA[a + t])
            pos.append(p)
            if off is not None:
                sid.append(len(off) - 1 if p >= n else max(s for s in range(len(off) - 1) if int(off[s]) <= p))
        start.append(start[-1] + c)
    return (np.array(start, np.uint64), np.array(pos, np.uint64), None if off is None else np.array(sid, np.uint64))


def string_ids(off, pos, n):
    """sid of occurrences() for many positions at once (the same rule by searchsorted)."""
    o = np.asarray(off, np.int64)
    p = np.asarray(pos, np.uint64)
    inside = p < np.uint64(n)
    return np.where(inside, np.searchsorted(o, np.where(inside, p, 0).astype(np.int64), side="right") - 1, o.size - 1).astype(np.uint64)


def cli_text(lb, ub, occ=None, off=None):
    """What `locate [--set] [--occ]` prints: "lb ub" per pattern, then its occurrences (occ = (start, pos, sid)): positions, or
    string:offset-in-string for a set."""
    out = []
    for i in range(len(lb)):
        line = "%d %d" % (lb[i], ub[i])
        if occ is not None:
            for t in range(int(occ[0][i]), int(occ[0][i + 1])):
                line += " %d" % occ[1][t] if off is None else " %d:%d" % (occ[2][t], int(occ[1][t]) - int(off[int(occ[2][t])]))
        out.append(line + "\n")
    return "".join(out)


# ---------------------------------------------------------------------------------------------------------------
# string sets and patterns
# ---------------------------------------------------------------------------------------------------------------
READS = "reads100"                                          # 2 000 DNA reads of 100 characters (CPU model and timing shape)
READS_SMALL = "reads100_650"                                # its first 650: 65 000 characters, what the GPU tests take
GST = list(GT.ALL)                                          # TINY, EDGES, word_edges, copies, prefixes, unary, tandem_pieces, single, bytes256
ALL = GST + [READS_SMALL, READS]
GPU = GST + [READS_SMALL]                                   # texts of at most 2^16 characters
_sets, _arrays, _expected = {}, {}, {}


def strings_of(name):
    if name in GST:
        return GT.strings_of(name)
    if name not in _sets:
        import inputs
        genome = inputs.dna(50000, 31)
        starts = np.random.RandomState(32).randint(0, genome.size - 100, 2000)
        reads = [genome[s:s + 100] for s in starts]
        _sets[READS], _sets[READS_SMALL] = reads, reads[:650]
    return _sets[name]


def add_set(name, strings):
    """A further named set, for a test that needs a size of its own; the catalogue lists (GST, ALL, GPU) do not change."""
    if name not in _sets:
        _sets[name] = list(strings)
    return name


def arrays(name):
    """(text, off, SA) of a named set: the oracle's generalized suffix array (64-bit), equal suffixes in text order."""
    if name not in _arrays:
        if name in GST:
            text, off, SA = GT.arrays(name)[:3]
        else:
            import oracle_lib as O
            ref = O.construct_ss(strings_of(name), bits=64)
            text, off, SA = ref["text"], np.asarray(ref["off"], np.uint64), ref["SA"]
        _arrays[name] = (np.asarray(text, np.uint8), np.asarray(off, np.uint64), SA)
    return _arrays[name]


WORD_EDGES = (31, 32, 33, 63, 64, 65)


def patterns_of(name, seed=5):
    """The patterns of a set, as a list of bytes:
      - for every length of LENGTHS: pieces of the text at its start, its end and seeded positions -- cut without regard to the
        strings, so many straddle two of them -- and the same with the last byte one up and one down;
      - every whole string (at most 200 of them, spread over the set);
      - a string plus the first two characters of the next one (at most 60);
      - suffixes of the strings that end exactly at bitmap bit 31, 32, 33, 63, 64 and 65, where an offset lies there;
      - the longest string with one more byte, below and above;
      - pieces with a byte the text lacks at position 0, k - 1 and k for the k of table_ks (where the text lacks one);
      - random patterns over the alphabet, 1 to 12 bytes."""
    text, off, SA = arrays(name)
    s, n = text.tobytes(), int(text.size)
    o = [int(x) for x in off]
    m_strings = len(o) - 1
    rng = np.random.RandomState(seed)
    present = np.zeros(256, bool)
    present[text] = True
    absent = [c for c in (0, 255, 66, 120) if not present[c]] or [int(c) for c in np.nonzero(~present)[0][:1]]      # (none in bytes256)
    alphabet = np.nonzero(present)[0].astype(np.uint8)
    ks = table_ks(text)[0]
    out = []
    for m in LENGTHS:
        if m == 0:
            out.append(b"")
            continue
        if m > n:
            continue
        for p in sorted(set([0, n - m] + [int(x) for x in rng.randint(0, n - m + 1, 3)])):
            sub = s[p:p + m]
            out.append(sub)
            if sub[-1] < 255:
                out.append(sub[:-1] + bytes([sub[-1] + 1]))
            if sub[-1] > 0:
                out.append(sub[:-1] + bytes([sub[-1] - 1]))
            for at in sorted(set(x for x in [0] + [k - 1 for k in ks] + list(ks) if 0 <= x < m and absent)):
                out.append(sub[:at] + bytes([absent[at % len(absent)]]) + sub[at + 1:])
    step = max(1, m_strings // 200)
    for t in range(0, m_strings, step):
        out.append(s[o[t]:o[t + 1]])
    for t in range(0, m_strings - 1, max(1, m_strings // 60)):
        out.append(s[o[t]:min(n, o[t + 1] + 2)])             # must not be found here (it may occur elsewhere)
    for t in range(m_strings):
        if o[t + 1] in WORD_EDGES:
            for ln in sorted(set([1, 2, min(9, o[t + 1] - o[t]), o[t + 1] - o[t]])):
                if ln <= o[t + 1] - o[t]:
                    out.append(s[o[t + 1] - ln:o[t + 1]])
                    out.append(s[o[t + 1] - ln:min(n, o[t + 1] + 1)])
    longest = max(range(m_strings), key=lambda t: o[t + 1] - o[t])
    whole = s[o[longest]:o[longest + 1]]
    out += [whole + bytes([int(text.min())]), whole + bytes([int(text.max())])] + [whole + bytes([c]) for c in absent[:1]]
    for ln in rng.randint(1, 13, 60):
        out.append(alphabet[rng.randint(0, alphabet.size, int(ln))].tobytes())
    return out


def expected(name):
    """(patterns, lb, ub) of a named set: the intervals by bisection over the oracle's generalized suffix array."""
    if name not in _expected:
        text, off, SA = arrays(name)
        pats = patterns_of(name)
        end = ends_of(off, int(text.size))
        s = text.tobytes()
        iv = [by_bisection(s, off, SA, P, end=end) for P in pats]
        _expected[name] = (pats, np.array([a for a, b in iv], np.int64), np.array([b for a, b in iv], np.int64))
    return _expected[name]
