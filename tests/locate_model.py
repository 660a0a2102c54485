"""Host model of the pattern search (psacx_locate_*) and of its lookup table (psacx_lookup_table_*), from the definitions in
include/psacx.h, and the catalogue of texts and patterns the CPU and GPU tests share.

The interval of a pattern is stated twice:

  by_definition(text, P)     lb = #{i : S[i..n) < P}, ub = lb + #{i : P is a prefix of S[i..n)}, counted over all suffixes with
                             Python's comparison of byte strings (unsigned bytes, a proper prefix is smaller);
  by_bisection(text, SA, P)  two binary searches over a suffix array (the oracle's): the first entry whose suffix, cut to m
                             bytes, is not below P, and the first that is above it.

The lookup table is stated from its definition (table_by_definition: the keys of all positions, counted), and the rule by which a
pattern uses it (with_table) restricts the bisection to the pattern's bucket -- or answers from the table alone when m <= k.
Nothing here shares code with the library."""
import numpy as np

MAX_KEYS = 1 << 30                                          # B^k beyond this: PSACX_EINVAL
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65]           # and n, n + 1 of each text


def _b(x):
    return x.tobytes() if isinstance(x, np.ndarray) else bytes(x)


def by_definition(text, P):
    s, P = _b(text), _b(P)
    n, m = len(s), len(P)
    # (a suffix is cut to m + 1 bytes before it is compared: a longer one compares with P, which has m, as that piece does)
    lb = sum(1 for i in range(n) if s[i:i + m + 1] < P)
    return lb, lb + sum(1 for i in range(n) if s[i:i + m] == P)


def by_bisection(text, SA, P, lo=0, hi=None):
    """[lb, ub) inside SA[lo:hi] (the whole array by default)."""
    s, P = _b(text), _b(P)
    m = len(P)
    hi = len(s) if hi is None else hi
    a, b = lo, hi
    while a < b:                                            # first entry with S[SA[mid]:][:m] >= P
        mid = (a + b) // 2
        p = int(SA[mid])
        if s[p:p + m] < P:
            a = mid + 1
        else:
            b = mid
    lb, b = a, hi
    while a < b:                                            # first entry with S[SA[mid]:][:m] > P
        mid = (a + b) // 2
        p = int(SA[mid])
        if s[p:p + m] <= P:
            a = mid + 1
        else:
            b = mid
    return lb, a


def codes_of(text):
    """(code[256] as uint16, sigma): 1..sigma in byte order of the bytes that occur, 0 for an absent byte."""
    present = np.zeros(256, bool)
    present[np.unique(np.asarray(text, np.uint8))] = True
    code = np.zeros(256, np.uint16)
    code[present] = np.arange(1, int(present.sum()) + 1)
    return code, int(present.sum())


def key_space(B, k):
    """B^k, or None where the library refuses the table."""
    e = B ** k
    return e if e <= MAX_KEYS else None


def smallest_k_above(B, limit):
    k = 1
    while B ** k <= limit:
        k += 1
    return k


def table_by_definition(text, k):
    """table[v] = #{i : key_k(i) < v} for v in [0, B^k], key_k(i) = sum_j code(S[i+j]) B^(k-1-j) with code 0 past the end."""
    t = np.asarray(text, np.uint8)
    code, sigma = codes_of(t)
    B = sigma + 1
    padded = np.concatenate([code[t].astype(np.int64), np.zeros(k, np.int64)])
    keys = np.zeros(t.size, np.int64)
    for j in range(k):
        keys = keys * B + padded[j:j + t.size]
    table = np.zeros(B ** k + 1, np.int64)
    table[1:] = np.cumsum(np.bincount(keys, minlength=B ** k))
    return table


def with_table(text, SA, table, code, k, P):
    """The interval by the rule of include/psacx.h, 'Use of the table by a pattern' (for a correct table and SA)."""
    P = _b(P)
    m, n = len(P), len(_b(text))
    B = int(code.max()) + 1
    j = min(m, k)
    cs = [int(code[c]) for c in P[:j]]
    if any(c == 0 for c in cs):
        return by_bisection(text, SA, P)
    v = 0
    for c in cs:
        v = v * B + c
    v *= B ** (k - j)
    w = v + B ** (k - j)
    if m <= k:
        return int(table[v]), int(table[w])
    return by_bisection(text, SA, P, int(table[v]), int(table[v + 1]))


# ---------------------------------------------------------------------------------------------------------------
# texts and patterns
# ---------------------------------------------------------------------------------------------------------------
TINY = ["tiny%d" % n for n in (1, 2, 3, 7, 8, 9, 17)]
EDGES = ["edge%d" % n for n in (63, 64, 65, 4095, 4096, 4097)]
SMALL = ["mississippi"] + TINY + EDGES + ["unary", "tandem", "bytes256"]
ALL = SMALL + ["dna"]
_texts, _sa = {}, {}


def text_of(name):
    """mississippi, the two-letter texts tiny1..17 and edge63..4097 of the checker models (intervals on both sides of 64 entries),
    unary (5000 x 'a': suffixes shorter than the pattern matter), tandem (period 37 x 1000), bytes256 (bytes 0, 1, 127, 128, 254
    and 255: a signed comparison orders them wrongly), dna (300 000)."""
    if name not in _texts:
        import checker_model as G
        import st_checker_model as S
        if name.startswith("tiny"):
            _texts[name] = G.text_of(name)
        elif name == "bytes256":
            _texts[name] = np.array([0, 1, 127, 128, 254, 255], np.uint8)[np.random.RandomState(12).randint(0, 6, 1500)]
        else:
            _texts[name] = S.text_of(name)
    return _texts[name]


def add_text(name, text):
    """A further named text, for a test that needs a size of its own; the catalogue lists (SMALL, ALL) do not change."""
    if name not in _texts:
        _texts[name] = np.ascontiguousarray(text, dtype=np.uint8)
    return name


def sa_of(name):
    """The oracle's suffix array of a named text (64-bit entries)."""
    if name not in _sa:
        import oracle_lib as O
        _sa[name] = O.construct(text_of(name), bits=64, lcp=False)["SA"]
    return _sa[name]


def table_ks(text):
    """The table sizes every text is tested with: k = 1, 2 and the smallest k with B^k > 2^16; and the smallest k the library refuses."""
    B = codes_of(text)[1] + 1
    return [1, 2, smallest_k_above(B, 1 << 16)], smallest_k_above(B, MAX_KEYS)


def patterns_of(name, seed=3):
    """The patterns of a text, as a list of bytes: for every length of LENGTHS, n and n + 1 -- substrings of the text (its start, its
    end, seeded positions), the same with the last byte one up and one down, the text's end extended past n, runs of a byte below
    and above every byte of the text, and substrings with a byte the text lacks at position 0, k - 1, k and last for the k of
    table_ks; then a pattern just below the smallest suffix and one just above the largest."""
    t = text_of(name)
    s, n = t.tobytes(), int(t.size)
    rng = np.random.RandomState(seed)
    present = np.zeros(256, bool)
    present[t] = True
    absent = [c for c in (0, 255, 66, 120) if not present[c]] or [int(np.nonzero(~present)[0][0])]
    lo_byte, hi_byte = int(t.min()), int(t.max())
    ks = table_ks(t)[0]
    out = []
    for m in LENGTHS + [n, n + 1]:
        if m == 0:
            out.append(b"")
            continue
        starts = sorted(set([0, max(0, n - m)] + [int(x) for x in rng.randint(0, max(1, n - m + 1), 3)])) if m <= n else []
        for p in starts:
            sub = s[p:p + m]
            out.append(sub)
            last = sub[-1]
            if last < 255:
                out.append(sub[:-1] + bytes([last + 1]))
            if last > 0:
                out.append(sub[:-1] + bytes([last - 1]))
            for pos in sorted(set(x for x in [0, m - 1] + [k - 1 for k in ks] + list(ks) if 0 <= x < m)):
                out.append(sub[:pos] + bytes([absent[pos % len(absent)]]) + sub[pos + 1:])
        tail = s[max(0, n - (m - 1)):]                      # the end of the text and one or more bytes beyond it
        out.append(tail + s[:1] * (m - len(tail)))
        out.append(tail + bytes([absent[0]]) * (m - len(tail)))
        if lo_byte > 0:
            out.append(bytes([lo_byte - 1]) * m)
        if hi_byte < 255:
            out.append(bytes([hi_byte + 1]) * m)
        out.append(bytes([lo_byte]) * m)
        out.append(bytes([hi_byte]) * m)
    SA = sa_of(name)
    first, last = s[int(SA[0]):], s[int(SA[n - 1]):]
    nz = [p for p, c in enumerate(first) if c > 0]
    if nz:
        out.append(first[:nz[0]] + bytes([first[nz[0]] - 1]))          # below the smallest suffix
    out.append(last + b"\x00")                                          # above the largest
    return out


_expected = {}


def expected(name):
    """(patterns, lb, ub) of a named text: the intervals by bisection over the oracle's suffix array."""
    if name not in _expected:
        pats = patterns_of(name)
        s, SA = text_of(name).tobytes(), sa_of(name)
        iv = [by_bisection(s, SA, P) for P in pats]
        _expected[name] = (pats, np.array([a for a, b in iv], np.int64), np.array([b for a, b in iv], np.int64))
    return _expected[name]
