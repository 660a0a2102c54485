"""Host model of the LZ77 calls (include/psacx.h: "LZ77 factorization"), for tests/test_lz_model_cpu.py and tests/test_gpu_lz77*.py.

LPF / SRC are stated twice:
  by_bytes(text)          all pairs (i, j < i) by byte comparison: the longest common prefix of every pair, which of the two
                          suffixes is the smaller, and among the earlier suffixes on either side of suffix i the nearest one
  by_ranks(SA, LCP)       the rank walk of the definition: nearest smaller values of SA by a stack, two minima of LCP
and the rest once:
  parse(lpf, src)         the sequential chain s_{k+1} = s_k + min(max(1, LPF[s_k]), n - s_k)
  decode(start, src, text)  byte-by-byte copies; the text is read only at literal phrases
  check_count(text, start, psrc)  the error count of psacx_check_lz77_dev_*, rule by rule
ONES (-1) stands for "all ones" of either index type."""
import json
import os

import numpy as np

import inputs

ONES = -1
NAMED = ["mississippi", "a300", "fib377", "abcab", "dna4096", "tandem3000"]
TINY = ["a1", "aa", "ab"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lz77_named.json")


def text_of(name):
    if name == "mississippi":
        return np.frombuffer(b"mississippi", np.uint8).copy()
    if name == "a300":
        return np.full(300, ord("a"), np.uint8)
    if name == "fib377":
        a, b = b"b", b"a"
        for _ in range(12):
            a, b = b, b + a
        return np.frombuffer(b, np.uint8).copy()
    if name == "abcab":
        return np.frombuffer(b"ab" * 50 + b"c" + b"ab" * 50, np.uint8).copy()
    if name == "dna4096":
        return inputs.dna(4096, 77)
    if name == "tandem3000":
        return inputs.tandem(3000, 97, inputs.dna(97, 5))
    if name == "dna65536":
        return inputs.dna(1 << 16, 78)
    return np.frombuffer({"a1": b"a", "aa": b"aa", "ab": b"ab"}[name], np.uint8).copy()


def _pair_lcps(t, d):
    """l[k] = lcp(S[k + d ..), S[k ..)) for k in [0, n - d): the run of matches from k on"""
    m = t.size - d
    eq = t[d:] == t[:m]
    r = np.arange(m)
    nf = np.where(eq, m, r)
    nf = np.minimum.accumulate(nf[::-1])[::-1]
    return nf - r


def by_bytes(text):
    """(lpf, src) as int64, src ONES where lpf is 0"""
    t = np.ascontiguousarray(text, np.uint8)
    n = int(t.size)
    raw = t.tobytes()
    best = np.zeros((2, n), np.int64)                  # [0]: over the earlier suffixes below suffix i, [1]: over those above
    sides = []
    for d in range(1, n):
        l = _pair_lcps(t, d)                           # pair (i, j) = (k + d, k)
        i = np.arange(d, n)
        ended = i + l == n                             # suffix i is a prefix of suffix j: j is the larger
        at = np.minimum(i + l, n - 1)
        above = ended | (t[at - d] > t[at])
        sides.append((l, above))
        for s in (0, 1):
            sel = above == bool(s)
            np.maximum.at(best[s], i[sel], l[sel])
    lpf, src = np.zeros(n, np.int64), np.full(n, ONES, np.int64)
    cand = [[[], []] for _ in range(n)]
    for d in range(1, n):
        l, above = sides[d - 1]
        i = np.arange(d, n)
        hit = (l > 0) & (l == best[above.astype(np.int64), i])
        for ii, ab in zip(i[hit].tolist(), above[hit].tolist()):
            cand[ii][int(ab)].append(ii - d)
    for i in range(n):
        lp, lq = int(best[0][i]), int(best[1][i])
        if lp >= lq and lp > 0:
            lpf[i], src[i] = lp, max(cand[i][0], key=lambda j: raw[j:])          # the nearest below: the largest of them
        elif lq > 0:
            lpf[i], src[i] = lq, min(cand[i][1], key=lambda j: raw[j:])          # the nearest above: the smallest of them
    return lpf, src


def _nearest_smaller(v):
    n = len(v)
    left, right = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    st = []
    for r in range(n):
        while st and v[st[-1]] >= v[r]:
            st.pop()
        left[r] = st[-1] if st else -1
        st.append(r)
    st = []
    for r in range(n - 1, -1, -1):
        while st and v[st[-1]] >= v[r]:
            st.pop()
        right[r] = st[-1] if st else -1
        st.append(r)
    return left, right


def _range_minima(v, lo, hi):
    """min v[lo[k] .. hi[k]) for lo < hi, by a sparse table"""
    tab = [np.asarray(v, np.int64)]
    while (2 << (len(tab) - 1)) <= len(v):
        h = 1 << (len(tab) - 1)
        tab.append(np.minimum(tab[-1][:-h], tab[-1][h:]))
    k = np.floor(np.log2(np.maximum(hi - lo, 1))).astype(np.int64)
    out = np.zeros(lo.size, np.int64)
    for lev in range(len(tab)):
        sel = k == lev
        out[sel] = np.minimum(tab[lev][lo[sel]], tab[lev][hi[sel] - (1 << lev)])
    return out


def by_ranks(SA, LCP):
    sa, lcp = np.asarray(SA).astype(np.int64), np.asarray(LCP).astype(np.int64)
    n = int(sa.size)
    p, q = _nearest_smaller(sa.tolist())
    r = np.arange(n)
    lp, lq = np.zeros(n, np.int64), np.zeros(n, np.int64)
    hp, hq = p >= 0, q >= 0
    lp[hp] = _range_minima(lcp, p[hp] + 1, r[hp] + 1)
    lq[hq] = _range_minima(lcp, r[hq] + 1, q[hq] + 1)
    lpf, src = np.zeros(n, np.int64), np.full(n, ONES, np.int64)
    first = (lp >= lq) & (lp > 0)
    second = ~first & (lq > 0)
    lpf[sa[first]], src[sa[first]] = lp[first], sa[p[first]]
    lpf[sa[second]], src[sa[second]] = lq[second], sa[q[second]]
    return lpf, src


def chain(lpf):
    """the phrase starts of any n values taken as LPF, with start[z] = n"""
    v = np.asarray(lpf).astype(np.uint64).tolist()
    n, s, out = len(v), 0, []
    while s < n:
        out.append(s)
        s += min(max(1, v[s]), n - s)
    out.append(n)
    return np.asarray(out, np.int64)


def parse(lpf, src):
    """(start with z + 1 entries, psrc with z entries); a phrase with LPF 0 has source ONES"""
    start = chain(lpf)
    at = start[:-1]
    l, s = np.asarray(lpf).astype(np.int64)[at], np.asarray(src).astype(np.int64)[at]
    return start, np.where(l == 0, ONES, s)


def decode(start, src, text):
    """the text the parse stands for; `text` is read at the literal phrases only"""
    out = bytearray()
    for k in range(len(start) - 1):
        a, b, s = int(start[k]), int(start[k + 1]), int(src[k])
        assert a == len(out)
        if s == ONES:
            assert b - a == 1
            out.append(int(text[a]))
        else:
            for t in range(b - a):
                out.append(out[s + t])
    return bytes(out)


def check_count(text, start, psrc):
    """the count of psacx_check_lz77_dev_* (z = len(psrc), start holds z + 1 entries of any value >= 0)"""
    t = np.asarray(text, np.uint8)
    st, ps = np.asarray(start, np.int64), np.asarray(psrc, np.int64)
    n, z = int(t.size), int(ps.size)
    bad = int(st[0] != 0) + int(st[z] != n)
    a, b = st[:-1], st[1:]
    order = b <= a
    bad += int(np.count_nonzero(order))
    bad += int(np.count_nonzero(~order & (ps == ONES) & (b - a != 1)))
    bad += int(np.count_nonzero((ps != ONES) & (ps >= a)))
    if z == 0:
        return bad + n
    x = np.arange(n)
    lo, hi = np.zeros(n, np.int64), np.full(n, z, np.int64)
    while True:
        act = hi - lo > 1
        if not act.any():
            break
        mid = lo + ((hi - lo) >> 1)
        le = st[mid] <= x
        lo = np.where(act & le, mid, lo)
        hi = np.where(act & ~le, mid, hi)
    ka, kb, s = st[lo], st[lo + 1], ps[lo]
    inside = (ka <= x) & (x < kb)
    copy = inside & (s != ONES) & (s < ka)
    at = np.where(copy, s + (x - ka), 0)
    wrong = copy & (t[at] != t)
    return bad + int(np.count_nonzero(~inside)) + int(np.count_nonzero(wrong))


# ---------------------------------------------------------------------------------------------------------------
_arrays, _ranks = {}, {}


def arrays(name):
    """(text, SA, LCP) of a named text, 64-bit, by the oracle"""
    if name not in _arrays:
        import oracle_lib as O
        t = text_of(name)
        ref = O.construct(t, bits=64)
        _arrays[name] = (t, ref["SA"], ref["LCP"])
    return _arrays[name]


def lpf_of(name):
    """by_ranks over the oracle's arrays, computed once per text (the CPU test holds it to by_bytes)"""
    if name not in _ranks:
        t, SA, LCP = arrays(name)
        _ranks[name] = by_ranks(SA, LCP)
    return _ranks[name]


def parse_of(name):
    return parse(*lpf_of(name))


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def cli_text(start, psrc):
    return "".join("%d %d %s\n" % (start[k], start[k + 1] - start[k], "-" if psrc[k] == ONES else str(int(psrc[k]))) for k in range(len(psrc)))


# ---------------------------------------------------------------------------------------------------------------
# LPF arrays that no text has, for the parse alone: name -> values (any uint64)
def synthetic(kind, n, B, top=0xFFFFFFFF):
    rng = np.random.RandomState(len(kind) * 1000 + n % 997)
    if kind == "zeros":
        return np.zeros(n, np.uint64)
    if kind == "ones":
        return np.full(n, top, np.uint64)             # top: all ones of the index type
    if kind == "n":
        return np.full(n, n, np.uint64)
    if kind == "tile_ends":                            # every phrase ends exactly on a tile end: lengths B - (i mod B)
        return (B - np.arange(n) % B).astype(np.uint64)
    if kind == "skip":                                 # tiles are passed over whole
        return np.full(n, B + 1, np.uint64)
    if kind == "geometric":
        return rng.geometric(1.0 / 16, n).astype(np.uint64)
    if kind == "half":                                 # one phrase of half the array between short ones
        v = rng.randint(0, 4, n).astype(np.uint64)
        v[n // 4 - 3:n // 4 + 3] = n // 2
        return v
    raise KeyError(kind)


SYNTHETIC = ["zeros", "ones", "n", "tile_ends", "skip", "geometric", "half"]


if __name__ == "__main__":                             # writes tests/golden/lz77_named.json from the model
    out = {}
    for name in NAMED:
        start, psrc = parse(*by_bytes(text_of(name)))
        out[name] = {"start": [int(x) for x in start], "src": [int(x) for x in psrc]}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
