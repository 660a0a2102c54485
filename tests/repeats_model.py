"""Host model of the BWT and repeat calls (include/psacx.h: "BWT and repeats"), for tests/test_repeats_model_cpu.py and
tests/test_gpu_bwt.py / test_gpu_repeats.py.

The repeats are stated three times:
  by_bytes(strings)              every substring of the strings with its occurrences and the sets of what stands to its left and to
                                 its right, a string start and a string end being a neighbour different from everything.  Right-maximal:
                                 at least two occurrences and more than one right neighbour; maximal: more than one on both sides;
                                 supermaximal: a maximal repeat that is a substring of no other maximal repeat.  n <= about 150.
  by_intervals(SA, LCP, bwt, first)   the bottom-up stack traversal of the LCP-intervals, which keeps the head of each; left-diversity
                                 and pairwise-distinctness by loops over bwt / first.  Any n.
  by_searches(LCP, bwt, first)   the formulation of the header, rank by rank: previous / next smaller value by a plain walk, the bit
                                 arrays D, F and St through prefix sums.  Small n (quadratic on a^n).
and once each: bwt_of (from the definition), inverse_bwt (LF walk), select (the filters).
A result is a list of (head, lb, ub, len), sorted by head."""
import json
import os

import numpy as np

import inputs

RIGHT, MAXIMAL, SUPER = 0, 1, 2
KINDS = {"right": RIGHT, "maximal": MAXIMAL, "super": SUPER}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "repeats_named.json")


def flatten(strings):
    """(text as uint8, offsets as int64 with m + 1 entries)"""
    parts = [np.frombuffer(bytes(s), np.uint8) for s in strings]
    off = np.zeros(len(parts) + 1, np.int64)
    off[1:] = np.cumsum([p.size for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)).copy(), off


def strings_of(text, offsets=None):
    t = np.asarray(text, np.uint8)
    if offsets is None:
        return [t.tobytes()]
    return [t[int(offsets[s]):int(offsets[s + 1])].tobytes() for s in range(len(offsets) - 1)]


def arrays_by_definition(strings):
    """(text, offsets, SA, LCP) as int64: every suffix ends with its string (an end sorts below every byte), equal suffixes lie in
    text order, LCP is cut at the string ends"""
    t, off = flatten(strings)
    sufs = []
    for s in range(len(off) - 1):
        b, e = int(off[s]), int(off[s + 1])
        sufs += [(t[i:e].tobytes(), i) for i in range(b, e)]
    sufs.sort()
    SA = np.array([i for _, i in sufs], np.int64)
    LCP = np.zeros(len(sufs), np.int64)
    for j in range(1, len(sufs)):
        a, b = sufs[j - 1][0], sufs[j][0]
        c = 0
        while c < len(a) and c < len(b) and a[c] == b[c]:
            c += 1
        LCP[j] = c
    return t, off, SA, LCP


def bwt_of(text, SA, offsets=None):
    """(bwt as uint8, first as bool, primary or -1) from the definition"""
    t, sa = np.asarray(text, np.uint8), np.asarray(SA).astype(np.int64)
    n = int(t.size)
    off = np.array([0, n], np.int64) if offsets is None else np.asarray(offsets).astype(np.int64)
    starts = np.zeros(n + 1, bool)
    starts[off[:-1]] = True
    last = np.zeros(n + 1, np.int64)                   # last[p]: the last position of the string that holds p
    for s in range(off.size - 1):
        last[off[s]:off[s + 1]] = off[s + 1] - 1
    first = starts[sa]
    bwt = np.where(first, t[last[sa]], t[np.maximum(sa - 1, 0)]).astype(np.uint8)
    at = np.nonzero(sa == 0)[0]
    return bwt, first, (int(at[0]) if at.size else -1)


def inverse_bwt(bwt, primary):
    """the one text whose SA-aligned BWT this is: the row of the end marker goes back in, then the LF walk from it"""
    b = np.asarray(bwt, np.uint8)
    n = int(b.size)
    if n == 0:
        return b""
    col = np.concatenate(([int(b[primary]) + 1], b.astype(np.int64) + 1))      # the last column of the text with an end marker 0
    col[primary + 1] = 0
    order = np.argsort(col, kind="stable")
    lf = np.empty(n + 1, np.int64)
    lf[order] = np.arange(n + 1)
    lf, col = lf.tolist(), col.tolist()
    out, r = bytearray(n), 0
    for k in range(n - 1, -1, -1):
        out[k] = col[r] - 1
        r = lf[r]
    return bytes(out)


# --------------------------------------------------------------------------------------------------------------- (a)
def by_bytes(strings):
    """{kind: set of (len, occurrence positions as a sorted tuple)}; positions count the strings back to back"""
    info = {}
    base = 0
    for sid, s in enumerate(strings):
        s = bytes(s)
        for i in range(len(s)):
            left = s[i - 1] if i else ("start", sid)
            for j in range(i + 1, len(s) + 1):
                right = s[j] if j < len(s) else ("end", sid)
                occ, ls, rs = info.setdefault(s[i:j], ([], set(), set()))
                occ.append(base + i)
                ls.add(left)
                rs.add(right)
        base += len(s)
    right = {w for w, (occ, ls, rs) in info.items() if len(occ) >= 2 and len(rs) > 1}
    maximal = {w for w in right if len(info[w][1]) > 1}
    sup = {w for w in maximal if not any(w != v and w in v for v in maximal)}
    named = lambda ws: {(len(w), tuple(sorted(info[w][0]))) for w in ws}  # noqa: E731
    return {RIGHT: named(right), MAXIMAL: named(maximal), SUPER: named(sup)}


def as_occurrences(result, SA):
    sa = np.asarray(SA).astype(np.int64)
    return {(int(ln), tuple(sorted(sa[lb:ub].tolist()))) for _, lb, ub, ln in result}


# --------------------------------------------------------------------------------------------------------------- (b)
def intervals(LCP):
    """(head, lb, ub, len) of every LCP-interval below the root, by the stack traversal; sorted by head"""
    L = np.asarray(LCP).astype(np.uint64).tolist()
    n = len(L)
    if n:
        L[0] = 0
    out, stack = [], [(0, 0, 0)]                      # (len, lb, head)
    for i in range(1, n + 1):
        cur = L[i] if i < n else 0                    # (the end closes everything but the root)
        lb, head = i - 1, i
        while stack[-1][0] > cur:
            ln, lb, h = stack.pop()
            out.append((h, lb, i, ln))
        if stack[-1][0] < cur:
            stack.append((cur, lb, head))
    out.sort()
    return out


def _range_reduce(v, lo, hi, op):
    """op over v[lo[k] .. hi[k]) for lo < hi (op = np.minimum or np.maximum), by a sparse table"""
    tab = [np.asarray(v)]
    while (2 << (len(tab) - 1)) <= len(v):
        h = 1 << (len(tab) - 1)
        tab.append(op(tab[-1][:-h], tab[-1][h:]))
    k = np.floor(np.log2(np.maximum(hi - lo, 1))).astype(np.int64)
    out = np.zeros(lo.size, tab[0].dtype)
    for lev in range(len(tab)):
        sel = k == lev
        out[sel] = op(tab[lev][lo[sel]], tab[lev][hi[sel] - (1 << lev)])
    return out


def by_intervals(LCP, bwt=None, first=None, kind=RIGHT):
    out = intervals(LCP)
    if kind == RIGHT or not out:
        return out
    L = np.asarray(LCP).astype(np.uint64)
    L[0] = 0
    b, f = np.asarray(bwt).astype(np.int64), np.asarray(first, bool)
    lb, ub, ln = triples(out)
    starts = np.concatenate(([0], np.cumsum(f)))
    starts = starts[ub] - starts[lb]
    if kind == MAXIMAL:                                # a string start, or two different bytes
        ok = (starts > 0) | (_range_reduce(b, lb, ub, np.minimum) != _range_reduce(b, lb, ub, np.maximum))
        return [r for r, good in zip(out, ok.tolist()) if good]
    # flat (no LCP value of the interval above its length), at most 256 ranks that start no string, and their bytes all different
    ok = (_range_reduce(L, lb + 1, ub, np.maximum) == ln.astype(np.uint64)) & ((ub - lb) - starts <= 256)
    keep = []
    for r, good in zip(out, ok.tolist()):
        if good:
            rest = b[r[1]:r[2]][~f[r[1]:r[2]]].tolist()
            if len(set(rest)) == len(rest):
                keep.append(r)
    return keep


# --------------------------------------------------------------------------------------------------------------- (c)
def by_searches(LCP, bwt=None, first=None, kind=RIGHT):
    L = np.asarray(LCP).astype(np.uint64).tolist()
    n = len(L)
    if n:
        L[0] = 0
    if kind != RIGHT:
        b, f = np.asarray(bwt).tolist(), [bool(x) for x in np.asarray(first)]
        D = [0] + [int(f[x] or f[x - 1] or b[x] != b[x - 1]) for x in range(1, n)]
        St = [0] + [int(L[x] != L[x - 1]) for x in range(1, n)]
        cD, cF, cS = (np.concatenate(([0], np.cumsum(v))).tolist() for v in (D, [int(x) for x in f], St))
    out = []
    for j in range(1, n):
        ln = L[j]
        if ln == 0:
            continue
        h = j - 1
        while L[h] > ln:
            h -= 1
        if L[h] == ln:
            continue
        e = j + 1
        while e < n and L[e] >= ln:
            e += 1
        lb, ub = h, e
        if kind == MAXIMAL and cD[ub] - cD[lb + 1] == 0:
            continue
        if kind == SUPER:
            if lb + 2 < ub and cS[ub] - cS[lb + 2] != 0:
                continue
            if (ub - lb) - (cF[ub] - cF[lb]) > 256:
                continue
            rest = [b[x] for x in range(lb, ub) if not f[x]]
            if len(set(rest)) != len(rest):
                continue
        out.append((j, lb, ub, ln))
    return out


def select(result, min_len=0, min_occ=0, max_occ=0):
    return [r for r in result if r[3] >= min_len and r[2] - r[1] >= max(2, min_occ) and (max_occ == 0 or r[2] - r[1] <= max_occ)]


def triples(result):
    """(lb, ub, len) as three int64 arrays, in the order of the heads"""
    a = np.asarray([r[1:] for r in result], np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


# ---------------------------------------------------------------------------------------------------------------
NAMED = {"mississippi": [b"mississippi"], "banana": [b"banana"], "abcab_cab": [b"abcab", b"cab"], "aaaa": [b"aaaa"]}


def named_results(name):
    """{kind name: [[lb, ub, len], ...]} and the arrays, from the definitions"""
    t, off, SA, LCP = arrays_by_definition(NAMED[name])
    bwt, first, primary = bwt_of(t, SA, off)
    out = {"SA": SA.tolist(), "LCP": LCP.tolist(), "bwt": bwt.tolist(), "first": [int(x) for x in first], "primary": primary}
    for kn, k in KINDS.items():
        out[kn] = [[int(lb), int(ub), int(ln)] for _, lb, ub, ln in by_intervals(LCP, bwt, first, k)]
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def words(name, rows):
    """the repeats of a golden entry as "word x occurrences" strings, sorted"""
    t, off = flatten(NAMED[name])
    sa = golden()[name]["SA"]
    return sorted("%s x%d" % (t[sa[lb]:sa[lb] + ln].tobytes().decode(), ub - lb) for lb, ub, ln in rows)


# --------------------------------------------------------------------------------------------------------------- texts of the GPU tests
def fibonacci(n):
    a, b = b"b", b"a"
    while len(b) < n:
        a, b = b, b + a
    return np.frombuffer(b[:n], np.uint8).copy()


def text_of(kind, n, seed=1):
    if kind == "dna2":
        return np.frombuffer(b"AC", np.uint8)[(inputs.splitmix64_stream(n, seed) & np.uint64(1)).astype(np.int64)]
    if kind == "dna4":
        return inputs.dna(n, seed)
    if kind == "a":
        return np.full(n, ord("a"), np.uint8)
    if kind == "fib":
        return fibonacci(n)
    if kind == "tandem7":
        return inputs.tandem(n, 7, np.frombuffer(b"ACGTTCA", np.uint8))
    if kind == "bytes256":
        return (inputs.splitmix64_stream(n, seed) & np.uint64(255)).astype(np.uint8)
    if kind == "planted":                              # reads with a planted repeat: the same 40 bytes at three places
        t = inputs.dna(n, seed).copy()
        w = min(40, n // 4)
        for at in (n // 7, n // 2, n - w):
            t[at:at + w] = t[:w]
        return t
    raise KeyError(kind)


TEXTS = ["dna2", "dna4", "a", "fib", "tandem7", "bytes256", "planted"]


def random_set(n, m, seed, sigma=4):
    """m strings over sigma letters with n bytes in all (every string has at least one byte)"""
    rng = np.random.RandomState(seed)
    t = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, sigma, n)]
    cuts = np.sort(rng.choice(np.arange(1, n), m - 1, replace=False)) if m > 1 else np.zeros(0, np.int64)
    off = np.concatenate(([0], cuts, [n])).astype(np.int64)
    return [t[off[s]:off[s + 1]].tobytes() for s in range(m)]


if __name__ == "__main__":                             # writes tests/golden/repeats_named.json from the model
    with open(GOLDEN, "w") as f:
        json.dump({name: named_results(name) for name in sorted(NAMED)}, f, separators=(",", ":"))
        f.write("\n")
