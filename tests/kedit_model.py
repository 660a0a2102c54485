"""Host model of the pattern search with edits (psacx_kedit_*; include/psacx.h: "pattern search with edits"), for
tests/test_kedit_model_cpu.py and tests/test_gpu_kedit*.py.

For pattern j of m bytes and a start t:  D(j, t) = min over 0 <= L <= end(t) - t of ed(P_j, S[t .. t + L)), L(j, t) the smallest L that
attains it; a hit is (j, t, L, D) with D <= e, and a pattern with m <= e has none.  The result is stated twice:
  by_definition(text, off, pats, e)    the whole dynamic programme from every start of every string, over every L up to the end of
                                       the string.  Texts up to a few hundred bytes.
  by_pieces(text, off, SA, pats, e)    the pipeline of the header: the intervals of the e + 1 pieces from locate_model /
                                       locate_gsa_model, every rank a candidate with s = SA[r] and t0 = s - b_i, the starts
                                       [max(start of s's string, t0 - e), min(s, t0 + e)], each decided by a dynamic programme in the
                                       band |L - i| <= e over the text up to min(end(t), t + m + e); the raw hits, and their unique.
                                       Also gives work = (candidates, raw hits).
A result is four int64 arrays (qid, tpos, len, dist) in ascending (pattern, t).  off is None for one text, else the m + 1 offsets of
the set.  Nothing here shares code with the library."""
import json
import os

import numpy as np

import kmismatch_model as X

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kedit_named.json")
BIG = 1 << 20

pattern_buffer, cuts, ends_array, intervals = X.pattern_buffer, X.cuts, X.ends_array, X.intervals
case, set_offsets, TEXTS, SIZES, REPETITIVE, NAMED, named_arrays = X.case, X.set_offsets, X.TEXTS, X.SIZES, X.REPETITIVE, X.NAMED, X.named_arrays
LENGTHS = tuple(m for m in X.LENGTHS if m > 1)


def starts_array(off, n):
    """the start of the string of every text position, as int64 (0 everywhere for one text)"""
    if off is None:
        return np.zeros(n, np.int64)
    o = np.asarray(off, np.int64)
    return np.repeat(o[:-1], np.diff(o))


def _quads(rows):
    a = np.array(sorted(rows), np.int64).reshape(-1, 4)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(), a[:, 3].copy()


def all_starts(t, end, P):
    """(D, L) of the pattern P from every start of the text, by the full dynamic programme: row i holds ed(P[0..i), S[t .. t + L)) for
    every L up to the end of t's string"""
    n = int(t.size)
    room = end - np.arange(n)                                  # the largest L of every start
    width = int(room.max())
    ar = np.arange(width + 1)
    allowed = ar[None, :] <= room[:, None]
    at = np.arange(n)[:, None] + ar[None, :-1]                 # the text position of the byte that takes L to L + 1
    chars = np.where(at < end[:, None], t[np.minimum(at, n - 1)], -1)
    F = np.where(allowed, ar[None, :], BIG)
    for c in P:
        G = np.empty_like(F)
        G[:, 0] = F[:, 0] + 1
        G[:, 1:] = np.minimum(F[:, :-1] + (chars != c), F[:, 1:] + 1)
        G = np.minimum.accumulate(G - ar[None, :], axis=1) + ar[None, :]       # insertions: G[L] = min over L' <= L of G[L'] + L - L'
        F = np.where(allowed, np.minimum(G, BIG), BIG)
    return F.min(axis=1), F.argmin(axis=1)


def by_definition(text, off, pats, e):
    t = np.asarray(text, np.uint8)
    n = int(t.size)
    end = ends_array(off, n)
    rows = []
    for j, P in enumerate(pats):
        P = np.frombuffer(bytes(P), np.uint8)
        if P.size <= e or n == 0:
            continue
        D, L = all_starts(t, end, P)
        rows += [(j, int(s), int(L[s]), int(D[s])) for s in np.nonzero(D <= e)[0]]
    return _quads(rows)


def banded(t, end, P, e, starts):
    """(D, L) of P from the given starts in the band |L - i| <= e over the text up to min(end(t), t + m + e): exact wherever D <= e;
    D > e elsewhere.  A start whose whole row exceeds e is dropped from the rows that follow: row minima never fall."""
    n, m = int(t.size), int(P.size)
    T = np.asarray(starts, np.int64)
    D, Lout = np.full(T.size, BIG, np.int64), np.zeros(T.size, np.int64)
    live = np.nonzero(np.minimum(end[T], T + m + e) - T >= m - e)[0]      # ed(P, W) >= m - |W|: a start with less text than m - e behind it is none
    T = T[live]
    lmax = (np.minimum(end[T], T + m + e) - T)[:, None]
    ks = np.arange(2 * e + 1, dtype=np.int16)[None, :]
    far = np.int16(1 << 12)                                    # "outside", in the 16-bit cells of the rows (e <= 15)
    padded = np.append(t, np.uint8(0))                         # (the byte behind the text is never compared: ok is False there)
    L = ks.astype(np.int64) - e
    F = np.where((L >= 0) & (L <= lmax), L, far).astype(np.int16)
    for i in range(m):
        L = i + 1 - e + ks.astype(np.int64)
        inside = (L >= 0) & (L <= lmax)
        ok = inside & (L >= 1)
        diag = np.where(ok, F + (padded[np.clip(T[:, None] + L - 1, 0, n)] != P[i]), far)
        G = np.minimum(diag[:, :-1], F[:, 1:] + np.int16(1))
        G = np.concatenate([G, diag[:, -1:]], axis=1)
        G = np.minimum.accumulate(G - ks, axis=1) + ks
        F = np.where(inside, np.minimum(G, far), far).astype(np.int16)
        if i % 16 == 15 or T.size == 1:
            keep = F.min(axis=1) <= e
            if not keep.all():
                F, T, lmax, live = F[keep], T[keep], lmax[keep], live[keep]
            if T.size == 0:
                return D, Lout
    D[live], Lout[live] = F.min(axis=1), m - e + F.argmin(axis=1)
    return D, Lout


def by_pieces(text, off, SA, pats, e):
    """((qid, tpos, len, dist), (candidates, raw hits))"""
    t = np.asarray(text, np.uint8)
    n = int(t.size)
    sa = np.asarray(SA, np.int64)
    end, first = ends_array(off, n), starts_array(off, n)
    pats = [bytes(P) for P in pats]
    long_enough = [j for j, P in enumerate(pats) if len(P) > e]
    pieces = [pats[j][b0:b1] for j in long_enough for b0, b1 in zip(cuts(len(pats[j]), e)[:-1], cuts(len(pats[j]), e)[1:])]
    iv = iter(intervals(t, off, sa, pieces) if n else [])
    rows, candidates, raw = [], 0, 0
    for j in long_enough:
        P = np.frombuffer(pats[j], np.uint8)
        b = cuts(int(P.size), e)
        asked = []
        for i in range(e + 1):
            lb, ub = next(iv)
            candidates += ub - lb
            s = sa[lb:ub]
            s = s[(s >= 0) & (s < n)]
            for dt in range(-e, e + 1):
                w = s - b[i] + dt
                asked.append(w[(w >= first[s]) & (w <= s)])
        asked = np.concatenate(asked) if asked else np.zeros(0, np.int64)
        if asked.size == 0:
            continue
        T, times = np.unique(asked, return_counts=True)
        D, L = banded(t, end, P, e, T)
        hit = D <= e
        raw += int(times[hit].sum())
        rows += [(j, int(a), int(l), int(d)) for a, l, d in zip(T[hit], L[hit], D[hit])]
    return _quads(rows), (int(candidates), int(raw))


def best(got):
    """the hits whose distance is the smallest among their pattern's hits (PSACX_KEDIT_BEST), stated directly"""
    qid, tpos, ln, dist = got
    least = {}
    for j, d in zip(qid.tolist(), dist.tolist()):
        least[j] = min(d, least.get(j, d))
    keep = np.array([d == least[j] for j, d in zip(qid.tolist(), dist.tolist())], bool).reshape(-1)
    return qid[keep], tpos[keep], ln[keep], dist[keep]


def true_hits(text, off, pats, e, got):
    """every reported quadruple is a hit with exactly that L and D by the banded programme from its own start, and none comes twice
    (the totality clause)"""
    t = np.asarray(text, np.uint8)
    n = int(t.size)
    end = ends_array(off, n)
    qid, tpos, ln, dist = got
    if np.unique(np.stack([qid, tpos]), axis=1).shape[1] != qid.size:
        return False
    for j in np.unique(qid):
        P = np.frombuffer(bytes(pats[int(j)]), np.uint8)
        at = qid == j
        if P.size <= e or np.any(tpos[at] < 0) or np.any(tpos[at] >= n):
            return False
        D, L = banded(t, end, P, e, tpos[at])
        if np.any(D > e) or not np.array_equal(D, dist[at]) or not np.array_equal(L, ln[at]):
            return False
    return True


# --------------------------------------------------------------------------------------------------------------- named examples
def named_results(name):
    t, off, SA, pats = named_arrays(name)
    out = {"SA": SA.tolist(), "patterns": [P.decode() for P in pats]}
    for e in (0, 1, 2):
        got, work = by_pieces(t, off, SA, pats, e)
        out["e%d" % e] = {"quadruples": [[int(x) for x in row] for row in zip(*got)], "work": list(work)}
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# --------------------------------------------------------------------------------------------------------------- the catalogue
def edited(P, count, rng, alphabet):
    """P after `count` edits at random places: substitutions by another byte of the alphabet, insertions of one, deletions"""
    P = bytearray(P)
    for _ in range(count):
        op = int(rng.randint(0, 3)) if P else 1
        at = int(rng.randint(0, len(P) + (op == 1)))
        if op == 0:
            others = [int(c) for c in alphabet if int(c) != P[at]]
            if others:
                P[at] = others[int(rng.randint(0, len(others)))]
        elif op == 1:
            P.insert(at, int(alphabet[int(rng.randint(0, len(alphabet)))]))
        else:
            del P[at]
    return bytes(P)


_pats, _results = {}, {}


def patterns_of(kind, text, e, seed=11, off=None):
    """The patterns of a text for e edits: windows of the LENGTHS, unedited and with 1, e and e + 1 edits; a deletion and an insertion
    at the first and at the last byte; windows at 0 and at n; the whole text and one byte more; m = e and m = e + 1; the empty pattern;
    a byte the text lacks; for a set (off) a window that ends exactly at a string end, one across it and one that starts within e of
    a string start.  Repetitive texts get windows of 9, 33, 64, 65 and 130 bytes up to n = 257 and fewer and shorter ones beyond: a piece
    of a^n owns about n candidates."""
    t = np.asarray(text, np.uint8)
    s, n = t.tobytes(), int(t.size)
    rng = np.random.RandomState(seed + n + 31 * e)
    present = np.zeros(256, bool)
    present[t] = True
    alphabet, absent = np.nonzero(present)[0], np.nonzero(~present)[0]
    letters = alphabet if alphabet.size > 1 or not absent.size else np.append(alphabet, absent[:1])
    few = kind in REPETITIVE
    many = few and n > 257                                  # (a piece of a repeat owns about n candidates: the long windows up to n = 257 only)
    out = [b""]
    for m in ((9, 33) if many else (9, 33, 64, 65, 130) if few else LENGTHS):
        m = min(m, n)
        a = int(rng.randint(0, n - m + 1))
        w = s[a:a + m]
        out.append(w)
        for c in sorted(set([1, e + 1] if many else [1, max(1, e), e + 1])):
            out.append(edited(w, c, rng, letters))
        if m in (9, 33):
            x = bytes(letters[:1])
            out += [w[1:], x + w, w[:-1], w + x]
    m = min(n, 12 if few else 40)
    out += [s[:m], s[n - m:], edited(s[:m], 1, rng, letters), edited(s[n - m:], 1, rng, letters)]
    out += [s, s + s[:1]]
    out += [s[:e], s[:min(n, e + 1)], b""]
    if absent.size:
        x = bytes([int(absent[0])])
        out += [x, s[:min(n, 5)] + x + s[:min(n, 5)]]
    if off is not None:
        o = [int(v) for v in off]
        k = len(o) // 2
        if 0 < k < len(o) - 1:
            m = min(9, o[k] - o[k - 1])
            out += [s[o[k] - m:o[k]], s[max(0, o[k] - 4):o[k] + 4], s[o[k] + min(e, 1):o[k] + 8]]
    return out


def patterns(c, e):
    """the patterns of a case of the catalogue (kmismatch_model.case), once"""
    k = (c.kind, c.n, c.off is not None, e)
    if k not in _pats:
        _pats[k] = patterns_of(c.kind, c.text, e, off=c.off)
    return _pats[k]


def results(c, e, pats=None, key=None, definition=False):
    """by_pieces of the case's own patterns (or of pats, memoised under key); definition: by_definition instead (hits only)"""
    k = (c.kind, c.n, c.off is not None, e, key, definition)
    if k not in _results:
        p = patterns(c, e) if pats is None else pats
        _results[k] = by_definition(c.text, c.off, p, e) if definition else by_pieces(c.text, c.off, c.SA, p, e)
    return _results[k]
