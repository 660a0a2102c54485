"""Host model of the maximal exact matches (psacx_mems_*; include/psacx.h: "maximal exact matches"), for
tests/test_mems_model_cpu.py and tests/test_gpu_mems*.py.

The result is stated twice:
  by_bytes(strings, pats, min_len, max_occ)       the byte definition over all (slot, text position): a match inside one pattern and
                                                  one string that can be extended neither to the right nor to the left, whose
                                                  pattern bytes occur at most max_occ times.  Small inputs.
  by_walk(SA, LCP, bwt, first, pats, stats, ...)  the shell walk of the header over SA / LCP, from the matching statistics
                                                  (len, lb, ub) of every slot, previous / next smaller value by a plain scan.  It
                                                  also counts the work: (shells, candidates).  by_walk_arrays: the same as arrays.
supermaximal() filters a MEM list by "contained in no other MEM's range of the same pattern"; by_walk(super=True) is the rule of
the header, whose work is (slots kept, ranks).  A result is a list of (slot, tpos, len) in the pinned order: ascending slot,
descending len, ascending rank.  Nothing here shares code with the library."""
import json
import os

import numpy as np

import match_model as M
import repeats_model as R

SUPER = 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mems_named.json")


def pattern_buffer(pats):
    """(pat as uint8, poff as uint64 with q + 1 entries)"""
    pats = [bytes(P) for P in pats]
    poff = np.zeros(len(pats) + 1, np.uint64)
    poff[1:] = np.cumsum([len(P) for P in pats])
    return np.frombuffer(b"".join(pats), np.uint8).copy(), poff


def slots_of(pats):
    """[(slot, first slot of its pattern, end of its pattern)] in buffer order"""
    out, at = [], 0
    for P in pats:
        out += [(at + i, at, at + len(P)) for i in range(len(P))]
        at += len(P)
    return out


# --------------------------------------------------------------------------------------------------------------- (a)
def by_bytes(strings, pats, min_len=1, max_occ=0):
    """set of (slot, tpos, len) from the definition"""
    strings = [bytes(s) for s in strings]
    buf = b"".join(bytes(P) for P in pats)
    min_len = max(min_len, 1)
    out = set()
    count = {}

    def occurrences(w):
        if w not in count:
            count[w] = sum(1 for s in strings for i in range(len(s) - len(w) + 1) if s[i:i + len(w)] == w)
        return count[w]
    for p, p0, p1 in slots_of(pats):
        base = 0
        for s in strings:
            for i in range(len(s)):
                d = 0
                while p + d < p1 and i + d < len(s) and buf[p + d] == s[i + d]:
                    d += 1
                if d < min_len:
                    continue
                if p > p0 and i > 0 and buf[p - 1] == s[i - 1]:
                    continue
                if max_occ and occurrences(buf[p:p + d]) > max_occ:
                    continue
                out.add((p, base + i, d))
            base += len(s)
    return out


def supermaximal(mems, pats):
    """the MEMs whose pattern range lies in no other MEM's range of the same pattern (a different range that contains it)"""
    ranges = {(p, p + l) for p, _, l in mems}
    owner = {}
    for p, p0, p1 in slots_of(pats):
        owner[p] = p0
    keep = set()
    for p, t, l in mems:
        a, b = p, p + l
        if not any((c, d) != (a, b) and c <= a and b <= d and owner[c] == owner[a] for c, d in ranges):
            keep.add((p, t, l))
    return keep


# --------------------------------------------------------------------------------------------------------------- (b)
def statistics(text, SA, pats, off=None):
    """(len, lb, ub) as int64 arrays, one entry per slot: the matching statistics by bisection over SA (match_model)"""
    qs = M.queries_of(pats, suffixes=True)
    s = np.asarray(text, np.uint8).tobytes()
    end = None if off is None else M.G.ends_of(off, len(s))
    seen, rows = {}, []
    for Q in qs:
        if Q not in seen:
            seen[Q] = M.by_bisection(s, SA, Q, off=off, end=end)
        rows.append(seen[Q])
    return tuple(np.array([r[i] for r in rows], np.int64) for i in range(3))


def _prev_below(L, x, v, limit):
    """the largest y <= x with L[y] < v (L[0] = 0 < v); with limit > 0 the search gives up below x - limit and says x - limit - 1"""
    w = 64
    while True:
        lo = max(0, x + 1 - w)
        hit = np.nonzero(L[lo:x + 1] < v)[0]
        if hit.size:
            return lo + int(hit[-1])
        if limit and w > limit:
            return max(0, x - limit - 1)
        w *= 4


def _next_below(L, x, v, limit):
    """the smallest y >= x with L[y] < v (L[n] = 0 < v); with limit > 0 the search gives up beyond x + limit and says x + limit + 1"""
    w = 64
    n = L.size - 1
    while True:
        hit = np.nonzero(L[x:x + w] < v)[0]
        if hit.size:
            return x + int(hit[0])
        if limit and w > limit:
            return min(n, x + limit + 1)
        w *= 4


def walk_chunks(SA, LCP, bwt, first, pats, stats, min_len=1, max_occ=0, super=False):
    """([(slot, kept ranks as an array in ascending order, len)] in the pinned order, (work0, work1)).  L[0] and L[n] are read as 0.
    The walk of a slot: shell 0 is [lb, ub) with l = len; the next shell has l' = max(L[lb], L[ub]), its interval reaches to the
    nearest values below l' on both sides, its ranks are what the interval gained.  A shell that fails min_len or max_occ ends the
    walk and is not counted.  A step that neither lowers l nor widens the interval ends it too."""
    n = int(np.asarray(SA).size)
    L = np.concatenate((np.asarray(LCP).astype(np.uint64), np.zeros(1, np.uint64)))
    if n:
        L[0] = 0
    b = np.asarray(bwt).astype(np.int64)
    f = np.asarray(first, bool)
    buf = b"".join(bytes(P) for P in pats)
    ln, slb, sub = (np.asarray(a).astype(np.uint64).tolist() for a in stats)
    min_len = max(min_len, 1)
    out, shells, cands = [], 0, 0
    prev_len = None
    for p, p0, p1 in slots_of(pats):
        l, lb, ub = min(ln[p], p1 - p), slb[p], sub[p]
        before, prev_len = (None if p == p0 else prev_len), l
        if not (lb < ub <= n) or l < min_len:
            continue
        if super:
            if before is not None and before > l:
                continue
            if max_occ and ub - lb > max_occ:
                continue
            shells += 1
            cands += ub - lb
            out.append((p, np.arange(lb, ub), l))
            continue
        ilb = iub = lb                                      # the interval so far (empty: shell 0 gains all of [lb, ub))
        nlb, nub, nl = lb, ub, l
        while True:
            if nl < min_len or (max_occ and nub - nlb > max_occ):
                break
            shells += 1
            cands += (ilb - nlb) + (nub - iub)
            r = np.concatenate((np.arange(nlb, ilb), np.arange(iub, nub)))
            if p != p0:
                r = r[f[r] | (b[r] != buf[p - 1])]
            if r.size:
                out.append((p, r, nl))
            ilb, iub, l = nlb, nub, nl
            nl = int(max(L[ilb], L[iub]))
            if nl >= l or nl < min_len:
                break
            nlb = _prev_below(L, ilb, nl, max_occ)
            nub = _next_below(L, iub, nl, max_occ)
            if nlb == ilb and nub == iub:
                break
    return out, (shells, cands)


def by_walk(SA, LCP, bwt, first, pats, stats, min_len=1, max_occ=0, super=False):
    """([(slot, tpos, len)] in the pinned order, (work0, work1)) of walk_chunks"""
    sa = np.asarray(SA).astype(np.int64)
    chunks, work = walk_chunks(SA, LCP, bwt, first, pats, stats, min_len, max_occ, super)
    return [(p, int(t), l) for p, r, l in chunks for t in sa[r]], work


def by_walk_arrays(SA, LCP, bwt, first, pats, stats, min_len=1, max_occ=0, super=False):
    """((qpos, tpos, len) as int64 arrays in the pinned order, (work0, work1)) of walk_chunks"""
    sa = np.asarray(SA).astype(np.int64)
    chunks, work = walk_chunks(SA, LCP, bwt, first, pats, stats, min_len, max_occ, super)
    if not chunks:
        z = np.zeros(0, np.int64)
        return (z, z, z), work
    sizes = np.array([r.size for _, r, _ in chunks], np.int64)
    qpos = np.repeat(np.array([p for p, _, _ in chunks], np.int64), sizes)
    ln = np.repeat(np.array([l for _, _, l in chunks], np.int64), sizes)
    return (qpos, sa[np.concatenate([r for _, r, _ in chunks])], ln), work


def in_order(result, SA):
    """is the list in the pinned order?  (ascending slot, descending len, ascending rank)"""
    isa = {int(t): r for r, t in enumerate(np.asarray(SA).tolist())}
    keys = [(p, -l, isa[t]) for p, t, l in result]
    return keys == sorted(keys) and len(set(keys)) == len(keys)


def arrays(result):
    """(qpos as uint64, tpos, len as int64)"""
    a = np.asarray(result, np.int64).reshape(-1, 3)
    return a[:, 0].astype(np.uint64), a[:, 1], a[:, 2]


def cli_text(result, pats, off=None):
    """what `mems --list` prints after the count: "pattern offset-in-pattern string position-in-string length" per MEM"""
    _, poff = pattern_buffer(pats)
    poff = poff.astype(np.int64)
    o = np.array([0], np.int64) if off is None else np.asarray(off).astype(np.int64)
    lines = []
    for p, t, l in result:
        j = int(np.searchsorted(poff, p, side="right")) - 1
        s = int(np.searchsorted(o, t, side="right")) - 1 if off is not None else 0
        lines.append("%d %d %d %d %d\n" % (j, p - int(poff[j]), s, t - int(o[s]), l))
    return "".join(lines)


# ---------------------------------------------------------------------------------------------------------------
NAMED = {
    "mississippi": ([b"mississippi"], [b"ississim", b"sip"]),
    "a20": ([b"a" * 20], [b"a" * 8]),
}


def named_arrays(name):
    strings, pats = NAMED[name]
    t, off, SA, LCP = R.arrays_by_definition(strings)
    bwt, first, _ = R.bwt_of(t, SA, off)
    return t, off, SA, LCP, bwt, first, pats


def named_results(name):
    t, off, SA, LCP, bwt, first, pats = named_arrays(name)
    stats = statistics(t, SA, pats, off if len(off) > 2 else None)
    out = {}
    for min_len in (1, 2, 3):
        for sup in (False, True):
            res, work = by_walk(SA, LCP, bwt, first, pats, stats, min_len, 0, sup)
            out["%s%d" % ("super" if sup else "mems", min_len)] = {"triples": [list(r) for r in res], "work": list(work)}
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":                             # writes tests/golden/mems_named.json from the model
    with open(GOLDEN, "w") as f:
        json.dump({name: named_results(name) for name in sorted(NAMED)}, f, separators=(",", ":"))
        f.write("\n")
