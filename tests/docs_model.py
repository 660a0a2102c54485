"""Host model of the document counts and document lists (include/psacx.h: "document counts and document lists"), for
tests/test_docs_model_cpu.py and tests/test_gpu_docs*.py.

The results are stated twice:
  by bytes      docs_by_bytes(strings, w): the strings that hold the word w, read from the strings themselves; docs_of_ranks /
                list_of_ranks: the strings of the suffixes SA[lb .. ub), and the first rank of each, by a plain walk.
  by the index  doc_of -> prev_of -> h_of (first minima of L[p + 1 .. r]) -> dup_of, then count_by_dup (the formula of the header with its
                clamps) and list_by_prev.
All arrays are int64 here; "all ones" is -1."""
import json
import os

import numpy as np

import repeats_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "docs_named.json")
NONE = -1


# ------------------------------------------------------------------------------------------------------------- by bytes
def docs_by_bytes(strings, w):
    """the strings that hold w, ascending"""
    w = bytes(w)
    return [s for s, x in enumerate(strings) if w in bytes(x)]


def docs_of_ranks(SA, off, lb, ub):
    """the distinct strings of the suffixes SA[lb .. ub), by a walk over the positions"""
    off = [int(x) for x in off]
    seen = set()
    for r in range(lb, ub):
        p = int(SA[r])
        seen.add(max(s for s in range(len(off) - 1) if off[s] <= p))
    return sorted(seen)


def list_of_ranks(SA, off, lb, ub):
    """[(rank, string, position)] of the first rank of each string in [lb, ub), ascending rank"""
    off = [int(x) for x in off]
    seen, out = set(), []
    for r in range(lb, ub):
        p = int(SA[r])
        s = max(s for s in range(len(off) - 1) if off[s] <= p)
        if s not in seen:
            seen.add(s)
            out.append((r, s, p))
    return out


# ------------------------------------------------------------------------------------------------------------- by the index
def doc_of(SA, off):
    """doc(r): the largest s < m with off[s] <= SA[r] (0 if there is none)"""
    off = np.asarray(off).astype(np.int64)
    m = off.size - 1
    return np.maximum(np.searchsorted(off[:m], np.asarray(SA).astype(np.int64), side="right") - 1, 0)


def prev_of(doc):
    """prev[r] = the largest p < r with doc[p] == doc[r], or -1"""
    doc = np.asarray(doc, np.int64)
    order = np.argsort(doc, kind="stable")
    prev = np.full(doc.size, NONE, np.int64)
    same = doc[order[1:]] == doc[order[:-1]]
    prev[order[1:][same]] = order[:-1][same]
    return prev


def first_min_at(L, lo, hi):
    """the position of the FIRST minimum of L[lo[k] .. hi[k]), lo < hi"""
    L = np.asarray(L).astype(np.int64)
    n = L.size
    assert n == 0 or int(L.max()) < (1 << 40) and n < (1 << 22)
    keys = L * (1 << 22) + np.arange(n)                # the smaller value, then the smaller position
    return M._range_reduce(keys, np.asarray(lo, np.int64), np.asarray(hi, np.int64), np.minimum) & ((1 << 22) - 1)


def h_of(prev, LCP):
    """h[x], n entries: the pairs (prev[r], r) whose first minimum of L[prev[r] + 1 .. r] lies at x"""
    prev = np.asarray(prev, np.int64)
    n = prev.size
    r = np.nonzero(prev != NONE)[0]
    h = np.zeros(n, np.int64)
    if r.size:
        np.add.at(h, first_min_at(LCP, prev[r] + 1, r + 1), 1)
    return h


def dup_of(h):
    """dup[i] = sum of h[x] over x < i, n + 1 entries"""
    return np.concatenate(([0], np.cumsum(np.asarray(h, np.int64))))


def index_of(SA, LCP, off):
    """(prev, dup) of a set"""
    prev = prev_of(doc_of(SA, off))
    return prev, dup_of(h_of(prev, LCP))


def count_by_dup(dup, lb, ub, n):
    """docs_j of psacx_doc_count_dev_*, clamps included"""
    dup = np.asarray(dup).astype(np.int64)
    lb, ub = np.asarray(lb).astype(np.int64), np.asarray(ub).astype(np.int64)
    ok = (lb < ub) & (ub <= n)
    a, b = np.where(ok, lb, 0), np.where(ok, ub, 1)
    dd = np.minimum(np.maximum(dup[b] - dup[np.minimum(a + 1, n)], 0), b - a - 1)
    return np.where(ok, (b - a) - dd, 0)


def list_by_prev(prev, SA, off, lb, ub, n):
    """(start with q + 1 entries, ranks, sid, pos) of psacx_doc_list_dev_*: intervals that are not lb <= ub <= n count 0; an SA entry >= n
    gives sid = m"""
    prev, SA = np.asarray(prev).astype(np.int64), np.asarray(SA).astype(np.int64)
    off = np.asarray(off).astype(np.int64)
    m = off.size - 1
    ranks = []
    start = [0]
    for a, b in zip(np.asarray(lb).astype(np.int64).tolist(), np.asarray(ub).astype(np.int64).tolist()):
        if 0 <= a <= b <= n:
            p = prev[a:b]
            ranks.append(a + np.nonzero((p == NONE) | ((p >= 0) & (p < a)))[0])
        start.append(start[-1] + (ranks[-1].size if 0 <= a <= b <= n else 0))
    ranks = np.concatenate(ranks) if ranks else np.zeros(0, np.int64)
    pos = SA[ranks]
    sid = np.where((pos >= n) | (pos < 0), m, doc_of(pos, off))
    return np.asarray(start, np.int64), ranks, sid, pos


# ------------------------------------------------------------------------------------------------------------- intervals
def is_lcp_interval(LCP, lb, ub):
    L = np.asarray(LCP).astype(np.int64).copy()
    n = L.size
    if not (0 <= lb < ub <= n):
        return False
    L[0] = 0
    inner = int(L[lb + 1:ub].min()) if ub > lb + 1 else (1 << 62)
    return (lb == 0 or int(L[lb]) < inner) and (ub == n or int(L[ub]) < inner)


def lcp_intervals(LCP):
    """(lb, ub, len) of every LCP-interval: the inner nodes, all singletons (len -1: the whole suffix) and [0, n) (len 0)"""
    n = len(LCP)
    out = [(lb, ub, ln) for _, lb, ub, ln in M.intervals(LCP)]
    out += [(r, r + 1, -1) for r in range(n)]
    if n:
        out.append((0, n, 0))
    return sorted(set(out))


def random_intervals(n, q, seed):
    rng = np.random.RandomState(seed)
    a, b = rng.randint(0, n + 1, q), rng.randint(0, n + 1, q)
    return np.minimum(a, b), np.maximum(a, b)


# ------------------------------------------------------------------------------------------------------------- named sets
W257 = [bytes([x]) + b"GATTACA" for x in range(256)] + [b"GATTACA"]
NAMED = {"miss": [b"mississippi", b"missouri", b"miss"], "acgt3": [b"acgt"] * 3, "w257": W257}
PATTERNS = {"miss": [b"miss", b"ss", b"i", b"ssi", b"ouri", b"s", b"m", b"x"], "acgt3": [b"acgt", b"cg", b"t", b"ca"],
            "w257": [b"GATTACA", b"A", b"TT", b"\x07G", b"\x07", b"ATTACAG"]}


def locate(strings, SA, pattern):
    """[lb, ub) of the suffixes that start with the pattern, from the bytes"""
    t, off = M.flatten(strings)
    end = np.zeros(t.size, np.int64)
    for s in range(off.size - 1):
        end[off[s]:off[s + 1]] = off[s + 1]
    hits = [r for r, p in enumerate(np.asarray(SA).tolist()) if t[p:min(end[p], p + len(pattern))].tobytes() == bytes(pattern)]
    if not hits:
        return 0, 0
    assert hits == list(range(hits[0], hits[-1] + 1))
    return hits[0], hits[-1] + 1


def named_results(name):
    """{"patterns": [{"pattern", "lb", "ub", "docs", "sid", "pos"}]} from the bytes"""
    strings = NAMED[name]
    t, off, SA, LCP = M.arrays_by_definition(strings)
    rows = []
    for p in PATTERNS[name]:
        lb, ub = locate(strings, SA, p)
        lst = list_of_ranks(SA, off, lb, ub)
        rows.append({"pattern": list(p), "lb": lb, "ub": ub, "docs": len(docs_by_bytes(strings, p)), "sid": [s for _, s, _ in lst],
                     "pos": [q for _, _, q in lst]})
    return {"patterns": rows}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":                             # writes tests/golden/docs_named.json from the model
    with open(GOLDEN, "w") as f:
        json.dump({name: named_results(name) for name in sorted(NAMED)}, f, separators=(",", ":"))
        f.write("\n")
