"""Host model of the generalized suffix tree's node table (psacx_suffix_tree_gsa_dev_*), of its GPU checker
(psacx_check_suffix_tree_gsa_dev_*), and a catalogue of wrong tables and wrong inputs to hand the checker.

The table is the one include/psacx.h defines.  text[0..n) holds the m strings back to back, off their m + 1 offsets;
L = LCP with L[0] read as 0 whatever is stored; start[p] = "a string starts at p, or p == n"; code() = alphabet code
(1..sigma in byte order); row = sigma + 2; head(x), l and r are those of the one-string table (st_checker_model.searches):

  gcell(s, d)  0 (the $) if s >= n, or d >= n - s, or (d > 0 and start[s + d]); else code(text[s + d])
  leaf i       x = i + 1 if i + 1 < n and L[i+1] > L[i], else i; id n + i, row head(x), c = gcell(SA[i], L[x])
  internal i   for i >= 1 with L[i] > 0 and head(i) == i: (p, d) = (r, L[r]) if r exists and L[r] > L[l], else
               (head(l), L[l]); id i, row p, c = gcell(SA[i], d)
  cells        a record with c >= 1 puts its id in cell (row, 1 + c); the records of a row with c == 0 put their smallest id
               in cell (row, 0) and their largest in cell (row, 1); every other cell is 0

records() states the records, expected_table() writes them, expect() applies the checker's counting rules, and
top_down_table() states the same table a second way, from the bytes of the suffixes alone.
"""
import numpy as np

import gsa_checker_model as G
import st_checker_model as S
from st_checker_model import codes_of, table_positions, INPUT_MUTANTS  # noqa: F401  (for the tests)


def gcells(text, code, flag, s, d):
    """gcell(s, d) for arrays of uint64 s and d; flag = gsa_checker_model.end_flags(off, n)."""
    n = np.uint64(text.size)
    s = s.astype(np.uint64); d = d.astype(np.uint64)
    room = np.where(s < n, n - np.minimum(s, n), np.uint64(0))
    ok = d < room
    at = np.where(ok, s + np.where(ok, d, np.uint64(0)), np.uint64(0)).astype(np.int64)
    ok &= ~((d > 0) & flag[at])
    return np.where(ok, code[text[at]], 0).astype(np.int64)


def records(text, off, SA, LCP):
    """(rows, c, ids) of every record, leaves first (record i is leaf i for i < n), as int64 / int64 / uint64 arrays."""
    text = np.asarray(text, np.uint8)
    n = text.size
    code, sigma = codes_of(text)
    flag = G.end_flags(off, n)
    L, head, left, right = S.searches(LCP)
    sa = SA.astype(np.uint64)
    i = np.arange(n, dtype=np.int64)
    nxt = np.minimum(i + 1, n - 1)
    x = np.where((i + 1 < n) & (L[nxt] > L), nxt, i)
    rows = [head[x]]
    cs = [gcells(text, code, flag, sa, L[x])]
    ids = [(np.uint64(n) + i.astype(np.uint64))]
    k = i[(i >= 1) & (L > 0) & (head == i)]
    if k.size:
        l, r = left[k], right[k]
        assert np.all(l >= 0)
        use_r = (r >= 0) & (L[np.maximum(r, 0)] > L[l])
        rows.append(np.where(use_r, r, head[l]))
        cs.append(gcells(text, code, flag, sa[k], np.where(use_r, L[np.maximum(r, 0)], L[l])))
        ids.append(k.astype(np.uint64))
    return np.concatenate(rows), np.concatenate(cs), np.concatenate(ids)


def as_cells(recs):
    """The records with the column of their cell in place of c (column 0 for c == 0): what the table mutants of
    st_checker_model expect."""
    rows, c, ids = recs
    return rows, np.where(c > 0, c + 1, 0), ids


def expected_table(text, off, SA, LCP, recs=None):
    rows, c, ids = recs if recs is not None else records(text, off, SA, LCP)
    n = np.asarray(text).size
    nodes = np.zeros((n, codes_of(text)[1] + 2), np.uint64)
    ch = c > 0
    nodes[rows[ch], c[ch] + 1] = ids[ch]
    if (~ch).any():
        lo = np.full(n, np.iinfo(np.uint64).max, np.uint64)
        hi = np.zeros(n, np.uint64)
        np.minimum.at(lo, rows[~ch], ids[~ch])
        np.maximum.at(hi, rows[~ch], ids[~ch])
        has = hi > 0                                         # (ids are nonzero)
        nodes[has, 0] = lo[has]
        nodes[has, 1] = hi[has]
    return nodes


def expect(text, off, SA, LCP, nodes, recs=None):
    """The four counters of psacx_check_suffix_tree_gsa_dev_* for this table over these arrays."""
    rows, c, ids = recs if recs is not None else records(text, off, SA, LCP)
    assert nodes.shape == (np.asarray(text).size, codes_of(text)[1] + 2)
    ch = c > 0
    by_char = int((nodes[rows[ch], c[ch] + 1] == ids[ch]).sum())
    lo, hi, v = nodes[rows[~ch], 0], nodes[rows[~ch], 1], ids[~ch]
    by_range = int(((lo != 0) & (lo <= v) & (v <= hi)).sum())
    witnesses = int(((lo != 0) & (lo <= hi) & (v == lo)).sum()) + int(((lo != 0) & (lo <= hi) & (v == hi)).sum())
    nonzero = int(np.count_nonzero(nodes))
    return [int(ids.size) - by_char - by_range, nonzero - by_char - witnesses, int(ids.size), nonzero]


def top_down_table(text, off, SA):
    """The same table from the top and from the bytes alone: a node is a run of neighbouring suffixes and the characters d they all
    share; the cell of each at depth d ($ where its string has ended) cuts the run into children: the $ suffixes are leaves whose
    first and last go to cells 0 and 1, a single suffix is a leaf, a longer run a node again.  A node is named by the first
    position at which two neighbours of its run share no more than all of them do.  Neither LCP, head() nor a stack."""
    text = np.asarray(text, np.uint8)
    n = text.size
    code, sigma = codes_of(text)
    flag = G.end_flags(off, n)
    sa = SA.astype(np.int64)
    shared = np.zeros(n, np.int64)                           # shared[j]: characters the suffixes j - 1 and j have in common
    if n > 1:
        shared[1:] = G.shared_by_characters(text, np.asarray(off, np.int64), sa[:-1], sa[1:])
    nodes = np.zeros((n, sigma + 2), np.uint64)
    todo = [(0, n, 0, 0)]                                    # suffixes a .. b - 1, depth, name
    while todo:
        a, b, d, me = todo.pop()
        c = gcells(text, code, flag, sa[a:b].astype(np.uint64), np.full(b - a, d, np.uint64))
        cut = np.concatenate(([0], np.nonzero(c[1:] != c[:-1])[0] + 1, [b - a]))
        for s, e in zip(cut[:-1] + a, cut[1:] + a):
            k = int(c[s - a])
            if k == 0:
                nodes[me, 0], nodes[me, 1] = n + s, n + e - 1
            elif e - s == 1:
                nodes[me, 1 + k] = n + s
            else:
                depth = int(shared[s + 1:e].min())
                child = int(s) + 1 + int(np.argmin(shared[s + 1:e]))
                nodes[me, 1 + k] = child
                todo.append((int(s), int(e), depth, child))
    return nodes


def single_string_relation(gst, st):
    """With one string: columns 2.. of the set's table are columns 1.. of the one-string table, columns 0 and 1 both its column 0."""
    return np.array_equal(gst[:, 2:], st[:, 1:]) and np.array_equal(gst[:, 0], st[:, 0]) and np.array_equal(gst[:, 1], st[:, 0])


# ---------------------------------------------------------------------------------------------------------------
# wrong tables: the classes of st_checker_model plus what only the two $ cells can be; f(nodes, n, where, recs, head)
# changes `nodes` in place near row `where` and says whether it could (recs as as_cells() gives them)
# ---------------------------------------------------------------------------------------------------------------
def _dollar_row(nodes, where, differ=False):
    return S._row_near(nodes, where, lambda a: (a[:, 0] != 0) & ((a[:, 0] != a[:, 1]) | (not differ)))


def _dollar(col, step):
    def f(nodes, n, where, recs, head):
        r = _dollar_row(nodes, where)
        if r is None:
            return False
        nodes[r, col] = int(nodes[r, col]) + step if step else 0
        return True
    return f


def _dollar_swap(nodes, n, where, recs, head):
    r = _dollar_row(nodes, where, differ=True)
    if r is None:
        return False
    nodes[r, 0], nodes[r, 1] = nodes[r, 1], nodes[r, 0]
    return True


def _dollar_stray(nodes, n, where, recs, head):
    r = S._row_near(nodes, where, lambda a: (a[:, 0] == 0) & (a[:, 1] == 0))
    if r is None:
        return False
    nodes[r, 0], nodes[r, 1] = n + r, min(n + r + 1, 2 * n - 1)
    return True


def _dollar_as_char(nodes, n, where, recs, head):
    r = _dollar_row(nodes, where)
    if r is None or nodes.shape[1] < 3:
        return False
    free = np.nonzero(nodes[r, 2:] == 0)[0]
    nodes[r, 2 + (int(free[0]) if free.size else 0)] = nodes[r, 0]
    return True


DOLLAR_MUTANTS = {
    "lo+1": _dollar(0, 1), "hi-1": _dollar(1, -1), "lo_zero": _dollar(0, 0), "hi_zero": _dollar(1, 0), "lo_hi_swap": _dollar_swap,
    "widen_lo": _dollar(0, -1), "widen_hi": _dollar(1, 1), "stray_pair": _dollar_stray, "dollar_as_char": _dollar_as_char,
}
TABLE_MUTANTS = dict(S.TABLE_MUTANTS)
TABLE_MUTANTS.update(DOLLAR_MUTANTS)


def mutate_table(recipe, nodes, head, recs):
    """A copy of `nodes` after the mutants [(class, row), ...] one after the other, and the classes that could be applied.
    head: searches(LCP)[1] of the arrays the table belongs to; recs: their records()."""
    out = nodes.copy()
    cells = as_cells(recs)
    done = [cls for cls, where in recipe if TABLE_MUTANTS[cls](out, out.shape[0], int(where), cells, head)]
    return out, done


# ---------------------------------------------------------------------------------------------------------------
# wrong inputs: the classes of st_checker_model on (text, SA, LCP), and an offset moved by one
# ---------------------------------------------------------------------------------------------------------------
OFFSET_MUTANTS = ("Goff+1", "Goff-1")
ALL_INPUT_MUTANTS = list(INPUT_MUTANTS) + list(OFFSET_MUTANTS)


def mutate_inputs(cls, where, text, off, SA, LCP, bits):
    """(text, off, SA, LCP) as copies (the arrays 64-bit) with one mutant applied, or None where the class does not apply."""
    t, o, s, l = text.copy(), np.asarray(off, np.uint64).copy(), SA.astype(np.uint64), LCP.astype(np.uint64)
    if cls in OFFSET_MUTANTS:
        could = G.GSA_MUTANTS[cls][0](t, o, s, None, l, int(where))
    else:
        could = INPUT_MUTANTS[cls](t, s, l, where=int(where), bits=bits)
    return (t, o, s, l) if could else None


# ---------------------------------------------------------------------------------------------------------------
# the string sets of the test modules, with the oracle's arrays
# ---------------------------------------------------------------------------------------------------------------
EDGES = ["edge%d" % n for n in (63, 64, 65, 4095, 4096, 4097)]
TINY = ["tiny%d" % n for n in G.TINY]
NAMED = ["copies", "prefixes", "unary", "tandem_pieces", "single"]
ALL = TINY + EDGES + ["word_edges"] + NAMED + ["bytes256"]
_sets, _arrays, _heads = {}, {}, {}


def strings_of(name):
    if name in TINY or name in NAMED:
        return G.strings_of(name)
    if name not in _sets:
        import inputs
        if name in EDGES:                                    # the two-letter texts of st_checker_model, cut unevenly
            t = S.text_of(name)
            _sets[name] = G._cut(t, np.random.RandomState(13).choice([1, 2, 3, 7, 33, 64, 150], t.size))
        elif name == "word_edges":                           # offsets 31, 32, 33, 63, 64, 65: the ends of the bitmap's words
            two = np.frombuffer(b"AC", np.uint8)
            _sets[name] = G._cut(two[(inputs.dna(90, 9) > 70).astype(np.int64)], [31, 1, 1, 30, 1, 1])
        else:                                                # all 256 bytes, some of them again: a row of 258 cells
            p = np.random.RandomState(6).permutation(256).astype(np.uint8)
            _sets[name] = G._cut(np.concatenate([p, p[40:100], p[120:156], p[:30]]), [100, 56, 100, 60, 36, 30])
    return _sets[name]


def arrays(name):
    """(text, off, SA, LCP, records, table) of a named set: the arrays from the oracle (64-bit), the table from the model."""
    if name not in _arrays:
        import oracle_lib as O
        ref = O.construct_ss(strings_of(name), bits=64)
        text, off = ref["text"], np.asarray(ref["off"], np.uint64)
        recs = records(text, off, ref["SA"], ref["LCP"])
        _arrays[name] = (text, off, ref["SA"], ref["LCP"], recs, expected_table(text, off, ref["SA"], ref["LCP"], recs))
    return _arrays[name]


def head_of(name):
    if name not in _heads:
        _heads[name] = S.searches(arrays(name)[3])[1]
    return _heads[name]
