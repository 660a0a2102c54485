"""Host model of the suffix-tree node table and of its GPU checker (psacx_check_suffix_tree_dev_*), and a catalogue
of wrong tables and wrong inputs to hand the checker.

The table is stated here without ANSV, from the definition in include/psacx.h.  L = LCP with L[0] read as 0 whatever is
stored, row = sigma + 1, code() = alphabet code (1..sigma in byte order, 0 = past the end):

  head(x)     the smallest j <= x with L[j] == L[x] and min(L[j..x]) == L[x]
  cell(s, d)  code(text[s + d]) if s < n and d < n - s, else 0
  leaf i      x = i + 1 if i + 1 < n and L[i+1] > L[i], else i; id n + i in cell (head(x), cell(SA[i], L[x]))
  internal i  for i >= 1 with L[i] > 0 and head(i) == i: l / r the nearest j < i / j > i with L[j] < L[i] (r may not
              exist); (p, d) = (r, L[r]) if r exists and L[r] > L[l], else (head(l), L[l]); id i in cell (p, cell(SA[i], d))

records() finds head, l and r with one monotone stack (O(n)); expected_table() writes the records into an empty table;
expect() applies the counting rules: out[2] = records, out[3] = nonzero cells, a record is matched iff its cell holds its
id, out[0] = records not matched, out[1] = out[3] - matched.  top_down_table() states the same table a second way.
"""
import numpy as np


def codes_of(text):
    """(code[256], sigma): codes 1..sigma in byte order of the characters that occur."""
    used = np.zeros(256, bool)
    used[np.asarray(text, np.uint8)] = True
    code = np.zeros(256, np.int64)
    code[used] = np.arange(1, int(used.sum()) + 1)
    return code, int(used.sum())


def _cells(text, code, s, d):
    """cell(s, d) for arrays of uint64 s and d."""
    n = np.uint64(text.size)
    s = s.astype(np.uint64); d = d.astype(np.uint64)
    room = np.where(s < n, n - np.minimum(s, n), np.uint64(0))
    ok = d < room
    at = np.where(ok, s + np.where(ok, d, np.uint64(0)), np.uint64(0)).astype(np.int64)
    return np.where(ok, code[text[at]], 0).astype(np.int64)


def searches(LCP):
    """(L, head, left, right) of the definition: L as a uint64 array with L[0] = 0; left / right = -1 where there is none
    (right is only filled in for heads: no other index has an internal record)."""
    n = LCP.size
    L = [int(x) for x in LCP]
    L[0] = 0
    head, left, right = [0] * n, [-1] * n, [-1] * n
    stack = []                                               # heads only, their values strictly rising
    for x in range(n):
        v = L[x]
        while stack and L[stack[-1]] > v:
            right[stack.pop()] = x
        if stack and L[stack[-1]] == v:
            head[x] = stack[-1]
            left[x] = left[stack[-1]]
        else:
            head[x] = x
            left[x] = stack[-1] if stack else -1
            stack.append(x)
    Lu = np.array(L, dtype=np.uint64) if n else np.zeros(0, np.uint64)
    return Lu, np.array(head, np.int64), np.array(left, np.int64), np.array(right, np.int64)


def records(text, SA, LCP):
    """(rows, cols, ids) of every record, leaves first (record i is leaf i for i < n), as int64 / int64 / uint64 arrays."""
    text = np.asarray(text, np.uint8)
    n = text.size
    code, sigma = codes_of(text)
    L, head, left, right = searches(LCP)
    sa = SA.astype(np.uint64)
    i = np.arange(n, dtype=np.int64)
    nxt = np.minimum(i + 1, n - 1)
    x = np.where((i + 1 < n) & (L[nxt] > L), nxt, i)
    rows = [head[x]]
    cols = [_cells(text, code, sa, L[x])]
    ids = [(np.uint64(n) + i.astype(np.uint64))]
    k = i[(i >= 1) & (L > 0) & (head == i)]
    if k.size:
        l, r = left[k], right[k]
        assert np.all(l >= 0)
        use_r = (r >= 0) & (L[np.maximum(r, 0)] > L[l])
        rows.append(np.where(use_r, r, head[l]))
        cols.append(_cells(text, code, sa[k], np.where(use_r, L[np.maximum(r, 0)], L[l])))
        ids.append(k.astype(np.uint64))
    return np.concatenate(rows), np.concatenate(cols), np.concatenate(ids)


def farthest_parent(recs, n):
    """max |i - row| over all records, i the LCP index the record belongs to (leaf n + i or internal i) and row the node it hangs
    under: how far the farthest search of the text has to go."""
    rows, cols, ids = recs
    own = np.where(ids >= np.uint64(n), ids - np.uint64(n), ids).astype(np.int64)
    return int(np.abs(own - rows).max())


def expected_table(text, SA, LCP, recs=None):
    rows, cols, ids = recs if recs is not None else records(text, SA, LCP)
    nodes = np.zeros((np.asarray(text).size, codes_of(text)[1] + 1), np.uint64)
    nodes[rows, cols] = ids
    return nodes


def expect(text, SA, LCP, nodes, recs=None):
    """The four counters of psacx_check_suffix_tree_dev_* for this table over these arrays."""
    rows, cols, ids = recs if recs is not None else records(text, SA, LCP)
    assert nodes.shape == (np.asarray(text).size, codes_of(text)[1] + 1)
    matched = int((nodes[rows, cols] == ids).sum())
    nonzero = int(np.count_nonzero(nodes))
    return [int(ids.size) - matched, nonzero - matched, int(ids.size), nonzero]


def top_down_table(text, SA, LCP):
    """The same table from the top: a node is a range of LCP indices; the leftmost of its minima names it, all of its minima
    cut its suffixes into children, and a child of more than one suffix is a node again (no stack of smaller values, no head())."""
    text = np.asarray(text, np.uint8)
    n = text.size
    code, sigma = codes_of(text)
    L = LCP.astype(np.uint64).copy()
    L[0] = 0
    nodes = np.zeros((n, sigma + 1), np.uint64)

    def cell(s, d):
        return int(code[text[s + d]]) if s < n and d < n - s else 0

    todo = [(0, n - 1)]                                      # LCP indices lo..hi; the suffixes are SA[max(lo - 1, 0) .. hi]
    while todo:
        lo, hi = todo.pop()
        seg = L[lo:hi + 1]
        d = int(seg.min())
        cuts = lo + np.nonzero(seg == seg.min())[0]
        me = int(cuts[0])
        first = lo - 1 if lo > 0 else 0
        starts = ([first] if first < me else []) + [int(c) for c in cuts]
        ends = starts[1:] + [hi + 1]
        for s, e in zip(starts, ends):                       # suffixes s .. e - 1
            if e - s == 1:
                nodes[me, cell(int(SA[s]), d)] = n + s
            else:
                sub = L[s + 1:e]
                child = s + 1 + int(np.argmin(sub))
                nodes[me, cell(int(SA[child]), d)] = child
                todo.append((s + 1, e - 1))
    return nodes


# ---------------------------------------------------------------------------------------------------------------
# wrong tables: every function changes `nodes` in place near row `where` and says whether it could
# ---------------------------------------------------------------------------------------------------------------
def _nearest(rows, where):
    rows = np.asarray(rows)
    if rows.size == 0:
        return None
    return int(rows[np.argmin(np.abs(rows.astype(np.int64) - int(where)) * 2 + (rows > where))])


def _row_near(nodes, where, rowpred):
    """The row nearest to `where` at which rowpred (rows of the table -> one bool per row) holds: the rows around it first."""
    n = nodes.shape[0]
    for w in (64, n):
        lo, hi = max(0, where - w), min(n, where + w + 1)
        ok = np.nonzero(rowpred(nodes[lo:hi]))[0]
        if ok.size:
            return lo + _nearest(ok, where - lo)
    return None


def _pick(nodes, where, pred):
    """(row, col) of the cell nearest to row `where` among those where pred (cells -> bools) holds."""
    r = _row_near(nodes, where, lambda a: pred(a).any(axis=1))
    if r is None:
        return None
    return r, int(np.nonzero(pred(nodes[r:r + 1])[0])[0][0])


def _zero(leaf):
    def f(nodes, n, where, recs, head):
        at = _pick(nodes, where, (lambda a: a >= n) if leaf else (lambda a: (a > 0) & (a < n)))
        if at is None:
            return False
        nodes[at] = 0
        return True
    return f


def _move_in_row(nodes, n, where, recs, head):
    at = _pick(nodes, where, lambda a: (a != 0) & (a == 0).any(axis=1)[:, None])
    if at is None:
        return False
    r, c = at
    nodes[r, int(np.nonzero(nodes[r] == 0)[0][0])] = nodes[r, c]
    nodes[r, c] = 0
    return True


def _move_row(nodes, n, where, recs, head):
    at = _pick(nodes, where, lambda a: a != 0)
    if at is None or n < 2:
        return False
    r, c = at
    free = np.nonzero(nodes[:, c] == 0)[0]
    r2 = _nearest(free[free != r], r)
    if r2 is None:
        return False
    nodes[r2, c] = nodes[r, c]
    nodes[r, c] = 0
    return True


def _swap(nodes, n, where, recs, head):
    r = _row_near(nodes, where, lambda a: (a != 0).sum(axis=1) >= 2)
    if r is None:
        return False
    c = np.nonzero(nodes[r])[0]
    nodes[r, c[0]], nodes[r, c[-1]] = nodes[r, c[-1]], nodes[r, c[0]]
    return True


def _stray(what):
    def f(nodes, n, where, recs, head):
        at = _pick(nodes, where, lambda a: a == 0)
        if at is None:
            return False
        nodes[at] = {"valid": n + at[0], "2n": 2 * n + at[0], "ones": (1 << 64) - 1}[what]
        return True
    return f


def _non_head(nodes, n, where, recs, head):
    other = np.nonzero(head != np.arange(n))[0]              # indices that are no heads ...
    other = other[head[other] > 0]                           # ... of an interval that has a record
    j = _nearest(other, where)
    if j is None:
        return False
    k = nodes.shape[0] + int(np.searchsorted(recs[2][nodes.shape[0]:], np.uint64(head[j])))          # the record of that head (the ids ascend)
    if k >= recs[2].size or int(recs[2][k]) != int(head[j]) or int(nodes[recs[0][k], recs[1][k]]) != int(head[j]):
        return False
    nodes[recs[0][k], recs[1][k]] = j
    return True


def _leaf_off_by_one(nodes, n, where, recs, head):
    at = _pick(nodes, where, lambda a: a >= n)
    if at is None:
        return False
    v = int(nodes[at])
    nodes[at] = v + 1 if v + 1 < 2 * n else v - 1
    return True


TABLE_MUTANTS = {
    "zero_leaf": _zero(True), "zero_internal": _zero(False), "move_in_row": _move_in_row, "move_row": _move_row, "swap": _swap,
    "stray_valid": _stray("valid"), "stray_2n": _stray("2n"), "stray_ones": _stray("ones"), "non_head": _non_head,
    "leaf_off_by_one": _leaf_off_by_one,
}


def mutate_table(recipe, nodes, head, recs):
    """A copy of `nodes` after the mutants [(class, row), ...] one after the other, and the classes that could be applied.
    head: searches(LCP)[1] of the arrays the table belongs to (head_of(name) for a named text)."""
    out = nodes.copy()
    done = [cls for cls, where in recipe if TABLE_MUTANTS[cls](out, out.shape[0], int(where), recs, head)]
    return out, done


def table_positions(n, LCP, seed=1):
    """Rows 0, 1, n - 1, the group and level edges 63 / 64 / 65 and 4095 / 4096 / 4097, the deepest node, three random rows."""
    want = [0, 1, n - 1, 63, 64, 65, 4095, 4096, 4097, int(np.argmax(LCP[1:])) + 1 if n > 1 else 0]
    want += [int(x) for x in np.random.RandomState(seed).randint(0, n, 3)]
    return sorted({w for w in want if 0 <= w < n})


# ---------------------------------------------------------------------------------------------------------------
# wrong inputs: (text, SA, LCP) changed in place at index `where`; `bits` is the index type (all ones depends on it)
# ---------------------------------------------------------------------------------------------------------------
def _lcp_set(what):
    def f(t, s, l, where, bits):
        i = max(1, min(int(where), t.size - 1))
        if t.size < 2 or (what == "zero" and int(l[i]) == 0):
            return False
        l[i] = {"plus": int(l[i]) + 1, "zero": 0, "ones": (1 << bits) - 1}[what]
        return True
    return f


def _lcp0(t, s, l, where, bits):
    l[0] = 7
    return True


def _sa_set(what):
    def f(t, s, l, where, bits):
        i = min(int(where), t.size - 1)
        if what == "swap":
            if t.size < 2:
                return False
            i = min(i, t.size - 2)
            s[i], s[i + 1] = s[i + 1], s[i]
        else:
            s[i] = {"ones": (1 << bits) - 1, "n": t.size}[what]
        return True
    return f


def _text(t, s, l, where, bits):
    """Another character that still occurs, at a position whose own character occurs elsewhere too (sigma stays)."""
    cnt = np.bincount(t, minlength=256)
    ok = np.nonzero(cnt[t] >= 2)[0]
    if ok.size == 0 or (cnt > 0).sum() < 2:
        return False
    j = _nearest(ok, where)
    others = np.nonzero(cnt > 0)[0]
    t[j] = others[others != t[j]][0]
    return True


INPUT_MUTANTS = {
    "L+": _lcp_set("plus"), "L0": _lcp_set("zero"), "Lones": _lcp_set("ones"), "L0th": _lcp0,
    "Sones": _sa_set("ones"), "Sn": _sa_set("n"), "Sswap": _sa_set("swap"), "Text": _text,
}


def mutate_inputs(cls, where, text, SA, LCP, bits):
    """(text, SA, LCP) as 64-bit copies with one mutant applied, or None where the class does not apply."""
    arrs = (text.copy(), SA.astype(np.uint64), LCP.astype(np.uint64))
    return arrs if INPUT_MUTANTS[cls](*arrs, where=int(where), bits=bits) else None


# ---------------------------------------------------------------------------------------------------------------
# the texts of the test modules, with the oracle's arrays
# ---------------------------------------------------------------------------------------------------------------
EDGE_SIZES = [1, 2, 3, 63, 64, 65, 4095, 4096, 4097]
NAMED = ["mississippi", "dna", "unary", "tandem", "hub", "perm256"]
SMALL = ["edge%d" % n for n in EDGE_SIZES] + ["mississippi", "unary", "tandem", "perm256"]        # at most 37 000 characters
ALL = ["edge%d" % n for n in EDGE_SIZES] + NAMED
_texts, _arrays, _heads = {}, {}, {}


def text_of(name):
    if not _texts:
        import inputs
        two = np.frombuffer(b"AC", np.uint8)
        _texts.update({"edge%d" % n: two[(inputs.dna(n, 7) > 70).astype(np.int64)] for n in EDGE_SIZES})
        xy = np.arange(200)
        hub = np.zeros((200, 200, 3), np.uint8)
        hub[:, :, 1] = 1 + xy[:, None]
        hub[:, :, 2] = 1 + xy[None, :]
        _texts.update({
            "mississippi": np.frombuffer(b"mississippi", np.uint8),
            "dna": inputs.dna(300000, 4),                                       # more than 64^3 entries: three pyramid levels
            "unary": np.full(5000, 97, np.uint8),                               # L[i] = i: every index a node, no smaller value to the right
            "tandem": inputs.tandem(37000, 37, inputs.dna(37, 5)),              # period 37 x 1000 (the unit starts with two different characters: LCP + 1 shows)
            "hub": hub.reshape(-1),                                             # 0, 1 + x, 1 + y for x, y < 200: plateaus of equal LCP
            "perm256": np.random.RandomState(6).permutation(256).astype(np.uint8),      # row of 257 cells, LCP all zero
        })
    return _texts[name]


def arrays(name):
    """(text, SA, LCP, records, table) of a named text: the arrays from the oracle (64-bit), the table from the model."""
    if name not in _arrays:
        import oracle_lib as O
        text = text_of(name)
        ref = O.construct(text, bits=64)
        recs = records(text, ref["SA"], ref["LCP"])
        _arrays[name] = (text, ref["SA"], ref["LCP"], recs, expected_table(text, ref["SA"], ref["LCP"], recs))
    return _arrays[name]


def head_of(name):
    if name not in _heads:
        _heads[name] = searches(arrays(name)[2])[1]
    return _heads[name]
