"""Host model of the two GPU checkers for generalized suffix arrays, and the wrong arrays only a string set can have.

psacx_check_gsa_dev_* (one GPU) and psacx_multi_check_gsa_dev_* (block-distributed) return four counters.  The functions
here compute the same four numbers from the definitions in include/psacx.h, in plain numpy and 64-bit integers.  They are
the rules of checker_model.py with "end of text" replaced by "end of the suffix's string"; end(p) is the offset at which
the string holding position p ends:

  common        e0 = #{i : SA[i] >= n or ISA[SA[i]] != i}.  Every other test runs at entries i that passed this one
                and, for i > 0, only if SA[i-1] < n.  e3 = [LCP given, entry 0 passed, LCP[0] != 0].
                Order at i > 0 with a = SA[i-1], b = SA[i]: fine iff t[a] < t[b], or t[a] == t[b] and one of
                  a + 1 == end(a) and b + 1 == end(b) and a < b          (equal suffixes: text order)
                  a + 1 == end(a) and b + 1 <  end(b)
                  neither suffix ends after one character and ISA[a+1] < ISA[b+1];
                e1 counts the entries that are not.
  one GPU       e2 = #{i > 0 examined : LCP[i] != number of characters a and b share before either string ends},
                whether or not the order test passed.
  distributed   LCP is examined only where the order test passed: want = 0 if t[a] != t[b], 1 if a + 1 == end(a) or
                b + 1 == end(b), else 1 + min(LCP[ISA[a+1] + 1 .. ISA[b+1]]) over the arrays as given; an entry whose order
                test passed with ISA[b+1] >= n is counted and no minimum is looked up.

The catalogue is checker_model.MUTANTS (every way SA / ISA / LCP / the text can be wrong; a mutant there is a function of
(text, SA, ISA, LCP, where)) plus GSA_MUTANTS, whose functions also see -- and may move -- the string offsets.
"""
import numpy as np

import checker_model as M
from checker_model import RangeMin, MUTANTS, mutate_many, blocks, positions  # noqa: F401  (positions, blocks: for the tests)


def end_flags(off, n):
    """flag[p] for p in 0 .. n: a string starts at p, or p == n."""
    f = np.zeros(n + 1, bool)
    f[np.asarray(off, np.int64)] = True
    return f


def ends_of(off, p):
    """end(p) for an array of positions."""
    off = np.asarray(off, np.int64)
    return off[np.searchsorted(off, p, side="right")]


class GsaTruth(object):
    """The correct ISA and LCP of a string set (from the oracle): the characters two suffixes share before either string
    ends are a range minimum of the true LCP array between their ranks."""

    def __init__(self, text, off, SA, ISA, LCP):
        self.n = text.size
        self.off = np.asarray(off, np.int64)
        self.SA = SA.astype(np.int64); self.ISA = ISA.astype(np.int64); self.LCP = LCP.astype(np.int64)
        self._rmq = None

    def shared(self, a, b, at=None):
        out = np.empty(a.size, np.int64)
        todo = np.ones(a.size, bool)
        if at is not None and self.n > 1:
            i = np.clip(at, 1, self.n - 1)
            same = (self.SA[i - 1] == a) & (self.SA[i] == b)
            out[same] = self.LCP[i[same]]
            todo &= ~same
        eq = todo & (a == b)
        out[eq] = ends_of(self.off, a[eq]) - a[eq]
        todo &= ~eq
        if todo.any():
            if self._rmq is None:
                self._rmq = RangeMin(self.LCP)
            ra, rb = self.ISA[a[todo]], self.ISA[b[todo]]
            out[todo] = self._rmq.query(np.minimum(ra, rb) + 1, np.maximum(ra, rb) + 1)
        return out


def shared_by_characters(text, off, a, b):
    """The same by direct comparison, one character of every pair still equal per step."""
    room = np.minimum(ends_of(off, a) - a, ends_of(off, b) - b)
    h = np.zeros(a.size, np.int64)
    act = np.arange(a.size)
    while act.size:
        good = h[act] < room[act]
        good[good] = text[a[act[good]] + h[act[good]]] == text[b[act[good]] + h[act[good]]]
        act = act[good]
        h[act] += 1
    return h


def _common(text, off, SA, ISA, LCP):
    n = int(text.size)
    assert n > 0 and SA.size == n and ISA.size == n and (LCP is None or LCP.size == n)
    flag = end_flags(off, n)
    SAu, ISAu = SA.astype(np.uint64), ISA.astype(np.uint64)
    in_range = SAu < np.uint64(n)
    sa = np.where(in_range, SAu, 0).astype(np.int64)
    passed = in_range & (ISAu[sa] == np.arange(n, dtype=np.uint64))
    e0 = n - int(passed.sum())
    e3 = int(LCP is not None and bool(passed[0]) and int(LCP[0]) != 0)
    ex = np.zeros(n, bool)
    ex[1:] = passed[1:] & in_range[:-1]
    i = np.nonzero(ex)[0]
    a, b = sa[i - 1], sa[i]
    ta, tb = text[a], text[b]
    ea, eb = flag[a + 1], flag[b + 1]
    na, nb = ISAu[np.minimum(a + 1, n - 1)], ISAu[np.minimum(b + 1, n - 1)]          # compared only where neither suffix ends
    ok = (ta < tb) | ((ta == tb) & ((ea & eb & (a < b)) | (ea & ~eb) | (~ea & ~eb & (na < nb))))
    return n, e0, e3, i, a, b, ta, tb, na, nb, ea, eb, ok


def _device(text, off, LCP, cm, truth):
    n, e0, e3, i, a, b, ta, tb, na, nb, ea, eb, ok = cm
    e2 = 0
    if LCP is not None and i.size:
        h = truth.shared(a, b, i) if truth is not None else shared_by_characters(text, np.asarray(off, np.int64), a, b)
        e2 = int((LCP[i].astype(np.uint64) != h.astype(np.uint64)).sum())
    return [e0, int((~ok).sum()), e2, e3]


def _multi(text, LCP, cm, rmq):
    n, e0, e3, i, a, b, ta, tb, na, nb, ea, eb, ok = cm
    e2 = 0
    if LCP is not None and i.size:
        L = LCP.astype(np.uint64)
        want = np.zeros(i.size, np.uint64)
        want[(ta == tb) & (ea | eb)] = 1
        rec = ok & (ta == tb) & ~ea & ~eb                   # the recurrence proper: na < nb holds here
        none = rec & (nb >= np.uint64(n))                   # a rank that is none: counted, nothing looked up
        ask = rec & ~none
        if ask.any():
            if rmq is None:
                rmq = RangeMin(LCP)
            want[ask] = rmq.query(na[ask].astype(np.int64) + 1, nb[ask].astype(np.int64) + 1).astype(np.uint64) + np.uint64(1)
        e2 = int(none.sum()) + int((ok & ~none & (L[i] != want)).sum())
    return [e0, int((~ok).sum()), e2, e3]


def expect_gsa_device(text, off, SA, ISA, LCP, truth=None):
    """[e0, e1, e2, e3] of psacx_check_gsa_dev_*.  truth: a GsaTruth of this very text and these very offsets (else characters
    are compared)."""
    return _device(text, off, LCP, _common(text, off, SA, ISA, LCP), truth)


def expect_gsa_multi(text, off, SA, ISA, LCP, rmq=None):
    """[e0, e1, e2, e3] of psacx_multi_check_gsa_dev_*, for any number of ranks and pieces.  rmq: a RangeMin of this very LCP."""
    return _multi(text, LCP, _common(text, off, SA, ISA, LCP), rmq)


def expect_gsa_both(text, off, SA, ISA, LCP, truth=None, rmq=None):
    cm = _common(text, off, SA, ISA, LCP)
    return _device(text, off, LCP, cm, truth), _multi(text, LCP, cm, rmq)


# ---------------------------------------------------------------------------------------------------------------
# the wrong arrays only a string set can have.  f(text, off, SA, ISA, LCP, where) changes its arguments in place and says
# whether it could; every class looks for the entry nearest to `where` at which it applies (the clean arrays are expected).
# ---------------------------------------------------------------------------------------------------------------
def _pairs(t, off, s, l):
    """(both in range, a, b, end(a), end(b)) of the entries 1 .. n - 1 (entry j is index j - 1)."""
    n = t.size
    ok = M._valid_sa(s)
    sa = np.where(ok, s, 0).astype(np.int64)
    a, b = sa[:-1], sa[1:]
    o = np.asarray(off, np.int64)
    return ok[:-1] & ok[1:], a, b, ends_of(o, a), ends_of(o, b)


def _swap(s, i, j):
    s[j - 1], s[j] = s[j], s[j - 1]
    i[int(s[j - 1])], i[int(s[j])] = j - 1, j


def _geq_swap(t, off, s, i, l, where):
    # two equal suffixes of different strings, which must stand in text order, exchanged in SA and ISA
    if t.size < 2:
        return False
    v, a, b, enda, endb = _pairs(t, off, s, l)
    L = l[1:].astype(np.int64)
    j = M._nearest(v & (L == enda - a) & (L == endb - b), max(int(where) - 1, 0))
    if j is None:
        return False
    _swap(s, i, j + 1)
    return True


def _concat_more(t, a, b, L, n):
    """where the suffixes a + L and b + L of the concatenated text both exist and start with the same character"""
    pa, pb = a + L, b + L
    both = (pa < n) & (pb < n)
    both[both] = t[pa[both]] == t[pb[both]]
    return both


def _gl_past_end(t, off, s, i, l, where):
    # an LCP entry that runs past a string end: the value the concatenated text would give
    n = t.size
    if n < 2:
        return False
    v, a, b, enda, endb = _pairs(t, off, s, l)
    L = l[1:].astype(np.int64)
    at_end = (a + L == enda) | (b + L == endb)
    j = M._nearest(v & at_end & _concat_more(t, a, b, np.minimum(L, n), n), max(int(where) - 1, 0))
    if j is None:
        return False
    x, y, h = int(a[j]), int(b[j]), int(L[j])
    while x + h < n and y + h < n and t[x + h] == t[y + h]:
        h += 1
    l[j + 1] = h
    return True


def _gorder_concat(t, off, s, i, l, where):
    # the order of the concatenated text where it differs: a ends first (so a comes first), but what follows a in the next
    # string is larger than what follows in b's own
    n = t.size
    if n < 2:
        return False
    v, a, b, enda, endb = _pairs(t, off, s, l)
    L = np.minimum(l[1:].astype(np.int64), n)
    m = v & (a + L == enda) & (b + L < endb) & (a + L < n)
    m[m] = t[(a + L)[m]] > t[(b + L)[m]]
    j = M._nearest(m, max(int(where) - 1, 0))
    if j is None:
        return False
    _swap(s, i, j + 1)
    return True


def _goff(step):
    def f(t, off, s, i, l, where):
        # the offsets handed to the checker moved by one character at one string (the arrays stay those of the true set)
        m = off.size - 1
        if m < 2:
            return False
        for k in range(m - 1):
            q = 1 + (int(where) + k) % (m - 1)
            if int(off[q - 1]) < int(off[q]) + step < int(off[q + 1]):
                off[q] = int(off[q]) + step
                return True
        return False
    return f


def _gl_one(value):
    def f(t, off, s, i, l, where):
        # an LCP of 1 at a suffix of one character (the base case of the recurrence) replaced
        if t.size < 2:
            return False
        v, a, b, enda, endb = _pairs(t, off, s, l)
        j = M._nearest(v & ((a + 1 == enda) | (b + 1 == endb)) & (l[1:] == 1), max(int(where) - 1, 0))
        if j is None:
            return False
        l[j + 1] = value
        return True
    return f


# name -> (function, positional, touches LCP only)
GSA_MUTANTS = {
    "Geq_swap": (_geq_swap, True, False),
    "Gl_past_end": (_gl_past_end, True, True),
    "Gorder_concat": (_gorder_concat, True, False),
    "Goff+1": (_goff(1), True, False),
    "Goff-1": (_goff(-1), True, False),
    "Gl_one0": (_gl_one(0), True, True),
    "Gl_one2": (_gl_one(2), True, True),
}
ALL = list(MUTANTS) + list(GSA_MUTANTS)
POSITIONAL = M.POSITIONAL + list(GSA_MUTANTS)
LCP_ONLY = M.LCP_ONLY + [k for k, v in GSA_MUTANTS.items() if v[2]]
MOVES_OFFSETS = ("Goff+1", "Goff-1")
# Arrays that are right for one set handed over with the offsets of another: nearly always wrong somewhere, but no rule says
# where, so no test asks these two classes for a positive count -- only for the model's counters.
MAY_PASS = MOVES_OFFSETS


def mutate_many_gsa(recipe, text, off, SA, ISA, LCP):
    """((text, off, SA, ISA, LCP) after the mutants [(class, where), ...] one after the other, the classes that applied)."""
    t, o, s, i, l = text.copy(), np.asarray(off, np.uint64).copy(), SA.copy(), ISA.copy(), LCP.copy()
    done = []
    for cls, where in recipe:
        if cls in GSA_MUTANTS:
            could = GSA_MUTANTS[cls][0](t, o, s, i, l, int(where))
        else:
            could = MUTANTS[cls][0](t, s, i, l, int(where))
        if could:
            done.append(cls)
    return (t, o, s, i, l), done


def mutate_gsa(name, text, off, SA, ISA, LCP, where=0):
    arrs, done = mutate_many_gsa([(name, where)], text, off, SA, ISA, LCP)
    return arrs if done else None


# ---------------------------------------------------------------------------------------------------------------
# the string sets both test modules use, with the oracle's arrays (nothing here is constructed on a GPU)
# ---------------------------------------------------------------------------------------------------------------
TINY = [1, 2, 3, 7, 8, 9, 17]                               # n around P for up to 8 ranks
BIG = ["reads", "copies", "prefixes", "unary", "tandem_pieces", "single"]
_sets, _arrays = {}, {}


def _cut(text, lengths):
    out, p = [], 0
    for k in lengths:
        if p >= text.size:
            break
        out.append(text[p:p + int(k)])
        p += int(k)
    if p < text.size:
        out.append(text[p:])
    return out


def strings_of(name):
    if not _sets:
        import inputs
        import oracle_lib as O
        rng = np.random.RandomState(11)
        genome = inputs.dna(60000, 21)
        starts = rng.randint(0, genome.size - 150, 400)
        _sets["reads"] = [genome[s:s + k] for s, k in zip(starts, rng.randint(100, 151, 400))]
        read = inputs.dna(120, 22)
        # deep ties: 150 copies of one read between a few others, and the read once more at the very end
        _sets["copies"] = [read] * 100 + [inputs.dna(90, 23)] + [read] * 50 + [inputs.dna(131, 24), read]
        long_read = inputs.dna(300, 25)
        _sets["prefixes"] = [long_read[:k] for k in rng.permutation(np.arange(1, 301))]
        _sets["unary"] = [np.full(k, 66, np.uint8) for k in rng.randint(1, 120, 150)]
        # a tandem repeat cut unevenly: neighbours share up to a whole piece, the range minima of the recurrence cross ranks
        _sets["tandem_pieces"] = _cut(inputs.tandem(60000, 512, O.rand_dna(512, 2)), rng.choice([1, 2, 50, 700, 1500, 3000], 200))
        _sets["single"] = [inputs.dna(30011, 26)]
        two = np.frombuffer(b"AC", np.uint8)
        for n in TINY:
            t = two[(inputs.dna(n, 7) > 70).astype(np.int64)]
            _sets["tiny%d" % n] = _cut(t, [2, 3, 1, 1, 3, 2, 1, 1, 1])      # (cut so that every class applies to the larger ones)
    return _sets[name]


def gsa_truth_of(text, off):
    import oracle_lib as O
    o = np.asarray(off, np.int64)
    ref = O.construct_ss([text[o[k]:o[k + 1]] for k in range(o.size - 1)], bits=64)
    return GsaTruth(text, off, ref["SA"], ref["ISA"], ref["LCP"])


def arrays(name, bits=64):
    """(text, offsets, SA, ISA, LCP, GsaTruth) of a named string set, the arrays from the oracle."""
    if (name, bits) not in _arrays:
        import oracle_lib as O
        ref = O.construct_ss(strings_of(name), bits=bits)
        _arrays[(name, bits)] = (ref["text"], ref["off"], ref["SA"], ref["ISA"], ref["LCP"],
                                 GsaTruth(ref["text"], ref["off"], ref["SA"], ref["ISA"], ref["LCP"]))
    return _arrays[(name, bits)]
