"""Host model of the two GPU checkers, and a catalogue of wrong arrays to hand them.

psacx_check_dev_* (one GPU) and psacx_multi_check_dev_* (block-distributed) return four counters.  The functions
here compute the same four numbers from the definitions in include/psacx.h, in plain numpy and 64-bit integers:

  common        e0 = #{i : SA[i] >= n or ISA[SA[i]] != i}.  Every other test runs at entries i that passed this one
                and, for i > 0, only if SA[i-1] < n.  e3 = [LCP given, entry 0 passed, LCP[0] != 0].
                Order at i > 0 with a = SA[i-1], b = SA[i]: fine iff t[a] < t[b] or (t[a] == t[b] and (a + 1 == n or
                (b + 1 < n and ISA[a+1] < ISA[b+1]))); e1 counts the entries that are not.
  one GPU       e2 = #{i > 0 examined : LCP[i] != number of characters the suffixes a and b share}, whether or not the
                order test passed.
  distributed   LCP is examined only where the order test passed: want = 0 if t[a] != t[b], 1 if a + 1 == n, else
                1 + min(LCP[ISA[a+1] + 1 .. ISA[b+1]]) over the arrays as given; e2 = #{LCP[i] != want}.  An entry whose
                order test passed with ISA[b+1] >= n (then ISA[a+1] < ISA[b+1] held between numbers that are no ranks) has
                no recurrence to satisfy: it is counted in e2 (check_verdict_kernel states the same rule).

The catalogue (MUTANTS) lists the ways SA / ISA / LCP / the text can be wrong, each a function
(text, SA, ISA, LCP, where) that changes the arrays in place and says whether it could; mutate() applies one to copies
and returns (text, SA, ISA, LCP), or None where the class cannot apply to these arrays at all.  A class that does not apply
at `where` moves to the nearest entry where it does.
"""
import numpy as np


class RangeMin(object):
    """Exact range minima over a fixed array: min(a[lo:hi]) for arrays of questions with lo < hi (sparse table)."""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.n = a.size
        self.lv = [a]
        k = 1
        while 2 * k <= a.size:
            prev = self.lv[-1]
            self.lv.append(np.minimum(prev[:-k], prev[k:]))
            k *= 2
        # all levels in one table where that stays small: a batch of questions is then two gathers
        self.tab = None
        if len(self.lv) * a.size * a.itemsize <= (1 << 28):
            self.tab = np.zeros((len(self.lv), a.size), a.dtype)
            for j, t in enumerate(self.lv):
                self.tab[j, :t.size] = t

    def query(self, lo, hi):
        lo = np.asarray(lo, np.int64); hi = np.asarray(hi, np.int64)
        assert np.all(lo < hi) and np.all(lo >= 0) and np.all(hi <= self.n)
        lev = (np.frexp((hi - lo).astype(np.float64))[1] - 1).astype(np.int64)          # floor(log2(hi - lo)), exact below 2^53
        if self.tab is not None:
            return np.minimum(self.tab[lev, lo], self.tab[lev, hi - (np.int64(1) << lev)])
        out = np.empty(lo.size, self.lv[0].dtype)
        for j in np.unique(lev):
            m = lev == j
            t = self.lv[j]
            out[m] = np.minimum(t[lo[m]], t[hi[m] - (1 << int(j))])
        return out


class Truth(object):
    """The correct ISA and LCP of a text (from the oracle), from which the number of characters any two suffixes
    share follows as a range minimum of the true LCP array between their ranks."""

    def __init__(self, text, SA, ISA, LCP):
        self.n = text.size
        self.SA = SA.astype(np.int64); self.ISA = ISA.astype(np.int64); self.LCP = LCP.astype(np.int64)
        self._rmq = None

    def shared(self, a, b, at=None):
        """Characters shared by the suffixes a[k] and b[k]; at[k]: an entry i with (SA0[i-1], SA0[i]) possibly == (a, b)."""
        out = np.empty(a.size, np.int64)
        todo = np.ones(a.size, bool)
        if at is not None and self.n > 1:
            i = np.clip(at, 1, self.n - 1)
            same = (self.SA[i - 1] == a) & (self.SA[i] == b)
            out[same] = self.LCP[i[same]]
            todo &= ~same
        eq = todo & (a == b)
        out[eq] = self.n - a[eq]
        todo &= ~eq
        if todo.any():
            if self._rmq is None:
                self._rmq = RangeMin(self.LCP)
            ra, rb = self.ISA[a[todo]], self.ISA[b[todo]]
            out[todo] = self._rmq.query(np.minimum(ra, rb) + 1, np.maximum(ra, rb) + 1)
        return out


def shared_by_characters(text, a, b):
    """The same by direct comparison, one character of every pair still equal per step: for texts with short repeats."""
    n = text.size
    h = np.zeros(a.size, np.int64)
    act = np.arange(a.size)
    while act.size:
        pa, pb = a[act] + h[act], b[act] + h[act]
        good = (pa < n) & (pb < n)
        good[good] = text[pa[good]] == text[pb[good]]
        act = act[good]
        h[act] += 1
    return h


def _common(text, SA, ISA, LCP):
    n = int(text.size)
    assert n > 0 and SA.size == n and ISA.size == n and (LCP is None or LCP.size == n)
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
    na, nb = ISAu[np.minimum(a + 1, n - 1)], ISAu[np.minimum(b + 1, n - 1)]          # read only where a + 1 < n and b + 1 < n
    a_last = a + 1 == n
    ok = (ta < tb) | ((ta == tb) & (a_last | ((b + 1 < n) & (na < nb))))
    return n, e0, e3, i, a, b, ta, tb, na, nb, a_last, ok


def _device(text, LCP, cm, truth):
    n, e0, e3, i, a, b, ta, tb, na, nb, a_last, ok = cm
    e2 = 0
    if LCP is not None and i.size:
        h = truth.shared(a, b, i) if truth is not None else shared_by_characters(text, a, b)
        e2 = int((LCP[i].astype(np.uint64) != h.astype(np.uint64)).sum())
    return [e0, int((~ok).sum()), e2, e3]


def _multi(text, LCP, cm, rmq):
    n, e0, e3, i, a, b, ta, tb, na, nb, a_last, ok = cm
    e2 = 0
    if LCP is not None and i.size:
        L = LCP.astype(np.uint64)
        want = np.zeros(i.size, np.uint64)
        want[(ta == tb) & a_last] = 1
        rec = ok & (ta == tb) & ~a_last                     # the recurrence proper: b + 1 < n and na < nb hold here
        none = rec & (nb >= np.uint64(n))                   # a rank that is none: counted, nothing looked up
        ask = rec & ~none
        if ask.any():
            if rmq is None:
                rmq = RangeMin(LCP)
            want[ask] = rmq.query(na[ask].astype(np.int64) + 1, nb[ask].astype(np.int64) + 1).astype(np.uint64) + np.uint64(1)
        e2 = int(none.sum()) + int((ok & ~none & (L[i] != want)).sum())
    return [e0, int((~ok).sum()), e2, e3]


def expect_device(text, SA, ISA, LCP, truth=None):
    """[e0, e1, e2, e3] of psacx_check_dev_*.  truth: a Truth of this very text (else characters are compared)."""
    return _device(text, LCP, _common(text, SA, ISA, LCP), truth)


def expect_multi(text, SA, ISA, LCP, rmq=None):
    """[e0, e1, e2, e3] of psacx_multi_check_dev_*, for any number of ranks and pieces.  rmq: a RangeMin of this very LCP."""
    return _multi(text, LCP, _common(text, SA, ISA, LCP), rmq)


def expect_both(text, SA, ISA, LCP, truth=None, rmq=None):
    """(expect_device, expect_multi) of the same arrays."""
    cm = _common(text, SA, ISA, LCP)
    return _device(text, LCP, cm, truth), _multi(text, LCP, cm, rmq)


# ---------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------
def _nearest(mask, where):
    """The index nearest to `where` at which mask holds (ties: the lower one), or None."""
    idx = np.nonzero(mask)[0]
    if idx.size == 0:
        return None
    k = np.searchsorted(idx, where)
    cand = [idx[q] for q in (k - 1, k) if 0 <= q < idx.size]
    return int(min(cand, key=lambda x: (abs(int(x) - int(where)), x)))


def _ones(a):
    return int(np.iinfo(a.dtype).max)


def _valid_sa(SA):
    return SA.astype(np.uint64) < np.uint64(SA.size)


# Every function below changes the arrays it is given in place and says whether it could (mutate() makes the copies).
def _lcp_mutant(apply, need_positive):
    def f(t, s, i, l, where):
        mask = np.ones(l.size, bool) if not need_positive else l > 0
        mask[0] = False                                      # LCP[0] has a class of its own
        j = _nearest(mask, where)
        if j is None:
            return False
        l[j] = apply(int(l[j]))
        return True
    return f


def _lbase(value):
    def f(t, s, i, l, where):
        n = t.size
        j = int(i[n - 1]) + 1                                # the entry whose predecessor is the one-character suffix
        if j >= n:
            return False
        l[j] = value if int(l[j]) != value else value + 1
        return True
    return f


def _lall(above):
    def f(t, s, i, l, where):
        if not (l > above).any():
            return False
        l[l > above] += 1
        return True
    return f


def _l0th(t, s, i, l, where):
    l[0] = 1
    return True


def _sswap(t, s, i, l, where):
    if t.size < 2:
        return False
    j = min(int(where), t.size - 2)
    s[j], s[j + 1] = s[j + 1], s[j]
    return True


def _siswap(kind):
    def f(t, s, i, l, where):
        n = t.size
        if n < 2:
            return False
        ok = _valid_sa(s)
        mask = ok[:-1] & ok[1:]
        sa = np.where(ok, s, 0).astype(np.int64)
        if kind == "eq":
            mask &= t[sa[:-1]] == t[sa[1:]]
        elif kind == "diff":
            mask &= t[sa[:-1]] != t[sa[1:]]
        else:
            mask &= (sa[:-1] == n - 1) | (sa[1:] == n - 1)
        j = _nearest(mask, where)
        if j is None:
            return False
        s[j], s[j + 1] = s[j + 1], s[j]
        i[int(s[j])], i[int(s[j + 1])] = j, j + 1
        return True
    return f


def _sdup(t, s, i, l, where):
    n = t.size
    if n < 2:
        return False
    s[int(where)] = s[(int(where) + max(1, n // 2)) % n]
    return True


def _srange(what):
    def f(t, s, i, l, where):
        n = t.size
        s[int(where)] = {"n": n, "far": n + 12345, "ones": _ones(s)}[what]
        return True
    return f


def _isa_mutant(what):
    def f(t, s, i, l, where):
        n = t.size
        j = _nearest(_valid_sa(s), where)
        if j is None or (n < 2 and what in ("near", "block")):
            return False
        x = int(s[j])                                        # the position whose rank entry j holds
        if what == "near":
            v = j + 1 if j + 1 < n else j - 1
        elif what == "block":
            v = (j + max(1, n // 2)) % n
        else:
            v = {"n": n, "2n": 2 * n, "ones": _ones(i)}[what]
        i[x] = v
        return True
    return f


def _text(t, s, i, l, where):
    j = _nearest(_valid_sa(s), where)
    if j is None:
        return False
    x = int(s[j])
    others = np.setdiff1d(np.unique(t), [t[x]])
    t[x] = others[0] if others.size else (int(t[x]) + 1) & 255
    return True


# name -> (function, positional, touches LCP only)
MUTANTS = {
    "L+": (_lcp_mutant(lambda v: v + 1, False), True, True),
    "L-": (_lcp_mutant(lambda v: v - 1, True), True, True),
    "L0": (_lcp_mutant(lambda v: 0, True), True, True),
    "Lbase0": (_lbase(0), False, True),
    "Lbase2": (_lbase(2), False, True),
    "Lall1": (_lall(0), False, True),
    "Lall2": (_lall(1), False, True),
    "L0th": (_l0th, False, True),
    "Sswap": (_sswap, True, False),
    "SIswap_eq": (_siswap("eq"), True, False),
    "SIswap_diff": (_siswap("diff"), True, False),
    "SIswap_last": (_siswap("last"), False, False),
    "Sdup": (_sdup, True, False),
    "Srange_n": (_srange("n"), True, False),
    "Srange_far": (_srange("far"), True, False),
    "Srange_ones": (_srange("ones"), True, False),
    "Iwrong_near": (_isa_mutant("near"), True, False),
    "Iwrong_block": (_isa_mutant("block"), True, False),
    "Irange_n": (_isa_mutant("n"), True, False),
    "Irange_2n": (_isa_mutant("2n"), True, False),
    "Irange_ones": (_isa_mutant("ones"), True, False),
    "Text": (_text, True, False),
}
POSITIONAL = [k for k, v in MUTANTS.items() if v[1]]
GLOBAL = [k for k, v in MUTANTS.items() if not v[1]]
LCP_ONLY = [k for k, v in MUTANTS.items() if v[2]]
WIDTH_DEPENDENT = ("Srange_ones", "Irange_ones")            # the only values that differ between the index types


def mutate_many(recipe, text, SA, ISA, LCP):
    """The arrays after the mutants [(class, where), ...] one after the other, and the classes that could be applied."""
    arrs = (text.copy(), SA.copy(), ISA.copy(), LCP.copy())
    done = [cls for cls, where in recipe if MUTANTS[cls][0](*arrs, int(where))]
    return arrs, done


def mutate(name, text, SA, ISA, LCP, where=0):
    """(text, SA, ISA, LCP) with one mutant applied, or None where the class cannot apply to these arrays."""
    arrs, done = mutate_many([(name, where)], text, SA, ISA, LCP)
    return arrs if done else None


def blocks(n, P):
    """(offsets, sizes) of mxx::blk_dist: the first n % P ranks hold one entry more."""
    sizes = [n // P + (1 if r < n % P else 0) for r in range(P)]
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    return offs[:-1], sizes


def positions(n, LCP, layouts, seed=1, every_edge=False):
    """{kind: [entries]} for the layouts [(P, chunks), ...] in use: entries 1 and n - 1, the first and last entry of a
    rank's block and of a piece of it (of the middle rank / middle piece, or of all with every_edge), the entry of the
    largest LCP value and three seeded random ones."""
    out = {"second": [min(1, n - 1)], "last": [n - 1], "block_first": [], "block_last": [], "piece_first": [], "piece_last": []}
    for P, chunks in layouts:
        offs, sizes = blocks(n, P)
        for r in (range(P) if every_edge else [P // 2]):
            if not sizes[r]:
                continue
            out["block_first"].append(offs[r]); out["block_last"].append(offs[r] + sizes[r] - 1)
            for q in (range(chunks) if every_edge else [chunks // 2]):
                lo, hi = sizes[r] * q // chunks, sizes[r] * (q + 1) // chunks
                if hi > lo:
                    out["piece_first"].append(offs[r] + lo); out["piece_last"].append(offs[r] + hi - 1)
    out["max_lcp"] = [int(np.argmax(LCP))]
    out["random"] = [int(x) for x in np.random.RandomState(seed).randint(0, n, 3)]
    return {k: sorted(set(v)) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------
# the texts both test modules use, with the oracle's arrays (the checkers take arrays: nothing here is constructed on a GPU)
# ---------------------------------------------------------------------------------------------------------------
TINY = [1, 2, 3, 7, 8, 9, 17]                               # n around P for up to 8 ranks: empty blocks, blocks of one entry
BIG = ["dna", "tandem", "unary", "low_entropy"]
_texts, _arrays = {}, {}


def text_of(name):
    if not _texts:
        import inputs
        import oracle_lib as O
        rng = np.random.RandomState(5)
        p = 0.5 ** np.arange(1, 21); p /= p.sum()
        _texts.update({"dna": inputs.dna(300007, 4), "tandem": inputs.tandem(120000, 512, O.rand_dna(512, 2)),
                       "unary": np.full(9001, 66, np.uint8), "low_entropy": (97 + rng.choice(20, size=200003, p=p)).astype(np.uint8)})
        two = np.frombuffer(b"AC", np.uint8)                 # two letters: repeats, so that every class applies, even this short
        _texts.update({"tiny%d" % n: two[(inputs.dna(n, 7) > 70).astype(np.int64)] for n in TINY})
    return _texts[name]


def truth_of(text):
    import oracle_lib as O
    ref = O.construct(text, bits=64)
    return Truth(text, ref["SA"], ref["ISA"], ref["LCP"])


def arrays(name, bits=64):
    """(text, SA, ISA, LCP, Truth) of a named text, the arrays from the oracle."""
    if (name, bits) not in _arrays:
        import oracle_lib as O
        text = text_of(name)
        ref = O.construct(text, bits=bits)
        _arrays[(name, bits)] = (text, ref["SA"], ref["ISA"], ref["LCP"], Truth(text, ref["SA"], ref["ISA"], ref["LCP"]))
    return _arrays[(name, bits)]
