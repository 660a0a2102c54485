"""Host model of the longest common extension (psacx_lce_*), from the definitions in include/psacx.h.  LCE is stated twice:

  by_bytes(text, off, a, b, e)            the largest d <= L with at most e positions j < d where S[a+j] != S[b+j], counted byte
                                          by byte; L = min(end(a) - a, end(b) - b), end(p) = n for one text and the end of p's
                                          string for a set; a position >= n is the empty suffix.
  by_walk(ISA, LCP, off, n, a, b, e)      the kangaroo walk over the oracle's ISA and LCP: lce_0 is the minimum of LCP between the
                                          two ranks, a mismatch is stepped over while the budget lasts.  The text is not read.

Nothing here shares code with the library."""
import numpy as np


def end_of(off, n, p):
    """end(p): n without offsets; else the smallest offset above p, clamped to (p, n]; p itself for p >= n."""
    if p >= n:
        return p
    if off is None:
        return n
    o = np.asarray(off, np.uint64)
    i = int(np.searchsorted(o, np.uint64(p), side="right"))
    e = int(o[i]) if i < o.size else n
    return max(p + 1, min(e, n))


def limit(off, n, a, b):
    return min(end_of(off, n, a) - a, end_of(off, n, b) - b)


def by_bytes(text, off, a, b, e):
    t = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else text
    n = int(t.size)
    L = limit(off, n, a, b)
    if L <= 0:
        return 0
    w = 64                                                  # (windows that grow: most answers are short and L is long)
    while True:
        w = min(L, w)
        differ = np.nonzero(t[a:a + w] != t[b:b + w])[0]    # the positions j < w with S[a+j] != S[b+j], ascending
        if differ.size > e:
            return int(differ[e])                           # d may not reach past the (e + 1)-th of them
        if w == L:
            return L
        w *= 8


def lce0_by_arrays(ISA, LCP, off, n, a, b):
    if a == b:
        return end_of(off, n, a) - a
    r, s = int(ISA[a]), int(ISA[b])
    lo, hi = min(r, s) + 1, max(r, s) + 1
    return int(np.min(LCP[lo:hi]))


def by_walk(ISA, LCP, off, n, a, b, e):
    if a >= n or b >= n:
        return 0
    L = limit(off, n, a, b)
    if a == b:
        return L
    d, budget = 0, e
    while True:
        d += lce0_by_arrays(ISA, LCP, off, n, a + d, b + d)
        assert d <= L                                      # (the generalized LCP is cut at string ends)
        if d >= L or budget == 0:
            return d
        budget -= 1
        d += 1
        if d >= L:
            return d


def many(ISA, LCP, off, n, a, b, e):
    return np.array([by_walk(ISA, LCP, off, n, int(x), int(y), e) for x, y in zip(a, b)], np.int64)


def cli_text(lens):
    """What `lce` prints: one length per pair."""
    return "".join("%d\n" % int(x) for x in lens)


# ---------------------------------------------------------------------------------------------------------------
# arrays of the shared catalogues (locate_model texts, locate_gsa_model sets), 64-bit, by the oracle
# ---------------------------------------------------------------------------------------------------------------
_plain, _sets = {}, {}


def arrays(name):
    """(text, SA, ISA, LCP) of a named text of locate_model."""
    if name not in _plain:
        import locate_model as L
        import oracle_lib as O
        t = L.text_of(name)
        ref = O.construct(t, bits=64)
        _plain[name] = (t, ref["SA"], ref["ISA"], ref["LCP"])
    return _plain[name]


def set_arrays(name):
    """(text, off, SA, ISA, LCP) of a named set of locate_gsa_model, by O.construct_ss."""
    if name not in _sets:
        import locate_gsa_model as G
        import oracle_lib as O
        ref = O.construct_ss(G.strings_of(name), bits=64)
        _sets[name] = (np.asarray(ref["text"], np.uint8), np.asarray(ref["off"], np.uint64), ref["SA"], ref["ISA"], ref["LCP"])
    return _sets[name]
