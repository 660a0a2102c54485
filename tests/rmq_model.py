"""Host model of the batched range minimum (psacx_rmq_*), from the definitions in include/psacx.h: the minimum of
values[lo .. min(hi, n)) by np.min and its first position by np.argmin, which returns the first of equal minima as
std::min_element and the reference's rmq<>::query do; an empty range gives all ones of the type and n.  Nothing here shares
code with the library."""
import numpy as np


def ones(dtype):
    return int(np.iinfo(dtype).max)


def query(values, lo, hi):
    """(min, arg) of one range as Python ints."""
    v = np.asarray(values)
    n = int(v.size)
    lo, hi = int(lo), min(int(hi), n)
    if lo >= hi:
        return ones(v.dtype), n
    s = v[lo:hi]
    return int(s.min()), lo + int(np.argmin(s))


def queries(values, lo, hi):
    """(min, arg) of many ranges as arrays of the values' type."""
    v = np.asarray(values)
    out = [query(v, a, b) for a, b in zip(lo, hi)]
    return np.array([m for m, _ in out], v.dtype), np.array([a for _, a in out], v.dtype)


class Table(object):
    """The same answers for many ranges of a large array at once, stated a second way: every value is replaced by its rank among
    the distinct values, rank * n + position orders (value, position) pairs, and a sparse table of those keys gives the smallest
    pair of a range as the smaller of two overlapping windows -- its position is the first minimum.  Agrees with query()
    (tests/test_rmq_lce_model_cpu.py)."""

    def __init__(self, values):
        self.v = np.asarray(values)
        self.n = n = int(self.v.size)
        rank = np.unique(self.v, return_inverse=True)[1].astype(np.int64).reshape(-1)
        self.rows = [rank * n + np.arange(n, dtype=np.int64)]
        w = 1
        while 2 * w <= n:
            prev = self.rows[-1]
            self.rows.append(np.minimum(prev[:n - 2 * w + 1], prev[w:n - w + 1]))
            w *= 2

    def queries(self, lo, hi):
        n = self.n
        lo = np.asarray(lo).astype(np.int64)
        hi = np.minimum(np.asarray(hi).astype(np.int64), n)
        mn = np.full(lo.size, ones(self.v.dtype), self.v.dtype)
        arg = np.full(lo.size, n, self.v.dtype)
        ok = np.nonzero(lo < hi)[0]
        if ok.size:
            a, b = lo[ok], hi[ok]
            k = np.floor(np.log2((b - a).astype(np.float64))).astype(np.int64)
            k = np.where((1 << (k + 1)) <= b - a, k + 1, k)          # (guards against a rounded logarithm)
            k = np.where((1 << k) > b - a, k - 1, k)
            key = np.empty(ok.size, np.int64)
            for lv in np.unique(k):
                sel = k == lv
                row = self.rows[int(lv)]
                key[sel] = np.minimum(row[a[sel]], row[b[sel] - (1 << int(lv))])
            pos = key % n
            arg[ok] = pos
            mn[ok] = self.v[pos]
        return mn, arg
