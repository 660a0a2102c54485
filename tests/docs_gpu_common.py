"""What tests/test_gpu_docs*.py share: a string set with SA, LCP (from the oracle), the index of LCP and the offsets in HBM, calls of
psacx_doc_index_dev_* / psacx_doc_count_dev_* / psacx_doc_list_dev_* whose outputs are pre-filled with a sentinel and have PAD entries of
room behind the last one, and the cases with the model's prev / dup and intervals, computed once."""
import numpy as np

import docs_model as D
import repeats_model as M
from repeats_gpu_common import BIG, SETS, Case, set_case
from rmq_gpu_common import Indexed, PAD, SENTINEL, first_bad

SIZES = [1, 2, 63, 64, 65, 4095, 4096, 4097]
SENTINEL64 = 0x5A5A5A5A5A5A5A5A
EXTRA = 25                                             # the intervals lcp_intervals() always ends with: [0, n) and 12 + 12 locate intervals

_cases = {}


def doc_case(name):
    """a Case of repeats_gpu_common with .prev, .dup (the model's, int64) and .m"""
    if name not in _cases:
        if name in SETS:
            c = set_case(name)
        elif name == "one":                            # m = 1
            c = Case([M.random_set(777, 1, 21)[0]], False)
        elif name == "uneven":                         # one string of 4000 bytes among 97 of one byte: uneven segments of the sort
            rng = np.random.RandomState(22)
            singles = [bytes([b"ACGT"[x]]) for x in rng.randint(0, 4, 97)]
            c = Case(singles[:40] + [M.random_set(4000, 1, 23, sigma=2)[0]] + singles[40:], False)
        elif name[0] == "r":                           # r<n>: a random set of n bytes
            n = int(name[1:])
            c = Case(M.random_set(n, max(1, min(n, n // 3 if n < 100 else n // 50)), 30 + n % 97, sigma=2 if n % 2 else 4), False)
        else:
            raise KeyError(name)
        c.m = int(c.off.size - 1)
        c.prev, c.dup = D.index_of(c.SA, c.LCP, c.off)
        _cases[name] = c
    return _cases[name]


def locate_host(case, pattern):
    """[lb, ub) of the suffixes of the set that start with the pattern, by two binary searches over SA on the bytes"""
    t, n, P = case.text, case.n, bytes(pattern)
    end = np.repeat(case.off[1:], np.diff(case.off))

    def head(r):
        p = int(case.SA[r])
        return t[p:min(int(end[p]), p + len(P))].tobytes()

    lo, hi = 0, n
    while lo < hi:
        mid = (lo + hi) // 2
        if head(mid) < P:
            lo = mid + 1
        else:
            hi = mid
    lb, hi = lo, n
    while lo < hi:
        mid = (lo + hi) // 2
        if head(mid) <= P:
            lo = mid + 1
        else:
            hi = mid
    return lb, lo


def lcp_intervals(case, limit=None, seed=5):
    """(lb, ub) of LCP-intervals of the case: the right-maximal ones, the singletons, [0, n), and the locate intervals of patterns that occur
    and of patterns that do not (lb == ub); with limit, a sample of the first two kinds"""
    key = ("ivs", limit)
    if key not in case._results:
        lb, ub, _ = M.triples(case.results(M.RIGHT))
        n = case.n
        lb, ub = np.concatenate((lb, np.arange(n))), np.concatenate((ub, np.arange(n) + 1))
        rng = np.random.RandomState(seed)
        if limit is not None and lb.size > limit:
            pick = np.sort(rng.choice(lb.size, limit, replace=False))
            lb, ub = lb[pick], ub[pick]
        extra = [(0, n)]
        for k in range((EXTRA - 1) // 2):
            s = int(rng.randint(0, case.m))
            a, e = int(case.off[s]), int(case.off[s + 1])
            i = int(rng.randint(a, e))
            P = case.text[i:min(e, i + 1 + int(rng.randint(0, 6)))].tobytes()
            extra.append(locate_host(case, P))
            assert extra[-1][0] < extra[-1][1]
            extra.append(locate_host(case, P + b"\xff"))
            assert extra[-1][0] == extra[-1][1]
        case._results[key] = (np.concatenate((lb, [x[0] for x in extra])).astype(np.int64), np.concatenate((ub, [x[1] for x in extra])).astype(np.int64))
    return case._results[key]


def signed(a):
    """a device array as int64, all ones as -1"""
    a = np.asarray(a)
    out = a.astype(np.int64)
    out[a == np.iinfo(a.dtype).max] = D.NONE
    return out


class DocIndex(object):
    """Offsets, SA, LCP with its index in HBM; prev / dup in HBM once build() or put_index() has run."""

    def __init__(self, dev, case, SA=None):
        self.dev, self.case, self.n, self.m = dev, case, case.n, case.m
        self.sa = np.ascontiguousarray((case.SA if SA is None else np.asarray(SA)).astype(dev.dt))
        self.d_sa = dev.put(self.sa)
        self.off = np.ascontiguousarray(case.off, dtype=np.uint64)
        self.d_off = dev.put(self.off)
        self.lcp = Indexed(dev, case.LCP.astype(dev.dt))
        self.d_prev = self.d_dup = None

    def build(self, want_prev=True, want_dup=True):
        """(prev, dup) as int64 as the device left them (all ones: -1); an output not asked for comes back as None"""
        import psac_amd
        dev, n = self.dev, self.n
        d_prev = dev.put(np.full(n + PAD, SENTINEL, dev.dt)) if want_prev else None
        d_dup = dev.put(np.full(n + 1 + PAD, SENTINEL, dev.dt)) if want_dup else None
        psac_amd.doc_index_device(dev.ctx, n, self.d_off, self.m, self.d_sa, self.lcp.d_v, self.lcp.d_index, d_prev, d_dup, dev.bits)
        prev = dup = None
        if want_prev:
            raw = dev.get(d_prev, n + PAD)
            assert np.all(raw[n:] == SENTINEL)
            prev, self.d_prev = signed(raw[:n]), d_prev
        if want_dup:
            raw = dev.get(d_dup, n + 1 + PAD)
            assert np.all(raw[n + 1:] == SENTINEL)
            dup, self.d_dup = raw[:n + 1].astype(np.int64), d_dup
        return prev, dup

    def put_index(self, prev=None, dup=None):
        """use these words as prev / dup"""
        if prev is not None:
            self.d_prev = self.dev.put(np.ascontiguousarray(prev, self.dev.dt))
        if dup is not None:
            self.d_dup = self.dev.put(np.ascontiguousarray(dup, self.dev.dt))

    def count(self, lb, ub):
        """docs as int64"""
        import psac_amd
        dev = self.dev
        a, b = np.asarray(lb).astype(dev.dt), np.asarray(ub).astype(dev.dt)
        q = int(a.size)
        d_lb, d_ub, d_docs = dev.put(a), dev.put(b), dev.put(np.full(q + PAD, SENTINEL, dev.dt))
        psac_amd.doc_count_device(dev.ctx, self.n, self.d_dup, d_lb, d_ub, q, d_docs, dev.bits)
        raw = dev.get(d_docs, q + PAD)
        assert np.all(raw[q:] == SENTINEL)
        assert np.array_equal(dev.get(d_lb, q), a) and np.array_equal(dev.get(d_ub, q), b)
        return raw[:q].astype(np.int64)

    def lists(self, lb, ub, room=None, cap=None, max_cand=0, want_sid=True, want_pos=True):
        """(start, sid, pos, total) whole as the device left them: start has q + 1 (+ PAD) entries, the lists `room` (+ PAD); room
        defaults to the size query's total, cap to room.  self.error: the code of a refused call, else 0."""
        import psac_amd
        dev = self.dev
        a, b = np.asarray(lb).astype(dev.dt), np.asarray(ub).astype(dev.dt)
        q = int(a.size)
        d_lb, d_ub = dev.put(a), dev.put(b)
        if room is None:
            d_size = dev.put(np.full(q + 1 + PAD, SENTINEL64, np.uint64))
            room = psac_amd.doc_list_device(dev.ctx, self.d_sa, self.n, self.d_off, self.m, self.d_prev, d_lb, d_ub, q, max_cand, d_size, None, None, 0,
                                            dev.bits)
            self.size_start = dev.get(d_size, q + 1 + PAD, np.uint64)
        d_start = dev.put(np.full(q + 1 + PAD, SENTINEL64, np.uint64))
        init = np.full(room + PAD, SENTINEL, dev.dt)
        d_sid, d_pos = (dev.put(init) if want_sid else None), (dev.put(init) if want_pos else None)
        total, self.error = None, 0
        try:
            total = psac_amd.doc_list_device(dev.ctx, self.d_sa, self.n, self.d_off, self.m, self.d_prev, d_lb, d_ub, q, max_cand, d_start, d_sid, d_pos,
                                             room if cap is None else cap, dev.bits)
        except psac_amd.PsacxError as e:
            self.error, total = e.code, e.total
        start = dev.get(d_start, q + 1 + PAD, np.uint64)
        sid = dev.get(d_sid, room + PAD) if want_sid else None
        pos = dev.get(d_pos, room + PAD) if want_pos else None
        assert np.array_equal(dev.get(d_lb, q), a) and np.array_equal(dev.get(d_ub, q), b)
        return start, sid, pos, total

    def run_lists(self, lb, ub, want, what):
        """the size query and the lists agree with want = (start, ranks, sid, pos) of the model; nothing behind them is touched"""
        q = len(lb)
        start, sid, pos, total = self.lists(lb, ub)
        w_start, _, w_sid, w_pos = want
        z = int(w_start[-1])
        assert self.error == 0 and total == z, (what, total, z)
        for got in (start, self.size_start):
            assert np.all(got[q + 1:] == SENTINEL64) and first_bad(got[:q + 1], w_start) is None, (what, first_bad(got[:q + 1], w_start))
        assert np.all(sid[z:] == SENTINEL) and np.all(pos[z:] == SENTINEL), what
        assert first_bad(sid[:z], w_sid) is None, (what, "sid", first_bad(sid[:z], w_sid))
        assert first_bad(pos[:z], w_pos) is None, (what, "pos", first_bad(pos[:z], w_pos))

    def unchanged(self):
        dev = self.dev
        ok = np.array_equal(dev.get(self.d_sa, self.n), self.sa) and np.array_equal(dev.get(self.d_off, self.m + 1, np.uint64), self.off)
        return bool(ok and self.lcp.unchanged())


def check_index(d, what, want_prev=None, want_dup=None):
    """prev and dup equal the model exactly, together and each output alone"""
    c = d.case
    want_prev = c.prev if want_prev is None else want_prev
    want_dup = c.dup if want_dup is None else want_dup
    for wp, wd in ((True, True), (True, False), (False, True)):
        prev, dup = d.build(wp, wd)
        if wp:
            assert first_bad(prev.astype(np.uint64), want_prev.astype(np.uint64)) is None, (what, "prev", first_bad(prev.astype(np.uint64), want_prev.astype(np.uint64)))
        if wd:
            assert first_bad(dup, want_dup) is None, (what, "dup", first_bad(dup, want_dup))
    d.build()


def check_queries(d, what, limit=None):
    """counts over the LCP-intervals and the malformed ones; lists over a sample of the right-maximal intervals and singletons, over [0, n),
    every locate interval (those with lb == ub too), the malformed ones and random arbitrary ones (prev / dup are in HBM)"""
    c, n = d.case, d.n
    lb, ub = lcp_intervals(c, limit)
    bad_lb, bad_ub = np.array([n, 1, 0, n + 1]), np.array([n - 1 if n else 0, 0, n + 1, n + 2])
    bad_lb[0] = n                                      # lb > ub
    qa, qb = np.concatenate((lb, bad_lb)), np.concatenate((ub, bad_ub))
    want = D.count_by_dup(c.dup, qa, qb, n)
    assert np.all(want[lb.size:] == 0)
    got = d.count(qa, qb)
    assert first_bad(got, want) is None, (what, "docs", first_bad(got, want))
    # lists: a sample of those intervals, arbitrary ones, empty ones and malformed ones
    rng = np.random.RandomState(n % 1000)
    inner = lb.size - EXTRA                            # right-maximal intervals and singletons: a sample; [0, n) and the locate intervals: all
    pick = np.concatenate((np.sort(rng.choice(inner, min(inner, 300), replace=False)), np.arange(inner, lb.size)))
    ra, rb = D.random_intervals(n, 200, n % 89)
    la, lu = np.concatenate((lb[pick], ra, bad_lb)), np.concatenate((ub[pick], rb, bad_ub))
    model = D.list_by_prev(c.prev, c.SA, c.off, la, lu, n)
    lens = np.diff(model[0])
    k = pick.size
    assert np.array_equal(lens[:k], D.count_by_dup(c.dup, la[:k], lu[:k], n))                  # the two halves of the index agree on LCP-intervals
    d.run_lists(la, lu, model, what)
    return la, lu, model
