"""What tests/test_gpu_kmismatch*.py share: text, SA, the bitmap of the string ends, a table and a pattern batch in HBM (SA from the
oracle, bitmap and table from the library's own device calls, which their own tests pin), calls of psacx_kmismatch_dev_* whose
outputs are pre-filled with a sentinel and have PAD entries of room behind the last one, and the comparison with the model
(tests/kmismatch_model.py), whose results are computed once per case and shared."""
import numpy as np

import kmismatch_model as X
import locate_model as L
from rmq_gpu_common import PAD, SENTINEL

SENTINEL64 = 0x5A5A5A5A5A5A5A5A
SENTINEL8 = 0x5A
BIG = (1 << 18) + 1


class KmmIndex(object):
    """Text, SA and (for a set) the bitmap in HBM, with a pattern batch.  SA: an array to use instead of the case's; k: the table in
    front of the search; table: entries to use instead of the built ones; shift: the pattern buffer starts that many bytes behind an
    allocation (1: an odd device address)."""

    def __init__(self, dev, case, pats, SA=None, k=0, table=None, shift=0):
        import psac_amd
        self.dev, self.case, self.n = dev, case, case.n
        self.text = case.text
        self.d_text = dev.put(self.text)
        self.sa = np.ascontiguousarray((case.SA if SA is None else np.asarray(SA)).astype(dev.dt))
        self.d_sa = dev.put(self.sa)
        self.words = (self.n >> 5) + 1
        self.d_ends = self.d_off = None
        if case.off is not None:
            self.off = np.ascontiguousarray(case.off, dtype=np.uint64)
            self.d_off = dev.put(self.off)
            self.d_ends = dev.room(self.words * 4)
            assert psac_amd.string_ends_device(dev.ctx, self.d_off, self.off.size - 1, self.n, self.d_ends) == self.words
            self.ends = dev.get(self.d_ends, self.words, np.uint32)
        self.pats = [bytes(P) for P in pats]
        self.pat, self.poff = X.pattern_buffer(self.pats)
        self.q, self.S = len(self.pats), int(self.poff[-1])
        self.shift = shift
        self.d_pat = dev.put(np.concatenate([np.zeros(shift, np.uint8), self.pat])) + shift
        self.d_poff = dev.put(self.poff)
        self.k, self.code, self.d_table, self.table = 0, None, None, None
        if k:
            self.set_table(k, table)

    def set_table(self, k, table=None):
        import psac_amd
        dev = self.dev
        size = (lambda d: psac_amd.lookup_table_device(dev.ctx, self.d_text, self.n, None, k, d, dev.bits)) if self.d_ends is None else \
               (lambda d: psac_amd.lookup_table_gsa_device(dev.ctx, self.d_text, self.n, self.d_ends, k, d, dev.bits))
        self.code, _, entries = size(None)
        if table is None:
            self.d_table = dev.room(entries * (dev.bits // 8))
            size(self.d_table)
            self.table = dev.get(self.d_table, entries)
        else:
            self.table = np.ascontiguousarray(np.resize(np.asarray(table), entries).astype(dev.dt))
            self.d_table = dev.put(self.table)
        self.k = k

    def no_table(self):
        self.k, self.code, self.d_table, self.table = 0, None, None, None

    def call(self, e, room, cap=None, lists=True, work=None, max_cand=0, poff=None, q=None):
        """(qid, tpos, dist, z): the lists have `room` entries (+ PAD) and come back whole; cap defaults to room"""
        import psac_amd
        dev = self.dev
        d_q = d_t = d_d = None
        if lists:
            d_q = dev.put(np.full(room + PAD, SENTINEL64, np.uint64))
            d_t, d_d = dev.put(np.full(room + PAD, SENTINEL, dev.dt)), dev.put(np.full(room + PAD, SENTINEL8, np.uint8))
        z = None
        try:
            z = psac_amd.kmismatch_device(dev.ctx, self.d_text, self.n, self.d_ends, self.d_sa, self.d_table, self.k, self.code, self.d_pat,
                                          self.d_poff if poff is None else poff, self.q if q is None else q, e, max_cand, d_q, d_t, d_d,
                                          room if cap is None else cap, dev.bits, work=work)
        finally:
            if lists:
                self.raw = dev.get(d_q, room + PAD, np.uint64), dev.get(d_t, room + PAD), dev.get(d_d, room + PAD, np.uint8)
        return (self.raw + (z,)) if lists else (None, None, None, z)

    def run(self, e):
        """((qid, tpos, dist) as int64 with z entries each, work): the count query agrees in z and work, and everything behind the
        lists is untouched"""
        w0, w1 = [], []
        z = self.call(e, 0, lists=False, work=w0)[3]
        qi, tp, di, z2 = self.call(e, z, work=w1)
        assert z2 == z and w0 == w1, (z, z2, w0, w1)
        assert np.all(qi[z:] == SENTINEL64) and np.all(tp[z:] == SENTINEL) and np.all(di[z:] == SENTINEL8)
        return (qi[:z].astype(np.int64), tp[:z].astype(np.int64), di[:z].astype(np.int64)), tuple(w1)

    def exact_positions(self):
        """the positions of psacx_occurrences_dev_* over psacx_locate_dev_* (or _gsa_) of the same patterns, as int64"""
        import psac_amd
        dev = self.dev
        d_lb, d_ub = dev.room(self.q * (dev.bits // 8)), dev.room(self.q * (dev.bits // 8))
        if self.d_ends is None:
            psac_amd.locate_device(dev.ctx, self.d_text, self.n, self.d_sa, self.d_table, self.k, self.code, self.d_pat, self.d_poff, self.q, d_lb, d_ub,
                                   dev.bits)
        else:
            psac_amd.locate_gsa_device(dev.ctx, self.d_text, self.n, self.d_ends, self.d_sa, self.d_table, self.k, self.code, self.d_pat, self.d_poff,
                                       self.q, d_lb, d_ub, dev.bits)
        # (an empty pattern is found everywhere and has no hits: its interval is emptied)
        lb, ub = dev.get(d_lb, self.q), dev.get(d_ub, self.q)
        empty = np.diff(self.poff.astype(np.int64)) == 0
        lb[empty] = 0
        ub[empty] = 0
        d_lb, d_ub = dev.put(lb), dev.put(ub)
        d_start = dev.room((self.q + 1) * 8)
        total = psac_amd.occurrences_device(dev.ctx, self.d_sa, self.n, None, 0, d_lb, d_ub, self.q, 0, d_start, None, None, 0, dev.bits)
        d_pos = dev.room(total * (dev.bits // 8))
        assert psac_amd.occurrences_device(dev.ctx, self.d_sa, self.n, None, 0, d_lb, d_ub, self.q, 0, d_start, d_pos, None, total, dev.bits) == total
        return dev.get(d_pos, total).astype(np.int64)

    def unchanged(self):
        dev = self.dev
        ok = np.array_equal(dev.get(self.d_text, self.n, np.uint8), self.text) and np.array_equal(dev.get(self.d_sa, self.n), self.sa)
        ok = ok and np.array_equal(dev.get(self.d_pat, self.S, np.uint8), self.pat) and np.array_equal(dev.get(self.d_poff, self.q + 1, np.uint64), self.poff)
        if self.d_ends is not None:
            ok = ok and np.array_equal(dev.get(self.d_ends, self.words, np.uint32), self.ends)
        if self.d_table is not None:
            ok = ok and np.array_equal(dev.get(self.d_table, self.table.size), self.table)
        return bool(ok)


def agree(got, want, what):
    """the device's (qid, tpos, dist) are the model's, in the pinned order"""
    for g, w, part in zip(got, want, ("qid", "tpos", "dist")):
        assert g.size == w.size, (what, part, g.size, w.size)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (what, part, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), int(bad.size))


def check(d, e, what, want=None):
    """one call against the model (want = (triples, work); by default the case's own patterns), the work counters included; returns
    (triples, work)"""
    got, work = d.run(e)
    wt, ww = d.case.results(e) if want is None else want
    agree(got, wt, what)
    assert work == tuple(ww), (what, work, ww)
    return got, work


def table_ks(text):
    """k = 1, 2 and the smallest k whose table has more than 2^16 entries"""
    B = int(np.unique(np.asarray(text, np.uint8)).size) + 1
    return (1, 2, L.smallest_k_above(B, 1 << 16))
