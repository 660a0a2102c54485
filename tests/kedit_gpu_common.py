"""What tests/test_gpu_kedit*.py share: the index and the pattern batch of tests/kmismatch_gpu_common.py in HBM, calls of
psacx_kedit_dev_* whose four outputs are pre-filled with a sentinel and have PAD entries of room behind the last one, and the
comparison with the model (tests/kedit_model.py), whose results are computed once per case and shared."""
import numpy as np

import kedit_model as K
from kmismatch_gpu_common import BIG, SENTINEL64, SENTINEL8, KmmIndex, table_ks  # noqa: F401
from rmq_gpu_common import PAD, SENTINEL

DEFINITION_UPTO = 65          # by_definition is the model up to this n, by_pieces (which test_kedit_model_cpu.py holds to it) beyond


class KedIndex(KmmIndex):
    """KmmIndex with the calls of the search with edits"""

    def call(self, e, room, cap=None, lists=True, work=None, max_cand=0, poff=None, q=None, flags=0):
        """(qid, tpos, len, dist, z): the lists have `room` entries (+ PAD) and come back whole; cap defaults to room"""
        import psac_amd
        dev = self.dev
        d_q = d_t = d_l = d_d = None
        if lists:
            d_q = dev.put(np.full(room + PAD, SENTINEL64, np.uint64))
            d_t, d_l = dev.put(np.full(room + PAD, SENTINEL, dev.dt)), dev.put(np.full(room + PAD, SENTINEL, dev.dt))
            d_d = dev.put(np.full(room + PAD, SENTINEL8, np.uint8))
        z = None
        try:
            z = psac_amd.kedit_device(dev.ctx, self.d_text, self.n, self.d_ends, self.d_sa, self.d_table, self.k, self.code, self.d_pat,
                                      self.d_poff if poff is None else poff, self.q if q is None else q, e, max_cand, flags, d_q, d_t, d_l, d_d,
                                      room if cap is None else cap, dev.bits, work=work)
        finally:
            if lists:
                self.raw = (dev.get(d_q, room + PAD, np.uint64), dev.get(d_t, room + PAD), dev.get(d_l, room + PAD),
                            dev.get(d_d, room + PAD, np.uint8))
        return (self.raw + (z,)) if lists else (None, None, None, None, z)

    def untouched(self, upto=0):
        q, t, l, d = self.raw
        return bool(np.all(q[upto:] == SENTINEL64) and np.all(t[upto:] == SENTINEL) and np.all(l[upto:] == SENTINEL) and np.all(d[upto:] == SENTINEL8))

    def run(self, e, flags=0):
        """((qid, tpos, len, dist) as int64 with z entries each, work): the count query agrees in z and work, and everything behind the
        lists is untouched"""
        w0, w1 = [], []
        z = self.call(e, 0, lists=False, work=w0, flags=flags)[4]
        qi, tp, ln, di, z2 = self.call(e, z, work=w1, flags=flags)
        assert z2 == z and w0 == w1, (z, z2, w0, w1)
        assert self.untouched(z)
        return (qi[:z].astype(np.int64), tp[:z].astype(np.int64), ln[:z].astype(np.int64), di[:z].astype(np.int64)), tuple(w1)


def agree(got, want, what):
    """the device's (qid, tpos, len, dist) are the model's, in the pinned order"""
    for g, w, part in zip(got, want, ("qid", "tpos", "len", "dist")):
        assert g.size == w.size, (what, part, g.size, w.size)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (what, part, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), int(bad.size))


def check(d, e, what, want=None, flags=0):
    """one call against the model (want = (quadruples, work); by default the case's own patterns by by_pieces, and by by_definition
    too up to DEFINITION_UPTO), the work counters included; returns (quadruples, work)"""
    got, work = d.run(e, flags)
    wq, ww = K.results(d.case, e) if want is None else want
    agree(got, K.best(wq) if flags else wq, what)
    assert work == tuple(ww), (what, work, ww)
    if want is None and d.n <= DEFINITION_UPTO and not flags:
        agree(got, K.results(d.case, e, definition=True), (what, "definition"))
    return got, work
