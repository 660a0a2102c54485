"""What tests/test_gpu_mems*.py share: text, SA, LCP with its index, the BWT and the matching statistics of a pattern batch in HBM
(SA and LCP from the oracle; statistics, index and BWT from the library's own device calls, which their own tests pin), calls of
psacx_mems_dev_* whose outputs are pre-filled with a sentinel and have PAD entries of room behind the last one, and the model
results, computed once per case and shared."""
import numpy as np

import mems_model as X
from repeats_gpu_common import RepIndex
from rmq_gpu_common import PAD, SENTINEL

SENTINEL64 = 0x5A5A5A5A5A5A5A5A
SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097]
BIG = (1 << 18) + 1
TEXTS = ["dna2", "dna4", "a", "fib", "tandem7", "bytes256"]
REPETITIVE = ("a", "fib", "tandem7")


def patterns_of(kind, text, whole, seed=5):
    """Pieces cut from the text, the same with one byte substituted, random ones, an empty pattern, one byte, a byte the text lacks
    (where it lacks one) and, where asked for, the whole text.  Repetitive texts get fewer and shorter pieces: every slot of a piece
    of a^n owns about n candidates."""
    t = np.asarray(text, np.uint8)
    s, n = t.tobytes(), int(t.size)
    rng = np.random.RandomState(seed + n)
    few = kind in REPETITIVE
    lengths = (1, 7, 17) if few else (1, 7, 8, 9, 63, 64, 65, 130)
    present = np.zeros(256, bool)
    present[t] = True
    alphabet = np.nonzero(present)[0]
    absent = np.nonzero(~present)[0]
    out = [b""]
    for m in lengths:
        m = min(m, n)
        a = int(rng.randint(0, n - m + 1))
        out.append(s[a:a + m])
        P = bytearray(s[a:a + m])
        P[int(rng.randint(0, m))] = int(alphabet[rng.randint(0, alphabet.size)])
        out.append(bytes(P))
    out.append(bytes(alphabet[rng.randint(0, alphabet.size, min(n, 20))].astype(np.uint8)))
    out += [b"", s[n // 2:n // 2 + 1]]
    if absent.size:
        out.append(bytes([int(absent[0])]))
        out.append(s[:min(n, 5)] + bytes([int(absent[0])]) + s[:min(n, 5)])
    if whole:
        out.append(s)
    return out + [b""]


class MemsIndex(RepIndex):
    """RepIndex with the library's BWT, and a pattern batch with its statistics in HBM (stats: arrays to use instead)."""

    def __init__(self, dev, case, pats, SA=None, LCP=None, index=None, bwt=None, stats=None):
        import psac_amd
        RepIndex.__init__(self, dev, case, SA=SA, LCP=LCP, index=index)
        if bwt is None:
            self.run_bwt(want_primary=False)
            self.bwt_in = dev.get(self.d_bwt, self.n, np.uint8), dev.get(self.d_first, self.words, np.uint32)
        else:
            self.put_bwt(*bwt)
            self.bwt_in = np.ascontiguousarray(bwt[0], np.uint8), np.ascontiguousarray(bwt[1], np.uint32)
        self.pats = [bytes(P) for P in pats]
        self.pat, self.poff = X.pattern_buffer(self.pats)
        self.q, self.S = len(self.pats), int(self.poff[-1])
        self.d_pat, self.d_poff = dev.put(self.pat), dev.put(self.poff)
        if stats is None:
            d = [dev.room(self.S * (dev.bits // 8)) for _ in range(3)]
            if self.S:
                if case.off is None:
                    psac_amd.match_device(dev.ctx, self.d_text, self.n, self.d_sa, None, 0, None, self.d_pat, self.d_poff, self.q, psac_amd.MATCH_SUFFIXES, 0,
                                          self.S, d[0], d[1], d[2], dev.bits)
                else:
                    psac_amd.match_gsa_device(dev.ctx, self.d_text, self.n, self.d_ends, self.d_sa, None, 0, None, self.d_pat, self.d_poff, self.q,
                                              psac_amd.MATCH_SUFFIXES, 0, self.S, d[0], d[1], d[2], dev.bits)
            self.stats = tuple(dev.get(p, self.S) for p in d)
            self.d_stats = d
        else:
            self.stats = tuple(np.ascontiguousarray(np.asarray(a).astype(dev.dt)) for a in stats)
            self.d_stats = [dev.put(a) for a in self.stats]

    def call(self, min_len, max_occ, flags, room, cap=None, lists=True, work=None):
        """(qpos, tpos, len, z): the lists have `room` entries (+ PAD) and come back whole; cap defaults to room"""
        import psac_amd
        dev = self.dev
        d_q = d_t = d_l = None
        if lists:
            d_q = dev.put(np.full(room + PAD, SENTINEL64, np.uint64))
            d_t, d_l = dev.put(np.full(room + PAD, SENTINEL, dev.dt)), dev.put(np.full(room + PAD, SENTINEL, dev.dt))
        z = None
        try:
            z = psac_amd.mems_device(dev.ctx, self.n, self.d_sa, self.lcp.d_v, self.lcp.d_index, self.d_bwt, self.d_first, self.d_pat, self.d_poff, self.q,
                                     self.d_stats[0], self.d_stats[1], self.d_stats[2], min_len, max_occ, flags, d_q, d_t, d_l,
                                     room if cap is None else cap, dev.bits, work=work)
        finally:
            if lists:
                self.raw = dev.get(d_q, room + PAD, np.uint64), dev.get(d_t, room + PAD), dev.get(d_l, room + PAD)
        return (self.raw + (z,)) if lists else (None, None, None, z)

    def run(self, min_len=1, max_occ=0, flags=0):
        """((qpos, tpos, len) as int64 with z entries each, work): the count query agrees in z and work, and everything behind the
        lists is untouched"""
        w0, w1 = [], []
        z = self.call(min_len, max_occ, flags, 0, lists=False, work=w0)[3]
        qp, tp, ln, z2 = self.call(min_len, max_occ, flags, z, work=w1)
        assert z2 == z and w0 == w1, (z, z2, w0, w1)
        assert np.all(qp[z:] == SENTINEL64) and np.all(tp[z:] == SENTINEL) and np.all(ln[z:] == SENTINEL)
        return (qp[:z].astype(np.int64), tp[:z].astype(np.int64), ln[:z].astype(np.int64)), tuple(w1)

    def unchanged(self):
        dev = self.dev
        ok = RepIndex.unchanged(self)
        ok = ok and np.array_equal(dev.get(self.d_bwt, self.n, np.uint8), self.bwt_in[0])
        ok = ok and np.array_equal(dev.get(self.d_first, self.words, np.uint32), self.bwt_in[1])
        ok = ok and np.array_equal(dev.get(self.d_pat, self.S, np.uint8), self.pat) and np.array_equal(dev.get(self.d_poff, self.q + 1, np.uint64), self.poff)
        for p, a in zip(self.d_stats, self.stats):
            ok = ok and np.array_equal(dev.get(p, self.S), a)
        return bool(ok)


_models = {}


def model(key, case, pats, stats, min_len=1, max_occ=0, flags=0):
    """((qpos, tpos, len), work) of the model for a case, memoised under key with the parameters; the statistics of a later call under
    the same key (the other index width) must be the ones the model ran on"""
    k = (key, min_len, max_occ, flags)
    st = tuple(np.asarray(a).astype(np.int64) for a in stats)
    if k not in _models:
        _models[k] = (st, X.by_walk_arrays(case.SA, case.LCP, case.bwt, case.first, pats, st, min_len, max_occ, super=bool(flags & X.SUPER)))
    assert all(np.array_equal(a, b) for a, b in zip(st, _models[k][0])), ("statistics differ between calls", key)
    return _models[k][1]


def agree(got, want, what):
    """the device's (qpos, tpos, len) are the model's, in the pinned order"""
    for g, w, part in zip(got, want, ("qpos", "tpos", "len")):
        assert g.size == w.size, (what, part, g.size, w.size)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (what, part, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), int(bad.size))


def check(d, key, what, min_len=1, max_occ=0, flags=0):
    """one call against the model, the work counters included; returns (triples, work)"""
    got, work = d.run(min_len, max_occ, flags)
    want, wwork = model(key, d.case, d.pats, d.stats, min_len, max_occ, flags)
    agree(got, want, what)
    assert work == tuple(wwork), (what, work, wwork)
    return got, work


def statistics_agree(d):
    """the device's statistics are the model's (small cases)"""
    want = X.statistics(d.case.text, d.case.SA, d.pats, d.case.off)
    return all(np.array_equal(np.asarray(g).astype(np.int64), w) for g, w in zip(d.stats, want))


def total(got, d):
    """the totality clause of include/psacx.h: l >= 1, slot < poff[q], tpos copied from SA (it is some SA entry), and l inside the
    slot's pattern where the statistics are no longer than it"""
    qp, tp, ln = got
    if qp.size == 0:
        return True
    ends = np.repeat(d.poff[1:].astype(np.int64), np.diff(d.poff.astype(np.int64)))
    ok = np.all(ln >= 1) and np.all((0 <= qp) & (qp < d.S)) and np.all(qp + ln <= ends[qp])
    return bool(ok and np.all(np.isin(tp, d.sa.astype(np.int64))))

