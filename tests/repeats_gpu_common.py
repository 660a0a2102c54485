"""What tests/test_gpu_bwt.py and tests/test_gpu_repeats.py share: text, SA, LCP and the index of LCP in HBM (SA and LCP from the
oracle), with calls of psacx_bwt_dev_* / psacx_repeats_dev_* whose outputs are pre-filled with a sentinel and have PAD entries of
room behind the last one, and the cases with their model results, computed once."""
import numpy as np

import repeats_model as M
from rmq_gpu_common import Indexed, PAD, SENTINEL

SENTINEL8 = 0x5A
SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097]        # bitmap words, one ballot, index groups; the second index level
BIG = (1 << 18) + 1                                                 # the third level of the index; 4097 words of 64 ranks


class Case(object):
    """A text or a string set with the oracle's SA and LCP and the model's BWT and repeats."""

    def __init__(self, strings, single):
        import oracle_lib as O
        self.strings = [bytes(s) for s in strings]
        self.text, off = M.flatten(self.strings)
        self.off = None if single else off
        self.n = int(self.text.size)
        ref = O.construct(self.text, bits=64) if single else O.construct_ss(self.strings, bits=64)
        self.SA, self.LCP = ref["SA"].astype(np.int64), ref["LCP"].astype(np.int64)
        self.bwt, self.first, self.primary = M.bwt_of(self.text, self.SA, self.off)
        self._results = {}

    def results(self, kind):
        if kind not in self._results:
            self._results[kind] = M.by_intervals(self.LCP, self.bwt, self.first, kind)
        return self._results[kind]

    def first_words(self):
        """the bitmap of psacx_bwt_dev_*: (n >> 5) + 1 words, bits at and beyond n clear"""
        bits = np.zeros(((self.n >> 5) + 1) * 32, np.uint8)
        bits[:self.n] = self.first
        return np.packbits(bits.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").reshape(-1).astype(np.uint32)


_cases = {}


def text_case(kind, n, seed=1):
    key = (kind, n, seed)
    if key not in _cases:
        _cases[key] = Case([M.text_of(kind, n, seed).tobytes()], True)
    return _cases[key]


def set_case(name):
    if name not in _cases:
        if name == "random":
            s = M.random_set(3000, 40, 11)
        elif name == "random2":
            s = M.random_set(4097, 700, 12, sigma=2)
        elif name == "singles":                        # m = n: every string has one byte
            s = M.random_set(300, 300, 13)
        elif name == "acgt3000":                       # 3000 identical strings: every interval holds 3000 ranks
            s = [b"ACGT"] * 3000
        elif name in ("w257", "w257twin"):             # x w for every byte x, and w itself; the twin has x = 7 twice instead of x = 8
            w = b"GATTACA"
            xs = list(range(256))
            if name == "w257twin":
                xs[8] = 7
            s = [bytes([x]) + w for x in xs] + [w]
        else:
            raise KeyError(name)
        _cases[name] = Case(s, False)
    return _cases[name]


SETS = ["random", "random2", "singles", "acgt3000", "w257", "w257twin"]


class RepIndex(object):
    """Text, SA, LCP with its index and, for a set, offsets and the bitmap of the string ends in HBM.  bwt / first: arrays to use
    instead of the device's own BWT; index: words to use instead of the built index."""

    def __init__(self, dev, case, SA=None, LCP=None, index=None):
        import psac_amd
        self.dev, self.case, self.n = dev, case, case.n
        self.text = case.text
        self.d_text = dev.put(self.text)
        self.sa = np.ascontiguousarray((case.SA if SA is None else np.asarray(SA)).astype(dev.dt))
        self.d_sa = dev.put(self.sa)
        self.lcp = Indexed(dev, (case.LCP if LCP is None else np.asarray(LCP)).astype(dev.dt), index)
        self.d_off = self.d_ends = None
        self.m = 0
        self.words = (self.n >> 5) + 1
        if case.off is not None:
            self.off = np.ascontiguousarray(case.off, dtype=np.uint64)
            self.m = int(self.off.size - 1)
            self.d_off = dev.put(self.off)
            self.d_ends = dev.room(self.words * 4)
            assert psac_amd.string_ends_device(dev.ctx, self.d_off, self.m, self.n, self.d_ends) == self.words
            self.ends = dev.get(self.d_ends, self.words, np.uint32)
        self.d_bwt = self.d_first = None

    def run_bwt(self, want_bwt=True, want_first=True, want_primary=True):
        """(bwt, first words, primary) as the device left them; an output not asked for comes back as None"""
        import psac_amd
        dev = self.dev
        self.d_bwt = dev.put(np.full(self.n + PAD, SENTINEL8, np.uint8)) if want_bwt else None
        self.d_first = dev.put(np.full(self.words + PAD, SENTINEL, np.uint32)) if want_first else None
        primary = psac_amd.bwt_device(dev.ctx, self.d_text, self.n, self.d_ends, self.d_sa, self.d_bwt, self.d_first, dev.bits, want_primary)
        bwt = first = None
        if want_bwt:
            raw = dev.get(self.d_bwt, self.n + PAD, np.uint8)
            assert np.all(raw[self.n:] == SENTINEL8)
            bwt = raw[:self.n]
        if want_first:
            raw = dev.get(self.d_first, self.words + PAD, np.uint32)
            assert np.all(raw[self.words:] == SENTINEL)
            first = raw[:self.words]
        return bwt, first, primary

    def put_bwt(self, bwt, first_words):
        """use these arrays as the BWT and the bitmap of the string starts"""
        self.d_bwt = self.dev.put(np.ascontiguousarray(bwt, np.uint8))
        self.d_first = self.dev.put(np.ascontiguousarray(first_words, np.uint32))

    def count(self, kind, min_len=0, min_occ=0, max_occ=0):
        import psac_amd
        left = kind != M.RIGHT
        return psac_amd.repeats_device(self.dev.ctx, self.n, self.lcp.d_v, self.lcp.d_index, self.d_bwt if left else None, self.d_first if left else None,
                                       kind, min_len, min_occ, max_occ, None, None, None, 0, self.dev.bits)

    def lists(self, kind, room, cap=None, min_len=0, min_occ=0, max_occ=0, want_len=True):
        """(lb, ub, len, z): the lists have `room` entries (+ PAD) and come back whole; cap defaults to room"""
        import psac_amd
        dev = self.dev
        init = np.full(room + PAD, SENTINEL, dev.dt)
        d_lb, d_ub, d_len = dev.put(init), dev.put(init), (dev.put(init) if want_len else None)
        self.d_lists = d_lb, d_ub, d_len
        z = None
        try:
            z = psac_amd.repeats_device(dev.ctx, self.n, self.lcp.d_v, self.lcp.d_index, self.d_bwt, self.d_first, kind, min_len, min_occ, max_occ,
                                        d_lb, d_ub, d_len, room if cap is None else cap, dev.bits)
        finally:
            self.raw = dev.get(d_lb, room + PAD), dev.get(d_ub, room + PAD), (dev.get(d_len, room + PAD) if want_len else None)
        return self.raw[0], self.raw[1], self.raw[2], z

    def run(self, kind, **filters):
        """(lb, ub, len) as int64 with z entries each; the count query agrees and everything behind the lists is untouched"""
        z = self.count(kind, **filters)
        lb, ub, ln, z2 = self.lists(kind, z, **filters)
        assert z2 == z and np.all(lb[z:] == SENTINEL) and np.all(ub[z:] == SENTINEL) and np.all(ln[z:] == SENTINEL)
        return lb[:z].astype(np.int64), ub[:z].astype(np.int64), ln[:z].astype(np.int64)

    def unchanged(self):
        dev = self.dev
        ok = np.array_equal(dev.get(self.d_text, self.n, np.uint8), self.text) and np.array_equal(dev.get(self.d_sa, self.n), self.sa)
        ok = ok and self.lcp.unchanged()
        if self.d_ends is not None:
            ok = ok and np.array_equal(dev.get(self.d_ends, self.words, np.uint32), self.ends)
        return bool(ok)


def agree(got, want_result, what):
    """the device's (lb, ub, len) are the model's triples, in the order of the heads"""
    want = M.triples(want_result)
    for g, w, part in zip(got, want, ("lb", "ub", "len")):
        assert g.size == w.size, (what, part, g.size, w.size)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (what, part, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]), int(bad.size))


def total(lb, ub, ln, n):
    """the totality clause of include/psacx.h"""
    return bool(np.all((0 <= lb) & (lb < ub) & (ub <= n) & (ub - lb >= 2) & (ln.astype(np.uint64) >= 1)))    # (all ones is a length)
