"""What tests/test_gpu_fm_extract*.py share: the FmDev of tests/fm_gpu_common.py with the text samples beside the blob, calls of
psacx_fm_text_samples_dev_* / psacx_fm_extract_dev_* whose outputs are pre-filled and have room behind the last entry that must stay as
it was, and the windows every case asks for."""
import numpy as np

import fm_extract_model as X
from fm_gpu_common import FILL64, FmDev
from rmq_gpu_common import PAD, SENTINEL

FILL8 = 0x5A
RATES = [1, 2, 3, 32, 64]                               # and n + 5


class ExtDev(FmDev):
    def __init__(self, dev, case):
        FmDev.__init__(self, dev, case)
        self.d_ts = self.ts = self.rate = None

    def entries(self, rate):
        import psac_amd
        return psac_amd.fm_text_samples_device(self.dev.ctx, self.n, None, self.d_off, self.m, rate, None, self.dev.bits)

    def samples(self, rate):
        """the sample array as the device left it, as int64; the entries behind it keep their fill"""
        import psac_amd
        dev = self.dev
        entries = self.entries(rate)
        assert entries == self.n // rate + max(self.m, 1)
        self.d_ts = dev.put(np.full(entries + PAD, SENTINEL, dev.dt))
        assert psac_amd.fm_text_samples_device(dev.ctx, self.n, self.d_sa, self.d_off, self.m, rate, self.d_ts, dev.bits) == entries
        raw = dev.get(self.d_ts, entries + PAD)
        assert np.all(raw[entries:] == SENTINEL)
        self.ts, self.rate = raw[:entries].copy(), rate
        return self.ts.astype(np.int64)

    def put_samples(self, ts, rate):
        self.ts, self.rate = np.ascontiguousarray(ts, dtype=self.dev.dt), rate
        self.d_ts = self.dev.put(self.ts)

    def extract(self, pos, ln, cap=None, query=False):
        """(total, start, out); out has PAD bytes more than cap (the expected total by default), pre-filled"""
        import psac_amd
        dev = self.dev
        p, l = np.asarray(pos).astype(dev.dt), np.asarray(ln).astype(dev.dt)
        q = int(p.size)
        want_total = int(X.by_bytes(self.case.strings, p, l)[0][-1])
        cap = want_total if cap is None else cap
        room = max(cap, want_total) + PAD
        d_pos, d_len = dev.put(p), dev.put(l)
        d_start = dev.put(np.full(q + 1, FILL64, np.uint64))
        d_out = dev.put(np.full(room, FILL8, np.uint8))
        try:
            total = psac_amd.fm_extract_device(dev.ctx, self.d_fm, self.info, self.d_ts, self.rate, self.d_off, self.m, d_pos, d_len, q, d_start,
                                               None if query else d_out, cap, dev.bits)
        finally:
            self.start, self.out = dev.get(d_start, q + 1, np.uint64), dev.get(d_out, room, np.uint8)
            assert np.array_equal(dev.get(d_pos, q), p) and np.array_equal(dev.get(d_len, q), l)
        return total, self.start, self.out

    def check(self, pos, ln):
        """the bytes equal the slices of the text, and nothing is written behind the total"""
        want = X.by_bytes(self.case.strings, pos, ln)
        total, start, out = self.extract(pos, ln)
        assert total == int(want[0][-1]) and np.array_equal(start, want[0])
        assert np.array_equal(out[:total], want[1]) and np.all(out[total:] == FILL8)
        return total

    def unchanged(self):
        ok = FmDev.unchanged(self)
        if self.d_ts is not None:
            ok = ok and np.array_equal(self.dev.get(self.d_ts, self.ts.size), self.ts)
        if self.d_off is not None:
            ok = ok and np.array_equal(self.dev.get(self.d_off, self.off.size, np.uint64), self.off)
        return bool(ok)


def whole_strings(c):
    off = np.array([0, c.n], np.int64) if c.single else c.off
    return off[:-1], np.diff(off)


def windows_of(c, rate, seed=9):
    """(pos, len): empty windows, windows that start on a string's last byte, that end exactly on a block boundary, exactly on a string's
    end and past it, windows at and beyond n, windows over whole short strings, and random ones"""
    n = c.n
    off = np.array([0, n], np.int64) if c.single else c.off
    rng = np.random.RandomState(seed)
    pos, ln = [], []

    def add(p, l):
        pos.append(int(p))
        ln.append(int(l))
    pick = np.unique(np.concatenate((np.arange(min(12, off.size - 1)), rng.randint(0, off.size - 1, 12), [off.size - 2])))
    for j in pick:
        a, e = int(off[j]), int(off[j + 1])
        add(e - 1, 1), add(e - 1, 5), add(e - 1, 0)                     # from the last byte
        add(a, e - a), add(a, e - a + 3), add(a, n + 7)                   # the string, and past its end
        add(max(a, e - 3), e - max(a, e - 3))                             # ends exactly on the string's end
        add(a + (e - a) // 2, 0)
    for k in np.unique(np.concatenate((np.arange(min(4, n // rate + 1)), rng.randint(0, n // rate + 1, 6)))):
        b = min(n, (int(k) + 1) * rate)
        if b:
            add(max(0, b - 5), b - max(0, b - 5))                         # ends exactly on a block boundary
            add(b - 1, 1)
        if b < n:
            add(b, 2 * rate + 1)                                          # starts on one
    for _ in range(30):
        add(rng.randint(0, n), rng.randint(0, 100))
    add(n, 1), add(n + 1, 5), add(n + 1000, 0), add(0, 0), add(n - 1, 1), add(0, n)
    return np.array(pos, np.int64), np.array(ln, np.int64)
