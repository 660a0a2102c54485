"""What tests/test_gpu_lz77.py and tests/test_gpu_lz77_verifier.py share: SA, LCP and the index of LCP in HBM with calls of
psacx_lpf_dev_* / psacx_lz77_dev_* whose outputs are pre-filled with a sentinel and have PAD entries of room behind the last one."""
import numpy as np

import lz_model as M
from rmq_gpu_common import Indexed, PAD, SENTINEL


def top_of(dev):
    return int(np.iinfo(dev.dt).max)


def to_model(dev, a):
    """device values as int64, all ones as M.ONES"""
    a = np.asarray(a)
    return np.where(a == dev.dt(top_of(dev)), M.ONES, a.astype(np.int64)).astype(np.int64)


def from_model(dev, a):
    a = np.asarray(a, np.int64)
    return np.where(a == M.ONES, top_of(dev), a).astype(dev.dt)


class LzIndex(object):
    """SA, LCP and the index of LCP in HBM (index: words to use instead of the built ones)."""

    def __init__(self, dev, SA, LCP, index=None):
        self.dev = dev
        self.sa = np.ascontiguousarray(np.asarray(SA).astype(dev.dt))
        self.n = int(self.sa.size)
        self.d_sa = dev.put(self.sa)
        self.lcp = Indexed(dev, np.asarray(LCP).astype(dev.dt), index)

    def lpf(self):
        """(lpf, src) as the device left them (n entries of the index type each); self.d_out keeps the device arrays"""
        import psac_amd
        dev = self.dev
        init = np.full(self.n + PAD, SENTINEL, dev.dt)
        d_lpf, d_src = dev.put(init), dev.put(init)
        try:
            psac_amd.lpf_device(dev.ctx, self.n, self.d_sa, self.lcp.d_v, self.lcp.d_index, d_lpf, d_src, dev.bits)
        finally:
            self.d_out = d_lpf, d_src
            self.raw = dev.get(d_lpf, self.n + PAD), dev.get(d_src, self.n + PAD)
        assert np.all(self.raw[0][self.n:] == SENTINEL) and np.all(self.raw[1][self.n:] == SENTINEL)
        return self.raw[0][:self.n], self.raw[1][:self.n]

    def unchanged(self):
        return bool(np.array_equal(self.dev.get(self.d_sa, self.n), self.sa) and self.lcp.unchanged())


class Parse(object):
    """psacx_lz77_dev_* over n values in HBM (src: None for "no sources")."""

    def __init__(self, dev, lpf, src=None):
        self.dev = dev
        self.lpf = np.ascontiguousarray(np.asarray(lpf).astype(dev.dt))
        self.n = int(self.lpf.size)
        self.d_lpf = dev.put(self.lpf)
        self.src = None if src is None else np.ascontiguousarray(np.asarray(src).astype(dev.dt))
        self.d_src = None if src is None else dev.put(self.src)

    def count(self):
        import psac_amd
        return psac_amd.lz77_device(self.dev.ctx, self.n, self.d_lpf, self.d_src, None, None, 0, self.dev.bits)

    def lists(self, room, cap=None):
        """(start, psrc, z): the lists have `room` entries (+ PAD) and come back whole; cap defaults to room"""
        import psac_amd
        dev = self.dev
        init = np.full(room + PAD, SENTINEL, dev.dt)
        self.d_start, self.d_psrc = dev.put(init), (None if self.src is None else dev.put(init))
        try:
            z = psac_amd.lz77_device(dev.ctx, self.n, self.d_lpf, self.d_src, self.d_start, self.d_psrc, room if cap is None else cap, dev.bits)
        finally:
            self.raw = dev.get(self.d_start, room + PAD), (None if self.src is None else dev.get(self.d_psrc, room + PAD))
        return self.raw[0], self.raw[1], z

    def run(self):
        """(start as int64 with z + 1 entries, psrc in the model's terms or None); everything behind the lists is untouched"""
        z = self.count()
        start, psrc, z2 = self.lists(z + 1)
        assert z2 == z and np.all(start[z + 1:] == SENTINEL)
        if psrc is not None:
            assert np.all(psrc[z:] == SENTINEL)
            psrc = to_model(self.dev, psrc[:z])
        return start[:z + 1].astype(np.int64), psrc

    def unchanged(self):
        ok = np.array_equal(self.dev.get(self.d_lpf, self.n), self.lpf)
        return bool(ok and (self.src is None or np.array_equal(self.dev.get(self.d_src, self.n), self.src)))


def total(lpf, src, n):
    """the totality clause of include/psacx.h over model-form arrays"""
    i = np.arange(n)
    lit = lpf == 0
    return bool(np.all(src[lit] == M.ONES) and np.all((src[~lit] >= 0) & (src[~lit] < i[~lit])) and np.all(lpf[~lit] >= 1) and np.all(lpf <= n - i))
