"""What tests/test_gpu_rmq.py and tests/test_gpu_lce.py share: device memory that is freed together, an array with its
range-minimum index in HBM, and calls of psacx_rmq_dev_* / psacx_lce_dev_* whose outputs are pre-filled with a sentinel and have
three entries of room behind the last result."""
import numpy as np

SENTINEL = 0x5A5A5A5A
PAD = 3


class Dev(object):
    def __init__(self, ctx, bits):
        self.ctx, self.bits, self.dt = ctx, bits, (np.uint32 if bits == 32 else np.uint64)
        self.held = []

    def room(self, nbytes):
        p = self.ctx.alloc(max(1, nbytes))
        self.held.append(p)
        return p

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.room(arr.nbytes)
        if arr.nbytes:
            self.ctx.h2d(p, arr)
        return p

    def get(self, p, count, dt=None):
        out = np.empty(count, dt or self.dt)
        if count:
            self.ctx.d2h(out, p)
        return out

    def close(self):
        for p in self.held:
            self.ctx.free(p)
        self.held = []


class Ranges(object):
    """q ranges in device memory (uploaded once, used by many calls)."""

    def __init__(self, dev, lo, hi):
        self.lo, self.hi = np.asarray(lo).astype(dev.dt), np.asarray(hi).astype(dev.dt)
        self.q = int(self.lo.size)
        self.d_lo, self.d_hi = dev.put(self.lo), dev.put(self.hi)

    def unchanged(self, dev):
        return np.array_equal(dev.get(self.d_lo, self.q), self.lo) and np.array_equal(dev.get(self.d_hi, self.q), self.hi)


class Indexed(object):
    """An array and its range-minimum index in HBM (index: words to use instead of the built ones)."""

    def __init__(self, dev, values, index=None):
        import psac_amd
        self.dev = dev
        self.v = np.ascontiguousarray(values, dtype=dev.dt)
        self.n = int(self.v.size)
        self.d_v = dev.put(self.v)
        self.entries = psac_amd.rmq_index_device(dev.ctx, None, self.n, None, dev.bits)
        assert 1 <= self.entries <= self.n // 16 + 4096
        if index is None:
            self.d_index = dev.room(self.entries * (dev.bits // 8))
            assert psac_amd.rmq_index_device(dev.ctx, self.d_v, self.n, self.d_index, dev.bits) == self.entries
            self.index = dev.get(self.d_index, self.entries)
        else:
            self.index = np.ascontiguousarray(index[:self.entries], dtype=dev.dt)
            assert self.index.size == self.entries
            self.d_index = dev.put(self.index)

    def rmq(self, r, want_min=True, want_arg=True, q=None):
        """(min, arg) of psacx_rmq_dev_* for the first q ranges of r (all by default); an output not asked for comes back as it was
        pre-filled.  The entries behind the last result must be untouched."""
        import psac_amd
        dev = self.dev
        q = r.q if q is None else q
        init = np.full(q + PAD, SENTINEL, dev.dt)
        d_min, d_arg = dev.put(init), dev.put(init)
        try:
            psac_amd.rmq_device(dev.ctx, self.d_v, self.n, self.d_index, r.d_lo, r.d_hi, q, d_min if want_min else None, d_arg if want_arg else None,
                                dev.bits)
        finally:
            self.raw = dev.get(d_min, q + PAD), dev.get(d_arg, q + PAD)
        assert np.all(self.raw[0][q:] == SENTINEL) and np.all(self.raw[1][q:] == SENTINEL)
        return self.raw[0][:q], self.raw[1][:q]

    def unchanged(self):
        return np.array_equal(self.dev.get(self.d_v, self.n), self.v) and np.array_equal(self.dev.get(self.d_index, self.entries), self.index)


class LceIndex(object):
    """ISA, LCP, the index of LCP and (for a set) the offsets in HBM."""

    def __init__(self, dev, ISA, LCP, off=None, index=None):
        self.dev = dev
        self.isa = np.ascontiguousarray(np.asarray(ISA).astype(dev.dt))
        self.n = int(self.isa.size)
        self.d_isa = dev.put(self.isa)
        self.lcp = Indexed(dev, np.asarray(LCP).astype(dev.dt), index)
        self.off = None if off is None else np.ascontiguousarray(off, dtype=np.uint64)
        self.m = 0 if off is None else int(self.off.size - 1)
        self.d_off = None if off is None else dev.put(self.off)

    def lce(self, a, b, e=0, plain=False):
        """lengths as int64 of psacx_lce_dev_* (plain: without the offsets)"""
        import psac_amd
        dev = self.dev
        pa, pb = np.asarray(a).astype(dev.dt), np.asarray(b).astype(dev.dt)
        q = int(pa.size)
        d_a, d_b = dev.put(pa), dev.put(pb)
        d_len = dev.put(np.full(q + PAD, SENTINEL, dev.dt))
        try:
            psac_amd.lce_device(dev.ctx, self.n, None if plain else self.d_off, self.m, self.d_isa, self.lcp.d_v, self.lcp.d_index, d_a, d_b, q, e, d_len,
                                dev.bits)
        finally:
            self.raw = dev.get(d_len, q + PAD)
        assert np.all(self.raw[q:] == SENTINEL)
        assert np.array_equal(dev.get(d_a, q), pa) and np.array_equal(dev.get(d_b, q), pb)
        return self.raw[:q].astype(np.int64)

    def unchanged(self):
        ok = np.array_equal(self.dev.get(self.d_isa, self.n), self.isa) and self.lcp.unchanged()
        if self.off is not None:
            ok = ok and np.array_equal(self.dev.get(self.d_off, self.m + 1, np.uint64), self.off)
        return bool(ok)


def first_bad(got, want):
    """None, or (slot, got, want, how many differ)"""
    bad = np.nonzero(np.asarray(got).astype(np.uint64) != np.asarray(want).astype(np.uint64))[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return i, int(got[i]), int(want[i]), int(bad.size)
