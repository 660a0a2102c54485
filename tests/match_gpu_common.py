"""What tests/test_gpu_match.py and tests/test_gpu_match_gsa.py share: an index (text, suffix array, and for a string set its
offsets and bitmap) in device memory, pattern batches uploaded once at an odd device address, and calls of psacx_match_dev_* /
psacx_match_gsa_dev_* whose three outputs are pre-filled with a sentinel."""
import numpy as np

import locate_gsa_model as G
import locate_model as L

SENTINEL = 0x5A5A5A5A


class Batch(object):
    """A pattern buffer (at an odd device address) and its offsets in device memory."""

    def __init__(self, dev, pats, off=None):
        import psac_amd
        self.pats = pats
        self.pat, own = psac_amd.pattern_buffer(pats)
        self.off = own if off is None else np.asarray(off, np.uint64)
        self.q, self.total = int(self.off.size - 1), int(own[-1])
        self.d_pat, self.d_off = dev.put(self.pat, shift=1), dev.put(self.off)
        assert self.d_pat % 2 == 1


class Index(object):
    """Text and suffix array -- of a named text of locate_model, or with set=True of a named set of locate_gsa_model (arrays: a
    (text, off, SA) of the caller's instead) -- in device memory, entries of `bits`; everything allocated through it is freed by
    close()."""

    def __init__(self, ctx, name, bits, set=False, SA=None, arrays=None):
        import psac_amd
        self.ctx, self.bits, self.dt, self.set = ctx, bits, (np.uint32 if bits == 32 else np.uint64), set
        self.held = []
        if set:
            self.text, self.off, sa = G.arrays(name) if arrays is None else arrays
            self.m = int(self.off.size - 1)
        else:
            self.text, self.off, sa = L.text_of(name), None, L.sa_of(name)
        self.n = int(self.text.size)
        self.d_text = self.put(self.text)
        self.sa = (sa if SA is None else SA).astype(self.dt)
        self.d_sa = self.put(self.sa)
        self.d_ends = None
        if set:
            self.d_soff = self.put(self.off)
            self.words = psac_amd.string_ends_device(ctx, None, self.m, self.n, None)
            self.d_ends = self.room(self.words * 4)
            psac_amd.string_ends_device(ctx, self.d_soff, self.m, self.n, self.d_ends)

    def room(self, nbytes):
        p = self.ctx.alloc(max(1, nbytes))
        self.held.append(p)
        return p

    def put(self, arr, shift=0):
        p = self.room(arr.nbytes + shift) + shift
        if arr.nbytes:
            self.ctx.h2d(p, arr)
        return p

    def get(self, p, count, dt):
        out = np.empty(count, dt)
        if count:
            self.ctx.d2h(out, p)
        return out

    def batch(self, pats, off=None):
        return Batch(self, pats, off)

    def table(self, k):
        """(device address, k, code) of the index's lookup table, as match() and locate() take it, and the table as built"""
        import psac_amd
        if self.set:
            code, sigma, entries = psac_amd.lookup_table_gsa_device(self.ctx, self.d_text, self.n, None, k, None, self.bits)
        else:
            code, sigma, entries = psac_amd.lookup_table_device(self.ctx, self.d_text, self.n, None, k, None, self.bits)
        d_table = self.room(entries * (self.bits // 8))
        if self.set:
            psac_amd.lookup_table_gsa_device(self.ctx, self.d_text, self.n, self.d_ends, k, d_table, self.bits)
        else:
            psac_amd.lookup_table_device(self.ctx, self.d_text, self.n, self.d_sa, k, d_table, self.bits)
        return (d_table, k, code), self.get(d_table, entries, self.dt)

    def match(self, b, table=None, suffixes=False, max_len=0, out_entries=None, flags=None, fill=SENTINEL, d_ends=None, plain=False):
        """(len, lb, ub) as int64 of psacx_match_gsa_dev_* for a set (plain: psacx_match_dev_* on the same arrays) or psacx_match_dev_*.
        The outputs have room for the results the batch really has and are pre-filled; they are kept in self.raw, also when the
        call raises.  out_entries / flags: what to pass instead of the right values."""
        import psac_amd
        d_table, k, code = table if table is not None else (None, 0, None)
        room = b.total if suffixes else b.q
        entries = room if out_entries is None else out_entries
        flags = (psac_amd.MATCH_SUFFIXES if suffixes else 0) if flags is None else flags
        init = np.full(room, fill, self.dt)
        d_out = [self.put(init) for _ in range(3)]
        try:
            if self.set and not plain:
                psac_amd.match_gsa_device(self.ctx, self.d_text, self.n, d_ends or self.d_ends, self.d_sa, d_table, k, code, b.d_pat, b.d_off, b.q, flags,
                                          max_len, entries, d_out[0], d_out[1], d_out[2], self.bits)
            else:
                psac_amd.match_device(self.ctx, self.d_text, self.n, self.d_sa, d_table, k, code, b.d_pat, b.d_off, b.q, flags, max_len, entries,
                                      d_out[0], d_out[1], d_out[2], self.bits)
        finally:
            self.raw = [self.get(p, room, self.dt) for p in d_out]
        return tuple(x.astype(np.int64) for x in self.raw)

    def untouched(self, fill=SENTINEL):
        return all(np.all(x == fill) for x in self.raw)

    def locate(self, b, table=None):
        """(lb, ub) as int64 of psacx_locate_dev_* / psacx_locate_gsa_dev_* on the same inputs"""
        import psac_amd
        d_table, k, code = table if table is not None else (None, 0, None)
        d_lb, d_ub = self.room(b.q * 8), self.room(b.q * 8)
        if self.set:
            psac_amd.locate_gsa_device(self.ctx, self.d_text, self.n, self.d_ends, self.d_sa, d_table, k, code, b.d_pat, b.d_off, b.q, d_lb, d_ub, self.bits)
        else:
            psac_amd.locate_device(self.ctx, self.d_text, self.n, self.d_sa, d_table, k, code, b.d_pat, b.d_off, b.q, d_lb, d_ub, self.bits)
        return self.get(d_lb, b.q, self.dt).astype(np.int64), self.get(d_ub, b.q, self.dt).astype(np.int64)

    def inputs_unchanged(self, batches=()):
        ok = np.array_equal(self.get(self.d_text, self.n, np.uint8), self.text) and np.array_equal(self.get(self.d_sa, self.n, self.dt), self.sa)
        if self.set:
            ok = ok and np.array_equal(self.get(self.d_soff, self.m + 1, np.uint64), self.off)
            ok = ok and np.array_equal(self.get(self.d_ends, self.words, np.uint32), G.ends_bitmap(self.off, self.n))
        for b in batches:
            ok = ok and np.array_equal(self.get(b.d_pat, b.pat.size, np.uint8), b.pat) and np.array_equal(self.get(b.d_off, b.off.size, np.uint64), b.off)
        return bool(ok)

    def close(self):
        for p in self.held:
            self.ctx.free(p)
        self.held = []


def first_difference(got, want, queries):
    """None, or (which of len / lb / ub, the slot, the query's length and head, got, want, how many differ)"""
    for what, g, w in zip(("len", "lb", "ub"), got, want):
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        if bad.size:
            i = int(bad[0])
            return what, i, len(queries[i]), queries[i][:24], int(g[i]), int(w[i]), int(bad.size)
    return None


def total_holds(got, queries, n, max_len=0):
    """The totality clause: len <= m (and <= max_len), lb <= ub <= n."""
    ln, lb, ub = got
    m = np.array([len(Q) for Q in queries], np.int64)
    return bool(np.all(ln <= m) and (not max_len or np.all(ln <= max_len)) and np.all(lb <= ub) and np.all(ub <= n))
