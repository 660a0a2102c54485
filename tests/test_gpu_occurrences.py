"""psacx_occurrences_dev_* against the plain loop of tests/locate_gsa_model.py: the intervals of every catalogue set, hand-made
batches (all empty, one interval over many tiles, long runs of empty intervals, inverted and overlong intervals, batch sizes
around a wave), limits, the capacity rules, the size query, one text, and SA entries beyond n."""
import numpy as np
import pytest

import locate_gsa_model as M

pytestmark = pytest.mark.gpu

FILL = 0x6B


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


class Occ(object):
    """SA and offsets of a set in device memory; run() calls psacx_occurrences_dev_* on a batch of intervals."""

    def __init__(self, ctx, SA, n, off, bits):
        self.ctx, self.bits, self.dt = ctx, bits, (np.uint32 if bits == 32 else np.uint64)
        self.n, self.off = int(n), off
        self.m = 0 if off is None else int(len(off) - 1)
        self.sa = np.asarray(SA).astype(self.dt)
        self.held = []
        self.d_sa = self.put(self.sa)
        self.d_off = None if off is None else self.put(np.asarray(off, np.uint64))

    def put(self, arr):
        p = self.ctx.alloc(max(1, arr.nbytes))
        self.held.append(p)
        if arr.nbytes:
            self.ctx.h2d(p, arr)
        return p

    def get(self, p, count, dt):
        out = np.empty(count, dt)
        if count:
            self.ctx.d2h(out, p)
        return out

    def run(self, lb, ub, limit=0, cap=None, query=False, sid=True, offsets=True):
        """(total, start, pos, sid) as the device left them; pos and sid have cap entries (the model's total by default) and one
        more, which must keep its fill.  query: d_pos = NULL."""
        import psac_amd
        lo, hi = np.asarray(lb).astype(self.dt), np.asarray(ub).astype(self.dt)
        q = int(lo.size)
        want_total = int(M.occurrences(self.sa, self.n, lo, hi, limit)[0][-1])
        cap = want_total if cap is None else cap
        d_lb, d_ub = self.put(lo), self.put(hi)
        d_start = self.put(np.full(q + 1, FILL, np.uint64))
        room = max(cap, want_total) + 1
        d_pos, d_sid = self.put(np.full(room, FILL, self.dt)), self.put(np.full(room, FILL, self.dt))
        with_sid = sid and self.off is not None
        try:
            self.total = psac_amd.occurrences_device(self.ctx, self.d_sa, self.n, self.d_off if offsets else None, self.m, d_lb, d_ub, q, limit, d_start,
                                                     None if query else d_pos, d_sid if with_sid and not query else None, cap, self.bits)
        finally:
            self.start = self.get(d_start, q + 1, np.uint64)
            self.pos, self.sid = self.get(d_pos, room, self.dt), self.get(d_sid, room, self.dt)
            same = (np.array_equal(self.get(self.d_sa, self.sa.size, self.dt), self.sa) and np.array_equal(self.get(d_lb, q, self.dt), lo)
                    and np.array_equal(self.get(d_ub, q, self.dt), hi))
        assert same                                                                      # no input is written
        return self.total, self.start, self.pos, self.sid

    def check(self, lb, ub, limit=0):
        """run() equals the model; nothing is written beyond the total."""
        want = M.occurrences(self.sa, self.n, np.asarray(lb).astype(self.dt), np.asarray(ub).astype(self.dt), limit)
        total, start, pos, sid = self.run(lb, ub, limit)
        assert total == int(want[0][-1]) and np.array_equal(start, want[0])
        assert np.array_equal(pos[:total].astype(np.uint64), want[1]) and np.all(pos[total:] == FILL)
        if self.off is not None:
            assert np.array_equal(sid[:total].astype(np.uint64), M.string_ids(self.off, want[1], self.n)) and np.all(sid[total:] == FILL)
        return total

    def close(self):
        for p in self.held:
            self.ctx.free(p)
        self.held = []


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", M.GPU)
def test_lists_of_the_catalogue_equal_the_model(ctx, name, bits):
    text, off, SA = M.arrays(name)
    pats, lb, ub = M.expected(name)
    o = Occ(ctx, SA, text.size, off, bits)
    try:
        total = o.check(lb, ub)
        assert total >= text.size                                                        # (the empty pattern is one of them)
        longest = int((ub - lb).max())
        for limit in sorted(set([1, 2, max(1, longest - 1)])):
            assert o.check(lb, ub, limit) <= total
    finally:
        o.close()


HAND_N = 4097                                                                            # unary: SA = n - 1 .. 0; four tiles and one slot
HAND_OFF = np.array([0, 1, 31, 32, 33, 64, 1000, 1001, 4096, HAND_N], np.uint64)


def hand_made_batches():
    """(lb, ub, limit, the total stated by hand or None) of the hand-made batches over HAND_N ranks, in a fixed order"""
    n = HAND_N
    empties = [9] * 1000
    out = [([], [], 0, 0),
           ([5] * 300, [5] * 300, 0, 0),                                                 # all empty
           ([0], [n], 0, n),                                                             # one interval over every tile
           ([0, 7], [n, n], 0, 2 * n - 7),
           ([3] + empties + [100], [10] + empties + [2500], 0, 7 + 2400),                # 1 000 empty intervals between two others
           ([9, 3, 100, 9], [9, 10, 2500, 9], 0, 7 + 2400),                              # an empty interval first and last
           ([7, 0, 5, n - 3, n], [6, n + 1, 9, n, n], 0, 4 + 3)]                         # lb > ub and ub > n count 0
    rng = np.random.RandomState(2)
    for q in (1, 63, 64, 65, 5000):
        lb = rng.randint(0, n, q)
        ub = np.minimum(n, lb + rng.choice([0, 0, 1, 2, 70, 1500], q, p=[.3, .3, .2, .1, .09, .01]))
        out += [(lb, ub, 0, None), (lb, ub, 3, None)]
    # many short intervals per tile, and more patterns than a workgroup holds at a time between two outputs
    out.append((np.arange(n - 1), np.arange(n - 1) + 1, 0, None))
    out.append(([1] + [2] * 3000 + [4], [2] + [2] * 3000 + [5], 0, None))
    return out


@pytest.mark.parametrize("bits", [32, 64])
def test_hand_made_batches(ctx, bits):
    SA = np.arange(HAND_N, dtype=np.uint64)[::-1].copy()
    o = Occ(ctx, SA, HAND_N, HAND_OFF, bits)
    try:
        for lb, ub, limit, by_hand in hand_made_batches():
            total = o.check(lb, ub, limit)
            assert by_hand is None or total == by_hand
    finally:
        o.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_capacity_size_query_and_arguments(ctx, bits):
    import psac_amd
    text, off, SA = M.arrays("edge4097")
    n = int(text.size)
    pats, lb, ub = M.expected("edge4097")
    o = Occ(ctx, SA, n, off, bits)
    try:
        want = M.occurrences(o.sa, n, lb, ub)
        total = int(want[0][-1])
        assert o.run(lb, ub, cap=total)[0] == total and np.array_equal(o.pos[:total].astype(np.uint64), want[1])
        with pytest.raises(psac_amd.PsacxError) as e:
            o.run(lb, ub, cap=total - 1)
        assert e.value.code == -2                                                        # PSACX_ERANGE: start is valid, pos keeps its fill
        assert np.array_equal(o.start, want[0]) and np.all(o.pos == FILL) and np.all(o.sid == FILL)
        assert o.run(lb, ub, query=True)[0] == total and np.array_equal(o.start, want[0]) and np.all(o.pos == FILL)
        assert o.run(lb, ub, limit=2, query=True)[0] == int(np.minimum(ub - lb, 2).sum())
        with pytest.raises(psac_amd.PsacxError) as e:
            o.run(lb, ub, offsets=False)                                                 # d_sid without d_offsets
        assert e.value.code == -1 and np.all(o.pos == FILL)
        assert o.run(lb, ub, sid=False, offsets=False)[0] == total and np.all(o.sid == FILL) and np.array_equal(o.pos[:total].astype(np.uint64), want[1])
        assert psac_amd.occurrences_device(ctx, o.d_sa, n, None, 0, None, None, 0, 0, None, None, None, 0, bits) == 0          # q == 0
    finally:
        o.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_one_text_and_entries_beyond_n(ctx, bits):
    import psac_amd
    import locate_model as L
    name = "edge4097"
    text, SA = L.text_of(name), L.sa_of(name)
    pats, lb, ub = L.expected(name)
    o = Occ(ctx, SA, text.size, None, bits)
    try:
        o.check(lb, ub)
        o.check(lb, ub, 5)
    finally:
        o.close()
    dt = np.uint32 if bits == 32 else np.uint64
    start, pos = psac_amd.occurrences(SA.astype(dt), lb, ub, limit=4, ctx=ctx)
    want = M.occurrences(SA, text.size, lb, ub, 4)
    assert pos.dtype == dt and np.array_equal(start, want[0]) and np.array_equal(pos.astype(np.uint64), want[1])
    # SA entries >= n pass through, and their string is m
    text, off, SA = M.arrays("word_edges")
    n, ones = int(text.size), (1 << bits) - 1
    beyond = SA.copy()
    beyond[[0, 31, 32, n - 1]] = [n, n + 7, ones, ones - 1]
    o = Occ(ctx, beyond, n, off, bits)
    try:
        total = o.check([0, 30, 0], [n, 34, 1])
        assert (o.sid[:total] == len(off) - 1).sum() == 4 + 2 + 1
    finally:
        o.close()
    start, pos, sid = psac_amd.occurrences(SA.astype(dt), [0, 5], [n, 9], offsets=off, ctx=ctx)
    assert start.tolist() == [0, n, n + 4] and np.array_equal(pos[:n].astype(np.uint64), SA) and np.array_equal(sid.astype(np.uint64), M.string_ids(off, pos, n))
