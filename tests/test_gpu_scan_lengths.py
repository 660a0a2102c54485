"""The exclusive scan of scan.hpp past its first 256 blocks, both index widths.

exclusive_scan_dev scans blocks of 4096 entries and then the block sums, by one workgroup in chunks of 256 with a carry from chunk
to chunk (scan_top_kernel): the second chunk begins beyond 2^20 entries.  Every scan of the other test files ends inside the first
chunk, while a lookup table for DNA with k = 10 has ten.  Two callers reach it with lengths a test can choose:

  - psacx_occurrences_dev_* with d_pos = NULL is the scan of arbitrary counts: lb = 0, ub = count <= n gives start[0 .. q] and the
    total.  Entry counts q + 1 = 2^20 - 1, 2^20, 2^20 + 1 (the last full chunk and a block of one entry in the second),
    2^20 + 4096, 2^20 + 4097 (one block into the second chunk, and an entry more) and 2^21 + 1 (the third chunk), over counts of all
    ones, all zero but the last, all zero but the first, random in 0 .. 3 with a few of n = 4097, and all n, whose total passes
    2^32.  The model is numpy.cumsum in uint64, held here to the plain loop of locate_gsa_model.occurrences on the hand-made batches
    of tests/test_gpu_occurrences.py.  One case produces lists: 2^20 + 4097 intervals, a few thousand outputs, PAD behind them.
  - psacx_lookup_table_dev_* / _gsa_dev_* over 12 300 characters of DNA and the same text cut into strings: k = 9, 1 953 126 entries,
    two chunks, and k = 10, 9 765 626 entries, ten chunks, in both table widths, against table_by_definition of the two models
    (numpy.bincount over the keys of the definition, then cumsum: the model the tables of k = 1, 2 are held to everywhere else, and
    here once more).  Locate and match with the table of k = 9 give the intervals of the run without a table, which are the model's."""
import numpy as np
import pytest

import locate_gsa_model as G
import locate_model as L
import match_model as M
from match_gpu_common import first_difference
from test_gpu_grid_trips import SET, TEXT, index_of

pytestmark = pytest.mark.gpu

N = 4097
FILL, PAD = 0x6B, 3
CHUNK = 256 * 4096                                  # entries of the scan whose block sums fill one chunk of scan_top_kernel
LENGTHS = [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 4096, CHUNK + 4097, 2 * CHUNK + 1]
PATTERNS = ["ones", "last", "first", "random", "all_n"]


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def scan_model(lb, ub, n, limit=0):
    """start[0 .. q] of psacx_occurrences_dev_*: the exclusive sums of the counts, in uint64"""
    lb, ub = np.asarray(lb).astype(np.uint64), np.asarray(ub).astype(np.uint64)
    c = np.where((lb <= ub) & (ub <= np.uint64(n)), ub - lb, np.uint64(0)).astype(np.uint64)
    if limit:
        c = np.minimum(c, np.uint64(limit))
    start = np.zeros(c.size + 1, np.uint64)
    np.cumsum(c, dtype=np.uint64, out=start[1:])
    return start


def counts_of(pattern, q, seed):
    c = np.zeros(q, np.uint64)
    if pattern == "ones":
        c[:] = 1
    elif pattern == "last":
        c[-1] = 5
    elif pattern == "first":
        c[0] = 5
    elif pattern == "random":
        rng = np.random.RandomState(seed)
        c[:] = rng.randint(0, 4, q)
        c[rng.randint(0, q, 7)] = N
        c[[0, q - 1, q // 2]] = N
    else:
        c[:] = N
    return c


class Scan(object):
    """SA of a^4097 and room for the largest batch in device memory; run() is one call of psacx_occurrences_dev_*."""

    def __init__(self, ctx, bits, room):
        self.ctx, self.bits, self.dt = ctx, bits, (np.uint32 if bits == 32 else np.uint64)
        self.sa = np.arange(N, dtype=self.dt)[::-1].copy()
        w = bits // 8
        self.d_sa, self.d_lb, self.d_ub, self.d_start = ctx.alloc(N * w), ctx.alloc(room * w), ctx.alloc(room * w), ctx.alloc((room + 1 + PAD) * 8)
        self.held = [self.d_sa, self.d_lb, self.d_ub, self.d_start]
        ctx.h2d(self.d_sa, self.sa)

    def run(self, lb, ub, d_pos=None, cap=0):
        """(total, start as the device left it); start has PAD entries of room behind entry q, which must keep their fill"""
        import psac_amd
        lb, ub = np.ascontiguousarray(lb, dtype=self.dt), np.ascontiguousarray(ub, dtype=self.dt)
        q = int(lb.size)
        self.ctx.h2d(self.d_lb, lb); self.ctx.h2d(self.d_ub, ub)
        self.ctx.h2d(self.d_start, np.full(q + 1 + PAD, FILL, np.uint64))
        total = psac_amd.occurrences_device(self.ctx, self.d_sa, N, None, 0, self.d_lb, self.d_ub, q, 0, self.d_start, d_pos, None, cap, self.bits)
        start = np.empty(q + 1 + PAD, np.uint64)
        self.ctx.d2h(start, self.d_start)
        assert np.all(start[q + 1:] == FILL)
        back = np.empty(q, self.dt)
        self.ctx.d2h(back, self.d_ub)
        assert np.array_equal(back, ub)                                      # no input is written
        return total, start[:q + 1]

    def close(self):
        for p in self.held:
            self.ctx.free(p)


def test_the_cumsum_model_is_the_plain_loop():
    # (on the host) scan_model against locate_gsa_model.occurrences on the hand-made batches, inverted and overlong intervals and
    # limits included: it is no second definition
    from test_gpu_occurrences import HAND_N, hand_made_batches
    sa = np.arange(HAND_N, dtype=np.uint64)[::-1]
    for lb, ub, limit, by_hand in hand_made_batches():
        want = G.occurrences(sa, HAND_N, lb, ub, limit)[0]
        got = scan_model(lb, ub, HAND_N, limit)
        assert got.dtype == np.uint64 and np.array_equal(got, want)
        assert by_hand is None or int(got[-1]) == by_hand


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_scans_past_the_first_chunk_of_block_sums(ctx, pattern, bits):
    s = Scan(ctx, bits, max(LENGTHS))
    try:
        # the device scan and the model on a small hand-made batch first, then the six lengths
        total, start = s.run([7, 0, 5, N - 3, N], [6, N + 1, 9, N, N])
        assert np.array_equal(start, scan_model([7, 0, 5, N - 3, N], [6, N + 1, 9, N, N], N)) and total == int(start[-1])
        for entries in LENGTHS:
            q = entries - 1
            ub = counts_of(pattern, q, entries % 1000)
            lb = np.zeros(q, np.uint64)
            want = scan_model(lb, ub, N)
            total, start = s.run(lb, ub)                                     # the size query
            bad = np.nonzero(start != want)[0]
            assert bad.size == 0, (entries, int(bad[0]), int(start[bad[0]]), int(want[bad[0]]), int(bad.size))
            assert total == int(want[-1]) == int(ub.sum(dtype=np.uint64))
            if pattern == "all_n":
                assert total > 1 << 32
    finally:
        s.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_lists_behind_a_scan_of_two_chunks(ctx, bits):
    # 2^20 + 4097 intervals, most of them empty, 3000 of 1 .. 3 ranks spread over both chunks: pos against SA, PAD behind it
    q = CHUNK + 4097
    rng = np.random.RandomState(19)
    at = np.unique(np.concatenate([rng.randint(0, q, 3000), [0, CHUNK - 1, CHUNK, CHUNK + 4095, CHUNK + 4096, q - 1]]))
    lb = rng.randint(0, N - 3, q).astype(np.uint64)
    ub = lb.copy()
    ub[at] += rng.randint(1, 4, at.size).astype(np.uint64)
    want = scan_model(lb, ub, N)
    total_want = int(want[-1])
    assert 3000 < total_want < 10000
    s = Scan(ctx, bits, q)
    try:
        d_pos = ctx.alloc((total_want + PAD) * (bits // 8))
        s.held.append(d_pos)
        ctx.h2d(d_pos, np.full(total_want + PAD, FILL, s.dt))
        total, start = s.run(lb, ub, d_pos, total_want)
        assert total == total_want and np.array_equal(start, want)
        pos = np.empty(total_want + PAD, s.dt)
        ctx.d2h(pos, d_pos)
        want_pos = np.concatenate([s.sa[int(lb[j]):int(ub[j])] for j in at])
        assert np.array_equal(pos[:total], want_pos) and np.all(pos[total:] == FILL)
        # ... which is what the plain loop gives for the intervals that are not empty
        plain = G.occurrences(s.sa, N, lb[at], ub[at])
        assert np.array_equal(plain[1], want_pos.astype(np.uint64)) and np.array_equal(plain[0], want[np.append(at, q)] - want[at[0]])
    finally:
        s.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["text", "set"])
def test_lookup_tables_of_two_and_ten_chunks(ctx, kind, bits):
    d = index_of(ctx, kind, bits)
    try:
        model = (lambda k: G.table_by_definition(d.text, d.off, k)) if d.set else (lambda k: L.table_by_definition(d.text, k))
        for k, entries in ((1, 6), (2, 26), (9, 1953126), (10, 9765626)):
            table, built = d.table(k)
            want = model(k)
            assert built.size == entries == want.size and (entries > CHUNK) == (k >= 9)
            bad = np.nonzero(built.astype(np.int64) != want)[0]
            assert bad.size == 0, (k, int(bad[0]), int(built[bad[0]]), int(want[bad[0]]), int(bad.size))
            assert int(built[-1]) == d.n
            if k != 9:
                continue
            # locate and match through the table of two chunks: the intervals of the run without a table, which are the model's
            pats, lb, ub = G.expected(SET) if d.set else L.expected(TEXT)
            b = d.batch(pats)
            plain, through = d.locate(b), d.locate(b, table)
            assert np.array_equal(plain[0], lb) and np.array_equal(plain[1], ub)
            assert first_difference((through[0], through[0], through[1]), (lb, lb, ub), pats) is None
            want_match = (M.expected_gsa(SET) if d.set else M.expected(TEXT))[1:]
            assert first_difference(d.match(b), want_match, pats) is None
            assert first_difference(d.match(b, table), want_match, pats) is None
        assert d.inputs_unchanged()
    finally:
        d.close()
