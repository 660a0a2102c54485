"""psacx_rmq_index_dev_* / psacx_rmq_dev_* against the host model (tests/rmq_model.py), both index widths: every sub-range of
small arrays on both sides of a group of 64; arrays of two and three index levels whose last group is partial, full and one over,
with range ends around every kind of group boundary and 20 000 random ranges, over value families with many equal minima, with
all ones, and with 64-bit values that differ in one half only; empty and over-long ranges; outputs left out; the size query; an
index of random words; batch sizes around a wave and 2^20 ranges.  Every call's outputs are pre-filled with a sentinel, the
ranges of an array are uploaded once, and the inputs are compared with what was uploaded after the calls
(tests/rmq_gpu_common.py)."""
import numpy as np
import pytest

import rmq_model as R
from rmq_gpu_common import SENTINEL, Dev, Indexed, Ranges, first_bad

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def families(n, bits, seed=1):
    """name -> values: 0/1 in long runs and three small values (many equal minima), ascending, descending, constant, all ones
    everywhere and everywhere but one entry; for 64 bits, values that differ only in the high half and only in the low half."""
    dt = np.uint32 if bits == 32 else np.uint64
    top = R.ones(dt)
    rng = np.random.RandomState(seed + n % 1000)
    runs = np.repeat(rng.randint(0, 2, n // 2 + 2), rng.randint(1, 300, n // 2 + 2))[:n]
    one_low = np.full(n, top, dt)
    if n:
        one_low[(2 * n) // 3] = top - 1
    out = {
        "runs01": runs.astype(dt),
        "three": rng.randint(0, 3, n).astype(dt),
        "ascending": np.arange(n).astype(dt),
        "descending": (n - 1 - np.arange(n)).astype(dt),
        "constant": np.full(n, 7, dt),
        "all_ones": np.full(n, top, dt),
        "ones_but_one": one_low,
    }
    if bits == 64:
        out["high_half"] = rng.randint(1, 5, n).astype(np.uint64) << np.uint64(32)
        out["low_half"] = (np.uint64(9) << np.uint64(40)) | rng.randint(0, 1 << 32, n, dtype=np.int64).astype(np.uint64)
    return out


def check(dev, values, r, want=None, **kw):
    """one array, its index, one call over the ranges r; the model's answers (computed here unless handed in)"""
    a = Indexed(dev, values)
    got = a.rmq(r, **kw)
    want = R.Table(a.v).queries(r.lo, r.hi) if want is None else want
    assert first_bad(got[0], want[0]) is None, ("min", first_bad(got[0], want[0]))
    bad = first_bad(got[1], want[1])
    assert bad is None, ("arg", bad, int(r.lo[bad[0]]), int(r.hi[bad[0]]))
    assert a.unchanged()
    return a


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 130])
def test_every_subrange_of_small_arrays(ctx, n, bits):
    dev = Dev(ctx, bits)
    try:
        lo, hi = np.nonzero(np.triu(np.ones((n + 1, n + 1), bool), 1))           # all 0 <= lo < hi <= n
        r = Ranges(dev, lo, hi)
        assert r.q == n * (n + 1) // 2
        for name, v in families(n, bits).items():
            check(dev, v, r)
        assert r.unchanged(dev)
    finally:
        dev.close()


def edge_ends(n):
    """0, n, and -2 .. +2 around multiples of 64, 4096 and 262144: the first two, one in the middle and the last two of each"""
    ends = {0, n}
    for g in (64, 4096, 262144):
        k = n // g
        for t in sorted(set(x for x in (1, 2, k // 2 + 1, k - 1, k, k + 1) if x >= 1)):
            ends.update(t * g + d for d in (-2, -1, 0, 1, 2))
    return sorted(e for e in ends if 0 <= e <= n + 2)


def big_ranges(n, seed=5):
    e = np.array(edge_ends(n), np.int64)
    lo, hi = [x.reshape(-1) for x in np.meshgrid(e, e, indexing="ij")]             # all combinations, the empty and inverted ones too
    rng = np.random.RandomState(seed)
    rl = rng.randint(0, n, 20000)
    length = np.where(rng.randint(0, 2, 20000) == 0, rng.randint(1, 200, 20000), rng.randint(1, n + 1, 20000))
    return np.concatenate([lo, rl]), np.concatenate([hi, rl + length])


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [4095, 4096, 4097, 262143, 262144, 262145])
def test_group_boundaries_and_random_ranges(ctx, n, bits):
    dev = Dev(ctx, bits)
    try:
        lo, hi = big_ranges(n)
        assert (hi > n).any() and (lo >= hi).any() and ((hi - lo > n // 2) & (hi <= n)).any()
        r = Ranges(dev, lo, hi)
        for name, v in families(n, bits).items():
            a = check(dev, v, r)
            assert a.entries >= 3 * ((n + 63) // 64)
        assert r.unchanged(dev)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_empty_and_over_long_ranges_get_the_pinned_answers(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        n = 130
        v = families(n, bits)["three"]
        top = R.ones(dev.dt)
        #             lo == hi      lo > hi     hi > n            lo >= n                   both beyond
        lo = np.array([0, 64, 130,  5, 129, 130,  0, 100, 129,     130, 131, top,            top - 1, 200], dtype=dev.dt)
        hi = np.array([0, 64, 130,  4, 3, 0,      131, 4000, top,  130, 140, top,            top, 100], dtype=dev.dt)
        r = Ranges(dev, lo, hi)
        a = Indexed(dev, v)
        mn, arg = a.rmq(r)
        empty = np.array([1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1], bool)
        assert np.all(mn[empty] == top) and np.all(arg[empty] == n)
        for j in np.nonzero(~empty)[0]:
            s = v[int(lo[j]):n]
            assert int(mn[j]) == int(s.min()) and int(arg[j]) == int(lo[j]) + int(np.argmin(s))
        assert a.unchanged() and r.unchanged(dev)
        # n == 0: every range is empty, and nothing is read
        z = Indexed(dev, np.zeros(0, dev.dt))
        mn, arg = z.rmq(Ranges(dev, [0, 0, 5], [0, 9, 2]))
        assert np.all(mn == top) and np.all(arg == 0)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_outputs_left_out(ctx, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        n = 4097
        v = families(n, bits)["runs01"]
        lo, hi = big_ranges(n)
        r = Ranges(dev, lo[:3000], hi[:3000])
        want = R.Table(v).queries(r.lo, r.hi)
        a = Indexed(dev, v)
        mn, arg = a.rmq(r, want_arg=False)
        assert first_bad(mn, want[0]) is None and np.all(arg == SENTINEL)
        mn, arg = a.rmq(r, want_min=False)
        assert first_bad(arg, want[1]) is None and np.all(mn == SENTINEL)
        with pytest.raises(psac_amd.PsacxError) as e:
            a.rmq(r, want_min=False, want_arg=False)
        assert e.value.code == -1                                                     # PSACX_EINVAL
        assert np.all(a.raw[0] == SENTINEL) and np.all(a.raw[1] == SENTINEL)
        assert a.unchanged() and r.unchanged(dev)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_size_query(ctx, bits):
    import psac_amd
    for n in (0, 1, 64, 65, 262145):
        entries = psac_amd.rmq_index_device(ctx, None, n, None, bits)
        assert 1 <= entries <= n // 16 + 4096, (n, entries)
    if bits == 32:
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.rmq_index_device(ctx, None, 1 << 32, None, bits)
        assert e.value.code == -2                                                     # PSACX_ERANGE


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [130, 4097, 262145])
def test_an_index_of_random_words_sends_nothing_out_of_range(ctx, n, bits):
    dev = Dev(ctx, bits)
    try:
        rng = np.random.RandomState(n)
        v = families(n, bits)["three"]
        lo, hi = big_ranges(n) if n > 130 else (rng.randint(0, n + 2, 3000), rng.randint(0, n + 3, 3000))
        r = Ranges(dev, lo, hi)
        for words in (rng.randint(0, 1 << 32, n // 16 + 4096, dtype=np.int64), rng.randint(0, 4, n // 16 + 4096), np.zeros(n // 16 + 4096, np.int64)):
            a = Indexed(dev, v, index=words.astype(dev.dt))
            mn, arg = a.rmq(r)                                                        # returns PSACX_OK
            arg = arg.astype(np.uint64)
            inside = (arg >= r.lo.astype(np.uint64)) & (arg < np.minimum(r.hi.astype(np.uint64), np.uint64(n)))
            assert np.all(inside | (arg == np.uint64(n)))
            assert a.unchanged()
        check(dev, v, r)                                                              # a correct call afterwards is right
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_batch_sizes(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        n = 262145
        v = families(n, bits)["runs01"]
        rng = np.random.RandomState(21)
        q = 1 << 20
        lo = rng.randint(0, n, q)
        length = np.where(rng.randint(0, 2, q) == 0, rng.randint(1, 200, q), rng.randint(1, n + 1, q))
        r = Ranges(dev, lo, lo + length)
        want = R.Table(v).queries(r.lo, r.hi)
        a = Indexed(dev, v)
        for size in (0, 1, 63, 64, 65, q):
            mn, arg = a.rmq(r, q=size)
            assert mn.size == size and first_bad(mn, want[0][:size]) is None and first_bad(arg, want[1][:size]) is None, size
        assert a.unchanged() and r.unchanged(dev)
    finally:
        dev.close()
