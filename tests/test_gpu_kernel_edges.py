"""The three building blocks that include/psacx.h offers on their own, at the key widths and in the forms the whole constructions
reach only in passing: the rank-pair sort (look-back, three-kernel, narrow-payload and two-word forms, every digit up to bit 63,
skipped passes between executed ones, no pass at all), ANSV on values up to 2^bits - 1 -- which is also what the kernels pad with --
and on 64-bit values that differ in one half only, and the host-pointer construction whose SA and LCP leave the device early while
the reduced-memory layout has the output arrays double as scratch.  Host references: np.lexsort (stable) for the sort, the oracle's
ANSV (pinned against the definition on the same value shapes in tests/test_oracle_golden.py), and for the host path the arrays of the
device-pointer path plus psacx_check_dev_*.  Everything goes through the C ABI.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

SMALL_SORT_MAX = 1 << 21                 # engine.hpp: below, the single-sweep look-back form; from here on three kernels per pass
SORT_TILE = {32: 6144, 64: 4096}         # engine.hpp: ScatterCfg<T>::TILE


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _vp(p):
    return C.c_void_p(p)


# ---------------------------------------------------------------------------------------------------------------------------------
# A. rank-pair sort
# ---------------------------------------------------------------------------------------------------------------------------------

def _small_sizes(bits):
    t = SORT_TILE[bits]
    return [1, 2, t - 1, t, t + 1]


def _large_sizes(bits):                   # the same key set on both sides of SMALL_SORT_MAX
    return [SMALL_SORT_MAX - 1, SMALL_SORT_MAX, SMALL_SORT_MAX + SORT_TILE[bits] + 1]


def _uniform(n, bits, seed):
    return (inputs.splitmix64_stream(n, seed) >> np.uint64(64 - bits)).astype(_dt(bits))


def _below(n, bits, seed, bound):
    return (inputs.splitmix64_stream(n, seed) % np.uint64(bound)).astype(_dt(bits))


def _mask(a, key_bits):
    width = a.dtype.itemsize * 8
    if key_bits == 0 or key_bits >= width:
        return a
    return a & a.dtype.type((1 << key_bits) - 1)


def _gap(n, bits, seed):                  # two digits with constant ones between them
    sh = np.uint64(40 if bits == 64 else 24)
    return ((_below(n, 64, seed, 256) << sh) | _below(n, 64, seed + 1, 256)).astype(_dt(bits))


def _keys(dist, n, bits, seed):
    """(b1, b2, key_bits) of a named key set."""
    dt = _dt(bits)
    const = dt(0x5A5A5A5A5A5A5A5A >> (64 - bits))
    if dist == "uniform":
        return _uniform(n, bits, seed), _uniform(n, bits, seed + 1), 0
    if dist.startswith("bits"):
        kb = int(dist[4:])
        return _mask(_uniform(n, bits, seed), kb), _mask(_uniform(n, bits, seed + 1), kb), kb
    if dist == "clamp":                   # more significant bits than the word has: all of them
        return _uniform(n, bits, seed), _uniform(n, bits, seed + 1), bits + 8
    if dist == "gap":
        return _gap(n, bits, seed), _gap(n, bits, seed + 2), 0
    if dist == "equal":
        return np.full(n, const, dt), np.full(n, const >> dt(3), dt), 0
    if dist == "b1_const":
        return np.full(n, const, dt), _uniform(n, bits, seed), 0
    if dist == "b1_const_one_digit":      # one executed pass: first and last at once
        return np.full(n, const, dt), _below(n, bits, seed, 256), 0
    if dist == "b2_const":
        return _uniform(n, bits, seed), np.full(n, const, dt), 0
    if dist == "ties":
        return _below(n, bits, seed, 4), _below(n, bits, seed + 1, 4), 0
    if dist == "hot":                     # all but about 1 in 1000 records share every digit of b1
        b1 = np.full(n, const, dt)
        other = inputs.splitmix64_stream(n, seed + 2) % np.uint64(1000) == 0
        b1[other] = _uniform(n, bits, seed)[other]
        return b1, _uniform(n, bits, seed + 1), 0
    if dist in ("sorted", "reverse"):
        b1, b2 = _below(n, bits, seed, 1 << 20) << dt(bits - 20), _uniform(n, bits, seed + 1)
        o = np.lexsort((b2, b1))
        if dist == "reverse":
            o = o[::-1]
        return np.ascontiguousarray(b1[o]), np.ascontiguousarray(b2[o]), 0
    raise ValueError(dist)


def _planned_passes(b1, b2, key_bits):
    """(executed, skipped): the plan holds ceil(bits / 8) digits per word (radix.hpp: make_plan); a digit on which all keys agree is skipped."""
    width = b1.dtype.itemsize * 8
    kb = width if key_bits == 0 or key_bits > width else key_bits
    per = (kb + 7) // 8
    executed = 0
    for w in (b1, b2):
        for i in range(per):
            d = (w >> w.dtype.type(8 * i)) & w.dtype.type(255)
            executed += int(d.min() != d.max())
    return executed, 2 * per - executed


def _order(b1, b2):
    """The stable order by (b1, b2): ties keep index order."""
    return np.lexsort((b2, b1))


def _launches(ctx):
    return [int(x) for x in ctx.stats().scatter_launches]


def _sort_standalone(ctx, b1, b2, key_bits):
    """psacx_pair_sort_dev_*: returns (b1, b2, idx) as the call left them and the statistics of the call."""
    bits, n = b1.dtype.itemsize * 8, b1.size
    d = [ctx.alloc(b1.nbytes) for _ in range(3)]
    try:
        ctx.h2d(d[0], b1); ctx.h2d(d[1], b2)
        fn = getattr(ctx._lib, "psacx_pair_sort_dev_u%d" % bits)
        ctx.check(fn(ctx.handle, _vp(d[0]), _vp(d[1]), _vp(d[2]), n, key_bits))
        stats = ctx.stats()
        out = [np.empty(n, b1.dtype) for _ in range(3)]
        for a, p in zip(out, d):
            ctx.d2h(a, p)
    finally:
        for p in d:
            ctx.free(p)
    return out[0], out[1], out[2], stats


def _sort_op(ctx, k1, k2, v, bits1, bits2):
    """psacx_op_pair_sort_*: explicit payload; k2 None = two-word records.  Returns the record arrays `where` names and the scatter
    kernels the call launched, per form."""
    bits, n = k1.dtype.itemsize * 8, k1.size
    names = ("k1", "k2", "v", "a1", "a2", "av")
    d = dict((nm, None if (k2 is None and nm in ("k2", "a2")) else ctx.alloc(k1.nbytes)) for nm in names)
    try:
        ctx.h2d(d["k1"], k1); ctx.h2d(d["v"], v)
        if k2 is not None:
            ctx.h2d(d["k2"], k2)
        before = _launches(ctx)
        where = C.c_int32(-1)
        fn = getattr(ctx._lib, "psacx_op_pair_sort_u%d" % bits)
        ctx.check(fn(ctx.handle, *([_vp(d[nm]) for nm in names] + [n, bits1, bits2, C.byref(where)])))
        launched = [a - b for a, b in zip(_launches(ctx), before)]
        assert where.value in (0, 1)
        out = []
        for nm in (("a1", "a2", "av") if where.value else ("k1", "k2", "v")):
            if d[nm] is None:
                out.append(None)
                continue
            a = np.empty(n, k1.dtype)
            ctx.d2h(a, d[nm])
            out.append(a)
    finally:
        for p in d.values():
            if p is not None:
                ctx.free(p)
    return out[0], out[1], out[2], launched


def _payload(n, bits, seed):
    """n distinct values that are not the index: a payload permuted wrongly cannot hide."""
    if bits == 64:
        return inputs.splitmix64_stream(n, seed)                                   # (a bijection of distinct states)
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed)).astype(np.uint32)      # (odd multiplier mod 2^32)


# key set -> sizes beyond the five around a tile (the >= 2^21 sizes only where the set needs them)
def _sort_cases(bits):
    L = _large_sizes(bits)
    cases = [("uniform", L), ("gap", L[:2]), ("equal", [L[1]]), ("b1_const", [L[1]]), ("b1_const_one_digit", [L[1]]), ("b2_const", [L[1]]),
             ("ties", L[:2]), ("hot", L[:2]), ("sorted", [L[1]]), ("reverse", [L[1]]), ("clamp", [])]
    for kb in (1, 7, 8, 9, 31, 32) + ((33, 63, 64) if bits == 64 else ()):
        cases.append(("bits%d" % kb, [L[1]] if kb in (1, bits - 1) else []))
    return cases


SORT_PARAMS = [(bits, dist, extra) for bits in (32, 64) for dist, extra in _sort_cases(bits)]


@pytest.mark.parametrize("bits,dist,extra", SORT_PARAMS, ids=["u%d-%s" % (b, d) for b, d, _ in SORT_PARAMS])
def test_pair_sort_key_sets(ctx, bits, dist, extra):
    # idxsort.hpp:23-83.  The stand-alone call makes up its payload (the index): below 2^21 records the look-back form, from there on
    # three kernels per pass, at 64 bits with the payload as 32-bit entries that the last pass widens (vn 1 / 2; vn 0 when one pass is
    # first and last).  The step op carries a payload of its own in full words.
    dt = _dt(bits)
    counts = {}
    for n in _small_sizes(bits) + list(extra):
        b1, b2, kb = _keys(dist, n, bits, 1000 + n % 997)
        order = _order(b1, b2)
        want1, want2 = b1[order], b2[order]
        o1, o2, oi, st = _sort_standalone(ctx, b1, b2, kb)
        assert np.array_equal(oi, order.astype(dt)), (dist, n, "idx")
        assert np.array_equal(o1, want1) and np.array_equal(o2, want2), (dist, n, "keys")
        executed, skipped = _planned_passes(b1, b2, kb)
        got = (int(st.rounds[0].sort_passes), int(st.rounds[0].sort_passes_skipped))
        launched = [int(x) for x in st.scatter_launches]
        print("pair_sort u%d %-18s n=%-8d key_bits=%-2d passes=%d skipped=%d scatter_launches=%s" % (bits, dist, n, kb, got[0], got[1], launched))
        assert got == (executed, skipped), (dist, n, got, (executed, skipped))
        # every executed pass is one scatter kernel of the form the size calls for
        assert launched == ([0, executed, 0] if n >= SMALL_SORT_MAX else [executed, 0, 0]), (dist, n, launched)
        counts[n] = got
        # the step op on the same keys
        v = _payload(n, bits, n)
        p1, p2, pv, launched = _sort_op(ctx, b1, b2, v, kb if kb else bits, kb if kb else bits)
        assert np.array_equal(pv, v[order]), (dist, n, "op payload")
        assert np.array_equal(p1, want1) and np.array_equal(p2, want2), (dist, n, "op keys")
        if n >= 2:
            assert launched == ([0, executed, 0] if n >= SMALL_SORT_MAX else [executed, 0, 0]), (dist, n, launched)
    if SMALL_SORT_MAX - 1 in counts and SMALL_SORT_MAX in counts:
        # the look-back form finds a constant digit in its histogram (one bin holds all n), the three-kernel form in the OR / AND
        # summary of the keys: the same verdict on the same key set
        assert counts[SMALL_SORT_MAX - 1] == counts[SMALL_SORT_MAX]


@pytest.mark.parametrize("bits", [32, 64])
def test_pair_sort_two_word_records(ctx, bits):
    # k2 = NULL / bits2 = 0 (dist_ops.hpp: op_pair_sort): records (k1, v), which exist in the three-kernel form only, at every size
    for dist in ("uniform", "gap", "equal"):
        for n in _small_sizes(bits) + (_large_sizes(bits) if dist == "uniform" else []):
            k1 = _keys(dist, n, bits, 77 + n % 997)[0]
            v = _payload(n, bits, 5)
            order = np.argsort(k1, kind="stable")
            p1, p2, pv, launched = _sort_op(ctx, k1, None, v, bits, 0)
            assert p2 is None
            assert np.array_equal(pv, v[order]) and np.array_equal(p1, k1[order]), (dist, n)
            executed = _planned_passes(k1, k1, 0)[0] // 2
            print("pair_sort u%d two-word %-8s n=%-8d scatter_launches=%s" % (bits, dist, n, launched))
            if n >= 2:
                assert launched == [0, 0, executed], (dist, n, launched)


# ---------------------------------------------------------------------------------------------------------------------------------
# B. ANSV
# ---------------------------------------------------------------------------------------------------------------------------------

ANSV_SMALL = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4097)          # a run is 16 elements, a tile 1024, pyramid levels 64, 4096, 2^18
ANSV_LARGE = (65537, (1 << 18) + 1, (1 << 20) + 777)
ALL_PAIRS = tuple((lt, rt) for lt in (0, 1, 2) for rt in (0, 1, 2))
FEW_PAIRS = ((0, 0), (2, 0), (1, 2))
NO1, NO2 = 2**64 - 1, 2**64 - 2          # NO2 is a word the kernel reserves for itself (ansv_tile.hpp: ANSV_NOCONT)


def _ansv_three_ways(ctx, v, lt, rt, nonsv):
    """(left, right) from the host-pointer call, the device-pointer call, and the device-pointer call on input that starts one element
    past a 16-byte boundary."""
    import psac_amd
    n, w = v.size, v.dtype.itemsize
    res = [psac_amd.ansv(v, lt, rt, nonsv=nonsv, ctx=ctx)]
    d_in, d_l, d_r = ctx.alloc((n + 4) * w), ctx.alloc(n * 8), ctx.alloc(n * 8)
    try:
        for off in (0, w):
            ctx.h2d(d_in + off, v)
            fill = np.full(n, 0x1234567812345678, np.uint64)          # (neither nonsv nor an index: every entry has to be written)
            ctx.h2d(d_l, fill); ctx.h2d(d_r, fill)
            psac_amd.ansv_device(ctx, d_in + off, n, d_l, d_r, w * 8, lt, rt, nonsv)
            L, R = np.empty(n, np.uint64), np.empty(n, np.uint64)
            ctx.d2h(L, d_l); ctx.d2h(R, d_r)
            res.append((L, R))
    finally:
        for p in (d_in, d_l, d_r):
            ctx.free(p)
    return res


def _ansv_check(ctx, v, pairs, nonsvs, tag):
    want = {}
    for nonsv in nonsvs:
        for lt, rt in pairs:
            for key in ((True, lt, nonsv), (False, rt, nonsv)):
                if key not in want:
                    want[key] = O.ansv(v, *key)
            for how, (L, R) in zip(("host", "device", "device+1"), _ansv_three_ways(ctx, v, lt, rt, nonsv)):
                assert np.array_equal(L, want[(True, lt, nonsv)]), tag + (v.size, lt, rt, nonsv, how, "left")
                assert np.array_equal(R, want[(False, rt, nonsv)]), tag + (v.size, lt, rt, nonsv, how, "right")


ANSV_PARAMS = [(dt, s) for dt in (np.uint32, np.uint64) for s in inputs.ANSV_EDGE_SHAPES + (inputs.ANSV_EDGE_SHAPES_64 if dt == np.uint64 else ())]


@pytest.mark.parametrize("dtype,shape", ANSV_PARAMS, ids=["%s-%s" % (np.dtype(d).name, s) for d, s in ANSV_PARAMS])
def test_ansv_full_value_range(ctx, dtype, shape):
    # ansv.hpp:2042-2051 over any integer array: values up to 2^bits - 1 = the kernels' padding (ansv_wave.hpp: answ_fetch, ansv_tile.hpp: the
    # window tables), 64-bit values whose halves travel apart between lanes, nonsv = a word the kernel uses inside.  What stands between the
    # padding and a wrong answer are the n_rel guards of a pass: with them in place the padding value itself cannot be seen from outside
    # (a build that pads with 0 answers the same), without the one of step 1 the values at the top of the range fail here.
    for n in ANSV_SMALL + ANSV_LARGE:
        v = inputs.ansv_edge_values(shape, n, dtype, seed=5)
        _ansv_check(ctx, v, ALL_PAIRS if n <= 4097 else FEW_PAIRS, (NO1, NO2), (np.dtype(dtype).name, shape))


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["uint32", "uint64"])
def test_ansv_nonsv_zero_and_n(ctx, dtype):
    # nonsv values that are also legal answers (index 0) or one past them
    for shape in ("uniform", "top3"):
        for n in (17, 1025, 65537):
            v = inputs.ansv_edge_values(shape, n, dtype, seed=9)
            _ansv_check(ctx, v, FEW_PAIRS, (0, n), (np.dtype(dtype).name, shape))


# ---------------------------------------------------------------------------------------------------------------------------------
# C. host-pointer construction: SA and LCP leave early (construct.hpp: EarlyOut) in the reduced-memory layout
# ---------------------------------------------------------------------------------------------------------------------------------
# An array leaves early from 8 * STAGE_CHUNK = 512 MiB on: the smallest such texts.  In the reduced layout the record arrays of the
# first round alias the output arrays, and the SA -> ISA inversion that runs while SA and LCP are on the wire is handed d_isa and a
# work array as scratch: it must touch neither d_sa nor d_lcp.

HOST_N = {64: (1 << 26) + 12345, 32: (1 << 27) + 1}
_host_cache = {}


def _host_text(case, bits):
    key = ("text", case, bits)
    if key not in _host_cache:
        t = inputs.dna(HOST_N[bits], 21)
        if case == "repeat":              # one repeat of 300 characters: refinement rounds follow the first round
            t[40000000:40000300] = t[1000:1300]
        _host_cache[key] = t
    return _host_cache[key]


def _device_reference(ctx, case, bits):
    """SA, ISA, LCP of the device-pointer path (same options), copied as they are, and the device checker's verdict on them."""
    import psac_amd
    key = ("ref", case, bits)
    if key not in _host_cache:
        text = _host_text(case, bits)
        n, w = text.size, bits // 8
        d_text = ctx.alloc(n)
        d = [ctx.alloc(n * w) for _ in range(3)]
        try:
            ctx.h2d(d_text, text)
            ds = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
            ds.construct_device(d_text, n, d[0], d[1], d[2])
            err = psac_amd.check_device(ctx, d_text, n, d[0], d[1], d[2], bits)
            arrs = [np.empty(n, _dt(bits)) for _ in range(3)]
            for a, p in zip(arrs, d):
                ctx.d2h(a, p)
        finally:
            for p in [d_text] + d:
                ctx.free(p)
        _host_cache[key] = (arrs, err)
    return _host_cache[key]


def _host_run(ctx, case, bits, lc=False):
    import psac_amd
    hs = psac_amd.SuffixArray(index_bits=bits, lcp=True, lc=lc, ctx=ctx)
    st = hs.construct(_host_text(case, bits))
    (sa, isa, lcp), err = _device_reference(ctx, case, bits)
    assert err == [0, 0, 0, 0]
    assert np.array_equal(hs.local_SA, sa), (case, bits, "SA")
    assert np.array_equal(hs.local_B, isa), (case, bits, "ISA")
    assert np.array_equal(hs.local_LCP, lcp), (case, bits, "LCP")
    print("host path %-6s u%d lc=%d rounds=%d ms_host[6]=%.1f" % (case, bits, lc, st.n_rounds, st.ms_host[6]))
    if (case, bits) != ("dna", 64):          # (only that text is used by more than one test)
        _host_cache.clear()
    return hs, st


@pytest.fixture
def diet(monkeypatch):
    monkeypatch.setenv("PSACX_FORCE_DIET", "1")            # (the wrappers' debug shim: psac_amd/_lib.py ENV_KNOBS)
    return monkeypatch


@pytest.fixture(scope="module", autouse=True)
def _drop_host_cache():
    yield
    _host_cache.clear()


def test_host_path_early_out_reduced_layout_u64(ctx, diet):
    # (a) random DNA, 64-bit indices: k = 21, no two 42-mers of 2^26 positions agree, the first round is the only one -> SA and LCP left early
    hs, st = _host_run(ctx, "dna", 64)
    assert st.n_rounds == 1 and st.ms_host[6] > 0


def test_host_path_no_early_out_reduced_layout_u64(ctx, diet):
    # (a) again with SA and LCP waiting for the construction to return: the same arrays
    diet.setenv("PSACX_NO_EARLY_OUT", "1")
    hs, st = _host_run(ctx, "dna", 64)
    assert st.n_rounds == 1 and st.ms_host[6] == 0


def test_host_path_early_copy_discarded_reduced_layout_u64(ctx, diet):
    # (b) one 300-character repeat: refinement rounds follow, what may have left after the first round is copied again
    hs, st = _host_run(ctx, "repeat", 64)
    assert st.n_rounds > 1 and st.ms_host[6] == 0
    assert 300 <= int(hs.local_LCP.max()) < 65536


def test_host_path_early_out_reduced_layout_lc_u64(ctx, diet):
    # (c) psacx_construct_lc_u64: the same path with the left-branching characters behind it
    hs, st = _host_run(ctx, "dna", 64, lc=True)
    assert st.n_rounds == 1 and st.ms_host[6] > 0
    text = _host_text("dna", 64)
    at = hs.local_SA[:-1].astype(np.int64)[1 << 20:(1 << 20) + 4096] + hs.local_LCP[1:].astype(np.int64)[1 << 20:(1 << 20) + 4096]
    want = np.where(at < text.size, text[np.minimum(at, text.size - 1)], 0).astype(np.uint8)
    assert np.array_equal(hs.local_Lc[(1 << 20) + 1:(1 << 20) + 4097], want)


def test_host_path_reduced_layout_u32(ctx, diet):
    # (d) 32-bit indices: k = 10, and among 2^27 positions about 2^54 / 2 / 4^20 = 8192 pairs of equal 20-mers are expected: the first
    # round leaves buckets unresolved, refinement rounds follow, nothing leaves early (the comment in tests/test_gpu_full_size.py:
    # "a few equal 2k-mers at 32 bits, they wait")
    hs, st = _host_run(ctx, "dna", 32)
    assert hs.k == 10 and st.n_rounds > 1 and st.ms_host[6] == 0
