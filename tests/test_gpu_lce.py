"""psacx_lce_dev_* against the host model (tests/lce_model.py: the byte-by-byte definition), both index widths, on the texts of
locate_model and the sets of locate_gsa_model with the oracle's ISA / LCP: all pairs of the tiny texts; for the others equal
positions, the text's ends and beyond, neighbours in SA, the extreme ranks, ranks around 64 and 4096, and random pairs; 0, 1, 2, 5
and n mismatches; in sets, pairs across strings, inside equal strings, at first and last characters, and pairs whose stepped-over
mismatch is the last character of a string; arrays that are no index; and the layers above: the host-pointer forms, psac_amd.lce
and psac_amd.rmq, the chain after a construction in HBM, the C++ mirror and the command line.  The text is never uploaded for
the device calls: nothing in them reads it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lce_model as E
import locate_gsa_model as G
import locate_model as L
import rmq_model as R
from rmq_gpu_common import Dev, LceIndex, first_bad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


_want = {}


def want_of(text, off, a, b, e):
    """the lengths by the byte-by-byte definition; computed once per batch and shared by the two index widths"""
    key = (text.size, text[:64].tobytes(), None if off is None else off.tobytes(), a.tobytes(), b.tobytes(), e)
    if key not in _want:
        _want[key] = np.array([E.by_bytes(text, off, int(x), int(y), e) for x, y in zip(a, b)], np.int64)
    return _want[key]


def agree(d, text, off, a, b, e, **kw):
    got = d.lce(a, b, e, **kw)
    bad = first_bad(got, want_of(text, off, a, b, e))
    assert bad is None, (e, bad, int(a[bad[0]]), int(b[bad[0]]))
    n = int(text.size)
    room = np.where((a < n) & (b < n), n - np.maximum(a, b), 0)
    assert np.all(got <= room)


def pairs_of_text(n, SA, seed=4):
    """(a, b) as int64 arrays: every pair of 0 .. n + 1 for a tiny text, else the catalogue of the module's docstring"""
    if n <= 17:
        a, b = [x.reshape(-1) for x in np.meshgrid(np.arange(n + 2), np.arange(n + 2), indexing="ij")]
        return a.astype(np.int64), b.astype(np.int64)
    rng = np.random.RandomState(seed)
    SA = SA.astype(np.int64)
    ends = [0, n - 1, n, n + 1]
    some = [int(x) for x in rng.randint(0, n, 12)]
    pr = [(p, p) for p in ends + some]
    pr += [(x, y) for x in ends for y in ends + some] + [(y, x) for x in ends for y in some]
    near = rng.randint(0, n - 1, 400)
    pr += [(int(SA[i]), int(SA[i + 1])) for i in near] + [(int(SA[i + 1]), int(SA[i])) for i in near[:50]]
    pr += [(int(SA[0]), int(SA[n - 1])), (int(SA[n - 1]), int(SA[0]))]
    ranks = [r for r in (0, 1, 62, 63, 64, 65, 66, 127, 128, 4094, 4095, 4096, 4097, 4098, n - 1) if r < n]
    pr += [(int(SA[r]), int(SA[s])) for r in ranks for s in ranks]
    pr += [tuple(int(x) for x in rng.randint(0, n, 2)) for _ in range(5000)]
    return np.array([p for p, _ in pr], np.int64), np.array([q for _, q in pr], np.int64)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", L.SMALL + ["dna"])
def test_texts_equal_the_model(ctx, name, bits):
    text, SA, ISA, LCP = E.arrays(name)
    n = int(text.size)
    a, b = pairs_of_text(n, SA)
    dev = Dev(ctx, bits)
    try:
        d = LceIndex(dev, ISA, LCP)
        for e in (0, 1, 2, 5, n):
            agree(d, text, None, a, b, e)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("name", ["unary", "tandem"])
def test_long_answers(name):
    # (what the catalogue holds, checked on the host: these two texts give answers of thousands of characters)
    text, SA, ISA, LCP = E.arrays(name)
    a, b = pairs_of_text(int(text.size), SA)
    keep = a[:600] != b[:600]
    assert (want_of(text, None, a[:600][keep], b[:600][keep], 0) > 2000).any()


def pairs_of_set(text, off, SA, seed=6):
    n, o = int(text.size), [int(x) for x in off]
    m = len(o) - 1
    if n <= 17:
        a, b = [x.reshape(-1) for x in np.meshgrid(np.arange(n + 2), np.arange(n + 2), indexing="ij")]
        return a.astype(np.int64), b.astype(np.int64)
    rng = np.random.RandomState(seed)
    SA = SA.astype(np.int64)
    pick = sorted(set([0, m - 1] + [int(x) for x in rng.randint(0, m, 10)]))
    firsts, lasts = [o[t] for t in pick], [o[t + 1] - 1 for t in pick]
    edge = sorted(set(firsts + lasts + [n - 1, n, n + 1]))
    pr = [(x, y) for x in edge for y in edge]                                        # first / last characters, equal positions, beyond n
    for t in pick:                                                                   # inside one string, and the same offset of two strings
        ln = o[t + 1] - o[t]
        for _ in range(20):
            x, y = (int(v) for v in rng.randint(0, ln, 2))
            u = pick[int(rng.randint(0, len(pick)))]
            pr += [(o[t] + x, o[t] + y), (o[t] + x, min(o[u] + x, n - 1))]
    near = rng.randint(0, n - 1, 400)
    pr += [(int(SA[i]), int(SA[i + 1])) for i in near] + [(int(SA[0]), int(SA[n - 1]))]
    ranks = [r for r in (0, 63, 64, 65, 4095, 4096, 4097, n - 1) if r < n]
    pr += [(int(SA[r]), int(SA[s])) for r in ranks for s in ranks]
    pr += [tuple(int(x) for x in rng.randint(0, n, 2)) for _ in range(3000)]
    return np.array([p for p, _ in pr], np.int64), np.array([q for _, q in pr], np.int64)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", G.GPU)
def test_sets_equal_the_model(ctx, name, bits):
    text, off, SA, ISA, LCP = E.set_arrays(name)
    n = int(text.size)
    a, b = pairs_of_set(text, off, SA)
    dev = Dev(ctx, bits)
    try:
        d = LceIndex(dev, ISA, LCP, off)
        for e in (0, 1, 2, 5, n):
            agree(d, text, off, a, b, e)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_a_stepped_over_mismatch_that_is_the_last_character_of_a_string(ctx, bits):
    name = G.READS_SMALL
    text, off, SA, ISA, LCP = E.set_arrays(name)
    n, o = int(text.size), [int(x) for x in off]
    rng = np.random.RandomState(11)
    a, b = [], []
    for t in rng.randint(0, len(o) - 1, 400):
        for j in (0, 1, 2, 3):
            x, y = o[t + 1] - 1 - j, int(rng.randint(0, n))
            # the two agree for j characters, differ in the string's last one, and b's string goes on behind it
            if E.by_bytes(text, off, x, y, 0) == j and E.limit(off, n, x, y) == j + 1 and E.end_of(off, n, y) - y > j + 1:
                a.append(x)
                b.append(y)
    assert len(a) >= 50
    a, b = np.array(a, np.int64), np.array(b, np.int64)
    dev = Dev(ctx, bits)
    try:
        d = LceIndex(dev, ISA, LCP, off)
        for e in (1, 2):
            got = d.lce(a, b, e)
            assert np.array_equal(got, want_of(text, off, a, b, e)) and np.array_equal(got, want_of(text, off, a, b, 0) + 1)
        for e in (0, 1, 2, 5):                                                       # and the other way round
            agree(d, text, off, b, a, e)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["mississippi", "edge4097"])
def test_a_set_of_one_string_equals_the_plain_form(ctx, name, bits):
    text, SA, ISA, LCP = E.arrays(name)
    n = int(text.size)
    a, b = pairs_of_text(n, SA)
    dev = Dev(ctx, bits)
    try:
        d = LceIndex(dev, ISA, LCP, np.array([0, n], np.uint64))
        for e in (0, 1, 5, n):
            assert np.array_equal(d.lce(a, b, e), d.lce(a, b, e, plain=True)), e
            agree(d, text, None, a, b, e)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_arrays_that_are_no_index(ctx, bits):
    name = G.READS_SMALL
    text, off, SA, ISA, LCP = E.set_arrays(name)
    n = int(text.size)
    a, b = pairs_of_set(text, off, SA)
    rng = np.random.RandomState(13)
    top = R.ones(np.uint32 if bits == 32 else np.uint64)
    shuffled = off.copy()
    rng.shuffle(shuffled)
    garbage = (rng.randint(0, 1 << 32, n // 16 + 4096, dtype=np.int64))
    cases = [
        (np.full(n, top, np.uint64), LCP, off, None),                              # an ISA of all ones
        (rng.randint(0, 2 * n, n).astype(np.uint64), LCP, off, None),               # a random ISA
        (ISA, rng.randint(0, 3 * n, n).astype(np.uint64), off, None),               # a random LCP
        (ISA, np.full(n, top, np.uint64), off, None),                              # an LCP of all ones
        (ISA, LCP, shuffled, None),                                                  # shuffled offsets
        (ISA, LCP, np.full(off.size, top if bits == 64 else (1 << 40), np.uint64), None),
        (ISA, LCP, off, garbage),                                                    # an index of random words
    ]
    room = np.where((a < n) & (b < n), n - np.maximum(a, b), 0)
    dev = Dev(ctx, bits)
    try:
        for isa, lcp, so, index in cases:
            d = LceIndex(dev, isa, lcp, so, index=index)
            for e in (0, 1, 5, n):
                for plain in (False, True):
                    got = d.lce(a, b, e, plain=plain)                                 # returns PSACX_OK
                    assert np.all(got <= room), (e, plain)
            assert d.unchanged()
        d = LceIndex(dev, ISA, LCP, off)                                              # a correct call afterwards is right
        agree(d, text, off, a, b, 2)
    finally:
        dev.close()


def test_refusals(ctx):
    import psac_amd
    text, off, SA, ISA, LCP = E.set_arrays("copies")
    dev = Dev(ctx, 64)
    try:
        d = LceIndex(dev, ISA, LCP, off)
        pa = dev.put(np.zeros(4, np.uint64))
        out = dev.put(np.full(4, 77, np.uint64))
        for m in (0, d.n + 1):                                                        # a set of no strings, or of more strings than characters
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.lce_device(ctx, d.n, d.d_off, m, d.d_isa, d.lcp.d_v, d.lcp.d_index, pa, pa, 4, 0, out, 64)
            assert e.value.code == -1
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.lce_device(ctx, d.n, None, 0, d.d_isa, d.lcp.d_v, d.lcp.d_index, pa, pa, 4, 0, None, 64)
        assert e.value.code == -1
        assert np.all(dev.get(out, 4) == 77)
        psac_amd.lce_device(ctx, d.n, None, 0, None, None, None, None, None, 0, 0, None, 64)      # q == 0
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_pointer_forms_and_python(ctx, bits):
    import psac_amd
    dt = np.uint32 if bits == 32 else np.uint64
    text, SA, ISA, LCP = E.arrays("mississippi")
    n = int(text.size)
    a, b = pairs_of_text(n, SA)
    for e in (0, 1, 2, n):
        got = psac_amd.lce(ISA.astype(dt), LCP.astype(dt), a, b, max_mismatch=e, ctx=ctx)
        assert got.dtype == dt and np.array_equal(got.astype(np.int64), want_of(text, None, a, b, e))
    lo, hi = [x.reshape(-1) for x in np.meshgrid(np.arange(n + 2), np.arange(n + 3), indexing="ij")]
    mn, arg = psac_amd.rmq(LCP.astype(dt), lo, hi, ctx=ctx)
    want = R.queries(LCP.astype(dt), lo, hi)
    assert np.array_equal(mn, want[0]) and np.array_equal(arg, want[1])
    stext, off, sSA, sISA, sLCP = E.set_arrays("copies")
    a, b = pairs_of_set(stext, off, sSA)
    for e in (0, 1, 5):
        got = psac_amd.lce(sISA.astype(dt), sLCP.astype(dt), a, b, max_mismatch=e, offsets=off, ctx=ctx)
        assert np.array_equal(got.astype(np.int64), want_of(stext, off, a, b, e))
    assert psac_amd.lce(ISA.astype(dt), LCP.astype(dt), [], [], ctx=ctx).size == 0
    # a larger array through the host form: three levels of index
    v = np.random.RandomState(3).randint(0, 50, 300000).astype(dt)
    lo = np.random.RandomState(4).randint(0, 300000, 2000)
    hi = lo + np.random.RandomState(5).randint(0, 300000, 2000)
    mn, arg = psac_amd.rmq(v, lo, hi, ctx=ctx)
    want = R.Table(v).queries(lo, hi)
    assert np.array_equal(mn, want[0]) and np.array_equal(arg, want[1])


@pytest.mark.parametrize("bits", [32, 64])
def test_lce_after_a_construction_in_hbm(ctx, bits):
    # the chain a user runs: construct_device leaves ISA and LCP in HBM, the index is built over LCP there, and the pairs are
    # answered there
    import psac_amd
    dt, w = (np.uint32 if bits == 32 else np.uint64), bits // 8
    dev = Dev(ctx, bits)
    try:
        text, SA, ISA, LCP = E.arrays("dna")
        n = int(text.size)
        d_text, d_sa, d_isa, d_lcp = dev.put(text), dev.room(n * w), dev.room(n * w), dev.room(n * w)
        psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx).construct_device(d_text, n, d_sa, d_isa, d_lcp)
        entries = psac_amd.rmq_index_device(ctx, None, n, None, bits)
        d_index = dev.room(entries * w)
        psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, bits)
        a, b = pairs_of_text(n, SA)
        d_a, d_b, d_len = dev.put(a.astype(dt)), dev.put(b.astype(dt)), dev.room(a.size * w)
        for e in (0, 3):
            psac_amd.lce_device(ctx, n, None, 0, d_isa, d_lcp, d_index, d_a, d_b, a.size, e, d_len, bits)
            assert np.array_equal(dev.get(d_len, a.size).astype(np.int64), want_of(text, None, a, b, e))

        stext, off, sSA, sISA, sLCP = E.set_arrays(G.READS_SMALL)
        n, m = int(stext.size), int(off.size - 1)
        d_text, d_off, d_sa, d_isa, d_lcp = dev.put(stext), dev.put(off), dev.room(n * w), dev.room(n * w), dev.room(n * w)
        fn = getattr(ctx._lib, "psacx_construct_gsa_dev_u%d" % bits)
        ctx.check(fn(ctx.handle, C.c_void_p(d_text), n, C.c_void_p(d_off), m, 0, 1, C.c_void_p(d_sa), C.c_void_p(d_isa), C.c_void_p(d_lcp)))
        entries = psac_amd.rmq_index_device(ctx, None, n, None, bits)
        d_index = dev.room(entries * w)
        psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, bits)
        a, b = pairs_of_set(stext, off, sSA)
        d_a, d_b, d_len = dev.put(a.astype(dt)), dev.put(b.astype(dt)), dev.room(a.size * w)
        for e in (0, 3):
            psac_amd.lce_device(ctx, n, d_off, m, d_isa, d_lcp, d_index, d_a, d_b, a.size, e, d_len, bits)
            assert np.array_equal(dev.get(d_len, a.size).astype(np.int64), want_of(stext, off, a, b, e))
    finally:
        dev.close()


def test_cpp_mirror_lce(tmp_path):
    from test_rmq_lce_model_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "lce header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64", "auto"])
def test_command_line(tmp_path, index):
    exe = os.path.join(ROOT, "psac_amd", "bin", "lce")
    text, SA, ISA, LCP = E.arrays("edge4097")
    n = int(text.size)
    a, b = pairs_of_text(n, SA)
    a, b = a[:700], b[:700]
    (tmp_path / "text").write_bytes(text.tobytes())
    (tmp_path / "pairs").write_text("".join("%d %d\n" % (x, y) for x, y in zip(a, b)))
    for e in (0, 2):
        r = subprocess.run([exe, "-f", str(tmp_path / "text"), "-p", str(tmp_path / "pairs"), "-e", str(e), "--index", index], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout == E.cli_text(want_of(text, None, a, b, e))
        assert "LCE time:" in r.stderr
    # a set: the lines of the file are the strings; positions as numbers and as string:offset
    strings = [bytes(s) if not isinstance(s, np.ndarray) else s.tobytes() for s in G.strings_of("copies")]
    assert all(b"\n" not in s for s in strings)
    stext, off, sSA, sISA, sLCP = E.set_arrays("copies")
    o = [int(x) for x in off]
    a, b = pairs_of_set(stext, off, sSA)
    a, b = a[:600], b[:600]

    def spell(p, i):
        if i % 2 or p >= o[-1]:
            return "%d" % p
        t = max(s for s in range(len(o) - 1) if o[s] <= p)
        return "%d:%d" % (t, p - o[t])
    (tmp_path / "set").write_bytes(b"\n".join(strings) + b"\n")
    (tmp_path / "spairs").write_text("".join("%s %s\n" % (spell(int(x), i), spell(int(y), i + 1)) for i, (x, y) in enumerate(zip(a, b))))
    out = tmp_path / "out.txt"
    r = subprocess.run([exe, "-f", str(tmp_path / "set"), "-p", str(tmp_path / "spairs"), "--set", "-e", "1", "--index", index, "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    assert out.read_text() == E.cli_text(want_of(stext, off, a, b, 1))
