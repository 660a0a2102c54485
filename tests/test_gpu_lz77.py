"""psacx_lpf_dev_* and psacx_lz77_dev_* against the host model (tests/lz_model.py: all pairs by byte comparison and the rank walk
over the oracle's arrays, which tests/test_lz_model_cpu.py holds to each other), both index widths:

  - LPF / SRC of the named texts -- mississippi (8 phrases), 300 times 'a' (2), the Fibonacci word of 377 letters (13), ("ab" x
    50) c ("ab" x 50) (5), 4096 random DNA (810), 3000 characters of a period-97 tandem repeat (38) -- and of n = 1, "aa", "ab",
    from the oracle's arrays; of the first two also from psacx_construct_dev_*'s own arrays; of 2^16 random DNA (9242 phrases)
    against the rank walk alone;
  - arrays that are no index: SA with a duplicate, with an entry >= n, LCP with all ones in the middle, an index of random words
    -- the call returns and every slot is (0, all ones) or (src < i, 1 <= lpf <= n - i);
  - the parse of LPF arrays no text has (all zeros, all ones, all n, phrases that end on every tile end, tiles passed over whole,
    geometric lengths of mean 16, one phrase of half the array) against the sequential chain: with PSACX_OPT_LZ_SMALL_TILES (tiles
    of 64 in groups of 4, so 256 positions a group) at n = 255, 256, 257 and 5000 -- every level, the walk over the groups
    included -- and with the default geometry (1024 x 128 = 2^17 a group) at 2^17 + 1, where the walk over the groups has two
    steps, and at 2^20 + 3;
  - the count query, PSACX_ERANGE with the lists untouched and z right, NULL d_src, n = 0;
  - the host-pointer forms, psac_amd.lpf / lz77, SuffixArray.lz77, lz77_decode, the C++ mirror and the command line.
Outputs are pre-filled with a sentinel and have PAD entries of room behind the last one, which must come back untouched; the
inputs must come back unchanged.  No text is uploaded for the two building calls."""
import os
import subprocess

import numpy as np
import pytest

import lz_model as M
from lz_gpu_common import LzIndex, Parse, from_model, to_model, top_of, total
from rmq_gpu_common import Dev, PAD, SENTINEL, first_bad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_B, SMALL_G = 64, 4
B, G = 1024, 128


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


@pytest.fixture
def small_tiles(ctx, monkeypatch):
    monkeypatch.setenv("PSACX_LZ_SMALL_TILES", "1")          # (the wrappers configure from the environment under the test suite)
    ctx.configure(lz_small_tiles=1)
    yield
    ctx.configure(lz_small_tiles=0)


def agree(dev, got, want, what):
    for g, w, part in zip(got, want, ("lpf", "src")):
        bad = first_bad(to_model(dev, g), w)
        assert bad is None, (what, part, bad)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", M.TINY + M.NAMED)
def test_lpf_of_the_named_texts_equals_the_model(ctx, name, bits):
    t, SA, LCP = M.arrays(name)
    dev = Dev(ctx, bits)
    try:
        d = LzIndex(dev, SA, LCP)
        out = d.lpf()
        agree(dev, out, M.lpf_of(name), name)
        assert d.unchanged()
        # ... and the parse cut from the device's own arrays is the recorded one
        p = Parse(dev, *out)
        start, psrc = p.run()
        want = M.parse_of(name)
        assert np.array_equal(start, want[0]) and np.array_equal(psrc, want[1])
        if name in M.NAMED:
            g = M.golden()[name]
            assert start.tolist() == g["start"] and psrc.tolist() == g["src"]
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["mississippi", "a300"])
def test_lpf_from_the_arrays_of_construct_dev(ctx, name, bits):
    import psac_amd
    t = M.text_of(name)
    n = int(t.size)
    dev = Dev(ctx, bits)
    try:
        w = bits // 8
        d_text, d_sa, d_isa, d_lcp = dev.put(t), dev.room(n * w), dev.room(n * w), dev.room(n * w)
        psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx).construct_device(d_text, n, d_sa, d_isa, d_lcp)
        d = LzIndex(dev, dev.get(d_sa, n), dev.get(d_lcp, n))
        agree(dev, d.lpf(), M.lpf_of(name), name)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_lpf_of_random_dna_equals_the_rank_walk(ctx, bits):
    t, SA, LCP = M.arrays("dna65536")
    dev = Dev(ctx, bits)
    try:
        d = LzIndex(dev, SA, LCP)
        out = d.lpf()
        agree(dev, out, M.lpf_of("dna65536"), "dna65536")
        assert d.unchanged()
        start, psrc = Parse(dev, *out).run()
        want = M.parse_of("dna65536")
        assert len(psrc) == 9242 and np.array_equal(start, want[0]) and np.array_equal(psrc, want[1])
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_arrays_that_are_no_index(ctx, bits):
    t, SA, LCP = M.arrays("dna4096")
    n = int(t.size)
    rng = np.random.RandomState(23)
    top = top_of(Dev(ctx, bits))
    dup = SA.copy()
    dup[n // 2] = dup[n // 3]                                                  # a duplicate: two ranks store at one slot
    far = SA.copy()
    far[[5, n // 2, n - 1]] = [n, n + 7, top]                                  # entries >= n write nothing
    ones = LCP.astype(np.uint64).copy()
    ones[n // 2 - 40:n // 2 + 40] = top                                        # all ones in the middle of LCP (and in its index)
    noise = rng.randint(0, 1 << 32, n // 16 + 4096, dtype=np.int64).astype(np.uint64)
    cases = [(dup, LCP, None), (far, LCP, None), (SA, ones, None), (SA, LCP, noise), (SA, LCP, np.zeros(n // 16 + 4096, np.uint64)),
             (rng.randint(0, 2 * n, n, dtype=np.int64).astype(np.uint64), rng.randint(0, 70, n, dtype=np.int64).astype(np.uint64), noise)]
    dev = Dev(ctx, bits)
    try:
        for k, (sa, lcp, index) in enumerate(cases):
            d = LzIndex(dev, sa, lcp, index)
            lpf, src = d.lpf()                                                 # returns PSACX_OK
            assert total(lpf.astype(np.int64), to_model(dev, src), n), k
            assert d.unchanged()
            start, psrc = Parse(dev, lpf, src).run()                           # any n values parse to a chain that ends at n
            assert np.array_equal(start, M.chain(lpf))
            dev.close()
        d = LzIndex(dev, SA, LCP)                                              # a correct call afterwards is right
        agree(dev, d.lpf(), M.lpf_of("dna4096"), "dna4096")
    finally:
        dev.close()


def parse_equals_the_chain(ctx, bits, kind, n, tile):
    dev = Dev(ctx, bits)
    try:
        v = M.synthetic(kind, n, tile, top_of(dev))
        if bits == 32:
            v = np.minimum(v, np.uint64(top_of(dev)))
        p = Parse(dev, v)                                                      # no sources
        start, psrc = p.run()
        want = M.chain(v)
        assert psrc is None
        bad = first_bad(start[:want.size], want[:start.size])
        assert start.size == want.size and bad is None, (kind, n, start.size, want.size, bad)
        assert p.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [SMALL_B * SMALL_G - 1, SMALL_B * SMALL_G, SMALL_B * SMALL_G + 1, 5000])
@pytest.mark.parametrize("kind", M.SYNTHETIC)
def test_parse_with_small_tiles(ctx, small_tiles, kind, n, bits):
    parse_equals_the_chain(ctx, bits, kind, n, SMALL_B)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [B * G + 1, (1 << 20) + 3])
@pytest.mark.parametrize("kind", M.SYNTHETIC)
def test_parse_with_the_default_tiles(ctx, kind, n, bits):
    parse_equals_the_chain(ctx, bits, kind, n, B)


@pytest.mark.parametrize("bits", [32, 64])
def test_parse_with_sources_and_small_tiles(ctx, small_tiles, bits):
    # the named texts once more through every level of the parse
    dev = Dev(ctx, bits)
    try:
        for name in ("tandem3000", "dna4096", "fib377"):
            lpf, src = M.lpf_of(name)
            start, psrc = Parse(dev, lpf, from_model(dev, src)).run()
            want = M.parse_of(name)
            assert np.array_equal(start, want[0]) and np.array_equal(psrc, want[1]), name
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_calling_conventions(ctx, bits):
    import psac_amd
    lpf, src = M.lpf_of("mississippi")
    want = M.parse_of("mississippi")
    dev = Dev(ctx, bits)
    try:
        p = Parse(dev, lpf, from_model(dev, src))
        assert p.count() == 8                                                  # the count query writes nothing and needs no lists
        for cap in (0, 1, 8):                                                  # z + 1 = 9 entries do not fit
            with pytest.raises(psac_amd.PsacxError) as e:
                p.lists(9, cap=cap)
            assert e.value.code == -2 and e.value.z == 8
            assert np.all(p.raw[0] == SENTINEL) and np.all(p.raw[1] == SENTINEL)
        start, psrc, z = p.lists(12, cap=9)
        assert z == 8 and np.array_equal(start[:9].astype(np.int64), want[0]) and np.array_equal(to_model(dev, psrc[:8]), want[1])
        assert np.all(start[9:] == SENTINEL) and np.all(psrc[8:] == SENTINEL)
        # without sources: the starts alone
        q = Parse(dev, lpf)
        start, none, z = q.lists(9)
        assert z == 8 and none is None and np.array_equal(start[:9].astype(np.int64), want[0])
        with pytest.raises(psac_amd.PsacxError) as e:                          # sources asked for, none given
            psac_amd.lz77_device(ctx, p.n, p.d_lpf, None, p.d_start, p.d_psrc, 9, bits)
        assert e.value.code == -1
        # n = 0: no phrases, start[0] = n = 0
        assert psac_amd.lz77_device(ctx, 0, None, None, None, None, 0, bits) == 0
        d_one = dev.put(np.full(1 + PAD, SENTINEL, dev.dt))
        assert psac_amd.lz77_device(ctx, 0, None, None, d_one, None, 1, bits) == 0
        got = dev.get(d_one, 1 + PAD)
        assert got[0] == 0 and np.all(got[1:] == SENTINEL)
        psac_amd.lpf_device(ctx, 0, None, None, None, d_one, d_one, bits)      # n = 0 is legal
        d = LzIndex(dev, *M.arrays("mississippi")[1:])
        for outs in ((None, d_one), (d_one, None)):                            # a NULL output
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.lpf_device(ctx, d.n, d.d_sa, d.lcp.d_v, d.lcp.d_index, outs[0], outs[1], bits)
            assert e.value.code == -1
        if bits == 32:                                                         # n beyond the index type
            for n in (0xFFFFFFFF, 1 << 33):
                with pytest.raises(psac_amd.PsacxError) as e:
                    psac_amd.lpf_device(ctx, n, d.d_sa, d.lcp.d_v, d.lcp.d_index, d_one, d_one, bits)
                assert e.value.code == -2
                with pytest.raises(psac_amd.PsacxError) as e:
                    psac_amd.lz77_device(ctx, n, p.d_lpf, None, None, None, 0, bits)
                assert e.value.code == -2
        assert np.all(dev.get(d_one, 1 + PAD)[1:] == SENTINEL)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_pointer_forms_and_python(ctx, bits):
    import psac_amd
    dt = np.uint32 if bits == 32 else np.uint64
    for name in ("mississippi", "tandem3000", "dna4096"):
        t, SA, LCP = M.arrays(name)
        lpf, src = psac_amd.lpf(SA.astype(dt), LCP.astype(dt), ctx=ctx)
        assert lpf.dtype == dt and src.dtype == dt
        want = M.lpf_of(name)
        dev = Dev(ctx, bits)
        assert np.array_equal(lpf.astype(np.int64), want[0]) and np.array_equal(to_model(dev, src), want[1])
        start, psrc = psac_amd.lz77(SA.astype(dt), LCP.astype(dt), ctx=ctx)
        wp = M.parse_of(name)
        assert start.dtype == dt and np.array_equal(start.astype(np.int64), wp[0]) and np.array_equal(to_model(dev, psrc), wp[1])
        literals = np.zeros(t.size, np.uint8)
        literals[wp[0][:-1][wp[1] == M.ONES]] = t[wp[0][:-1][wp[1] == M.ONES]]
        assert psac_amd.lz77_decode(start, psrc, literals) == t.tobytes()       # the round trip, from the literals alone
    # the chain a user runs: construct, then .lz77, then lz77_decode
    text = M.text_of("fib377").tobytes()
    sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
    with pytest.raises(ValueError):
        sa.lz77()                                                              # nothing constructed
    sa.construct(text)
    start, psrc = sa.lz77()
    assert start.size == 14 and psac_amd.lz77_decode(start, psrc, text) == text
    with pytest.raises(ValueError):
        nolcp = psac_amd.SuffixArray(index_bits=bits, lcp=False, ctx=ctx)
        nolcp.construct(text)
        nolcp.lz77()
    with pytest.raises(ValueError):
        ss = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
        ss.construct_ss([b"abab", b"babab"])
        ss.lz77()                                                              # a string set: out of scope


def test_cpp_mirror_lz77(tmp_path):
    from test_lz_build_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "lz77 header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64", "auto"])
def test_command_line(tmp_path, index):
    exe = os.path.join(ROOT, "psac_amd", "bin", "lz77")
    (tmp_path / "text").write_bytes(b"mississippi")
    r = subprocess.run([exe, "-f", str(tmp_path / "text"), "--index", index, "--list", "-c"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "z: 8 n/z: 1.375\nerrors: 0\n" + M.cli_text(*M.parse_of("mississippi"))
    assert "LPF time:" in r.stderr and "Parse time:" in r.stderr
    (tmp_path / "dna").write_bytes(M.text_of("dna4096").tobytes())
    r = subprocess.run([exe, "-f", str(tmp_path / "dna"), "--index", index, "-c"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: 810 n/z: %g\nerrors: 0\n" % (4096 / 810.0), r.stdout + r.stderr
