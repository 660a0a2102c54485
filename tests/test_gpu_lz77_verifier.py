"""psacx_check_lz77_dev_* against the model's count (tests/lz_model.py: check_count, rule by rule as include/psacx.h lists
them), exactly, both index widths:

  - 0 errors on the parse of every named text, of 2^16 random DNA, and on the device's own parse of its own LPF array;
  - the wrong parses of tests/test_lz_model_cpu.py over mississippi, whose counts are stated there by hand -- a source one off,
    a source >= start, a literal of length 2, starts out of order, start[0] != 0, start[z] != n, a phrase one byte too long --
    and the same seven mutations of the parses of 4096 random DNA and of the tandem repeat, against the model's count;
  - lists of random words: the call returns the model's count, whatever the lists hold;
  - refusals.
The text is uploaded for the checker alone; text and lists must come back unchanged."""
import numpy as np
import pytest

import lz_model as M
from lz_gpu_common import LzIndex, Parse, from_model
from rmq_gpu_common import Dev
from test_lz_model_cpu import wrong_parses

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def device_count(dev, t, start, psrc):
    import psac_amd
    st, ps = np.asarray(start).astype(dev.dt), from_model(dev, psrc)
    d_text, d_start, d_psrc = dev.put(t), dev.put(st), dev.put(ps)
    got = psac_amd.check_lz77_device(dev.ctx, d_text, int(t.size), d_start, d_psrc, int(ps.size), dev.bits)
    assert np.array_equal(dev.get(d_text, t.size, np.uint8), t) and np.array_equal(dev.get(d_start, st.size), st)
    assert np.array_equal(dev.get(d_psrc, ps.size), ps)
    return got


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", M.TINY + M.NAMED + ["dna65536"])
def test_correct_parses_have_no_errors(ctx, name, bits):
    t = M.text_of(name)
    dev = Dev(ctx, bits)
    try:
        assert device_count(dev, t, *M.parse_of(name)) == 0
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_the_device_parse_of_the_device_lpf_round_trips(ctx, bits):
    import psac_amd
    t, SA, LCP = M.arrays("dna65536")
    dev = Dev(ctx, bits)
    try:
        p = Parse(dev, *LzIndex(dev, SA, LCP).lpf())
        z = p.count()
        p.lists(z + 1)
        assert psac_amd.check_lz77_device(ctx, dev.put(t), int(t.size), p.d_start, p.d_psrc, z, bits) == 0
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_wrong_parses_of_mississippi_have_the_stated_counts(ctx, bits):
    t = M.text_of("mississippi")
    dev = Dev(ctx, bits)
    try:
        for name, (s, p), want in wrong_parses(t, *M.parse_of("mississippi")):
            assert want > 0 and device_count(dev, t, s, p) == want, name
    finally:
        dev.close()


def mutations(t, start, src):
    """the seven kinds of the catalogue at a phrase in the middle of a longer parse"""
    n, z = int(t.size), int(src.size)
    k = next(i for i in range(z // 2, z) if src[i] != M.ONES and start[i + 1] - start[i] >= 2 and start[i + 1] < n)
    lit = next(i for i in range(1, z - 1) if src[i] == M.ONES) if np.any(src[1:z - 1] == M.ONES) else None
    out = []
    s, p = start.copy(), src.copy(); p[k] += 1; out.append(("source one off", s, p))
    s, p = start.copy(), src.copy(); p[k] = s[k]; out.append(("source >= start", s, p))
    if lit is not None:
        s, p = np.delete(start, lit + 1), np.delete(src, lit + 1); out.append(("literal of length 2", s, p))
    s, p = start.copy(), src.copy(); s[k], s[k + 1] = s[k + 1], s[k]; out.append(("starts out of order", s, p))
    s, p = start.copy(), src.copy(); s[0] = 1; out.append(("start[0] != 0", s, p))
    s, p = start.copy(), src.copy(); s[-1] = n - 1; out.append(("start[z] != n", s, p))
    s, p = start.copy(), src.copy(); s[k + 1] += 1; out.append(("one byte too long", s, p))
    return out


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["dna4096", "tandem3000", "abcab"])
def test_wrong_parses_have_the_models_count(ctx, name, bits):
    t = M.text_of(name)
    dev = Dev(ctx, bits)
    try:
        for what, s, p in mutations(t, *M.parse_of(name)):
            want = M.check_count(t, s, p)
            assert want > 0, (name, what)
            assert device_count(dev, t, s, p) == want, (name, what)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_lists_of_random_words(ctx, bits):
    t = M.text_of("dna4096")
    n = int(t.size)
    rng = np.random.RandomState(41)
    dev = Dev(ctx, bits)
    try:
        for z, below in ((1, n), (17, 2 * n), (n, n), (n, 1 << 31)):
            s = rng.randint(0, below, z + 1, dtype=np.int64)
            p = rng.randint(0, below, z, dtype=np.int64)
            p[::3] = M.ONES
            assert device_count(dev, t, s, p) == M.check_count(t, s, p)
            s = np.sort(s)                                                     # ascending starts, sources of any kind
            assert device_count(dev, t, s, p) == M.check_count(t, s, p)
    finally:
        dev.close()


def test_refusals_and_no_text(ctx):
    import psac_amd
    dev = Dev(ctx, 64)
    try:
        d_zero, d_text = dev.put(np.zeros(2, np.uint64)), dev.put(np.zeros(4, np.uint8))
        assert psac_amd.check_lz77_device(ctx, None, 0, d_zero, None, 0, 64) == 0          # the empty parse of the empty text
        assert psac_amd.check_lz77_device(ctx, d_text, 4, d_zero, None, 0, 64) == 5        # no phrases: start[z] != n and four positions
        for args in ((d_text, 4, None, d_zero, 1), (d_text, 4, d_zero, None, 1), (None, 4, d_zero, d_zero, 1), (d_text, 1, d_zero, d_zero, 2)):
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.check_lz77_device(ctx, args[0], args[1], args[2], args[3], args[4], 64)
            assert e.value.code == -1, args
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.check_lz77_device(ctx, d_text, 1 << 33, d_zero, d_zero, 1, 32)
        assert e.value.code == -2
    finally:
        dev.close()
