"""psacx_bwt_dev_* against the host model (tests/repeats_model.py: the BWT from its definition), both index widths, SA from the oracle:

  - one text at n = 1, 2, 3, 31, 32, 33, 63, 64, 65 (bitmap words, one wave's ballot), 4095, 4096, 4097 and 2^18 + 1, over random
    texts of 2 and 4 letters, a^n, a Fibonacci word, a period-7 tandem repeat, all 256 byte values and reads with a planted repeat;
    the BWT byte by byte, `first` bit by bit with the words at and beyond n, the primary, and the round trip through bwt_decode;
  - string sets: random ones, m = n, 3000 identical strings, 257 strings that share a suffix;
  - each of the NULL outputs, both NULL, n = 0, n beyond the index type;
  - totality: SA with entries >= n, without a zero, with two zeros -- the call returns, the room behind the outputs is untouched,
    an entry >= n gives byte 0 and a clear bit;
  - the host-pointer forms, psac_amd.bwt and SuffixArray.bwt from bytes.
Outputs are pre-filled with a sentinel and have PAD entries of room behind the last one, which must come back untouched; the
inputs must come back unchanged."""
import numpy as np
import pytest

import repeats_model as M
from repeats_gpu_common import BIG, SETS, SIZES, RepIndex, set_case, text_case
from rmq_gpu_common import Dev, PAD, SENTINEL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def check_bwt(dev, case, decode=True):
    import psac_amd
    d = RepIndex(dev, case)
    bwt, first, primary = d.run_bwt()
    bad = np.nonzero(bwt != case.bwt)[0]
    assert bad.size == 0, (int(bad[0]), int(bwt[bad[0]]), int(case.bwt[bad[0]]), int(bad.size))
    assert np.array_equal(first, case.first_words())
    assert primary == case.primary and int(case.SA[primary]) == 0
    assert d.unchanged()
    if decode and case.off is None:
        assert psac_amd.bwt_decode(bwt, primary) == case.text.tobytes()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", SIZES)
def test_bwt_of_one_text_equals_the_model(ctx, n, bits):
    dev = Dev(ctx, bits)
    try:
        for kind in M.TEXTS:
            check_bwt(dev, text_case(kind, n))
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_bwt_at_the_third_index_level(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        check_bwt(dev, text_case("dna4", BIG))
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", SETS)
def test_bwt_of_a_string_set_equals_the_model(ctx, name, bits):
    dev = Dev(ctx, bits)
    try:
        case = set_case(name)
        check_bwt(dev, case)
        assert int(case.first.sum()) == len(case.strings)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_null_outputs_and_refusals(ctx, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        for case in (text_case("dna4", 4097), set_case("random")):
            d = RepIndex(dev, case)
            bwt, first, primary = d.run_bwt(want_first=False)
            assert first is None and np.array_equal(bwt, case.bwt) and primary == case.primary
            bwt, first, primary = d.run_bwt(want_bwt=False)
            assert bwt is None and np.array_equal(first, case.first_words()) and primary == case.primary
            bwt, first, primary = d.run_bwt(want_primary=False)
            assert primary is None and np.array_equal(bwt, case.bwt) and np.array_equal(first, case.first_words())
            with pytest.raises(psac_amd.PsacxError) as e:
                d.run_bwt(want_bwt=False, want_first=False)
            assert e.value.code == -1
        d_one = dev.put(np.full(1 + PAD, SENTINEL, np.uint32))
        assert psac_amd.bwt_device(ctx, None, 0, None, None, None, d_one, bits) == 0xFFFFFFFFFFFFFFFF       # n = 0: one clear word, no primary
        assert dev.get(d_one, 1 + PAD, np.uint32).tolist() == [0] + [SENTINEL] * PAD
        if bits == 32:
            for n in (0xFFFFFFFF, 1 << 33):
                with pytest.raises(psac_amd.PsacxError) as e:
                    psac_amd.bwt_device(ctx, d.d_text, n, None, d.d_sa, d.d_bwt, None, bits)
                assert e.value.code == -2
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["text", "set"])
def test_totality_over_arrays_that_are_no_suffix_array(ctx, name, bits):
    dev = Dev(ctx, bits)
    try:
        case = text_case("dna4", 4097) if name == "text" else set_case("random")
        n, top = case.n, int(np.iinfo(dev.dt).max)
        rng = np.random.RandomState(5)
        at = rng.choice(n, 200, replace=False)
        for what in ("beyond", "no zero", "two zeros"):
            sa = case.SA.astype(np.uint64)
            zero = int(np.nonzero(sa == 0)[0][0])
            if what == "beyond":
                sa[at[:100]] = n
                sa[at[100:]] = top
                sa[zero] = 0
            elif what == "no zero":
                sa[zero] = 1
            else:
                sa[(zero + 1000) % n] = 0
            d = RepIndex(dev, case, SA=sa)
            bwt, first, primary = d.run_bwt()              # (the room behind both outputs is checked there)
            assert d.unchanged()
            want_bwt, want_first, _ = M.bwt_of(case.text, np.where(sa < n, sa, 0).astype(np.int64), case.off)
            inside = sa < n
            want_bwt[~inside], want_first[~inside] = 0, False
            assert np.array_equal(bwt, want_bwt)
            bits_got = np.unpackbits(first.astype("<u4").view(np.uint8), bitorder="little")
            assert np.array_equal(bits_got[:n].astype(bool), want_first) and not bits_got[n:].any()
            zeros = np.nonzero(sa == 0)[0]
            assert primary == 0xFFFFFFFFFFFFFFFF if zeros.size == 0 else primary in zeros.tolist()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_pointer_forms_and_python(ctx, bits):
    import psac_amd
    dt = np.uint32 if bits == 32 else np.uint64
    for case in (text_case("fib", 4097), text_case("bytes256", 4096), set_case("random"), set_case("w257")):
        bwt, primary = psac_amd.bwt(case.text, case.SA.astype(dt), offsets=case.off, ctx=ctx)
        assert bwt.dtype == np.uint8 and np.array_equal(bwt, case.bwt) and primary == case.primary
    with pytest.raises(psac_amd.PsacxError) as e:                                  # offsets that do not end at n
        psac_amd.bwt(b"abcab", np.array([3, 0, 4, 1, 2], dt), offsets=[0, 2, 4], ctx=ctx)
    assert e.value.code == -1
    # the chain a user runs: construct, then .bwt, then bwt_decode
    text = M.text_of("planted", 3001, 9).tobytes()
    sa = psac_amd.SuffixArray(index_bits=bits, ctx=ctx)
    with pytest.raises(ValueError):
        sa.bwt()                                                                   # nothing constructed
    sa.construct(text)
    bwt, primary = sa.bwt()
    assert int(sa.local_SA[primary]) == 0 and psac_amd.bwt_decode(bwt, primary) == text
    strings = set_case("random").strings
    ss = psac_amd.SuffixArray(index_bits=bits, ctx=ctx)
    ss.construct_ss(strings)
    bwt, primary = ss.bwt()
    assert np.array_equal(bwt, set_case("random").bwt) and primary == set_case("random").primary
