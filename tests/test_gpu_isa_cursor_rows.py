"""The packed partition levels of the SA -> ISA path run their tiles striped over the parent classes instead of in order, so that
the workgroups running together do not all reserve and write in one class.  Tiles are independent, so SA / ISA / LCP must not change: every
case is checked on its own (order property + Kasai) and array for array against the same construction with PSACX_NO_SPREAD_CURSORS=1 (tiles
in order).  64-bit words, one-word records from 2^21 characters on; the sizes put class and stripe boundaries where they can go wrong, and the
texts vary how the records of the fused first level (rebucket_first_kernel) fall into the classes the later levels read."""
import numpy as np
import pytest

import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def _two_symbols(n, seed):
    # 90 % 'a': a few huge top-digit buckets of the prefix sort, many smaller than a tile
    return np.where(inputs.splitmix64_stream(n, seed) % np.uint64(10) == 0, ord("b"), ord("a")).astype(np.uint8)


def _dna_equal_tail(n, seed):
    # the last 2k - 1 characters equal (k <= 32 characters of two bits in a 64-bit word): the short suffixes fall into one bucket
    t = inputs.dna(n, seed).copy()
    t[n - 63:] = ord("A")
    return t


CASES = {
    "dna_1level_257classes": lambda: inputs.dna((1 << 22) + 4097, 5),           # one level; buckets of about 16 K records: every fourth tile straddles two
    "dna_2levels_class_of_77": lambda: inputs.dna((1 << 23) + 77, 6),           # two levels, the second class of level 1 holds 77 positions
    "dna_3classes_short_last": lambda: inputs.dna((1 << 24) + 8191, 7),         # three classes, the stripes of level 2 over a short last class
    "ascii128_half_empty": lambda: inputs.ascii128((1 << 22) + 1, 8),           # half the top-digit buckets are empty
    "two_symbols_skewed": lambda: _two_symbols((1 << 22) + 3, 9),
    "dna_equal_tail": lambda: _dna_equal_tail(1 << 22, 10),
}
ALWAYS_TOO = ("dna_1level_257classes", "dna_2levels_class_of_77", "dna_3classes_short_last")
PARAMS = [(name, False) for name in CASES] + [(name, True) for name in ALWAYS_TOO]


def _run(ctx, text):
    import psac_amd
    sa = psac_amd.SuffixArray(index_bits=64, lcp=True, ctx=ctx)
    sa.construct(text)
    return sa


@pytest.mark.parametrize("name,always", PARAMS, ids=["%s%s" % (n, "-one_word_always" if a else "") for n, a in PARAMS])
def test_spread_cursors_same_arrays(ctx, monkeypatch, name, always):
    text = CASES[name]()
    monkeypatch.setenv("PSACX_ONE_WORD_MIN", "21")
    if always:
        monkeypatch.setenv("PSACX_ONE_WORD_ALWAYS", "1")
    sa = _run(ctx, text)
    assert O.check_sa(text, sa.local_SA, sa.local_B) == 0
    assert np.array_equal(O.kasai(text, sa.local_SA, sa.local_B), sa.local_LCP)
    SA, B, LCP = sa.local_SA.copy(), sa.local_B.copy(), sa.local_LCP.copy()
    monkeypatch.setenv("PSACX_NO_SPREAD_CURSORS", "1")
    one = _run(ctx, text)
    assert np.array_equal(one.local_SA, SA) and np.array_equal(one.local_B, B) and np.array_equal(one.local_LCP, LCP)


def test_spread_cursors_refinement_levels(ctx, monkeypatch):
    # the other callers of the packed levels: the ISA entries of the refinement rounds (IsaLevels, with tiles skipped inside heavy runs and
    # class regions filled to their counts only) and the rank requests (gather_by_levels) on a repeat whose rounds stay large
    n = (1 << 24) + 4321
    text = inputs.tandem(n, 96, inputs.dna(96, 5))
    monkeypatch.setenv("PSACX_ISA_UPDATE", "levels")
    monkeypatch.setenv("PSACX_GATHER", "levels")
    sa = _run(ctx, text)
    assert len(sa.rounds) > 1
    assert np.array_equal(sa.local_B[sa.local_SA.astype(np.int64)], np.arange(n, dtype=np.uint64))
    SA, B, LCP = sa.local_SA.copy(), sa.local_B.copy(), sa.local_LCP.copy()
    monkeypatch.setenv("PSACX_NO_SPREAD_CURSORS", "1")
    one = _run(ctx, text)
    assert np.array_equal(one.local_SA, SA) and np.array_equal(one.local_B, B) and np.array_equal(one.local_LCP, LCP)
