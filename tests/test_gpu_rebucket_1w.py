"""The first round on one-word records runs rebucket_first_1w_kernel, the 32-bit form of rebucket_first_kernel.  What it writes
must be what the generic kernel writes, so every case is constructed twice, by default and with PSACX_GENERIC_REBUCKET=1 (the generic
kernel), and SA, ISA, LCP and the log of the rounds must agree; the default run is also checked on its own (order property + Kasai).
psacx_stats.rebucket_1w says which kernel ran: the cases of LEAN assert that the default run took the new one and the pinned run did not.
64-bit indices, LCP on, PSACX_ONE_WORD_MIN=21.  The arithmetic of the kernel at n = 2^32 is covered on the host
(test_rebucket_1w_math_cpu.py)."""
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
    # 90 % 'a': one bit per character, a few huge top-digit buckets, many smaller than a tile, long tie groups
    return np.where(inputs.splitmix64_stream(n, seed) % np.uint64(10) == 0, ord("b"), ord("a")).astype(np.uint8)


def _dna_equal_tail(n, seed):
    # the last 2k - 1 characters equal: the short suffixes share their packed prefix with long ones; the length caps decide heads and LCP
    t = inputs.dna(n, seed).copy()
    t[n - 63:] = ord("A")
    return t


def _dna_copied_stretch(n, seed, src, dst):
    # one stretch of 5000 characters at a second place: about 4900 buckets of two suffixes each, spread over the sorted order
    # (seed and places chosen on the host so that some of them lie across the tile borders the test asserts)
    t = inputs.dna(n, seed).copy()
    t[dst:dst + 5000] = t[src:src + 5000]
    return t


def _two_symbols_even(n, seed):
    # one bit per character, both symbols as often: 32-character leading parts, hardly any shared by more than two suffixes
    return np.where(inputs.splitmix64_stream(n, seed) & np.uint64(1), ord("b"), ord("a")).astype(np.uint8)


TAIL_AT, TAIL_LEN, TAIL_RUN = 1000003, 40, 22


def _dna_short_tail_pairs(n, seed):
    # the last 40 characters (shorter than a window) are those at TAIL_AT, where 22 'A' (the code the end of the text is padded with) follow:
    # short suffix n - 40 + i and long suffix TAIL_AT + i have the same packed window for i <= 20 and tie in a group of two; only the cap by
    # the length makes the second a head and gives its LCP.  No leading part (16 characters) is shared by more than 8 suffixes.
    t = inputs.dna(n, seed).copy()
    p, m, r = TAIL_AT, TAIL_LEN, TAIL_RUN
    t[p + m - 1] = ord("C")
    t[p + m:p + m + r] = ord("A")
    t[p + m + r] = ord("C")
    t[n - m:] = t[p:p + m]
    return t


def _dna_few_copies(n, seed):
    # 2000 stretches of 300 characters at a second place, every third at a third one too: 1.3 million suffixes in buckets of two or three
    # that the first round leaves unresolved, in tie groups of at most 6: refinement rounds follow, most tiles write their ids
    t = inputs.dna(n, seed).copy()
    half = n // 2
    for r in range(2000):
        src = 1000 * r + 17
        t[half + 1000 * r + 5:half + 1000 * r + 305] = t[src:src + 300]
        if r % 3 == 0:
            t[half + half // 2 + 1000 * r + 11:half + half // 2 + 1000 * r + 311] = t[src:src + 300]
    return t


# The seven texts of the first group are at the smallest sizes at which the first round runs in two stages (2^21 characters; 2^22 where a case
# needs more).  They do not reach the new kernel: the engine takes the one-word prefix sort only where its bucket tables fit into the sort's
# scratch (from 2^23 characters on for these texts), so both runs of such a case take the generic kernel -- a parity check of the option at
# sizes where it must change nothing.
SMALL = {
    "dna_last_tile_of_3": lambda: inputs.dna((1 << 21) + 4097 + 3, 21),
    "dna_one_short_of_16": lambda: inputs.dna((1 << 22) + 8191, 22),
    "ascii128_lc7": lambda: inputs.ascii128((1 << 21) + 1, 23),
    "two_symbols_lc1": lambda: _two_symbols((1 << 21) + 3, 24),
    "dna_equal_tail": lambda: _dna_equal_tail(1 << 21, 25),
    "mutated_many_unresolved": lambda: inputs.mutated((1 << 22) + 1234, 4096, 26),
    "dna_buckets_across_tiles": lambda: _dna_copied_stretch(1 << 21, 11, 300000, 1200143),
}
# The texts that do reach it, at 2^23 characters.  The records stay one-word up to the rebucket kernel only if no more than 8 suffixes share
# a leading part (else the tie stage takes its radix path and the generic kernel follows), which a skewed two-symbol text, a long equal tail
# and a tandem repeat do not meet: those three come as texts with the same property in groups of at most 8.
LEAN = {
    "dna_last_tile_of_3_8m": lambda: inputs.dna((1 << 23) + 4097 + 3, 21),          # the last scan tile holds 3 records
    "dna_one_short_of_16_8m": lambda: inputs.dna((1 << 23) + 8191, 22),             # one record short of a whole number of 16-record runs
    "ascii128_lc7_8m": lambda: inputs.ascii128((1 << 23) + 1, 23),                  # seven bits per character, a top digit over two characters, half the buckets empty
    "two_symbols_even_lc1_8m": lambda: _two_symbols_even((1 << 23) + 3, 24),        # one bit per character
    "dna_short_tail_pairs_8m": lambda: _dna_short_tail_pairs(1 << 23, 25),          # the length caps decide heads and LCP
    "dna_few_copies_8m": lambda: _dna_few_copies((1 << 23) + 1234, 26),             # many unresolved buckets, refinement rounds on Bsa / n_active / n_unf
    "dna_buckets_across_tiles_8m": lambda: _dna_copied_stretch(1 << 23, 13, 300000, 5200169),
}
CASES = dict(SMALL)
CASES.update(LEAN)
PARAMS = [(name, False) for name in CASES] + [("dna_last_tile_of_3", True), ("dna_last_tile_of_3_8m", True)]


def _run(ctx, text):
    import psac_amd
    sa = psac_amd.SuffixArray(index_bits=64, lcp=True, ctx=ctx)
    sa.construct(text)
    return sa


@pytest.mark.parametrize("name,always", PARAMS, ids=["%s%s" % (n, "-one_word_always" if a else "") for n, a in PARAMS])
def test_lean_rebucket_same_arrays(ctx, monkeypatch, name, always):
    text = CASES[name]()
    monkeypatch.setenv("PSACX_ONE_WORD_MIN", "21")
    if always:
        monkeypatch.setenv("PSACX_ONE_WORD_ALWAYS", "1")
    sa = _run(ctx, text)
    st = ctx.stats()
    print("%s: n %d, rounds %d, one-word passes %d, lean kernel %d" % (name, text.size, len(sa.rounds), st.onew_passes, st.rebucket_1w))
    if name in LEAN:
        assert st.rebucket_1w == 1
    n = text.size
    assert O.check_sa(text, sa.local_SA, sa.local_B) == 0
    kasai = O.kasai(text, sa.local_SA, sa.local_B)
    assert np.array_equal(kasai, sa.local_LCP)
    if name in ("mutated_many_unresolved", "dna_few_copies_8m"):
        assert len(sa.rounds) > 1
    if name.startswith("dna_buckets_across_tiles"):
        # (the SA is the text's only one by now, and the LCP array the oracle's) some bucket of the first round -- neighbours that share a whole
        # window -- lies across an odd multiple of the scan tile, and some across a multiple of two tiles
        across = kasai >= 2 * sa.k
        assert across[4096::8192].any() and across[8192::8192].any()
    if name == "dna_short_tail_pairs_8m":
        # every short suffix n - 40 + i, i <= 20, sorts right before its long twin, and their LCP is the short one's length
        assert 2 * sa.k > TAIL_LEN
        for i in range(0, TAIL_LEN - 19):
            r = int(sa.local_B[n - TAIL_LEN + i])
            assert int(sa.local_SA[r + 1]) == TAIL_AT + i and int(sa.local_LCP[r + 1]) == TAIL_LEN - i
    SA, B, LCP, rounds = sa.local_SA.copy(), sa.local_B.copy(), sa.local_LCP.copy(), list(sa.rounds)
    monkeypatch.setenv("PSACX_GENERIC_REBUCKET", "1")
    gen = _run(ctx, text)
    assert ctx.stats().rebucket_1w == 0
    assert np.array_equal(gen.local_SA, SA) and np.array_equal(gen.local_B, B) and np.array_equal(gen.local_LCP, LCP)
    assert list(gen.rounds) == rounds
