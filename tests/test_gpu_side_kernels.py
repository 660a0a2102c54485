"""The tile histograms of the top digit and the tie scan of the one-word first round run persistent kernels (top_digit_hist_waves_kernel,
tie_resolve_1w_waves_kernel: DESIGN.md 3.2, 3.6); PSACX_PLAIN_SIDE_KERNELS=1 pins the kernels with one workgroup per tile they replace.
A wrong histogram table makes the pass on the top digit write outside its buckets, so the table is compared first, by a program of its
own that launches nothing but the two histogram kernels (tests/cpp/top_digit_hist_parity.hip, built with the library).  Then every text is
constructed twice, by default and with the option, and SA, ISA, LCP and the log of the rounds must agree; the default run is also checked on
its own (order property + Kasai).  64-bit indices, LCP on, PSACX_ONE_WORD_MIN=21; the texts are at 2^23 characters, the smallest size at
which the one-word sort runs."""
import os
import subprocess

import numpy as np
import pytest

import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "psac_amd", "bin", "top_digit_hist_parity")
TIE_TILE = 8192


def test_top_digit_hist_tables_agree():
    # (first in the file: before the constructions below scatter by the new kernel's table)
    r = subprocess.run([PARITY], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    print(out[-3000:])
    assert r.returncode == 0, out[-3000:]


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


# ---- the seven texts of test_gpu_rebucket_1w.py that reach the one-word sort (copied, not imported): tie groups of 2 .. 8, groups across tile
# borders, short suffixes that tie with long ones, one, two and seven bits per character
def _dna_copied_stretch(n, seed, src, dst):
    # one stretch of 5000 characters at a second place: about 4900 buckets of two suffixes each, spread over the sorted order
    t = inputs.dna(n, seed).copy()
    t[dst:dst + 5000] = t[src:src + 5000]
    return t


def _two_symbols_even(n, seed):
    # one bit per character, both symbols as often: 32-character leading parts, hardly any shared by more than two suffixes
    return np.where(inputs.splitmix64_stream(n, seed) & np.uint64(1), ord("b"), ord("a")).astype(np.uint8)


TAIL_AT, TAIL_LEN, TAIL_RUN = 1000003, 40, 22


def _dna_short_tail_pairs(n, seed):
    # the last 40 characters (shorter than a window) are those at TAIL_AT, where 22 'A' (the code the end of the text is padded with) follow:
    # short suffix n - 40 + i and long suffix TAIL_AT + i have the same packed window for i <= 20 and tie in a group of two
    t = inputs.dna(n, seed).copy()
    p, m, r = TAIL_AT, TAIL_LEN, TAIL_RUN
    t[p + m - 1] = ord("C")
    t[p + m:p + m + r] = ord("A")
    t[p + m + r] = ord("C")
    t[n - m:] = t[p:p + m]
    return t


def _dna_few_copies(n, seed):
    # 2000 stretches of 300 characters at a second place, every third at a third one too: tie groups of at most 6, refinement rounds follow
    t = inputs.dna(n, seed).copy()
    half = n // 2
    for r in range(2000):
        src = 1000 * r + 17
        t[half + 1000 * r + 5:half + 1000 * r + 305] = t[src:src + 300]
        if r % 3 == 0:
            t[half + half // 2 + 1000 * r + 11:half + half // 2 + 1000 * r + 311] = t[src:src + 300]
    return t


# ---- a group longer than eight: one stretch of 40 characters at 12 places.  The tie scan reports it (`big`), all ties take the radix path and
# the generic rebucket kernel follows
LONG_AT = [300007 + 650011 * i for i in range(12)]


def _dna_long_group(n, seed):
    t = inputs.dna(n, seed).copy()
    for p in LONG_AT[1:]:
        t[p:p + 40] = t[LONG_AT[0]:LONG_AT[0] + 40]
    return t


# ---- a group of two across a border of the tie scan's tiles (8192 places): the 40 characters at EDGE_SRC stand at EDGE_DST too.  Seed and
# places were picked on the host with the oracle: the two suffixes sort to the places 5 * 8192 - 1 and 5 * 8192 (asserted below) -- the byte
# before a tile and the byte after it, which the kernel loads on their own, and a leader whose group lies in the next workgroup's tile
EDGE_SEED, EDGE_SRC, EDGE_DST, EDGE_AT = 31, 980614, 5200169, 5 * TIE_TILE


def _dna_group_across_tie_tiles(n):
    t = inputs.dna(n, EDGE_SEED).copy()
    t[EDGE_DST:EDGE_DST + 40] = t[EDGE_SRC:EDGE_SRC + 40]
    return t


LEAN = {
    "dna_last_tile_of_3_8m": lambda: inputs.dna((1 << 23) + 4097 + 3, 21),
    "dna_one_short_of_16_8m": lambda: inputs.dna((1 << 23) + 8191, 22),
    "ascii128_lc7_8m": lambda: inputs.ascii128((1 << 23) + 1, 23),
    "two_symbols_even_lc1_8m": lambda: _two_symbols_even((1 << 23) + 3, 24),
    "dna_short_tail_pairs_8m": lambda: _dna_short_tail_pairs(1 << 23, 25),
    "dna_few_copies_8m": lambda: _dna_few_copies((1 << 23) + 1234, 26),
    "dna_buckets_across_tiles_8m": lambda: _dna_copied_stretch(1 << 23, 13, 300000, 5200169),
}
CASES = dict(LEAN)
CASES["dna_long_group_8m"] = lambda: _dna_long_group(1 << 23, 27)
CASES["dna_group_across_tie_tiles_8m"] = lambda: _dna_group_across_tie_tiles(1 << 23)


def _run(ctx, text):
    import psac_amd
    sa = psac_amd.SuffixArray(index_bits=64, lcp=True, ctx=ctx)
    sa.construct(text)
    return sa


@pytest.mark.parametrize("name", list(CASES))
def test_side_kernels_same_arrays(ctx, monkeypatch, name):
    text = CASES[name]()
    n = text.size
    monkeypatch.setenv("PSACX_ONE_WORD_MIN", "21")
    sa = _run(ctx, text)
    st = ctx.stats()
    print("%s: n %d, rounds %d, one-word passes %d, lean rebucket %d" % (name, n, len(sa.rounds), st.onew_passes, st.rebucket_1w))
    assert st.onew_passes > 0
    # the records stay one-word up to the rebucket kernel unless the tie scan met a group of more than eight
    assert st.rebucket_1w == (0 if name == "dna_long_group_8m" else 1)
    assert O.check_sa(text, sa.local_SA, sa.local_B) == 0
    kasai = O.kasai(text, sa.local_SA, sa.local_B)
    assert np.array_equal(kasai, sa.local_LCP)
    if name == "dna_buckets_across_tiles_8m":
        across = kasai >= 2 * sa.k
        assert across[4096::8192].any() and across[8192::8192].any()
    if name == "dna_long_group_8m":
        ranks = np.sort(sa.local_B[np.array(LONG_AT)].astype(np.int64))
        assert ranks[-1] - ranks[0] == len(LONG_AT) - 1 and (kasai[ranks[1:]] >= 40).all()          # twelve neighbours that share 40 characters
    if name == "dna_group_across_tie_tiles_8m":
        assert sorted((int(sa.local_B[EDGE_SRC]), int(sa.local_B[EDGE_DST]))) == [EDGE_AT - 1, EDGE_AT]
        assert kasai[EDGE_AT] >= 40
    SA, B, LCP, rounds = sa.local_SA.copy(), sa.local_B.copy(), sa.local_LCP.copy(), list(sa.rounds)
    monkeypatch.setenv("PSACX_PLAIN_SIDE_KERNELS", "1")
    plain = _run(ctx, text)
    assert ctx.stats().onew_passes > 0
    assert np.array_equal(plain.local_SA, SA) and np.array_equal(plain.local_B, B) and np.array_equal(plain.local_LCP, LCP)
    assert list(plain.rounds) == rounds
