"""The one-word prefix sort of the first round sorts the digits above the last 16 prefix bits most significant first and orders the groups
that agree in them on chip (group_sort16_kernel) -- inside the 256 buckets at 32 leading bits, inside 65 536 sub-buckets at 40.
The records it leaves must be those of the LSD passes, so every text is constructed twice, by default and with PSACX_LSD_BUCKET_PASSES=1,
and SA, ISA, LCP and the log of the rounds must agree.  psacx_stats.group_sort says what ran: 1 = groups sorted on chip, 2 = a group longer
than the cap (512) found, the digits sorted LSD inside the partition reached, 0 = the LSD passes.  Every case names the value it must see in
the default run (the pinned run must report 0), and the sizes of its groups are counted on the host first, so that a case cannot pass on
the path it was not written for.  PSACX_FIRST_LEAD=40 sorts a small text on the 40 leading bits of a text of 2^32 characters: the only way
to the sub-bucket passes at these sizes.  64-bit indices, LCP on, PSACX_ONE_WORD_MIN=21."""
import numpy as np
import pytest

import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

CAP = 512          # radix.hpp: GROUP_CAP


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


# ---- text makers (copied from test_gpu_rebucket_1w.py, not imported)
def _two_symbols(n, seed):
    # 90 % 'a': one bit per character, a few huge buckets and groups, long tie groups
    return np.where(inputs.splitmix64_stream(n, seed) % np.uint64(10) == 0, ord("b"), ord("a")).astype(np.uint8)


def _two_symbols_even(n, seed):
    return np.where(inputs.splitmix64_stream(n, seed) & np.uint64(1), ord("b"), ord("a")).astype(np.uint8)


TAIL_AT, TAIL_LEN, TAIL_RUN = 1000003, 40, 22


def _dna_short_tail_pairs(n, seed):
    # the last 40 characters (shorter than a window) are those at TAIL_AT, where 22 'A' (the code the end of the text is padded with) follow:
    # short suffix n - 40 + i and long suffix TAIL_AT + i have the same packed window for i <= 20 and tie; the stable order of the sort
    # and the length caps decide
    t = inputs.dna(n, seed).copy()
    p, m, r = TAIL_AT, TAIL_LEN, TAIL_RUN
    t[p + m - 1] = ord("C")
    t[p + m:p + m + r] = ord("A")
    t[p + m + r] = ord("C")
    t[n - m:] = t[p:p + m]
    return t


# ---- the groups of a text, on the host: the suffixes that agree in the leading `bits` bits of their packed prefix (characters coded in
# byte order with ceil(log2(sigma)) bits, most significant first, the end of the text padded with zeros)
def _group_sizes(text, bits):
    present = np.zeros(256, bool)
    present[np.unique(text)] = True
    code = (np.cumsum(present) - 1).astype(np.uint32)[text]
    sigma = int(present.sum())
    l = max(1, int(np.ceil(np.log2(sigma))))
    m = (bits + l - 1) // l
    padded = np.concatenate([code, np.zeros(m, np.uint32)]).astype(np.uint64)
    v = np.zeros(text.size, np.uint64)
    for j in range(m):
        v = (v << np.uint64(l)) | padded[j:j + text.size]
    v >>= np.uint64(l * m - bits)
    return np.bincount(v.astype(np.int64), minlength=1 << bits)


def _plant(n, seed, motif, want):
    # random DNA with `motif` at so many places that exactly `want` suffixes begin with it (counted, not assumed)
    t = inputs.dna(n, seed).copy()
    mo = np.frombuffer(motif.encode(), np.uint8)
    k = mo.size

    def count():
        hit = np.ones(n - k + 1, bool)
        for j in range(k):
            hit &= t[j:n - k + 1 + j] == mo[j]
        return int(hit.sum())
    at, have = 4099, count()
    while have < want:
        for _ in range(want - have):
            t[at:at + k] = mo
            at += 397
        have = count()
    assert have == want and at < n - 4096
    return t


def _planted_sub_bucket(n, seed):
    # case 6: an 8-character motif at 10 000 places: at 40 leading bits the sub-bucket of its 16 bits holds some 10 000 records -- three tiles,
    # the last one partial -- and its groups (12 characters) stay far below the cap
    return _plant(n, seed, "CGTTGCAT", 10000)


N6 = (1 << 22) + 1234
# (at its natural 32 leading bits a text of 2^22 characters does not take the one-word sort at all -- its bucket tables do not fit the sort's scratch,
#  test_gpu_rebucket_1w.py -- so the pair of the 256-bucket form is twice as long; PSACX_FIRST_LEAD=40 comes with the room its tables need)
N7 = (1 << 23) + 1234
# name -> (text, PSACX_FIRST_LEAD or None, PSACX_ONE_WORD_ALWAYS, group_sort expected, bits above the last 16 of the prefix, oracle check)
CASES = {
    "dna_last_tile_of_3": (lambda: inputs.dna((1 << 23) + 4097 + 3, 21), None, False, 1, 16, True),
    "dna_groups_of_256": (lambda: inputs.dna((1 << 24) - 1, 22), None, False, 1, 16, False),
    "ascii128_lc7": (lambda: inputs.ascii128((1 << 23) + 1, 23), None, False, 1, 16, False),
    "two_symbols_even_lc1": (lambda: _two_symbols_even((1 << 23) + 3, 24), None, False, 1, 16, False),
    "dna_last_tile_of_3_lead40": (lambda: inputs.dna((1 << 23) + 4097 + 3, 21), 40, False, 1, 24, False),
    "ascii128_lc7_lead40": (lambda: inputs.ascii128((1 << 23) + 1, 23), 40, False, 1, 24, False),
    "planted_sub_bucket_lead40": (lambda: _planted_sub_bucket(N6, 31), 40, False, 1, 24, False),
    "planted_group_cap_lead40": (lambda: _plant(N6, 32, "CGTTGCATTACG", CAP), 40, False, 1, 24, False),
    "planted_group_cap_plus_1_lead40": (lambda: _plant(N6, 32, "CGTTGCATTACG", CAP + 1), 40, False, 2, 24, False),
    "planted_group_cap_lead32": (lambda: _plant(N7, 33, "CGTTGCAT", CAP), None, False, 1, 16, False),
    "planted_group_cap_plus_1_lead32": (lambda: _plant(N7, 33, "CGTTGCAT", CAP + 1), None, False, 2, 16, False),
    "two_symbols_skewed_always": (lambda: _two_symbols((1 << 23) + 3, 24), None, True, 2, 16, False),
    "dna_short_tail_pairs": (lambda: _dna_short_tail_pairs(1 << 23, 25), None, False, 1, 16, True),
    "dna_short_tail_pairs_lead40": (lambda: _dna_short_tail_pairs(1 << 23, 25), 40, False, 1, 24, False),
}


def _run(ctx, text):
    import psac_amd
    sa = psac_amd.SuffixArray(index_bits=64, lcp=True, ctx=ctx)
    sa.construct(text)
    return sa


@pytest.mark.parametrize("name", list(CASES))
def test_group_sort_same_arrays(ctx, monkeypatch, name):
    make, lead, always, expect, gbits, oracle = CASES[name]
    text = make()
    n = text.size
    # the condition the case is named for holds on the host: the largest group against the cap
    sizes = _group_sizes(text, gbits)
    largest = int(sizes.max())
    print("%s: n %d, largest group of %d bits %d, groups %d" % (name, n, gbits, largest, int((sizes > 0).sum())))
    assert (largest <= CAP) == (expect == 1)
    if name.startswith("planted_group_cap"):
        assert largest == (CAP if expect == 1 else CAP + 1)
    if name == "planted_sub_bucket_lead40":
        sub = int(_group_sizes(text, 16).max())
        assert 8192 < sub < 12288 and sub % 4096 != 0            # three tiles of 4096 records, the last one partial
    monkeypatch.setenv("PSACX_ONE_WORD_MIN", "21")
    if lead:
        monkeypatch.setenv("PSACX_FIRST_LEAD", str(lead))
    if always:
        monkeypatch.setenv("PSACX_ONE_WORD_ALWAYS", "1")
    sa = _run(ctx, text)
    st = ctx.stats()
    print("%s: rounds %d, one-word passes %d, group_sort %d" % (name, len(sa.rounds), st.onew_passes, st.group_sort))
    assert st.onew_passes > 0
    assert st.group_sort == expect
    if oracle:
        assert O.check_sa(text, sa.local_SA, sa.local_B) == 0
        assert np.array_equal(O.kasai(text, sa.local_SA, sa.local_B), sa.local_LCP)
    if name.startswith("dna_short_tail_pairs"):
        # every short suffix n - 40 + i, i <= 20, sorts right before its long twin, and their LCP is the short one's length
        assert 2 * sa.k > TAIL_LEN
        for i in range(0, TAIL_LEN - 19):
            r = int(sa.local_B[n - TAIL_LEN + i])
            assert int(sa.local_SA[r + 1]) == TAIL_AT + i and int(sa.local_LCP[r + 1]) == TAIL_LEN - i
    SA, B, LCP, rounds = sa.local_SA.copy(), sa.local_B.copy(), sa.local_LCP.copy(), list(sa.rounds)
    monkeypatch.setenv("PSACX_LSD_BUCKET_PASSES", "1")
    lsd = _run(ctx, text)
    assert ctx.stats().group_sort == 0 and ctx.stats().onew_passes > 0
    assert np.array_equal(lsd.local_SA, SA) and np.array_equal(lsd.local_B, B) and np.array_equal(lsd.local_LCP, LCP)
    assert list(lsd.rounds) == rounds


@pytest.mark.parametrize("lead", [16, 36, 48, 40])
def test_first_lead_bounds(ctx, monkeypatch, lead):
    # PSACX_FIRST_LEAD is ignored when it is below bits(n - 1) + 3 (16), no multiple of 8 (36) or above 40 (48): arrays and round log are those
    # of the run without it.  40 is honoured on this text (word 1 of DNA holds 64 bits): more leading bits, the same arrays.
    text = inputs.dna((1 << 21) + 5, 41)
    monkeypatch.setenv("PSACX_ONE_WORD_MIN", "21")
    ref = _run(ctx, text)
    SA, B, LCP, rounds = ref.local_SA.copy(), ref.local_B.copy(), ref.local_LCP.copy(), list(ref.rounds)
    monkeypatch.setenv("PSACX_FIRST_LEAD", str(lead))
    sa = _run(ctx, text)
    assert np.array_equal(sa.local_SA, SA) and np.array_equal(sa.local_B, B) and np.array_equal(sa.local_LCP, LCP)
    if lead != 40:
        assert list(sa.rounds) == rounds
