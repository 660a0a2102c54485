"""The tie stage of the one-word first round on the tie BITS the group sort leaves (psac_amd/csrc/tie_bits.hpp), against the oracle
and against the tie bytes it replaces (PSACX_TIE_BYTES=1, that is PSACX_OPT_PLAIN_SIDE_KERNELS = 2).

Random DNA with planted repeats, 2^23 characters at the natural 32 leading bits and 2^22 at 40 (PSACX_FIRST_LEAD=40: the sub-bucket passes, suffix
fields of 32 bits) -- the smallest texts whose first round takes the group form either way: at 32 leading bits a text of 2^22 characters does not
take the one-word sort at all, its bucket tables do not fit the sort's scratch (test_gpu_group_sort.py).  The planted repeats:
  - a stretch of 40 characters at g places for g = 2 .. 8: tie groups of 2 .. 8 members, some twenty of each;
  - in the second text a stretch at 9 places too: a group of 9, which the tie scan reports and all ties take the radix path;
  - T^16 ACGTAC at three places: nothing sorts behind T^16, so that group lies at the last places of the array;
  - GACG T^12 CATG at two places: the group at the end of the top-digit bucket GACG;
  - among the few thousand groups there are leaders at places 63 mod 64, the last bit of a word.
The host asserts these shapes on the oracle's arrays.  Every text is constructed by default -- psacx_stats.tie_form says the bits were read -- and with
the bytes pinned; SA, ISA, LCP and the round log must be the oracle's both times, and psacx_stats.rebucket_1w what it was: 1, and 0 behind the group
of 9.  64-bit indices, LCP on."""
import numpy as np
import pytest

import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

STRETCH = 40


def _place(i):
    return 70003 + 90001 * i


def _text(n, with_nine):
    t = inputs.dna(n, 61).copy()
    i = 0
    for g in list(range(2, 9)) + ([9] if with_nine else []):
        src = _place(i)
        for j in range(g):
            t[_place(i + j):_place(i + j) + STRETCH] = t[src:src + STRETCH]
        i += g
    lut = b"ACG"
    for j in range(3):                                   # (C before, a different character behind each)
        p = 33013 + 1000003 * j
        t[p:p + 24] = np.frombuffer(b"C" + b"T" * 16 + b"ACGTAC" + lut[j:j + 1], dtype=np.uint8)
    for j in range(2):
        p = 555557 + 2000003 * j
        t[p:p + 21] = np.frombuffer(b"GACG" + b"T" * 12 + b"CATG" + lut[j:j + 1], dtype=np.uint8)
    return t


LAST_AT = [33013 + 1000003 * j + 1 for j in range(3)]
BUCKET_END_AT = [555557 + 2000003 * j for j in range(2)]


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, logn, nine in (("groups_2_to_8", 23, False), ("group_of_9", 23, True), ("groups_2_to_8_lead40", 22, False)):
        text = _text(1 << logn, nine)
        out[name] = (text, O.construct(text, bits=64))
    return out


def _groups(lcp, chars):
    """leaders and sizes of the runs of neighbours that share `chars` characters"""
    tie = np.zeros(lcp.size + 1, dtype=bool)
    tie[1:lcp.size] = lcp[1:] >= chars
    lead = np.flatnonzero(~tie[:-1] & tie[1:])
    ends = np.flatnonzero(tie[:-1] & ~tie[1:])
    return lead, ends - lead + 1


def _run(ctx, text):
    import psac_amd
    sa = psac_amd.SuffixArray(index_bits=64, lcp=True, ctx=ctx)
    sa.construct(text)
    return sa


def _same(sa, ref):
    assert np.array_equal(sa.local_SA, ref["SA"]) and np.array_equal(sa.local_B, ref["ISA"]) and np.array_equal(sa.local_LCP, ref["LCP"])
    assert [(h, b, e) for (h, b, e, *_rest) in sa.rounds] == [(h, b, e) for h, b, e, _ in ref["trace"]]


@pytest.mark.parametrize("name,lead", [("groups_2_to_8", None), ("groups_2_to_8_lead40", 40), ("group_of_9", None)])
def test_tie_bits_same_arrays(ctx, cases, monkeypatch, name, lead):
    text, ref = cases[name]
    N = text.size
    chars = (lead or 32) // 2                          # two bits per character
    leaders, sizes = _groups(ref["LCP"], chars)
    have = set(int(x) for x in np.unique(sizes))
    print("%s, %d leading bits: %d groups, sizes %s, %d leaders at 63 mod 64" % (name, lead or 32, leaders.size, sorted(have), int((leaders % 64 == 63).sum())))
    assert set(range(2, 9)) <= have and max(have) == (9 if name == "group_of_9" else 8)
    assert (leaders % 64 == 63).any()
    isa = ref["ISA"]
    assert sorted(int(isa[p]) for p in LAST_AT) == [N - 3, N - 2, N - 1] and int(leaders[-1]) == N - 3 and int(sizes[-1]) == 3
    r = sorted(int(isa[p]) for p in BUCKET_END_AT)
    assert r[1] == r[0] + 1 and r[0] in leaders and bytes(text[int(ref["SA"][r[1] + 1]):][:4]) != b"GACG"
    monkeypatch.setenv("PSACX_ONE_WORD_MIN", "21")
    if lead:
        monkeypatch.setenv("PSACX_FIRST_LEAD", str(lead))
    sa = _run(ctx, text)
    st = ctx.stats()
    print("default: one-word passes %d, group_sort %d, tie_form %d, lean rebucket %d" % (st.onew_passes, st.group_sort, st.tie_form, st.rebucket_1w))
    assert st.onew_passes > 0 and st.group_sort == 1
    assert st.tie_form == 2
    lean = 0 if name == "group_of_9" else 1
    assert st.rebucket_1w == lean
    _same(sa, ref)
    monkeypatch.setenv("PSACX_TIE_BYTES", "1")
    by = _run(ctx, text)
    st = ctx.stats()
    print("bytes pinned: one-word passes %d, group_sort %d, tie_form %d, lean rebucket %d" % (st.onew_passes, st.group_sort, st.tie_form, st.rebucket_1w))
    assert st.onew_passes > 0 and st.group_sort == 1 and st.tie_form == 1 and st.rebucket_1w == lean
    _same(by, ref)
    assert np.array_equal(by.local_SA, sa.local_SA) and np.array_equal(by.local_B, sa.local_B) and np.array_equal(by.local_LCP, sa.local_LCP)
    assert list(by.rounds) == list(sa.rounds)
