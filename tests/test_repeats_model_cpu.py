"""The host model of the BWT and repeat calls (tests/repeats_model.py) against itself, without a GPU: the three formulations of the
right-maximal, maximal and supermaximal repeats agree on random texts and string sets -- every substring with unique sentinels, the
stack traversal of the LCP-intervals, and the per-rank searches with the bit arrays D, F and St that the kernel is written to --,
the BWT inverts, the named results of tests/golden/repeats_named.json are the ones stated by hand in the issue, and
psac_amd.bwt_decode is the model's inverse."""
import numpy as np
import pytest

import repeats_model as M


def random_cases():
    rng = np.random.RandomState(2004)
    for it in range(300):
        sigma, m = 1 + it % 4, 1 + (it // 4) % 8
        n = int(rng.randint(m, 41))
        yield M.random_set(n, m, 1000 + it, sigma)


def test_the_three_formulations_agree_on_random_texts_and_sets():
    seen = {M.RIGHT: 0, M.MAXIMAL: 0, M.SUPER: 0}
    for strings in random_cases():
        t, off, SA, LCP = M.arrays_by_definition(strings)
        bwt, first, _ = M.bwt_of(t, SA, off)
        a = M.by_bytes(strings)
        for kind in (M.RIGHT, M.MAXIMAL, M.SUPER):
            b = M.by_intervals(LCP, bwt, first, kind)
            c = M.by_searches(LCP, bwt, first, kind)
            assert b == c, (strings, kind)
            assert len(b) == len(a[kind]) and M.as_occurrences(b, SA) == a[kind], (strings, kind)
            assert all(0 <= lb < h < ub <= len(SA) and ub - lb >= 2 and ln >= 1 for h, lb, ub, ln in b)
            seen[kind] += len(b)
    assert min(seen.values()) > 300                    # (the cases are not empty of repeats)


@pytest.mark.parametrize("kind", ["a", "fib", "dna2", "tandem7", "bytes256"])
def test_intervals_and_searches_agree_beyond_the_byte_model(kind):
    t = M.text_of(kind, 300, 5)
    _, off, SA, LCP = M.arrays_by_definition([t.tobytes()])
    bwt, first, _ = M.bwt_of(t, SA)
    for k in (M.RIGHT, M.MAXIMAL, M.SUPER):
        assert M.by_intervals(LCP, bwt, first, k) == M.by_searches(LCP, bwt, first, k)
    if kind == "a":                                    # n - 1 nested maximal repeats that all end at n, one supermaximal
        assert M.by_intervals(LCP, bwt, first, M.MAXIMAL) == [(j, j - 1, 300, j) for j in range(1, 300)]
        assert M.by_intervals(LCP, bwt, first, M.SUPER) == [(299, 298, 300, 299)]


def test_the_bwt_inverts():
    rng = np.random.RandomState(7)
    for it in range(200):
        n = int(rng.randint(1, 60))
        t = np.frombuffer(b"ab\xff\x00", np.uint8)[rng.randint(0, 1 + it % 4, n)]
        _, _, SA, _ = M.arrays_by_definition([t.tobytes()])
        bwt, first, primary = M.bwt_of(t, SA)
        assert int(SA[primary]) == 0 and first.sum() == 1 and first[primary]
        assert M.inverse_bwt(bwt, primary) == t.tobytes()
    bwt, _, primary = M.bwt_of(np.frombuffer(b"banana", np.uint8), [5, 3, 1, 0, 4, 2])
    assert bwt.tobytes() == b"nnbaaa" and primary == 3


def test_the_bwt_of_a_set_is_cyclic_per_string():
    t, off, SA, LCP = M.arrays_by_definition([b"abcab", b"cab"])
    bwt, first, primary = M.bwt_of(t, SA, off)
    # suffixes: ab(3) ab(6) abcab(0) b(4) b(7) bcab(1) cab(2) cab(5)
    assert SA.tolist() == [3, 6, 0, 4, 7, 1, 2, 5] and LCP.tolist() == [0, 2, 2, 0, 1, 1, 0, 3]
    assert bwt.tobytes() == b"ccbaaabb" and first.tolist() == [0, 0, 1, 0, 0, 0, 0, 1] and primary == 2


def test_the_named_results_are_the_ones_stated_by_hand():
    g = M.golden()
    for name in M.NAMED:
        assert g[name] == M.named_results(name), name
    mi = g["mississippi"]
    assert mi["SA"] == [10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2] and mi["LCP"] == [0, 1, 1, 4, 0, 0, 1, 0, 2, 1, 3]
    assert M.words("mississippi", mi["right"]) == ["i x4", "issi x2", "p x2", "s x4", "si x2", "ssi x2"]
    # i = SA[0:4) = {10, 7, 4, 1}: rank 4 is the whole text, which starts with m
    assert mi["maximal"] == [[0, 4, 1], [2, 4, 4], [5, 7, 1], [7, 11, 1]]
    assert M.words("mississippi", mi["super"]) == ["issi x2", "p x2"]
    ba = g["banana"]
    assert M.words("banana", ba["maximal"]) == ["a x3", "ana x2"] and M.words("banana", ba["super"]) == ["ana x2"]
    ab = g["abcab_cab"]
    assert M.words("abcab_cab", ab["right"]) == ["ab x3", "b x3", "cab x2"]
    assert M.words("abcab_cab", ab["maximal"]) == ["ab x3", "cab x2"] and M.words("abcab_cab", ab["super"]) == ["cab x2"]
    aa = g["aaaa"]
    assert M.words("aaaa", aa["maximal"]) == ["a x4", "aa x3", "aaa x2"] and M.words("aaaa", aa["super"]) == ["aaa x2"]


def test_the_filters():
    r = M.by_intervals(M.golden()["mississippi"]["LCP"])
    assert M.select(r) == M.select(r, 1, 2, 0) == r
    assert [x[1:] for x in M.select(r, min_len=2)] == [(2, 4, 4), (7, 9, 2), (9, 11, 3)]          # issi, si, ssi
    assert [x[1:] for x in M.select(r, min_occ=3)] == [(0, 4, 1), (7, 11, 1)]
    assert [x[1:] for x in M.select(r, max_occ=2, min_len=3)] == [(2, 4, 4), (9, 11, 3)]


def test_bwt_decode_is_the_models_inverse():
    import psac_amd
    for kind in ("dna4", "fib", "bytes256", "a"):
        t = M.text_of(kind, 777, 3)
        _, _, SA, _ = M.arrays_by_definition([t.tobytes()])
        bwt, _, primary = M.bwt_of(t, SA)
        assert psac_amd.bwt_decode(bwt, primary) == M.inverse_bwt(bwt, primary) == t.tobytes()
    assert psac_amd.bwt_decode(np.zeros(0, np.uint8), 0) == b""
