"""The host model of the maximal exact matches (tests/mems_model.py) against itself: the shell walk of include/psacx.h ("maximal exact
matches") gives what the byte definition gives, the rule for PSACX_MEMS_SUPER gives the matches contained in no other, the order is
the pinned one, and the named cases of tests/golden/mems_named.json hold the values stated here by hand."""
import numpy as np
import pytest

import mems_model as X
import repeats_model as R


def random_case(rng):
    sigma = int(rng.randint(1, 5))
    letters = b"ACGT"[:sigma]
    word = lambda lo, hi: bytes(letters[i] for i in rng.randint(0, sigma, int(rng.randint(lo, hi + 1))))  # noqa: E731
    strings = [word(1, 14) for _ in range(int(rng.randint(1, 6)))]
    pats = [word(0, 12) for _ in range(int(rng.randint(1, 5)))]
    if rng.randint(0, 3) == 0:
        pats.insert(int(rng.randint(0, len(pats) + 1)), b"")
    if rng.randint(0, 3) == 0:
        pats.append(word(1, 1))
    if rng.randint(0, 2) == 0:                             # a piece of the text, so that long matches exist
        s = strings[int(rng.randint(0, len(strings)))]
        a = int(rng.randint(0, len(s)))
        pats.append(s[a:a + int(rng.randint(1, 9))])
    return strings, pats


def arrays_of(strings):
    t, off, SA, LCP = R.arrays_by_definition(strings)
    bwt, first, _ = R.bwt_of(t, SA, off)
    return t, off, SA, LCP, bwt, first


@pytest.mark.parametrize("block", range(6))
def test_the_walk_gives_the_byte_definition(block):
    rng = np.random.RandomState(100 + block)
    seen = 0
    for _ in range(50):
        strings, pats = random_case(rng)
        t, off, SA, LCP, bwt, first = arrays_of(strings)
        stats = X.statistics(t, SA, pats, off)
        for min_len in (1, 2, 3):
            for max_occ in (0, 1, 3):
                got, work = X.by_walk(SA, LCP, bwt, first, pats, stats, min_len, max_occ)
                want = X.by_bytes(strings, pats, min_len, max_occ)
                assert len(got) == len(set(got)) and set(got) == want, (strings, pats, min_len, max_occ)
                assert X.in_order(got, SA)
                assert work[1] >= len(got) and work[0] <= work[1]
                if max_occ == 0:
                    free = work
                else:
                    assert work[0] <= free[0] and work[1] <= free[1]
                seen += len(got)
    assert seen > 1000


@pytest.mark.parametrize("block", range(4))
def test_the_super_rule_gives_the_matches_contained_in_no_other(block):
    rng = np.random.RandomState(200 + block)
    for _ in range(50):
        strings, pats = random_case(rng)
        t, off, SA, LCP, bwt, first = arrays_of(strings)
        stats = X.statistics(t, SA, pats, off)
        for min_len in (1, 2, 3):
            for max_occ in (0, 1, 3):
                got, work = X.by_walk(SA, LCP, bwt, first, pats, stats, min_len, max_occ, super=True)
                want = X.supermaximal(X.by_bytes(strings, pats, min_len, max_occ), pats)
                assert len(got) == len(set(got)) and set(got) == want, (strings, pats, min_len, max_occ)
                assert X.in_order(got, SA) and work[1] == len(got)


def test_one_text_is_the_set_of_one_string():
    rng = np.random.RandomState(7)
    for _ in range(30):
        strings, pats = random_case(rng)
        strings = strings[:1]
        t, off, SA, LCP, bwt, first = arrays_of(strings)
        a = X.by_walk(SA, LCP, bwt, first, pats, X.statistics(t, SA, pats, None), 2)
        b = X.by_walk(SA, LCP, bwt, first, pats, X.statistics(t, SA, pats, off), 2)
        assert a == b and set(a[0]) == X.by_bytes(strings, pats, 2)


def test_a_statistic_longer_than_its_pattern_is_cut_and_a_broken_interval_gives_no_shell():
    t, off, SA, LCP, bwt, first, pats = X.named_arrays("mississippi")
    ln, lb, ub = (a.copy() for a in X.statistics(t, SA, pats))
    want = X.by_walk(SA, LCP, bwt, first, pats, (ln, lb, ub), 1)
    ends = {p: p1 for p, _, p1 in X.slots_of(pats)}
    cut, _ = X.by_walk(SA, LCP, bwt, first, pats, (ln + 100, lb, ub), 1)
    assert cut and all(l >= 1 and p + l <= ends[p] for p, _, l in cut)
    lb[3], ub[3] = ub[3], lb[3]
    ub[9] = len(t) + 1
    got, _ = X.by_walk(SA, LCP, bwt, first, pats, (ln, lb, ub), 1)
    assert got == [r for r in want[0] if r[0] not in (3, 9)]


def test_named_cases_hold_the_values_stated_by_hand():
    g = X.golden()
    for name in X.NAMED:
        assert g[name] == X.named_results(name), name      # the file is what the model writes
    mi = g["mississippi"]                                  # patterns ississim (slots 0-7) and sip (slots 8-10)
    assert [len(mi["mems%d" % k]["triples"]) for k in (1, 2, 3)] == [24, 5, 4]
    assert mi["mems3"]["triples"] == [[0, 1, 7], [0, 4, 4], [3, 1, 4], [8, 6, 3]]
    assert [mi["mems%d" % k]["work"] for k in (1, 2, 3)] == [[23, 39], [12, 15], [8, 10]]
    assert mi["super1"]["triples"] == [[0, 1, 7], [7, 0, 1], [8, 6, 3]]
    a = g["a20"]                                           # a^20 with the pattern a^8
    assert len(a["mems2"]["triples"]) == 25 and a["mems2"]["work"] == [28, 133]
    strings, pats = X.NAMED["mississippi"]
    assert set(map(tuple, mi["mems1"]["triples"])) == X.by_bytes(strings, pats, 1)
    assert set(map(tuple, a["mems2"]["triples"])) == X.by_bytes(*X.NAMED["a20"], min_len=2)


def test_cli_text():
    strings, pats = [b"abcab", b"cab"], [b"bcabc", b"", b"ca"]
    t, off, SA, LCP, bwt, first = arrays_of(strings)
    got, _ = X.by_walk(SA, LCP, bwt, first, pats, X.statistics(t, SA, pats, off), 2)
    assert got == [(0, 1, 4), (1, 5, 3), (2, 0, 3), (5, 2, 2), (5, 5, 2)]
    assert X.cli_text(got, pats, off) == "0 0 0 1 4\n0 1 1 0 3\n0 2 0 0 3\n2 0 0 2 2\n2 0 1 0 2\n"
