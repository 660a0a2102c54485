"""The host model of the pattern search with mismatches (tests/kmismatch_model.py) against itself: the pipeline of include/psacx.h
("pattern search with mismatches": pieces, candidates, the first exact piece) gives what the comparison of every window gives, in the
pinned order, on the catalogue the GPU tests use and on random small sets; and the named cases of tests/golden/kmismatch_named.json
hold the values stated here by hand."""
import numpy as np
import pytest

import kmismatch_model as X
import repeats_model as R


def same(a, b):
    return all(x.size == y.size and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
@pytest.mark.parametrize("kind", X.TEXTS)
def test_the_pieces_give_what_the_windows_give_on_the_catalogue(kind, as_set):
    hits = 0
    for n in X.SIZES:
        c = X.case(kind, n, as_set)
        for e in (0, 1, 2, 3) + ((15,) if n == 65 else ()):
            pats = c.patterns(e)
            got, work = c.results(e)
            assert same(got, X.by_windows(c.text, c.off, c.SA, pats, e)), (kind, n, e)
            assert X.true_hits(c.text, c.off, pats, e, got)
            assert work[0] >= work[1] >= got[0].size
            hits += got[0].size
    assert hits > 100


@pytest.mark.parametrize("block", range(4))
def test_the_pieces_give_what_the_windows_give_on_random_sets(block):
    rng = np.random.RandomState(300 + block)
    seen = 0
    for _ in range(60):
        sigma = int(rng.randint(1, 4))
        word = lambda lo, hi: bytes(b"ACG"[i] for i in rng.randint(0, sigma, int(rng.randint(lo, hi + 1))))  # noqa: E731
        strings = [word(1, 14) for _ in range(int(rng.randint(1, 6)))]
        pats = [word(0, 12) for _ in range(int(rng.randint(1, 6)))]
        t, off, SA, _ = R.arrays_by_definition(strings)
        for e in (0, 1, 2, 3, 5):
            got, work = X.by_pieces(t, off, SA, pats, e)
            assert same(got, X.by_windows(t, off, SA, pats, e)), (strings, pats, e)
            assert all(len(pats[int(j)]) >= e + 1 for j in got[0])
            seen += got[0].size
    assert seen > 1000


def test_m_of_e_has_no_hits_and_m_of_e_plus_one_has_every_window_with_an_equal_byte():
    t, off, SA, pats = X.named_arrays("mississippi")
    for e in (1, 2, 3):
        got, work = X.by_pieces(t, None, SA, [b"sip"[:e], b"spmi"[:e + 1]], e)
        assert np.all(got[0] == 1)                            # m = e: nothing, and no candidate is counted for it
        P = b"spmi"[:e + 1]
        want = sorted(w for w in range(len(t) - e) if any(t[w + x] == P[x] for x in range(e + 1)))
        assert sorted(got[1].tolist()) == want
        assert work[0] == sum(int(np.sum(t == c)) for c in P)


def test_named_cases_hold_the_values_stated_by_hand():
    g = X.golden()
    for name in X.NAMED:
        assert g[name] == X.named_results(name), name         # the file is what the model writes
    mi = g["mississippi"]                                     # patterns issi, ssippx, m, "", sip
    assert mi["e0"]["triples"] == [[0, 4, 0], [0, 1, 0], [2, 0, 0], [4, 6, 0]]        # issi: issippi sorts before ississippi
    # one mismatch: ssippx is ssippi at 5; sip is sis at 3 (from its piece s, after the exact one at 6)
    assert mi["e1"]["triples"] == [[0, 4, 0], [0, 1, 0], [1, 5, 1], [4, 6, 0], [4, 3, 1]]
    assert mi["e1"]["work"] == [11, 11]
    assert [2, 0, 0] not in mi["e1"]["triples"]               # m (one byte) is shorter than e + 1
    ab = g["abcab_cab"]                                       # the set abcab, cab; patterns cab, abc, bc, cb, abcabc
    # bc occurs at 1 only: the bytes at 4 and 5 are b and c of two strings.  abcabc would be the two strings laid together.
    assert ab["e0"]["triples"] == [[0, 2, 0], [0, 5, 0], [1, 0, 0], [2, 1, 0]]
    # cb with one mismatch: ca at 2 and 5 from the piece c, then ab at 3, 6 and 0 from the piece b in suffix order (b, b, bcab)
    assert ab["e1"]["triples"][4:] == [[3, 2, 1], [3, 5, 1], [3, 3, 1], [3, 6, 1], [3, 0, 1]]
    assert ab["e1"]["work"] == [21, 13] and ab["e2"]["triples"] == [[0, 2, 0], [0, 5, 0], [1, 0, 0]]
