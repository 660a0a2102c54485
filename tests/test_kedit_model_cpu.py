"""The host model of the pattern search with edits (tests/kedit_model.py) against itself: the pipeline of include/psacx.h ("pattern
search with edits": pieces, candidates, the starts around the diagonal, the banded programme, the unique) gives what the full dynamic
programme from every start gives, on the catalogue the GPU tests use and on random small sets; e = 0 is the sorted occurrences;
every hit of the search with mismatches is a hit here with at most its distance; PSACX_KEDIT_BEST is held to a direct statement; and
the named cases of tests/golden/kedit_named.json hold the values stated here by hand."""
import numpy as np
import pytest

import kedit_model as K
import kmismatch_model as X
import locate_gsa_model as G
import locate_model as L
import repeats_model as R

SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 257]


def same(a, b):
    return all(x.size == y.size and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
@pytest.mark.parametrize("kind", K.TEXTS)
def test_the_pieces_give_what_the_definition_gives_on_the_catalogue(kind, as_set):
    hits = 0
    for n in SIZES:
        c = K.case(kind, n, as_set)
        for e in (0, 1, 2, 3):
            pats = K.patterns(c, e)
            got, work = K.results(c, e)
            assert same(got, K.by_definition(c.text, c.off, pats, e)), (kind, n, e)
            assert K.true_hits(c.text, c.off, pats, e, got)
            assert work[1] >= got[0].size and all(len(pats[int(j)]) > e for j in got[0])
            assert np.all(got[3] <= e) and np.all(np.abs(got[2] - np.array([len(pats[int(j)]) for j in got[0]], np.int64)) <= got[3])
            hits += got[0].size
    assert hits > 100


@pytest.mark.parametrize("block", range(4))
def test_the_pieces_give_what_the_definition_gives_on_random_sets(block):
    rng = np.random.RandomState(500 + block)
    seen = 0
    for _ in range(60):
        sigma = int(rng.randint(1, 4))
        word = lambda lo, hi: bytes(b"ACG"[i] for i in rng.randint(0, sigma, int(rng.randint(lo, hi + 1))))  # noqa: E731
        strings = [word(1, 14) for _ in range(int(rng.randint(1, 6)))]
        pats = [word(0, 12) for _ in range(int(rng.randint(1, 6)))]
        t, off, SA, _ = R.arrays_by_definition(strings)
        for e in (0, 1, 2, 3, 4):
            got, work = K.by_pieces(t, off, SA, pats, e)
            assert same(got, K.by_definition(t, off, pats, e)), (strings, pats, e)
            seen += got[0].size
    assert seen > 1000


@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
def test_no_edits_are_the_sorted_occurrences(as_set):
    for kind in K.TEXTS:
        for n in (33, 257):
            c = K.case(kind, n, as_set)
            pats = K.patterns(c, 0)
            got, work = K.results(c, 0)
            s = c.text.tobytes()
            want = []
            for j, P in enumerate(pats):
                if len(P) == 0:
                    continue
                lb, ub = L.by_bisection(s, c.SA, P) if c.off is None else G.by_bisection(s, c.off, c.SA, P, end=G.ends_of(c.off, n))
                want += [(j, int(p), len(P), 0) for p in sorted(c.SA[lb:ub].tolist())]
            assert [tuple(r) for r in zip(*(a.tolist() for a in got))] == want, (kind, n)


@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
def test_every_hit_with_mismatches_is_a_hit_with_edits_at_no_greater_distance(as_set):
    seen = 0
    for kind in K.TEXTS:
        c = K.case(kind, 257, as_set)
        for e in (1, 2, 3):
            pats = c.patterns(e)                               # the patterns of the search with mismatches
            (qid, tpos, dist), _ = c.results(e)
            got = K.by_pieces(c.text, c.off, c.SA, pats, e)[0]
            mine = {(int(j), int(t)): int(d) for j, t, _, d in zip(*got)}
            for j, t, d in zip(qid.tolist(), tpos.tolist(), dist.tolist()):
                assert (j, t) in mine and mine[(j, t)] <= d, (kind, e, j, t, d)
                seen += 1
    assert seen > 100


def test_best_against_a_direct_statement():
    kept = dropped = 0
    for kind in K.TEXTS:
        c = K.case(kind, 257, False)
        pats = K.patterns(c, 2)
        got = K.results(c, 2)[0]
        b = K.best(got)
        rows, rows_b = list(zip(*(a.tolist() for a in got))), list(zip(*(a.tolist() for a in b)))
        for j in set(got[0].tolist()):
            mine = [r for r in rows if r[0] == j]
            least = min(r[3] for r in mine)
            assert [r for r in rows_b if r[0] == j] == [r for r in mine if r[3] == least]
        kept, dropped = kept + len(rows_b), dropped + len(rows) - len(rows_b)
    assert kept > 50 and dropped > 50


def test_named_cases_hold_the_values_stated_by_hand():
    g = K.golden()
    for name in K.NAMED:
        assert g[name] == K.named_results(name), name         # the file is what the model writes
    mi = g["mississippi"]                                     # patterns issi, ssippx, m, "", sip
    assert mi["e0"]["quadruples"] == [[0, 1, 4, 0], [0, 4, 4, 0], [2, 0, 1, 0], [4, 6, 3, 0]]
    # one edit: issi at 1 and 4 bring the starts beside them (ssi at 2 and 5, and sissi / ississ at 3 ...); ssippx is ssipp at 5
    e1 = mi["e1"]["quadruples"]
    assert [r for r in e1 if r[0] == 1] == [[1, 5, 5, 1]]
    assert [0, 1, 4, 0] in e1 and [0, 4, 4, 0] in e1 and [0, 2, 3, 1] in e1 and [0, 5, 3, 1] in e1 and [0, 0, 5, 1] in e1
    assert not [r for r in e1 if r[0] in (2, 3)]              # m (one byte) and the empty pattern have m <= e
    assert [r for r in e1 if r[0] == 4 and r[3] == 0] == [[4, 6, 3, 0]]
    ab = g["abcab_cab"]                                       # the set abcab, cab; patterns cab, abc, bc, cb, abcabc
    assert ab["e0"]["quadruples"] == [[0, 2, 3, 0], [0, 5, 3, 0], [1, 0, 3, 0], [2, 1, 2, 0]]
    # abcabc with one edit is the whole first string (its last byte deleted), never the two strings laid together
    assert [r for r in ab["e1"]["quadruples"] if r[0] == 4] == [[4, 0, 5, 1]]
    assert all(r[1] + r[2] <= (5 if r[1] < 5 else 8) for e in ("e0", "e1", "e2") for r in ab[e]["quadruples"])
