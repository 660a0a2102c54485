"""The two statements of tests/docs_model.py agree: the strings that hold a word, read from the bytes, against prev / h / dup and the
formula of include/psacx.h ("document counts and document lists"); the golden file of the named sets; and the interval kind on which
the count formula is wrong, pinned as wrong.  No GPU."""
import numpy as np

import docs_model as D
import repeats_model as M


def small_sets():
    out = [D.NAMED["miss"], D.NAMED["acgt3"], [b"a"], [b"ab", b"ab"], [b"abab", b"ab"], [b"aaaa", b"aa", b"a", b"aaa"], [b"banana", b"ananas", b"bandana", b"banana"]]
    for seed in range(60):
        rng = np.random.RandomState(1000 + seed)
        n, sigma = int(rng.randint(2, 40)), int(rng.randint(1, 4))
        s = M.random_set(n, int(rng.randint(1, min(n, 9) + 1)), seed, sigma=sigma)
        if seed % 3 == 0:                              # duplicate strings
            s = s + [s[0]] + s[-1:]
        out.append(s)
    return out


def check_set(strings, lists_seed):
    """number of LCP-intervals checked"""
    t, off, SA, LCP = M.arrays_by_definition(strings)
    n, m = int(t.size), len(strings)
    prev, dup = D.index_of(SA, LCP, off)
    assert dup[0] == 0 and dup[n] == n - m and (n == 0 or D.h_of(prev, LCP)[0] == 0)
    ivs = D.lcp_intervals(LCP)
    lb, ub = np.array([i[0] for i in ivs], np.int64), np.array([i[1] for i in ivs], np.int64)
    got = D.count_by_dup(dup, lb, ub, n)
    assert np.array_equal(got, (ub - lb) - (dup[ub] - dup[lb + 1]))            # on LCP-intervals the clamps do nothing
    for (a, b, ln), g in zip(ivs, got.tolist()):
        assert D.is_lcp_interval(LCP, a, b), (strings, a, b)
        by_ranks = D.docs_of_ranks(SA, off, a, b)
        if ln >= 0:                                    # an inner node or the root: the strings that hold the word
            assert by_ranks == D.docs_by_bytes(strings, t[SA[a]:SA[a] + ln].tobytes()), (strings, a, b)
        assert g == len(by_ranks), (strings, a, b, g, by_ranks)
    # lists: any interval
    qa, qb = D.random_intervals(n, 40, lists_seed)
    qa, qb = np.concatenate((qa, lb)), np.concatenate((qb, ub))
    start, ranks, sid, pos = D.list_by_prev(prev, SA, off, qa, qb, n)
    for j, (a, b) in enumerate(zip(qa.tolist(), qb.tolist())):
        want = D.list_of_ranks(SA, off, a, b)
        s, e = int(start[j]), int(start[j + 1])
        assert ranks[s:e].tolist() == [r for r, _, _ in want], (strings, a, b)
        assert sid[s:e].tolist() == [x for _, x, _ in want] and pos[s:e].tolist() == [p for _, _, p in want]
    return len(ivs)


def test_counts_and_lists_agree_with_the_bytes():
    total = sum(check_set(s, 7 + k) for k, s in enumerate(small_sets()))
    assert total > 1500


def test_w257():
    assert check_set(D.NAMED["w257"], 3) > 2000


def test_totality_of_the_count_formula():
    rng = np.random.RandomState(5)
    n = 50
    dup = rng.randint(0, 1 << 30, n + 1)               # not monotone
    lb, ub = D.random_intervals(n, 400, 9)
    lb, ub = np.concatenate((lb, [3, 0, 7])), np.concatenate((ub, [2, n + 1, 7]))
    got = D.count_by_dup(dup, lb, ub, n)
    ok = (lb < ub) & (ub <= n)
    assert np.all(got[~ok] == 0) and np.all((got[ok] >= 1) & (got[ok] <= (ub - lb)[ok]))


def test_the_count_formula_is_wrong_on_an_overlaps_interval():
    # the suffixes that ARE "ab" (psacx_overlaps_*: T(j, d)): ranks [0, 2), followed by "abab", so L[ub] equals the inner value and the
    # pair (0, 2) of the first string has its first minimum at rank 1, inside.  The header sends such callers to the list.
    strings = [b"abab", b"ab"]
    t, off, SA, LCP = M.arrays_by_definition(strings)
    assert SA.tolist() == [2, 4, 0, 3, 5, 1] and LCP.tolist() == [0, 2, 2, 0, 1, 1]
    assert not D.is_lcp_interval(LCP, 0, 2) and int(LCP[2]) == int(LCP[1])
    prev, dup = D.index_of(SA, LCP, off)
    assert D.docs_of_ranks(SA, off, 0, 2) == [0, 1]
    assert D.count_by_dup(dup, [0], [2], 6).tolist() == [1]                    # wrong, as the header says
    start, ranks, sid, pos = D.list_by_prev(prev, SA, off, [0], [2], 6)
    assert start.tolist() == [0, 2] and sid.tolist() == [0, 1] and pos.tolist() == [2, 4]


def test_golden_named_sets():
    gold = D.golden()
    assert sorted(gold) == sorted(D.NAMED)
    for name in D.NAMED:
        assert gold[name] == D.named_results(name), name
    rows = {bytes(r["pattern"]): r for r in gold["miss"]["patterns"]}
    assert rows[b"miss"]["docs"] == 3 and rows[b"ssi"]["docs"] == 1 and rows[b"ssi"]["ub"] - rows[b"ssi"]["lb"] == 2
    assert rows[b"x"]["docs"] == 0 and rows[b"x"]["lb"] == rows[b"x"]["ub"]
    assert rows[b"s"]["docs"] == 3 and rows[b"s"]["ub"] - rows[b"s"]["lb"] == 8 and rows[b"s"]["sid"] == [2, 0, 1]
    assert all(r["docs"] == 3 for r in gold["acgt3"]["patterns"][:3]) and gold["acgt3"]["patterns"][3]["docs"] == 0
    w = {bytes(r["pattern"]): r for r in gold["w257"]["patterns"]}
    assert w[b"GATTACA"]["docs"] == 257 and w[b"\x07"]["docs"] == 1 and w[b"ATTACAG"]["docs"] == 0
    # and by the index
    for name, strings in D.NAMED.items():
        t, off, SA, LCP = M.arrays_by_definition(strings)
        prev, dup = D.index_of(SA, LCP, off)
        lb = np.array([r["lb"] for r in gold[name]["patterns"]]); ub = np.array([r["ub"] for r in gold[name]["patterns"]])
        assert D.count_by_dup(dup, lb, ub, t.size).tolist() == [r["docs"] for r in gold[name]["patterns"]]
        start, ranks, sid, pos = D.list_by_prev(prev, SA, off, lb, ub, t.size)
        assert sid.tolist() == sum((r["sid"] for r in gold[name]["patterns"]), [])
        assert pos.tolist() == sum((r["pos"] for r in gold[name]["patterns"]), [])
