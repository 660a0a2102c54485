"""The host model of the two GPU checkers (tests/checker_model.py) and its catalogue of wrong arrays, without a GPU:
the model accepts the oracle's arrays, sees every mutant of the catalogue, agrees with the reference restatement's own
checker and with a scalar restatement of the definitions, and gives the hand-computed counts of the two cases where
only the anchors of the LCP recurrence can object."""
import numpy as np
import pytest

import checker_model as M
import inputs
import oracle_lib as O

from checker_model import BIG, TINY, arrays, truth_of

LAYOUTS = [(1, 7), (3, 7), (8, 7), (1, 40)]


def all_mutants(name, layouts=LAYOUTS, every_edge=False):
    """(class, where, arrays, Truth) for every class at every position of a text; arrays None where a class cannot apply."""
    text, SA, ISA, LCP, tr = arrays(name)
    pos = M.positions(text.size, LCP, layouts, every_edge=every_edge)
    where = sorted({w for v in pos.values() for w in v})
    for cls in M.MUTANTS:
        for w in (where if cls in M.POSITIONAL else [0]):
            r = M.mutate(cls, text, SA, ISA, LCP, w)
            yield cls, w, r, (None if r is None else tr if cls != "Text" else truth_of(r[0]))


def scalar_model(text, SA, ISA, LCP, distributed):
    """The definitions of include/psacx.h entry by entry, Python integers, naive minima."""
    n = len(text)
    t = [int(x) for x in text]; sa = [int(x) for x in SA]; isa = [int(x) for x in ISA]
    lcp = None if LCP is None else [int(x) for x in LCP]
    e = [0, 0, 0, 0]
    for i in range(n):
        b = sa[i]
        if b >= n or isa[b] != i:
            e[0] += 1
            continue
        if i == 0:
            e[3] += int(lcp is not None and lcp[0] != 0)
            continue
        a = sa[i - 1]
        if a >= n:
            continue
        ok = t[a] < t[b] or (t[a] == t[b] and (a + 1 == n or (b + 1 < n and isa[a + 1] < isa[b + 1])))
        e[1] += int(not ok)
        if lcp is None:
            continue
        if not distributed:
            h = 0
            while a + h < n and b + h < n and t[a + h] == t[b + h]:
                h += 1
            e[2] += int(lcp[i] != h)
        elif ok:
            if t[a] != t[b]:
                want = 0
            elif a + 1 == n:
                want = 1
            elif isa[b + 1] >= n:
                want = None                                  # no rank: counted
            else:
                want = 1 + min(lcp[isa[a + 1] + 1: isa[b + 1] + 1])
            e[2] += int(want is None or lcp[i] != want)
    return e


@pytest.mark.parametrize("name", BIG + ["tiny%d" % n for n in TINY])
def test_models_accept_the_oracles_arrays(name):
    for bits in (32, 64):
        text, SA, ISA, LCP, tr = arrays(name, bits)
        assert M.expect_device(text, SA, ISA, LCP, truth=tr) == [0, 0, 0, 0]
        assert M.expect_multi(text, SA, ISA, LCP) == [0, 0, 0, 0]
        assert M.expect_device(text, SA, ISA, None) == [0, 0, 0, 0] and M.expect_multi(text, SA, ISA, None) == [0, 0, 0, 0]
        assert O.check_sa(text, SA, ISA) == 0 and np.array_equal(O.kasai(text, SA, ISA), LCP)


@pytest.mark.parametrize("name", BIG)
def test_model_sees_every_mutant(name):
    text, SA, ISA, LCP, tr = arrays(name)
    rmq = M.RangeMin(LCP)
    unseen, missing = [], []
    for cls, w, r, tr_m in all_mutants(name):
        if r is None:
            missing.append(cls)
            continue
        dev, mul = M.expect_both(*r, truth=tr_m, rmq=rmq if cls not in M.LCP_ONLY else None)
        if sum(dev) == 0 or sum(mul) == 0:
            unseen.append((cls, w, dev, mul))
        if cls == "L0th":
            assert dev == [0, 0, 0, 1] and mul == [0, 0, 0, 1]
        if cls == "Sswap":
            assert dev[0] == 2 and mul[0] == 2
        if cls.startswith("SIswap"):
            assert dev[0] == 0 and mul[0] == 0 and dev[1] >= 1 and mul[1] >= 1
        if cls in M.LCP_ONLY and cls != "L0th":
            assert dev[:2] == [0, 0] and mul[:2] == [0, 0] and dev[2] >= 1 and mul[2] >= 1 and dev[3] == mul[3] == 0
        if cls.startswith(("Sdup", "Srange", "Iwrong", "Irange")):
            assert dev[0] >= 1 and mul[0] >= 1
        if cls not in M.LCP_ONLY:                             # the same arrays without LCP: e2 = e3 = 0, e0 / e1 as before
            d0, m0 = M.expect_both(r[0], r[1], r[2], None)
            assert d0 == [dev[0], dev[1], 0, 0] and m0 == [mul[0], mul[1], 0, 0]
            assert sum(d0) > 0 and sum(m0) > 0 or cls == "Text"          # (a changed character can leave the order right and only LCP wrong)
    assert not unseen
    # a unary text has no two neighbours with different first characters; every other class applies to every text
    assert set(missing) <= ({"SIswap_diff"} if name == "unary" else set())


@pytest.mark.parametrize("name", ["tiny%d" % n for n in TINY] + ["small"])
def test_model_equals_the_definitions_entry_by_entry(name):
    # the vectorised model against a scalar restatement, for every class at every entry of texts small enough for that
    if name == "small":
        text = np.concatenate([inputs.dna(150, 3), inputs.dna(150, 3)[:90], np.full(40, 67, np.uint8)])
        ref = O.construct(text, bits=32)
        SA, ISA, LCP = ref["SA"], ref["ISA"], ref["LCP"]
    else:
        text, SA, ISA, LCP, _ = arrays(name, 32)
    n = text.size
    seen = 0
    for cls in M.MUTANTS:
        for w in (range(0, n, 1 if n < 20 else 13) if cls in M.POSITIONAL else [0]):
            r = M.mutate(cls, text, SA, ISA, LCP, w)
            if r is None:
                continue
            seen += 1
            for lcp in (r[3], None):
                assert M.expect_device(r[0], r[1], r[2], lcp) == scalar_model(r[0], r[1], r[2], lcp, False), (cls, w)
                assert M.expect_multi(r[0], r[1], r[2], lcp) == scalar_model(r[0], r[1], r[2], lcp, True), (cls, w)
            if cls != "Text":                                 # (in a text this short a changed character can leave every array right)
                assert sum(M.expect_multi(*r)) > 0 and sum(M.expect_device(*r)) > 0, (cls, w)
    assert seen >= (3 if n == 1 else 10)


def test_shared_prefixes_by_rank_and_by_characters_agree():
    text, SA, ISA, LCP, tr = arrays("dna")
    rng = np.random.RandomState(2)
    a, b = rng.randint(0, text.size, 5000), rng.randint(0, text.size, 5000)
    a[:50] = b[:50]
    near = rng.randint(1, text.size, 5000)
    a[100:200], b[100:200] = SA[near[100:200] - 1], SA[near[100:200]]
    assert np.array_equal(tr.shared(a.astype(np.int64), b.astype(np.int64), near), M.shared_by_characters(text, a, b))
    t2, S2, I2, L2, tr2 = arrays("tandem")
    a, b = rng.randint(0, 3000, 300).astype(np.int64), rng.randint(0, 3000, 300).astype(np.int64)
    tail = t2[-4000:]                                         # a text whose repeats are short enough to compare by characters
    ref = O.construct(tail, bits=64)
    assert np.array_equal(M.Truth(tail, ref["SA"], ref["ISA"], ref["LCP"]).shared(a, b), M.shared_by_characters(tail, a, b))


@pytest.mark.parametrize("name", ["dna", "tandem", "tiny17"])
def test_model_agrees_with_the_reference_checker(name):
    # expect_device: e0 = e1 = 0 exactly where the restatement's check_sa accepts, and e2 = 0 exactly where LCP is Kasai's
    text, SA, ISA, LCP, tr = arrays(name, 32)
    n = text.size
    cases = [("clean", 0, (text, SA, ISA, LCP))]
    for k, cls in enumerate(M.MUTANTS):
        r = M.mutate(cls, text, SA, ISA, LCP, (k * 7919 + 1) % n)
        if r is not None:
            cases.append((cls, k, r))
    for cls, k, r in cases:
        dev = M.expect_device(*r, truth=tr if cls != "Text" else truth_of(r[0]))
        assert (dev[:2] == [0, 0]) == (O.check_sa(r[0], r[1], r[2]) == 0), cls
        if cls in M.LCP_ONLY or cls == "clean":               # (Kasai needs a valid SA / ISA pair to walk)
            assert (dev[2] == 0 and dev[3] == 0) == bool(np.array_equal(O.kasai(r[0], r[1], r[2]), r[3])), cls


def test_only_the_anchors_of_the_recurrence_object_to_an_inflated_lcp():
    # every LCP entry > 0 raised by one satisfies LCP[i] = 1 + min(...) wherever the minimum is itself raised: what is left
    # are the pairs whose suffixes one further differ in their first character (LCP 1 over a minimum of 0) and the
    # one-character suffix.  Four letters: 4 x 3 boundaries between second characters + 1 = 13; one letter: 1.
    for name, want in (("dna", 13), ("tandem", 13), ("unary", 1)):
        text, SA, ISA, LCP, tr = arrays(name)
        r = M.mutate("Lall1", text, SA, ISA, LCP)
        assert M.expect_multi(*r) == [0, 0, want, 0]
        assert M.expect_device(*r, truth=tr) == [0, 0, int((LCP > 0).sum()), 0]


def test_positions_cover_the_edges_of_blocks_and_pieces():
    n = 300007
    pos = M.positions(n, np.arange(n), [(3, 7)], every_edge=True)
    offs, sizes = M.blocks(n, 3)
    assert sizes == [100003, 100002, 100002] and pos["block_first"] == offs and pos["block_last"] == [o + s - 1 for o, s in zip(offs, sizes)]
    assert len(pos["piece_first"]) == 21 and offs[1] + sizes[1] * 3 // 7 in pos["piece_first"] and offs[1] + sizes[1] * 4 // 7 - 1 in pos["piece_last"]
    assert pos["second"] == [1] and pos["last"] == [n - 1] and pos["max_lcp"] == [n - 1] and len(pos["random"]) == 3
    tiny = M.positions(3, np.zeros(3), [(8, 40)], every_edge=True)          # empty blocks and empty pieces leave no edge
    assert tiny["block_first"] == [0, 1, 2] and tiny["piece_first"] == [0, 1, 2]
