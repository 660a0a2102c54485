"""The host model of the two GPU checkers for generalized suffix arrays (tests/gsa_checker_model.py), without a GPU: the
model accepts the oracle's arrays of every string set, equals a naive entry-by-entry count written from the definitions
of include/psacx.h (Python byte-string comparison of the suffixes, a loop for the range minimum) for every class of wrong
arrays, old and new, and every class applies to at least one set.  The library's entry points exist and refuse a null
context."""
import ctypes as C

import numpy as np
import pytest

import gsa_checker_model as G
import checker_model as M
import oracle_lib as O

from gsa_checker_model import BIG, TINY, arrays

LAYOUTS = [(1, 7), (3, 7), (8, 7)]


def naive_counts(text, off, SA, ISA, LCP, distributed):
    """The counting rules of psacx_check_gsa_dev_* / psacx_multi_check_gsa_dev_*, one entry at a time."""
    n = len(text)
    raw = bytes(bytearray(int(x) for x in text))
    sa = [int(x) for x in SA]; isa = [int(x) for x in ISA]
    lcp = None if LCP is None else [int(x) for x in LCP]
    end = [0] * n
    for k in range(len(off) - 1):
        for p in range(int(off[k]), int(off[k + 1])):
            end[p] = int(off[k + 1])
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
        a_one, b_one = a + 1 == end[a], b + 1 == end[b]
        if raw[a] != raw[b]:
            ok = raw[a] < raw[b]
        elif a_one and b_one:
            ok = a < b
        elif a_one:
            ok = True
        elif b_one:
            ok = False
        else:
            ok = isa[a + 1] < isa[b + 1]
        e[1] += int(not ok)
        if lcp is None:
            continue
        if not distributed:
            x, y = raw[a:end[a]], raw[b:end[b]]
            h = 0
            while h < len(x) and h < len(y) and x[h] == y[h]:
                h += 1
            e[2] += int(lcp[i] != h)
        elif ok:
            if raw[a] != raw[b]:
                want = 0
            elif a_one or b_one:
                want = 1
            elif isa[b + 1] >= n:
                want = None                                  # no rank: counted
            else:
                lo = None
                for q in range(isa[a + 1] + 1, isa[b + 1] + 1):
                    lo = lcp[q] if lo is None or lcp[q] < lo else lo
                want = 1 + lo
            e[2] += int(want is None or lcp[i] != want)
    return e


def truth_for(cls, r, tr):
    return tr if cls != "Text" and cls not in G.MOVES_OFFSETS else G.gsa_truth_of(r[0], r[1])


@pytest.mark.parametrize("name", BIG + ["tiny%d" % n for n in TINY])
def test_models_accept_the_oracles_arrays(name):
    for bits in (32, 64):
        text, off, SA, ISA, LCP, tr = arrays(name, bits)
        assert int(off[0]) == 0 and int(off[-1]) == text.size
        assert G.expect_gsa_device(text, off, SA, ISA, LCP, truth=tr) == [0, 0, 0, 0]
        assert G.expect_gsa_device(text, off, SA, ISA, LCP) == [0, 0, 0, 0]            # by characters
        assert G.expect_gsa_multi(text, off, SA, ISA, LCP) == [0, 0, 0, 0]
        assert G.expect_gsa_device(text, off, SA, ISA, None) == [0, 0, 0, 0] and G.expect_gsa_multi(text, off, SA, ISA, None) == [0, 0, 0, 0]


def test_the_plain_model_rejects_a_correct_gsa_and_one_string_is_a_plain_text():
    # why the string sets need checkers of their own: read as one text, a correct GSA is out of order and its LCP too short
    text, off, SA, ISA, LCP, tr = arrays("reads")
    plain = M.expect_device(text, SA, ISA, LCP)
    assert plain[0] == 0 and plain[1] > 0 and plain[2] > 0
    # one string: the arrays are those of the text, and both pairs of models agree on them
    text, off, SA, ISA, LCP, tr = arrays("single")
    ref = O.construct(text, bits=64)
    assert np.array_equal(ref["SA"], SA) and np.array_equal(ref["ISA"], ISA) and np.array_equal(ref["LCP"], LCP)
    assert M.expect_device(text, SA, ISA, LCP) == M.expect_multi(text, SA, ISA, LCP) == [0, 0, 0, 0]


def small_sets():
    import inputs
    rng = np.random.RandomState(4)
    read = inputs.dna(23, 31)
    two = np.frombuffer(b"AC", np.uint8)
    sets = {
        "abab": [b"abab", b"baba"],
        "reads": [inputs.dna(400, 32)[s:s + k] for s, k in zip(rng.randint(0, 370, 12), rng.randint(8, 30, 12))],
        "copies": [read, read, inputs.dna(9, 33), read, read[:11], read],
        "prefixes": [read[:k] for k in (5, 1, 23, 2, 17, 9, 1)],
        "unary": [np.full(k, 66, np.uint8) for k in (3, 1, 7, 2, 1, 5)],
        "tandem": G._cut(np.tile(two[[0, 1, 1, 0, 1]], 40), [1, 30, 2, 57, 13, 1, 45]),
        "single": [inputs.dna(150, 34)],
    }
    sets.update({"tiny%d" % n: G.strings_of("tiny%d" % n) for n in TINY})
    return sets


@pytest.mark.parametrize("name", list(small_sets()))
def test_model_equals_the_definitions_entry_by_entry(name):
    ref = O.construct_ss(small_sets()[name], bits=32)
    text, off, SA, ISA, LCP = ref["text"], ref["off"], ref["SA"], ref["ISA"], ref["LCP"]
    n = text.size
    by_def_sa, by_def_lcp = O.gsa_by_definition(small_sets()[name])
    assert np.array_equal(by_def_sa, SA) and np.array_equal(by_def_lcp, LCP)
    assert naive_counts(text, off, SA, ISA, LCP, False) == naive_counts(text, off, SA, ISA, LCP, True) == [0, 0, 0, 0]
    seen = set()
    for cls in G.ALL:
        for w in (range(0, n, 1 if n < 40 else 11) if cls in G.POSITIONAL else [0]):
            r = G.mutate_gsa(cls, text, off, SA, ISA, LCP, w)
            if r is None:
                continue
            seen.add(cls)
            for lcp in (r[4], None):
                dev, mul = naive_counts(r[0], r[1], r[2], r[3], lcp, False), naive_counts(r[0], r[1], r[2], r[3], lcp, True)
                assert G.expect_gsa_device(r[0], r[1], r[2], r[3], lcp) == dev, (cls, w)
                assert G.expect_gsa_multi(r[0], r[1], r[2], r[3], lcp) == mul, (cls, w)
                if lcp is not None:
                    assert G.expect_gsa_device(*r, truth=truth_for(cls, r, G.GsaTruth(text, off, SA, ISA, LCP))) == dev, (cls, w)
                    if cls in G.GSA_MUTANTS and cls not in G.MAY_PASS:
                        assert sum(dev) > 0 and sum(mul) > 0, (cls, w)
    assert len(seen) >= (3 if n == 1 else 8)


def test_every_class_applies_to_a_small_set():
    seen = set()
    for name, strings in small_sets().items():
        ref = O.construct_ss(strings, bits=32)
        for cls in G.ALL:
            if G.mutate_gsa(cls, ref["text"], ref["off"], ref["SA"], ref["ISA"], ref["LCP"], ref["text"].size // 2) is not None:
                seen.add(cls)
    assert seen == set(G.ALL)


@pytest.mark.parametrize("name", BIG)
def test_model_sees_every_mutant(name):
    text, off, SA, ISA, LCP, tr = arrays(name)
    rmq = G.RangeMin(LCP)
    pos = G.positions(text.size, LCP, LAYOUTS)
    where = sorted({w for v in pos.values() for w in v})
    unseen = []
    for cls in G.ALL:
        for w in (where if cls in G.POSITIONAL else [0]):
            r = G.mutate_gsa(cls, text, off, SA, ISA, LCP, w)
            if r is None:
                continue
            _applies.setdefault(cls, set()).add(name)
            dev, mul = G.expect_gsa_both(*r, truth=truth_for(cls, r, tr), rmq=rmq if cls not in G.LCP_ONLY else None)
            if cls in G.MAY_PASS:
                continue
            if sum(dev) == 0 or sum(mul) == 0:
                unseen.append((cls, w, dev, mul))
            if cls in ("Geq_swap", "Gorder_concat"):
                assert dev[0] == 0 and mul[0] == 0 and dev[1] >= 1 and mul[1] >= 1
            if cls in G.LCP_ONLY and cls != "L0th":
                assert dev[:2] == [0, 0] and mul[:2] == [0, 0] and dev[2] >= 1 and mul[2] >= 1 and dev[3] == mul[3] == 0
            if cls not in G.LCP_ONLY:
                d0, m0 = G.expect_gsa_both(r[0], r[1], r[2], r[3], None)
                assert d0 == [dev[0], dev[1], 0, 0] and m0 == [mul[0], mul[1], 0, 0]
    assert not unseen


_applies = {}


def test_every_class_of_the_catalogue_applies_to_a_set():
    for name in BIG:
        text, off, SA, ISA, LCP, tr = arrays(name)
        for cls in G.ALL:
            if G.mutate_gsa(cls, text, off, SA, ISA, LCP, text.size // 3) is not None:
                _applies.setdefault(cls, set()).add(name)
    assert set(_applies) == set(G.ALL), sorted(set(G.ALL) - set(_applies))
    # the classes that need two strings do not apply to one; each of them applies to the reads or to the copies
    for cls in G.GSA_MUTANTS:
        assert _applies[cls] & {"reads", "copies"}, cls
    assert not _applies["Geq_swap"] & {"single"} and not _applies["Goff+1"] & {"single"}


def test_the_library_has_the_entry_points_and_refuses_a_null_context():
    from psac_amd import _lib
    lib = _lib.load()
    err = (C.c_uint64 * 4)()
    for suf in ("u32", "u64"):
        assert getattr(lib, "psacx_check_gsa_dev_" + suf)(None, None, 0, None, 0, None, None, None, err) == -1          # PSACX_EINVAL
        assert getattr(lib, "psacx_multi_check_gsa_dev_" + suf)(None, None, None, None, 0, None, None, None, err) == -1
    assert lib.psacx_check_gsa_dev_u64(None, None, 5, None, 1, None, None, None, err) == -1
