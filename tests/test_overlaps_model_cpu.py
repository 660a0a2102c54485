"""The two statements of the suffix-prefix overlaps (tests/overlaps_model.py) agree: all pairs by byte comparison, straight from
the definition, and the walk over the oracle's SA / ISA / LCP with a scalar previous-smaller search.

  - every slot (lb, ub) is equal, on the named small sets, the 300 copies and the reads, at min_len 1, 2 and the longest length
    (reads: 16), with and without the whole strings;
  - the union of SA[lb..ub) over the slots is the brute-force list of (slot, pos, sid);
  - borders of a string and whole strings that are prefixes of it are reported, and what is not asked stays 0, 0;
  - the reads are a real case: thousands of non-empty slots, a handful of steps per string."""

import numpy as np
import pytest

import overlaps_model as V


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("name", V.SMALL + ["copies300"])
def test_bytes_and_walk_agree_on_the_named_sets(name, whole):
    text, off, SA, ISA, LCP = V.set_arrays(name)
    for min_len in V.min_lens(name) + [3, 8, int(text.size) + 1]:
        a = V.by_bytes(text, off, min_len, whole)
        b = V.slots(name, min_len, whole) if min_len in V.min_lens(name) else V.by_walk(off, SA, ISA, LCP, min_len, whole)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), min_len
        assert np.all(a[0] <= a[1]) and np.all(a[1] <= text.size)


@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("name", V.SMALL)
def test_the_slots_expand_to_the_pair_list(name, whole):
    text, off, SA, ISA, LCP = V.set_arrays(name)
    for min_len in V.min_lens(name):
        lb, ub = V.slots(name, min_len, whole)
        assert V.pairs_of_slots(off, SA, lb, ub) == V.pairs_by_bytes(text, off, min_len, whole)


def test_what_the_definition_reports():
    text, off, SA, ISA, LCP = V.set_arrays("abab")                              # abab babab ab abab: offsets 0 4 9 11 15
    pairs = V.pairs_by_bytes(text, off, 1, False)
    assert (1, 2, 0) in pairs                                                    # "ab" is a border of string 0: its own suffix at 2
    assert (1, 9, 2) in pairs                                                    # string 2 = "ab" whole is a prefix of string 0
    assert (1, 7, 1) in pairs and (1, 13, 3) in pairs                            # the ends of babab and of the other abab
    assert (4, 8, 1) in pairs and (4, 3, 0) in pairs                             # "b" onto babab: from its own end, and from abab
    assert (4, 3, 0) not in V.pairs_by_bytes(text, off, 2, False)                # (one byte: not asked at min_len 2)
    lb, ub = V.slots("abab", 1, False)
    assert ub[3] == 0 and lb[3] == 0                                             # d == L is not asked without the whole strings
    lb, ub = V.slots("abab", 1, True)
    assert ub[3] - lb[3] == 3                                                    # abab ends abab, babab and the other abab
    assert sorted(int(SA[x]) for x in range(int(lb[3]), int(ub[3]))) == [0, 5, 11]
    lb, ub = V.slots("abab", 2, False)
    assert lb[0] == 0 and ub[0] == 0 and ub[1] > lb[1]                           # below min_len: empty


def test_the_chain_of_the_unary_set_is_as_long_as_the_string():
    text, off, SA, ISA, LCP = V.set_arrays("unary")
    steps = []
    V.by_walk(off, SA, ISA, LCP, 1, True, steps)
    assert steps == [4, 3, 2, 1]


@pytest.mark.parametrize("name", ["reads", "reads_mut"])
def test_reads(name):
    text, off, SA, ISA, LCP = V.set_arrays(name)
    assert int(text.size) == 32768 and off.size == 513
    for whole in (False, True):
        steps = []
        lb, ub = V.by_walk(off, SA, ISA, LCP, 16, whole, steps)
        a = V.by_bytes(text, off, 16, whole)
        assert np.array_equal(a[0], lb) and np.array_equal(a[1], ub)
        slots, pairs = int(np.count_nonzero(ub > lb)), int(np.sum(ub - lb))
        assert slots > 0 and pairs >= slots               # (2950 / 3139 and 3462 / 3715 on the reads, 742 / 786 and 1254 / 1308 once mutated)
        assert 1 <= np.mean(steps) <= 12
        assert len(V.pairs_of_slots(off, SA, lb, ub)) == pairs
        print(name, whole, "slots", slots, "pairs", pairs, "steps per string", np.mean(steps))
