"""The host model of the suffix-tree node table and of its checker (tests/st_checker_model.py) against the oracle, the
mississippi known answer and a second, top-down statement of the table; and its verdict on every class of mutant.  No GPU:
tests/test_gpu_st_verifier.py holds psacx_check_suffix_tree_dev_* to this model."""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
import st_checker_model as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_kat.json")


@pytest.mark.parametrize("name", S.ALL)
def test_model_table_equals_the_oracle(name):
    text, SA, LCP, recs, table = S.arrays(name)
    want = O.suffix_tree(text, SA, LCP)
    assert table.shape == want.shape and np.array_equal(table, want)
    # records = nonzero cells: no two records share a cell
    assert int(np.count_nonzero(table)) == recs[2].size
    assert S.expect(text, SA, LCP, table, recs) == [0, 0, recs[2].size, recs[2].size]
    assert S.expect(text, SA, LCP, want) == [0, 0, recs[2].size, recs[2].size]


def test_model_table_equals_the_mississippi_known_answer():
    m = json.load(open(GOLDEN))["mississippi"]
    text, SA, LCP, recs, table = S.arrays("mississippi")
    assert table.reshape(-1).tolist() == m["suffix_tree_nodes"]


@pytest.mark.parametrize("name", S.SMALL + ["hub", "dna30000"])
def test_model_table_equals_the_top_down_statement(name):
    if name == "dna30000":                       # (one numpy call per node: the whole 300 000 characters would take seconds)
        text = S.text_of("dna")[:30000].copy()
        ref = O.construct(text, bits=64)
        SA, LCP = ref["SA"], ref["LCP"]
        table = S.expected_table(text, SA, LCP)
    else:
        text, SA, LCP, recs, table = S.arrays(name)
    assert np.array_equal(S.top_down_table(text, SA, LCP), table)


def test_stored_lcp0_is_never_used_as_a_value():
    for name in ("mississippi", "edge65", "unary"):
        text, SA, LCP, recs, table = S.arrays(name)
        l = LCP.copy()
        l[0] = 7
        got = S.records(text, SA, l)
        assert all(np.array_equal(a, b) for a, b in zip(got, recs))


def test_measured_verdicts_on_mississippi():
    text, SA, LCP, recs, table = S.arrays("mississippi")
    n = text.size
    t = table.copy()
    r, c = [int(x[0]) for x in np.nonzero(t >= n)]
    t[r, c] = 0                                  # a leaf cell zeroed
    assert S.expect(text, SA, LCP, t, recs) == [1, 0, 17, 16]
    t = table.copy()
    r, c = [int(x[0]) for x in np.nonzero(t == 0)]
    t[r, c] = n + 3                              # a stray leaf id in an empty cell
    assert S.expect(text, SA, LCP, t, recs) == [0, 1, 17, 18]
    t = table.copy()
    r = int(np.nonzero((t != 0).sum(axis=1) >= 2)[0][0])
    c = np.nonzero(t[r])[0]
    t[r, c[0]], t[r, c[1]] = t[r, c[1]], t[r, c[0]]          # two children swapped
    assert S.expect(text, SA, LCP, t, recs) == [2, 2, 17, 17]
    l = LCP.copy()
    l[5] += 1
    assert S.expect(text, SA, l, table) == [4, 4, 17, 17]


@pytest.mark.parametrize("name", ["mississippi", "edge65", "edge4097", "unary", "tandem", "perm256"])
def test_every_table_mutant_alone_is_caught(name):
    text, SA, LCP, recs, table = S.arrays(name)
    R = recs[2].size
    seen = set()
    for cls in S.TABLE_MUTANTS:
        for w in S.table_positions(text.size, LCP):
            bad, done = S.mutate_table([(cls, w)], table, S.head_of(name), recs)
            if not done:
                continue
            seen.add(cls)
            out = S.expect(text, SA, LCP, bad, recs)
            assert out[0] + out[1] > 0 and out[2] == R, (cls, w, out)
            assert out[3] == int(np.count_nonzero(bad))
    # what a text cannot carry: no internal node (perm256), no free cell beside a child ...
    assert seen >= {"zero_leaf", "move_row", "stray_valid", "stray_2n", "stray_ones", "leaf_off_by_one"}
    if name in ("mississippi", "tandem", "edge4097"):
        assert seen == set(S.TABLE_MUTANTS)


# classes that cannot show on a text, with the reason
HARMLESS = {
    "unary": {"Text"},          # one letter: there is no other character to put
    "perm256": {"L0", "Text"},  # LCP is all zero already; every character occurs once, so replacing one would change sigma
    "tandem": {"Text"},         # no record reads the characters at the few positions tried (the table below still decides each case)
}


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["mississippi", "edge65", "edge4097", "unary", "tandem", "perm256"])
def test_an_input_mutant_is_caught_exactly_when_it_changes_the_table(name, bits):
    # A wrong input need not make the table wrong (LCP + 1 where the longer suffix ends, a swap of two suffixes with the same edge
    # character ...).  Each mutant on its own: the verdict on the clean table is nonzero exactly when the correct table of the
    # changed arrays (expected_table, written record by record) differs from the clean one; and every class is caught somewhere on
    # every text but for the stated exceptions.
    text, SA, LCP, recs, table = S.arrays(name)
    seen = set()
    for cls in S.INPUT_MUTANTS:
        for w in S.table_positions(text.size, LCP)[:6]:
            arrs = S.mutate_inputs(cls, w, text, SA, LCP, bits)
            if arrs is None:
                continue
            out = S.expect(arrs[0], arrs[1], arrs[2], table)
            if cls == "L0th":                    # the stored LCP[0] is no input of the table
                assert out[:2] == [0, 0]
                continue
            theirs = S.records(*arrs)
            assert len(set(zip(theirs[0].tolist(), theirs[1].tolist()))) == theirs[2].size or out[0] > 0       # (two records in one cell: one of them is unmatched)
            assert (out[0] + out[1] > 0) == (not np.array_equal(S.expected_table(*arrs, recs=theirs), table)), (cls, w, out)
            if out[0] + out[1] > 0:
                seen.add(cls)
    assert seen == set(S.INPUT_MUTANTS) - {"L0th"} - HARMLESS.get(name, set())


def test_farthest_parents_of_the_named_texts():
    # the figures the GPU tests quote for what each text exercises
    far = {name: S.farthest_parent(S.arrays(name)[3], S.arrays(name)[0].size) for name in ("dna", "tandem", "hub", "perm256")}
    assert far == {"dna": 243572, "tandem": 24000, "hub": 119601, "perm256": 255}
    assert int(S.arrays("tandem")[2].max()) == 36963 and int(S.arrays("unary")[2].max()) == 4999 and int(S.arrays("hub")[2].max()) == 2
    assert S.arrays("dna")[0].size > 64 ** 3
