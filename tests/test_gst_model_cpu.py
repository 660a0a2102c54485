"""The host model of the generalized suffix tree's node table and of its checker (tests/gst_model.py) against a second, top-down
statement of the table from the suffixes' bytes, against the one-string model where the set is one string, and its verdict on
every class of mutant; and the Python entry points on a machine without a GPU.  tests/test_gpu_gst.py holds
psacx_suffix_tree_gsa_dev_* and tests/test_gpu_gst_verifier.py psacx_check_suffix_tree_gsa_dev_* to this model."""
import os
import subprocess

import numpy as np
import pytest

import gst_model as T
import oracle_lib as O
import st_checker_model as S


def _clean(text, off, SA, LCP, table):
    recs = T.records(text, off, SA, LCP)
    R = int(recs[2].size)
    return T.expect(text, off, SA, LCP, table, recs) == [0, 0, R, int(np.count_nonzero(table))]


def test_model_equals_the_top_down_statement_on_random_tiny_sets():
    # 1-6 strings of 1-8 characters over 1-3 symbols: unary sets, duplicate strings and n = 1 among them
    rng = np.random.RandomState(5)
    seen = {"unary": 0, "duplicates": 0, "n1": 0, "dollar_ranges": 0}
    for _ in range(300):
        sigma = int(rng.randint(1, 4))
        strings = [rng.randint(65, 65 + sigma, int(rng.randint(1, 9))).astype(np.uint8) for _ in range(int(rng.randint(1, 7)))]
        ref = O.construct_ss(strings, bits=64)
        text, off = ref["text"], np.asarray(ref["off"], np.uint64)
        table = T.expected_table(text, off, ref["SA"], ref["LCP"])
        assert np.array_equal(table, T.top_down_table(text, off, ref["SA"])), [bytes(s) for s in strings]
        assert _clean(text, off, ref["SA"], ref["LCP"], table)
        assert not table[0, 0] and not table[0, 1]           # the root has no $-leaf
        seen["unary"] += sigma == 1
        seen["duplicates"] += len({bytes(s) for s in strings}) < len(strings)
        seen["n1"] += text.size == 1
        seen["dollar_ranges"] += bool((table[:, 0] != table[:, 1]).any())
    assert all(seen.values()), seen


@pytest.mark.parametrize("name", T.TINY + ["copies", "prefixes", "unary", "word_edges", "bytes256", "edge65"])
def test_model_equals_the_top_down_statement(name):
    text, off, SA, LCP, recs, table = T.arrays(name)
    assert table.shape == (text.size, S.codes_of(text)[1] + 2)
    assert np.array_equal(table, T.top_down_table(text, off, SA))
    assert _clean(text, off, SA, LCP, table)
    # on a correct generalized suffix array the $ records of a row are leaves, neighbours in SA
    rows, c, ids = recs
    d = c == 0
    assert np.all(ids[d] >= text.size)
    lo, hi = table[:, 0], table[:, 1]
    assert int(d.sum()) == int((hi - lo + 1)[lo != 0].sum())
    if name == "copies":
        assert int((hi - lo + 1)[lo != 0].max()) == 151


@pytest.mark.parametrize("name", ["single", "mississippi", "edge4097", "unary1"])
def test_one_string_gives_the_one_string_table(name):
    if name == "single":
        text, off, SA, LCP, recs, table = T.arrays(name)
    else:
        text, SA, LCP = S.arrays("unary" if name == "unary1" else name)[:3]
        off = np.array([0, text.size], np.uint64)
        table = T.expected_table(text, off, SA, LCP)
    assert T.single_string_relation(table, S.expected_table(text, SA, LCP))
    assert _clean(text, off, SA, LCP, table)


def test_stored_lcp0_is_never_used_as_a_value():
    for name in ("tiny9", "copies", "word_edges"):
        text, off, SA, LCP, recs, table = T.arrays(name)
        l = LCP.copy()
        l[0] = 7
        assert all(np.array_equal(a, b) for a, b in zip(T.records(text, off, SA, l), recs))


def test_measured_verdicts_on_a_small_set():
    # "ab", "ab", "b": suffixes ab ab b b b in SA order 0 2 1 3 4, LCP 0 2 0 1 1
    ref = O.construct_ss([b"ab", b"ab", b"b"], bits=64)
    text, off, SA, LCP = ref["text"], ref["off"], ref["SA"], ref["LCP"]
    assert SA.tolist() == [0, 2, 1, 3, 4] and LCP.tolist() == [0, 2, 0, 1, 1]
    table = T.expected_table(text, off, SA, LCP)
    #            $lo $hi  a   b
    assert table.tolist() == [[0, 0, 1, 3],       # root: "ab.." is node 1, "b.." node 3
                              [5, 6, 0, 0],       # node 1 = "ab": the two equal suffixes, leaves 5 and 6
                              [0, 0, 0, 0],
                              [7, 9, 0, 0],       # node 3 = "b": leaves 7, 8, 9
                              [0, 0, 0, 0]]
    assert T.expect(text, off, SA, LCP, table) == [0, 0, 7, 6]            # 7 records in 6 cells: leaf 8 lies inside its range
    t = table.copy(); t[3, 0] = 8
    assert T.expect(text, off, SA, LCP, t) == [1, 0, 7, 6]                # leaf 7 falls out (leaf 8 now witnesses the cell)
    t = table.copy(); t[3, 1] = 10
    assert T.expect(text, off, SA, LCP, t) == [0, 1, 7, 6]                # a range one too wide: every record matched, 10 has no witness
    t = table.copy(); t[2, 0] = t[2, 1] = 8
    assert T.expect(text, off, SA, LCP, t) == [0, 2, 7, 8]                # a stray pair


@pytest.mark.parametrize("name", ["tiny17", "edge65", "edge4097", "copies", "unary", "word_edges", "bytes256"])
def test_a_table_is_clean_exactly_when_it_is_the_table(name):
    text, off, SA, LCP, recs, table = T.arrays(name)
    R = int(recs[2].size)
    seen = set()
    for cls in T.TABLE_MUTANTS:
        for w in T.table_positions(text.size, LCP):
            bad, done = T.mutate_table([(cls, w)], table, T.head_of(name), recs)
            if not done:
                continue
            seen.add(cls)
            out = T.expect(text, off, SA, LCP, bad, recs)
            assert (out[0] == 0 and out[1] == 0) == np.array_equal(bad, table), (cls, w, out)
            assert not np.array_equal(bad, table), (cls, w)
            assert out[1] >= 0 and out[2] == R and out[3] == int(np.count_nonzero(bad))
    assert seen >= set(T.DOLLAR_MUTANTS) | {"zero_leaf", "move_row", "stray_valid", "stray_2n", "stray_ones", "leaf_off_by_one"}
    if name in ("edge4097", "copies"):
        assert seen == set(T.TABLE_MUTANTS)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["tiny17", "edge65", "copies", "word_edges"])
def test_input_mutants_have_a_verdict(name, bits):
    # the model is total: whatever SA, LCP, text and (valid) offsets hold, it names four counters; the stored LCP[0] is no input
    text, off, SA, LCP, recs, table = T.arrays(name)
    seen = set()
    for cls in T.ALL_INPUT_MUTANTS:
        for w in T.table_positions(text.size, LCP)[:6]:
            arrs = T.mutate_inputs(cls, w, text, off, SA, LCP, bits)
            if arrs is None:
                continue
            out = T.expect(arrs[0], arrs[1], arrs[2], arrs[3], table)
            assert out[1] >= 0 and out[3] == int(np.count_nonzero(table))
            if cls == "L0th":
                assert out[:2] == [0, 0]
            elif out[0] + out[1] > 0:
                seen.add(cls)
    assert seen >= {"L+", "Lones", "Sones", "Sn", "Goff+1", "Goff-1"}


def test_entry_points_exist_and_fail_loudly_without_a_gpu():
    import psac_amd
    from psac_amd import _lib
    lib = _lib.load()
    for suf in ("u32", "u64"):
        for nm in ("psacx_suffix_tree_gsa_", "psacx_suffix_tree_gsa_dev_", "psacx_check_suffix_tree_gsa_dev_"):
            assert hasattr(lib, nm + suf)
    for nm in ("suffix_tree_gsa", "suffix_tree_gsa_device", "check_suffix_tree_gsa_device"):
        assert callable(getattr(psac_amd, nm)) and nm in psac_amd.__all__
    import torch
    if not torch.cuda.is_available():
        text, off, SA, LCP, recs, table = T.arrays("tiny9")
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.suffix_tree_gsa(text, off, SA, LCP)
        assert e.value.code == -6                            # PSACX_ENOGPU: no CPU fallback


def build_cpp_program(tmp_path):
    """tests/cpp/test_gst.cpp (construct_gst of include/suffix_array.hpp) built warning-free as C++11 against the library."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, lib = str(tmp_path / "test_gst"), os.path.join(root, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(root, "tests", "cpp", "test_gst.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "gst header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)
