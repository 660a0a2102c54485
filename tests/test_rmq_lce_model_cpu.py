"""The host models of the range minimum and the longest common extension agree with themselves and with the reference.

  - lce_model: the byte-by-byte definition and the kangaroo walk over the oracle's ISA / LCP give the same length for all pairs of
    positions 0 .. n + 1 of the tiny texts and sets of locate_model / locate_gsa_model, for e in {0, 1, 2, 5, n}; and for sampled
    pairs of the larger ones.
  - rmq_model: tests/golden/rmq_reference.json holds the positions the reference's rmq<>::query returned (recorded once by a
    program that includes its rmq.hpp) on the shapes of its own test -- sizes 1, 13, 32, 64, 127, 233, 1025 with values
    rand() % 10, and the 0/1 array of its multiple-minima test, size 1000.  The model returns the same positions: "first minimum"
    means here what it means there.  The two statements of the model (query, Table) agree as well."""
import json
import os

import numpy as np
import pytest

import lce_model as E
import locate_gsa_model as G
import locate_model as L
import rmq_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mismatches(n):
    return [0, 1, 2, 5, n]


@pytest.mark.parametrize("name", ["mississippi"] + L.TINY)
def test_bytes_and_walk_agree_on_all_pairs_of_the_tiny_texts(name):
    text, SA, ISA, LCP = E.arrays(name)
    n = int(text.size)
    for e in mismatches(n):
        for a in range(n + 2):
            for b in range(n + 2):
                assert E.by_bytes(text, None, a, b, e) == E.by_walk(ISA, LCP, None, n, a, b, e), (a, b, e)


def tiny_sets():
    return [s for s in G.GST if sum(len(x) for x in G.strings_of(s)) <= 40]


def test_there_are_tiny_sets():
    assert len(tiny_sets()) >= 3


@pytest.mark.parametrize("name", G.GST)
def test_bytes_and_walk_agree_on_the_sets(name):
    text, off, SA, ISA, LCP = E.set_arrays(name)
    n = int(text.size)
    if n <= 40:
        pairs = [(a, b) for a in range(n + 2) for b in range(n + 2)]
    else:
        rng = np.random.RandomState(7)
        o = [int(x) for x in off]
        edge = sorted(set(x for p in o for x in (p - 1, p, p + 1) if 0 <= x <= n + 1))[:40]
        pairs = [(a, b) for a in edge for b in edge] + [tuple(int(x) for x in rng.randint(0, n + 2, 2)) for _ in range(400)]
        pairs += [(int(SA[i]), int(SA[i + 1])) for i in rng.randint(0, n - 1, 200)]
    for e in mismatches(n):
        for a, b in (pairs if e < n or n <= 40 else pairs[::37]):        # (a walk with e = n takes a range minimum per mismatch)
            assert E.by_bytes(text, off, a, b, e) == E.by_walk(ISA, LCP, off, n, a, b, e), (a, b, e)


@pytest.mark.parametrize("name", ["edge65", "edge4097", "unary", "tandem", "bytes256"])
def test_bytes_and_walk_agree_on_sampled_pairs(name):
    text, SA, ISA, LCP = E.arrays(name)
    n = int(text.size)
    rng = np.random.RandomState(8)
    pairs = [tuple(int(x) for x in rng.randint(0, n + 2, 2)) for _ in range(150)]
    pairs += [(int(SA[i]), int(SA[i + 1])) for i in rng.randint(0, n - 1, 100)] + [(0, n - 1), (n - 1, n), (n, n + 1), (5, 5)]
    for e in (0, 1, 5, n):
        for a, b in (pairs if e < n else pairs[::11]):
            assert E.by_bytes(text, None, a, b, e) == E.by_walk(ISA, LCP, None, n, a, b, e), (a, b, e)


def test_one_string_set_equals_the_plain_form():
    text, SA, ISA, LCP = E.arrays("mississippi")
    n = int(text.size)
    off = np.array([0, n], np.uint64)
    for e in (0, 2):
        for a in range(n + 2):
            for b in range(n + 2):
                assert E.by_bytes(text, off, a, b, e) == E.by_bytes(text, None, a, b, e)


def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "rmq_reference.json")))["cases"]


def test_golden_has_the_shapes_of_the_reference_test():
    cases = golden()
    assert [len(c["values"]) for c in cases] == [1, 13, 32, 64, 127, 233, 1025, 1000]
    assert all(len(c["ranges"]) >= min(90, len(c["values"])) for c in cases)
    assert set(cases[-1]["values"]) == {0, 1} and all(max(c["values"]) <= 9 for c in cases[:-1])


@pytest.mark.parametrize("case", range(8))
def test_first_minimum_means_what_the_reference_returns(case):
    c = golden()[case]
    v = np.array(c["values"], np.uint64)
    t = R.Table(v)
    rg = np.array(c["ranges"], np.int64)
    for lo, hi, pos in c["ranges"]:
        assert R.query(v, lo, hi) == (int(v[pos]), pos), (lo, hi)
    mn, arg = t.queries(rg[:, 0], rg[:, 1])
    assert np.array_equal(arg, rg[:, 2].astype(np.uint64)) and np.array_equal(mn, v[rg[:, 2]])


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_the_two_statements_of_the_range_minimum_agree(dtype):
    rng = np.random.RandomState(3)
    top = R.ones(dtype)
    for n in (1, 2, 63, 64, 65, 130, 1000):
        for v in (rng.randint(0, 3, n).astype(dtype), np.full(n, top, dtype), np.full(n, top, dtype) - rng.randint(0, 2, n).astype(dtype)):
            t = R.Table(v)
            lo = rng.randint(0, n + 2, 500)
            hi = rng.randint(0, n + 3, 500)
            a = R.queries(v, lo, hi)
            b = t.queries(lo, hi)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the empty-range rule
    v = np.array([4, 2, 2, 7], dtype)
    assert R.query(v, 2, 2) == (top, 4) and R.query(v, 3, 1) == (top, 4) and R.query(v, 4, 9) == (top, 4) and R.query(v, 1, 99) == (2, 1)


def test_the_lengths_the_cpp_program_states_by_hand():
    # tests/cpp/test_lce.cpp
    t = np.frombuffer(b"mississippi", np.uint8)
    a, b = [1, 2, 0, 3, 4, 10, 11], [4, 5, 1, 6, 4, 7, 3]
    for e, want in ((0, [4, 3, 0, 2, 7, 1, 0]), (1, [5, 4, 1, 3, 7, 1, 0]), (100, [7, 6, 10, 5, 7, 1, 0])):
        assert [E.by_bytes(t, None, x, y, e) for x, y in zip(a, b)] == want
    assert E.by_bytes(t, None, 1, 4, 2) == 7
    off = np.array([0, 6, 11], np.uint64)
    a, b = [1, 2, 3, 2, 4, 5, 6], [7, 6, 6, 5, 4, 6, 11]
    for e, want in ((0, [1, 1, 2, 1, 2, 1, 0]), (1, [2, 2, 3, 1, 2, 1, 0])):
        assert [E.by_bytes(t, off, x, y, e) for x, y in zip(a, b)] == want
    lcp = np.array([0, 1, 1, 4, 0, 0, 1, 0, 2, 1, 3], np.uint64)
    assert np.array_equal(E.arrays("mississippi")[3], lcp)
    top = R.ones(np.uint64)
    assert [R.query(lcp, l, h) for l, h in zip([0, 1, 3, 5, 8, 1], [11, 4, 4, 5, 20, 11])] == [(0, 0), (1, 1), (4, 3), (top, 11), (1, 9), (0, 4)]


def build_cpp_program(tmp_path):
    """tests/cpp/test_lce.cpp (lce and range_min of include/suffix_array.hpp) built warning-free as C++11 against the library."""
    import subprocess
    exe, lib = str(tmp_path / "test_lce"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_lce.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    import subprocess
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "lce header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_cli_refuses_malformed_pairs_and_fails_loudly_without_a_gpu(tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "psac_amd", "bin", "lce")
    (tmp_path / "t.txt").write_bytes(b"mississippi")
    (tmp_path / "bad.txt").write_bytes(b"1 4\n3\n")
    (tmp_path / "colon.txt").write_bytes(b"0:1 1:2\n")
    (tmp_path / "p.txt").write_bytes(b"1 4\n")
    for pairs in ("bad.txt", "colon.txt"):                  # one position only; string:offset without --set
        r = subprocess.run([exe, "-f", str(tmp_path / "t.txt"), "-p", str(tmp_path / pairs)], capture_output=True, text=True)
        assert r.returncode != 0 and "no pair of positions" in r.stderr
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-f", str(tmp_path / "t.txt"), "-p", str(tmp_path / "p.txt"), "-e", "1"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
