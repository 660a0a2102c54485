"""What the overlaps call adds above the ABI builds without a GPU and fails loudly without one: tests/cpp/test_overlaps.cpp
(overlaps of include/suffix_array.hpp) compiles warning-free as C++11 against the library, the values it states by hand are the
model's, and the command line refuses what it cannot read."""
import os
import subprocess

import numpy as np

import overlaps_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpp_program(tmp_path):
    exe, lib = str(tmp_path / "test_overlaps"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_overlaps.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "overlaps header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_the_intervals_the_cpp_program_states_by_hand():
    text, off, SA, ISA, LCP = V.set_arrays("abab")
    assert [int(x) for x in off] == [0, 4, 9, 11, 15]
    assert [int(x) for x in SA] == [2, 7, 9, 13, 0, 5, 11, 3, 8, 10, 14, 1, 6, 12, 4]
    stated = {
        (1, False): ([0, 0, 0, 0, 7, 0, 11, 0, 0, 0, 0, 0, 0, 0, 0], [0, 4, 0, 0, 11, 0, 14, 0, 0, 0, 0, 0, 4, 0, 0]),
        (1, True): ([0, 0, 0, 4, 7, 0, 11, 0, 14, 0, 0, 0, 0, 0, 4], [0, 4, 0, 7, 11, 0, 14, 0, 15, 0, 4, 0, 4, 0, 7]),
        (2, True): ([0, 0, 0, 4, 0, 0, 11, 0, 14, 0, 0, 0, 0, 0, 4], [0, 4, 0, 7, 0, 0, 14, 0, 15, 0, 4, 0, 4, 0, 7]),
        (6, True): ([0] * 15, [0] * 15),
    }
    for (min_len, whole), (lb, ub) in stated.items():
        got = V.by_bytes(text, off, min_len, whole)
        assert got[0].tolist() == lb and got[1].tolist() == ub, (min_len, whole)
    pairs = V.pairs_by_bytes(text, off, 2, True)
    assert len(pairs) == 22 and pairs[:7] == [(1, 2, 0), (1, 7, 1), (1, 9, 2), (1, 13, 3), (3, 0, 0), (3, 5, 1), (3, 11, 3)]
    assert V.cli_text(off, pairs[:5]) == "0 0 2\n0 1 2\n0 2 2\n0 3 2\n0 0 4\n"


def test_cli_refuses_what_it_cannot_read_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "overlaps")
    (tmp_path / "reads").write_bytes(b"abab\nbabab\nab\nabab\n")
    (tmp_path / "empty").write_bytes(b"\n\n")
    for args, words in ((["-f", str(tmp_path / "reads"), "-l", "0"], "at least 1"), (["-f", str(tmp_path / "reads"), "-l", "x"], "no length"),
                        (["-f", str(tmp_path / "empty")], "empty input"), (["-f", str(tmp_path / "none")], "cannot open"),
                        (["-f", str(tmp_path / "reads"), "--index", "16"], "USAGE"), ([], "USAGE")):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and words in r.stderr, args
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-f", str(tmp_path / "reads"), "--list"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr


def test_the_reads_are_what_the_gpu_test_says():
    # the figures in the docstring of tests/test_gpu_overlaps.py
    for name, want in (("reads", ((2950, 3139), (3462, 3715))), ("reads_mut", ((742, 786), (1254, 1308)))):
        for whole in (False, True):
            lb, ub = V.slots(name, 16, whole)
            assert (int(np.count_nonzero(ub > lb)), int(np.sum(ub - lb))) == want[whole], (name, whole)
