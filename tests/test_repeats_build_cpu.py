"""What the BWT and repeat calls add above the ABI builds without a GPU and fails loudly without one: tests/cpp/test_repeats.cpp (bwt
and repeats of include/suffix_array.hpp) compiles warning-free as C++11 against the library, the lists it states by hand are the
model's, the wrappers exist, and the command line refuses what it cannot read."""
import os
import subprocess

import numpy as np

import repeats_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpp_program(tmp_path):
    exe, lib = str(tmp_path / "test_repeats"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_repeats.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "repeats header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_the_lists_the_cpp_program_states_by_hand():
    g = M.golden()
    cols = lambda rows: [list(c) for c in zip(*rows)]  # noqa: E731
    mi = g["mississippi"]
    assert bytes(mi["bwt"]) == b"pssmipissii" and mi["primary"] == 4
    assert cols(mi["right"]) == [[0, 2, 5, 7, 7, 9], [4, 4, 7, 9, 11, 11], [1, 4, 1, 2, 1, 3]]
    assert cols(mi["maximal"]) == [[0, 2, 5, 7], [4, 4, 7, 11], [1, 4, 1, 1]] and cols(mi["super"]) == [[2, 5], [4, 7], [4, 1]]
    r = M.by_intervals(mi["LCP"])
    assert [x[1] for x in M.select(r, 2, 2, 2)] == [2, 7, 9] and [x[3] for x in M.select(r, 2, 2, 2)] == [4, 2, 3]
    ba = g["banana"]
    assert bytes(ba["bwt"]) == b"nnbaaa" and ba["primary"] == 3
    assert cols(ba["maximal"]) == [[0, 1], [3, 3], [1, 3]] and ba["super"] == [[1, 3, 3]]
    ab = g["abcab_cab"]
    assert bytes(ab["bwt"]) == b"ccbaaabb" and ab["primary"] == 2
    assert cols(ab["right"]) == [[0, 3, 6], [3, 6, 8], [2, 1, 3]] and cols(ab["maximal"]) == [[0, 6], [3, 8], [2, 3]] and ab["super"] == [[6, 8, 3]]


def test_the_wrappers_are_there():
    import psac_amd
    from psac_amd import _lib
    for name in ("bwt_device", "repeats_device", "bwt", "bwt_decode", "repeats"):
        assert callable(getattr(psac_amd, name)), name
    assert callable(psac_amd.SuffixArray.bwt) and callable(psac_amd.SuffixArray.repeats)
    assert psac_amd.REPEATS_KINDS["right"] == 0 and psac_amd.REPEATS_KINDS["maximal"] == 1 and psac_amd.REPEATS_KINDS["super"] == 2
    for name in ("psacx_bwt_dev_u32", "psacx_bwt_dev_u64", "psacx_repeats_dev_u32", "psacx_repeats_dev_u64", "psacx_bwt_u32", "psacx_bwt_u64",
                 "psacx_repeats_u32", "psacx_repeats_u64"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    assert psac_amd.bwt_decode(np.frombuffer(b"nnbaaa", np.uint8), 3) == b"banana"


def test_cli_refuses_what_it_cannot_read_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "repeats")
    (tmp_path / "text").write_bytes(b"mississippi")
    (tmp_path / "empty").write_bytes(b"")
    (tmp_path / "lines").write_bytes(b"\n\n")
    text = str(tmp_path / "text")
    for args, words in ((["-f", str(tmp_path / "empty")], "empty input"), (["-f", str(tmp_path / "lines"), "--set"], "empty input"),
                        (["-f", str(tmp_path / "none")], "cannot open"), (["-f", text, "--index", "16"], "USAGE"),
                        (["-f", text, "--kind", "tandem"], "USAGE"), (["-f", text, "-l", "x"], "USAGE"), ([], "USAGE")):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and words in r.stderr, args
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-f", text, "--list", "--kind", "super"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
