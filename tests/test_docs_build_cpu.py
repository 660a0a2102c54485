"""What the document counts and lists add above the ABI builds without a GPU and fails loudly without one: tests/cpp/test_docs.cpp
(doc_count, doc_list and common_repeats of include/suffix_array.hpp) compiles warning-free as C++11 against the library, the lists it
states by hand are the model's, and the wrappers exist."""
import os
import subprocess

import numpy as np

import docs_model as D
import repeats_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpp_program(tmp_path):
    exe, lib = str(tmp_path / "test_docs"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_docs.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "docs header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_the_lists_the_cpp_program_states_by_hand():
    strings = D.NAMED["miss"]
    t, off, SA, LCP = M.arrays_by_definition(strings)
    assert SA.tolist() == [10, 18, 7, 20, 4, 1, 12, 19, 0, 11, 15, 9, 8, 17, 22, 6, 3, 14, 21, 5, 2, 13, 16]
    prev, dup = D.index_of(SA, LCP, off)
    lb, ub = np.array([7, 18, 0, 19, 10, 14, 0]), np.array([10, 22, 7, 21, 11, 22, 0])
    assert [D.locate(strings, SA, p) for p in (b"miss", b"ss", b"i", b"ssi", b"ouri", b"s")] == list(zip(lb[:6].tolist(), ub[:6].tolist()))
    assert D.count_by_dup(dup, lb, ub, 23).tolist() == [3, 3, 3, 1, 1, 3, 0]
    start, _, sid, pos = D.list_by_prev(prev, SA, off, lb, ub, 23)
    assert start.tolist() == [0, 3, 6, 9, 10, 11, 14, 14] and sid.tolist() == [2, 0, 1, 2, 0, 1, 0, 1, 2, 0, 1, 2, 0, 1]
    assert pos.tolist() == [19, 0, 11, 21, 5, 13, 10, 18, 20, 5, 15, 22, 6, 14]
    assert D.count_by_dup(dup, [0, 22, 0], [1, 23, 23], 23).tolist() == [1, 1, 3]
    start, _, sid, pos = D.list_by_prev(prev, SA, off, [3, 9], [9, 3], 23)
    assert start.tolist() == [0, 3, 3] and sid.tolist() == [2, 0, 1] and pos.tolist() == [20, 4, 12]
    rlb, rub, rln = M.triples(M.by_intervals(LCP))
    docs = D.count_by_dup(dup, rlb, rub, 23)
    keep = docs >= 3
    assert rlb[keep].tolist() == [0, 3, 7, 14, 18] and rub[keep].tolist() == [7, 7, 10, 22, 22] and rln[keep].tolist() == [1, 3, 4, 1, 2]
    assert rlb[docs == 1].tolist() == [4, 11, 15, 19] and rln[docs == 1].tolist() == [4, 1, 2, 3]
    t, off, SA, LCP = M.arrays_by_definition([b"abab", b"ab"])
    prev, dup = D.index_of(SA, LCP, off)
    assert D.count_by_dup(dup, [0, 0], [3, 2], 6).tolist() == [2, 1]
    start, _, sid, pos = D.list_by_prev(prev, SA, off, [0, 3], [6, 6], 6)
    assert start.tolist() == [0, 2, 4] and sid.tolist() == [0, 1, 0, 1] and pos.tolist() == [2, 4, 3, 5]


def test_the_wrappers_are_there():
    import psac_amd
    from psac_amd import _lib
    for name in ("doc_index_device", "doc_count_device", "doc_list_device", "doc_count", "doc_list"):
        assert callable(getattr(psac_amd, name)), name
    for name in ("doc_count", "doc_list", "common_repeats"):
        assert callable(getattr(psac_amd.SuffixArray, name)), name
    lib = _lib.load()
    for suf in ("u32", "u64"):
        for name, args in (("psacx_doc_index_dev_", 9), ("psacx_doc_count_dev_", 7), ("psacx_doc_list_dev_", 15), ("psacx_doc_count_", 10), ("psacx_doc_list_", 14)):
            assert name + suf in _lib.EXPORTS and len(getattr(lib, name + suf).argtypes) == args, name + suf


def test_clis_refuse_the_flags_without_a_set_and_fail_loudly_without_a_gpu(tmp_path):
    locate, repeats = os.path.join(ROOT, "psac_amd", "bin", "locate"), os.path.join(ROOT, "psac_amd", "bin", "repeats")
    (tmp_path / "set").write_bytes(b"mississippi\nmissouri\nmiss\n")
    (tmp_path / "pats").write_bytes(b"miss\n")
    text, pats = str(tmp_path / "set"), str(tmp_path / "pats")
    for args in ([locate, "-f", text, "-q", pats, "--docs"], [locate, "-f", text, "-q", pats, "--doc-list", "3"], [repeats, "-f", text, "--min-docs", "2"],
                 [repeats, "-f", text, "--set", "--max-docs", "2"], [repeats, "-f", text, "--set", "--min-docs", "x"]):
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "USAGE" in r.stderr, args
    import torch
    if not torch.cuda.is_available():
        for args in ([locate, "-f", text, "-q", pats, "--set", "--docs", "--doc-list"], [repeats, "-f", text, "--set", "--min-docs", "2"]):
            r = subprocess.run(args, capture_output=True, text=True)
            assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr, args
