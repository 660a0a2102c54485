"""What the search with mismatches adds above the ABI builds without a GPU and fails loudly without one: tests/cpp/test_kmismatch.cpp
(kmismatch of include/suffix_array.hpp) compiles warning-free as C++11 against the library, the lists it states by hand are the
model's, the wrappers exist, and the command line refuses what it cannot read."""
import os
import subprocess

import kmismatch_model as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpp_program(tmp_path):
    exe, lib = str(tmp_path / "test_kmismatch"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_kmismatch.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "kmismatch header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_the_lists_the_cpp_program_states_by_hand():
    cols = lambda got: [a.tolist() for a in got]  # noqa: E731
    t, off, SA, pats = X.named_arrays("mississippi")
    assert cols(X.by_pieces(t, off, SA, pats, 0)[0]) == [[0, 0, 2, 4], [4, 1, 0, 6], [0, 0, 0, 0]]
    assert cols(X.by_pieces(t, off, SA, pats, 1)[0]) == [[0, 0, 1, 4, 4], [4, 1, 5, 6, 3], [0, 0, 1, 0, 1]]
    assert X.by_pieces(t, off, SA, pats, 2)[0][0].size == 10
    t, off, SA, pats = X.named_arrays("abcab_cab")
    assert cols(X.by_pieces(t, off, SA, pats, 0)[0]) == [[0, 0, 1, 2], [2, 5, 0, 1], [0, 0, 0, 0]]
    assert cols(X.by_pieces(t, off, SA, pats, 1)[0]) == [[0, 0, 1, 2, 3, 3, 3, 3, 3], [2, 5, 0, 1, 2, 5, 3, 6, 0], [0, 0, 0, 0, 1, 1, 1, 1, 1]]


def test_the_wrappers_are_there():
    import psac_amd
    from psac_amd import _lib
    for name in ("kmismatch_device", "kmismatch"):
        assert callable(getattr(psac_amd, name)) and name in psac_amd.__all__, name
    assert callable(psac_amd.SuffixArray.kmismatch)
    for name in ("psacx_kmismatch_dev_u32", "psacx_kmismatch_dev_u64", "psacx_kmismatch_u32", "psacx_kmismatch_u64"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    header = open(os.path.join(ROOT, "include", "psacx.h")).read()
    enum = header[header.index("PSACX_OPT_RESET = 0"):header.index("PSACX_OPT_COUNT")].replace("= 0", "").replace("\n", " ")
    names = [x.strip() for x in enum.split(",") if x.strip()]
    assert names.index("PSACX_OPT_MEMS_STOP") == _lib.KERNEL_OPTIONS["mems_stop"] == 27           # (the indices before it keep their values)
    assert names.index("PSACX_OPT_KMISMATCH_STOP") == _lib.KERNEL_OPTIONS["kmismatch_stop"] == 28  # (tools/kmismatch_time.py times the stages by it)
    for suf in ("u32", "u64"):
        assert len(getattr(_lib.load(), "psacx_kmismatch_dev_" + suf).argtypes) == 19
        assert len(getattr(_lib.load(), "psacx_kmismatch_" + suf).argtypes) == 17


def test_cli_refuses_what_it_cannot_read_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "kmismatch")
    (tmp_path / "text").write_bytes(b"mississippi")
    (tmp_path / "pats").write_bytes(b"issi\nssippx\n")
    (tmp_path / "empty").write_bytes(b"")
    (tmp_path / "lines").write_bytes(b"\n\n")
    text, pats = str(tmp_path / "text"), str(tmp_path / "pats")
    for args, words in ((["-f", str(tmp_path / "empty"), "-q", pats, "-e", "1"], "empty input"),
                        (["-f", str(tmp_path / "lines"), "-q", pats, "-e", "1", "--set"], "empty input"),
                        (["-f", str(tmp_path / "none"), "-q", pats, "-e", "1"], "cannot open"),
                        (["-f", text, "-q", str(tmp_path / "none"), "-e", "1"], "cannot open"),
                        (["-f", text, "-q", pats, "-e", "1", "--index", "16"], "USAGE"), (["-f", text, "-q", pats], "USAGE"),
                        (["-f", text, "-e", "1"], "USAGE"), (["-f", text, "-q", pats, "-e", "x"], "USAGE"),
                        (["-f", text, "-q", pats, "-e", "16"], "USAGE"), (["-f", text, "-q", pats, "-e", "1", "--max-cand", "x"], "USAGE"),
                        (["-f", text, "-q", pats, "-e", "1", "--edit"], "USAGE"), ([], "USAGE")):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and words in r.stderr, args
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-f", text, "-q", pats, "-e", "1", "--list"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
