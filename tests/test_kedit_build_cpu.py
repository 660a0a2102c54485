"""What the search with edits adds above the ABI builds without a GPU and fails loudly without one: tests/cpp/test_kedit.cpp (kedit of
include/suffix_array.hpp) compiles warning-free as C++11 against the library, the lists it states by hand are the model's, the
wrappers exist with their argument counts, the option has its index, and the command line refuses what it cannot read."""
import os
import subprocess

import kedit_model as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpp_program(tmp_path):
    exe, lib = str(tmp_path / "test_kedit"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_kedit.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "kedit header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_the_lists_the_cpp_program_states_by_hand():
    cols = lambda got: [a.tolist() for a in got]  # noqa: E731
    t, off, SA, pats = K.named_arrays("mississippi")
    assert cols(K.by_pieces(t, off, SA, pats, 0)[0]) == [[0, 0, 2, 4], [1, 4, 0, 6], [4, 4, 1, 3], [0, 0, 0, 0]]
    one = K.by_pieces(t, off, SA, pats, 1)[0]
    assert cols(one) == [[0, 0, 0, 0, 0, 0, 1, 4, 4, 4, 4], [0, 1, 2, 3, 4, 5, 5, 3, 5, 6, 7], [5, 4, 3, 5, 4, 3, 5, 2, 4, 3, 2],
                         [1, 0, 1, 1, 0, 1, 1, 1, 1, 0, 1]]
    assert cols(K.best(one)) == [[0, 0, 1, 4], [1, 4, 5, 6], [4, 4, 5, 3], [0, 0, 1, 0]]
    assert K.by_pieces(t, off, SA, pats, 2)[0][0].size == 22
    t, off, SA, pats = K.named_arrays("abcab_cab")
    assert cols(K.by_pieces(t, off, SA, pats, 0)[0]) == [[0, 0, 1, 2], [2, 5, 0, 1], [3, 3, 3, 2], [0, 0, 0, 0]]
    assert cols(K.best(K.by_pieces(t, off, SA, pats, 1)[0])) == [[0, 0, 1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4], [2, 5, 0, 1, 0, 1, 2, 3, 4, 5, 6, 7, 0],
                                                                 [3, 3, 3, 2, 2, 1, 1, 2, 1, 1, 2, 1, 5], [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1]]
    for name in K.NAMED:                                      # and by the definition
        t, off, SA, pats = K.named_arrays(name)
        for e in (0, 1, 2):
            assert cols(K.by_pieces(t, off, SA, pats, e)[0]) == cols(K.by_definition(t, off, pats, e))


def test_the_wrappers_are_there():
    import psac_amd
    from psac_amd import _lib
    for name in ("kedit_device", "kedit"):
        assert callable(getattr(psac_amd, name)) and name in psac_amd.__all__, name
    assert callable(psac_amd.SuffixArray.kedit) and psac_amd.KEDIT_BEST == _lib.PSACX_KEDIT_BEST == 1
    for name in ("psacx_kedit_dev_u32", "psacx_kedit_dev_u64", "psacx_kedit_u32", "psacx_kedit_u64"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    header = open(os.path.join(ROOT, "include", "psacx.h")).read()
    assert "#define PSACX_KEDIT_BEST 1u" in header
    enum = header[header.index("PSACX_OPT_RESET = 0"):header.index("PSACX_OPT_COUNT")].replace("= 0", "").replace("\n", " ")
    names = [x.strip() for x in enum.split(",") if x.strip()]
    assert names.index("PSACX_OPT_KMISMATCH_STOP") == _lib.KERNEL_OPTIONS["kmismatch_stop"] == 28  # (the indices before it keep their values)
    assert names.index("PSACX_OPT_KEDIT_STOP") == _lib.KERNEL_OPTIONS["kedit_stop"] == 29 == len(names) - 1   # (tools/kedit_time.py times the stages by it)
    for suf in ("u32", "u64"):
        assert len(getattr(_lib.load(), "psacx_kedit_dev_" + suf).argtypes) == 21
        assert len(getattr(_lib.load(), "psacx_kedit_" + suf).argtypes) == 19


def test_cli_refuses_what_it_cannot_read_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "kedit")
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
        r = subprocess.run([exe, "-f", text, "-q", pats, "-e", "1", "--best", "--list"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
