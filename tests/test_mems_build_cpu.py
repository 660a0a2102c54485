"""What the maximal-exact-match calls add above the ABI builds without a GPU and fails loudly without one: tests/cpp/test_mems.cpp (mems
of include/suffix_array.hpp) compiles warning-free as C++11 against the library, the lists it states by hand are the model's, the
wrappers exist, and the command line refuses what it cannot read."""
import os
import subprocess

import mems_model as X
import repeats_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpp_program(tmp_path):
    exe, lib = str(tmp_path / "test_mems"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_mems.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "mems header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_the_lists_the_cpp_program_states_by_hand():
    cols = lambda rows: [list(c) for c in zip(*rows)]  # noqa: E731
    t, off, SA, LCP, bwt, first, pats = X.named_arrays("mississippi")
    stats = X.statistics(t, SA, pats)
    walk = lambda *a: X.by_walk(SA, LCP, bwt, first, pats, stats, *a)[0]  # noqa: E731
    assert cols(walk(3)) == [[0, 0, 3, 8], [1, 4, 1, 6], [7, 4, 4, 3]]
    assert cols(walk(2)) == [[0, 0, 3, 8, 8], [1, 4, 1, 6, 3], [7, 4, 4, 3, 2]]
    assert len(walk(1)) == 24 and walk(0) == walk(1)
    assert cols(walk(3, 1)) == [[0, 8], [1, 6], [7, 3]]
    assert cols(walk(1, 0, True)) == [[0, 7, 8], [1, 0, 6], [7, 1, 3]]
    strings, pats = [b"abcab", b"cab"], [b"bcabc", b"", b"ca"]
    t, off, SA, LCP = R.arrays_by_definition(strings)
    bwt, first, _ = R.bwt_of(t, SA, off)
    stats = X.statistics(t, SA, pats, off)
    assert cols(X.by_walk(SA, LCP, bwt, first, pats, stats, 2)[0]) == [[0, 1, 2, 5, 5], [1, 5, 0, 2, 5], [4, 3, 3, 2, 2]]
    assert cols(X.by_walk(SA, LCP, bwt, first, pats, stats, 2, 0, True)[0]) == [[0, 2, 5, 5], [1, 0, 2, 5], [4, 3, 2, 2]]


def test_the_wrappers_are_there():
    import psac_amd
    from psac_amd import _lib
    for name in ("mems_device", "mems"):
        assert callable(getattr(psac_amd, name)), name
    assert callable(psac_amd.SuffixArray.mems)
    assert psac_amd.MEMS_SUPER == 1 and _lib.PSACX_MEMS_SUPER == 1
    for name in ("psacx_mems_dev_u32", "psacx_mems_dev_u64", "psacx_mems_u32", "psacx_mems_u64"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name), name
    header = open(os.path.join(ROOT, "include", "psacx.h")).read()
    enum = header[header.index("PSACX_OPT_RESET = 0"):header.index("PSACX_OPT_COUNT")].replace("= 0", "").replace("\n", " ")
    names = [x.strip() for x in enum.split(",") if x.strip()]
    assert names.index("PSACX_OPT_MEMS_STOP") == _lib.KERNEL_OPTIONS["mems_stop"] == 27      # (tools/mems_time.py times the stages by it)
    for suf in ("u32", "u64"):
        assert len(getattr(_lib.load(), "psacx_mems_dev_" + suf).argtypes) == 22 and len(getattr(_lib.load(), "psacx_mems_" + suf).argtypes) == 19


def test_cli_refuses_what_it_cannot_read_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "mems")
    (tmp_path / "text").write_bytes(b"mississippi")
    (tmp_path / "pats").write_bytes(b"ississim\nsip\n")
    (tmp_path / "empty").write_bytes(b"")
    (tmp_path / "lines").write_bytes(b"\n\n")
    text, pats = str(tmp_path / "text"), str(tmp_path / "pats")
    for args, words in ((["-f", str(tmp_path / "empty"), "-q", pats, "-l", "1"], "empty input"),
                        (["-f", str(tmp_path / "lines"), "-q", pats, "-l", "1", "--set"], "empty input"),
                        (["-f", str(tmp_path / "none"), "-q", pats, "-l", "1"], "cannot open"),
                        (["-f", text, "-q", str(tmp_path / "none"), "-l", "1"], "cannot open"),
                        (["-f", text, "-q", pats, "-l", "1", "--index", "16"], "USAGE"), (["-f", text, "-q", pats], "USAGE"),
                        (["-f", text, "-l", "1"], "USAGE"), (["-f", text, "-q", pats, "-l", "x"], "USAGE"),
                        (["-f", text, "-q", pats, "-l", "1", "--max-occ", "x"], "USAGE"), (["-f", text, "-q", pats, "-l", "1", "--mum"], "USAGE"),
                        ([], "USAGE")):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and words in r.stderr, args
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-f", text, "-q", pats, "-l", "2", "--list", "--super"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
