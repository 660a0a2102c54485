"""What the LZ77 calls add above the ABI builds without a GPU and fails loudly without one: tests/cpp/test_lz77.cpp (lz77 of
include/suffix_array.hpp) compiles warning-free as C++11 against the library, the phrases it states by hand are the model's, the
option that shrinks the parse's tiles is known by name, and the command line refuses what it cannot read."""
import os
import subprocess

import lz_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cpp_program(tmp_path):
    exe, lib = str(tmp_path / "test_lz77"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_lz77.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "lz77 header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_the_phrases_the_cpp_program_states_by_hand():
    for name, start, src in (("mississippi", [0, 1, 2, 3, 4, 8, 9, 10, 11], [-1, -1, -1, 2, 1, -1, 8, 7]), ("a300", [0, 1, 300], [-1, 0]),
                             ("abcab", [0, 1, 2, 100, 101, 201], [-1, -1, 0, -1, 0])):
        got = M.parse(*M.by_bytes(M.text_of(name)))
        assert got[0].tolist() == start and got[1].tolist() == src, name


def test_the_option_and_the_wrappers_are_there():
    import psac_amd
    from psac_amd import _lib
    assert _lib.OPTIONS["lz_small_tiles"] == 24
    # the option that cuts the grids of the stride loops, the next number, and the counter of the cut launches: the last field of the
    # statistics, as in include/psacx.h
    assert _lib.OPTIONS["grid_cap"] == 25 == max(_lib.OPTIONS.values()) and len(set(_lib.OPTIONS.values())) == len(_lib.OPTIONS)
    assert _lib.Stats._fields_[-1][0] == "grid_cuts" and _lib.Stats.grid_cuts.size == 8
    with open(os.path.join(ROOT, "include", "psacx.h")) as f:
        header = f.read()
    enum = header[header.index("PSACX_OPT_RESET = 0"):header.index("PSACX_OPT_COUNT")].replace("= 0", "").replace("\n", " ")
    names = [x.strip() for x in enum.split(",") if x.strip()]
    assert names.index("PSACX_OPT_GRID_CAP") == 25 and names.index("PSACX_OPT_LZ_SMALL_TILES") == 24
    assert header.index("uint64_t grid_cuts;") > header.index("uint64_t group_sort;") and header.index("} psacx_stats;") > header.index("uint64_t grid_cuts;")
    for name in ("lpf_device", "lz77_device", "check_lz77_device", "lpf", "lz77", "lz77_decode"):
        assert callable(getattr(psac_amd, name)), name
    start, src = M.parse_of("mississippi")
    import numpy as np
    u = np.where(src == M.ONES, 0xFFFFFFFF, src).astype(np.uint32)
    literals = b"mis\0\0\0\0\0p\0\0"                                   # the decoder reads the text at literal phrases only
    assert psac_amd.lz77_decode(start.astype(np.uint32), u, literals) == b"mississippi"


def test_cli_refuses_what_it_cannot_read_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "lz77")
    (tmp_path / "text").write_bytes(b"mississippi")
    (tmp_path / "empty").write_bytes(b"")
    for args, words in ((["-f", str(tmp_path / "empty")], "empty input"), (["-f", str(tmp_path / "none")], "cannot open"),
                        (["-f", str(tmp_path / "text"), "--index", "16"], "USAGE"), ([], "USAGE")):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and words in r.stderr, args
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-f", str(tmp_path / "text"), "--list", "-c"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
