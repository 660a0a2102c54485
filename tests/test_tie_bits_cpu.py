"""The rules of the tie bits (psac_amd/csrc/tie_bits.hpp) on the host (no GPU).

tests/cpp/test_tie_bits.cpp puts the words of random and hand-made batches together the way group_sort16_kernel<.., BITS> does -- row by row, two
words per row, merged in any order -- and compares them bit by bit with the definition; it finds the leaders and lengths of the tie groups of bit
streams with the functions the tie scan uses and compares them with a walk over the bits.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_tie_bits_program(tmp_path):
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "test_tie_bits")
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "psac_amd", "csrc"), "-o", exe,
           os.path.join(HERE, "cpp", "test_tie_bits.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "tie bit tests passed" in r.stdout, r.stdout[-4000:] + r.stderr


def test_the_option_value_and_the_stats_field_are_there():
    from psac_amd import _lib
    names = [f[0] for f in _lib.Stats._fields_]
    assert names.index("tie_form") == names.index("group_sort") + 1 and _lib.Stats.tie_form.size == 8
    assert (_lib.PSACX_SIDE_PLAIN, _lib.PSACX_SIDE_TIE_BYTES) == (1, 2)
    with open(os.path.join(os.path.dirname(HERE), "include", "psacx.h")) as f:
        header = f.read()
    assert header.index("uint64_t group_sort;") < header.index("uint64_t tie_form;") < header.index("uint64_t grid_cuts;")
    assert "2 = TIE_BYTES" in header
