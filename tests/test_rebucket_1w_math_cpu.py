"""The 32-bit arithmetic of rebucket_first_1w_kernel against the generic kernel's formulas, on the host (no GPU).

psac_amd/csrc/rebucket_1w_math.hpp holds what differs between the two kernels as small functions a host compiler can include:
bits -> characters without a division, the LCP of two leading parts, the short-suffix test and cap, and the rank / id relation.
tests/cpp/test_rebucket_1w_math.cpp checks them against the generic forms, at n = 2^32 too, which no small GPU test reaches.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_rebucket_1w_math_program(tmp_path):
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "test_rebucket_1w_math")
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "psac_amd", "csrc"), "-o", exe,
           os.path.join(HERE, "cpp", "test_rebucket_1w_math.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "rebucket 1w math tests passed" in r.stdout, r.stdout + r.stderr
