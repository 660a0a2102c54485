"""The ordering rule of group_sort16_kernel's one counting round (psac_amd/csrc/group_rank.hpp) on the host (no GPU).

tests/cpp/test_group_rank.cpp runs the host model of tests/cpp/group_rank_model.hpp -- composite key, one counting round with the slots of a bucket in any
order, rank inside the bucket, the decision for the way back -- on the tables tests/cpp/group_sort16_direct.hip runs on the device, against
std::stable_sort by the 16 bits inside every group.
"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_group_rank_program(tmp_path):
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "test_group_rank")
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "psac_amd", "csrc"), "-o", exe,
           os.path.join(HERE, "cpp", "test_group_rank.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "group rank tests passed" in r.stdout, r.stdout[-4000:] + r.stderr
