"""The layouts of the sorter's scratch (psac_amd/csrc/sort_scratch.hpp) on the host (no GPU).

tests/cpp/test_sort_scratch.cpp walks sizes, tile shapes and bucket distributions (tests/cpp/sort_scratch_sweep.hpp) and
  1. prints every value -- the pass layout, sort_desc_bytes, every offset of the one-word layouts with and without the group form, the
     two allocation bounds -- and this test compares them, all of them and nothing else, with tests/golden/sort_scratch_layout.json: the values
     the functions of the commit named in that file gave (engine.hpp, construct.hpp: carve, multi_first_round.hpp: sort_first_one_word before the
     layouts moved into one header; recorded by a host program that included that commit's engine.hpp and walked the same sweep);
  2. checks that the regions of every layout are disjoint and aligned, that a pass of n records fits sort_desc_bytes(n), and that each bound
     covers the exact need of every layout it is used to allocate for.
"""
import json
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_sort_scratch_program(tmp_path):
    root = os.path.dirname(HERE)
    exe = str(tmp_path / "test_sort_scratch")
    cmd = ["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(root, "psac_amd", "csrc"), "-o", exe,
           os.path.join(HERE, "cpp", "test_sort_scratch.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "sort scratch tests passed" in r.stdout, r.stdout[-4000:] + r.stderr
    got = {}
    for line in r.stdout.splitlines():
        if "|" in line:
            name, values = line.split("|")
            assert name not in got
            got[name] = [int(v) for v in values.split()]
    with open(os.path.join(HERE, "golden", "sort_scratch_layout.json")) as f:
        golden = json.load(f)
    assert len(golden["parent"]) == 40
    want = golden["values"]
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, list(wrong.items())[:5]
