"""group_sort16_kernel in its form that writes tie bits (psac_amd/csrc/radix.hpp, template argument BITS), with one counting round and with counting
rounds only, launched on tables made on the host (tests/cpp/group_sort16_bits_direct.hip, built with the library): the records must be those of
std::stable_sort inside every group and the words of bits those of the definition, entry by entry -- bit p set iff the places p - 1 and p lie in one
batch and agree above the suffix field.  The tables: those of test_gpu_group_sort16_direct.py at 1024 groups, and tables whose batches are full of
ties -- across the places 63 | 64 of a batch, across word borders, at the last record of a batch, none across the border of two groups with the same
16 bits, a run of 20 equal records behind the counting rounds, single groups of 385 .. 512 records, empty groups, a record count that is no multiple
of 64, first places beyond 2^32 that are no multiple of 64."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = os.path.join(ROOT, "psac_amd", "bin", "group_sort16_bits_direct")


def test_group_sort16_bits_kernel_against_stable_sort_and_the_definition():
    r = subprocess.run([DIRECT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    print(out[-4000:])
    assert r.returncode == 0, out[-4000:]
    assert "tables agree" in out
