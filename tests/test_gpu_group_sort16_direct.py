"""group_sort16_kernel in both its forms, launched on tables made on the host, leaves the records and tie bytes of std::stable_sort inside every group
(tests/cpp/group_sort16_direct.hip, built with the library): the parity program of test_gpu_prefix_sort_1w_parity.py sorts texts whose batches nearly
all hold several short groups; the tables here have the shape of 2^32 characters -- one group of some 256 records per batch -- and the edges of the
kernel's own decisions: the rows, the batch cut, the largest bucket that still takes the rank loop, the groups and chunks it must leave alone."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT = os.path.join(ROOT, "psac_amd", "bin", "group_sort16_direct")


def test_group_sort16_kernel_against_stable_sort():
    r = subprocess.run([DIRECT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    print(out[-3000:])
    assert r.returncode == 0, out[-3000:]
    assert "tables agree" in out
