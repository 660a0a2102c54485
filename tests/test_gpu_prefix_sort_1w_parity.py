"""prefix_sort_1w in its group form leaves the records and tie bytes of the LSD bucket passes, bit for bit (tests/cpp/prefix_sort_1w_parity.hip,
built with the library): the constructions of test_gpu_group_sort.py cannot see the order among records that tie on the prefix."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "psac_amd", "bin", "prefix_sort_1w_parity")


def test_prefix_sort_1w_records_agree():
    r = subprocess.run([PARITY], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    print(out[-3000:])
    assert r.returncode == 0, out[-3000:]
    assert "cases agree" in out
