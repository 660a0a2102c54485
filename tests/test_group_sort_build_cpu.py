"""The build leaves the parity program of the one-word prefix sort (tests/cpp/prefix_sort_1w_parity.hip, a target of
psac_amd/csrc/Makefile); tests/test_gpu_prefix_sort_1w_parity.py runs it on the GPU."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parity_program_is_built():
    path = os.path.join(ROOT, "psac_amd", "bin", "prefix_sort_1w_parity")
    assert os.path.isfile(path) and os.access(path, os.X_OK)
