"""The build leaves the parity program of the top-digit histogram kernels (tests/cpp/top_digit_hist_parity.hip, a target of
psac_amd/csrc/Makefile); tests/test_gpu_side_kernels.py runs it on the GPU."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parity_program_is_built():
    path = os.path.join(ROOT, "psac_amd", "bin", "top_digit_hist_parity")
    assert os.path.isfile(path) and os.access(path, os.X_OK)
