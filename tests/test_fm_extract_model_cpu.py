"""Text samples and extraction of the FM-index on the CPU: the two statements of tests/fm_extract_model.py held to each other and to
the reader of any words, the sample arrays of the named sets pinned in tests/golden/fm_extract_named.json, what the scheme loses without
the samples of the string ends, the wrappers and exports, the C++ mirror compiling warning-free as C++11, and the new flags of fmindex."""
import json
import os
import subprocess

import numpy as np
import pytest

import fm_extract_model as X
import fm_model as F
import repeats_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [1, 2, 3, 8, 32]                                # and n + 5


def queries_of(strings, seed):
    """every whole string, every position alone, and random windows, some past their string's end, some empty, some at or beyond n"""
    t, off = M.flatten(strings)
    n = int(t.size)
    rng = np.random.RandomState(seed)
    pos = off[:-1].tolist() + list(range(n)) + rng.randint(0, n, 40).tolist() + [n, n + 3, 0, n - 1]
    ln = np.diff(off).tolist() + [1] * n + rng.randint(0, 20, 40).tolist() + [5, 1, 0, 0]
    return pos, ln


def check_two_ways(strings, seed=5, rates=None):
    t, off, SA, LCP = M.arrays_by_definition(strings)
    p = F.Pipeline(strings, SA, 2)
    blob, Y = F.blob_of(p, 4)
    pos, ln = queries_of(strings, seed)
    want = X.by_bytes(strings, pos, ln)
    assert want[0][-1] >= 2 * t.size - 1
    for rate in (rates or RATES + [int(t.size) + 5]):
        e = X.Extractor(strings, SA, rate)
        assert e.ts.size == t.size // rate + len(strings)
        assert np.array_equal(SA[e.ts[:t.size // rate]], (np.arange(t.size // rate) + 1) * rate - 1)
        assert np.array_equal(SA[e.ts[t.size // rate:]], off[1:] - 1)
        got = e.extract(pos, ln)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), rate
        assert e.strings() == [bytes(s) for s in strings], rate
        got = X.blob_extract(blob, Y, p.code, p.sigma, e.ts, rate, off, pos, ln)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), rate
        if len(strings) == 1:                           # one text may pass no offsets
            got = X.blob_extract(blob, Y, p.code, p.sigma, e.ts, rate, None, pos, ln)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), rate


@pytest.mark.parametrize("name", sorted(F.NAMED) + ["every_end"])
def test_named_sets_two_ways(name):
    check_two_ways(F.NAMED[name] if name in F.NAMED else X.EVERY_END)


@pytest.mark.parametrize("seed,sigma,m", [(1, 2, 5), (2, 4, 9), (3, 37, 4), (4, 1, 3), (5, 4, 1), (6, 1, 1)])
def test_random_sets_two_ways(seed, sigma, m):
    check_two_ways(F.random_set(64 + 17 * seed, m, seed, sigma), seed)


@pytest.mark.parametrize("name", sorted(F.NAMED))
def test_sample_arrays_of_the_named_sets_are_pinned(name):
    assert X.golden()[name] == json.loads(json.dumps(X.named_results(name)))
    if name == "mississippi":                          # SA 10 7 4 1 0 9 8 6 3 5 2: the ranks of the positions 1 3 5 7 9, then of 10
        assert X.golden()[name]["ts"]["2"] == [3, 8, 9, 1, 5, 0]


def test_without_the_end_samples_every_tail_behind_the_last_block_sample_is_lost():
    strings = F.NAMED["miss3"]
    SA = M.arrays_by_definition(strings)[2]
    assert X.Extractor(strings, SA, 4).strings() == strings
    # samples at 3 7 11 15 19: 11 and 19 start the next string, where w is STOP, and the last block [20, 23) has none
    assert X.Extractor(strings, SA, 4, end_samples=False).strings() == [b"mississi\0\0\0", b"misso\0\0\0", b"m\0\0\0"]
    assert X.Extractor(strings, SA, 2, end_samples=False).strings() == [b"mississipp\0", b"missour\0", b"mis\0"]
    assert X.Extractor(strings, SA, 1, end_samples=False).strings() == strings         # every position is a sample


def test_the_reader_is_total_on_garbage():
    strings = F.random_set(200, 9, 3, 4)
    t, off, SA, LCP = M.arrays_by_definition(strings)
    p = F.Pipeline(strings, SA, 2)
    blob, Y = F.blob_of(p, 4)
    pos, ln = queries_of(strings, 1)
    want = X.by_bytes(strings, pos, ln)
    rng = np.random.RandomState(2)
    junk = rng.randint(0, 2 ** 32, 2 * blob.size).astype(np.uint32).view(np.uint64)
    for rate in (1, 3, 32):
        ts = X.sample_arrays(strings, SA, rate)
        ones = np.full(ts.size, 0xFFFFFFFF, np.int64)
        got = X.blob_extract(blob, Y, p.code, p.sigma, ones, rate, off, pos, ln)        # every sample clamps to n: zeros of the right lengths
        assert np.array_equal(got[0], want[0]) and not got[1].any()
        got = X.blob_extract(junk, Y, p.code, p.sigma, ts, rate, off, pos, ln)
        assert np.array_equal(got[0], want[0]) and got[1].size == want[1].size
        got = X.blob_extract(blob, Y, p.code, p.sigma, rng.randint(0, 2 * t.size, ts.size), rate, off, pos, ln)
        assert np.array_equal(got[0], want[0]) and set(got[1].tolist()) <= set(t.tolist()) | {0}


def test_the_wrappers_and_exports_are_there():
    import psac_amd
    from psac_amd import _lib
    import inspect
    for name in ("fm_text_samples_device", "fm_extract_device"):
        assert callable(getattr(psac_amd, name)) and name in psac_amd.__all__, name
    for name in ("extract", "text", "context"):
        assert callable(getattr(psac_amd.FMIndex, name)), name
    assert inspect.signature(psac_amd.fm_index).parameters["text_rate"].default == 0
    assert inspect.signature(psac_amd.SuffixArray.fm_index).parameters["text_rate"].default == 0
    lib = _lib.load()
    for suf in ("u32", "u64"):
        for name, args in (("psacx_fm_text_samples_dev_", 8), ("psacx_fm_extract_dev_", 14)):
            assert name + suf in _lib.EXPORTS and len(getattr(lib, name + suf).argtypes) == args, name + suf


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe, lib = str(tmp_path / "test_fm_extract"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fm_extract.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "fm extract header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_fmindex_refuses_bad_extraction_flags(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "fmindex")
    (tmp_path / "set").write_bytes(b"mississippi\nmissouri\nmiss\n")
    (tmp_path / "pats").write_bytes(b"miss\n")
    text, pats, out = str(tmp_path / "set"), str(tmp_path / "pats"), str(tmp_path / "out")
    head = [exe, "-f", text, "-q", pats]
    for args in (head + ["--text-rate", "x"], head + ["--text-rate"], head + ["--restore", out], head + ["--text-rate", "0", "--restore", out],
                 head + ["--text-rate", "4", "--context", "3"], head + ["--occ", "--context", "3"], head + ["--text-rate", "4", "--occ", "--context", "x"],
                 head + ["--text-rate", "4", "--restore"]):
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "USAGE" in r.stderr, args
    assert not os.path.exists(out)
