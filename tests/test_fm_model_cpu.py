"""The FM-index on the CPU: the two statements of tests/fm_model.py held to each other, to the locate models on patterns that occur, and
to the blob the header describes; the two mistakes the header warns of, pinned; the golden file; the wrappers and exports; the C++
mirror compiles warning-free as C++11 and fails loudly without a GPU; fmindex refuses bad flags."""
import json
import os
import subprocess

import numpy as np
import pytest

import fm_model as F
import locate_gsa_model as G
import locate_model as L
import repeats_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_sets():
    out = [F.random_set(60, 5, seed, sigma) for seed, sigma in ((1, 2), (2, 4), (3, 7), (4, 3))]
    out.append([b"a", b"b", b"c", b"abc", b"cab", b"bca", b"c"])           # strings that end in every symbol, one-byte strings
    out.append([b"aaaaaaa"])
    out.append([bytes([1 + (i * 7) % 11 for i in range(70)])])
    return out


def patterns_for(strings, seed):
    rng = np.random.RandomState(seed)
    t, off = M.flatten(strings)
    pats = [b""]
    for _ in range(25):
        a = int(rng.randint(0, t.size))
        pats.append(t[a:a + int(rng.randint(1, 6))].tobytes())               # occurs in the flat text, maybe only across a boundary
    alphabet = sorted(set(t.tolist()))
    for _ in range(10):
        pats.append(bytes(alphabet[int(x)] for x in rng.randint(0, len(alphabet), int(rng.randint(1, 5)))))
    pats += [bytes(s) for s in strings[:3]] + [b"\xff", bytes([alphabet[0], 255])]
    return pats


@pytest.mark.parametrize("name", sorted(F.NAMED))
def test_named_inputs_two_ways_and_golden(name):
    strings = F.NAMED[name]
    t, off, SA, LCP = M.arrays_by_definition(strings)
    want = F.golden()[name]
    assert want == json.loads(json.dumps(F.named_results(name)))
    for sample in (0, 1, 2, 3, 8):
        p = F.Pipeline(strings, SA, sample)
        for row in want["patterns"]:
            P = bytes(row["pattern"])
            assert p.search(P) == (row["lb"], row["ub"]), (name, P)
            if sample:
                assert p.locate(P) == row["pos"], (name, P, sample)
        if sample:
            assert [p.walk(r)[0] for r in range(p.n)] == SA.tolist()


def test_the_two_mistakes_the_header_warns_of():
    strings = F.NAMED["mississippi"]
    t, off, SA, LCP = M.arrays_by_definition(strings)
    assert SA.tolist() == [10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2]
    p = F.Pipeline(strings, SA)
    assert p.search(b"iss") == (2, 4) and p.search(b"ippi") == (1, 2)
    assert F.by_bytes(strings, SA, b"iss")[:2] == (2, 4) and F.by_bytes(strings, SA, b"ippi")[:2] == (1, 2)
    assert F.Pipeline(strings, SA, use_E=False).search(b"iss") == (1, 3)              # without E[c]
    assert F.Pipeline(strings, SA, lf_first_step=True).search(b"ippi") == (0, 0)      # [0, n) pushed through LF on the first byte
    for r in range(p.n):                                                              # SA[LF(r)] = SA[r] - 1
        if p.w[r]:
            assert SA[p.lf(r)] == SA[r] - 1


@pytest.mark.parametrize("k", range(7))
def test_random_sets_two_ways_and_against_locate(k):
    strings = random_sets()[k]
    t, off, SA, LCP = M.arrays_by_definition(strings)
    p = F.Pipeline(strings, SA, 3)
    single = len(strings) == 1
    for P in patterns_for(strings, 10 + k):
        lb, ub, pos = F.by_bytes(strings, SA, P)
        assert p.search(P) == (lb, ub), P
        assert p.locate(P) == pos
        assert p.locate(P, limit=2) == pos[:2]
        if ub > lb:                                     # a pattern that occurs: locate's interval
            assert (L.by_bisection(t, SA, P) if single else G.by_bisection(t, off, SA, P)) == (lb, ub), P
    for r in range(p.n):
        if p.w[r]:
            assert SA[p.lf(r)] == SA[r] - 1
    assert int(p.E.sum()) == len(strings) and int(p.cnt.sum()) == p.n


@pytest.mark.parametrize("itemsize", [4, 8])
def test_the_blob_of_the_header_answers_as_the_pipeline(itemsize):
    for strings in [F.NAMED["miss3"], F.NAMED["aa4"]] + random_sets()[:5]:
        t, off, SA, LCP = M.arrays_by_definition(strings)
        for sample in (0, 1, 3, 100):
            p = F.Pipeline(strings, SA, sample)
            blob, Y = F.blob_of(p, itemsize)
            assert blob.size == Y["words"] and 8 * Y["words"] <= F.size_bound_bytes(p.n, p.bits, sample, int(p.val.size), itemsize)
            for P in patterns_for(strings, 5):
                assert F.blob_search(blob, Y, p.code, p.sigma, P) == p.search(P), P
            if sample:
                assert [F.blob_walk(blob, Y, p.sigma, r) for r in range(p.n)] == SA.tolist()


def test_garbage_blobs_have_total_answers():
    strings = F.random_set(200, 6, 9, 4)
    t, off, SA, LCP = M.arrays_by_definition(strings)
    p = F.Pipeline(strings, SA, 4)
    good, Y = F.blob_of(p, 4)
    rng = np.random.RandomState(1)
    junk = rng.randint(0, 2 ** 32, 2 * good.size).astype(np.uint32).view(np.uint64)
    clear = good.copy()
    clear[Y["marks_at"]:Y["val_at"]] = 0                # marks all clear, sample = 4
    for blob in (junk, clear):
        for P in patterns_for(strings, 3):
            lb, ub = F.blob_search(blob, Y, p.code, p.sigma, P)
            assert 0 <= lb <= ub <= p.n
        for r in range(p.n):
            v = F.blob_walk(blob, Y, p.sigma, r)
            assert 0 <= v <= 0xFFFFFFFF
    assert all(F.blob_walk(clear, Y, p.sigma, r) == 0xFFFFFFFF for r in range(p.n))


def test_the_values_the_cpp_program_states_by_hand():
    strings = F.NAMED["mississippi"]
    t, off, SA, LCP = M.arrays_by_definition(strings)
    p = F.Pipeline(strings, SA, 2)
    pats = [b"iss", b"ippi", b"i", b"x", b"", b"mississippi", b"im"]
    assert [p.search(P) for P in pats] == [(2, 4), (1, 2), (0, 4), (0, 0), (0, 11), (4, 5), (0, 0)]
    assert sum((p.locate(P) for P in pats), []) == [4, 1, 7, 10, 7, 4, 1, 10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2, 0]
    assert sum((p.locate(P, 2) for P in pats), []) == [4, 1, 7, 10, 7, 10, 7, 0]
    strings = F.NAMED["miss3"]
    t, off, SA, LCP = M.arrays_by_definition(strings)
    p = F.Pipeline(strings, SA, 3)
    pats = [b"miss", b"ss", b"ssi", b"ouri", b"im", b"ssm", b"missouri"]
    assert [p.search(P) for P in pats] == [(7, 10), (18, 22), (19, 21), (10, 11), (0, 0), (0, 0), (9, 10)]
    pos = sum((p.locate(P) for P in pats), [])
    assert pos == [19, 0, 11, 21, 5, 2, 13, 5, 2, 15, 11]
    assert (np.searchsorted(off, pos, side="right") - 1).tolist() == [2, 0, 1, 2, 0, 0, 1, 0, 0, 1, 1]


def test_the_wrappers_and_exports_are_there():
    import ctypes as C
    import psac_amd
    from psac_amd import _lib
    for name in ("fm_index_device", "fm_count_device", "fm_occurrences_device", "fm_search", "fm_index", "FMIndex"):
        assert callable(getattr(psac_amd, name)), name
    assert callable(psac_amd.SuffixArray.fm_index)
    for name in ("count", "locate", "nbytes", "free"):
        assert hasattr(psac_amd.FMIndex, name), name
    assert C.sizeof(_lib.FmInfo) == 4 * 8 + 2 * 4 + 512
    lib = _lib.load()
    for suf in ("u32", "u64"):
        for name, args in (("psacx_fm_index_dev_", 8), ("psacx_fm_count_dev_", 8), ("psacx_fm_occurrences_dev_", 14), ("psacx_fm_search_", 18)):
            assert name + suf in _lib.EXPORTS and len(getattr(lib, name + suf).argtypes) == args, name + suf


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe, lib = str(tmp_path / "test_fm"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fm.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "fm header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_fmindex_refuses_bad_flags_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "fmindex")
    (tmp_path / "set").write_bytes(b"mississippi\nmissouri\nmiss\n")
    (tmp_path / "pats").write_bytes(b"miss\n")
    text, pats = str(tmp_path / "set"), str(tmp_path / "pats")
    for args in ([exe], [exe, "-f", text], [exe, "-f", text, "-q", pats, "-s", "x"], [exe, "-f", text, "-q", pats, "--index", "16"],
                 [exe, "-f", text, "-q", pats, "--bogus"], [exe, "-f", text, "-q", pats, "-s", "0", "--occ"], [exe, "-f", text, "-q", pats, "-s"]):
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "USAGE" in r.stderr, args
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-f", text, "-q", pats, "--set", "--occ"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
