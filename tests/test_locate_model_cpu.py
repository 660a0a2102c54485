"""The host model of the pattern search (tests/locate_model.py) against itself and against the reference's expectations: the
interval counted from the definition equals the interval by bisection over the oracle's suffix array, the table from the
definition has the properties include/psacx.h states, and the table rule gives the interval of the search without a table.
Also what can be checked of the new entry points without a GPU: they exist, are wrapped, and fail loudly."""
import json
import os
import subprocess

import numpy as np
import pytest

import locate_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "locate_mississippi.json")) as f:
        return json.load(f)


def test_reference_expectations_on_mississippi():
    g = golden()
    assert len(g["found"]) == 16 and len(g["not_found"]) == 5
    SA = M.sa_of("mississippi")
    assert SA.tolist() == [10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2]
    for e in g["found"]:
        P = e["pattern"].encode()
        assert M.by_definition(e["text"].encode(), P) == (e["lb"], e["ub"]), e
        assert M.by_bisection(e["text"].encode(), SA, P) == (e["lb"], e["ub"]), e
    for e in g["not_found"]:
        P = e["pattern"].encode()
        lb, ub = M.by_definition(e["text"].encode(), P)
        assert lb == ub and M.by_bisection(e["text"].encode(), SA, P) == (lb, ub), e
    # this project pins the insertion point
    assert M.by_definition(b"mississippi", b"misx") == (5, 5) and M.by_definition(b"mississippi", b"ississippii") == (4, 4)
    assert M.by_definition(b"mississippi", b"") == (0, 11)


@pytest.mark.parametrize("name", M.SMALL)
def test_definition_equals_bisection(name):
    text = M.text_of(name)
    pats, lb, ub = M.expected(name)
    n = int(text.size)
    # counting over all suffixes is quadratic: every pattern on the short texts, a spread of them on the longer ones
    step = 1 if n <= 100 else (7 if n <= 5000 else 61)
    seen = 0
    for i in range(0, len(pats), step):
        if len(pats[i]) > 5000 and n > 5000:
            continue
        assert M.by_definition(text, pats[i]) == (lb[i], ub[i]), (name, i, pats[i][:40])
        seen += 1
    assert seen >= 3
    assert np.all(lb <= ub) and np.all(ub <= n)
    # the catalogue reaches what it is meant to reach
    lens = set(len(P) for P in pats)
    assert set(M.LENGTHS) | {n, n + 1} <= lens
    assert (ub > lb).any() and (ub == lb).any() and (lb == 0).any() and (lb == n).any()


def test_unary_intervals():
    text = M.text_of("unary")
    n = int(text.size)
    SA = M.sa_of("unary")
    for m in (1, 2, 64, n - 1, n):
        assert M.by_bisection(text, SA, b"a" * m) == (m - 1, n)             # the m - 1 shorter suffixes are smaller
    assert M.by_bisection(text, SA, b"a" * (n + 1)) == (n, n)


@pytest.mark.parametrize("name", ["mississippi", "tiny1", "tiny9", "edge65", "unary", "bytes256", "tandem"])
def test_table_from_the_definition(name):
    text = M.text_of(name)
    n, SA = int(text.size), M.sa_of(name)
    code, sigma = M.codes_of(text)
    B = sigma + 1
    ks, refused = M.table_ks(text)
    assert B ** ks[2] > (1 << 16) and M.key_space(B, ks[2]) is not None and M.key_space(B, refused) is None and M.key_space(B, refused - 1) is not None
    for k in ks[:2] + ([ks[2]] if n <= 5000 else []):
        table = M.table_by_definition(text, k)
        assert table.size == B ** k + 1 and table[0] == 0 and table[-1] == n and np.all(np.diff(table) >= 0)
        # bucket v is SA[table[v] : table[v+1]]: the suffixes whose first k characters (code 0 past the end) spell v
        s = text.tobytes()
        for v in np.nonzero(np.diff(table))[0][:50]:
            for r in (int(table[v]), int(table[v + 1]) - 1):
                p, key = int(SA[r]), 0
                for j in range(k):
                    key = key * B + (int(code[s[p + j]]) if p + j < n else 0)
                assert key == v
        # a suffix shorter than k has a bucket whose key ends in zeros: the one-character suffix
        if k > 1:
            key = 0
            for j in range(k):
                key = key * B + (int(code[s[n - 1 + j]]) if n - 1 + j < n else 0)
            assert table[key + 1] - table[key] >= 1 and key % B == 0


@pytest.mark.parametrize("name", ["mississippi", "tiny3", "tiny17", "edge64", "edge4097", "unary", "bytes256", "tandem"])
def test_table_rule_gives_the_interval_without_a_table(name):
    text = M.text_of(name)
    SA = M.sa_of(name)
    code, sigma = M.codes_of(text)
    pats, lb, ub = M.expected(name)
    ks = M.table_ks(text)[0]
    for k in ks[:2] + ([ks[2]] if text.size <= 5000 else []):
        table = M.table_by_definition(text, k)
        for i, P in enumerate(pats):
            if len(P) > 5000:
                continue
            assert M.with_table(text, SA, table, code, k, P) == (lb[i], ub[i]), (name, k, i, P[:40])


def test_entry_points_exist_and_fail_loudly_without_a_gpu():
    import psac_amd
    from psac_amd import _lib
    lib = _lib.load()
    for nm in ("psacx_lookup_table_dev_", "psacx_locate_dev_", "psacx_locate_"):
        for suf in ("u32", "u64"):
            assert hasattr(lib, nm + suf) and nm + suf in _lib.EXPORTS
    for nm in ("lookup_table_device", "locate_device", "locate"):
        assert callable(getattr(psac_amd, nm)) and nm in psac_amd.__all__
    pat, off = psac_amd.pattern_buffer([b"ab", "", np.array([1, 2, 3], np.uint8)])
    assert pat.tolist() == [97, 98, 1, 2, 3] and off.tolist() == [0, 2, 2, 5] and off.dtype == np.uint64
    assert _lib.OPTIONS["locate_shape"] == 18 and _lib.OPTIONS["locate_count"] == 19
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.locate(b"mississippi", M.sa_of("mississippi"), [b"ssi"])
        assert e.value.code == -6                            # PSACX_ENOGPU: no CPU fallback


def build_cpp_program(tmp_path):
    """tests/cpp/test_locate.cpp (locate of include/suffix_array.hpp) built warning-free as C++11 against the library."""
    exe, lib = str(tmp_path / "test_locate"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_locate.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "locate header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_cli_is_built_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "locate")
    assert os.path.exists(exe)
    assert subprocess.run([exe], capture_output=True, text=True).returncode != 0            # -f and -q are required
    (tmp_path / "t.txt").write_bytes(b"mississippi")
    (tmp_path / "q.txt").write_bytes(b"ssi\n")
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-f", str(tmp_path / "t.txt"), "-q", str(tmp_path / "q.txt")], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
