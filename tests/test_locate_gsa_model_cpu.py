"""The host model of the pattern search over string sets (tests/locate_gsa_model.py) against itself: the interval counted from
the definition equals the interval by bisection over the oracle's generalized suffix array and the occurrence set, the table from
key_k has the properties include/psacx.h states, the table rule gives the interval of the search without a table, and with one
string everything equals the plain model.  Also what can be checked of the new entry points without a GPU: they exist, are
wrapped, the C++ mirror compiles, and all of them fail loudly."""
import json
import os
import subprocess

import numpy as np
import pytest

import locate_gsa_model as M
import locate_model as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sampled(name, pats):
    """Counting over all suffixes is quadratic: every pattern on the short sets, a spread of them on the longer ones."""
    n = int(M.arrays(name)[0].size)
    return range(0, len(pats), 1 if n <= 300 else (5 if n <= 5000 else (41 if n <= 70000 else 97)))


@pytest.mark.parametrize("name", M.ALL)
def test_definition_bisection_and_occurrence_set_agree(name):
    text, off, SA = M.arrays(name)
    n = int(text.size)
    pats, lb, ub = M.expected(name)
    assert np.all(lb <= ub) and np.all(ub <= n)
    seen = 0
    for i in sampled(name, pats):
        assert M.by_definition(text, off, pats[i]) == (lb[i], ub[i]), (name, i, pats[i][:40])
        assert sorted(int(x) for x in SA[lb[i]:ub[i]]) == M.occurrence_set(text, off, pats[i]), (name, i)
        seen += 1
    assert seen >= 3
    lens = set(len(P) for P in pats)
    assert set(m for m in M.LENGTHS if m <= n) <= lens
    assert (ub > lb).any() and (lb == 0).any()
    if len(off) > 2:
        # a string plus the start of the next one is a piece of the text, but no occurrence in the set unless it occurs elsewhere
        s = text.tobytes()
        o = [int(x) for x in off]
        P = s[o[0]:o[1] + min(2, o[2] - o[1])]
        a, b = M.by_bisection(s, off, SA, P)
        assert o[0] not in [int(x) for x in SA[a:b]] and L.by_definition(s, P)[1] - L.by_definition(s, P)[0] >= 1


def test_word_edges_reaches_the_ends_of_the_bitmap_words():
    text, off, SA = M.arrays("word_edges")
    assert [int(x) for x in off][1:7] == list(M.WORD_EDGES)
    bits = M.ends_bitmap(off, int(text.size))
    assert bits.size == (text.size >> 5) + 1 and bits[0] == 1 | (1 << 31) and bits[1] == 1 | 2 | (1 << 31) and bits[2] == 1 | 2 | (1 << (90 - 64))
    pats = M.patterns_of("word_edges")
    s = text.tobytes()
    for e in M.WORD_EDGES:
        assert s[e - 1:e] in pats and s[e - 1:e + 1] in pats


@pytest.mark.parametrize("name", ["tiny9", "tiny17", "edge65", "word_edges", "prefixes", "unary", "copies", "bytes256", M.READS_SMALL])
def test_table_from_the_definition_and_its_rule(name):
    text, off, SA = M.arrays(name)
    n = int(text.size)
    code, sigma = M.codes_of(text)
    B = sigma + 1
    pats, lb, ub = M.expected(name)
    end = M.ends_of(off, n)
    s = text.tobytes()
    ks = M.table_ks(text)[0]
    for k in ks[:2] + ([ks[2]] if n <= 5000 else []):
        table = M.table_by_definition(text, off, k)
        assert table.size == B ** k + 1 and table[0] == 0 and table[-1] == n and np.all(np.diff(table) >= 0)
        keys = M.keys_by_definition(text, off, k)[0]
        assert np.all(np.diff(keys[SA.astype(np.int64)]) >= 0)                      # bucket v is SA[table[v] : table[v+1]]
        for i, P in enumerate(pats):
            assert M.with_table(s, off, SA, table, code, k, P, end=end) == (lb[i], ub[i]), (name, k, i, P[:40])
    if len(off) > 2 and ks[1] == 2:
        # the last character of a string has a key that ends in zeros whatever follows it in the text
        keys = M.keys_by_definition(text, off, 2)[0]
        assert all(int(keys[int(e) - 1]) % B == 0 for e in off[1:])


@pytest.mark.parametrize("name", L.SMALL)
def test_one_string_equals_the_plain_model(name):
    text, SA = L.text_of(name), L.sa_of(name)
    off = np.array([0, text.size], np.uint64)
    pats, lb, ub = L.expected(name)
    s = text.tobytes()
    end = M.ends_of(off, int(text.size))
    for i, P in enumerate(pats):
        assert M.by_bisection(s, off, SA, P, end=end) == (lb[i], ub[i]), (name, i)
    for k in (1, 2):
        assert np.array_equal(M.table_by_definition(text, off, k), L.table_by_definition(text, k))
    for P in pats[::max(1, len(pats) // 8)]:
        if text.size <= 5000 and len(P) <= 5000:
            assert M.by_definition(text, off, P) == L.by_definition(text, P)


def test_mississippi_in_two_strings():
    with open(os.path.join(ROOT, "tests", "golden", "locate_gsa_mississippi.json")) as f:
        g = json.load(f)
    assert g["strings"] == ["missis", "sippi"] and len(g["patterns"]) >= 20
    import oracle_lib as O
    ref = O.construct_ss([np.frombuffer(x.encode(), np.uint8) for x in g["strings"]], bits=64)
    text, off, SA = ref["text"], np.asarray(ref["off"], np.uint64), ref["SA"]
    assert SA.tolist() == g["SA"] == [10, 7, 4, 1, 0, 9, 8, 5, 6, 3, 2] and off.tolist() == [0, 6, 11]
    differs = 0
    for e in g["patterns"]:
        P = e["pattern"].encode()
        assert M.by_definition(text, off, P) == (e["lb"], e["ub"]), e
        assert M.by_bisection(text, off, SA, P) == (e["lb"], e["ub"]), e
        assert [int(x) for x in SA[e["lb"]:e["ub"]]] == e["occurrences"]
        differs += L.by_definition(text, P) != (e["lb"], e["ub"])
    assert differs >= 5                                       # "ssis", "sis", "issi" ...: the seam matters
    by = {e["pattern"]: (e["lb"], e["ub"]) for e in g["patterns"]}
    assert by["ssi"] == (10, 11) and by["sissi"] == (10, 10) and by["s"] == (7, 11) and by[""] == (0, 11)


def test_occurrence_lists_by_the_plain_loop():
    text, off, SA = M.arrays("tiny17")
    n = int(text.size)
    lb = [0, 3, 5, n, 9, 2]
    ub = [n, 3, 4, n, n + 1, 6]
    start, pos, sid = M.occurrences(SA, n, lb, ub, 0, off)
    assert start.tolist() == [0, n, n, n, n, n, n + 4] and pos.tolist() == SA.tolist() + SA[2:6].tolist()
    assert np.array_equal(sid, M.string_ids(off, pos, n)) and all(int(off[s]) <= p < int(off[s + 1]) for s, p in zip(sid.tolist(), pos.tolist()))
    start, pos, sid = M.occurrences(SA, n, lb, ub, 3)
    assert start.tolist() == [0, 3, 3, 3, 3, 3, 6] and sid is None and pos.tolist() == SA[:3].tolist() + SA[2:5].tolist()
    beyond = SA.copy()
    beyond[1] = n + 5
    assert M.occurrences(beyond, n, [0], [3], 0, off)[2].tolist()[1] == len(off) - 1
    assert M.cli_text([1, 4], [3, 4], M.occurrences(SA, n, [1, 4], [3, 4], 0, off), off).count(":") == 2


def test_entry_points_exist_and_fail_loudly_without_a_gpu():
    import psac_amd
    from psac_amd import _lib
    lib = _lib.load()
    names = ["psacx_string_ends_dev"] + [nm + suf for nm in ("psacx_lookup_table_gsa_dev_", "psacx_locate_gsa_dev_", "psacx_locate_gsa_", "psacx_occurrences_dev_")
                                         for suf in ("u32", "u64")]
    for nm in names:
        assert hasattr(lib, nm) and nm in _lib.EXPORTS
    for nm in ("string_ends_device", "lookup_table_gsa_device", "locate_gsa_device", "occurrences_device", "occurrences", "locate"):
        assert callable(getattr(psac_amd, nm)) and nm in psac_amd.__all__
    import torch
    if not torch.cuda.is_available():
        text, off, SA = M.arrays("tiny9")
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.locate(text, SA, [b"AC"], offsets=off)
        assert e.value.code == -6                            # PSACX_ENOGPU: no CPU fallback
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.occurrences(SA, [0], [1])
        assert e.value.code == -6


def build_cpp_program(tmp_path):
    """tests/cpp/test_locate_gsa.cpp (locate over a string set and occurrences of include/suffix_array.hpp) built warning-free as
    C++11 against the library."""
    exe, lib = str(tmp_path / "test_locate_gsa"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_locate_gsa.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_as_cxx11_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "locate_gsa header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_cli_takes_the_new_flags_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "locate")
    (tmp_path / "t.txt").write_bytes(b"missis\nsippi\n")
    (tmp_path / "q.txt").write_bytes(b"ssi\n")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--set" in r.stderr and "--occ" in r.stderr
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe, "-f", str(tmp_path / "t.txt"), "-q", str(tmp_path / "q.txt"), "--set", "--occ", "3"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
