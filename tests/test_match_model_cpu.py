"""The host model of the longest-match search (tests/match_model.py) against itself: the answer from the definition equals the
answer by bisection over the oracle's suffix array, on the catalogue and on random tiny texts and sets; values checked by hand;
the table rule; the expansion of the suffix mode.  Also what can be checked of the new entry points without a GPU: they exist,
are wrapped, and fail loudly."""
import os
import subprocess

import numpy as np
import pytest

import locate_model as L
import locate_gsa_model as G
import match_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHORT = [name for name in L.ALL if L.text_of(name).size <= 100]              # mississippi, tiny1..17, edge63..65
UP_TO_5000 = [name for name in L.ALL if L.text_of(name).size <= 5000]


def kinds(ln, pats):
    m = np.array([len(P) for P in pats])
    # len == 0 (the empty pattern among them), 0 < len < m, and len == m > 0
    return int((ln == 0).sum()), int(((ln > 0) & (ln < m)).sum()), int(((ln == m) & (m > 0)).sum())


@pytest.mark.parametrize("name", UP_TO_5000)
def test_definition_equals_bisection(name):
    text = L.text_of(name)
    n = int(text.size)
    pats, ln, lb, ub = M.expected(name)
    # the definition is quadratic: every pattern on the short texts, a spread of them on the longer ones
    step = 1 if n <= 100 else 5
    for i in range(0, len(pats), step):
        assert M.by_definition(text, pats[i]) == (ln[i], lb[i], ub[i]), (name, i, pats[i][:40])
    assert np.all(ln <= [len(P) for P in pats]) and np.all(lb < ub) and np.all(ub <= n)          # never empty on a correct SA
    # where the pattern occurs the interval is locate's
    _, llb, lub = L.expected(name)
    full = ln == [len(P) for P in pats]
    assert np.array_equal(lb[full], llb[full]) and np.array_equal(ub[full], lub[full]) and np.all(llb[~full] == lub[~full])


@pytest.mark.parametrize("name", L.ALL)
def test_every_text_has_queries_of_all_three_kinds(name):
    pats, ln, lb, ub = M.expected(name)
    none, part, whole = kinds(ln, pats)
    assert none > 0 and part > 0 and whole > 0, (name, none, part, whole)
    if name == "dna":
        assert (none, part, whole) == (88, 345, 61)
    if name == "unary":
        assert (none, part, whole) == (88, 277, 84)


def test_values_checked_by_hand_on_mississippi():
    SA = L.sa_of("mississippi")
    assert SA.tolist() == [10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2]
    # i ippi issippi ississippi mississippi pi ppi sippi sissippi ssippi ssissippi
    hand = {b"misx": (3, 4, 5), b"issix": (4, 2, 4), b"piss": (2, 5, 6), b"x": (0, 0, 11), b"": (0, 0, 11), b"ssi": (3, 9, 11),
            b"issississi": (7, 3, 4),          # "ississi" occurs once, at 1: m-ississi-ppi
            b"mississippi": (11, 4, 5), b"mississippii": (11, 4, 5), b"a": (0, 0, 11), b"ia": (1, 0, 4)}
    for Q, want in hand.items():
        assert M.by_definition(b"mississippi", Q) == want, Q
        assert M.by_bisection(b"mississippi", SA, Q) == want, Q


def test_a_query_that_only_matches_across_the_seam():
    # the two-string split of test_locate_gsa_model_cpu.py: "missis" + "sippi"
    text, off = b"mississippi", [0, 6, 11]
    SA = [10, 7, 4, 1, 0, 9, 8, 5, 6, 3, 2]                 # i ippi is issis missis pi ppi s sippi sis ssis
    assert M.by_definition(text, b"ssip") == (4, 9, 10)
    assert M.by_definition(text, b"ssip", off) == (3, 10, 11) == M.by_bisection(text, SA, b"ssip", off)
    assert M.by_definition(text, b"mississippi", off) == (6, 4, 5) == M.by_bisection(text, SA, b"mississippi", off)
    assert M.by_definition(text, b"sissi", off) == (3, 9, 10) == M.by_bisection(text, SA, b"sissi", off)
    assert M.by_definition(text, b"issip", off) == (4, 3, 4) == M.by_bisection(text, SA, b"issip", off)


SETS_UP_TO_5000 = [name for name in G.GST if G.arrays(name)[0].size <= 5000]


@pytest.mark.parametrize("name", SETS_UP_TO_5000)
def test_definition_equals_bisection_on_sets(name):
    text, off, SA = G.arrays(name)
    n = int(text.size)
    pats, ln, lb, ub = M.expected_gsa(name)
    step = 1 if n <= 100 else 5
    for i in range(0, len(pats), step):
        assert M.by_definition(text, pats[i], off) == (ln[i], lb[i], ub[i]), (name, i, pats[i][:40])
    assert np.all(lb < ub) and np.all(ub <= n)
    longest = int(np.max(np.diff(off.astype(np.int64))))
    assert np.all(ln <= longest)                            # a match never crosses a string end
    _, llb, lub = G.expected(name)
    full = ln == [len(P) for P in pats]
    assert np.array_equal(lb[full], llb[full]) and np.array_equal(ub[full], lub[full])


def test_random_tiny_texts_and_sets():
    rng = np.random.RandomState(77)
    import oracle_lib as O
    for it in range(300):
        sigma = int(rng.randint(1, 4))
        n = int(rng.randint(1, 25))
        text = (97 + rng.randint(0, sigma, n)).astype(np.uint8)
        s = text.tobytes()
        queries = [(97 + rng.randint(0, sigma + 1, int(rng.randint(0, 9)))).astype(np.uint8).tobytes() for _ in range(6)] + [s, s[n // 2:] + b"a"]
        if it % 2 == 0:
            SA = O.construct(text, bits=64, lcp=False)["SA"]
            for Q in queries:
                assert M.by_definition(s, Q) == M.by_bisection(s, SA, Q), (s, Q)
        else:
            cuts = sorted(set([0, n] + [int(x) for x in rng.randint(1, n + 1, int(rng.randint(0, 4)))]))
            strings = [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
            ref = O.construct_ss(strings, bits=64)
            assert [int(x) for x in ref["off"]] == cuts
            for Q in queries:
                assert M.by_definition(s, Q, cuts) == M.by_bisection(s, ref["SA"], Q, cuts), (s, cuts, Q)


@pytest.mark.parametrize("name", ["mississippi", "tiny3", "tiny17", "edge64", "edge4097", "unary", "bytes256", "tandem"])
def test_table_rule_gives_the_answer_without_a_table(name):
    text, SA = L.text_of(name), L.sa_of(name)
    code, sigma = L.codes_of(text)
    ks = L.table_ks(text)[0]
    for max_len in (0, 2, 9):
        pats, ln, lb, ub = M.expected(name, max_len)
        queries = M.queries_of(pats, False, max_len)
        for k in ks[:2] + ([ks[2]] if text.size <= 5000 else []):
            table = L.table_by_definition(text, k)
            for i, Q in enumerate(queries):
                assert M.with_table(text, SA, table, code, k, Q) == (ln[i], lb[i], ub[i]), (name, k, max_len, i, Q[:40])


@pytest.mark.parametrize("name", [name for name in ("word_edges", "copies", "prefixes", "unary", "bytes256", "edge65") if name in SETS_UP_TO_5000])
def test_table_rule_on_sets(name):
    text, off, SA = G.arrays(name)
    code, sigma = L.codes_of(text)
    end = G.ends_of(off, int(text.size))
    pats, ln, lb, ub = M.expected_gsa(name)
    for k in L.table_ks(text)[0][:2]:
        table = G.table_by_definition(text, off, k)
        for i, Q in enumerate(pats):
            assert M.with_table(text, SA, table, code, k, Q, off=off, end=end) == (ln[i], lb[i], ub[i]), (name, k, i, Q[:40])


def test_suffix_mode_expansion():
    pats = [b"", b"abc", b"", b"", b"de", b""]
    assert M.queries_of(pats) == pats
    assert M.queries_of(pats, True) == [b"abc", b"bc", b"c", b"de", b"e"]
    assert M.queries_of(pats, True, 2) == [b"ab", b"bc", b"c", b"de", b"e"]
    assert M.queries_of(pats, False, 1) == [b"", b"a", b"", b"", b"d", b""]
    # the pieces of the suffix-mode tests: empty patterns at the front, in the middle and at the end, patterns ending at 64 and 256
    pieces = M.pieces_of(L.text_of("edge4097"))
    ends = np.cumsum([len(P) for P in pieces]).tolist()
    assert pieces[0] == b"" and pieces[-1] == b"" and any(P == b"" for P in pieces[1:-1]) and 64 in ends and 256 in ends
    assert set(len(P) for P in pieces) >= set(M.PIECE_LENGTHS)
    assert M.cli_text([3, 0], [4, 0], [5, 11]) == "3 4 5\n0 0 11\n"


def test_entry_points_exist_and_fail_loudly_without_a_gpu():
    import psac_amd
    from psac_amd import _lib
    lib = _lib.load()
    for nm in ("psacx_match_dev_", "psacx_match_gsa_dev_", "psacx_match_", "psacx_match_gsa_"):
        for suf in ("u32", "u64"):
            assert hasattr(lib, nm + suf) and nm + suf in _lib.EXPORTS
    for nm in ("match_device", "match_gsa_device", "match"):
        assert callable(getattr(psac_amd, nm)) and nm in psac_amd.__all__
    assert psac_amd.MATCH_SUFFIXES == 1
    import torch
    if not torch.cuda.is_available():
        for kw in ({}, {"suffixes": True, "max_len": 3}, {"offsets": [0, 6, 11]}):
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.match(b"mississippi", L.sa_of("mississippi"), [b"ssix"], **kw)
            assert e.value.code == -6                        # PSACX_ENOGPU: no CPU fallback


def build_cpp_program(tmp_path):
    """tests/cpp/test_match.cpp (match of include/suffix_array.hpp) built warning-free as C++11 against the library."""
    exe, lib = str(tmp_path / "test_match"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_match.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def test_cpp_mirror_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    exe = build_cpp_program(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "match header tests passed" not in r.stdout and "psacx" in (r.stdout + r.stderr)


def test_cli_accepts_longest_and_fails_loudly_without_a_gpu(tmp_path):
    exe = os.path.join(ROOT, "psac_amd", "bin", "locate")
    (tmp_path / "t.txt").write_bytes(b"mississippi")
    (tmp_path / "q.txt").write_bytes(b"ssix\n")
    base = [exe, "-f", str(tmp_path / "t.txt"), "-q", str(tmp_path / "q.txt")]
    # --suffixes and --max-len belong to --longest
    for extra in (["--suffixes"], ["--max-len", "3"]):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout == "" and "--longest" in r.stderr
    import torch
    if not torch.cuda.is_available():
        for extra in (["--longest"], ["--longest", "--suffixes", "--max-len", "3"], ["--longest", "--set", "--occ", "2"]):
            r = subprocess.run(base + extra, capture_output=True, text=True)
            assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr and "unknown argument" not in r.stderr
