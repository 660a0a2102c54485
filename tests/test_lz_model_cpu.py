"""The two statements of LPF / SRC (tests/lz_model.py) agree -- all pairs by byte comparison, straight from "the longest factor
at i that also starts before i", and the rank walk of include/psacx.h over the oracle's SA and LCP -- and the parse cut from
them is the recorded one:

  - both arrays are equal on the named texts and on n = 1, "aa", "ab";
  - the parse decodes to the text (the decoder reads the text at literals only) and the checker's count of it is 0;
  - tests/golden/lz77_named.json holds start and src of every named text, as the model wrote them;
  - the figures of the named texts: mississippi 8 phrases, stated one by one; 300 times 'a' 2, the second 299 bytes from 0; the
    Fibonacci word of 377 letters 13 (the Fibonacci numbers 3 .. 144 between three single letters and a rest of 2), longest previous factor 231; ("ab" x 50) c ("ab" x 50)
    5, longest 100; 4096 random DNA (inputs.dna(4096, 77)) 810; 3000 characters of a period-97 tandem repeat 38, longest
    previous factor n - 97;
  - the checker's count of the wrong parses of tests/test_gpu_lz77_verifier.py, stated here by hand for mississippi."""
import numpy as np
import pytest

import lz_model as M

Z = {"mississippi": 8, "a300": 2, "fib377": 13, "abcab": 5, "dna4096": 810, "tandem3000": 38}
LONGEST = {"mississippi": 4, "a300": 299, "fib377": 231, "abcab": 100, "dna4096": 11, "tandem3000": 3000 - 97}


@pytest.mark.parametrize("name", M.TINY + M.NAMED)
def test_bytes_and_ranks_agree(name):
    t = M.text_of(name)
    a, b = M.by_bytes(t), M.lpf_of(name)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    n = int(t.size)
    i = np.arange(n)
    lit = a[0] == 0
    assert np.all(a[1][lit] == M.ONES) and np.all(a[1][~lit] < i[~lit]) and np.all(a[1][~lit] >= 0) and np.all(a[0] <= n - i)
    for k in np.nonzero(~lit)[0][:200]:                # the factor is in the text where SRC says
        l, s = int(a[0][k]), int(a[1][k])
        assert t[s:s + l].tobytes() == t[k:k + l].tobytes()
        assert k + l == n or t[s + l] != t[k + l]


@pytest.mark.parametrize("name", M.TINY + M.NAMED + ["dna65536"])
def test_the_parse_decodes_and_checks(name):
    t = M.text_of(name)
    start, src = M.parse_of(name)
    assert start[0] == 0 and start[-1] == t.size and np.all(np.diff(start) > 0)
    assert M.decode(start, src, t) == t.tobytes()
    blind = np.where(src == M.ONES, t[start[:-1]], 0).astype(np.uint8)      # only the literals of the text
    literals = np.zeros(t.size, np.uint8)
    literals[start[:-1]] = blind
    assert M.decode(start, src, literals) == t.tobytes()
    assert M.check_count(t, start, src) == 0


@pytest.mark.parametrize("name", M.NAMED)
def test_golden_and_figures(name):
    start, src = M.parse_of(name)
    g = M.golden()[name]
    assert g["start"] == start.tolist() and g["src"] == src.tolist()
    assert len(src) == Z[name]
    assert int(M.lpf_of(name)[0].max()) == LONGEST[name]


def test_the_phrases_stated_by_hand():
    start, src = M.parse_of("mississippi")
    assert list(zip(start[:-1].tolist(), np.diff(start).tolist(), src.tolist())) == [
        (0, 1, -1), (1, 1, -1), (2, 1, -1), (3, 1, 2), (4, 4, 1), (8, 1, -1), (9, 1, 8), (10, 1, 7)]
    assert M.cli_text(start, src) == "0 1 -\n1 1 -\n2 1 -\n3 1 2\n4 4 1\n8 1 -\n9 1 8\n10 1 7\n"
    start, src = M.parse_of("a300")
    assert start.tolist() == [0, 1, 300] and src.tolist() == [-1, 0]           # the copy overlaps its phrase
    start, src = M.parse_of("fib377")
    assert np.diff(start).tolist() == [1, 1, 1, 3, 5, 8, 13, 21, 34, 55, 89, 144, 2]
    start, src = M.parse_of("abcab")
    assert start.tolist() == [0, 1, 2, 100, 101, 201] and src.tolist() == [-1, -1, 0, -1, 0]
    start, src = M.parse_of("tandem3000")
    assert start[-2:].tolist() == [99, 3000] and int(src[-1]) == 99 - 97      # the rest of the text is one phrase, a period back


def test_the_parse_is_greedy():
    # every phrase is as long as the longest previous factor at its start allows, by the byte statement
    for name in M.NAMED:
        lpf = M.by_bytes(M.text_of(name))[0]
        start, src = M.parse_of(name)
        assert np.array_equal(np.diff(start), np.maximum(1, lpf[start[:-1]]))


def test_the_chain_of_values_no_text_has():
    for kind in M.SYNTHETIC:
        for n in (1, 255, 256, 257, 5000):
            v = M.synthetic(kind, n, 64)
            s = M.chain(v)
            assert s[0] == 0 and s[-1] == n and np.all(np.diff(s) > 0)
    assert M.chain(M.synthetic("zeros", 300, 64)).size == 301
    assert M.chain(M.synthetic("ones", 300, 64)).tolist() == [0, 300] and M.chain(M.synthetic("n", 300, 64)).tolist() == [0, 300]
    assert np.all(M.chain(M.synthetic("tile_ends", 5000, 64))[1:-1] % 64 == 0)
    assert np.all(np.diff(M.chain(M.synthetic("skip", 5000, 64)))[:-1] == 65)
    assert int(np.diff(M.chain(M.synthetic("half", 5000, 64))).max()) == 2500


def test_the_count_of_wrong_parses():
    t = M.text_of("mississippi")
    start, src = M.parse_of("mississippi")
    assert M.check_count(t, start, src) == 0
    for name, (s, p), want in wrong_parses(t, start, src):
        assert M.check_count(t, s, p) == want, name


def wrong_parses(t, start, src):
    """(name, (start, src), errors) for mississippi: what tests/test_gpu_lz77_verifier.py feeds the device checker"""
    n = int(t.size)
    out = []
    s, p = start.copy(), src.copy()
    p[4] = 0                                           # issi from 0: m != i, i != s, s == s, s != i
    out.append(("source one off", (s, p), 3))
    s, p = start.copy(), src.copy()
    p[3] = 3                                           # a source at its own start
    out.append(("source >= start", (s, p), 1))
    s, p = np.delete(start, 1), np.delete(src, 1)      # m and i as one literal: the phrase, not its bytes
    out.append(("literal of length 2", (s, p), 1))
    s, p = start.copy(), src.copy()
    s[2], s[3] = s[3], s[2]                            # 0 1 3 2 4: phrase 1 = [1, 3) is a literal of two bytes, phrase 2 = [3, 2) descends,
    out.append(("starts out of order", (s, p), 3))     # phrase 3 = [2, 4) has its source at its start; positions 2 and 3 find phrases 1 and 3
    s, p = start.copy(), src.copy()
    s[0] = 1
    out.append(("start[0] != 0", (s, p), 3))           # start[0], phrase 0 is empty, position 0 is in no phrase
    s, p = start.copy(), src.copy()
    s[-1] = n - 1
    out.append(("start[z] != n", (s, p), 3))           # start[z], phrase z - 1 is empty, position n - 1 is in no phrase
    s, p = start.copy(), src.copy()
    s[5] = 9                                           # issi from 1 one byte longer: p != s at position 8, and the phrase [9, 9) behind it is empty
    out.append(("one byte too long", (s, p), 2))
    return out
