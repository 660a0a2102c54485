"""psacx_mems_dev_* against the host model (tests/mems_model.py, whose two formulations tests/test_mems_model_cpu.py holds to each
other), both index widths, SA and LCP from the oracle; statistics, index and BWT from the library's own device calls:

  - one text at n = 1, 2, 3, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097 and 2^18 + 1 (the third index level) over random texts of 2 and
    4 letters, a^n, a Fibonacci word, a period-7 tandem repeat and all 256 byte values, with pieces cut from the text, the same with a
    byte substituted, random patterns, the whole text, an empty pattern, one byte and a byte absent from the text; at n <= 65 also
    against the byte definition (the whole text is a pattern there, for the random texts at n = 4097, and in a test of
    its own at 2^18 + 1).  What bounds a case is its number of candidates, about (slots) x (occurrences of the first min_len
    bytes): beyond n = 65 the random texts run with min_len 4 (10 at 2^18 + 1) and with max_occ 3 at min_len 1, the repetitive
    texts with short pieces at min_len 1, the whole text as a pattern with max_occ 2 (which ends nearly every walk at once), and a^(2^18+1)
    with the pattern aaa, one slot of which owns 2^18 candidates;
  - string sets: random ones, m = n, 3000 identical strings ACGT, patterns that span two strings; small sets against the bytes;
  - the edges of the expansion and the compaction, with the model's work asserted: a slot that owns exactly 1023, 1024 and 1025
    candidates; a slot with more than 2 * OCC_TILE candidates between slots with none; a tile of candidates filled by 1024 shells
    of one candidate each (every shell has a candidate, so no tile of 1024 candidates meets more than OCC_CHUNK = 1024 shells:
    the second chunk of a tile exists only for PSACX_MEMS_SUPER, where slots without ranks lie between the kept ones, and is
    tested there); a survivor on the last mark of a tile behind 1023 dead marks, on the first mark of a tile, and tiles
    without any (the first candidate of a batch always survives -- its slot starts a pattern, or the slot in front of it holds a
    longer match -- so "nothing before it" is meant inside the tile);
  - max_occ 1, 2 and large with the work counters; PSACX_MEMS_SUPER; the count query; PSACX_ERANGE at cap = z - 1; the NULL and flag
    rules; malformed poff; q == 0;
  - totality: LCP of noise and of all ones, an index of noise, bwt / first of noise, statistics of noise;
  - the host-pointer forms, psac_amd.mems, SuffixArray.mems, the C++ program and the command line on the named cases.
Outputs are pre-filled with a sentinel and have PAD entries of room behind the last one, which must come back untouched; the inputs
must come back unchanged."""
import os
import subprocess

import numpy as np
import pytest

import mems_gpu_common
import mems_model as X
import repeats_model as R
from mems_gpu_common import BIG, REPETITIVE, SENTINEL64, SIZES, TEXTS, MemsIndex, agree, check, patterns_of, statistics_agree, total
from repeats_gpu_common import Case, set_case, text_case
from rmq_gpu_common import Dev, PAD, SENTINEL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OCC_TILE = OCC_CHUNK = 1024


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def against_bytes(d, got, min_len, max_occ=0, flags=0):
    want = X.by_bytes(d.case.strings, d.pats, min_len, max_occ)
    if flags:
        want = X.supermaximal(want, d.pats)
    assert set(zip(*(a.tolist() for a in got))) == want and got[0].size == len(want)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", SIZES)
def test_mems_of_one_text_equal_the_model(ctx, n, bits):
    dev = Dev(ctx, bits)
    try:
        for kind in TEXTS:
            case = text_case(kind, n)
            small, rep = n <= 65, kind in REPETITIVE
            d = MemsIndex(dev, case, patterns_of(kind, case.text, whole=small or (not rep and n == 4097)))
            key = ("text", kind, n)
            if small:
                assert statistics_agree(d)
                for min_len, max_occ, flags in ((1, 0, 0), (2, 0, 0), (1, 1, 0), (2, 3, 0), (1, 0, X.SUPER), (2, 2, X.SUPER)):
                    got, _ = check(d, key, (kind, n, min_len, max_occ, flags), min_len, max_occ, flags)
                    against_bytes(d, got, min_len, max_occ, flags)
            elif rep:
                check(d, key, (kind, n), 1)
                check(d, key, (kind, n, "super"), 1, 0, X.SUPER)
                w = MemsIndex(dev, case, [case.text.tobytes()])
                check(w, key + ("whole",), (kind, n, "whole"), 1, 2)
                assert w.unchanged()
            else:
                check(d, key, (kind, n), 4)
                check(d, key, (kind, n, "occ"), 1, 3)
                check(d, key, (kind, n, "super"), 1, 0, X.SUPER)
            assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", TEXTS)
def test_mems_at_the_third_index_level(ctx, kind, bits):
    dev = Dev(ctx, bits)
    try:
        case = text_case(kind, BIG)
        key = ("text", kind, BIG)
        d = MemsIndex(dev, case, patterns_of(kind, case.text, whole=False))
        if kind in REPETITIVE:
            check(d, key, (kind, "occ"), 1, 8)
            if kind == "a":
                a = MemsIndex(dev, case, [b"aaa"])
                _, work = check(a, key + ("aaa",), (kind, "aaa"), 2)
                assert work == (3, 2 * BIG - 2)            # slot 0: BIG - 2 ranks and 1; slot 1: BIG - 1 and -- below min_len -- nothing more
        else:
            check(d, key, kind, 10 if kind != "bytes256" else 2)
            check(d, key, (kind, "super"), 6, 0, X.SUPER)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_the_whole_text_as_one_pattern_at_the_third_index_level(ctx, bits):
    """S = 2^18 + 1 slots of one pattern on random DNA: the search in poff with one long pattern, the scans over the slots in their
    second block and beyond and, with max_occ 1, one shell of one candidate per slot -- every suffix of the text but the last few is unique, its
    parent interval is not -- so candidate starts over nearly 2^18 shells and 257 tiles of 1024 shells each; only slot 0 is not
    extensible to the left.  PSACX_MEMS_SUPER keeps slot 0 alone.  (The model walks this in 3 s, max_occ 2 in 6 s, 400 000 shells;
    on a^n the interval of slot p holds p + 1 ranks, so max_occ ends all walks but three at once.)"""
    dev = Dev(ctx, bits)
    try:
        case = text_case("dna4", BIG)
        d = MemsIndex(dev, case, [case.text.tobytes()])
        got, work = check(d, ("whole", "dna4", BIG), "dna4 whole", 1, 1)
        assert BIG - 64 < work[0] == work[1] < BIG and [a.tolist() for a in got] == [[0], [0], [BIG]]      # (the last few suffixes occur elsewhere too)
        got, work = check(d, ("whole", "dna4", BIG), "dna4 whole super", 1, 0, X.SUPER)
        assert work == (1, 1) and [a.tolist() for a in got] == [[0], [0], [BIG]]
        assert d.unchanged()
    finally:
        dev.close()


def set_patterns(case):
    s, off = case.text.tobytes(), case.off
    pats = patterns_of("set", case.text, whole=False)
    for j in (1, len(off) // 2, len(off) - 2):              # patterns that span two strings of the set
        if 0 < j < len(off) - 1:
            pats.append(s[max(0, int(off[j]) - 3):int(off[j]) + 3])
    return pats + case.strings[:2] + [case.strings[-1] + case.strings[0]]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["random", "random2", "singles", "acgt3000"])
def test_mems_of_a_string_set_equal_the_model(ctx, name, bits):
    dev = Dev(ctx, bits)
    try:
        case = set_case(name)
        d = MemsIndex(dev, case, set_patterns(case))
        for min_len, max_occ, flags in ((1 if name != "random2" else 3, 0, 0), (2, 2, 0), (1, 0, X.SUPER), (1, 3000, 0)):
            got, work = check(d, ("set", name), (name, min_len, max_occ, flags), min_len, max_occ, flags)
            if name == "acgt3000" and (min_len, max_occ, flags) == (1, 0, 0):
                # a string end makes a match right-maximal: the pattern ACGT matches each of the 3000 strings whole
                p = d.pats.index(b"ACGT")
                assert int(np.sum((got[0] == int(d.poff[p])) & (got[2] == 4))) == 3000
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_small_sets_equal_the_byte_definition(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        for it, (n, m, sigma) in enumerate(((2, 2, 1), (9, 3, 2), (33, 5, 2), (64, 8, 3), (65, 2, 4), (40, 40, 2))):
            case = Case(R.random_set(n, m, 50 + it, sigma), False)
            d = MemsIndex(dev, case, set_patterns(case))
            assert statistics_agree(d)
            for min_len, max_occ, flags in ((1, 0, 0), (2, 1, 0), (3, 3, 0), (1, 0, X.SUPER), (2, 3, X.SUPER)):
                got, _ = check(d, ("small set", it), (n, m, sigma, min_len, max_occ, flags), min_len, max_occ, flags)
                against_bytes(d, got, min_len, max_occ, flags)
            assert d.unchanged()
        g = X.golden()
        for name in X.NAMED:                                # the named results, stated by hand in the CPU tests
            strings, pats = X.NAMED[name]
            d = MemsIndex(dev, Case(strings, True), pats)
            for min_len in (1, 2, 3):
                for flags, word in ((0, "mems"), (X.SUPER, "super")):
                    got, work = d.run(min_len, 0, flags)
                    want = g[name]["%s%d" % (word, min_len)]
                    assert [list(x) for x in zip(*(a.tolist() for a in got))] == want["triples"] and list(work) == want["work"], (name, word, min_len)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_edges_of_the_expansion_and_the_compaction(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        for n in (OCC_TILE - 1, OCC_TILE, OCC_TILE + 1):    # one slot, one shell, n candidates
            d = MemsIndex(dev, text_case("a", n), [b"a"])
            got, work = check(d, ("edge a", n), ("a", n), 1)
            assert work == (1, n) and got[0].size == n
        # a slot with more than two tiles of candidates between slots that own none
        d = MemsIndex(dev, text_case("a", 4097), [b"bb", b"aa", b"bb"])
        got, work = check(d, "edge aa", "bb aa bb", 1)
        assert work == (3, 2 * 4097) and 4097 > 2 * OCC_TILE + 1
        # slot 3 (the second a) owns 4097 candidates of which only the last one -- the rank of the whole text -- survives: the marks of
        # [4097 + 1, 2 * 4097 - 1) are dead, whole tiles of them, and the survivor is alone in the last tile
        assert got[0].tolist().count(3) == 1 and got[0].size == 4097 + 1
        # 1024 shells of one candidate each fill the first tile: text a^40, pattern a^100, min_len 20 -- each of the slots 0 .. 60 has the
        # whole text as its one match and 21 shells of one rank, 1281 in all, before the first shell with two
        d = MemsIndex(dev, text_case("a", 40), [b"a" * 100])
        got, work = check(d, "edge singles", "a^40 / a^100", 20)
        assert work[0] > 61 * 21 > OCC_CHUNK and got[0].tolist()[:21] == [0] * 21 and got[2].tolist()[:21] == list(range(40, 19, -1))
        # the survivor of slot 1 of aa on a^1024 is candidate 2047, the last mark of tile 1, behind 1023 dead marks
        d = MemsIndex(dev, text_case("a", 1024), [b"aa"])
        got, work = check(d, "edge last mark", "a^1024 / aa", 1)
        assert work == (3, 2048) and got[0].tolist() == [0] * 1024 + [1] and int(got[1][-1]) == 0
        # the survivors of aaa on a^1025 are candidates 0 .. 1024, 2048 -- the first mark of tile 2 -- and 3074
        d = MemsIndex(dev, text_case("a", 1025), [b"aaa"])
        got, work = check(d, "edge first mark", "a^1025 / aaa", 1)
        assert work == (6, 3 * 1025) and got[0].tolist() == [0] * 1025 + [1, 2] and got[1][-2:].tolist() == [0, 0]
        # PSACX_MEMS_SUPER: more than OCC_CHUNK slots inside one tile of ranks, every other one without ranks
        case = Case([b"A" + b"C" * 100], True)
        d = MemsIndex(dev, case, [b"A", b"G"] * 1500)
        got, work = check(d, "edge super chunk", "A G x 1500", 1, 0, X.SUPER)
        assert work == (1500, 1500) and got[0].tolist() == list(range(0, 3000, 2))
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_max_occ_bounds_the_work(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        for kind in ("dna2", "tandem7", "fib"):
            case = text_case(kind, 4097)
            d = MemsIndex(dev, case, patterns_of(kind, case.text, whole=False))
            free = check(d, ("text", kind, 4097, "free"), (kind, 0), 2)[1]
            for max_occ in (1, 2, 1 << 40):
                got, work = check(d, ("text", kind, 4097, "free"), (kind, max_occ), 2, max_occ)
                if max_occ < 3:
                    assert work[0] < free[0] and work[1] < free[1]          # (what the model says: check has compared both)
                else:
                    assert work == free
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_count_query_erange_null_and_flag_rules(ctx, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        case = text_case("dna2", 4097)
        d = MemsIndex(dev, case, patterns_of("dna2", case.text, whole=False))
        for flags in (0, X.SUPER):
            z = d.call(6, 0, flags, 0, lists=False)[3]
            assert z > 2
            with pytest.raises(psac_amd.PsacxError) as e:
                d.call(6, 0, flags, z, cap=z - 1)
            assert e.value.code == -2 and e.value.z == z
            assert np.all(d.raw[0] == SENTINEL64) and np.all(d.raw[1] == SENTINEL) and np.all(d.raw[2] == SENTINEL)
            assert d.call(0, 3, flags, 0, lists=False)[3] == d.call(1, 3, flags, 0, lists=False)[3] > 0      # min_len 0 and 1 mean the same
        with pytest.raises(psac_amd.PsacxError) as e:
            d.call(6, 0, 2, 10)
        assert e.value.code == -1
        with pytest.raises(psac_amd.PsacxError) as e:
            d.call(6, 0, 0xFFFFFFFE, 10)
        assert e.value.code == -1
        args = lambda q, t, ln: (ctx, d.n, d.d_sa, d.lcp.d_v, d.lcp.d_index, d.d_bwt, d.d_first, d.d_pat, d.d_poff, d.q, d.d_stats[0], d.d_stats[1],  # noqa: E731
                                 d.d_stats[2], 6, 0, 0, q, t, ln, 10, bits)
        room = dev.put(np.full(10 + PAD, SENTINEL64, np.uint64))
        for q, t, ln in ((None, room, room), (room, None, room), (room, room, None), (None, None, room), (room, None, None)):
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.mems_device(*args(q, t, ln))
            assert e.value.code == -1
        assert np.all(dev.get(room, 10 + PAD, np.uint64) == SENTINEL64)
        # q == 0 and n == 0
        work = []
        assert psac_amd.mems_device(ctx, d.n, d.d_sa, d.lcp.d_v, d.lcp.d_index, d.d_bwt, d.d_first, d.d_pat, d.d_poff, 0, None, None, None, 1, 0, 0,
                                    None, None, None, 0, bits, work=work) == 0 and work == [0, 0]
        assert psac_amd.mems_device(ctx, 0, None, None, None, None, None, d.d_pat, d.d_poff, d.q, None, None, None, 1, 0, 0, None, None, None, 0, bits) == 0
        # only empty patterns
        e0 = MemsIndex(dev, case, [b"", b""])
        assert e0.run(1)[0][0].size == 0
        # malformed offsets: found on the device, nothing written
        for bad in (np.concatenate(([1], d.poff[1:])), np.concatenate((d.poff[:3], [0], d.poff[4:]))):
            d_bad = dev.put(np.ascontiguousarray(bad, np.uint64))
            keep, d.d_poff = d.d_poff, d_bad
            try:
                for flags in (0, X.SUPER):
                    with pytest.raises(psac_amd.PsacxError) as e:
                        d.call(1, 0, flags, 50)
                    assert e.value.code == -1 and np.all(d.raw[0] == SENTINEL64) and np.all(d.raw[1] == SENTINEL)
            finally:
                d.d_poff = keep
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_the_timing_option_ends_the_call_after_a_stage(ctx, bits, monkeypatch):
    """PSACX_OPT_MEMS_STOP 1..3: z = 0, the work counters as ever, nothing written; 0 and PSACX_MEMS_SUPER: the whole call"""
    dev = Dev(ctx, bits)
    try:
        case = text_case("dna2", 4097)
        d = MemsIndex(dev, case, patterns_of("dna2", case.text, whole=False))
        want, work = d.run(4)
        for stop in (1, 2, 3):
            monkeypatch.setenv("PSACX_MEMS_STOP", str(stop))        # (the wrappers configure from the environment under the test suite)
            ctx.configure(mems_stop=stop)
            w = []
            qp, tp, ln, z = d.call(4, 0, 0, 8, work=w)
            assert z == 0 and tuple(w) == work and np.all(qp == SENTINEL64) and np.all(tp == SENTINEL) and np.all(ln == SENTINEL)
            got, swork = d.run(4, 0, X.SUPER)
            agree(got, mems_gpu_common.model(("stop", "super"), case, d.pats, d.stats, 4, 0, X.SUPER)[0], ("super", stop))
        monkeypatch.delenv("PSACX_MEMS_STOP")
        ctx.configure(mems_stop=0)
        agree(d.run(4)[0], want, "after the option")
        with pytest.raises(Exception):
            ctx.configure(mems_stop=4)
        assert d.unchanged()
    finally:
        ctx.configure(mems_stop=0)
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_totality_on_arrays_of_noise(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        n = 4097
        case = text_case("dna2", n)
        pats = patterns_of("dna2", case.text, whole=False)
        rng = np.random.RandomState(3)
        ones = int(np.iinfo(dev.dt).max)
        noise = lambda size, top: rng.randint(0, top, size).astype(np.uint64)  # noqa: E731
        S = sum(len(P) for P in pats)
        words = (n >> 5) + 1
        variants = {
            "lcp noise": dict(LCP=noise(n, 40)),
            "lcp wild": dict(LCP=np.where(rng.randint(0, 2, n) == 1, np.full(n, ones, np.uint64), noise(n, 1 << 31))),
            "lcp ones": dict(LCP=np.full(n, ones, np.uint64)),
            "index noise": dict(index=noise(n // 16 + 4096, 30)),
            "bwt noise": dict(bwt=(noise(n, 256).astype(np.uint8), rng.randint(0, 1 << 32, words).astype(np.uint32))),
            "stats noise": dict(stats=(noise(S, 2 * n), noise(S, n + 50), noise(S, n + 50))),
            "stats huge": dict(stats=(np.full(S, ones, np.uint64), np.zeros(S, np.uint64), np.full(S, 7, np.uint64))),
        }
        for what, v in sorted(variants.items()):
            d = MemsIndex(dev, case, pats, **v)
            for min_len, max_occ, flags in ((12, 0, 0), (1, 5, 0), (12, 0, X.SUPER), (1, 3, X.SUPER)):
                got, work = d.run(min_len, max_occ, flags)
                assert total(got, d), (what, min_len, max_occ, flags)
                assert work[1] >= got[0].size
            assert d.unchanged(), what
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_forms_and_wrappers_on_the_named_cases(ctx, bits):
    import psac_amd
    dt = np.uint32 if bits == 32 else np.uint64
    g = X.golden()
    for name in X.NAMED:
        strings, pats = X.NAMED[name]
        t, off, SA, LCP = R.arrays_by_definition(strings)
        for min_len in (1, 2, 3):
            for sup, word in ((False, "mems"), (True, "super")):
                want = g[name]["%s%d" % (word, min_len)]["triples"]
                for k in (0, 2):
                    got = psac_amd.mems(t, SA.astype(dt), LCP.astype(dt), pats, min_len, k=k, super=sup, ctx=ctx)
                    assert got[0].dtype == np.uint64 and got[1].dtype == dt and got[2].dtype == dt
                    assert [list(x) for x in zip(*(a.tolist() for a in got))] == want, (name, word, min_len, k)
        sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
        sa.construct(b"".join(strings))
        got = sa.mems(pats, 2)
        assert [list(x) for x in zip(*(a.tolist() for a in got))] == g[name]["mems2"]["triples"]
    # a set through the host form, offsets and all, and max_occ
    strings, pats = [b"abcab", b"cab"], [b"bcabc", b"", b"ca"]
    t, off, SA, LCP = R.arrays_by_definition(strings)
    got = psac_amd.mems(t, SA.astype(dt), LCP.astype(dt), pats, 2, offsets=off, ctx=ctx)
    assert list(zip(*(a.tolist() for a in got))) == [(0, 1, 4), (1, 5, 3), (2, 0, 3), (5, 2, 2), (5, 5, 2)]
    got = psac_amd.mems(t, SA.astype(dt), LCP.astype(dt), pats, 2, offsets=off, max_occ=1, ctx=ctx)
    assert set(zip(*(a.tolist() for a in got))) == X.by_bytes(strings, pats, 2, 1)
    sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
    sa.construct_ss(strings)
    got = sa.mems(pats, 2, super=True)
    assert list(zip(*(a.tolist() for a in got))) == [(0, 1, 4), (2, 0, 3), (5, 2, 2), (5, 5, 2)]
    assert psac_amd.mems(t, SA.astype(dt), LCP.astype(dt), [], 1, ctx=ctx)[0].size == 0
    with pytest.raises(ValueError):
        psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx).mems(pats, 1)


def test_cpp_program(tmp_path):
    from test_mems_build_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "mems header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64"])
def test_command_line(tmp_path, index):
    exe = os.path.join(ROOT, "psac_amd", "bin", "mems")
    g = X.golden()
    strings, pats = X.NAMED["mississippi"]
    (tmp_path / "text").write_bytes(strings[0])
    (tmp_path / "pats").write_bytes(b"\n".join(pats) + b"\n")
    base = [exe, "-f", str(tmp_path / "text"), "-q", str(tmp_path / "pats"), "--index", index]
    for min_len in (1, 3):
        for sup, word in (([], "mems"), (["--super"], "super")):
            want = [tuple(r) for r in g["mississippi"]["%s%d" % (word, min_len)]["triples"]]
            r = subprocess.run(base + ["-l", str(min_len), "--list"] + sup, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert r.stdout == "z: %d\n" % len(want) + X.cli_text(want, pats), (min_len, word)
    r = subprocess.run(base + ["-l", "1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: 24\n"
    r = subprocess.run(base + ["-l", "1", "--list", "2", "-k", "2", "--max-occ", "1"], capture_output=True, text=True)
    want = sorted(X.by_bytes(strings, pats, 1, 1))
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "z: %d" % len(want) and len(r.stdout.splitlines()) == 3
    # a set: one string per line
    strings, spats = [b"abcab", b"cab"], [b"bcabc", b"", b"ca"]
    (tmp_path / "set").write_bytes(b"\n".join(strings) + b"\n")
    (tmp_path / "spats").write_bytes(b"\n".join(spats))
    r = subprocess.run([exe, "-f", str(tmp_path / "set"), "--set", "-q", str(tmp_path / "spats"), "-l", "2", "--list", "--index", index],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: 5\n0 0 0 1 4\n0 1 1 0 3\n0 2 0 0 3\n2 0 0 2 2\n2 0 1 0 2\n", r.stdout + r.stderr
