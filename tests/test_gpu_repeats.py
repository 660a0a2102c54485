"""psacx_repeats_dev_* against the host model (tests/repeats_model.py, whose formulations tests/test_repeats_model_cpu.py holds to
each other), both index widths, SA and LCP from the oracle, BWT and `first` from psacx_bwt_dev_* (which tests/test_gpu_bwt.py holds
to the model):

  - the three kinds against the stack traversal of the LCP-intervals at n = 1, 2, 3, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097 and
    2^18 + 1 (the third level of the index), and against every substring with unique sentinels where n <= 65, over random texts of 2
    and 4 letters, a^n (n - 1 nested maximal repeats that all end at n, one supermaximal), a Fibonacci word, a period-7 tandem
    repeat, all 256 byte values and reads with a planted repeat;
  - string sets: random ones, m = n, 3000 identical strings "ACGT" (the whole-string interval is supermaximal with 3000 occurrences
    and no rank that does not start a string; the intervals of depth 1 to 3 fail the bound of 256 from the directory alone), 256
    strings x w for every byte x plus w itself (w is supermaximal with 257 occurrences) and its twin with one x doubled (it is not);
  - every filter alone and combined; the count query; PSACX_ERANGE at cap = z - 1 with z right and the lists untouched; the NULL
    rules and an unknown kind; d_len NULL;
  - a^2049 with min_len 1023, 1024, 1025 and 2048: the first selected rank on the last slot of a tile of the compaction, on the first
    two slots of the next and alone in the third, with nothing selected in front of it;
  - z of the right-maximal kind == edges - n of psacx_suffix_tree_dev_* on the same arrays;
  - d_lb / d_ub of a maximal-repeat call handed to psacx_occurrences_dev_* give the model's occurrence positions;
  - totality: LCP[0] overwritten (the result does not change), LCP entries of all ones, an index of noise, bwt / first of noise --
    the calls return, the room behind the lists is untouched, every triple has 0 <= lb < ub <= n, ub - lb >= 2 and len >= 1;
  - the host-pointer forms, psac_amd.repeats, SuffixArray.repeats from bytes, the C++ mirror and the command line.
The tile counts are scanned per tile of 1024 ranks, so their scan reaches a second block of 4096 entries only beyond 2^22 ranks; the
same scan (exclusive_scan_dev over 64-bit entries) runs over the directories, one entry per 64 ranks, and takes its second block at
2^18 + 1 ranks, which is tested for the maximal and supermaximal kinds.
Outputs are pre-filled with a sentinel and have PAD entries of room behind the last one, which must come back untouched; the
inputs must come back unchanged."""
import os
import subprocess

import numpy as np
import pytest

import repeats_model as M
from repeats_gpu_common import BIG, SETS, SIZES, RepIndex, agree, set_case, text_case, total
from rmq_gpu_common import Dev, PAD, SENTINEL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_KINDS = (M.RIGHT, M.MAXIMAL, M.SUPER)


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def check_case(dev, case, what, by_bytes=False):
    d = RepIndex(dev, case)
    bwt, first, _ = d.run_bwt()
    assert np.array_equal(bwt, case.bwt)
    a = M.by_bytes(case.strings) if by_bytes else None
    for kind in ALL_KINDS:
        got = d.run(kind)
        agree(got, case.results(kind), (what, kind))
        if a is not None:
            assert M.as_occurrences([(0, lb, ub, ln) for lb, ub, ln in zip(*got)], case.SA) == a[kind], (what, kind)
    assert d.unchanged()
    return d


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", SIZES)
def test_repeats_of_one_text_equal_the_model(ctx, n, bits):
    dev = Dev(ctx, bits)
    try:
        for kind in M.TEXTS:
            case = text_case(kind, n)
            check_case(dev, case, (kind, n), by_bytes=n <= 65)
            if kind == "a" and n >= 2:
                assert case.results(M.MAXIMAL) == [(j, j - 1, n, j) for j in range(1, n)] and case.results(M.SUPER) == [(n - 1, n - 2, n, n - 1)]
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["dna4", "tandem7"])
def test_repeats_at_the_third_index_level(ctx, kind, bits):
    dev = Dev(ctx, bits)
    try:
        check_case(dev, text_case(kind, BIG), (kind, BIG))
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", SETS)
def test_repeats_of_a_string_set_equal_the_model(ctx, name, bits):
    dev = Dev(ctx, bits)
    try:
        case = set_case(name)
        check_case(dev, case, name, by_bytes=False)
        sup = case.results(M.SUPER)
        if name == "acgt3000":
            assert [(ub - lb, ln) for _, lb, ub, ln in sup] == [(3000, 4)]          # ACGT; CGT, GT and T have one left byte each
            assert len(case.results(M.RIGHT)) == 4 and len(case.results(M.MAXIMAL)) == 1
        if name == "w257":
            assert (257, 7) in [(ub - lb, ln) for _, lb, ub, ln in sup]
        if name == "w257twin":
            assert 7 not in [ln for _, lb, ub, ln in sup] and (2, 8) in [(ub - lb, ln) for _, lb, ub, ln in sup]
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_small_sets_equal_the_byte_model(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        from repeats_gpu_common import Case
        for it, (n, m, sigma) in enumerate(((2, 2, 1), (9, 3, 2), (33, 5, 2), (64, 8, 3), (65, 2, 4), (40, 40, 2))):
            check_case(dev, Case(M.random_set(n, m, 50 + it, sigma), False), (n, m, sigma), by_bytes=True)
        for name in M.NAMED:                                # the named results, stated by hand in the CPU tests
            case = Case(M.NAMED[name], len(M.NAMED[name]) == 1)
            d = check_case(dev, case, name, by_bytes=True)
            for kn, k in M.KINDS.items():
                assert [list(x) for x in zip(*(a.tolist() for a in d.run(k)))] == M.golden()[name][kn], (name, kn)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_filters_count_query_and_erange(ctx, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        for case in (text_case("planted", 4097), text_case("fib", 4096), set_case("random2")):
            d = RepIndex(dev, case)
            d.run_bwt()
            for kind in ALL_KINDS:
                full = case.results(kind)
                for f in (dict(min_len=0), dict(min_len=1), dict(min_len=3), dict(min_len=9), dict(min_occ=1), dict(min_occ=3), dict(min_occ=40),
                          dict(max_occ=2), dict(max_occ=5), dict(min_len=2, min_occ=3, max_occ=9), dict(min_len=10 ** 6), dict(min_occ=3, max_occ=2)):
                    agree(d.run(kind, **f), M.select(full, **f), (kind, f))
                # one entry of room too little: z is right and nothing is written
                z = len(full)
                assert z > 0
                with pytest.raises(psac_amd.PsacxError) as e:
                    d.lists(kind, z, cap=z - 1)
                assert e.value.code == -2 and e.value.z == z
                assert all(np.all(r == SENTINEL) for r in d.raw)
                # d_len NULL
                lb, ub, ln, z2 = d.lists(kind, z, want_len=False)
                assert z2 == z and ln is None
                agree((lb[:z].astype(np.int64), ub[:z].astype(np.int64)), full, (kind, "no len"))
                assert np.all(lb[z:] == SENTINEL) and np.all(ub[z:] == SENTINEL)
            assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("min_len", [1023, 1024, 1025, 2048])
def test_first_selected_rank_at_a_tile_edge(ctx, min_len, bits):
    # a^2049: rank j is a head with L[j] = j, so min_len puts the first selected rank on the last slot of the first tile of 1024 ranks
    # of the compaction, on the first and second slot of the second tile, and on the one rank of the third, with nothing selected
    # in front of it
    n = 2049
    dev = Dev(ctx, bits)
    try:
        case = text_case("a", n)
        d = RepIndex(dev, case)
        d.run_bwt()
        for kind in (M.RIGHT, M.MAXIMAL):
            want = M.select(case.results(kind), min_len=min_len)
            assert d.count(kind, min_len=min_len) == len(want) == n - min_len
            agree(d.run(kind, min_len=min_len), want, (kind, min_len))          # (run: the count query, then the lists)
        assert M.select(case.results(M.MAXIMAL), min_len=min_len) == [(j, j - 1, n, j) for j in range(min_len, n)]
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_null_rules_and_refusals(ctx, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        case = text_case("dna4", 4097)
        d = RepIndex(dev, case)
        d.run_bwt()
        call = lambda *a: psac_amd.repeats_device(ctx, *(a + (bits,)))  # noqa: E731
        lcp, index, room = d.lcp.d_v, d.lcp.d_index, dev.put(np.full(case.n + PAD, SENTINEL, dev.dt))
        # the right-maximal kind reads neither bwt nor first
        assert call(case.n, lcp, index, None, None, M.RIGHT, 0, 0, 0, None, None, None, 0) == len(case.results(M.RIGHT))
        for kind in (M.MAXIMAL, M.SUPER):
            for b, f in ((None, d.d_first), (d.d_bwt, None), (None, None)):
                with pytest.raises(psac_amd.PsacxError) as e:
                    call(case.n, lcp, index, b, f, kind, 0, 0, 0, None, None, None, 0)
                assert e.value.code == -1
        for kind in (3, 7, 0xFFFFFFFF):
            with pytest.raises(psac_amd.PsacxError) as e:
                call(case.n, lcp, index, d.d_bwt, d.d_first, kind, 0, 0, 0, None, None, None, 0)
            assert e.value.code == -1
        for lb, ub, ln in ((None, room, None), (room, None, None), (None, None, room)):
            with pytest.raises(psac_amd.PsacxError) as e:
                call(case.n, lcp, index, d.d_bwt, d.d_first, M.MAXIMAL, 0, 0, 0, lb, ub, ln, case.n)
            assert e.value.code == -1
        for n in (0, 1):                                        # no rank above 0: nothing is read
            assert call(n, None, None, None, None, M.RIGHT, 0, 0, 0, room, room, room, 5) == 0
        if bits == 32:
            for n in (0xFFFFFFFF, 1 << 33):
                with pytest.raises(psac_amd.PsacxError) as e:
                    call(n, lcp, index, d.d_bwt, d.d_first, M.MAXIMAL, 0, 0, 0, None, None, None, 0)
                assert e.value.code == -2
        assert np.all(dev.get(room, case.n + PAD) == SENTINEL)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_right_maximal_count_equals_the_inner_nodes_of_the_suffix_tree(ctx, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        for kind in ("dna4", "fib", "tandem7"):
            case = text_case(kind, 4097)
            d = RepIndex(dev, case)
            sigma, _ = psac_amd.suffix_tree_device(ctx, d.d_text, case.n, None, None, None, bits)
            d_nodes = dev.room(case.n * (sigma + 1) * 8)
            _, edges = psac_amd.suffix_tree_device(ctx, d.d_text, case.n, d.d_sa, d.lcp.d_v, d_nodes, bits)
            # every leaf and every inner node below the root has one edge above it
            assert d.count(M.RIGHT) == edges - case.n == len(case.results(M.RIGHT))
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["text", "set"])
def test_occurrences_of_the_maximal_repeats(ctx, name, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        case = text_case("planted", 4097) if name == "text" else set_case("random")
        d = RepIndex(dev, case)
        d.run_bwt()
        want = M.select(case.results(M.MAXIMAL), min_len=4)
        z = len(want)
        lb, ub, ln, z2 = d.lists(M.MAXIMAL, z, min_len=4)
        assert z2 == z
        d_lb, d_ub, _ = d.d_lists
        d_start = dev.room((z + 1) * 8)
        tot = psac_amd.occurrences_device(ctx, d.d_sa, case.n, d.d_off, d.m, d_lb, d_ub, z, 0, d_start, None, None, 0, bits)
        assert tot == sum(r[2] - r[1] for r in want)
        d_pos, d_sid = dev.room(tot * (bits // 8)), (dev.room(tot * (bits // 8)) if d.d_off else None)
        assert psac_amd.occurrences_device(ctx, d.d_sa, case.n, d.d_off, d.m, d_lb, d_ub, z, 0, d_start, d_pos, d_sid, tot, bits) == tot
        start, pos = dev.get(d_start, z + 1, np.uint64).astype(np.int64), dev.get(d_pos, tot).astype(np.int64)
        raw = case.text.tobytes()
        for k, (_, a, b, length) in enumerate(want):
            mine = pos[start[k]:start[k + 1]]
            assert np.array_equal(mine, case.SA[a:b])
            word = raw[mine[0]:mine[0] + length]
            assert len(word) == length and all(raw[p:p + length] == word for p in mine.tolist())
        if d.d_off:
            sid = dev.get(d_sid, tot).astype(np.int64)
            assert np.array_equal(sid, np.searchsorted(case.off, pos, side="right") - 1)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_totality_over_arrays_that_are_no_index(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        case = text_case("planted", 4097)
        n, top = case.n, int(np.iinfo(dev.dt).max)
        rng = np.random.RandomState(17)
        good = RepIndex(dev, case)
        bwt, first, _ = good.run_bwt()
        # LCP[0] holds anything: the result is the one of the arrays as they were (the index is built over the array as given)
        for v in (1, 2, 7, top):
            lcp = case.LCP.astype(np.uint64)
            lcp[0] = v
            d = RepIndex(dev, case, LCP=lcp)
            d.put_bwt(bwt, first)
            for kind in ALL_KINDS:
                agree(d.run(kind), case.results(kind), ("LCP[0]", v, kind))
        noise = lambda size, dt: rng.randint(0, 1 << 32, size).astype(dt)  # noqa: E731
        lcp_ones = case.LCP.astype(np.uint64)
        lcp_ones[rng.choice(n, 300, replace=False)] = top
        variants = {
            "lcp of all ones": dict(LCP=lcp_ones),
            "index of small noise": dict(index=rng.randint(0, 9, n // 16 + 4096).astype(dev.dt)),
            "index of wide noise": dict(index=noise(n // 16 + 4096, dev.dt)),
            "index of ones": dict(index=np.full(n // 16 + 4096, top, dev.dt)),
            "index of zeros": dict(index=np.zeros(n // 16 + 4096, dev.dt)),
        }
        for what, args in variants.items():
            d = RepIndex(dev, case, **args)
            d.put_bwt(bwt, first)
            for kind in ALL_KINDS:
                lb, ub, ln = d.run(kind)                        # (the room behind the lists is checked there)
                assert total(lb, ub, ln, n), (what, kind)
            assert d.unchanged()
        for what in ("bwt of noise", "first of noise", "first of ones"):
            d = RepIndex(dev, case)
            b = noise(n, np.uint8) if what == "bwt of noise" else bwt
            f = noise(first.size, np.uint32) if what == "first of noise" else np.full(first.size, 0xFFFFFFFF, np.uint32) if what == "first of ones" else first
            d.put_bwt(b, f)
            for kind in ALL_KINDS:
                lb, ub, ln = d.run(kind)
                assert total(lb, ub, ln, n), (what, kind)
                if what == "first of ones":                     # bits at and beyond n are not read: the starts are the ranks 0 .. n - 1
                    agree((lb, ub, ln), M.by_intervals(case.LCP, bwt, np.ones(n, bool), kind), (what, kind))
                elif what == "bwt of noise":
                    agree((lb, ub, ln), M.by_intervals(case.LCP, b, case.first, kind), (what, kind))
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_pointer_forms_and_python(ctx, bits):
    import psac_amd
    dt = np.uint32 if bits == 32 else np.uint64
    for case in (text_case("planted", 4097), text_case("fib", 4096), set_case("random"), set_case("w257twin")):
        for kn, k in M.KINDS.items():
            for f in (dict(), dict(min_len=3, min_occ=3, max_occ=50)):
                lb, ub, ln = psac_amd.repeats(case.text, case.SA.astype(dt), case.LCP.astype(dt), kind=kn, offsets=case.off, ctx=ctx, **f)
                assert lb.dtype == dt and ub.dtype == dt and ln.dtype == dt
                agree((lb.astype(np.int64), ub.astype(np.int64), ln.astype(np.int64)), M.select(case.results(k), **f), (kn, f))
    with pytest.raises(psac_amd.PsacxError) as e:
        psac_amd.repeats(b"abcab", np.array([3, 0, 4, 1, 2], dt), np.array([0, 2, 0, 1, 0], dt), kind=5, ctx=ctx)
    assert e.value.code == -1
    # the chains a user runs: construct, then .repeats; construct_ss, then .repeats and occurrences
    case = text_case("planted", 4097)
    sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
    with pytest.raises(ValueError):
        sa.repeats()                                                               # nothing constructed
    sa.construct(case.text)
    for kn, k in M.KINDS.items():
        got = sa.repeats(kn, min_len=2)
        agree(tuple(a.astype(np.int64) for a in got), M.select(case.results(k), min_len=2), kn)
    with pytest.raises(ValueError):
        nolcp = psac_amd.SuffixArray(index_bits=bits, lcp=False, ctx=ctx)
        nolcp.construct(case.text)
        nolcp.repeats()
    case = set_case("random")
    ss = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
    ss.construct_ss(case.strings)
    lb, ub, ln = ss.repeats("super")
    agree((lb.astype(np.int64), ub.astype(np.int64), ln.astype(np.int64)), case.results(M.SUPER), "set")
    start, pos, sid = psac_amd.occurrences(ss.local_SA, lb, ub, offsets=ss.string_offsets, ctx=ctx)[:3]
    assert int(start[-1]) == int((ub - lb).sum()) and np.array_equal(pos[:int(start[1])].astype(np.int64), case.SA[int(lb[0]):int(ub[0])])


def test_cpp_mirror_repeats(tmp_path):
    from test_repeats_build_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "repeats header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64", "auto"])
def test_command_line(tmp_path, index):
    exe = os.path.join(ROOT, "psac_amd", "bin", "repeats")
    (tmp_path / "text").write_bytes(b"mississippi")
    out = str(tmp_path / "bwt")
    r = subprocess.run([exe, "-f", str(tmp_path / "text"), "--index", index, "--kind", "right", "--list", "--bwt", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "z: 6\nprimary: 4\n0 4 1 1\n2 4 4 1\n5 7 1 8\n7 9 2 3\n7 11 1 2\n9 11 3 2\n"
    assert open(out, "rb").read() == b"pssmipissii" and "BWT time:" in r.stderr and "Repeats time:" in r.stderr
    r = subprocess.run([exe, "-f", str(tmp_path / "text"), "--index", index, "--kind", "super", "--list", "1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: 2\n2 4 4 1\n", r.stdout + r.stderr
    r = subprocess.run([exe, "-f", str(tmp_path / "text"), "--index", index, "-l", "2", "--min-occ", "2", "--max-occ", "2", "--kind", "right"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: 3\n", r.stdout + r.stderr
    (tmp_path / "set").write_bytes(b"abcab\ncab\n")
    r = subprocess.run([exe, "-f", str(tmp_path / "set"), "--set", "--index", index, "--list"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: 2\n0 3 2 0\n6 8 3 2\n", r.stdout + r.stderr
    case = text_case("planted", 4097)
    (tmp_path / "dna").write_bytes(case.text.tobytes())
    r = subprocess.run([exe, "-f", str(tmp_path / "dna"), "--index", index, "--kind", "maximal", "-l", "5"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: %d\n" % len(M.select(case.results(M.MAXIMAL), min_len=5)), r.stdout + r.stderr
