"""psacx_kmismatch_dev_* against the host model (tests/kmismatch_model.py, whose two formulations tests/test_kmismatch_model_cpu.py
holds to each other on the same catalogue), both index widths, SA from the oracle:

  - one text and the same text cut into a set at odd places, at n = 1, 2, 3, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097 over random texts
    of 2 and 4 letters, a^n, a Fibonacci word, a period-7 tandem repeat and all 256 byte values; patterns of 1, 7, 8, 9, 31, 32, 33, 63,
    64, 65 and 130 bytes cut from the text (the word masks, the piece cuts and the switch from pattern words in registers to the
    pattern buffer at 32), the same with 1 to e + 1 bytes substituted, windows at 0 and at n, the whole text, a longer pattern, an
    empty one, m = e and m = e + 1, a byte the text lacks, and for the set a window that ends at a string end and one across it;
    e = 0, 1, 2, 3, and e = 15 once per text; without a table, with k = 1, 2 and a table of more than 2^16 entries;
  - triples and work equal the model's; the count query agrees; the sentinel stands behind z; the inputs are unchanged; with e = 0
    the positions are those of psacx_occurrences_dev_* over psacx_locate_dev_*;
  - batches of 63, 64 and 65 patterns; 1023, 1024 and 1025 candidates; more than 2 x 1024 candidates inside one piece; the pattern
    buffer at an odd address;
  - PSACX_ERANGE at cap = z - 1 and at max_cand = work[0] - 1; PSACX_EINVAL for e = 16, malformed offsets, mixed NULL lists and
    mixed table arguments; q = 0 and n = 0; the timing option PSACX_OPT_KMISMATCH_STOP;
  - totality: a shuffled SA, an SA with entries >= n and a table of noise give only true hits;
  - the host-pointer form, psac_amd.kmismatch, SuffixArray.kmismatch, the C++ program and the command line on the named cases."""
import os
import subprocess

import numpy as np
import pytest

import kmismatch_model as X
from kmismatch_gpu_common import SENTINEL64, SENTINEL8, KmmIndex, check, table_ks
from rmq_gpu_common import Dev, SENTINEL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -2


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
@pytest.mark.parametrize("n", X.SIZES)
def test_hits_equal_the_model(ctx, n, as_set, bits):
    dev = Dev(ctx, bits)
    try:
        for kind in X.TEXTS:
            case = X.case(kind, n, as_set)
            for e in (0, 1, 2, 3):
                d = KmmIndex(dev, case, case.patterns(e))
                got, _ = check(d, e, (kind, n, e))
                if e == 0:
                    assert np.array_equal(got[1], d.exact_positions()), (kind, n)
                for k in table_ks(case.text):
                    d.set_table(k)
                    check(d, e, (kind, n, e, "k", k))
                    if e == 0 and k == 2:
                        assert np.array_equal(got[1], d.exact_positions()), (kind, n, "k")
                assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
@pytest.mark.parametrize("kind", X.TEXTS)
def test_fifteen_mismatches(ctx, kind, as_set, bits):
    dev = Dev(ctx, bits)
    try:
        case = X.case(kind, 4097, as_set)
        d = KmmIndex(dev, case, case.patterns(15), k=2)
        got, work = check(d, 15, (kind, 15))
        assert X.true_hits(case.text, case.off, d.pats, 15, got) and work[0] > 0
        d.no_table()
        check(d, 15, (kind, 15, "no table"))
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_batches_of_63_64_and_65_patterns_and_an_odd_buffer_address(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        case = X.case("dna4", 4097)
        s = case.text.tobytes()
        rng = np.random.RandomState(3)
        for q in (63, 64, 65):
            pats = []
            for _ in range(q):
                a, m = int(rng.randint(0, 4000)), int(rng.randint(0, 70))
                pats.append(X.substituted(s[a:a + m], int(rng.randint(0, 3)), rng, np.frombuffer(b"ACGT", np.uint8)) if m else b"")
            want = X.by_pieces(case.text, None, case.SA, pats, 2)
            for shift in (0, 1):
                d = KmmIndex(dev, case, pats, shift=shift)
                assert (d.d_pat & 1) == shift
                check(d, 2, (q, shift), want)
                assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_tile_ownership(ctx, bits):
    """a^n and the pattern a^(e+1): e + 1 pieces a with n candidates each; n - e windows, each tested from every piece and reported
    from piece 0.  1024 candidates at n = 512 with e = 1, 1023 at n = 341 with e = 2, 1025 at n = 205 with e = 4.  a^3000 has more
    than 2 x 1024 candidates inside each single piece, so whole tiles lie inside one piece and others begin in one and end in the
    next."""
    dev = Dev(ctx, bits)
    try:
        for n, e, cands in ((512, 1, 1024), (341, 2, 1023), (205, 4, 1025), (3000, 1, 6000), (3000, 0, 3000)):
            case = X.case("a", n)
            pats = [b"", b"a" * (e + 1), b"b"]
            d = KmmIndex(dev, case, pats)
            got, work = check(d, e, (n, e), X.by_pieces(case.text, None, case.SA, pats, e))
            assert work[0] == cands and got[0].size == n - e and np.all(got[2] == 0) and np.all(got[0] == 1)
            assert work[1] == (e + 1) * (n - e)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_refusals(ctx, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        case = X.case("dna2", 4097)
        d = KmmIndex(dev, case, case.patterns(2))
        (qi, tp, di), work = d.run(2)
        z = qi.size
        assert z > 10 and work[0] > z
        # cap = z - 1: PSACX_ERANGE, z valid, lists untouched
        with pytest.raises(psac_amd.PsacxError) as err:
            d.call(2, z, cap=z - 1)
        assert err.value.code == ERANGE and err.value.z == z
        assert np.all(d.raw[0] == SENTINEL64) and np.all(d.raw[1] == SENTINEL) and np.all(d.raw[2] == SENTINEL8)
        # max_cand = work[0] - 1: PSACX_ERANGE with z = 0 and work[0] valid; work[0] itself passes
        w = []
        with pytest.raises(psac_amd.PsacxError) as err:
            d.call(2, z, max_cand=work[0] - 1, work=w)
        assert err.value.code == ERANGE and err.value.z == 0 and w == [work[0], 0]
        assert np.all(d.raw[0] == SENTINEL64) and np.all(d.raw[1] == SENTINEL) and np.all(d.raw[2] == SENTINEL8)
        assert d.call(2, z, max_cand=work[0])[3] == z
        # e = 16
        with pytest.raises(psac_amd.PsacxError) as err:
            d.call(16, z)
        assert err.value.code == EINVAL and np.all(d.raw[0] == SENTINEL64)
        # malformed offsets: a first offset that is not 0, and a descending pair
        j = int(np.nonzero(d.poff)[0][1])                    # poff[j - 1] > 0
        for at, value in ((0, 1), (j, int(d.poff[j - 1]) - 1), (d.q, 0)):
            bad = d.poff.copy()
            bad[at] = value
            with pytest.raises(psac_amd.PsacxError) as err:
                d.call(2, z, poff=dev.put(bad))
            assert err.value.code == EINVAL and np.all(d.raw[0] == SENTINEL64) and np.all(d.raw[1] == SENTINEL) and np.all(d.raw[2] == SENTINEL8)
        # mixed NULL lists
        room = dev.room(8 * (z + 1))
        for lists in ((room, None, None), (None, room, None), (None, None, room), (room, room, None), (None, room, room)):
            with pytest.raises(psac_amd.PsacxError) as err:
                psac_amd.kmismatch_device(ctx, d.d_text, d.n, None, d.d_sa, None, 0, None, d.d_pat, d.d_poff, d.q, 2, 0, lists[0], lists[1], lists[2], z, bits)
            assert err.value.code == EINVAL
        # mixed table arguments
        d.set_table(2)
        for table, k, code in ((d.d_table, 0, d.code), (d.d_table, 2, None), (None, 2, d.code), (None, 0, d.code), (d.d_table, 0, None)):
            with pytest.raises(psac_amd.PsacxError) as err:
                psac_amd.kmismatch_device(ctx, d.d_text, d.n, None, d.d_sa, table, k, code, d.d_pat, d.d_poff, d.q, 2, 0, None, None, None, 0, bits)
            assert err.value.code == EINVAL
        # no pattern buffer: only a batch of empty patterns may come without one
        empty = dev.put(np.zeros(4, np.uint64))
        assert psac_amd.kmismatch_device(ctx, d.d_text, d.n, None, d.d_sa, None, 0, None, None, empty, 3, 2, 0, None, None, None, 0, bits) == 0
        with pytest.raises(psac_amd.PsacxError) as err:
            psac_amd.kmismatch_device(ctx, d.d_text, d.n, None, d.d_sa, None, 0, None, None, d.d_poff, d.q, 2, 0, None, None, None, 0, bits)
        assert err.value.code == EINVAL
        # q = 0 and n = 0
        w = []
        assert d.call(2, 0, q=0, work=w)[3] == 0 and w == [0, 0]
        assert psac_amd.kmismatch_device(ctx, d.d_text, 0, None, d.d_sa, None, 0, None, d.d_pat, d.d_poff, d.q, 2, 0, None, None, None, 0, bits) == 0
        assert d.unchanged()
    finally:
        dev.close()


def test_the_timing_option_ends_the_call_after_a_stage(ctx, monkeypatch):
    import psac_amd
    dev = Dev(ctx, 32)
    try:
        case = X.case("dna2", 4097)
        d = KmmIndex(dev, case, case.patterns(2))
        (qi, _, _), work = d.run(2)
        for stage, want in ((1, (work[0], 0)), (2, work)):
            monkeypatch.setenv("PSACX_KMISMATCH_STOP", str(stage))      # (the wrappers configure from the environment under the test suite)
            ctx.configure(kmismatch_stop=stage)
            w = []
            got = d.call(2, qi.size, work=w)
            assert got[3] == 0 and tuple(w) == want and np.all(got[0] == SENTINEL64) and np.all(got[1] == SENTINEL) and np.all(got[2] == SENTINEL8)
        monkeypatch.delenv("PSACX_KMISMATCH_STOP")
        with pytest.raises(psac_amd.PsacxError):
            ctx.configure(kmismatch_stop=3)
        ctx.configure(kmismatch_stop=0)
        assert d.run(2)[1] == work and d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
def test_wrong_arrays_give_only_true_hits(ctx, as_set, bits):
    dev = Dev(ctx, bits)
    try:
        rng = np.random.RandomState(17)
        for kind, n in (("dna2", 4097), ("tandem7", 4095), ("bytes256", 65)):
            case = X.case(kind, n, as_set)
            pats = case.patterns(2)
            shuffled = case.SA[rng.permutation(n)]
            beyond = case.SA.copy()
            beyond[rng.randint(0, n, n // 3 + 1)] = n + rng.randint(0, 1000, n // 3 + 1)
            beyond[rng.randint(0, n, 3)] = (1 << (bits - 1)) - 1
            for what, SA in (("shuffled", shuffled), ("beyond", beyond), ("right", None)):
                d = KmmIndex(dev, case, pats, SA=SA)
                for k, table in ((0, None), (2, rng.randint(0, 1 << 31, 1 << 12)), (1, np.full(4, (1 << (bits - 1)) + 5, np.uint64))):
                    if k:
                        d.set_table(k, table)
                    got, work = d.run(2)
                    assert X.true_hits(case.text, case.off, pats, 2, got), (kind, what, k)
                    assert work[1] <= work[0] and got[0].size <= work[1]
                    assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_forms_and_wrappers_on_the_named_cases(ctx, bits):
    import psac_amd
    dt = np.uint32 if bits == 32 else np.uint64
    g = X.golden()
    rows = lambda got: [list(x) for x in zip(*(a.tolist() for a in got))]  # noqa: E731
    for name in X.NAMED:
        t, off, SA, pats = X.named_arrays(name)
        for e in (0, 1, 2):
            for k in (0, 2):
                got = psac_amd.kmismatch(t, SA.astype(dt), pats, e, k=k, offsets=off, ctx=ctx)
                assert got[0].dtype == np.uint64 and got[1].dtype == dt and got[2].dtype == np.uint8
                assert rows(got) == g[name]["e%d" % e]["triples"], (name, e, k)
        sa = psac_amd.SuffixArray(index_bits=bits, ctx=ctx)
        if off is None:
            sa.construct(t.tobytes())
        else:
            sa.construct_ss(X.NAMED[name][0])
        assert rows(sa.kmismatch(pats, 1)) == g[name]["e1"]["triples"]
        assert rows(sa.kmismatch(pats, 1, k=2)) == g[name]["e1"]["triples"]
    t, off, SA, pats = X.named_arrays("abcab_cab")
    with pytest.raises(psac_amd.PsacxError) as err:         # 21 candidates
        psac_amd.kmismatch(t, SA.astype(dt), pats, 1, offsets=off, max_cand=20, ctx=ctx)
    assert err.value.code == ERANGE
    assert len(psac_amd.kmismatch(t, SA.astype(dt), pats, 1, offsets=off, max_cand=21, ctx=ctx)[0]) == 9
    with pytest.raises(psac_amd.PsacxError) as err:         # offsets that do not end at n
        psac_amd.kmismatch(t, SA.astype(dt), pats, 1, offsets=np.array([0, 5, 7]), ctx=ctx)
    assert err.value.code == EINVAL
    assert all(a.size == 0 for a in psac_amd.kmismatch(t, SA.astype(dt), [], 1, ctx=ctx))
    # the raw host form: the count query, and a cap too small
    lib = ctx._lib
    fn = getattr(lib, "psacx_kmismatch_u%d" % bits)
    import ctypes as C
    pat, poff = X.pattern_buffer(pats)
    sa_, o64 = np.ascontiguousarray(SA.astype(dt)), np.ascontiguousarray(off, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    z = C.c_uint64(77)
    head = [ctx.handle, p(t), t.size, p(o64), o64.size - 1, p(sa_), p(pat), p(poff), len(pats), 0, 1, 0]
    assert fn(*(head + [None, None, None, 0, C.byref(z)])) == 0 and z.value == 9
    qid, tpos, dist = np.full(9, SENTINEL64, np.uint64), np.full(9, SENTINEL, dt), np.full(9, SENTINEL8, np.uint8)
    assert fn(*(head + [p(qid), p(tpos), p(dist), 8, C.byref(z)])) == ERANGE and z.value == 9
    assert np.all(qid == SENTINEL64) and np.all(tpos == SENTINEL) and np.all(dist == SENTINEL8)
    assert fn(*(head + [p(qid), None, p(dist), 9, C.byref(z)])) == EINVAL


def test_cpp_program(tmp_path):
    from test_kmismatch_build_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "kmismatch header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64"])
def test_command_line(tmp_path, index):
    exe = os.path.join(ROOT, "psac_amd", "bin", "kmismatch")
    g = X.golden()
    strings, pats = X.NAMED["mississippi"]
    (tmp_path / "text").write_bytes(strings[0])
    (tmp_path / "pats").write_bytes(b"\n".join(pats) + b"\n")
    base = [exe, "-f", str(tmp_path / "text"), "-q", str(tmp_path / "pats"), "--index", index]
    for e in (0, 1, 2):
        want = g["mississippi"]["e%d" % e]
        head = "z: %d\ncandidates: %d\ntested: %d\n" % (len(want["triples"]), want["work"][0], want["work"][1])
        for extra in ([], ["-k", "2"]):
            r = subprocess.run(base + ["-e", str(e), "--list"] + extra, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert r.stdout == head + "".join("%d 0 %d %d\n" % tuple(row) for row in want["triples"]), (e, extra)
        r = subprocess.run(base + ["-e", str(e)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == head
    r = subprocess.run(base + ["-e", "2", "--list", "3"], capture_output=True, text=True)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 6
    r = subprocess.run(base + ["-e", "2", "--max-cand", "22"], capture_output=True, text=True)      # 23 candidates
    assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
    # a set: one string per line; positions are printed inside their string
    strings, pats = X.NAMED["abcab_cab"]
    (tmp_path / "set").write_bytes(b"\n".join(strings) + b"\n")
    (tmp_path / "spats").write_bytes(b"\n".join(pats) + b"\n")
    r = subprocess.run([exe, "-f", str(tmp_path / "set"), "-q", str(tmp_path / "spats"), "--index", index, "--set", "-e", "1", "--list"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "z: 9\ncandidates: 21\ntested: 13\n0 0 2 0\n0 1 0 0\n1 0 0 0\n2 0 1 0\n3 0 2 1\n3 1 0 1\n3 0 3 1\n3 1 1 1\n3 0 0 1\n"
