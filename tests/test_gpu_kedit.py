"""psacx_kedit_dev_* against the host model (tests/kedit_model.py, whose two statements tests/test_kedit_model_cpu.py holds to each
other), both index widths, SA from the oracle:

  - one text and the same text cut into a set at odd places, at n = 1, 2, 3, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097 over the text
    kinds of the catalogue; the patterns of kedit_model.patterns_of; e = 0, 1, 2, 3; without a table and with k = 1, 2; the model is
    by_definition up to n = 65 and by_pieces beyond; hits, work and order equal the model's, the count query agrees, the sentinel
    stands behind z, the inputs are unchanged;
  - e = 15 on patterns of 16, 17, 130 and 300 bytes; e = 4, 5, 8 and 9 once (the buckets of the band);
  - batches of 63, 64 and 65 patterns and the pattern buffer at an odd address;
  - 1023, 1024, 1025 and 2049 candidates, and the same numbers of raw hits; a tandem repeat and a^n, where every piece and every shift
    finds the same start;
  - PSACX_KEDIT_BEST; cap = z and cap = z - 1; every refusal of the header with the outputs untouched; PSACX_OPT_KEDIT_STOP; the
    statistics of the context after a call;
  - totality: a shuffled SA, an SA with entries >= n and a table of noise give only true quadruples, none twice;
  - the host-pointer form, psac_amd.kedit, SuffixArray.kedit, the C++ program and the command line on the named cases."""
import os
import subprocess

import numpy as np
import pytest

import kedit_model as K
from kedit_gpu_common import SENTINEL64, SENTINEL8, KedIndex, check
from rmq_gpu_common import Dev, SENTINEL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ERANGE = -1, -2
BEST = 1


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
@pytest.mark.parametrize("n", K.SIZES)
def test_hits_equal_the_model(ctx, n, as_set, bits):
    dev = Dev(ctx, bits)
    try:
        for kind in K.TEXTS:
            case = K.case(kind, n, as_set)
            for e in (0, 1, 2, 3):
                d = KedIndex(dev, case, K.patterns(case, e))
                got, _ = check(d, e, (kind, n, e))
                if e == 0:                                   # the occurrences of locate and occurrences, by position inside every pattern
                    per_pattern = np.split(d.exact_positions(), np.cumsum(np.bincount(got[0], minlength=d.q))[:-1])
                    assert np.array_equal(got[1], np.concatenate([np.sort(x) for x in per_pattern])), (kind, n)
                for k in (1, 2):
                    d.set_table(k)
                    check(d, e, (kind, n, e, "k", k))
                assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
def test_fifteen_edits_and_the_buckets_of_the_band(ctx, as_set, bits):
    dev = Dev(ctx, bits)
    try:
        case = K.case("dna4", 4097, as_set)
        s = case.text.tobytes()
        rng = np.random.RandomState(5)
        letters = np.frombuffer(b"ACGT", np.uint8)
        for e in (15, 4, 5, 8, 9):
            pats = []
            for m in (16, 17, 130, 300):
                a = int(rng.randint(0, 4097 - m))
                pats += [s[a:a + m], K.edited(s[a:a + m], e // 2, rng, letters), K.edited(s[a:a + m], e, rng, letters), K.edited(s[a:a + m], e + 1, rng, letters)]
            pats += [s[:e], s[:e + 1], s[4097 - 40:], b""]
            want = K.by_pieces(case.text, case.off, case.SA, pats, e)
            d = KedIndex(dev, case, pats, k=2)
            got, work = check(d, e, (e, "k2"), want)
            assert K.true_hits(case.text, case.off, d.pats, e, got) and got[0].size > 8 and work[1] > got[0].size
            d.no_table()
            check(d, e, (e, "no table"), want)
            check(d, e, (e, "best"), want, flags=BEST)
            assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_batches_of_63_64_and_65_patterns_and_an_odd_buffer_address(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        case = K.case("dna4", 4097)
        s = case.text.tobytes()
        rng = np.random.RandomState(3)
        for q in (63, 64, 65):
            pats = []
            for _ in range(q):
                a, m = int(rng.randint(0, 4000)), int(rng.randint(0, 70))
                pats.append(K.edited(s[a:a + m], int(rng.randint(0, 3)), rng, np.frombuffer(b"ACGT", np.uint8)) if m else b"")
            want = K.by_pieces(case.text, None, case.SA, pats, 2)
            for shift in (0, 1):
                d = KedIndex(dev, case, pats, shift=shift)
                assert (d.d_pat & 1) == shift
                check(d, 2, (q, shift), want)
                assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_tile_ownership_and_the_unique(ctx, bits):
    """a^n and the pattern a^(e+1): e + 1 pieces a with n candidates each, and every start of the text a hit (the last e ones at the
    distance of the bytes they lack), found from every piece and every shift.  Candidates: 1024 at n = 512 with e = 1, 1023 at n = 341
    with e = 2, 1025 at n = 205 with e = 4, 2049 at n = 683 with e = 2.  Raw hits with e = 0 are the candidates: n = 1023, 1024, 1025,
    2049.  a^3000 has more than 2 x 1024 candidates inside each single piece.  A period-7 tandem repeat and two periods of it."""
    dev = Dev(ctx, bits)
    try:
        for n, e, cands in ((512, 1, 1024), (341, 2, 1023), (205, 4, 1025), (683, 2, 2049), (3000, 1, 6000), (1023, 0, 1023), (1024, 0, 1024),
                            (1025, 0, 1025), (2049, 0, 2049)):
            case = K.case("a", n)
            pats = [b"", b"a" * (e + 1), b"b"]
            d = KedIndex(dev, case, pats)
            got, work = check(d, e, (n, e), K.by_pieces(case.text, None, case.SA, pats, e))
            assert work[0] == cands and got[0].size == n and np.all(got[0] == 1) and np.array_equal(got[1], np.arange(n))
            assert np.array_equal(got[3], np.maximum(0, e + 1 - (n - np.arange(n)))) and work[1] >= n and (e == 0 or work[1] > 2 * n)
            if e == 0:
                assert work[1] == cands
        case = K.case("tandem7", 4095)
        pats = [case.text[:14].tobytes(), case.text[3:24].tobytes()]
        want = K.by_pieces(case.text, None, case.SA, pats, 2)
        got, work = check(KedIndex(dev, case, pats), 2, "tandem7", want)
        assert work[1] > 2 * got[0].size and got[0].size > 4095     # (found from several pieces and shifts)
        check(KedIndex(dev, case, pats), 2, "tandem7 best", want, flags=BEST)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
def test_best_keeps_the_smallest_distance_of_every_pattern(ctx, as_set, bits):
    dev = Dev(ctx, bits)
    try:
        for kind in ("dna2", "fib", "bytes256"):
            case = K.case(kind, 4097, as_set)
            for e in (1, 3):
                d = KedIndex(dev, case, K.patterns(case, e))
                all_, _ = d.run(e)
                got, _ = check(d, e, (kind, e, "best"), flags=BEST)
                assert 0 < got[0].size < all_[0].size and d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_refusals(ctx, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        case = K.case("dna2", 4097)
        d = KedIndex(dev, case, K.patterns(case, 2))
        (qi, tp, ln, di), work = d.run(2)
        z = qi.size
        assert z > 10 and work[1] > z
        # cap = z: the lists; cap = z - 1: PSACX_ERANGE, z valid, lists untouched
        assert d.call(2, z, cap=z)[4] == z
        for flags in (0, BEST):
            zf = d.call(2, 0, lists=False, flags=flags)[4]
            with pytest.raises(psac_amd.PsacxError) as err:
                d.call(2, z, cap=zf - 1, flags=flags)
            assert err.value.code == ERANGE and err.value.z == zf and d.untouched()
        # max_cand = work[0] - 1: PSACX_ERANGE with z = 0 and work[0] valid; work[0] itself passes
        w = []
        with pytest.raises(psac_amd.PsacxError) as err:
            d.call(2, z, max_cand=work[0] - 1, work=w)
        assert err.value.code == ERANGE and err.value.z == 0 and w == [work[0], 0] and d.untouched()
        assert d.call(2, z, max_cand=work[0])[4] == z
        # e = 16, unknown flag bits
        for e, flags in ((16, 0), (2, 2), (2, 1 << 31), (2, 3)):
            with pytest.raises(psac_amd.PsacxError) as err:
                d.call(e, z, flags=flags)
            assert err.value.code == EINVAL and d.untouched()
        # malformed offsets: a first offset that is not 0, and a descending pair
        j = int(np.nonzero(d.poff)[0][1])                    # poff[j - 1] > 0
        for at, value in ((0, 1), (j, int(d.poff[j - 1]) - 1), (d.q, 0)):
            bad = d.poff.copy()
            bad[at] = value
            with pytest.raises(psac_amd.PsacxError) as err:
                d.call(2, z, poff=dev.put(bad))
            assert err.value.code == EINVAL and d.untouched()
        # mixed NULL lists
        room = dev.room(8 * (z + 1))
        for lists in ((room, None, None, None), (None, room, None, None), (None, None, room, None), (None, None, None, room), (room, room, room, None),
                      (None, room, room, room), (room, room, None, room)):
            with pytest.raises(psac_amd.PsacxError) as err:
                psac_amd.kedit_device(ctx, d.d_text, d.n, None, d.d_sa, None, 0, None, d.d_pat, d.d_poff, d.q, 2, 0, 0, lists[0], lists[1], lists[2], lists[3], z,
                                      bits)
            assert err.value.code == EINVAL
        # mixed table arguments
        d.set_table(2)
        for table, k, code in ((d.d_table, 0, d.code), (d.d_table, 2, None), (None, 2, d.code), (None, 0, d.code), (d.d_table, 0, None)):
            with pytest.raises(psac_amd.PsacxError) as err:
                psac_amd.kedit_device(ctx, d.d_text, d.n, None, d.d_sa, table, k, code, d.d_pat, d.d_poff, d.q, 2, 0, 0, None, None, None, None, 0, bits)
            assert err.value.code == EINVAL
        # no pattern buffer: only a batch of empty patterns may come without one
        empty = dev.put(np.zeros(4, np.uint64))
        assert psac_amd.kedit_device(ctx, d.d_text, d.n, None, d.d_sa, None, 0, None, None, empty, 3, 2, 0, 0, None, None, None, None, 0, bits) == 0
        with pytest.raises(psac_amd.PsacxError) as err:
            psac_amd.kedit_device(ctx, d.d_text, d.n, None, d.d_sa, None, 0, None, None, d.d_poff, d.q, 2, 0, 0, None, None, None, None, 0, bits)
        assert err.value.code == EINVAL
        # q = 0 and n = 0; n beyond the index type and, with 32 bits, q = 2^32
        w = []
        assert d.call(2, 0, q=0, work=w)[4] == 0 and w == [0, 0]
        assert psac_amd.kedit_device(ctx, d.d_text, 0, None, d.d_sa, None, 0, None, d.d_pat, d.d_poff, d.q, 2, 0, 0, None, None, None, None, 0, bits) == 0
        if bits == 32:
            for n, q in ((1 << 32, d.q), (d.n, 1 << 32)):
                with pytest.raises(psac_amd.PsacxError) as err:
                    psac_amd.kedit_device(ctx, d.d_text, n, None, d.d_sa, None, 0, None, d.d_pat, d.d_poff, q, 2, 0, 0, None, None, None, None, 0, bits)
                assert err.value.code == ERANGE
        assert d.unchanged()
    finally:
        dev.close()


def test_the_timing_option_ends_the_call_after_a_stage(ctx, monkeypatch):
    import psac_amd
    dev = Dev(ctx, 32)
    try:
        case = K.case("dna2", 4097)
        d = KedIndex(dev, case, K.patterns(case, 2))
        (qi, _, _, _), work = d.run(2)
        for stage, want in ((1, (work[0], 0)), (2, work), (3, work)):
            monkeypatch.setenv("PSACX_KEDIT_STOP", str(stage))          # (the wrappers configure from the environment under the test suite)
            ctx.configure(kedit_stop=stage)
            w = []
            got = d.call(2, qi.size, work=w)
            assert got[4] == 0 and tuple(w) == want and d.untouched()
        monkeypatch.delenv("PSACX_KEDIT_STOP")
        with pytest.raises(psac_amd.PsacxError):
            ctx.configure(kedit_stop=4)
        ctx.configure(kedit_stop=0)
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
            case = K.case(kind, n, as_set)
            pats = K.patterns(case, 2)
            shuffled = case.SA[rng.permutation(n)]
            beyond = case.SA.copy()
            beyond[rng.randint(0, n, n // 3 + 1)] = n + rng.randint(0, 1000, n // 3 + 1)
            beyond[rng.randint(0, n, 3)] = (1 << (bits - 1)) - 1
            for what, SA in (("shuffled", shuffled), ("beyond", beyond), ("right", None)):
                d = KedIndex(dev, case, pats, SA=SA)
                for k, table in ((0, None), (2, rng.randint(0, 1 << 31, 1 << 12)), (1, np.full(4, (1 << (bits - 1)) + 5, np.uint64))):
                    if k:
                        d.set_table(k, table)
                    for flags in (0, BEST):
                        got, work = d.run(2, flags)
                        assert K.true_hits(case.text, case.off, pats, 2, got), (kind, what, k, flags)
                        assert got[0].size <= work[1] and np.all(np.diff(got[0]) >= 0)
                    assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_forms_and_wrappers_on_the_named_cases(ctx, bits):
    import psac_amd
    dt = np.uint32 if bits == 32 else np.uint64
    g = K.golden()
    rows = lambda got: [list(x) for x in zip(*(a.tolist() for a in got))]  # noqa: E731
    for name in K.NAMED:
        t, off, SA, pats = K.named_arrays(name)
        for e in (0, 1, 2):
            want = g[name]["e%d" % e]["quadruples"]
            for k in (0, 2):
                got = psac_amd.kedit(t, SA.astype(dt), pats, e, k=k, offsets=off, ctx=ctx)
                assert got[0].dtype == np.uint64 and got[1].dtype == dt and got[2].dtype == dt and got[3].dtype == np.uint8
                assert rows(got) == want, (name, e, k)
            least = {}
            for r in want:
                least[r[0]] = min(r[3], least.get(r[0], 99))
            assert rows(psac_amd.kedit(t, SA.astype(dt), pats, e, offsets=off, best=True, ctx=ctx)) == [r for r in want if r[3] == least[r[0]]]
        sa = psac_amd.SuffixArray(index_bits=bits, ctx=ctx)
        if off is None:
            sa.construct(t.tobytes())
        else:
            sa.construct_ss(K.NAMED[name][0])
        assert rows(sa.kedit(pats, 1)) == g[name]["e1"]["quadruples"]
        assert rows(sa.kedit(pats, 1, k=2)) == g[name]["e1"]["quadruples"]
        assert all(r[3] == least[r[0]] for r in rows(sa.kedit(pats, 2, best=True)))
    t, off, SA, pats = K.named_arrays("abcab_cab")
    with pytest.raises(psac_amd.PsacxError) as err:         # 21 candidates
        psac_amd.kedit(t, SA.astype(dt), pats, 1, offsets=off, max_cand=20, ctx=ctx)
    assert err.value.code == ERANGE
    assert len(psac_amd.kedit(t, SA.astype(dt), pats, 1, offsets=off, max_cand=21, ctx=ctx)[0]) == 25
    with pytest.raises(psac_amd.PsacxError) as err:         # offsets that do not end at n
        psac_amd.kedit(t, SA.astype(dt), pats, 1, offsets=np.array([0, 5, 7]), ctx=ctx)
    assert err.value.code == EINVAL
    assert all(a.size == 0 for a in psac_amd.kedit(t, SA.astype(dt), [], 1, ctx=ctx))
    # the raw host form: the count query, a cap too small, mixed lists, an unknown flag
    import ctypes as C
    fn = getattr(ctx._lib, "psacx_kedit_u%d" % bits)
    pat, poff = K.pattern_buffer(pats)
    sa_, o64 = np.ascontiguousarray(SA.astype(dt)), np.ascontiguousarray(off, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    z = C.c_uint64(77)
    head = [ctx.handle, p(t), t.size, p(o64), o64.size - 1, p(sa_), p(pat), p(poff), len(pats), 0, 1, 0]
    assert fn(*(head + [0, None, None, None, None, 0, C.byref(z)])) == 0 and z.value == 25
    qid, tpos, ln, dist = np.full(25, SENTINEL64, np.uint64), np.full(25, SENTINEL, dt), np.full(25, SENTINEL, dt), np.full(25, SENTINEL8, np.uint8)
    assert fn(*(head + [0, p(qid), p(tpos), p(ln), p(dist), 24, C.byref(z)])) == ERANGE and z.value == 25
    assert np.all(qid == SENTINEL64) and np.all(tpos == SENTINEL) and np.all(ln == SENTINEL) and np.all(dist == SENTINEL8)
    assert fn(*(head + [0, p(qid), None, p(ln), p(dist), 25, C.byref(z)])) == EINVAL
    assert fn(*(head + [4, None, None, None, None, 0, C.byref(z)])) == EINVAL


def test_the_statistics_of_the_context_survive_a_call(ctx):
    """the sort of the raw hits leaves psacx_get_stats as it was: the last construction is still there"""
    import ctypes as C
    import psac_amd
    case = K.case("dna2", 4097)
    sa = psac_amd.SuffixArray(index_bits=32, ctx=ctx)
    sa.construct(case.text.tobytes())

    def snapshot():
        st = ctx.stats()
        st.grid_cuts = 0                                      # (counts launches since the context was made)
        st.locate_fetches[0] = st.locate_fetches[1] = 0       # (the piece searches' own)
        return bytes(C.string_at(C.addressof(st), C.sizeof(st)))
    before = snapshot()
    assert ctx.stats().n_rounds > 0
    got = sa.kedit(K.patterns(case, 2), 2)
    assert got[0].size > 1000 and snapshot() == before


def test_cpp_program(tmp_path):
    from test_kedit_build_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "kedit header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64"])
def test_command_line(tmp_path, index):
    exe = os.path.join(ROOT, "psac_amd", "bin", "kedit")
    g = K.golden()
    strings, pats = K.NAMED["mississippi"]
    (tmp_path / "text").write_bytes(strings[0])
    (tmp_path / "pats").write_bytes(b"\n".join(pats) + b"\n")
    base = [exe, "-f", str(tmp_path / "text"), "-q", str(tmp_path / "pats"), "--index", index]
    for e in (0, 1, 2):
        want = g["mississippi"]["e%d" % e]
        head = "z: %d\ncandidates: %d\nraw hits: %d\n" % (len(want["quadruples"]), want["work"][0], want["work"][1])
        for extra in ([], ["-k", "2"]):
            r = subprocess.run(base + ["-e", str(e), "--list"] + extra, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert r.stdout == head + "".join("%d 0 %d %d %d\n" % tuple(row) for row in want["quadruples"]), (e, extra)
        r = subprocess.run(base + ["-e", str(e)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == head
    r = subprocess.run(base + ["-e", "2", "--list", "3"], capture_output=True, text=True)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 6
    r = subprocess.run(base + ["-e", "1", "--best", "--list"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == "z: 4" and r.stdout.splitlines()[3:] == ["0 0 1 4 0", "0 0 4 4 0", "1 0 5 5 1", "4 0 6 3 0"]
    r = subprocess.run(base + ["-e", "2", "--max-cand", "22"], capture_output=True, text=True)      # 23 candidates
    assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr
    # a set: one string per line; positions are printed inside their string
    strings, pats = K.NAMED["abcab_cab"]
    (tmp_path / "set").write_bytes(b"\n".join(strings) + b"\n")
    (tmp_path / "spats").write_bytes(b"\n".join(pats) + b"\n")
    r = subprocess.run([exe, "-f", str(tmp_path / "set"), "-q", str(tmp_path / "spats"), "--index", index, "--set", "-e", "0", "--list"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "z: 4\ncandidates: 4\nraw hits: 4\n0 0 2 3 0\n0 1 0 3 0\n1 0 0 3 0\n2 0 1 2 0\n"
