"""psacx_match_gsa_dev_* against the host model (tests/match_model.py) on the catalogue of string sets and patterns of
locate_gsa_model, both index widths, without a table and with tables of k = 1, 2 and one with more than 2^16 entries, capped
and uncapped; the suffix mode; a set of one string against the plain form; arrays that are no suffix array, table or bitmap;
refusals; the fetch counters; and the layers above: the host-pointer form through psac_amd.match(offsets=), the chain after a
construction in HBM with occurrence lists and string ids, and the `locate --set --longest` command line.
Every call takes the pattern buffer at an odd device address and outputs pre-filled with a sentinel (tests/match_gpu_common.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import locate_gsa_model as G
import locate_model as L
import match_model as M
from match_gpu_common import Index, first_difference, total_holds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", G.GPU)
def test_catalogue_equals_the_model(ctx, name, bits):
    pats, ln, lb, ub = M.expected_gsa(name)
    full = ln == np.array([len(P) for P in pats])
    d = Index(ctx, name, bits, set=True)
    try:
        b = d.batch(pats)
        for table in [None] + [d.table(k)[0] for k in L.table_ks(d.text)[0]]:
            k = table[1] if table else 0
            got = d.match(b, table)
            assert first_difference(got, (ln, lb, ub), pats) is None, k
            loc = d.locate(b, table)                                              # where the pattern occurs: locate's interval
            assert np.array_equal(got[1][full], loc[0][full]) and np.array_equal(got[2][full], loc[1][full]), k
            for max_len in sorted(set([1, 8, 9] + ([k, k + 1] if k else []))):
                want = M.expected_gsa(name, max_len)[1:]
                got = d.match(b, table, max_len=max_len)
                assert first_difference(got, want, pats) is None, (k, max_len)
                assert np.all(got[0] <= max_len)
        assert d.inputs_unchanged([b])
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", G.GPU)
def test_suffix_mode_equals_the_model(ctx, name, bits):
    # (unary, copies and prefixes are among them: suffixes that end inside the matched length)
    d = Index(ctx, name, bits, set=True)
    try:
        pieces = M.pieces_of(d.text)
        b = d.batch(pieces)
        ks = L.table_ks(d.text)[0]
        tables = [None, d.table(ks[1])[0], d.table(ks[2])[0]]
        for max_len in (0, 32):
            queries = M.queries_of(pieces, True, max_len)
            assert len(queries) == b.total
            want = M.answers(("set pieces", name, max_len), queries, d.text, G.arrays(name)[2], d.off)
            own = d.batch(queries)                                                # every suffix handed in as a pattern of its own
            for table in tables:
                got = d.match(b, table, suffixes=True, max_len=max_len)
                assert first_difference(got, want, queries) is None, (max_len, table and table[1])
                alone = d.match(own, table)
                assert first_difference(got, alone, queries) is None, (max_len, table and table[1])
        assert d.inputs_unchanged([b])
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_one_string_equals_the_plain_form(ctx, bits):
    for name in ("mississippi", "tiny1", "edge65", "unary", "bytes256", "tandem"):
        text, sa = L.text_of(name), L.sa_of(name)
        pats, ln, lb, ub = M.expected(name)
        pieces = M.pieces_of(text)
        d = Index(ctx, name, bits, set=True, arrays=(text, np.array([0, text.size], np.uint64), sa))
        try:
            b, bs = d.batch(pats), d.batch(pieces)
            for table in (None, d.table(L.table_ks(text)[0][1])[0]):
                got = d.match(b, table)
                assert first_difference(got, (ln, lb, ub), pats) is None, name
                # the plain entry point on the same arrays (with one string the two tables are the same table)
                assert first_difference(got, d.match(b, table, plain=True), pats) is None, name
                for max_len in (0, 32):
                    queries = M.queries_of(pieces, True, max_len)
                    got = d.match(bs, table, suffixes=True, max_len=max_len)
                    assert first_difference(got, d.match(bs, table, suffixes=True, max_len=max_len, plain=True), queries) is None, name
                    assert first_difference(got, M.answers(("pieces", name, max_len), queries, text, sa), queries) is None, name
        finally:
            d.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["tiny9", "edge65", "word_edges", "edge4097", "bytes256", "unary"])
def test_arrays_that_are_no_suffix_array_table_or_bitmap(ctx, name, bits):
    # the classes test_gpu_locate_gsa.py runs.  Only the totality clause holds: len <= m, len <= max_len, lb <= ub <= n; no input is written
    text, off, right = G.arrays(name)
    pats = G.patterns_of(name)
    pieces = M.pieces_of(text)
    n = int(text.size)
    rng = np.random.RandomState(4)
    ones = (1 << bits) - 1
    beyond = right.copy()
    beyond[rng.randint(0, n, max(1, n // 3))] = np.array([n, n + 12345, ones], np.uint64)[rng.randint(0, 3, max(1, n // 3))]
    for SA in (beyond, np.arange(n, dtype=np.uint64)[::-1].copy(), rng.permutation(n).astype(np.uint64)):
        d = Index(ctx, name, bits, set=True, SA=SA)
        try:
            k = L.table_ks(text)[0][1]
            table, built = d.table(k)
            wrong = built.astype(np.uint64)[::-1].copy()                                          # descending: inverted buckets
            wrong[rng.randint(0, built.size, max(1, built.size // 2))] = np.array([n + 1, 2 * n + 7, ones], np.uint64)[rng.randint(0, 3, max(1, built.size // 2))]
            d_wrong = d.put(wrong.astype(d.dt))
            d_all, d_none = d.put(np.full(d.words, 0xFFFFFFFF, np.uint32)), d.put(np.zeros(d.words, np.uint32))
            b, bs = d.batch(pats), d.batch(pieces)
            for d_ends in (None, d_all, d_none):
                for tb in (None, table, (d_wrong, k, table[2])):
                    for max_len in (0, 9):
                        assert total_holds(d.match(b, tb, max_len=max_len, d_ends=d_ends), pats, n, max_len)
                        assert total_holds(d.match(bs, tb, suffixes=True, max_len=max_len, d_ends=d_ends), M.queries_of(pieces, True), n, max_len)
            assert d.inputs_unchanged([b, bs])
        finally:
            d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_refusals_leave_the_sentinel(ctx, bits):
    import psac_amd
    d = Index(ctx, "edge4097", bits, set=True)
    try:
        pats = [b"AC", b"", b"CCA", b"A"] * 40
        good = psac_amd.pattern_buffer(pats)[1]
        table = d.table(2)[0]
        ok = d.batch(pats)

        def refused(b, **kw):
            with pytest.raises(psac_amd.PsacxError) as e:
                d.match(b, fill=0x77, **kw)
            return e.value.code == -1 and d.untouched(0x77)

        for what in ("first", "descending", "descending_last"):
            off = good.copy()
            if what == "first":
                off[0] = 1
            elif what == "descending":
                off[70], off[71] = off[71], off[70]
            else:
                off[-1] = off[-2] - 1
            b = d.batch(pats, off=off)
            for tb in (None, table):
                assert refused(b, table=tb), what
                assert refused(b, table=tb, suffixes=True, out_entries=int(off[-1])), what
        for tb in (None, table):
            for delta in (-1, 1):
                assert refused(ok, table=tb, out_entries=ok.q + delta)
                assert refused(ok, table=tb, suffixes=True, out_entries=ok.total + delta)
            for flags in (2, 3, 0x80000000):
                assert refused(ok, table=tb, flags=flags)
        for mix in ((table[0], 0, None), (None, 2, table[2]), (table[0], 2, None), (None, 0, table[2])):
            assert refused(ok, table=mix)
        # the set form needs its bitmap
        init = np.full(ok.q, 0x77, d.dt)
        d_out = [d.put(init) for _ in range(3)]
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.match_gsa_device(ctx, d.d_text, d.n, None, d.d_sa, None, 0, None, ok.d_pat, ok.d_off, ok.q, 0, 0, ok.q, d_out[0], d_out[1], d_out[2], bits)
        assert e.value.code == -1 and all(np.all(d.get(p, ok.q, d.dt) == 0x77) for p in d_out)
        assert d.match(d.batch([]))[0].size == 0 and d.match(d.batch([b"", b""]), suffixes=True)[0].size == 0
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_fetch_counters(ctx, bits, monkeypatch):
    for name in ("word_edges", "copies", "prefixes", "unary", "bytes256"):
        pats, ln, lb, ub = M.expected_gsa(name)
        occurring = [P for P, x in zip(pats, ln) if x == len(P)]
        d = Index(ctx, name, bits, set=True)
        try:
            b, bo = d.batch(pats), d.batch(occurring)
            for table in (None, d.table(L.table_ks(d.text)[0][1])[0]):
                monkeypatch.setenv("PSACX_LOCATE_COUNT", "1")
                got = d.match(b, table)
                assert first_difference(got, (ln, lb, ub), pats) is None
                counted = list(ctx.stats().locate_fetches)
                assert counted[0] > 0 and counted[1] > 0
                got = d.match(bo, table)
                by_match = list(ctx.stats().locate_fetches)
                loc = d.locate(bo, table)
                assert list(ctx.stats().locate_fetches) == by_match and by_match[0] > 0, (name, by_match)
                assert np.array_equal(got[1], loc[0]) and np.array_equal(got[2], loc[1])
                monkeypatch.delenv("PSACX_LOCATE_COUNT")
                d.match(b, table)
                assert list(ctx.stats().locate_fetches) == [0, 0]
        finally:
            monkeypatch.delenv("PSACX_LOCATE_COUNT", raising=False)
            d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_pointer_form_and_python(ctx, bits):
    import psac_amd
    for name in ("tiny9", "word_edges", "copies", "prefixes", "bytes256"):
        text, off, SA = G.arrays(name)
        sa = SA.astype(np.uint32 if bits == 32 else np.uint64)
        pats, ln, lb, ub = M.expected_gsa(name)
        pieces = M.pieces_of(text)
        for k in (0, 1, L.table_ks(text)[0][2]):
            got = psac_amd.match(text, sa, pats, k=k, offsets=off, ctx=ctx)
            assert got[0].dtype == sa.dtype and first_difference(got, (ln, lb, ub), pats) is None, (name, k)
            queries = M.queries_of(pieces, True, 32)
            got = psac_amd.match(text, sa, pieces, k=k, offsets=off, suffixes=True, max_len=32, ctx=ctx)
            assert first_difference(got, M.answers(("set pieces", name, 32), queries, text, SA, off), queries) is None, (name, k)
        with pytest.raises(psac_amd.PsacxError) as e:                               # offsets that do not end at n
            psac_amd.match(text, sa, pats, offsets=np.array([0, text.size + 1], np.uint64), ctx=ctx)
        assert e.value.code == -1


def test_match_after_a_construction_in_hbm_and_occurrences(ctx):
    # the chain a user runs: construct_gsa_device leaves SA in HBM; bitmap, table and search read it there; the occurrence lists
    # take the intervals as they are and name the strings
    import psac_amd
    name = G.READS_SMALL
    pats, ln, lb, ub = M.expected_gsa(name)
    text, off, SA = G.arrays(name)
    d = Index(ctx, name, 32, set=True)
    try:
        d_isa = d.room(d.n * 4)
        d.d_sa = d.room(d.n * 4)
        ctx.check(ctx._lib.psacx_construct_gsa_dev_u32(ctx.handle, C.c_void_p(d.d_text), d.n, C.c_void_p(d.d_soff), d.m, 0, 0, C.c_void_p(d.d_sa),
                                                       C.c_void_p(d_isa), None))
        table = d.table(8)[0]
        b = d.batch(pats)
        init = np.full(b.q, 0x5A5A5A5A, np.uint32)
        d_len, d_lb, d_ub = d.put(init), d.put(init), d.put(init)
        psac_amd.match_gsa_device(ctx, d.d_text, d.n, d.d_ends, d.d_sa, table[0], 8, table[2], b.d_pat, b.d_off, b.q, 0, 0, b.q, d_len, d_lb, d_ub, 32)
        got = [d.get(p, b.q, np.uint32).astype(np.int64) for p in (d_len, d_lb, d_ub)]
        assert first_difference(got, (ln, lb, ub), pats) is None
        limit = 4
        d_start = d.room((b.q + 1) * 8)
        total = psac_amd.occurrences_device(ctx, d.d_sa, d.n, d.d_soff, d.m, d_lb, d_ub, b.q, limit, d_start, None, None, 0, 32)
        d_pos, d_sid = d.room(total * 4), d.room(total * 4)
        psac_amd.occurrences_device(ctx, d.d_sa, d.n, d.d_soff, d.m, d_lb, d_ub, b.q, limit, d_start, d_pos, d_sid, total, 32)
        start, pos, _ = G.occurrences(SA, d.n, lb, ub, limit)
        assert total == int(start[-1]) >= b.q
        assert np.array_equal(d.get(d_start, b.q + 1, np.uint64), start) and np.array_equal(d.get(d_pos, total, np.uint32), pos)
        assert np.array_equal(d.get(d_sid, total, np.uint32), G.string_ids(off, pos, d.n))
    finally:
        d.close()


@pytest.mark.parametrize("index", ["32", "64", "auto"])
def test_command_line(tmp_path, index):
    exe = os.path.join(ROOT, "psac_amd", "bin", "locate")
    name = "edge4097"
    text, off, SA = G.arrays(name)
    n = int(text.size)
    o = [int(x) for x in off]
    pats = [P for P in G.patterns_of(name) if b"\n" not in P and len(P) <= 100][:120] + [b"", b""]      # one pattern per line
    (tmp_path / "set").write_bytes(b"".join(text.tobytes()[a:b] + b"\n" for a, b in zip(o[:-1], o[1:])))
    (tmp_path / "patterns").write_bytes(b"".join(P + b"\n" for P in pats))
    base = [exe, "-f", str(tmp_path / "set"), "-q", str(tmp_path / "patterns"), "--index", index, "--set", "--longest"]
    want = M.answers(("set cli", name), pats, text, SA, off)
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == M.cli_text(*want), r.stderr
    assert "Ends time: " in r.stderr and "Match time: " in r.stderr and "Locate time" not in r.stderr
    queries = M.queries_of(pats, True, 9)
    w9 = M.answers(("set cli9", name), queries, text, SA, off)
    r = subprocess.run(base + ["--suffixes", "--max-len", "9", "-k", "5", "--occ", "3"], capture_output=True, text=True)
    start, pos, _ = G.occurrences(SA, n, w9[1], w9[2], 3)
    assert r.returncode == 0 and r.stdout == M.cli_text(w9[0], w9[1], w9[2], (start, pos, G.string_ids(off, pos, n)), off), r.stderr
    assert "Table time: " in r.stderr and "Match time: " in r.stderr and "Occurrences time: " in r.stderr
