"""psacx_match_dev_* against the host model (tests/match_model.py) on the catalogue of texts and patterns of locate_model, both
index widths, without a table and with tables of k = 1, 2 and one with more than 2^16 entries, capped and uncapped; the suffix
mode (matching statistics) on pieces with substituted bytes and empty patterns; batch sizes and totals around a wave and a
workgroup; arrays that are no suffix array or table; refusals; the fetch counters; and the layers above: the host-pointer form,
psac_amd.match, the chain after a construction in HBM, intervals fed to the occurrence lists, the C++ mirror, the command line.
Every call takes the pattern buffer at an odd device address and outputs pre-filled with a sentinel (tests/match_gpu_common.py)."""
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
@pytest.mark.parametrize("name", L.ALL)
def test_catalogue_equals_the_model(ctx, name, bits):
    pats, ln, lb, ub = M.expected(name)
    full = ln == np.array([len(P) for P in pats])
    d = Index(ctx, name, bits)
    try:
        b = d.batch(pats)
        for table in [None] + [d.table(k)[0] for k in L.table_ks(d.text)[0]]:
            k = table[1] if table else 0
            got = d.match(b, table)
            assert first_difference(got, (ln, lb, ub), pats) is None, k
            loc = d.locate(b, table)                                              # where the pattern occurs: locate's interval
            assert np.array_equal(got[1][full], loc[0][full]) and np.array_equal(got[2][full], loc[1][full]), k
            for max_len in sorted(set([1, 8, 9] + ([k, k + 1] if k else []))):
                want = M.expected(name, max_len)[1:]
                got = d.match(b, table, max_len=max_len)
                assert first_difference(got, want, pats) is None, (k, max_len)
                assert np.all(got[0] <= max_len)
        assert d.inputs_unchanged([b])
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", L.ALL)
def test_suffix_mode_equals_the_model(ctx, name, bits):
    d = Index(ctx, name, bits)
    try:
        pieces = M.pieces_of(d.text)
        b = d.batch(pieces)
        ks = L.table_ks(d.text)[0]
        tables = [None, d.table(ks[1])[0], d.table(ks[2])[0]]
        for max_len in (0, 32):
            queries = M.queries_of(pieces, True, max_len)
            assert len(queries) == b.total
            want = M.answers(("pieces", name, max_len), queries, d.text, L.sa_of(name))
            own = d.batch(queries)                                                # every suffix handed in as a pattern of its own
            for table in tables:
                got = d.match(b, table, suffixes=True, max_len=max_len)
                assert first_difference(got, want, queries) is None, (max_len, table and table[1])
                alone = d.match(own, table)
                assert first_difference(got, alone, queries) is None, (max_len, table and table[1])
        assert d.inputs_unchanged([b])
    finally:
        d.close()


SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 4097)


@pytest.mark.parametrize("bits", [32, 64])
def test_batch_sizes_and_totals(ctx, bits):
    name = "dna"
    text = L.text_of(name)
    s, n, SA = text.tobytes(), int(text.size), L.sa_of(name)
    rng = np.random.RandomState(9)
    pats = []
    for i in range(max(SIZES)):
        m = int(rng.choice([1, 5, 8, 12, 16, 20, 31, 32, 33, 64, 100]))
        p = int(rng.randint(0, n - m + 1))
        P = bytearray(s[p:p + m])
        if i % 2:
            P[int(rng.randint(0, m))] = int(rng.choice([65, 67, 71, 84, 78]))     # (N does not occur)
        pats.append(bytes(P))
    want = M.answers(("sizes", name), pats, text, SA)
    m_of = np.array([len(P) for P in pats])
    assert (want[0] == m_of).any() and ((want[0] > 0) & (want[0] < m_of)).any() and (want[2] - want[1] > 64).any()
    d = Index(ctx, name, bits)
    try:
        table = d.table(5)[0]
        for q in SIZES:
            b = d.batch(pats[:q])
            for tb in (None, table):
                got = d.match(b, tb)
                assert got[0].size == q and first_difference(got, [w[:q] for w in want], pats) is None, (q, tb and tb[1])
        # the suffix mode with these totals: pieces of 13 bytes (the last one shorter), every third with an N in it, an empty
        # pattern after every tenth
        for total in SIZES:
            pieces, at = [], 0
            while at < total:
                P = bytearray(s[at * 7:at * 7 + min(13, total - at)])
                if len(pieces) % 3 == 2:
                    P[len(pieces) % len(P)] = 78
                pieces.append(bytes(P))
                at += len(P)
                if len(pieces) % 10 == 0:
                    pieces.append(b"")
            pieces = pieces or [b"", b""]
            queries = M.queries_of(pieces, True)
            assert len(queries) == total
            w = M.answers(("totals", name, total), queries, text, SA)
            b = d.batch(pieces)
            for tb in (None, table):
                got = d.match(b, tb, suffixes=True)
                assert got[0].size == total and first_difference(got, w, queries) is None, (total, tb and tb[1])
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["tiny9", "edge65", "edge4097", "bytes256", "unary"])
def test_arrays_that_are_no_suffix_array_or_table(ctx, name, bits):
    # the classes test_gpu_locate.py runs.  Only the totality clause holds: len <= m, len <= max_len, lb <= ub <= n; no input is written
    pats = L.patterns_of(name)
    text = L.text_of(name)
    n = int(text.size)
    rng = np.random.RandomState(4)
    ones = (1 << bits) - 1
    shuffled = rng.permutation(n).astype(np.uint64)
    beyond = L.sa_of(name).copy()
    beyond[rng.randint(0, n, max(1, n // 3))] = np.array([n, n + 12345, ones], np.uint64)[rng.randint(0, 3, max(1, n // 3))]
    pieces = M.pieces_of(text)
    for SA in (shuffled, beyond, np.full(n, ones, np.uint64)):
        d = Index(ctx, name, bits, SA=SA)
        try:
            k = L.table_ks(text)[0][1]
            table, built = d.table(k)
            wrong = built.astype(np.uint64)[::-1].copy()                                          # descending: inverted buckets
            wrong[rng.randint(0, built.size, max(1, built.size // 2))] = np.array([n + 1, 2 * n + 7, ones], np.uint64)[rng.randint(0, 3, max(1, built.size // 2))]
            d_wrong = d.put(wrong.astype(d.dt))
            b, bs = d.batch(pats), d.batch(pieces)
            for tb in (None, table, (d_wrong, k, table[2])):
                for max_len in (0, 9):
                    assert total_holds(d.match(b, tb, max_len=max_len), pats, n, max_len)
                    assert total_holds(d.match(bs, tb, suffixes=True, max_len=max_len), M.queries_of(pieces, True), n, max_len)
            assert d.inputs_unchanged([b, bs])
        finally:
            d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_refusals_leave_the_sentinel(ctx, bits):
    import psac_amd
    d = Index(ctx, "edge4097", bits)
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
                # (the room is that of the patterns' own offsets; malformed offsets must not be trusted for it either)
                assert refused(b, table=tb, suffixes=True, out_entries=int(off[-1])), what
        for tb in (None, table):
            for delta in (-1, 1):
                assert refused(ok, table=tb, out_entries=ok.q + delta)
                assert refused(ok, table=tb, suffixes=True, out_entries=ok.total + delta)
            assert refused(ok, table=tb, out_entries=ok.total)                     # the other mode's count
            for flags in (2, 3, 0x80000000):
                assert refused(ok, table=tb, flags=flags)
        for mix in ((table[0], 0, None), (None, 2, table[2]), (table[0], 2, None), (None, 0, table[2])):
            assert refused(ok, table=mix)
        # equal neighbours are empty patterns; q == 0 is fine in both modes
        got = d.match(d.batch([b"", b"", b"A"]))
        assert got[0].tolist()[:2] == [0, 0] and got[1].tolist()[:2] == [0, 0] and got[2].tolist()[:2] == [d.n, d.n]
        assert d.match(d.batch([]))[0].size == 0 and d.match(d.batch([]), suffixes=True)[0].size == 0
        assert d.match(d.batch([b"", b""]), suffixes=True)[0].size == 0             # no slot to fill
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_fetch_counters(ctx, bits, monkeypatch):
    # PSACX_OPT_LOCATE_COUNT (here through the debug shim's PSACX_LOCATE_COUNT): the results do not change, the counters are filled,
    # and on a batch of patterns that all occur both searches are those of locate, probe for probe
    for name in ("mississippi", "edge4097", "unary", "bytes256", "tandem"):
        pats, ln, lb, ub = M.expected(name)
        occurring = [P for P, x in zip(pats, ln) if x == len(P)]
        d = Index(ctx, name, bits)
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
    for name in ("mississippi", "tiny1", "edge65", "bytes256", "tandem"):
        text = L.text_of(name)
        sa = L.sa_of(name).astype(np.uint32 if bits == 32 else np.uint64)
        pats, ln, lb, ub = M.expected(name)
        pieces = M.pieces_of(text)
        ks = L.table_ks(text)
        for k in (0, 1, ks[0][2]):
            got = psac_amd.match(text, sa, pats, k=k, ctx=ctx)
            assert got[0].dtype == sa.dtype and first_difference(got, (ln, lb, ub), pats) is None, (name, k)
            got = psac_amd.match(text, sa, pats, k=k, max_len=9, ctx=ctx)
            assert first_difference(got, M.expected(name, 9)[1:], pats) is None, (name, k)
            queries = M.queries_of(pieces, True, 32)
            got = psac_amd.match(text, sa, pieces, k=k, suffixes=True, max_len=32, ctx=ctx)
            assert first_difference(got, M.answers(("pieces", name, 32), queries, text, L.sa_of(name)), queries) is None, (name, k)
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.match(text, sa, pats, k=ks[1], ctx=ctx)
        assert e.value.code == -1
        assert psac_amd.match(text, sa, [], k=1, ctx=ctx)[0].size == 0
        assert psac_amd.match(text, sa, [b"", b""], suffixes=True, ctx=ctx)[0].size == 0
        assert [x.tolist() for x in psac_amd.match(text, sa, [b"", b""], ctx=ctx)] == [[0, 0], [0, 0], [text.size, text.size]]


def test_match_after_a_construction_in_hbm_and_occurrences(ctx):
    # the chain a user runs: construct_device leaves SA in HBM, table and search read it there, and the occurrence lists take the
    # intervals as they are
    import psac_amd
    name = "dna"
    pats, ln, lb, ub = M.expected(name)
    d = Index(ctx, name, 32)
    try:
        d_isa = d.room(d.n * 4)
        d.d_sa = d.room(d.n * 4)
        psac_amd.SuffixArray(index_bits=32, ctx=ctx).construct_device(d.d_text, d.n, d.d_sa, d_isa)
        table = d.table(8)[0]
        b = d.batch(pats)
        init = np.full(b.q, 0x5A5A5A5A, np.uint32)
        d_len, d_lb, d_ub = d.put(init), d.put(init), d.put(init)
        psac_amd.match_device(ctx, d.d_text, d.n, d.d_sa, table[0], 8, table[2], b.d_pat, b.d_off, b.q, 0, 0, b.q, d_len, d_lb, d_ub, 32)
        got = [d.get(p, b.q, np.uint32).astype(np.int64) for p in (d_len, d_lb, d_ub)]
        assert first_difference(got, (ln, lb, ub), pats) is None
        limit = 5
        d_start = d.room((b.q + 1) * 8)
        total = psac_amd.occurrences_device(ctx, d.d_sa, d.n, None, 0, d_lb, d_ub, b.q, limit, d_start, None, None, 0, 32)
        d_pos = d.room(total * 4)
        psac_amd.occurrences_device(ctx, d.d_sa, d.n, None, 0, d_lb, d_ub, b.q, limit, d_start, d_pos, None, total, 32)
        start, pos, _ = G.occurrences(L.sa_of(name), d.n, lb, ub, limit)
        assert total == int(start[-1]) > b.q                 # never empty: every query lists at least one occurrence of its prefix
        assert np.array_equal(d.get(d_start, b.q + 1, np.uint64), start) and np.array_equal(d.get(d_pos, total, np.uint32), pos)
        s = d.text.tobytes()
        for i in (0, b.q // 2, b.q - 1):
            for t in range(int(start[i]), int(start[i + 1])):
                assert s[int(pos[t]):int(pos[t]) + int(ln[i])] == pats[i][:int(ln[i])]
    finally:
        d.close()


def test_cpp_mirror_match(tmp_path):
    from test_match_model_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "match header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64", "auto"])
def test_command_line(tmp_path, index):
    name = "edge4097"
    text, SA = L.text_of(name), L.sa_of(name)
    n = int(text.size)
    pats = [P for P in L.patterns_of(name) if b"\n" not in P and len(P) <= 100][:120] + [b"", b""]      # one pattern per line
    exe = os.path.join(ROOT, "psac_amd", "bin", "locate")
    (tmp_path / "text").write_bytes(text.tobytes())
    (tmp_path / "patterns").write_bytes(b"".join(P + b"\n" for P in pats))
    base = [exe, "-f", str(tmp_path / "text"), "-q", str(tmp_path / "patterns"), "--index", index]
    want = M.answers(("cli", name), pats, text, SA)
    r = subprocess.run(base + ["--longest"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == M.cli_text(*want), r.stderr
    assert "SA time: " in r.stderr and "Match time: " in r.stderr and "Locate time" not in r.stderr
    # every suffix, capped, with a table, the occurrences on the same line
    queries = M.queries_of(pats, True, 9)
    w9 = M.answers(("cli9", name), queries, text, SA)
    out = tmp_path / "out"
    r = subprocess.run(base + ["--longest", "--suffixes", "--max-len", "9", "-k", "5", "--occ", "3", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "", r.stderr
    assert out.read_text() == M.cli_text(w9[0], w9[1], w9[2], G.occurrences(SA, n, w9[1], w9[2], 3))
    assert "Table time: " in r.stderr and "Match time: " in r.stderr and "Occurrences time: " in r.stderr
    # without --longest the tool prints what it printed before
    lb, ub = zip(*[L.by_bisection(text, SA, P) for P in pats])
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == G.cli_text(lb, ub) and "Locate time: " in r.stderr and "Match time" not in r.stderr
