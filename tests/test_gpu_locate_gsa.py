"""psacx_string_ends_dev, psacx_lookup_table_gsa_dev_* and psacx_locate_gsa_dev_* against the host model
(tests/locate_gsa_model.py) on its catalogue of string sets and patterns, both index widths, without a table and with tables of
k = 1, 2 and one with more than 2^16 entries; batch sizes around a wave, the pattern buffer at an odd device address; arrays that
are no suffix array, table or bitmap; malformed offsets of either kind; and the layers above: the host-pointer form, Python's
locate(..., offsets=), the C++ mirror, the `locate --set [--occ]` command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gsa_checker_model as G
import locate_gsa_model as M
import locate_model as L

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


class Dev(object):
    """Text, offsets, bitmap and suffix array of a named set in device memory, entries of `bits`; everything allocated through it
    is freed by close().  The text's last byte is the last byte of its allocation, and so is the pattern buffer's."""

    def __init__(self, ctx, name, bits, SA=None, arrays=None):
        import psac_amd
        self.ctx, self.bits, self.dt = ctx, bits, (np.uint32 if bits == 32 else np.uint64)
        self.text, self.off, sa = M.arrays(name) if arrays is None else arrays
        self.n, self.m = int(self.text.size), int(self.off.size - 1)
        self.held = []
        self.d_text = self.put(self.text)
        self.d_off = self.put(self.off)
        self.sa = (sa if SA is None else SA).astype(self.dt)
        self.d_sa = self.put(self.sa)
        self.words = psac_amd.string_ends_device(ctx, None, self.m, self.n, None)
        self.d_ends = self.put(np.full(self.words, 0xABABABAB, np.uint32))            # (the call clears the bitmap itself)
        assert psac_amd.string_ends_device(ctx, self.d_off, self.m, self.n, self.d_ends) == self.words

    def room(self, nbytes):
        p = self.ctx.alloc(max(1, nbytes))
        self.held.append(p)
        return p

    def put(self, arr, shift=0):
        p = self.room(arr.nbytes + shift) + shift
        if arr.nbytes:
            self.ctx.h2d(p, arr)
        return p

    def get(self, p, count, dt):
        out = np.empty(count, dt)
        if count:
            self.ctx.d2h(out, p)
        return out

    def table(self, k, d_ends=None):
        """(device address, code, sigma, entries, the table as the device built it)"""
        import psac_amd
        code, sigma, entries = psac_amd.lookup_table_gsa_device(self.ctx, self.d_text, self.n, None, k, None, self.bits)
        d_table = self.put(np.full(entries, 0xAB, self.dt))
        assert psac_amd.lookup_table_gsa_device(self.ctx, self.d_text, self.n, d_ends or self.d_ends, k, d_table, self.bits)[1:] == (sigma, entries)
        return d_table, code, sigma, entries, self.get(d_table, entries, self.dt)

    def locate(self, pats, d_table=None, k=0, code=None, off=None, fill=None, d_ends=None, plain=False):
        """(lb, ub) of psacx_locate_gsa_dev_* (plain: of psacx_locate_dev_* on the same arrays); the pattern buffer starts at an odd
        address.  off: offsets to pass instead of the patterns' own."""
        import psac_amd
        pat, own = psac_amd.pattern_buffer(pats)
        off = own if off is None else off
        q = int(off.size - 1)
        d_pat, d_off = self.put(pat, shift=1), self.put(off)
        assert d_pat % 2 == 1
        lb0 = np.full(q, 0x5A5A5A5A if fill is None else fill, self.dt)
        d_lb, d_ub = self.put(lb0), self.put(lb0)
        try:
            if plain:
                psac_amd.locate_device(self.ctx, self.d_text, self.n, self.d_sa, d_table, k, code, d_pat, d_off, q, d_lb, d_ub, self.bits)
            else:
                psac_amd.locate_gsa_device(self.ctx, self.d_text, self.n, d_ends or self.d_ends, self.d_sa, d_table, k, code, d_pat, d_off, q, d_lb,
                                           d_ub, self.bits)
        finally:
            self.lb, self.ub = self.get(d_lb, q, self.dt), self.get(d_ub, q, self.dt)
        return self.lb.astype(np.int64), self.ub.astype(np.int64)

    def inputs_unchanged(self):
        return (np.array_equal(self.get(self.d_text, self.n, np.uint8), self.text) and np.array_equal(self.get(self.d_sa, self.n, self.dt), self.sa)
                and np.array_equal(self.get(self.d_off, self.m + 1, np.uint64), self.off)
                and np.array_equal(self.get(self.d_ends, self.words, np.uint32), M.ends_bitmap(self.off, self.n)))

    def close(self):
        for p in self.held:
            self.ctx.free(p)
        self.held = []


def first_difference(got, want, pats):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else (int(bad[0]), len(pats[bad[0]]), pats[bad[0]][:24], int(got[bad[0]]), int(want[bad[0]]), int(bad.size))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", M.GPU)
def test_bitmap_tables_and_intervals_equal_the_model(ctx, name, bits):
    import psac_amd
    pats, lb, ub = M.expected(name)
    d = Dev(ctx, name, bits)
    try:
        assert d.words == (d.n >> 5) + 1
        assert np.array_equal(d.get(d.d_ends, d.words, np.uint32), M.ends_bitmap(d.off, d.n))
        got = d.locate(pats)
        assert first_difference(got[0], lb, pats) is None and first_difference(got[1], ub, pats) is None
        ks, refused = M.table_ks(d.text)
        want_code, want_sigma = M.codes_of(d.text)
        for k in ks:
            d_table, code, sigma, entries, table = d.table(k)
            assert sigma == want_sigma and np.array_equal(code, want_code) and entries == (sigma + 1) ** k + 1
            assert np.array_equal(table.astype(np.int64), M.table_by_definition(d.text, d.off, k)), k
            with_table = d.locate(pats, d_table, k, code)
            assert first_difference(with_table[0], lb, pats) is None and first_difference(with_table[1], ub, pats) is None, k
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.lookup_table_gsa_device(ctx, d.d_text, d.n, d.d_ends, refused, None, bits)
        assert e.value.code == -1
        code, sigma, entries = psac_amd.lookup_table_gsa_device(ctx, d.d_text, d.n, d.d_ends, refused - 1, None, bits)      # the largest that is taken
        assert entries == (sigma + 1) ** (refused - 1) + 1 <= (1 << 30) + 1
        assert d.inputs_unchanged()
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_one_string_equals_the_plain_entry_points(ctx, bits):
    import psac_amd
    # `single` of the catalogue, and a text of the plain catalogue taken as a set of one
    text = L.text_of("edge4097")
    for name, arrays in (("single", None), ("edge4097", (text, np.array([0, text.size], np.uint64), L.sa_of("edge4097")))):
        d = Dev(ctx, name, bits, arrays=arrays)
        try:
            assert d.m == 1
            pats = M.expected(name)[0] if arrays is None else L.expected(name)[0]
            for k in (0, 1, 2, M.table_ks(d.text)[0][2]):
                args, plain_args = (), ()
                if k:
                    d_table, code, sigma, entries, table = d.table(k)
                    d_plain = d.put(np.zeros(entries, d.dt))
                    assert psac_amd.lookup_table_device(ctx, d.d_text, d.n, d.d_sa, k, d_plain, bits)[1:] == (sigma, entries)
                    assert np.array_equal(table, d.get(d_plain, entries, d.dt)), (name, k)
                    args, plain_args = (d_table, k, code), (d_plain, k, code)
                got, want = d.locate(pats, *args), d.locate(pats, *plain_args, plain=True)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, k)
        finally:
            d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_batch_sizes(ctx, bits):
    # 4 000 patterns of mixed lengths cut from the reads without regard to their ends, half of them with one byte changed; every
    # batch size is a prefix of them
    name = M.READS_SMALL
    text, off, SA = M.arrays(name)
    s, n = text.tobytes(), int(text.size)
    end = M.ends_of(off, n)
    rng = np.random.RandomState(8)
    pats = []
    for i in range(4000):
        m = int(rng.choice([1, 3, 5, 8, 12, 16, 20, 31, 32, 33, 64, 100]))
        p = int(rng.randint(0, n - m + 1))
        P = bytearray(s[p:p + m])
        if i % 2:
            P[int(rng.randint(0, m))] = int(rng.choice([65, 67, 71, 84]))
        pats.append(bytes(P))
    want = [M.by_bisection(s, off, SA, P, end=end) for P in pats]
    lb, ub = np.array([a for a, b in want], np.int64), np.array([b for a, b in want], np.int64)
    assert (ub - lb > 64).any() and (ub - lb == 1).any() and (ub == lb).any()
    d = Dev(ctx, name, bits)
    try:
        d_table, code, sigma, entries, table = d.table(5)
        for q in (0, 1, 63, 64, 65, 4000):
            for args in ((), (d_table, 5, code)):
                got = d.locate(pats[:q], *args)
                assert got[0].size == q
                assert first_difference(got[0], lb[:q], pats) is None and first_difference(got[1], ub[:q], pats) is None, (q, args[1:2])
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["tiny9", "edge65", "word_edges", "edge4097", "bytes256", "unary"])
def test_arrays_that_are_no_suffix_array_table_or_bitmap(ctx, name, bits):
    # whatever SA, table and bitmap hold: PSACX_OK, and lb <= ub <= n
    pats, lb, ub = M.expected(name)
    text, off, right = M.arrays(name)
    n = int(text.size)
    rng = np.random.RandomState(4)
    ones = (1 << bits) - 1
    beyond = right.copy()
    beyond[rng.randint(0, n, max(1, n // 3))] = np.array([n, n + 12345, ones], np.uint64)[rng.randint(0, 3, max(1, n // 3))]
    for SA in (beyond, np.arange(n, dtype=np.uint64)[::-1].copy(), rng.permutation(n).astype(np.uint64)):
        d = Dev(ctx, name, bits, SA=SA)
        try:
            k = M.table_ks(text)[0][1]
            d_table, code, sigma, entries, table = d.table(k)
            assert np.array_equal(table.astype(np.int64), M.table_by_definition(text, off, k))          # the table does not depend on SA
            d_ff = d.put(np.full(entries, ones, np.uint64).astype(d.dt))
            d_all, d_none = d.put(np.full(d.words, 0xFFFFFFFF, np.uint32)), d.put(np.zeros(d.words, np.uint32))
            for d_ends in (None, d_all, d_none):
                for args in ((), (d_table, k, code), (d_ff, k, code)):
                    got = d.locate(pats, *args, d_ends=d_ends)
                    assert np.all(got[0] <= got[1]) and np.all(got[1] <= n), (d_ends, args[1:2])
                # a table over any bitmap is a table: B^k + 1 ascending entries from 0 to n
                t = d.table(k, d_ends=d_ends)[4].astype(np.int64)
                assert t[0] == 0 and t[-1] == n and np.all(np.diff(t) >= 0)
        finally:
            d.close()
    # on the right arrays a bitmap of all ones leaves one character per suffix, one of all zeros the plain search's suffixes
    d = Dev(ctx, name, bits)
    try:
        d_all = d.put(np.full(d.words, 0xFFFFFFFF, np.uint32))
        got = d.locate([b"", text.tobytes()[:1], text.tobytes()[:2]], d_ends=d_all)
        assert got[0][0] == 0 and got[1][0] == n and got[1][1] - got[0][1] <= int((text == text[0]).sum())
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_malformed_offsets_of_either_kind_are_refused_before_anything_is_written(ctx, bits):
    import psac_amd
    d = Dev(ctx, "edge4097", bits)
    try:
        # the strings' offsets.  The two offset mutants of the checker models move one offset by one character and keep the strict
        # ascent: they are the well-formed offsets of another set, which no rule can refuse (psacx_check_gsa_dev_* takes them
        # too, and counts what does not fit) -- the bitmap is then that of the offsets as given.
        fill = np.full(d.words, 0x77777777, np.uint32)
        for cls in G.MOVES_OFFSETS:
            o = d.off.copy()
            assert G.GSA_MUTANTS[cls][0](d.text.copy(), o, d.sa.astype(np.uint64), None, None, d.n // 2) and not np.array_equal(o, d.off)
            d_o, d_bits = d.put(o), d.put(fill)
            assert psac_amd.string_ends_device(ctx, d_o, d.m, d.n, d_bits) == d.words
            assert np.array_equal(d.get(d_bits, d.words, np.uint32), M.ends_bitmap(o, d.n))
        # malformed: a first offset that is not 0, a last one that is not n, an empty string, a descending pair
        mutants = []
        o = d.off.copy(); o[0] = 1; mutants.append(o)
        o = d.off.copy(); o[-1] = d.n - 1; mutants.append(o)
        o = d.off.copy(); o[-1] = d.n + 1; mutants.append(o)
        o = d.off.copy(); o[5] = o[4]; mutants.append(o)
        o = d.off.copy(); o[7], o[8] = o[8], o[7]; mutants.append(o)
        for o in mutants:
            assert not np.array_equal(o, d.off)
            d_o, d_bits = d.put(o), d.put(fill)
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.string_ends_device(ctx, d_o, d.m, d.n, d_bits)
            assert e.value.code == -1 and np.array_equal(d.get(d_bits, d.words, np.uint32), fill)
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.locate(d.text, d.sa, [b"AC"], offsets=o, ctx=ctx)
            assert e.value.code == -1
        # the patterns' offsets
        pats = [b"AC", b"", b"CCA", b"A"] * 40
        good = psac_amd.pattern_buffer(pats)[1]
        d_table, code, sigma, entries, table = d.table(2)
        for what in ("first", "descending", "descending_last"):
            off = good.copy()
            if what == "first":
                off[0] = 1
            elif what == "descending":
                off[70], off[71] = off[71], off[70]
            else:
                off[-1] = off[-2] - 1
            for args in ((), (d_table, 2, code)):
                with pytest.raises(psac_amd.PsacxError) as e:
                    d.locate(pats, *args, off=off, fill=0x77)
                assert e.value.code == -1
                assert np.all(d.lb == 0x77) and np.all(d.ub == 0x77)
        # equal neighbours are empty patterns, q == 0 is fine, and the forms with and without a table do not mix
        got = d.locate([b"", b"", b"A"])
        assert got[0][:2].tolist() == [0, 0] and got[1][:2].tolist() == [d.n, d.n]
        assert d.locate([])[0].size == 0
        for args in ((d_table, 0, None), (None, 2, code), (d_table, 2, None), (None, 0, code)):
            with pytest.raises(psac_amd.PsacxError) as e:
                d.locate(pats, *args)
            assert e.value.code == -1
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_the_eight_lane_option_changes_nothing_and_fetches_are_counted(ctx, bits, monkeypatch):
    for name in ("word_edges", "edge4097", "unary"):
        pats, lb, ub = M.expected(name)
        d = Dev(ctx, name, bits)
        try:
            k = M.table_ks(d.text)[0][1]
            d_table, code, sigma, entries, table = d.table(k)
            for args in ((), (d_table, k, code)):
                fetched = {}
                for shape in ("lane", "group"):
                    monkeypatch.setenv("PSACX_LOCATE_SHAPE", shape)
                    monkeypatch.setenv("PSACX_LOCATE_COUNT", "1")
                    got = d.locate(pats, *args)
                    assert first_difference(got[0], lb, pats) is None and first_difference(got[1], ub, pats) is None, (name, shape, args[1:2])
                    fetched[shape] = list(ctx.stats().locate_fetches)
                    monkeypatch.delenv("PSACX_LOCATE_COUNT")
                    d.locate(pats, *args)
                    assert list(ctx.stats().locate_fetches) == [0, 0]
                assert fetched["lane"] == fetched["group"] and fetched["lane"][1] >= fetched["lane"][0] > 0, (name, fetched)
        finally:
            monkeypatch.delenv("PSACX_LOCATE_SHAPE", raising=False)
            d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_pointer_form_and_python_locate(ctx, bits):
    import psac_amd
    for name in ("tiny1", "tiny17", "word_edges", "edge65", "bytes256", "prefixes"):
        pats, lb, ub = M.expected(name)
        text, off, SA = M.arrays(name)
        sa = SA.astype(np.uint32 if bits == 32 else np.uint64)
        ks = M.table_ks(text)
        for k in (0, 1, ks[0][2]):
            got = psac_amd.locate(text, sa, pats, k=k, ctx=ctx, offsets=off)
            assert got[0].dtype == sa.dtype and np.array_equal(got[0], lb) and np.array_equal(got[1], ub), (name, k)
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.locate(text, sa, pats, k=ks[1], ctx=ctx, offsets=off)
        assert e.value.code == -1
        assert psac_amd.locate(text, sa, [], k=1, ctx=ctx, offsets=off)[0].size == 0
        assert [x.tolist() for x in psac_amd.locate(text, sa, [b"", b""], ctx=ctx, offsets=off)] == [[0, 0], [text.size, text.size]]


def test_locate_after_a_construction_in_hbm(ctx):
    # the chain a user runs: construct_gsa_device leaves SA in HBM, the bitmap, the table and the search read it there
    import psac_amd
    name = M.READS_SMALL
    pats, lb, ub = M.expected(name)
    d = Dev(ctx, name, 32)
    try:
        d_isa = d.room(d.n * 4)
        d.d_sa = d.room(d.n * 4)
        ctx.check(ctx._lib.psacx_construct_gsa_dev_u32(ctx.handle, C.c_void_p(d.d_text), d.n, C.c_void_p(d.d_off), d.m, 0, 0, C.c_void_p(d.d_sa),
                                                       C.c_void_p(d_isa), None))
        d_table, code, sigma, entries, table = d.table(8)
        got = d.locate(pats, d_table, 8, code)
        assert np.array_equal(got[0], lb) and np.array_equal(got[1], ub)
    finally:
        d.close()


def test_cpp_mirror_locate_and_occurrences(tmp_path):
    from test_locate_gsa_model_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "locate_gsa header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64", "auto"])
def test_command_line(tmp_path, index):
    exe = os.path.join(ROOT, "psac_amd", "bin", "locate")
    name = "edge4097"
    text, off, SA = M.arrays(name)
    n = int(text.size)
    o = [int(x) for x in off]
    pats, lb, ub = M.expected(name)
    keep = [i for i, P in enumerate(pats) if b"\n" not in P]                    # one pattern per line
    (tmp_path / "set").write_bytes(b"".join(text.tobytes()[a:b] + b"\n" for a, b in zip(o[:-1], o[1:])))
    (tmp_path / "patterns").write_bytes(b"".join(pats[i] + b"\n" for i in keep))
    base = [exe, "-q", str(tmp_path / "patterns"), "--index", index, "-f"]
    r = subprocess.run(base + [str(tmp_path / "set"), "--set"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == M.cli_text(lb[keep], ub[keep]), r.stderr
    assert "SA time: " in r.stderr and "Ends time: " in r.stderr and "Locate time: " in r.stderr and "Occurrences time" not in r.stderr
    for limit in (0, 3):
        occ = M.occurrences(SA, n, lb[keep], ub[keep], limit, off)
        r = subprocess.run(base + [str(tmp_path / "set"), "--set", "-k", "5", "--occ"] + ([str(limit)] if limit else []), capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout == M.cli_text(lb[keep], ub[keep], occ, off), r.stderr
        assert "Table time: " in r.stderr and "Occurrences time: " in r.stderr
    # one text: the default output is what it was, and --occ adds positions
    plain = L.text_of(name)
    ppats, plb, pub = L.expected(name)
    pkeep = [i for i, P in enumerate(ppats) if b"\n" not in P]
    (tmp_path / "text").write_bytes(plain.tobytes())
    (tmp_path / "patterns").write_bytes(b"".join(ppats[i] + b"\n" for i in pkeep))
    r = subprocess.run(base + [str(tmp_path / "text")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "".join("%d %d\n" % (plb[i], pub[i]) for i in pkeep), r.stderr
    assert "Ends time" not in r.stderr and "Occurrences time" not in r.stderr
    r = subprocess.run(base + [str(tmp_path / "text"), "--occ", "2"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == M.cli_text(plb[pkeep], pub[pkeep], M.occurrences(L.sa_of(name), plain.size, plb[pkeep], pub[pkeep], 2)), r.stderr
