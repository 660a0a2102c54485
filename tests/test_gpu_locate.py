"""psacx_lookup_table_dev_* and psacx_locate_dev_* against the host model (tests/locate_model.py) on its catalogue of texts and
patterns, both index widths, without a table and with tables of k = 1, 2 and one with more than 2^16 entries; batch sizes around a
wave, the pattern buffer at an odd device address; arrays that are no suffix array or table; malformed offsets; and the layers
above: the host-pointer form, the C++ mirror, the `locate` command line."""
import os
import subprocess

import numpy as np
import pytest

import locate_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


class Dev(object):
    """Text and suffix array of a named text in device memory, entries of `bits`; everything allocated through it is freed by close()."""

    def __init__(self, ctx, name, bits, SA=None):
        self.ctx, self.bits, self.dt = ctx, bits, (np.uint32 if bits == 32 else np.uint64)
        self.text = M.text_of(name)
        self.n = int(self.text.size)
        self.held = []
        self.d_text = self.put(self.text)
        self.sa = (M.sa_of(name) if SA is None else SA).astype(self.dt)
        self.d_sa = self.put(self.sa)

    def room(self, nbytes):
        p = self.ctx.alloc(max(1, nbytes))
        self.held.append(p)
        return p

    def put(self, arr, shift=0):
        p = self.room(arr.nbytes + shift) + shift
        if arr.nbytes:
            self.ctx.h2d(p, arr)
        return p

    def table(self, k):
        """(device address, code, sigma, entries, the table as the device built it)"""
        import psac_amd
        code, sigma, entries = psac_amd.lookup_table_device(self.ctx, self.d_text, self.n, None, k, None, self.bits)
        d_table = self.put(np.full(entries, 0xAB, self.dt))                            # (the call clears the table itself)
        assert psac_amd.lookup_table_device(self.ctx, self.d_text, self.n, self.d_sa, k, d_table, self.bits)[1:] == (sigma, entries)
        got = np.empty(entries, self.dt)
        self.ctx.d2h(got, d_table)
        return d_table, code, sigma, entries, got

    def locate(self, pats, d_table=None, k=0, code=None, off=None, fill=None):
        """(lb, ub) of psacx_locate_dev_*; the pattern buffer starts at an odd address.  off: offsets to pass instead of the patterns' own."""
        import psac_amd
        pat, own = psac_amd.pattern_buffer(pats)
        off = own if off is None else off
        q = int(off.size - 1)
        d_pat, d_off = self.put(pat, shift=1), self.put(off)
        assert d_pat % 2 == 1
        lb0 = np.full(q, 0x5A5A5A5A if fill is None else fill, self.dt)
        d_lb, d_ub = self.put(lb0), self.put(lb0)
        try:
            psac_amd.locate_device(self.ctx, self.d_text, self.n, self.d_sa, d_table, k, code, d_pat, d_off, q, d_lb, d_ub, self.bits)
        finally:
            self.lb, self.ub = np.empty(q, self.dt), np.empty(q, self.dt)
            if q:
                self.ctx.d2h(self.lb, d_lb); self.ctx.d2h(self.ub, d_ub)
        return self.lb.astype(np.int64), self.ub.astype(np.int64)

    def close(self):
        for p in self.held:
            self.ctx.free(p)
        self.held = []


def first_difference(got, want, pats):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else (int(bad[0]), len(pats[bad[0]]), pats[bad[0]][:24], int(got[bad[0]]), int(want[bad[0]]), int(bad.size))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", M.ALL)
def test_intervals_and_tables_equal_the_model(ctx, name, bits):
    pats, lb, ub = M.expected(name)
    d = Dev(ctx, name, bits)
    try:
        got = d.locate(pats)
        assert first_difference(got[0], lb, pats) is None and first_difference(got[1], ub, pats) is None
        ks, refused = M.table_ks(d.text)
        want_code, want_sigma = M.codes_of(d.text)
        for k in ks:
            d_table, code, sigma, entries, table = d.table(k)
            assert sigma == want_sigma and np.array_equal(code, want_code) and entries == (sigma + 1) ** k + 1
            assert np.array_equal(table.astype(np.int64), M.table_by_definition(d.text, k)), k
            with_table = d.locate(pats, d_table, k, code)
            assert first_difference(with_table[0], lb, pats) is None and first_difference(with_table[1], ub, pats) is None, k
        import psac_amd
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.lookup_table_device(ctx, d.d_text, d.n, None, refused, None, bits)
        assert e.value.code == -1
        code, sigma, entries = psac_amd.lookup_table_device(ctx, d.d_text, d.n, None, refused - 1, None, bits)      # the largest that is taken
        assert entries == (sigma + 1) ** (refused - 1) + 1 <= (1 << 30) + 1
        # no input is written
        t2, s2 = np.empty_like(d.text), np.empty_like(d.sa)
        ctx.d2h(t2, d.d_text); ctx.d2h(s2, d.d_sa)
        assert np.array_equal(t2, d.text) and np.array_equal(s2, d.sa)
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_both_kernel_shapes_agree_with_the_model(ctx, bits, monkeypatch):
    # Eight lanes per pattern (PSACX_OPT_LOCATE_SHAPE = 2, here through the debug shim's PSACX_LOCATE_SHAPE) answers as one pattern
    # per lane does.  The counting kernels tell the shapes apart: both take the same bisection steps, so they fetch the same SA
    # entries, but a group reads every 8-byte piece of its 64-character window where a lane stops at the first piece that differs.
    for name in ("mississippi", "edge4097", "unary", "bytes256", "tandem"):
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
                assert fetched["lane"][0] == fetched["group"][0] > 0, (name, fetched)
                assert fetched["group"][1] > fetched["lane"][1] > 0, (name, fetched)
        finally:
            monkeypatch.delenv("PSACX_LOCATE_SHAPE", raising=False)
            d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_batch_sizes(ctx, bits):
    # 10 000 patterns of mixed lengths cut from the DNA text, half of them with one byte changed; every batch size is a prefix of them
    name = "dna"
    text = M.text_of(name)
    s, n, SA = text.tobytes(), int(text.size), M.sa_of(name)
    rng = np.random.RandomState(8)
    pats = []
    for i in range(10000):
        m = int(rng.choice([1, 5, 8, 12, 16, 20, 31, 32, 33, 64, 100]))
        p = int(rng.randint(0, n - m + 1))
        P = bytearray(s[p:p + m])
        if i % 2:
            P[int(rng.randint(0, m))] = int(rng.choice([65, 67, 71, 84]))
        pats.append(bytes(P))
    want = [M.by_bisection(s, SA, P) for P in pats]
    lb, ub = np.array([a for a, b in want], np.int64), np.array([b for a, b in want], np.int64)
    assert (ub - lb > 64).any() and (ub - lb == 1).any() and (ub == lb).any()
    d = Dev(ctx, name, bits)
    try:
        d_table, code, sigma, entries, table = d.table(5)
        for q in (0, 1, 63, 64, 65, 10000):
            for args in ((), (d_table, 5, code)):
                got = d.locate(pats[:q], *args)
                assert got[0].size == q
                assert first_difference(got[0], lb[:q], pats) is None and first_difference(got[1], ub[:q], pats) is None, (q, args[1:2])
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["tiny9", "edge65", "edge4097", "bytes256", "unary"])
def test_arrays_that_are_no_suffix_array_or_table(ctx, name, bits):
    # whatever SA and table hold: PSACX_OK, and lb <= ub <= n
    pats, lb, ub = M.expected(name)
    text = M.text_of(name)
    n = int(text.size)
    rng = np.random.RandomState(4)
    ones = (1 << bits) - 1
    shuffled = rng.permutation(n).astype(np.uint64)
    beyond = M.sa_of(name).copy()
    beyond[rng.randint(0, n, max(1, n // 3))] = np.array([n, n + 12345, ones], np.uint64)[rng.randint(0, 3, max(1, n // 3))]
    for SA in (shuffled, beyond, np.full(n, ones, np.uint64)):
        d = Dev(ctx, name, bits, SA=SA)
        try:
            k = M.table_ks(text)[0][1]
            d_table, code, sigma, entries, table = d.table(k)
            assert np.array_equal(table.astype(np.int64), M.table_by_definition(text, k))          # the table does not depend on SA
            wrong = table.astype(np.uint64)[::-1].copy()                                          # descending
            wrong[rng.randint(0, entries, max(1, entries // 2))] = np.array([n + 1, 2 * n + 7, ones], np.uint64)[rng.randint(0, 3, max(1, entries // 2))]
            d_wrong = d.put(wrong.astype(d.dt))
            for args in ((), (d_table, k, code), (d_wrong, k, code)):
                got = d.locate(pats, *args)
                assert np.all(got[0] <= got[1]) and np.all(got[1] <= n)
        finally:
            d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_malformed_offsets_are_refused_before_anything_is_written(ctx, bits):
    import psac_amd
    d = Dev(ctx, "edge4097", bits)
    try:
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
def test_host_pointer_form(ctx, bits):
    import psac_amd
    for name in ("mississippi", "tiny1", "edge65", "bytes256", "tandem"):
        pats, lb, ub = M.expected(name)
        text = M.text_of(name)
        sa = M.sa_of(name).astype(np.uint32 if bits == 32 else np.uint64)
        ks = M.table_ks(text)
        for k in (0, 1, ks[0][2]):
            got = psac_amd.locate(text, sa, pats, k=k, ctx=ctx)
            assert got[0].dtype == sa.dtype and np.array_equal(got[0], lb) and np.array_equal(got[1], ub), (name, k)
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.locate(text, sa, pats, k=ks[1], ctx=ctx)
        assert e.value.code == -1
        assert psac_amd.locate(text, sa, [], k=1, ctx=ctx)[0].size == 0
        assert [x.tolist() for x in psac_amd.locate(text, sa, [b"", b""], ctx=ctx)] == [[0, 0], [text.size, text.size]]


def test_locate_after_a_construction_in_hbm(ctx):
    # the chain a user runs: construct_device leaves SA in HBM, the table and the search read it there
    import psac_amd
    name = "dna"
    pats, lb, ub = M.expected(name)
    d = Dev(ctx, name, 32)
    try:
        d_isa = d.room(d.n * 4)
        d.d_sa = d.room(d.n * 4)
        psac_amd.SuffixArray(index_bits=32, ctx=ctx).construct_device(d.d_text, d.n, d.d_sa, d_isa)
        d_table, code, sigma, entries, table = d.table(8)
        got = d.locate(pats, d_table, 8, code)
        assert np.array_equal(got[0], lb) and np.array_equal(got[1], ub)
    finally:
        d.close()


def test_cpp_mirror_locate(tmp_path):
    # locate(sa, begin, end, patterns, k) for both index types against intervals stated by hand, and its refusal on two ranks
    from test_locate_model_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "locate header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64", "auto"])
def test_command_line(tmp_path, index):
    name = "edge4097"
    text = M.text_of(name)
    pats, lb, ub = M.expected(name)
    keep = [i for i, P in enumerate(pats) if b"\n" not in P]                    # one pattern per line
    exe = os.path.join(ROOT, "psac_amd", "bin", "locate")
    (tmp_path / "text").write_bytes(text.tobytes())
    (tmp_path / "patterns").write_bytes(b"".join(pats[i] + b"\n" for i in keep))
    want = "".join("%d %d\n" % (lb[i], ub[i]) for i in keep)
    r = subprocess.run([exe, "-f", str(tmp_path / "text"), "-q", str(tmp_path / "patterns"), "--index", index], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == want, r.stderr
    assert "SA time: " in r.stderr and "Locate time: " in r.stderr and " ms" in r.stderr and "Table time" not in r.stderr
    out = tmp_path / "intervals"
    r = subprocess.run([exe, "-f", str(tmp_path / "text"), "-q", str(tmp_path / "patterns"), "-k", "5", "--index", index, "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "" and out.read_text() == want, r.stderr
    assert "Table time: " in r.stderr and "Table entries: %d" % (3 ** 5 + 1) in r.stderr and "Locate time: " in r.stderr
    r = subprocess.run([exe, "-f", str(tmp_path / "text"), "-q", str(tmp_path / "patterns"), "-k", "40"], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout == "" and "psacx" in r.stderr            # 3^40 keys: refused
