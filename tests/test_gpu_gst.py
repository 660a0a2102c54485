"""psacx_suffix_tree_gsa_dev_*: the node table of a string set built from arrays resident in HBM, cell for cell against the host
model (tests/gst_model.py, whose arrays come from the oracle's construct_ss), with the host-pointer form, the size query, a
stored LCP[0] that is not zero, malformed offsets, and the device checker's verdict on every table built; and `gsac -t`.

What the sets are for:
  tiny<n>        n = 1, 2, 3, 7, 8, 9, 17 characters in strings of one to three
  edge<n>        the two-letter texts of st_checker_model with n = 63 .. 4097, cut unevenly: ends of the 64-entry groups and of the
                 pyramid levels of the searches
  word_edges     offsets 31, 32, 33, 63, 64, 65: the ends of the words of the string-end bitmap
  copies         151 copies of one read: a $-range of 151 leaves under one node
  prefixes       every prefix of one read; unary: one letter; tandem_pieces: a tandem repeat cut unevenly (60 000 characters)
  single         one string: the table of psacx_suffix_tree_dev_* with its column 0 doubled
  bytes256       all 256 bytes: a row of 258 cells
"""
import os
import re
import subprocess

import numpy as np
import pytest

import gsa_checker_model as G
import gst_model as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


class Dev(object):
    """A string set and its arrays in HBM, as the index type under test; the table is allocated once sigma is known."""

    def __init__(self, ctx, text, off, SA, LCP, bits, cells):
        self.ctx, self.n, self.m, self.bits = ctx, int(text.size), int(off.size - 1), bits
        self.dt = np.uint32 if bits == 32 else np.uint64
        w = bits // 8
        self.text, self.off = ctx.alloc(self.n), ctx.alloc(off.size * 8)
        self.sa, self.lcp, self.nodes = ctx.alloc(self.n * w), ctx.alloc(self.n * w), ctx.alloc(cells * 8)
        ctx.h2d(self.text, text); ctx.h2d(self.off, np.asarray(off, np.uint64))
        ctx.h2d(self.sa, SA.astype(self.dt)); ctx.h2d(self.lcp, LCP.astype(self.dt))

    def build(self):
        import psac_amd
        return psac_amd.suffix_tree_gsa_device(self.ctx, self.text, self.n, self.off, self.m, self.sa, self.lcp, self.nodes, self.bits)

    def check(self):
        import psac_amd
        return psac_amd.check_suffix_tree_gsa_device(self.ctx, self.text, self.n, self.off, self.m, self.sa, self.lcp, self.nodes, self.bits)

    def table(self, shape):
        got = np.empty(shape, np.uint64)
        self.ctx.d2h(got, self.nodes)
        return got

    def close(self):
        for p in (self.text, self.off, self.sa, self.lcp, self.nodes):
            self.ctx.free(p)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", T.ALL)
def test_device_table_equals_the_model(ctx, name, bits):
    import psac_amd
    text, off, SA, LCP, recs, table = T.arrays(name)
    n, R = int(text.size), int(recs[2].size)
    g = Dev(ctx, text, off, SA, LCP, bits, table.size)
    try:
        # the size query needs no arrays
        assert psac_amd.suffix_tree_gsa_device(ctx, g.text, n, None, 0, None, None, None, bits) == (table.shape[1] - 2, 0)
        assert psac_amd.suffix_tree_gsa_device(ctx, g.text, n, g.off, g.m, None, None, None, bits) == (table.shape[1] - 2, 0)
        ctx.h2d(g.nodes, np.full(table.size, 0xDEADBEEF, np.uint64))                       # (the call clears the table itself)
        assert g.build() == (table.shape[1] - 2, R)
        got = g.table(table.shape)
        assert np.array_equal(got, table), np.argwhere(got != table)[:5]
        assert g.check() == [0, 0, R, int(np.count_nonzero(table))]
        # the host-pointer form gives the same table
        dt = np.uint32 if bits == 32 else np.uint64
        assert np.array_equal(psac_amd.suffix_tree_gsa(text, off, SA.astype(dt), LCP.astype(dt), ctx=ctx), table)
        # the inputs are byte-identical afterwards
        t2, o2, s2, l2 = np.empty_like(text), np.empty(off.size, np.uint64), np.empty(n, dt), np.empty(n, dt)
        ctx.d2h(t2, g.text); ctx.d2h(o2, g.off); ctx.d2h(s2, g.sa); ctx.d2h(l2, g.lcp)
        assert np.array_equal(t2, text) and np.array_equal(o2, off) and np.array_equal(s2, SA) and np.array_equal(l2, LCP)
    finally:
        g.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_one_string_gives_the_one_string_table(ctx, bits):
    import psac_amd
    text, off, SA, LCP, recs, table = T.arrays("single")
    n = int(text.size)
    g = Dev(ctx, text, off, SA, LCP, bits, table.size)
    try:
        sigma, edges = g.build()
        st = np.empty((n, sigma + 1), np.uint64)
        assert psac_amd.suffix_tree_device(ctx, g.text, n, g.sa, g.lcp, g.nodes, bits) == (sigma, edges)
        ctx.d2h(st, g.nodes)
        assert T.single_string_relation(table, st)
    finally:
        g.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["tiny9", "edge65", "edge4097", "copies", "tandem_pieces"])
def test_a_stored_lcp0_is_never_used_as_a_value(ctx, name, bits):
    # 7 occurs elsewhere in the LCP arrays of the larger sets, which would end a search for equal values early if it were read
    text, off, SA, LCP, recs, table = T.arrays(name)
    R = int(recs[2].size)
    g = Dev(ctx, text, off, SA, LCP, bits, table.size)
    try:
        for v in (7, int(np.iinfo(g.dt).max)):
            l = LCP.astype(g.dt)
            l[0] = v
            ctx.h2d(g.lcp, l)
            assert g.build() == (table.shape[1] - 2, R), v
            assert np.array_equal(g.table(table.shape), table), v
            assert g.check() == [0, 0, R, int(np.count_nonzero(table))], v
            back = np.empty_like(l)
            ctx.d2h(back, g.lcp)
            assert np.array_equal(back, l)                   # no input is written
    finally:
        g.close()
    if name in ("copies", "tandem_pieces", "edge4097"):
        assert int((LCP[1:] == 7).sum()) > 0


@pytest.mark.parametrize("bits", [32, 64])
def test_malformed_offsets_are_refused(ctx, bits):
    import psac_amd
    text, off, SA, LCP, recs, table = T.arrays("tiny17")
    n = int(text.size)
    g = Dev(ctx, text, off, SA, LCP, bits, table.size)
    try:
        bad = []
        o = off.copy(); o[0] = 1; bad.append(o)                                  # does not start at 0
        o = off.copy(); o[-1] = n - 1; bad.append(o)                             # does not end at n
        o = off.copy(); o[-1] = n + 1; bad.append(o)
        o = off.copy(); o[2] = o[1]; bad.append(o)                               # an empty string
        o = off.copy(); o[1], o[2] = o[2], o[1]; bad.append(o)                   # not ascending
        o = off.copy(); o[1] = np.iinfo(np.uint64).max; bad.append(o)
        for o in bad:
            ctx.h2d(g.off, o)
            for call in (g.build, g.check):
                with pytest.raises(psac_amd.PsacxError) as e:
                    call()
                assert e.value.code == -1, o
            dt = np.uint32 if bits == 32 else np.uint64
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.suffix_tree_gsa(text, o, SA.astype(dt), LCP.astype(dt), ctx=ctx)
            assert e.value.code == -1, o
        with pytest.raises(psac_amd.PsacxError) as e:        # more strings than characters
            psac_amd.suffix_tree_gsa_device(ctx, g.text, n, g.off, n + 1, g.sa, g.lcp, g.nodes, bits)
        assert e.value.code == -1
    finally:
        g.close()


def test_gsac_tree_cli(tmp_path):
    # gsac -t: the lines of a file -> GSA + LCP -> the table in HBM; the edge count is the model's record count
    gsac = os.path.join(ROOT, "psac_amd", "bin", "gsac")
    strings = G.strings_of("reads")
    f = tmp_path / "reads.txt"
    f.write_bytes(b"\n".join(bytes(x) for x in strings) + b"\n")
    import oracle_lib as O
    ref = O.construct_ss(strings, bits=64)
    R = int(T.records(ref["text"], ref["off"], ref["SA"], ref["LCP"])[2].size)
    r = subprocess.run([gsac, "-f", str(f), "-t", "--check-device"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "[SUCCESS] GSA correct" in r.stdout and "[SUCCESS] Suffix Tree is correct" in r.stdout and "[ERROR]" not in r.stderr
    assert "ST time: " in r.stderr and int(re.search(r"ST edges: (\d+)", r.stderr).group(1)) == R
    plain = subprocess.run([gsac, "-f", str(f), "-t"], capture_output=True, text=True)                  # -t implies -l; no verdict unless asked
    assert plain.returncode == 0 and "Suffix Tree" not in plain.stdout and int(re.search(r"ST edges: (\d+)", plain.stderr).group(1)) == R
    # one GPU only: refused, not gathered
    for extra in (["--gpus", "2"], ["--gpus-on-device", "0,2"]):
        r = subprocess.run([gsac, "-f", str(f), "-t"] + extra, capture_output=True, text=True)
        assert r.returncode != 0 and "one GPU" in r.stderr and "ST edges" not in r.stderr


def test_cpp_mirror_construct_gst(tmp_path):
    # construct_gst(sa, ss) for both index types against a table stated cell by cell, and its refusal on two ranks
    from test_gst_model_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "gst header tests passed" in r.stdout, r.stdout + r.stderr
