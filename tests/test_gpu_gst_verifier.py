"""psacx_check_suffix_tree_gsa_dev_* against its host model (tests/gst_model.py).

Nothing is constructed on the GPU: the oracle's SA / LCP and the model's table are made wrong on the host in every way of the
model's catalogues and uploaded, and the checker must return exactly the four counters the model predicts, for both index
types.  Table mutants come in batches (the model predicts any combination): class k + j at position j in batch k, so as many
batches as there are classes put every class at every position -- rows 0, 1, n - 1, the group and level edges 63 / 64 / 65 and
4095 / 4096 / 4097, the deepest node and three random rows; each test asserts that every class of its catalogue applied.  Input mutants -- SA, LCP, the text or an offset damaged, the table
clean -- come one at a time; every call must return, whatever the arrays hold (Sones, Lones: all ones are never an index).
"""
import numpy as np
import pytest

import gst_model as T

pytestmark = pytest.mark.gpu

SETS = ["tiny17", "edge65", "edge4097", "word_edges", "copies", "prefixes", "unary", "tandem_pieces", "bytes256"]
# the classes a set cannot carry: no index of bytes256 shares its interval with a head that has a record; unary has one letter
NOT_ON = {"bytes256": {"non_head"}, "unary": {"Text"}}
INPUT_SETS = ["tiny17", "edge65", "edge4097", "word_edges", "copies", "unary", "bytes256"]


class Dev(object):
    """Text, offsets, SA, LCP and the table of one set in HBM, as the index type under test."""

    def __init__(self, text, off, cells, bits):
        import psac_amd
        self.ctx = psac_amd.Context(0)
        self.n, self.m, self.bits, self.dt = int(text.size), int(off.size - 1), bits, np.uint32 if bits == 32 else np.uint64
        w = bits // 8
        self.d = {"text": self.ctx.alloc(self.n), "off": self.ctx.alloc(off.size * 8), "SA": self.ctx.alloc(self.n * w),
                  "LCP": self.ctx.alloc(self.n * w), "nodes": self.ctx.alloc(cells * 8)}

    def put(self, **arrs):
        for k, a in arrs.items():
            if k in ("SA", "LCP"):
                a = a.astype(self.dt)               # (all ones stay all ones: the mutants were made for this width)
            self.ctx.h2d(self.d[k], a)

    def check(self):
        import psac_amd
        d = self.d
        return psac_amd.check_suffix_tree_gsa_device(self.ctx, d["text"], self.n, d["off"], self.m, d["SA"], d["LCP"], d["nodes"], self.bits)

    def close(self):
        for p in self.d.values():
            self.ctx.free(p)
        self.ctx.close()


def table_recipes(name):
    text, off, SA, LCP, recs, table = T.arrays(name)
    pos = T.table_positions(text.size, LCP)
    cls = list(T.TABLE_MUTANTS)
    return [[(cls[(k + j) % len(cls)], w) for j, w in enumerate(pos)] for k in range(len(cls))]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", SETS)
def test_clean_arrays_and_wrong_tables(name, bits):
    text, off, SA, LCP, recs, table = T.arrays(name)
    R, cells = int(recs[2].size), int(np.count_nonzero(table))
    bad, applied = [], set()
    g = Dev(text, off, table.size, bits)
    try:
        g.put(text=text, off=off, SA=SA, LCP=LCP, nodes=table)
        assert g.check() == [0, 0, R, cells]
        for k, recipe in enumerate(table_recipes(name)):
            wrong, done = T.mutate_table(recipe, table, T.head_of(name), recs)
            if not done:
                continue
            applied.update(done)
            want = T.expect(text, off, SA, LCP, wrong, recs)
            assert want[0] + want[1] > 0 and want[2] == R
            g.put(nodes=wrong)
            got = g.check()
            if got != want:
                bad.append("%s batch %d %s: checker %s, model %s" % (name, k, done, got, want))
    finally:
        g.close()
    assert applied == set(T.TABLE_MUTANTS) - NOT_ON.get(name, set())         # (no class hides by never applying)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", INPUT_SETS)
def test_wrong_inputs_one_at_a_time(name, bits):
    text, off, SA, LCP, recs, table = T.arrays(name)
    R, cells = int(recs[2].size), int(np.count_nonzero(table))
    pos = T.table_positions(text.size, LCP)
    bad, caught, applied = [], set(), set()
    g = Dev(text, off, table.size, bits)
    try:
        g.put(text=text, off=off, SA=SA, LCP=LCP, nodes=table)
        for cls in T.ALL_INPUT_MUTANTS:
            for w in (pos if cls != "L0th" else [0]):
                arrs = T.mutate_inputs(cls, w, text, off, SA, LCP, bits)
                if arrs is None:
                    continue
                applied.add(cls)
                want = T.expect(arrs[0], arrs[1], arrs[2], arrs[3], table)
                if want[0] + want[1] > 0:
                    caught.add(cls)
                g.put(text=arrs[0], off=arrs[1], SA=arrs[2], LCP=arrs[3])
                got = g.check()
                if got != want:
                    bad.append("%s %s at %d: checker %s, model %s" % (name, cls, w, got, want))
                if cls == "L0th":
                    assert want == [0, 0, R, cells]          # the stored LCP[0] is never used as a value
        g.put(text=text, off=off, SA=SA, LCP=LCP)
        assert g.check() == [0, 0, R, cells]
    finally:
        g.close()
    assert applied == set(T.ALL_INPUT_MUTANTS) - NOT_ON.get(name, set())     # (no class hides by never applying)
    if text.size >= 11:
        assert caught >= {"L+", "Lones", "Sones", "Sn"}
    assert not bad, "\n".join(bad)
