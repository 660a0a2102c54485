"""psacx_check_suffix_tree_dev_* against its host model (tests/st_checker_model.py).

Nothing is constructed on the GPU: the oracle's SA / LCP and the model's table are made wrong on the host in every way of
the model's two catalogues and uploaded, and the checker must return exactly the four counters the model predicts, for both
index types.  Table mutants come in batches (the model predicts any combination): class k + j at position j in batch k, so
ten batches put every class at every position -- rows 0, 1, n - 1, the group and level edges 63 / 64 / 65 and
4095 / 4096 / 4097, the deepest node and three random rows; the two large texts take two and three batches.  Input mutants
come one at a time on the texts of at most 37 000 characters, plus two on the 300 000-character text.

What the texts are for.  "Farthest parent" is st_checker_model.farthest_parent: max |i - row| over all records, i the LCP
index a record belongs to and row the node it hangs under; tests/test_st_checker_model_cpu.py asserts these figures.
  edge<n>      n = 1, 2, 3, 63, 64, 65, 4095, 4096, 4097 over two letters: ends of the 64-entry groups and pyramid levels
  dna          300 000 characters, more than 64^3 entries, so three levels above the array; farthest parent 243 572 entries away
  unary        L[i] = i: every index is a node and no index has a smaller value to its right; largest LCP 4 999
  tandem       period 37 x 1000: farthest parent 24 000 entries away, largest LCP 36 963
  hub          0, 1 + x, 1 + y for x, y < 200: plateaus of equal LCP (largest LCP 2), farthest parent 119 601 entries away,
               reached through equal values; row of 202 cells
  perm256      all 256 bytes once: row of 257 cells, LCP all zero, the root has 256 children
"""
import numpy as np
import pytest

import st_checker_model as S

pytestmark = pytest.mark.gpu

BATCHES = {"dna": [0, 3, 7], "hub": [0, 5]}


class Dev(object):
    """Text, SA, LCP and the table of one text in HBM, as the index type under test."""

    def __init__(self, text, row, bits):
        import psac_amd
        self.ctx = psac_amd.Context(0)
        self.n, self.bits, self.dt = int(text.size), bits, np.uint32 if bits == 32 else np.uint64
        w = bits // 8
        self.d = {"text": self.ctx.alloc(self.n), "SA": self.ctx.alloc(self.n * w), "LCP": self.ctx.alloc(self.n * w),
                  "nodes": self.ctx.alloc(self.n * row * 8)}

    def put(self, **arrs):
        for k, a in arrs.items():
            if k in ("SA", "LCP"):
                a = a.astype(self.dt)               # (all ones stay all ones: the mutants were made for this width)
            self.ctx.h2d(self.d[k], a)

    def check(self):
        import psac_amd
        return psac_amd.check_suffix_tree_device(self.ctx, self.d["text"], self.n, self.d["SA"], self.d["LCP"], self.d["nodes"], self.bits)

    def close(self):
        for p in self.d.values():
            self.ctx.free(p)
        self.ctx.close()


def table_recipes(name):
    text, SA, LCP, recs, table = S.arrays(name)
    pos = S.table_positions(text.size, LCP)
    cls = list(S.TABLE_MUTANTS)
    return [[(cls[(k + j) % len(cls)], w) for j, w in enumerate(pos)] for k in BATCHES.get(name, range(len(cls)))]


_tables = {}


def table_case(name, k, recipe):
    """(wrong table, classes applied, model's counters) of batch k; the counters are kept, the table made again."""
    text, SA, LCP, recs, table = S.arrays(name)
    bad, done = S.mutate_table(recipe, table, S.head_of(name), recs)
    if (name, k) not in _tables:
        _tables[(name, k)] = S.expect(text, SA, LCP, bad, recs)
    return bad, done, _tables[(name, k)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", S.ALL)
def test_clean_arrays_and_wrong_tables(name, bits):
    text, SA, LCP, recs, table = S.arrays(name)
    R = int(recs[2].size)
    bad, classes = [], set()
    g = Dev(text, table.shape[1], bits)
    try:
        g.put(text=text, SA=SA, LCP=LCP, nodes=table)
        assert g.check() == [0, 0, R, R]
        for k, recipe in enumerate(table_recipes(name)):
            wrong, done, want = table_case(name, k, recipe)
            if not done:
                continue
            classes.update(done)
            assert want[0] + want[1] > 0 and want[2] == R
            g.put(nodes=wrong)
            got = g.check()
            if got != want:
                bad.append("%s batch %d %s: checker %s, model %s" % (name, k, done, got, want))
    finally:
        g.close()
    if text.size >= 11 and name != "perm256":                # (one letter or no internal node: some classes have nothing to change)
        assert classes >= set(S.TABLE_MUTANTS) - ({"move_in_row", "non_head"} if name == "unary" else set())
    assert not bad, "\n".join(bad)


_inputs = {}


def input_case(name, cls, w, bits):
    text, SA, LCP, recs, table = S.arrays(name)
    arrs = S.mutate_inputs(cls, w, text, SA, LCP, bits)
    if arrs is None:
        return None, None
    key = (name, cls, w, bits if cls in ("Lones", "Sones") else 0)          # the all-ones values are asked of the model per index type
    if key not in _inputs:
        _inputs[key] = S.expect(arrs[0], arrs[1], arrs[2], table)
    return arrs, _inputs[key]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", S.SMALL + ["dna"])
def test_wrong_inputs_one_at_a_time(name, bits):
    text, SA, LCP, recs, table = S.arrays(name)
    R = int(recs[2].size)
    pos = S.table_positions(text.size, LCP)
    todo = [(cls, w) for cls in S.INPUT_MUTANTS for w in (pos if cls != "L0th" else [0])]
    if name == "dna":
        todo = [("L+", pos[len(pos) // 2]), ("Sswap", pos[-2])]
    bad, caught = [], set()
    g = Dev(text, table.shape[1], bits)
    try:
        g.put(text=text, SA=SA, LCP=LCP, nodes=table)
        for cls, w in todo:
            arrs, want = input_case(name, cls, w, bits)
            if arrs is None:
                continue
            if want[0] + want[1] > 0:
                caught.add(cls)
            g.put(**{"Text": {"text": arrs[0]}, "S": {"SA": arrs[1]}, "L": {"LCP": arrs[2]}}["Text" if cls == "Text" else cls[0]])
            got = g.check()
            if got != want:
                bad.append("%s %s at %d: checker %s, model %s" % (name, cls, w, got, want))
            if cls == "L0th":
                assert want == [0, 0, R, R]          # the stored LCP[0] is never used as a value
            g.put(**{"Text": {"text": text}, "S": {"SA": SA}, "L": {"LCP": LCP}}["Text" if cls == "Text" else cls[0]])
        assert g.check() == [0, 0, R, R]
    finally:
        g.close()
    if text.size >= 11 and name != "dna":
        assert caught >= {"L+", "Lones", "Sones", "Sn"}
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["edge65", "mississippi", "perm256", "edge4097"])
def test_table_at_an_address_that_is_no_multiple_of_16(name, bits):
    # the pass that counts the nonzero cells reads 16 bytes at a time only where the table is aligned for it: here the table starts
    # 8 bytes into an allocation (rows of 3, 5, 257 and 3 cells; edge4097 has more cells than the grid has threads per step)
    import psac_amd
    text, SA, LCP, recs, table = S.arrays(name)
    R = int(recs[2].size)
    g = Dev(text, table.shape[1] + 1, bits)                  # (room for the 8 bytes in front)
    try:
        g.put(text=text, SA=SA, LCP=LCP)
        off = g.d["nodes"] + 8
        check = lambda: psac_amd.check_suffix_tree_device(g.ctx, g.d["text"], g.n, g.d["SA"], g.d["LCP"], off, bits)
        g.ctx.h2d(off, table)
        assert check() == [0, 0, R, R]
        for k, recipe in enumerate(table_recipes(name)[:3]):
            wrong, done, want = table_case(name, k, recipe)
            g.ctx.h2d(off, wrong)
            assert check() == want, (k, done)
    finally:
        g.close()
