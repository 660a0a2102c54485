"""The two GPU checkers against their host model (tests/checker_model.py) over the catalogue of wrong arrays.

psacx_check_dev_* and psacx_multi_check_dev_* are the only verdict on every result too large to compare with the oracle
(bench.py's `verified`, tests/test_gpu_full_size.py, the memory tests of tests/test_gpu_multi.py).  Here the oracle's own
arrays are made wrong on the host in every way of the catalogue, uploaded whole, and each checker must return exactly the
four counters the model predicts -- for both index types, on one GPU and on 1, 2, 3, 4 and 8 ranks, the blocks verified
whole and in pieces (PSACX_MULTI_CHECK_CHUNKS), with wrong entries on the edges of blocks and pieces.  Nothing is
constructed on the GPU, so no construction bug can hide a checker bug.

What runs where (the model predicts any combination of mutants exactly, so most layouts see them several at a time):
  * every class alone at every kind of position: one GPU, 1 rank and 3 ranks in seven pieces, on the tandem repeat (range
    minima across ranks); every class alone once on the other texts (one GPU);
  * every (ranks, pieces, index type): clean arrays of two texts (rotating), then every class in batches whose positions are
    all first / last entries of all blocks and pieces, entries 1 and n - 1, the largest LCP value and three random ones; the
    same batches again without LCP;
  * tiny texts (n around the number of ranks: empty blocks, one-entry blocks, more pieces than entries): every class alone;
  * 3 Mi characters on one rank in 40 pieces (the kept pyramid with running-minimum tables) and one rank whose every fetch
    goes through RCCL.
"""
import ctypes as C

import numpy as np
import pytest

import checker_model as M
from checker_model import BIG, TINY, arrays, truth_of

pytestmark = pytest.mark.gpu

ALONE_TEXT = "tandem"
ALONE_LAYOUTS = [(3, 7), (1, 7)]
CONFIGS = [(P, ch) for P in (1, 2, 3, 4, 8) for ch in (0, 7)] + [(1, 40)]
BATCH = 24


def narrow(a, bits):
    """The 64-bit arrays as the index type under test (all ones stay all ones; every other value fits)."""
    return a if bits == 64 or a.dtype == np.uint8 else a.astype(np.uint32)


class OneGpu(object):
    def __init__(self, n, bits):
        import psac_amd
        self.ctx = psac_amd.Context(0)
        self.n, self.bits = n, bits
        self.d = [self.ctx.alloc(max(n, 1))] + [self.ctx.alloc(n * bits // 8) for _ in range(3)]

    def check(self, arrs, lcp=True):
        import psac_amd
        for p, a in zip(self.d, arrs):
            self.ctx.h2d(p, narrow(a, self.bits))
        return psac_amd.check_device(self.ctx, self.d[0], self.n, self.d[1], self.d[2], self.d[3] if lcp else None, self.bits)

    def close(self):
        for p in self.d:
            self.ctx.free(p)
        self.ctx.close()


class Ranks(object):
    """Device buffers for the blocks of a text of n characters on the ranks of mg."""

    def __init__(self, mg, n, bits):
        self.mg, self.lib, self.n, self.bits = mg, mg._lib, n, bits
        self.offs, self.sizes = M.blocks(n, mg.nranks)
        self.held = []
        self.d = [[self._alloc(r, max(self.sizes[r] * (1 if k == 0 else bits // 8), 1)) for r in range(mg.nranks)] for k in range(4)]

    def _alloc(self, r, nbytes):
        p = C.c_void_p()
        assert self.lib.psacx_dev_alloc(self.mg.rank_ctx(r), C.byref(p), nbytes) == 0
        self.held.append((r, p))
        return p.value

    def check(self, arrs, lcp=True):
        for k, a in enumerate(arrs):
            a = narrow(a, self.bits)
            for r in range(self.mg.nranks):
                blk = np.ascontiguousarray(a[self.offs[r]:self.offs[r] + self.sizes[r]])
                if blk.size:
                    assert self.lib.psacx_copy_h2d(self.mg.rank_ctx(r), C.c_void_p(self.d[k][r]), blk.ctypes.data_as(C.c_void_p), blk.nbytes) == 0
        return self.mg.check_device(self.d[0], self.sizes, self.d[1], self.d[2], self.d[3] if lcp else None, self.bits)

    def close(self):
        for r, p in self.held:
            self.lib.psacx_dev_free(self.mg.rank_ctx(r), p)


def multi(P):
    import psac_amd
    return psac_amd.MultiContext([0] * P)


def set_chunks(monkeypatch, chunks):
    if chunks:
        monkeypatch.setenv("PSACX_MULTI_CHECK_CHUNKS", str(chunks))
    else:
        monkeypatch.delenv("PSACX_MULTI_CHECK_CHUNKS", raising=False)


_expected, _rmq = {}, {}


def case(name, recipe):
    """(arrays, classes applied, model's device counters, model's distributed counters, the same two without LCP) of the
    text `name` after the mutants of `recipe`; the counters are kept, the arrays made again."""
    text, SA, ISA, LCP, tr = arrays(name)
    arrs, done = M.mutate_many(recipe, text, SA, ISA, LCP)
    key = (name, tuple(recipe))
    if key not in _expected:
        if name not in _rmq:
            _rmq[name] = M.RangeMin(LCP)
        lcp_same = all(c not in M.LCP_ONLY for c in done)
        truth = tr if "Text" not in done else truth_of(arrs[0])
        with_lcp = M.expect_both(*arrs, truth=truth, rmq=_rmq[name] if lcp_same else None)
        without = M.expect_both(arrs[0], arrs[1], arrs[2], None)
        per_bits = {64: with_lcp + without}
        if any(c in M.WIDTH_DEPENDENT for c in done):         # all ones is another number in the narrow type: ask the model again
            a32 = [narrow(a, 32) for a in arrs]
            per_bits[32] = M.expect_both(*a32, truth=truth, rmq=None) + M.expect_both(a32[0], a32[1], a32[2], None)
        else:
            per_bits[32] = per_bits[64]
        _expected[key] = per_bits
    return arrs, done, _expected[key]


def alone_recipes(name, layouts, one_per_class=False):
    text, SA, ISA, LCP, tr = arrays(name)
    pos = M.positions(text.size, LCP, layouts)
    where = sorted({w for v in pos.values() for w in v})
    out = []
    for k, cls in enumerate(M.MUTANTS):
        ws = where if cls in M.POSITIONAL else [0]
        if one_per_class:
            ws = [ws[k % len(ws)]]
        out += [[(cls, w)] for w in ws]
    return out


def batch_recipes(name, P, chunks):
    """Every class at least once, every edge of every block and piece of this layout at least once, BATCH mutants at a time
    at positions spread over the whole array; the classes that change everything at once (Lall) in batches of their own."""
    text, SA, ISA, LCP, tr = arrays(name)
    pos = M.positions(text.size, LCP, [(P, max(chunks, 1))], seed=P * 100 + chunks, every_edge=True)
    where = sorted({w for v in pos.values() for w in v})
    while len(where) < len(M.POSITIONAL):                     # few edges: more positions, so that every class has one
        where = sorted(set(where) | {(where[-1] * 7 + 3 * len(where)) % text.size})
    nb = (len(where) + BATCH - 1) // BATCH
    out = []
    for q in range(nb):
        out.append([(M.POSITIONAL[(q + k * nb + P) % len(M.POSITIONAL)], w) for k, w in enumerate(where[q::nb])])
    out[0] += [("Lbase0", 0), ("L0th", 0), ("SIswap_last", 0)]
    out[-1] += [("Lbase2", 0)]
    return out + [[("Lall1", 0)], [("Lall2", 0)]]


def compare(bad, got, want, what):
    if got != want:
        bad.append("%s: checker %s, model %s" % (what, got, want))


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_one_gpu_checker_every_class_alone_at_every_kind_of_position(bits):
    bad, classes = [], set()
    for name in BIG:
        text = arrays(name)[0]
        g = OneGpu(text.size, bits)
        try:
            assert g.check(arrays(name)[:4]) == [0, 0, 0, 0] and g.check(arrays(name)[:4], lcp=False) == [0, 0, 0, 0]
            for recipe in alone_recipes(name, ALONE_LAYOUTS, one_per_class=name != ALONE_TEXT):
                arrs, done, want = case(name, recipe)
                if not done:
                    continue
                classes.add(done[0])
                assert sum(want[bits][0]) > 0
                compare(bad, g.check(arrs), want[bits][0], "%s %s" % (name, recipe))
                if done[0] not in M.LCP_ONLY:
                    compare(bad, g.check(arrs, lcp=False), want[bits][2], "%s %s without LCP" % (name, recipe))
        finally:
            g.close()
    assert classes == set(M.MUTANTS)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("P", [1, 3])
def test_distributed_checker_every_class_alone_at_every_kind_of_position(P, bits, monkeypatch):
    set_chunks(monkeypatch, 7)
    bad, classes = [], set()
    mg = multi(P)
    try:
        text = arrays(ALONE_TEXT)[0]
        g = Ranks(mg, text.size, bits)
        assert g.check(arrays(ALONE_TEXT)[:4]) == [0, 0, 0, 0] and g.check(arrays(ALONE_TEXT)[:4], lcp=False) == [0, 0, 0, 0]
        for recipe in alone_recipes(ALONE_TEXT, ALONE_LAYOUTS):
            arrs, done, want = case(ALONE_TEXT, recipe)
            if not done:
                continue
            classes.add(done[0])
            assert sum(want[bits][1]) > 0
            compare(bad, g.check(arrs), want[bits][1], str(recipe))
            if done[0] not in M.LCP_ONLY:
                compare(bad, g.check(arrs, lcp=False), want[bits][3], "%s without LCP" % recipe)
        g.close()
    finally:
        mg.close()
    assert classes == set(M.MUTANTS)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("P,chunks", CONFIGS)
def test_distributed_checker_every_layout_sees_every_class(P, chunks, bits, monkeypatch):
    set_chunks(monkeypatch, chunks)
    k = CONFIGS.index((P, chunks))
    bad, classes = [], set()
    mg = multi(P)
    try:
        for name in (BIG[k % 4], BIG[(k + 1) % 4]):
            text = arrays(name)[0]
            g = Ranks(mg, text.size, bits)
            assert g.check(arrays(name)[:4]) == [0, 0, 0, 0] and g.check(arrays(name)[:4], lcp=False) == [0, 0, 0, 0]
            for recipe in batch_recipes(name, P, chunks):
                arrs, done, want = case(name, recipe)
                classes.update(done)
                assert sum(want[bits][1]) > 0
                compare(bad, g.check(arrs), want[bits][1], "%s %s" % (name, recipe))
                if any(c not in M.LCP_ONLY for c in done):
                    compare(bad, g.check(arrs, lcp=False), want[bits][3], "%s %s without LCP" % (name, recipe))
            g.close()
    finally:
        mg.close()
    assert classes == set(M.MUTANTS)
    assert not bad, "\n".join(bad)


TINY_LAYOUTS = [(1, 0), (1, 40), (2, 7), (3, 0), (4, 7), (8, 0), (8, 7), (3, 40)]


@pytest.mark.parametrize("bits", [32, 64])
def test_tiny_texts_empty_blocks_and_empty_pieces(bits, monkeypatch):
    # n in {1, 2, 3, P - 1, P, P + 1, 2 P + 1} for 8 ranks: blocks of no or one entry, 40 pieces of a block of two; every
    # class alone at entries 0, 1, the middle and the last.  Every mutant goes to the one-GPU checker and to one of the
    # layouts, which take turns (three of the eight have 8 ranks); every layout must have met every class in the end.
    bad, seen = [], set()
    ctxs = {P: multi(P) for P in sorted({P for P, _ in TINY_LAYOUTS})}
    try:
        turn = {}
        for n in TINY:
            name = "tiny%d" % n
            text, SA, ISA, LCP, tr = arrays(name)
            one = OneGpu(n, bits)
            ranks = {P: Ranks(mg, n, bits) for P, mg in ctxs.items()}
            assert one.check((text, SA, ISA, LCP)) == [0, 0, 0, 0]
            for P, chunks in TINY_LAYOUTS:
                set_chunks(monkeypatch, chunks)
                assert ranks[P].check((text, SA, ISA, LCP)) == [0, 0, 0, 0], (n, P, chunks)
                assert ranks[P].check((text, SA, ISA, LCP), lcp=False) == [0, 0, 0, 0], (n, P, chunks)
            for cls in M.MUTANTS:
                for w in (sorted({0, min(1, n - 1), n // 2, n - 1}) if cls in M.POSITIONAL else [0]):
                    arrs, done, want = case(name, [(cls, w)])
                    if not done:
                        continue
                    compare(bad, one.check(arrs), want[bits][0], "one GPU n=%d %s at %d" % (n, cls, w))
                    turn[cls] = turn.get(cls, list(M.MUTANTS).index(cls)) + 1
                    for k in ([turn[cls]] if cls in M.POSITIONAL else [turn[cls], turn[cls] + 4]):          # (the classes without a position come once per text)
                        P, chunks = TINY_LAYOUTS[k % len(TINY_LAYOUTS)]
                        seen.add((P, chunks, cls))
                        set_chunks(monkeypatch, chunks)
                        compare(bad, ranks[P].check(arrs), want[bits][1], "n=%d %s at %d, %d ranks, %d pieces" % (n, cls, w, P, chunks))
                        if cls not in M.LCP_ONLY:
                            compare(bad, ranks[P].check(arrs, lcp=False), want[bits][3], "n=%d %s at %d, %d ranks, %d pieces, without LCP" % (n, cls, w, P, chunks))
            one.close()
            for r in ranks.values():
                r.close()
    finally:
        for mg in ctxs.values():
            mg.close()
    unmet = [(P, chunks, cls) for P, chunks in TINY_LAYOUTS for cls in M.MUTANTS if (P, chunks, cls) not in seen]
    assert not unmet, unmet
    assert not bad, "\n".join(bad)


def test_one_rank_in_40_pieces_of_a_large_text(monkeypatch):
    # 3 Mi characters in 40 pieces: every piece asks 78643 range minima (>= 2^16, fewer than m / 32), which go to the kept
    # pyramid of four levels with the running-minimum tables of its middle levels beside it
    import inputs
    import oracle_lib as O
    set_chunks(monkeypatch, 40)
    text = inputs.dna(3 << 20, 9)
    ref = O.construct(text, bits=32)
    SA, ISA, LCP = ref["SA"], ref["ISA"], ref["LCP"]
    n = text.size
    pos = M.positions(n, LCP, [(1, 40)], seed=3, every_edge=True)
    where = sorted({w for v in pos.values() for w in v})
    classes = ["L+", "L-", "SIswap_eq", "SIswap_diff"]
    recipes = [[(classes[k % 4], w) for k, w in enumerate(where)] + [("SIswap_last", 0)], [("Lall1", 0)], [("Lall2", 0)]]
    bad = []
    mg = multi(1)
    try:
        for bits in (32, 64):
            g = Ranks(mg, n, bits)
            wide = lambda arrs: [a if bits == 32 or a.dtype == np.uint8 else a.astype(np.uint64) for a in arrs]
            assert g.check(wide((text, SA, ISA, LCP))) == [0, 0, 0, 0]
            for recipe in recipes:
                arrs, done = M.mutate_many(recipe, text, SA, ISA, LCP)
                key = ("large", tuple(recipe))
                if key not in _expected:
                    _expected[key] = M.expect_multi(*arrs)
                assert sum(_expected[key]) > 0 and len(done) == len(recipe)
                compare(bad, g.check(wide(arrs)), _expected[key], "%d bits %s" % (bits, recipe[:4]))
            g.close()
    finally:
        mg.close()
    assert not bad, "\n".join(bad)


def test_one_rank_whose_every_fetch_goes_through_rccl():
    import psac_amd
    mg = psac_amd.MultiContext.for_rank(0, 1, 0, psac_amd.unique_id(), force_wire=True)
    bad, classes = [], set()
    try:
        assert mg.nranks == 1
        text = arrays(ALONE_TEXT)[0]
        for bits in (32, 64):
            g = Ranks(mg, text.size, bits)
            assert g.check(arrays(ALONE_TEXT)[:4]) == [0, 0, 0, 0]
            for recipe in alone_recipes(ALONE_TEXT, ALONE_LAYOUTS, one_per_class=True):
                arrs, done, want = case(ALONE_TEXT, recipe)
                classes.update(done)
                compare(bad, g.check(arrs), want[bits][1], "%d bits %s" % (bits, recipe))
            g.close()
    finally:
        mg.close()
    assert classes == set(M.MUTANTS)
    assert not bad, "\n".join(bad)
