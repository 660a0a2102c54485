"""The two GPU checkers for generalized suffix arrays against their host model (tests/gsa_checker_model.py).

psacx_check_gsa_dev_* and psacx_multi_check_gsa_dev_* are the only verdict on a generalized suffix array too large to
compare with the oracle.  As tests/test_gpu_verifiers.py does for the plain pair, the oracle's own arrays of string sets
are made wrong on the host -- in every way of the plain catalogue and in the ways only a string set can be wrong (equal
suffixes of two strings swapped, an LCP value or an order taken from the concatenated text, the offsets moved by one, the
LCP of a one-character suffix replaced) -- and uploaded, and each checker must return exactly the model's four counters:
both index types, one GPU and 1, 2, 3, 4 and 8 ranks sharing device 0, the blocks whole and in 7 pieces, wrong entries on
the edges of blocks and pieces, with and without LCP, clean arrays first.  Nothing is constructed on the GPU.

What runs where:
  * every class alone at every kind of position (entries 1 and n - 1, first / last of a block and of a piece, the largest LCP
    value): one GPU, 1 rank and 3 ranks in seven pieces, on the tandem repeat cut into uneven pieces (range minima across
    ranks); every class alone once on the other sets (one GPU) and on the single string (1 and 3 ranks);
  * every (ranks, pieces, index type): clean arrays of two sets (rotating), then every class in batches at all first / last
    entries of all blocks and pieces, entries 1 and n - 1, the largest LCP value and three random ones; again without LCP;
  * tiny sets (n around the number of ranks): every class alone, one GPU and the layouts in turn;
  * malformed offsets: PSACX_EINVAL from both.
"""
import ctypes as C

import numpy as np
import pytest

import gsa_checker_model as G
from gsa_checker_model import BIG, TINY, arrays

pytestmark = pytest.mark.gpu

ALONE_SET = "tandem_pieces"
ALONE_LAYOUTS = [(3, 7)]
CONFIGS = [(P, ch) for P in (1, 2, 3, 4, 8) for ch in (0, 7)]
BATCH = 24
SETS = [s for s in BIG if s != "single"] + ["single"]       # (the rotation below starts at the sets with many strings)


def narrow(a, bits):
    return a if bits == 64 or a.dtype == np.uint8 else a.astype(np.uint32)


class OneGpu(object):
    def __init__(self, n, m_max, bits):
        import psac_amd
        self.ctx = psac_amd.Context(0)
        self.n, self.bits = n, bits
        self.d = [self.ctx.alloc(max(n, 1))] + [self.ctx.alloc(n * bits // 8) for _ in range(3)]
        self.d_off = self.ctx.alloc((m_max + 1) * 8)

    def _upload(self, arrs):
        text, off, SA, ISA, LCP = arrs
        for p, a in zip(self.d, (text, SA, ISA, LCP)):
            self.ctx.h2d(p, narrow(a, self.bits))
        off = np.ascontiguousarray(off, np.uint64)
        self.ctx.h2d(self.d_off, off)
        return off.size - 1

    def call(self, arrs):
        """(return code, counters) of the C entry point for (text, offsets, SA, ISA, LCP)"""
        m = self._upload(arrs)
        err = (C.c_uint64 * 4)()
        fn = getattr(self.ctx._lib, "psacx_check_gsa_dev_u%d" % self.bits)
        rc = fn(self.ctx.handle, C.c_void_p(self.d[0]), self.n, C.c_void_p(self.d_off), m, C.c_void_p(self.d[1]), C.c_void_p(self.d[2]), C.c_void_p(self.d[3]), err)
        return rc, list(err)

    def check(self, arrs, lcp=True):
        import psac_amd
        m = self._upload(arrs)
        return psac_amd.check_gsa_device(self.ctx, self.d[0], self.n, self.d_off, m, self.d[1], self.d[2], self.d[3] if lcp else None, self.bits)

    def close(self):
        for p in self.d + [self.d_off]:
            self.ctx.free(p)
        self.ctx.close()


class Ranks(object):
    """Device buffers for the blocks of a text of n characters on the ranks of mg."""

    def __init__(self, mg, n, bits):
        self.mg, self.lib, self.n, self.bits = mg, mg._lib, n, bits
        self.offs, self.sizes = G.blocks(n, mg.nranks)
        self.held = []
        self.d = [[self._alloc(r, max(self.sizes[r] * (1 if k == 0 else bits // 8), 1)) for r in range(mg.nranks)] for k in range(4)]

    def _alloc(self, r, nbytes):
        p = C.c_void_p()
        assert self.lib.psacx_dev_alloc(self.mg.rank_ctx(r), C.byref(p), nbytes) == 0
        self.held.append((r, p))
        return p.value

    def check(self, arrs, lcp=True):
        text, off, SA, ISA, LCP = arrs
        for k, a in enumerate((text, SA, ISA, LCP)):
            a = narrow(a, self.bits)
            for r in range(self.mg.nranks):
                blk = np.ascontiguousarray(a[self.offs[r]:self.offs[r] + self.sizes[r]])
                if blk.size:
                    assert self.lib.psacx_copy_h2d(self.mg.rank_ctx(r), C.c_void_p(self.d[k][r]), blk.ctypes.data_as(C.c_void_p), blk.nbytes) == 0
        return self.mg.check_gsa_device(self.d[0], self.sizes, off, self.d[1], self.d[2], self.d[3] if lcp else None, self.bits)

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


def clean(name):
    return arrays(name)[:5]


def case(name, recipe):
    """(arrays, classes applied, {bits: [device, distributed, device without LCP, distributed without LCP]}) of the set
    `name` after the mutants of `recipe`; the counters are kept, the arrays made again."""
    text, off, SA, ISA, LCP, tr = arrays(name)
    arrs, done = G.mutate_many_gsa(recipe, text, off, SA, ISA, LCP)
    key = (name, tuple(recipe))
    if key not in _expected:
        if name not in _rmq:
            _rmq[name] = G.RangeMin(LCP)
        lcp_same = all(c not in G.LCP_ONLY for c in done)
        truth = tr if "Text" not in done and not any(c in G.MOVES_OFFSETS for c in done) else G.gsa_truth_of(arrs[0], arrs[1])
        with_lcp = G.expect_gsa_both(*arrs, truth=truth, rmq=_rmq[name] if lcp_same else None)
        without = G.expect_gsa_both(arrs[0], arrs[1], arrs[2], arrs[3], None)
        per_bits = {64: list(with_lcp) + list(without)}
        if any(c in G.M.WIDTH_DEPENDENT for c in done):      # all ones is another number in the narrow type: ask the model again
            a32 = [arrs[0], arrs[1]] + [narrow(a, 32) for a in arrs[2:]]
            per_bits[32] = list(G.expect_gsa_both(*a32, truth=truth)) + list(G.expect_gsa_both(a32[0], a32[1], a32[2], a32[3], None))
        else:
            per_bits[32] = per_bits[64]
        _expected[key] = per_bits
    return arrs, done, _expected[key]


def must_object(done):
    return any(c not in G.MAY_PASS for c in done)


def alone_recipes(name, layouts, one_per_class=False):
    text, off, SA, ISA, LCP, tr = arrays(name)
    pos = G.positions(text.size, LCP, layouts)
    where = sorted({w for kind, v in pos.items() if kind != "random" for w in v})        # (the batches bring random entries)
    out = []
    for k, cls in enumerate(G.ALL):
        ws = where if cls in G.POSITIONAL else [0]
        if one_per_class:
            ws = [ws[k % len(ws)]]
        out += [[(cls, w)] for w in ws]
    return out


def batch_recipes(name, P, chunks):
    """Every class at least once, every edge of every block and piece of this layout at least once, BATCH mutants at a time;
    the classes that change everything at once (Lall) and the moved offsets in batches of their own."""
    text, off, SA, ISA, LCP, tr = arrays(name)
    pos = G.positions(text.size, LCP, [(P, max(chunks, 1))], seed=P * 100 + chunks, every_edge=True)
    where = sorted({w for v in pos.values() for w in v})
    classes = [c for c in G.POSITIONAL if c not in G.MOVES_OFFSETS]
    while len(where) < len(classes):
        where = sorted(set(where) | {(where[-1] * 7 + 3 * len(where)) % text.size})
    nb = (len(where) + BATCH - 1) // BATCH
    out = []
    for q in range(nb):
        out.append([(classes[(q + k * nb + P) % len(classes)], w) for k, w in enumerate(where[q::nb])])
    out[0] += [("Lbase0", 0), ("L0th", 0), ("SIswap_last", 0)]
    out[-1] += [("Lbase2", 0)]
    return out + [[("Lall1", 0)], [("Lall2", 0)], [("Goff+1", where[len(where) // 2])], [("Goff-1", where[len(where) // 3])]]


def compare(bad, got, want, what):
    if got != want:
        bad.append("%s: checker %s, model %s" % (what, got, want))


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_one_gpu_checker_every_class_alone_at_every_kind_of_position(bits):
    bad, classes = [], set()
    for name in BIG:
        text, off = arrays(name)[:2]
        g = OneGpu(text.size, off.size - 1, bits)
        try:
            assert g.check(clean(name)) == [0, 0, 0, 0] and g.check(clean(name), lcp=False) == [0, 0, 0, 0]
            for recipe in alone_recipes(name, ALONE_LAYOUTS, one_per_class=name != ALONE_SET):
                arrs, done, want = case(name, recipe)
                if not done:
                    continue
                classes.add(done[0])
                assert sum(want[bits][0]) > 0 or not must_object(done)
                compare(bad, g.check(arrs), want[bits][0], "%s %s" % (name, recipe))
                if done[0] not in G.LCP_ONLY:
                    compare(bad, g.check(arrs, lcp=False), want[bits][2], "%s %s without LCP" % (name, recipe))
        finally:
            g.close()
    assert classes == set(G.ALL)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("P", [1, 3])
def test_distributed_checker_every_class_alone_at_every_kind_of_position(P, bits, monkeypatch):
    set_chunks(monkeypatch, 7)
    bad, classes = [], set()
    mg = multi(P)
    try:
        for name, one in ((ALONE_SET, False), ("single", True)):          # (one string: the classes of the plain catalogue)
            g = Ranks(mg, arrays(name)[0].size, bits)
            assert g.check(clean(name)) == [0, 0, 0, 0] and g.check(clean(name), lcp=False) == [0, 0, 0, 0]
            for recipe in alone_recipes(name, ALONE_LAYOUTS, one_per_class=one):
                arrs, done, want = case(name, recipe)
                if not done:
                    continue
                classes.add(done[0])
                assert sum(want[bits][1]) > 0 or not must_object(done)
                compare(bad, g.check(arrs), want[bits][1], "%s %s" % (name, recipe))
                if done[0] not in G.LCP_ONLY:
                    compare(bad, g.check(arrs, lcp=False), want[bits][3], "%s %s without LCP" % (name, recipe))
            g.close()
    finally:
        mg.close()
    assert classes == set(G.ALL)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("P,chunks", CONFIGS)
def test_distributed_checker_every_layout_sees_every_class(P, chunks, bits, monkeypatch):
    set_chunks(monkeypatch, chunks)
    k = CONFIGS.index((P, chunks))
    bad, classes = [], set()
    mg = multi(P)
    try:
        for name in (SETS[k % 5], SETS[(k + 1) % 5]):         # two of the five sets with several strings, in turn
            g = Ranks(mg, arrays(name)[0].size, bits)
            assert g.check(clean(name)) == [0, 0, 0, 0] and g.check(clean(name), lcp=False) == [0, 0, 0, 0]
            for recipe in batch_recipes(name, P, chunks):
                arrs, done, want = case(name, recipe)
                if not done:
                    continue
                classes.update(done)
                assert sum(want[bits][1]) > 0 or not must_object(done)
                compare(bad, g.check(arrs), want[bits][1], "%s %s" % (name, recipe))
                if any(c not in G.LCP_ONLY for c in done):
                    compare(bad, g.check(arrs, lcp=False), want[bits][3], "%s %s without LCP" % (name, recipe))
            g.close()
    finally:
        mg.close()
    assert classes == set(G.ALL), sorted(set(G.ALL) - classes)      # (what a unary set cannot show, its partner does)
    assert not bad, "\n".join(bad)


TINY_LAYOUTS = [(1, 0), (2, 7), (3, 0), (4, 7), (8, 0), (8, 7)]


@pytest.mark.parametrize("bits", [32, 64])
def test_tiny_sets_empty_blocks_and_empty_pieces(bits, monkeypatch):
    bad, seen = [], set()
    ctxs = {P: multi(P) for P in sorted({P for P, _ in TINY_LAYOUTS})}
    try:
        turn = {}
        for n in TINY:
            name = "tiny%d" % n
            text, off = arrays(name)[:2]
            one = OneGpu(n, off.size - 1, bits)
            ranks = {P: Ranks(mg, n, bits) for P, mg in ctxs.items()}
            assert one.check(clean(name)) == [0, 0, 0, 0]
            for P, chunks in TINY_LAYOUTS:
                set_chunks(monkeypatch, chunks)
                assert ranks[P].check(clean(name)) == [0, 0, 0, 0], (n, P, chunks)
                assert ranks[P].check(clean(name), lcp=False) == [0, 0, 0, 0], (n, P, chunks)
            for cls in G.ALL:
                for w in (sorted({0, n // 2, n - 1}) if cls in G.POSITIONAL else [0]):
                    arrs, done, want = case(name, [(cls, w)])
                    if not done:
                        continue
                    compare(bad, one.check(arrs), want[bits][0], "one GPU n=%d %s at %d" % (n, cls, w))
                    turn[cls] = turn.get(cls, G.ALL.index(cls)) + 1
                    P, chunks = TINY_LAYOUTS[turn[cls] % len(TINY_LAYOUTS)]
                    seen.add(cls)
                    set_chunks(monkeypatch, chunks)
                    compare(bad, ranks[P].check(arrs), want[bits][1], "n=%d %s at %d, %d ranks, %d pieces" % (n, cls, w, P, chunks))
                    if cls not in G.LCP_ONLY:
                        compare(bad, ranks[P].check(arrs, lcp=False), want[bits][3], "n=%d %s at %d, %d ranks, %d pieces, without LCP" % (n, cls, w, P, chunks))
            one.close()
            for r in ranks.values():
                r.close()
    finally:
        for mg in ctxs.values():
            mg.close()
    assert seen == set(G.ALL), sorted(set(G.ALL) - seen)
    assert not bad, "\n".join(bad)


def test_malformed_offsets_are_refused_by_both_checkers():
    from psac_amd import PsacxError
    text, off, SA, ISA, LCP = clean("reads")
    n, m = text.size, off.size - 1
    bad1 = off.copy(); bad1[0] = 1                           # does not start at 0
    bad2 = off.copy(); bad2[-1] = n - 1                      # does not end at n
    bad3 = off.copy(); bad3[2] = bad3[1]                     # an empty string
    bad4 = off.copy(); bad4[2], bad4[3] = off[3], off[2]     # not ascending
    bad5 = off.copy(); bad5[m // 2] = n + 5                  # past the end (would be a store outside the bitmap)
    mg = multi(2)
    try:
        for bits in (32, 64):
            one = OneGpu(n, m, bits)
            ranks = Ranks(mg, n, bits)
            assert one.call((text, off, SA, ISA, LCP)) == (0, [0, 0, 0, 0])
            for bad in (bad1, bad2, bad3, bad4, bad5):
                assert one.call((text, bad, SA, ISA, LCP))[0] == -1
                with pytest.raises(PsacxError) as e:
                    ranks.check((text, bad, SA, ISA, LCP))
                assert e.value.code == -1
            assert ranks.check((text, off, SA, ISA, LCP)) == [0, 0, 0, 0]       # and both still work afterwards
            assert one.check((text, off, SA, ISA, LCP)) == [0, 0, 0, 0]
            one.close(); ranks.close()
    finally:
        mg.close()
