"""What real leftovers do: one context runs a fixed, seeded shuffle of about 30 calls drawn from every family of the library --
constructions of texts and string sets through host and device pointers, the stand-alone sort, ANSV, the suffix-tree builder, the
checkers on right and on wrong arrays, and the query calls -- whose sizes go up and down: a construction of 2^20 characters, then one of
100, then queries on an index of 12 300 characters, and so on, with psacx_trim at three points in between.  Every suite before this one
made a context per test or per module and ran its calls in one fixed order with sizes that only grew, so no operation ever ran on the
scratch another operation had used, and no small call on the slab of a large one.

Every result must equal, bit for bit, the result of the same call on a context made for it alone, and the host model's or the oracle's
where the family has one (the construction of 2^20 characters: the reference's checksums in tests/golden/reference_kat.json).  Two
seeds.  The seeded order is printed on failure.

A missing clearing memset shows here when the call before left something else in the word: with the 32 bytes of check_dev, the
three words of search_with_slab_words or the counter of check_lz77_dev left uncleared, every case of this file fails."""
import json
import os

import numpy as np
import pytest

import inputs
import lce_model as E
import locate_model as L
import lz_model as Z
import match_model as M
import oracle_lib as O
import overlaps_model as V
import repeats_model as R
import rmq_model as Q
import st_checker_model as S
from test_gpu_grid_trips import TEXT, names, rep_case

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (20260, 7)
TRIMS = 3
NONE = 2**64 - 1

_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def dt_of(bits):
    return np.uint32 if bits == 32 else np.uint64


def kat_row():
    with open(os.path.join(HERE, "golden", "reference_kat.json")) as f:
        return [r for r in json.load(f)["checksums"] if r["name"] == "ascii128_1M_42"][0]


def text_named(name):
    from test_oracle_golden import make_input
    if name == "kat1M":
        return memo("kat1M", lambda: make_input(kat_row()))
    if name == "dna12300":
        return memo("dna12300", lambda: inputs.dna(12300, 41))
    if name == "tandem":
        return memo("tandem", lambda: inputs.tandem(40000, 256, O.rand_dna(256, 3)))
    kind, n = name[:3], int(name[3:])
    assert kind == "dna"
    return memo(name, lambda: O.rand_dna(n, 13))


def oracle(name, bits):
    return memo(("oracle", name, bits), lambda: O.construct(text_named(name), bits=bits))


STRINGS = [bytes(inputs.dna(300, 4))[:int(x)] for x in np.random.RandomState(11).randint(1, 300, size=300)]


# ---- the calls: name -> (run(ctx) -> list of arrays / numbers, model() -> the same list or None)
def construction(name, bits, device):
    def run(ctx):
        import psac_amd
        text = text_named(name)
        sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
        if not device:
            sa.construct(text)
            return [sa.local_SA, sa.local_B, sa.local_LCP]
        n, w = int(text.size), bits // 8
        d = [ctx.alloc(n)] + [ctx.alloc(n * w) for _ in range(3)]
        try:
            ctx.h2d(d[0], text)
            sa.construct_device(d[0], n, d[1], d[2], d[3])
            out = [np.empty(n, sa.dtype) for _ in range(3)]
            for a, p in zip(out, d[1:]):
                ctx.d2h(a, p)
        finally:
            for p in d:
                ctx.free(p)
        return out

    def model():
        if name == "kat1M":
            return None                                                   # (its checksums are checked in agree_with_model)
        ref = oracle(name, bits)
        return [ref["SA"], ref["ISA"], ref["LCP"]]
    return run, model


def string_set(bits):
    def run(ctx):
        import psac_amd
        sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
        sa.construct_ss(STRINGS)
        return [sa.local_SA, sa.local_B, sa.local_LCP]

    def model():
        ref = memo(("ss", bits), lambda: O.construct_ss(STRINGS, bits=bits))
        return [ref["SA"], ref["ISA"], ref["LCP"]]
    return run, model


def pair_sort(n, bits):
    def keys():
        rng = np.random.RandomState(n % 1000)
        return rng.randint(0, 50, n).astype(dt_of(bits)), rng.randint(0, 1 << 20, n).astype(dt_of(bits))

    def run(ctx):
        from test_gpu_kernel_edges import _sort_standalone
        b1, b2 = keys()
        return list(_sort_standalone(ctx, b1, b2, 21)[:3])

    def model():
        b1, b2 = keys()
        order = np.lexsort((b2, b1))
        return [b1[order], b2[order], order.astype(dt_of(bits))]
    return run, model


def ansv(n, bits, device):
    def values():
        return inputs.ansv_edge_values("top3", n, dt_of(bits), seed=5)

    def run(ctx):
        import psac_amd
        v = values()
        if not device:
            return list(psac_amd.ansv(v, 2, 0, nonsv=NONE, ctx=ctx))
        d_in, d_l, d_r = ctx.alloc(v.nbytes), ctx.alloc(n * 8), ctx.alloc(n * 8)
        try:
            ctx.h2d(d_in, v)
            psac_amd.ansv_device(ctx, d_in, n, d_l, d_r, bits, 2, 0, NONE)
            out = [np.empty(n, np.uint64), np.empty(n, np.uint64)]
            ctx.d2h(out[0], d_l); ctx.d2h(out[1], d_r)
        finally:
            for p in (d_in, d_l, d_r):
                ctx.free(p)
        return out

    def model():
        return memo(("ansv", n, bits), lambda: [O.ansv(values(), True, 2, NONE), O.ansv(values(), False, 0, NONE)])
    return run, model


def suffix_tree(name, bits):
    def run(ctx):
        import psac_amd
        text, SA, LCP, recs, table = S.arrays(name)
        return [psac_amd.suffix_tree(text, SA.astype(dt_of(bits)), LCP.astype(dt_of(bits)), ctx=ctx)]

    def model():
        return [S.arrays(name)[4]]
    return run, model


def checker(name, bits, wrong):
    def arrays_of():
        ref = oracle(name, bits)
        lcp = ref["LCP"].copy()
        if wrong:
            lcp[1000] += 77
        return text_named(name), ref["SA"], ref["ISA"], lcp

    def run(ctx):
        import psac_amd
        text, SA, ISA, LCP = arrays_of()
        n, w = int(text.size), bits // 8
        d = [ctx.alloc(n)] + [ctx.alloc(n * w) for _ in range(3)]
        try:
            for p, a in zip(d, (text, SA, ISA, LCP)):
                ctx.h2d(p, a if a.dtype == np.uint8 else a.astype(dt_of(bits)))
            return [np.array(psac_amd.check_device(ctx, d[0], n, d[1], d[2], d[3], bits), np.uint64)]
        finally:
            for p in d:
                ctx.free(p)

    def model():
        import checker_model as CM
        text, SA, ISA, LCP = arrays_of()
        want = CM.expect_both(text, SA.astype(np.uint64), ISA.astype(np.uint64), LCP.astype(np.uint64))[0]
        assert (sum(want) > 0) == wrong
        return [np.array(want, np.uint64)]
    return run, model


def index12300(bits):
    names()
    ref = oracle("dna12300", bits)
    return (text_named("dna12300"),) + tuple(ref[k].astype(dt_of(bits)) for k in ("SA", "ISA", "LCP"))


def locate(bits, k):
    def run(ctx):
        import psac_amd
        text, SA = index12300(bits)[:2]
        return list(psac_amd.locate(text, SA, L.expected(TEXT)[0], k=k, ctx=ctx))

    def model():
        names()
        return [a.astype(dt_of(bits)) for a in L.expected(TEXT)[1:]]
    return run, model


def match(bits, k):
    def run(ctx):
        import psac_amd
        text, SA = index12300(bits)[:2]
        return list(psac_amd.match(text, SA, M.expected(TEXT)[0], k=k, ctx=ctx))

    def model():
        names()
        return [np.asarray(a).astype(dt_of(bits)) for a in M.expected(TEXT)[1:]]
    return run, model


def occurrences(bits):
    def intervals():
        names()
        return L.expected(TEXT)[1:]

    def run(ctx):
        import psac_amd
        lb, ub = intervals()
        return list(psac_amd.occurrences(index12300(bits)[1], lb, ub, limit=5, ctx=ctx))

    def model():
        import locate_gsa_model as G
        lb, ub = intervals()
        start, pos, _ = G.occurrences(index12300(bits)[1], 12300, lb, ub, 5)
        return [np.asarray(start, np.uint64), np.asarray(pos).astype(dt_of(bits))]
    return run, model


def rmq(bits):
    def ranges():
        rng = np.random.RandomState(9)
        lo = rng.randint(0, 12300, 3000)
        return lo, np.minimum(12300, lo + rng.choice([0, 1, 2, 65, 4097, 12300], lo.size))

    def run(ctx):
        import psac_amd
        return list(psac_amd.rmq(index12300(bits)[3], *ranges(), ctx=ctx))

    def model():
        lo, hi = ranges()
        want = Q.Table(index12300(bits)[3]).queries(lo, hi)
        return [np.asarray(w).astype(dt_of(bits)) for w in want]
    return run, model


def lce(bits):
    def pairs():
        rng = np.random.RandomState(10)
        SA = index12300(bits)[1].astype(np.int64)
        i = rng.randint(0, 12299, 600)
        return np.concatenate([SA[i], rng.randint(0, 12302, 200)]), np.concatenate([SA[i + 1], rng.randint(0, 12302, 200)])

    def run(ctx):
        import psac_amd
        text, SA, ISA, LCP = index12300(bits)
        return [psac_amd.lce(ISA, LCP, *pairs(), max_mismatch=1, ctx=ctx)]

    def model():
        text = index12300(bits)[0]
        return [np.array([E.by_bytes(text, None, int(x), int(y), 1) for x, y in zip(*pairs())]).astype(dt_of(bits))]
    return run, model


def overlaps(bits):
    name = "copies300"

    def run(ctx):
        import psac_amd
        text, off, SA, ISA, LCP = V.set_arrays(name)
        d = dt_of(bits)
        return list(psac_amd.overlaps(int(text.size), off, SA.astype(d), ISA.astype(d), LCP.astype(d), V.min_lens(name)[0], True, ctx=ctx))

    def model():
        return [np.asarray(w).astype(dt_of(bits)) for w in V.slots(name, V.min_lens(name)[0], True)]
    return run, model


def lz77(name, bits):
    def run(ctx):
        import psac_amd
        t, SA, LCP = Z.arrays(name)
        d = dt_of(bits)
        return list(psac_amd.lpf(SA.astype(d), LCP.astype(d), ctx=ctx)) + list(psac_amd.lz77(SA.astype(d), LCP.astype(d), ctx=ctx))

    def model():
        ones = int(np.iinfo(dt_of(bits)).max)
        unsigned = lambda a: np.where(np.asarray(a) == Z.ONES, ones, np.asarray(a)).astype(dt_of(bits))      # noqa: E731
        lpf, src = Z.lpf_of(name)
        start, psrc = Z.parse_of(name)
        return [unsigned(lpf), None, unsigned(start), unsigned(psrc)]     # (any source of the right length is a right answer: lz_model.py)
    return run, model


def lz77_checker(name, bits, wrong):
    def parse():
        start, src = Z.parse_of(name)
        if wrong:
            from test_gpu_lz77_verifier import mutations
            _, start, src = mutations(Z.text_of(name), start, src)[0]
        return start, src

    def run(ctx):
        from rmq_gpu_common import Dev
        from test_gpu_lz77_verifier import device_count
        dev = Dev(ctx, bits)
        try:
            return [np.uint64(device_count(dev, Z.text_of(name), *parse()))]
        finally:
            dev.close()

    def model():
        want = Z.check_count(Z.text_of(name), *parse())
        assert (want > 0) == wrong
        return [np.uint64(want)]
    return run, model


def bwt_and_repeats(which, bits, kind):
    def run(ctx):
        import psac_amd
        c = rep_case(which)
        d = dt_of(bits)
        b, primary = psac_amd.bwt(c.text, c.SA.astype(d), offsets=c.off, ctx=ctx)
        return [b, np.uint64(primary)] + list(psac_amd.repeats(c.text, c.SA.astype(d), c.LCP.astype(d), kind=kind, min_len=2, offsets=c.off, ctx=ctx))

    def model():
        c = rep_case(which)
        want = R.triples(R.select(c.results(kind), min_len=2))
        return [c.bwt, np.uint64(c.primary)] + [np.asarray(w).astype(dt_of(bits)) for w in want]
    return run, model


def calls():
    """about 30 calls, every family, sizes mixed; the shuffle orders them"""
    c = {}
    c["construct kat1M u64 host"] = construction("kat1M", 64, False)
    c["construct kat1M u64 device"] = construction("kat1M", 64, True)
    c["construct dna100 u32 host"] = construction("dna100", 32, False)
    c["construct dna100 u64 device"] = construction("dna100", 64, True)
    c["construct dna4097 u32 device"] = construction("dna4097", 32, True)
    c["construct tandem u32 host"] = construction("tandem", 32, False)
    c["construct tandem u64 device"] = construction("tandem", 64, True)
    c["construct dna12300 u32 device"] = construction("dna12300", 32, True)
    c["string set u32"] = string_set(32)
    c["string set u64"] = string_set(64)
    c["pair sort 4097 u32"] = pair_sort(4097, 32)
    c["pair sort 2^21+1 u64"] = pair_sort((1 << 21) + 1, 64)
    c["ansv 65537 u32 host"] = ansv(65537, 32, False)
    c["ansv 4097 u64 device"] = ansv(4097, 64, True)
    c["suffix tree edge4097 u32"] = suffix_tree("edge4097", 32)
    c["suffix tree tandem u64"] = suffix_tree("tandem", 64)
    c["check dna12300 u32 right"] = checker("dna12300", 32, False)
    c["check dna12300 u64 wrong"] = checker("dna12300", 64, True)
    c["locate u32 k2"] = locate(32, 2)
    c["locate u64 k0"] = locate(64, 0)
    c["match u32 k0"] = match(32, 0)
    c["match u64 k2"] = match(64, 2)
    c["occurrences u32"] = occurrences(32)
    c["rmq u64"] = rmq(64)
    c["lce u32"] = lce(32)
    c["overlaps u64"] = overlaps(64)
    c["lpf and lz77 dna4096 u32"] = lz77("dna4096", 32)
    c["lpf and lz77 tandem3000 u64"] = lz77("tandem3000", 64)
    c["check lz77 dna4096 u64 right"] = lz77_checker("dna4096", 64, False)
    c["check lz77 tandem3000 u32 wrong"] = lz77_checker("tandem3000", 32, True)
    c["bwt and maximal repeats text4097 u32"] = bwt_and_repeats("text4097", 32, R.MAXIMAL)
    c["bwt and supermaximal repeats set4095 u64"] = bwt_and_repeats("set4095", 64, R.SUPER)
    return c


CALLS = calls()
_alone = {}


def alone(name):
    """the result of the call on a context made for it alone (no option set): computed once, shared, never written"""
    if name not in _alone:
        import psac_amd
        ctx = psac_amd.Context(0)
        try:
            _alone[name] = CALLS[name][0](ctx)
        finally:
            ctx.close()
    return _alone[name]


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b)) and np.asarray(a).dtype == np.asarray(b).dtype


def agree_with_model(name, got):
    want = CALLS[name][1]()
    if name.startswith("construct kat1M"):
        row = kat_row()
        assert ["%016x" % O.fnv(a) for a in got] == [row["sa"], row["isa"], row["lcp"]], name
        return
    assert len(got) == len(want), name
    for k, (g, w) in enumerate(zip(got, want)):
        if w is not None:
            assert np.array_equal(np.asarray(g).astype(np.uint64), np.asarray(w).astype(np.uint64)), (name, k)


def order_of(seed):
    rng = np.random.RandomState(seed)
    order = [sorted(CALLS)[i] for i in rng.permutation(len(CALLS))]
    # sizes go down as well as up whatever the shuffle says: the largest construction is followed by the smallest
    order.remove("construct dna100 u32 host")
    order.insert(order.index("construct kat1M u64 host") + 1, "construct dna100 u32 host")
    trims = sorted(rng.choice(np.arange(3, len(order) - 2), TRIMS, replace=False).tolist())
    return order, trims


def test_the_models_agree_with_a_context_of_ones_own():
    assert 28 <= len(CALLS) <= 34
    for name in sorted(CALLS):
        agree_with_model(name, alone(name))


@pytest.mark.parametrize("seed", SEEDS)
def test_shuffled_calls_on_one_context(seed):
    import psac_amd
    order, trims = order_of(seed)
    ctx = psac_amd.Context(0)
    done = []
    try:
        for step, name in enumerate(order):
            if step in trims:
                ctx.check(ctx._lib.psacx_trim(ctx.handle))
                done.append("psacx_trim")
            done.append(name)
            got = CALLS[name][0](ctx)
            want = alone(name)
            assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want)), "differs from the call alone"
            agree_with_model(name, got)
        assert done.count("psacx_trim") == TRIMS
    except BaseException:
        print("seed %d: failed in the last of\n  %s" % (seed, "\n  ".join(done)))
        raise
    finally:
        ctx.close()
