"""The scratch of the FM-index calls on a context that other calls have used: on ONE context a seeded shuffle of FM calls (sizes going up and
down, both forms: FMIndex through the device calls and psacx_fm_search_*) between locate, occurrences, repeats, document calls, the build of
a range-minimum index and psacx_trim.  Every result must equal, bit for bit, the same call on a context made for it alone, and the bytes.
The block sums of the scans, the histogram and the counts per cell lie in the ctx slab, where the other calls keep theirs; the code arrays
are the call's own memory.  A use out of order shows here."""
import numpy as np
import pytest

import locate_gsa_model as G
from fm_gpu_common import expected, fm_case, patterns_of
from test_gpu_call_sequences import CALLS, same
from test_gpu_docs_sequences import doc_call

pytestmark = pytest.mark.gpu

FMS = [("set", 4097, 4), ("text", 63, 2), ("set", 65, 7), ("text", 4097, 256), ("text", 2, 1), ("set", 4097, 8), ("text", 64, 4), ("set", 63, 4)]
OTHERS = ["locate u32 k2", "occurrences u32", "rmq u64", "locate u64 k0", "trim", "trim", "bwt and maximal repeats text4097 u32", "docs r4097", "docs r63"]


def fm_call(ctx, key, bits):
    import psac_amd
    c = fm_case(*key)
    dt = np.uint32 if bits == 32 else np.uint64
    off = None if c.single else c.off
    pats = patterns_of(c)
    fm = psac_amd.fm_index(c.text, c.SA.astype(dt), sample=3, offsets=off, ctx=ctx)
    try:
        out = list(fm.count(pats)) + list(fm.locate(pats, limit=5))
    finally:
        fm.free()
    return out + list(psac_amd.fm_search(c.text, c.SA.astype(dt), pats, sample=32, limit=5, offsets=off, ctx=ctx))


_alone = {}


def alone(key, bits):
    if (key, bits) not in _alone:
        import psac_amd
        ctx = psac_amd.Context(0)
        try:
            _alone[(key, bits)] = fm_call(ctx, key, bits)
        finally:
            ctx.close()
    return _alone[(key, bits)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("seed", [1, 2])
def test_fm_calls_between_other_calls_on_one_context(seed, bits):
    import psac_amd
    steps = [("fm", key) for key in FMS] + [("other", name) for name in OTHERS]
    order = [steps[i] for i in np.random.RandomState(seed).permutation(len(steps))]
    ctx = psac_amd.Context(0)
    done = []
    try:
        for what, arg in order:
            done.append("%s %r" % (what, arg))
            if what == "other":
                if arg == "trim":
                    ctx.check(ctx._lib.psacx_trim(ctx.handle))
                elif arg.startswith("docs "):
                    doc_call(ctx, arg[5:], bits)
                else:
                    CALLS[arg][0](ctx)
                continue
            got = fm_call(ctx, arg, bits)
            want = alone(arg, bits)
            assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want)), "differs from the call alone"
            c = fm_case(*arg)
            lb, ub = expected(c, patterns_of(c))
            occ = G.occurrences(c.SA.astype(np.uint64), c.n, lb.astype(np.uint64), ub.astype(np.uint64), 5)
            model = [lb, ub, occ[0], occ[1]] + ([] if c.single else [G.string_ids(c.off.astype(np.uint64), occ[1], c.n)])
            model = model + model
            assert len(got) == len(model) and all(np.array_equal(np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)) for g, w in zip(got, model)), \
                "differs from the bytes"
    except BaseException:
        print("seed %d: failed in the last of\n  %s" % (seed, "\n  ".join(done)))
        raise
    finally:
        ctx.close()
