"""The scratch of psacx_kedit_* on a context that other calls have used: on ONE context a seeded shuffle of kedit calls (sizes going up
and down, with and without a table, one text and a set, with and without PSACX_KEDIT_BEST) between locate, occurrences, mems,
kmismatch, the build of a range-minimum index and psacx_trim.  Every kedit result must equal, bit for bit, the same call on a context
made for it alone, and the host model.  The words of the piece search and the block sums of the scans lie at the base of the ctx
slab, where the other calls keep theirs, and the buffers of the sort of the raw hits are laid over them between two scans; everything
else is the call's own memory.  A missing clearing memset or a use out of order shows here."""
import numpy as np
import pytest

import kedit_model as K
from test_gpu_call_sequences import CALLS, same
from test_gpu_kmismatch_sequences import kmm_call
from test_gpu_mems_sequences import mems_call

pytestmark = pytest.mark.gpu

KED = [  # (kind, n, set, e, k, best)
    ("dna4", 4097, False, 2, 0, False), ("a", 65, False, 1, 1, True), ("dna2", 4095, True, 3, 2, False), ("bytes256", 31, False, 0, 0, False),
    ("tandem7", 4097, True, 1, 0, True), ("fib", 4096, False, 2, 2, False), ("dna4", 33, True, 0, 1, True), ("dna2", 4097, False, 3, 0, True),
]
OTHERS = ["locate u32 k2", "occurrences u32", "rmq u64", "locate u64 k0", "trim", "trim", "mems", "kmismatch"]


def ked_call(ctx, row, bits):
    import psac_amd
    kind, n, as_set, e, k, best = row
    c = K.case(kind, n, as_set)
    dt = np.uint32 if bits == 32 else np.uint64
    return list(psac_amd.kedit(c.text, c.SA.astype(dt), K.patterns(c, e), e, k=k, offsets=c.off, best=best, ctx=ctx))


_alone = {}


def alone(row, bits):
    if (row, bits) not in _alone:
        import psac_amd
        ctx = psac_amd.Context(0)
        try:
            _alone[(row, bits)] = ked_call(ctx, row, bits)
        finally:
            ctx.close()
    return _alone[(row, bits)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("seed", [1, 2])
def test_kedit_between_other_calls_on_one_context(seed, bits):
    import psac_amd
    steps = [("kedit", row) for row in KED] + [("other", name) for name in OTHERS]
    order = [steps[i] for i in np.random.RandomState(seed).permutation(len(steps))]
    ctx = psac_amd.Context(0)
    done = []
    try:
        for what, arg in order:
            done.append("%s %r" % (what, arg))
            if what == "other":
                if arg == "trim":
                    ctx.check(ctx._lib.psacx_trim(ctx.handle))
                elif arg == "mems":
                    mems_call(ctx, ("text", "dna4", 4097), bits, 3, 0, False)
                elif arg == "kmismatch":
                    kmm_call(ctx, ("dna4", 4097, False, 2, 0), bits)
                else:
                    CALLS[arg][0](ctx)
                continue
            got = ked_call(ctx, arg, bits)
            want = alone(arg, bits)
            assert len(got) == 4 and all(same(g, w) for g, w in zip(got, want)), "differs from the call alone"
            kind, n, as_set, e, k, best = arg
            model, _ = K.results(K.case(kind, n, as_set), e)
            model = K.best(model) if best else model
            assert all(np.array_equal(np.asarray(g).astype(np.int64), w) for g, w in zip(got, model)), "differs from the model"
    except BaseException:
        print("seed %d: failed in the last of\n  %s" % (seed, "\n  ".join(done)))
        raise
    finally:
        ctx.close()
