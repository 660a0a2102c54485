"""The scratch of psacx_kmismatch_* on a context that other calls have used: on ONE context a seeded shuffle of kmismatch calls (sizes
going up and down, with and without a table, one text and a set) between locate, occurrences, mems, the build of a range-minimum index
and psacx_trim.  Every kmismatch result must equal, bit for bit, the same call on a context made for it alone, and the host model.
The words of the piece search and the block sums of the two scans lie at the base of the ctx slab, where the other calls keep theirs;
everything else is the call's own memory.  A missing clearing memset shows here."""
import numpy as np
import pytest

import kmismatch_model as X
from test_gpu_call_sequences import CALLS, same
from test_gpu_mems_sequences import mems_call

pytestmark = pytest.mark.gpu

KMM = [  # (kind, n, set, e, k)
    ("dna4", 4097, False, 2, 0), ("a", 65, False, 1, 1), ("dna2", 4095, True, 3, 2), ("bytes256", 31, False, 0, 0),
    ("tandem7", 4097, True, 1, 0), ("fib", 4096, False, 2, 2), ("dna4", 33, True, 0, 1),
]
OTHERS = ["locate u32 k2", "occurrences u32", "rmq u64", "locate u64 k0", "trim", "trim", "mems"]


def kmm_call(ctx, row, bits):
    import psac_amd
    kind, n, as_set, e, k = row
    c = X.case(kind, n, as_set)
    dt = np.uint32 if bits == 32 else np.uint64
    return list(psac_amd.kmismatch(c.text, c.SA.astype(dt), c.patterns(e), e, k=k, offsets=c.off, ctx=ctx))


_alone = {}


def alone(row, bits):
    if (row, bits) not in _alone:
        import psac_amd
        ctx = psac_amd.Context(0)
        try:
            _alone[(row, bits)] = kmm_call(ctx, row, bits)
        finally:
            ctx.close()
    return _alone[(row, bits)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("seed", [1, 2])
def test_kmismatch_between_other_calls_on_one_context(seed, bits):
    import psac_amd
    steps = [("kmismatch", row) for row in KMM] + [("other", name) for name in OTHERS]
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
                else:
                    CALLS[arg][0](ctx)
                continue
            got = kmm_call(ctx, arg, bits)
            want = alone(arg, bits)
            assert len(got) == 3 and all(same(g, w) for g, w in zip(got, want)), "differs from the call alone"
            kind, n, as_set, e, k = arg
            model, _ = X.case(kind, n, as_set).results(e)
            assert all(np.array_equal(np.asarray(g).astype(np.int64), w) for g, w in zip(got, model)), "differs from the model"
    except BaseException:
        print("seed %d: failed in the last of\n  %s" % (seed, "\n  ".join(done)))
        raise
    finally:
        ctx.close()
