"""The scratch of psacx_doc_count_* / psacx_doc_list_* on a context that other calls have used: on ONE context a seeded shuffle of doc
calls (sizes going up and down) between locate, occurrences, mems, kmismatch, the build of a range-minimum index and psacx_trim.  Every
result must equal, bit for bit, the same call on a context made for it alone, and the host model.  The buffers of the rank-pair sort and
the block sums of the scans lie at the base of the ctx slab, where the other calls keep theirs; everything else is the call's own memory.
A missing clearing memset or a use out of order shows here."""
import numpy as np
import pytest

import docs_model as D
from docs_gpu_common import doc_case, lcp_intervals
from test_gpu_call_sequences import CALLS, same
from test_gpu_kmismatch_sequences import kmm_call
from test_gpu_mems_sequences import mems_call

pytestmark = pytest.mark.gpu

DOCS = ["r4097", "r63", "acgt3000", "r2", "uneven", "r4095", "w257", "r1", "random2", "r65"]
OTHERS = ["locate u32 k2", "occurrences u32", "rmq u64", "locate u64 k0", "trim", "trim", "mems", "kmismatch"]


def intervals(c):
    lb, ub = lcp_intervals(c)
    ra, rb = D.random_intervals(c.n, 100, c.n % 53)
    return lb, ub, np.concatenate((lb[::7], ra)), np.concatenate((ub[::7], rb))


def doc_call(ctx, name, bits):
    import psac_amd
    c = doc_case(name)
    dt = np.uint32 if bits == 32 else np.uint64
    lb, ub, la, lu = intervals(c)
    sa, lcp = c.SA.astype(dt), c.LCP.astype(dt)
    return [psac_amd.doc_count(sa, lcp, c.off, lb, ub, ctx=ctx)] + list(psac_amd.doc_list(sa, c.off, la, lu, ctx=ctx))


_alone = {}


def alone(name, bits):
    if (name, bits) not in _alone:
        import psac_amd
        ctx = psac_amd.Context(0)
        try:
            _alone[(name, bits)] = doc_call(ctx, name, bits)
        finally:
            ctx.close()
    return _alone[(name, bits)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("seed", [1, 2])
def test_doc_calls_between_other_calls_on_one_context(seed, bits):
    import psac_amd
    steps = [("docs", name) for name in DOCS] + [("other", name) for name in OTHERS]
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
            got = doc_call(ctx, arg, bits)
            want = alone(arg, bits)
            assert len(got) == 4 and all(same(g, w) for g, w in zip(got, want)), "differs from the call alone"
            c = doc_case(arg)
            lb, ub, la, lu = intervals(c)
            start, _, sid, pos = D.list_by_prev(c.prev, c.SA, c.off, la, lu, c.n)
            model = [D.count_by_dup(c.dup, lb, ub, c.n), start, sid, pos]
            assert all(np.array_equal(np.asarray(g).astype(np.int64), w) for g, w in zip(got, model)), "differs from the model"
    except BaseException:
        print("seed %d: failed in the last of\n  %s" % (seed, "\n  ".join(done)))
        raise
    finally:
        ctx.close()
