"""The scratch of psacx_mems_* on a context that other calls have used: on ONE context a construction, repeats, lz77, occurrences and
then mems, with sizes going up and down and psacx_trim in between.  Every mems result must equal, bit for bit, the same call on a
context made for it alone, and the host model.  The count arrays of the walk live in the ctx slab behind the block sums of the scan,
where the directories of the repeats, the pyramid of the parse and the words of the searches have been; the kept-slot counter of
PSACX_MEMS_SUPER is one word there.  A missing clearing memset shows here."""
import numpy as np
import pytest

import lz_model as Z
import mems_model as X
from mems_gpu_common import patterns_of
from repeats_gpu_common import set_case, text_case
from test_gpu_call_sequences import CALLS, same

pytestmark = pytest.mark.gpu

ROUNDS = [  # (case, min_len, max_occ, super, the calls in front of it)
    (("text", "dna4", 4097), 3, 0, False, ["construct dna12300 u32 device", "bwt and maximal repeats text4097 u32"]),
    (("text", "a", 65), 1, 0, False, ["lpf and lz77 dna4096 u32", "occurrences u32"]),
    (("set", "random2"), 2, 3, False, ["construct tandem u32 host", "bwt and supermaximal repeats set4095 u64", "trim"]),
    (("text", "dna2", 4097), 4, 0, True, ["lpf and lz77 tandem3000 u64", "occurrences u32"]),
    (("text", "tandem7", 4097), 1, 0, False, ["trim", "construct dna100 u32 host"]),
    (("text", "dna4", 31), 1, 0, True, ["bwt and maximal repeats text4097 u32", "match u32 k0"]),
    (("set", "acgt3000"), 1, 0, False, ["construct dna4097 u32 device", "trim", "rmq u64"]),
]


def case_of(key):
    if key[0] == "set":
        c = set_case(key[1])
        s = c.text.tobytes()
        return c, patterns_of("set", c.text, whole=False) + [s[int(c.off[1]) - 2:int(c.off[1]) + 2]] + c.strings[:2]
    c = text_case(key[1], key[2])
    return c, patterns_of(key[1], c.text, whole=False)


def mems_call(ctx, key, bits, min_len, max_occ, sup):
    import psac_amd
    c, pats = case_of(key)
    dt = np.uint32 if bits == 32 else np.uint64
    return list(psac_amd.mems(c.text, c.SA.astype(dt), c.LCP.astype(dt), pats, min_len, k=0, offsets=c.off, max_occ=max_occ, super=sup, ctx=ctx))


_alone = {}


def alone(key, bits, *params):
    k = (key, bits) + params
    if k not in _alone:
        import psac_amd
        ctx = psac_amd.Context(0)
        try:
            _alone[k] = mems_call(ctx, key, bits, *params)
        finally:
            ctx.close()
    return _alone[k]


@pytest.mark.parametrize("bits", [32, 64])
def test_mems_behind_other_calls_on_one_context(bits):
    import psac_amd
    ctx = psac_amd.Context(0)
    done = []
    try:
        for key, min_len, max_occ, sup, before in ROUNDS:
            for name in before:
                done.append(name)
                if name == "trim":
                    ctx.check(ctx._lib.psacx_trim(ctx.handle))
                else:
                    CALLS[name][0](ctx)
            done.append("mems %r" % (key,))
            got = mems_call(ctx, key, bits, min_len, max_occ, sup)
            want = alone(key, bits, min_len, max_occ, sup)
            assert len(got) == 3 and all(same(g, w) for g, w in zip(got, want)), "differs from the call alone"
            c, pats = case_of(key)
            m, _ = X.by_walk_arrays(c.SA, c.LCP, c.bwt, c.first, pats, X.statistics(c.text, c.SA, pats, c.off), min_len, max_occ, sup)
            assert all(np.array_equal(np.asarray(g).astype(np.int64), w) for g, w in zip(got, m)), "differs from the model"
    except BaseException:
        print("failed in the last of\n  %s" % "\n  ".join(done))
        raise
    finally:
        ctx.close()
