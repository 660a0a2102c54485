"""The scratch of the text-sample build and of the extraction on a context that other calls have used: on ONE context a seeded shuffle of
sample builds and extractions (sizes going up and down) between count / locate calls of the same index, occurrences, locate, the build of a
range-minimum index and psacx_trim.  Every result must equal, bit for bit, the same call on a context made for it alone, and the bytes.
The bitmap of the string ends of the sample build, the block sums of the scans and the segment starts of the extraction lie in the ctx
slab, where the other calls keep theirs.  A use out of order shows here."""
import numpy as np
import pytest

import fm_extract_model as X
import locate_gsa_model as G
from fm_extract_gpu_common import whole_strings, windows_of
from fm_gpu_common import expected, fm_case, patterns_of
from test_gpu_call_sequences import CALLS, same

pytestmark = pytest.mark.gpu

FMS = [("set", 4097, 4, 32), ("text", 63, 4, 2), ("set", 65, 4, 3), ("text", 4097, 256, 64), ("text", 2, 1, 1), ("set", 4097, 1, 5000), ("text", 64, 4, 64),
       ("set", 63, 4, 1)]
OTHERS = ["locate u32 k2", "occurrences u32", "rmq u64", "locate u64 k0", "trim", "trim", "trim"]


def queries(c, rate):
    whole, wins = whole_strings(c), windows_of(c, rate)
    return np.concatenate((whole[0], wins[0])), np.concatenate((whole[1], wins[1]))


def ext_call(ctx, key, bits):
    import psac_amd
    c = fm_case(*key[:3])
    dt = np.uint32 if bits == 32 else np.uint64
    pats = patterns_of(c)
    fm = psac_amd.fm_index(c.text, c.SA.astype(dt), sample=3, offsets=None if c.single else c.off, ctx=ctx, text_rate=key[3])
    try:
        out = list(fm.extract(*queries(c, key[3])))
        out += list(fm.count(pats))
        out += list(fm.extract(np.arange(c.n), 1))
        out += list(fm.locate(pats, limit=5))
        text = fm.text()
        out.append(np.frombuffer(text if c.single else b"".join(text), np.uint8))
    finally:
        fm.free()
    return out


_alone = {}


def alone(key, bits):
    if (key, bits) not in _alone:
        import psac_amd
        ctx = psac_amd.Context(0)
        try:
            _alone[(key, bits)] = ext_call(ctx, key, bits)
        finally:
            ctx.close()
    return _alone[(key, bits)]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("seed", [1, 2])
def test_extract_calls_between_other_calls_on_one_context(seed, bits):
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
                else:
                    CALLS[arg][0](ctx)
                continue
            got = ext_call(ctx, arg, bits)
            want = alone(arg, bits)
            assert len(got) == len(want) and all(same(g, w) for g, w in zip(got, want)), "differs from the call alone"
            c = fm_case(*arg[:3])
            lb, ub = expected(c, patterns_of(c))
            occ = G.occurrences(c.SA.astype(np.uint64), c.n, lb.astype(np.uint64), ub.astype(np.uint64), 5)
            model = list(X.by_bytes(c.strings, *queries(c, arg[3]))) + [lb, ub] + [np.arange(c.n + 1), c.text, occ[0], occ[1]]
            model += ([] if c.single else [G.string_ids(c.off.astype(np.uint64), occ[1], c.n)]) + [c.text]
            assert len(got) == len(model) and all(np.array_equal(np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)) for g, w in zip(got, model)), \
                "differs from the bytes"
    except BaseException:
        print("seed %d: failed in the last of\n  %s" % (seed, "\n  ".join(done)))
        raise
    finally:
        ctx.close()
