"""The second and later trips of the grid-stride loops of psacx_fm_index_dev_*, psacx_fm_count_dev_* and psacx_fm_occurrences_dev_*: a text
of 4097 bytes and a set of 2^18 + 1 once more against the bytes with PSACX_OPT_GRID_CAP cutting every grid of grid_for() to 1 and to 3
workgroups, both index widths (tests/test_gpu_grid_trips.py has the reasons and the fixture).  Every case states the workgroups its
launches ask for -- a thread per rank for the histogram and the codes, a wave per 64 ranks for the levels and the marks, a thread per
pattern for the search and per interval for the counts, a workgroup per 1024 slots for the walk -- and sees psacx_stats.grid_cuts rise
across the build, the count and the occurrence call.  The scans size their grids themselves."""
import numpy as np
import pytest

import fm_model as F
from fm_gpu_common import BIG, FmDev, expected, fm_case, patterns_of, pipeline_of
from rmq_gpu_common import Dev, first_bad
from test_gpu_grid_trips import OCC_TILE, asked, cap, ctx, cut, strides  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [4097, BIG])
def test_fm_calls_with_cut_grids(ctx, cap, n, bits):
    dev = Dev(ctx, bits)
    try:
        c = fm_case("text" if n == 4097 else "set", n, 4)
        d = FmDev(dev, c)
        strides(cap, asked(n), asked(n + 64))
        with cut(ctx):
            blob = d.build(32)
        if n == 4097:
            assert first_bad(blob, F.blob_of(pipeline_of(c, 32), bits // 8)[0]) is None
        pats = patterns_of(c)
        pats = pats * (-(-(3 * 256 + 1) // len(pats)))          # more than 3 x 256 patterns
        lb, ub = expected(c, pats)
        strides(cap, asked(len(pats)))
        with cut(ctx):
            got = d.count(pats)
        assert first_bad(got[0], lb) is None and first_bad(got[1], ub) is None
        lb, ub = lb[1:], ub[1:]                                 # (without the empty pattern and its n occurrences)
        total = int(np.sum(np.minimum(ub - lb, 50)))
        strides(cap, asked(lb.size + 1), asked(total, OCC_TILE // 256))
        with cut(ctx):
            assert d.check_occurrences(lb, ub, limit=50) == total
        assert d.unchanged()
    finally:
        dev.close()
