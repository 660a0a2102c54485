"""The second and later trips of the grid-stride loops of psacx_fm_text_samples_dev_* and psacx_fm_extract_dev_*: a text of 4097 bytes
and a set of 2^18 + 1 once more against the bytes with PSACX_OPT_GRID_CAP cutting every grid of grid_for() to 1 and to 3 workgroups, both
index widths (tests/test_gpu_grid_trips.py has the reasons and the fixture).  Every case states the workgroups its launches ask for -- a
thread per rank for the samples, a thread per query for the lengths and segment counts, a workgroup per 1024 segments for the walk, of
which there are more than 3 x 1024 -- and sees psacx_stats.grid_cuts rise across the sample build and the extraction.  The scans size
their grids themselves."""
import numpy as np
import pytest

import fm_extract_model as X
from fm_extract_gpu_common import ExtDev, whole_strings
from fm_gpu_common import BIG, fm_case
from rmq_gpu_common import Dev, first_bad
from test_gpu_grid_trips import OCC_TILE, asked, cap, ctx, cut, strides  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [4097, BIG])
def test_samples_and_extraction_with_cut_grids(ctx, cap, n, bits):
    dev = Dev(ctx, bits)
    try:
        c = fm_case("text" if n == 4097 else "set", n, 4)
        d = ExtDev(dev, c)
        d.build(0)
        rate = 1 if n == 4097 else 32
        strides(cap, asked(n))
        with cut(ctx):
            ts = d.samples(rate)
        assert first_bad(ts, X.sample_arrays(c.strings, c.SA, rate)) is None
        if n == 4097:                                   # every position a query of its own, and a block of its own
            pos, ln = np.arange(n), np.ones(n, np.int64)
            segments = n
        else:                                           # every string, in blocks of 32
            pos, ln = whole_strings(c)
            segments = int(np.sum((pos + ln - 1) // rate - pos // rate + 1))
        assert segments > 3 * OCC_TILE
        strides(cap, asked(pos.size + 1), asked(segments, OCC_TILE // 256))
        with cut(ctx):
            assert d.check(pos, ln) == n
        assert d.unchanged()
    finally:
        dev.close()
