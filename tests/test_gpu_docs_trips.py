"""The second and later trips of the grid-stride loops of psacx_doc_index_dev_*, psacx_doc_count_dev_* and psacx_doc_list_dev_*: the
random sets of 4097 and 2^18 + 1 bytes once more against the host model with PSACX_OPT_GRID_CAP cutting every grid of grid_for() to 1 and to
3 workgroups, both index widths (tests/test_gpu_grid_trips.py has the reasons and the fixture).  Every case states the workgroups its
launches ask for -- a thread per rank for the keys, the key summary or histogram of the sort and prev, sixteen lanes per rank for the
pairs, a thread per interval for the counts, the candidate numbers and the starts, a workgroup per 1024 candidates for the marks, their
tile counts and the compaction -- and sees psacx_stats.grid_cuts rise across each call.  The passes of the sort and the scans size their
grids themselves."""
import numpy as np
import pytest

import docs_model as D
from docs_gpu_common import BIG, DocIndex, check_index, check_queries, doc_case, lcp_intervals
from rmq_gpu_common import Dev, first_bad
from test_gpu_grid_trips import LANES, OCC_TILE, asked, cap, ctx, cut, strides  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [4097, BIG])
def test_doc_calls_with_cut_grids(ctx, cap, n, bits):
    dev = Dev(ctx, bits)
    try:
        c = doc_case("r%d" % n)
        d = DocIndex(dev, c)
        strides(cap, asked(n), asked(n * LANES))
        with cut(ctx):
            check_index(d, (n, "index"))
        lb, ub = lcp_intervals(c)
        strides(cap, asked(lb.size))
        with cut(ctx):
            got = d.count(lb, ub)
        assert first_bad(got, D.count_by_dup(c.dup, lb, ub, n)) is None
        with cut(ctx):
            la, lu, _ = check_queries(d, (n, "queries"), limit=20000)
        la, lu = np.tile(la, 2), np.tile(lu, 2)         # more than 3 x 256 intervals
        cand = int(np.sum(np.where((la <= lu) & (lu <= n), lu - la, 0)))
        strides(cap, asked(la.size + 1), asked(cand, OCC_TILE // 256))
        with cut(ctx):
            d.run_lists(la, lu, D.list_by_prev(c.prev, c.SA, c.off, la, lu, n), (n, "lists"))
        assert d.unchanged()
    finally:
        dev.close()
