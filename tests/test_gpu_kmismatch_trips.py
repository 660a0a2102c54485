"""The second and later trips of the grid-stride loops of psacx_kmismatch_dev_*: one text and a set at 4097 and 2^18 + 1 once more
against the host model with PSACX_OPT_GRID_CAP cutting every grid of grid_for() to 1 and to 3 workgroups, both index widths
(tests/test_gpu_grid_trips.py has the reasons and the fixture).  Every case states the workgroups its launches ask for -- a thread per
piece for the piece offsets, the search and the counts, a workgroup per 1024 candidates for the marks, the tile counts and the
triples -- and sees psacx_stats.grid_cuts rise across the call.  At 2^18 + 1 the model is the pipeline alone (by_pieces).

And once 2^18 patterns of 8 bytes with e = 3: 2^20 + 1 piece offsets and candidate starts, the second chunk of the block sums of the
scan.  The model would take a million bisections; the counters and the hits are stated with numpy instead."""
import numpy as np
import pytest

import kmismatch_model as X
from kmismatch_gpu_common import BIG, KmmIndex, check
from rmq_gpu_common import Dev
from test_gpu_grid_trips import OCC_TILE, asked, cap, ctx, cut, strides  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
@pytest.mark.parametrize("n", [4097, BIG])
@pytest.mark.parametrize("kind", ["dna2", "tandem7"])
def test_main_cases_with_cut_grids(ctx, cap, kind, n, as_set, bits):
    dev = Dev(ctx, bits)
    try:
        case = X.case(kind, n, as_set)
        pats = case.patterns(2) * (16 if kind == "tandem7" else 8)     # more than 3 * 256 pieces
        d = KmmIndex(dev, case, pats, k=2 if as_set else 0)
        with cut(ctx):
            _, work = check(d, 2, (kind, n, as_set), case.results(2, pats, "x8"))
        strides(cap, asked(d.q * 3), asked(work[0], OCC_TILE // 256))
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_a_million_pieces(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        n, q, m, e = 4097, 1 << 18, 8, 3
        case = X.case("bytes256", n)
        t = case.text
        rng = np.random.RandomState(23)
        at = rng.randint(0, n - m + 1, q)
        rows = t[at[:, None] + np.arange(m)[None, :]].copy()
        d_want = (np.arange(q) % 3).astype(np.int64)        # 0, 1 or 2 bytes substituted, each by its complement: in pieces 0 and 2
        rows[d_want >= 1, 1] ^= 0xFF
        rows[d_want >= 2, 5] ^= 0xFF
        pats = [r.tobytes() for r in rows]
        d = KmmIndex(dev, case, pats)
        assert d.q * (e + 1) + 1 > (1 << 20)
        (qid, tpos, dist), work = d.run(e)
        # the candidates: the occurrences of every two-byte piece; tested: those whose window lies inside the text
        pair = t[:-1].astype(np.int64) * 256 + t[1:]
        key = np.sort(pair * (n + 1) + np.arange(n - 1))
        piece = rows[:, 0::2].astype(np.int64) * 256 + rows[:, 1::2]                         # q x 4
        lo = np.searchsorted(key, piece * (n + 1), "left")
        counts = np.searchsorted(key, piece * (n + 1) + n, "right") - lo
        starts = np.cumsum(counts.reshape(-1))
        assert work[0] == int(starts[-1])
        b = np.arange(4)[None, :] * 2
        inside = np.searchsorted(key, piece * (n + 1) + (n - m + b), "right") - np.searchsorted(key, piece * (n + 1) + b, "left")
        assert work[1] == int(inside.sum())
        # every pattern is found where it was cut, with the bytes substituted as its distance; the hits are true and in order
        assert np.all(np.isin(np.arange(q) * n + at + d_want * n * q, qid * n + tpos + dist * n * q))
        assert np.all(np.diff(qid) >= 0) and np.all(dist <= e)
        sample = rng.choice(qid.size, 1024, replace=False)
        assert X.true_hits(t, None, pats, e, (qid[sample], tpos[sample], dist[sample]))
        same = np.sum(t[tpos[:, None] + np.arange(m)[None, :]] != rows[qid], axis=1)
        assert np.array_equal(same, dist)
    finally:
        dev.close()
