"""The second and later trips of the grid-stride loops of psacx_kedit_dev_*: one text and a set at 4097 and 2^18 + 1 once more against
the host model with PSACX_OPT_GRID_CAP cutting every grid of grid_for() to 1 and to 3 workgroups, both index widths
(tests/test_gpu_grid_trips.py has the reasons and the fixture).  Every case states the workgroups its launches ask for -- a thread per
piece for the piece offsets, the search and the counts, a workgroup per 1024 candidates for the masks, a thread per candidate for the
raw pairs, a thread per raw hit for the marks of the unique, a thread per hit for the forward pass -- and sees psacx_stats.grid_cuts
rise across the call.  The batch is the case's own patterns several times over, more than 3 x 256 of them; the model runs them once
and its lists are laid one behind the other.  At 2^18 + 1 the text is the random one of 2 letters and the patterns those of 31 to
300 bytes: a piece of a repeat or of a few letters occurs n / 7 or n / 8 times there, which makes tens of millions of hits and
minutes of one workgroup, and the whole text is one lane walking 2^18 rows; all of these run at 4097.  The model is the pipeline
alone (by_pieces).

And once 128 patterns aa with e = 1 on a^4097: more than 2^20 candidates, so the scan of their counts takes the second chunk of its
block sums, and more than 2^21 raw hits, where the rank-pair sort changes from its look-back form to its three-kernel form
(SMALL_SORT_MAX = 2^21 in sort_scratch.hpp; the tandem repeat at 4097 above passes it too, with 2.7 million raw hits, the random text
stays below it with 1.3 million, and e = 15 in tests/test_gpu_kedit.py passes it once more)."""
import numpy as np
import pytest

import kedit_model as K
from kedit_gpu_common import BIG, KedIndex, check
from rmq_gpu_common import Dev
from test_gpu_grid_trips import OCC_TILE, asked, cap, ctx, cut, strides  # noqa: F401

pytestmark = pytest.mark.gpu


def several(case, e, shortest, longest):
    """(patterns, (quadruples, work)) of the case's patterns of shortest .. longest bytes, as often as gives more than 3 * 256 of them"""
    pats = [P for P in K.patterns(case, e) if shortest <= len(P) <= longest]
    reps = 3 * 256 // len(pats) + 1
    (qid, tpos, ln, dist), work = K.results(case, e, pats, (shortest, longest))
    want = (np.concatenate([qid + r * len(pats) for r in range(reps)]), np.tile(tpos, reps), np.tile(ln, reps), np.tile(dist, reps))
    return pats * reps, (want, (work[0] * reps, work[1] * reps))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("as_set", [False, True], ids=["text", "set"])
@pytest.mark.parametrize("kind,n", [("dna2", 4097), ("tandem7", 4097), ("dna2", BIG)])
def test_main_cases_with_cut_grids(ctx, cap, kind, n, as_set, bits):
    dev = Dev(ctx, bits)
    try:
        case = K.case(kind, n, as_set)
        pats, want = several(case, 2, *((31, 300) if n == BIG else (0, n + 1)))
        d = KedIndex(dev, case, pats, k=2 if as_set else 0)
        with cut(ctx):
            got, work = check(d, 2, (kind, n, as_set), want)
        strides(cap, asked(d.q), asked(work[0], OCC_TILE // 256), asked(work[0]), asked(work[1]), asked(got[0].size))
        with cut(ctx):
            check(d, 2, (kind, n, as_set, "best"), want, flags=1)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_two_million_raw_hits(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        n, q, e = 4097, 128, 1
        case = K.case("a", n)
        d = KedIndex(dev, case, [b"aa"] * q)
        (qid, tpos, ln, dist), work = d.run(e)
        # every piece a occurs n times; piece 0 at s reaches the starts s - 1 and s, piece 1 (t0 = s - 1) the starts s - 2 .. s, each
        # a hit where it is not below 0 (aa against a from n - 1 on: one deletion)
        assert work[0] == q * 2 * n > (1 << 20)
        assert work[1] == q * ((2 * n - 1) + (3 * n - 3)) > (1 << 21)
        assert np.array_equal(qid, np.repeat(np.arange(q), n)) and np.array_equal(tpos, np.tile(np.arange(n), q))
        assert np.array_equal(ln, np.tile(np.minimum(2, n - np.arange(n)), q)) and np.array_equal(dist, np.tile(np.arange(n) == n - 1, q))
        assert d.unchanged()
    finally:
        dev.close()
