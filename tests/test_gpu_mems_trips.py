"""The second and later trips of the grid-stride loops of psacx_mems_dev_*: the one-text and set cases at 4097 and 2^18 + 1 once more
against the host model with PSACX_OPT_GRID_CAP cutting every grid of grid_for() to 1 and to 3 workgroups, both index widths
(tests/test_gpu_grid_trips.py has the reasons and the fixture).  Every case states the workgroups its launches ask for -- sixteen
lanes per slot for the two walks, a workgroup per 1024 candidates for the marks, the tile counts and the triples, a thread per slot
and a workgroup per 1024 ranks for PSACX_MEMS_SUPER -- and sees psacx_stats.grid_cuts rise across the call."""
import pytest

import mems_model as X
from mems_gpu_common import BIG, MemsIndex, check, patterns_of
from repeats_gpu_common import set_case, text_case
from rmq_gpu_common import Dev
from test_gpu_grid_trips import LANES, OCC_TILE, asked, cap, ctx, cut, strides  # noqa: F401
from test_gpu_mems import set_patterns

pytestmark = pytest.mark.gpu


def trips(ctx, cap, d, key, what, min_len, max_occ=0, marks=True, ranks=True):
    """marks / ranks: the shape has candidates / kept ranks for more tiles of 1024 than the cap allows workgroups (where it has not,
    the launches over them do not stride and only the walk, or the count of the kept slots, does)"""
    with cut(ctx):
        _, work = check(d, key, what, min_len, max_occ)
    strides(cap, asked((d.S + 1) * LANES))
    if marks:
        strides(cap, asked(work[1], OCC_TILE // 256))
    with cut(ctx):
        _, work = check(d, key, (what, "super"), min_len, max_occ, X.SUPER)
    strides(cap, asked(d.S + 1))
    if ranks:
        strides(cap, asked(work[1], OCC_TILE // 256))
    assert d.unchanged()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [4097, BIG])
@pytest.mark.parametrize("kind", ["dna2", "tandem7"])
def test_one_text(ctx, cap, kind, n, bits):
    dev = Dev(ctx, bits)
    try:
        case = text_case(kind, n)
        d = MemsIndex(dev, case, patterns_of(kind, case.text, whole=False) * (2 if kind == "dna2" else 16))
        if kind == "dna2":                                  # (few slots are kept: 772 ranks at 4097, 18 at 2^18 + 1)
            trips(ctx, cap, d, ("trips", kind, n), (kind, n), 4 if n == 4097 else 10, ranks=False)
        elif n == 4097:                                     # repetitive: short pieces, about 1.4 million candidates
            trips(ctx, cap, d, ("trips", kind, n), (kind, n), 1)
        else:                                               # every piece occurs n / 7 times: max_occ ends every walk at once
            trips(ctx, cap, d, ("trips", kind, n), (kind, n), 1, 8, marks=False, ranks=False)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["random2", "acgt3000"])
def test_string_set(ctx, cap, name, bits):
    dev = Dev(ctx, bits)
    try:
        case = set_case(name)
        d = MemsIndex(dev, case, set_patterns(case) * 2)
        trips(ctx, cap, d, ("trips", name), name, 2 if name == "random2" else 1, ranks=name != "random2")
    finally:
        dev.close()
