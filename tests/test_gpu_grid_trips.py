"""The second and later trips of the query layer's grid-stride loops: every query call once more against its host model, with
PSACX_OPT_GRID_CAP cutting every grid of grid_for() to 1 and to 3 workgroups, both index widths.

At the default bound of 8 or 16 workgroups per CU no shape the suite can afford makes these loops stride (their second trip
begins between 2^15 patterns and 2^23 characters), while the shapes the calls are made for take hundreds of trips.  With cap 1 one
workgroup takes every trip of a launch in sequence -- state it leaves in LDS or in registers meets the next trip, and its four
waves take different numbers of trips of the wave-stride loops --; with cap 3 the stride divides no tile count here and the last
trip leaves some workgroups without work.  Every case
  - states, by plain arithmetic from its shape, the workgroups the launches it is about ask for (asked(): items / 256), more than
    the cap, and at cap 1 three or more (strides());
  - sees psacx_stats.grid_cuts rise across the call (cut());
  - compares the outputs with the host model the call's own test file uses, through that file's helpers, which keep their
    sentinel / PAD / inputs-unchanged checks.
Where a launch of the call does not reach the arithmetic at the shape used, the case says so.  The fixture `cap` sets the option as
the suite sets every option: the variable PSACX_GRID_CAP for the debug shim the wrappers call, and ctx.configure.

Not run under a cap: psacx_construct_* and everything of the sorter and the multi-GPU engine (kernels there wait for other
workgroups).  The ANSV kernels inside psacx_lpf_dev_* and the suffix-tree builders size their grids themselves, not through
grid_for(), so the cap does not reach them."""
import numpy as np
import pytest

import gst_model as T
import inputs
import lce_model as E
import locate_gsa_model as G
import locate_model as L
import lz_model as Z
import match_model as M
import overlaps_model as V
import repeats_model as R
import rmq_model as Q
import st_checker_model as S
from lz_gpu_common import LzIndex, Parse, from_model
from match_gpu_common import Index, first_difference, total_holds
from repeats_gpu_common import Case, RepIndex, agree, set_case, text_case
from rmq_gpu_common import Dev, Indexed, LceIndex, Ranges, first_bad

pytestmark = pytest.mark.gpu

CAPS = (1, 3)
LANES = 16                      # rmq.hpp: RMQ_LANES, the lanes per query, rank or string of the kernels over the index of LCP
STRIP = 16                      # lookup_table.hpp: LOCATE_STRIP, the text positions of a thread of kmer_count_kernel
LDS_BINS = 4096                 # lookup_table.hpp: LOCATE_LDS_BINS, tables up to this many entries are counted in LDS
OCC_TILE = 1024                 # occurrences.hpp: output slots of a workgroup of occ_expand_kernel
SELECT_TILE = 1024              # repeats.hpp: REP_TILE, and the default tile of the LZ77 parse


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(params=CAPS, ids=lambda v: "cap%d" % v)
def cap(request, ctx, monkeypatch):
    monkeypatch.setenv("PSACX_GRID_CAP", str(request.param))     # (the wrappers configure from the environment under the test suite)
    ctx.configure(grid_cap=request.param)
    yield request.param
    ctx.configure(grid_cap=0)


@pytest.fixture
def small_tiles(ctx, monkeypatch):
    monkeypatch.setenv("PSACX_LZ_SMALL_TILES", "1")
    ctx.configure(lz_small_tiles=1)
    yield
    ctx.configure(lz_small_tiles=0)


def asked(items, per=1):
    """the workgroups of 256 threads grid_for() is asked for: one thread per `per` items"""
    return max(1, -(-(-(-int(items) // per)) // 256))


def strides(cap, *groups):
    """every launch named asks for more workgroups than the cap, and a workgroup alone takes three trips or more"""
    for g in groups:
        assert g > cap and (cap > 1 or g >= 3), (cap, groups)


class cut(object):
    """with cut(ctx): the calls inside launched at least one grid smaller than asked for"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.before = int(self.ctx.stats().grid_cuts)
        return self

    def __exit__(self, kind, value, tb):
        if kind is None:
            assert int(self.ctx.stats().grid_cuts) > self.before
        return False


# ---------------------------------------------------------------------------------------------------------------
# lookup table, locate, match: 12 300 characters of DNA (769 strips of 16: 4 workgroups), one text and cut into strings
# ---------------------------------------------------------------------------------------------------------------
N_DNA = 12300
TEXT, SET = "dna12300", "dna12300_set"


def names():
    text = inputs.dna(N_DNA, 41)
    L.add_text(TEXT, text)
    cuts = np.sort(np.random.RandomState(42).choice(np.arange(1, N_DNA), 119, replace=False))      # 120 strings of 1 .. some hundred characters
    G.add_set(SET, np.split(text, cuts))
    return TEXT, SET


def index_of(ctx, kind, bits):
    text, sset = names()
    return Index(ctx, sset, bits, set=True) if kind == "set" else Index(ctx, text, bits)


def repeated(pats, *answers):
    """the catalogue's list repeated until it has more than 3 * 256 patterns, and the model's answers with it"""
    reps = -(-(3 * 256 + 1) // len(pats))
    return (pats * reps,) + tuple(np.tile(a, reps) for a in answers)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["text", "set"])
def test_lookup_table(ctx, cap, kind, bits):
    d = index_of(ctx, kind, bits)
    try:
        assert d.n >= STRIP * 256 * 3 + 1
        strides(cap, asked(d.n, STRIP))                                   # kmer_count_kernel (and the character histogram in front of it)
        B = L.codes_of(d.text)[1] + 1
        ks = (1, 2, L.smallest_k_above(B, LDS_BINS - 1))
        assert [B ** k + 1 > LDS_BINS for k in ks] == [False, False, True]          # bins in LDS twice, global atomics once
        for k in ks:
            with cut(ctx):
                table = d.table(k)[1]
            want = G.table_by_definition(d.text, d.off, k) if d.set else L.table_by_definition(d.text, k)
            assert table.size == B ** k + 1 and np.array_equal(table.astype(np.int64), want), k
        assert d.inputs_unchanged()
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["text", "set"])
def test_locate(ctx, cap, kind, bits, monkeypatch):
    d = index_of(ctx, kind, bits)
    try:
        pats, lb, ub = repeated(*(G.expected(SET) if d.set else L.expected(TEXT)))
        b = d.batch(pats)
        strides(cap, asked(b.q))                                          # search_offsets_kernel, and locate_kernel in the lane shape
        for table in (None, d.table(2)[0]):
            for shape in ("lane",) if d.set else ("lane", "group"):
                monkeypatch.setenv("PSACX_LOCATE_SHAPE", shape)
                if shape == "group":
                    strides(cap, asked(8 * b.q))
                with cut(ctx):
                    got = d.locate(b, table)
                bad = first_difference((got[0], got[0], got[1]), (lb, lb, ub), pats)
                assert bad is None, (shape, table and table[1], bad)
        assert d.inputs_unchanged([b])
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["text", "set"])
def test_match(ctx, cap, kind, bits):
    d = index_of(ctx, kind, bits)
    try:
        SA = G.arrays(SET)[2] if d.set else L.sa_of(TEXT)
        expected = (lambda max_len=0: M.expected_gsa(SET, max_len)) if d.set else (lambda max_len=0: M.expected(TEXT, max_len))
        pats, ln, lb, ub = repeated(*expected())
        b = d.batch(pats)
        strides(cap, asked(b.q))                                          # search_offsets_kernel and match_kernel, a lane per query
        pieces = M.pieces_of(d.text)                                      # the suffix mode: a lane per byte of the pattern buffer
        bp = d.batch(pieces)
        strides(cap, asked(bp.total))
        queries = M.queries_of(pieces, True)
        want_suffixes = M.answers(("pieces", SET if d.set else TEXT, 0), queries, d.text, SA, d.off)
        for table in (None, d.table(2)[0]):
            k = table and table[1]
            with cut(ctx):
                got = d.match(b, table)
            assert first_difference(got, (ln, lb, ub), pats) is None and total_holds(got, pats, d.n), k
            with cut(ctx):
                got = d.match(b, table, max_len=8)
            assert first_difference(got, repeated(*expected(8))[1:], pats) is None and np.all(got[0] <= 8), k
            with cut(ctx):
                got = d.match(bp, table, suffixes=True)
            assert first_difference(got, want_suffixes, queries) is None, k
        assert d.inputs_unchanged([b, bp])
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_malformed_offsets_are_refused_in_a_later_trip(ctx, cap, bits):
    # the one wrong offset lies in the last 256 of more than 3 * 256: in the fourth trip of the one workgroup, in the second of the
    # first of three
    import psac_amd
    d = index_of(ctx, "text", bits)
    try:
        pats = [b"AC", b"", b"CCA", b"A"] * 200
        good = psac_amd.pattern_buffer(pats)[1]
        strides(cap, asked(len(pats)))
        table = d.table(2)[0]
        for what in ("descending", "descending_last"):
            off = good.copy()
            if what == "descending":
                off[790], off[791] = off[791], off[790]
            else:
                off[-1] = off[-2] - 1
            b = d.batch(pats, off)
            for tb in (None, table):
                for call in (lambda: d.match(b, tb), lambda: d.locate(b, tb)):
                    with cut(ctx):
                        with pytest.raises(psac_amd.PsacxError) as e:
                            call()
                    assert e.value.code == -1
                d.match(d.batch(pats), tb)                                # (a correct batch afterwards is taken)
                with pytest.raises(psac_amd.PsacxError):
                    d.match(b, tb)
                assert d.untouched()                                      # nothing was written before the refusal
    finally:
        d.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_fetch_counters_do_not_depend_on_the_grid(ctx, cap, bits, monkeypatch):
    # The counters of PSACX_LOCATE_COUNT are sums of per-lane counts, added up once per lane after its last trip: on the catalogue's
    # own lists they equal tests/golden/query_fetches.json whatever the grid.  The lists are as long as they are: the text edge4097
    # has 479 patterns, two workgroups in the lane shape, so cap 3 cuts its group shape (15 workgroups) and its suffix mode (a lane
    # per byte) only, and cap 1 every launch; the set `prefixes` has 799, four workgroups.
    import json
    from test_gpu_query_fetches import GOLDEN, check, plain_cases, set_cases
    with open(GOLDEN) as f:
        golden = json.load(f)
    monkeypatch.setenv("PSACX_LOCATE_COUNT", "1")
    assert asked(8 * len(L.patterns_of("edge4097"))) > cap
    strides(cap, asked(len(G.patterns_of("prefixes"))))
    with cut(ctx):
        got = plain_cases(ctx, "edge4097", bits)
    with cut(ctx):
        got.update(set_cases(ctx, "prefixes", bits))
    assert len(got) == 14
    check(got, golden)


# ---------------------------------------------------------------------------------------------------------------
# occurrence lists
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
def test_occurrences(ctx, cap, bits):
    from test_gpu_occurrences import FILL, HAND_N, HAND_OFF, Occ, hand_made_batches
    n = HAND_N
    o = Occ(ctx, np.arange(n, dtype=np.uint64)[::-1].copy(), n, HAND_OFF, bits)
    try:
        for lb, ub, limit, by_hand in hand_made_batches():                # with the string ids; check(): the model's start, pos and sid
            total = o.check(lb, ub, limit)
            assert by_hand is None or total == by_hand
        # one interval over every tile and one over all but seven slots: 8 output tiles of occ_expand_kernel
        strides(cap, asked(2 * n - 7, OCC_TILE // 256))
        with cut(ctx):
            assert o.check([0, 7], [n, n]) == 2 * n - 7
        # more than 3 * 256 intervals: occ_counts_kernel, a thread per entry of start[]
        rng = np.random.RandomState(3)
        lb = rng.randint(0, n, 3 * 256 + 200)
        ub = np.minimum(n, lb + rng.choice([0, 1, 2, 9, 70], lb.size))
        want = G.occurrences(o.sa, n, lb, ub)
        strides(cap, asked(lb.size + 1), asked(int(want[0][-1]), OCC_TILE // 256))
        for limit in (0, 3):
            with cut(ctx):
                o.check(lb, ub, limit)
        with cut(ctx):                                                    # the size query
            assert o.run(lb, ub, query=True)[0] == int(want[0][-1])
        assert np.array_equal(o.start, want[0]) and np.all(o.pos == FILL) and np.all(o.sid == FILL)
        with cut(ctx):                                                    # without string ids
            total = o.run(lb, ub, sid=False, offsets=False)[0]
        assert np.array_equal(o.pos[:total].astype(np.uint64), want[1]) and np.all(o.pos[total:] == FILL) and np.all(o.sid == FILL)
    finally:
        o.close()


# ---------------------------------------------------------------------------------------------------------------
# BWT, the rank directories (through the repeats that read them) and the repeats
# ---------------------------------------------------------------------------------------------------------------
_sets = {}


def rep_case(which):
    """texts and sets of 4097 characters and of 4095 = 63 (mod 64): 65 and 64 chunks of 64 ranks, which the four waves of one
    workgroup, and the twelve of three, do not share evenly"""
    if which.startswith("text"):
        return text_case("planted" if which == "text4097" else "dna4", int(which[4:]))
    if which == "set4097":
        return set_case("random2")
    if which not in _sets:
        _sets[which] = Case(R.random_set(4095, 300, 14), False)
    return _sets[which]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("which", ["text4097", "text4095", "set4097", "set4095"])
def test_bwt_and_repeats(ctx, cap, which, bits):
    case = rep_case(which)
    n = case.n
    assert n == int(which[-4:]) and (n % 64 == 63 or n == 4097)
    dev = Dev(ctx, bits)
    try:
        # bwt_kernel, bwt_change_kernel, lcp_step_kernel: a lane per rank; repeats_kernel: 16 lanes per rank; select_count_kernel and
        # select_emit_kernel: a workgroup per tile of 1024 ranks; pyramid_level_kernel of level 1 (the index build): a lane per value
        strides(cap, asked(n + 64), asked(n * LANES), asked(-(-n // SELECT_TILE) * 256), asked(-(-n // 64) * 64))
        with cut(ctx):
            d = RepIndex(dev, case)
        with cut(ctx):
            bwt, first, primary = d.run_bwt()
        assert np.array_equal(bwt, case.bwt) and np.array_equal(first, case.first_words()) and primary == case.primary
        for kind in (R.RIGHT, R.MAXIMAL, R.SUPER):
            with cut(ctx):
                got = d.run(kind)                                         # (run: the count query, then the lists)
            agree(got, case.results(kind), (which, kind))
            with cut(ctx):
                got = d.run(kind, min_len=3, min_occ=3)
            agree(got, R.select(case.results(kind), min_len=3, min_occ=3), (which, kind, "filtered"))
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("min_len", [1023, 1024, 1025, 2048])
def test_first_selected_rank_at_a_tile_edge(ctx, cap, min_len, bits):
    # a^2049 as in tests/test_gpu_repeats.py: three tiles of the compaction.  With cap 1 the one workgroup passes over the tiles
    # without a selected rank and emits in a later trip; with cap 3 every workgroup of the compaction takes one tile, and what
    # strides is repeats_kernel and the kernels of the directories.
    n = 2049
    dev = Dev(ctx, bits)
    try:
        strides(cap, asked(n * LANES), asked(n + 64))
        if cap == 1:
            strides(cap, asked(-(-n // SELECT_TILE) * 256))
        case = text_case("a", n)
        d = RepIndex(dev, case)
        d.run_bwt()
        for kind in (R.RIGHT, R.MAXIMAL):
            want = R.select(case.results(kind), min_len=min_len)
            with cut(ctx):
                assert d.count(kind, min_len=min_len) == len(want) == n - min_len
            with cut(ctx):
                agree(d.run(kind, min_len=min_len), want, (kind, min_len))
        assert d.unchanged()
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------
# range-minimum index, rmq, lce, overlaps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("n", [4097, 3 * 64 * 256 + 65])
def test_rmq_index_and_queries(ctx, cap, n, bits):
    # n = 4097: pyramid_level_kernel of level 1 asks for 17 workgroups, pyramid_aux_kernel (a lane per entry of a level, 65 here) for
    # one; at 3 * 64 * 256 + 65 values level 1 has 769 entries and pyramid_aux_kernel strides too
    from test_gpu_rmq import big_ranges, families
    dev = Dev(ctx, bits)
    try:
        lo, hi = big_ranges(n)
        r = Ranges(dev, lo[:6000], hi[:6000])
        strides(cap, asked(-(-n // 64) * 64), asked(r.q * LANES))
        if n > 4097:
            strides(cap, asked(-(-n // 64)))
        fam = families(n, bits)
        for name in ("three", "runs01", "ones_but_one"):
            with cut(ctx):
                a = Indexed(dev, fam[name])
            with cut(ctx):
                got = a.rmq(r)
            want = Q.Table(a.v).queries(r.lo, r.hi)
            assert first_bad(got[0], want[0]) is None and first_bad(got[1], want[1]) is None, name
            assert a.unchanged()
        assert r.unchanged(dev)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["text", "set"])
def test_lce(ctx, cap, kind, bits):
    from test_gpu_lce import agree as lce_agree, pairs_of_set, pairs_of_text
    name = "edge4097"
    dev = Dev(ctx, bits)
    try:
        if kind == "text":
            text, SA, ISA, LCP = E.arrays(name)
            off, (a, b) = None, pairs_of_text(int(text.size), SA)
        else:
            text, off, SA, ISA, LCP = E.set_arrays(name)
            a, b = pairs_of_set(text, off, SA)
        assert text.size == 4097
        strides(cap, asked(a.size * LANES))
        d = LceIndex(dev, ISA, LCP, off)
        for e in (0, 2):
            with cut(ctx):
                lce_agree(d, text, off, a, b, e)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["reads", "copies300"])
def test_overlaps(ctx, cap, name, bits):
    # 512 reads of 64 bytes and 300 copies of one string: more than 3 * 16 strings, 16 lanes each
    from test_gpu_overlaps import OverlapIndex, agree as overlaps_agree
    text, off, SA, ISA, LCP = V.set_arrays(name)
    dev = Dev(ctx, bits)
    try:
        d = OverlapIndex(dev, off, SA, ISA, LCP)
        assert d.m > 3 * 16
        strides(cap, asked(d.m * LANES))
        for whole in (False, True):
            for min_len in ([16] if name == "reads" else V.min_lens(name)):
                with cut(ctx):
                    lb, ub = overlaps_agree(d, name, min_len, whole)
                assert name != "reads" or np.count_nonzero(ub > lb) > 0               # (an all-zero result cannot pass)
        assert d.unchanged()
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------
# lpf, lz77 and its checker
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["dna4096", "tandem3000"])
def test_lpf_and_parse_of_the_named_texts(ctx, cap, name, bits):
    # lpf_kernel: 16 lanes per rank.  The parse at the default geometry has one group of 2^17 positions, so lz_exit_kernel and
    # lz_mark_kernel ask for one workgroup (the next test makes them stride); select_emit_kernel takes a tile of 1024 positions per
    # workgroup: four for dna4096, three for tandem3000
    from test_gpu_lz77 import agree as lz_agree
    t, SA, LCP = Z.arrays(name)
    n = int(t.size)
    dev = Dev(ctx, bits)
    try:
        strides(cap, asked(n * LANES))
        parse_strides = name == "dna4096" or cap == 1                     # (three tiles under cap 3: the parse of tandem3000 runs as ever)
        if parse_strides:
            strides(cap, asked(-(-n // SELECT_TILE) * 256))
        with cut(ctx):
            d = LzIndex(dev, SA, LCP)
        with cut(ctx):
            out = d.lpf()
        lz_agree(dev, out, Z.lpf_of(name), name)
        assert d.unchanged()
        before = int(ctx.stats().grid_cuts)
        start, psrc = Parse(dev, *out).run()
        assert (int(ctx.stats().grid_cuts) > before) == parse_strides
        want = Z.parse_of(name)
        assert np.array_equal(start, want[0]) and np.array_equal(psrc, want[1])
        g = Z.golden()[name]
        assert start.tolist() == g["start"] and psrc.tolist() == g["src"]
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", Z.SYNTHETIC)
def test_parse_of_5000_values_with_small_tiles(ctx, cap, small_tiles, kind, bits):
    # tiles of 64 in groups of 4: 20 groups, a workgroup each in lz_exit_kernel and lz_mark_kernel, and 79 tiles of the compaction
    from test_gpu_lz77 import SMALL_B, SMALL_G, parse_equals_the_chain
    n = 5000
    strides(cap, asked(-(-n // (SMALL_B * SMALL_G)) * 256), asked(-(-n // SMALL_B) * 256))
    with cut(ctx):
        parse_equals_the_chain(ctx, bits, kind, n, SMALL_B)


@pytest.mark.parametrize("bits", [32, 64])
def test_parse_with_sources_and_small_tiles(ctx, cap, small_tiles, bits):
    dev = Dev(ctx, bits)
    try:
        for name in ("tandem3000", "dna4096"):
            lpf, src = Z.lpf_of(name)
            strides(cap, asked(-(-lpf.size // 256) * 256))
            with cut(ctx):
                start, psrc = Parse(dev, lpf, from_model(dev, src)).run()
            want = Z.parse_of(name)
            assert np.array_equal(start, want[0]) and np.array_equal(psrc, want[1]), name
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["dna4096", "tandem3000"])
def test_lz77_checker(ctx, cap, name, bits):
    # check_lz77_kernel: a thread per text position and phrase; its count is the model's, on the right parse and on every wrong one
    from test_gpu_lz77_verifier import device_count, mutations
    t = Z.text_of(name)
    dev = Dev(ctx, bits)
    try:
        strides(cap, asked(t.size + 1))
        start, src = Z.parse_of(name)
        with cut(ctx):
            assert device_count(dev, t, start, src) == 0 == Z.check_count(t, start, src)
        for what, s, p in mutations(t, start, src):
            want = Z.check_count(t, s, p)
            with cut(ctx):
                assert device_count(dev, t, s, p) == want > 0, (name, what)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------
# suffix tree and generalized suffix tree: the builders and their device checkers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["edge4097", "tandem"])
def test_suffix_tree_builder_and_checker(ctx, cap, name, bits):
    # st_nodes_kernel and st_check_kernel: a thread per LCP index; count_nonzero_kernel: a thread per two cells
    import psac_amd
    from test_gpu_st_verifier import table_case, table_recipes
    text, SA, LCP, recs, table = S.arrays(name)
    dt = np.uint32 if bits == 32 else np.uint64
    sa, lcp = SA.astype(dt), LCP.astype(dt)
    n, w, R = int(text.size), bits // 8, int(recs[2].size)
    strides(cap, asked(n), asked(n * table.shape[1] // 2 + 1))
    d_text, d_sa, d_lcp, d_nodes = ctx.alloc(n), ctx.alloc(n * w), ctx.alloc(n * w), ctx.alloc(table.size * 8)
    try:
        ctx.h2d(d_text, text); ctx.h2d(d_sa, sa); ctx.h2d(d_lcp, lcp)
        ctx.h2d(d_nodes, np.full(table.size, 0xDEADBEEF, np.uint64))                               # (the call clears the table itself)
        with cut(ctx):
            assert psac_amd.suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits) == (table.shape[1] - 1, R)
        got = np.empty_like(table)
        ctx.d2h(got, d_nodes)
        assert np.array_equal(got, table)
        with cut(ctx):
            assert psac_amd.check_suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits) == [0, 0, R, R]
        wrong, done, want = table_case(name, 0, table_recipes(name)[0])
        assert done and want[0] + want[1] > 0 and want[2] == R
        ctx.h2d(d_nodes, wrong)
        with cut(ctx):
            assert psac_amd.check_suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits) == want
        t2, s2, l2 = np.empty_like(text), np.empty_like(sa), np.empty_like(lcp)
        ctx.d2h(t2, d_text); ctx.d2h(s2, d_sa); ctx.d2h(l2, d_lcp)
        assert np.array_equal(t2, text) and np.array_equal(s2, sa) and np.array_equal(l2, lcp)
    finally:
        for p in (d_text, d_sa, d_lcp, d_nodes):
            ctx.free(p)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["edge4097", "copies"])
def test_generalized_suffix_tree_builder_and_checker(ctx, cap, name, bits):
    from test_gpu_gst import Dev as Gst
    from test_gpu_gst_verifier import table_recipes
    text, off, SA, LCP, recs, table = T.arrays(name)
    n, R, cells = int(text.size), int(recs[2].size), int(np.count_nonzero(table))
    strides(cap, asked(n), asked(n * table.shape[1] // 2 + 1))
    g = Gst(ctx, text, off, SA, LCP, bits, table.size)
    try:
        ctx.h2d(g.nodes, np.full(table.size, 0xDEADBEEF, np.uint64))
        with cut(ctx):
            assert g.build() == (table.shape[1] - 2, R)
        got = g.table(table.shape)
        assert np.array_equal(got, table), np.argwhere(got != table)[:5]
        with cut(ctx):
            assert g.check() == [0, 0, R, cells]
        wrong, done = T.mutate_table(table_recipes(name)[0], table, T.head_of(name), recs)
        want = T.expect(text, off, SA, LCP, wrong, recs)
        assert done and want[0] + want[1] > 0 and want[2] == R
        ctx.h2d(g.nodes, wrong)
        with cut(ctx):
            assert g.check() == want
    finally:
        g.close()
