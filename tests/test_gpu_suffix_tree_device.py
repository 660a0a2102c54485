"""psacx_suffix_tree_dev_*: the suffix-tree node table built from arrays resident in HBM, against the oracle and against the
host-pointer entry point on the texts of tests/st_checker_model.py; the construct -> tree -> checker chain without a host copy
of anything but the final table (fetched here only to compare it); and `psac -t --resident`."""
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import st_checker_model as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", S.ALL)
def test_device_table_equals_oracle_and_host_entry_point(ctx, name, bits):
    import psac_amd
    text, SA, LCP, recs, table = S.arrays(name)
    dt = np.uint32 if bits == 32 else np.uint64
    sa, lcp = SA.astype(dt), LCP.astype(dt)
    n, w = int(text.size), bits // 8
    want = O.suffix_tree(text, sa, lcp)
    d_text, d_sa, d_lcp = ctx.alloc(n), ctx.alloc(n * w), ctx.alloc(n * w)
    d_nodes = None
    try:
        ctx.h2d(d_text, text); ctx.h2d(d_sa, sa); ctx.h2d(d_lcp, lcp)
        sigma, edges = psac_amd.suffix_tree_device(ctx, d_text, n, None, None, None, bits)         # the size query
        assert sigma == want.shape[1] - 1 and edges == 0
        d_nodes = ctx.alloc(n * (sigma + 1) * 8)
        ctx.h2d(d_nodes, np.full(n * (sigma + 1), 0xDEADBEEF, np.uint64))                          # (the call clears the table itself)
        assert psac_amd.suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits) == (sigma, int(np.count_nonzero(want)))
        got = np.empty((n, sigma + 1), np.uint64)
        ctx.d2h(got, d_nodes)
        assert np.array_equal(got, want)
        assert np.array_equal(psac_amd.suffix_tree(text, sa, lcp, ctx=ctx), want)            # the host-pointer entry point keeps its results
        # the inputs are byte-identical afterwards
        t2, s2, l2 = np.empty_like(text), np.empty_like(sa), np.empty_like(lcp)
        ctx.d2h(t2, d_text); ctx.d2h(s2, d_sa); ctx.d2h(l2, d_lcp)
        assert np.array_equal(t2, text) and np.array_equal(s2, sa) and np.array_equal(l2, lcp)
        R = int(recs[2].size)
        assert psac_amd.check_suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits) == [0, 0, R, R]
    finally:
        for p in (d_text, d_sa, d_lcp, d_nodes):
            if p:
                ctx.free(p)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["edge65", "edge4097", "mississippi", "tandem", "hub"])
def test_a_stored_lcp0_that_is_not_zero_is_read_as_zero(ctx, name, bits):
    # construct_device always stores LCP[0] = 0.  With a larger value there, the left search of every node directly under the
    # root answers "none" (nothing to its left is <= its depth any more): the builder takes parent 0 at depth 0 instead of indexing
    # LCP with "none".  As long as the stored value occurs nowhere else in LCP (an equal entry could end a furthest_eq search
    # early) the table is exactly the table of LCP[0] = 0, which the model states; the checker, which never uses the stored value,
    # agrees.  The values of an LCP array are downward closed (two suffixes that share k characters have successors that share
    # k - 1), so a value that occurs nowhere else lies above all of them: the largest + 1 and all ones.
    import psac_amd
    text, SA, LCP, recs, table = S.arrays(name)
    dt = np.uint32 if bits == 32 else np.uint64
    sa, lcp = SA.astype(dt), LCP.astype(dt)
    n, w = int(text.size), bits // 8
    want = O.suffix_tree(text, sa, lcp)
    d_text, d_sa, d_lcp = ctx.alloc(n), ctx.alloc(n * w), ctx.alloc(n * w)
    d_nodes = None
    try:
        ctx.h2d(d_text, text); ctx.h2d(d_sa, sa); ctx.h2d(d_lcp, lcp)
        sigma, edges = psac_amd.suffix_tree_device(ctx, d_text, n, None, None, None, bits)         # the size query
        assert sigma == want.shape[1] - 1 and edges == 0
        d_nodes = ctx.alloc(n * (sigma + 1) * 8)
        ctx.h2d(d_nodes, np.full(n * (sigma + 1), 0xDEADBEEF, np.uint64))                          # (the call clears the table itself)
        assert psac_amd.suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits) == (sigma, int(np.count_nonzero(want)))
        got = np.empty((n, sigma + 1), np.uint64)
        ctx.d2h(got, d_nodes)
        assert np.array_equal(got, want)
        assert np.array_equal(psac_amd.suffix_tree(text, sa, lcp, ctx=ctx), want)            # the host-pointer entry point keeps its results
        # the inputs are byte-identical afterwards
        t2, s2, l2 = np.empty_like(text), np.empty_like(sa), np.empty_like(lcp)
        ctx.d2h(t2, d_text); ctx.d2h(s2, d_sa); ctx.d2h(l2, d_lcp)
        assert np.array_equal(t2, text) and np.array_equal(s2, sa) and np.array_equal(l2, lcp)
        R = int(recs[2].size)
        assert psac_amd.check_suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits) == [0, 0, R, R]
    finally:
        for p in (d_text, d_sa, d_lcp, d_nodes):
            if p:
                ctx.free(p)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["edge65", "edge4097", "mississippi", "tandem", "hub"])
def test_a_stored_lcp0_that_is_not_zero_is_read_as_zero(ctx, name, bits):
    # construct_device always stores LCP[0] = 0.  With another value there, every left search whose value lies below it answers
    # "none" and every one above it answers 0: the builder takes parent 0 at depth 0 for both instead of indexing LCP with "none"
    # or using the stored value.  As long as the stored value occurs nowhere else in LCP (an equal entry could end a furthest_eq
    # search early) the table is exactly the table of LCP[0] = 0, which the model states; the checker, which never uses the
    # stored value, agrees.  Two values: one above every entry (all left searches of depth-1 nodes end in "none") and one inside
    # the range of the entries where the text leaves a gap.
    import psac_amd
    text, SA, LCP, recs, table = S.arrays(name)
    dt = np.uint32 if bits == 32 else np.uint64
    n, w, R = int(text.size), bits // 8, int(recs[2].size)
    d_text, d_sa, d_lcp, d_nodes = ctx.alloc(n), ctx.alloc(n * w), ctx.alloc(n * w), ctx.alloc(table.size * 8)
    try:
        ctx.h2d(d_text, text); ctx.h2d(d_sa, SA.astype(dt))
        for v in [int(LCP.max()) + 1, int(np.iinfo(dt).max)]:
            lcp = LCP.astype(dt)
            lcp[0] = v
            ctx.h2d(d_lcp, lcp)
            assert psac_amd.suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits) == (table.shape[1] - 1, R), v
            got = np.empty_like(table)
            ctx.d2h(got, d_nodes)
            assert np.array_equal(got, table), v
            assert psac_amd.check_suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits) == [0, 0, R, R], v
    finally:
        for p in (d_text, d_sa, d_lcp, d_nodes):
            ctx.free(p)


def test_chain_construct_tree_checker_in_hbm(ctx):
    # 2^20 random DNA characters, 64-bit: nothing leaves the device between the three calls
    import inputs
    import psac_amd
    n = 1 << 20
    text = inputs.dna(n, 21)
    d_text, d_sa, d_isa, d_lcp = ctx.alloc(n), ctx.alloc(n * 8), ctx.alloc(n * 8), ctx.alloc(n * 8)
    d_nodes = None
    try:
        ctx.h2d(d_text, text)
        sa = psac_amd.SuffixArray(index_bits=64, lcp=True, ctx=ctx)
        sa.construct_device(d_text, n, d_sa, d_isa, d_lcp)
        sigma, _ = psac_amd.suffix_tree_device(ctx, d_text, n, None, None, None, 64)
        assert sigma == 4
        d_nodes = ctx.alloc(n * 5 * 8)
        sigma, edges = psac_amd.suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, 64)
        assert psac_amd.check_device(ctx, d_text, n, d_sa, d_isa, d_lcp, 64) == [0, 0, 0, 0]
        assert psac_amd.check_suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, 64) == [0, 0, edges, edges]
        ref = O.construct(text, bits=64)
        want = O.suffix_tree(text, ref["SA"], ref["LCP"])
        got = np.empty((n, 5), np.uint64)
        ctx.d2h(got, d_nodes)
        assert np.array_equal(got, want) and edges == int(np.count_nonzero(want))
    finally:
        for p in (d_text, d_sa, d_isa, d_lcp, d_nodes):
            if p:
                ctx.free(p)


def test_psac_resident_tree_cli():
    psac = os.path.join(ROOT, "psac_amd", "bin", "psac")
    plain = subprocess.run([psac, "-t", "-r", "100000"], capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    r = subprocess.run([psac, "-t", "--resident", "-c", "-r", "100000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "[SUCCESS] Suffix Tree is correct" in r.stderr and "[SUCCESS] Suffix Array and LCP are correct" in r.stderr
    for line in ("SA time: ", "ST time: ", "Total  : "):
        assert line in r.stderr
    edges = [re.search(r"ST edges: (\d+)", x.stderr).group(1) for x in (plain, r)]
    assert edges[0] == edges[1] and int(edges[0]) > 100000
    # -o with --resident is an error, as -t -o is
    assert subprocess.run([psac, "-t", "--resident", "-o", "x", "-r", "1000"], capture_output=True).returncode != 0
