#!/usr/bin/env python3
"""Time of the device-resident chain for a set of reads: tools/gst_time.py [log2 characters (28)] [index bits (32)] [coverage (16)] [repeats (3)].

The set: reads of 100..150 characters taken at random places of a random genome of n / coverage characters over ACGT, 2^log2
characters in all, laid back to back.  Reports the host-clock milliseconds (each call returns after the stream has drained) of
psacx_construct_gsa_dev_* with LCP, psacx_suffix_tree_gsa_dev_* into a table allocated before and psacx_check_suffix_tree_gsa_dev_*,
after one warm-up call each, with the verdicts of psacx_check_gsa_dev_* and of the tree checker; then, for comparison, the same
for the same bytes taken as ONE string (psacx_construct_dev_*, psacx_suffix_tree_dev_*, psacx_check_suffix_tree_dev_*: the
counterpart of tools/st_time.py), and the set's builder and checker on those one-string arrays with m = 1, which have the wider
row and the bitmap read but hardly a $-leaf.  Nothing but counters comes back to the host."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import psac_amd


def reads(n, coverage, seed=17):
    """(text, offsets): reads of 100..150 characters of a random genome, n characters in all (the last read is cut to fit)."""
    rng = np.random.RandomState(seed)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, max(n // coverage, 200))]
    lengths = rng.randint(100, 151, n // 100 + 1).astype(np.int64)
    ends = np.cumsum(lengths)
    m = int(np.searchsorted(ends, n)) + 1                   # the first m reads cover n characters
    lengths = lengths[:m]
    lengths[-1] -= int(ends[m - 1]) - n
    off = np.zeros(m + 1, np.uint64)
    off[1:] = np.cumsum(lengths)
    starts = rng.randint(0, genome.size - 150, m).astype(np.int64)
    at = np.repeat(starts - off[:-1].astype(np.int64), lengths) + np.arange(n, dtype=np.int64)
    return genome[at], off


def main():
    logn = int(sys.argv[1]) if len(sys.argv) > 1 else 28
    bits = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    coverage = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    n, w = 1 << logn, bits // 8
    text, off = reads(n, coverage)
    m = int(off.size - 1)
    ctx = psac_amd.Context(0)
    lib = ctx._lib
    d_text, d_off = ctx.alloc(n), ctx.alloc(off.size * 8)
    ctx.h2d(d_text, text); ctx.h2d(d_off, off)
    del text
    d_sa, d_isa, d_lcp = ctx.alloc(n * w), ctx.alloc(n * w), ctx.alloc(n * w)
    vp = C.c_void_p

    def timed(call):
        out = call()                                         # warm-up
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter(); out = call(); ms.append((time.perf_counter() - t0) * 1e3)
        return out, ms

    fmt = lambda v: " ".join("%.2f" % x for x in v)
    print("n = 2^%d = %d characters in %d reads of a %d-character genome, uint%d" % (logn, n, m, max(n // coverage, 200), bits))

    def construct_gsa():
        ctx._pre()
        ctx.check(getattr(lib, "psacx_construct_gsa_dev_u%d" % bits)(ctx.handle, vp(d_text), n, vp(d_off), m, 0, psac_amd.suffix_array.PSACX_LCP,
                                                                     vp(d_sa), vp(d_isa), vp(d_lcp)))

    # ---- the string set
    _, ms = timed(construct_gsa)
    print("psacx_construct_gsa_dev_u%d (SA + ISA + LCP)     ms: %s" % (bits, fmt(ms)))
    print("psacx_check_gsa_dev_u%d verdict %s" % (bits, psac_amd.check_gsa_device(ctx, d_text, n, d_off, m, d_sa, d_isa, d_lcp, bits)))
    sigma, _ = psac_amd.suffix_tree_gsa_device(ctx, d_text, n, None, 0, None, None, None, bits)
    table_bytes = n * (sigma + 2) * 8
    d_nodes = ctx.alloc(table_bytes)
    (sigma, edges), ms = timed(lambda: psac_amd.suffix_tree_gsa_device(ctx, d_text, n, d_off, m, d_sa, d_lcp, d_nodes, bits))
    print("psacx_suffix_tree_gsa_dev_u%d                    ms: %s   sigma %d, edges %d" % (bits, fmt(ms), sigma, edges))
    gout, ms = timed(lambda: psac_amd.check_suffix_tree_gsa_device(ctx, d_text, n, d_off, m, d_sa, d_lcp, d_nodes, bits))
    print("psacx_check_suffix_tree_gsa_dev_u%d              ms: %s   verdict %s" % (bits, fmt(ms), gout))
    print("node table: %d rows x %d cells x 8 = %d bytes (%.2f GiB), resident in HBM" % (n, sigma + 2, table_bytes, table_bytes / 2.0 ** 30))

    # ---- the same bytes as one string
    sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
    _, ms = timed(lambda: sa.construct_device(d_text, n, d_sa, d_isa, d_lcp))
    print("one string: psacx_construct_dev_u%d              ms: %s" % (bits, fmt(ms)))
    (sigma1, edges1), ms = timed(lambda: psac_amd.suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits))
    print("one string: psacx_suffix_tree_dev_u%d            ms: %s   sigma %d, edges %d" % (bits, fmt(ms), sigma1, edges1))
    out1, ms = timed(lambda: psac_amd.check_suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits))
    print("one string: psacx_check_suffix_tree_dev_u%d      ms: %s   verdict %s" % (bits, fmt(ms), out1))
    print("one string: node table %d rows x %d cells x 8 = %d bytes (%.2f GiB)" % (n, sigma1 + 1, n * (sigma1 + 1) * 8, n * (sigma1 + 1) * 8 / 2.0 ** 30))
    # ---- the set's builder and checker on those one-string arrays (m = 1: the wider row and the bitmap read, hardly a $-leaf)
    ctx.h2d(d_off, np.array([0, n], np.uint64))
    (_, edges2), ms = timed(lambda: psac_amd.suffix_tree_gsa_device(ctx, d_text, n, d_off, 1, d_sa, d_lcp, d_nodes, bits))
    print("one string as a set: psacx_suffix_tree_gsa_dev_u%d       ms: %s   edges %d" % (bits, fmt(ms), edges2))
    out2, ms = timed(lambda: psac_amd.check_suffix_tree_gsa_device(ctx, d_text, n, d_off, 1, d_sa, d_lcp, d_nodes, bits))
    print("one string as a set: psacx_check_suffix_tree_gsa_dev_u%d ms: %s   verdict %s" % (bits, fmt(ms), out2))
    for p in (d_text, d_off, d_sa, d_isa, d_lcp, d_nodes):
        ctx.free(p)
    ctx.close()
    ok = gout[:2] == [0, 0] and gout[2] == edges and out1[:2] == [0, 0] and out1[3] == edges1 and out2[:2] == [0, 0] and edges2 == edges1
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
