#!/usr/bin/env python3
"""Time of the device-resident suffix-tree chain: tools/st_time.py [log2 characters (28)] [index bits (32)] [kind (dna)] [repeats (3)].

kind: dna | ascii | tandem | mutated (psacx_synth_text_dev kinds 0..3, period 1024), generated in HBM.  Reports the host-clock
milliseconds (each call returns after the stream has drained) of psacx_construct_dev_* with LCP, psacx_suffix_tree_dev_* into a
table allocated before, and psacx_check_suffix_tree_dev_*, after one warm-up call each; the verdicts of psacx_check_dev_* and of
the tree checker; and the bytes the table occupies.  Nothing but counters comes back to the host."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import psac_amd

KINDS = {"dna": 0, "ascii": 1, "tandem": 2, "mutated": 3}


def main():
    logn = int(sys.argv[1]) if len(sys.argv) > 1 else 28
    bits = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    kind = sys.argv[3] if len(sys.argv) > 3 else "dna"
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    n, w = 1 << logn, bits // 8
    ctx = psac_amd.Context(0)
    d_text = ctx.alloc(n)
    ctx.check(ctx._lib.psacx_synth_text_dev(ctx.handle, C.c_void_p(d_text), n, 0, KINDS[kind], 17, 1024))
    d_sa, d_isa, d_lcp = ctx.alloc(n * w), ctx.alloc(n * w), ctx.alloc(n * w)
    sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)

    def timed(call):
        out = call()                                         # warm-up
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter(); out = call(); ms.append((time.perf_counter() - t0) * 1e3)
        return out, ms

    fmt = lambda v: " ".join("%.2f" % x for x in v)
    print("n = 2^%d = %d characters of %s, uint%d" % (logn, n, kind, bits))
    _, ms = timed(lambda: sa.construct_device(d_text, n, d_sa, d_isa, d_lcp))
    print("psacx_construct_dev_u%d (SA + ISA + LCP)   ms: %s" % (bits, fmt(ms)))
    sigma, _ = psac_amd.suffix_tree_device(ctx, d_text, n, None, None, None, bits)
    table_bytes = n * (sigma + 1) * 8
    d_nodes = ctx.alloc(table_bytes)
    (sigma, edges), ms = timed(lambda: psac_amd.suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits))
    print("psacx_suffix_tree_dev_u%d                  ms: %s   sigma %d, edges %d" % (bits, fmt(ms), sigma, edges))
    out, ms = timed(lambda: psac_amd.check_suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, bits))
    print("psacx_check_suffix_tree_dev_u%d            ms: %s   verdict %s" % (bits, fmt(ms), out))
    print("psacx_check_dev_u%d verdict %s" % (bits, psac_amd.check_device(ctx, d_text, n, d_sa, d_isa, d_lcp, bits)))
    print("node table: %d rows x %d cells x 8 = %d bytes (%.2f GiB), resident in HBM" % (n, sigma + 1, table_bytes, table_bytes / 2.0 ** 30))
    for p in (d_text, d_sa, d_isa, d_lcp, d_nodes):
        ctx.free(p)
    ctx.close()
    return 0 if out[:2] == [0, 0] and out[3] == edges else 1


if __name__ == "__main__":
    sys.exit(main())
