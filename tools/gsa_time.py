#!/usr/bin/env python3
"""Generalized suffix array at scale: tools/gsa_time.py <log2 total characters> <read length> <bits>.
Random DNA reads of equal length; SA+ISA+LCP through psacx_construct_gsa_*, verified whole by psacx_check_gsa_dev_*."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")      # PSACX_* variables select the forms of single stages (psac_amd/_lib.py: ENV_KNOBS)
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import inputs
import psac_amd

logn = int(sys.argv[1]); rl = int(sys.argv[2]); bits = int(sys.argv[3])
n = (1 << logn) // rl * rl
text = inputs.dna(n, 3)
off = np.arange(0, n + 1, rl, dtype=np.uint64)
ctx = psac_amd.Context(0)
sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
lib = ctx._lib
SA = np.empty(n, sa.dtype); ISA = np.empty(n, sa.dtype); LCP = np.empty(n, sa.dtype)
fn = getattr(lib, "psacx_construct_gsa_u%d" % bits)
for it in range(2):
    t0 = time.perf_counter()
    ctx.check(fn(ctx.handle, text.ctypes.data, n, off.ctypes.data, off.size - 1, 0, 1 | 4, SA.ctypes.data, ISA.ctypes.data, LCP.ctypes.data))
    dt = time.perf_counter() - t0
s = ctx.stats()
# the whole result back in HBM for the device checker's verdict (psacx_check_gsa_dev_*: order with equal suffixes in text order, every LCP value)
w = bits // 8
bufs = [ctx.alloc(n), ctx.alloc(off.nbytes)] + [ctx.alloc(n * w) for _ in range(3)]
for p, a in zip(bufs, (text, off, SA, ISA, LCP)):
    ctx.h2d(p, a)
err = psac_amd.check_gsa_device(ctx, bufs[0], n, bufs[1], off.size - 1, bufs[2], bufs[3], bufs[4], bits)
for p in bufs:
    ctx.free(p)
print("GSA of %d reads x %d (n = %d), uint%d: %.1f ms host call (device %.1f ms), %d rounds, %s (device checker: %s)"
      % (n // rl, rl, n, bits, dt * 1e3, s.ms_total, s.n_rounds, "verified" if not any(err) else "WRONG", err))
sys.exit(1 if any(err) else 0)
