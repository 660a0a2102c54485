#!/usr/bin/env python3
"""Time of the device checkers on reads: tools/gsa_check_time.py [log2 characters (28)] [repeats (3)].

DNA generated in HBM, cut into reads of 100-150 characters.  The same bytes are constructed twice with 32-bit indices: as
one text (psacx_construct_dev_u32, verified by psacx_check_dev_u32 and psacx_multi_check_dev_u32) and as a string set
(psacx_construct_gsa_dev_u32, verified by psacx_check_gsa_dev_u32 and psacx_multi_check_gsa_dev_u32).  One GPU: HIP events
on the context's stream around each call after a warm-up call.  Distributed (1 and 4 ranks sharing the device, the blocks
being slices of the same arrays): a host clock around the call, which returns after every rank's stream has drained.
Also the least free device memory seen while psacx_check_gsa_dev_u32 runs (polled from a second thread) against the free
memory before it: the checker's peak extra memory."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import psac_amd
from psac_amd._lib import PSACX_LCP


def read_offsets(n, seed=5):
    rng = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(rng.randint(100, 151, size=n // 100 + 2))]).astype(np.uint64)
    return np.concatenate([off[off < n], [n]]).astype(np.uint64)


def main():
    logn = int(sys.argv[1]) if len(sys.argv) > 1 else 28
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    n = 1 << logn
    stream = torch.cuda.Stream()
    ctx = psac_amd.Context(0, stream=stream.cuda_stream)
    lib = ctx._lib
    vp = C.c_void_p
    off = read_offsets(n)
    m = off.size - 1
    d_text = ctx.alloc(n)
    ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, 0, 17, 1024))
    d_off = ctx.alloc(off.nbytes); ctx.h2d(d_off, off)
    plain = [ctx.alloc(n * 4) for _ in range(3)]
    gsa = [ctx.alloc(n * 4) for _ in range(3)]
    ctx._pre()
    ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, PSACX_LCP, vp(plain[0]), vp(plain[1]), vp(plain[2])))
    ctx.check(lib.psacx_construct_gsa_dev_u32(ctx.handle, vp(d_text), n, vp(d_off), m, 0, PSACX_LCP, vp(gsa[0]), vp(gsa[1]), vp(gsa[2])))
    ctx.check(lib.psacx_trim(ctx.handle))                    # the constructions' workspace goes back before memory is watched
    print("n = 2^%d = %d characters in %d reads of 100-150, uint32, device %s" % (logn, n, m, torch.cuda.get_device_name(0)))

    def timed(call):
        err = call()                                         # warm-up
        ev, host = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream); err = call(); e1.record(stream)
            e1.synchronize()
            host.append((time.perf_counter() - t0) * 1e3); ev.append(e0.elapsed_time(e1))
        return err, ev, host

    fmt = lambda v: " ".join("%.2f" % x for x in v)
    for lcp in (True, False):
        tag = "SA+ISA+LCP" if lcp else "SA+ISA"
        e, ev, host = timed(lambda: psac_amd.check_device(ctx, d_text, n, plain[0], plain[1], plain[2] if lcp else None, 32))
        print("one GPU  psacx_check_dev_u32      %-10s errors %s  events ms: %s  host ms: %s" % (tag, e, fmt(ev), fmt(host)))
        e, ev, host = timed(lambda: psac_amd.check_gsa_device(ctx, d_text, n, d_off, m, gsa[0], gsa[1], gsa[2] if lcp else None, 32))
        print("one GPU  psacx_check_gsa_dev_u32  %-10s errors %s  events ms: %s  host ms: %s" % (tag, e, fmt(ev), fmt(host)))

    # peak extra device memory of the one-GPU GSA checker
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    low, stop = [before], [False]

    def poll():
        while not stop[0]:
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
    th = threading.Thread(target=poll); th.start()
    for _ in range(5):
        psac_amd.check_gsa_device(ctx, d_text, n, d_off, m, gsa[0], gsa[1], gsa[2], 32)
    stop[0] = True; th.join()
    print("psacx_check_gsa_dev_u32 peak extra device memory: %d bytes (free before %d, least free during 5 calls %d); bitmap (n / 32 + 1) * 4 = %d bytes, "
          "slab 4096 bytes (allocated before)" % (before - low[0], before, low[0], (n // 32 + 1) * 4))

    for P in (1, 4):
        mg = psac_amd.MultiContext([0] * P)
        offs, sizes = [], []
        for r in range(P):
            sizes.append(n // P + (1 if r < n % P else 0)); offs.append(sum(sizes[:-1]))
        blocks = lambda base, w: [base + o * w for o in offs]
        for lcp in (True, False):
            tag = "SA+ISA+LCP" if lcp else "SA+ISA"
            for name, call in (("psacx_multi_check_dev_u32    ", lambda: mg.check_device(blocks(d_text, 1), sizes, blocks(plain[0], 4), blocks(plain[1], 4), blocks(plain[2], 4) if lcp else None, 32)),
                               ("psacx_multi_check_gsa_dev_u32", lambda: mg.check_gsa_device(blocks(d_text, 1), sizes, off, blocks(gsa[0], 4), blocks(gsa[1], 4), blocks(gsa[2], 4) if lcp else None, 32))):
                e = call()
                host = []
                for _ in range(reps):
                    t0 = time.perf_counter(); e = call(); host.append((time.perf_counter() - t0) * 1e3)
                print("%d rank%s  %s %-10s errors %s  host ms: %s" % (P, " " if P == 1 else "s", name, tag, e, fmt(host)))
        mg.close()
    for p in [d_text, d_off] + plain + gsa:
        ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
