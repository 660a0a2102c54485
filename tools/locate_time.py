#!/usr/bin/env python3
"""Time of the pattern search and of its lookup table: tools/locate_time.py --rate=R [log2 characters (28)] [log2 patterns per kind (20)] [repeats (7)].

Random DNA generated in HBM, uint32, the suffix array constructed there (psacx_construct_dev_u32).  Two batches in shuffled order:
patterns of length 32 cut from the text (they occur) and random patterns of length 32 (they do not).  Timed with HIP events on the
context's stream, after a warm-up call of every variant, the variants taking turns inside every repeat; median, least and largest
of the repeats are printed:
  - psacx_lookup_table_dev_u32 for three values of k, and psacx_locate_dev_u32 with each table;
  - the search without a table;
  - the other kernel shape (eight lanes per pattern, PSACX_OPT_LOCATE_SHAPE = 2) without a table and with the middle k.
The counting kernels (PSACX_OPT_LOCATE_COUNT, a run of their own) give the SA entries and text words fetched per pattern; one of
each per bisection step waits for the one before it.  Against them stands the rate at which this chip serves independent random
fetches, which tools/ubench_gather prints at the span of SA and text: --rate=<its "G requests/s">, required (for 2^28 uint32 the
gather4 line of `tools/ubench_gather 27 28`, 1 GiB).  floor = patterns x fetches per pattern / rate.  No threshold: the ratio is printed.
A sample of 4096 patterns of every batch is verified on the host against the text and the suffix array."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import psac_amd


def verify_sample(text, SA, pats, m, lb, ub, sample):
    """text[SA[lb]:][:m] == P where lb < ub, and neither SA[lb-1] nor SA[ub] matches."""
    n = text.size
    bad = 0
    for i in sample:
        P = pats[i * m:(i + 1) * m].tobytes()
        at = lambda r: text[int(SA[r]):int(SA[r]) + m].tobytes()
        a, b = int(lb[i]), int(ub[i])
        ok = a <= b <= n
        if ok and a < b:
            ok = at(a) == P and at(b - 1) == P
        if ok and a > 0:
            ok = at(a - 1) < P
        if ok and b < n:
            ok = at(b) > P
        bad += not ok
    return bad


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rate = None
    for a in sys.argv[1:]:
        if a.startswith("--rate="):
            rate = float(a.split("=")[1])
    if rate is None:
        sys.exit("--rate=<G requests/s> is required: the gather4 rate tools/ubench_gather prints at the span of SA (tools/ubench_gather 27 28 for 2^28 uint32)")
    logn = int(args[0]) if len(args) > 0 else 28
    logq = int(args[1]) if len(args) > 1 else 20
    reps = int(args[2]) if len(args) > 2 else 7
    n, q, m = 1 << logn, 1 << logq, 32
    stream = torch.cuda.Stream()
    ctx = psac_amd.Context(0, stream=stream.cuda_stream)
    lib, vp = ctx._lib, C.c_void_p
    d_text, d_sa, d_isa = ctx.alloc(n), ctx.alloc(n * 4), ctx.alloc(n * 4)
    ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, 0, 17, 1024))
    ctx._pre()
    ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, 0, vp(d_sa), vp(d_isa), None))
    ctx.free(d_isa)
    ctx.check(lib.psacx_trim(ctx.handle))
    text, SA = np.empty(n, np.uint8), np.empty(n, np.uint32)
    ctx.d2h(text, d_text); ctx.d2h(SA, d_sa)
    print("n = 2^%d DNA, uint32, %d patterns of length %d per batch, %d repeats, device %s" % (logn, q, m, reps, torch.cuda.get_device_name(0)))

    rng = np.random.RandomState(11)
    starts = rng.randint(0, n - m + 1, q).astype(np.int64)                      # random order: the batch is shuffled as it is made
    batches = {"cut from the text": text[(starts[:, None] + np.arange(m)[None, :]).reshape(-1)].copy(),
               "random": np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, q * m)]}
    off = (np.arange(q + 1, dtype=np.uint64) * np.uint64(m))
    d_off = ctx.alloc(off.nbytes); ctx.h2d(d_off, off)
    d_pat = {k: ctx.alloc(v.nbytes) for k, v in batches.items()}
    for k, v in batches.items():
        ctx.h2d(d_pat[k], v)
    d_lb, d_ub = ctx.alloc(q * 4), ctx.alloc(q * 4)

    code, sigma, _ = psac_amd.lookup_table_device(ctx, d_text, n, None, 1, None, 32)
    B = sigma + 1
    ks = [k for k in (8, 10, 11) if B ** k <= 1 << 30] if B == 5 else [1, 2, 3]
    tables = {}
    for k in ks:
        entries = psac_amd.lookup_table_device(ctx, d_text, n, None, k, None, 32)[2]
        tables[k] = ctx.alloc(entries * 4)

    def timed(variants):
        """{name: [ms per repeat]}; every variant once as warm-up, then in turns."""
        for name, call in variants:
            call()
        out = {name: [] for name, call in variants}
        for _ in range(reps):
            for name, call in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream); call(); e1.record(stream)
                e1.synchronize()
                out[name].append(e0.elapsed_time(e1))
        return out

    def show(name, ms, per=None):
        med = float(np.median(ms))
        extra = "" if per is None else "  %8.2f M patterns/s" % (per / med / 1e3)
        print("%-58s median %8.3f ms  (least %8.3f, largest %8.3f)%s" % (name, med, min(ms), max(ms), extra))
        return med

    res = timed([("psacx_lookup_table_dev_u32 k = %d (%d entries)" % (k, B ** k + 1),
                  (lambda k=k: psac_amd.lookup_table_device(ctx, d_text, n, d_sa, k, tables[k], 32))) for k in ks])
    for name, ms in res.items():
        show(name, ms)

    def shape(s):
        os.environ["PSACX_LOCATE_SHAPE"] = "group" if s == 2 else "lane"

    def run(batch, k, s=1):
        shape(s)
        psac_amd.locate_device(ctx, d_text, n, d_sa, tables[k] if k else None, k, code if k else None, d_pat[batch], d_off, q, d_lb, d_ub, 32)

    medians = {}
    lb, ub = np.empty(q, np.uint32), np.empty(q, np.uint32)
    sample = rng.randint(0, q, 4096)
    for batch in batches:
        print("-- patterns %s" % batch)
        variants = [("one pattern per lane, no table", (lambda: run(batch, 0)))]
        variants += [("one pattern per lane, k = %d" % k, (lambda k=k: run(batch, k))) for k in ks]
        variants += [("eight lanes per pattern, no table", (lambda: run(batch, 0, 2))),
                     ("eight lanes per pattern, k = %d" % ks[1], (lambda: run(batch, ks[1], 2)))]
        res = timed(variants)
        for name, ms in res.items():
            medians[(batch, name)] = show(name, ms, q)
        # fetches per pattern (counting kernels, not timed), the floor they give, and the host check of a sample
        os.environ["PSACX_LOCATE_COUNT"] = "1"
        for k in [0] + ks:
            run(batch, k)
            f = ctx.stats().locate_fetches
            ctx.d2h(lb, d_lb); ctx.d2h(ub, d_ub)
            bad = verify_sample(text, SA, batches[batch], m, lb, ub, sample)
            per = (f[0] + f[1]) / float(q)
            floor_ms = q * per / (rate * 1e9) * 1e3
            name = "one pattern per lane, " + ("no table" if k == 0 else "k = %d" % k)
            print("%-34s %6.2f SA entries + %6.2f text words = %6.2f fetches per pattern; floor at %.1f G/s %7.3f ms; measured / floor %5.2f; "
                  "found %d of %d; sample of 4096 wrong: %d" % (name, f[0] / float(q), f[1] / float(q), per, rate, floor_ms,
                                                               medians[(batch, name)] / floor_ms, int((ub > lb).sum()), q, bad))
            assert bad == 0
        del os.environ["PSACX_LOCATE_COUNT"]
    for p in [d_text, d_sa, d_off, d_lb, d_ub] + list(d_pat.values()) + list(tables.values()):
        ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
