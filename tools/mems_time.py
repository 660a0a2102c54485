#!/usr/bin/env python3
"""Time of the maximal exact matches beside the matching statistics they start from:
tools/mems_time.py --rate=R --store-rate=S [log2 characters (28)] [log2 reads (13)] [repeats (7)].

The method of tools/match_time.py: the text generated in HBM (psacx_synth_text_dev), uint32, SA and LCP constructed there, the
range-minimum index, the BWT and the statistics built by the library's own device calls and resident; HIP events on the context's
stream; after a warm-up call of every variant the variants take turns inside every repeat; median, least and largest are printed.
Batches:
  - random DNA, 2^13 reads of 128 bytes cut from the text with 2 % of their bytes substituted, min_len 20;
  - the same with PSACX_MEMS_SUPER;
  - the tandem repeat of period 1024, reads of 128 cut from it (nothing substituted), min_len 20, max_occ 0 against max_occ 16.  Every slot of such a
    read occurs n / 1024 times, so without max_occ a slot owns 2^18 candidates at n = 2^28: the batch is 16 reads (2^11 slots, 2^29
    candidates, half a GiB of mark bytes), not 2^13, which would need 2^38 mark bytes.
Per batch: the statistics call, the count query and the call that writes the lists (which repeats the count), with work[0] and
work[1].  The stages of a call are timed by the option PSACX_OPT_MEMS_STOP, which ends the call after its counting walk and scans (1),
after the writing walk (2), after the marks (3): the stage times are the differences, repeat by repeat, of the truncated calls, the
count query and the lists call, which take turns inside every repeat.

The fetch floor is read from the code, not profiled, stage by stage:
  walk          per slot three statistics entries, L[lb], L[ub]: 5 requests; per shell the loads of two searches -- one group of 64
                entries each, two 128-byte lines for uint32 -- and L at both new ends: 6 requests;
                (5 slots + 6 shells) / rate, and 3 stores per shell / store rate in the writing walk
  marks         per candidate one bwt byte and one word of `first`: 2 candidates / rate (neighbouring candidates of a shell are
                neighbouring ranks, so a long shell is served by lines, not by requests, and lies far below this floor)
  tile counts   the mark bytes streamed once at 8 TB/s, and the scan
  triples       per MEM one SA entry / rate and three stores / store rate
with rate = the gather4 line and store rate = the scatter8 line tools/ubench_gather prints at the span of the arrays.
PSACX_MEMS_SUPER: 4 requests per slot (three statistics entries and the left neighbour's length) for the count, per rank one SA
entry and three stores for the lists.
A sample of the triples of every batch is verified on the host by byte comparison: equal bytes, not extensible to either side."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import psac_amd

READ = 128


def verify(text, pat, poff_step, qpos, tpos, ln, min_len, rng, count=1024):
    """the number of wrong triples in a sample: bytes equal, l >= min_len, not extensible to the right or to the left"""
    bad = 0
    n = text.size
    for i in rng.randint(0, qpos.size, min(count, qpos.size)) if qpos.size else []:
        p, t, l = int(qpos[i]), int(tpos[i]), int(ln[i])
        p0, p1 = p // poff_step * poff_step, (p // poff_step + 1) * poff_step
        ok = l >= min_len and p + l <= p1 and t + l <= n and pat[p:p + l].tobytes() == text[t:t + l].tobytes()
        ok = ok and (p + l == p1 or t + l == n or pat[p + l] != text[t + l])
        ok = ok and (p == p0 or t == 0 or pat[p - 1] != text[t - 1])
        bad += not ok
    return bad


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rate = store = None
    for a in sys.argv[1:]:
        if a.startswith("--rate="):
            rate = float(a.split("=")[1])
        if a.startswith("--store-rate="):
            store = float(a.split("=")[1])
    if rate is None or store is None:
        sys.exit("--rate=<G requests/s> and --store-rate=<G requests/s> are required: the gather4 and scatter8 lines of tools/ubench_gather 27 28")
    logn = int(args[0]) if len(args) > 0 else 28
    logr = int(args[1]) if len(args) > 1 else 13
    reps = int(args[2]) if len(args) > 2 else 7
    n = 1 << logn
    stream = torch.cuda.Stream()
    ctx = psac_amd.Context(0, stream=stream.cuda_stream)
    lib, vp = ctx._lib, C.c_void_p
    rng = np.random.RandomState(11)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    print("n = 2^%d, uint32, reads of %d, %d repeats, device %s" % (logn, READ, reps, torch.cuda.get_device_name(0)))

    def timed(variants):
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

    for kind, period, reads, runs in ((0, 1024, 1 << logr, ((20, 0, 0), (20, 0, psac_amd.MEMS_SUPER))), (2, 1024, 16, ((20, 0, 0), (20, 16, 0)))):
        d_text, d_sa, d_isa, d_lcp = ctx.alloc(n), ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 4)
        ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, kind, 17, period))
        ctx._pre()
        ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, psac_amd.suffix_array.PSACX_LCP, vp(d_sa), vp(d_isa), vp(d_lcp)))
        ctx.free(d_isa)
        ctx.check(lib.psacx_trim(ctx.handle))
        d_index = ctx.alloc(psac_amd.rmq_index_device(ctx, None, n, None, 32) * 4)
        psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, 32)
        d_bwt, d_first = ctx.alloc(n), ctx.alloc(((n >> 5) + 1) * 4)
        psac_amd.bwt_device(ctx, d_text, n, None, d_sa, d_bwt, d_first, 32, want_primary=False)
        text = np.empty(n, np.uint8)
        ctx.d2h(text, d_text)
        starts = rng.randint(0, n - READ + 1, reads).astype(np.int64)
        pat = text[(starts[:, None] + np.arange(READ)[None, :]).reshape(-1)].copy()
        if kind == 0:
            where = rng.randint(0, pat.size, pat.size // 50)
            pat[where] = acgt[rng.randint(0, 4, where.size)]
        S = int(pat.size)
        poff = np.arange(reads + 1, dtype=np.uint64) * np.uint64(READ)
        d_pat, d_poff = ctx.alloc(S), ctx.alloc(poff.nbytes)
        ctx.h2d(d_pat, pat); ctx.h2d(d_poff, poff)
        d_ml, d_mlb, d_mub = ctx.alloc(S * 4), ctx.alloc(S * 4), ctx.alloc(S * 4)
        print("== %s, %d reads of %d%s (%d slots)" % ("random DNA" if kind == 0 else "tandem repeat, period %d" % period, reads, READ,
                                                  " with 2 % substituted" if kind == 0 else "", S))

        def stats():
            psac_amd.match_device(ctx, d_text, n, d_sa, None, 0, None, d_pat, d_poff, reads, psac_amd.MATCH_SUFFIXES, 0, S, d_ml, d_mlb, d_mub, 32)
        for min_len, max_occ, flags in runs:
            stats()
            work = []

            def mems(d_q=None, d_t=None, d_l=None, cap=0):
                return psac_amd.mems_device(ctx, n, d_sa, d_lcp, d_index, d_bwt, d_first, d_pat, d_poff, reads, d_ml, d_mlb, d_mub, min_len, max_occ, flags,
                                            d_q, d_t, d_l, cap, 32, work=work)
            z = mems()
            room = max(z, 1)
            d_q, d_t, d_l = ctx.alloc(room * 8), ctx.alloc(room * 4), ctx.alloc(room * 4)
            sup = bool(flags)

            def stopped(stage):
                def call():
                    os.environ["PSACX_MEMS_STOP"] = str(stage)
                    try:
                        mems()
                    finally:
                        del os.environ["PSACX_MEMS_STOP"]
                return call
            variants = [("statistics", stats)] + ([] if sup else [("stop%d" % k, stopped(k)) for k in (1, 2, 3)])
            res = timed(variants + [("count", mems), ("lists", lambda: mems(d_q, d_t, d_l, z))])
            G, St = rate * 1e9, store * 1e9
            print("-- min_len %d, max_occ %d%s: z = %d, work = %d / %d (%s)"
                  % (min_len, max_occ, ", PSACX_MEMS_SUPER" if sup else "", z, work[0], work[1], "slots kept / ranks" if sup else "shells / candidates"))

            def line(name, ms, fl):
                med = float(np.median(ms))
                tail = "" if fl is None else "; floor %8.3f ms; %s" % (fl, "measured / floor %6.2f" % (med / fl) if fl >= 0.005 else "no ratio: the floor is below 5 us")
                print("%-28s median %9.3f ms (least %9.3f, largest %9.3f)%s" % (name, med, min(ms), max(ms), tail))
            diff = lambda a, b: [x - y for x, y in zip(res[a], res[b])]  # noqa: E731
            emit = (z / G + 3 * z / St) * 1e3
            line("statistics", res["statistics"], None)
            if sup:
                line("count: slots, scan", res["count"], 4 * S / G * 1e3)
                line("lists - count: expansion", diff("lists", "count"), emit)
                line("lists", res["lists"], 4 * S / G * 1e3 + emit)
            else:
                walk = (5 * S + 6 * work[0]) / G * 1e3
                line("counting walk, two scans", res["stop1"], walk)
                line("writing walk", diff("stop2", "stop1"), walk + 3 * work[0] / St * 1e3)
                line("marks", diff("stop3", "stop2"), 2 * work[1] / G * 1e3)
                line("tile counts, scan", diff("count", "stop3"), work[1] / 8e12 * 1e3)
                line("count query", res["count"], 2 * walk + 3 * work[0] / St * 1e3 + 2 * work[1] / G * 1e3 + work[1] / 8e12 * 1e3)
                line("lists - count: triples", diff("lists", "count"), emit)
                line("lists", res["lists"], 2 * walk + 3 * work[0] / St * 1e3 + 2 * work[1] / G * 1e3 + work[1] / 8e12 * 1e3 + emit)
            qpos, tpos, ln = np.empty(room, np.uint64), np.empty(room, np.uint32), np.empty(room, np.uint32)
            ctx.d2h(qpos, d_q); ctx.d2h(tpos, d_t); ctx.d2h(ln, d_l)
            bad = verify(text, pat, READ, qpos[:z], tpos[:z], ln[:z], min_len, rng)
            print("sample of %d triples wrong: %d" % (min(1024, z), bad))
            assert bad == 0
            for p in (d_q, d_t, d_l):
                ctx.free(p)
        for p in (d_text, d_sa, d_lcp, d_index, d_bwt, d_first, d_pat, d_poff, d_ml, d_mlb, d_mub):
            ctx.free(p)
        ctx.check(lib.psacx_trim(ctx.handle))
    ctx.close()


if __name__ == "__main__":
    main()
