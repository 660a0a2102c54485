#!/usr/bin/env python3
"""Time of the range-minimum index, the batched range minima and the longest common extensions:
tools/lce_time.py --rate=R [--texts=dna,mutated] [log2 characters (28)] [log2 queries per batch (20)] [repeats (7)].

The method of tools/match_time.py: the text is generated in HBM (psacx_synth_text_dev: random DNA, and the repeated reads with
mutations of bench.py, period 65536 with one substitution in 200), uint32, and SA, ISA and LCP are constructed there.  Timed:
  - the index build (psacx_rmq_index_dev_*), beside the time pyramid_level_kernel alone takes for level 1 in the same call
    (psacx_profile: psacx_stats.ms_rmq_build) -- the one pass over LCP, which is what the build cannot do without;
  - 2^20 ranges of length 2, 100, 10^4 and 10^7 at random places, with and without the position of the minimum;
  - 2^20 random pairs of positions with 0 and with 4 mismatches;
  - 2^20 pairs of positions that are neighbours in SA (long answers on the repetitive text), 0 and 4 mismatches.
HIP events on the context's stream, after a warm-up call of every variant, the variants taking turns inside every repeat; median,
least and largest of the repeats are printed.  Beside every line: floor = queries x line fetches per query / rate, and measured /
floor.  rate = --rate=<G requests/s>, the gather4 line tools/ubench_gather prints at the span of the array (`tools/ubench_gather
27 28` for 2^28 uint32).  The line fetches per query are counted on the host for the batch as rmq.hpp decomposes a range -- a line
is 128 bytes, a group of 64 uint32 entries is two lines, a single entry of the index is one:
  - minimum: level 0 costs one group where the range lies in one group, else a group per end that is not aligned; every level
    above costs one entry per end that is not aligned, and the level on which the range closes inside one group costs that group
    (one entry if it touches an end of the group);
  - position: the groups of the walk up from lo to the level F on which the first minimum's block lies in lo's group, and down
    again: 2 F + 1 groups;
  - LCE: two lines of ISA and the minimum's lines per jump, jumps = 1 + the mismatches stepped over (counted from the answers with
    0 .. e - 1 mismatches); the minimum's lines of the later jumps are taken to be those of the first.
The range ends and the results (8 or 12 bytes per query, coalesced) are not counted.  No threshold: the ratios are printed.
A sample of 1024 queries of every batch is verified on the host: a plain minimum of the slice, and bytes compared one by one."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import psac_amd

KINDS = {"dna": (0, 17, 1024, "random DNA"), "mutated": (3, 7, 1 << 16, "repeated reads with mutations (period 65536, one substitution in 200)")}


def min_lines(lo, hi, n):
    """128-byte lines the minimum of [lo, hi) reads (uint32), per query, as rmq_min of rmq.hpp decomposes the range"""
    l, r = lo.astype(np.int64).copy(), hi.astype(np.int64).copy()
    lines = np.zeros(l.size, np.int64)
    open_ = l < r
    length, level = n, 0
    while open_.any():
        one = open_ & ((l >> 6) == ((r - 1) >> 6))
        two = open_ & ~one
        if level == 0:
            lines[one] += 2
            lines[two] += 2 * ((l[two] & 63) != 0) + 2 * ((r[two] & 63) != 0)
        else:
            edge = ((l[one] & 63) == 0) | ((r[one] & 63) == 0)
            lines[one] += np.where(edge, 1, 2)
            lines[two] += ((l[two] & 63) != 0).astype(np.int64) + ((r[two] & 63) != 0)
        l, r = np.where(two, (l + 63) >> 6, l), np.where(two, r >> 6, r)
        open_ = two & (l < r)
        level += 1
        length = (length + 63) >> 6
        if length <= 1:
            break
    return lines


def arg_lines(lo, arg, ok):
    """lines of the walk for the first minimum: 2 F + 1 groups of two lines"""
    F = np.zeros(lo.size, np.int64)
    a, b = lo.astype(np.int64) >> 6, arg.astype(np.int64) >> 6
    while True:
        far = ok & (a != b)
        if not far.any():
            break
        F[far] += 1
        a, b = a >> 6, b >> 6
    return np.where(ok, 2 * (2 * F + 1), 0)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rate, texts = None, ["dna", "mutated"]
    for a in sys.argv[1:]:
        if a.startswith("--rate="):
            rate = float(a.split("=")[1])
        if a.startswith("--texts="):
            texts = a.split("=")[1].split(",")
    if rate is None:
        sys.exit("--rate=<G requests/s> is required: the gather4 rate tools/ubench_gather prints at the span of the array (tools/ubench_gather 27 28 for 2^28 uint32)")
    logn = int(args[0]) if len(args) > 0 else 28
    logq = int(args[1]) if len(args) > 1 else 20
    reps = int(args[2]) if len(args) > 2 else 7
    n, q = 1 << logn, 1 << logq
    stream = torch.cuda.Stream()
    ctx = psac_amd.Context(0, stream=stream.cuda_stream)
    lib, vp = ctx._lib, C.c_void_p

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

    def report(name, ms, lines):
        med = float(np.median(ms))
        per = float(lines.mean())
        floor_ms = q * per / (rate * 1e9) * 1e3
        print("%-44s median %8.3f ms (least %8.3f, largest %8.3f) %8.2f M queries/s; %6.2f line fetches per query; floor %7.3f ms; measured / floor %6.2f"
              % (name, med, min(ms), max(ms), q / med / 1e3, per, floor_ms, med / floor_ms if floor_ms else 0.0))

    for which in texts:
        kind, seed, period, label = KINDS[which]
        d_text, d_sa, d_isa, d_lcp = ctx.alloc(n), ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 4)
        ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, kind, seed, period))
        ctx._pre()
        ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, psac_amd.suffix_array.PSACX_LCP, vp(d_sa), vp(d_isa), vp(d_lcp)))
        ctx.check(lib.psacx_trim(ctx.handle))
        text, SA, ISA, LCP = np.empty(n, np.uint8), np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint32)
        ctx.d2h(text, d_text); ctx.d2h(SA, d_sa); ctx.d2h(ISA, d_isa); ctx.d2h(LCP, d_lcp)
        ctx.free(d_sa)
        print("== n = 2^%d %s, uint32, %d queries per batch, %d repeats, rate %.1f G requests/s, device %s"
              % (logn, label, q, reps, rate, torch.cuda.get_device_name(0)))
        print("mean LCP %.1f, largest %d" % (float(LCP.mean(dtype=np.float64)), int(LCP.max())))

        entries = psac_amd.rmq_index_device(ctx, None, n, None, 32)
        d_index = ctx.alloc(entries * 4)
        ctx.check(lib.psacx_profile(ctx.handle, 1))
        level1 = []

        def build():
            psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, 32)
            level1.append(ctx.stats().ms_rmq_build)
        ms = timed([("index", build)])["index"]
        ctx.check(lib.psacx_profile(ctx.handle, 0))
        l1 = level1[1:]
        print("index build: %d entries (%.2f%% of the array); median %7.3f ms (least %7.3f, largest %7.3f); pyramid_level_kernel of level 1 alone: "
              "median %7.3f ms (least %7.3f, largest %7.3f); build / level 1 %5.2f; level 1 reads %.2f GB/s"
              % (entries, 100.0 * entries / n, float(np.median(ms)), min(ms), max(ms), float(np.median(l1)), min(l1), max(l1),
                 float(np.median(ms)) / float(np.median(l1)), n * 4 / float(np.median(l1)) / 1e6))

        rng = np.random.RandomState(11)
        sample = rng.randint(0, q, 1024)
        d_lo, d_hi, d_min, d_arg = ctx.alloc(q * 4), ctx.alloc(q * 4), ctx.alloc(q * 4), ctx.alloc(q * 4)
        mn, arg = np.empty(q, np.uint32), np.empty(q, np.uint32)
        for length in (2, 100, 10 ** 4, 10 ** 7):
            if length >= n:
                continue
            lo = rng.randint(0, n - length + 1, q).astype(np.uint32)
            hi = (lo + np.uint32(length)).astype(np.uint32)
            ctx.h2d(d_lo, lo); ctx.h2d(d_hi, hi)
            res = timed([("min", lambda: psac_amd.rmq_device(ctx, d_lcp, n, d_index, d_lo, d_hi, q, d_min, None, 32)),
                         ("min + arg", lambda: psac_amd.rmq_device(ctx, d_lcp, n, d_index, d_lo, d_hi, q, d_min, d_arg, 32))])
            ctx.d2h(mn, d_min); ctx.d2h(arg, d_arg)
            base = min_lines(lo, hi, n)
            report("ranges of %d, minimum" % length, res["min"], base)
            report("ranges of %d, minimum and position" % length, res["min + arg"], base + arg_lines(lo, arg, np.ones(q, bool)))
            bad = 0
            for i in sample:
                s = LCP[int(lo[i]):int(hi[i])]
                bad += (int(mn[i]), int(arg[i])) != (int(s.min()), int(lo[i]) + int(np.argmin(s)))
            print("sample of 1024 wrong: %d" % bad)
            assert bad == 0

        d_a, d_b, d_len = d_lo, d_hi, d_min
        ln = np.empty(q, np.uint32)
        near = rng.randint(0, n - 1, q)
        batches = [("random pairs", rng.randint(0, n, q).astype(np.uint32), rng.randint(0, n, q).astype(np.uint32)),
                   ("neighbours in SA", SA[near], SA[near + 1])]
        for name, a, b in batches:
            ctx.h2d(d_a, a); ctx.h2d(d_b, b)
            res = timed([("e0", lambda: psac_amd.lce_device(ctx, n, None, 0, d_isa, d_lcp, d_index, d_a, d_b, q, 0, d_len, 32)),
                         ("e4", lambda: psac_amd.lce_device(ctx, n, None, 0, d_isa, d_lcp, d_index, d_a, d_b, q, 4, d_len, 32))])
            r, s = ISA[a].astype(np.int64), ISA[b].astype(np.int64)
            first = min_lines(np.minimum(r, s) + 1, np.maximum(r, s) + 1, n)
            room = (n - np.maximum(a, b)).astype(np.int64)
            jumps = np.ones(q, np.int64)
            answers = {}
            for e in (0, 1, 2, 3, 4):
                psac_amd.lce_device(ctx, n, None, 0, d_isa, d_lcp, d_index, d_a, d_b, q, e, d_len, 32)
                ctx.d2h(ln, d_len)
                answers[e] = ln.copy()
                if e < 4:
                    jumps += (ln.astype(np.int64) < room) & (a != b)
            report("LCE, %s, 0 mismatches" % name, res["e0"], 2 + first)
            report("LCE, %s, 4 mismatches" % name, res["e4"], jumps * (2 + first))
            print("mean length %.1f with 0 mismatches, %.1f with 4; mean jumps with 4: %.2f"
                  % (float(answers[0].mean(dtype=np.float64)), float(answers[4].mean(dtype=np.float64)), float(jumps.mean())))
            bad = 0
            for i in sample:
                x, y, L = int(a[i]), int(b[i]), int(room[i])
                for e in (0, 4):
                    d, miss, w = L, 0, 4096
                    at = 0
                    while at < L:                       # bytes compared one by one, a window at a time
                        differ = np.nonzero(text[x + at:x + min(L, at + w)] != text[y + at:y + min(L, at + w)])[0]
                        if miss + differ.size > e:
                            d = at + int(differ[e - miss])
                            break
                        miss += differ.size
                        at += w
                    bad += int(answers[e][i]) != d
            print("sample of 1024 wrong: %d" % bad)
            assert bad == 0
        for p in (d_text, d_isa, d_lcp, d_index, d_lo, d_hi, d_min, d_arg):
            ctx.free(p)
        ctx.check(lib.psacx_trim(ctx.handle))
    ctx.close()


if __name__ == "__main__":
    main()
