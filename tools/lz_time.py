#!/usr/bin/env python3
"""Time of the LZ77 factorization in HBM, stage by stage:
tools/lz_time.py --rate=R --store-rate=S [--texts=dna,tandem,mutated] [log2 characters (28)] [repeats (5)] [log2 characters of the width check (26)].

The method of tools/lce_time.py: the text is generated in HBM (psacx_synth_text_dev: random DNA, the tandem repeat of period 1024,
and the repeated reads with mutations of bench.py, period 65536 with one substitution in 200, as the genome-like text), uint32, and
SA, ISA and LCP are constructed there (timed once, so that the parse stands beside what it costs on top).  Timed, HIP events on the
context's stream, after a warm-up call, median / least / largest of the repeats:
  - neighbours: psacx_ansv_dev_* nearest smaller / nearest smaller over SA, beside the same call over LCP of the same text;
  - LPF: psacx_lpf_dev_*, the whole call (it allocates and clears, finds the neighbours and runs lpf_kernel) and the call less the
    neighbours, against the fetch model of DESIGN.md 4.8: per rank the 128-byte lines the two range minima touch (counted on the
    host as rmq_min decomposes a range, tools/lce_time.py: min_lines, over a sample of 2^20 ranks in 64 runs), one SA fetch and
    two random stores; floor = n x (lines + 1) / rate + 2 n / store rate + 20 n bytes / 8 TB/s, with rate = the gather4 line and
    store rate = the scatter8 line tools/ubench_gather prints at the span of the arrays (`tools/ubench_gather 27 28`);
  - parse: psacx_lz77_dev_* as a user calls it (the count query, then the lists), with bytes moved / time / 8 TB/s: per position
    the entry read twice, the exit written, the mark cleared and read (3 w + 2 bytes, twice: the count query runs these passes too),
    per phrase the four entries lz_emit_kernel reads and writes;
    at the main size and a quarter of it -- a linear parse takes 4 times as long;
  - check: psacx_check_lz77_dev_*; every parse must come back with 0 errors.
Then z at uint32 equals z at uint64 on the smaller size."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import psac_amd
from lce_time import min_lines

KINDS = {"dna": (0, 17, 1024, "random DNA"), "tandem": (2, 17, 1024, "tandem repeat of period 1024"),
         "mutated": (3, 7, 1 << 16, "repeated reads with mutations (period 65536, one substitution in 200)")}
HBM = 8e12


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rate, store, texts = None, None, ["dna", "tandem", "mutated"]
    for a in sys.argv[1:]:
        if a.startswith("--rate="):
            rate = float(a.split("=")[1])
        if a.startswith("--store-rate="):
            store = float(a.split("=")[1])
        if a.startswith("--texts="):
            texts = a.split("=")[1].split(",")
    if rate is None or store is None:
        sys.exit("--rate=<G requests/s> and --store-rate=<G requests/s> are required: the gather4 and scatter8 lines of tools/ubench_gather 27 28")
    logn = int(args[0]) if len(args) > 0 else 28
    reps = int(args[1]) if len(args) > 1 else 5
    logw = int(args[2]) if len(args) > 2 else 26
    stream = torch.cuda.Stream()
    ctx = psac_amd.Context(0, stream=stream.cuda_stream)
    lib, vp = ctx._lib, C.c_void_p

    def timed(call, count=reps):
        call()
        out = []
        for _ in range(count):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); call(); e1.record(stream)
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    def line(name, ms, more=""):
        print("%-34s median %9.3f ms (least %9.3f, largest %9.3f)%s" % (name, float(np.median(ms)), min(ms), max(ms), more))
        return float(np.median(ms))

    def arrays(which, n, bits):
        """text, SA, LCP in HBM (ISA's memory is returned for LPF), and the construction's time"""
        kind, seed, period, label = KINDS[which]
        w = bits // 8
        d_text, d_sa, d_isa, d_lcp = ctx.alloc(n), ctx.alloc(n * w), ctx.alloc(n * w), ctx.alloc(n * w)
        ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, kind, seed, period))
        ctx._pre()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ctx.check(getattr(lib, "psacx_construct_dev_u%d" % bits)(ctx.handle, vp(d_text), n, 0, psac_amd.suffix_array.PSACX_LCP, vp(d_sa), vp(d_isa), vp(d_lcp)))
        e1.record(stream); e1.synchronize()
        ctx.check(lib.psacx_trim(ctx.handle))
        entries = psac_amd.rmq_index_device(ctx, None, n, None, bits)
        d_index = ctx.alloc(entries * w)
        psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, bits)
        return d_text, d_sa, d_isa, d_lcp, d_index, e0.elapsed_time(e1)

    def parse(n, d_lpf, d_src, bits, d_start, d_psrc, room):
        z = psac_amd.lz77_device(ctx, n, d_lpf, d_src, None, None, 0, bits)
        assert z + 1 <= room
        return psac_amd.lz77_device(ctx, n, d_lpf, d_src, d_start, d_psrc, z + 1, bits)

    for which in texts:
        label = KINDS[which][3]
        n = 1 << logn
        d_text, d_sa, d_lpf, d_lcp, d_index, ms_sa = arrays(which, n, 32)
        print("== n = 2^%d %s, uint32, %d repeats, gather %.1f and store %.1f G requests/s, device %s"
              % (logn, label, reps, rate, store, torch.cuda.get_device_name(0)))
        print("construction (SA, ISA, LCP)        %9.3f ms" % ms_sa)
        t_index = line("index of LCP", timed(lambda: psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, 32)))
        d_left, d_right, d_src = ctx.alloc(n * 8), ctx.alloc(n * 8), ctx.alloc(n * 4)
        t_lcp = line("neighbours of LCP (ansv 0 / 0)", timed(lambda: psac_amd.ansv_device(ctx, d_lcp, n, d_left, d_right, 32, 0, 0, n)))
        t_nb = line("neighbours of SA (ansv 0 / 0)", timed(lambda: psac_amd.ansv_device(ctx, d_sa, n, d_left, d_right, 32, 0, 0, n)))
        print("neighbours: SA / LCP %.2f" % (t_nb / t_lcp))
        # the lines of the two range minima, over 64 runs of 2^14 ranks
        run = min(n // 64, 1 << 14)
        lines, has = [], 0
        for k in range(64):
            r0 = k * (n // 64)
            left, right = np.empty(run, np.uint64), np.empty(run, np.uint64)
            ctx.d2h(left, d_left + r0 * 8); ctx.d2h(right, d_right + r0 * 8)
            r = np.arange(r0, r0 + run, dtype=np.int64)
            hp, hq = left < r.astype(np.uint64), (right > r.astype(np.uint64)) & (right < n)
            lo = np.concatenate([left[hp].astype(np.int64) + 1, r[hq] + 1])
            hi = np.concatenate([r[hp] + 1, right[hq].astype(np.int64) + 1])
            lines.append(min_lines(lo, hi, n).sum())
            has += int(np.count_nonzero(hp | hq))
        per = float(np.sum(lines)) / (64 * run)
        floor = (n * (per + 1) / (rate * 1e9) + 2.0 * n / (store * 1e9) + 20.0 * n / HBM) * 1e3
        t_call = line("LPF call", timed(lambda: psac_amd.lpf_device(ctx, n, d_sa, d_lcp, d_index, d_lpf, d_src, 32)))
        print("LPF less the neighbours            %9.3f ms; %.2f line fetches per rank for the two minima (%.1f%% of the sampled ranks have a neighbour); "
              "floor %.3f ms; measured / floor %.2f" % (t_call - t_nb, per, 100.0 * has / (64 * run), floor, (t_call - t_nb) / floor))
        ctx.free(d_left); ctx.free(d_right)
        z = psac_amd.lz77_device(ctx, n, d_lpf, d_src, None, None, 0, 32)
        d_start, d_psrc = ctx.alloc((z + 1) * 4), ctx.alloc((z + 1) * 4)
        t_parse = {}
        for m in (n, n >> 2):                           # a prefix of the factor array parses as an array of its own (lengths are clamped)
            zm = parse(m, d_lpf, d_src, 32, d_start, d_psrc, z + 1)
            moved = 2 * m * (3 * 4 + 2) + zm * 4 * 4   # (the count query runs the passes over the positions a second time)
            t_parse[m] = line("parse of 2^%d (z = %d)" % (int(np.log2(m)), zm), timed(lambda: parse(m, d_lpf, d_src, 32, d_start, d_psrc, z + 1)))
            print("parse of 2^%d: bytes moved / time / 8 TB/s = %.3f" % (int(np.log2(m)), moved / (t_parse[m] * 1e-3) / HBM))
        print("parse: time at 2^%d / time at 2^%d = %.2f (linear: 4)" % (logn, logn - 2, t_parse[n] / t_parse[n >> 2]))
        assert parse(n, d_lpf, d_src, 32, d_start, d_psrc, z + 1) == z
        t_check = line("check", timed(lambda: psac_amd.check_lz77_device(ctx, d_text, n, d_start, d_psrc, z, 32)))
        errors = psac_amd.check_lz77_device(ctx, d_text, n, d_start, d_psrc, z, 32)
        print("z = %d, n / z = %.2f, errors of the device verdict: %d" % (z, n / float(z), errors))
        assert errors == 0
        chain = t_index + t_call + t_parse[n]
        print("SA / LCP in HBM to the phrase lists: index + LPF call + parse = %.3f ms; construction of the same text %.3f ms: %.1f%% on top"
              % (chain, ms_sa, 100.0 * chain / ms_sa))
        for p in (d_text, d_sa, d_lpf, d_lcp, d_index, d_src, d_start, d_psrc):
            ctx.free(p)
        ctx.check(lib.psacx_trim(ctx.handle))
        # both widths at the smaller size
        zs = {}
        m = 1 << logw
        for bits in (32, 64):
            w = bits // 8
            d_text, d_sa, d_lpf, d_lcp, d_index, _ = arrays(which, m, bits)
            d_src = ctx.alloc(m * w)
            psac_amd.lpf_device(ctx, m, d_sa, d_lcp, d_index, d_lpf, d_src, bits)
            zs[bits] = psac_amd.lz77_device(ctx, m, d_lpf, d_src, None, None, 0, bits)
            d_start, d_psrc = ctx.alloc((zs[bits] + 1) * w), ctx.alloc((zs[bits] + 1) * w)
            assert psac_amd.lz77_device(ctx, m, d_lpf, d_src, d_start, d_psrc, zs[bits] + 1, bits) == zs[bits]
            assert psac_amd.check_lz77_device(ctx, d_text, m, d_start, d_psrc, zs[bits], bits) == 0
            for p in (d_text, d_sa, d_lpf, d_lcp, d_index, d_src, d_start, d_psrc):
                ctx.free(p)
            ctx.check(lib.psacx_trim(ctx.handle))
        print("2^%d: z at uint32 %d, at uint64 %d, both verified" % (logw, zs[32], zs[64]))
        assert zs[32] == zs[64]
    ctx.close()


if __name__ == "__main__":
    main()
