#!/usr/bin/env python3
"""Time of the text samples and the extraction of the FM-index in HBM:
tools/fm_extract_time.py --rate=R [--texts=dna,tandem] [log2 characters (28)] [log2 windows (20)] [repeats (5)].

The method of tools/fm_time.py: the text is generated in HBM (psacx_synth_text_dev: random DNA, and the tandem repeat of period 1024), one
text, uint32; the suffix array is constructed there, the BWT and the first bitmap are made, the index is built with sample 32, and the
text samples with text_rate 32 and 64.  Timed, HIP events on the context's stream, after a warm-up call, median / least / largest of the
repeats:
  - the sample build: psacx_fm_text_samples_dev_*;
  - 2^20 windows of 64 bytes at random positions, and 2^20 windows of 200 bytes;
  - one query that restores the whole text, and the same bytes as one query per read of 100.
Every result is compared with the text.  Beside each line two yardsticks:
  model   the sample build streams SA once: 4 n bytes in at the HBM rate, 4 bytes per sample out.  An LF step is `bits` dependent cells
          at the request rate tools/ubench_gather measures (--rate, its gather8 line at the span of the blob; the 16-byte cell is one
          request).  A window takes len + rate / 2 expected steps (the walk from the sample at the right end of its last block), the
          restore n steps.
  copy    the same number of bytes copied from a resident text, device to device."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import psac_amd

KINDS = {"dna": (0, 17, 1024, "random DNA"), "tandem": (2, 17, 1024, "tandem repeat of period 1024")}
SAMPLE, RATES, READ = 32, (32, 64), 100
HBM = 8e12


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rate, texts = None, ["dna", "tandem"]
    for a in sys.argv[1:]:
        if a.startswith("--rate="):
            rate = float(a.split("=")[1])
        if a.startswith("--texts="):
            texts = a.split("=")[1].split(",")
    if rate is None:
        sys.exit("--rate=<G requests/s> is required: the gather8 line of tools/ubench_gather at the span of the blob")
    logn = int(args[0]) if len(args) > 0 else 28
    logq = int(args[1]) if len(args) > 1 else 20
    reps = int(args[2]) if len(args) > 2 else 5
    n, q = 1 << logn, 1 << logq
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

    def line(name, ms, floor=None, copy=None):
        med = float(np.median(ms))
        more = "" if floor is None else "; model %.3f ms; measured / model %.2f" % (floor * 1e3, med / (floor * 1e3))
        more += "" if copy is None else "; copy %.3f ms; measured / copy %.1f" % (copy, med / copy)
        print("%-58s median %9.3f ms (least %9.3f, largest %9.3f)%s" % (name, med, min(ms), max(ms), more))
        return med

    for which in texts:
        kind, seed, period, label = KINDS[which]
        d_text, d_sa, d_isa = ctx.alloc(n), ctx.alloc(n * 4), ctx.alloc(n * 4)
        ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, kind, seed, period))
        ctx._pre()
        ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, 0, vp(d_sa), vp(d_isa), None))
        ctx.free(d_isa)
        ctx.check(lib.psacx_trim(ctx.handle))
        d_bwt, d_first = ctx.alloc(n), ctx.alloc(4 * ((n >> 5) + 1))
        psac_amd.bwt_device(ctx, d_text, n, None, d_sa, d_bwt, d_first, 32, want_primary=False)
        info = psac_amd.fm_index_device(ctx, n, d_bwt, d_first, d_sa, SAMPLE, None, 32)
        d_fm = ctx.alloc(int(info.words) * 8)
        info = psac_amd.fm_index_device(ctx, n, d_bwt, d_first, d_sa, SAMPLE, d_fm, 32)
        ctx.free(d_bwt); ctx.free(d_first)
        bits, blob = int(info.bits), int(info.words) * 8
        text = np.empty(n, np.uint8)
        ctx.d2h(text, d_text)
        print("== n = 2^%d %s, one text, uint32, sample %d, %d repeats, gather %.1f G requests/s, device %s"
              % (logn, label, SAMPLE, reps, rate, torch.cuda.get_device_name(0)))
        rng = np.random.RandomState(13)
        batches = [("%d windows of 64 bytes" % q, rng.randint(0, n - 64, q), 64), ("%d windows of 200 bytes" % q, rng.randint(0, n - 200, q), 200),
                   ("one query for the whole text", np.zeros(1, np.int64), n),
                   ("the whole text, one query per read of %d" % READ, np.arange(0, n, READ), READ)]
        src = torch.empty(n, dtype=torch.uint8, device="cuda")
        dst = torch.empty(n, dtype=torch.uint8, device="cuda")

        def copy_ms(total):
            with torch.cuda.stream(stream):
                return float(np.median(timed(lambda: dst[:total].copy_(src[:total]))))
        for text_rate in RATES:
            entries = psac_amd.fm_text_samples_device(ctx, n, None, None, 0, text_rate, None, 32)
            d_ts = ctx.alloc(entries * 4)
            build = lambda: psac_amd.fm_text_samples_device(ctx, n, d_sa, None, 0, text_rate, d_ts, 32)  # noqa: E731
            print("text_rate %d: %d samples, %d bytes; index with them %d bytes = %.3f bytes per character; index / (text + SA) = %.3f"
                  % (text_rate, entries, 4 * entries, blob + 4 * entries, (blob + 4 * entries) / float(n), (blob + 4 * entries) / (5.0 * n)))
            line("  sample build", timed(build), (4.0 * n + 4.0 * entries) / HBM)
            for name, pos, length in batches:
                k = int(pos.size)
                total = int(np.minimum(length, n - pos).sum())
                if total > n:
                    continue
                p, l = pos.astype(np.uint32), np.full(k, length, np.uint32)
                d_pos, d_len, d_start = ctx.alloc(4 * k), ctx.alloc(4 * k), ctx.alloc(8 * (k + 1))
                ctx.h2d(d_pos, p); ctx.h2d(d_len, l)
                assert psac_amd.fm_extract_device(ctx, d_fm, info, d_ts, text_rate, None, 0, d_pos, d_len, k, d_start, None, 0, 32) == total
                d_out = ctx.alloc(total)
                ms = timed(lambda: psac_amd.fm_extract_device(ctx, d_fm, info, d_ts, text_rate, None, 0, d_pos, d_len, k, d_start, d_out, total, 32))
                got = np.empty(total, np.uint8)
                ctx.d2h(got, d_out)
                if length == n:
                    assert np.array_equal(got, text)
                elif k * length == total:
                    some = slice(0, k, max(1, k >> 16))             # (every 16th window of 2^20: the index array of all of them is large)
                    assert np.array_equal(got.reshape(k, length)[some], text[(pos[some, None] + np.arange(length)[None, :])])
                else:
                    assert np.array_equal(got, text[:total])
                steps = float(n) if total == n else k * (length + text_rate / 2.0)
                line("  extract: %s" % name, ms, steps * bits / (rate * 1e9), copy_ms(total))
                for d in (d_pos, d_len, d_start, d_out):
                    ctx.free(d)
            ctx.free(d_ts)
        del text, src, dst
        for p in (d_text, d_sa, d_fm):
            ctx.free(p)
        ctx.check(lib.psacx_trim(ctx.handle))
    ctx.close()


if __name__ == "__main__":
    main()
