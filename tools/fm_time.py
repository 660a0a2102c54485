#!/usr/bin/env python3
"""Time of the FM-index in HBM: tools/fm_time.py --rate=R [--texts=dna,tandem] [log2 characters (28)] [log2 patterns (20)] [repeats (5)].

The method of tools/doc_time.py: the text is generated in HBM (psacx_synth_text_dev: random DNA, and the tandem repeat of period 1024),
one text, uint32; the suffix array is constructed there, the BWT and the first bitmap are made, and the index is built with sample 32.
Timed, HIP events on the context's stream, after a warm-up call, median / least / largest of the repeats:
  - the build: psacx_fm_index_dev_* as a whole, and per stage what the call itself measures under psacx_profile (psacx_stats ms_kmer:
    histogram, mark count and codes; ms_sort_scatter: the levels; ms_rebucket: marks and samples);
  - the index bytes against text + SA;
  - the count: psacx_fm_count_dev_* over 2^20 patterns of 32 bytes cut from the text, and over 2^20 random ones, beside psacx_locate_dev_*
    with the k = 11 table on the same batches;
  - the occurrences: psacx_fm_occurrences_dev_* for 2^20 singleton intervals and for a few long ones (2^24 ranks in 16 intervals), beside
    psacx_occurrences_dev_* on the same intervals.
Beside each line a fetch model at the request rate tools/ubench_gather measures (--rate, its gather8 line at the span of the blob; the
16-byte cell of the index is one request):
  build   histogram and codes: n bytes in twice, n / 8 of bitmap, 2 n out.  Levels: per level 2 n in twice (count, emit), 2 n scattered
          out at the store rate of a 2-byte scatter, which the model takes as one request per code, and 16 bytes per cell.  Marks: 4 n in
          twice, 4 bytes per mark out.
  count   2 * bits cells per step and pattern byte after the first: (L - 1) * 2 * bits requests for a pattern that occurs; a random
          pattern ends after about log4(n) steps.
  walk    bits + 1 cells per LF step, (sample - 1) / 2 expected steps, one mark cell and one val entry at the end."""
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
PAT, SAMPLE, K = 32, 32, 11
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

    def line(name, ms, floor=None):
        med = float(np.median(ms))
        more = "" if floor is None else "; model %.3f ms; measured / model %.2f" % (floor * 1e3, med / (floor * 1e3))
        print("%-52s median %9.3f ms (least %9.3f, largest %9.3f)%s" % (name, med, min(ms), max(ms), more))
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
        build = lambda: psac_amd.fm_index_device(ctx, n, d_bwt, d_first, d_sa, SAMPLE, d_fm, 32)  # noqa: E731
        info = build()
        bits, marks, blob = int(info.bits), int(info.marks), int(info.words) * 8
        print("== n = 2^%d %s, one text, uint32, sample %d, %d repeats, gather %.1f G requests/s, device %s"
              % (logn, label, SAMPLE, reps, rate, torch.cuda.get_device_name(0)))
        print("index: sigma %d, %d levels, %d marks, %d bytes = %.3f bytes per character; text + SA: %d bytes; index / (text + SA) = %.3f"
              % (info.sigma, bits, marks, blob, blob / float(n), 5 * n, blob / (5.0 * n)))
        counting = psac_amd.fm_index_device(ctx, n, d_bwt, d_first, None, 0, None, 32)
        print("index without samples: %d bytes = %.3f bytes per character" % (int(counting.words) * 8, int(counting.words) * 8.0 / n))
        # ---- the build
        line("build: size query", timed(lambda: psac_amd.fm_index_device(ctx, n, d_bwt, d_first, d_sa, SAMPLE, None, 32)))
        line("build: whole call", timed(build))
        cells = (n >> 6) + 1
        floors = {"histogram, mark count, codes": (2.0 * n + n / 4.0 + 4.0 * n + 2.0 * n) / HBM,
                  "levels": bits * ((4.0 * n + 16.0 * cells + 24.0 * cells) / HBM + (n if bits > 1 else 0) * (bits - 1.0) / bits / (rate * 1e9)),
                  "marks and samples": (8.0 * n + n / 4.0 + 4.0 * marks + 40.0 * cells) / HBM}
        out = [(name, []) for name in floors]
        ctx.check(lib.psacx_profile(ctx.handle, 1))
        for _ in range(reps + 1):
            build()
            st = ctx.stats()
            for (name, ms), v in zip(out, (st.ms_kmer, st.ms_sort_scatter, st.ms_rebucket)):
                ms.append(float(v))
        ctx.check(lib.psacx_profile(ctx.handle, 0))
        worst = None
        for name, ms in out:
            med = line("  stage: %s" % name, ms[1:], floors[name])
            ratio = med / (floors[name] * 1e3)
            worst = (ratio, name) if worst is None or ratio > worst[0] else worst
        print("  the stage furthest from its model, the stage to change first: %s (%.2f x)" % (worst[1], worst[0]))
        # ---- 2^20 patterns that occur, 2^20 random ones
        text = np.empty(n, np.uint8)
        ctx.d2h(text, d_text)
        rng = np.random.RandomState(11)
        starts = rng.randint(0, n - PAT, q).astype(np.int64)
        occurring = text[(starts[:, None] + np.arange(PAT)[None, :]).reshape(-1)].copy()
        letters = np.unique(text[:1 << 20])
        del text
        random = letters[rng.randint(0, letters.size, q * PAT)].astype(np.uint8)
        poff = np.arange(q + 1, dtype=np.uint64) * np.uint64(PAT)
        d_poff = ctx.alloc(poff.nbytes); ctx.h2d(d_poff, poff)
        code, sigma, entries = psac_amd.lookup_table_device(ctx, d_text, n, None, K, None, 32)
        d_table = ctx.alloc(entries * 4)
        code, sigma, entries = psac_amd.lookup_table_device(ctx, d_text, n, d_sa, K, d_table, 32)
        d_lb, d_ub, d_l2, d_u2 = (ctx.alloc(q * 4) for _ in range(4))
        for name, pats in (("occurring", occurring), ("random", random)):
            d_pat = ctx.alloc(pats.nbytes); ctx.h2d(d_pat, pats)
            fm_ms = timed(lambda: psac_amd.fm_count_device(ctx, d_fm, info, d_pat, d_poff, q, d_lb, d_ub, 32))
            lo_ms = timed(lambda: psac_amd.locate_device(ctx, d_text, n, d_sa, d_table, K, code, d_pat, d_poff, q, d_l2, d_u2, 32))
            a, b, a2, b2 = (np.empty(q, np.uint32) for _ in range(4))
            ctx.d2h(a, d_lb); ctx.d2h(b, d_ub); ctx.d2h(a2, d_l2); ctx.d2h(b2, d_u2)
            hit = b > a
            assert np.array_equal(hit, b2 > a2) and np.array_equal(a[hit], a2[hit]) and np.array_equal(b[hit], b2[hit])      # locate's intervals
            steps = (PAT - 1.0) if name == "occurring" else max(1.0, np.log(n) / np.log(max(2, sigma)))
            f = line("count: %d %s patterns of %d bytes" % (q, name, PAT), fm_ms, q * steps * 2.0 * bits / (rate * 1e9))
            l = line("  psacx_locate_dev_* with the k = %d table, same batch" % K, lo_ms)
            print("  count / locate = %.2f (patterns that occur: %d)" % (f / l, int(np.count_nonzero(hit))))
            ctx.free(d_pat)
        # ---- occurrences: singletons, and a few long intervals
        d_start = ctx.alloc((q + 1) * 8)
        for name, lo, hi in (("%d singletons" % q, rng.randint(0, n, q), None), ("16 intervals of 2^%d ranks" % (logn - 8), np.arange(16) * (n >> 4), n >> 8)):
            lo = lo.astype(np.uint32)
            hi = (lo + np.uint32(1 if hi is None else hi)).astype(np.uint32)
            k = int(lo.size)
            ctx.h2d(d_lb, lo); ctx.h2d(d_ub, hi)
            total = psac_amd.fm_occurrences_device(ctx, d_fm, info, None, 0, d_lb, d_ub, k, 0, d_start, None, None, 0, 32)
            d_pos, d_p2 = ctx.alloc(total * 4), ctx.alloc(total * 4)
            fm_ms = timed(lambda: psac_amd.fm_occurrences_device(ctx, d_fm, info, None, 0, d_lb, d_ub, k, 0, d_start, d_pos, None, total, 32))
            sa_ms = timed(lambda: psac_amd.occurrences_device(ctx, d_sa, n, None, 0, d_lb, d_ub, k, 0, d_start, d_p2, None, total, 32))
            p1, p2 = np.empty(total, np.uint32), np.empty(total, np.uint32)
            ctx.d2h(p1, d_pos); ctx.d2h(p2, d_p2)
            assert np.array_equal(p1, p2)
            model = total * ((SAMPLE - 1) / 2.0 * (bits + 1.0) + 2.0) / (rate * 1e9)
            f = line("occurrences: %s (%d positions)" % (name, total), fm_ms, model)
            l = line("  psacx_occurrences_dev_* on the suffix array, same batch", sa_ms, total / (rate * 1e9))
            print("  walk / suffix array = %.1f" % (f / l))
            ctx.free(d_pos); ctx.free(d_p2)
        for p in (d_text, d_sa, d_bwt, d_first, d_fm, d_poff, d_table, d_lb, d_ub, d_l2, d_u2, d_start):
            ctx.free(p)
        ctx.check(lib.psacx_trim(ctx.handle))
    ctx.close()


if __name__ == "__main__":
    main()
