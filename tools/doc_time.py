#!/usr/bin/env python3
"""Time of the document index, the document counts and the document lists in HBM:
tools/doc_time.py --rate=R [--texts=dna,tandem] [log2 characters (28)] [log2 intervals (20)] [repeats (5)].

The method of tools/repeats_time.py: the text is generated in HBM (psacx_synth_text_dev: random DNA, as tools/locate_gsa_time.py takes it,
and the tandem repeat of period 1024), cut into reads of 100 characters, uint32; the generalized suffix array and its LCP are constructed
there and the range-minimum index of LCP is built.  Timed, HIP events on the context's stream, after a warm-up call, median / least /
largest of the repeats:
  - the index: psacx_doc_index_dev_* with both outputs, with prev alone and with dup alone, and, per stage, what the call itself
    measures under psacx_profile (events on its stream around the keys, the sort with its waits, prev and the pairs, the scan: psacx_stats
    ms_kmer, ms_sort_scatter, ms_rebucket, ms_finalize);
  - the same build on [b"ab"] * (2^20 + 1), where every atomic of the pairs stage hits one cell;
  - the counts: psacx_doc_count_dev_* over 2^20 locate intervals (patterns of 32 characters cut from the reads);
  - the lists: psacx_doc_list_dev_* over the first of those intervals that hold at most 2^28 ranks together, the size query and the call
    that writes, with candidates and outputs stated.
Beside each line a fetch model at the request rate tools/ubench_gather measures (--rate, its gather4 line at the span of the arrays):
  index   keys: 4 n bytes streamed in, 8 n out, and one search of the offsets per rank, log2(m) fetches of which all but the last few hit
          the cache: counted as 2.  Pairs: a non-adjacent pair costs at least two group loads of two 128-byte lines (the minimum, then
          its position) and one atomic; an adjacent pair one atomic, and 8 n bytes of keys streamed twice.  That floor holds for short
          ranges; the second line counts every range as tall as the index, which is what a read set gives.  Sort: one pass per 8 bits
          of m - 1, each reading and writing two key words and a payload word per rank, 24 n bytes.  Scan: 12 n bytes.
  counts  two fetches per interval, 12 q bytes streamed.
  lists   per candidate 4 bytes of prev streamed and a mark byte written and read twice; per listed rank one SA fetch and, as for the keys,
          2 fetches of the offsets; 8 bytes written."""
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
READ, PAT = 100, 32
HBM = 8e12
ONES = 0xFFFFFFFF


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rate, texts = None, ["dna", "tandem"]
    for a in sys.argv[1:]:
        if a.startswith("--rate="):
            rate = float(a.split("=")[1])
        if a.startswith("--texts="):
            texts = a.split("=")[1].split(",")
    if rate is None:
        sys.exit("--rate=<G requests/s> is required: the gather4 line of tools/ubench_gather 27 28")
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
        more = "" if floor is None else "; floor %.3f ms; measured / floor %.2f" % (floor * 1e3, med / (floor * 1e3))
        print("%-44s median %9.3f ms (least %9.3f, largest %9.3f)%s" % (name, med, min(ms), max(ms), more))
        return med

    def stages(build, d_prev, d_dup):
        """[(stage, [ms per repeat])] of the build with both outputs, as the call measures them itself"""
        out = [("keys", []), ("sort", []), ("prev and pairs", []), ("scan", [])]
        ctx.check(lib.psacx_profile(ctx.handle, 1))
        for _ in range(reps + 1):
            build(d_prev, d_dup)
            st = ctx.stats()
            for (name, ms), v in zip(out, (st.ms_kmer, st.ms_sort_scatter, st.ms_rebucket, st.ms_finalize)):
                ms.append(float(v))
        ctx.check(lib.psacx_profile(ctx.handle, 0))
        return [(name, ms[1:]) for name, ms in out]

    off = np.append(np.arange(0, n, READ, dtype=np.uint64), np.uint64(n))
    m = int(off.size - 1)
    for which in texts:
        kind, seed, period, label = KINDS[which]
        d_text, d_sa, d_isa, d_lcp = ctx.alloc(n), ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 4)
        d_soff = ctx.alloc(off.nbytes); ctx.h2d(d_soff, off)
        ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, kind, seed, period))
        ctx._pre()
        ctx.check(lib.psacx_construct_gsa_dev_u32(ctx.handle, vp(d_text), n, vp(d_soff), m, 0, psac_amd.suffix_array.PSACX_LCP, vp(d_sa), vp(d_isa), vp(d_lcp)))
        ctx.free(d_isa)
        ctx.check(lib.psacx_trim(ctx.handle))
        entries = psac_amd.rmq_index_device(ctx, None, n, None, 32)
        d_index = ctx.alloc(entries * 4)
        psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, 32)
        print("== n = 2^%d %s in %d reads of %d, uint32, %d repeats, gather %.1f G requests/s, device %s"
              % (logn, label, m, READ, reps, rate, torch.cuda.get_device_name(0)))
        # ---- the index
        d_prev, d_dup = ctx.alloc(n * 4), ctx.alloc((n + 1) * 4)
        build = lambda p, d: psac_amd.doc_index_device(ctx, n, d_soff, m, d_sa, d_lcp, d_index, p, d, 32)  # noqa: E731
        build(d_prev, d_dup)
        prev = np.empty(n, np.uint32)
        ctx.d2h(prev, d_prev)
        paired = prev != ONES
        adjacent = int(np.count_nonzero(paired & (prev + np.uint32(1) == np.arange(n, dtype=np.uint32))))
        far = int(np.count_nonzero(paired)) - adjacent
        del prev, paired
        print("pairs: %d adjacent, %d with a range-minimum search (%.1f%% of the ranks)" % (adjacent, far, 100.0 * far / n))
        line("index: prev alone (keys, sort, scatter)", timed(lambda: build(d_prev, None)))
        line("index: dup alone (keys, sort, pairs, scan)", timed(lambda: build(None, d_dup)))
        line("index: prev and dup", timed(lambda: build(d_prev, d_dup)))
        lev, left = 1, n
        while left > 64:
            left, lev = (left + 63) >> 6, lev + 1
        passes = (max(1, (m - 1).bit_length()) + 7) // 8
        floors = {"keys": 12.0 * n / HBM + 2.0 * n / (rate * 1e9), "sort": passes * 24.0 * n / HBM,
                  "prev and pairs": (5.0 * far + adjacent) / (rate * 1e9) + 20.0 * n / HBM, "scan": 12.0 * n / HBM}
        tall = (far * (4.0 + 2.0 * (lev - 1) + 2.0 * (2 * lev - 1) + 1.0) + adjacent) / (rate * 1e9) + 20.0 * n / HBM
        for name, ms in stages(build, d_prev, d_dup):
            line("  stage: %s" % name, ms, floors[name])
            if name == "prev and pairs":
                print("  prev and pairs, every range as tall as the index (%d levels): model %.3f ms; measured / model %.2f"
                      % (lev, tall * 1e3, float(np.median(ms)) / (tall * 1e3)))
        # ---- 2^20 locate intervals
        text = np.empty(n, np.uint8)
        ctx.d2h(text, d_text)
        rng = np.random.RandomState(11)
        starts = rng.randint(0, n // READ, q).astype(np.int64) * READ + rng.randint(0, READ - PAT + 1, q)
        pats = text[(starts[:, None] + np.arange(PAT)[None, :]).reshape(-1)].copy()
        del text
        poff = np.arange(q + 1, dtype=np.uint64) * np.uint64(PAT)
        d_pat, d_poff = ctx.alloc(pats.nbytes), ctx.alloc(poff.nbytes)
        ctx.h2d(d_pat, pats); ctx.h2d(d_poff, poff)
        words = psac_amd.string_ends_device(ctx, None, m, n, None)
        d_ends = ctx.alloc(words * 4)
        psac_amd.string_ends_device(ctx, d_soff, m, n, d_ends)
        d_lb, d_ub, d_docs = ctx.alloc(q * 4), ctx.alloc(q * 4), ctx.alloc(q * 4)
        psac_amd.locate_gsa_device(ctx, d_text, n, d_ends, d_sa, None, 0, None, d_pat, d_poff, q, d_lb, d_ub, 32)
        lb, ub = np.empty(q, np.uint32), np.empty(q, np.uint32)
        ctx.d2h(lb, d_lb); ctx.d2h(ub, d_ub)
        occ = ub.astype(np.int64) - lb
        line("counts: %d intervals" % q, timed(lambda: psac_amd.doc_count_device(ctx, n, d_dup, d_lb, d_ub, q, d_docs, 32)), 2.0 * q / (rate * 1e9) + 12.0 * q / HBM)
        docs = np.empty(q, np.uint32)
        ctx.d2h(docs, d_docs)
        print("  occurrences per interval: mean %.1f, largest %d; strings per interval: mean %.1f, largest %d"
              % (occ.mean(), occ.max(), docs.mean(), docs.max()))
        # ---- lists: the first intervals that hold at most 2^28 ranks together
        ql = int(np.searchsorted(np.cumsum(occ), 1 << 28, side="right"))
        ql = max(1, min(q, ql))
        cand = int(occ[:ql].sum())
        d_start = ctx.alloc((ql + 1) * 8)
        size = lambda: psac_amd.doc_list_device(ctx, d_sa, n, d_soff, m, d_prev, d_lb, d_ub, ql, 0, d_start, None, None, 0, 32)  # noqa: E731
        z = size()
        assert z == int(docs[:ql].sum()), (z, int(docs[:ql].sum()))      # locate intervals are LCP-intervals: the two halves of the index agree
        d_sid, d_pos = ctx.alloc(max(1, z) * 4), ctx.alloc(max(1, z) * 4)
        marks = (4.0 * cand + 3.0 * cand) / HBM + 24.0 * ql / HBM
        line("lists: size query, %d intervals" % ql, timed(size), marks)
        write = lambda: psac_amd.doc_list_device(ctx, d_sa, n, d_soff, m, d_prev, d_lb, d_ub, ql, 0, d_start, d_sid, d_pos, z, 32)  # noqa: E731
        line("lists: sid and pos", timed(write), marks + cand / HBM + 3.0 * z / (rate * 1e9) + 8.0 * z / HBM)
        print("  candidates %d, listed %d" % (cand, z))
        for p in (d_text, d_sa, d_lcp, d_soff, d_index, d_prev, d_dup, d_pat, d_poff, d_ends, d_lb, d_ub, d_docs, d_start, d_sid, d_pos):
            ctx.free(p)
        ctx.check(lib.psacx_trim(ctx.handle))
    # ---- every atomic on one cell: m copies of ab; the ab suffixes in text order, then the b suffixes; h[m] = m
    m = (1 << 20) + 1
    n = 2 * m
    SA = np.concatenate((2 * np.arange(m), 2 * np.arange(m) + 1)).astype(np.uint32)
    LCP = np.concatenate(([0], np.full(m - 1, 2), [0], np.full(m - 1, 1))).astype(np.uint32)
    off = (2 * np.arange(m + 1)).astype(np.uint64)
    d_sa, d_lcp, d_soff = ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(off.nbytes)
    ctx.h2d(d_sa, SA); ctx.h2d(d_lcp, LCP); ctx.h2d(d_soff, off)
    d_index = ctx.alloc(psac_amd.rmq_index_device(ctx, None, n, None, 32) * 4)
    psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, 32)
    d_prev, d_dup = ctx.alloc(n * 4), ctx.alloc((n + 1) * 4)
    build = lambda p, d: psac_amd.doc_index_device(ctx, n, d_soff, m, d_sa, d_lcp, d_index, p, d, 32)  # noqa: E731
    print("== n = %d, %d strings ab: %d pairs, every one adds to h[%d]" % (n, m, m, m))
    line("index: prev and dup", timed(lambda: build(d_prev, d_dup)))
    for name, ms in stages(build, d_prev, d_dup):
        line("  stage: %s" % name, ms)
    dup = np.empty(n + 1, np.uint32)
    ctx.d2h(dup, d_dup)
    assert np.all(dup[:m + 1] == 0) and np.all(dup[m + 1:] == m)
    ctx.close()


if __name__ == "__main__":
    main()
