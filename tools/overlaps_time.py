#!/usr/bin/env python3
"""Time of the suffix-prefix overlaps of a set of reads:
tools/overlaps_time.py --rate=R [--sample=S (4096)] [--prefix-reads=P (65536)] [log2 characters (28)] [coverage (16)] [repeats (7)].

The set is that of tools/gst_time.py: reads of 100..150 characters at random places of a random genome of n / coverage characters,
uint32.  SA, ISA and LCP are constructed in HBM, the range-minimum index of LCP and the bitmap of the string ends are built beside
them.  Timed, for min_len 32 and 64, with and without the whole strings:
  - psacx_overlaps_dev_* (the clear of its two outputs included), and that clear on its own (two memsets of n entries);
  - psacx_occurrences_dev_* over the result with q = n (the size query and the expansion, as a caller runs them).
HIP events on the context's stream, after a warm-up call of every variant, the variants taking turns inside every repeat; median,
least and largest of the repeats are printed.  Beside the kernel: steps per string, 128-byte lines fetched per string, floor =
strings x lines per string / rate, and (measured - clear) / floor.  rate = --rate=<G requests/s>, the gather4 line tools/ubench_gather
prints at the span of SA (`tools/ubench_gather 27 28` for 2^28 uint32).  Steps and lines are counted on the host for a sample of S
strings, as overlaps.hpp decomposes a walk -- a line is 128 bytes, a group of 64 uint32 entries is two lines:
  - a step: LCP[i] and SA[i], one line each, and the same two again after a left search; the bitmap word, one line;
  - the left search (rmq_last): 2 F + 1 groups, F = the level on which the answer's block lies in the group of i - 1;
  - the run end: per round the distinct lines of the probed SA entries and of their bitmap words;
  - the whole string's step: the groups of rmq_first for the right end, counted as the left search is.
ISA[o_j] is one line and the two offsets are one; the results are not counted.  No threshold: the ratios are printed.
The sample's slots are compared with a walk on the host that uses no index (a scan for the previous smaller value).

Comparison: what the same answer costs through a call that exists without this one -- psacx_locate_gsa_dev_* over every prefix of
length >= min_len of P reads (no table), scaled to all reads.  It returns every occurrence of a prefix, not the ones that end their
string, so the caller would still have to filter; the line is a lower bound of that way."""
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
from gst_time import reads


def search_groups(a, b):
    """groups a search from group position a to the answer b loads: 2 F + 1, F = levels until both lie in one group"""
    F = 0
    while (a >> 6) != (b >> 6):
        a, b, F = a >> 6, b >> 6, F + 1
    return 2 * F + 1


def walk(j, off, ends, SA, ISA, LCP, n, min_len, whole):
    """(steps, lines, [(slot, lb, ub)]) of string j as overlaps_kernel walks it; previous smaller values by a scan"""
    o, oe = int(off[j]), int(off[j + 1])
    L = oe - o
    r = int(ISA[o])
    i, d = r, (L if whole else L - 1)
    steps, lines, out = 0, 2, []
    while d >= min_len and d >= 1:
        steps += 1
        lines += 2
        if int(LCP[i]) >= d:
            x = i - 1
            while x >= 0 and int(LCP[x]) > d - 1:
                x -= 1
            if x < 0:
                break
            lines += 2 * search_groups(i - 1, x) + 2
            i = x
        s = int(SA[i])
        lines += 1
        if s + d <= n and (ends[(s + d) >> 5] >> ((s + d) & 31)) & 1:
            hi = r
            if d == L:
                hi = r + 1
                while hi < n and int(LCP[hi]) > d - 1:
                    hi += 1
                if r + 1 < n:
                    lines += 2 * search_groups(r + 1, min(hi, n - 1))
            hi = max(hi, i + 1)
            lo = i + 1
            while lo < hi:
                w = (hi - lo + 15) // 16
                xs = [lo + t * w for t in range(16) if lo + t * w < hi]
                held = [int(SA[x]) + d <= n and bool((ends[(int(SA[x]) + d) >> 5] >> ((int(SA[x]) + d) & 31)) & 1) for x in xs]
                lines += len(set(x >> 5 for x in xs)) + len(set((int(SA[x]) + d) >> 10 for x in xs if int(SA[x]) + d <= n))
                f = held.index(False) if False in held else len(held)
                if f == 0:
                    break
                nxt = lo + f * w
                lo += (f - 1) * w + 1
                if f < 16 and nxt < hi:
                    hi = nxt
            out.append((o + d - 1, i, lo))
        d = int(LCP[i])
    return steps, lines, out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rate, sample, prefix_reads = None, 4096, 1 << 16
    for a in sys.argv[1:]:
        if a.startswith("--rate="):
            rate = float(a.split("=")[1])
        if a.startswith("--sample="):
            sample = int(a.split("=")[1])
        if a.startswith("--prefix-reads="):
            prefix_reads = int(a.split("=")[1])
    if rate is None:
        sys.exit("--rate=<G requests/s> is required: the gather4 rate tools/ubench_gather prints at the span of SA (tools/ubench_gather 27 28 for 2^28 uint32)")
    logn = int(args[0]) if len(args) > 0 else 28
    coverage = int(args[1]) if len(args) > 1 else 16
    reps = int(args[2]) if len(args) > 2 else 7
    n = 1 << logn
    text, off = reads(n, coverage)
    m = int(off.size - 1)
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

    def fmt(ms):
        return "median %9.3f ms (least %9.3f, largest %9.3f)" % (float(np.median(ms)), min(ms), max(ms))

    d_text, d_off = ctx.alloc(n), ctx.alloc(off.size * 8)
    ctx.h2d(d_text, text); ctx.h2d(d_off, off)
    d_sa, d_isa, d_lcp = ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 4)
    ctx._pre()
    ctx.check(lib.psacx_construct_gsa_dev_u32(ctx.handle, vp(d_text), n, vp(d_off), m, 0, psac_amd.suffix_array.PSACX_LCP, vp(d_sa), vp(d_isa), vp(d_lcp)))
    ctx.check(lib.psacx_trim(ctx.handle))
    SA, ISA, LCP = np.empty(n, np.uint32), np.empty(n, np.uint32), np.empty(n, np.uint32)
    ctx.d2h(SA, d_sa); ctx.d2h(ISA, d_isa); ctx.d2h(LCP, d_lcp)
    entries = psac_amd.rmq_index_device(ctx, None, n, None, 32)
    d_index = ctx.alloc(entries * 4)
    psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, 32)
    words = psac_amd.string_ends_device(ctx, None, m, n, None)
    d_ends = ctx.alloc(words * 4)
    psac_amd.string_ends_device(ctx, d_off, m, n, d_ends)
    ends = np.empty(words, np.uint32)
    ctx.d2h(ends, d_ends)
    print("== n = 2^%d = %d characters in %d reads of a %d-character genome, uint32, %d repeats, rate %.1f G requests/s, device %s"
          % (logn, n, m, max(n // coverage, 200), reps, rate, torch.cuda.get_device_name(0)))
    print("mean LCP %.1f, largest %d" % (float(LCP.mean(dtype=np.float64)), int(LCP.max())))

    d_lb, d_ub, d_start = ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc((n + 1) * 8)
    lb, ub = np.empty(n, np.uint32), np.empty(n, np.uint32)
    rng = np.random.RandomState(23)
    picked = rng.randint(0, m, sample)
    hip = C.CDLL(None)                                       # (the HIP runtime the library brought into the process)
    hip.hipMemsetAsync.argtypes = [vp, C.c_int, C.c_size_t, vp]

    def clear():                                             # (on memory of the same size that the next call overwrites: the results stay)
        assert hip.hipMemsetAsync(d_start, 0, n * 4, stream.cuda_stream) == 0 and hip.hipMemsetAsync(d_start + n * 4, 0, n * 4, stream.cuda_stream) == 0

    for min_len in (32, 64):
        for whole in (False, True):
            flags = psac_amd.OVERLAP_WHOLE if whole else 0
            state = {}

            def run():
                psac_amd.overlaps_device(ctx, n, d_off, m, d_ends, d_sa, d_isa, d_lcp, d_index, min_len, flags, d_lb, d_ub, 32)

            def lists():
                total = psac_amd.occurrences_device(ctx, d_sa, n, d_off, m, d_lb, d_ub, n, 0, d_start, None, None, 0, 32)
                if "pos" not in state:
                    state["pos"], state["sid"], state["total"] = ctx.alloc(max(1, total) * 4), ctx.alloc(max(1, total) * 4), total
                psac_amd.occurrences_device(ctx, d_sa, n, d_off, m, d_lb, d_ub, n, 0, d_start, state["pos"], state["sid"], total, 32)
            run()
            res = timed([("overlaps", run), ("clear", clear), ("occurrences", lists)])
            run()
            ctx.d2h(lb, d_lb); ctx.d2h(ub, d_ub)
            slots, pairs = int(np.count_nonzero(ub > lb)), int((ub.astype(np.int64) - lb.astype(np.int64)).sum())
            steps, lines, bad = 0, 0, 0
            for j in picked:
                s, l, out = walk(int(j), off, ends, SA, ISA, LCP, n, min_len, whole)
                steps += s
                lines += l
                o, oe = int(off[j]), int(off[j + 1])
                got = [(p, int(lb[p]), int(ub[p])) for p in range(o, oe) if ub[p] > lb[p]]
                bad += sorted(out) != got
            per_steps, per_lines = steps / float(sample), lines / float(sample)
            floor_ms = m * per_lines / (rate * 1e9) * 1e3
            med, clr = float(np.median(res["overlaps"])), float(np.median(res["clear"]))
            print("-- min_len %d%s: %d non-empty slots, %d pairs" % (min_len, ", whole strings" if whole else "", slots, pairs))
            print("overlaps     %s %8.2f M strings/s; %5.2f steps and %6.2f line fetches per string; floor %8.3f ms; (measured - clear) / floor %6.2f"
                  % (fmt(res["overlaps"]), m / med / 1e3, per_steps, per_lines, floor_ms, (med - clr) / floor_ms))
            print("clear alone  %s" % fmt(res["clear"]))
            print("occurrences  %s %8.2f M pairs/s" % (fmt(res["occurrences"]), pairs / float(np.median(res["occurrences"])) / 1e3))
            print("sample of %d strings wrong: %d" % (sample, bad))
            assert bad == 0 and state["total"] == pairs
            ctx.free(state["pos"]); ctx.free(state["sid"])

    # the same question through locate: every prefix of length >= min_len of P reads, a chunk of reads per call
    for min_len in (32, 64):
        P = min(prefix_reads, m)
        chunk, total_ms, patterns, hits = 2048, 0.0, 0, 0
        for c0 in range(0, P, chunk):
            js = np.arange(c0, min(P, c0 + chunk))
            L = (off[js + 1] - off[js]).astype(np.int64)
            cnt = np.maximum(L - min_len, 0)                                  # depths min_len .. L - 1
            q = int(cnt.sum())
            if q == 0:
                continue
            owner = np.repeat(np.arange(js.size), cnt)
            depth = np.arange(q, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + min_len
            poff = np.zeros(q + 1, np.uint64)
            poff[1:] = np.cumsum(depth)
            at = np.repeat(off[js][owner].astype(np.int64) - poff[:-1].astype(np.int64), depth) + np.arange(int(poff[-1]), dtype=np.int64)
            pat = text[at]
            d_pat, d_poff, d_plb, d_pub = ctx.alloc(pat.size), ctx.alloc(poff.size * 8), ctx.alloc(q * 4), ctx.alloc(q * 4)
            ctx.h2d(d_pat, pat); ctx.h2d(d_poff, poff)
            call = lambda: psac_amd.locate_gsa_device(ctx, d_text, n, d_ends, d_sa, None, 0, None, d_pat, d_poff, q, d_plb, d_pub, 32)  # noqa: E731
            ms = timed([("locate", call)])["locate"]
            total_ms += float(np.median(ms))
            patterns += q
            plb, pub = np.empty(q, np.uint32), np.empty(q, np.uint32)
            ctx.d2h(plb, d_plb); ctx.d2h(pub, d_pub)
            hits += int((pub.astype(np.int64) - plb.astype(np.int64)).sum())
            for p in (d_pat, d_poff, d_plb, d_pub):
                ctx.free(p)
        print("locate_gsa over every prefix >= %d of %d reads: %d patterns, %d occurrences (not only string ends), %9.3f ms; scaled to %d reads: %10.1f ms"
              % (min_len, P, patterns, hits, total_ms, m, total_ms * m / float(P)))
    for p in (d_text, d_off, d_sa, d_isa, d_lcp, d_index, d_ends, d_lb, d_ub, d_start):
        ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
