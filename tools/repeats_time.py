#!/usr/bin/env python3
"""Time of the BWT and of the repeat enumeration in HBM:
tools/repeats_time.py --rate=R --store-rate=S [--texts=dna,tandem,mutated] [log2 characters (28)] [repeats (5)].

The method of tools/lz_time.py: the text is generated in HBM (psacx_synth_text_dev: random DNA, the tandem repeat of period 1024, and
the repeated reads with mutations of bench.py), uint32, and SA, ISA and LCP are constructed there.  Timed, HIP events on the context's
stream, after a warm-up call, median / least / largest of the repeats:
  - BWT: psacx_bwt_dev_* with both outputs, against n gathered bytes at the gather rate (+ 4 n bytes of SA read and n written at 8 TB/s);
  - directories: the count query of kind 1 (and 2) with min_len = all ones less the same query of kind 0.  The filters come before the
    directory tests, so the three walks are the same and the difference is what building D and F (and St) and their scans costs;
  - per kind the count query and the count query + the lists, z, and the heads as a share of the ranks;
  - z of the right-maximal kind == edges - n of psacx_suffix_tree_dev_* where its table fits the free memory.
Beside each count query the fetch model of DESIGN.md 4.9.  Counted on the host over 64 runs of 2^12 ranks: for every rank with
L[j] > 0 the levels u the left search of rmq_last climbs until the 64-group that holds the previous value <= L[j] (a stack over the
2^16 ranks in front of the run finds it), 2 u + 1 group loads of two 128-byte lines each at uint32; for every head the same for the
right search of rmq_first to the next smaller value (psacx_ansv_dev_* gives it).  A head of kind 1 adds 4 directory fetches, of
kind 2 8 and the bwt bytes and bitmap words of its walk where it gets that far (one fetch per 16 ranks, counted for every head
that is flat: an upper bound).
    floor = (ranks x left lines + heads x (right lines + directory fetches)) / rate + (4 n + 2 n) bytes / 8 TB/s
            [+ 2 stores per selected head / store rate + 12 z bytes / 8 TB/s for the lists],
with rate = the gather4 line and store rate = the scatter8 line tools/ubench_gather prints at the span of the arrays."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import psac_amd

KINDS = {"dna": (0, 17, 1024, "random DNA"), "tandem": (2, 17, 1024, "tandem repeat of period 1024"),
         "mutated": (3, 7, 1 << 16, "repeated reads with mutations (period 65536, one substitution in 200)")}
NAMES = ("right-maximal", "maximal", "supermaximal")
HBM = 8e12
ONES = 0xFFFFFFFF


def levels(a, b):
    """the levels a search climbs from position a until the 64-group of its level also holds position b"""
    u = np.zeros(a.size, np.int64)
    x, y = a >> 6, b >> 6
    while np.any(x != y):
        u += x != y
        x, y = x >> 6, y >> 6
    return u


def sample(ctx, d_lcp, d_right, n, runs=64, run=1 << 12, back=1 << 16):
    """(ranks with L > 0, their left lines, heads, their right lines, flat heads' walk fetches, ranks whose left value lies outside the window)"""
    pos = heads = flat_fetch = lost = 0
    left_lines = right_lines = 0.0
    top = 0
    m = n
    while m > 64:
        m = (m + 63) >> 6
        top += 1
    for k in range(runs):
        r0 = k * (n // runs)
        w0 = max(0, r0 - back)
        L = np.empty(r0 + run - w0, np.uint32)
        ctx.d2h(L, d_lcp + w0 * 4)
        right = np.empty(run, np.uint64)
        ctx.d2h(right, d_right + r0 * 8)
        v = L.tolist()
        if w0 == 0:
            v[0] = 0
        st, h = [], np.full(run, -1, np.int64)
        for i, x in enumerate(v):                       # previous value <= x
            while st and v[st[-1]] > x:
                st.pop()
            if i + w0 >= r0:
                h[i + w0 - r0] = st[-1] + w0 if st else -1
            st.append(i)
        j = np.arange(r0, r0 + run, dtype=np.int64)
        lj = np.asarray(v[r0 - w0:], np.int64)
        live = (lj > 0) & (j >= 1)
        found = live & (h >= 0)
        lost += int(np.count_nonzero(live & (h < 0)))
        u = np.where(found, levels(np.maximum(j - 1, 0), np.maximum(h, 0)), top)
        pos += int(np.count_nonzero(live))
        left_lines += float(np.sum(2 * (2 * u[live] + 1)))
        lh = np.asarray(v, np.int64)[np.where(h >= 0, h - w0, 0)]
        head = found & (lh < lj)
        e = right.astype(np.int64)
        none = e >= n
        vv = np.where(none, top, levels(j + 1, np.where(none, j + 1, e)))
        heads += int(np.count_nonzero(head))
        right_lines += float(np.sum(2 * np.where(none[head], vv[head] + 1, 2 * vv[head] + 1)))
        occ = np.where(none, n, e) - np.maximum(h, 0)
        lo, hi = np.maximum(h, 0) + 1 - w0, np.minimum(np.where(none, n, e), r0 + run) - w0
        for t in np.nonzero(head)[0].tolist():          # flat: every value of the interval equals its length (as far as the window shows)
            if hi[t] - lo[t] <= 4096 and all(x == lj[t] for x in v[lo[t]:hi[t]]):
                flat_fetch += 2 * ((int(occ[t]) + 15) // 16)
    return pos, left_lines, heads, right_lines, flat_fetch, lost


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
        print("%-38s median %9.3f ms (least %9.3f, largest %9.3f)%s" % (name, float(np.median(ms)), min(ms), max(ms), more))
        return float(np.median(ms))

    for which in texts:
        kind, seed, period, label = KINDS[which]
        n = 1 << logn
        d_text, d_sa, d_isa, d_lcp = ctx.alloc(n), ctx.alloc(n * 4), ctx.alloc(n * 4), ctx.alloc(n * 4)
        ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, kind, seed, period))
        ctx._pre()
        ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, psac_amd.suffix_array.PSACX_LCP, vp(d_sa), vp(d_isa), vp(d_lcp)))
        ctx.free(d_isa)
        ctx.check(lib.psacx_trim(ctx.handle))
        entries = psac_amd.rmq_index_device(ctx, None, n, None, 32)
        d_index = ctx.alloc(entries * 4)
        psac_amd.rmq_index_device(ctx, d_lcp, n, d_index, 32)
        print("== n = 2^%d %s, uint32, %d repeats, gather %.1f and store %.1f G requests/s, device %s"
              % (logn, label, reps, rate, store, torch.cuda.get_device_name(0)))
        d_bwt, d_first = ctx.alloc(n), ctx.alloc(((n >> 5) + 1) * 4)
        t_bwt = line("BWT", timed(lambda: psac_amd.bwt_device(ctx, d_text, n, None, d_sa, d_bwt, d_first, 32)))
        floor = (n / (rate * 1e9) + 5.0 * n / HBM) * 1e3
        print("BWT: n gathered bytes at the gather rate + 5 n streamed bytes: floor %.3f ms; measured / floor %.2f" % (floor, t_bwt / floor))
        count = lambda k, min_len=0: psac_amd.repeats_device(ctx, n, d_lcp, d_index, d_bwt, d_first, k, min_len, 0, 0, None, None, None, 0, 32)  # noqa: E731
        base = line("walk alone (kind 0, min_len all ones)", timed(lambda: count(0, ONES)))
        for k in (1, 2):
            t = line("the same walk, kind %d" % k, timed(lambda: count(k, ONES)))
            print("directories of kind %d (%s): %.3f ms" % (k, "D, F" if k == 1 else "D, F, St", t - base))
        # the fetch model
        d_left, d_right = ctx.alloc(n * 8), ctx.alloc(n * 8)
        psac_amd.ansv_device(ctx, d_lcp, n, d_left, d_right, 32, 0, 0, n)
        ctx.free(d_left)
        pos, left_lines, heads, right_lines, flat_fetch, lost = sample(ctx, d_lcp, d_right, n)
        ctx.free(d_right)
        sampled = 64 * (1 << 12)
        scale = n / float(sampled)
        print("sample of %d ranks: %.1f%% have L > 0, %.2f left lines each; heads %.2f%% of the ranks, %.2f right lines each; %d ranks whose previous "
              "value lies outside the window (counted to the top level)" % (sampled, 100.0 * pos / sampled, left_lines / max(1, pos),
                                                                          100.0 * heads / sampled, right_lines / max(1, heads), lost))
        z = {}
        for k in (0, 1, 2):
            z[k] = count(k)
            extra = (0, 4, 8)[k] * heads + (flat_fetch if k == 2 else 0)
            walk = (left_lines + right_lines + extra) * scale / (rate * 1e9) + 6.0 * n / HBM
            t_count = line("%s: count query" % NAMES[k], timed(lambda: count(k)))
            print("%s: z = %d; floor %.3f ms; measured / floor %.2f" % (NAMES[k], z[k], walk * 1e3, t_count / (walk * 1e3)))
            room = max(1, z[k])
            d_lb, d_ub, d_len = ctx.alloc(room * 4), ctx.alloc(room * 4), ctx.alloc(room * 4)

            def both():
                zz = count(k)
                return psac_amd.repeats_device(ctx, n, d_lcp, d_index, d_bwt, d_first, k, 0, 0, 0, d_lb, d_ub, d_len, zz, 32)
            t_both = line("%s: count query + lists" % NAMES[k], timed(both))
            lists = 2 * walk + 2.0 * z[k] / (store * 1e9) + 12.0 * z[k] / HBM
            print("%s: count + lists: floor %.3f ms; measured / floor %.2f" % (NAMES[k], lists * 1e3, t_both / (lists * 1e3)))
            for p in (d_lb, d_ub, d_len):
                ctx.free(p)
        print("heads: %.2f%% of the ranks (z of the right-maximal kind / n)" % (100.0 * z[0] / n))
        sigma, _ = psac_amd.suffix_tree_device(ctx, d_text, n, None, None, None, 32)
        table = n * (sigma + 1) * 8
        free = torch.cuda.mem_get_info()[0]
        if table + (8 << 30) < free:
            d_nodes = ctx.alloc(table)
            _, edges = psac_amd.suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, 32)
            ctx.free(d_nodes)
            print("suffix tree of the same arrays: edges - n = %d, z of the right-maximal kind %d" % (edges - n, z[0]))
            assert edges - n == z[0]
        else:
            print("suffix tree: the table of %.1f GiB does not fit beside the arrays (%.1f GiB free); the identity is not checked at this size"
                  % (table / 2.0 ** 30, free / 2.0 ** 30))
        for p in (d_text, d_sa, d_lcp, d_index, d_bwt, d_first):
            ctx.free(p)
        ctx.check(lib.psacx_trim(ctx.handle))
    ctx.close()


if __name__ == "__main__":
    main()
