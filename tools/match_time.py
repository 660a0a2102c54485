#!/usr/bin/env python3
"""Time of the longest-match search beside the pattern search of the same library:
tools/match_time.py --rate=R [--set] [--first=N] [log2 characters (28)] [log2 queries per batch (20)] [repeats (7)].

The method of tools/locate_time.py: random DNA generated in HBM, uint32, the suffix array constructed there; with --set the text
is taken as reads of 100 characters and the generalized suffix array is constructed (the twin of tools/locate_gsa_time.py).
Batches in shuffled order, 2^20 queries each:
  - patterns of 32 bytes cut from the text (from inside one read with --set): they occur;
  - the same with one byte substituted at a random position;
  - random patterns of 32 bytes;
  - the suffix mode over 2^13 reads of 128 bytes cut from the text with four bytes substituted in each (2^20 slots), cut to
    max_len = 32, and uncapped.
Every batch runs without a table and with k = 10 and 11.  Timed with HIP events on the context's stream, after a warm-up call of
every variant, the variants taking turns inside every repeat; median, least and largest of the repeats are printed.  The yardstick
is psacx_locate_dev_* (psacx_locate_gsa_dev_*) of the same library on the same batch in the same run, where the batch has one
query per pattern: the time ratio match / locate stands beside the ratio of the fetches the counting kernels report
(PSACX_OPT_LOCATE_COUNT, a run of their own), which is what it should be if both run at the chip's rate for dependent random
requests.  floor = queries x fetches per query / rate, rate = --rate=<G requests/s>, the gather4 line tools/ubench_gather prints at
the span of SA (`tools/ubench_gather 27 28` for 2^28 uint32).  No threshold: the ratios are printed.
--first=N runs the first N batches only (a counter collection on one batch).
A sample of 1024 queries of every batch is verified on the host by a bisection of its own over text and suffix array."""
import os as _os; _os.environ.setdefault("PSACX_ENV_KNOBS", "1")
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import psac_amd

READ = 100


def host_answer(text, SA, Q, read):
    """(len, lb, ub) of one query by bisection on the host; read = 0: one text, else the strings are reads of that length."""
    n, m = text.size, len(Q)

    def at(r, d=m):
        p = int(SA[r])
        e = n if not read else min(n, (p // read + 1) * read)
        return text[p:min(e, p + d)].tobytes()

    def first(lo, hi, pred):
        while lo < hi:
            mid = (lo + hi) // 2
            if pred(mid):
                hi = mid
            else:
                lo = mid + 1
        return lo
    ip = first(0, n, lambda r: at(r) >= Q)
    d = 0
    for r in (ip - 1, ip):
        if 0 <= r < n:
            s, c = at(r), 0
            while c < len(s) and s[c] == Q[c]:
                c += 1
            d = max(d, c)
    P = Q[:d]
    return d, first(0, n, lambda r: at(r, d) >= P), first(0, n, lambda r: at(r, d) > P)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rate, as_set, first = None, "--set" in sys.argv[1:], None
    for a in sys.argv[1:]:
        if a.startswith("--rate="):
            rate = float(a.split("=")[1])
        if a.startswith("--first="):
            first = int(a.split("=")[1])
    if rate is None:
        sys.exit("--rate=<G requests/s> is required: the gather4 rate tools/ubench_gather prints at the span of SA (tools/ubench_gather 27 28 for 2^28 uint32)")
    logn = int(args[0]) if len(args) > 0 else 28
    logq = int(args[1]) if len(args) > 1 else 20
    reps = int(args[2]) if len(args) > 2 else 7
    n, q, m, long_m = 1 << logn, 1 << logq, 32, 128
    stream = torch.cuda.Stream()
    ctx = psac_amd.Context(0, stream=stream.cuda_stream)
    lib, vp = ctx._lib, C.c_void_p
    d_text, d_sa, d_isa = ctx.alloc(n), ctx.alloc(n * 4), ctx.alloc(n * 4)
    ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, 0, 17, 1024))
    ctx._pre()
    d_ends, read = None, 0
    if as_set:
        read = READ
        soff = np.append(np.arange(0, n, READ, dtype=np.uint64), np.uint64(n))
        strings = int(soff.size - 1)
        d_soff = ctx.alloc(soff.nbytes); ctx.h2d(d_soff, soff)
        ctx.check(lib.psacx_construct_gsa_dev_u32(ctx.handle, vp(d_text), n, vp(d_soff), strings, 0, 0, vp(d_sa), vp(d_isa), None))
        d_ends = ctx.alloc(psac_amd.string_ends_device(ctx, None, strings, n, None) * 4)
        psac_amd.string_ends_device(ctx, d_soff, strings, n, d_ends)
    else:
        ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, 0, vp(d_sa), vp(d_isa), None))
    ctx.free(d_isa)
    ctx.check(lib.psacx_trim(ctx.handle))
    text, SA = np.empty(n, np.uint8), np.empty(n, np.uint32)
    ctx.d2h(text, d_text); ctx.d2h(SA, d_sa)
    print("n = 2^%d DNA%s, uint32, %d queries per batch, %d repeats, device %s"
          % (logn, " in reads of %d" % READ if as_set else "", q, reps, torch.cuda.get_device_name(0)))

    rng = np.random.RandomState(11)
    acgt = np.frombuffer(b"ACGT", np.uint8)

    def cut(count, length):                                 # shuffled as it is made; inside one read with --set
        if as_set:
            starts = rng.randint(0, n // READ, count).astype(np.int64) * READ + rng.randint(0, READ - min(length, READ) + 1, count)
        else:
            starts = rng.randint(0, n - length + 1, count).astype(np.int64)
        starts = np.minimum(starts, n - length)
        return text[(starts[:, None] + np.arange(length)[None, :]).reshape(-1)].copy()

    found = cut(q, m)
    one_off = found.copy()
    where = np.arange(q, dtype=np.int64) * m + rng.randint(0, m, q)
    one_off[where] = acgt[(np.searchsorted(acgt, one_off[where]) + rng.randint(1, 4, q)) % 4]       # always another letter
    reads = cut(q // long_m, long_m)
    where = rng.randint(0, reads.size, 4 * (q // long_m))
    reads[where] = acgt[rng.randint(0, 4, where.size)]
    # name: (pattern buffer, pattern length, suffix mode, max_len)
    batches = [("cut from the text", found, m, False, 0), ("cut, one byte substituted", one_off, m, False, 0),
               ("random", acgt[rng.randint(0, 4, q * m)], m, False, 0),
               ("every suffix of %d reads of %d, max_len 32" % (q // long_m, long_m), reads, long_m, True, 32),
               ("every suffix of %d reads of %d, uncapped" % (q // long_m, long_m), reads, long_m, True, 0)]
    d_len, d_lb, d_ub = ctx.alloc(q * 4), ctx.alloc(q * 4), ctx.alloc(q * 4)

    code, sigma, _ = psac_amd.lookup_table_device(ctx, d_text, n, None, 1, None, 32)
    B = sigma + 1
    ks = [10, 11] if B == 5 else [1, 2]
    tables = {}
    for k in ks:
        if as_set:
            entries = psac_amd.lookup_table_gsa_device(ctx, d_text, n, None, k, None, 32)[2]
            tables[k] = ctx.alloc(entries * 4)
            psac_amd.lookup_table_gsa_device(ctx, d_text, n, d_ends, k, tables[k], 32)
        else:
            entries = psac_amd.lookup_table_device(ctx, d_text, n, None, k, None, 32)[2]
            tables[k] = ctx.alloc(entries * 4)
            psac_amd.lookup_table_device(ctx, d_text, n, d_sa, k, tables[k], 32)

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

    sample = rng.randint(0, q, 1024)
    ln, lb, ub = np.empty(q, np.uint32), np.empty(q, np.uint32), np.empty(q, np.uint32)
    for name, buf, plen, suffixes, max_len in batches[:first]:
        count = buf.size // plen
        poff = np.arange(count + 1, dtype=np.uint64) * np.uint64(plen)
        d_pat, d_poff = ctx.alloc(buf.nbytes), ctx.alloc(poff.nbytes)
        ctx.h2d(d_pat, buf); ctx.h2d(d_poff, poff)
        flags = psac_amd.MATCH_SUFFIXES if suffixes else 0
        assert (buf.size if suffixes else count) == q

        def match(k):
            tb, cd = (tables[k], code) if k else (None, None)
            if as_set:
                psac_amd.match_gsa_device(ctx, d_text, n, d_ends, d_sa, tb, k, cd, d_pat, d_poff, count, flags, max_len, q, d_len, d_lb, d_ub, 32)
            else:
                psac_amd.match_device(ctx, d_text, n, d_sa, tb, k, cd, d_pat, d_poff, count, flags, max_len, q, d_len, d_lb, d_ub, 32)

        def locate(k):
            tb, cd = (tables[k], code) if k else (None, None)
            if as_set:
                psac_amd.locate_gsa_device(ctx, d_text, n, d_ends, d_sa, tb, k, cd, d_pat, d_poff, count, d_lb, d_ub, 32)
            else:
                psac_amd.locate_device(ctx, d_text, n, d_sa, tb, k, cd, d_pat, d_poff, count, d_lb, d_ub, 32)

        print("-- %s" % name)
        variants = []
        for k in [0] + ks:
            variants.append(("match k = %d" % k, (lambda k=k: match(k))))
            if not suffixes:
                variants.append(("locate k = %d" % k, (lambda k=k: locate(k))))
        res = timed(variants)
        os.environ["PSACX_LOCATE_COUNT"] = "1"
        for k in [0] + ks:
            ms = res["match k = %d" % k]
            med = float(np.median(ms))
            match(k)
            f = ctx.stats().locate_fetches
            per = (f[0] + f[1]) / float(q)
            floor_ms = q * per / (rate * 1e9) * 1e3
            ctx.d2h(ln, d_len); ctx.d2h(lb, d_lb); ctx.d2h(ub, d_ub)
            line = ("match  %-9s median %7.3f ms (least %7.3f, largest %7.3f) %8.2f M queries/s; %5.2f SA + %5.2f text = %6.2f fetches per query; "
                    "floor %6.3f ms; measured / floor %5.2f; mean len %5.2f" % ("no table" if k == 0 else "k = %d" % k, med, min(ms), max(ms), q / med / 1e3,
                                                                               f[0] / float(q), f[1] / float(q), per, floor_ms,
                                                                               med / floor_ms if floor_ms else 0.0, float(ln.mean())))
            print(line)
            if not suffixes:
                ls = res["locate k = %d" % k]
                lmed = float(np.median(ls))
                locate(k)
                g = ctx.stats().locate_fetches
                lper = (g[0] + g[1]) / float(q)
                print("locate %-9s median %7.3f ms (least %7.3f, largest %7.3f) %8.2f M queries/s; %5.2f SA + %5.2f text = %6.2f fetches per query; "
                      "time match / locate %5.2f; fetches match / locate %5.2f"
                      % ("no table" if k == 0 else "k = %d" % k, lmed, min(ls), max(ls), q / lmed / 1e3, g[0] / float(q), g[1] / float(q), lper, med / lmed,
                         per / lper if lper else 0.0))
            if k == ks[0]:                                  # the host check of a sample, once per batch (the tests compare the forms)
                bad = 0
                for i in sample:
                    if suffixes:
                        e = (int(i) // plen + 1) * plen
                        Q = buf[int(i):min(e, int(i) + max_len) if max_len else e].tobytes()
                    else:
                        Q = buf[int(i) * plen:(int(i) + 1) * plen].tobytes()
                    bad += host_answer(text, SA, Q, read) != (int(ln[i]), int(lb[i]), int(ub[i]))
                print("sample of 1024 wrong: %d" % bad)
                assert bad == 0
        del os.environ["PSACX_LOCATE_COUNT"]
        ctx.free(d_pat); ctx.free(d_poff)
    for p in [d_text, d_sa, d_len, d_lb, d_ub] + list(tables.values()):
        ctx.free(p)
    ctx.close()


if __name__ == "__main__":
    main()
