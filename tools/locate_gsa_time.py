#!/usr/bin/env python3
"""Time of the pattern search over a string set, of its bitmap and table, and of the occurrence lists:
tools/locate_gsa_time.py --rate=R [log2 characters (28)] [log2 patterns per kind (20)] [repeats (7)].

Random DNA generated in HBM and taken as reads of 100 characters, uint32, the generalized suffix array constructed there
(psacx_construct_gsa_dev_u32).  Two batches in shuffled order: patterns of length 32 cut from the reads (they occur) and random
patterns of length 32 (they do not).  Timed as tools/locate_time.py does: HIP events on the context's stream, after a warm-up call
of every variant, the variants taking turns inside every repeat; median, least and largest of the repeats are printed.
  1. psacx_string_ends_dev, and psacx_lookup_table_gsa_dev_u32 beside psacx_lookup_table_dev_u32 for k = 10 and 11.
  2. psacx_locate_gsa_dev_u32 beside psacx_locate_dev_u32 of the same build on the same text taken as one string (the plain suffix
     array is constructed too), without a table and with k = 10 and 11, the ratio of the two, and the fetch counts of the counting
     kernels (PSACX_OPT_LOCATE_COUNT; bitmap words are not counted).  What to expect: one more independent fetch per step, so a
     ratio close to 1.
  3. (The plain rows are what tools/locate_time.py prints for the reads' text; run it from the parent commit in the same session
     to see that the plain entry points have not moved.)
  4. psacx_occurrences_dev_u32: outputs per second and bytes per second (4 read + 4 written per output, start and lb aside) for
     two batches with the same total -- one occurrence for each of the patterns cut from the reads (limit = 1), and the four
     one-byte patterns with limit = total / 4 -- their ratio, and the first against --rate=<G requests/s>, the rate
     tools/ubench_gather prints for independent random 4-byte fetches at the span of SA (gather4 of `tools/ubench_gather 27 28`).
     The same pair again at 16 times the total, from hand-made intervals ([i, i + 1) at random i against four long ones).
A sample of 4096 patterns of every batch is verified on the host against the text, the offsets and the suffix array."""
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


def verify_sample(text, SA, pats, m, lb, ub, sample, read):
    """S[SA[lb]..end) starts with P where lb < ub, and neither SA[lb-1] nor SA[ub] does; read = 0: one text."""
    n = text.size
    bad = 0
    for i in sample:
        P = pats[i * m:(i + 1) * m].tobytes()

        def at(r):
            p = int(SA[r])
            e = n if not read else min(n, (p // read + 1) * read)
            return text[p:min(e, p + m)].tobytes()
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
    off = np.append(np.arange(0, n, READ, dtype=np.uint64), np.uint64(n))
    ms_ = int(off.size - 1)
    d_text, d_isa = ctx.alloc(n), ctx.alloc(n * 4)
    d_sa = {"set": ctx.alloc(n * 4), "plain": ctx.alloc(n * 4)}
    d_soff = ctx.alloc(off.nbytes); ctx.h2d(d_soff, off)
    ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, 0, 17, 1024))
    ctx._pre()
    ctx.check(lib.psacx_construct_gsa_dev_u32(ctx.handle, vp(d_text), n, vp(d_soff), ms_, 0, 0, vp(d_sa["set"]), vp(d_isa), None))
    ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, 0, vp(d_sa["plain"]), vp(d_isa), None))
    ctx.free(d_isa)
    ctx.check(lib.psacx_trim(ctx.handle))
    text = np.empty(n, np.uint8)
    SA = {k: np.empty(n, np.uint32) for k in d_sa}
    ctx.d2h(text, d_text)
    for k in d_sa:
        ctx.d2h(SA[k], d_sa[k])
    print("n = 2^%d DNA in %d reads of %d, uint32, %d patterns of length %d per batch, %d repeats, device %s"
          % (logn, ms_, READ, q, m, reps, torch.cuda.get_device_name(0)))

    rng = np.random.RandomState(11)
    starts = (rng.randint(0, n // READ, q).astype(np.int64) * READ + rng.randint(0, READ - m + 1, q))         # inside one read each
    batches = {"cut from the reads": text[(starts[:, None] + np.arange(m)[None, :]).reshape(-1)].copy(),
               "random": np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, q * m)]}
    poff = (np.arange(q + 1, dtype=np.uint64) * np.uint64(m))
    d_poff = ctx.alloc(poff.nbytes); ctx.h2d(d_poff, poff)
    d_pat = {k: ctx.alloc(v.nbytes) for k, v in batches.items()}
    for k, v in batches.items():
        ctx.h2d(d_pat[k], v)
    d_lb, d_ub = ctx.alloc(q * 4), ctx.alloc(q * 4)
    words = psac_amd.string_ends_device(ctx, None, ms_, n, None)
    d_ends = ctx.alloc(words * 4)

    code, sigma, _ = psac_amd.lookup_table_device(ctx, d_text, n, None, 1, None, 32)
    B = sigma + 1
    ks = [10, 11] if B == 5 else [1, 2]
    tables = {}
    for k in ks:
        entries = psac_amd.lookup_table_device(ctx, d_text, n, None, k, None, 32)[2]
        tables[("set", k)], tables[("plain", k)] = ctx.alloc(entries * 4), ctx.alloc(entries * 4)

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

    def show(name, ms, per=None, unit="M patterns/s"):
        med = float(np.median(ms))
        extra = "" if per is None else "  %8.2f %s" % (per / med / 1e3, unit)
        print("%-58s median %8.3f ms  (least %8.3f, largest %8.3f)%s" % (name, med, min(ms), max(ms), extra))
        return med

    print("-- 1. bitmap and tables")
    variants = [("psacx_string_ends_dev (%d words)" % words, (lambda: psac_amd.string_ends_device(ctx, d_soff, ms_, n, d_ends)))]
    for k in ks:
        variants.append(("psacx_lookup_table_gsa_dev_u32 k = %d (%d entries)" % (k, B ** k + 1),
                         (lambda k=k: psac_amd.lookup_table_gsa_device(ctx, d_text, n, d_ends, k, tables[("set", k)], 32))))
        variants.append(("psacx_lookup_table_dev_u32 k = %d" % k,
                         (lambda k=k: psac_amd.lookup_table_device(ctx, d_text, n, None, k, tables[("plain", k)], 32))))
    for name, ms in timed(variants).items():
        show(name, ms)

    def run(kind, batch, k):
        t = tables[(kind, k)] if k else None
        if kind == "set":
            psac_amd.locate_gsa_device(ctx, d_text, n, d_ends, d_sa[kind], t, k, code if k else None, d_pat[batch], d_poff, q, d_lb, d_ub, 32)
        else:
            psac_amd.locate_device(ctx, d_text, n, d_sa[kind], t, k, code if k else None, d_pat[batch], d_poff, q, d_lb, d_ub, 32)

    os.environ["PSACX_LOCATE_SHAPE"] = "lane"
    lb, ub = np.empty(q, np.uint32), np.empty(q, np.uint32)
    sample = rng.randint(0, q, 4096)
    label = {"set": "string set", "plain": "one text  "}
    for batch in batches:
        print("-- 2. patterns %s" % batch)
        variants = [("%s, %s" % (label[kind], "no table" if k == 0 else "k = %d" % k), (lambda kind=kind, k=k: run(kind, batch, k)))
                    for k in [0] + ks for kind in ("set", "plain")]
        med = {name: show(name, ms, q) for name, ms in timed(variants).items()}
        os.environ["PSACX_LOCATE_COUNT"] = "1"
        for k in [0] + ks:
            f = {}
            for kind in ("set", "plain"):
                run(kind, batch, k)
                f[kind] = list(ctx.stats().locate_fetches)
                ctx.d2h(lb, d_lb); ctx.d2h(ub, d_ub)
                bad = verify_sample(text, SA[kind], batches[batch], m, lb, ub, sample, READ if kind == "set" else 0)
                assert bad == 0, (kind, k, bad)
                found = int((ub > lb).sum())
                f[kind].append(found)
            tag = "no table" if k == 0 else "k = %d" % k
            a, b = med["%s, %s" % (label["set"], tag)], med["%s, %s" % (label["plain"], tag)]
            print("%-10s string set / one text = %5.3f; fetches per pattern (SA entries + text words): set %6.2f + %6.2f, one text %6.2f + %6.2f; "
                  "found %d / %d of %d; samples of 4096 wrong: 0"
                  % (tag, a / b, f["set"][0] / float(q), f["set"][1] / float(q), f["plain"][0] / float(q), f["plain"][1] / float(q),
                     f["set"][2], f["plain"][2], q))
        del os.environ["PSACX_LOCATE_COUNT"]

    print("-- 4. occurrence lists (psacx_occurrences_dev_u32; SA of the set)")
    run("set", "cut from the reads", ks[-1])                                    # d_lb / d_ub: every pattern occurs
    d_start = ctx.alloc((q + 1) * 8)
    one = np.frombuffer(b"ACGT", np.uint8)
    d_one, d_one_off = ctx.alloc(4), ctx.alloc(5 * 8)
    ctx.h2d(d_one, one); ctx.h2d(d_one_off, np.arange(5, dtype=np.uint64))
    d_lb4, d_ub4, d_start4 = ctx.alloc(16), ctx.alloc(16), ctx.alloc(5 * 8)
    psac_amd.locate_gsa_device(ctx, d_text, n, d_ends, d_sa["set"], None, 0, None, d_one, d_one_off, 4, d_lb4, d_ub4, 32)
    big = 16 * q
    at = rng.randint(0, n, big).astype(np.uint32)
    d_lbh, d_ubh, d_starth = ctx.alloc(big * 4), ctx.alloc(big * 4), ctx.alloc((big + 1) * 8)
    ctx.h2d(d_lbh, at); ctx.h2d(d_ubh, at + np.uint32(1))
    d_pos = ctx.alloc(big * 4)

    def occ(d_l, d_u, count, limit, d_st, want):
        got = psac_amd.occurrences_device(ctx, d_sa["set"], n, None, 0, d_l, d_u, count, limit, d_st, d_pos, None, want, 32)
        assert got == want, (got, want)

    for total, many, few in ((q, (d_lb, d_ub, q, 1, d_start), (d_lb4, d_ub4, 4, q // 4, d_start4)),
                             (big, (d_lbh, d_ubh, big, 0, d_starth), (d_lb4, d_ub4, 4, big // 4, d_start4))):
        names = ("%d intervals, one occurrence each" % many[2], "4 one-byte patterns, %d occurrences each" % few[3])
        res = timed([(names[0], (lambda: occ(*many, want=total))), (names[1], (lambda: occ(*few, want=total)))])
        med = [show(nm, res[nm], total, "M outputs/s") for nm in names]
        print("total %d outputs: %.2f / %.2f G outputs/s = %.2f / %.2f GB/s; skewed / even = %.3f; even batch against %.1f G independent fetches/s: %.2f"
              % (total, total / med[0] / 1e6, total / med[1] / 1e6, 8 * total / med[0] / 1e6, 8 * total / med[1] / 1e6, med[1] / med[0], rate,
                 total / med[0] / 1e6 / rate))
    ctx.close()


if __name__ == "__main__":
    main()
