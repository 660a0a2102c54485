#!/usr/bin/env python3
"""Time of the pattern search with mismatches beside what a user pays today for the same pieces:
tools/kmismatch_time.py --rate=R --store-rate=S [log2 characters (28)] [log2 reads (13)] [repeats (7)].

The method of tools/mems_time.py: the text generated in HBM (psacx_synth_text_dev), uint32, SA constructed there, the table built by
the library's own device call and resident; HIP events on the context's stream; after a warm-up call of every variant the variants
take turns inside every repeat; median, least and largest are printed.
Batches:
  - random DNA, 2^13 reads of 128 bytes cut from the text with 2 % of their bytes substituted, e = 2 and e = 4, k = 11 and no table;
  - the same with 2^20 reads;
  - the tandem repeat of period 1024, reads of 128 cut from it, e = 2: every piece occurs n / 1024 times, so 16 reads own 48 x 2^18
    candidates.  First with a max_cand that refuses the batch (the time of the guard), then 128 reads without it: 0.1 G candidates,
    whose mark bytes stay below half a GiB.
Per batch: the call stopped after the piece searches and the scan (PSACX_OPT_KMISMATCH_STOP 1) and after the marks (2), the count
query and the call that writes the lists (which repeats the count), with work[0], work[1] and z; the stage times are the
differences, repeat by repeat.  Beside them psacx_locate_dev_* plus psacx_occurrences_dev_* over the same pieces (their offsets made
on the host): what the existing calls take before any byte is verified.

The fetch floor is read from the code, not profiled, stage by stage:
  pieces        the SA entries and text words the piece searches fetch (counted by PSACX_LOCATE_COUNT in a call of its own) / rate
  marks         per candidate one SA entry and one text word; per hit ceil(m / 8) - 1 text words more: (2 c + 15 z) / rate
  tile counts   the mark bytes streamed once at 8 TB/s, and the scan
  triples       per hit one SA entry / rate and three stores / store rate
with rate = the gather4 line and store rate = the scatter8 line tools/ubench_gather prints at the span of the arrays.
A sample of the triples of every batch is verified on the host by byte comparison."""
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


def verify(text, pat, qid, tpos, dist, e, rng, count=1024):
    """the number of wrong triples in a sample: the window lies in the text and differs from the read in exactly dist <= e bytes"""
    bad = 0
    for i in rng.randint(0, qid.size, min(count, qid.size)) if qid.size else []:
        j, t, d = int(qid[i]), int(tpos[i]), int(dist[i])
        ok = t + READ <= text.size and d <= e and int(np.sum(pat[j * READ:(j + 1) * READ] != text[t:t + READ])) == d
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
    G, St = rate * 1e9, store * 1e9
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

    def line(name, ms, fl):
        med = float(np.median(ms))
        tail = "" if fl is None else "; floor %8.3f ms; %s" % (fl, "measured / floor %6.2f" % (med / fl) if fl >= 0.005 else "no ratio: the floor is below 5 us")
        print("%-34s median %9.3f ms (least %9.3f, largest %9.3f)%s" % (name, med, min(ms), max(ms), tail))

    tandem_reads = 128
    for kind, batches in ((0, [(1 << logr, 2, 11), (1 << logr, 2, 0), (1 << logr, 4, 11), (1 << logr, 4, 0), (1 << 20, 2, 11), (1 << 20, 4, 11)]),
                          (2, [(16, 2, 0), (tandem_reads, 2, 0)])):
        d_text, d_sa, d_isa = ctx.alloc(n), ctx.alloc(n * 4), ctx.alloc(n * 4)
        ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, kind, 17, 1024))
        ctx._pre()
        ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, 0, vp(d_sa), vp(d_isa), None))
        ctx.free(d_isa)
        ctx.check(lib.psacx_trim(ctx.handle))
        text = np.empty(n, np.uint8)
        ctx.d2h(text, d_text)
        tables = {}
        for reads, e, k in batches:
            if k and k not in tables:
                code, _, entries = psac_amd.lookup_table_device(ctx, d_text, n, None, k, None, 32)
                tables[k] = (ctx.alloc(entries * 4), code)
                psac_amd.lookup_table_device(ctx, d_text, n, d_sa, k, tables[k][0], 32)
            d_table, code = tables[k] if k else (None, None)
            starts = rng.randint(0, n - READ + 1, reads).astype(np.int64)
            pat = text[(starts[:, None] + np.arange(READ)[None, :]).reshape(-1)].copy()
            if kind == 0:
                where = rng.randint(0, pat.size, pat.size // 50)
                pat[where] = acgt[rng.randint(0, 4, where.size)]
            poff = np.arange(reads + 1, dtype=np.uint64) * np.uint64(READ)
            cuts = np.array([i * READ // (e + 1) for i in range(e + 1)], np.uint64)
            boff = np.concatenate([(poff[:-1, None] + cuts[None, :]).reshape(-1), poff[-1:]])
            Q = reads * (e + 1)
            d_pat, d_poff, d_boff = ctx.alloc(pat.size), ctx.alloc(poff.nbytes), ctx.alloc(boff.nbytes)
            ctx.h2d(d_pat, pat); ctx.h2d(d_poff, poff); ctx.h2d(d_boff, boff)
            d_lb, d_ub, d_start = ctx.alloc(Q * 4), ctx.alloc(Q * 4), ctx.alloc((Q + 1) * 8)
            work = []

            def kmm(d_q=None, d_t=None, d_d=None, cap=0, max_cand=0):
                return psac_amd.kmismatch_device(ctx, d_text, n, None, d_sa, d_table, k, code, d_pat, d_poff, reads, e, max_cand, d_q, d_t, d_d, cap, 32,
                                                 work=work)

            def stopped(stage):
                def call():
                    os.environ["PSACX_KMISMATCH_STOP"] = str(stage)
                    try:
                        kmm()
                    finally:
                        del os.environ["PSACX_KMISMATCH_STOP"]
                return call
            print("== %s, %d reads of %d%s, e = %d, %s" % ("random DNA" if kind == 0 else "tandem repeat, period 1024", reads, READ,
                                                        " with 2 % substituted" if kind == 0 else "", e, "k = %d" % k if k else "no table"))
            if kind == 2 and reads == 16:                   # the guard: refused before anything sized by the candidates exists
                stopped(1)()
                cands = work[0]

                def refused():
                    try:
                        kmm(max_cand=cands - 1)
                    except psac_amd.PsacxError as err:
                        assert err.code == -2 and err.z == 0
                    else:
                        raise AssertionError("max_cand did not refuse the batch")
                res = timed([("refused", refused)])
                print("-- candidates = %d, max_cand = %d" % (cands, cands - 1))
                line("refused by max_cand", res["refused"], None)
            z = kmm()
            cands, tested = work
            room = max(z, 1)
            d_q, d_t, d_d = ctx.alloc(room * 8), ctx.alloc(room * 4), ctx.alloc(room)
            pos_total = [0]

            def today(expand):
                def call():
                    psac_amd.locate_device(ctx, d_text, n, d_sa, d_table, k, code, d_pat, d_boff, Q, d_lb, d_ub, 32)
                    pos_total[0] = psac_amd.occurrences_device(ctx, d_sa, n, None, 0, d_lb, d_ub, Q, 0, d_start, d_pos if expand else None, None, cands, 32)
                return call
            d_pos = ctx.alloc(max(cands, 1) * 4)
            res = timed([("stop1", stopped(1)), ("stop2", stopped(2)), ("count", kmm), ("lists", lambda: kmm(d_q, d_t, d_d, z)),
                         ("today count", today(False)), ("today lists", today(True))])
            assert pos_total[0] == cands
            os.environ["PSACX_LOCATE_COUNT"] = "1"          # the fetches of the piece searches, in a call of its own
            stopped(1)()
            f = ctx.stats().locate_fetches
            del os.environ["PSACX_LOCATE_COUNT"]
            print("-- candidates = %d, tested = %d, z = %d; the piece searches fetch %.2f SA entries + %.2f text words per piece"
                  % (cands, tested, z, f[0] / float(Q), f[1] / float(Q)))
            diff = lambda a, b: [x - y for x, y in zip(res[a], res[b])]  # noqa: E731
            pieces = (f[0] + f[1]) / G * 1e3
            marks = (2 * cands + (READ // 8 - 1) * z) / G * 1e3
            tiles = cands / 8e12 * 1e3
            emit = (z / G + 3 * z / St) * 1e3
            line("pieces, searches, scan", res["stop1"], pieces)
            line("marks", diff("stop2", "stop1"), marks)
            line("tile counts, scan", diff("count", "stop2"), tiles)
            line("count query", res["count"], pieces + marks + tiles)
            line("lists - count: triples", diff("lists", "count"), emit)
            line("lists", res["lists"], pieces + marks + tiles + emit)
            line("locate + occurrences, count", res["today count"], pieces)
            line("locate + occurrences, positions", res["today lists"], pieces + (cands / G + cands / St) * 1e3)
            qid, tpos, dist = np.empty(room, np.uint64), np.empty(room, np.uint32), np.empty(room, np.uint8)
            ctx.d2h(qid, d_q); ctx.d2h(tpos, d_t); ctx.d2h(dist, d_d)
            bad = verify(text, pat, qid[:z], tpos[:z], dist[:z], e, rng)
            found = np.unique(qid[:z]).size
            print("reads with a hit: %d of %d; sample of %d triples wrong: %d" % (found, reads, min(1024, z), bad))
            assert bad == 0
            for p in (d_q, d_t, d_d, d_pos, d_pat, d_poff, d_boff, d_lb, d_ub, d_start):
                ctx.free(p)
        for p in [d_text, d_sa] + [t[0] for t in tables.values()]:
            ctx.free(p)
        ctx.check(lib.psacx_trim(ctx.handle))
    ctx.close()


if __name__ == "__main__":
    main()
