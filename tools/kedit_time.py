#!/usr/bin/env python3
"""Time of the pattern search with edits beside the search with mismatches on the same reads:
tools/kedit_time.py --rate=R --store-rate=S [log2 characters (28)] [log2 reads (20)] [repeats (5)].

The method of tools/kmismatch_time.py: the text generated in HBM (psacx_synth_text_dev), uint32, SA constructed there, the table
(k = 11) built by the library's own device call and resident; HIP events on the context's stream; after a warm-up call of every
variant the variants take turns inside every repeat; median, least and largest are printed.
Batches:
  - random DNA, 2^20 reads of 128 bytes cut from the text with 2 % of their bytes substituted, e = 2 and e = 4;
  - the same reads with 1 % substituted and 1 % single-byte insertions or deletions, e = 2 and e = 4;
  - the tandem repeat of period 1024, reads of 128 cut from it, e = 2: every piece occurs n / 1024 times.  First 16 reads with a max_cand
    that refuses the batch (the time of the guard), then 32 reads without it.
Per batch: the call stopped after the piece searches and the scan (PSACX_OPT_KEDIT_STOP 1), after the verification and the scan of the
raw hits (2), after the sort and the unique (3), the count query and the call that writes the lists (the same pipeline once more), with
work[0], work[1] and z; the stage times are the differences, repeat by repeat.  Beside them psacx_kmismatch_dev_* on the same batch,
count and lists: the ratio on the substitution-only batch is the price of allowing insertions and deletions.

The floor is read from the code, not profiled, stage by stage:
  pieces        the SA entries and text words the piece searches fetch (counted by PSACX_LOCATE_COUNT in a call of its own) / rate
  verification  instructions: a row of the band costs I(EB) instructions in the compiled loop (50, 76, 129, 229, 420 for EB = 1, 2, 4,
                8, 15); a candidate that yields raw hits walks all 128 rows, and there are at least raw / (2e + 1) of them; every other
                one walks at least e + 1 rows before every cell can exceed e.  Lane-instructions / (256 CUs x 64 lanes x 2.4 GHz).
  raw pairs     per raw hit two entries stored by neighbouring lanes, per candidate 12 bytes written and read once: streams at 8 TB/s
  sort, unique  the passes of the rank-pair sort over three entries per raw hit: 2 x 12 bytes per raw hit and pass at 8 TB/s, one pass
                per 8 bits of q - 1 and per 8 bits of n - 1 (a pass whose digit is constant is skipped)
  quadruples    per hit a forward pass of 128 rows in the band 2 EB + 1, about half the instructions of a verification row, and four
                stores / store rate
with rate = the gather4 line and store rate = the scatter8 line tools/ubench_gather prints at the span of the arrays.
A sample of the quadruples of every batch is verified on the host by the full dynamic programme from their start."""
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
ROW = {1: 50, 2: 76, 4: 129, 8: 229, 15: 420}           # instructions of a row of ked_verify_kernel's loop by bucket, from the gfx950 code
LANES = 256 * 64 * 2.4e9


def bucket(e):
    return min(b for b in ROW if b >= max(e, 1))


def verify(text, pat, poff, qid, tpos, ln, dist, e, rng, count=256):
    """the number of wrong quadruples in a sample: D and the smallest L by the full programme over L <= m + e + 1 from the start"""
    bad = 0
    for i in rng.randint(0, qid.size, min(count, qid.size)) if qid.size else []:
        j, t = int(qid[i]), int(tpos[i])
        P = pat[int(poff[j]):int(poff[j + 1])]
        W = text[t:t + P.size + e + 1].astype(np.int64)
        ar = np.arange(W.size + 1)
        F = ar.copy()
        for c in P:
            G = np.empty_like(F)
            G[0] = F[0] + 1
            G[1:] = np.minimum(F[:-1] + (W != c), F[1:] + 1)
            F = np.minimum.accumulate(G - ar) + ar
        bad += not (int(F.min()) == int(dist[i]) <= e and int(F.argmin()) == int(ln[i]))
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
    logr = int(args[1]) if len(args) > 1 else 20
    reps = int(args[2]) if len(args) > 2 else 5
    n, K = 1 << logn, 11
    stream = torch.cuda.Stream()
    ctx = psac_amd.Context(0, stream=stream.cuda_stream)
    lib, vp = ctx._lib, C.c_void_p
    rng = np.random.RandomState(11)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    G, St = rate * 1e9, store * 1e9
    print("n = 2^%d, uint32, reads of %d, k = %d, %d repeats, device %s" % (logn, READ, K, reps, torch.cuda.get_device_name(0)))

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
        print("%-36s median %9.3f ms (least %9.3f, largest %9.3f)%s" % (name, med, min(ms), max(ms), tail))

    def reads_of(text, reads, indels):
        """reads cut from the text: 2 % substituted, or 1 % substituted and 1 % single-byte insertions or deletions"""
        starts = rng.randint(8, n - READ - 8, reads).astype(np.int64)
        at = np.arange(READ, dtype=np.int64)[None, :] + np.zeros((reads, 1), np.int64)
        fresh = np.zeros((reads, READ), bool)
        if indels:
            ev = rng.rand(reads, READ) < 0.01
            gone = ev & (rng.rand(reads, READ) < 0.5)           # a text byte left out in front of this place
            fresh = ev & ~gone                                  # a byte put in at this place
            at += np.cumsum(gone, axis=1) - np.cumsum(fresh, axis=1)
        pat = text[(starts[:, None] + at).reshape(-1)].reshape(reads, READ)
        fresh |= rng.rand(reads, READ) < (0.01 if indels else 0.02)
        pat[fresh] = acgt[rng.randint(0, 4, int(fresh.sum()))]
        return pat.reshape(-1).copy()

    for kind, batches in ((0, [(1 << logr, 2, False), (1 << logr, 4, False), (1 << logr, 2, True), (1 << logr, 4, True)]),
                          (2, [(16, 2, False), (32, 2, False)])):
        d_text, d_sa, d_isa = ctx.alloc(n), ctx.alloc(n * 4), ctx.alloc(n * 4)
        ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), n, 0, kind, 17, 1024))
        ctx._pre()
        ctx.check(lib.psacx_construct_dev_u32(ctx.handle, vp(d_text), n, 0, 0, vp(d_sa), vp(d_isa), None))
        ctx.free(d_isa)
        ctx.check(lib.psacx_trim(ctx.handle))
        text = np.empty(n, np.uint8)
        ctx.d2h(text, d_text)
        k = K if kind == 0 else 0
        d_table = code = None
        if k:
            code, _, entries = psac_amd.lookup_table_device(ctx, d_text, n, None, k, None, 32)
            d_table = ctx.alloc(entries * 4)
            psac_amd.lookup_table_device(ctx, d_text, n, d_sa, k, d_table, 32)
        for reads, e, indels in batches:
            pat = reads_of(text, reads, indels)
            poff = np.arange(reads + 1, dtype=np.uint64) * np.uint64(READ)
            Q = reads * (e + 1)
            d_pat, d_poff = ctx.alloc(pat.size), ctx.alloc(poff.nbytes)
            ctx.h2d(d_pat, pat); ctx.h2d(d_poff, poff)
            work, mwork = [], []

            def ked(d_q=None, d_t=None, d_l=None, d_d=None, cap=0, max_cand=0):
                return psac_amd.kedit_device(ctx, d_text, n, None, d_sa, d_table, k, code, d_pat, d_poff, reads, e, max_cand, 0, d_q, d_t, d_l, d_d, cap, 32,
                                             work=work)

            def kmm(d_q=None, d_t=None, d_d=None, cap=0):
                return psac_amd.kmismatch_device(ctx, d_text, n, None, d_sa, d_table, k, code, d_pat, d_poff, reads, e, 0, d_q, d_t, d_d, cap, 32, work=mwork)

            def stopped(stage):
                def call():
                    os.environ["PSACX_KEDIT_STOP"] = str(stage)
                    try:
                        ked()
                    finally:
                        del os.environ["PSACX_KEDIT_STOP"]
                return call
            what = "random DNA" if kind == 0 else "tandem repeat, period 1024"
            how = "" if kind else (" with 1 % substituted and 1 % inserted or deleted" if indels else " with 2 % substituted")
            print("== %s, %d reads of %d%s, e = %d, %s" % (what, reads, READ, how, e, "k = %d" % k if k else "no table"))
            if kind == 2 and reads == 16:                   # the guard: refused before anything sized by the candidates exists
                stopped(1)()
                cands = work[0]

                def refused():
                    try:
                        ked(max_cand=cands - 1)
                    except psac_amd.PsacxError as err:
                        assert err.code == -2 and err.z == 0
                    else:
                        raise AssertionError("max_cand did not refuse the batch")
                res = timed([("refused", refused)])
                print("-- candidates = %d, max_cand = %d" % (cands, cands - 1))
                line("refused by max_cand", res["refused"], None)
                ctx.free(d_pat); ctx.free(d_poff)
                continue
            z = ked()
            cands, raw = work
            zm = kmm()
            room, mroom = max(z, 1), max(zm, 1)
            d_q, d_t, d_l, d_d = ctx.alloc(room * 8), ctx.alloc(room * 4), ctx.alloc(room * 4), ctx.alloc(room)
            m_q, m_t, m_d = ctx.alloc(mroom * 8), ctx.alloc(mroom * 4), ctx.alloc(mroom)
            res = timed([("stop1", stopped(1)), ("stop2", stopped(2)), ("stop3", stopped(3)), ("count", ked),
                         ("lists", lambda: ked(d_q, d_t, d_l, d_d, z)), ("kmm count", kmm), ("kmm lists", lambda: kmm(m_q, m_t, m_d, zm))])
            os.environ["PSACX_LOCATE_COUNT"] = "1"          # the fetches of the piece searches, in a call of its own
            stopped(1)()
            f = ctx.stats().locate_fetches
            del os.environ["PSACX_LOCATE_COUNT"]
            print("-- candidates = %d, raw hits = %d, z = %d; kmismatch: z = %d; the piece searches fetch %.2f SA entries + %.2f text words per piece"
                  % (cands, raw, z, zm, f[0] / float(Q), f[1] / float(Q)))
            diff = lambda a, b: [x - y for x, y in zip(res[a], res[b])]  # noqa: E731
            row = ROW[bucket(e)]
            true = min(cands, raw // (2 * e + 1))
            pieces = (f[0] + f[1]) / G * 1e3
            band = (true * READ + (cands - true) * (e + 1)) * row / LANES * 1e3
            pairs = (8 * raw + 2 * 12 * cands) / 8e12 * 1e3
            passes = -(-int(reads - 1).bit_length() // 8) + -(-int(n - 1).bit_length() // 8)
            sort = passes * 2 * 12 * raw / 8e12 * 1e3
            quads = (z * READ * row / 2 / LANES + 4 * z / St) * 1e3
            line("pieces, searches, scan", res["stop1"], pieces)
            line("verification, scan of raw hits", diff("stop2", "stop1"), band)
            line("raw pairs, sort, unique", diff("stop3", "stop2"), pairs + sort)
            line("count query", res["count"], pieces + band + pairs + sort)
            line("lists - count: quadruples", diff("lists", "count"), quads)
            line("lists", res["lists"], pieces + band + pairs + sort + quads)
            line("kmismatch, count", res["kmm count"], None)
            line("kmismatch, lists", res["kmm lists"], None)
            print("kedit / kmismatch: count %.2f, lists %.2f" % (np.median(res["count"]) / np.median(res["kmm count"]),
                                                                np.median(res["lists"]) / np.median(res["kmm lists"])))
            qid, tpos, ln, dist = np.empty(room, np.uint64), np.empty(room, np.uint32), np.empty(room, np.uint32), np.empty(room, np.uint8)
            ctx.d2h(qid, d_q); ctx.d2h(tpos, d_t); ctx.d2h(ln, d_l); ctx.d2h(dist, d_d)
            bad = verify(text, pat, poff, qid[:z], tpos[:z], ln[:z], dist[:z], e, rng)
            mq = np.empty(mroom, np.uint64)
            ctx.d2h(mq, m_q)
            print("reads with a hit: %d of %d (kmismatch: %d); sample of %d quadruples wrong: %d"
                  % (np.unique(qid[:z]).size, reads, np.unique(mq[:zm]).size, min(256, z), bad))
            assert bad == 0
            for p in (d_q, d_t, d_l, d_d, m_q, m_t, m_d, d_pat, d_poff):
                ctx.free(p)
        for p in [d_text, d_sa] + ([d_table] if d_table else []):
            ctx.free(p)
        ctx.check(lib.psacx_trim(ctx.handle))
    ctx.close()


if __name__ == "__main__":
    main()
