"""psacx_fm_index_dev_*, psacx_fm_count_dev_*, psacx_fm_occurrences_dev_* and what stands above them against tests/fm_model.py: the
blob word for word as the header lays it out, the intervals of locate for every pattern that occurs and (0, 0) otherwise, positions equal
to SA[lb .. ub) in order, for texts and sets of 1 .. 4097 bytes over alphabets of 1 .. 256 bytes, both widths, every sample rate; limits
and capacities; the refusals; garbage blobs; the Python and C++ mirrors and the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fm_model as F
import locate_gsa_model as G
from fm_gpu_common import SAMPLES, SIGMAS, SIZES, FmDev, expected, fm_case, named_case, patterns_of, pipeline_of
from rmq_gpu_common import Dev, SENTINEL, first_bad

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def check_case(ctx, c, bits, samples):
    dev = Dev(ctx, bits)
    try:
        d = FmDev(dev, c)
        pats = patterns_of(c)
        lb, ub = expected(c, pats)
        assert np.any(ub > lb) and (c.n < 3 or np.any(ub[1:] == 0))
        for sample in samples:
            blob = d.build(sample)
            p = pipeline_of(c, sample)
            want, Y = F.blob_of(p, bits // 8)
            i = d.info
            assert (int(i.n), int(i.words), int(i.sample), int(i.marks), int(i.sigma), int(i.bits)) == (c.n, Y["words"], sample, int(p.val.size), p.sigma, p.bits)
            assert np.array_equal(np.array(i.code[:], np.int64), p.code)
            assert 8 * int(i.words) <= F.size_bound_bytes(c.n, p.bits, sample, int(i.marks), bits // 8)
            assert first_bad(blob, want) is None, (c.n, p.sigma, sample)
            got = d.count(pats)
            assert first_bad(got[0], lb) is None and first_bad(got[1], ub) is None, (c.n, p.sigma, sample)
            if sample:
                d.check_occurrences(lb, ub)
                d.check_occurrences(lb, ub, limit=2)
                d.check_occurrences(np.arange(c.n), np.arange(c.n) + 1)            # every rank walks to a mark
            assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["text", "set"])
@pytest.mark.parametrize("n", SIZES)
def test_index_counts_and_positions(ctx, n, kind, bits):
    for sigma in SIGMAS + ([256] if n == 4097 else []):
        if sigma > n or (kind == "set" and n == 1 and sigma > 1):
            continue
        c = fm_case(kind, n, sigma)
        check_case(ctx, c, bits, [0] + SAMPLES + [n + 5] if sigma in (1, 4, 256) else [3, 32])


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", sorted(F.NAMED) + ["every_end"])
def test_named_sets(ctx, name, bits):
    c = named_case(name)
    p = pipeline_of(c, 2)
    assert name != "every_end" or all(int(p.E[s]) > 0 for s in range(1, p.sigma + 1))          # strings that end in every symbol
    check_case(ctx, c, bits, [0, 1, 2, 3, 8])
    if name in F.NAMED:
        dev = Dev(ctx, bits)
        try:
            d = FmDev(dev, c)
            d.build(2)
            rows = F.golden()[name]["patterns"]
            lb, ub = d.count([bytes(r["pattern"]) for r in rows])
            assert lb.tolist() == [r["lb"] for r in rows] and ub.tolist() == [r["ub"] for r in rows]
            total, start, pos, sid = d.occurrences(lb, ub)
            assert pos[:total].tolist() == sum((r["pos"] for r in rows), [])
        finally:
            dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_limits_capacities_and_hand_made_batches(ctx, bits):
    from test_gpu_occurrences import hand_made_batches, HAND_N
    import psac_amd
    c = fm_case("set", HAND_N, 4)
    dev = Dev(ctx, bits)
    try:
        d = FmDev(dev, c)
        d.build(32)
        for lb, ub, limit, _ in hand_made_batches():
            d.check_occurrences(lb, ub, limit)
        lb, ub = np.array([0, 7, 100]), np.array([50, 7, 300])
        total, start, pos, sid = d.occurrences(lb, ub, query=True)                   # the size query writes no list
        assert total == 250 and start.tolist() == [0, 50, 50, 250] and np.all(pos == SENTINEL) and np.all(sid == SENTINEL)
        with pytest.raises(psac_amd.PsacxError) as e:                                 # one slot short: start and the total are valid
            d.occurrences(lb, ub, cap=249)
        assert e.value.code == -2 and e.value.total == 250 and d.start.tolist() == [0, 50, 50, 250] and np.all(d.pos == SENTINEL)
        total, start, pos, sid = d.occurrences(lb, ub, sid=False)                     # without sid
        assert total == 250 and np.array_equal(pos[:250].astype(np.int64), np.concatenate((c.SA[0:50], c.SA[100:300]))) and np.all(sid == SENTINEL)
        assert d.occurrences([], [])[0] == 0 and d.start[0] == 0                      # q == 0
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_refusals(ctx, bits):
    import psac_amd
    from psac_amd import _lib
    c = fm_case("set", 65, 4)
    dev = Dev(ctx, bits)
    try:
        d = FmDev(dev, c)

        def code_of(call):
            with pytest.raises(psac_amd.PsacxError) as e:
                call()
            return e.value.code
        fm = psac_amd.fm_index_device
        assert code_of(lambda: fm(ctx, c.n, d.d_bwt, None, d.d_sa, 4, None, bits)) == -1                  # no first bitmap
        assert code_of(lambda: fm(ctx, c.n, d.d_bwt, d.d_first, None, 4, None, bits)) == -1               # samples without SA
        assert code_of(lambda: fm(ctx, c.n, None, d.d_first, None, 0, None, bits)) == -1
        assert code_of(lambda: fm(ctx, (1 << 32) if bits == 32 else (1 << 49), d.d_bwt, d.d_first, None, 0, None, bits)) == -2
        empty = fm(ctx, 0, None, d.d_first, None, 0, None, bits)                                              # n == 0 is an index
        assert int(empty.n) == 0 and int(empty.words) == F.layout(0, 1, 0, 0, bits // 8)["words"]
        d0 = FmDev(dev, c)
        d0.put_blob(np.zeros(int(empty.words), np.uint64), empty)
        lb, ub = d0.count([b"", b"A", b"ACGT"])
        assert lb.tolist() == [0, 0, 0] and ub.tolist() == [0, 0, 0]
        d.build(0)                                                                                            # counts only
        pats = patterns_of(c)
        want = expected(c, pats)
        got = d.count(pats)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert code_of(lambda: d.occurrences(want[0], want[1])) == -1
        d.build(3)
        good = d.info
        for field, delta in (("bits", 1), ("words", 1), ("words", -1), ("marks", 2), ("sigma", 60), ("n", 64), ("sample", -3)):
            bad = _lib.FmInfo.from_buffer_copy(bytes(good))
            setattr(bad, field, getattr(bad, field) + delta)
            d.info = bad
            assert code_of(lambda: d.count(pats)) == -1, field
            assert code_of(lambda: d.occurrences(want[0], want[1])) == -1, field
        bad = _lib.FmInfo.from_buffer_copy(bytes(good))
        bad.code[65] = 200                                                                                    # a code beyond sigma
        d.info = bad
        assert code_of(lambda: d.count(pats)) == -1
        d.info = good
        pat, off = psac_amd.pattern_buffer(pats)                                                             # malformed offsets: nothing written
        off[3] = off[5]
        d_pat, d_poff = dev.put(pat), dev.put(off)
        d_lb, d_ub = dev.put(np.full(len(pats), SENTINEL, dev.dt)), dev.put(np.full(len(pats), SENTINEL, dev.dt))
        assert code_of(lambda: psac_amd.fm_count_device(ctx, d.d_fm, good, d_pat, d_poff, len(pats), d_lb, d_ub, bits)) == -1
        assert np.all(dev.get(d_lb, len(pats)) == SENTINEL) and np.all(dev.get(d_ub, len(pats)) == SENTINEL)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_garbage_blobs_keep_the_totality_rules(ctx, bits):
    c = fm_case("set", 1000, 4, seed=7)
    ones = (1 << bits) - 1
    dev = Dev(ctx, bits)
    try:
        d = FmDev(dev, c)
        good = d.build(4).copy()
        info = d.info
        Y = d.layout()
        p = pipeline_of(c, 4)
        pats = patterns_of(c)
        rng = np.random.RandomState(bits)
        junk = rng.randint(0, 2 ** 32, 2 * good.size).astype(np.uint32).view(np.uint64)
        small = junk.copy()                             # random words below 2 n: ranks and tables that land inside more often
        small %= np.uint64(2 * c.n)
        val_ones = good.copy()
        val_ones[Y["val_at"]:] = np.uint64(0xFFFFFFFFFFFFFFFF)
        clear = good.copy()
        clear[Y["marks_at"]:Y["val_at"]] = 0
        ranks = np.arange(c.n)
        for name, blob in (("junk", junk), ("small", small), ("val", val_ones), ("clear", clear)):
            d.put_blob(blob, info)
            lb, ub = d.count(pats)
            assert np.all(0 <= lb) and np.all(lb <= ub) and np.all(ub <= c.n), name
            want = [F.blob_search(blob, Y, p.code, p.sigma, P) for P in pats]
            assert lb.tolist() == [x[0] for x in want] and ub.tolist() == [x[1] for x in want], name
            total, start, pos, sid = d.occurrences(ranks, ranks + 1)
            assert total == c.n
            walk = [F.blob_walk(blob, Y, p.sigma, r) for r in range(c.n)]
            assert pos[:total].tolist() == walk, name
            assert np.all((sid[:total] == c.m) == (pos[:total].astype(np.uint64) >= c.n)), name
            if name == "clear":
                assert walk == [ones] * c.n
            if name == "val":                           # the searches do not read val
                assert np.array_equal(lb, expected(c, pats)[0]) and np.array_equal(ub, expected(c, pats)[1])
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_python_mirrors_answer_after_the_suffix_array_is_gone(bits):
    import psac_amd
    ctx = psac_amd.Context(0)
    try:
        for kind in ("text", "set"):
            c = fm_case(kind, 4097, 4)
            pats = patterns_of(c)
            lb, ub = expected(c, pats)
            sa = psac_amd.SuffixArray(index_bits=bits, ctx=ctx)
            if c.single:
                sa.construct(c.text)
            else:
                sa.construct_ss(c.strings)
            assert np.array_equal(sa.local_SA.astype(np.int64), c.SA)
            fm = sa.fm_index(sample=8)
            counting = sa.fm_index(sample=0)
            assert counting.nbytes < fm.nbytes < c.n * (1 + bits // 8)
            sa.local_SA = sa.local_B = sa._text = None
            del sa
            ctx.check(ctx._lib.psacx_trim(ctx.handle))
            got = fm.count(pats)
            assert np.array_equal(got[0].astype(np.int64), lb) and np.array_equal(got[1].astype(np.int64), ub)
            got = counting.count(pats)
            assert np.array_equal(got[0].astype(np.int64), lb) and np.array_equal(got[1].astype(np.int64), ub)
            for limit in (0, 3):
                want = G.occurrences(c.SA.astype(np.uint64), c.n, lb.astype(np.uint64), ub.astype(np.uint64), limit)
                out = fm.locate(pats, limit=limit)
                assert np.array_equal(out[0], want[0]) and np.array_equal(out[1].astype(np.uint64), want[1])
                if not c.single:
                    assert np.array_equal(out[2].astype(np.uint64), G.string_ids(c.off.astype(np.uint64), want[1], c.n))
            with pytest.raises(psac_amd.PsacxError):
                counting.locate(pats)
            fm.free()
            counting.free()
            with pytest.raises(ValueError):
                fm.count(pats)
            dt = np.uint32 if bits == 32 else np.uint64
            off = None if c.single else c.off
            res = psac_amd.fm_search(c.text, c.SA.astype(dt), pats, sample=5, limit=0, offsets=off, ctx=ctx)
            want = G.occurrences(c.SA.astype(np.uint64), c.n, lb.astype(np.uint64), ub.astype(np.uint64), 0)
            assert np.array_equal(res[0].astype(np.int64), lb) and np.array_equal(res[1].astype(np.int64), ub)
            assert np.array_equal(res[2], want[0]) and np.array_equal(res[3].astype(np.uint64), want[1])
            if not c.single:
                assert np.array_equal(res[4].astype(np.uint64), G.string_ids(c.off.astype(np.uint64), want[1], c.n))
            res = psac_amd.fm_search(c.text, c.SA.astype(dt), pats, offsets=off, positions=False, ctx=ctx)
            assert np.array_equal(res[0].astype(np.int64), lb) and np.array_equal(res[1].astype(np.int64), ub)
            if not c.single:
                continue
            start, total = np.zeros(len(pats) + 1, np.uint64), C.c_uint64(0)                   # the capacity rule of the host-pointer form
            pat, poff = psac_amd.pattern_buffer(pats)
            one, l2, u2, t = np.zeros(1, dt), np.zeros(len(pats), dt), np.zeros(len(pats), dt), np.ascontiguousarray(c.text)
            s2 = c.SA.astype(dt)
            rc = getattr(ctx._lib, "psacx_fm_search_u%d" % bits)(ctx.handle, t.ctypes.data, c.n, None, 0, s2.ctypes.data, 5, pat.ctypes.data, poff.ctypes.data,
                                                                len(pats), l2.ctypes.data, u2.ctypes.data, 0, start.ctypes.data, one.ctypes.data, None, 0,
                                                                C.byref(total))
            assert rc == -2 and total.value == int(want[0][-1]) and np.array_equal(start, want[0]) and np.array_equal(l2.astype(np.int64), lb)
    finally:
        ctx.close()


def test_cpp_mirror_and_command_line(tmp_path):
    exe, lib = str(tmp_path / "test_fm"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fm.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "fm header tests passed" in r.stdout, r.stdout + r.stderr
    cli = os.path.join(ROOT, "psac_amd", "bin", "fmindex")
    c = named_case("miss3")
    pats = [bytes(x) for x in F.PATTERNS["miss3"] if x]
    (tmp_path / "set").write_bytes(b"".join(s + b"\n" for s in c.strings))
    (tmp_path / "pats").write_bytes(b"".join(p + b"\n" for p in pats))
    lb, ub = expected(c, pats)
    for index in ("32", "64"):
        for extra, limit in (([], None), (["--occ"], 0), (["--occ", "2", "-s", "3"], 2), (["-s", "0"], None)):
            r = subprocess.run([cli, "-f", str(tmp_path / "set"), "-q", str(tmp_path / "pats"), "--set", "--index", index] + extra, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            occ = None
            if limit is not None:
                start, pos = G.occurrences(c.SA.astype(np.uint64), c.n, lb.astype(np.uint64), ub.astype(np.uint64), limit)[:2]
                occ = (start, pos, G.string_ids(c.off.astype(np.uint64), pos, c.n))
            assert r.stdout == G.cli_text(lb, ub, occ, c.off if occ else None), (index, extra)
            assert "Index bytes: " in r.stderr and "(text + SA: %d)" % (c.n * (1 + int(index) // 8)) in r.stderr
    (tmp_path / "text").write_bytes(b"mississippi")
    (tmp_path / "p1").write_bytes(b"iss\nippi\nx\n")
    r = subprocess.run([cli, "-f", str(tmp_path / "text"), "-q", str(tmp_path / "p1"), "--occ", "-s", "2"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "2 4 4 1\n1 2 7\n0 0\n", r.stdout + r.stderr
