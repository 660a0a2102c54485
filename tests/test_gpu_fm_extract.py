"""psacx_fm_text_samples_dev_*, psacx_fm_extract_dev_* and what stands above them against tests/fm_extract_model.py: the sample array
entry by entry, every string restored, every position as a query of its own, one query over everything, windows at every edge (empty,
from a string's last byte, up to a block boundary, up to and past a string's end, at and beyond n, in strings shorter than the rate),
for texts and sets of 1 .. 4097 bytes over alphabets of 1, 4 and 256 bytes, both widths, every rate; the size query and the capacity
rule; the refusals; garbage samples and blobs; the Python and C++ mirrors and fmindex --restore / --context."""
import os
import subprocess

import numpy as np
import pytest

import fm_extract_model as X
import fm_model as F
from fm_extract_gpu_common import FILL8, RATES, ExtDev, whole_strings, windows_of
from fm_gpu_common import FILL64, SIZES, fm_case, named_case, patterns_of, pipeline_of
from rmq_gpu_common import Dev, first_bad

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


def check_case(ctx, c, bits, rates):
    dev = Dev(ctx, bits)
    try:
        d = ExtDev(dev, c)
        d.build(0)                                      # the extraction reads neither marks nor val
        strings = c.strings
        for rate in rates:
            ts = d.samples(rate)
            assert first_bad(ts, X.sample_arrays(strings, c.SA, rate)) is None, (c.n, rate)
            assert d.check(*whole_strings(c)) == c.n
            assert d.check(np.arange(c.n), np.ones(c.n, np.int64)) == c.n
            d.check([0], [c.n])
            d.check(*windows_of(c, rate))
            assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["text", "set"])
@pytest.mark.parametrize("n", SIZES)
def test_samples_strings_positions_and_windows(ctx, n, kind, bits):
    for sigma in [1, 4] + ([256] if n == 4097 else []):
        if sigma > n or (kind == "set" and n == 1 and sigma > 1):
            continue
        c = fm_case(kind, n, sigma)
        if kind == "set" and n == 4097:
            lens = np.diff(c.off)
            assert lens.min() == 1 and 32 < lens.max() < 64                # strings of one byte, strings shorter than the rate, and longer
        check_case(ctx, c, bits, RATES + [n + 5])


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", sorted(F.NAMED) + ["every_end"])
def test_named_sets(ctx, name, bits):
    c = named_case(name)
    check_case(ctx, c, bits, [1, 2, 3, 8])
    if name in F.NAMED:
        gold = X.golden()[name]
        assert gold["SA"] == c.SA.tolist()
        dev = Dev(ctx, bits)
        try:
            d = ExtDev(dev, c)
            d.build(0)
            for rate in X.RATES:
                assert d.samples(rate).tolist() == gold["ts"][str(rate)]
                total, start, out = d.extract(*whole_strings(c))
                assert [out[int(start[j]):int(start[j + 1])].tobytes() for j in range(c.m)] == c.strings
        finally:
            dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_size_query_and_capacity(ctx, bits):
    import psac_amd
    c = fm_case("set", 4097, 4)
    dev = Dev(ctx, bits)
    try:
        d = ExtDev(dev, c)
        d.build(0)
        d.samples(32)
        pos, ln = windows_of(c, 32)
        want = X.by_bytes(c.strings, pos, ln)
        total, start, out = d.extract(pos, ln, query=True)                            # the size query writes no byte
        assert total == int(want[0][-1]) and np.array_equal(start, want[0]) and np.all(out == FILL8)
        with pytest.raises(psac_amd.PsacxError) as e:                                 # one byte short: start and the total are valid
            d.extract(pos, ln, cap=total - 1)
        assert e.value.code == -2 and e.value.total == total and np.array_equal(d.start, want[0]) and np.all(d.out == FILL8)
        assert d.extract([], [])[0] == 0 and d.start[0] == 0                          # q == 0
        assert d.extract([c.n, c.n + 1, 0], [4, 4, 0])[0] == 0 and d.start.tolist() == [0, 0, 0, 0] and np.all(d.out == FILL8)
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
        d = ExtDev(dev, c)
        d.build(3)
        d.samples(4)
        pos, ln = windows_of(c, 4)
        big = (1 << 32) if bits == 32 else (1 << 49)

        def code_of(call):
            with pytest.raises(psac_amd.PsacxError) as e:
                call()
            return e.value.code
        ts = psac_amd.fm_text_samples_device
        assert code_of(lambda: ts(ctx, c.n, d.d_sa, d.d_off, d.m, 0, d.d_ts, bits)) == -1                     # rate 0
        assert code_of(lambda: ts(ctx, c.n, d.d_sa, d.d_off, d.m, 0, None, bits)) == -1
        assert code_of(lambda: ts(ctx, c.n, None, d.d_off, d.m, 4, d.d_ts, bits)) == -1                       # no SA
        assert code_of(lambda: ts(ctx, c.n, d.d_sa, d.d_off, 0, 4, d.d_ts, bits)) == -1                       # m out of range
        assert code_of(lambda: ts(ctx, c.n, d.d_sa, d.d_off, c.n + 1, 4, d.d_ts, bits)) == -1
        assert code_of(lambda: ts(ctx, big, d.d_sa, None, 0, 4, None, bits)) == -2                            # n beyond the index type
        assert ts(ctx, 0, None, None, 0, 4, None, bits) == 1 and ts(ctx, 0, None, None, 0, 4, d.d_ts, bits) == 1      # n == 0
        assert ts(ctx, c.n, None, None, 0, c.n + 5, None, bits) == 1 and ts(ctx, c.n, None, d.d_off, d.m, 4, None, bits) == c.n // 4 + d.m
        bad_off = d.off.copy()
        bad_off[3] = bad_off[2]                                                                               # malformed offsets: nothing written
        d_bad = dev.put(bad_off)
        assert code_of(lambda: ts(ctx, c.n, d.d_sa, d_bad, d.m, 4, d.d_ts, bits)) == -1
        good_off = d.d_off
        d.d_off = d_bad
        assert code_of(lambda: d.extract(pos, ln)) == -1 and np.all(d.out == FILL8) and np.all(d.start == FILL64)
        d.d_off = good_off
        assert d.unchanged()
        good_rate, good_ts = d.rate, d.d_ts
        d.rate = 0
        assert code_of(lambda: d.extract(pos, ln)) == -1
        d.rate, d.d_ts = good_rate, None
        assert code_of(lambda: d.extract(pos, ln)) == -1
        d.d_ts = good_ts
        good = d.info
        for field, delta, code in (("bits", 1, -1), ("words", 1, -1), ("words", -1, -1), ("marks", 2, -1), ("sigma", 60, -1), ("n", 64, -1),
                                   ("n", big, -2)):
            bad = _lib.FmInfo.from_buffer_copy(bytes(good))
            setattr(bad, field, getattr(bad, field) + delta)
            d.info = bad
            assert code_of(lambda: d.extract(pos, ln)) == code, field
            assert np.all(d.out == FILL8)
        bad = _lib.FmInfo.from_buffer_copy(bytes(good))
        bad.code[65] = 200                                                                                    # a code beyond sigma
        d.info = bad
        assert code_of(lambda: d.extract(pos, ln)) == -1
        d.info = good
        d.check(pos, ln)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_garbage_samples_and_blobs_keep_the_totality_rules(ctx, bits):
    c = fm_case("set", 1000, 4, seed=7)
    dev = Dev(ctx, bits)
    try:
        d = ExtDev(dev, c)
        good = d.build(0).copy()
        info, Y, p = d.info, d.layout(), pipeline_of(c, 0)
        rng = np.random.RandomState(bits)
        junk = rng.randint(0, 2 ** 32, 2 * good.size).astype(np.uint32).view(np.uint64)
        small = junk % np.uint64(2 * c.n)               # random words below 2 n: ranks and tables that land inside more often
        whole = whole_strings(c)
        wins = windows_of(c, 5)
        pos = np.concatenate((whole[0], np.arange(0, c.n, 3), wins[0]))
        ln = np.concatenate((whole[1], np.ones(len(range(0, c.n, 3)), np.int64), wins[1]))
        want = X.by_bytes(c.strings, pos, ln)
        for rate in (5, 32):
            ts = d.samples(rate)
            ones = np.full(ts.size, (1 << bits) - 1, np.uint64)
            for name, blob, samples in (("good", good, ts), ("ones", good, ones), ("random samples", good, rng.randint(0, 2 * c.n, ts.size)),
                                        ("junk", junk, ts), ("small", small, ts), ("small, random samples", small, rng.randint(0, 2 * c.n, ts.size))):
                d.put_blob(blob, info)
                d.put_samples(samples, rate)
                total, start, out = d.extract(pos, ln)                     # (returns PSACX_OK: the wrapper raises otherwise)
                assert total == int(want[0][-1]) and np.array_equal(start, want[0]), name
                assert np.all(out[total:] == FILL8), name
                model = X.blob_extract(blob, Y, p.code, p.sigma, d.ts, rate, c.off, pos, ln)
                assert np.array_equal(out[:total], model[1]), (name, rate)
                if name == "good":
                    assert np.array_equal(out[:total], want[1])
                if name == "ones":
                    assert not out[:total].any()
                assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_python_mirrors_give_the_text_back_after_text_and_suffix_array_are_gone(bits):
    import psac_amd
    ctx = psac_amd.Context(0)
    try:
        for kind in ("text", "set"):
            c = fm_case(kind, 4097, 4)
            sa = psac_amd.SuffixArray(index_bits=bits, ctx=ctx)
            if c.single:
                sa.construct(c.text)
            else:
                sa.construct_ss(c.strings)
            plain = sa.fm_index(sample=8)
            fm = sa.fm_index(sample=8, text_rate=32)
            assert fm.nbytes == plain.nbytes + (c.n // 32 + c.m) * (bits // 8)
            sa.local_SA = sa.local_B = sa._text = None
            del sa
            ctx.check(ctx._lib.psacx_trim(ctx.handle))
            assert fm.text() == (c.strings[0] if c.single else c.strings)
            pos, ln = windows_of(c, 32)
            want = X.by_bytes(c.strings, pos, ln)
            got = fm.extract(pos, ln)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            got = fm.extract(pos, 7)                                                   # one length for all
            want = X.by_bytes(c.strings, pos, [7] * len(pos))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            pats = [P for P in patterns_of(c) if P][:30]
            for limit in (0, 3):
                res = fm.context(pats, 4, limit=limit)
                loc = fm.locate(pats, limit=limit)
                assert len(res) == len(loc) + 2 and all(np.array_equal(a, b) for a, b in zip(res, loc))
                wstart, out = res[-2], res[-1]
                start, occ = res[0].astype(np.int64), res[1].astype(np.int64)
                assert occ.size and wstart.size == occ.size + 1
                for j, P in enumerate(pats):
                    for o in range(int(start[j]), int(start[j + 1])):
                        sid = int(np.searchsorted(c.off, occ[o], side="right")) - 1
                        a, b = max(int(c.off[sid]), int(occ[o]) - 4), min(int(c.off[sid + 1]), int(occ[o]) + len(P) + 4)
                        assert out[int(wstart[o]):int(wstart[o + 1])].tobytes() == c.text[a:b].tobytes(), (P, o)
            for call in (lambda: plain.extract([0], [1]), plain.text, lambda: plain.context(pats, 4)):
                with pytest.raises(ValueError):
                    call()
            assert np.array_equal(plain.count(pats)[0], fm.count(pats)[0])           # text_rate = 0 changes nothing
            fm.free()
            plain.free()
            with pytest.raises(ValueError):
                fm.extract([0], [1])
    finally:
        ctx.close()


def test_cpp_mirror_and_command_line(tmp_path):
    exe, lib = str(tmp_path / "test_fm_extract"), os.path.join(ROOT, "psac_amd", "lib")
    b = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_fm_extract.cpp"),
                        "-L" + lib, "-lpsacx", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "fm extract header tests passed" in r.stdout, r.stdout + r.stderr
    cli = os.path.join(ROOT, "psac_amd", "bin", "fmindex")
    c = fm_case("set", 4097, 4)
    (tmp_path / "set").write_bytes(b"".join(s + b"\n" for s in c.strings))             # (the bytes of this case are no newlines)
    (tmp_path / "text").write_bytes(fm_case("text", 4097, 256).text.tobytes())         # every byte value, newlines among them
    (tmp_path / "pats").write_bytes(b"".join(s + b"\n" for s in c.strings[:3]))
    for name, extra in (("set", ["--set"]), ("text", [])):
        for index in ("32", "64"):
            for rate in ("32", "5000"):
                out = tmp_path / ("out_%s_%s_%s" % (name, index, rate))
                r = subprocess.run([cli, "-f", str(tmp_path / name), "-q", str(tmp_path / "pats"), "--index", index, "--text-rate", rate,
                                    "--restore", str(out)] + extra, capture_output=True)
                assert r.returncode == 0, r.stderr
                assert out.read_bytes() == (tmp_path / name).read_bytes(), (name, index, rate)
                assert b"Restore time: " in r.stderr
    (tmp_path / "m3").write_bytes(b"mississippi\nmissouri\nmiss\n")
    (tmp_path / "p3").write_bytes(b"ss\nouri\nx\n")
    plain = subprocess.run([cli, "-f", str(tmp_path / "m3"), "-q", str(tmp_path / "p3"), "--set", "--occ", "-s", "3"], capture_output=True, text=True)
    r = subprocess.run([cli, "-f", str(tmp_path / "m3"), "-q", str(tmp_path / "p3"), "--set", "--occ", "-s", "3", "--text-rate", "4", "--context", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0 and plain.returncode == 0, r.stderr
    assert plain.stdout == "18 22 2:2 0:5 0:2 1:2\n10 11 1:4\n0 0\n"
    assert r.stdout == ("18 22 2:2 0:5 0:2 1:2\n\t2:2\tmiss\n\t0:5\tsissip\n\t0:2\tmissis\n\t1:2\tmissou\n"
                        "10 11 1:4\n\t1:4\tssouri\n0 0\n")
    bytes_of = lambda err: int(err.split("Index bytes: ")[1].split()[0])  # noqa: E731
    assert bytes_of(r.stderr) == bytes_of(plain.stderr) + 4 * (23 // 4 + 3)
