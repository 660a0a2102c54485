"""psacx_overlaps_dev_* against the host model (tests/overlaps_model.py: all pairs by byte comparison, and the walk over the
oracle's arrays, which tests/test_overlaps_model_cpu.py holds to each other), both index widths:

  - the named sets -- abab / babab / ab / abab, the unary set whose chain is as long as its string, one string of one byte, three
    equal bytes, lengths 31 / 32 / 33 / 64 over one letter (bit tests on both sides of a bitmap word, the last at bit n), 300
    copies of one string (a run longer than 256: more than two rounds of the 16-way partition), borders -- each at min_len 1, 2
    and the longest length, with and without PSACX_OVERLAP_WHOLE, and min_len above every length (all slots 0);
  - 512 reads of 64 bytes from 4096 random DNA, and the same with 2 % substitutions, at min_len 16: 2950 non-empty slots / 3139
    pairs, 3462 / 3715 with the whole strings (742 / 786 and 1254 / 1308 once mutated);
  - psacx_occurrences_dev_* over the result with q = n equals the model's (slot, pos, sid) list;
  - arrays that are no index: SA, ISA, LCP, the index and the bitmap corrupted in turn -- the call returns, lb <= ub <= n;
  - refusals leave the outputs as they were;
  - the host-pointer form, psac_amd.overlaps, SuffixArray.overlaps, the C++ mirror and the command line.
Outputs are pre-filled with a sentinel and have PAD entries of room behind entry n, which must come back untouched; the inputs
must come back unchanged.  The text is never uploaded for the device calls."""
import os
import subprocess

import numpy as np
import pytest

import overlaps_model as V
import rmq_model as R
from rmq_gpu_common import Dev, Indexed, PAD, SENTINEL, first_bad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHOLE = 1


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


class OverlapIndex(object):
    """offsets, SA, ISA, LCP, the index of LCP and the bitmap of the string ends in HBM (index / ends: words to use instead of the
    built ones)."""

    def __init__(self, dev, off, SA, ISA, LCP, index=None, ends=None):
        import psac_amd
        self.dev = dev
        self.off = np.ascontiguousarray(off, dtype=np.uint64)
        self.m = int(self.off.size - 1)
        self.sa = np.ascontiguousarray(np.asarray(SA).astype(dev.dt))
        self.isa = np.ascontiguousarray(np.asarray(ISA).astype(dev.dt))
        self.n = int(self.sa.size)
        self.d_off, self.d_sa, self.d_isa = dev.put(self.off), dev.put(self.sa), dev.put(self.isa)
        self.lcp = Indexed(dev, np.asarray(LCP).astype(dev.dt), index)
        words = psac_amd.string_ends_device(dev.ctx, None, self.m, self.n, None)
        assert words == (self.n >> 5) + 1
        if ends is None:
            self.d_ends = dev.room(words * 4)
            psac_amd.string_ends_device(dev.ctx, self.d_off, self.m, self.n, self.d_ends)
            self.ends = dev.get(self.d_ends, words, np.uint32)
        else:
            self.ends = np.ascontiguousarray(ends[:words], dtype=np.uint32)
            assert self.ends.size == words
            self.d_ends = dev.put(self.ends)

    def run(self, min_len, flags=0, d_off=None, n=None):
        """(lb, ub) as int64 of psacx_overlaps_dev_*; self.raw keeps the two arrays with their pads, also after a refusal"""
        import psac_amd
        dev = self.dev
        init = np.full(self.n + PAD, SENTINEL, dev.dt)
        d_lb, d_ub = dev.put(init), dev.put(init)
        try:
            psac_amd.overlaps_device(dev.ctx, self.n if n is None else n, self.d_off if d_off is None else d_off, self.m, self.d_ends, self.d_sa,
                                     self.d_isa, self.lcp.d_v, self.lcp.d_index, min_len, flags, d_lb, d_ub, dev.bits)
        finally:
            self.d_out = d_lb, d_ub
            self.raw = dev.get(d_lb, self.n + PAD), dev.get(d_ub, self.n + PAD)
        assert np.all(self.raw[0][self.n:] == SENTINEL) and np.all(self.raw[1][self.n:] == SENTINEL)
        return self.raw[0][:self.n].astype(np.int64), self.raw[1][:self.n].astype(np.int64)

    def unchanged(self):
        dev = self.dev
        return bool(np.array_equal(dev.get(self.d_off, self.m + 1, np.uint64), self.off) and np.array_equal(dev.get(self.d_sa, self.n), self.sa)
                    and np.array_equal(dev.get(self.d_isa, self.n), self.isa) and self.lcp.unchanged()
                    and np.array_equal(dev.get(self.d_ends, self.ends.size, np.uint32), self.ends))


def agree(d, name, min_len, whole):
    want = V.slots(name, min_len, whole)
    got = d.run(min_len, WHOLE if whole else 0)
    for g, w in zip(got, want):
        bad = first_bad(g, w)
        assert bad is None, (name, min_len, whole, bad)
    return got


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", V.SMALL + ["copies300"])
def test_named_sets_equal_the_model(ctx, name, bits):
    text, off, SA, ISA, LCP = V.set_arrays(name)
    dev = Dev(ctx, bits)
    try:
        d = OverlapIndex(dev, off, SA, ISA, LCP)
        for whole in (False, True):
            for min_len in V.min_lens(name):
                agree(d, name, min_len, whole)
            lb, ub = d.run(max(len(x) for x in V.strings_of(name)) + 1, WHOLE if whole else 0)      # above every length
            assert not lb.any() and not ub.any()
        assert d.unchanged()
    finally:
        dev.close()


def test_the_named_sets_say_something():
    # (on the host) the cases above are not all-zero results, and the 300 copies hold a run longer than 256
    for name in V.SMALL + ["copies300"]:
        lb, ub = V.slots(name, 1, True)
        assert np.count_nonzero(ub > lb) > 0, name
    lb, ub = V.slots("copies300", 1, True)
    assert int((ub - lb).max()) == 300
    text, off, SA, ISA, LCP = V.set_arrays("word_edges")
    assert [int(x) for x in off] == [0, 31, 63, 96, 160]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["reads", "reads_mut"])
def test_reads_equal_the_model_and_expand_to_its_pairs(ctx, name, bits):
    import psac_amd
    text, off, SA, ISA, LCP = V.set_arrays(name)
    n = int(text.size)
    dev = Dev(ctx, bits)
    try:
        d = OverlapIndex(dev, off, SA, ISA, LCP)
        for whole in (False, True):
            want = V.slots(name, 16, whole)
            assert np.count_nonzero(want[1] > want[0]) > 0                                # an all-zero result cannot pass
            agree(d, name, 16, whole)
            # the lists behind the slots: psacx_occurrences_dev_* over the two arrays as they are, q = n
            d_lb, d_ub = d.d_out
            d_start = dev.room((n + 1) * 8)
            total = psac_amd.occurrences_device(ctx, d.d_sa, n, d.d_off, d.m, d_lb, d_ub, n, 0, d_start, None, None, 0, bits)
            pairs = V.pairs_of_slots(off, SA, want[0], want[1])
            assert total == len(pairs) > 0
            d_pos, d_sid = dev.room(total * (bits // 8)), dev.room(total * (bits // 8))
            assert psac_amd.occurrences_device(ctx, d.d_sa, n, d.d_off, d.m, d_lb, d_ub, n, 0, d_start, d_pos, d_sid, total, bits) == total
            start = dev.get(d_start, n + 1, np.uint64).astype(np.int64)
            slot = np.repeat(np.arange(n), np.diff(start))
            got = list(zip(slot.tolist(), dev.get(d_pos, total).astype(np.int64).tolist(), dev.get(d_sid, total).astype(np.int64).tolist()))
            assert got == pairs                                                           # (equal suffixes lie in text order: SA order is sorted)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_arrays_that_are_no_index(ctx, bits):
    name = "reads"
    text, off, SA, ISA, LCP = V.set_arrays(name)
    n = int(text.size)
    rng = np.random.RandomState(17)
    top = int(R.ones(np.uint32 if bits == 32 else np.uint64))
    words = (n >> 5) + 1

    def noise(count, below=1 << 32):
        return rng.randint(0, below, count, dtype=np.int64).astype(np.uint64)
    ones = np.full(n, top, np.uint64)
    ascending = np.arange(n, dtype=np.uint64) + np.uint64(n)                             # no previous smaller value exists
    built = dict(index=None, ends=None)
    cases = [
        (noise(n), ISA, LCP, built), (noise(n, 2 * n), ISA, LCP, built), (ones, ISA, LCP, built),                         # SA
        (SA, noise(n), LCP, built), (SA, noise(n, 2 * n), LCP, built), (SA, ones, LCP, built),                            # ISA
        (SA, ISA, noise(n), built), (SA, ISA, noise(n, 70), built), (SA, ISA, ones, built), (SA, ISA, ascending, built),  # LCP, index of it
        (SA, ISA, LCP, dict(index=noise(n // 16 + 4096), ends=None)),                                                     # index
        (SA, ISA, LCP, dict(index=np.full(n // 16 + 4096, top, np.uint64), ends=None)),
        (SA, ISA, LCP, dict(index=np.zeros(n // 16 + 4096, np.uint64), ends=None)),                                       # every search "finds" at once
        (SA, ISA, noise(n, 70), dict(index=np.zeros(n // 16 + 4096, np.uint64), ends=None)),
        (SA, ISA, LCP, dict(index=None, ends=noise(words).astype(np.uint32))),                                            # bitmap
        (SA, ISA, LCP, dict(index=None, ends=np.full(words, 0xFFFFFFFF, np.uint32))),
        (SA, ISA, LCP, dict(index=None, ends=np.zeros(words, np.uint32))),
        (noise(n, 2 * n), noise(n, 2 * n), noise(n, 70), dict(index=noise(n // 16 + 4096), ends=noise(words).astype(np.uint32))),
    ]
    dev = Dev(ctx, bits)
    try:
        for k, (sa, isa, lcp, kw) in enumerate(cases):
            d = OverlapIndex(dev, off, sa, isa, lcp, **kw)
            for min_len, flags in ((1, 0), (1, WHOLE), (16, WHOLE)):
                lb, ub = d.run(min_len, flags)                                            # returns PSACX_OK
                assert np.all(lb <= ub) and np.all(ub <= n), (k, min_len, flags)
            assert d.unchanged()
            dev.close()
        d = OverlapIndex(dev, off, SA, ISA, LCP)                                          # a correct call afterwards is right
        agree(d, name, 16, True)
    finally:
        dev.close()


def test_refusals(ctx):
    import psac_amd
    text, off, SA, ISA, LCP = V.set_arrays("abab")
    dev = Dev(ctx, 64)
    try:
        d = OverlapIndex(dev, off, SA, ISA, LCP)
        short = off.copy()
        short[-1] -= 1                                                                    # does not end at n
        flat = off.copy()
        flat[2] = flat[1]                                                                 # an empty string
        late = off.copy()
        late[0] = 1                                                                       # does not start at 0
        for kw in (dict(min_len=0), dict(min_len=1, flags=2), dict(min_len=1, flags=WHOLE | 4), dict(min_len=1, d_off=dev.put(short)),
                   dict(min_len=1, d_off=dev.put(flat)), dict(min_len=1, d_off=dev.put(late))):
            with pytest.raises(psac_amd.PsacxError) as e:
                d.run(**kw)
            assert e.value.code == -1, kw
            assert np.all(d.raw[0] == SENTINEL) and np.all(d.raw[1] == SENTINEL), kw
        assert d.unchanged()
        # no strings, or no text: nothing to do
        psac_amd.overlaps_device(ctx, d.n, None, 0, None, None, None, None, None, 1, 0, None, None, 64)
        psac_amd.overlaps_device(ctx, 0, None, 3, None, None, None, None, None, 1, 0, None, None, 64)
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_host_pointer_form_and_python(ctx, bits):
    import psac_amd
    dt = np.uint32 if bits == 32 else np.uint64
    text, off, SA, ISA, LCP = V.set_arrays("reads")
    dev = Dev(ctx, bits)
    try:
        d = OverlapIndex(dev, off, SA, ISA, LCP)
        for whole in (False, True):
            dev_form = d.run(16, WHOLE if whole else 0)
            assert np.count_nonzero(dev_form[1] > dev_form[0]) > 0
            for first in (int(text.size), text):                                          # n as a number, or anything with a length
                lb, ub = psac_amd.overlaps(first, off, SA.astype(dt), ISA.astype(dt), LCP.astype(dt), 16, whole=whole, ctx=ctx)
                assert lb.dtype == dt and ub.dtype == dt
                assert np.array_equal(lb.astype(np.int64), dev_form[0]) and np.array_equal(ub.astype(np.int64), dev_form[1])
    finally:
        dev.close()
    with pytest.raises(psac_amd.PsacxError) as e:
        psac_amd.overlaps(int(text.size), off, SA.astype(dt), ISA.astype(dt), LCP.astype(dt), 0, ctx=ctx)
    assert e.value.code == -1
    # the chain a user runs: construct_ss, then .overlaps, then occurrences
    sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
    sa.construct_ss(V.strings_of("borders"))
    for whole in (False, True):
        lb, ub = sa.overlaps(1, whole=whole)
        want = V.slots("borders", 1, whole)
        assert np.array_equal(lb.astype(np.int64), want[0]) and np.array_equal(ub.astype(np.int64), want[1])
        start, pos, sid = psac_amd.occurrences(sa.local_SA, lb, ub, offsets=sa.string_offsets, ctx=ctx)
        slot = np.repeat(np.arange(sa.n), np.diff(start.astype(np.int64)))
        btext, boff = V.set_arrays("borders")[:2]
        assert list(zip(slot.tolist(), pos.astype(np.int64).tolist(), sid.astype(np.int64).tolist())) == V.pairs_by_bytes(btext, boff, 1, whole)
    with pytest.raises(ValueError):
        psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx).overlaps(1)


def test_cpp_mirror_overlaps(tmp_path):
    from test_overlaps_build_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "overlaps header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64", "auto"])
def test_command_line(tmp_path, index):
    exe = os.path.join(ROOT, "psac_amd", "bin", "overlaps")
    for name in ("abab", "reads"):
        strings = V.strings_of(name)
        text, off, SA, ISA, LCP = V.set_arrays(name)
        (tmp_path / name).write_bytes(b"\n".join(strings) + b"\n")
        for min_len, whole in ((1, False), (2, True)) if name == "abab" else ((16, True),):
            lb, ub = V.slots(name, min_len, whole)
            r = subprocess.run([exe, "-f", str(tmp_path / name), "-l", str(min_len), "--index", index, "--list"] + (["--whole"] if whole else []),
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert r.stdout == V.cli_text(off, V.pairs_of_slots(off, SA, lb, ub))
            assert "Overlaps time:" in r.stderr
            r = subprocess.run([exe, "-f", str(tmp_path / name), "-l", str(min_len), "--index", index] + (["--whole"] if whole else []),
                               capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout == "", r.stderr
            assert "slots: %d pairs: %d" % (np.count_nonzero(ub > lb), int(np.sum(ub - lb))) in r.stderr
