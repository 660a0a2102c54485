"""Host model of the text samples and the extraction of the FM-index (include/psacx.h: "FM-index", text samples), for
tests/test_fm_extract_model_cpu.py and the test_gpu_fm_extract*.py files.

The answers are stated twice:
  by_bytes(strings, pos, length)        the slice of the flattened text, clipped at the end of the string that holds pos
  Extractor(strings, SA, rate)          the pipeline: the sample arrays from SA, then segment by segment as the kernel is specified: the
                                        sample at the right end of the block or at the string's end, the head symbol from C, then w and LF
and the words once: blob_extract reads ANY blob and ANY samples by the rules of the kernel, clamps and the zero fill included, so that
garbage has a defined answer too (as blob_search / blob_walk of fm_model.py).  Strings are bytes; a text is a set of one string."""
import json
import os

import numpy as np

import fm_model as F
import repeats_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fm_extract_named.json")
RATES = [1, 2, 3]                                        # of the golden file
EVERY_END = [b"a", b"b", b"c", b"abc", b"cab", b"bca", b"c", b"abc"]


def last_le(a, cnt, o):
    """the largest j in [0, cnt) with a[j] <= o by the bisection of occ_last_le (occurrences.hpp), whatever a holds"""
    lo, hi = 0, cnt
    while hi - lo > 1:
        mid = lo + ((hi - lo) >> 1)
        if int(a[mid]) <= o:
            lo = mid
        else:
            hi = mid
    return lo


# --------------------------------------------------------------------------------------------------------------- by bytes
def clip(off, n, pos, length):
    """(a, clipped length) of one query; off: the m + 1 offsets"""
    if pos >= n:
        return pos, 0
    s = int(np.searchsorted(off, pos, side="right")) - 1
    return pos, max(0, min(int(length), int(off[s + 1]) - pos))


def by_bytes(strings, pos, length):
    """(start, bytes): the prefix sums of the clipped lengths and the slices, back to back"""
    t, off = M.flatten(strings)
    parts = []
    for p, l in zip(pos, length):
        a, cl = clip(off, t.size, int(p), int(l))
        parts.append(t[a:a + cl])
    start = np.concatenate(([0], np.cumsum([x.size for x in parts]))).astype(np.uint64)
    return start, (np.concatenate(parts) if parts else np.zeros(0, np.uint8)).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------- the pipeline
def sample_arrays(strings, SA, rate, end_samples=True):
    """ts: the rank of the suffix at (k + 1) * rate - 1 for k < n // rate, then the rank of the suffix at the last byte of every string"""
    t, off = M.flatten(strings)
    n = int(t.size)
    isa = np.zeros(n, np.int64)
    isa[np.asarray(SA).astype(np.int64)] = np.arange(n)
    ts = [int(isa[(k + 1) * rate - 1]) for k in range(n // rate)]
    if end_samples:
        ts += [int(isa[int(off[j + 1]) - 1]) for j in range(off.size - 1)]
    return np.array(ts, np.int64)


class Extractor(object):
    """end_samples=False is the scheme without the samples of the string ends: a segment whose block sample lies in the next string, or
    whose block has none, is entered from there and loses its bytes (zeros), which shows why the end samples are there."""

    def __init__(self, strings, SA, rate, end_samples=True):
        self.p = F.Pipeline(strings, SA, 0)
        self.rate, self.end_samples = int(rate), end_samples
        self.n, self.off = self.p.n, self.p.off
        self.blocks = self.n // self.rate
        self.ts = sample_arrays(strings, SA, rate, end_samples)
        self.decode = np.zeros(self.p.sigma + 1, np.uint8)
        for b in range(256):
            if self.p.code[b]:
                self.decode[self.p.code[b]] = b

    def head(self, x):
        """the symbol c with C[c] <= x < C[c + 1]: the first symbol of the suffix of rank x"""
        c = int(np.searchsorted(self.p.C[:self.p.sigma + 2], x, side="right")) - 1
        assert 1 <= c <= self.p.sigma
        return c

    def segment(self, out, base, a, b, k, s):
        """the bytes of [a, b) inside block k into out[base + (p - a)]"""
        rate, e = self.rate, int(self.off[s + 1])
        lo, hi = max(a, k * rate), min(b, (k + 1) * rate)
        if (k + 1) * rate <= e or not self.end_samples:
            if k >= self.blocks:
                return                                  # (without end samples only: no sample to the right)
            P, x = (k + 1) * rate - 1, int(self.ts[k])
        else:
            P, x = e - 1, int(self.ts[self.blocks + s])
        c = self.head(x)
        for pos in range(P, lo - 1, -1):
            if pos < hi:
                out[base + pos - a] = self.decode[c]
            if pos == lo:
                break
            c = int(self.p.w[x])
            if c == 0:
                return                                  # STOP: entered from another string
            x = self.p.lf(x)

    def extract(self, pos, length):
        cl = [clip(self.off, self.n, int(p), int(l)) for p, l in zip(pos, length)]
        start = np.concatenate(([0], np.cumsum([x[1] for x in cl]))).astype(np.uint64)
        out = np.zeros(int(start[-1]), np.uint8)
        for i, (a, l) in enumerate(cl):
            if l == 0:
                continue
            s = int(np.searchsorted(self.off, a, side="right")) - 1
            for k in range(a // self.rate, (a + l - 1) // self.rate + 1):
                self.segment(out, int(start[i]), a, a + l, k, s)
        return start, out

    def strings(self):
        start, out = self.extract(self.off[:-1], np.diff(self.off))
        return [out[int(start[j]):int(start[j + 1])].tobytes() for j in range(self.off.size - 1)]


# --------------------------------------------------------------------------------------------------------------- any words
def blob_extract(blob, Y, code, sigma, ts, rate, off, pos, length):
    """(start, bytes) over any blob and any samples by the rules of the kernels.  Y: fm_model.layout; code: the 256 codes of the
    descriptor; ts: n // rate + max(m, 1) entries; off: VALID offsets (m + 1 of them) or None for one text."""
    n, bits, tab, cells = Y["n"], Y["bits"], Y["tab"], Y["cells"]
    blocks = n // rate
    rate = min(rate, n + 1)
    m = 1 if off is None else len(off) - 1
    off = [0, n] if off is None else [int(x) for x in off]
    assert len(ts) == blocks + max(m, 1)
    dec = [0] * F.SYMS
    for ch in range(256):
        if code[ch]:
            dec[int(code[ch])] = ch
    C = [int(blob[tab + F.TAB_C + c]) for c in range(sigma + 1)]
    cl = []
    for p, l in zip(pos, length):
        a, l, c = int(p), int(l), 0
        if a < n:
            e = min(off[last_le(off, m, a) + 1], n)
            if e > a:
                c = min(l, e - a)
        cl.append(c)
    start = np.concatenate(([0], np.cumsum(cl))).astype(np.uint64)
    out = np.zeros(int(start[-1]), np.uint8)
    for i, c_len in enumerate(cl):
        if not c_len:
            continue
        a = int(pos[i])
        b, base = a + c_len, int(start[i])
        s = last_le(off, m, a)
        e = min(off[s + 1], n)
        for k in range(a // rate, (b - 1) // rate + 1):
            blo, bhi = k * rate, (k + 1) * rate
            lo, hi = max(a, blo), min(b, bhi)
            inner = bhi <= e
            P = (bhi if inner else e) - 1
            r = min(int(ts[k if inner else blocks + s]), n)
            c = last_le(C, sigma + 1, r) if r < n else 0
            live = c != 0
            p = P
            while True:
                if p < hi:
                    out[base + p - a] = dec[c] if live else 0
                if p == lo:
                    break
                if live:
                    c, x = 0, r
                    for l in range(bits):
                        at = 2 * cells * l
                        rk, bit = F._rank1(blob, at, x), F._bit(blob, at, x)
                        c = (c << 1) | bit
                        x = (int(blob[tab + F.TAB_Z + l]) + rk) & F.MASK if bit else (x - rk) & F.MASK
                        x = min(x, n)
                    live = c != 0 and c <= sigma
                    if live:
                        r = (x + int(blob[tab + F.TAB_D + c])) & F.MASK
                        live = r < n
                p -= 1
    return start, out


# --------------------------------------------------------------------------------------------------------------- golden file
def named(name):
    return F.NAMED[name]


def named_results(name):
    strings = named(name)
    SA = M.arrays_by_definition(strings)[2]
    return {"strings": [list(s) for s in strings], "SA": np.asarray(SA).tolist(),
            "ts": {str(rate): sample_arrays(strings, SA, rate).tolist() for rate in RATES}}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":                             # writes tests/golden/fm_extract_named.json from the model
    with open(GOLDEN, "w") as f:
        json.dump({name: named_results(name) for name in sorted(F.NAMED)}, f, separators=(",", ":"))
        f.write("\n")
