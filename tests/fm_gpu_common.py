"""What tests/test_gpu_fm*.py share: a text or string set with the oracle's SA and the model's BWT and first bitmap in HBM, calls of
psacx_fm_index_dev_* / psacx_fm_count_dev_* / psacx_fm_occurrences_dev_* whose outputs are pre-filled and have room behind the last
entry that must stay as it was, the expected intervals by bisection on the bytes, and the cases, computed once."""
import numpy as np

import fm_model as F
import locate_gsa_model as G
import repeats_model as M
from repeats_gpu_common import BIG, Case  # noqa: F401
from rmq_gpu_common import PAD, SENTINEL

FILL64 = 0x6B6B6B6B6B6B6B6B
SIZES = [1, 2, 63, 64, 65, 4097]
SIGMAS = [1, 2, 4, 7, 8]                               # 7 + STOP fills three bits, 8 needs a fourth level; 256 (nine bits) at 4097 only
SAMPLES = [1, 2, 3, 32]                                # and one above n

_cases = {}


def fm_case(kind, n, sigma, seed=1):
    """kind "text": one string; "set": about n / 8 strings (at least 2 where n allows), some of them equal, some of one byte"""
    key = (kind, n, sigma, seed)
    if key not in _cases:
        if kind == "text":
            c = Case(F.random_set(n, 1, seed + n + sigma, sigma), True)
            c.off = np.array([0, n], np.int64)
            c.single = True
        else:
            m = max(1, min(n, max(2, n // 8)))
            s = F.random_set(n, m, seed + 2 * n + sigma, sigma)
            if m >= 4:                                  # two pairs of equal strings of the lengths they had
                s[1] = (s[0] * (len(s[1]) // len(s[0]) + 1))[:len(s[1])]
                s[3] = s[2][:len(s[3])] + s[3][len(s[2]):]
            c = Case(s, False)
            c.single = False
        c.m = int(c.off.size - 1)
        c.end = np.repeat(c.off[1:], np.diff(c.off))
        _cases[key] = c
    return _cases[key]


def named_case(name):
    if name not in _cases:
        strings = F.NAMED[name] if name in F.NAMED else {"every_end": [b"a", b"b", b"c", b"abc", b"cab", b"bca", b"c", b"abc"]}[name]
        c = Case(strings, False)
        c.single = False
        c.m = int(c.off.size - 1)
        c.end = np.repeat(c.off[1:], np.diff(c.off))
        _cases[name] = c
    return _cases[name]


def interval_of(c, P):
    """[lb, ub) of the suffixes, cut at their string's end, that start with P, by two bisections on the bytes; (0, 0) where there are none"""
    P = bytes(P)
    if not P:
        return 0, c.n

    def head(r):
        p = int(c.SA[r])
        return c.text[p:min(int(c.end[p]), p + len(P))].tobytes()
    lo, hi = 0, c.n
    while lo < hi:
        mid = (lo + hi) // 2
        if head(mid) < P:
            lo = mid + 1
        else:
            hi = mid
    lb, hi = lo, c.n
    while lo < hi:
        mid = (lo + hi) // 2
        if head(mid) <= P:
            lo = mid + 1
        else:
            hi = mid
    return (lb, lo) if lo > lb else (0, 0)


def patterns_of(c, seed=3, count=40):
    """patterns that occur, that occur in the flat text only across a string boundary, random ones, whole strings, the empty one, and
    ones with a byte the text does not hold (where there is one)"""
    rng = np.random.RandomState(seed)
    t = c.text
    pats = [b""]
    for _ in range(count):
        a = int(rng.randint(0, c.n))
        pats.append(t[a:a + 1 + int(rng.randint(0, 8))].tobytes())
    for s in range(1, c.m):                             # across a boundary
        b = int(c.off[s])
        pats.append(t[max(0, b - 2):b + 2].tobytes())
        if len(pats) > 2 * count:
            break
    alphabet = sorted(set(t.tolist()))
    for _ in range(count // 2):
        pats.append(bytes(alphabet[int(x)] for x in rng.randint(0, len(alphabet), 1 + int(rng.randint(0, 12)))))
    pats += [bytes(s) for s in c.strings[:4] if len(s) <= 200]
    absent = [b for b in range(256) if b not in set(alphabet)]
    if absent:
        pats += [bytes([absent[0]]), t[:2].tobytes() + bytes([absent[-1]]), bytes([absent[0]]) + t[:2].tobytes()]
    return pats


def expected(c, pats):
    key = ("fm", tuple(pats))
    if key not in c._results:
        iv = [interval_of(c, P) for P in pats]
        c._results[key] = np.array([x[0] for x in iv], np.int64), np.array([x[1] for x in iv], np.int64)
    return c._results[key]


class FmDev(object):
    """BWT, first bitmap, SA and offsets of a case in HBM, and the index once build() has run (or put_blob() has put other words there)"""

    def __init__(self, dev, case):
        self.dev, self.case, self.n, self.m = dev, case, case.n, (0 if case.single else case.m)
        self.bwt, self.first = np.ascontiguousarray(case.bwt), case.first_words()
        self.sa = np.ascontiguousarray(case.SA.astype(dev.dt))
        self.d_bwt, self.d_first, self.d_sa = dev.put(self.bwt), dev.put(self.first), dev.put(self.sa)
        self.off = np.ascontiguousarray(case.off, dtype=np.uint64)
        self.d_off = None if case.single else dev.put(self.off)
        self.d_fm = self.info = None

    def size(self, sample):
        import psac_amd
        return psac_amd.fm_index_device(self.dev.ctx, self.n, self.d_bwt, self.d_first, self.d_sa if sample else None, sample, None, self.dev.bits)

    def build(self, sample):
        """the blob as the device left it, as uint64 words; the words behind it keep their fill"""
        import psac_amd
        dev = self.dev
        q = self.size(sample)
        words = int(q.words)
        self.d_fm = dev.put(np.full(words + PAD, FILL64, np.uint64))
        self.info = psac_amd.fm_index_device(dev.ctx, self.n, self.d_bwt, self.d_first, self.d_sa if sample else None, sample, self.d_fm, dev.bits)
        assert bytes(self.info) == bytes(q), "the size query and the build fill the same descriptor"
        raw = dev.get(self.d_fm, words + PAD, np.uint64)
        assert np.all(raw[words:] == FILL64)
        self.blob = raw[:words]
        return self.blob

    def put_blob(self, words, info):
        self.d_fm, self.info, self.blob = self.dev.put(np.ascontiguousarray(words, dtype=np.uint64)), info, np.asarray(words)

    def layout(self):
        i = self.info
        return F.layout(int(i.n), int(i.bits), int(i.sample), int(i.marks), self.dev.bits // 8)

    def count(self, pats):
        """(lb, ub) as int64"""
        import psac_amd
        dev = self.dev
        pat, off = psac_amd.pattern_buffer(pats)
        q = int(off.size - 1)
        d_pat, d_poff = dev.put(np.concatenate((pat, np.zeros(1, np.uint8)))), dev.put(off)
        init = np.full(q + PAD, SENTINEL, dev.dt)
        d_lb, d_ub = dev.put(init), dev.put(init)
        psac_amd.fm_count_device(dev.ctx, self.d_fm, self.info, d_pat, d_poff, q, d_lb, d_ub, dev.bits)
        lb, ub = dev.get(d_lb, q + PAD), dev.get(d_ub, q + PAD)
        assert np.all(lb[q:] == SENTINEL) and np.all(ub[q:] == SENTINEL)
        assert np.array_equal(dev.get(d_pat, pat.size, np.uint8), pat) and np.array_equal(dev.get(d_poff, q + 1, np.uint64), off)
        return lb[:q].astype(np.int64), ub[:q].astype(np.int64)

    def occurrences(self, lb, ub, limit=0, cap=None, query=False, sid=True):
        """(total, start, pos, sid); pos and sid have one entry more than cap (the expected total by default), pre-filled"""
        import psac_amd
        dev = self.dev
        lo, hi = np.asarray(lb).astype(dev.dt), np.asarray(ub).astype(dev.dt)
        q = int(lo.size)
        want_total = int(G.occurrences(self.sa, self.n, lo, hi, limit)[0][-1])
        cap = want_total if cap is None else cap
        room = max(cap, want_total) + 1
        d_lb, d_ub = dev.put(lo), dev.put(hi)
        d_start = dev.put(np.full(q + 1, FILL64, np.uint64))
        d_pos, d_sid = dev.put(np.full(room, SENTINEL, dev.dt)), dev.put(np.full(room, SENTINEL, dev.dt))
        with_sid = sid and self.d_off is not None
        try:
            total = psac_amd.fm_occurrences_device(dev.ctx, self.d_fm, self.info, self.d_off, self.m, d_lb, d_ub, q, limit, d_start,
                                                   None if query else d_pos, d_sid if with_sid and not query else None, cap, dev.bits)
        finally:
            self.start = dev.get(d_start, q + 1, np.uint64)
            self.pos, self.sid = dev.get(d_pos, room), dev.get(d_sid, room)
            assert np.array_equal(dev.get(d_lb, q), lo) and np.array_equal(dev.get(d_ub, q), hi)
        return total, self.start, self.pos, self.sid

    def check_occurrences(self, lb, ub, limit=0):
        """the lists equal SA[lb .. ub) in order (tests/locate_gsa_model.py), and nothing is written behind the total"""
        lo, hi = np.asarray(lb).astype(self.dev.dt), np.asarray(ub).astype(self.dev.dt)
        want = G.occurrences(self.sa, self.n, lo, hi, limit)
        total, start, pos, sid = self.occurrences(lb, ub, limit)
        assert total == int(want[0][-1]) and np.array_equal(start, want[0])
        assert np.array_equal(pos[:total].astype(np.uint64), want[1]) and np.all(pos[total:] == SENTINEL)
        if self.d_off is not None:
            assert np.array_equal(sid[:total].astype(np.uint64), G.string_ids(self.off, want[1], self.n)) and np.all(sid[total:] == SENTINEL)
        return total

    def unchanged(self):
        dev = self.dev
        ok = (np.array_equal(dev.get(self.d_bwt, self.n, np.uint8), self.bwt) and np.array_equal(dev.get(self.d_first, self.first.size, np.uint32), self.first)
              and np.array_equal(dev.get(self.d_sa, self.n), self.sa))
        if self.d_fm is not None:
            ok = ok and np.array_equal(dev.get(self.d_fm, self.blob.size, np.uint64), self.blob)
        return bool(ok)


def pipeline_of(c, sample):
    key = ("pipe", sample)
    if key not in c._results:
        c._results[key] = F.Pipeline(c.strings, c.SA, sample)
    return c._results[key]
