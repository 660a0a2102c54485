"""Host model of the FM-index calls (include/psacx.h: "FM-index"), for tests/test_fm_model_cpu.py and the test_gpu_fm*.py files.

The answers are stated twice:
  by_bytes(strings, SA, P)        the ranks whose suffix, cut at its string's end, starts with P, and the positions from SA; (0, 0) where
                                  there are none.
  Pipeline(strings, SA, sample)   the definitions of the header one after another: code, w with STOP, cnt, C, E, a naive rank_c, LF,
                                  the first-step rule of the backward search, the marks, val and the walk.
and the blob once: blob_of(pipeline, itemsize) lays the index out word for word as the header describes it, and blob_search /
blob_walk read ANY array of words by the rules of the kernels, clamps included, so that a garbage blob has a defined answer too.
Strings are bytes; a text is a set of one string."""
import json
import os

import numpy as np

import repeats_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fm_named.json")
TAB_Z, TAB_C, TAB_D, TAB_WORDS, SYMS = 0, 16, 16 + 264, 16 + 2 * 264, 264
MASK = (1 << 64) - 1

NAMED = {"mississippi": [b"mississippi"],
         "miss3": [b"mississippi", b"missouri", b"miss"],
         "abab": [b"abab", b"ab"],
         "aa4": [b"aa", b"aa", b"a", b"aa"]}
PATTERNS = {"mississippi": [b"iss", b"ippi", b"i", b"s", b"ssi", b"mississippi", b"pi", b"x", b"issx", b"", b"im", b"ississippi"],
            "miss3": [b"miss", b"iss", b"i", b"ss", b"missouri", b"im", b"ssm", b"ri", b"", b"s", b"z", b"ouri"],
            "abab": [b"ab", b"abab", b"ba", b"b", b"a", b"bab", b"baa", b"aba", b""],
            "aa4": [b"a", b"aa", b"aaa", b"", b"b"]}


def random_set(n, m, seed, sigma):
    """m strings with n bytes in all over sigma byte values (spread over 0 .. 255 for sigma < 256; every value is used where n allows and
    every string has at least one byte)"""
    rng = np.random.RandomState(seed)
    letters = np.arange(256, dtype=np.uint8) if sigma == 256 else (np.arange(sigma) * (255 // max(1, sigma)) + 1).astype(np.uint8)
    t = letters[rng.randint(0, sigma, n)]
    t[:min(n, sigma)] = letters[:min(n, sigma)]
    rng.shuffle(t)
    cuts = np.sort(rng.choice(np.arange(1, n), m - 1, replace=False)) if m > 1 else np.zeros(0, np.int64)
    off = np.concatenate(([0], cuts, [n])).astype(np.int64)
    return [t[off[s]:off[s + 1]].tobytes() for s in range(m)]


# --------------------------------------------------------------------------------------------------------------- by bytes
def by_bytes(strings, SA, P):
    """(lb, ub, positions in rank order); lb = ub = 0 where P does not occur.  The empty pattern gives [0, n)."""
    t, off = M.flatten(strings)
    end = np.zeros(t.size + 1, np.int64)
    for s in range(off.size - 1):
        end[off[s]:off[s + 1]] = off[s + 1]
    sa = np.asarray(SA).astype(np.int64).tolist()
    P = bytes(P)
    hits = [r for r, p in enumerate(sa) if p + len(P) <= end[p] and t[p:p + len(P)].tobytes() == P]
    if not hits:
        return 0, 0, []
    assert hits == list(range(hits[0], hits[-1] + 1)), "the ranks of a pattern are one interval"
    return hits[0], hits[-1] + 1, [sa[r] for r in hits]


# --------------------------------------------------------------------------------------------------------------- the pipeline
def bits_of(sigma):
    b = 1
    while (1 << b) < sigma + 1:
        b += 1
    return b


class Pipeline(object):
    def __init__(self, strings, SA, sample=0, use_E=True, lf_first_step=False):
        t, off = M.flatten(strings)
        self.t, self.off, self.n = t, off, int(t.size)
        self.SA = np.asarray(SA).astype(np.int64)
        self.bwt, self.first, _ = M.bwt_of(t, self.SA, off)
        present = sorted(set(t.tolist()))
        self.sigma = len(present)
        self.bits = bits_of(self.sigma)
        self.code = np.zeros(256, np.int64)
        for i, b in enumerate(present):
            self.code[b] = i + 1
        self.w = np.where(self.first, 0, self.code[self.bwt]).astype(np.int64)
        heads = self.code[t[self.SA]] if self.n else np.zeros(0, np.int64)
        self.cnt = np.bincount(heads, minlength=self.sigma + 2).astype(np.int64)
        self.C = np.concatenate(([0], np.cumsum(self.cnt)))[:self.sigma + 2]
        self.E = np.bincount(self.code[self.bwt[self.first]], minlength=self.sigma + 2).astype(np.int64) if self.n else np.zeros(self.sigma + 2, np.int64)
        self.use_E, self.lf_first_step = use_E, lf_first_step       # (the two mistakes of the header, kept to show what they cost)
        self.sample = int(sample)
        if self.sample:
            self.marked = self.first | (self.SA % self.sample == 0)
            self.val = self.SA[self.marked]
        else:
            self.marked, self.val = np.zeros(self.n, bool), np.zeros(0, np.int64)

    def rank_c(self, c, r):
        return int(np.count_nonzero(self.w[:r] == c))

    def lf_bound(self, c, r):
        return int(self.C[c]) + (int(self.E[c]) if self.use_E else 0) + self.rank_c(c, r)

    def lf(self, r):
        c = int(self.w[r])
        assert c != 0
        return self.lf_bound(c, r)

    def search(self, P):
        lb, ub = 0, self.n
        P = bytes(P)
        for i in range(len(P) - 1, -1, -1):
            c = int(self.code[P[i]])
            if c == 0:
                return 0, 0
            if i == len(P) - 1 and not self.lf_first_step:
                lb, ub = int(self.C[c]), int(self.C[c]) + int(self.cnt[c])
            else:
                lb, ub = self.lf_bound(c, lb), self.lf_bound(c, ub)
            if lb >= ub:
                return 0, 0
        return lb, ub

    def walk(self, r):
        """(SA[r], steps) through the marks"""
        steps = 0
        while not self.marked[r]:
            r = self.lf(r)
            steps += 1
            assert steps < self.sample, "fewer than `sample` steps reach a mark"
        return int(self.val[int(np.count_nonzero(self.marked[:r]))]) + steps, steps

    def locate(self, P, limit=0):
        lb, ub = self.search(P)
        c = ub - lb if not limit else min(ub - lb, limit)
        return [self.walk(r)[0] for r in range(lb, lb + c)]


# --------------------------------------------------------------------------------------------------------------- the blob
def layout(n, bits, sample, marks, itemsize):
    cells = (n >> 6) + 1
    tab = 2 * cells * bits
    marks_at = tab + TAB_WORDS
    val_at = marks_at + (2 * cells if sample else 0)
    return {"n": n, "bits": bits, "sample": sample, "marks": marks, "itemsize": itemsize, "cells": cells, "tab": tab, "marks_at": marks_at,
            "val_at": val_at, "words": val_at + (marks * itemsize + 7) // 8}


def size_bound_bytes(n, bits, sample, marks, itemsize):
    """the bound the header states"""
    cells = (n >> 6) + 1
    return 16 * bits * cells + (16 * cells if sample else 0) + itemsize * marks + 16384


def _cells_of(bitvec, n):
    """the cells of a bit vector of n bits as words {ones in front, 64 bits}"""
    cells = (n >> 6) + 1
    out = np.zeros(2 * cells, np.uint64)
    ones = 0
    for x in range(cells):
        word = 0
        for k, b in enumerate(bitvec[64 * x:64 * x + 64]):
            if b:
                word |= 1 << k
        out[2 * x], out[2 * x + 1] = ones, word
        ones += bin(word).count("1")
    return out


def blob_of(p, itemsize):
    """(words as uint64, layout) of a Pipeline, from the description of the header"""
    Y = layout(p.n, p.bits, p.sample, int(p.val.size), itemsize)
    blob = np.zeros(Y["words"], np.uint64)
    order = p.w.tolist()
    for l in range(p.bits):
        shift = p.bits - 1 - l
        bitvec = [(c >> shift) & 1 for c in order]
        blob[2 * Y["cells"] * l:2 * Y["cells"] * (l + 1)] = _cells_of(bitvec, p.n)
        blob[Y["tab"] + TAB_Z + l] = bitvec.count(0)
        order = [c for c, b in zip(order, bitvec) if not b] + [c for c, b in zip(order, bitvec) if b]
    for c in range(p.sigma + 2):
        blob[Y["tab"] + TAB_C + c] = int(p.C[c])
    for c in range(1, p.sigma + 1):
        start = order.index(c) if c in order else sum(1 for x in order if _rev(x, p.bits) < _rev(c, p.bits))
        blob[Y["tab"] + TAB_D + c] = (int(p.C[c]) + int(p.E[c]) - start) & MASK
    if p.sample:
        blob[Y["marks_at"]:Y["val_at"]] = _cells_of(p.marked.tolist(), p.n)
        val = np.zeros((Y["words"] - Y["val_at"]) * 8 // itemsize, np.uint32 if itemsize == 4 else np.uint64)
        val[:p.val.size] = p.val
        blob[Y["val_at"]:] = val.view(np.uint64)
    return blob, Y


def _rev(c, bits):
    return int(format(c, "0%db" % bits)[::-1], 2)


def _rank1(blob, at, p):
    ones, word = int(blob[at + 2 * (p >> 6)]), int(blob[at + 2 * (p >> 6) + 1])
    return (ones + bin(word & ((1 << (p & 63)) - 1)).count("1")) & MASK


def _bit(blob, at, p):
    return (int(blob[at + 2 * (p >> 6) + 1]) >> (p & 63)) & 1


def blob_search(blob, Y, code, sigma, P):
    """the backward search over any words, by the rules of the kernel: positions clamped to n, a miss pinned to (0, 0)"""
    n, bits, tab = Y["n"], Y["bits"], Y["tab"]
    P = bytes(P)
    lb, ub = 0, n
    for i in range(len(P) - 1, -1, -1):
        if lb >= ub:
            break
        c = int(code[P[i]])
        if c == 0:
            return 0, 0
        if i == len(P) - 1:
            lb, ub = int(blob[tab + TAB_C + c]), int(blob[tab + TAB_C + c + 1])
        else:
            for l in range(bits):
                at = 2 * Y["cells"] * l
                ra, rb = _rank1(blob, at, lb), _rank1(blob, at, ub)
                if (c >> (bits - 1 - l)) & 1:
                    Z = int(blob[tab + TAB_Z + l])
                    lb, ub = (Z + ra) & MASK, (Z + rb) & MASK
                else:
                    lb, ub = (lb - ra) & MASK, (ub - rb) & MASK
                lb, ub = min(lb, n), min(ub, n)
            D = int(blob[tab + TAB_D + c])
            lb, ub = (lb + D) & MASK, (ub + D) & MASK
        lb, ub = min(lb, n), min(ub, n)
    if lb >= ub and len(P):
        return 0, 0
    return lb, ub


def blob_walk(blob, Y, sigma, r):
    """the position of rank r < n over any words, by the rules of the kernel; all ones of the index type where no mark comes up"""
    n, bits, tab, itemsize = Y["n"], Y["bits"], Y["tab"], Y["itemsize"]
    ones = (1 << (8 * itemsize)) - 1
    val = blob[Y["val_at"]:].view(np.uint32 if itemsize == 4 else np.uint64)
    steps = 0
    while steps < min(Y["sample"], n) and r < n:
        if _bit(blob, Y["marks_at"], r):
            at = _rank1(blob, Y["marks_at"], r)
            return (int(val[at]) + steps) & ones if at < Y["marks"] else ones
        c, p = 0, r
        for l in range(bits):
            at = 2 * Y["cells"] * l
            rk, bit = _rank1(blob, at, p), _bit(blob, at, p)
            c = (c << 1) | bit
            p = (int(blob[tab + TAB_Z + l]) + rk) & MASK if bit else (p - rk) & MASK
            p = min(p, n)
        if c == 0 or c > sigma:
            return ones
        r = (p + int(blob[tab + TAB_D + c])) & MASK
        steps += 1
    return ones


# --------------------------------------------------------------------------------------------------------------- golden file
def named_results(name, sample=2):
    strings = NAMED[name]
    t, off, SA, LCP = M.arrays_by_definition(strings)
    rows = []
    for P in PATTERNS[name]:
        lb, ub, pos = by_bytes(strings, SA, P)
        rows.append({"pattern": list(P), "lb": lb, "ub": ub, "pos": pos})
    p = Pipeline(strings, SA, sample)
    return {"strings": [list(s) for s in strings], "SA": SA.tolist(), "w": p.w.tolist(), "C": p.C.tolist(), "E": p.E.tolist(), "sample": sample,
            "marked": [int(x) for x in p.marked], "val": p.val.tolist(), "patterns": rows}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":                             # writes tests/golden/fm_named.json from the model
    with open(GOLDEN, "w") as f:
        json.dump({name: named_results(name) for name in sorted(NAMED)}, f, separators=(",", ":"))
        f.write("\n")
