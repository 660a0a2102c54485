"""psacx_doc_index_dev_*, psacx_doc_count_dev_* and psacx_doc_list_dev_* against the host model (tests/docs_model.py), both index widths:
the index word for word, the counts over every LCP-interval, the lists over those and arbitrary intervals, the refusals, and what the
header promises whatever the index holds.  Outputs are pre-filled with a sentinel and have PAD entries of room (docs_gpu_common)."""
import numpy as np
import pytest

import docs_model as D
from docs_gpu_common import BIG, SETS, SIZES, DocIndex, check_index, check_queries, doc_case, lcp_intervals
from rmq_gpu_common import Dev, PAD, SENTINEL, first_bad

pytestmark = pytest.mark.gpu

NAMES = SETS + ["one", "uneven"] + ["r%d" % n for n in SIZES]


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", NAMES)
def test_index_counts_and_lists(ctx, name, bits):
    dev = Dev(ctx, bits)
    try:
        d = DocIndex(dev, doc_case(name))
        check_index(d, name)
        check_queries(d, name)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_big(ctx, bits):
    # the third level of the range-minimum index, more than one block of the scans
    dev = Dev(ctx, bits)
    try:
        d = DocIndex(dev, doc_case("r%d" % BIG))
        check_index(d, "big")
        lb, ub = lcp_intervals(d.case)                 # counts over every LCP-interval
        got = d.count(lb, ub)
        assert first_bad(got, D.count_by_dup(d.case.dup, lb, ub, d.n)) is None
        check_queries(d, "big", limit=20000)
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_golden_named_sets(ctx, bits):
    import psac_amd
    dt = np.uint32 if bits == 32 else np.uint64
    for name, gold in D.golden().items():
        sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
        sa.construct_ss(D.NAMED[name])
        rows = gold["patterns"]
        lb, ub = np.array([r["lb"] for r in rows], dt), np.array([r["ub"] for r in rows], dt)
        loc = psac_amd.locate(sa._text, sa.local_SA, [bytes(r["pattern"]) for r in rows], offsets=sa.string_offsets, ctx=ctx)
        occur = lb < ub
        assert np.array_equal(loc[0][occur], lb[occur]) and np.array_equal(loc[1][occur], ub[occur]) and np.all(loc[0][~occur] == loc[1][~occur])
        assert sa.doc_count(loc[0], loc[1]).tolist() == [r["docs"] for r in rows], name
        start, sid, pos = sa.doc_list(loc[0], loc[1])
        assert np.diff(start.astype(np.int64)).tolist() == [r["docs"] for r in rows]
        assert sid.tolist() == sum((r["sid"] for r in rows), []) and pos.tolist() == sum((r["pos"] for r in rows), []), name


@pytest.mark.parametrize("bits", [32, 64])
def test_common_repeats(ctx, bits):
    import psac_amd
    strings = [b"xxbananayy", b"bandana", b"zbanan", b"qq"]
    sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
    sa.construct_ss(strings)
    lb, ub, ln, docs = sa.common_repeats(3)
    words = {sa._text[int(sa.local_SA[a]):int(sa.local_SA[a]) + int(k)].tobytes(): int(x) for a, k, x in zip(lb, ln, docs)}
    for w, x in words.items():
        assert x == len(D.docs_by_bytes(strings, w)) >= 3, (w, x)
    assert int(ln.max()) == 3 and {w for w in words if len(w) == 3} == {b"ban", b"ana"}       # the longest substrings common to three strings
    assert b"an" in words and b"a" in words and b"banan" not in words
    lb2, _, _, docs2 = sa.common_repeats(2, max_docs=2)
    assert lb2.size and np.all(docs2 == 2)


def test_cpp_mirror_docs(tmp_path):
    import subprocess
    from test_docs_build_cpu import build_cpp_program
    r = subprocess.run([build_cpp_program(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0 and "docs header tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("index", ["32", "64", "auto"])
def test_command_lines(tmp_path, index):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    locate, repeats = os.path.join(root, "psac_amd", "bin", "locate"), os.path.join(root, "psac_amd", "bin", "repeats")
    (tmp_path / "set").write_bytes(b"mississippi\nmissouri\nmiss\n")
    (tmp_path / "pats").write_bytes(b"miss\nss\nssi\nx\n")
    base = [locate, "-f", str(tmp_path / "set"), "-q", str(tmp_path / "pats"), "--set", "--index", index]
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout.splitlines()[:3] == ["7 10", "18 22", "19 21"], plain.stdout + plain.stderr
    gone = plain.stdout.splitlines()[3]
    r = subprocess.run(base + ["--docs"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == ["7 10 3", "18 22 3", "19 21 1", gone + " 0"] and "Docs time:" in r.stderr, r.stdout + r.stderr
    r = subprocess.run(base + ["--doc-list"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == ["7 10 2:0 0:0 1:0", "18 22 2:2 0:5 1:2", "19 21 0:5", gone], r.stdout + r.stderr
    r = subprocess.run(base + ["--docs", "--doc-list", "1", "-k", "2"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == ["7 10 3 2:0", "18 22 3 2:2", "19 21 1 0:5", gone + " 0"], r.stdout + r.stderr
    base = [repeats, "-f", str(tmp_path / "set"), "--set", "--index", index, "--kind", "right"]
    r = subprocess.run(base + ["--min-docs", "3", "--list"], capture_output=True, text=True)
    assert r.returncode == 0 and "Docs time:" in r.stderr, r.stderr
    assert r.stdout == "z: 5\n0 7 1 1 3\n3 7 3 1 3\n7 10 4 0 3\n14 22 1 2 3\n18 22 2 2 3\nlongest: 7 10 4 0 3\n", r.stdout
    r = subprocess.run(base + ["--min-docs", "3"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: 5\nlongest: 7 10 4 0 3\n", r.stdout + r.stderr
    r = subprocess.run(base + ["--min-docs", "1", "--max-docs", "1", "--list", "2"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: 4\n4 6 4 1 1\n11 13 1 8 1\nlongest: 4 6 4 1 1\n", r.stdout + r.stderr
    r = subprocess.run(base + ["--min-docs", "4"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "z: 0\nlongest: none\n", r.stdout + r.stderr


@pytest.mark.parametrize("bits", [32, 64])
def test_refusals_and_size_queries(ctx, bits):
    import psac_amd
    dev = Dev(ctx, bits)
    try:
        d = DocIndex(dev, doc_case("r4097"))
        d.build()
        n = d.n
        lb, ub = D.random_intervals(n, 300, 3)
        model = D.list_by_prev(d.case.prev, d.case.SA, d.case.off, lb, ub, n)
        z, cand = int(model[0][-1]), int((ub - lb).sum())
        assert z > 1 and cand > 2048
        # cap one short: the code, start and total valid, lists untouched
        start, sid, pos, total = d.lists(lb, ub, room=z, cap=z - 1)
        assert d.error == -2 and total == z and first_bad(start[:lb.size + 1], model[0]) is None
        assert np.all(sid == SENTINEL) and np.all(pos == SENTINEL)
        # max_cand: refused below the number of candidates, before anything is written; accepted at it
        start, sid, pos, total = d.lists(lb, ub, room=z, max_cand=cand - 1)
        assert d.error == -2 and total == 0 and np.all(sid == SENTINEL) and np.all(pos == SENTINEL) and np.all(start == start[0])
        start, sid, pos, total = d.lists(lb, ub, room=z, max_cand=cand)
        assert d.error == 0 and total == z and first_bad(sid[:z], model[2]) is None
        # d_pos == NULL on its own; d_pos without d_sid is an error
        start, sid, pos, total = d.lists(lb, ub, room=z, want_pos=False)
        assert d.error == 0 and total == z and first_bad(sid[:z], model[2]) is None and np.all(sid[z:] == SENTINEL)
        d_start = dev.room(8 * (lb.size + 1))
        d_lb, d_ub = dev.put(lb.astype(dev.dt)), dev.put(ub.astype(dev.dt))
        with pytest.raises(psac_amd.PsacxError) as e:
            psac_amd.doc_list_device(ctx, d.d_sa, n, d.d_off, d.m, d.d_prev, d_lb, d_ub, lb.size, 0, d_start, None, dev.room(8 * z), z, bits)
        assert e.value.code == -1
        # the index: both outputs NULL, m == 0, m > n; n == 0 and q == 0 are fine
        for args in ((n, d.m, None, None), (n, 0, d.d_prev, d.d_dup), (n, n + 1, d.d_prev, d.d_dup)):
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.doc_index_device(ctx, args[0], d.d_off, args[1], d.d_sa, d.lcp.d_v, d.lcp.d_index, args[2], args[3], bits)
            assert e.value.code == -1
        psac_amd.doc_index_device(ctx, 0, None, 1, None, None, None, d.d_prev, d.d_dup, bits)
        psac_amd.doc_count_device(ctx, n, d.d_dup, None, None, 0, None, bits)
        assert psac_amd.doc_list_device(ctx, d.d_sa, n, d.d_off, d.m, d.d_prev, None, None, 0, 0, None, None, None, 0, bits) == 0
        if bits == 32:
            with pytest.raises(psac_amd.PsacxError) as e:
                psac_amd.doc_index_device(ctx, 1 << 32, d.d_off, d.m, d.d_sa, d.lcp.d_v, d.lcp.d_index, d.d_prev, d.d_dup, bits)
            assert e.value.code == -2
        check_index(d, "after the refusals")
        assert d.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_totality(ctx, bits):
    dev = Dev(ctx, bits)
    try:
        c = doc_case("r4097")
        n = c.n
        rng = np.random.RandomState(17)
        top = int(np.iinfo(dev.dt).max)
        words = lambda k: rng.randint(0, 1 << (32 if bits == 32 else 62), k, dtype=np.int64)  # noqa: E731  (int64 holds them: the model computes as the device)
        lb, ub = D.random_intervals(n, 500, 4)
        # a dup that is not monotone: 1 <= docs <= ub - lb, 0 for the malformed, and exactly the clamped formula
        d = DocIndex(dev, c)
        dup = words(n + 1)
        d.put_index(dup=dup)
        qa, qb = np.concatenate((lb, [5, 0])), np.concatenate((ub, [4, n + 1]))
        got = d.count(qa, qb)
        ok = (qa < qb) & (qb <= n)
        assert np.all(got[~ok] == 0) and np.all((got[ok] >= 1) & (got[ok] <= (qb - qa)[ok]))
        assert np.array_equal(got, D.count_by_dup(dup, qa, qb, n))
        # a prev of random words (some below n, some all ones): only which ranks are listed changes
        prev = words(n)
        prev[rng.randint(0, n, n // 2)] = rng.randint(0, n, n // 2)
        ones = rng.randint(0, n, n // 8)
        prev[ones] = D.NONE
        on_device = prev.astype(dev.dt)
        on_device[ones] = top
        d.put_index(prev=on_device)
        d.run_lists(lb, ub, D.list_by_prev(prev, c.SA, c.off, lb, ub, n), "random prev")
        assert d.unchanged()
        # SA entries >= n: sid = m in the lists; the index stays the model's over that SA
        bad = c.SA.copy()
        at = rng.choice(n, 200, replace=False)
        bad[at] = n + rng.randint(0, 1 << 20, 200)
        bad[at[0]] = top if bits == 32 else (1 << 62)
        d2 = DocIndex(dev, c, SA=bad)
        prev2, dup2 = D.index_of(bad, c.LCP, c.off)
        check_index(d2, "SA beyond n", prev2, dup2)
        model = D.list_by_prev(prev2, bad, c.off, lb, ub, n)
        assert np.any(model[2] == c.m)
        d2.run_lists(lb, ub, model, "SA beyond n")
        assert d2.unchanged()
    finally:
        dev.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_identical_strings_past_the_change_of_form_of_the_sort(ctx, bits):
    # [b"ab"] * (2^20 + 1): n = 2 m > 2^21 records, so the rank-pair sort runs in its three-kernel form, and every atomic of the pairs stage
    # hits h[m].  SA: the ab suffixes in text order, then the b suffixes; LCP 2 among the first, 0 at rank m, 1 behind it.
    dev = Dev(ctx, bits)
    try:
        m = (1 << 20) + 1
        n = 2 * m

        class Closed(object):
            pass

        c = Closed()
        c.n, c.m = n, m
        c.SA = np.concatenate((2 * np.arange(m), 2 * np.arange(m) + 1))
        c.LCP = np.concatenate(([0], np.full(m - 1, 2), [0], np.full(m - 1, 1)))
        c.off = 2 * np.arange(m + 1)
        d = DocIndex(dev, c)
        prev, dup = d.build()
        assert np.all(prev[:m] == D.NONE) and np.array_equal(prev[m:], np.arange(m))
        assert np.all(dup[:m + 1] == 0) and np.all(dup[m + 1:] == m)           # h[m] = m and nothing else
        assert d.count([0, m, 0], [m, n, n]).tolist() == [m, m, m]
        start, sid, pos, total = d.lists([0, m, 0, m - 2], [m, n, n, m + 2])
        assert d.error == 0 and total == 3 * m + 4 and start[:5].tolist() == [0, m, 2 * m, 3 * m, 3 * m + 4]
        assert np.array_equal(sid[:m], np.arange(m)) and np.array_equal(sid[m:2 * m], np.arange(m)) and np.array_equal(sid[2 * m:3 * m], np.arange(m))
        assert sid[3 * m:total].tolist() == [m - 2, m - 1, 0, 1] and pos[3 * m:total].tolist() == [2 * m - 4, 2 * m - 2, 1, 3]
        assert np.array_equal(pos[m:2 * m], 2 * np.arange(m) + 1) and np.all(sid[total:] == SENTINEL) and np.all(pos[total:] == SENTINEL)
        assert d.unchanged()
    finally:
        dev.close()
