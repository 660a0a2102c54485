"""The bisection steps of the search kernels, pinned: with PSACX_LOCATE_COUNT the counters of psacx_locate_dev_*,
psacx_locate_gsa_dev_*, psacx_match_dev_* and psacx_match_gsa_dev_* (SA entries fetched, text words fetched) equal the pairs
recorded in tests/golden/query_fetches.json, exactly: they are sums of deterministic per-lane counts.  The other query tests compare
the counters with each other only, so a change that moved every kernel's probes alike would pass them; DESIGN.md section 4.5
states that the kernels take the same steps "probe for probe", and this holds them to it.

Both index widths.  Plain texts: mississippi, edge4097, unary, bytes256 and tandem of locate_model over their own pattern lists,
without a table and with the first k of table_ks: locate in both kernel shapes, match plain, over every suffix, and cut to 8 bytes.
String sets: locate and match over the catalogue of locate_gsa_model with its pattern lists.

`python tests/test_gpu_query_fetches.py --record` writes the JSON (on a GPU); it holds the pairs keyed by case and nothing else."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "query_fetches.json")
PLAIN = ("mississippi", "edge4097", "unary", "bytes256", "tandem")


def plain_cases(ctx, name, bits):
    """{case: [SA entries, text words]} of one plain text; PSACX_LOCATE_COUNT is set by the caller"""
    import locate_model as L
    from match_gpu_common import Index
    out = {}
    d = Index(ctx, name, bits)
    try:
        b = d.batch(L.patterns_of(name))
        for table in (None, d.table(L.table_ks(d.text)[0][0])[0]):
            runs = [("locate lane", "lane", lambda: d.locate(b, table)), ("locate group", "group", lambda: d.locate(b, table)),
                    ("match", "lane", lambda: d.match(b, table)), ("match suffixes", "lane", lambda: d.match(b, table, suffixes=True)),
                    ("match max_len 8", "lane", lambda: d.match(b, table, max_len=8))]
            for what, shape, call in runs:
                os.environ["PSACX_LOCATE_SHAPE"] = shape
                call()
                out["u%d %s k=%d %s" % (bits, name, table[1] if table else 0, what)] = [int(x) for x in ctx.stats().locate_fetches]
    finally:
        os.environ.pop("PSACX_LOCATE_SHAPE", None)
        d.close()
    return out


def set_cases(ctx, name, bits):
    """the same of one string set"""
    import locate_gsa_model as G
    import locate_model as L
    from match_gpu_common import Index
    out = {}
    d = Index(ctx, name, bits, set=True)
    try:
        b = d.batch(G.patterns_of(name))
        for table in (None, d.table(L.table_ks(d.text)[0][0])[0]):
            for what, call in (("locate", lambda: d.locate(b, table)), ("match", lambda: d.match(b, table))):
                call()
                out["u%d set %s k=%d %s" % (bits, name, table[1] if table else 0, what)] = [int(x) for x in ctx.stats().locate_fetches]
    finally:
        d.close()
    return out


def set_names():
    import locate_gsa_model as G
    return list(G.GPU)


@pytest.fixture(scope="module")
def ctx():
    import psac_amd
    c = psac_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def check(got, golden):
    for case, pair in got.items():
        print(case, pair, golden.get(case))
    assert all(min(pair) > 0 for pair in got.values())                         # the counting kernels ran
    assert got == {case: golden.get(case) for case in got}


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", PLAIN)
def test_plain_text_fetches_equal_the_recorded(ctx, golden, name, bits, monkeypatch):
    monkeypatch.setenv("PSACX_LOCATE_COUNT", "1")
    got = plain_cases(ctx, name, bits)
    assert len(got) == 10
    check(got, golden)


@pytest.mark.parametrize("bits", [32, 64])
def test_string_set_fetches_equal_the_recorded(ctx, golden, bits, monkeypatch):
    monkeypatch.setenv("PSACX_LOCATE_COUNT", "1")
    got = {}
    for name in set_names():
        got.update(set_cases(ctx, name, bits))
    assert len(got) == 4 * len(set_names())
    check(got, golden)


def test_the_recording_holds_these_cases_only(golden):
    cases = ["u%d %s k=%d %s" % (bits, name, k, what) for bits in (32, 64) for name in PLAIN for k in (0, 1)
             for what in ("locate lane", "locate group", "match", "match suffixes", "match max_len 8")]
    cases += ["u%d set %s k=%d %s" % (bits, name, k, what) for bits in (32, 64) for name in set_names() for k in (0, 1) for what in ("locate", "match")]
    assert sorted(golden) == sorted(cases)
    assert all(isinstance(v, list) and len(v) == 2 and all(isinstance(x, int) for x in v) for v in golden.values())


def record():
    os.environ["PSACX_ENV_KNOBS"] = "1"                                        # (tests/conftest.py does this for the suite)
    os.environ["PSACX_LOCATE_COUNT"] = "1"
    sys.path.insert(0, os.path.dirname(HERE))
    import psac_amd
    ctx = psac_amd.Context(0)
    out = {}
    for bits in (32, 64):
        for name in PLAIN:
            out.update(plain_cases(ctx, name, bits))
        for name in set_names():
            out.update(set_cases(ctx, name, bits))
    ctx.close()
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: [%d, %d]" % (json.dumps(case), pair[0], pair[1]) for case, pair in sorted(out.items())) + "\n}\n")
    print("recorded %d cases in %s" % (len(out), GOLDEN))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_query_fetches.py --record")
    record()
