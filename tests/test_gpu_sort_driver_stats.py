"""The launch sequence of the sorter's host driver, pinned: after ONE construction on a fresh Context the counters the driver bumps --
scatter_launches[3], scatter_records[3], scatter_bytes[3], hist_bytes, onew_passes, group_sort --, workspace_bytes and the pass counts of
round 0 equal the values recorded in tests/golden/sort_driver_stats.json, exactly.  The parity tests compare the arrays the sorts leave;
a driver that ran a pass twice, took another form of a pass or allocated more would pass them.  The values were recorded on the library of
the commit named in the file, before the driver was rearranged (sort_scratch.hpp, launch_scatter3): the rearranged driver must repeat them.

Normal memory layout, LCP on, fixed-seed texts.  The cases, and the launch of radix_scatter3_kernel in dispatch_pass3 (engine.hpp) each
is there for -- the template arguments after <T, BLOCK, ITEMS> are <EXT, MINW, NOKO, VN, CLSB, DNEXT3>; dispatch_pass3 has eight such
launches, (a) .. (h) below:
  64-bit indices, inputs.dna(2^23 + 4097 + 3, 21), PSACX_ONE_WORD_MIN=21
    u64 dna default               the one-word prefix sort in its group form at 24 bits in the word (no launch of dispatch_pass3 in the first sort)
    u64 dna first_lead40          ... with the sub-bucket tables (PSACX_FIRST_LEAD=40: the supplement of the scratch in carve)
    u64 dna lsd                   ... as LSD bucket passes (PSACX_LSD_BUCKET_PASSES)
    u64 dna no_one_word           two-word records, 32-bit payloads: (a) <false, 6, true, 1, 8, true> digit byte out, first and middle passes;
                                  (c) <false, 6, true, 2> the widening last pass
    u64 dna no_one_word no_dig    (b) <false, 6, true, 1> the same passes without digit bytes (PSACX_NO_DIGIT_BYTES): the only case that reaches (b)
    u64 dna one_stage             three-word records, 32-bit payloads: (d) <false, 1, false, 1, 8, true> digit byte out; (f) <false, 1, false, 2> last pass
    u64 dna one_stage no_dig      (e) <false, 1, false, 1> without digit bytes; (f)
  u32 dna 2^21+5                  32-bit indices, inputs.dna(2^21 + 5, 41): (h) <false, 1, true> two-word records of 32-bit words, word payloads
  u32 / u64 dna 2^20+3            inputs.dna(2^20 + 3, 7): below SMALL_SORT_MAX, no launch of dispatch_pass3: the single-sweep look-back form
                                  (radix_scatter_kernel) with the device-side scan, which runs only while SortScratch::take keeps d_hist, d_base and
                                  d_desc back to back
  u64 two_symbols 2^23+3          the _two_symbols text of test_gpu_group_sort.py (PSACX_ONE_WORD_ALWAYS): long tie groups, the tie stage's radix path: a pair_sort of
                                  three-word records whose 32-bit payloads come in as such -- (d) and (f) with v32_in -- and refinement rounds
  u32 string set 2^21             inputs.dna(2^21, 9) cut into some 20 000 strings: key_pairs_kernel<..., GSA> and one sort over both words:
                                  (g) <false, 1> three-word records, word payloads
The first round's two ways from the two-stage sort to one sort over both words, and the reduced-memory layout in its first-round forms (the
texts are those of test_gpu_parity.py; test_the_recorded_cases_reach_their_paths holds the relations that show each path was taken):
  u64 rep probe                   a tiled text: the probe of the one-word sort finds nearly every sampled prefix repeated -> one sort over both words
  u64 rep probe first_lead40      ... the same with room for the tables of the one-word passes (a text of 2^22 characters in 256 even buckets has none in
                                  the scratch of its size; PSACX_FIRST_LEAD=40 adds the supplement of carve): the probe alone stands between this case and
  u64 rep always first_lead40     ... the probe off (PSACX_ONE_WORD_ALWAYS): the one-word passes run
  u64 third                       a third of the text repeats: the one-word sort gives up before it writes anything (PSACX_RETRY_1W: the probe's lower threshold,
                                  and at this size no room for its tables either), two stages stay: the keys are made and the two-array passes run
  u64 third no_one_word           ... the same passes asked for outright (PSACX_NO_ONE_WORD)
  u64 / u32 tandem diet           inputs.tandem(2^21 + 5, 1024, ...), PSACX_FORCE_DIET, PSACX_DIET_CAP=2^19: more ties than the reduced layout has room
                                  for -> the first round again as one sort (the abandoned attempt's passes stay in the counters), rounds in slabs
  u64 / u32 tandem diet one_stage ... one sort from the start (PSACX_ONE_STAGE)
  u64 dna diet                    inputs.dna(2^22 + 1, 6), PSACX_FORCE_DIET: two stages in the reduced layout, an even number of passes that starts from the
                                  output buffers (no room for the one-word tables at this size: the keys are made, two-array passes)
  u64 dna diet 2^23               the text of `u64 dna default`, PSACX_FORCE_DIET: the one-word form in the reduced layout, the same parity rule

`python tests/test_gpu_sort_driver_stats.py --record <commit>` writes the JSON (on a GPU) with the commit it was recorded on."""
import json
import os
import sys

import numpy as np
import pytest

import inputs

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sort_driver_stats.json")
N1 = (1 << 23) + 4097 + 3


def _dna_n1():
    return inputs.dna(N1, 21)


def _two_symbols():
    n = (1 << 23) + 3          # (test_gpu_group_sort.py: _two_symbols(n, 24))
    return np.where(inputs.splitmix64_stream(n, 24) % np.uint64(10) == 0, ord("b"), ord("a")).astype(np.uint8)


def _string_set():
    rng = np.random.RandomState(3)
    text = inputs.dna(1 << 21, 9)
    cuts = np.unique(np.concatenate([[0, text.size], rng.randint(1, text.size, size=20000)]))
    return [bytes(text[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


def _rep():
    rep = np.tile(inputs.dna(1 << 12, 9), 1 << 10)
    rep[::4099] = 84
    return rep


def _third():
    third = inputs.dna((1 << 22) + 9, 31)
    third[: (1 << 22) // 3] = np.tile(inputs.dna(1 << 11, 33), (1 << 22) // 3 // (1 << 11) + 1)[: (1 << 22) // 3]
    return third


def _tandem():
    return inputs.tandem((1 << 21) + 5, 1024, inputs.dna(1024, 3))


# name -> (index bits, text maker, string set?, PSACX_* variables)
ONE_WORD = {"PSACX_ONE_WORD_MIN": "21"}
DIET = {"PSACX_FORCE_DIET": "1", "PSACX_DIET_CAP": str(1 << 19)}
CASES = {
    "u64 dna default": (64, _dna_n1, False, ONE_WORD),
    "u64 dna first_lead40": (64, _dna_n1, False, dict(ONE_WORD, PSACX_FIRST_LEAD="40")),
    "u64 dna lsd": (64, _dna_n1, False, dict(ONE_WORD, PSACX_LSD_BUCKET_PASSES="1")),
    "u64 dna no_one_word": (64, _dna_n1, False, dict(ONE_WORD, PSACX_NO_ONE_WORD="1")),
    "u64 dna no_one_word no_dig": (64, _dna_n1, False, dict(ONE_WORD, PSACX_NO_ONE_WORD="1", PSACX_NO_DIGIT_BYTES="1")),
    "u64 dna one_stage": (64, _dna_n1, False, dict(ONE_WORD, PSACX_ONE_STAGE="1")),
    "u64 dna one_stage no_dig": (64, _dna_n1, False, dict(ONE_WORD, PSACX_ONE_STAGE="1", PSACX_NO_DIGIT_BYTES="1")),
    "u32 dna 2^21+5": (32, lambda: inputs.dna((1 << 21) + 5, 41), False, {}),
    "u32 dna 2^20+3": (32, lambda: inputs.dna((1 << 20) + 3, 7), False, {}),
    "u64 dna 2^20+3": (64, lambda: inputs.dna((1 << 20) + 3, 7), False, {}),
    "u64 two_symbols 2^23+3": (64, _two_symbols, False, dict(ONE_WORD, PSACX_ONE_WORD_ALWAYS="1")),
    "u32 string set 2^21": (32, _string_set, True, {}),
    "u64 rep probe": (64, _rep, False, ONE_WORD),
    "u64 rep probe first_lead40": (64, _rep, False, dict(ONE_WORD, PSACX_FIRST_LEAD="40")),
    "u64 rep always first_lead40": (64, _rep, False, dict(ONE_WORD, PSACX_FIRST_LEAD="40", PSACX_ONE_WORD_ALWAYS="1")),
    "u64 third": (64, _third, False, ONE_WORD),
    "u64 third no_one_word": (64, _third, False, dict(ONE_WORD, PSACX_NO_ONE_WORD="1")),
    "u64 tandem diet": (64, _tandem, False, DIET),
    "u32 tandem diet": (32, _tandem, False, DIET),
    "u64 tandem diet one_stage": (64, _tandem, False, dict(DIET, PSACX_ONE_STAGE="1")),
    "u32 tandem diet one_stage": (32, _tandem, False, dict(DIET, PSACX_ONE_STAGE="1")),
    "u64 dna diet": (64, lambda: inputs.dna((1 << 22) + 1, 6), False, dict(ONE_WORD, PSACX_FORCE_DIET="1")),
    "u64 dna diet 2^23": (64, _dna_n1, False, dict(ONE_WORD, PSACX_FORCE_DIET="1")),
}
KNOBS = sorted({k for c in CASES.values() for k in c[3]})


def run_case(name, setenv):
    """the pinned values of one case: a fresh Context, one construction; setenv(name, value) sets a PSACX_* variable"""
    import psac_amd
    bits, make, is_set, env = CASES[name]
    for k, v in env.items():
        setenv(k, v)
    ctx = psac_amd.Context(0)
    try:
        sa = psac_amd.SuffixArray(index_bits=bits, lcp=True, ctx=ctx)
        if is_set:
            sa.construct_ss(make())
        else:
            sa.construct(make())
        s = ctx.stats()
        return {"scatter_launches": [int(x) for x in s.scatter_launches], "scatter_records": [int(x) for x in s.scatter_records],
                "scatter_bytes": [int(x) for x in s.scatter_bytes], "hist_bytes": int(s.hist_bytes), "onew_passes": int(s.onew_passes),
                "group_sort": int(s.group_sort), "workspace_bytes": int(s.workspace_bytes),
                "round0_sort_passes": int(s.rounds[0].sort_passes), "round0_sort_passes_skipped": int(s.rounds[0].sort_passes_skipped)}
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_driver_stats_equal_the_recorded(golden, monkeypatch, name):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    got = run_case(name, monkeypatch.setenv)
    want = golden["cases"].get(name)
    print(name, got, want)
    assert sum(got["scatter_launches"]) > 0 and got["workspace_bytes"] > 0          # the counters are live
    assert got == want


def test_the_recording_holds_these_cases_only(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    assert len(golden["parent"]) == 40 and int(golden["parent"], 16) >= 0
    keys = sorted(["scatter_launches", "scatter_records", "scatter_bytes", "hist_bytes", "onew_passes", "group_sort", "workspace_bytes",
                   "round0_sort_passes", "round0_sort_passes_skipped"])
    assert all(sorted(v) == keys for v in golden["cases"].values())


def test_the_recorded_cases_reach_their_paths(golden):
    # equality with a recording does not show that a case takes the path it is named for: these relations between recorded values do
    c = golden["cases"]
    # the probe gave the two-stage sort up before any one-word pass; with the probe off the passes run
    for name in ("u64 rep probe", "u64 rep probe first_lead40"):
        assert c[name]["onew_passes"] == 0 and c[name]["group_sort"] == 0
    assert c["u64 rep always first_lead40"]["onew_passes"] > 0
    # the probe kept two stages in two-array passes: the launches of the form asked for outright
    assert c["u64 third"]["onew_passes"] == 0
    assert c["u64 third"]["scatter_launches"] == c["u64 third no_one_word"]["scatter_launches"]
    # the passes of the abandoned two-stage attempt are counted on top of those of the one sort that stood
    for bits in ("u64", "u32"):
        assert sum(c[bits + " tandem diet"]["scatter_launches"]) > sum(c[bits + " tandem diet one_stage"]["scatter_launches"])
    # the one-word form ran in the reduced layout
    assert c["u64 dna diet 2^23"]["onew_passes"] > 0 and c["u64 dna diet 2^23"]["workspace_bytes"] < c["u64 dna default"]["workspace_bytes"]


def record(commit):
    os.environ["PSACX_ENV_KNOBS"] = "1"                                        # (tests/conftest.py does this for the suite)
    sys.path.insert(0, os.path.dirname(HERE))
    out = {}
    for name in CASES:
        for k in KNOBS:
            os.environ.pop(k, None)
        out[name] = run_case(name, os.environ.__setitem__)
        print(name, out[name])
    with open(GOLDEN, "w") as f:
        f.write('{\n"parent": %s,\n"cases": {\n' % json.dumps(commit) + ",\n".join("%s: %s" % (json.dumps(n), json.dumps(v, sort_keys=True)) for n, v in out.items()) + "\n}\n}\n")
    print("recorded %d cases in %s" % (len(out), GOLDEN))


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_sort_driver_stats.py --record <commit the library was built from>")
    record(sys.argv[2])
