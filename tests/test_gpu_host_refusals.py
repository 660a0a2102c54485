"""The refusals of the host-pointer forms that take a pattern batch -- psacx_locate_*, psacx_locate_gsa_*, psacx_match_*,
psacx_match_gsa_*, psacx_mems_*, psacx_kmismatch_*, psacx_kedit_*, psacx_fm_search_* -- pinned call by call, in both widths.

The calls go through ctypes to the C ABI itself: the Python wrappers normalise their arguments and never send most of these.  One
table of cases (CASES) is applied to every call it has an argument for: malformed batches, missing arrays, offsets that do not fit,
a table that cannot be built, count queries, lists that are too short or partly missing, and the valid controls.  Every output
array is pre-filled with the sentinel of the suites.  Per case the return code, *z / *total (pre-set to the sentinel too: a call
that refuses before it sets it leaves the sentinel) and "every output byte is still the sentinel" are compared with
tests/golden/host_refusals.json, and the outputs of the valid controls with the host models.

The JSON is a recording of the library, not of a model: `python tests/test_gpu_host_refusals.py [path]` writes it (on a GPU).  It was
recorded once, on the commit before the host forms were folded onto one staged batch, and stays as recorded: a case that differs
is a change of behaviour.  Texts: mississippi and the set abcab, cab; nothing above n = 11 and q = 3."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import fm_model as F
import kedit_model as K
import kmismatch_model as X
import locate_gsa_model as G
import locate_model as L
import match_model as M
import mems_model as MM
import repeats_model as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_refusals.json")
SENTINEL64 = 0x5A5A5A5A5A5A5A5A
ROOM = 256                                              # entries of every list; no valid control here has as many hits
E, SAMPLE = 1, 2                                        # the errors of kmismatch / kedit; the SA sample of fm_search
WIDTHS = ("u32", "u64")
INPUTS = ("mississippi", "abcab_cab")
# name: (takes offsets: never / may / must, has k, the lists, has *z or *total)
CALLS = {
    "locate": ("never", True, ("lb", "ub"), False),
    "locate_gsa": ("must", True, ("lb", "ub"), False),
    "match": ("never", True, ("len", "lb", "ub"), False),
    "match_gsa": ("must", True, ("len", "lb", "ub"), False),
    "mems": ("may", True, ("qpos", "tpos", "len"), True),
    "kmismatch": ("may", True, ("qid", "tpos", "dist"), True),
    "kedit": ("may", True, ("qid", "tpos", "len", "dist"), True),
    "fm_search": ("may", False, ("start", "pos", "sid"), True),
}
WIDE = ("qpos", "qid", "start")                          # 64-bit whatever the width
CONTROLS = ("valid", "k2")


def pairs():
    """(call, input): the plain calls take the text, the _gsa calls the set, the others both"""
    out = []
    for call, (offs, _, _, _) in CALLS.items():
        out += [(call, name) for name in INPUTS if (offs != "never" or name == "mississippi") and (offs != "must" or name != "mississippi")]
    return out


class Input(object):
    """text, offsets (always there; `is_set` says whether a call that may go without gets them), SA, LCP and three patterns"""

    def __init__(self, name):
        strings, pats = X.NAMED[name]
        self.strings, self.pats = strings, [bytes(P) for P in pats[:3]]
        self.text, self.off, self.SA, self.LCP = R.arrays_by_definition(strings)
        self.n, self.m, self.is_set = int(self.text.size), len(strings), len(strings) > 1
        self.pat, self.poff = X.pattern_buffer(self.pats)


_inputs, _wants = {}, {}


def input_of(name):
    if name not in _inputs:
        _inputs[name] = Input(name)
    return _inputs[name]


def want_of(call, name):
    """the model's outputs of the valid control, as {output: int64 array}, and its z (None where the call has none)"""
    if (call, name) not in _wants:
        I = input_of(name)
        s, off = I.text.tobytes(), (I.off if I.is_set else None)
        if call in ("locate", "locate_gsa"):
            iv = [L.by_bisection(s, I.SA, P) if call == "locate" else G.by_bisection(s, I.off, I.SA, P) for P in I.pats]
            w, z = {"lb": [a for a, _ in iv], "ub": [b for _, b in iv]}, None
        elif call in ("match", "match_gsa"):
            rows = [M.by_bisection(s, I.SA, P, off=(None if call == "match" else I.off)) for P in I.pats]
            w, z = {"len": [r[0] for r in rows], "lb": [r[1] for r in rows], "ub": [r[2] for r in rows]}, None
        elif call == "mems":
            bwt, first, _ = R.bwt_of(I.text, I.SA, I.off)
            (qp, tp, ln), _ = MM.by_walk_arrays(I.SA, I.LCP, bwt, first, I.pats, MM.statistics(I.text, I.SA, I.pats, off))
            w, z = {"qpos": qp, "tpos": tp, "len": ln}, int(qp.size)
        elif call == "kmismatch":
            (qi, tp, di), _ = X.by_pieces(I.text, off, I.SA, I.pats, E)
            w, z = {"qid": qi, "tpos": tp, "dist": di}, int(qi.size)
        elif call == "kedit":
            (qi, tp, ln, di), _ = K.by_pieces(I.text, off, I.SA, I.pats, E)
            w, z = {"qid": qi, "tpos": tp, "len": ln, "dist": di}, int(qi.size)
        else:
            rows = [F.by_bytes(I.strings, I.SA, P) for P in I.pats]
            pos = [p for r in rows for p in r[2]]
            w = {"lb": [r[0] for r in rows], "ub": [r[1] for r in rows], "start": np.cumsum([0] + [len(r[2]) for r in rows]), "pos": pos}
            if I.is_set:
                w["sid"] = G.string_ids(I.off, pos, I.n)
            z = len(pos)
        _wants[(call, name)] = ({k: np.asarray(v, np.int64).reshape(-1) for k, v in w.items()}, z)
    return _wants[(call, name)]


# ---------------------------------------------------------------------------------------------------------------
# the cases: each changes the arguments of the valid control.  A: text, n, off, m, SA, LCP, pat, poff, q, k, cap and `null`, the
# outputs passed as NULL.  needs: "off" a call that takes offsets, "k" one that takes k, "cap" one that has lists with a cap.
# ---------------------------------------------------------------------------------------------------------------
def _set(**kw):
    return lambda A, I, lists, z: A.update(kw)


def _offsets(m=None, last=None):
    def change(A, I, lists, z):
        off = np.zeros(I.n + 2, np.uint64)                  # (room for the m + 1 entries of every m asked for here)
        off[:I.m + 1] = I.off
        if last is not None:
            off[I.m] = last(I)
        A.update(off=off, m=I.m if m is None else m(I))
    return change


def _poff(change):
    def apply(A, I, lists, z):
        p = I.poff.copy()
        change(p)
        A["poff"] = p
    return apply


def _descend(p):
    p[1], p[2] = p[2], p[1]                               # poff[1] > poff[2]; poff[0] = 0 and poff[q] stay


CASES = [
    # name, needs, change
    ("valid", None, _set()),
    ("q0", None, _set(q=0)),
    ("empty_patterns_pat_null", None, lambda A, I, lists, z: A.update(pat=None, poff=np.zeros(4, np.uint64))),
    ("pat_null", None, _set(pat=None)),
    ("poff0_is_1", None, _poff(lambda p: p.__setitem__(0, 1))),
    ("poff_descends", None, _poff(_descend)),
    ("poff_null", None, _set(poff=None)),
    ("n0", None, _set(n=0)),
    ("text_null", None, _set(text=None)),
    ("sa_null", None, _set(SA=None)),
    ("offsets_m0", "off", _offsets(m=lambda I: 0)),
    ("offsets_m_n_plus_1", "off", _offsets(m=lambda I: I.n + 1)),
    ("offsets_end_short", "off", _offsets(last=lambda I: I.n - 1)),
    ("k2", "k", _set(k=2)),
    ("k40", "k", _set(k=40)),
    ("count_query", None, lambda A, I, lists, z: A.update(null=set(lists))),
    ("cap_z_minus_1", "cap", lambda A, I, lists, z: A.update(cap=z - 1)),
    ("first_list_null", None, lambda A, I, lists, z: A.update(null={lists[0]})),
]


def cases_of(call):
    offs, has_k, _, has_z = CALLS[call]
    return [(name, change) for name, needs, change in CASES
            if needs is None or (needs == "off" and offs != "never") or (needs == "k" and has_k) or (needs == "cap" and has_z)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_case(lib, handle, suf, call, name, change):
    """(rc, z, untouched, outputs): one call of psacx_<call>_<suf> with the case's arguments on fresh outputs"""
    I = input_of(name)
    dt = np.uint32 if suf == "u32" else np.uint64
    offs, _, lists, has_z = CALLS[call]
    wz = want_of(call, name)[1]
    given = offs == "must" or (offs == "may" and I.is_set)
    A = dict(text=I.text, n=I.n, off=I.off.astype(np.uint64) if given else None, m=I.m if given else 0, SA=I.SA.astype(dt), LCP=I.LCP.astype(dt),
             pat=I.pat, poff=I.poff, q=3, k=0, cap=ROOM, null=set())
    change(A, I, lists, wz)
    names = (("lb", "ub") if call == "fm_search" else ()) + lists
    if call == "fm_search" and A["off"] is None:
        names = tuple(x for x in names if x != "sid")      # (the string numbers need the offsets)
    out = {x: np.full(ROOM * 8, 0x5A, np.uint8).view(np.uint8 if x == "dist" else np.uint64 if x in WIDE else dt)[:ROOM] for x in names}
    o = {x: (None if x in A["null"] else _p(out[x])) for x in names}
    z = C.c_uint64(SENTINEL64)
    fn = getattr(lib, "psacx_%s_%s" % (call, suf))
    t, n, sa, pat, poff, q, k = _p(A["text"]), A["n"], _p(A["SA"]), _p(A["pat"]), _p(A["poff"]), A["q"], A["k"]
    off, m = _p(A["off"]), A["m"]
    if call == "locate":
        rc = fn(handle, t, n, sa, pat, poff, q, k, o["lb"], o["ub"])
    elif call == "locate_gsa":
        rc = fn(handle, t, n, off, m, sa, pat, poff, q, k, o["lb"], o["ub"])
    elif call == "match":
        rc = fn(handle, t, n, sa, pat, poff, q, k, 0, 0, o["len"], o["lb"], o["ub"])
    elif call == "match_gsa":
        rc = fn(handle, t, n, off, m, sa, pat, poff, q, k, 0, 0, o["len"], o["lb"], o["ub"])
    elif call == "mems":
        rc = fn(handle, t, n, off, m, sa, _p(A["LCP"]), pat, poff, q, k, 1, 0, 0, o["qpos"], o["tpos"], o["len"], A["cap"], C.byref(z))
    elif call == "kmismatch":
        rc = fn(handle, t, n, off, m, sa, pat, poff, q, k, E, 0, o["qid"], o["tpos"], o["dist"], A["cap"], C.byref(z))
    elif call == "kedit":
        rc = fn(handle, t, n, off, m, sa, pat, poff, q, k, E, 0, 0, o["qid"], o["tpos"], o["len"], o["dist"], A["cap"], C.byref(z))
    else:
        rc = fn(handle, t, n, off, m, sa, SAMPLE, pat, poff, q, o["lb"], o["ub"], 0, o["start"], o["pos"], o.get("sid"), A["cap"], C.byref(z))
    untouched = all(bool(np.all(a.view(np.uint8) == 0x5A)) for a in out.values())
    return int(rc), (int(z.value) if has_z else None), untouched, out


def record(lib, handle):
    return {suf: {"%s/%s" % (call, name): {case: list(run_case(lib, handle, suf, call, name, change)[:3]) for case, change in cases_of(call)}
                  for call, name in pairs()} for suf in WIDTHS}


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


@pytest.mark.gpu
@pytest.mark.parametrize("suf", WIDTHS)
@pytest.mark.parametrize("call,name", pairs())
def test_host_refusals(ctx, golden, suf, call, name):
    rec = golden[suf]["%s/%s" % (call, name)]
    assert sorted(rec) == sorted(case for case, _ in cases_of(call))
    want, wz = want_of(call, name)
    for case, change in cases_of(call):
        rc, z, untouched, out = run_case(ctx._lib, ctx.handle, suf, call, name, change)
        assert [rc, z, untouched] == rec[case], (case, [rc, z, untouched], rec[case])
        if case in CONTROLS:                                # the outputs themselves, and nothing behind them
            assert rc == 0 and z == wz, (case, rc, z, wz)
            for x, a in out.items():
                w = want[x]
                assert np.array_equal(a[:w.size].astype(np.int64), w), (case, x, a[:w.size].tolist(), w.tolist())
                assert np.all(a[w.size:].view(np.uint8) == 0x5A), (case, x)
        elif case == "count_query" and wz is not None:
            assert rc == 0 and z == (0 if call == "fm_search" else wz), (case, rc, z, wz)


if __name__ == "__main__":                             # writes tests/golden/host_refusals.json (or the path given) from the library
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import psac_amd
    c = psac_amd.Context(0)
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(record(c._lib, c.handle), f, indent=0, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    c.close()
