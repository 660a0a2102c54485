"""Python mirror of the reference's suffix_array<> interface for one rank / one GPU."""
import ctypes as C
import sys

import numpy as np

from . import _lib
from ._lib import PSACX_LCP, PSACX_NO_FAST, PSACX_PROFILE, PsacxError, Stats
from ._lib import PSACX_MATCH_SUFFIXES as MATCH_SUFFIXES
from ._lib import PSACX_OVERLAP_WHOLE as OVERLAP_WHOLE

NEAREST_SM, NEAREST_EQ, FURTHEST_EQ = 0, 1, 2      # ansv_common.hpp:20-22


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Context(object):
    """One HIP device + stream + reusable HBM workspace (psacx_ctx)."""

    def __init__(self, device=0, stream=None):
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.psacx_create(C.byref(h), int(device), C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise PsacxError(rc, self._lib.psacx_strerror(rc).decode())
        self.handle = h
        self.device = device

    def check(self, rc):
        if rc != 0:
            msg = self._lib.psacx_strerror(rc).decode()
            detail = self._lib.psacx_last_hip_error(self.handle).decode()
            raise PsacxError(rc, msg + (" [" + detail + "]" if detail else ""))

    def stats(self):
        s = Stats()
        self.check(self._lib.psacx_get_stats(self.handle, C.byref(s)))
        return s

    def configure(self, **options):
        """psacx_configure: pins the form of single stages (include/psacx.h), e.g. configure(force_diet=1, diet_cap=1 << 20), configure(reset=0)."""
        for name, value in options.items():
            self.check(self._lib.psacx_configure(self.handle, _lib.OPTIONS[name] if name in _lib.OPTIONS else _lib.KERNEL_OPTIONS[name], int(value)))

    def _pre(self):
        """Before every call that runs the engine: with _lib.ENV_KNOBS the options come from PSACX_* variables (debug shim)."""
        if _lib.ENV_KNOBS:
            self.check(self._lib.psacx_configure_from_env(self.handle))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.psacx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # raw device memory (for callers without their own HIP bindings)
    def alloc(self, nbytes):
        p = C.c_void_p()
        self.check(self._lib.psacx_dev_alloc(self.handle, C.byref(p), nbytes))
        return p.value

    def free(self, p):
        self.check(self._lib.psacx_dev_free(self.handle, C.c_void_p(p)))

    def h2d(self, dptr, arr):
        a = np.ascontiguousarray(arr)
        self.check(self._lib.psacx_copy_h2d(self.handle, C.c_void_p(dptr), _ptr(a), a.nbytes))

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        self.check(self._lib.psacx_copy_d2h(self.handle, _ptr(arr), C.c_void_p(dptr), arr.nbytes))


def parse_stringset(strings, sep=None):
    """simple_dstringset::parse (stringset.hpp:43-72) on one rank: returns (characters of all strings
    back to back as uint8, uint64 offsets[m + 1]).  A flat buffer is cut at runs of `sep`; empty
    strings do not exist in a set."""
    if isinstance(strings, (list, tuple)):
        parts = [np.frombuffer(x.encode("latin-1") if isinstance(x, str) else bytes(x), dtype=np.uint8) for x in strings]
        parts = [p for p in parts if p.size]
        off = np.zeros(len(parts) + 1, np.uint64)
        if parts:
            off[1:] = np.cumsum([p.size for p in parts])
        return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), off
    flat = strings
    if isinstance(flat, str):
        flat = flat.encode("latin-1")
    flat = np.frombuffer(bytes(flat), dtype=np.uint8) if isinstance(flat, (bytes, bytearray)) \
        else np.ascontiguousarray(flat, dtype=np.uint8)
    s = ord('$') if sep is None else (ord(sep) if isinstance(sep, (str, bytes)) else int(sep))
    keep = flat != s
    text = np.ascontiguousarray(flat[keep])
    # a string starts at every kept character whose predecessor is a separator (or the start)
    prev_sep = np.ones(flat.size, bool)
    prev_sep[1:] = ~keep[:-1]
    starts_flat = np.nonzero(keep & prev_sep)[0]
    kept_before = np.cumsum(keep) - keep            # kept characters before each flat position
    off = np.zeros(starts_flat.size + 1, np.uint64)
    off[:-1] = kept_before[starts_flat]
    off[-1] = text.size
    return text, off


class SuffixArray(object):
    """suffix_array<char, index_t, LCP> for a whole text held by one rank.

    Fields follow the reference (suffix_array.hpp:180-212): n, local_size,
    local_SA, local_B (0-based inverse suffix array after construct()),
    local_LCP (empty unless lcp=True), local_Lc (left-branching characters,
    suffix_array.hpp:211-212, empty unless lc=True; lc implies lcp).  `log` receives the reference's stderr
    lines ("Alphabet: ...", "iteration h: unfinished buckets = ...").
    """

    def __init__(self, index_bits=64, lcp=False, ctx=None, log=None, lc=False):
        if index_bits not in (32, 64):
            raise ValueError("index_bits must be 32 or 64")
        self.index_bits = index_bits
        self.lc = bool(lc)
        self.lcp = bool(lcp) or self.lc
        self.ctx = ctx if ctx is not None else Context(0)
        self.dtype = np.uint32 if index_bits == 32 else np.uint64
        self.log = log
        self.n = 0
        self.local_size = 0
        self.p = 1
        self.local_SA = np.zeros(0, self.dtype)
        self.local_B = np.zeros(0, self.dtype)
        self.local_LCP = np.zeros(0, self.dtype)
        self.local_Lc = np.zeros(0, np.uint8)
        self.k = 0
        self.sigma = 0
        self.bits_per_char = 0
        self.rounds = []

    def _flags(self, fast_resolval, profile):
        f = 0
        if self.lcp:
            f |= PSACX_LCP
        if not fast_resolval:
            f |= PSACX_NO_FAST
        if profile:
            f |= PSACX_PROFILE
        return f

    def _after(self):
        s = self.ctx.stats()
        self.k, self.sigma, self.bits_per_char = s.k, s.sigma, s.bits_per_char
        self.rounds = [(r.h, r.unfinished_buckets, r.unfinished_elements, r.active, r.sort_passes,
                        r.sort_passes_skipped) for r in s.rounds[:s.n_rounds]]
        if self.log is not None:
            for r in self.rounds:
                self.log.write("iteration %d: unfinished buckets = %d, unfinished elements = %d\n" % r[:3])
        return s

    def construct(self, text, fast_resolval=True, k=0, profile=False):
        """suffix_array::construct(begin, end, fast_resolval, k) (suffix_array.hpp:469-486)."""
        if isinstance(text, str):
            text = text.encode("latin-1")
        t = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) \
            else np.ascontiguousarray(text, dtype=np.uint8)
        n = int(t.size)
        if n == 0:
            raise ValueError("empty input")
        if self.index_bits == 32 and n > 0xFFFFFFFE:
            raise PsacxError(-2, "input too long for the index type")
        self.n = self.local_size = n
        self.local_SA = np.empty(n, self.dtype)
        self.local_B = np.empty(n, self.dtype)
        self.local_LCP = np.empty(n, self.dtype) if self.lcp else np.zeros(0, self.dtype)
        self.local_Lc = np.empty(n, np.uint8) if self.lc else np.zeros(0, np.uint8)
        args = [self.ctx.handle, _ptr(t), n, int(k), self._flags(fast_resolval, profile), _ptr(self.local_SA),
                _ptr(self.local_B), _ptr(self.local_LCP) if self.lcp else None]
        if self.lc:
            fn = getattr(self.ctx._lib, "psacx_construct_lc_u%d" % self.index_bits)
            args.append(_ptr(self.local_Lc))
        else:
            fn = getattr(self.ctx._lib, "psacx_construct_u%d" % self.index_bits)
        self.ctx._pre()
        self.ctx.check(fn(*args))
        self._text, self._text_off = t, None
        return self._after()

    def construct_into(self, text, SA, B, LCP=None, fast_resolval=True, k=0):
        """construct() writing into result arrays the caller already holds (a second construct() on the same
        object reuses its vectors in the reference, test/test_psac.cpp:148-170).  Returns (SA, B, LCP)."""
        t = np.ascontiguousarray(text, dtype=np.uint8)
        n = int(t.size)
        assert SA.size == n and B.size == n and SA.dtype == self.dtype and B.dtype == self.dtype
        assert (LCP is not None and LCP.size == n) or not self.lcp
        fn = getattr(self.ctx._lib, "psacx_construct_u%d" % self.index_bits)
        self.ctx._pre()
        self.ctx.check(fn(self.ctx.handle, _ptr(t), n, int(k), self._flags(fast_resolval, False), _ptr(SA), _ptr(B),
                          _ptr(LCP) if self.lcp else None))
        self.n = self.local_size = n
        self._after()
        return SA, B, LCP

    def construct_ss(self, strings, sep=None, k=0, profile=False):
        """suffix_array::construct_ss(simple_dstringset&, alphabet) (suffix_array.hpp:267-363): the
        generalized suffix array of a set of strings.  `strings` is a list of byte strings, or one
        flat buffer cut at runs of `sep` (stringset.hpp:43-72, default '$' as stringset.hpp:147; gsac
        passes '\\n', src/gsac.cpp:170).
        Positions in local_SA count the characters of the strings back to back, separators left out."""
        text, off = parse_stringset(strings, sep)
        n = int(text.size)
        if n == 0:
            raise ValueError("empty input")
        if self.index_bits == 32 and n > 0xFFFFFFFE:
            raise PsacxError(-2, "input too long for the index type")
        if self.lc:
            raise ValueError("left-branching characters are not defined for string sets")
        self.n = self.local_size = n
        self.local_SA = np.empty(n, self.dtype)
        self.local_B = np.empty(n, self.dtype)
        self.local_LCP = np.empty(n, self.dtype) if self.lcp else np.zeros(0, self.dtype)
        fn = getattr(self.ctx._lib, "psacx_construct_gsa_u%d" % self.index_bits)
        self.ctx._pre()
        self.ctx.check(fn(self.ctx.handle, _ptr(text), n, _ptr(off), int(off.size - 1), int(k), self._flags(True, profile),
                          _ptr(self.local_SA), _ptr(self.local_B), _ptr(self.local_LCP) if self.lcp else None))
        self.string_offsets = off
        self._text, self._text_off = text, off
        return self._after()

    def overlaps(self, min_len, whole=False):
        """The suffix-prefix overlaps of the string set of the last construct_ss (which needs lcp=True): overlaps() over its arrays."""
        if getattr(self, "string_offsets", None) is None or not self.lcp or self.local_LCP.size != self.n:
            raise ValueError("overlaps needs construct_ss with lcp=True first")
        return overlaps(self.n, self.string_offsets, self.local_SA, self.local_B, self.local_LCP, min_len, whole, ctx=self.ctx)

    def lz77(self):
        """The greedy LZ77 parse (start, src) of the text of the last construct (which needs lcp=True): lz77() over its arrays."""
        if getattr(self.ctx, "nranks", 1) != 1:
            raise ValueError("lz77 needs a single-rank context (the parse runs on one GPU)")
        if getattr(self, "string_offsets", None) is not None or not self.lcp or self.n == 0 or self.local_LCP.size != self.n:
            raise ValueError("lz77 needs construct of one text with lcp=True first")
        return lz77(self.local_SA, self.local_LCP, ctx=self.ctx)

    def bwt(self):
        """(bwt, primary) of the text or string set of the last construct / construct_ss: bwt() over its arrays."""
        if getattr(self.ctx, "nranks", 1) != 1:
            raise ValueError("bwt needs a single-rank context (the transform runs on one GPU)")
        if getattr(self, "_text", None) is None or self._text.size != self.n or self.local_SA.size != self.n:
            raise ValueError("bwt needs construct or construct_ss first")
        return bwt(self._text, self.local_SA, offsets=self._text_off, ctx=self.ctx)

    def repeats(self, kind="maximal", min_len=1, min_occ=2, max_occ=0):
        """(lb, ub, length) of the repeats of the text or string set of the last construct / construct_ss (which needs lcp=True):
        repeats() over its arrays."""
        if getattr(self.ctx, "nranks", 1) != 1:
            raise ValueError("repeats needs a single-rank context (the enumeration runs on one GPU)")
        if getattr(self, "_text", None) is None or self._text.size != self.n or not self.lcp or self.local_LCP.size != self.n:
            raise ValueError("repeats needs construct or construct_ss with lcp=True first")
        return repeats(self._text, self.local_SA, self.local_LCP, kind, min_len, min_occ, max_occ, offsets=self._text_off, ctx=self.ctx)

    def _doc_ready(self, what, need_lcp):
        if getattr(self.ctx, "nranks", 1) != 1:
            raise ValueError("%s needs a single-rank context (the index is built on one GPU)" % what)
        if getattr(self, "string_offsets", None) is None or self.local_SA.size != self.n or (need_lcp and (not self.lcp or self.local_LCP.size != self.n)):
            raise ValueError("%s needs construct_ss%s first" % (what, " with lcp=True" if need_lcp else ""))

    def doc_count(self, lb, ub):
        """The number of distinct strings in each LCP-interval [lb[j], ub[j]) of the string set of the last construct_ss (which needs
        lcp=True): doc_count() over its arrays."""
        self._doc_ready("doc_count", True)
        return doc_count(self.local_SA, self.local_LCP, self.string_offsets, lb, ub, ctx=self.ctx)

    def doc_list(self, lb, ub, max_cand=0):
        """(start, sid, pos): each string of the intervals [lb[j], ub[j]) once, over the string set of the last construct_ss:
        doc_list() over its arrays."""
        self._doc_ready("doc_list", False)
        return doc_list(self.local_SA, self.string_offsets, lb, ub, max_cand=max_cand, ctx=self.ctx)

    def common_repeats(self, min_docs, max_docs=0, kind="right", min_len=1):
        """(lb, ub, length, docs) of the repeats of the string set of the last construct_ss (which needs lcp=True) that occur in at
        least min_docs strings (and in at most max_docs where max_docs > 0): repeats(), then doc_count(), then a filter.  The filter
        runs on the host in numpy; the repeats are not filtered on the device.  The longest substring common to at least min_docs
        strings is the row at the argmax of length."""
        self._doc_ready("common_repeats", True)
        lb, ub, ln = self.repeats(kind, min_len=min_len)
        docs = self.doc_count(lb, ub)
        keep = (docs >= min_docs) & ((docs <= max_docs) if max_docs else True)
        return lb[keep], ub[keep], ln[keep], docs[keep]

    def fm_index(self, sample=32, text_rate=0):
        """The FMIndex of the text or string set of the last construct / construct_ss: fm_index() over its arrays.  The index owns its
        memory in HBM alone and stays usable after this object, its text and its arrays are gone; sample=0 builds one that counts only; text_rate > 0 adds the text samples, with which the index gives the
        text back (FMIndex.extract, .text, .context)."""
        if getattr(self.ctx, "nranks", 1) != 1:
            raise ValueError("fm_index needs a single-rank context (the index is built on one GPU)")
        if getattr(self, "_text", None) is None or self._text.size != self.n or self.local_SA.size != self.n:
            raise ValueError("fm_index needs construct or construct_ss first")
        return fm_index(self._text, self.local_SA, sample=sample, offsets=self._text_off, ctx=self.ctx, text_rate=text_rate)

    def mems(self, patterns, min_len, k=0, max_occ=0, super=False):
        """(qpos, tpos, len) of the maximal exact matches of the patterns against the text or string set of the last construct /
        construct_ss (which needs lcp=True): mems() over its arrays."""
        if getattr(self.ctx, "nranks", 1) != 1:
            raise ValueError("mems needs a single-rank context (the search runs on one GPU)")
        if getattr(self, "_text", None) is None or self._text.size != self.n or not self.lcp or self.local_LCP.size != self.n:
            raise ValueError("mems needs construct or construct_ss with lcp=True first")
        return mems(self._text, self.local_SA, self.local_LCP, patterns, min_len, k=k, offsets=self._text_off, max_occ=max_occ, super=super,
                    ctx=self.ctx)

    def kmismatch(self, patterns, e, k=0, max_cand=0):
        """(qid, tpos, dist) of the occurrences of the patterns with at most e substituted bytes in the text or string set of the last
        construct / construct_ss: kmismatch() over its arrays."""
        if getattr(self.ctx, "nranks", 1) != 1:
            raise ValueError("kmismatch needs a single-rank context (the search runs on one GPU)")
        if getattr(self, "_text", None) is None or self._text.size != self.n or self.local_SA.size != self.n:
            raise ValueError("kmismatch needs construct or construct_ss first")
        return kmismatch(self._text, self.local_SA, patterns, e, k=k, offsets=self._text_off, max_cand=max_cand, ctx=self.ctx)

    def kedit(self, patterns, e, k=0, max_cand=0, best=False):
        """(qid, tpos, len, dist) of the places where the patterns occur within edit distance e in the text (or string set) of the last
        construct / construct_ss: kedit() over its arrays."""
        if getattr(self.ctx, "nranks", 1) != 1:
            raise ValueError("kedit needs a single-rank context (the search runs on one GPU)")
        if getattr(self, "_text", None) is None or self._text.size != self.n or self.local_SA.size != self.n:
            raise ValueError("kedit needs construct or construct_ss first")
        return kedit(self._text, self.local_SA, patterns, e, k=k, offsets=self._text_off, max_cand=max_cand, best=best, ctx=self.ctx)

    def construct_device(self, d_text, n, d_sa, d_isa, d_lcp=None, fast_resolval=True, k=0, profile=False, d_lc=None):
        """Same with every buffer already resident in HBM (raw device addresses)."""
        args = [self.ctx.handle, C.c_void_p(d_text), int(n), int(k), self._flags(fast_resolval, profile),
                C.c_void_p(d_sa), C.c_void_p(d_isa), C.c_void_p(d_lcp) if d_lcp else None]
        if d_lc:
            fn = getattr(self.ctx._lib, "psacx_construct_lc_dev_u%d" % self.index_bits)
            args.append(C.c_void_p(d_lc))
        else:
            fn = getattr(self.ctx._lib, "psacx_construct_dev_u%d" % self.index_bits)
        self.ctx._pre()
        self.ctx.check(fn(*args))
        self.n = self.local_size = int(n)
        return self._after()


def suffix_tree(text, SA, LCP, ctx=None):
    """construct_suffix_tree(sa, begin, end, comm) (suffix_tree.hpp:413-499) at one rank: the
    n x (sigma + 1) node table (see psacx_suffix_tree_* in include/psacx.h)."""
    if isinstance(text, str):
        text = text.encode("latin-1")
    t = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    sa, lcp = np.ascontiguousarray(SA), np.ascontiguousarray(LCP)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_suffix_tree_u%d" % (sa.dtype.itemsize * 8))
    sigma = C.c_uint32(0)
    ctx.check(fn(ctx.handle, _ptr(t), t.size, None, None, None, C.byref(sigma)))
    nodes = np.zeros(t.size * (sigma.value + 1), np.uint64)
    ctx.check(fn(ctx.handle, _ptr(t), t.size, _ptr(sa), _ptr(lcp), _ptr(nodes), C.byref(sigma)))
    return nodes.reshape(t.size, sigma.value + 1)


def suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, index_bits):
    """psacx_suffix_tree_dev_*: the node table of suffix_tree() with every array resident in HBM (raw device addresses), e.g.
    the SA / LCP construct_device left there.  d_nodes receives n x (sigma + 1) uint64 cells; with d_nodes=None only sigma is
    computed, to size it.  Returns (sigma, edges): edges = records written = nonzero cells (0 for the query)."""
    fn = getattr(ctx._lib, "psacx_suffix_tree_dev_u%d" % index_bits)
    sigma, edges = C.c_uint32(0), C.c_uint64(0)
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_sa) if d_sa else None, C.c_void_p(d_lcp) if d_lcp else None,
                 C.c_void_p(d_nodes) if d_nodes else None, C.byref(sigma), C.byref(edges)))
    return sigma.value, edges.value


def check_suffix_tree_device(ctx, d_text, n, d_sa, d_lcp, d_nodes, index_bits):
    """psacx_check_suffix_tree_dev_*: is the table at d_nodes the suffix tree of the text / SA / LCP as given (all in HBM)?
    Returns [records not matched, nonzero cells no record accounts for, records, nonzero cells]; correct iff the first two
    are zero.  SA and LCP themselves are check_device's business."""
    out = (C.c_uint64 * 4)()
    fn = getattr(ctx._lib, "psacx_check_suffix_tree_dev_u%d" % index_bits)
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_sa), C.c_void_p(d_lcp), C.c_void_p(d_nodes), out))
    return list(out)


def suffix_tree_gsa(text, offsets, SA, LCP, ctx=None):
    """construct_gst with gst_edgechars (suffix_tree.hpp:501-608) at one rank: the n x (sigma + 2) node table of a string set
    (psacx_suffix_tree_gsa_* in include/psacx.h) from the characters of the strings back to back, their m + 1 offsets and the
    SA / LCP construct_ss leaves (SuffixArray.string_offsets, local_SA, local_LCP)."""
    if isinstance(text, str):
        text = text.encode("latin-1")
    t = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    sa, lcp = np.ascontiguousarray(SA), np.ascontiguousarray(LCP)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_suffix_tree_gsa_u%d" % (sa.dtype.itemsize * 8))
    sigma = C.c_uint32(0)
    ctx.check(fn(ctx.handle, _ptr(t), t.size, _ptr(off), off.size - 1, None, None, None, C.byref(sigma)))
    nodes = np.zeros(t.size * (sigma.value + 2), np.uint64)
    ctx.check(fn(ctx.handle, _ptr(t), t.size, _ptr(off), off.size - 1, _ptr(sa), _ptr(lcp), _ptr(nodes), C.byref(sigma)))
    return nodes.reshape(t.size, sigma.value + 2)


def suffix_tree_gsa_device(ctx, d_text, n, d_off, m, d_sa, d_lcp, d_nodes, index_bits):
    """psacx_suffix_tree_gsa_dev_*: the node table of suffix_tree_gsa() with every array resident in HBM (raw device addresses),
    e.g. what psacx_construct_gsa_dev_* left there; d_off holds the m + 1 string offsets as uint64.  d_nodes receives
    n x (sigma + 2) uint64 cells; with d_nodes=None only sigma is computed, to size it.  Returns (sigma, edges): edges = records
    written, leaf + internal (0 for the query)."""
    fn = getattr(ctx._lib, "psacx_suffix_tree_gsa_dev_u%d" % index_bits)
    sigma, edges = C.c_uint32(0), C.c_uint64(0)
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_off) if d_off else None, int(m), C.c_void_p(d_sa) if d_sa else None,
                 C.c_void_p(d_lcp) if d_lcp else None, C.c_void_p(d_nodes) if d_nodes else None, C.byref(sigma), C.byref(edges)))
    return sigma.value, edges.value


def check_suffix_tree_gsa_device(ctx, d_text, n, d_off, m, d_sa, d_lcp, d_nodes, index_bits):
    """psacx_check_suffix_tree_gsa_dev_*: is the table at d_nodes the suffix tree of the string set / SA / LCP as given (all in
    HBM)?  Returns [records not matched, nonzero cells no record accounts for, records, nonzero cells]; correct iff the first
    two are zero.  SA and LCP themselves are check_gsa_device's business."""
    out = (C.c_uint64 * 4)()
    fn = getattr(ctx._lib, "psacx_check_suffix_tree_gsa_dev_u%d" % index_bits)
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_off), int(m), C.c_void_p(d_sa), C.c_void_p(d_lcp), C.c_void_p(d_nodes), out))
    return list(out)


def pattern_buffer(patterns):
    """The layout psacx_locate_* takes: (the patterns back to back as uint8, their q + 1 offsets as uint64).  A pattern is bytes, a str
    (latin-1) or an array of bytes; an empty one is legal."""
    parts = [np.frombuffer(x.encode("latin-1") if isinstance(x, str) else bytes(x), dtype=np.uint8) if isinstance(x, (str, bytes, bytearray))
             else np.ascontiguousarray(x, dtype=np.uint8) for x in patterns]
    off = np.zeros(len(parts) + 1, np.uint64)
    if parts:
        off[1:] = np.cumsum([p.size for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), off


def lookup_table_device(ctx, d_text, n, d_sa, k, d_table, index_bits):
    """psacx_lookup_table_dev_*: the k-mer lookup table of a text resident in HBM (lookup_index, lookup_table.hpp:36-149, with dense
    keys; include/psacx.h defines it).  d_table receives B^k + 1 entries of the index type, B = sigma + 1; with d_table=None only
    the sizes are computed (d_sa may be None then).  Returns (code, sigma, entries): code = the 256 alphabet codes as uint16,
    which locate_device takes."""
    fn = getattr(ctx._lib, "psacx_lookup_table_dev_u%d" % index_bits)
    code = np.zeros(256, np.uint16)
    sigma, entries = C.c_uint32(0), C.c_uint64(0)
    ctx._pre()
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_sa) if d_sa else None, int(k), C.c_void_p(d_table) if d_table else None,
                 _ptr(code), C.byref(sigma), C.byref(entries)))
    return code, sigma.value, entries.value


def locate_device(ctx, d_text, n, d_sa, d_table, k, code, d_pat, d_poff, q, d_lb, d_ub, index_bits):
    """psacx_locate_dev_*: [lb, ub) of q patterns in the suffix array at d_sa (sa_index::locate, seq_query.hpp:246-251), everything
    resident in HBM (raw device addresses): d_pat the patterns back to back, d_poff their q + 1 uint64 offsets, d_lb / d_ub q entries
    of the index type each.  d_table / k / code as lookup_table_device left them, or None / 0 / None for the search without a table."""
    fn = getattr(ctx._lib, "psacx_locate_dev_u%d" % index_bits)
    cd = None if code is None else np.ascontiguousarray(code, dtype=np.uint16)
    ctx._pre()
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_sa), C.c_void_p(d_table) if d_table else None, int(k),
                 _ptr(cd) if cd is not None else None, C.c_void_p(d_pat), C.c_void_p(d_poff), int(q), C.c_void_p(d_lb), C.c_void_p(d_ub)))


def string_ends_device(ctx, d_off, m, n, d_ends):
    """psacx_string_ends_dev: the bitmap of the string ends of a set resident in HBM -- bit p = "a string starts at p, or p == n" --
    from its m + 1 uint64 offsets at d_off, into the (n >> 5) + 1 uint32 words at d_ends.  It belongs to the index as the lookup
    table does: lookup_table_gsa_device and locate_gsa_device take it.  With d_ends=None only the size is computed.  Returns the
    number of words."""
    words = C.c_uint64(0)
    ctx._pre()
    ctx.check(ctx._lib.psacx_string_ends_dev(ctx.handle, C.c_void_p(d_off) if d_off else None, int(m), int(n),
                                             C.c_void_p(d_ends) if d_ends else None, C.byref(words)))
    return words.value


def lookup_table_gsa_device(ctx, d_text, n, d_ends, k, d_table, index_bits):
    """psacx_lookup_table_gsa_dev_*: lookup_table_device for a string set, its keys cut at the string ends of the bitmap at d_ends
    (string_ends_device).  With d_table=None only the sizes are computed.  Returns (code, sigma, entries)."""
    fn = getattr(ctx._lib, "psacx_lookup_table_gsa_dev_u%d" % index_bits)
    code = np.zeros(256, np.uint16)
    sigma, entries = C.c_uint32(0), C.c_uint64(0)
    ctx._pre()
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_ends) if d_ends else None, int(k), C.c_void_p(d_table) if d_table else None,
                 _ptr(code), C.byref(sigma), C.byref(entries)))
    return code, sigma.value, entries.value


def locate_gsa_device(ctx, d_text, n, d_ends, d_sa, d_table, k, code, d_pat, d_poff, q, d_lb, d_ub, index_bits):
    """psacx_locate_gsa_dev_*: locate_device over the generalized suffix array of a string set: suffix i ends where its string
    ends, so no pattern matches across two strings.  d_ends is the bitmap of string_ends_device; d_table / k / code as
    lookup_table_gsa_device left them, or None / 0 / None."""
    fn = getattr(ctx._lib, "psacx_locate_gsa_dev_u%d" % index_bits)
    cd = None if code is None else np.ascontiguousarray(code, dtype=np.uint16)
    ctx._pre()
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_ends) if d_ends else None, C.c_void_p(d_sa),
                 C.c_void_p(d_table) if d_table else None, int(k), _ptr(cd) if cd is not None else None, C.c_void_p(d_pat), C.c_void_p(d_poff),
                 int(q), C.c_void_p(d_lb), C.c_void_p(d_ub)))


def occurrences_device(ctx, d_sa, n, d_off, m, d_lb, d_ub, q, limit, d_start, d_pos, d_sid, cap, index_bits):
    """psacx_occurrences_dev_*: the occurrence lists of q intervals resident in HBM.  d_start receives q + 1 uint64 (the exclusive
    prefix sums of the counts, each capped at limit where limit > 0), d_pos the positions SA[lb_j + t] in SA order, d_sid (with
    d_off, the m + 1 string offsets) the string holding each.  d_pos=None is the size query.  Returns the total; raises
    PsacxError -2 where it exceeds cap, with d_start valid and d_pos untouched."""
    fn = getattr(ctx._lib, "psacx_occurrences_dev_u%d" % index_bits)
    total = C.c_uint64(0)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    ctx.check(fn(ctx.handle, opt(d_sa), int(n), opt(d_off), int(m), opt(d_lb), opt(d_ub), int(q), int(limit), opt(d_start), opt(d_pos), opt(d_sid),
                 int(cap), C.byref(total)))
    return total.value


def locate(text, SA, patterns, k=0, ctx=None, offsets=None):
    """psacx_locate_*: (lb, ub) arrays -- pattern i occurs at SA[lb[i]:ub[i]]; where it does not occur lb[i] == ub[i] is its insertion
    point -- for a list of patterns (bytes, str or byte arrays) in the suffix array SA of text.  k > 0 builds the k-mer lookup table
    first and starts every search in its bucket; the answers are the same.  Host arrays; everything is staged for the call.
    offsets: text is a string set laid back to back, offsets its m + 1 string offsets and SA its generalized suffix array
    (psacx_locate_gsa_*); a pattern then never matches across two strings."""
    if isinstance(text, str):
        text = text.encode("latin-1")
    t = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    sa = np.ascontiguousarray(SA)
    if sa.dtype not in (np.uint32, np.uint64):
        raise TypeError("locate needs a uint32 or uint64 suffix array")
    pat, off = pattern_buffer(patterns)
    q = int(off.size - 1)
    lb, ub = np.zeros(q, sa.dtype), np.zeros(q, sa.dtype)
    ctx = ctx if ctx is not None else Context(0)
    ctx._pre()
    if offsets is None:
        fn = getattr(ctx._lib, "psacx_locate_u%d" % (sa.dtype.itemsize * 8))
        ctx.check(fn(ctx.handle, _ptr(t), t.size, _ptr(sa), _ptr(pat) if pat.size else None, _ptr(off), q, int(k), _ptr(lb), _ptr(ub)))
    else:
        so = np.ascontiguousarray(offsets, dtype=np.uint64)
        fn = getattr(ctx._lib, "psacx_locate_gsa_u%d" % (sa.dtype.itemsize * 8))
        ctx.check(fn(ctx.handle, _ptr(t), t.size, _ptr(so), so.size - 1, _ptr(sa), _ptr(pat) if pat.size else None, _ptr(off), q, int(k), _ptr(lb),
                     _ptr(ub)))
    return lb, ub


def match_device(ctx, d_text, n, d_sa, d_table, k, code, d_pat, d_poff, q, flags, max_len, out_entries, d_len, d_lb, d_ub, index_bits):
    """psacx_match_dev_*: for every query the length of its longest prefix that occurs and the locate interval of that prefix
    (include/psacx.h: "longest match and matching statistics"), everything resident in HBM.  Arguments as locate_device; flags = 0
    takes one query per pattern (out_entries = q), MATCH_SUFFIXES one per byte of the pattern buffer (out_entries = poff[q]);
    max_len > 0 cuts every query to that many bytes.  d_len / d_lb / d_ub receive out_entries entries of the index type each."""
    fn = getattr(ctx._lib, "psacx_match_dev_u%d" % index_bits)
    cd = None if code is None else np.ascontiguousarray(code, dtype=np.uint16)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_sa), opt(d_table), int(k), _ptr(cd) if cd is not None else None,
                 C.c_void_p(d_pat), C.c_void_p(d_poff), int(q), int(flags), int(max_len), int(out_entries), opt(d_len), opt(d_lb), opt(d_ub)))


def match_gsa_device(ctx, d_text, n, d_ends, d_sa, d_table, k, code, d_pat, d_poff, q, flags, max_len, out_entries, d_len, d_lb, d_ub, index_bits):
    """psacx_match_gsa_dev_*: match_device over the generalized suffix array of a string set; d_ends is the bitmap of
    string_ends_device, and a match never crosses a string end."""
    fn = getattr(ctx._lib, "psacx_match_gsa_dev_u%d" % index_bits)
    cd = None if code is None else np.ascontiguousarray(code, dtype=np.uint16)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), opt(d_ends), C.c_void_p(d_sa), opt(d_table), int(k), _ptr(cd) if cd is not None else None,
                 C.c_void_p(d_pat), C.c_void_p(d_poff), int(q), int(flags), int(max_len), int(out_entries), opt(d_len), opt(d_lb), opt(d_ub)))


def match(text, SA, patterns, k=0, offsets=None, suffixes=False, max_len=0, ctx=None):
    """psacx_match_*: (len, lb, ub) arrays -- the longest prefix of query i that occurs in text has len[i] bytes and occurs at
    SA[lb[i]:ub[i]]; len[i] == 0 gives [0, n).  One query per pattern, or with suffixes=True one per byte of the pattern buffer (the
    query at buffer position p is the rest of its pattern from p on: the matching statistics of every pattern), in buffer order.
    max_len > 0 cuts every query to that many bytes.  k > 0 puts the k-mer lookup table in front; the answers are the same.
    offsets: text is a string set and SA its generalized suffix array (psacx_match_gsa_*); a match never crosses a string end.
    Host arrays; everything is staged for the call."""
    if isinstance(text, str):
        text = text.encode("latin-1")
    t = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)
    sa = np.ascontiguousarray(SA)
    if sa.dtype not in (np.uint32, np.uint64):
        raise TypeError("match needs a uint32 or uint64 suffix array")
    pat, off = pattern_buffer(patterns)
    q = int(off.size - 1)
    entries = int(off[q]) if suffixes else q
    ln, lb, ub = np.zeros(entries, sa.dtype), np.zeros(entries, sa.dtype), np.zeros(entries, sa.dtype)
    flags = MATCH_SUFFIXES if suffixes else 0
    ctx = ctx if ctx is not None else Context(0)
    ctx._pre()
    if offsets is None:
        fn = getattr(ctx._lib, "psacx_match_u%d" % (sa.dtype.itemsize * 8))
        ctx.check(fn(ctx.handle, _ptr(t), t.size, _ptr(sa), _ptr(pat) if pat.size else None, _ptr(off), q, int(k), flags, int(max_len), _ptr(ln),
                     _ptr(lb), _ptr(ub)))
    else:
        so = np.ascontiguousarray(offsets, dtype=np.uint64)
        fn = getattr(ctx._lib, "psacx_match_gsa_u%d" % (sa.dtype.itemsize * 8))
        ctx.check(fn(ctx.handle, _ptr(t), t.size, _ptr(so), so.size - 1, _ptr(sa), _ptr(pat) if pat.size else None, _ptr(off), q, int(k), flags,
                     int(max_len), _ptr(ln), _ptr(lb), _ptr(ub)))
    return ln, lb, ub


def occurrences(SA, lb, ub, limit=0, offsets=None, ctx=None):
    """(start, pos) -- or (start, pos, sid) with offsets -- of the intervals [lb[j], ub[j]) of locate(): the occurrences of
    pattern j are pos[start[j]:start[j + 1]] = SA[lb[j]:ub[j]], in SA order, at most limit of them where limit > 0; sid names
    the string of the set holding each.  Host arrays, staged for the call; the lists are made on the GPU (psacx_occurrences_dev_*)."""
    sa = np.ascontiguousarray(SA)
    if sa.dtype not in (np.uint32, np.uint64):
        raise TypeError("occurrences needs a uint32 or uint64 suffix array")
    bits = sa.dtype.itemsize * 8
    lo, hi = np.ascontiguousarray(lb, dtype=sa.dtype), np.ascontiguousarray(ub, dtype=sa.dtype)
    if lo.size != hi.size:
        raise ValueError("lb and ub differ in length")
    q, n = int(lo.size), int(sa.size)
    so = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    m = 0 if so is None else int(so.size - 1)
    ctx = ctx if ctx is not None else Context(0)
    start = np.zeros(q + 1, np.uint64)
    held = []

    def put(arr):
        p = ctx.alloc(max(1, arr.nbytes))
        held.append(p)
        if arr.nbytes:
            ctx.h2d(p, arr)
        return p
    try:
        d_sa, d_lb, d_ub, d_start = put(sa), put(lo), put(hi), put(start)
        d_off = None if so is None else put(so)
        total = occurrences_device(ctx, d_sa, n, d_off, m, d_lb, d_ub, q, limit, d_start, None, None, 0, bits)
        pos, sid = np.zeros(total, sa.dtype), np.zeros(total, sa.dtype)
        d_pos, d_sid = put(pos), (None if so is None else put(sid))
        occurrences_device(ctx, d_sa, n, d_off, m, d_lb, d_ub, q, limit, d_start, d_pos, d_sid, total, bits)
        ctx.d2h(start, d_start)
        if total:
            ctx.d2h(pos, d_pos)
            if so is not None:
                ctx.d2h(sid, d_sid)
    finally:
        for p in held:
            ctx.free(p)
    return (start, pos) if so is None else (start, pos, sid)


def rmq_index_device(ctx, d_values, n, d_index, index_bits):
    """psacx_rmq_index_dev_*: the range-minimum index of n values resident in HBM (include/psacx.h: "range minimum and longest
    common extension").  d_index=None is the size query.  Returns the number of index entries (of the index type)."""
    fn = getattr(ctx._lib, "psacx_rmq_index_dev_u%d" % index_bits)
    entries = C.c_uint64(0)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx.check(fn(ctx.handle, opt(d_values), int(n), opt(d_index), C.byref(entries)))
    return entries.value


def rmq_device(ctx, d_values, n, d_index, d_lo, d_hi, q, d_min, d_arg, index_bits):
    """psacx_rmq_dev_*: for each of q ranges [lo, min(hi, n)) the minimum and the smallest position that holds it; an empty range
    gives all ones and n.  d_min or d_arg may be None."""
    fn = getattr(ctx._lib, "psacx_rmq_dev_u%d" % index_bits)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx.check(fn(ctx.handle, opt(d_values), int(n), opt(d_index), opt(d_lo), opt(d_hi), int(q), opt(d_min), opt(d_arg)))


def lce_device(ctx, n, d_off, m, d_isa, d_lcp, d_index, d_a, d_b, q, max_mismatch, d_len, index_bits):
    """psacx_lce_dev_*: the longest common extension of q pairs of text positions with up to max_mismatch mismatches, from ISA, LCP
    and the range-minimum index of LCP, all resident in HBM.  d_off (with m): the m + 1 offsets of a string set, None for one text."""
    fn = getattr(ctx._lib, "psacx_lce_dev_u%d" % index_bits)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx.check(fn(ctx.handle, int(n), opt(d_off), int(m), opt(d_isa), opt(d_lcp), opt(d_index), opt(d_a), opt(d_b), int(q), int(max_mismatch),
                 opt(d_len)))


def rmq(values, lo, hi, ctx=None):
    """psacx_rmq_*: (min, arg) arrays -- the minimum of values[lo[j]:hi[j]] and the first position holding it; an empty range
    gives all ones and len(values).  Host arrays; everything is staged for the call."""
    v = np.ascontiguousarray(values)
    if v.dtype not in (np.uint32, np.uint64):
        raise TypeError("rmq needs uint32 or uint64 values")
    l, h = np.ascontiguousarray(lo, dtype=v.dtype), np.ascontiguousarray(hi, dtype=v.dtype)
    if l.size != h.size:
        raise ValueError("lo and hi differ in length")
    mn, arg = np.zeros(l.size, v.dtype), np.zeros(l.size, v.dtype)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_rmq_u%d" % (v.dtype.itemsize * 8))
    ctx.check(fn(ctx.handle, _ptr(v), v.size, _ptr(l), _ptr(h), l.size, _ptr(mn), _ptr(arg)))
    return mn, arg


def lce(ISA, LCP, a, b, max_mismatch=0, offsets=None, ctx=None):
    """psacx_lce_*: how far the text positions a[j] and b[j] agree when up to max_mismatch differing characters are stepped over,
    from the inverse suffix array and the LCP array alone.  offsets: the arrays are those of a string set (construct_gsa) and an
    extension ends where either string does.  Host arrays; everything is staged for the call."""
    isa, lcp = np.ascontiguousarray(ISA), np.ascontiguousarray(LCP)
    if isa.dtype not in (np.uint32, np.uint64) or lcp.dtype != isa.dtype or lcp.size != isa.size:
        raise TypeError("lce needs ISA and LCP of one length, both uint32 or both uint64")
    pa, pb = np.ascontiguousarray(a, dtype=isa.dtype), np.ascontiguousarray(b, dtype=isa.dtype)
    if pa.size != pb.size:
        raise ValueError("a and b differ in length")
    out = np.zeros(pa.size, isa.dtype)
    so = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_lce_u%d" % (isa.dtype.itemsize * 8))
    ctx.check(fn(ctx.handle, isa.size, _ptr(so) if so is not None else None, 0 if so is None else so.size - 1, _ptr(isa), _ptr(lcp), _ptr(pa),
                 _ptr(pb), pa.size, int(max_mismatch), _ptr(out)))
    return out


def overlaps_device(ctx, n, d_off, m, d_ends, d_sa, d_isa, d_lcp, d_index, min_len, flags, d_lb, d_ub, index_bits):
    """psacx_overlaps_dev_*: the suffix-prefix overlaps of a string set resident in HBM (include/psacx.h: "suffix-prefix overlaps").
    d_ends is the bitmap of string_ends_device, d_index the index of rmq_index_device over d_lcp; flags is 0 or OVERLAP_WHOLE.
    d_lb / d_ub receive n entries of the index type each: slot o_j + d - 1 holds the interval of the suffixes that are the first d
    bytes of string j, or 0, 0.  occurrences_device takes the two as they are, with q = n."""
    fn = getattr(ctx._lib, "psacx_overlaps_dev_u%d" % index_bits)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx.check(fn(ctx.handle, int(n), opt(d_off), int(m), opt(d_ends), opt(d_sa), opt(d_isa), opt(d_lcp), opt(d_index), int(min_len), int(flags),
                 opt(d_lb), opt(d_ub)))


def overlaps(text_len_or_text, offsets, SA, ISA, LCP, min_len, whole=False, ctx=None):
    """psacx_overlaps_*: (lb, ub) arrays of n entries -- for string j and a length d in [min_len, L_j - 1] (whole=True: up to L_j)
    the suffixes that are exactly the first d bytes of string j are SA[lb[p]:ub[p]] with p = offsets[j] + d - 1; every other slot
    holds 0, 0.  Borders of string j and whole strings that are its prefixes are among them.  From the arrays of a string set
    (construct_ss with lcp) alone: the first argument only gives n, as a number or as anything with a length.  Host arrays;
    everything is staged for the call.  occurrences(SA, lb, ub, offsets=offsets) lists positions and source strings."""
    n = int(text_len_or_text) if isinstance(text_len_or_text, (int, np.integer)) else len(text_len_or_text)
    sa, isa, lcp = np.ascontiguousarray(SA), np.ascontiguousarray(ISA), np.ascontiguousarray(LCP)
    if sa.dtype not in (np.uint32, np.uint64) or isa.dtype != sa.dtype or lcp.dtype != sa.dtype:
        raise TypeError("overlaps needs SA, ISA and LCP all uint32 or all uint64")
    if sa.size != n or isa.size != n or lcp.size != n:
        raise ValueError("SA, ISA and LCP must have n entries each")
    so = np.ascontiguousarray(offsets, dtype=np.uint64)
    lb, ub = np.zeros(n, sa.dtype), np.zeros(n, sa.dtype)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_overlaps_u%d" % (sa.dtype.itemsize * 8))
    ctx.check(fn(ctx.handle, n, _ptr(so), max(0, so.size - 1), _ptr(sa), _ptr(isa), _ptr(lcp), int(min_len), OVERLAP_WHOLE if whole else 0,
                 _ptr(lb), _ptr(ub)))
    return lb, ub


def lpf_device(ctx, n, d_sa, d_lcp, d_index, d_lpf, d_src, index_bits):
    """psacx_lpf_dev_*: the longest previous factor of every position and a source for each, from SA, LCP and the index of
    rmq_index_device over d_lcp, all resident in HBM (include/psacx.h: "LZ77 factorization").  d_lpf / d_src receive n entries of the
    index type each: src < i and 1 <= lpf <= n - i, or 0 and all ones."""
    fn = getattr(ctx._lib, "psacx_lpf_dev_u%d" % index_bits)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx.check(fn(ctx.handle, int(n), opt(d_sa), opt(d_lcp), opt(d_index), opt(d_lpf), opt(d_src)))


def lz77_device(ctx, n, d_lpf, d_src, d_start, d_psrc, cap, index_bits):
    """psacx_lz77_dev_*: the greedy parse cut from an LPF array in HBM.  d_start receives z + 1 entries (start[z] = n), d_psrc z
    entries (all ones for a literal); d_start=None is the count query; d_src=None parses any n values without sources.  Returns z;
    raises PsacxError -2 where z + 1 exceeds cap, with the lists untouched and z in the error's attribute z."""
    fn = getattr(ctx._lib, "psacx_lz77_dev_u%d" % index_bits)
    z = C.c_uint64(0)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    try:
        ctx.check(fn(ctx.handle, int(n), opt(d_lpf), opt(d_src), opt(d_start), opt(d_psrc), int(cap), C.byref(z)))
    except PsacxError as e:
        e.z = z.value
        raise
    return z.value


def check_lz77_device(ctx, d_text, n, d_start, d_psrc, z, index_bits):
    """psacx_check_lz77_dev_*: the number of violations of "start / psrc decode to the text"; 0 means the parse round-trips.  It does
    not prove the parse greedy."""
    fn = getattr(ctx._lib, "psacx_check_lz77_dev_u%d" % index_bits)
    errors = C.c_uint64(0)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx.check(fn(ctx.handle, opt(d_text), int(n), opt(d_start), opt(d_psrc), int(z), C.byref(errors)))
    return errors.value


def _sa_lcp(SA, LCP, what):
    sa, lcp = np.ascontiguousarray(SA), np.ascontiguousarray(LCP)
    if sa.dtype not in (np.uint32, np.uint64) or lcp.dtype != sa.dtype:
        raise TypeError(what + " needs SA and LCP both uint32 or both uint64")
    if sa.size != lcp.size:
        raise ValueError("SA and LCP must have n entries each")
    return sa, lcp


def lpf(SA, LCP, ctx=None):
    """psacx_lpf_*: (lpf, src) of the text whose suffix array and LCP array these are -- lpf[i] the length of the longest factor at i
    that also starts before i, src[i] where (all ones where lpf[i] is 0).  Host arrays; everything is staged for the call."""
    sa, lcp = _sa_lcp(SA, LCP, "lpf")
    out, src = np.zeros(sa.size, sa.dtype), np.zeros(sa.size, sa.dtype)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_lpf_u%d" % (sa.dtype.itemsize * 8))
    ctx.check(fn(ctx.handle, sa.size, _ptr(sa), _ptr(lcp), _ptr(out), _ptr(src)))
    return out, src


def lz77(SA, LCP, ctx=None):
    """psacx_lz77_*: (start, src) of the greedy LZ77 parse -- phrase k is text[start[k]:start[k + 1]], a copy from src[k], or one
    literal byte where src[k] is all ones; start has z + 1 entries and ends with n.  A copy may overlap its phrase."""
    sa, lcp = _sa_lcp(SA, LCP, "lz77")
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_lz77_u%d" % (sa.dtype.itemsize * 8))
    z = C.c_uint64(0)
    ctx._pre()
    ctx.check(fn(ctx.handle, sa.size, _ptr(sa), _ptr(lcp), None, None, 0, C.byref(z)))
    start, src = np.zeros(z.value + 1, sa.dtype), np.zeros(z.value, sa.dtype)
    ctx.check(fn(ctx.handle, sa.size, _ptr(sa), _ptr(lcp), _ptr(start), _ptr(src) if z.value else _ptr(start), z.value + 1, C.byref(z)))
    return start, src


def lz77_decode(start, src, text):
    """The text a parse stands for, as bytes: copies are made byte by byte (a source may overlap its phrase), and `text` is read at
    the literal phrases only."""
    st = np.asarray(start)
    ones = int(np.iinfo(np.asarray(src).dtype).max)
    out = bytearray()
    for k in range(st.size - 1):
        a, b, s = int(st[k]), int(st[k + 1]), int(src[k])
        if s == ones:
            out.append(int(text[a]) if not isinstance(text, str) else ord(text[a]))
        else:
            for t in range(b - a):
                out.append(out[s + t])
    return bytes(out)


REPEATS_KINDS = {"right": _lib.PSACX_REPEATS_RIGHT, "maximal": _lib.PSACX_REPEATS_MAXIMAL, "super": _lib.PSACX_REPEATS_SUPERMAXIMAL,
                 "supermaximal": _lib.PSACX_REPEATS_SUPERMAXIMAL}


def bwt_device(ctx, d_text, n, d_ends, d_sa, d_bwt, d_first, index_bits, want_primary=True):
    """psacx_bwt_dev_*: the Burrows-Wheeler transform aligned with SA, bwt[r] = text[SA[r] - 1], cyclic per string (include/psacx.h:
    "BWT and repeats").  d_ends is the bitmap of string_ends_device, or None for one text.  d_bwt receives n bytes, d_first the
    bitmap ((n >> 5) + 1 words of 32) of the ranks that start a string; either may be None.  Returns the rank of position 0 (all ones
    of 64 bits where no SA entry is 0), or None with want_primary=False."""
    fn = getattr(ctx._lib, "psacx_bwt_dev_u%d" % index_bits)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    primary = C.c_uint64(0)
    ctx.check(fn(ctx.handle, opt(d_text), int(n), opt(d_ends), opt(d_sa), opt(d_bwt), opt(d_first), C.byref(primary) if want_primary else None))
    return primary.value if want_primary else None


def repeats_device(ctx, n, d_lcp, d_index, d_bwt, d_first, kind, min_len, min_occ, max_occ, d_lb, d_ub, d_len, cap, index_bits):
    """psacx_repeats_dev_*: the repeats of one kind (0 right-maximal, 1 maximal, 2 supermaximal) as LCP-intervals, from LCP, the index
    of rmq_index_device over it, and the two outputs of bwt_device (not read by kind 0).  d_lb / d_ub / d_len receive z entries each in
    the order of the interval heads; d_lb=None is the count query; d_len may be None.  Returns z; raises PsacxError -2 where z exceeds
    cap, with the lists untouched and z in the error's attribute z.  occurrences_device takes d_lb and d_ub as they are."""
    fn = getattr(ctx._lib, "psacx_repeats_dev_u%d" % index_bits)
    z = C.c_uint64(0)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    try:
        ctx.check(fn(ctx.handle, int(n), opt(d_lcp), opt(d_index), opt(d_bwt), opt(d_first), int(kind), int(min_len), int(min_occ), int(max_occ),
                     opt(d_lb), opt(d_ub), opt(d_len), int(cap), C.byref(z)))
    except PsacxError as e:
        e.z = z.value
        raise
    return z.value


def _text_bytes(text):
    if isinstance(text, str):
        text = text.encode("latin-1")
    return np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8)


def bwt(text, SA, offsets=None, ctx=None):
    """psacx_bwt_*: (bwt, primary) -- bwt[r] = text[SA[r] - 1] as uint8, aligned with SA; where SA[r] starts a string (with
    offsets=None: where it is 0) the last byte of that string.  primary is the rank of position 0.  This is not libdivsufsort's divbwt
    layout.  Host arrays; everything is staged for the call."""
    t, sa = _text_bytes(text), np.ascontiguousarray(SA)
    if sa.dtype not in (np.uint32, np.uint64):
        raise TypeError("bwt needs SA as uint32 or uint64")
    if sa.size != t.size:
        raise ValueError("SA must have one entry per byte of the text")
    so = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    out = np.zeros(t.size, np.uint8)
    primary = C.c_uint64(0)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_bwt_u%d" % (sa.dtype.itemsize * 8))
    ctx.check(fn(ctx.handle, _ptr(t), t.size, _ptr(so) if so is not None else None, 0 if so is None else so.size - 1, _ptr(sa), _ptr(out),
                 C.byref(primary)))
    return out, primary.value


def bwt_decode(bwt, primary):
    """The text of an SA-aligned BWT of one text, as bytes: the row of the end marker goes back in at primary + 1, then one LF walk.
    Host only."""
    b = np.asarray(bwt, np.uint8)
    n = int(b.size)
    if n == 0:
        return b""
    if not 0 <= int(primary) < n:
        raise ValueError("primary must be a rank of the text")
    col = np.concatenate(([int(b[primary]) + 1], b.astype(np.int64) + 1))
    col[int(primary) + 1] = 0
    lf = np.empty(n + 1, np.int64)
    lf[np.argsort(col, kind="stable")] = np.arange(n + 1)
    out = np.empty(n, np.uint8)
    r = 0
    for k in range(n - 1, -1, -1):
        out[k] = col[r] - 1
        r = lf[r]
    return out.tobytes()


def repeats(text, SA, LCP, kind="maximal", min_len=1, min_occ=2, max_occ=0, offsets=None, ctx=None):
    """psacx_repeats_*: (lb, ub, length) of the repeats of one kind ("right", "maximal", "super"): repeat k is
    text[SA[lb[k]]:SA[lb[k]] + length[k]] and occurs exactly at SA[lb[k]:ub[k]].  Filters: length >= min_len, min_occ <= occurrences,
    and occurrences <= max_occ where max_occ > 0.  With offsets the text is a string set, whose string ends and starts differ from
    every character.  occurrences(SA, lb, ub, offsets=offsets) lists positions and strings.  Host arrays; everything is staged."""
    k = REPEATS_KINDS[kind] if isinstance(kind, str) else int(kind)
    sa, lcp = _sa_lcp(SA, LCP, "repeats")
    t = _text_bytes(text)
    if t.size != sa.size:
        raise ValueError("SA and LCP must have one entry per byte of the text")
    so = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_repeats_u%d" % (sa.dtype.itemsize * 8))
    z = C.c_uint64(0)
    head = [ctx.handle, _ptr(t), t.size, _ptr(so) if so is not None else None, 0 if so is None else so.size - 1, _ptr(sa), _ptr(lcp), k,
            int(min_len), int(min_occ), int(max_occ)]
    ctx.check(fn(*(head + [None, None, None, 0, C.byref(z)])))
    lb, ub, ln = (np.zeros(max(1, z.value), sa.dtype) for _ in range(3))
    ctx.check(fn(*(head + [_ptr(lb), _ptr(ub), _ptr(ln), z.value, C.byref(z)])))
    return lb[:z.value], ub[:z.value], ln[:z.value]


def doc_index_device(ctx, n, d_off, m, d_sa, d_lcp, d_index, d_prev, d_dup, index_bits):
    """psacx_doc_index_dev_*: the document index of a string set resident in HBM (include/psacx.h: "document counts and document
    lists"): d_prev receives n entries, d_dup n + 1; either may be None (d_lcp and d_index, the index of rmq_index_device over it, are
    read for d_dup alone)."""
    fn = getattr(ctx._lib, "psacx_doc_index_dev_u%d" % index_bits)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    ctx.check(fn(ctx.handle, int(n), opt(d_off), int(m), opt(d_sa), opt(d_lcp), opt(d_index), opt(d_prev), opt(d_dup)))


def doc_count_device(ctx, n, d_dup, d_lb, d_ub, q, d_docs, index_bits):
    """psacx_doc_count_dev_*: d_docs[j] = the number of distinct strings in the LCP-interval [lb_j, ub_j), from d_dup of
    doc_index_device; 0 unless lb_j < ub_j <= n."""
    fn = getattr(ctx._lib, "psacx_doc_count_dev_u%d" % index_bits)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    ctx.check(fn(ctx.handle, int(n), opt(d_dup), opt(d_lb), opt(d_ub), int(q), opt(d_docs)))


def doc_list_device(ctx, d_sa, n, d_off, m, d_prev, d_lb, d_ub, q, max_cand, d_start, d_sid, d_pos, cap, index_bits):
    """psacx_doc_list_dev_*: each string of the intervals [lb_j, ub_j) once, from d_prev of doc_index_device.  d_start receives q + 1
    uint64 (the exclusive prefix sums of the list lengths), d_sid the strings and d_pos (may be None) the positions of their first
    ranks, in rank order.  d_sid=None is the size query.  Returns the total; raises PsacxError -2 where it exceeds cap (d_start valid,
    lists untouched, the total in the error's attribute total) or where the intervals hold more than max_cand > 0 ranks."""
    fn = getattr(ctx._lib, "psacx_doc_list_dev_u%d" % index_bits)
    total = C.c_uint64(0)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    try:
        ctx.check(fn(ctx.handle, opt(d_sa), int(n), opt(d_off), int(m), opt(d_prev), opt(d_lb), opt(d_ub), int(q), int(max_cand), opt(d_start),
                     opt(d_sid), opt(d_pos), int(cap), C.byref(total)))
    except PsacxError as e:
        e.total = total.value
        raise
    return total.value


def _doc_args(SA, offsets, lb, ub, what):
    sa = np.ascontiguousarray(SA)
    if sa.dtype not in (np.uint32, np.uint64):
        raise TypeError("%s needs SA as uint32 or uint64" % what)
    so = np.ascontiguousarray(offsets, dtype=np.uint64)
    a, b = np.ascontiguousarray(lb, dtype=sa.dtype), np.ascontiguousarray(ub, dtype=sa.dtype)
    if a.shape != b.shape or a.ndim != 1:
        raise ValueError("lb and ub must be two flat arrays of one length")
    return sa, so, a, b


def doc_count(SA, LCP, offsets, lb, ub, ctx=None):
    """psacx_doc_count_*: the number of distinct strings of the set (offsets: its m + 1 string offsets) among the suffixes
    SA[lb[j]:ub[j]], for LCP-intervals: what locate / match / repeats / mems return, singletons and [0, n).  The intervals of overlaps()
    are none: use doc_list for them.  Host arrays; everything is staged for the call."""
    sa, so, a, b = _doc_args(SA, offsets, lb, ub, "doc_count")
    lcp = np.ascontiguousarray(LCP)
    if lcp.dtype != sa.dtype or lcp.size != sa.size:
        raise ValueError("SA and LCP must have the same type and length")
    out = np.zeros(a.size, sa.dtype)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_doc_count_u%d" % (sa.dtype.itemsize * 8))
    ctx._pre()
    ctx.check(fn(ctx.handle, sa.size, _ptr(so), so.size - 1, _ptr(sa), _ptr(lcp), _ptr(a), _ptr(b), a.size, _ptr(out)))
    return out


def doc_list(SA, offsets, lb, ub, max_cand=0, ctx=None):
    """psacx_doc_list_*: (start, sid, pos) -- the strings that own a suffix in SA[lb[j]:ub[j]] are sid[start[j]:start[j + 1]], each once,
    in the order of their first rank, and pos is where that suffix starts.  Any interval.  max_cand > 0 refuses (PsacxError -2) a batch
    whose intervals hold more ranks.  Host arrays; everything is staged for the call."""
    sa, so, a, b = _doc_args(SA, offsets, lb, ub, "doc_list")
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_doc_list_u%d" % (sa.dtype.itemsize * 8))
    start = np.zeros(a.size + 1, np.uint64)
    total = C.c_uint64(0)
    head = [ctx.handle, _ptr(sa), sa.size, _ptr(so), so.size - 1, _ptr(a), _ptr(b), a.size, int(max_cand), _ptr(start)]
    ctx._pre()
    ctx.check(fn(*(head + [None, None, 0, C.byref(total)])))
    sid, pos = (np.zeros(max(1, total.value), sa.dtype) for _ in range(2))
    ctx.check(fn(*(head + [_ptr(sid), _ptr(pos), total.value, C.byref(total)])))
    return start, sid[:total.value], pos[:total.value]


def fm_index_device(ctx, n, d_bwt, d_first, d_sa, sample, d_fm, index_bits):
    """psacx_fm_index_dev_*: the FM-index of the text or string set whose BWT and first bitmap bwt_device left at d_bwt / d_first
    (include/psacx.h: "FM-index"), into the 64-bit words at d_fm.  sample > 0 keeps SA[r] of every rank that starts a string or whose
    position is a multiple of sample (d_sa is read only then); sample == 0 builds an index that counts only.  d_fm=None is the size
    query.  Returns the descriptor (_lib.FmInfo: n, words, sample, marks, sigma, bits, code), which every query takes back."""
    fn = getattr(ctx._lib, "psacx_fm_index_dev_u%d" % index_bits)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    info = _lib.FmInfo()
    ctx._pre()
    ctx.check(fn(ctx.handle, int(n), opt(d_bwt), opt(d_first), opt(d_sa), int(sample), opt(d_fm), C.byref(info)))
    return info


def fm_count_device(ctx, d_fm, info, d_pat, d_poff, q, d_lb, d_ub, index_bits):
    """psacx_fm_count_dev_*: backward search of q patterns (d_pat / d_poff as locate_device takes them) over the index at d_fm.  d_lb /
    d_ub receive the interval of locate_device / locate_gsa_device for every pattern that occurs, and lb = ub = 0 (not locate's insertion
    point) for one that does not."""
    fn = getattr(ctx._lib, "psacx_fm_count_dev_u%d" % index_bits)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    ctx.check(fn(ctx.handle, opt(d_fm), C.byref(info), opt(d_pat), opt(d_poff), int(q), opt(d_lb), opt(d_ub)))


def fm_occurrences_device(ctx, d_fm, info, d_off, m, d_lb, d_ub, q, limit, d_start, d_pos, d_sid, cap, index_bits):
    """psacx_fm_occurrences_dev_*: occurrences_device without a suffix array: every position comes from the walk to a sampled rank of
    the index at d_fm (built with sample > 0; PsacxError -1 otherwise).  d_pos=None is the size query.  Returns the total; raises
    PsacxError -2 where it exceeds cap, with d_start valid, d_pos untouched and the total in the error's attribute total."""
    fn = getattr(ctx._lib, "psacx_fm_occurrences_dev_u%d" % index_bits)
    total = C.c_uint64(0)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    try:
        ctx.check(fn(ctx.handle, opt(d_fm), C.byref(info), opt(d_off), int(m), opt(d_lb), opt(d_ub), int(q), int(limit), opt(d_start), opt(d_pos),
                     opt(d_sid), int(cap), C.byref(total)))
    except PsacxError as e:
        e.total = total.value
        raise
    return total.value


def fm_text_samples_device(ctx, n, d_sa, d_off, m, rate, d_ts, index_bits):
    """psacx_fm_text_samples_dev_*: the text samples of an FM-index from the suffix array at d_sa: d_ts[k] = the rank of the suffix at
    position (k + 1) * rate - 1 for k < n // rate, and behind them the rank of the suffix at the last byte of every string (d_off: its
    m + 1 offsets; None for one text).  d_ts=None is the size query.  Returns the number of entries, n // rate + max(m, 1)."""
    fn = getattr(ctx._lib, "psacx_fm_text_samples_dev_u%d" % index_bits)
    entries = C.c_uint64(0)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    ctx.check(fn(ctx.handle, int(n), opt(d_sa), opt(d_off), int(m), int(rate), opt(d_ts), C.byref(entries)))
    return entries.value


def fm_extract_device(ctx, d_fm, info, d_ts, rate, d_off, m, d_pos, d_len, q, d_start, d_out, cap, index_bits):
    """psacx_fm_extract_dev_*: the bytes S[pos .. pos + len) of q queries, each clipped at the end of its string, from the index at
    d_fm and the text samples at d_ts (fm_text_samples_device, with the same rate, d_off and m).  d_start receives the q + 1 prefix
    sums of the clipped lengths, d_out the bytes; d_out=None is the size query.  Returns the total; raises PsacxError -2 where it
    exceeds cap, with d_start valid, d_out untouched and the total in the error's attribute total."""
    fn = getattr(ctx._lib, "psacx_fm_extract_dev_u%d" % index_bits)
    total = C.c_uint64(0)
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    try:
        ctx.check(fn(ctx.handle, opt(d_fm), C.byref(info), opt(d_ts), int(rate), opt(d_off), int(m), opt(d_pos), opt(d_len), int(q),
                     opt(d_start), opt(d_out), int(cap), C.byref(total)))
    except PsacxError as e:
        e.total = total.value
        raise
    return total.value


def fm_search(text, SA, patterns, sample=32, limit=0, offsets=None, positions=True, ctx=None):
    """psacx_fm_search_*: (lb, ub) of the patterns by backward search over an FM-index built for the call, and with positions=True
    (lb, ub, start, pos) -- or (lb, ub, start, pos, sid) with offsets -- where the occurrences of pattern j are pos[start[j]:start[j + 1]]
    = SA[lb[j]:ub[j]], at most limit of them where limit > 0.  A pattern that does not occur has lb = ub = 0.  Host arrays; everything is
    staged for the call, and with positions the call runs twice: once to size the lists, once to fill them."""
    t, sa = _text_bytes(text), np.ascontiguousarray(SA)
    if sa.dtype not in (np.uint32, np.uint64):
        raise TypeError("fm_search needs SA as uint32 or uint64")
    if sa.size != t.size:
        raise ValueError("SA must have one entry per byte of the text")
    so = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    pat, off = pattern_buffer(patterns)
    q = int(off.size - 1)
    lb, ub = np.zeros(q, sa.dtype), np.zeros(q, sa.dtype)
    ctx = ctx if ctx is not None else Context(0)
    fn = getattr(ctx._lib, "psacx_fm_search_u%d" % (sa.dtype.itemsize * 8))
    head = [ctx.handle, _ptr(t), t.size, _ptr(so) if so is not None else None, 0 if so is None else so.size - 1, _ptr(sa), int(sample),
            _ptr(pat) if pat.size else None, _ptr(off), q, _ptr(lb), _ptr(ub), int(limit)]
    ctx._pre()
    if not positions:
        ctx.check(fn(*(head + [None, None, None, 0, None])))
        return lb, ub
    start = np.zeros(q + 1, np.uint64)
    total = C.c_uint64(0)
    one = np.zeros(1, sa.dtype)
    rc = fn(*(head + [_ptr(start), _ptr(one), None, 0, C.byref(total)]))
    if rc != -2 or total.value == 0:
        ctx.check(rc)
    pos, sid = np.zeros(max(1, total.value), sa.dtype), np.zeros(max(1, total.value), sa.dtype)
    if total.value:
        ctx.check(fn(*(head + [_ptr(start), _ptr(pos), _ptr(sid) if so is not None else None, total.value, C.byref(total)])))
    pos, sid = pos[:total.value], sid[:total.value]
    return (lb, ub, start, pos) if so is None else (lb, ub, start, pos, sid)


class FMIndex(object):
    """An FM-index resident in HBM (SuffixArray.fm_index).  It owns the blob, its descriptor and, for a string set, the m + 1 string
    offsets that name the string of a position; it needs neither the text nor the suffix array it was built from.  Built with
    text_rate > 0 it owns the text samples too (nbytes counts them) and gives the bytes back: extract, text, context."""

    def __init__(self, ctx, d_fm, info, index_bits, d_off=None, m=0, d_ts=None, text_rate=0, text_entries=0, offsets=None):
        self.ctx, self.d_fm, self.info, self.index_bits, self.d_off, self.m = ctx, d_fm, info, index_bits, d_off, m
        self.dtype = np.uint32 if index_bits == 32 else np.uint64
        self.d_ts, self.text_rate, self.text_entries = d_ts, int(text_rate), int(text_entries)
        self.offsets = None if offsets is None else np.array(offsets, dtype=np.uint64)          # (host copy: text() names the strings by it)

    @property
    def nbytes(self):
        return int(self.info.words) * 8 + self.text_entries * (self.index_bits // 8)

    def _with(self, arrays, body):
        held = []
        try:
            for a in arrays:
                p = self.ctx.alloc(max(1, a.nbytes))
                held.append(p)
                if a.nbytes:
                    self.ctx.h2d(p, a)
            return body(*held)
        finally:
            for p in held:
                self.ctx.free(p)

    def count(self, patterns):
        """(lb, ub): pattern j occurs ub[j] - lb[j] times, at the ranks [lb[j], ub[j]) of the suffix array; lb = ub = 0 where it does not."""
        if self.d_fm is None:
            raise ValueError("the index has been freed")
        pat, off = pattern_buffer(patterns)
        q = int(off.size - 1)
        lb, ub = np.zeros(q, self.dtype), np.zeros(q, self.dtype)

        def body(d_pat, d_poff, d_lb, d_ub):
            fm_count_device(self.ctx, self.d_fm, self.info, d_pat, d_poff, q, d_lb, d_ub, self.index_bits)
            if q:
                self.ctx.d2h(lb, d_lb)
                self.ctx.d2h(ub, d_ub)
        self._with([pat, off, lb, ub], body)
        return lb, ub

    def locate(self, patterns, limit=0):
        """(start, pos) -- (start, pos, sid) for a string set -- the occurrences of pattern j are pos[start[j]:start[j + 1]], in the order
        of the suffix array, at most limit of them where limit > 0.  Needs an index built with sample > 0."""
        lb, ub = self.count(patterns)
        q = int(lb.size)
        start = np.zeros(q + 1, np.uint64)
        out = {}

        def body(d_lb, d_ub, d_start):
            args = (self.ctx, self.d_fm, self.info, self.d_off, self.m, d_lb, d_ub, q, limit, d_start)
            total = fm_occurrences_device(*(args + (None, None, 0, self.index_bits)))
            pos, sid = np.zeros(total, self.dtype), np.zeros(total, self.dtype)

            def lists(d_pos, d_sid):
                fm_occurrences_device(*(args + (d_pos, d_sid if self.d_off else None, total, self.index_bits)))
                self.ctx.d2h(start, d_start)
                if total:
                    self.ctx.d2h(pos, d_pos)
                    if self.d_off:
                        self.ctx.d2h(sid, d_sid)
            self._with([pos, sid], lists)
            out["pos"], out["sid"] = pos, sid
        self._with([lb, ub, start], body)
        return (start, out["pos"], out["sid"]) if self.d_off else (start, out["pos"])

    def extract(self, pos, length):
        """(start, bytes): query i is the bytes S[pos[i] .. pos[i] + length[i]) clipped at the end of the string that holds pos[i]
        (nothing for a pos at or beyond n); they are bytes[start[i]:start[i + 1]], a uint8 array.  length may be one number for all.
        Needs an index built with text_rate > 0."""
        if self.d_fm is None:
            raise ValueError("the index has been freed")
        if not self.d_ts:
            raise ValueError("the index has no text samples (build it with text_rate > 0)")
        p = np.ascontiguousarray(np.atleast_1d(pos), dtype=self.dtype)
        ln = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(length), p.shape), dtype=self.dtype)
        q = int(p.size)
        start = np.zeros(q + 1, np.uint64)
        got = {}

        def body(d_pos, d_len, d_start):
            args = (self.ctx, self.d_fm, self.info, self.d_ts, self.text_rate, self.d_off, self.m, d_pos, d_len, q, d_start)
            total = fm_extract_device(*(args + (None, 0, self.index_bits)))
            out = np.zeros(total, np.uint8)

            def fill(d_out):
                fm_extract_device(*(args + (d_out, total, self.index_bits)))
                self.ctx.d2h(start, d_start)
                if total:
                    self.ctx.d2h(out, d_out)
            self._with([out], fill)
            got["out"] = out
        self._with([p, ln, start], body)
        return start, got["out"]

    def text(self):
        """The whole text back from the index, as bytes; for a string set the list of its strings."""
        n = int(self.info.n)
        if self.offsets is None:
            return self.extract([0], [n])[1].tobytes()
        start, out = self.extract(self.offsets[:-1], np.diff(self.offsets))
        return [out[int(start[j]):int(start[j + 1])].tobytes() for j in range(self.m)]

    def context(self, patterns, width, limit=0):
        """locate(patterns, limit), then the window [pos - width, pos + len(pattern) + width) of every occurrence, clipped to its
        string: (start, pos, wstart, bytes) -- (start, pos, sid, wstart, bytes) for a string set -- where the window of occurrence o is
        bytes[wstart[o]:wstart[o + 1]]."""
        if not self.d_ts:
            raise ValueError("the index has no text samples (build it with text_rate > 0)")
        res = self.locate(patterns, limit)
        start, pos = res[0], res[1].astype(np.int64)
        lens = np.repeat(np.array([len(bytes(P)) for P in patterns], np.int64), np.diff(start.astype(np.int64)))
        lo = np.zeros(pos.size, np.int64)
        if self.offsets is not None and pos.size:
            lo = self.offsets.astype(np.int64)[res[2].astype(np.int64)]
        a = np.maximum(lo, pos - int(width))
        wstart, out = self.extract(a, pos + lens + int(width) - a)
        return tuple(res) + (wstart, out)

    def free(self):
        for name in ("d_fm", "d_off", "d_ts"):
            p = getattr(self, name, None)
            if p and getattr(self.ctx, "handle", None):
                self.ctx.free(p)
            setattr(self, name, None)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def fm_index(text, SA, sample=32, offsets=None, ctx=None, text_rate=0):
    """The FMIndex of a text (or, with offsets, a string set) and its suffix array: text and SA are staged, the bitmap of the string
    ends, the BWT and the index are built in HBM, and everything but the index is freed again.  text_rate > 0 builds the text samples
    beside it (one rank per text_rate positions and one per string), which extract / text / context need."""
    t, sa = _text_bytes(text), np.ascontiguousarray(SA)
    if sa.dtype not in (np.uint32, np.uint64):
        raise TypeError("fm_index needs SA as uint32 or uint64")
    if sa.size != t.size:
        raise ValueError("SA must have one entry per byte of the text")
    bits, n = sa.dtype.itemsize * 8, int(t.size)
    so = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    m = 0 if so is None else int(so.size - 1)
    ctx = ctx if ctx is not None else Context(0)
    held, keep = [], {}

    def put(arr=None, nbytes=0):
        p = ctx.alloc(max(1, arr.nbytes if arr is not None else nbytes))
        held.append(p)
        if arr is not None and arr.nbytes:
            ctx.h2d(p, arr)
        return p
    try:
        d_text, d_sa = put(t), put(sa)
        d_bwt, d_first = put(nbytes=n), put(nbytes=4 * ((n >> 5) + 1))
        d_ends = None
        if so is not None:
            d_off = put(so)
            d_ends = put(nbytes=4 * ((n >> 5) + 1))
            string_ends_device(ctx, d_off, m, n, d_ends)
            held.remove(d_off)
            keep["off"] = d_off
        bwt_device(ctx, d_text, n, d_ends, d_sa, d_bwt, d_first, bits, want_primary=False)
        info = fm_index_device(ctx, n, d_bwt, d_first, d_sa if sample else None, sample, None, bits)
        keep["fm"] = ctx.alloc(max(8, int(info.words) * 8))
        info = fm_index_device(ctx, n, d_bwt, d_first, d_sa if sample else None, sample, keep["fm"], bits)
        entries = 0
        if text_rate:
            entries = fm_text_samples_device(ctx, n, None, keep.get("off"), m, text_rate, None, bits)
            keep["ts"] = ctx.alloc(max(8, entries * (bits // 8)))
            fm_text_samples_device(ctx, n, d_sa, keep.get("off"), m, text_rate, keep["ts"], bits)
    except Exception:
        for p in keep.values():
            ctx.free(p)
        raise
    finally:
        for p in held:
            ctx.free(p)
    return FMIndex(ctx, keep["fm"], info, bits, keep.get("off"), m, keep.get("ts"), text_rate, entries, so)


MEMS_SUPER = _lib.PSACX_MEMS_SUPER


def mems_device(ctx, n, d_sa, d_lcp, d_index, d_bwt, d_first, d_pat, d_poff, q, d_mlen, d_mlb, d_mub, min_len, max_occ, flags, d_qpos, d_tpos,
                d_len, cap, index_bits, work=None):
    """psacx_mems_dev_*: the maximal exact matches of q patterns against the index resident in HBM (include/psacx.h: "maximal exact
    matches"), from SA, LCP, the index of rmq_index_device over it, the two outputs of bwt_device and the three outputs of
    match_device / match_gsa_device with MATCH_SUFFIXES and max_len = 0.  flags is 0 or MEMS_SUPER.  d_qpos (uint64) / d_tpos / d_len
    receive z entries each in the pinned order; d_qpos=None is the count query.  work, where given, is a list that receives the two
    work counters.  Returns z; raises PsacxError -2 where z exceeds cap, with the lists untouched and z in the error's attribute z."""
    fn = getattr(ctx._lib, "psacx_mems_dev_u%d" % index_bits)
    z = C.c_uint64(0)
    w = (C.c_uint64 * 2)()
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    try:
        ctx.check(fn(ctx.handle, int(n), opt(d_sa), opt(d_lcp), opt(d_index), opt(d_bwt), opt(d_first), opt(d_pat), opt(d_poff), int(q), opt(d_mlen),
                     opt(d_mlb), opt(d_mub), int(min_len), int(max_occ), int(flags), opt(d_qpos), opt(d_tpos), opt(d_len), int(cap), C.byref(z),
                     w if work is not None else None))
    except PsacxError as e:
        e.z = z.value
        raise
    finally:
        if work is not None:
            work[:] = [int(w[0]), int(w[1])]
    return z.value


def mems(text, SA, LCP, patterns, min_len, k=0, offsets=None, max_occ=0, super=False, ctx=None):
    """psacx_mems_*: (qpos, tpos, len) of the maximal exact matches of the patterns against the text: MEM i is
    pat[qpos[i]:qpos[i] + len[i]] == text[tpos[i]:tpos[i] + len[i]] with len[i] >= min_len, extensible on neither side inside its
    pattern and its string; qpos counts bytes of the pattern buffer (pattern_buffer(patterns)).  max_occ > 0 keeps matches whose
    bytes occur at most that often (1: unique in the text); super=True keeps those contained in no other match of their pattern
    (SMEMs).  Order: ascending qpos, then descending len, then suffix-array rank.  k > 0 puts the k-mer lookup table in front of
    the matching statistics.  offsets: text is a string set and SA / LCP its generalized arrays.  Host arrays; everything is staged."""
    sa, lcp = _sa_lcp(SA, LCP, "mems")
    t = _text_bytes(text)
    if t.size != sa.size:
        raise ValueError("SA and LCP must have one entry per byte of the text")
    pat, off = pattern_buffer(patterns)
    so = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    ctx = ctx if ctx is not None else Context(0)
    ctx._pre()
    fn = getattr(ctx._lib, "psacx_mems_u%d" % (sa.dtype.itemsize * 8))
    z = C.c_uint64(0)
    head = [ctx.handle, _ptr(t), t.size, _ptr(so) if so is not None else None, 0 if so is None else so.size - 1, _ptr(sa), _ptr(lcp),
            _ptr(pat) if pat.size else None, _ptr(off), int(off.size - 1), int(k), int(min_len), int(max_occ), MEMS_SUPER if super else 0]
    ctx.check(fn(*(head + [None, None, None, 0, C.byref(z)])))
    qpos = np.zeros(max(1, z.value), np.uint64)
    tpos, ln = (np.zeros(max(1, z.value), sa.dtype) for _ in range(2))
    ctx.check(fn(*(head + [_ptr(qpos), _ptr(tpos), _ptr(ln), z.value, C.byref(z)])))
    return qpos[:z.value], tpos[:z.value], ln[:z.value]


def kmismatch_device(ctx, d_text, n, d_ends, d_sa, d_table, k, code, d_pat, d_poff, q, e, max_cand, d_qid, d_tpos, d_dist, cap, index_bits,
                     work=None):
    """psacx_kmismatch_dev_*: the occurrences of q patterns with at most e substituted bytes (include/psacx.h: "pattern search with
    mismatches"), everything resident in HBM.  d_ends=None: one text; otherwise the bitmap of string_ends_device.  d_table / k / code
    as for locate_device (over a set: the table of lookup_table_gsa_device).  d_qid (uint64) / d_tpos (index type) / d_dist (uint8)
    receive z entries each in the pinned order; d_qid=None is the count query.  max_cand > 0 refuses a batch with more candidates.
    work, where given, is a list that receives the two work counters.  Returns z; raises PsacxError -2 where z exceeds cap or the
    candidates max_cand, with the lists untouched and z in the error's attribute z."""
    fn = getattr(ctx._lib, "psacx_kmismatch_dev_u%d" % index_bits)
    cd = None if code is None else np.ascontiguousarray(code, dtype=np.uint16)
    z = C.c_uint64(0)
    w = (C.c_uint64 * 2)()
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    try:
        ctx.check(fn(ctx.handle, opt(d_text), int(n), opt(d_ends), opt(d_sa), opt(d_table), int(k), _ptr(cd) if cd is not None else None, opt(d_pat),
                     opt(d_poff), int(q), int(e), int(max_cand), opt(d_qid), opt(d_tpos), opt(d_dist), int(cap), C.byref(z),
                     w if work is not None else None))
    except PsacxError as err:
        err.z = z.value
        raise
    finally:
        if work is not None:
            work[:] = [int(w[0]), int(w[1])]
    return z.value


def kmismatch(text, SA, patterns, e, k=0, offsets=None, max_cand=0, ctx=None):
    """psacx_kmismatch_*: (qid, tpos, dist) of the occurrences of the patterns in the text with at most e substituted bytes: hit i is
    pattern qid[i] at text[tpos[i]:tpos[i] + len(pattern)], inside one string, with dist[i] <= e differing bytes.  Patterns shorter
    than e + 1 bytes have no hits.  Order: ascending pattern, then the first piece of the pattern that occurs exactly there, then
    suffix-array rank.  k > 0 puts the k-mer lookup table in front of the piece searches; max_cand > 0 refuses (PsacxError -2) a
    batch whose pieces occur more often than that in all.  offsets: text is a string set and SA its generalized suffix array.  Host
    arrays; everything is staged."""
    sa = np.ascontiguousarray(SA)
    if sa.dtype not in (np.uint32, np.uint64):
        raise ValueError("kmismatch: SA must be uint32 or uint64")
    t = _text_bytes(text)
    if t.size != sa.size:
        raise ValueError("SA must have one entry per byte of the text")
    pat, off = pattern_buffer(patterns)
    so = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    ctx = ctx if ctx is not None else Context(0)
    ctx._pre()
    fn = getattr(ctx._lib, "psacx_kmismatch_u%d" % (sa.dtype.itemsize * 8))
    z = C.c_uint64(0)
    head = [ctx.handle, _ptr(t), t.size, _ptr(so) if so is not None else None, 0 if so is None else so.size - 1, _ptr(sa),
            _ptr(pat) if pat.size else None, _ptr(off), int(off.size - 1), int(k), int(e), int(max_cand)]
    ctx.check(fn(*(head + [None, None, None, 0, C.byref(z)])))
    qid = np.zeros(max(1, z.value), np.uint64)
    tpos = np.zeros(max(1, z.value), sa.dtype)
    dist = np.zeros(max(1, z.value), np.uint8)
    ctx.check(fn(*(head + [_ptr(qid), _ptr(tpos), _ptr(dist), z.value, C.byref(z)])))
    return qid[:z.value], tpos[:z.value], dist[:z.value]


KEDIT_BEST = 1


def kedit_device(ctx, d_text, n, d_ends, d_sa, d_table, k, code, d_pat, d_poff, q, e, max_cand, flags, d_qid, d_tpos, d_len, d_dist, cap,
                 index_bits, work=None):
    """psacx_kedit_dev_*: where q patterns occur within edit distance e (include/psacx.h: "pattern search with edits"), everything
    resident in HBM.  The arguments of kmismatch_device, and flags (KEDIT_BEST: only the hits of the smallest distance of every
    pattern) and d_len (index type) beside d_qid (uint64) / d_tpos (index type) / d_dist (uint8), which receive z entries each in
    ascending (pattern, position); d_qid=None is the count query.  work, where given, is a list that receives the candidates and
    the raw hits.  Returns z; raises PsacxError -2 where z exceeds cap or the candidates max_cand, with the lists untouched and z in
    the error's attribute z."""
    fn = getattr(ctx._lib, "psacx_kedit_dev_u%d" % index_bits)
    cd = None if code is None else np.ascontiguousarray(code, dtype=np.uint16)
    z = C.c_uint64(0)
    w = (C.c_uint64 * 2)()
    opt = lambda p: C.c_void_p(p) if p else None  # noqa: E731
    ctx._pre()
    try:
        ctx.check(fn(ctx.handle, opt(d_text), int(n), opt(d_ends), opt(d_sa), opt(d_table), int(k), _ptr(cd) if cd is not None else None, opt(d_pat),
                     opt(d_poff), int(q), int(e), int(max_cand), int(flags), opt(d_qid), opt(d_tpos), opt(d_len), opt(d_dist), int(cap), C.byref(z),
                     w if work is not None else None))
    except PsacxError as err:
        err.z = z.value
        raise
    finally:
        if work is not None:
            work[:] = [int(w[0]), int(w[1])]
    return z.value


def kedit(text, SA, patterns, e, k=0, offsets=None, max_cand=0, best=False, ctx=None):
    """psacx_kedit_*: (qid, tpos, len, dist) of the places where the patterns occur in the text within edit distance e: hit i is
    pattern qid[i] against text[tpos[i]:tpos[i] + len[i]], inside one string, at unit-cost Levenshtein distance dist[i] <= e, the
    smallest over all lengths from that start, and len[i] the shortest length that attains it.  Patterns of at most e bytes have no
    hits.  Order: ascending pattern, then ascending position.  best: only the hits of the smallest distance of every pattern.  k,
    max_cand, offsets as for kmismatch.  Host arrays; everything is staged."""
    sa = np.ascontiguousarray(SA)
    if sa.dtype not in (np.uint32, np.uint64):
        raise ValueError("kedit: SA must be uint32 or uint64")
    t = _text_bytes(text)
    if t.size != sa.size:
        raise ValueError("SA must have one entry per byte of the text")
    pat, off = pattern_buffer(patterns)
    so = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    ctx = ctx if ctx is not None else Context(0)
    ctx._pre()
    fn = getattr(ctx._lib, "psacx_kedit_u%d" % (sa.dtype.itemsize * 8))
    z = C.c_uint64(0)
    head = [ctx.handle, _ptr(t), t.size, _ptr(so) if so is not None else None, 0 if so is None else so.size - 1, _ptr(sa),
            _ptr(pat) if pat.size else None, _ptr(off), int(off.size - 1), int(k), int(e), int(max_cand), KEDIT_BEST if best else 0]
    ctx.check(fn(*(head + [None, None, None, None, 0, C.byref(z)])))
    qid = np.zeros(max(1, z.value), np.uint64)
    tpos, ln = (np.zeros(max(1, z.value), sa.dtype) for _ in range(2))
    dist = np.zeros(max(1, z.value), np.uint8)
    ctx.check(fn(*(head + [_ptr(qid), _ptr(tpos), _ptr(ln), _ptr(dist), z.value, C.byref(z)])))
    return qid[:z.value], tpos[:z.value], ln[:z.value], dist[:z.value]


def check_device(ctx, d_text, n, d_sa, d_isa, d_lcp, index_bits):
    """check_SA / check_lcp on buffers resident in HBM (check_suffix_array.hpp:56-126).  Returns the four
    error counters of psacx_check_dev_*; all zero means correct."""
    err = (C.c_uint64 * 4)()
    fn = getattr(ctx._lib, "psacx_check_dev_u%d" % index_bits)
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_sa), C.c_void_p(d_isa),
                 C.c_void_p(d_lcp) if d_lcp else None, err))
    return list(err)


def check_gsa_device(ctx, d_text, n, d_off, m, d_sa, d_isa, d_lcp, index_bits):
    """The same for a generalized suffix array resident in HBM (gl_check_gsa, src/gsac.cpp:85-135): d_off holds the
    m + 1 string offsets on the device, as psacx_construct_gsa_dev_* takes them.  Returns the four error counters of
    psacx_check_gsa_dev_*; all zero means correct, equal suffixes in text order included."""
    err = (C.c_uint64 * 4)()
    fn = getattr(ctx._lib, "psacx_check_gsa_dev_u%d" % index_bits)
    ctx.check(fn(ctx.handle, C.c_void_p(d_text), int(n), C.c_void_p(d_off), int(m), C.c_void_p(d_sa), C.c_void_p(d_isa),
                 C.c_void_p(d_lcp) if d_lcp else None, err))
    return list(err)


def ansv_device(ctx, d_in, n, d_left, d_right, index_bits, left_type=NEAREST_SM, right_type=NEAREST_SM, nonsv=0):
    """ansv<T, left_type, right_type> with the input (n index_t) and both results (n uint64 each) resident in
    HBM, e.g. over the LCP array construct_device left there (suffix_tree.hpp:62)."""
    fn = getattr(ctx._lib, "psacx_ansv_dev_u%d" % index_bits)
    ctx.check(fn(ctx.handle, C.c_void_p(d_in), int(n), int(left_type), int(right_type), int(nonsv),
                 C.c_void_p(d_left), C.c_void_p(d_right)))


def ansv(values, left_type=NEAREST_SM, right_type=NEAREST_SM, nonsv=0, ctx=None):
    """ansv<T,left_type,right_type>(in, left_nsv, right_nsv, comm) (ansv.hpp:2042-2051), one rank."""
    v = np.ascontiguousarray(values)
    if v.dtype not in (np.uint32, np.uint64):
        raise TypeError("ansv needs uint32 or uint64 input")
    ctx = ctx if ctx is not None else Context(0)
    left = np.empty(v.size, np.uint64)
    right = np.empty(v.size, np.uint64)
    fn = getattr(ctx._lib, "psacx_ansv_u%d" % (v.dtype.itemsize * 8))
    ctx.check(fn(ctx.handle, _ptr(v), v.size, int(left_type), int(right_type), int(nonsv), _ptr(left), _ptr(right)))
    return left, right
