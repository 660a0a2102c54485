// search.hpp -- kernels of the searches over a suffix array resident in HBM: the pattern search (psacx_locate_dev_*,
// psacx_locate_gsa_dev_*) and the longest-match search (psacx_match_dev_*, psacx_match_gsa_dev_*), over one text or over the
// generalized suffix array of a string set.  include/psacx.h defines lb(P), ub(P), len(Q), code() and key_k();
// tests/locate_model.py, tests/locate_gsa_model.py and tests/match_model.py state them on the host.
//
// Stands in for sa_index::locate (the reference's include/seq_query.hpp:246-251: two binary searches over SA with a string
// comparison per step), in the character-skipping form of bs_esa_index without its LCP arrays.
//
// A bisection step (search_step) is two dependent random fetches -- SA[mid], then the text at SA[mid] + offset -- so a search is
// bound by the number of requests a wave keeps in flight, not by bytes.  One pattern per lane (G = 1) keeps 64 independent
// searches in flight per wave; eight lanes per pattern (locate_kernel<T, 8>) compare 64 characters per step instead of 8 and
// keep 8 searches in flight.  DESIGN.md section 4.3 says which is the default and why.
//
// Over a string set (SET) suffix i is S[i..end(i)), and end(i) comes from the bitmap of the string ends (bit p = "a string starts
// at p, or p == n"; psacx_string_ends_dev).  A step stays two dependent fetches: once SA[mid] = s has arrived, the bitmap words
// that cover [s + from, s + from + 8] and the text word at s + from have addresses that are both known, so they are issued
// together and the text word is cut at the first set bit afterwards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occurrences.hpp"         // occ_last_le: the suffix mode finds the pattern that holds a buffer position as the lists do
#include "sa_kernels.hpp"

namespace psacx {

// up to 8 bytes at p as one big-endian word (the first byte on top, zeros below the last): words of two strings then compare as
// the strings do, bytes as unsigned values.  avail = bytes that exist at p; nothing beyond them is read.
__device__ __forceinline__ uint64_t locate_load_be(const uint8_t* __restrict__ p, uint64_t avail) {
    if (avail >= 8) {
        uint64_t w;
        __builtin_memcpy(&w, p, 8);                       // one unaligned 8-byte load
        return __builtin_bswap64(w);
    }
    uint64_t w = 0;
    for (unsigned j = 0; j < (unsigned)avail; ++j) w |= (uint64_t)p[j] << (56 - 8 * j);
    return w;
}

// the top cnt bytes of w (cnt <= 8)
__device__ __forceinline__ uint64_t locate_keep(uint64_t w, unsigned cnt) {
    return cnt >= 8 ? w : (cnt == 0 ? 0 : (w & ~(~0ull >> (8 * cnt))));
}

// the first 32 bytes of a pattern P[0..m) in registers: big-endian words, zero-padded.  (The compare functions select among them
// in place: as a function of its own the selection is laid out as branches, 35 to 60 instructions more per kernel.)
struct PatternWords { uint64_t p0, p1, p2, p3; };

__device__ __forceinline__ PatternWords pattern_words(const uint8_t* __restrict__ P, uint64_t m) {
    return {locate_load_be(P, m), m > 8 ? locate_load_be(P + 8, m - 8) : 0, m > 16 ? locate_load_be(P + 16, m - 16) : 0,
            m > 24 ? locate_load_be(P + 24, m - 24) : 0};
}

// Pattern P[0..m) against the suffix that starts at s, from character `from` on (the characters before it are taken as equal).
// An s >= n is the empty suffix.  h = characters the two share (at most m); returns -1: the suffix is smaller than P (a proper
// prefix of P included), 0: P is a prefix of the suffix, +1: the suffix is larger and P is no prefix of it.
// The comparison restarts at the 8-byte piece of P that holds `from`, so that the first 32 bytes of P come from registers (w);
// later pieces are read from the pattern buffer, never beyond m.  The text is never read at or beyond n.  fetches counts the
// text words read.
__device__ __forceinline__ int locate_compare(const uint8_t* __restrict__ text, uint64_t n, uint64_t s, const uint8_t* __restrict__ pat,
                                              uint64_t m, const PatternWords& w, uint64_t from, uint64_t& h, unsigned& fetches) {
    const uint64_t avail = s < n ? n - s : 0;
    const uint64_t end = m < avail ? m : avail;
    for (uint64_t h8 = from & ~(uint64_t)7; h8 < end; h8 += 8) {
        const unsigned cnt = end - h8 < 8 ? (unsigned)(end - h8) : 8u;
        const uint64_t tw = locate_keep(locate_load_be(text + s + h8, avail - h8), cnt);
        ++fetches;
        const uint64_t j = h8 >> 3;
        const uint64_t pw = locate_keep(j == 0 ? w.p0 : j == 1 ? w.p1 : j == 2 ? w.p2 : j == 3 ? w.p3 : locate_load_be(pat + h8, m - h8), cnt);
        if (tw != pw) { h = h8 + ((unsigned)__builtin_clzll(tw ^ pw) >> 3); return tw < pw ? -1 : 1; }
    }
    h = end;
    return end == m ? 0 : -1;
}

// The same by the G = 8 lanes that share a pattern: lane g compares piece g of a 64-character window, the first lane with a
// difference tells the others.  All lanes of a group hold the same arguments and receive the same answer.  fetches counts the
// text words this lane read: the lanes of a group add theirs up, so the count is per 8-byte load as in locate_compare.
__device__ __forceinline__ int locate_compare_group(const uint8_t* __restrict__ text, uint64_t n, uint64_t s, const uint8_t* __restrict__ pat,
                                                    uint64_t m, uint64_t from, uint64_t& h, unsigned& fetches) {
    const unsigned lane = threadIdx.x & 63u, g = lane & 7u, first = lane & ~7u;
    const uint64_t avail = s < n ? n - s : 0;
    const uint64_t end = m < avail ? m : avail;
    for (uint64_t w0 = from & ~(uint64_t)7; w0 < end; w0 += 64) {
        const uint64_t h8 = w0 + 8 * g;
        uint64_t tw = 0, pw = 0;
        if (h8 < end) {
            const unsigned cnt = end - h8 < 8 ? (unsigned)(end - h8) : 8u;
            tw = locate_keep(locate_load_be(text + s + h8, avail - h8), cnt);
            pw = locate_keep(locate_load_be(pat + h8, m - h8), cnt);
            ++fetches;
        }
        const unsigned differ = (unsigned)(__ballot(tw != pw) >> first) & 0xffu;
        if (differ) {
            const int src = (int)first + __ffs(differ) - 1;
            const unsigned long long mine = h8 + (tw != pw ? ((unsigned)__builtin_clzll(tw ^ pw) >> 3) : 0u);
            h = __shfl(mine, src);
            return __shfl(tw < pw ? -1 : 1, src);
        }
    }
    h = end;
    return end == m ? 0 : -1;
}

// Pattern P[0..m) against the suffix S[s..end(s)) from character `from` on: locate_compare with the suffix cut at the end of its
// string.  ends has (n >> 5) + 1 words.  The comparison restarts at h8 = the 8-byte piece of P that holds `from`.  The suffix is
// known to have `from` characters, and may have exactly that many: so a step looks at the nine bits s + h8 .. s + h8 + 8, "the
// suffix has 0 .. 8 characters from s + h8 on" (bit s itself, the start of the suffix's own string, says nothing).  The words
// read lie between the one of bit s + h8 and the one of bit min(s + m, n): at most ceil(m / 32) + 1 of them, each once (win holds
// the word in use and the one after it, fetched by one 8-byte load at the start: a request costs what a text word costs).
// Whatever the bitmap holds, the text is never read at or beyond n and the bitmap never beyond bit n.  fetches counts the text
// words only.
__device__ __forceinline__ int locate_compare_gsa(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends, uint64_t s,
                                                  const uint8_t* __restrict__ pat, uint64_t m, const PatternWords& w, uint64_t from, uint64_t& h,
                                                  unsigned& fetches) {
    const uint64_t avail = s < n ? n - s : 0;
    const uint64_t end = m < avail ? m : avail;
    uint64_t h8 = from & ~(uint64_t)7;
    if (h8 >= end) { h = end; return end == m ? 0 : -1; }
    const uint64_t last = (s + end) >> 5;                   // (s + end <= n: inside the bitmap)
    uint64_t wi = (s + h8) >> 5;
    uint64_t win;                                           // words wi (low half) and wi + 1: one request where both are needed
    if (wi + 1 <= last) __builtin_memcpy(&win, ends + wi, 8); else win = ends[wi];
    for (; h8 < end; h8 += 8) {
        const uint64_t b = s + h8;
        if ((b >> 5) != wi) { ++wi; win = (win >> 32) | (wi + 1 <= last ? (uint64_t)ends[wi + 1] << 32 : 0ull); }
        const uint64_t room = locate_load_be(text + s + h8, avail - h8);
        ++fetches;
        unsigned cnt = end - h8 < 8 ? (unsigned)(end - h8) : 8u;
        const uint32_t e9 = (uint32_t)((win >> (b & 31)) & ((2u << cnt) - 1u)) & (h8 ? ~0u : ~1u);
        const bool ended = e9 != 0;                         // the string ends after cnt <= 8 of these characters
        if (ended) cnt = (unsigned)__ffs((int)e9) - 1u;
        const uint64_t tw = locate_keep(room, cnt);
        const uint64_t j = h8 >> 3;
        const uint64_t pw = locate_keep(j == 0 ? w.p0 : j == 1 ? w.p1 : j == 2 ? w.p2 : j == 3 ? w.p3 : locate_load_be(pat + h8, m - h8), cnt);
        if (tw != pw) { h = h8 + ((unsigned)__builtin_clzll(tw ^ pw) >> 3); return tw < pw ? -1 : 1; }
        if (ended) { h = h8 + cnt; return h == m ? 0 : -1; }
    }
    h = end;
    return end == m ? 0 : -1;
}

// One bisection step of every search here: fetch SA[mid] and compare P[0..m) with that suffix from min(l, r) on, l / r being the
// characters P is known to share with the entries on the two sides of the range (every suffix between them shares min(l, r)).
// G lanes per pattern (1 or 8; eight lanes read the pattern from its buffer, not from w); SET: the suffix ends where its string
// ends, otherwise ends is not read.  n_sa / n_text count the SA entries and text words fetched.
template <typename T, int G, bool SET>
__device__ __forceinline__ int search_step(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends, const T* __restrict__ SA,
                                           uint64_t mid, const uint8_t* __restrict__ P, uint64_t m, const PatternWords& w, uint64_t l, uint64_t r,
                                           uint64_t& h, unsigned& n_sa, unsigned& n_text) {
    static_assert(G == 1 || (G == 8 && !SET), "eight lanes per pattern search one text only");
    const uint64_t s = (uint64_t)SA[mid], from = l < r ? l : r;
    ++n_sa;
    if (G == 8) return locate_compare_group(text, n, s, P, m, from, h, n_text);
    return SET ? locate_compare_gsa(text, n, ends, s, P, m, w, from, h, n_text) : locate_compare(text, n, s, P, m, w, from, h, n_text);
}

// The first entry in [lo, hi) whose suffix is not smaller than P[0..m), or with UPPER the first that is larger and does not carry
// it as a prefix; hi if there is none.  l / r = characters P shares with the entries at lo - 1 / hi.
template <typename T, int G, bool SET, bool UPPER>
__device__ __forceinline__ uint64_t search_bound(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends, const T* __restrict__ SA,
                                                 uint64_t lo, uint64_t hi, const uint8_t* __restrict__ P, uint64_t m, const PatternWords& w, uint64_t l,
                                                 uint64_t r, unsigned& n_sa, unsigned& n_text) {
    uint64_t h = 0;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const int rel = search_step<T, G, SET>(text, n, ends, SA, mid, P, m, w, l, r, h, n_sa, n_text);
        if (UPPER ? rel <= 0 : rel < 0) { lo = mid + 1; l = h; }
        else { hi = mid; r = h; }
    }
    return lo;
}

// the alphabet codes of a table in LDS, by all 256 threads of the workgroup (nothing is staged where there is no table)
__device__ __forceinline__ const uint16_t* search_stage_codes(const CodeTable& code, bool have_table) {
    __shared__ uint16_t s_code[256];
    if (have_table) s_code[threadIdx.x] = code.c[threadIdx.x];
    __syncthreads();
    return s_code;
}

// counters[0] += SA entries fetched, counters[1] += text words fetched (an SA entry is fetched once per group of G lanes, a text
// word by the lane that compares it)
template <int G>
__device__ __forceinline__ void search_count(unsigned long long* __restrict__ counters, unsigned n_sa, unsigned n_text) {
    if ((G == 1 || (threadIdx.x & (G - 1)) == 0) && n_sa) atomicAdd(&counters[0], (unsigned long long)n_sa);
    if (n_text) atomicAdd(&counters[1], (unsigned long long)n_text);
}

// poff[0] == 0, poff[i] <= poff[i + 1] for the q + 1 offsets and, where check_total is set (the suffix mode of the longest match),
// poff[q] == total -- or *bad becomes nonzero.  (static: locate.hip launches it; kmismatch.hip includes this header for the word compare
// and reaches the check through locate_dev)
static __global__ __launch_bounds__(256) void search_offsets_kernel(const uint64_t* __restrict__ poff, uint64_t q, bool check_total, uint64_t total,
                                                                    unsigned long long* bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool wrong = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < q; i += stride) {
        if (i == 0 && poff[0] != 0) wrong = true;
        if (poff[i + 1] < poff[i]) wrong = true;
        if (i == q - 1 && check_total && poff[q] != total) wrong = true;
    }
    if (wrong) atomicOr(bad, 1ull);
}

// [lb(P), ub(P)) of the q patterns pat[poff[i] .. poff[i+1]).  G lanes per pattern (1 or 8).  SET: the text is a string set and
// ends the bitmap of its string ends (G = 1 only); otherwise ends is not read.  table == nullptr: no lookup table (k is 0
// then); else table[B^k + 1] with B = sigma + 1 and code[] the alphabet codes (include/psacx.h: "Use of the table by a
// pattern"; over a set the table of psacx_lookup_table_gsa_dev_*, keys cut at string ends, used by the same rule).  Nothing is
// done if *bad is set (malformed offsets).  Total for any SA, table and bitmap: SA entries >= n are empty suffixes, table entries
// are clamped to n, a bucket with lo > hi is empty, and ub is searched inside [lb, hi], so lb <= ub <= n whatever the arrays
// hold.  COUNT: search_count; bitmap words are not counted.
template <typename T, int G, bool SET, bool COUNT>
__global__ __launch_bounds__(256) void locate_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends,
                                                     const T* __restrict__ SA, const T* __restrict__ table, uint32_t k, uint32_t B, CodeTable code,
                                                     const uint8_t* __restrict__ pat, const uint64_t* __restrict__ poff, uint64_t q,
                                                     T* __restrict__ out_lb, T* __restrict__ out_ub, const unsigned long long* __restrict__ bad,
                                                     unsigned long long* __restrict__ counters) {
    const uint16_t* s_code = search_stage_codes(code, table != nullptr);
    if (*bad) return;
    const uint64_t stride = ((uint64_t)gridDim.x * blockDim.x) / G;
    unsigned n_sa = 0, n_text = 0;
    for (uint64_t pid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G; pid < q; pid += stride) {
        const uint64_t o = poff[pid], m = poff[pid + 1] - o;
        const uint8_t* __restrict__ P = pat + o;
        uint64_t lo = 0, hi = n, base = 0;
        bool done = false;
        if (m == 0) done = true;                                           // [0, n)
        else if (table) {
            const uint32_t j = m < k ? (uint32_t)m : k;
            uint64_t v = 0;
            bool in_alphabet = true;
            for (uint32_t i = 0; i < j; ++i) {
                const uint32_t cd = s_code[P[i]];
                in_alphabet = in_alphabet && cd != 0;
                v = v * B + cd;
            }
            if (in_alphabet) {
                uint64_t width = 1;                                        // B^(k - j)
                for (uint32_t i = j; i < k; ++i) width *= B;
                v *= width;
                const uint64_t a = (uint64_t)table[v], b = (uint64_t)table[v + (m <= k ? width : 1)];
                lo = a < n ? a : n;
                hi = b < n ? b : n;
                if (hi < lo) hi = lo;
                if (m <= k) done = true; else base = k;
            }
        }
        if (!done) {
            const PatternWords w = G == 1 ? pattern_words(P, m) : PatternWords{0, 0, 0, 0};
            // lb: the first entry whose suffix is not smaller than P.  The smallest entry seen to be larger than P bounds the
            // second search.
            uint64_t l = base, r = base, ub_hi = hi, ub_r = base, h = 0;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                const int rel = search_step<T, G, SET>(text, n, ends, SA, mid, P, m, w, l, r, h, n_sa, n_text);
                if (rel < 0) { lo = mid + 1; l = h; }
                else { hi = mid; r = h; if (rel > 0) { ub_hi = mid; ub_r = h; } }
            }
            // ub: the first entry in [lb, ub_hi] that is larger than P.  If lb < ub_hi, the entry at lb was seen to carry P as a prefix.
            hi = search_bound<T, G, SET, true>(text, n, ends, SA, lo, ub_hi, P, m, w, m, ub_r, n_sa, n_text);
        }
        if (G == 1 || (threadIdx.x & (G - 1)) == 0) { out_lb[pid] = (T)lo; out_ub[pid] = (T)hi; }
    }
    if (COUNT) search_count<G>(counters, n_sa, n_text);
}

// MATCH_SUFFIXES of include/psacx.h, as the kernel sees it
#define MATCH_MODE_SUFFIXES 1u

// len(Q) and [lb, ub) of Q[0..len) for `entries` queries, one query per lane (the shape DESIGN.md section 4.3 measured to win).
// mode == 0: query i is pat[poff[i] .. poff[i+1]) and entries == q.  MATCH_MODE_SUFFIXES: query p is pat[p .. poff[j+1]) for the
// pattern j that holds buffer position p, and entries == poff[q] (search_offsets_kernel has checked that, so the search for j
// stays inside poff).  max_len > 0 cuts every query to that many bytes.  SET: as in locate_kernel.  DESIGN.md section 4.5 has the
// two phases and what they cost.
//
// Phase 1 is the lb bisection of locate_kernel.  It ends at the insertion point ip with l / r = the characters Q shares with the
// suffixes at ip - 1 / ip, where those were probed; a side that was never probed lies outside the range, where no entry shares
// more than `base` characters.  len = max(l, r).  On the way it keeps, per side, the nearest probed entry that shares fewer
// characters than the side's last one: [lb_lo, ub_hi) then holds every entry that can carry Q[0..len).
// Phase 2 finds the interval of Q[0..len) by comparing with the query cut to len: its first entry inside [lb_lo, ip - 1] if the
// left neighbour carries it, the first entry that does not inside [ip, ub_hi] if the right one does.  For len == m this is the
// ub search of locate_kernel, probe for probe.
//
// With a table the longest prefix of at most min(m, k) bytes that occurs is found from table entries alone (a bucket of a longer
// prefix lies inside that of a shorter one, so non-emptiness is monotone): a walk down from the longest prefix without a code-0
// byte.  Only a query whose first k bytes occur, with m > k, is searched, inside its bucket and with base = k.
//
// Total for any SA, table and bitmap: SA is read inside [0, n) only, the table inside its B^k + 1 entries, len <= m and
// lb <= ub <= n.  Nothing is done if *bad is set.  COUNT: search_count.
template <typename T, bool SET, bool COUNT>
__global__ __launch_bounds__(256) void match_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends,
                                                    const T* __restrict__ SA, const T* __restrict__ table, uint32_t k, uint32_t B, CodeTable code,
                                                    const uint8_t* __restrict__ pat, const uint64_t* __restrict__ poff, uint64_t q, uint32_t mode,
                                                    uint64_t max_len, uint64_t entries, T* __restrict__ out_len, T* __restrict__ out_lb,
                                                    T* __restrict__ out_ub, const unsigned long long* __restrict__ bad,
                                                    unsigned long long* __restrict__ counters) {
    const uint16_t* s_code = search_stage_codes(code, table != nullptr);
    if (*bad) return;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned n_sa = 0, n_text = 0;
    for (uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; slot < entries; slot += stride) {
        uint64_t o, e;
        if (mode & MATCH_MODE_SUFFIXES) { o = slot; e = poff[occ_last_le(poff, q + 1, slot) + 1]; }    // (poff[q] == entries > slot)
        else { o = poff[slot]; e = poff[slot + 1]; }
        uint64_t m = e - o;
        if (max_len && m > max_len) m = max_len;
        const uint8_t* __restrict__ P = pat + o;
        uint64_t lo = 0, hi = n, base = 0, len = 0;
        bool done = false;
        if (m == 0) done = true;                                           // len 0, [0, n)
        else if (table) {
            uint32_t j = m < k ? (uint32_t)m : k, v = 0;                   // (B^k <= 2^30: keys and widths fit 32 bits)
            for (uint32_t i = 0; i < j; ++i) {
                const uint32_t cd = s_code[P[i]];
                if (cd == 0) { j = i; break; }                             // an absent byte: no longer prefix occurs
                v = v * B + cd;
            }
            uint32_t width = 1;                                            // B^(k - j)
            for (uint32_t i = j; i < k; ++i) width *= B;
            while (j) {                                                    // v < B^j, so (v + 1) * width <= B^k
                const uint64_t a = (uint64_t)table[(uint64_t)v * width], b = (uint64_t)table[(uint64_t)(v + 1) * width];
                lo = a < n ? a : n;
                hi = b < n ? b : n;
                if (lo < hi) break;
                v /= B; width *= B; --j;
            }
            if (j == 0) { lo = 0; hi = n; done = true; }
            else if (j == k && m > k) base = k;
            else { len = j; done = true; }
        }
        if (!done) {
            const PatternWords w = pattern_words(P, m);
            uint64_t l = base, r = base, h = 0;
            uint64_t lb_lo = lo, lb_l = base;                              // the entries before lb_lo share fewer than l characters: at most lb_l
            uint64_t ub_hi = hi, ub_r = base;                              // the entries from ub_hi on share fewer than r: at most ub_r
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                const int rel = search_step<T, 1, SET>(text, n, ends, SA, mid, P, m, w, l, r, h, n_sa, n_text);
                if (rel < 0) { if (h > l) { lb_lo = lo; lb_l = l; } lo = mid + 1; l = h; }
                else { if (h > r) { ub_hi = hi; ub_r = r; } hi = mid; r = h; }
            }
            const uint64_t ip = lo;
            len = l > r ? l : r;
            if (len <= base) { len = base; lo = lb_lo; hi = ub_hi; }       // nothing beyond the range's own prefix: the whole range
            else {
                // (l > base: the left side was probed, lb_lo <= ip - 1; r > base: the right side was probed, ip < ub_hi)
                lo = l == len ? search_bound<T, 1, SET, false>(text, n, ends, SA, lb_lo, ip - 1, P, len, w, lb_l, len, n_sa, n_text) : ip;
                hi = r == len ? search_bound<T, 1, SET, true>(text, n, ends, SA, ip, ub_hi, P, len, w, len, ub_r, n_sa, n_text) : ip;
            }
        }
        out_len[slot] = (T)len; out_lb[slot] = (T)lo; out_ub[slot] = (T)hi;
    }
    if (COUNT) search_count<1>(counters, n_sa, n_text);
}

} // namespace psacx
