// match.hpp -- kernels of the longest-match search over a suffix array resident in HBM (psacx_match_dev_* and
// psacx_match_gsa_dev_*).  include/psacx.h defines len(Q) and the interval of the matched prefix ("longest match and matching
// statistics"); tests/match_model.py states them on the host.
//
// One query per lane, as locate_kernel<T, 1>: the shape DESIGN.md section 4.3 measured to win.  The comparisons are
// locate_compare (locate.hpp) and locate_compare_gsa (locate_gsa.hpp), called with the query cut to the length that matters;
// neither header is changed.  DESIGN.md section 4.5 has the kernel's two phases and what they cost.
#pragma once
#include "locate_gsa.hpp"

namespace psacx {

// MATCH_SUFFIXES of include/psacx.h, as the kernel sees it
#define MATCH_MODE_SUFFIXES 1u

// poff[0] == 0, poff[i] <= poff[i + 1] for the q + 1 offsets and, where check_total is set, poff[q] == total -- or *bad becomes
// nonzero.  (locate_offsets_kernel with the third rule.)
__global__ __launch_bounds__(256) void match_offsets_kernel(const uint64_t* __restrict__ poff, uint64_t q, bool check_total, uint64_t total,
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

template <bool SET>
__device__ __forceinline__ int match_compare(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends, uint64_t s,
                                             const uint8_t* __restrict__ pat, uint64_t m, uint64_t p0, uint64_t p1, uint64_t p2, uint64_t p3,
                                             uint64_t from, uint64_t& h, unsigned& fetches) {
    return SET ? locate_compare_gsa(text, n, ends, s, pat, m, p0, p1, p2, p3, from, h, fetches)
               : locate_compare(text, n, s, pat, m, p0, p1, p2, p3, from, h, fetches);
}

// len(Q) and [lb, ub) of Q[0..len) for `entries` queries.  mode == 0: query i is pat[poff[i] .. poff[i+1]) and entries == q.
// MATCH_MODE_SUFFIXES: query p is pat[p .. poff[j+1]) for the pattern j that holds buffer position p, and entries == poff[q]
// (match_offsets_kernel has checked that, so the search for j stays inside poff).  max_len > 0 cuts every query to that many bytes.
// SET: suffix i ends where its string ends (ends = the bitmap of psacx_string_ends_dev); otherwise ends is not read.
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
// lb <= ub <= n.  Nothing is done if *bad is set.  COUNT: counters[0] += SA entries fetched, counters[1] += text words fetched.
template <typename T, bool SET, bool COUNT>
__global__ __launch_bounds__(256) void match_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends,
                                                    const T* __restrict__ SA, const T* __restrict__ table, uint32_t k, uint32_t B, CodeTable code,
                                                    const uint8_t* __restrict__ pat, const uint64_t* __restrict__ poff, uint64_t q, uint32_t mode,
                                                    uint64_t max_len, uint64_t entries, T* __restrict__ out_len, T* __restrict__ out_lb,
                                                    T* __restrict__ out_ub, const unsigned long long* __restrict__ bad,
                                                    unsigned long long* __restrict__ counters) {
    __shared__ uint16_t s_code[256];
    if (table) s_code[threadIdx.x] = code.c[threadIdx.x];
    __syncthreads();
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
            const uint64_t p0 = locate_load_be(P, m), p1 = m > 8 ? locate_load_be(P + 8, m - 8) : 0, p2 = m > 16 ? locate_load_be(P + 16, m - 16) : 0,
                           p3 = m > 24 ? locate_load_be(P + 24, m - 24) : 0;
            uint64_t l = base, r = base, h = 0;
            uint64_t lb_lo = lo, lb_l = base;                              // the entries before lb_lo share fewer than l characters: at most lb_l
            uint64_t ub_hi = hi, ub_r = base;                              // the entries from ub_hi on share fewer than r: at most ub_r
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1), s = (uint64_t)SA[mid];
                ++n_sa;
                const int rel = match_compare<SET>(text, n, ends, s, P, m, p0, p1, p2, p3, l < r ? l : r, h, n_text);
                if (rel < 0) { if (h > l) { lb_lo = lo; lb_l = l; } lo = mid + 1; l = h; }
                else { if (h > r) { ub_hi = hi; ub_r = r; } hi = mid; r = h; }
            }
            const uint64_t ip = lo;
            len = l > r ? l : r;
            if (len <= base) { len = base; lo = lb_lo; hi = ub_hi; }       // nothing beyond the range's own prefix: the whole range
            else {
                uint64_t x = ip, y = ip, cl, cr;
                if (l == len) {                                            // (l > base: the left side was probed, lb_lo <= ip - 1)
                    x = lb_lo; y = ip - 1; cl = lb_l; cr = len;
                    while (x < y) {
                        const uint64_t mid = x + ((y - x) >> 1), s = (uint64_t)SA[mid];
                        ++n_sa;
                        const int rel = match_compare<SET>(text, n, ends, s, P, len, p0, p1, p2, p3, cl < cr ? cl : cr, h, n_text);
                        if (rel < 0) { x = mid + 1; cl = h; }
                        else { y = mid; cr = h; }
                    }
                }
                const uint64_t lb = x;
                y = ip;
                if (r == len) {                                            // (r > base: the right side was probed, ip < ub_hi)
                    x = ip; y = ub_hi; cl = len; cr = ub_r;
                    while (x < y) {
                        const uint64_t mid = x + ((y - x) >> 1), s = (uint64_t)SA[mid];
                        ++n_sa;
                        const int rel = match_compare<SET>(text, n, ends, s, P, len, p0, p1, p2, p3, cl < cr ? cl : cr, h, n_text);
                        if (rel <= 0) { x = mid + 1; cl = h; }
                        else { y = mid; cr = h; }
                    }
                    y = x;
                }
                lo = lb; hi = y;
            }
        }
        out_len[slot] = (T)len; out_lb[slot] = (T)lo; out_ub[slot] = (T)hi;
    }
    if (COUNT) {
        if (n_sa) atomicAdd(&counters[0], (unsigned long long)n_sa);
        if (n_text) atomicAdd(&counters[1], (unsigned long long)n_text);
    }
}

} // namespace psacx
