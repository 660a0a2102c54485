// locate_gsa.hpp -- kernels of the pattern search over the generalized suffix array of a string set resident in HBM
// (psacx_locate_gsa_dev_*) and of the occurrence lists (psacx_occurrences_dev_*).  include/psacx.h defines both ("pattern search
// over string sets", "occurrence lists"); tests/locate_gsa_model.py states them on the host.
//
// The search is locate_kernel<T, 1> of locate.hpp with one change: suffix i is S[i..end(i)), and end(i) comes from the bitmap of
// the string ends (bit p = "a string starts at p, or p == n"; psacx_string_ends_dev).  A bisection step stays two dependent
// fetches: once SA[mid] = s has arrived, the bitmap words that cover [s + from, s + from + 8] and the text word at s + from have
// addresses that are both known, so they are issued together and the text word is cut at the first set bit afterwards.
#pragma once
#include "locate.hpp"

namespace psacx {

// Pattern P[0..m) against the suffix S[s..end(s)) from character `from` on: locate_compare with the suffix cut at the end of its
// string.  ends has (n >> 5) + 1 words.  The comparison restarts at h8 = the 8-byte piece of P that holds `from`.  The suffix is
// known to have `from` characters, and may have exactly that many: so a step looks at the nine bits s + h8 .. s + h8 + 8, "the
// suffix has 0 .. 8 characters from s + h8 on" (bit s itself, the start of the suffix's own string, says nothing).  The words
// read lie between the one of bit s + h8 and the one of bit min(s + m, n): at most ceil(m / 32) + 1 of them, each once (win holds
// the word in use and the one after it, fetched by one 8-byte load at the start: a request costs what a text word costs).  Whatever the bitmap holds, the text is never read at or beyond n and the bitmap
// never beyond bit n.  fetches counts the text words only.
__device__ __forceinline__ int locate_compare_gsa(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends, uint64_t s,
                                                  const uint8_t* __restrict__ pat, uint64_t m, uint64_t p0, uint64_t p1, uint64_t p2, uint64_t p3,
                                                  uint64_t from, uint64_t& h, unsigned& fetches) {
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
        const uint64_t pw = locate_keep(j == 0 ? p0 : j == 1 ? p1 : j == 2 ? p2 : j == 3 ? p3 : locate_load_be(pat + h8, m - h8), cnt);
        if (tw != pw) { h = h8 + ((unsigned)__builtin_clzll(tw ^ pw) >> 3); return tw < pw ? -1 : 1; }
        if (ended) { h = h8 + cnt; return h == m ? 0 : -1; }
    }
    h = end;
    return end == m ? 0 : -1;
}

// locate_kernel<T, 1, COUNT> over a string set: [lb(P), ub(P)) with suffix i = S[i..end(i)).  The table is that of
// psacx_lookup_table_gsa_dev_* (keys cut at string ends) and is used by the same rule.  Total for any SA, table and bitmap:
// lb <= ub <= n.  COUNT: counters[0] += SA entries fetched, counters[1] += text words fetched; bitmap words are not counted.
template <typename T, bool COUNT>
__global__ __launch_bounds__(256) void locate_gsa_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends,
                                                         const T* __restrict__ SA, const T* __restrict__ table, uint32_t k, uint32_t B, CodeTable code,
                                                         const uint8_t* __restrict__ pat, const uint64_t* __restrict__ poff, uint64_t q,
                                                         T* __restrict__ out_lb, T* __restrict__ out_ub, const unsigned long long* __restrict__ bad,
                                                         unsigned long long* __restrict__ counters) {
    __shared__ uint16_t s_code[256];
    if (table) s_code[threadIdx.x] = code.c[threadIdx.x];
    __syncthreads();
    if (*bad) return;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned n_sa = 0, n_text = 0;
    for (uint64_t pid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; pid < q; pid += stride) {
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
            const uint64_t p0 = locate_load_be(P, m), p1 = m > 8 ? locate_load_be(P + 8, m - 8) : 0, p2 = m > 16 ? locate_load_be(P + 16, m - 16) : 0,
                           p3 = m > 24 ? locate_load_be(P + 24, m - 24) : 0;
            // the two searches of locate_kernel: lb, then ub inside [lb, the smallest entry seen to be larger than P]
            uint64_t l = base, r = base, ub_hi = hi, ub_r = base, h = 0;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1), s = (uint64_t)SA[mid];
                ++n_sa;
                const int rel = locate_compare_gsa(text, n, ends, s, P, m, p0, p1, p2, p3, l < r ? l : r, h, n_text);
                if (rel < 0) { lo = mid + 1; l = h; }
                else { hi = mid; r = h; if (rel > 0) { ub_hi = mid; ub_r = h; } }
            }
            hi = ub_hi; l = m; r = ub_r;
            const uint64_t lb = lo;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1), s = (uint64_t)SA[mid];
                ++n_sa;
                const int rel = locate_compare_gsa(text, n, ends, s, P, m, p0, p1, p2, p3, l < r ? l : r, h, n_text);
                if (rel <= 0) { lo = mid + 1; l = h; }
                else { hi = mid; r = h; }
            }
            hi = lo; lo = lb;
        }
        out_lb[pid] = (T)lo; out_ub[pid] = (T)hi;
    }
    if (COUNT) {
        if (n_sa) atomicAdd(&counters[0], (unsigned long long)n_sa);
        if (n_text) atomicAdd(&counters[1], (unsigned long long)n_text);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// occurrence lists: counts, their exclusive prefix sums (scan_*_kernel of locate.hpp), and an output-balanced expansion
// ---------------------------------------------------------------------------------------------------------------
// start[j] = c_j = ub_j - lb_j if lb_j <= ub_j <= n, else 0, capped at limit where limit > 0; start[q] = 0
template <typename T>
__global__ __launch_bounds__(256) void occ_counts_kernel(const T* __restrict__ lb, const T* __restrict__ ub, uint64_t q, uint64_t n, uint64_t limit,
                                                         uint64_t* __restrict__ start) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= q; j += stride) {
        uint64_t c = 0;
        if (j < q) {
            const uint64_t a = (uint64_t)lb[j], b = (uint64_t)ub[j];
            if (a <= b && b <= n) c = b - a;
            if (limit && c > limit) c = limit;
        }
        start[j] = c;
    }
}

#define OCC_TILE 1024              // output slots per workgroup: 4 per thread, slot o0 + t + 256 i, so that a wave stores 64 neighbours
#define OCC_CHUNK 1024             // entries of start[] a workgroup holds in LDS at a time

// the largest j in [0, cnt) with a[j] <= o; a ascends and a[0] <= o
template <typename P>
__device__ __forceinline__ uint64_t occ_last_le(P a, uint64_t cnt, uint64_t o) {
    uint64_t lo = 0, hi = cnt;
    while (hi - lo > 1) { const uint64_t mid = lo + ((hi - lo) >> 1); if (a[mid] <= o) lo = mid; else hi = mid; }
    return lo;
}

// pos[start_j + t] = SA[lb_j + t] for t < c_j, and sid[] = the string holding it (m for a pos >= n) where sid != nullptr.
// A workgroup owns the output slots [o0, o1) of its tile, whatever the counts are: it finds the pattern that holds its first
// open slot by one binary search in start[] (the last j with start[j] <= slot: runs of empty intervals before it are skipped),
// takes start[j .. j + OCC_CHUNK] into LDS, and every thread looks its slots up there.  A tile inside one long interval
// takes one search and one chunk; a tile over many short intervals takes one search and one chunk per OCC_CHUNK patterns.  So the
// cost is one search per tile, one LDS search per output and one read of start[] per pattern, however the counts are spread.
// start[] is the scan of the counts this call took from lb / ub, so lb_j + t < ub_j <= n for every slot.
template <typename T>
__global__ __launch_bounds__(256) void occ_expand_kernel(const T* __restrict__ SA, uint64_t n, const uint64_t* __restrict__ off, uint64_t m,
                                                         const T* __restrict__ lb, uint64_t q, const uint64_t* __restrict__ start, uint64_t total,
                                                         T* __restrict__ pos, T* __restrict__ sid) {
    __shared__ uint64_t s_start[OCC_CHUNK + 1];
    for (uint64_t o0 = (uint64_t)blockIdx.x * OCC_TILE; o0 < total; o0 += (uint64_t)gridDim.x * OCC_TILE) {
        const uint64_t o1 = o0 + OCC_TILE < total ? o0 + OCC_TILE : total;
        uint64_t open = o0;                                                 // the first slot not written yet (the same in every thread)
        while (open < o1) {
            const uint64_t j0 = occ_last_le(start, q + 1, open);            // (start[q] = total > open, so j0 < q and interval j0 holds `open`)
            const uint64_t cnt = q - j0 < OCC_CHUNK ? q - j0 : OCC_CHUNK;   // patterns j0 .. j0 + cnt - 1, and the start of the one after them
            __syncthreads();
            for (uint64_t i = threadIdx.x; i <= cnt; i += blockDim.x) s_start[i] = start[j0 + i];
            __syncthreads();
            const uint64_t upto = s_start[cnt] < o1 ? s_start[cnt] : o1;    // > open
            for (uint64_t o = o0 + threadIdx.x; o < upto; o += blockDim.x) {
                if (o < open) continue;
                const uint64_t i = occ_last_le(s_start, cnt, o);
                const uint64_t p = (uint64_t)SA[(uint64_t)lb[j0 + i] + (o - s_start[i])];
                pos[o] = (T)p;
                if (sid) sid[o] = (T)(p >= n ? m : occ_last_le(off, m, p));
            }
            open = upto;
        }
    }
}

} // namespace psacx
