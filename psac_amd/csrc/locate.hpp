// locate.hpp -- kernels of the pattern search over a suffix array resident in HBM (psacx_locate_dev_*) and of its k-mer lookup
// table (psacx_lookup_table_dev_*).  include/psacx.h defines lb(P), ub(P), code(), key_k() and the table; tests/locate_model.py
// states them on the host.
//
// Stands in for sa_index::locate (the reference's include/seq_query.hpp:246-251: two binary searches over SA with a string
// comparison per step), in the character-skipping form of bs_esa_index without its LCP arrays, and for lookup_index::construct
// (lookup_table.hpp:36-149: k-mer histogram + scan).
//
// A bisection step is two dependent random fetches -- SA[mid], then the text at SA[mid] + offset -- so a search is bound by the
// number of requests a wave keeps in flight, not by bytes.  One pattern per lane (locate_kernel<T, 1>) keeps 64 independent
// searches in flight per wave; eight lanes per pattern (locate_kernel<T, 8>) compare 64 characters per step instead of 8 and
// keep 8 searches in flight.  DESIGN.md section 4.3 says which is the default and why.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

// Pattern P[0..m) against the suffix that starts at s, from character `from` on (the characters before it are taken as equal).
// An s >= n is the empty suffix.  h = characters the two share (at most m); returns -1: the suffix is smaller than P (a proper
// prefix of P included), 0: P is a prefix of the suffix, +1: the suffix is larger and P is no prefix of it.
// The comparison restarts at the 8-byte piece of P that holds `from`, so that the first 32 bytes of P come from registers
// (p0..p3, big-endian, zero-padded); later pieces are read from the pattern buffer, never beyond m.  The text is never read at or
// beyond n.  fetches counts the text words read.
__device__ __forceinline__ int locate_compare(const uint8_t* __restrict__ text, uint64_t n, uint64_t s, const uint8_t* __restrict__ pat,
                                              uint64_t m, uint64_t p0, uint64_t p1, uint64_t p2, uint64_t p3, uint64_t from, uint64_t& h,
                                              unsigned& fetches) {
    const uint64_t avail = s < n ? n - s : 0;
    const uint64_t end = m < avail ? m : avail;
    for (uint64_t h8 = from & ~(uint64_t)7; h8 < end; h8 += 8) {
        const unsigned cnt = end - h8 < 8 ? (unsigned)(end - h8) : 8u;
        const uint64_t tw = locate_keep(locate_load_be(text + s + h8, avail - h8), cnt);
        ++fetches;
        const uint64_t j = h8 >> 3;
        const uint64_t pw = locate_keep(j == 0 ? p0 : j == 1 ? p1 : j == 2 ? p2 : j == 3 ? p3 : locate_load_be(pat + h8, m - h8), cnt);
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

// poff[0] == 0 and poff[i] <= poff[i + 1] for the q + 1 offsets, or *bad becomes nonzero
__global__ __launch_bounds__(256) void locate_offsets_kernel(const uint64_t* __restrict__ poff, uint64_t q, unsigned long long* bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool wrong = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < q; i += stride) {
        if (i == 0 && poff[0] != 0) wrong = true;
        if (poff[i + 1] < poff[i]) wrong = true;
    }
    if (wrong) atomicOr(bad, 1ull);
}

// [lb(P), ub(P)) of the q patterns pat[poff[i] .. poff[i+1]).  G lanes per pattern (1 or 8).  table == nullptr: no lookup table
// (k is 0 then); else table[B^k + 1] with B = sigma + 1 and code[] the alphabet codes (include/psacx.h: "Use of the table by a
// pattern").  Nothing is done if *bad is set (malformed offsets).  Total for any SA and table: SA entries >= n are empty
// suffixes, table entries are clamped to n, a bucket with lo > hi is empty, and ub is searched inside [lb, hi], so
// lb <= ub <= n whatever the arrays hold.  COUNT: counters[0] += SA entries fetched, counters[1] += text words fetched.
template <typename T, int G, bool COUNT>
__global__ __launch_bounds__(256) void locate_kernel(const uint8_t* __restrict__ text, uint64_t n, const T* __restrict__ SA,
                                                     const T* __restrict__ table, uint32_t k, uint32_t B, CodeTable code,
                                                     const uint8_t* __restrict__ pat, const uint64_t* __restrict__ poff, uint64_t q,
                                                     T* __restrict__ out_lb, T* __restrict__ out_ub, const unsigned long long* __restrict__ bad,
                                                     unsigned long long* __restrict__ counters) {
    __shared__ uint16_t s_code[256];
    if (table) s_code[threadIdx.x] = code.c[threadIdx.x];
    __syncthreads();
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
            uint64_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;
            if (G == 1) {
                p0 = locate_load_be(P, m);
                if (m > 8) p1 = locate_load_be(P + 8, m - 8);
                if (m > 16) p2 = locate_load_be(P + 16, m - 16);
                if (m > 24) p3 = locate_load_be(P + 24, m - 24);
            }
            // lb: the first entry whose suffix is not smaller than P.  l / r = characters P shares with the suffixes at lo - 1 / hi;
            // every suffix between them shares min(l, r).  The smallest entry seen to be larger than P bounds the second search.
            uint64_t l = base, r = base, ub_hi = hi, ub_r = base, h = 0;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1), s = (uint64_t)SA[mid];
                ++n_sa;
                const int rel = G == 1 ? locate_compare(text, n, s, P, m, p0, p1, p2, p3, l < r ? l : r, h, n_text)
                                       : locate_compare_group(text, n, s, P, m, l < r ? l : r, h, n_text);
                if (rel < 0) { lo = mid + 1; l = h; }
                else { hi = mid; r = h; if (rel > 0) { ub_hi = mid; ub_r = h; } }
            }
            // ub: the first entry in [lb, ub_hi] that is larger than P.  If lb < ub_hi, the entry at lb was seen to carry P as a prefix.
            hi = ub_hi; l = m; r = ub_r;
            const uint64_t lb = lo;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1), s = (uint64_t)SA[mid];
                ++n_sa;
                const int rel = G == 1 ? locate_compare(text, n, s, P, m, p0, p1, p2, p3, l < r ? l : r, h, n_text)
                                       : locate_compare_group(text, n, s, P, m, l < r ? l : r, h, n_text);
                if (rel <= 0) { lo = mid + 1; l = h; }
                else { hi = mid; r = h; }
            }
            hi = lo; lo = lb;
        }
        if (G == 1 || (threadIdx.x & (G - 1)) == 0) { out_lb[pid] = (T)lo; out_ub[pid] = (T)hi; }
    }
    if (COUNT) {                                                           // (an SA entry is fetched once per group, a text word by the lane that compares it)
        if ((G == 1 || (threadIdx.x & (G - 1)) == 0) && n_sa) atomicAdd(&counters[0], (unsigned long long)n_sa);
        if (n_text) atomicAdd(&counters[1], (unsigned long long)n_text);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// the lookup table: counts of the keys, then their exclusive prefix sums in place
// ---------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ void locate_count_add(T* p, unsigned long long v);
template <> __device__ __forceinline__ void locate_count_add<uint32_t>(uint32_t* p, unsigned long long v) { atomicAdd(p, (uint32_t)v); }
template <> __device__ __forceinline__ void locate_count_add<uint64_t>(uint64_t* p, unsigned long long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), v);
}

#define LOCATE_STRIP 16            // consecutive text positions per thread: their keys roll from one to the next
#define LOCATE_LDS_BINS 4096       // tables up to this many entries are counted in LDS first (a DNA table of k = 1 has 5 bins)

// key_k(i) of a string set, read character by character: code 0 from the end of i's string on.  room = characters from i to that
// end (anything above k where there are more).
__device__ __forceinline__ uint64_t kmer_key_cut(const uint8_t* __restrict__ text, uint64_t n, const uint16_t* s_code, uint32_t k, uint32_t B,
                                                 uint64_t i, unsigned room) {
    uint64_t key = 0;
    for (uint32_t j = 0; j < k; ++j) key = key * B + (j < room && i + j < n ? s_code[text[i + j]] : 0u);
    return key;
}

// table[key_k(i)] += 1 for every text position i; key_k reads code 0 past the end of the text.  top = B^(k-1).
// SET: the text is a string set and key_k reads code 0 past the end of i's string (psacx_lookup_table_gsa_dev_*); ends is the
// bitmap of psacx_string_ends_dev, (n >> 5) + 1 words.  A strip takes the 64 bits after its first position into a register
// (k <= 30, so they reach past the last character of its last key); the key still rolls from one position to the next, and is
// read afresh where a string starts.  Without SET, ends is not read.
template <typename T, bool IN_LDS, bool SET>
__global__ __launch_bounds__(256) void kmer_count_kernel(const uint8_t* __restrict__ text, uint64_t n, uint32_t k, uint32_t B, uint64_t top,
                                                         CodeTable code, T* __restrict__ table, uint64_t entries, const uint32_t* __restrict__ ends) {
    __shared__ uint16_t s_code[256];
    __shared__ unsigned long long s_bins[IN_LDS ? LOCATE_LDS_BINS : 1];
    s_code[threadIdx.x] = code.c[threadIdx.x];
    if (IN_LDS) for (uint64_t v = threadIdx.x; v < entries; v += blockDim.x) s_bins[v] = 0;
    __syncthreads();
    const uint64_t strips = (n + LOCATE_STRIP - 1) / LOCATE_STRIP, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t st = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; st < strips; st += stride) {
        const uint64_t i0 = st * LOCATE_STRIP, i1 = i0 + LOCATE_STRIP < n ? i0 + LOCATE_STRIP : n;
        uint64_t key = 0;
        if (SET) {
            // bit t of win = bit i0 + 1 + t of the bitmap; i0 is a multiple of 16, so the shift is 1 or 17
            const uint64_t w = (i0 + 1) >> 5, words = (n >> 5) + 1;
            const unsigned sh = (unsigned)((i0 + 1) & 31);
            const uint64_t w0 = ends[w], w1 = w + 1 < words ? ends[w + 1] : 0u, w2 = w + 2 < words ? ends[w + 2] : 0u;
            const uint64_t win = (w0 >> sh) | (w1 << (32 - sh)) | (w2 << (64 - sh));
            key = kmer_key_cut(text, n, s_code, k, B, i0, win ? (unsigned)__builtin_ctzll(win) + 1u : 64u);
            for (uint64_t i = i0; i < i1; ++i) {
                if (IN_LDS) atomicAdd(&s_bins[key], 1ull); else locate_count_add<T>(&table[key], 1ull);
                const uint64_t after = win >> (i + 1 - i0);                 // bit t = bit i + 2 + t of the bitmap
                const unsigned room = after ? (unsigned)__builtin_ctzll(after) + 1u : 64u;      // characters from i + 1 to the end of its string
                if ((win >> (i - i0)) & 1) key = kmer_key_cut(text, n, s_code, k, B, i + 1, room);      // a string starts at i + 1
                else key = (key - (uint64_t)s_code[text[i]] * top) * B + (k - 1 < room && i + k < n ? s_code[text[i + k]] : 0u);
            }
            continue;
        }
        for (uint32_t j = 0; j < k; ++j) key = key * B + (i0 + j < n ? s_code[text[i0 + j]] : 0u);
        for (uint64_t i = i0; i < i1; ++i) {
            if (IN_LDS) atomicAdd(&s_bins[key], 1ull); else locate_count_add<T>(&table[key], 1ull);
            key = (key - (uint64_t)s_code[text[i]] * top) * B + (i + k < n ? s_code[text[i + k]] : 0u);
        }
    }
    if (IN_LDS) {
        __syncthreads();
        for (uint64_t v = threadIdx.x; v < entries; v += blockDim.x) if (s_bins[v]) locate_count_add<T>(&table[v], s_bins[v]);
    }
}

#define LOCATE_SCAN_ITEMS 16       // entries per thread; a block of 256 threads scans 4096

// exclusive prefix sums of one value per thread over the block (256 threads); total = their sum
__device__ __forceinline__ unsigned long long locate_block_exscan(unsigned long long v, unsigned long long* sh, unsigned long long& total) {
    const unsigned t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (unsigned d = 1; d < 256; d <<= 1) {
        const unsigned long long add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const unsigned long long incl = sh[t];
    total = sh[255];
    __syncthreads();
    return incl - v;
}

template <typename T>
__global__ __launch_bounds__(256) void scan_sums_kernel(const T* __restrict__ a, uint64_t len, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long sh[256];
    const uint64_t first = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * LOCATE_SCAN_ITEMS;
    unsigned long long v = 0, total;
    for (int j = 0; j < LOCATE_SCAN_ITEMS; ++j) if (first + j < len) v += a[first + j];
    (void)locate_block_exscan(v, sh, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: sums[0..nb) become their exclusive prefix sums
__global__ __launch_bounds__(256) void scan_top_kernel(unsigned long long* __restrict__ sums, uint64_t nb) {
    __shared__ unsigned long long sh[256];
    unsigned long long carry = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += 256) {
        const uint64_t i = b0 + threadIdx.x;
        const unsigned long long v = i < nb ? sums[i] : 0;
        unsigned long long total;
        const unsigned long long ex = locate_block_exscan(v, sh, total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void scan_apply_kernel(T* __restrict__ a, uint64_t len, const unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long sh[256];
    const uint64_t first = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * LOCATE_SCAN_ITEMS;
    unsigned long long item[LOCATE_SCAN_ITEMS], v = 0, total;
    for (int j = 0; j < LOCATE_SCAN_ITEMS; ++j) { item[j] = first + j < len ? (unsigned long long)a[first + j] : 0; v += item[j]; }
    unsigned long long run = sums[blockIdx.x] + locate_block_exscan(v, sh, total);
    for (int j = 0; j < LOCATE_SCAN_ITEMS; ++j) {
        if (first + j < len) a[first + j] = (T)run;
        run += item[j];
    }
}

} // namespace psacx
