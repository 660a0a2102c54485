// kedit.hpp -- pattern search with up to e edits (unit-cost Levenshtein distance) over the index resident in HBM: text, SA and, for a
// string set, the bitmap of the string ends (include/psacx.h: "pattern search with edits").  The reference has no counterpart; kernels
// only, the calls are in kedit.hip.  Pieces, their search and the numbering of the candidates are those of kmismatch.hpp.
//
// Verification.  ked_verify_kernel has the structure of kmm_verify_kernel: a workgroup owns the OCC_TILE candidate numbers of its
// tile whatever the pieces are, one lane per candidate fetches s = SA[r] and takes the diagonal t0 = s - b_i.  The starts to examine
// are t in [max(lo, t0 - e), min(s, t0 + e)], lo the start of s's string.  One right-to-left pass gives D for all of them at once:
//     C[i][p] = min over L of ed(P[i..m), S[p..p + L)),  p + L <= hi (the end of s's string),  D(j, t) = C[0][t]
//     C[m][p] = 0,   C[i][p] = min(C[i + 1][p + 1] + (P[i] != S[p]), C[i + 1][p] + 1, C[i][p + 1] + 1)
// in the band of the W = 4 EB + 1 diagonals p - i in [t0 - 2 EB, t0 + 2 EB]: an alignment of cost <= e from a start within e of t0
// stays within 2e of t0.  EB >= e is a compile-time bucket (1, 2, 4, 8, 15), so the row lives in W registers with static indices and
// the loops over it unroll fully; the text bytes of the row sit in W more registers and move by one per row, so a row costs one
// text byte and one pattern byte of loads.  Values saturate at KED_CAP > 15, which also stands for "outside": the cells beyond hi
// start there and stay there, a cell at hi gets m - i from above, and the cells below lo never feed a cell at or above it.  A lane
// leaves as soon as every cell of its row exceeds e: row minima never fall on the way to row 0.  The result is a 32-bit mask, bit
// t - (t0 - e), and its popcount as a 64-bit count for the scan.
//
// Raw hits.  ked_emit_kernel writes (j, t) of every set bit at the scanned count of its candidate.  After pair_sort and the unique
// (ked_unique_kernel marks the first of equal neighbours; select.hpp compacts), ked_align_kernel runs, for the surviving (j, t) only,
// the forward pass F[i][L] = ed(P[0..i), S[t..t + L)) in the band |L - i| <= EB and takes D = min F[m][L] and the smallest L that
// attains it.  D <= e implies L <= m + e, so band and window lose nothing.
//
// Whatever SA and table hold: a candidate is a rank below n (occ_counts_kernel), an s >= n is passed over, text is read at
// lo <= p < hi <= n only, the bitmap inside the words of bits max(0, t0 - 2 EB) .. min(n, t0 + m + 2 EB + 1), and a bit is set only
// after the pass over all m rows, so every pair emitted is a true hit and the forward pass gives its exact L and D.
#pragma once
#include "kmismatch.hpp"

namespace psacx {

constexpr uint32_t KED_MAX_E = KMM_MAX_E;               // 2e + 1 <= 31 starts: one 32-bit mask per candidate
constexpr uint32_t KED_CAP = 64;                        // the saturated distance: above every e, and "outside the band or the string"

// the largest position <= s and >= floor with its bit set, or floor (floor <= s; bits below floor are not looked at)
__device__ __forceinline__ uint64_t ked_string_start(const uint32_t* __restrict__ ends, uint64_t s, uint64_t floor) {
    const uint64_t wf = floor >> 5;
    uint64_t w = s >> 5;
    uint32_t x = ends[w] & (~0u >> (31 - (unsigned)(s & 31)));
    while (!x && w > wf) x = ends[--w];
    if (!x) return floor;
    const uint64_t p = (w << 5) + (31 - (uint64_t)__clz((int)x));
    return p > floor ? p : floor;
}

// the smallest position > s and <= limit with its bit set, or limit (s < limit <= n, so the words read lie inside the bitmap)
__device__ __forceinline__ uint64_t ked_string_end(const uint32_t* __restrict__ ends, uint64_t s, uint64_t limit) {
    const uint64_t wl = limit >> 5;
    uint64_t w = (s + 1) >> 5;
    uint32_t x = ends[w] & (~0u << ((s + 1) & 31));
    while (!x && w < wl) x = ends[++w];
    if (!x) return limit;
    const uint64_t p = (w << 5) + (uint64_t)(__ffs((int)x) - 1);
    return p < limit ? p : limit;
}

__device__ __forceinline__ uint32_t ked_byte(const uint8_t* __restrict__ text, int64_t p, int64_t lo, int64_t hi) {
    return p >= lo && p < hi ? (uint32_t)text[p] : 256u;                      // (256: no byte of a pattern)
}

// The starts t = t0 + dt, |dt| <= e, lo <= t <= s, with D(P, t) <= e, as bits dt + e.  lo <= s < hi <= n bound the string of s (or
// the part of it the band can reach); P has m >= 1 bytes.
template <int EB>
__device__ __forceinline__ uint32_t ked_starts(const uint8_t* __restrict__ text, int64_t lo, int64_t hi, int64_t s, int64_t t0,
                                               const uint8_t* __restrict__ P, uint64_t m, uint32_t e) {
    constexpr int W = 4 * EB + 1;
    uint32_t R[W], Tc[W];
    int64_t p0 = (int64_t)m - 1 + t0 - 2 * EB;                                // the text position of cell 0 in row m - 1
#pragma unroll
    for (int k = 0; k < W; ++k) {
        R[k] = p0 + 1 + k <= hi ? 0u : KED_CAP;                               // row m
        Tc[k] = ked_byte(text, p0 + k, lo, hi);
    }
    for (uint64_t i = m; i-- > 0;) {
        const uint32_t pc = P[i];
        uint32_t right = KED_CAP, lowest = KED_CAP;
#pragma unroll
        for (int k = W - 1; k >= 0; --k) {
            const uint32_t up = k > 0 ? R[k - 1] : KED_CAP;
            const uint32_t v = min(min(R[k] + (Tc[k] != pc ? 1u : 0u), min(up, right) + 1u), KED_CAP);
            R[k] = v;
            right = v;
            lowest = min(lowest, v);
        }
        if (lowest > e) return 0u;
#pragma unroll
        for (int k = W - 1; k > 0; --k) Tc[k] = Tc[k - 1];
        --p0;
        Tc[0] = ked_byte(text, p0, lo, hi);
    }
    uint32_t mask = 0;
#pragma unroll
    for (int dt = -EB; dt <= EB; ++dt) {
        const int64_t t = t0 + dt;
        const bool in = (dt < 0 ? (uint32_t)-dt : (uint32_t)dt) <= e && t >= lo && t <= s;
        if (in && R[dt + 2 * EB] <= e) mask |= 1u << (uint32_t)(dt + (int)e);
    }
    return mask;
}

// mask[o] = the starts of candidate o with D <= e (bit t - (t0 - e)) and cnt[o] = their number, for o < total.  The structure of
// kmm_verify_kernel over cstart[0 .. Q], boff and lb.  SET: ends is the bitmap of the string ends, otherwise it is not read.
template <typename T, bool SET, int EB>
__global__ __launch_bounds__(256) void ked_verify_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends,
                                                         const T* __restrict__ SA, const uint8_t* __restrict__ pat, const uint64_t* __restrict__ boff,
                                                         const T* __restrict__ lb, const uint64_t* __restrict__ cstart, uint64_t Q, uint32_t E1,
                                                         uint64_t total, uint32_t* __restrict__ mask, uint64_t* __restrict__ cnt) {
    __shared__ uint64_t s_start[OCC_CHUNK + 1];
    for (uint64_t o0 = (uint64_t)blockIdx.x * OCC_TILE; o0 < total; o0 += (uint64_t)gridDim.x * OCC_TILE) {
        const uint64_t o1 = o0 + OCC_TILE < total ? o0 + OCC_TILE : total;
        uint64_t open = o0;                                                  // the first candidate not done yet (the same in every thread)
        while (open < o1) {
            const uint64_t j0 = occ_last_le(cstart, Q + 1, open);
            if (j0 >= Q) break;
            const uint64_t cn = Q - j0 < OCC_CHUNK ? Q - j0 : OCC_CHUNK;
            __syncthreads();
            for (uint64_t i = threadIdx.x; i <= cn; i += blockDim.x) s_start[i] = cstart[j0 + i];
            __syncthreads();
            const uint64_t upto = s_start[cn] < o1 ? s_start[cn] : o1;
            if (upto <= open) break;                                         // (starts that do not ascend: not this call's scan)
            for (uint64_t o = o0 + threadIdx.x; o < upto; o += blockDim.x) {
                if (o < open) continue;
                const uint64_t i = occ_last_le(s_start, cn, o), x = j0 + i;
                const uint64_t r = (uint64_t)lb[x] + (o - s_start[i]);       // < ub_x <= n: the counts came from these entries
                const uint64_t j = x >> 32 ? x / E1 : (uint64_t)((uint32_t)x / E1);
                const uint64_t* __restrict__ cut = boff + j * E1;
                const uint64_t p0 = cut[0], m = cut[E1] - p0, b = boff[x] - p0;
                const uint64_t s = r < n ? (uint64_t)SA[r] : n;
                uint32_t bits = 0;
                if (s < n && m > 0) {
                    const int64_t t0 = (int64_t)s - (int64_t)b;
                    const uint64_t floor = t0 > 2 * EB ? (uint64_t)(t0 - 2 * EB) : 0;
                    uint64_t limit = (uint64_t)t0 + m + 2 * EB + 1;          // (t0 + m >= s, so limit > s)
                    if (limit > n) limit = n;
                    const uint64_t lo = SET ? ked_string_start(ends, s, floor) : floor;
                    const uint64_t hi = SET ? ked_string_end(ends, s, limit) : limit;
                    bits = ked_starts<EB>(text, (int64_t)lo, (int64_t)hi, (int64_t)s, t0, pat + p0, m, E1 - 1);
                }
                mask[o] = bits;
                cnt[o] = (uint64_t)__popc(bits);
            }
            open = upto;
        }
    }
}

// (j, t) of every bit of every mask, at cnt[o] (scanned) onwards in ascending t
template <typename T>
__global__ __launch_bounds__(256) void ked_emit_kernel(const uint32_t* __restrict__ mask, const uint64_t* __restrict__ cnt, uint64_t total,
                                                       const uint64_t* __restrict__ boff, const T* __restrict__ lb, const uint64_t* __restrict__ cstart,
                                                       uint64_t Q, uint32_t E1, const T* __restrict__ SA, uint64_t n, T* __restrict__ k1, T* __restrict__ k2) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += stride) {
        uint32_t bits = mask[o];
        if (!bits) continue;
        const uint64_t x = occ_last_le(cstart, Q + 1, o);
        if (x >= Q) continue;
        const uint64_t r = (uint64_t)lb[x] + (o - cstart[x]);
        const uint64_t j = x / E1;
        const int64_t s = r < n ? (int64_t)SA[r] : 0, b = (int64_t)(boff[x] - boff[j * E1]);
        const int64_t first = s - b - (int64_t)(E1 - 1);                     // the start of bit 0 (a set bit: its start is >= 0)
        uint64_t at = cnt[o];
        while (bits) {
            const int d = __ffs((int)bits) - 1;
            bits &= bits - 1;
            k1[at] = (T)j;
            k2[at] = (T)(first + d);
            ++at;
        }
    }
}

// marks[x] = 1 iff the sorted pair x differs from pair x - 1, for x < raw; marks holds whole tiles, the rest is cleared
template <typename T>
__global__ __launch_bounds__(256) void ked_unique_kernel(const T* __restrict__ k1, const T* __restrict__ k2, uint64_t raw, uint64_t padded,
                                                         unsigned char* __restrict__ marks) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < padded; x += stride)
        marks[x] = x < raw && (x == 0 || k1[x] != k1[x - 1] || k2[x] != k2[x - 1]) ? 1 : 0;
}

// The functor of select_emit_kernel after the unique: the k-th distinct pair
template <typename T>
struct KedPairEmit {
    const T* __restrict__ k1;
    const T* __restrict__ k2;
    uint64_t* __restrict__ qid;
    T* __restrict__ tpos;
    __device__ __forceinline__ void operator()(uint64_t at, uint64_t x) const { qid[at] = (uint64_t)k1[x]; tpos[at] = k2[x]; }
    __device__ __forceinline__ void finish(uint64_t) const {}
};

// D = min over L <= hi - t of ed(P, S[t .. t + L)) and the smallest L that attains it, exact where D <= e <= EB (else D > e, capped
// at KED_CAP).  Forward, row i over L = i - EB + k, k = 0 .. 2 EB.
template <int EB>
__device__ __forceinline__ uint32_t ked_align(const uint8_t* __restrict__ text, int64_t t, int64_t hi, const uint8_t* __restrict__ P, uint64_t m, uint64_t* L) {
    constexpr int W = 2 * EB + 1;
    const int64_t lmax = hi - t;
    uint32_t R[W], Tc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        R[k] = k >= EB && k - EB <= lmax ? (uint32_t)(k - EB) : KED_CAP;     // row 0: L = k - EB
        Tc[k] = ked_byte(text, t - EB + k, t, hi);                           // the byte that the step to row 1 compares in cell k: S[t + L - 1], L = 1 - EB + k
    }
    for (uint64_t i = 0; i < m; ++i) {
        const uint32_t pc = P[i];
        const int64_t l0 = (int64_t)i + 1 - EB;                              // L of cell 0 in row i + 1
        uint32_t left = KED_CAP;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const uint32_t up = k + 1 < W ? R[k + 1] : KED_CAP;
            uint32_t v = min(min(R[k] + (Tc[k] != pc ? 1u : 0u), min(up, left) + 1u), KED_CAP);
            if (l0 + k > lmax) v = KED_CAP;
            R[k] = v;
            left = v;
        }
#pragma unroll
        for (int k = 0; k + 1 < W; ++k) Tc[k] = Tc[k + 1];
        Tc[W - 1] = ked_byte(text, t + (int64_t)i + 1 + EB, t, hi);
    }
    uint32_t d = KED_CAP;
    int at = 0;
#pragma unroll
    for (int k = 0; k < W; ++k)
        if (R[k] < d) { d = R[k]; at = k; }
    *L = (uint64_t)((int64_t)m - EB + at);
    return d;
}

// len[x], dist[x] of the hit (qid[x], tpos[x]), x < z; best (where given): best[j] = the smallest distance among the hits of pattern j
template <typename T, bool SET, int EB>
__global__ __launch_bounds__(256) void ked_align_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends,
                                                        const uint8_t* __restrict__ pat, const uint64_t* __restrict__ poff, uint64_t q,
                                                        const uint64_t* __restrict__ qid, const T* __restrict__ tpos, uint64_t z, T* __restrict__ len,
                                                        uint8_t* __restrict__ dist, uint32_t* __restrict__ best) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < z; x += stride) {
        const uint64_t j = qid[x], t = (uint64_t)tpos[x];
        uint64_t L = 0;
        uint32_t d = KED_CAP;
        if (j < q && t < n) {                                                // (always: they are this call's own pairs)
            const uint64_t p0 = poff[j], m = poff[j + 1] - p0;
            uint64_t limit = t + m + EB + 1;
            if (limit > n) limit = n;
            const uint64_t hi = SET ? ked_string_end(ends, t, limit) : limit;
            d = ked_align<EB>(text, (int64_t)t, (int64_t)hi, pat + p0, m, &L);
            if (best) atomicMin(best + j, d);
        }
        len[x] = (T)L;
        dist[x] = (uint8_t)d;
    }
}

// marks[x] = 1 iff hit x has the smallest distance of its pattern, for x < z; whole tiles, the rest cleared
__global__ __launch_bounds__(256) void ked_best_kernel(const uint64_t* __restrict__ qid, const uint8_t* __restrict__ dist, const uint32_t* __restrict__ best,
                                                       uint64_t z, uint64_t padded, unsigned char* __restrict__ marks) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < padded; x += stride)
        marks[x] = x < z && (uint32_t)dist[x] == best[qid[x]] ? 1 : 0;
}

// The functor of select_emit_kernel for PSACX_KEDIT_BEST: the k-th kept hit goes from the call's own lists to the caller's
template <typename T>
struct KedBestEmit {
    const uint64_t* __restrict__ qid0;
    const T* __restrict__ tpos0;
    const T* __restrict__ len0;
    const uint8_t* __restrict__ dist0;
    uint64_t* __restrict__ qid;
    T* __restrict__ tpos;
    T* __restrict__ len;
    uint8_t* __restrict__ dist;
    __device__ __forceinline__ void operator()(uint64_t at, uint64_t x) const {
        qid[at] = qid0[x]; tpos[at] = tpos0[x]; len[at] = len0[x]; dist[at] = dist0[x];
    }
    __device__ __forceinline__ void finish(uint64_t) const {}
};

} // namespace psacx
