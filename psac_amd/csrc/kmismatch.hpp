// kmismatch.hpp -- pattern search with up to e mismatches (substitutions) over the index resident in HBM: text, SA and, for a string
// set, the bitmap of the string ends (include/psacx.h: "pattern search with mismatches").  The reference has no counterpart; kernels
// only, the calls are in kmismatch.hip.
//
// Pieces.  kmm_pieces_kernel cuts pattern j of m_j bytes at b_i = floor(i m_j / (e + 1)), i = 0 .. e + 1, and writes the boundaries of
// all patterns as one offset array of q (e + 1) patterns over the same pattern buffer: the pieces are searched by locate_kernel as
// they are.  A pattern shorter than e + 1 bytes has empty pieces, whose interval would be [0, n): kmm_short_kernel empties the
// intervals of its pieces, so it owns no candidate.
//
// Verification.  kmm_verify_kernel: balanced by candidates as occ_expand_kernel is by outputs.  A workgroup owns the OCC_TILE
// candidate numbers of its tile whatever the pieces are: one binary search in the candidate starts for its first piece, OCC_CHUNK
// starts in LDS, one LDS search per candidate.  Candidate o is rank r of piece x = j (e + 1) + i: one lane fetches s = SA[r], takes
// t = s - b_i, and -- where the window [t, t + m_j) lies inside the text and inside one string -- compares the pattern with the
// text there, 8 bytes per step, left to right: the differing bytes of a word are counted by a SWAR byte test and a popcount,
// piece by piece; a piece before i without a difference ends the comparison (the alignment is reported from that piece), and so
// does d > e.  One mark byte per candidate, 1 | (d << 1) for a hit and 0 otherwise, stored to neighbouring addresses by
// neighbouring lanes.
//
// Compaction.  The mark bytes go through select.hpp in tiles of OCC_TILE (it reads bit 0 only, so the distance rides along);
// KmmEmit finds the piece of a hit by a search over all candidate starts (one per hit, not per candidate), fetches SA[r] once more
// and stores the triple.
//
// Whatever SA and table hold: the intervals are locate_kernel's, lb <= ub <= n, and the counts are occ_counts_kernel's, so every
// candidate is a rank below n; an s outside [b_i, n) or a window that leaves the text or its string is not compared; the
// comparison reads the text inside [t, t + m_j) and the bitmap inside the words of bits t + 1 .. t + m_j - 1; and a mark is set only
// after all m_j bytes were compared with at most e differences, so every triple is a true hit with exactly that d.
#pragma once
#include "occurrences.hpp"
#include "search.hpp"
#include "select.hpp"

namespace psacx {

constexpr uint32_t KMM_MAX_E = 15;                     // d <= 15: 1 | (d << 1) fits the mark byte
static_assert(OCC_TILE == (int)SELECT_TILE_MAX, "a tile of candidates is a tile of the compaction");

// boff[j (e + 1) + i] = poff[j] + floor(i m_j / (e + 1)) for j < q, i <= e, and boff[q (e + 1)] = poff[q]; E1 = e + 1.  The boundaries
// start at 0 and ascend iff poff does: boff[j E1] = poff[j], and the search that takes them checks that (search_offsets_kernel).
// (static: kmismatch.hip and kedit.hip both launch it)
static __global__ __launch_bounds__(256) void kmm_pieces_kernel(const uint64_t* __restrict__ poff, uint64_t q, uint32_t E1, uint64_t* __restrict__ boff) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, Q = q * E1;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x <= Q; x += stride) {
        const uint64_t j = x / E1, i = x - j * E1;
        const uint64_t p0 = poff[j];
        boff[x] = i == 0 ? p0 : p0 + i * (poff[j + 1] - p0) / E1;            // (i > 0: j < q)
    }
}

// the intervals of the pieces of a pattern shorter than E1 bytes become empty
template <typename T>
__global__ __launch_bounds__(256) void kmm_short_kernel(const uint64_t* __restrict__ poff, uint64_t q, uint32_t E1, T* __restrict__ lb, T* __restrict__ ub) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, Q = q * E1;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < Q; x += stride) {
        const uint64_t j = x / E1;
        if (poff[j + 1] - poff[j] < E1) { lb[x] = 0; ub[x] = 0; }
    }
}

// bit 7 of every byte of x that is not zero
__device__ __forceinline__ uint64_t kmm_nonzero_bytes(uint64_t x) {
    const uint64_t low7 = 0x7f7f7f7f7f7f7f7full;
    return (((x & low7) + low7) | x) & ~low7;
}

// the bytes u .. v - 1 of a big-endian word (byte 0 on top), 0 <= u < v <= 8
__device__ __forceinline__ uint64_t kmm_bytes(unsigned u, unsigned v) {
    return (~0ull >> (8 * u)) & (v >= 8 ? ~0ull : ~(~0ull >> (8 * v)));
}

// no bit of bits t + 1 .. t + m - 1 is set: the window [t, t + m) lies inside one string.  t + m <= n, so the words read lie inside the
// (n >> 5) + 1 of the bitmap: those of bits t + 1 and t + m - 1 and the ones between, each once.
__device__ __forceinline__ bool kmm_one_string(const uint32_t* __restrict__ ends, uint64_t t, uint64_t m) {
    if (m < 2) return true;
    const uint64_t a = t + 1, z = t + m - 1, wa = a >> 5, wz = z >> 5;
    for (uint64_t w = wa; w <= wz; ++w) {
        uint32_t word = ends[w];
        if (w == wa) word &= ~0u << (a & 31);
        if (w == wz) word &= ~0u >> (31 - (unsigned)(z & 31));
        if (word) return false;
    }
    return true;
}

// The pattern P[0..m) against text[t..t + m) (inside the text), whose piece boundaries are cut[0 .. E1] - cut[0]: the number of
// differing bytes, or ~0u as soon as it exceeds e or one of the pieces before ip has none.  The comparison goes by the 8-byte words
// of the pattern, so that the first 32 bytes of P come from registers (w); later words are read from the pattern buffer, never
// beyond m.  A word is split where a piece before ip ends; from piece ip on the pieces no longer matter.
__device__ __forceinline__ unsigned kmm_distance(const uint8_t* __restrict__ text, uint64_t n, uint64_t t, const uint8_t* __restrict__ P, uint64_t m,
                                                 const PatternWords& w, const uint64_t* __restrict__ cut, unsigned ip, unsigned e) {
    const uint64_t p0 = cut[0];
    unsigned d = 0, in_piece = 0, cp = 0;
    uint64_t next = ip ? cut[1] - p0 : ~0ull;                                // where piece cp ends, while cp < ip
    for (uint64_t h8 = 0; h8 < m; h8 += 8) {
        const unsigned cnt = m - h8 < 8 ? (unsigned)(m - h8) : 8u;
        const uint64_t tw = locate_load_be(text + t + h8, n - t - h8);
        const uint64_t j = h8 >> 3;
        const uint64_t pw = j == 0 ? w.p0 : j == 1 ? w.p1 : j == 2 ? w.p2 : j == 3 ? w.p3 : locate_load_be(P + h8, m - h8);
        const uint64_t y = kmm_nonzero_bytes(tw ^ pw);
        unsigned u = 0;                                                      // the bytes before u of this word are counted
        while (next < h8 + cnt) {                                            // (next > h8 + u or piece cp is empty: the pieces of m >= E1 are not)
            const unsigned v = (unsigned)(next - h8);
            if (v > u) { const unsigned c = (unsigned)__popcll(y & kmm_bytes(u, v)); d += c; in_piece += c; u = v; }
            if (in_piece == 0) return ~0u;
            in_piece = 0;
            ++cp;
            next = cp < ip ? cut[cp + 1] - p0 : ~0ull;
        }
        const unsigned c = (unsigned)__popcll(y & kmm_bytes(u, cnt));
        d += c; in_piece += c;
        if (d > e) return ~0u;
    }
    return d;
}

// marks[o] = 1 | (d << 1) iff candidate o is a hit with d mismatches, else 0, for o < total; *tested += the candidates whose window
// lies inside the text and one string.  The structure of occ_expand_kernel over cstart[0 .. Q], the scan of the counts of the Q
// piece intervals lb / ub, which ends with total; boff are the Q + 1 piece boundaries.  SET: ends is the bitmap of the string ends,
// otherwise it is not read.
template <typename T, bool SET>
__global__ __launch_bounds__(256) void kmm_verify_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends,
                                                         const T* __restrict__ SA, const uint8_t* __restrict__ pat, const uint64_t* __restrict__ boff,
                                                         const T* __restrict__ lb, const uint64_t* __restrict__ cstart, uint64_t Q, uint32_t E1,
                                                         uint64_t total, unsigned char* __restrict__ marks, unsigned long long* __restrict__ tested) {
    __shared__ uint64_t s_start[OCC_CHUNK + 1];
    __shared__ uint64_t s_red[256 / WAVE];
    uint64_t ntested = 0;
    for (uint64_t o0 = (uint64_t)blockIdx.x * OCC_TILE; o0 < total; o0 += (uint64_t)gridDim.x * OCC_TILE) {
        const uint64_t o1 = o0 + OCC_TILE < total ? o0 + OCC_TILE : total;
        uint64_t open = o0;                                                  // the first candidate not marked yet (the same in every thread)
        while (open < o1) {
            const uint64_t j0 = occ_last_le(cstart, Q + 1, open);            // (cstart[Q] = total > open, so j0 < Q and piece j0 holds `open`)
            if (j0 >= Q) break;
            const uint64_t cnt = Q - j0 < OCC_CHUNK ? Q - j0 : OCC_CHUNK;
            __syncthreads();
            for (uint64_t i = threadIdx.x; i <= cnt; i += blockDim.x) s_start[i] = cstart[j0 + i];
            __syncthreads();
            const uint64_t upto = s_start[cnt] < o1 ? s_start[cnt] : o1;
            if (upto <= open) break;                                         // (starts that do not ascend: not this call's scan)
            for (uint64_t o = o0 + threadIdx.x; o < upto; o += blockDim.x) {
                if (o < open) continue;
                const uint64_t i = occ_last_le(s_start, cnt, o), x = j0 + i;
                const uint64_t r = (uint64_t)lb[x] + (o - s_start[i]);       // < ub_x <= n: the counts came from these entries
                const uint64_t j = x >> 32 ? x / E1 : (uint64_t)((uint32_t)x / E1);
                const unsigned ip = (unsigned)(x - j * E1);
                const uint64_t* __restrict__ cut = boff + j * E1;
                const uint64_t p0 = cut[0], m = cut[E1] - p0, b = boff[x] - p0;
                const uint64_t s = r < n ? (uint64_t)SA[r] : n;
                unsigned char mark = 0;
                if (s >= b && s < n && s - b + m <= n && (!SET || kmm_one_string(ends, s - b, m))) {
                    ++ntested;
                    const uint8_t* __restrict__ P = pat + p0;
                    const unsigned d = kmm_distance(text, n, s - b, P, m, pattern_words(P, m), cut, ip, E1 - 1);
                    if (d != ~0u) mark = (unsigned char)(1u | (d << 1));
                }
                marks[o] = mark;
            }
            open = upto;
        }
    }
    const uint64_t sum = block_reduce<256, uint64_t>(ntested, OpSum(), s_red);
    if (threadIdx.x == 0 && sum) atomicAdd(tested, (unsigned long long)sum);
}

// The functor of select_emit_kernel: the k-th hit o gives the triple (pattern, SA[r] - b_i, distance)
template <typename T>
struct KmmEmit {
    const uint64_t* __restrict__ boff;
    const T* __restrict__ lb;
    const uint64_t* __restrict__ cstart;
    uint64_t Q;
    uint32_t E1;
    const T* __restrict__ SA;
    uint64_t n;
    const unsigned char* __restrict__ marks;
    uint64_t* __restrict__ qid;
    T* __restrict__ tpos;
    uint8_t* __restrict__ dist;
    __device__ __forceinline__ void operator()(uint64_t at, uint64_t o) const {
        const uint64_t x = occ_last_le(cstart, Q + 1, o);
        if (x >= Q) return;
        const uint64_t r = (uint64_t)lb[x] + (o - cstart[x]);
        const uint64_t j = x / E1;
        const uint64_t s = r < n ? (uint64_t)SA[r] : 0, b = boff[x] - boff[j * E1];
        qid[at] = j;
        tpos[at] = (T)(s - b);                                               // (a hit: s >= b was seen by kmm_verify_kernel, and no input is written)
        dist[at] = (uint8_t)(marks[o] >> 1);
    }
    __device__ __forceinline__ void finish(uint64_t) const {}
};

} // namespace psacx
