// fm.hpp -- the FM-index of a text or a string set, resident in HBM as one array of 64-bit words: a binary wavelet matrix over the
// BWT with a STOP symbol, its per-symbol tables, and a sampled suffix array (include/psacx.h: "FM-index").  Backward search counts a
// pattern without text or SA; the LF walk to a sampled rank gives its positions.  The reference has no counterpart; kernels only, the
// calls are in fm.hip.
//
// Symbols.  w[r] = 0 (STOP) where first[r], else code[bwt[r]], codes 1 .. sigma in byte order; bits = ceil(log2(sigma + 1)), 1 .. 9.
//
// Blob, in words of 64 bits (FmLayout):
//     levels    bits x cells cells of two words {ones in front of this cell, 64 bits}, cells = (n >> 6) + 1, most significant bit of
//               the code first; level l holds the ranks ordered stably by the bit-reversed top l bits of their code
//     tables    FM_TAB_WORDS words: Z[l] = the zeros of level l; C[c], c = 0 .. sigma + 1 (C[sigma + 1] = n); D[c] = C[c] + E[c] - (the
//               start of c in the order behind the last level), modulo 2^64
//     marks     cells cells as above over "first[r] or SA[r] % sample == 0"           (sample > 0 only)
//     val       marks entries of the index type, val[rank_marks(r)] = SA[r]            (sample > 0 only)
// One rank is ONE 16-byte load: the directory entry and its word share a cell (RankDir of repeats.hpp keeps them apart).
//
// A bound p goes through the levels by p = bit ? Z[l] + rank1(p) : p - rank1(p) on the bits of c and ends at (start of c) + rank_c(p),
// so LF costs `bits` dependent cells and one add of D[c].  The same descent on the bits it finds at p reads the symbol at p and its
// rank together: an LF step of the walk costs `bits` cells and one mark cell.
//
// Totality.  Every position is clamped to n before it selects a cell, every table index is at most sigma, every val index is below
// marks: whatever the blob holds, nothing is read outside its words.  A search takes L steps, a walk at most min(sample, n).
//
// Build, streaming: fm_hist_kernel (bytes and last bytes of strings), fm_codes_kernel (w as 16-bit codes), then per level
// fm_level_count_kernel (one ballot per wave, its popcount), the scan of scan.hpp, and fm_level_emit_kernel (the same ballot again:
// lane 0 stores the cell, every lane sends its code to bit ? Z + rank1 : r - rank1 of the next order; the rank comes from the scanned
// count and the ballot in registers, so the cells just written are not read back).  The marks take the same two kernels and the scan.
#pragma once
#include "engine.hpp"
#include "occurrences.hpp"

namespace psacx {

constexpr uint64_t FM_SYMS = 264;                      // room for the codes 0 .. 257 of a table
constexpr uint64_t FM_TAB_Z = 0;                       // 16 words: Z[l]
constexpr uint64_t FM_TAB_C = 16;                      // FM_SYMS words: C[c]
constexpr uint64_t FM_TAB_D = FM_TAB_C + FM_SYMS;      // FM_SYMS words: D[c]
constexpr uint64_t FM_TAB_WORDS = FM_TAB_D + FM_SYMS;  // 544 (even: the cells behind the tables stay 16-byte aligned)

inline uint32_t fm_bits_of(uint32_t sigma) {
    uint32_t b = 1;
    while ((1u << b) < sigma + 1u) ++b;
    return b;
}

// where the parts of a blob start, in words; the same on the host and in the kernels
struct FmLayout {
    const uint64_t* fm;
    uint64_t n, cells, tab, marks_at, val_at, words, marks, sample;
    uint32_t sigma, bits;
};

inline void fm_layout(uint64_t n, uint32_t sigma, uint32_t bits, uint64_t sample, uint64_t marks, size_t entry_bytes, FmLayout& Y) {
    Y.fm = nullptr;
    Y.n = n; Y.sigma = sigma; Y.bits = bits; Y.sample = sample; Y.marks = marks;
    Y.cells = (n >> 6) + 1;
    Y.tab = 2 * Y.cells * bits;
    Y.marks_at = Y.tab + FM_TAB_WORDS;
    Y.val_at = Y.marks_at + (sample ? 2 * Y.cells : 0);
    Y.words = Y.val_at + (marks * entry_bytes + 7) / 8;
}

// bit p of a bitmap of 32-bit words (the first bitmap of psacx_bwt_dev_*)
__device__ __forceinline__ bool fm_bit(const uint32_t* __restrict__ bits, uint64_t p) { return (bits[p >> 5] >> (p & 31)) & 1u; }

// the cell that holds position p <= n of the cell array at word `at`
__device__ __forceinline__ ulonglong2 fm_cell(const FmLayout& Y, uint64_t at, uint64_t p) {
    return reinterpret_cast<const ulonglong2*>(Y.fm + at)[p >> 6];
}
__device__ __forceinline__ uint64_t fm_rank1(const ulonglong2& cell, uint64_t p) {
    return cell.x + (uint64_t)__popcll(cell.y & ((1ull << (p & 63)) - 1ull));
}

// the tables of a blob and the codes of its descriptor into LDS, by the 256 threads of a workgroup
__device__ __forceinline__ void fm_stage(const FmLayout& Y, const CodeTable& code, uint16_t* s_code, uint64_t* s_tab) {
    s_code[threadIdx.x] = code.c[threadIdx.x];
    for (uint64_t i = threadIdx.x; i < FM_TAB_WORDS; i += blockDim.x) s_tab[i] = Y.fm[Y.tab + i];
    __syncthreads();
}

// hist[b] += the ranks r with bwt[r] == b, hist[256 + b] += those of them that start a string.  Sixteen copies of the table in LDS, one
// per lane modulo 16, so that the few bytes of a small alphabet do not queue on one counter; flushed well before 32 bits run out.
__global__ __launch_bounds__(256) void fm_hist_kernel(uint64_t n, const uint8_t* __restrict__ bwt, const uint32_t* __restrict__ first,
                                                      unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s_h[16][512];
    for (int i = threadIdx.x; i < 16 * 512; i += 256) (&s_h[0][0])[i] = 0;
    __syncthreads();
    const unsigned copy = threadIdx.x & 15;
    uint32_t trips = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base < n; base += (uint64_t)gridDim.x * 256) {
        const uint64_t r = base + threadIdx.x;
        if (r < n) {
            const unsigned b = bwt[r];
            atomicAdd(&s_h[copy][b], 1u);
            if (fm_bit(first, r)) atomicAdd(&s_h[copy][256 + b], 1u);
        }
        if ((++trips & 0xFFFFFu) == 0) {               // (the same trip in every thread of the workgroup)
            __syncthreads();
            for (int i = threadIdx.x; i < 512; i += 256) {
                unsigned long long s = 0;
                for (int k = 0; k < 16; ++k) { s += s_h[k][i]; s_h[k][i] = 0; }
                if (s) atomicAdd(&hist[i], s);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 256) {
        unsigned long long s = 0;
        for (int k = 0; k < 16; ++k) s += s_h[k][i];
        if (s) atomicAdd(&hist[i], s);
    }
}

// w[r] = 0 where first[r], else code[bwt[r]]
__global__ __launch_bounds__(256) void fm_codes_kernel(uint64_t n, const uint8_t* __restrict__ bwt, const uint32_t* __restrict__ first, CodeTable code,
                                                       uint16_t* __restrict__ w) {
    __shared__ uint16_t s_code[256];
    s_code[threadIdx.x] = code.c[threadIdx.x];
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) w[r] = fm_bit(first, r) ? (uint16_t)0 : s_code[bwt[r]];
}

// cnt[x] = the codes of chunk x (64 ranks) with bit `shift` set, x < cells
__global__ __launch_bounds__(256) void fm_level_count_kernel(uint64_t n, const uint16_t* __restrict__ w, unsigned shift, uint64_t* __restrict__ cnt) {
    const unsigned lane = lane_id();
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
    const uint64_t cells = (n >> 6) + 1;
    for (uint64_t x = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; x < cells; x += nwaves) {
        const uint64_t r = (x << 6) + lane;
        const uint64_t ballot = __ballot(r < n && ((w[r] >> shift) & 1u));
        if (lane == 0) cnt[x] = (uint64_t)__popcll(ballot);
    }
}

// The cells of a level from the scanned counts, and, with next != nullptr, its stable partition: the code of rank r goes to
// Z + rank1(r) if its bit is set and to r - rank1(r) if not (Z = the zeros of the level, so both stay below n).
__global__ __launch_bounds__(256) void fm_level_emit_kernel(uint64_t n, const uint16_t* __restrict__ w, unsigned shift, const uint64_t* __restrict__ cnt,
                                                            uint64_t Z, ulonglong2* __restrict__ level, uint16_t* __restrict__ next) {
    const unsigned lane = lane_id();
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
    const uint64_t cells = (n >> 6) + 1;
    for (uint64_t x = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; x < cells; x += nwaves) {
        const uint64_t r = (x << 6) + lane;
        const uint16_t code = r < n ? w[r] : (uint16_t)0;
        const bool bit = r < n && ((code >> shift) & 1u);
        const uint64_t ballot = __ballot(bit), ones = cnt[x];
        if (lane == 0) level[x] = make_ulonglong2(ones, ballot);
        if (next && r < n) {
            const uint64_t rk = ones + (uint64_t)__popcll(ballot & ((1ull << lane) - 1ull));
            const uint64_t dst = bit ? Z + rk : r - rk;
            if (dst < n) next[dst] = code;
        }
    }
}

// is rank r < n marked: it starts a string, or its position is a multiple of sample (mask = sample - 1 where sample is a power of two, else 0)
template <typename T>
__device__ __forceinline__ bool fm_marked(const uint32_t* __restrict__ first, const T* __restrict__ SA, uint64_t r, uint64_t sample, uint64_t mask) {
    if (fm_bit(first, r)) return true;
    const uint64_t s = (uint64_t)SA[r];
    return mask ? (s & mask) == 0 : (sample == 1 || s % sample == 0);
}

// cnt[x] = the marked ranks of chunk x, x < cells; cnt[cells] = 0, which the scan turns into their number
template <typename T>
__global__ __launch_bounds__(256) void fm_mark_count_kernel(uint64_t n, const uint32_t* __restrict__ first, const T* __restrict__ SA, uint64_t sample,
                                                            uint64_t mask, uint64_t* __restrict__ cnt) {
    const unsigned lane = lane_id();
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
    const uint64_t cells = (n >> 6) + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[cells] = 0;
    for (uint64_t x = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; x < cells; x += nwaves) {
        const uint64_t r = (x << 6) + lane;
        const uint64_t ballot = __ballot(r < n && fm_marked<T>(first, SA, r, sample, mask));
        if (lane == 0) cnt[x] = (uint64_t)__popcll(ballot);
    }
}

// the mark cells from the scanned counts, and val[rank_marks(r)] = SA[r] for every marked rank (an index at or beyond `marks` is dropped)
template <typename T>
__global__ __launch_bounds__(256) void fm_mark_emit_kernel(uint64_t n, const uint32_t* __restrict__ first, const T* __restrict__ SA, uint64_t sample,
                                                           uint64_t mask, const uint64_t* __restrict__ cnt, uint64_t marks,
                                                           ulonglong2* __restrict__ cells_out, T* __restrict__ val) {
    const unsigned lane = lane_id();
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
    const uint64_t cells = (n >> 6) + 1;
    for (uint64_t x = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; x < cells; x += nwaves) {
        const uint64_t r = (x << 6) + lane;
        const bool mark = r < n && fm_marked<T>(first, SA, r, sample, mask);
        const uint64_t ballot = __ballot(mark), ones = cnt[x];
        if (lane == 0) cells_out[x] = make_ulonglong2(ones, ballot);
        if (mark) {
            const uint64_t at = ones + (uint64_t)__popcll(ballot & ((1ull << lane) - 1ull));
            if (at < marks) val[at] = SA[r];
        }
    }
}

// Backward search, one pattern per lane: [lb, ub) of pat[poff[j] .. poff[j + 1]), or lb = ub = 0 where it does not occur.  The first
// step is [C[c], C[c + 1]); every further step takes both bounds through the levels together, so that their two cells are in flight at
// once.  Nothing is done if *bad is set (malformed offsets, search_offsets_kernel of search.hpp).
template <typename T>
__global__ __launch_bounds__(256) void fm_count_kernel(FmLayout Y, CodeTable code, const uint8_t* __restrict__ pat, const uint64_t* __restrict__ poff,
                                                       uint64_t q, T* __restrict__ out_lb, T* __restrict__ out_ub,
                                                       const unsigned long long* __restrict__ bad) {
    __shared__ uint16_t s_code[256];
    __shared__ uint64_t s_tab[FM_TAB_WORDS];
    fm_stage(Y, code, s_code, s_tab);
    if (*bad) return;
    const uint64_t n = Y.n, stride = (uint64_t)gridDim.x * blockDim.x;
    const unsigned bits = Y.bits;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < q; j += stride) {
        const uint64_t o = poff[j], len = poff[j + 1] - o;
        const uint8_t* __restrict__ P = pat + o;
        uint64_t lb = 0, ub = n;
        for (uint64_t i = len; i-- > 0 && lb < ub;) {
            const unsigned c = s_code[P[i]];
            if (c == 0) { lb = ub = 0; break; }
            if (i == len - 1) {
                lb = s_tab[FM_TAB_C + c]; ub = s_tab[FM_TAB_C + c + 1];
            } else {
                for (unsigned l = 0; l < bits; ++l) {
                    const uint64_t at = 2 * Y.cells * l;
                    const ulonglong2 ca = fm_cell(Y, at, lb), cb = fm_cell(Y, at, ub);
                    const uint64_t ra = fm_rank1(ca, lb), rb = fm_rank1(cb, ub);
                    if ((c >> (bits - 1 - l)) & 1u) { const uint64_t Z = s_tab[FM_TAB_Z + l]; lb = Z + ra; ub = Z + rb; }
                    else { lb -= ra; ub -= rb; }
                    lb = lb < n ? lb : n;
                    ub = ub < n ? ub : n;
                }
                lb += s_tab[FM_TAB_D + c]; ub += s_tab[FM_TAB_D + c];
            }
            lb = lb < n ? lb : n;
            ub = ub < n ? ub : n;
        }
        if (lb >= ub && len) lb = ub = 0;
        out_lb[j] = (T)lb;
        out_ub[j] = (T)ub;
    }
}

// The functor of occ_tile_walk for the occurrence lists of an FM-index: slot o of interval x is rank r = lb[x] + (o - first); the walk
// tests r's mark, and where it is clear reads the symbol at r and its rank in one descent and steps to LF(r).  pos[o] = val + steps, or
// all ones where no mark came up within min(sample, n) steps (no intact index does that); sid[o] as in occ_expand_kernel.
template <typename T>
struct FmWalk {
    FmLayout Y;
    const uint64_t* s_tab;
    const uint64_t* __restrict__ off;
    uint64_t m;
    const T* __restrict__ lb;
    T* __restrict__ pos;
    T* __restrict__ sid;
    __device__ __forceinline__ void operator()(uint64_t o, uint64_t x, uint64_t first) const {
        const uint64_t n = Y.n, most = Y.sample < n ? Y.sample : n;
        const T* __restrict__ val = reinterpret_cast<const T*>(Y.fm + Y.val_at);
        uint64_t r = (uint64_t)lb[x] + (o - first);
        T p = (T)~(T)0;
        for (uint64_t steps = 0; steps < most && r < n; ++steps) {
            const ulonglong2 mc = fm_cell(Y, Y.marks_at, r);
            if ((mc.y >> (r & 63)) & 1ull) {
                const uint64_t at = fm_rank1(mc, r);
                if (at < Y.marks) p = (T)((uint64_t)val[at] + steps);
                break;
            }
            unsigned c = 0;
            uint64_t at_r = r;
            for (unsigned l = 0; l < Y.bits; ++l) {
                const ulonglong2 cl = fm_cell(Y, 2 * Y.cells * l, at_r);
                const uint64_t rk = fm_rank1(cl, at_r);
                const unsigned bit = (unsigned)((cl.y >> (at_r & 63)) & 1ull);
                c = (c << 1) | bit;
                at_r = bit ? s_tab[FM_TAB_Z + l] + rk : at_r - rk;
                at_r = at_r < n ? at_r : n;
            }
            if (c == 0 || c > Y.sigma) break;           // (STOP: the rank starts a string and is marked in an intact index)
            r = at_r + s_tab[FM_TAB_D + c];
        }
        pos[o] = p;
        if (sid) sid[o] = (T)((uint64_t)p >= n ? m : occ_last_le(off, m, (uint64_t)p));
    }
};

// pos[start_j + t] = SA[lb_j + t] through the walk, for every slot below total; tiles and chunks as occ_expand_kernel
template <typename T>
__global__ __launch_bounds__(256) void fm_occ_kernel(FmLayout Y, const uint64_t* __restrict__ off, uint64_t m, const T* __restrict__ lb, uint64_t q,
                                                     const uint64_t* __restrict__ start, uint64_t total, T* __restrict__ pos, T* __restrict__ sid) {
    __shared__ uint64_t s_start[OCC_CHUNK + 1];
    __shared__ uint64_t s_tab[FM_TAB_WORDS];
    for (uint64_t i = threadIdx.x; i < FM_TAB_WORDS; i += blockDim.x) s_tab[i] = Y.fm[Y.tab + i];
    __syncthreads();
    const FmWalk<T> walk{Y, s_tab, off, m, lb, pos, sid};
    for (uint64_t o0 = (uint64_t)blockIdx.x * OCC_TILE; o0 < total; o0 += (uint64_t)gridDim.x * OCC_TILE) {
        const uint64_t o1 = o0 + OCC_TILE < total ? o0 + OCC_TILE : total;
        occ_tile_walk(start, q, o0, o1, s_start, walk);
    }
}

} // namespace psacx
