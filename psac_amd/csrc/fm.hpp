// fm.hpp -- the FM-index of a text or a string set, resident in HBM as one array of 64-bit words: a binary wavelet matrix over the
// BWT with a STOP symbol, its per-symbol tables, and a sampled suffix array (include/psacx.h: "FM-index").  Backward search counts a
// pattern without text or SA; the LF walk to a sampled rank gives its positions; the LF walk from the sampled rank of a text position
// gives the bytes to its left (text samples, at the end of this file).  The reference has no counterpart; kernels only, the calls are in
// fm.hip.
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

// The descent that reads the symbol at rank r < n and its rank together: the code w[r], bit by bit from the cells, and in at_r where r
// stands behind the last level, so that LF(r) = at_r + D[code].  Every position is clamped to n before it selects a cell.
__device__ __forceinline__ unsigned fm_symbol_rank(const FmLayout& Y, const uint64_t* s_tab, uint64_t r, uint64_t& at_r) {
    const uint64_t n = Y.n;
    unsigned c = 0;
    at_r = r;
    for (unsigned l = 0; l < Y.bits; ++l) {
        const ulonglong2 cl = fm_cell(Y, 2 * Y.cells * l, at_r);
        const uint64_t rk = fm_rank1(cl, at_r);
        const unsigned bit = (unsigned)((cl.y >> (at_r & 63)) & 1ull);
        c = (c << 1) | bit;
        at_r = bit ? s_tab[FM_TAB_Z + l] + rk : at_r - rk;
        at_r = at_r < n ? at_r : n;
    }
    return c;
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
            uint64_t at_r;
            const unsigned c = fm_symbol_rank(Y, s_tab, r, at_r);
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

// ---- text samples and extraction (include/psacx.h: "FM-index", text samples) ----
//
// ts[k] = the rank of the suffix at position (k + 1) * rate - 1, k < blocks = n / rate; ts[blocks + j] = the rank of the suffix at the
// last byte of string j.  From the sample at the right end of a block, or at its string's end where that comes first, the bytes to the
// left come out under LF: the head symbol of the sampled rank from C, every further byte from the descent at the rank.  STOP stands at the
// ranks of string starts, so no walk leaves its string, and no walk can be entered from the next one: hence the end samples.
//
// The calls hand the kernels a rate of at most n + 1 (every rate above n gives blocks = 0 and one block for all positions, as n + 1
// does), so that (k + 1) * rate does not wrap; shift = log2(rate) where rate is a power of two, else 64.

__device__ __forceinline__ uint64_t fm_block_of(uint64_t p, uint64_t rate, unsigned shift) { return shift < 64 ? p >> shift : p / rate; }

struct FmDecode { uint8_t b[FM_SYMS]; };               // code -> byte, from the descriptor; b[0] = 0

// One pass over the ranks: r goes to the slot of SA[r] where SA[r] + 1 is a multiple of rate, and to the end slot of its string where
// SA[r] + 1 ends one (ends: the bitmap of the string ends; nullptr for one text, whose end is n).  An SA entry at or beyond n is skipped.
// With 32-bit entries the division is one of 32 bits (rate <= n + 1 and SA[r] + 1 <= n, both below 2^32).
template <typename T>
__global__ __launch_bounds__(256) void fm_text_samples_kernel(uint64_t n, const T* __restrict__ SA, const uint32_t* __restrict__ ends,
                                                              const uint64_t* __restrict__ off, uint64_t m, uint64_t rate, unsigned shift,
                                                              uint64_t blocks, T* __restrict__ ts) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const uint64_t p = (uint64_t)SA[r];
        if (p >= n) continue;
        const uint64_t e = p + 1;
        const uint64_t k = shift < 64 ? e >> shift : sizeof(T) == 4 ? (uint64_t)((uint32_t)e / (uint32_t)rate) : e / rate;
        if (k * rate == e && k - 1 < blocks) ts[k - 1] = (T)r;                                     // (k >= 1 here: e >= 1)
        if (ends ? fm_bit(ends, e) : e == n) ts[blocks + (off ? occ_last_le(off, m, p) : 0)] = (T)r;
    }
}

// start[j] = the length of query j clipped at the end of the string that holds pos[j] (0 for a pos at or beyond n), segs[j] = the
// rate-aligned blocks its range meets; start[q] = segs[q] = 0.  off: valid offsets, or nullptr for one text.
template <typename T>
__global__ __launch_bounds__(256) void fm_extract_counts_kernel(uint64_t n, const uint64_t* __restrict__ off, uint64_t m, uint64_t rate, unsigned shift,
                                                                const T* __restrict__ pos, const T* __restrict__ len, uint64_t q,
                                                                uint64_t* __restrict__ start, uint64_t* __restrict__ segs) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= q; j += stride) {
        uint64_t cl = 0, sg = 0;
        if (j < q) {
            const uint64_t a = (uint64_t)pos[j], l = (uint64_t)len[j];
            if (a < n) {
                uint64_t e = off ? off[occ_last_le(off, m, a) + 1] : n;
                e = e < n ? e : n;
                if (e > a) cl = l < e - a ? l : e - a;
                if (cl) sg = fm_block_of(a + cl - 1, rate, shift) - fm_block_of(a, rate, shift) + 1;
            }
        }
        start[j] = cl;
        segs[j] = sg;
    }
}

// The functor of occ_tile_walk for the extraction: slot o is segment o - first of query x, the part of [a, b) = [pos[x], pos[x] +
// clipped length) inside block k = a / rate + (o - first).  The lane starts at the sample of position P = min((k + 1) * rate, e) - 1, e
// the end of the string of a; the sample is clamped to n; the head symbol of that rank is the last c <= sigma with C[c] <= rank, by a
// search of the table in LDS; then it steps P - lo < min(rate, n) times to the left, lo = max(a, k * rate), and stores the bytes whose
// position lies below hi = min(b, (k + 1) * rate).  A sample of n, a head symbol 0, STOP, a code beyond sigma or a rank of n ends the
// walk: the positions not reached get byte 0.  Slot and sample index stay inside by construction: k < blocks where (k + 1) * rate <= e
// <= n, the string of a is below max(m, 1), and out[start[x] + (p - a)] with p < b lies below start[x + 1].
template <typename T>
struct FmExtract {
    FmLayout Y;
    const uint64_t* s_tab;
    const uint8_t* s_dec;
    const T* __restrict__ ts;
    uint64_t blocks, rate;
    unsigned shift;
    const uint64_t* __restrict__ off;
    uint64_t m;
    const T* __restrict__ pos;
    const uint64_t* __restrict__ start;
    uint8_t* __restrict__ out;
    __device__ __forceinline__ void operator()(uint64_t o, uint64_t x, uint64_t first) const {
        const uint64_t n = Y.n, a = (uint64_t)pos[x], base = start[x], b = a + (start[x + 1] - base);
        if (a >= n || b > n || b <= a) return;          // (not with the starts this call has scanned)
        const uint64_t k = fm_block_of(a, rate, shift) + (o - first);
        const uint64_t s = off ? occ_last_le(off, m, a) : 0;
        uint64_t e = off ? off[s + 1] : n;
        e = e < n ? e : n;
        const uint64_t blo = k * rate, bhi = blo + rate;
        const uint64_t lo = a > blo ? a : blo, hi = b < bhi ? b : bhi;
        if (blo >= b || e < b) return;                  // (the same)
        const bool inner = bhi <= e;
        const uint64_t P = (inner ? bhi : e) - 1;
        uint64_t r = (uint64_t)ts[inner ? k : blocks + s];
        r = r < n ? r : n;
        unsigned c = r < n ? (unsigned)occ_last_le(s_tab + FM_TAB_C, (uint64_t)Y.sigma + 1, r) : 0u;
        bool live = c != 0;
        for (uint64_t p = P;; --p) {
            if (p < hi) out[base + (p - a)] = live ? s_dec[c] : (uint8_t)0;
            if (p == lo) break;
            if (live) {
                uint64_t at_r;
                c = fm_symbol_rank(Y, s_tab, r, at_r);
                live = c != 0 && c <= Y.sigma;
                if (live) { r = at_r + s_tab[FM_TAB_D + c]; live = r < n; }
            }
        }
    }
};

// out[start_x + t] = S[pos_x + t] for every query x and t below its clipped length; tiles of segments as fm_occ_kernel has tiles of slots
template <typename T>
__global__ __launch_bounds__(256) void fm_extract_kernel(FmLayout Y, FmDecode dec, const T* __restrict__ ts, uint64_t blocks, uint64_t rate, unsigned shift,
                                                         const uint64_t* __restrict__ off, uint64_t m, const T* __restrict__ pos, uint64_t q,
                                                         const uint64_t* __restrict__ start, const uint64_t* __restrict__ segs, uint64_t nsegs,
                                                         uint8_t* __restrict__ out) {
    __shared__ uint64_t s_seg[OCC_CHUNK + 1];
    __shared__ uint64_t s_tab[FM_TAB_WORDS];
    __shared__ uint8_t s_dec[FM_SYMS];
    for (uint64_t i = threadIdx.x; i < FM_TAB_WORDS; i += blockDim.x) s_tab[i] = Y.fm[Y.tab + i];
    for (uint64_t i = threadIdx.x; i < FM_SYMS; i += blockDim.x) s_dec[i] = dec.b[i];
    __syncthreads();
    const FmExtract<T> walk{Y, s_tab, s_dec, ts, blocks, rate, shift, off, m, pos, start, out};
    for (uint64_t o0 = (uint64_t)blockIdx.x * OCC_TILE; o0 < nsegs; o0 += (uint64_t)gridDim.x * OCC_TILE) {
        const uint64_t o1 = o0 + OCC_TILE < nsegs ? o0 + OCC_TILE : nsegs;
        occ_tile_walk(segs, q, o0, o1, s_seg, walk);
    }
}

} // namespace psacx
