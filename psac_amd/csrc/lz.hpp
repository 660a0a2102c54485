// lz.hpp -- the longest-previous-factor array and the greedy LZ77 parse of one text from SA, LCP and the range-minimum index of
// LCP, all resident in HBM, and the round-trip check of a parse against the text (include/psacx.h: "LZ77 factorization").  The
// reference has no counterpart; kernels only, the calls are in lz.hip.  The text is an argument of the check alone.
//
// LPF.  For rank r with i = SA[r] the two candidates are the nearest ranks p < r < q whose SA entry is below i: nearest smaller
// values of SA on both sides (launch_ansv_tiles over SA itself).  lpf_kernel takes RMQ_LANES = 16 lanes per rank, as rmq_kernel:
// two rmq_min over LCP, [p + 1, r + 1) and [r + 1, q + 1), one SA fetch for the winner, and lane 0 stores LPF and SRC at slot i.
// A rank without a factor stores nothing (the call has cleared both arrays), so ranks that share a slot -- no SA has them --
// can only mix two valid pairs.
//
// Parse.  The phrase starts are the path from 0 to n in the forest next(i) = i + len(i), len(i) = min(max(1, LPF[i]), n - i).
// Tiles of B positions, groups of G tiles (LzGeometry).
//  1. lz_exit_kernel: a workgroup per group goes through its tiles from the last to the first.  A tile's next() is brought into
//     LDS and doubled log2(B) times, after which every position holds its exit, the first chain position at or behind the tile's
//     end; an exit inside the group is replaced by that position's group exit, which the step before has written.  G dependent
//     tile-wide gathers per workgroup, all groups in parallel.
//  2. lz_top_kernel: one lane walks the group exits from 0 and leaves each group's entry: ceil(n / (B G)) dependent loads.
//  3. lz_mark_kernel: a workgroup per entered group goes through its tiles from the first to the last; in a tile that holds the
//     running position the same doubling carries a mark along (after round k the first 2^(k+1) chain positions are marked), and
//     the running position becomes its exit.  G dependent tile loads per workgroup.
//  4. the tile counts are scanned and the marked positions and their sources are written in order: the compaction of select.hpp, whose
//     functor here is LzEmit.
// No kernel holds a chain of dependent global loads longer than max(G, ceil(n / (B G))) (+ the scan's own).
//
// Check.  check_lz77_kernel: one lane per text position finds its phrase by a binary search in start and compares its byte with
// the byte at the same offset of the source; one lane per phrase checks the order of the starts and the shape of the phrase.
#pragma once
#include "rmq.hpp"
#include "select.hpp"

namespace psacx {

constexpr int LZ_TILE_MAX = 1024;                      // B: positions of a tile, at most
constexpr int LZ_PER = LZ_TILE_MAX / 256;              // tile positions a thread of the doubling rounds owns
static_assert((unsigned)LZ_TILE_MAX <= SELECT_TILE_MAX, "the compaction takes a tile per workgroup");

struct LzGeometry {
    unsigned B, G, rounds;                             // rounds = ceil(log2(B))
};

// default: B = 1024, G = 128; small (PSACX_OPT_LZ_SMALL_TILES, tests): B = 64, G = 4, every level at n of a few hundred
inline LzGeometry lz_geometry(bool small) {
    LzGeometry g;
    g.B = small ? 64u : (unsigned)LZ_TILE_MAX;
    g.G = small ? 4u : 128u;
    g.rounds = 0;
    while ((1u << g.rounds) < g.B) ++g.rounds;
    return g;
}

template <typename T>
__global__ __launch_bounds__(256) void lpf_kernel(uint64_t n, const T* __restrict__ SA, const T* __restrict__ LCP, const T* __restrict__ index,
                                                  const uint64_t* __restrict__ left, const uint64_t* __restrict__ right, T* __restrict__ lpf,
                                                  T* __restrict__ src) {
    RmqLayout Y;
    rmq_layout(n, Y);
    const unsigned sub = threadIdx.x % RMQ_LANES;
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / RMQ_LANES;
    const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / RMQ_LANES;
    for (uint64_t r = group; r < n; r += ngroups) {
        const uint64_t i = (uint64_t)SA[r];
        if (i >= n) continue;
        const uint64_t p = left[r], q = right[r];
        const bool has_p = p < r, has_q = q > r && q < n;                  // (anything else: "none", whatever the neighbour arrays hold)
        T lp = 0, lq = 0;
        if (has_p) lp = rmq_min<T>(LCP, index, Y, sub, p + 1, r + 1);
        if (has_q) lq = rmq_min<T>(LCP, index, Y, sub, r + 1, q + 1);
        if (sub != 0) continue;
        uint64_t len = 0, w = n;
        if (lp >= lq && lp > 0) { len = (uint64_t)lp; w = p; }
        else if (lq > 0) { len = (uint64_t)lq; w = q; }
        if (w >= n) continue;
        const uint64_t s = (uint64_t)SA[w];
        if (s >= i) continue;                                               // (no SA of a text: the slot keeps 0, all ones)
        if (len > n - i) len = n - i;
        lpf[i] = (T)len;
        src[i] = (T)s;
    }
}

// next(i) of the parse, for i < n: in (i, n]
template <typename T>
__device__ __forceinline__ uint64_t lz_next(const T* __restrict__ lpf, uint64_t i, uint64_t n) {
    uint64_t len = (uint64_t)lpf[i];
    if (len < 1) len = 1;
    if (len > n - i) len = n - i;
    return i + len;
}

// E[j], j < B: next() of position ts + j (n where there is none).  After `rounds` doublings every entry is at or behind te.
template <typename T>
__device__ __forceinline__ void lz_tile_load(const T* __restrict__ lpf, uint64_t n, uint64_t ts, unsigned B, uint64_t* E) {
    for (unsigned j = threadIdx.x; j < B; j += blockDim.x) E[j] = ts + j < n ? lz_next<T>(lpf, ts + j, n) : n;
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(256) void lz_exit_kernel(const T* __restrict__ lpf, uint64_t n, LzGeometry geo, uint64_t ngroups, T* gexit) {
    __shared__ uint64_t E[LZ_TILE_MAX];
    const unsigned B = geo.B;
    const uint64_t span = (uint64_t)B * geo.G;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const uint64_t gs = g * span;
        const uint64_t ge = gs + span < n ? gs + span : n;
        const uint64_t tiles = (ge - gs + B - 1) / B;
        for (uint64_t t = tiles; t-- > 0;) {
            const uint64_t ts = gs + t * B;
            const uint64_t te = ts + B < n ? ts + B : n;
            lz_tile_load<T>(lpf, n, ts, B, E);
            for (unsigned k = 0; k < geo.rounds; ++k) {
                uint64_t e[LZ_PER];
#pragma unroll
                for (int d = 0; d < LZ_PER; ++d) {
                    const unsigned j = threadIdx.x + d * 256;
                    e[d] = j < B ? E[j] : n;
                    if (e[d] < te) e[d] = E[e[d] - ts];
                }
                __syncthreads();
#pragma unroll
                for (int d = 0; d < LZ_PER; ++d) { const unsigned j = threadIdx.x + d * 256; if (j < B) E[j] = e[d]; }
                __syncthreads();
            }
            for (unsigned j = threadIdx.x; j < B && ts + j < n; j += blockDim.x) {
                uint64_t x = E[j];
                if (x < ge) x = (uint64_t)gexit[x];                        // a later tile of this group: written one step ago
                gexit[ts + j] = (T)x;
            }
            __syncthreads();                                                // (the stores are visible to the workgroup; E is free again)
        }
    }
}

// gentry[g]: the chain position that enters group g, or all ones.  One lane.
template <typename T>
__global__ void lz_top_kernel(const T* __restrict__ gexit, uint64_t n, uint64_t span, uint64_t* __restrict__ gentry) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint64_t pos = 0;
    while (pos < n) {
        gentry[pos / span] = pos;
        const uint64_t nx = (uint64_t)gexit[pos];
        if (nx <= pos) break;                                               // (lz_exit_kernel writes nothing of the kind)
        pos = nx;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void lz_mark_kernel(const T* __restrict__ lpf, uint64_t n, LzGeometry geo, uint64_t ngroups,
                                                      const uint64_t* __restrict__ gentry, unsigned char* __restrict__ marks,
                                                      uint64_t* __restrict__ counts) {
    __shared__ uint64_t E[LZ_TILE_MAX];
    __shared__ unsigned char M[LZ_TILE_MAX];
    __shared__ unsigned cnt;
    const unsigned B = geo.B;
    const uint64_t span = (uint64_t)B * geo.G;
    for (uint64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        uint64_t pos = gentry[g];
        const uint64_t gs = g * span;
        const uint64_t ge = gs + span < n ? gs + span : n;
        if (pos < gs || pos >= ge) continue;                                // no phrase starts in this group
        const uint64_t tiles = (ge - gs + B - 1) / B;
        for (uint64_t t = (pos - gs) / B; t < tiles && pos < ge; ++t) {
            const uint64_t ts = gs + t * B;
            const uint64_t te = ts + B < n ? ts + B : n;
            if (pos >= te) continue;                                        // the chain passes over this tile
            for (unsigned j = threadIdx.x; j < B; j += blockDim.x) M[j] = ts + j == pos;
            if (threadIdx.x == 0) cnt = 0;
            lz_tile_load<T>(lpf, n, ts, B, E);
            for (unsigned k = 0; k < geo.rounds; ++k) {
                uint64_t e[LZ_PER], e2[LZ_PER];
                bool m[LZ_PER];
#pragma unroll
                for (int d = 0; d < LZ_PER; ++d) {
                    const unsigned j = threadIdx.x + d * 256;
                    e[d] = j < B ? E[j] : n;
                    m[d] = j < B && M[j];
                    e2[d] = e[d] < te ? E[e[d] - ts] : e[d];
                }
                __syncthreads();
#pragma unroll
                for (int d = 0; d < LZ_PER; ++d) {
                    const unsigned j = threadIdx.x + d * 256;
                    if (j >= B) continue;
                    if (m[d] && e[d] < te) M[e[d] - ts] = 1;
                    E[j] = e2[d];
                }
                __syncthreads();
            }
            unsigned mine = 0;
            for (unsigned j = threadIdx.x; j < B; j += blockDim.x) {
                const unsigned char v = M[j];
                if (v) { marks[ts + j] = 1; ++mine; }                      // (the call has cleared marks, whole tiles of them)
            }
            mine = wave_reduce<uint32_t>(mine, OpSum());
            if (lane_id() == 0 && mine) atomicAdd(&cnt, mine);
            const uint64_t nx = E[pos - ts];                                // the exit of the running position
            __syncthreads();
            if (threadIdx.x == 0) counts[ts / B] = cnt;
            pos = nx > pos ? nx : n;
            __syncthreads();
        }
    }
}

// The functor of select_emit_kernel: start[k], psrc[k] of the k-th marked position (psrc == nullptr: the starts alone); start[z] = n.
template <typename T>
struct LzEmit {
    const T* __restrict__ lpf;
    const T* __restrict__ src;
    uint64_t n;
    T* __restrict__ start;
    T* __restrict__ psrc;
    __device__ __forceinline__ void operator()(uint64_t at, uint64_t pos) const {
        start[at] = (T)pos;
        if (psrc) psrc[at] = lpf[pos] == 0 ? ~(T)0 : src[pos];
    }
    __device__ __forceinline__ void finish(uint64_t z) const { start[z] = (T)n; }
};

// the phrase of position x: the largest k < z with start[k] <= x as a bisection finds it (k = 0 where there is none); z >= 1
template <typename T>
__device__ __forceinline__ uint64_t lz_phrase_of(const T* __restrict__ start, uint64_t z, uint64_t x) {
    uint64_t lo = 0, hi = z;                           // start[lo] <= x < start[hi] where the starts ascend
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)start[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

// errors += the violations of a parse (include/psacx.h lists them); items 0 .. max(n, z + 1): item x is text position x and phrase x
template <typename T>
__global__ __launch_bounds__(256) void check_lz77_kernel(const uint8_t* __restrict__ text, uint64_t n, const T* __restrict__ start,
                                                         const T* __restrict__ psrc, uint64_t z, unsigned long long* __restrict__ errors) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t items = n > z + 1 ? n : z + 1;
    unsigned bad = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < items; x += stride) {
        if (x == 0 && (uint64_t)start[0] != 0) ++bad;
        if (x == z && (uint64_t)start[z] != n) ++bad;
        if (x < z) {                                    // phrase x
            const uint64_t a = (uint64_t)start[x], b = (uint64_t)start[x + 1];
            const T s = psrc[x];
            if (b <= a) ++bad;
            else if (s == ~(T)0 && b - a != 1) ++bad;
            if (s != ~(T)0 && (uint64_t)s >= a) ++bad;
        }
        if (x < n) {                                    // text position x
            bool ok = false;
            if (z > 0) {
                const uint64_t k = lz_phrase_of<T>(start, z, x);
                const uint64_t a = (uint64_t)start[k], b = (uint64_t)start[k + 1];
                if (a <= x && x < b) {                  // (x - a + s < x < n: the source byte is inside the text)
                    const T s = psrc[k];
                    ok = s == ~(T)0 || (uint64_t)s >= a || text[(uint64_t)s + (x - a)] == text[x];
                }
            }
            if (!ok) ++bad;
        }
    }
    bad = wave_reduce<uint32_t>(bad, OpSum());
    if (lane_id() == 0 && bad) atomicAdd(errors, (unsigned long long)bad);
}

} // namespace psacx
