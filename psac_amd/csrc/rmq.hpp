// rmq.hpp -- range-minimum and longest-common-extension queries over an array resident in HBM (include/psacx.h: "range minimum
// and longest common extension").  Stands in for rmq<>::query (the reference's include/rmq.hpp:186: the FIRST minimum of a range)
// and for the queries par_rmq.hpp answers per rank; kernels only, the calls are in rmq.hip.
//
// The index is the 64-ary min-pyramid of sa_kernels.hpp from level 1 upwards, each level with its running minima pre[] / suf[]
// (pyramid_level_kernel, pyramid_aux_kernel build it).  Level 0 is the caller's array.  The index holds values only: every
// address a query forms follows from lo, hi and n alone, so an index of random words cannot send a load out of range.
//
// Shape: RMQ_LANES = 16 lanes per query, four queries per wave.
//  - Above level 0 a range costs at most two loads per level (suf[l], pre[r-1]); lane t of the 16 owns load t, so the loads of all
//    levels leave together, one per lane.
//  - At level 0 (and on the one level where the range ends inside a single group) a group of 64 entries is 4 entries per lane:
//    one 16-byte load per lane for 32-bit entries, two for 64-bit ones.  Up to two such groups per query (left and right end).
//  - One wait, then a minimum over the 16 lanes by four xor-shuffles.
//  - The first minimum is found after the value v is known: lo itself if values[lo] <= v, else the nearest j > lo with
//    values[j] <= v -- the non-strict right search of nsv.hpp, a group per step, first qualifying position = minimum over lanes.
#pragma once
#include "engine.hpp"

namespace psacx {

constexpr int RMQ_LANES = 16;                   // lanes per query
constexpr int RMQ_PER = 64 / RMQ_LANES;         // entries of a 64-group per lane

// Where the levels lie in the index, as a function of n alone (host and device agree on it by construction).
// Level L in [1, nlev) has len[L] entries at lvl[L], pre[L], suf[L] (offsets in entries, each a multiple of 4).
struct RmqLayout {
    int nlev;                                   // levels including level 0; the top level is one group of <= 64 entries
    uint64_t len[PYR_MAX];
    uint64_t lvl[PYR_MAX], pre[PYR_MAX], suf[PYR_MAX];
    uint64_t entries;                           // >= 1
};

__host__ __device__ inline void rmq_layout(uint64_t n, RmqLayout& Y) {
    Y.nlev = 1; Y.len[0] = n; Y.lvl[0] = Y.pre[0] = Y.suf[0] = 0;
    for (int L = 1; L < PYR_MAX; ++L) { Y.len[L] = 0; Y.lvl[L] = Y.pre[L] = Y.suf[L] = 0; }
    uint64_t len = n, off = 0;
    while (len > 64 && Y.nlev < PYR_MAX) {
        len = (len + 63) >> 6;
        const uint64_t room = (len + 3) & ~3ull;
        const int L = Y.nlev++;
        Y.len[L] = len;
        Y.lvl[L] = off; Y.pre[L] = off + room; Y.suf[L] = off + 2 * room;
        off += 3 * room;
    }
    Y.entries = off ? off : 1;
}

template <typename T>
__device__ __forceinline__ T rmq_group_reduce(T v) {
#pragma unroll
    for (int m = RMQ_LANES / 2; m >= 1; m >>= 1) { const T o = shfl_xor<T>(v, m); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint64_t rmq_group_reduce_pos(uint64_t v) { return rmq_group_reduce<uint64_t>(v); }

// this lane's RMQ_PER entries of the 64-group `g` of a[0..len): entries g * 64 + sub * RMQ_PER + d; out of [0, len) -> all ones
template <typename T>
__device__ __forceinline__ void rmq_load_part(const T* __restrict__ a, uint64_t len, uint64_t g, unsigned sub, T (&x)[RMQ_PER]) {
    load_run<T, RMQ_PER>(a, (g << 6) + (uint64_t)sub * RMQ_PER, len, x, ~(T)0);
}

// minimum of this lane's part of group g restricted to positions [l, r)
template <typename T>
__device__ __forceinline__ T rmq_part_min(const T (&x)[RMQ_PER], uint64_t g, unsigned sub, uint64_t l, uint64_t r) {
    const uint64_t e0 = (g << 6) + (uint64_t)sub * RMQ_PER;
    T m = ~(T)0;
#pragma unroll
    for (int d = 0; d < RMQ_PER; ++d) if (e0 + d >= l && e0 + d < r && x[d] < m) m = x[d];
    return m;
}

// The minimum of values[l .. r), 0 <= l < r <= n, by the 16 lanes of one group (all of them call this with the same l, r).
// Loads: level 0 at most two groups; every level above at most two single entries, or one group where the range ends.
template <typename T>
__device__ __forceinline__ T rmq_min(const T* __restrict__ values, const T* __restrict__ index, const RmqLayout& Y, unsigned sub,
                                     uint64_t l, uint64_t r) {
    T m = ~(T)0;
    // level 0 and the level on which the range closes: whole groups, a part per lane
    T xa[RMQ_PER], xb[RMQ_PER], xw[RMQ_PER];
    uint64_t ga = 0, gb = 0, gw = 0, la = 0, ra = 0, lb = 0, rb = 0, lw = 0, rw = 0;
    bool has_a = false, has_b = false, has_w = false;
    const T* aw = values;
    uint64_t lenw = 0;
    T t = ~(T)0;                                       // this lane's single table entry
    bool done = false;
#pragma unroll
    for (int L = 0; L < PYR_MAX; ++L) {
        if (done || L >= Y.nlev) continue;
        const bool one = (l >> 6) == ((r - 1) >> 6);
        if (L == 0) {
            if (one) { has_a = true; ga = l >> 6; la = l; ra = r; done = true; }
            else {
                if (l & 63) { has_a = true; ga = l >> 6; la = l; ra = (ga + 1) << 6; }
                if (r & 63) { has_b = true; gb = r >> 6; lb = gb << 6; rb = r; }
            }
        } else if (one) {
            if ((l & 63) == 0) { if (sub == 2u * (L - 1)) t = index[Y.pre[L] + r - 1]; }
            else if ((r & 63) == 0) { if (sub == 2u * (L - 1)) t = index[Y.suf[L] + l]; }
            else { has_w = true; aw = index + Y.lvl[L]; lenw = Y.len[L]; gw = l >> 6; lw = l; rw = r; }
            done = true;
        } else {
            if ((l & 63) && sub == 2u * (L - 1)) t = index[Y.suf[L] + l];
            if ((r & 63) && sub == 2u * (L - 1) + 1u) t = index[Y.pre[L] + r - 1];
        }
        if (!done) { l = (l + 63) >> 6; r >>= 6; if (l >= r) done = true; }
    }
    if (has_a) rmq_load_part<T>(values, Y.len[0], ga, sub, xa);
    if (has_b) rmq_load_part<T>(values, Y.len[0], gb, sub, xb);
    if (has_w) rmq_load_part<T>(aw, lenw, gw, sub, xw);
    if (has_a) { const T v = rmq_part_min<T>(xa, ga, sub, la, ra); m = v < m ? v : m; }
    if (has_b) { const T v = rmq_part_min<T>(xb, gb, sub, lb, rb); m = v < m ? v : m; }
    if (has_w) { const T v = rmq_part_min<T>(xw, gw, sub, lw, rw); m = v < m ? v : m; }
    m = t < m ? t : m;
    return rmq_group_reduce<T>(m);
}

// first position p of group g of a[0..len) with from <= p < to and a[p] <= v, over the 16 lanes; ~0 if none
template <typename T>
__device__ __forceinline__ uint64_t rmq_first_le(const T* __restrict__ a, uint64_t len, uint64_t g, unsigned sub, uint64_t from, uint64_t to,
                                                 T v) {
    T x[RMQ_PER];
    rmq_load_part<T>(a, len, g, sub, x);
    if (to > len) to = len;
    const uint64_t e0 = (g << 6) + (uint64_t)sub * RMQ_PER;
    uint64_t p = ~0ull;
#pragma unroll
    for (int d = RMQ_PER - 1; d >= 0; --d) if (e0 + d >= from && e0 + d < to && x[d] <= v) p = e0 + d;
    return rmq_group_reduce_pos(p);
}

// The smallest position in [l, r) that holds a value <= v (v = the range's minimum), or n if the arrays offer none (they
// then are no index of each other).  The walk of nsv_search<T, false> with a group per step: up while the rest of the group
// holds nothing, then down into the first child that qualifies.  At most 2 nlev - 1 dependent group loads; none of the
// addresses comes from memory.
template <typename T>
__device__ __forceinline__ uint64_t rmq_first(const T* __restrict__ values, const T* __restrict__ index, const RmqLayout& Y, unsigned sub,
                                              uint64_t l, uint64_t r, T v, uint64_t n) {
    uint64_t p = l, j = ~0ull;
    int found = -1;                                    // the level j was found on
    bool open = true;
    // (both loops are unrolled with guards so that the layout stays in registers: a level indexed at run time would go to scratch)
#pragma unroll
    for (int L = 0; L < PYR_MAX; ++L) {
        if (!open || L >= Y.nlev) continue;
        const T* a = L ? index + Y.lvl[L] : values;
        // level 0 looks at [l, r) of l's group; above, at the entries after p's own (their blocks lie wholly behind l)
        const uint64_t from = L ? p + 1 : p;
        const uint64_t to = L ? Y.len[L] : r;
        j = rmq_first_le<T>(a, Y.len[L], p >> 6, sub, from, to, v);
        if (j != ~0ull) { found = L; open = false; }
        else if ((((p >> 6) + 1) << 6) >= to) open = false;       // nothing behind this group on this level
        p >>= 6;
    }
    if (found < 0) return n;
#pragma unroll
    for (int L = PYR_MAX - 1; L > 0; --L) {
        if (L > found || j == ~0ull) continue;                      // (j == ~0: the parent qualified, no child does -- no index of these values)
        const T* a = (L - 1) ? index + Y.lvl[L - 1] : values;
        j = rmq_first_le<T>(a, Y.len[L - 1], j, sub, 0, ~0ull, v);
    }
    return (j >= l && j < r) ? j : n;
}

// The left mirror of the two above.  Positions travel as p + 1 so that 0 is "none" and the group's answer is a maximum.
__device__ __forceinline__ uint64_t rmq_group_reduce_last(uint64_t v) {
#pragma unroll
    for (int m = RMQ_LANES / 2; m >= 1; m >>= 1) { const uint64_t o = shfl_xor<uint64_t>(v, m); v = o > v ? o : v; }
    return v;
}

// last position p of group g of a[0..len) with p < to and a[p] <= v, over the 16 lanes; ~0 if none
template <typename T>
__device__ __forceinline__ uint64_t rmq_last_le(const T* __restrict__ a, uint64_t len, uint64_t g, unsigned sub, uint64_t to, T v) {
    T x[RMQ_PER];
    rmq_load_part<T>(a, len, g, sub, x);
    if (to > len) to = len;
    const uint64_t e0 = (g << 6) + (uint64_t)sub * RMQ_PER;
    uint64_t p1 = 0;
#pragma unroll
    for (int d = 0; d < RMQ_PER; ++d) if (e0 + d < to && x[d] <= v) p1 = e0 + d + 1;
    return rmq_group_reduce_last(p1) - 1;                          // (0 - 1 = ~0: none)
}

// The largest position below i (0 <= i <= n) that holds a value <= v, or n if there is none: the previous value <= v, which in
// LCP is the step from a node of the suffix tree to the ancestor of depth <= v.  The walk of rmq_first turned round: up while
// the part of the group in front of p holds nothing, then down into the last child that qualifies.  At most 2 nlev - 1
// dependent group loads, one or two where the answer is near; none of the addresses comes from memory.
template <typename T>
__device__ __forceinline__ uint64_t rmq_last(const T* __restrict__ values, const T* __restrict__ index, const RmqLayout& Y, unsigned sub,
                                             uint64_t i, T v, uint64_t n) {
    if (i == 0 || i > n) return n;
    uint64_t p = i - 1, j = ~0ull;                      // p: the last candidate on level 0, the entry that holds it above
    int found = -1;
    bool open = true;
#pragma unroll
    for (int L = 0; L < PYR_MAX; ++L) {
        if (!open || L >= Y.nlev) continue;
        const T* a = L ? index + Y.lvl[L] : values;
        // level 0 looks at the group of p up to p itself; above, at the entries in front of p's own (their blocks lie wholly below i)
        j = rmq_last_le<T>(a, Y.len[L], p >> 6, sub, L ? p : p + 1, v);
        if (j != ~0ull) { found = L; open = false; }
        else if ((p >> 6) == 0) open = false;           // nothing in front of this group on this level
        p >>= 6;
    }
    if (found < 0) return n;
#pragma unroll
    for (int L = PYR_MAX - 1; L > 0; --L) {
        if (L > found || j == ~0ull) continue;          // (j == ~0: the parent qualified, no child does -- no index of these values)
        const T* a = (L - 1) ? index + Y.lvl[L - 1] : values;
        j = rmq_last_le<T>(a, Y.len[L - 1], j, sub, ~0ull, v);
    }
    return j < i ? j : n;
}

template <typename T>
__global__ __launch_bounds__(256) void rmq_kernel(const T* __restrict__ values, uint64_t n, const T* __restrict__ index,
                                                  const T* __restrict__ lo, const T* __restrict__ hi, uint64_t q,
                                                  T* __restrict__ out_min, T* __restrict__ out_arg) {
    RmqLayout Y;
    rmq_layout(n, Y);
    const unsigned sub = threadIdx.x % RMQ_LANES;
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / RMQ_LANES;
    const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / RMQ_LANES;
    for (uint64_t i = group; i < q; i += ngroups) {
        const uint64_t l = (uint64_t)lo[i];
        uint64_t r = (uint64_t)hi[i];
        if (r > n) r = n;
        T m = ~(T)0;
        uint64_t at = n;
        if (l < r) {
            m = rmq_min<T>(values, index, Y, sub, l, r);
            if (out_arg) at = rmq_first<T>(values, index, Y, sub, l, r, m, n);
        }
        if (sub == 0) {
            if (out_min) out_min[i] = m;
            if (out_arg) out_arg[i] = (T)at;
        }
    }
}

// end(p) of the set form: the smallest offset above p, clamped to (p, n]; p < n.  The offsets are only searched.
__device__ __forceinline__ uint64_t lce_string_end(const uint64_t* __restrict__ off, uint64_t m, uint64_t p, uint64_t n) {
    uint64_t lo = 0, hi = m + 1;                       // first index in [0, m] with off[idx] > p, or m + 1
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] > p) hi = mid; else lo = mid + 1;
    }
    uint64_t e = lo <= m ? off[lo] : n;
    if (e > n) e = n;
    if (e <= p) e = p + 1;
    return e;
}

// lce_0 of two distinct positions below n from the arrays: both ranks are asked for together, then one range minimum
template <typename T>
__device__ __forceinline__ uint64_t lce_zero(const T* __restrict__ ISA, const T* __restrict__ LCP, const T* __restrict__ index,
                                             const RmqLayout& Y, unsigned sub, uint64_t a, uint64_t b, uint64_t n) {
    uint64_t r = (uint64_t)ISA[a], s = (uint64_t)ISA[b];
    if (r >= n) r = n - 1;
    if (s >= n) s = n - 1;
    const uint64_t l = (r < s ? r : s) + 1, h = (r < s ? s : r) + 1;
    if (l >= h) return ~0ull;                          // equal ranks of distinct positions: no ISA; the caller clamps
    return (uint64_t)rmq_min<T>(LCP, index, Y, sub, l, h);
}

template <typename T, bool SET>
__global__ __launch_bounds__(256) void lce_kernel(uint64_t n, const uint64_t* __restrict__ off, uint64_t ms, const T* __restrict__ ISA,
                                                  const T* __restrict__ LCP, const T* __restrict__ index, const T* __restrict__ pa,
                                                  const T* __restrict__ pb, uint64_t q, uint64_t e, T* __restrict__ out) {
    RmqLayout Y;
    rmq_layout(n, Y);
    const unsigned sub = threadIdx.x % RMQ_LANES;
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / RMQ_LANES;
    const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / RMQ_LANES;
    for (uint64_t i = group; i < q; i += ngroups) {
        const uint64_t a = (uint64_t)pa[i], b = (uint64_t)pb[i];
        uint64_t d = 0;
        if (a < n && b < n) {
            const uint64_t room = n - (a > b ? a : b);
            if (a == b) {
                d = SET ? lce_string_end(off, ms, a, n) - a : room;
            } else if (e == 0) {
                // (the generalized LCP is cut at string ends: no end() here, in either form)
                d = lce_zero<T>(ISA, LCP, index, Y, sub, a, b, n);
                if (d > room) d = room;
            } else {
                uint64_t Lm = room;
                if (SET) {
                    const uint64_t ea = lce_string_end(off, ms, a, n) - a, eb = lce_string_end(off, ms, b, n) - b;
                    Lm = ea < eb ? ea : eb;            // (<= room: both ends are clamped to n)
                }
                uint64_t budget = e;
                for (;;) {                             // d grows by at least one per turn and stops at Lm
                    const uint64_t j = lce_zero<T>(ISA, LCP, index, Y, sub, a + d, b + d, n);
                    d = j > Lm - d ? Lm : d + j;
                    if (d >= Lm || budget == 0) break;
                    --budget; ++d;                     // the byte at d differs by definition: step over it
                    if (d >= Lm) break;
                }
            }
        }
        if (sub == 0) out[i] = (T)d;
    }
}

} // namespace psacx
