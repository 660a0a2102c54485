// overlaps.hpp -- the suffix-prefix overlaps of a string set from ISA, LCP, the range-minimum index of LCP and the bitmap of the
// string ends, all resident in HBM (include/psacx.h: "suffix-prefix overlaps").  The reference has no counterpart; kernel only, the
// calls are in rmq.hip.  The text is no argument.
//
// The overlaps of string j sit on the path from its leaf, rank r = ISA[o_j], to the root.  A step at depth d:
//  - i = olb(j, d) is r or the previous position with LCP <= d - 1 (rmq_last), the first suffix that starts with X(j, d);
//  - the slot is non-empty iff that suffix ends after d bytes: bit SA[i] + d of the bitmap;
//  - the suffixes that are X(j, d) are a run from i, since an end sorts below every character: its end is the first x whose bit
//    SA[x] + d is clear, searched in (i, hi) by a 16-way partition, lane t probing point t, one ballot per round;
//  - the next depth is LCP[i]: in between, olb stays i and SA[i] is longer, so those slots are empty and are not searched.
//
// Shape: RMQ_LANES = 16 lanes per string, as the queries of rmq.hpp; LCP[i] and SA[i] of a step leave together, the bitmap word
// depends on SA[i]: two dependent round trips per step plus the left search.  Lane 0 writes.  No LDS.
//
// Whatever the arrays hold: i stays below n, every SA entry is tested against n before it addresses the bitmap, d falls strictly
// from step to step (a step whose LCP[i] does not fall below d ends the walk), and a slot is written only below n.
#pragma once
#include "rmq.hpp"

namespace psacx {

constexpr uint32_t OVERLAP_WHOLE = 1u;                 // PSACX_OVERLAP_WHOLE

// does the suffix at s end after exactly d bytes, as far as the bitmap says?  (s + d > n: no, and nothing is read)
__device__ __forceinline__ bool overlap_ends_at(const uint32_t* __restrict__ ends, uint64_t n, uint64_t s, uint64_t d) {
    if (s > n || d > n - s) return false;
    const uint64_t p = s + d;
    return (ends[p >> 5] >> (p & 31)) & 1u;
}

// The first x in [lo, hi) whose suffix SA[x] does not end after d bytes, or hi: the predicate is monotone on a correct index.
// A round cuts the range into 16 pieces of w entries and probes the first entry of each; the piece after the last probe that
// holds is what is left, so the range shrinks below w = ceil(len / 16) and the loop ends whatever the probes say.
template <typename T>
__device__ __forceinline__ uint64_t overlap_run_end(const T* __restrict__ SA, const uint32_t* __restrict__ ends, uint64_t n, unsigned sub,
                                                    uint64_t lo, uint64_t hi, uint64_t d) {
    const unsigned shift = (unsigned)lane_id() & ~(unsigned)(RMQ_LANES - 1);
    while (lo < hi) {
        const uint64_t w = (hi - lo + RMQ_LANES - 1) / RMQ_LANES;
        const uint64_t x = lo + (uint64_t)sub * w;
        const bool in = x < hi && overlap_ends_at(ends, n, (uint64_t)SA[x], d);
        const unsigned held = (unsigned)(__ballot(in) >> shift) & ((1u << RMQ_LANES) - 1u);
        const unsigned f = (unsigned)__ffs((int)~held) - 1u;         // the first probe that does not hold, 16 if all do
        if (f == 0) return lo;
        const uint64_t next = lo + (uint64_t)f * w;                  // probe f, where there is one
        lo += (uint64_t)(f - 1) * w + 1;
        if (f < (unsigned)RMQ_LANES && next < hi) hi = next;
    }
    return lo;
}

template <typename T>
__global__ __launch_bounds__(256) void overlaps_kernel(uint64_t n, const uint64_t* __restrict__ off, uint64_t m, const uint32_t* __restrict__ ends,
                                                       const T* __restrict__ SA, const T* __restrict__ ISA, const T* __restrict__ LCP,
                                                       const T* __restrict__ index, uint64_t min_len, uint32_t flags, T* __restrict__ out_lb,
                                                       T* __restrict__ out_ub) {
    RmqLayout Y;
    rmq_layout(n, Y);
    const unsigned sub = threadIdx.x % RMQ_LANES;
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / RMQ_LANES;
    const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / RMQ_LANES;
    for (uint64_t j = group; j < m; j += ngroups) {
        const uint64_t o = off[j], oe = off[j + 1];
        if (o >= oe || oe > n) continue;                               // (the call has checked the offsets)
        const uint64_t len = oe - o;
        const uint64_t r = (uint64_t)ISA[o];
        if (r >= n) continue;
        uint64_t i = r;
        uint64_t d = (flags & OVERLAP_WHOLE) ? len : len - 1;
        while (d >= min_len && d >= 1) {
            uint64_t lcp = (uint64_t)LCP[i], s = (uint64_t)SA[i];
            if (lcp >= d) {
                i = rmq_last<T>(LCP, index, Y, sub, i, (T)(d - 1), n);
                if (i >= n) break;                                     // no previous value <= d - 1
                lcp = (uint64_t)LCP[i]; s = (uint64_t)SA[i];
                if (lcp >= d) break;                                   // no index of these values
            }
            if (overlap_ends_at(ends, n, s, d)) {
                uint64_t hi = r;
                if (d == len) {                                        // the whole string: the run may pass r
                    hi = r + 1 < n ? rmq_first<T>(LCP, index, Y, sub, r + 1, n, (T)(d - 1), n) : n;
                }
                if (hi < i + 1) hi = i + 1;
                const uint64_t ub = overlap_run_end<T>(SA, ends, n, sub, i + 1, hi, d);
                const uint64_t p = o + d - 1;
                if (sub == 0 && p < n) { out_lb[p] = (T)i; out_ub[p] = (T)ub; }
            }
            d = lcp;                                                   // (< d: the walk ends after at most len steps)
        }
    }
}

} // namespace psacx
