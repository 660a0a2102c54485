// docs.hpp -- document counts and document lists over a string set: in how many strings, and in which, the suffixes of an interval of the
// generalized suffix array start (include/psacx.h: "document counts and document lists").  The reference has no counterpart; kernels
// only, the calls are in docs.hip.
//
// Index.  doc_keys_kernel: one rank per lane, the key (doc(r), r) from one SA entry (streamed) and one search of the offsets.  The
// rank-pair sort orders the keys by their first word and keeps the ranks of a string in ascending order (it is stable and the second word
// is not a key).  Neighbours of equal doc in the sorted keys are the pairs (p, r), p = prev[r].
//  - doc_prev_kernel: one sorted key per lane.  prev[r] = p or all ones; an adjacent pair (p = r - 1) has its minimum at r and adds to
//    h[r] at once.
//  - doc_pairs_kernel: RMQ_LANES = 16 lanes per sorted key, as rmq_kernel.  Every other pair asks rmq_min and rmq_first for the first
//    minimum x of L[p + 1 .. r]; lane 0 adds to h[x] by one vector atomic.
// h lives in the caller's dup[] (n + 1 entries, cleared first), whose exclusive scan (scan.hpp) is dup.
//
// Counts.  doc_count_kernel: one interval per lane, two fetches.
//
// Lists.  The candidates are the ranks of all intervals, numbered through the scan of the interval lengths.  doc_mark_kernel walks its
// tiles by occ_tile_walk (occurrences.hpp): a workgroup owns OCC_TILE candidates, whatever the intervals are, and marks those whose prev
// lies in front of their interval.  doc_tile_kernel counts the marks of a tile and of each run of 64 candidates in front of it inside its tile;
// doc_start_kernel reads the number of marks in front of an interval's first candidate from them (the tile sums after their scan, one
// run count and at most 63 mark bytes).  The ordered compaction of select.hpp hands the marked candidates to DocListEmit, which fetches
// SA and searches the offsets.
#pragma once
#include "occurrences.hpp"
#include "rmq.hpp"
#include "select.hpp"

namespace psacx {

constexpr int DOC_RUN = 64;                            // candidates of a run count of the lists: OCC_TILE / DOC_RUN counts per tile

// k1[r] = doc(r) = the largest s < m with off[s] <= SA[r] (0 if there is none: the offsets are only searched), k2[r] = r
template <typename T>
__global__ __launch_bounds__(256) void doc_keys_kernel(const T* __restrict__ SA, uint64_t n, const uint64_t* __restrict__ off, uint64_t m,
                                                       T* __restrict__ k1, T* __restrict__ k2) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        k1[r] = (T)occ_last_le(off, m, (uint64_t)SA[r]);
        k2[r] = (T)r;
    }
}

__device__ __forceinline__ void doc_add(uint32_t* cell) { atomicAdd(cell, 1u); }
__device__ __forceinline__ void doc_add(uint64_t* cell) { atomicAdd(reinterpret_cast<unsigned long long*>(cell), 1ull); }

// k1 / k2: the sorted keys.  prev[k2[i]] = k2[i - 1] where k1[i] == k1[i - 1], else all ones; h[r] += 1 for a pair (r - 1, r).
// A second word that is no rank below n (no output of this sort) is passed over.  prev or h may be nullptr.
template <typename T>
__global__ __launch_bounds__(256) void doc_prev_kernel(const T* __restrict__ k1, const T* __restrict__ k2, uint64_t n, T* __restrict__ prev,
                                                       T* __restrict__ h) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t r = (uint64_t)k2[i];
        if (r >= n) continue;
        T p = ~(T)0;
        if (i >= 1 && k1[i] == k1[i - 1]) p = k2[i - 1];
        if (prev) prev[r] = p;
        if (h && p != ~(T)0 && (uint64_t)p + 1 == r) doc_add(h + r);
    }
}

// h[x] += 1 for every pair (p, r) of the sorted keys with p + 1 < r, x = the first minimum of L[p + 1 .. r]
template <typename T>
__global__ __launch_bounds__(256) void doc_pairs_kernel(const T* __restrict__ k1, const T* __restrict__ k2, uint64_t n, const T* __restrict__ LCP,
                                                        const T* __restrict__ index, T* __restrict__ h) {
    RmqLayout Y;
    rmq_layout(n, Y);
    const unsigned sub = threadIdx.x % RMQ_LANES;
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / RMQ_LANES;
    const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / RMQ_LANES;
    for (uint64_t i = group + 1; i < n; i += ngroups) {
        if (k1[i] != k1[i - 1]) continue;
        const uint64_t p = (uint64_t)k2[i - 1], r = (uint64_t)k2[i];
        if (r >= n || p >= r || p + 1 == r) continue;                       // (p < r < n: what the sort leaves; an adjacent pair is doc_prev_kernel's)
        const T v = rmq_min<T>(LCP, index, Y, sub, p + 1, r + 1);
        const uint64_t x = rmq_first<T>(LCP, index, Y, sub, p + 1, r + 1, v, n);
        if (sub == 0 && x < n) doc_add(h + x);                              // (x == n: the index is none of these values)
    }
}

// docs[j] = (ub - lb) - min(sat(dup[ub] - dup[lb + 1]), ub - lb - 1) if lb < ub <= n, else 0
template <typename T>
__global__ __launch_bounds__(256) void doc_count_kernel(uint64_t n, const T* __restrict__ dup, const T* __restrict__ lb, const T* __restrict__ ub,
                                                        uint64_t q, T* __restrict__ docs) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < q; j += stride) {
        const uint64_t a = (uint64_t)lb[j], b = (uint64_t)ub[j];
        uint64_t d = 0;
        if (a < b && b <= n) {
            const uint64_t hi = (uint64_t)dup[b], lo = (uint64_t)dup[a + 1];      // a + 1 <= b <= n: inside the n + 1 entries
            uint64_t dd = hi > lo ? hi - lo : 0;
            if (dd > b - a - 1) dd = b - a - 1;
            d = (b - a) - dd;
        }
        docs[j] = (T)d;
    }
}

// marks[o] = 1 iff candidate o, rank r = lb_x + (o - cstart[x]) of interval x, has prev[r] < lb_x or all ones, for o < total.  cstart[0 .. q]:
// the scan of the counts occ_counts_kernel took from lb / ub, which ends with total.
template <typename T>
__global__ __launch_bounds__(256) void doc_mark_kernel(const T* __restrict__ prev, const T* __restrict__ lb, const uint64_t* __restrict__ cstart,
                                                       uint64_t q, uint64_t total, unsigned char* __restrict__ marks) {
    __shared__ uint64_t s_start[OCC_CHUNK + 1];
    for (uint64_t o0 = (uint64_t)blockIdx.x * OCC_TILE; o0 < total; o0 += (uint64_t)gridDim.x * OCC_TILE) {
        const uint64_t o1 = o0 + OCC_TILE < total ? o0 + OCC_TILE : total;
        occ_tile_walk(cstart, q, o0, o1, s_start, [&](uint64_t o, uint64_t x, uint64_t first) {
            const uint64_t a = (uint64_t)lb[x];
            const T p = prev[a + (o - first)];                              // the rank is < ub <= n: the counts came from these entries
            marks[o] = (p == ~(T)0 || (uint64_t)p < a) ? 1 : 0;
        });
    }
}

// counts[t] = the marks of tile t; runs[t * (OCC_TILE / DOC_RUN) + w] = the marks of tile t in front of its run w of DOC_RUN candidates.
// marks holds whole tiles.
static __global__ __launch_bounds__(256) void doc_tile_kernel(const unsigned char* __restrict__ marks, uint64_t ntiles, uint64_t* __restrict__ counts,
                                                       uint32_t* __restrict__ runs) {
    static_assert(OCC_TILE == 256 * SELECT_PER && DOC_RUN % SELECT_PER == 0, "every thread counts one word");
    constexpr unsigned PER_RUN = DOC_RUN / SELECT_PER;                      // threads of a run
    __shared__ uint32_t sh[256 / WAVE + 1];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t word = *reinterpret_cast<const uint32_t*>(marks + t * OCC_TILE + threadIdx.x * SELECT_PER) & 0x01010101u;
        uint32_t total;
        const uint32_t before = block_scan_exclusive<256, uint32_t>((uint32_t)__popc(word), OpSum(), 0u, sh, &total);
        if (threadIdx.x % PER_RUN == 0) runs[t * (OCC_TILE / DOC_RUN) + threadIdx.x / PER_RUN] = before;
        if (threadIdx.x == 0) counts[t] = total;
    }
}

// start[j] = the marks in front of candidate cstart[j], j <= q.  counts: the exclusive sums of the tile counts, ntiles + 1 entries.
static __global__ __launch_bounds__(256) void doc_start_kernel(const uint64_t* __restrict__ cstart, uint64_t q, uint64_t total,
                                                        const unsigned char* __restrict__ marks, uint64_t ntiles, const uint64_t* __restrict__ counts,
                                                        const uint32_t* __restrict__ runs, uint64_t* __restrict__ start) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j <= q; j += stride) {
        const uint64_t o = cstart[j];
        uint64_t s = counts[ntiles];
        if (o < total) {
            const uint64_t run = o / DOC_RUN;
            s = counts[o / OCC_TILE] + runs[run];
            const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(marks + run * DOC_RUN);
            const unsigned in = (unsigned)(o % DOC_RUN);
            for (unsigned k = 0; k * 4 < in; ++k) {
                uint32_t word = w[k] & 0x01010101u;
                if (in - k * 4 < 4) word &= (1u << (8 * (in - k * 4))) - 1u;
                s += (uint64_t)__popc(word);
            }
        }
        start[j] = s;
    }
}

// The functor of select_emit_kernel: the k-th marked candidate o gives pos[k] = SA[r] and sid[k] = its string (m for a pos >= n)
template <typename T>
struct DocListEmit {
    const T* __restrict__ SA;
    uint64_t n;
    const uint64_t* __restrict__ off;
    uint64_t m;
    const T* __restrict__ lb;
    const uint64_t* __restrict__ cstart;
    uint64_t q;
    T* __restrict__ sid;
    T* __restrict__ pos;
    __device__ __forceinline__ void operator()(uint64_t at, uint64_t o) const {
        const uint64_t x = occ_last_le(cstart, q + 1, o);
        if (x >= q) return;
        const uint64_t r = (uint64_t)lb[x] + (o - cstart[x]);
        const uint64_t p = r < n ? (uint64_t)SA[r] : n;
        sid[at] = (T)(p >= n ? m : occ_last_le(off, m, p));
        if (pos) pos[at] = (T)p;
    }
    __device__ __forceinline__ void finish(uint64_t) const {}
};

} // namespace psacx
