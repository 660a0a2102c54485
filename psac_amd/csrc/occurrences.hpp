// occurrences.hpp -- kernels of the occurrence lists (psacx_occurrences_dev_*): the counts of the intervals, whose exclusive prefix
// sums scan.hpp takes, and an output-balanced expansion.  include/psacx.h defines them ("occurrence lists");
// tests/locate_gsa_model.py states them on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psacx {

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

// The walk of a workgroup of 256 threads over the slots [o0, o1) of its tile, for kernels that number slots through start[0 .. q], the
// scan of q counts that ends with the number of slots (o1 at most that): f(o, x, first) once for every slot o, by one thread, where x
// is the interval that holds o and first = start[x].  One search in start[] per stretch of OCC_CHUNK intervals, one LDS search per slot
// (the comment of occ_expand_kernel below has the reasons).  s_start: OCC_CHUNK + 1 words of LDS.  Starts that do not ascend end the walk.
template <typename F>
__device__ __forceinline__ void occ_tile_walk(const uint64_t* __restrict__ start, uint64_t q, uint64_t o0, uint64_t o1, uint64_t* s_start, F f) {
    uint64_t open = o0;                                                     // the first slot not visited yet (the same in every thread)
    while (open < o1) {
        const uint64_t j0 = occ_last_le(start, q + 1, open);                // (start[q] > open, so j0 < q and interval j0 holds `open`)
        if (j0 >= q) break;
        const uint64_t cnt = q - j0 < OCC_CHUNK ? q - j0 : OCC_CHUNK;
        __syncthreads();
        for (uint64_t i = threadIdx.x; i <= cnt; i += blockDim.x) s_start[i] = start[j0 + i];
        __syncthreads();
        const uint64_t upto = s_start[cnt] < o1 ? s_start[cnt] : o1;
        if (upto <= open) break;
        for (uint64_t o = o0 + threadIdx.x; o < upto; o += blockDim.x) {
            if (o < open) continue;
            const uint64_t i = occ_last_le(s_start, cnt, o);
            f(o, j0 + i, s_start[i]);
        }
        open = upto;
    }
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
