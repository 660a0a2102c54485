// scan.hpp -- exclusive prefix sums in place of an array resident in HBM: what turns the key counts into the lookup table
// (lookup_table.hpp) and the interval counts into the starts of the occurrence lists (occurrences.hpp).
#pragma once
#include "engine.hpp"

namespace psacx {

#define LOCATE_SCAN_ITEMS 16              // entries per thread; a block of 256 threads scans 4096

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

// a[0..len) becomes its exclusive prefix sums; queued on the ctx stream.  The block sums live in the slab, which grows with len.
template <typename T>
int exclusive_scan_dev(psacx_ctx* c, T* d_a, uint64_t len) {
    const uint64_t nb = (len + 256 * LOCATE_SCAN_ITEMS - 1) / (256 * LOCATE_SCAN_ITEMS);
    PSACX_TRY(ensure_slab(c, nb * sizeof(unsigned long long) + 4096));
    unsigned long long* d_sums = reinterpret_cast<unsigned long long*>(c->slab);
    hipLaunchKernelGGL((scan_sums_kernel<T>), dim3((unsigned)nb), dim3(256), 0, c->stream, (const T*)d_a, len, d_sums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(256), 0, c->stream, d_sums, nb);
    hipLaunchKernelGGL((scan_apply_kernel<T>), dim3((unsigned)nb), dim3(256), 0, c->stream, d_a, len, (const unsigned long long*)d_sums);
    PSACX_HIP(c, hipGetLastError());
    return PSACX_OK;
}

} // namespace psacx
