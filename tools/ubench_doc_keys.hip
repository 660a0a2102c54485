// The first stage of psacx_doc_index_dev_* two ways: doc(r) of every rank by the binary search over the offsets (doc_keys_kernel of
// docs.hpp, as the library runs it) and by a rank directory over the bitmap of the string starts (RankDir / rank_bits of repeats.hpp: one
// directory entry and one bitmap word).  n = 2^LOGN positions in m = 2^LOGM strings of equal length, SA a permutation that scatters
// neighbouring ranks over the text (r times an odd constant, mod n), uint32.  Prints both times, the bytes each form keeps beside the
// offsets, and checks that the keys agree.  The directory form needs the bitmap, its popcounts and their scan first; that build is timed too.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -Ipsac_amd/csrc -o tools/ubench_doc_keys tools/ubench_doc_keys.hip ; tools/ubench_doc_keys [LOGN (28)] [LOGM (21)]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "docs.hpp"
#include "repeats.hpp"

using namespace psacx;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ __launch_bounds__(256) void make_sa_kernel(uint32_t* sa, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) sa[r] = (uint32_t)((r * 2654435761ull) & (n - 1));
}

// bit p of the bitmap: a string starts at p > 0; cnt[w] = the bits of word w
__global__ __launch_bounds__(256) void start_bits_kernel(const uint64_t* __restrict__ off, uint64_t m, uint64_t n, uint64_t* __restrict__ bits,
                                                         uint64_t* __restrict__ cnt) {
    const uint64_t words = (n >> 6) + 1, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += stride) {
        // the offsets inside [64 w, 64 w + 64): found by one search, then walked
        uint64_t word = 0;
        uint64_t s = occ_last_le(off, m, w << 6);
        if (off[s] < (w << 6) || s == 0) ++s;
        for (; s < m && off[s] < ((w + 1) << 6); ++s) word |= 1ull << (off[s] & 63);
        bits[w] = word;
        cnt[w] = (uint64_t)__popcll(word);
    }
}

// one block: cnt[0 .. words) become their exclusive prefix sums (a plain loop of block scans; the build is not what is measured closely)
__global__ __launch_bounds__(1024) void dir_scan_kernel(uint64_t* cnt, uint64_t words) {
    __shared__ uint64_t sh[1024];
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < words; b0 += 1024) {
        const uint64_t i = b0 + threadIdx.x, v = i < words ? cnt[i] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (unsigned d = 1; d < 1024; d <<= 1) {
            const uint64_t add = threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < words) cnt[i] = carry + sh[threadIdx.x] - v;
        carry += sh[1023];
        __syncthreads();
    }
}

// k1[r] = the string starts in (0, SA[r]] = doc(r), k2[r] = r
__global__ __launch_bounds__(256) void dir_keys_kernel(const uint32_t* __restrict__ SA, uint64_t n, RankDir R, uint32_t* __restrict__ k1,
                                                       uint32_t* __restrict__ k2) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        k1[r] = (uint32_t)rank_bits(R, (uint64_t)SA[r] + 1);
        k2[r] = (uint32_t)r;
    }
}

int main(int argc, char** argv) {
    const int logn = argc > 1 ? atoi(argv[1]) : 28, logm = argc > 2 ? atoi(argv[2]) : 21;
    if (logn < 8 || logn > 31 || logm < 0 || logm > logn) { std::fprintf(stderr, "usage: ubench_doc_keys [LOGN 8..31] [LOGM 0..LOGN]\n"); return 1; }
    const uint64_t n = 1ull << logn, m = 1ull << logm, words = (n >> 6) + 1;
    std::vector<uint64_t> off(m + 1);
    for (uint64_t s = 0; s <= m; ++s) off[s] = s << (logn - logm);
    uint32_t *sa, *k1, *k2, *j1, *j2;
    uint64_t *d_off, *bits, *dir;
    CK(hipMalloc(&sa, n * 4)); CK(hipMalloc(&k1, n * 4)); CK(hipMalloc(&k2, n * 4)); CK(hipMalloc(&j1, n * 4)); CK(hipMalloc(&j2, n * 4));
    CK(hipMalloc(&d_off, (m + 1) * 8)); CK(hipMalloc(&bits, (words + 1) * 8)); CK(hipMalloc(&dir, (words + 1) * 8));
    CK(hipMemcpy(d_off, off.data(), (m + 1) * 8, hipMemcpyHostToDevice));
    CK(hipMemset(bits, 0, (words + 1) * 8)); CK(hipMemset(dir, 0, (words + 1) * 8));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int grid = prop.multiProcessorCount * 8;
    hipLaunchKernelGGL(make_sa_kernel, dim3(grid), dim3(256), 0, 0, sa, n);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int reps = 7;
    float t[3][reps];
    for (int it = -1; it < reps; ++it) {
        float ms;
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL((doc_keys_kernel<uint32_t>), dim3(grid), dim3(256), 0, 0, (const uint32_t*)sa, n, (const uint64_t*)d_off, m, k1, k2);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        if (it >= 0) t[0][it] = ms;
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(start_bits_kernel, dim3(grid), dim3(256), 0, 0, (const uint64_t*)d_off, m, n, bits, dir);
        hipLaunchKernelGGL(dir_scan_kernel, dim3(1), dim3(1024), 0, 0, dir, words);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        if (it >= 0) t[1][it] = ms;
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(dir_keys_kernel, dim3(grid), dim3(256), 0, 0, (const uint32_t*)sa, n, RankDir{bits, dir}, j1, j2);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1)); CK(hipEventElapsedTime(&ms, e0, e1));
        if (it >= 0) t[2][it] = ms;
    }
    CK(hipGetLastError());
    std::vector<uint32_t> a(n), b(n);
    CK(hipMemcpy(a.data(), k1, n * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(b.data(), j1, n * 4, hipMemcpyDeviceToHost));
    uint64_t differ = 0;
    for (uint64_t r = 0; r < n; ++r) differ += a[r] != b[r];
    const char* names[3] = {"keys by the search of the offsets", "bitmap, popcounts and their scan", "keys by the rank directory"};
    std::printf("n = 2^%d positions in m = 2^%d strings, uint32, %d repeats, device %s\n", logn, logm, reps, prop.name);
    for (int k = 0; k < 3; ++k) {
        std::sort(t[k], t[k] + reps);
        std::printf("%-36s median %8.3f ms (least %8.3f, largest %8.3f)\n", names[k], t[k][reps / 2], t[k][0], t[k][reps - 1]);
    }
    std::printf("beside the offsets (%.1f MiB): nothing for the search; %.1f MiB of bitmap and directory for the other form\n", (m + 1) * 8 / 1048576.0,
                2.0 * words * 8 / 1048576.0);
    std::printf("keys that differ: %llu\n", (unsigned long long)differ);
    return differ ? 1 : 0;
}
