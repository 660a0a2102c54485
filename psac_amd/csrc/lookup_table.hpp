// lookup_table.hpp -- kernel of the k-mer lookup table in front of the pattern search (psacx_lookup_table_dev_*,
// psacx_lookup_table_gsa_dev_*): the counts of the keys; scan.hpp turns them into their exclusive prefix sums in place.
// include/psacx.h defines code(), key_k() and the table; tests/locate_model.py and tests/locate_gsa_model.py state them on the host.
//
// Stands in for lookup_index::construct (the reference's include/lookup_table.hpp:36-149: k-mer histogram + scan).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sa_kernels.hpp"

namespace psacx {

template <typename T> __device__ __forceinline__ void locate_count_add(T* p, unsigned long long v);
template <> __device__ __forceinline__ void locate_count_add<uint32_t>(uint32_t* p, unsigned long long v) { atomicAdd(p, (uint32_t)v); }
template <> __device__ __forceinline__ void locate_count_add<uint64_t>(uint64_t* p, unsigned long long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), v);
}

#define LOCATE_STRIP 16            // consecutive text positions per thread: their keys roll from one to the next
#define LOCATE_LDS_BINS 4096       // tables up to this many entries are counted in LDS first (a DNA table of k = 1 has 5 bins)

// key_k(i) of a string set, read character by character: code 0 from the end of i's string on.  room = characters from i to that
// end (anything above k where there are more).
__device__ __forceinline__ uint64_t kmer_key_cut(const uint8_t* __restrict__ text, uint64_t n, const uint16_t* s_code, uint32_t k, uint32_t B,
                                                 uint64_t i, unsigned room) {
    uint64_t key = 0;
    for (uint32_t j = 0; j < k; ++j) key = key * B + (j < room && i + j < n ? s_code[text[i + j]] : 0u);
    return key;
}

// table[key_k(i)] += 1 for every text position i; key_k reads code 0 past the end of the text.  top = B^(k-1).
// SET: the text is a string set and key_k reads code 0 past the end of i's string (psacx_lookup_table_gsa_dev_*); ends is the
// bitmap of psacx_string_ends_dev, (n >> 5) + 1 words.  A strip takes the 64 bits after its first position into a register
// (k <= 30, so they reach past the last character of its last key); the key still rolls from one position to the next, and is
// read afresh where a string starts.  Without SET, ends is not read.
template <typename T, bool IN_LDS, bool SET>
__global__ __launch_bounds__(256) void kmer_count_kernel(const uint8_t* __restrict__ text, uint64_t n, uint32_t k, uint32_t B, uint64_t top,
                                                         CodeTable code, T* __restrict__ table, uint64_t entries, const uint32_t* __restrict__ ends) {
    __shared__ uint16_t s_code[256];
    __shared__ unsigned long long s_bins[IN_LDS ? LOCATE_LDS_BINS : 1];
    s_code[threadIdx.x] = code.c[threadIdx.x];
    if (IN_LDS) for (uint64_t v = threadIdx.x; v < entries; v += blockDim.x) s_bins[v] = 0;
    __syncthreads();
    const uint64_t strips = (n + LOCATE_STRIP - 1) / LOCATE_STRIP, stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t st = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; st < strips; st += stride) {
        const uint64_t i0 = st * LOCATE_STRIP, i1 = i0 + LOCATE_STRIP < n ? i0 + LOCATE_STRIP : n;
        uint64_t key = 0;
        if (SET) {
            // bit t of win = bit i0 + 1 + t of the bitmap; i0 is a multiple of 16, so the shift is 1 or 17
            const uint64_t w = (i0 + 1) >> 5, words = (n >> 5) + 1;
            const unsigned sh = (unsigned)((i0 + 1) & 31);
            const uint64_t w0 = ends[w], w1 = w + 1 < words ? ends[w + 1] : 0u, w2 = w + 2 < words ? ends[w + 2] : 0u;
            const uint64_t win = (w0 >> sh) | (w1 << (32 - sh)) | (w2 << (64 - sh));
            key = kmer_key_cut(text, n, s_code, k, B, i0, win ? (unsigned)__builtin_ctzll(win) + 1u : 64u);
            for (uint64_t i = i0; i < i1; ++i) {
                if (IN_LDS) atomicAdd(&s_bins[key], 1ull); else locate_count_add<T>(&table[key], 1ull);
                const uint64_t after = win >> (i + 1 - i0);                 // bit t = bit i + 2 + t of the bitmap
                const unsigned room = after ? (unsigned)__builtin_ctzll(after) + 1u : 64u;      // characters from i + 1 to the end of its string
                if ((win >> (i - i0)) & 1) key = kmer_key_cut(text, n, s_code, k, B, i + 1, room);      // a string starts at i + 1
                else key = (key - (uint64_t)s_code[text[i]] * top) * B + (k - 1 < room && i + k < n ? s_code[text[i + k]] : 0u);
            }
            continue;
        }
        for (uint32_t j = 0; j < k; ++j) key = key * B + (i0 + j < n ? s_code[text[i0 + j]] : 0u);
        for (uint64_t i = i0; i < i1; ++i) {
            if (IN_LDS) atomicAdd(&s_bins[key], 1ull); else locate_count_add<T>(&table[key], 1ull);
            key = (key - (uint64_t)s_code[text[i]] * top) * B + (i + k < n ? s_code[text[i + k]] : 0u);
        }
    }
    if (IN_LDS) {
        __syncthreads();
        for (uint64_t v = threadIdx.x; v < entries; v += blockDim.x) if (s_bins[v]) locate_count_add<T>(&table[v], s_bins[v]);
    }
}

} // namespace psacx
