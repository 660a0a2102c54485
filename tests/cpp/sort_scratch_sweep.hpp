// The sizes and bucket distributions tests/cpp/test_sort_scratch.cpp sweeps, and the format of a recorded line: `name|v v v ...`.
// The program that recorded tests/golden/sort_scratch_layout.json from the parent commit's engine.hpp walked the same sweep.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

namespace sweep {

constexpr int NB = 256;                                  // buckets of the top digit
constexpr int TILE_1W = 4096;                            // tile of the bucket passes (engine.hpp: 512 x PSACX_1W_ITEMS)
const int PASS_TILES[2] = {512 * 12, 512 * 8};           // ScatterCfg: 32-bit and 64-bit words

// n of the pass layout and of sort_desc_bytes: the ends, the tile of the smallest configuration, the steps of slab_tiles_for
// (2^16 and 2^19 tiles of either shape), SMALL_SORT_MAX, and the large texts
inline std::vector<uint64_t> pass_sizes() {
    std::vector<uint64_t> v = {1, 2047, 2048, 1ull << 16, (1ull << 21) - 1, 1ull << 21, 1ull << 30, 1ull << 32, 1ull << 34, 1ull << 35};
    for (int t = 0; t < 2; ++t)
        for (int sh = 16; sh <= 19; sh += 3)
            for (int d = -1; d <= 1; ++d) v.push_back(((uint64_t)PASS_TILES[t] << sh) + (uint64_t)(int64_t)d);
    return v;
}
// records of a one-word sort (one GPU) / characters of a rank's block (multi-GPU engine)
inline std::vector<uint64_t> onew_sizes() {
    return {4097, (1ull << 22) + 1234, (1ull << 23) + 4100, (1ull << 24) - 1, 1ull << 28, (1ull << 30) - 1, 1ull << 30, 1ull << 32};
}
inline std::vector<uint64_t> block_sizes() { return {128, 4096, (1ull << 20) + 7, 1ull << 24, 1ull << 28, 1ull << 30, 1ull << 32, 1ull << 34}; }

inline uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

const char* const DIST[5] = {"one_bucket", "even", "one_per_bucket", "geometric", "random"};
// bucket_off[0 .. 256] of n records in distribution d; one_per_bucket ignores n (256 records).  Returns the number of records.
inline uint64_t fill(int d, uint64_t n, unsigned long long* off) {
    uint64_t cnt[NB];
    for (int b = 0; b < NB; ++b) cnt[b] = 0;
    if (d == 0) cnt[137] = n;
    else if (d == 1) for (int b = 0; b < NB; ++b) cnt[b] = n / NB + ((uint64_t)b < n % NB ? 1 : 0);
    else if (d == 2) for (int b = 0; b < NB; ++b) cnt[b] = 1;
    else if (d == 3) {
        uint64_t left = n;
        for (int b = 0; b < NB && b < 63; ++b) { cnt[b] = n >> (b + 1); left -= cnt[b]; }
        cnt[0] += left;
    } else {
        uint64_t s = 12345, w[NB], W = 0, left = n;
        for (int b = 0; b < NB; ++b) { const uint64_t x = splitmix(s); w[b] = (x & 7) == 0 ? 0 : (x >> 8) % 1000 + 1; W += w[b]; }
        for (int b = 0; b < NB; ++b) { cnt[b] = (uint64_t)((unsigned __int128)n * w[b] / W); left -= cnt[b]; }
        cnt[0] += left;
    }
    uint64_t at = 0;
    for (int b = 0; b < NB; ++b) { off[b] = at; at += cnt[b]; }
    off[NB] = at;
    return at;
}

inline void line(const char* name, const std::vector<uint64_t>& v) {
    std::printf("%s|", name);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%llu", i ? " " : "", (unsigned long long)v[i]);
    std::printf("\n");
}

}  // namespace sweep
