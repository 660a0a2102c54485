// sort_scratch.hpp -- where the radix sorter keeps its tables: the scratch of a three-kernel pass, of the bucket passes over one-word
// records, how much of it a sort allocates, and the sorter's words in the ctx's pinned host memory.  Plain C++ without a HIP header, so
// that a host compiler can include it (tests/cpp/test_sort_scratch.cpp checks the layouts against the allocation bounds on the CPU).
// Every size and offset of these tables is written down here and nowhere else.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace psacx {

constexpr int RADIX_BITS = 8;
constexpr int RADIX = 1 << RADIX_BITS;
constexpr int MAX_PASSES = 2 * (64 / RADIX_BITS);   // two 64-bit key words
constexpr int SLAB_TILES = 64;                       // tiles per slab of the three-kernel offset scan (smallest slab)
// Very long inputs use longer slabs: the scan over the slab totals is one workgroup walking them one after the other
// (1.7 ms per pass at 2^20 tiles with 64-tile slabs, 2 % of a 4 GiB construction), the scan inside a slab runs in
// parallel over slabs.
// (a slab is one workgroup walking its tiles one after the other, the slab totals one workgroup walking the slabs: measured with
//  both sizes in one process, 2^29 64-bit records (2^17 tiles): 4.3 ms of histogram + scans per sort with slabs of 1024 tiles,
//  3.2 with 256 or 128; 2^32 records (2^20 tiles): 29.1 with 1024, 28.1 with 512, 31.3 with 128)
inline unsigned slab_tiles_for(uint64_t ntiles) { return ntiles > (1u << 19) ? 512u : ntiles > (1u << 16) ? 256u : (unsigned)SLAB_TILES; }

constexpr int SORT_TILE_MIN = 2048;   // smallest tile of any scatter configuration
constexpr uint64_t SMALL_SORT_MAX = 1ull << 21;   // below: single-sweep scatter passes with decoupled look-back
constexpr int GROUP_CAP = 512;        // longest group group_sort16_kernel orders on chip (radix.hpp)
constexpr unsigned ONEW_SUB = RADIX * RADIX;        // sub-buckets of the group form at 32 prefix bits in the word
constexpr size_t SLAB_INFO_BYTES = 32;              // sizeof(SlabInfo) (radix.hpp asserts it)
constexpr size_t SCRATCH_COUNTER_BYTES = 256;     // every layout below starts with the tile counter of its scatter kernels, a word with 256 bytes to itself
inline size_t scratch_up(size_t x) { return (x + 255) & ~(size_t)255; }

// ---- three-kernel pass: the tile counter, the per-tile histograms, the slab totals behind them
struct PassScratch {
    unsigned* counter; unsigned* tile_hist; unsigned long long* slab_tot;
    uint64_t ntiles, nslabs; unsigned slab_tiles;
    size_t bytes;            // from `base` to the end of the slab totals
};
inline PassScratch pass_scratch(char* base, uint64_t ntiles) {
    PassScratch p;
    p.ntiles = ntiles; p.slab_tiles = slab_tiles_for(ntiles); p.nslabs = (ntiles + p.slab_tiles - 1) / p.slab_tiles;
    const size_t tot = SCRATCH_COUNTER_BYTES + scratch_up(ntiles * RADIX * sizeof(unsigned));
    p.counter = reinterpret_cast<unsigned*>(base);
    p.tile_hist = reinterpret_cast<unsigned*>(base + SCRATCH_COUNTER_BYTES);
    p.slab_tot = reinterpret_cast<unsigned long long*>(base + tot);
    p.bytes = tot + p.nslabs * RADIX * sizeof(unsigned long long);
    return p;
}

// what a sort of n records allocates (SortScratch::d_desc): room for pass_scratch of any tile shape, or the look-back descriptors
inline size_t sort_desc_bytes(uint64_t n) {
    const uint64_t nt = (n + SORT_TILE_MIN - 1) / SORT_TILE_MIN + 1;
    // look-back descriptors, or (three-kernel form) per-tile counters + per-slab totals
    size_t b = 1024 + nt * RADIX * sizeof(uint64_t) + (nt / SLAB_TILES + 2) * RADIX * sizeof(uint64_t);
    // small sorts (look-back form): one descriptor region per pass, so that one memset serves the whole sort
    if (n < SMALL_SORT_MAX) b = std::max<size_t>(b, (size_t)MAX_PASSES * (512 + nt * RADIX * sizeof(uint32_t)));
    return b;
}
// ---- bucket passes over one-word records (engine.hpp: onew_bucket_passes).  Byte offsets from the scratch base, in the order they lie, the
// tile counter at 0; need = the end of the last region.  Without the group form a layout ends behind tabs: the offsets from max_word on equal need.
struct OneWordLayout {
    unsigned slab; uint64_t total_slabs, vtiles;
    bool group;              // the group form of onew_bucket_passes may run (onew_group_layout)
    uint64_t sub_tiles;      // rows of the tile tables its sub-bucket passes need (0: none)
    size_t tile_hist;        // rows of RADIX counts: the tiles of the 256 buckets, or of the sub-buckets if those are more
    size_t slab_tot, base2;  // the slab totals of the 256-bucket form; the RADIX x RADIX digit starts of every bucket
    size_t tabs, slab_info;  // bucket_off[257], slab_start[257] (OneWordTabs); slab_info[total_slabs] at the next multiple of 32
    size_t max_word, zero_row;                           // group form: the largest group (two words); a row of zeros, the slab row of every sub-bucket
    size_t sub_off, first_tile, tile_sub, group_base, need;     // with sub_tiles: the 65 537 starts of the sub-buckets, their first tiles, the sub-bucket of every tile, the 2^24 group starts
};
inline void onew_place(OneWordLayout& l) {
    l.tile_hist = SCRATCH_COUNTER_BYTES;
    l.slab_tot = l.tile_hist + scratch_up((size_t)std::max(l.vtiles, l.sub_tiles) * RADIX * sizeof(unsigned));
    l.base2 = l.slab_tot + scratch_up((size_t)l.total_slabs * RADIX * sizeof(unsigned long long));
    l.tabs = l.base2 + (size_t)RADIX * RADIX * 8;
    l.slab_info = l.tabs + ((2 * (RADIX + 1) * sizeof(unsigned long long) + 31) & ~(size_t)31);
    l.max_word = l.tabs + scratch_up(2 * (RADIX + 1) * sizeof(unsigned long long) + 64 + l.total_slabs * SLAB_INFO_BYTES);
    l.zero_row = l.group ? l.max_word + 256 : l.max_word;
    l.sub_off = l.group ? l.zero_row + (size_t)RADIX * 8 : l.max_word;
    l.first_tile = l.sub_tiles ? l.sub_off + scratch_up((size_t)(ONEW_SUB + 1) * 8) : l.sub_off;
    l.tile_sub = l.sub_tiles ? l.first_tile + scratch_up((size_t)(ONEW_SUB + 1) * 4) : l.sub_off;
    l.group_base = l.sub_tiles ? l.tile_sub + scratch_up((size_t)l.sub_tiles * 4) : l.sub_off;
    l.need = l.sub_tiles ? l.group_base + (size_t)ONEW_SUB * RADIX * 8 : l.sub_off;
}
// The 256-bucket form.  h_tabs: bucket_off[0 .. 256] filled in (start of every bucket's records; buckets without records own nothing),
// slab_start[0 .. 256] behind it is written here: every bucket owns whole slabs of tiles.
template <int TILE>
inline OneWordLayout onew_layout(unsigned long long* h_tabs, uint64_t ntiles_hint) {
    OneWordLayout lay;
    lay.slab = ntiles_hint >= (1u << 16) ? 64u : 16u;
    uint64_t total_slabs = 0;
    for (int d = 0; d < RADIX; ++d) {
        const uint64_t cnt = h_tabs[d + 1] - h_tabs[d];
        h_tabs[RADIX + 1 + d] = total_slabs;
        total_slabs += ((cnt + TILE - 1) / TILE + lay.slab - 1) / lay.slab;
    }
    h_tabs[2 * RADIX + 1] = total_slabs;
    lay.total_slabs = total_slabs; lay.vtiles = total_slabs * lay.slab;
    lay.group = false; lay.sub_tiles = 0;
    onew_place(lay);
    return lay;
}
// The group form of the bucket passes (onew_bucket_passes): the upper digits of the rest most significant digit first, the last 16 prefix bits
// ordered on chip inside the groups that agree in everything above them (radix.hpp: group_sort16_kernel).  It runs for 24 or 32 prefix bits in
// the word when a group is expected to hold at most half of GROUP_CAP records (texts of 2^22 .. 2^24 and of 2^30 .. 2^32 characters), and when the
// scratch has room for its tables behind those of the 256-bucket form: a word for the largest group, and at 32 bits the tables of the 65 536
// sub-buckets (radix.hpp: OneWordTabs) -- their starts, first tiles, the sub-bucket of every tile, a row of zeros, the 2^24 group starts -- and
// tile histograms of n / tile + 65 536 rows.  Returns `lay` with the form switched on, or `lay` as it is.
template <int TILE>
inline OneWordLayout onew_group_layout(const OneWordLayout& lay, uint64_t nrec, unsigned low, size_t scratch_bytes) {
    if ((low != 24 && low != 32) || (nrec >> (low - 16 + 8)) > (uint64_t)GROUP_CAP / 2) return lay;
    OneWordLayout g = lay;
    g.group = true;
    if (low == 32) g.sub_tiles = nrec / TILE + ONEW_SUB;            // (every sub-bucket owns ceil(size / tile) tiles)
    onew_place(g);
    return (g.need > scratch_bytes || g.sub_tiles >= (1ull << 31)) ? lay : g;
}
// ---- upper bounds of the one-word layouts, for the callers that allocate before the bucket sizes are known
// What carve (construct.hpp) adds to sort_desc_bytes(n) with PSACX_OPT_FIRST_LEAD = 40 below 2^30 characters: a small text sorted on 40
// leading bits needs the sub-bucket tables of a large one (tile histograms of n / tile + 65 536 rows, the 2^24 group starts, the rest in 8 MiB)
inline size_t onew_sub_bucket_supplement(uint64_t n) {
    return (size_t)(n / SORT_TILE_MIN + ONEW_SUB) * RADIX * sizeof(unsigned) + (size_t)ONEW_SUB * RADIX * 8 + (8u << 20);
}
// The multi-GPU engine (multi_first_round.hpp: sort_first_one_word) allocates a rank's scratch before the buckets are dealt.  multi_bucket_bound: the 256-bucket layout of the
// largest share a rank of m characters accepts (m + m / 8 + 256 + a tile of records: its tiles and 64 more per bucket, slabs of 16); multi_top_digit_bound: pass_scratch of the rank's ntiles, or the probe's table.
template <int TILE>
inline size_t multi_bucket_bound(uint64_t m) {
    const uint64_t cap_rec = m + m / 8 + 256 + (uint64_t)TILE;
    const uint64_t vt_ub = (cap_rec + TILE - 1) / TILE + (uint64_t)RADIX * 64 + 64;
    return 256 + scratch_up((size_t)vt_ub * RADIX * sizeof(unsigned)) + scratch_up((size_t)(vt_ub / 16 + RADIX) * RADIX * 8) +
           (size_t)RADIX * RADIX * 8 + 2 * (RADIX + 1) * 8 + 64 + (size_t)(vt_ub / 16 + RADIX) * SLAB_INFO_BYTES + 4096;
}
inline size_t multi_top_digit_bound(uint64_t ntiles, uint64_t probe_slots) {
    return 256 + std::max<size_t>(scratch_up((size_t)ntiles * RADIX * sizeof(unsigned)) + (ntiles / slab_tiles_for(ntiles) + 2) * RADIX * 8, probe_slots * 8) + 4096;
}
// ---- the sorter's words in ctx->pinned (byte offsets).  ensure_pinned is asked for PINNED_SORT_BYTES + 4096 at least.
constexpr size_t PINNED_SORT_BYTES = 2 * sizeof(unsigned long long) * MAX_PASSES * RADIX;
constexpr size_t PIN_TIE_BIG = 64;           // construct.hpp: a word -- the long tie groups of the first round; later the probe of a round's neighbours
constexpr size_t PIN_OVER = 96;              // construct.hpp: two words of a refinement round
constexpr size_t PIN_LIGHT = 112;            // construct.hpp: a word of the heavy / light split
constexpr size_t PIN_ID = 128;               // construct.hpp: one entry of Bsa
constexpr size_t PIN_SUMMARY = 256;          // SortScratch::h_summary, 4 words
constexpr size_t PIN_CONST_DIGITS = 384;     // MAX_PASSES flags radix_hist_scan_kernel stores: the passes whose digit is constant
constexpr size_t PIN_HIST = 1024;            // SortScratch::h_hist [MAX_PASSES][RADIX]; before the sorts the character histogram; class_partition's starts
constexpr size_t PIN_BASE = PIN_HIST + sizeof(unsigned long long) * MAX_PASSES * RADIX;        // SortScratch::h_base [MAX_PASSES][RADIX]
constexpr size_t PIN_TABS = PIN_BASE + (size_t)RADIX * 8;            // prefix_sort_1w: bucket_off[257], slab_start[257] behind the 256 digit starts read back
constexpr size_t PIN_GROUP_WORD = PIN_BASE + 4 * (size_t)RADIX * 8;  // prefix_sort_1w: the largest group (behind the tables)
constexpr size_t PIN_MULTI = 32768;          // the multi-GPU engine's read-back words (at most 2048 bytes)
static_assert(PIN_TIE_BIG + 8 <= PIN_OVER && PIN_OVER + 16 <= PIN_LIGHT && PIN_LIGHT + 8 <= PIN_ID && PIN_ID + 8 <= PIN_SUMMARY, "the words of a refinement round");
static_assert(PIN_SUMMARY + 4 * 8 <= PIN_CONST_DIGITS && PIN_CONST_DIGITS + MAX_PASSES * 4 <= PIN_HIST, "pair_sort: summary, constant-digit flags, histograms");
static_assert(PIN_TABS + 2 * (RADIX + 1) * 8 <= PIN_GROUP_WORD && PIN_GROUP_WORD + 8 <= PIN_HIST + PINNED_SORT_BYTES, "prefix_sort_1w: digit starts, bucket tables, group word inside h_base");
static_assert(PIN_BASE == PIN_HIST + PINNED_SORT_BYTES / 2, "h_hist and h_base fill what ensure_pinned is asked for behind PIN_HIST");
// May overlap: PIN_TABS and PIN_GROUP_WORD lie inside h_base -- the stream has consumed prefix_sort_1w's tables before the host-side scan of a later pair_sort fills h_base.
// May overlap: PIN_MULTI starts inside h_hist and runs on into h_base -- the multi engine reads its words back between the sorts, never during one.

}  // namespace psacx
