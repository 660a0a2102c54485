// sort_scratch.hpp on the host: prints every layout and bound of the sweep (sort_scratch_sweep.hpp) as `name|values` lines --
// tests/test_sort_scratch_cpu.py compares them with the values recorded from the parent commit -- and checks here that the regions of
// every layout are disjoint and aligned, and that what the callers allocate covers what the layouts need.
// g++ -std=c++11 -Wall -Werror -I psac_amd/csrc
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sort_scratch.hpp"
#include "sort_scratch_sweep.hpp"

using namespace psacx;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } } while (0)

static char* const BASE = reinterpret_cast<char*>((uintptr_t)1 << 40);          // a scratch base (never dereferenced)
static size_t off_of(const void* p) { return (size_t)(reinterpret_cast<const char*>(p) - BASE); }
static bool al(size_t x) { return (x & 255) == 0; }

static void pass_layouts() {
    for (uint64_t n : sweep::pass_sizes()) {
        for (int t = 0; t < 2; ++t) {
            const uint64_t tile = (uint64_t)sweep::PASS_TILES[t], ntiles = (n + tile - 1) / tile;
            const PassScratch p = pass_scratch(BASE, ntiles);
            char name[96];
            std::snprintf(name, sizeof(name), "pass n=%llu tile=%llu", (unsigned long long)n, (unsigned long long)tile);
            sweep::line(name, {p.ntiles, p.slab_tiles, p.nslabs, off_of(p.tile_hist), off_of(p.slab_tot), p.bytes});
            CHECK(off_of(p.counter) == 0 && off_of(p.tile_hist) >= sizeof(unsigned), "%s", name);
            CHECK(al(off_of(p.tile_hist)) && al(off_of(p.slab_tot)), "%s", name);
            CHECK(off_of(p.tile_hist) + ntiles * RADIX * sizeof(unsigned) <= off_of(p.slab_tot), "%s", name);
            CHECK((uint64_t)p.slab_tiles * p.nslabs >= ntiles && off_of(p.slab_tot) + p.nslabs * RADIX * 8 == p.bytes, "%s", name);
            CHECK(p.bytes <= sort_desc_bytes(n), "%s: %llu bytes, sort_desc_bytes %llu", name, (unsigned long long)p.bytes, (unsigned long long)sort_desc_bytes(n));
        }
        char name[64];
        std::snprintf(name, sizeof(name), "desc n=%llu", (unsigned long long)n);
        sweep::line(name, {sort_desc_bytes(n)});
    }
}

// the regions of a one-word layout lie in order, apart, aligned as the kernels expect
static void check_regions(const OneWordLayout& l, const char* name) {
    CHECK(l.tile_hist == SCRATCH_COUNTER_BYTES, "%s", name);
    CHECK(al(l.tile_hist) && al(l.slab_tot) && al(l.base2) && al(l.tabs) && (l.slab_info & 31) == 0 && al(l.max_word) && al(l.zero_row) && al(l.sub_off) &&
          al(l.first_tile) && al(l.tile_sub) && al(l.group_base) && al(l.need), "%s", name);
    CHECK(l.tile_hist + std::max(l.vtiles, l.sub_tiles) * RADIX * sizeof(unsigned) <= l.slab_tot, "%s", name);
    CHECK(l.slab_tot + l.total_slabs * RADIX * 8 <= l.base2, "%s", name);
    CHECK(l.base2 + (size_t)RADIX * RADIX * 8 <= l.tabs, "%s", name);
    CHECK(l.tabs + 2 * (RADIX + 1) * 8 <= l.slab_info && l.slab_info + l.total_slabs * SLAB_INFO_BYTES <= l.max_word, "%s", name);
    if (!l.group) {
        CHECK(l.sub_tiles == 0 && l.zero_row == l.need && l.sub_off == l.need && l.first_tile == l.need && l.tile_sub == l.need && l.group_base == l.need && l.max_word == l.need, "%s", name);
        return;
    }
    CHECK(l.max_word + 16 <= l.zero_row && l.zero_row + (size_t)RADIX * 8 <= l.sub_off, "%s", name);
    if (l.sub_tiles) {
        CHECK(l.sub_off + (size_t)(ONEW_SUB + 1) * 8 <= l.first_tile && l.first_tile + (size_t)(ONEW_SUB + 1) * 4 <= l.tile_sub, "%s", name);
        CHECK(l.tile_sub + l.sub_tiles * 4 <= l.group_base && l.group_base + (size_t)ONEW_SUB * RADIX * 8 == l.need, "%s", name);
    } else
        CHECK(l.first_tile == l.sub_off && l.tile_sub == l.sub_off && l.group_base == l.sub_off && l.need == l.sub_off, "%s", name);
}

static void onew_layouts() {
    constexpr int TILE = sweep::TILE_1W;
    const size_t HUGE_ROOM = ~(size_t)0 >> 1;
    for (int d = 0; d < 5; ++d) {
        std::vector<uint64_t> sizes = sweep::onew_sizes();
        if (d == 2) sizes.assign(1, (uint64_t)sweep::NB);
        for (uint64_t n0 : sizes) {
            std::vector<unsigned long long> tabs(2 * (RADIX + 1), 0);
            const uint64_t n = sweep::fill(d, n0, tabs.data());
            const OneWordLayout lay = onew_layout<TILE>(tabs.data(), (n + TILE - 1) / TILE);
            uint64_t slabsum = 0;
            for (int b = 0; b <= RADIX; ++b) slabsum += (uint64_t)(b + 1) * tabs[RADIX + 1 + b];
            char name[128];
            std::snprintf(name, sizeof(name), "onew %s n=%llu", sweep::DIST[d], (unsigned long long)n);
            sweep::line(name, {lay.slab, lay.total_slabs, lay.vtiles, lay.tile_hist, lay.slab_tot, lay.base2, lay.tabs, lay.slab_info, lay.need, slabsum});
            check_regions(lay, name);
            CHECK(!lay.group && tabs[2 * RADIX + 1] == lay.total_slabs && lay.vtiles == lay.total_slabs * lay.slab, "%s", name);
            const size_t rooms[3] = {sort_desc_bytes(n), sort_desc_bytes(n) + onew_sub_bucket_supplement(n), HUGE_ROOM};
            const char* const room_names[3] = {"desc", "desc+supplement", "huge"};
            for (unsigned low = 16; low <= 32; low += 8)
                for (int r = 0; r < 3; ++r) {
                    const OneWordLayout g = onew_group_layout<TILE>(lay, n, low, rooms[r]);
                    std::snprintf(name, sizeof(name), "group %s n=%llu low=%u room=%s", sweep::DIST[d], (unsigned long long)n, low, room_names[r]);
                    std::vector<uint64_t> v = {g.group ? 1u : 0u, g.sub_tiles, g.slab_tot, g.base2, g.tabs, g.slab_info, g.need};
                    if (g.group) { v.push_back(g.max_word); v.push_back(g.zero_row); v.push_back(g.sub_off); v.push_back(g.first_tile); v.push_back(g.tile_sub); v.push_back(g.group_base); }
                    sweep::line(name, v);
                    check_regions(g, name);
                    CHECK(g.need <= rooms[r] || !g.group, "%s", name);
                    CHECK(g.group || g.need == lay.need, "%s", name);
                    // carve's supplement (PSACX_OPT_FIRST_LEAD = 40 below 2^30 characters) has room for the sub-bucket form of every distribution
                    if (low == 32 && r == 2 && n < (1ull << 30)) {
                        CHECK(g.group && g.sub_tiles, "%s", name);
                        CHECK(g.need <= rooms[1], "%s: need %llu, carve allocates %llu", name, (unsigned long long)g.need, (unsigned long long)rooms[1]);
                    }
                }
        }
    }
    for (uint64_t n : sweep::onew_sizes()) {
        char name[64];
        std::snprintf(name, sizeof(name), "supplement n=%llu", (unsigned long long)n);
        sweep::line(name, {onew_sub_bucket_supplement(n)});
    }
}

// what sort_first_one_word allocates per rank of m characters covers the pass on the top digit, the probe's table, and the bucket passes of
// the largest share it accepts in any distribution
static void multi_bounds() {
    constexpr int TILE = sweep::TILE_1W, TILE0 = 512 * 8;
    for (uint64_t m : sweep::block_sizes()) {
        const uint64_t stride = std::max<uint64_t>(64, m >> 20), samples = m / stride;
        uint64_t slots = 1; while (slots < 4 * samples) slots <<= 1;
        const uint64_t nrec[2] = {m, m - std::min<uint64_t>(m, 127)};            // (a block that holds the short suffixes of the text has fewer records)
        std::vector<uint64_t> v;
        for (int k = 0; k < 2; ++k) {
            const uint64_t ntiles0 = (nrec[k] + TILE0 - 1) / TILE0;
            const size_t a = multi_top_digit_bound(ntiles0, slots);
            v.push_back(a);
            CHECK(pass_scratch(BASE, ntiles0).bytes <= a && SCRATCH_COUNTER_BYTES + slots * 8 <= a, "m=%llu", (unsigned long long)m);
        }
        const size_t b = multi_bucket_bound<TILE>(m);
        v.push_back(b);
        char name[64];
        std::snprintf(name, sizeof(name), "multi m=%llu", (unsigned long long)m);
        sweep::line(name, v);
        const uint64_t share = m + m / 8 + 256 + TILE;
        for (int d = 0; d < 5; ++d) {
            std::vector<unsigned long long> tabs(2 * (RADIX + 1), 0);
            const uint64_t n = sweep::fill(d, share, tabs.data());
            const OneWordLayout lay = onew_layout<TILE>(tabs.data(), (n + TILE - 1) / TILE);
            CHECK(lay.need <= b, "m=%llu %s: need %llu, bound %llu", (unsigned long long)m, sweep::DIST[d], (unsigned long long)lay.need, (unsigned long long)b);
        }
    }
}

int main() {
    pass_layouts();
    onew_layouts();
    multi_bounds();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("sort scratch tests passed\n");
    return 0;
}
