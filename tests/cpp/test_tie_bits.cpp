// The rules of psac_amd/csrc/tie_bits.hpp on the host (no GPU), against brute force:
//   - the words put together row by row (tests/cpp/tie_bits_model.hpp: words_by_rows, the way of group_sort16_kernel<.., BITS>) are the words of the
//     definition, bit by bit, whatever the order the batches are merged in -- batches that start and end inside a word, a tied pair across the
//     places 63 | 64 of a batch and across a word border, the last record of a batch tied, batches of one record, equal prefixes on both sides of
//     a batch border (no bit), first places from 2^32 on;
//   - tie_leaders and tie_group_length find the groups a walk over the bits finds: every leader, its length up to TIE_GROUP_MAX, longer as longer.
// Plain C++11; tests/test_tie_bits_cpu.py builds it, once more with -fsanitize=address,undefined, and runs both.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include "tie_bits_model.hpp"

using namespace tie_bits_model;

static uint64_t mix(uint64_t& state) {          // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++failures > 20) std::exit(1); } } while (0)

// records in sorted order whose prefixes (above sfield) repeat with probability 1 / spread; the suffix fields are all different
static std::vector<uint64_t> sorted_records(unsigned n, int sfield, unsigned spread, uint64_t seed) {
    std::vector<uint64_t> rec(n);
    uint64_t prefix = 1;
    for (unsigned i = 0; i < n; ++i) {
        if (mix(seed) % spread) ++prefix;
        rec[i] = prefix << sfield | ((mix(seed) & 0xFFFFFFull) << 8 | (i & 255));
    }
    return rec;
}

static void check_words(const char* name, const std::vector<uint64_t>& rec, uint64_t origin, const std::vector<Span>& batches, int sfield, uint64_t seed) {
    const std::vector<uint64_t> want = words_brute(rec, origin, batches, sfield);
    std::vector<unsigned> order(batches.size());
    for (unsigned i = 0; i < order.size(); ++i) order[i] = i;
    for (int turn = 0; turn < 3; ++turn) {
        if (turn == 1) std::reverse(order.begin(), order.end());
        if (turn == 2) for (size_t p = order.size(); p > 1; --p) std::swap(order[p - 1], order[mix(seed) % p]);
        const std::vector<uint64_t> got = words_by_rows(rec, origin, batches, sfield, order);
        CHECK(got.size() == want.size(), "%s: %zu words against %zu", name, got.size(), want.size());
        for (size_t i = 0; i < want.size() && i < got.size(); ++i)
            CHECK(got[i] == want[i], "%s, order %d, word %zu: %016llx, the definition gives %016llx", name, turn, i, (unsigned long long)got[i], (unsigned long long)want[i]);
    }
    uint64_t set = 0;
    for (uint64_t w : want) set += (uint64_t)__builtin_popcountll(w);
    std::printf("ok   %-34s %zu records from place %llu, %zu batches, %llu bits\n", name, rec.size(), (unsigned long long)origin, batches.size(), (unsigned long long)set);
}

// the groups of a bit stream by a walk over its bits, against tie_leaders / tie_group_length
static void check_groups(const char* name, const std::vector<uint64_t>& words, uint64_t nplaces) {
    std::vector<uint64_t> leaders;
    std::vector<unsigned> lengths;
    for (uint64_t p = 0; p + 1 < nplaces; ++p)
        if (!psacx::tie_bit(words.data(), p) && psacx::tie_bit(words.data(), p + 1)) {
            unsigned len = 1;
            while (p + len < nplaces && psacx::tie_bit(words.data(), p + len)) ++len;
            leaders.push_back(p); lengths.push_back(len);
        }
    size_t at = 0;
    unsigned longest = 0;
    for (uint64_t w = 0; w * 64 < nplaces; ++w) {
        const unsigned next0 = (w + 1) * 64 < nplaces ? (unsigned)(words[w + 1] & 1) : 0u;
        uint64_t lead = psacx::tie_leaders(words[w], next0);
        while (lead) {
            const uint64_t q = w * 64 + (unsigned)__builtin_ctzll(lead);
            lead &= lead - 1;
            CHECK(at < leaders.size() && leaders[at] == q, "%s: leader %llu is not the next one of the walk", name, (unsigned long long)q);
            if (at < leaders.size()) {
                const unsigned len = psacx::tie_group_length(words.data(), nplaces, q, psacx::TIE_GROUP_MAX);
                const unsigned want = std::min(lengths[at], psacx::TIE_GROUP_MAX + 1);
                CHECK(len == want, "%s: group at %llu has %u members, counted as %u", name, (unsigned long long)q, lengths[at], len);
                longest = std::max(longest, lengths[at]);
            }
            ++at;
        }
    }
    CHECK(at == leaders.size(), "%s: %zu leaders found, the walk finds %zu", name, at, leaders.size());
    std::printf("ok   %-34s %zu groups, the longest of %u\n", name, leaders.size(), longest);
}

int main() {
    uint64_t seed = 7;
    {
        // random batches of 1 .. 512 records from a place inside a word; every third border between two batches has equal prefixes on both sides
        for (int sfield = 32; sfield <= 40; sfield += 8) {
            for (uint64_t origin : {(uint64_t)0, (uint64_t)37, (uint64_t)((1ull << 32) - 100), (uint64_t)((3ull << 31) + 63)}) {
                std::vector<uint64_t> rec = sorted_records(9001, sfield, 3, seed += 11);
                std::vector<Span> batches;
                uint64_t a = origin;
                while (a < origin + rec.size()) {
                    unsigned count = 1 + (unsigned)(mix(seed) % 512);
                    if (mix(seed) % 5 == 0) count = 1 + (unsigned)(mix(seed) % 3);
                    count = (unsigned)std::min<uint64_t>(count, origin + rec.size() - a);
                    if (a > origin && batches.size() % 3 == 0) rec[a - origin] = (rec[a - 1 - origin] >> sfield << sfield) | (rec[a - origin] & 0xFFFFFFFFull);
                    batches.push_back({a, count});
                    a += count;
                    if (mix(seed) % 7 == 0) a += mix(seed) % 70;          // (places no batch covers: a group the sort leaves alone)
                }
                while (!batches.empty() && batches.back().a + batches.back().count > origin + rec.size()) batches.pop_back();
                check_words(sfield == 32 ? "random batches, sfield 32" : "random batches, sfield 40", rec, origin, batches, sfield, seed);
            }
        }
    }
    {
        // every record equal: all bits but the first of every batch -- across 63 | 64 of a batch, across word borders, the last record
        std::vector<uint64_t> rec(2000);
        for (size_t i = 0; i < rec.size(); ++i) rec[i] = 0xABCDull << 32 | i;
        const std::vector<Span> batches = {{5, 385}, {390, 512}, {902, 64}, {966, 1}, {967, 65}, {1032, 128}, {1160, 129}, {1289, 511}, {1800, 200}};
        check_words("all equal", rec, 0, batches, 32, seed);
        const std::vector<uint64_t> w = words_brute(rec, 0, batches, 32);
        for (const Span& b : batches) {
            CHECK(!psacx::tie_bit(w.data(), b.a), "all equal: the first place %llu of a batch has a bit", (unsigned long long)b.a);
            for (unsigned i = 1; i < b.count; ++i) CHECK(psacx::tie_bit(w.data(), b.a + i), "all equal: place %llu has no bit", (unsigned long long)(b.a + i));
        }
    }
    {
        // groups of every length 2 .. 12 at every offset of a word, leaders at 63 mod 64, a group that ends at the last place
        const uint64_t nplaces = 64 * 800 + 17;
        std::vector<uint64_t> words((nplaces + 63) / 64 + 1, 0);
        uint64_t p = 3;
        for (unsigned len = 2; len <= 12; ++len)
            for (unsigned off = 0; off < 64 && p + 200 < nplaces; ++off) {
                while ((p & 63) != off) ++p;
                for (unsigned i = 1; i < len; ++i) words[(p + i) >> 6] |= 1ull << ((p + i) & 63);
                p += len + 1;
            }
        for (unsigned i = 1; i < 5; ++i) words[(nplaces - 5 + i) >> 6] |= 1ull << ((nplaces - 5 + i) & 63);
        check_groups("lengths 2 .. 12 at every offset", words, nplaces);
        // random streams, sparse and dense
        for (unsigned density : {200u, 8u, 2u}) {
            std::vector<uint64_t> rnd((nplaces + 63) / 64 + 1, 0);
            for (uint64_t q = 1; q < nplaces; ++q) if (mix(seed) % density == 0 || (density == 2 && mix(seed) % 3)) rnd[q >> 6] |= 1ull << (q & 63);
            check_groups(density == 200 ? "random bits, 1 in 200" : density == 8 ? "random bits, 1 in 8" : "random bits, dense", rnd, nplaces);
        }
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("tie bit tests passed\n");
    return 0;
}
