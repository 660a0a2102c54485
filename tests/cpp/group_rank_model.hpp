// Host model of group_sort16_kernel (psac_amd/csrc/radix.hpp) on the rule of psac_amd/csrc/group_rank.hpp: how a chunk of 64 groups is cut into
// batches, which batches take the way back to the counting rounds, and where the one counting round puts every record of a batch.  Shared by
// tests/cpp/test_group_rank.cpp (host only) and tests/cpp/group_sort16_direct.hip (against the kernel).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>
#include "group_rank.hpp"

namespace group_rank_model {

constexpr unsigned CAP = 512, CHUNK = 64;          // sort_scratch.hpp: GROUP_CAP; the groups a wave takes per trip

static inline uint64_t mix(uint64_t& state) {          // splitmix64
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Batch { uint64_t group, a; unsigned run, count; };          // first group, first record, groups, records

// the batches of the table `starts` (ngroups entries; the last group ends at nrec) in the order the kernel takes them; batch_cap: GROUP_RANK_BATCH in
// the form with one counting round (a single group up to CAP is then a batch of its own), CAP in the form of counting rounds only.
// Chunks whose starts are not monotone or leave [0, nrec] give no batch, groups longer than CAP neither.
static inline std::vector<Batch> cut(const std::vector<uint64_t>& starts, uint64_t nrec, unsigned batch_cap) {
    std::vector<Batch> out;
    const uint64_t ngroups = starts.size();
    for (uint64_t g0 = 0; g0 < ngroups; g0 += CHUNK) {
        uint64_t s[CHUNK + 1];
        for (unsigned l = 0; l <= CHUNK; ++l) s[l] = g0 + l < ngroups ? starts[g0 + l] : nrec;
        bool good = true;
        for (unsigned l = 0; l < CHUNK; ++l) good = good && s[l + 1] >= s[l] && s[l + 1] <= nrec;
        if (!good) continue;
        unsigned g = 0;
        while (g < CHUNK) {
            unsigned run = 0;
            while (g + run < CHUNK && s[g + run + 1] - s[g] <= batch_cap) ++run;
            if (run == 0 && batch_cap < CAP && s[g + 1] - s[g] <= CAP) run = 1;
            if (run == 0) { ++g; continue; }
            const unsigned count = (unsigned)(s[g + run] - s[g]);
            if (count) out.push_back({g0 + g, s[g], run, count});
            g += run;
        }
    }
    return out;
}

// the largest bucket of the one counting round on a batch
static inline unsigned largest_bucket(const uint64_t* rec, const Batch& b, int sfield) {
    const unsigned gbits = psacx::group_rank_gbits(b.run), first = (unsigned)b.group & 255u;
    unsigned cnt[256] = {0}, m = 0;
    for (unsigned p = 0; p < b.count; ++p) m = std::max(m, ++cnt[psacx::group_rank_bucket(psacx::group_rank_ckey(rec[p], sfield, first, gbits), gbits)]);
    return m;
}
// does the kernel order this batch by the counting rounds although it runs in the form with one round?
static inline bool way_back(const uint64_t* rec, const Batch& b, int sfield) {
    if (b.count < 2) return false;
    return b.count > psacx::GROUP_RANK_BATCH || !psacx::group_rank_fits(largest_bucket(rec, b, sfield));
}

// The one counting round on a batch (rec: its records, in place order).  The slots inside a bucket are handed out in an order drawn from `seed`: any
// order must give the same result.  out[final place] = record.  Returns false (out untouched) when the batch takes the way back.
static inline bool one_round(const uint64_t* rec, const Batch& b, int sfield, uint64_t seed, std::vector<uint64_t>& out) {
    using namespace psacx;
    if (way_back(rec, b, sfield)) return false;
    const unsigned n = b.count, gbits = group_rank_gbits(b.run), first = (unsigned)b.group & 255u;
    std::vector<unsigned> order(n), slot(n), bucket(n), key(n);
    for (unsigned p = 0; p < n; ++p) order[p] = p;
    for (unsigned p = n; p > 1; --p) std::swap(order[p - 1], order[mix(seed) % p]);
    unsigned cnt[256] = {0}, start[257] = {0}, largest = 0;
    for (unsigned q = 0; q < n; ++q) {
        const unsigned p = order[q], ck = group_rank_ckey(rec[p], sfield, first, gbits);
        bucket[p] = group_rank_bucket(ck, gbits);
        key[p] = group_rank_key(ck, p);
        slot[p] = cnt[bucket[p]]++;
        largest = std::max(largest, slot[p] + 1);
    }
    for (unsigned d = 0; d < 256; ++d) start[d + 1] = start[d] + cnt[d];
    std::vector<unsigned> keys(n + GROUP_RANK_MAX + 2, GROUP_RANK_FILL);
    for (unsigned p = 0; p < n; ++p) keys[start[bucket[p]] + slot[p]] = key[p];
    const unsigned window = 2 * ((largest - 1) / 2 + 1);          // the kernel reads two keys per trip while the first lies inside the largest bucket
    out.assign(n, 0);
    std::vector<bool> taken(n, false);
    for (unsigned p = 0; p < n; ++p) {
        const unsigned at = start[bucket[p]] + group_rank_below(&keys[start[bucket[p]]], window, key[p]);
        if (at >= n || taken[at]) return out.clear(), true;          // (not a permutation: the caller's comparison fails on the empty result)
        taken[at] = true;
        out[at] = rec[p];
    }
    return true;
}

// what every form must leave: the stable order by the 16 bits at sfield inside every group of the batch (ends: the group ends relative to b.a)
static inline std::vector<uint64_t> expected(const uint64_t* rec, const std::vector<uint64_t>& starts, uint64_t nrec, const Batch& b, int sfield) {
    std::vector<uint64_t> out(rec, rec + b.count);
    for (unsigned j = 0; j < b.run; ++j) {
        const uint64_t g = b.group + j, lo = starts[g] - b.a, hi = (g + 1 < starts.size() ? starts[g + 1] : nrec) - b.a;
        std::stable_sort(out.begin() + lo, out.begin() + hi, [sfield](uint64_t x, uint64_t y) { return ((x >> sfield) & 0xFFFF) < ((y >> sfield) & 0xFFFF); });
    }
    return out;
}

// ---- the tables both programs run ----
struct Table { const char* name; int sfield; std::vector<uint64_t> starts; std::vector<uint64_t> rec; int expect_back; };          // expect_back: 0 = no batch, 1 = every batch of two or more records, -1 = not stated
enum KeyKind { UNIFORM, ONE_KEY, ONE_D1, BUCKET_OF };

// record of group g: the digit above the 16 bits numbers the group inside its bucket of 256, the low 32 bits are distinct (serial)
static inline uint64_t make_rec(uint64_t g, unsigned key16, int sfield, uint64_t serial, uint64_t junk) {
    uint64_t top = (junk << 24 | (g & 255) << 16 | key16) << sfield;          // (bits above the group digit: whatever the earlier passes sorted on)
    return top | (serial & 0xFFFFFFFFull);
}
// sizes[g] records per group; kind: how the 16 bits are drawn; arg: the bucket size for BUCKET_OF
static inline Table make_table(const char* name, int sfield, const std::vector<unsigned>& sizes, KeyKind kind, unsigned arg, uint64_t seed, int expect_back) {
    Table t{name, sfield, {}, {}, expect_back};
    uint64_t at = 0;
    for (uint64_t g = 0; g < sizes.size(); ++g) {
        t.starts.push_back(at);
        const unsigned one = (unsigned)mix(seed) & 0xFFFF;
        for (unsigned i = 0; i < sizes[g]; ++i, ++at) {
            unsigned k = (unsigned)mix(seed) & 0xFFFF;
            if (kind == ONE_KEY) k = one;
            if (kind == ONE_D1) k = (one & 0xFF00) | ((i * 37 + 11) & 0xFF);          // (distinct low bytes up to 256 records, not in order)
            if (kind == BUCKET_OF) k = i < arg ? (0x4200 | (k & 0xFF)) : ((i % 180 + 0x43) << 8 | (k & 0xFF));          // arg records in bucket 0x42, at most 2 in any other
            t.rec.push_back(make_rec(g, k, sfield, at * 2654435761ull + 12345, mix(seed) & 0xFF));
        }
    }
    return t;
}
static inline std::vector<unsigned> poisson_like(unsigned ngroups, unsigned mean, uint64_t seed) {          // mean - 104 + 16 draws from 0 .. 13: deviation 16, as Poisson at 256
    std::vector<unsigned> v(ngroups);
    for (unsigned& x : v) { x = mean - 104; for (int j = 0; j < 16; ++j) x += (unsigned)(mix(seed) % 14); }
    return v;
}
static inline std::vector<Table> tables(unsigned ngroups) {
    using psacx::GROUP_RANK_MAX;
    std::vector<Table> t;
    t.push_back(make_table("poisson256_uniform", 32, poisson_like(ngroups, 256, 1), UNIFORM, 0, 101, 0));
    {
        // the sizes where the rows, the batch cut and the cap change, empty groups at both ends of a chunk of 64 and the last group of the table
        const unsigned edge[] = {0, 1, 63, 64, 65, 511, 512, 0, 383, 384, 385, 2, 127, 128, 129, 320};
        std::vector<unsigned> sizes(ngroups);
        for (unsigned g = 0; g < ngroups; ++g) sizes[g] = g % 64 == 0 || g % 64 == 63 ? 0 : edge[(g * 7 + g / 64) % 16];
        sizes[ngroups - 1] = 65;
        t.push_back(make_table("edge_sizes", 32, sizes, UNIFORM, 0, 102, -1));
    }
    t.push_back(make_table("one_key_per_group", 32, poisson_like(ngroups, 256, 3), ONE_KEY, 0, 103, 1));
    t.push_back(make_table("one_d1_distinct_d0", 32, std::vector<unsigned>(ngroups, 200), ONE_D1, 0, 104, 1));
    t.push_back(make_table("largest_bucket_B", 32, std::vector<unsigned>(ngroups, 300), BUCKET_OF, GROUP_RANK_MAX, 105, 0));
    t.push_back(make_table("largest_bucket_B_plus_1", 32, std::vector<unsigned>(ngroups, 300), BUCKET_OF, GROUP_RANK_MAX + 1, 106, 1));
    {
        std::vector<unsigned> sizes = poisson_like(ngroups, 256, 7);
        sizes[ngroups / 2 + 5] = 513;          // left as it is
        t.push_back(make_table("group_of_513", 32, sizes, UNIFORM, 0, 107, 0));
    }
    {
        Table nm = make_table("starts_not_monotone", 32, poisson_like(ngroups, 256, 8), UNIFORM, 0, 108, 0);
        std::swap(nm.starts[64 + 9], nm.starts[64 + 10]);          // the second chunk is left as it is
        t.push_back(nm);
    }
    t.push_back(make_table("groups_of_64", 32, std::vector<unsigned>(ngroups, 64), UNIFORM, 0, 109, 0));
    t.push_back(make_table("groups_of_128", 32, std::vector<unsigned>(ngroups, 128), UNIFORM, 0, 110, 0));
    t.push_back(make_table("poisson256_sfield40", 40, poisson_like(ngroups, 256, 11), UNIFORM, 0, 111, 0));
    return t;
}

} // namespace group_rank_model
