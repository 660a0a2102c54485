// The ordering rule of group_sort16_kernel's one counting round (psac_amd/csrc/group_rank.hpp) on the host: for every table of
// tests/cpp/group_rank_model.hpp -- the shapes tests/cpp/group_sort16_direct.hip runs on the device -- the host model of the round, with the slots
// of every bucket handed out in three different orders, must leave the permutation of std::stable_sort by the 16 bits inside every group, and the
// batches that take the way back must be the ones the table is named for.  No GPU.
#include <cstdio>
#include <cstdlib>
#include "group_rank_model.hpp"

using namespace group_rank_model;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); if (++fails > 20) std::exit(1); } } while (0)

int main() {
    using namespace psacx;
    // the pieces of the rule
    CHECK(group_rank_gbits(1) == 0 && group_rank_gbits(2) == 1 && group_rank_gbits(3) == 2 && group_rank_gbits(4) == 2 && group_rank_gbits(5) == 3 &&
          group_rank_gbits(64) == 6, "gbits");
    for (unsigned run = 1; run <= 64; ++run) {
        const unsigned gb = group_rank_gbits(run);
        CHECK(run <= 1u << gb && (gb == 0 || run > 1u << (gb - 1)), "gbits(%u) = %u", run, gb);
        // every record, whatever it holds, lands in a bucket below 256 with a key below the filler; the bucket never falls when the key grows
        uint64_t seed = run;
        unsigned last_key = 0, last_bucket = 0;
        for (int sf : {32, 40})
            for (unsigned j = 0; j < 2000; ++j) {
                const unsigned ck = group_rank_ckey(mix(seed), sf, (unsigned)mix(seed) & 255, gb), b = group_rank_bucket(ck, gb), k = group_rank_key(ck, (unsigned)mix(seed) & 511);
                CHECK(ck < 1u << (16 + gb) && b < 256 && k < GROUP_RANK_FILL, "range: run %u", run);
                if (j) CHECK((k < last_key) == (b < last_bucket) || b == last_bucket, "buckets follow the keys: run %u", run);
                last_key = k; last_bucket = b;
            }
        // the group number inside the batch comes out of the digit above the 16 bits, across the wrap of that digit too
        CHECK(group_rank_ckey(make_rec(250 + run - 1, 0xBEEF, 32, 7, 0xAA), 32, 250, gb) == ((run - 1) << 16 | 0xBEEF), "ckey: run %u", run);
    }
    CHECK(group_rank_fits(GROUP_RANK_MAX) && !group_rank_fits(GROUP_RANK_MAX + 1) && GROUP_RANK_MAX + 2 <= 64 && GROUP_RANK_MAX < GROUP_RANK_BATCH, "the bound");
    CHECK(GROUP_RANK_BATCH % 64 == 0 && GROUP_RANK_BATCH <= CAP && CAP == 1u << GROUP_RANK_PLACE_BITS, "the batch");
    {
        const unsigned keys[5] = {5, 9, 2, GROUP_RANK_FILL, GROUP_RANK_FILL};
        CHECK(group_rank_below(keys, 5, 9) == 2 && group_rank_below(keys, 5, 2) == 0 && group_rank_below(keys, 0, 9) == 0, "below");
    }

    for (const Table& t : tables(192)) {
        const uint64_t nrec = t.rec.size();
        std::vector<uint64_t> want = t.rec;
        uint64_t back = 0, two_or_more = 0, by_rank = 0;
        for (const Batch& b : cut(t.starts, nrec, GROUP_RANK_BATCH)) {
            const uint64_t* rec = &t.rec[b.a];
            const std::vector<uint64_t> exp = expected(rec, t.starts, nrec, b, t.sfield);
            std::copy(exp.begin(), exp.end(), want.begin() + b.a);
            CHECK(b.count <= CAP && (b.run == 1 || b.count <= GROUP_RANK_BATCH) && b.group % CHUNK + b.run <= CHUNK, "%s: batch at group %llu", t.name, (unsigned long long)b.group);
            two_or_more += b.count >= 2;
            if (way_back(rec, b, t.sfield)) { ++back; continue; }
            for (uint64_t seed : {1ull, 2ull, 3ull}) {          // three orders of the slots
                std::vector<uint64_t> got;
                CHECK(one_round(rec, b, t.sfield, seed * 1000003 + b.group, got), "%s: way back?", t.name);
                CHECK(got == exp, "%s: batch at group %llu (%u groups, %u records), slot order %llu: not the stable order", t.name, (unsigned long long)b.group, b.run,
                      b.count, (unsigned long long)seed);
            }
            ++by_rank;
        }
        // the batches of the form of counting rounds only cover the same records
        uint64_t covered[2] = {0, 0};
        for (const Batch& b : cut(t.starts, nrec, GROUP_RANK_BATCH)) covered[0] += b.count;
        for (const Batch& b : cut(t.starts, nrec, CAP)) covered[1] += b.count;
        CHECK(covered[0] == covered[1], "%s: the two cuts cover %llu and %llu records", t.name, (unsigned long long)covered[0], (unsigned long long)covered[1]);
        if (t.expect_back == 0) CHECK(back == 0, "%s: %llu batches take the way back, none expected", t.name, (unsigned long long)back);
        if (t.expect_back == 1) CHECK(back == two_or_more && back > 0, "%s: %llu of %llu batches take the way back, all expected", t.name, (unsigned long long)back, (unsigned long long)two_or_more);
        std::printf("%-28s records %8llu batches by rank %6llu way back %6llu\n", t.name, (unsigned long long)nrec, (unsigned long long)by_rank, (unsigned long long)back);
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("group rank tests passed\n");
    return 0;
}
