// The ordering rule of group_sort16_kernel's one counting round (radix.hpp), in plain C++: the kernel and the host model of
// tests/cpp/test_group_rank.cpp both include it.
//
// A batch is `run` consecutive groups of one chunk, at most GROUP_CAP records in all.  Their stable order by the 16 prefix bits at
// `sfield`, group after group, is the order of the composite keys
//     key = (number of the group inside the batch, the 16 bits, place of the record in the batch)
// which are distinct because the place is part of them.  One counting round on the top 8 bits of (group number, 16 bits) spreads the
// batch over 256 buckets -- about one record each at 256 records, two at GROUP_CAP -- that follow each other in key order; a
// returning add on the bucket's counter gives every record a slot of its own inside the bucket, IN ANY ORDER, and its key goes to
// keys[bucket start + slot].  The place of a record is then its bucket's start plus the number of smaller keys in its bucket.  The
// kernel counts them over keys[start .. start + largest bucket) without looking at the bucket's end: what lies behind the bucket are
// the keys of later buckets, or the filler behind the last key, all of them larger.  That loop is linear in the largest bucket, so a
// batch whose largest bucket exceeds GROUP_RANK_MAX takes the stable counting rounds instead (group_rank_fits).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PSACX_RANK_FN __host__ __device__ inline
#else
#define PSACX_RANK_FN inline
#endif

namespace psacx {

// the largest bucket the rank loop takes; measured at 2^32 records of random DNA (profiles/group_sort_rounds_ab.txt)
#ifndef PSACX_GROUP_RANK_MAX
#define PSACX_GROUP_RANK_MAX 16
#endif
constexpr unsigned GROUP_RANK_MAX = PSACX_GROUP_RANK_MAX;
// records of a batch at most: six rows of 64, which the kernel holds with their keys and places in 96 vector registers.  Groups are gathered into
// batches up to this size; a single group between it and GROUP_CAP is a batch of its own and takes the counting rounds
constexpr unsigned GROUP_RANK_BATCH = 384;
constexpr unsigned GROUP_RANK_PLACE_BITS = 9;          // places of a batch: below GROUP_CAP = 512 (sort_scratch.hpp)
constexpr unsigned GROUP_RANK_FILL = ~0u;              // behind the last key: larger than every key (those stay below 2^31)

// bits that number the groups of a batch of `run` (1 .. 64) groups
PSACX_RANK_FN unsigned group_rank_gbits(unsigned run) { return run > 1 ? 32u - (unsigned)__builtin_clz(run - 1) : 0u; }
// (group number inside the batch, 16 prefix bits) of a record: below 2^(16 + gbits) whatever the record holds.  first_digit: the digit above the
// 16 bits in the records of the batch's first group (that digit numbers the groups of a bucket)
PSACX_RANK_FN unsigned group_rank_ckey(uint64_t rec, int sfield, unsigned first_digit, unsigned gbits) {
    return ((unsigned)(rec >> sfield) - (first_digit << 16)) & ((1u << (16 + gbits)) - 1u);
}
PSACX_RANK_FN unsigned group_rank_bucket(unsigned ckey, unsigned gbits) { return ckey >> (8 + gbits); }          // below 256
PSACX_RANK_FN unsigned group_rank_key(unsigned ckey, unsigned place) { return ckey << GROUP_RANK_PLACE_BITS | place; }
// does a batch whose largest bucket holds `largest` records take the rank loop?
PSACX_RANK_FN bool group_rank_fits(unsigned largest) { return largest <= GROUP_RANK_MAX; }
// keys among keys[0 .. n) that are smaller than key
PSACX_RANK_FN unsigned group_rank_below(const unsigned* keys, unsigned n, unsigned key) {
    unsigned c = 0;
    for (unsigned j = 0; j < n; ++j) c += keys[j] < key ? 1u : 0u;
    return c;
}

} // namespace psacx
