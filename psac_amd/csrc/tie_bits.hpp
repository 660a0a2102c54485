// The tie bits of the one-word first round, in plain C++: group_sort16_kernel<.., BITS> (radix.hpp) writes them, tie_resolve_1w_waves_kernel<.., BITS>
// (sa_kernels.hpp) reads them, and the host model of tests/cpp/test_tie_bits.cpp includes the same rules.
//
// Bit p of the stream is bit p & 63 of word p >> 6.  It is set iff p > 0, the records at the places p - 1 and p lie in one batch of the group
// sort and agree in everything above their suffix field (rec >> sfield): the two suffixes tie on the sorted prefix.  A batch holds whole groups
// of one top-digit bucket, and two groups differ above their low 16 prefix bits, so this is the predicate of the tie scan on records,
// (x >> sfield) == (y >> sfield) with no bucket starting at p.
//   - a row of a batch is 64 consecutive places from a place that need not be a multiple of 64: its 64 bits land in two words
//     (tie_row_low, tie_row_high), and a word can hold bits of two batches of two waves -- the writers OR their parts into zeroed words;
//   - a tie group is a place whose bit is clear followed by a run of set bits: its leader is the place before the run (tie_leaders), its
//     length the run plus one (tie_group_length); a run of TIE_GROUP_MAX or more bits is a group the tie scan does not order itself.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PSACX_TIE_FN __host__ __device__ inline
#else
#define PSACX_TIE_FN inline
#endif

namespace psacx {

constexpr unsigned TIE_GROUP_MAX = 8;          // members of the longest group the tie scan orders itself (first_round.hpp: TG)

// do two neighbouring records of a batch tie?  (the suffix field takes at least 32 bits: only the upper halves decide)
PSACX_TIE_FN bool tie_pair(uint64_t before, uint64_t rec, int sfield) { return (before >> sfield) == (rec >> sfield); }
PSACX_TIE_FN bool tie_pair_high(uint32_t before_hi, uint32_t rec_hi, int sfield) { return ((before_hi ^ rec_hi) >> (sfield - 32)) == 0; }

// a row of 64 bits whose first place is `first`: what it adds to word first >> 6 and to the word behind it
PSACX_TIE_FN uint64_t tie_row_low(uint64_t row, uint64_t first) { return row << (first & 63); }
PSACX_TIE_FN uint64_t tie_row_high(uint64_t row, uint64_t first) { return (first & 63) ? row >> (64 - (first & 63)) : 0ull; }

// the leaders among the 64 places of a word: bit q set iff place q starts a group, that is bit q is clear and bit q + 1 is set.
// next0: bit 0 of the word behind (0 behind the last word)
PSACX_TIE_FN uint64_t tie_leaders(uint64_t word, unsigned next0) { return ((word >> 1) | ((uint64_t)(next0 & 1u) << 63)) & ~word; }

PSACX_TIE_FN bool tie_bit(const uint64_t* words, uint64_t p) { return (words[p >> 6] >> (p & 63)) & 1ull; }
// members of the group whose leader is place q (bit q clear, bit q + 1 set), counted up to `cap` + 1: a result above cap says "longer than cap".
// nplaces: places of the stream
PSACX_TIE_FN unsigned tie_group_length(const uint64_t* words, uint64_t nplaces, uint64_t q, unsigned cap) {
    unsigned len = 1;
    while (len <= cap && q + len < nplaces && tie_bit(words, q + len)) ++len;
    return len;
}

} // namespace psacx
