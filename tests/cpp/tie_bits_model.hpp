// Host model of the tie bits (psac_amd/csrc/tie_bits.hpp): the words a set of batches must leave, place by place, and the same words put together the
// way group_sort16_kernel<.., BITS> does it, row by row with the functions of that header.  Shared by tests/cpp/test_tie_bits.cpp (host only) and
// tests/cpp/group_sort16_bits_direct.hip (against the kernel).
#pragma once
#include <cstdint>
#include <vector>
#include "tie_bits.hpp"

namespace tie_bits_model {

struct Span { uint64_t a; unsigned count; };          // a batch: its first place and its records

// Brute force.  rec[p - origin] is the record at place p (the places of the table are origin .. origin + rec.size()); the words returned start with
// the word of place `origin`, so bit p is bit p & 63 of entry (p >> 6) - (origin >> 6).
static inline std::vector<uint64_t> words_brute(const std::vector<uint64_t>& rec, uint64_t origin, const std::vector<Span>& batches, int sfield) {
    std::vector<uint64_t> w((origin + rec.size() + 63) / 64 - origin / 64 + 1, 0);
    for (const Span& b : batches)
        for (unsigned i = 1; i < b.count; ++i) {
            const uint64_t p = b.a + i;
            if ((rec[p - origin] >> sfield) == (rec[p - 1 - origin] >> sfield)) w[(p >> 6) - (origin >> 6)] |= 1ull << (p & 63);
        }
    return w;
}

// The kernel's way: rows of 64 places from the first place of every batch, one mask per row, two words per mask.  `order`: the batches in the
// order they are merged in (any order must give the same words)
static inline std::vector<uint64_t> words_by_rows(const std::vector<uint64_t>& rec, uint64_t origin, const std::vector<Span>& batches, int sfield,
                                                  const std::vector<unsigned>& order) {
    std::vector<uint64_t> w((origin + rec.size() + 63) / 64 - origin / 64 + 1, 0);
    for (unsigned o : order) {
        const Span& b = batches[o];
        uint64_t carry = 0;
        const unsigned rows = (b.count + 63) / 64;
        for (unsigned i = 0; i < rows; ++i) {
            uint64_t row = 0;
            for (unsigned l = 0; l < 64 && i * 64 + l < b.count; ++l) {
                const uint64_t p = b.a + i * 64 + l;
                if (i * 64 + l == 0) continue;
                const uint64_t x = rec[p - 1 - origin], y = rec[p - origin];
                if (psacx::tie_pair_high((uint32_t)(x >> 32), (uint32_t)(y >> 32), sfield)) row |= 1ull << l;
            }
            w[((b.a >> 6) - (origin >> 6)) + i] |= carry | psacx::tie_row_low(row, b.a);
            carry = psacx::tie_row_high(row, b.a);
        }
        w[((b.a >> 6) - (origin >> 6)) + rows] |= carry;
    }
    return w;
}

} // namespace tie_bits_model
