// rebucket_1w_math.hpp -- the arithmetic of rebucket_first_1w_kernel (sa_kernels.hpp) that differs from the generic kernel's.
//
// The generic kernel of the first round compares two records as 64-bit words (window_lcp), divides by the bits per character once per
// record and takes suffix lengths as 64-bit differences (first_round_len).  On one-word records of at most 2^32 suffixes a record is its
// bucket (the top digit of the sorted prefix, known from its place), the 32-bit rest of the prefix and a 32-bit suffix, and all of that
// is done in 32 bits.  The pieces are here as small functions that a host compiler can include without HIP, so that they are tested on
// the CPU against the generic formulas, at n = 2^32 too (tests/cpp/test_rebucket_1w_math.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RB1W_HD __host__ __device__ __forceinline__
#else
#define RB1W_HD inline
#endif

namespace psacx {

constexpr unsigned RB1W_DIGIT_BITS = 8;        // bits of the top digit (the bucket number)
constexpr unsigned RB1W_RECIP_SHIFT = 10;

RB1W_HD unsigned rb1w_clz32(uint32_t x) { return x ? (unsigned)__builtin_clz(x) : 32u; }
RB1W_HD unsigned rb1w_clz64(uint64_t x) { return x ? (unsigned)__builtin_clzll(x) : 64u; }

// ---- bits -> characters without a division
// floor(bits / lc) = (bits * ceil(2^10 / lc)) >> 10 as long as bits * lc < 2^10: the error of the rounded-up reciprocal, bits * (recip * lc
// - 2^10) / (lc * 2^10), stays below 1 / lc then.  bits <= 64 and lc <= 8 here.  The reciprocal is made once per launch, on the host.
RB1W_HD uint32_t rb1w_recip(unsigned lc) { return ((1u << RB1W_RECIP_SHIFT) + lc - 1u) / lc; }
RB1W_HD unsigned rb1w_chars(unsigned bits, uint32_t recip) { return (bits * recip) >> RB1W_RECIP_SHIFT; }

// What the kernel needs to know about the shape of the records and the text, made by the host (rb1w_shape).
struct Rb1wShape {
    uint32_t recip;      // rb1w_recip(bits per character)
    uint32_t low;        // bits of the sorted prefix below the top digit (the rest: at most 32)
    uint32_t sfield;     // width of the suffix field of a record (64 - low)
    uint32_t two_k;      // characters of a window (at most 255: first-round LCP values travel as bytes)
    uint32_t nm1;        // n - 1, n <= 2^32
    uint32_t bits1, bits2;      // bits of word 1 / word 2 of a window (c1 * lc, c2 * lc)
    uint32_t c1;
};
inline Rb1wShape rb1w_shape(unsigned lc, unsigned c1, unsigned c2, unsigned low, unsigned sfield, uint64_t n) {
    Rb1wShape s;
    s.recip = rb1w_recip(lc); s.low = low; s.sfield = sfield; s.two_k = c1 + c2; s.nm1 = (uint32_t)(n - 1);
    s.bits1 = c1 * lc; s.bits2 = c2 * lc; s.c1 = c1;
    return s;
}
// the assumptions of the 32-bit form; the caller takes the generic kernel when they do not hold
inline bool rb1w_fits(unsigned lc, unsigned c1, unsigned c2, unsigned low, unsigned sfield, uint64_t n) {
    return n >= 1 && n <= (1ull << 32) && lc >= 1 && lc <= 8 && c1 + c2 <= 255 && low <= 32 && sfield >= 32 && low + sfield == 64 && c1 * lc <= 64 && c2 * lc <= 64 &&
           RB1W_DIGIT_BITS + low <= c1 * lc;
}

// ---- characters two leading parts share from the left
// A leading part is (bucket << low) | rest, the top RB1W_DIGIT_BITS + low bits of word 1.  Same bucket, rests differ (the common case):
// the shared bits are the digit's eight, plus the equal top bits of the rests inside their `low`-bit field.
RB1W_HD unsigned rb1w_lead_lcp_rest(uint32_t ra, uint32_t rb, const Rb1wShape& s) {      // ra != rb
    return rb1w_chars(RB1W_DIGIT_BITS + s.low - 32u + rb1w_clz32(ra ^ rb), s.recip);
}
RB1W_HD unsigned rb1w_lead_lcp_bucket(unsigned ba, unsigned bb, const Rb1wShape& s) {      // ba != bb, both below 256
    return rb1w_chars(rb1w_clz32((uint32_t)(ba ^ bb)) - (32u - RB1W_DIGIT_BITS), s.recip);
}
// any two leading parts; equal ones share the whole window as far as the leading parts can tell (the kernel reads both words of such
// records then: rb1w_window_lcp).  The kernel does not call this function: it knows which of the three cases it is in before it computes
// (every record takes the _rest form, a bucket border found by the cursor the _bucket form, equal leading parts rb1w_window_lcp).  It is
// here so that the host test can hold the three forms, cut as the kernel cuts them, against window_lcp on whole words.
RB1W_HD unsigned rb1w_lead_lcp(unsigned ba, uint32_t ra, unsigned bb, uint32_t rb, const Rb1wShape& s) {
    if (ba != bb) return rb1w_lead_lcp_bucket(ba, bb, s);
    if (ra != rb) return rb1w_lead_lcp_rest(ra, rb, s);
    return s.two_k;
}
// two whole windows (window_lcp of sa_kernels.hpp on 64-bit words, without its divisions)
RB1W_HD unsigned rb1w_window_lcp(uint64_t x1, uint64_t x2, uint64_t y1, uint64_t y2, const Rb1wShape& s) {
    if (x1 != y1) return rb1w_chars(rb1w_clz64(x1 ^ y1) - (64u - s.bits1), s.recip);
    if (x2 != y2) return s.c1 + rb1w_chars(rb1w_clz64(x2 ^ y2) - (64u - s.bits2), s.recip);
    return s.two_k;
}

// ---- suffixes shorter than a window
// The first-round LCP of two suffixes is capped by their lengths n - sa, which matters only where n - sa < 2k.  n may be 2^32, which is 0 in
// 32 bits, and then n - 0 is too; n - 1 - sa is below 2^32 for every n <= 2^32 and every suffix, so the test is made on that.
RB1W_HD bool rb1w_short(uint32_t sa, const Rb1wShape& s) { return s.nm1 - sa < s.two_k - 1u; }      // n - sa < 2k
RB1W_HD unsigned rb1w_cap(unsigned c, uint32_t sa, const Rb1wShape& s) {                                // min(c, n - sa), c <= 2k
    const uint32_t rem = s.nm1 - sa;
    return (rb1w_short(sa, s) && rem + 1u < c) ? rem + 1u : c;
}

// ---- bucket ids and ranks
// The id of a bucket is the position of its head + 1 (1 .. 2^32: 33 bits); the rank that goes into the inversion's pair is id - 1.  The
// kernel carries ranks, which fit in 32 bits at every position, and widens to an id where it stores one.
RB1W_HD uint32_t rb1w_rank_of_head(uint64_t e) { return (uint32_t)e; }               // e < 2^32
RB1W_HD uint32_t rb1w_rank_of_id(uint64_t id) { return (uint32_t)(id - 1u); }        // id in 1 .. 2^32
RB1W_HD uint64_t rb1w_id_of_rank(uint32_t rank) { return (uint64_t)rank + 1u; }

} // namespace psacx
