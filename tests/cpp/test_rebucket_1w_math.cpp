// The arithmetic of rebucket_first_1w_kernel (psac_amd/csrc/rebucket_1w_math.hpp) against the generic kernel's formulas, on the host.
// The generic forms (window_lcp, first_round_len, onew_word1 of sa_kernels.hpp) are written out again here as the reference.
// Built and run by tests/test_rebucket_1w_math_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "rebucket_1w_math.hpp"

using namespace psacx;

// ---- the generic formulas
struct KeyShape { unsigned lc, c1, c2; };
static unsigned clz64(uint64_t x) { return x ? (unsigned)__builtin_clzll(x) : 64u; }
static unsigned window_lcp(uint64_t x1, uint64_t x2, uint64_t y1, uint64_t y2, const KeyShape& ks) {
    if (x1 != y1) return (clz64(x1 ^ y1) - (64u - ks.c1 * ks.lc)) / ks.lc;
    if (x2 != y2) return ks.c1 + (clz64(x2 ^ y2) - (64u - ks.c2 * ks.lc)) / ks.lc;
    return ks.c1 + ks.c2;
}
static uint64_t first_round_len(uint64_t ng, uint64_t sa) { return ng - sa; }
static uint64_t onew_word1(unsigned low, unsigned lo1, unsigned b, uint64_t rest) { return (((uint64_t)b << low) | rest) << lo1; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static long failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static void test_chars() {
    for (unsigned lc = 1; lc <= 8; ++lc) {
        const uint32_t recip = rb1w_recip(lc);
        for (unsigned bits = 0; bits <= 64; ++bits) CHECK(rb1w_chars(bits, recip) == bits / lc, "chars bits=%u lc=%u: %u", bits, lc, rb1w_chars(bits, recip));
    }
}

static void check_pair(const KeyShape& ks, const Rb1wShape& sh, unsigned lo1, unsigned ba, uint32_t ra, unsigned bb, uint32_t rb) {
    const unsigned want = window_lcp(onew_word1(sh.low, lo1, ba, ra), 0, onew_word1(sh.low, lo1, bb, rb), 0, ks);
    const unsigned got = rb1w_lead_lcp(ba, ra, bb, rb, sh);
    CHECK(got == want, "lead lcp lc=%u low=%u (%u,%08x) (%u,%08x): %u, want %u", ks.lc, sh.low, ba, ra, bb, rb, got, want);
    if (ba == bb && ra != rb) CHECK(rb1w_lead_lcp_rest(ra, rb, sh) == want, "rest form lc=%u low=%u %08x %08x", ks.lc, sh.low, ra, rb);
    if (ba != bb) CHECK(rb1w_lead_lcp_bucket(ba, bb, sh) == want, "bucket form lc=%u %u %u", ks.lc, ba, bb);
}

static void test_lead_lcp() {
    const unsigned lcs[] = {1, 2, 3, 5, 7, 8};
    for (unsigned lc : lcs) {
        KeyShape ks;
        ks.lc = lc; ks.c1 = 64 / lc; ks.c2 = ks.c1;          // a 64-bit word holds floor(64 / lc) characters
        for (unsigned low = 16; low <= 32; low += 8) {
            if (RB1W_DIGIT_BITS + low > ks.c1 * lc) continue;
            const unsigned lo1 = ks.c1 * lc - RB1W_DIGIT_BITS - low;
            const unsigned sfield = 64 - low;
            CHECK(rb1w_fits(lc, ks.c1, ks.c2, low, sfield, 1ull << 32), "fits lc=%u low=%u", lc, low);
            const Rb1wShape sh = rb1w_shape(lc, ks.c1, ks.c2, low, sfield, 1ull << 32);
            const uint32_t rmask = low == 32 ? 0xFFFFFFFFu : ((1u << low) - 1u);
            // differ only in the bucket (every bit of it), only in the rest (every bit of it, the last kept one included), equal
            for (unsigned bit = 0; bit < 8; ++bit)
                for (int t = 0; t < 64; ++t) {
                    const unsigned b = (unsigned)rng() & 255u;
                    const uint32_t r = (uint32_t)rng() & rmask;
                    check_pair(ks, sh, lo1, b, r, b ^ (1u << bit), r);
                    check_pair(ks, sh, lo1, b, r, (b ^ (1u << bit)) & ~((1u << bit) - 1u), r);
                }
            for (unsigned bit = 0; bit < low; ++bit)
                for (int t = 0; t < 64; ++t) {
                    const unsigned b = (unsigned)rng() & 255u;
                    const uint32_t r = (uint32_t)rng() & rmask;
                    check_pair(ks, sh, lo1, b, r, b, r ^ (1u << bit));
                    check_pair(ks, sh, lo1, b, r, b, (r ^ (1u << bit)) ^ ((uint32_t)rng() & ((1u << bit) - 1u)));
                }
            for (int t = 0; t < 256; ++t) {
                const unsigned b = (unsigned)t;
                const uint32_t r = (uint32_t)rng() & rmask;
                check_pair(ks, sh, lo1, b, r, b, r);
                check_pair(ks, sh, lo1, b, 0, b, 0);
                check_pair(ks, sh, lo1, b, rmask, b, rmask);
            }
            // random pairs: half of them in one bucket, the first difference of the rests anywhere
            for (int t = 0; t < 1000000; ++t) {
                const uint64_t x = rng(), y = rng();
                const unsigned ba = (unsigned)x & 255u;
                const unsigned bb = (x >> 8) & 1u ? ba : (unsigned)y & 255u;
                const uint32_t ra = (uint32_t)(x >> 32) & rmask;
                const unsigned keep = (unsigned)(y >> 8) % (low + 1u);          // leading bits of the rest that agree
                const uint32_t diff = keep >= low ? 0u : ((uint32_t)(y >> 32) & (rmask >> keep));
                check_pair(ks, sh, lo1, ba, ra, bb, ra ^ diff);
            }
            // whole windows of tied records against window_lcp (the kernel's form has no division)
            for (int t = 0; t < 200000; ++t) {
                const uint64_t m1 = ks.c1 * lc == 64 ? ~0ull : ((1ull << (ks.c1 * lc)) - 1ull), m2 = ks.c2 * lc == 64 ? ~0ull : ((1ull << (ks.c2 * lc)) - 1ull);
                const uint64_t x1 = rng() & m1, x2 = rng() & m2;
                const unsigned mode = (unsigned)rng() % 3u;
                const uint64_t d = (rng() >> ((unsigned)rng() & 63u));
                const uint64_t y1 = mode == 0 ? (x1 ^ (d & m1)) : x1, y2 = mode == 1 ? (x2 ^ (d & m2)) : (mode == 0 ? rng() & m2 : x2);
                CHECK(rb1w_window_lcp(x1, x2, y1, y2, sh) == window_lcp(x1, x2, y1, y2, ks), "window lcp lc=%u", lc);
            }
        }
    }
}

static void test_short() {
    const unsigned two_ks[] = {2, 3, 18, 64, 128, 255};
    for (unsigned two_k : two_ks) {
        const uint64_t ns[] = {1, (uint64_t)two_k - 1, two_k, (uint64_t)two_k + 1, 1ull << 31, (1ull << 32) - 2, (1ull << 32) - 1, 1ull << 32};
        for (uint64_t n : ns) {
            if (n == 0) continue;
            Rb1wShape sh = rb1w_shape(1, two_k - two_k / 2, two_k / 2, 32, 32, n);
            CHECK(sh.two_k == two_k, "shape");
            const int64_t cand[] = {0, 1, (int64_t)n - 2 * (int64_t)two_k, (int64_t)n - (int64_t)two_k - 1, (int64_t)n - (int64_t)two_k, (int64_t)n - (int64_t)two_k + 1,
                                    (int64_t)n - 2, (int64_t)n - 1};
            for (int64_t s : cand) {
                if (s < 0 || (uint64_t)s >= n) continue;
                const uint64_t len = first_round_len(n, (uint64_t)s);
                CHECK(rb1w_short((uint32_t)s, sh) == (len < two_k), "short n=%llu sa=%lld 2k=%u", (unsigned long long)n, (long long)s, two_k);
                for (unsigned c = 0; c <= two_k; ++c) {
                    const uint64_t want = c < len ? c : len;
                    CHECK(rb1w_cap(c, (uint32_t)s, sh) == want, "cap n=%llu sa=%lld c=%u 2k=%u: %u, want %llu", (unsigned long long)n, (long long)s, c, two_k,
                          rb1w_cap(c, (uint32_t)s, sh), (unsigned long long)want);
                }
            }
        }
    }
    // n = 2^32, suffix 0: the length is 0 in 32 bits; it must not count as short
    const Rb1wShape sh = rb1w_shape(2, 32, 32, 32, 32, 1ull << 32);
    CHECK(!rb1w_short(0u, sh) && rb1w_cap(64u, 0u, sh) == 64u, "n = 2^32, suffix 0");
    CHECK(rb1w_short(0xFFFFFFFFu, sh) && rb1w_cap(64u, 0xFFFFFFFFu, sh) == 1u, "n = 2^32, last suffix");
}

static void test_rank_id() {
    const uint64_t pos[] = {0, 1, 4095, 4096, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 2, (1ull << 32) - 1};
    for (uint64_t e : pos) {
        const uint64_t id = e + 1;                                  // the generic kernel: id of a head at position e (off = 0)
        const uint32_t pair_rank = (uint32_t)(id - 1);              // ... and the rank it puts into the pair
        CHECK(rb1w_rank_of_head(e) == pair_rank, "rank of head %llu", (unsigned long long)e);
        CHECK(rb1w_rank_of_id(id) == pair_rank, "rank of id %llu", (unsigned long long)id);
        CHECK(rb1w_id_of_rank(rb1w_rank_of_head(e)) == id, "id of rank %llu", (unsigned long long)e);
    }
    CHECK(rb1w_id_of_rank(0xFFFFFFFFu) == (1ull << 32), "id 2^32");
    CHECK(!rb1w_fits(2, 32, 32, 32, 32, (1ull << 32) + 1) && !rb1w_fits(8, 8, 8, 24, 32, 1ull << 30) && rb1w_fits(2, 32, 32, 32, 32, 1ull << 32), "fits");
    // a tile-local scan value of 0 means "no head in the tile before this run": the rank comes from the tile's carry then
    CHECK(rb1w_rank_of_id(1) == 0u && rb1w_rank_of_id(1ull << 32) == 0xFFFFFFFFu, "carry");
}

int main() {
    test_chars();
    test_lead_lcp();
    test_short();
    test_rank_id();
    if (failures) { std::printf("%ld checks failed\n", failures); return 1; }
    std::printf("rebucket 1w math tests passed\n");
    return 0;
}
