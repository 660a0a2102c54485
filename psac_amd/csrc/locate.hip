// locate.hip -- the queries over a suffix array resident in HBM: batched pattern search and the k-mer lookup table in front of it
// (include/psacx.h: "pattern search"), the same over string sets and the occurrence lists, and the longest-match search
// ("longest match and matching statistics").  Kernels in search.hpp, lookup_table.hpp, occurrences.hpp and scan.hpp.
//
// Stands in for sa_index::locate (the reference's include/seq_query.hpp:246-251) and lookup_index (lookup_table.hpp:36-149),
// which desa-main -c -q drives (src/desa_main.cpp).  One GPU; no LCP, Lc or RMQ is consulted: on one GPU the text is as near as
// they are.
#include "engine.hpp"
#include "lookup_table.hpp"
#include "occurrences.hpp"
#include "scan.hpp"
#include "search.hpp"
#include "staging.hpp"

namespace psacx {

static const uint64_t LOCATE_MAX_KEYS = 1ull << 30;

// B^k, or 0 if that exceeds LOCATE_MAX_KEYS
static uint64_t key_space(uint32_t B, uint32_t k) {
    uint64_t e = 1;
    for (uint32_t i = 0; i < k; ++i) { e *= B; if (e > LOCATE_MAX_KEYS) return 0; }
    return e;
}

// a runtime flag as a template argument: f(std::true_type()) or f(std::false_type())
template <typename F>
static void with_flag(bool flag, F f) {
    if (flag) f(std::true_type()); else f(std::false_type());
}

// The table by counting: every text position adds one to the bin of its key, then the bins become their exclusive prefix sums.
// The SA is not consulted -- the table is defined by the text alone and must not inherit a wrong SA.
// tab / B = sigma + 1 / keys = B^k as table_alphabet left them; d_table has keys + 1 entries.  Queued on the ctx stream.
// d_ends != nullptr: the text is a string set with that bitmap of its string ends, and the keys are cut there.
template <typename T>
static int lookup_table_fill(psacx_ctx* c, const uint8_t* d_text, uint64_t n, uint32_t k, uint32_t B, uint64_t keys, const CodeTable& tab, T* d_table,
                             const uint32_t* d_ends = nullptr) {
    const uint64_t E = keys + 1;
    PSACX_HIP(c, hipMemsetAsync(d_table, 0, E * sizeof(T), c->stream));
    const int grid = grid_for(c, (n + LOCATE_STRIP - 1) / LOCATE_STRIP, 256, 8);
    with_flag(E <= LOCATE_LDS_BINS, [&](auto in_lds) {
        with_flag(d_ends != nullptr, [&](auto set) {
            hipLaunchKernelGGL((kmer_count_kernel<T, decltype(in_lds)::value, decltype(set)::value>), dim3(grid), dim3(256), 0, c->stream, d_text, n, k, B,
                               keys / B, tab, d_table, E, d_ends);
        });
    });
    PSACX_HIP(c, hipGetLastError());
    return exclusive_scan_dev<T>(c, d_table, E);
}

// code(), sigma and B^k of a text resident in HBM (one device histogram); PSACX_EINVAL where B^k exceeds LOCATE_MAX_KEYS
static int table_alphabet(psacx_ctx* c, const uint8_t* d_text, uint64_t n, uint32_t k, CodeTable& tab, uint32_t& sigma, uint64_t& keys) {
    PSACX_TRY(ensure_slab(c, 4096));
    PSACX_TRY(tree_alphabet_dev(c, d_text, n, reinterpret_cast<unsigned long long*>(c->slab), tab, sigma));
    keys = key_space(sigma + 1, k);
    return keys ? PSACX_OK : PSACX_EINVAL;
}

// d_ends != nullptr: psacx_lookup_table_gsa_dev_*
template <typename T>
int lookup_table_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const T* /*d_SA*/, uint32_t k, T* d_table, uint16_t* code, uint32_t* sigma,
                     uint64_t* entries, const uint32_t* d_ends = nullptr) {
    if (!c || !d_text || !code || !sigma || !entries || n == 0 || k == 0) return PSACX_EINVAL;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    PSACX_HIP(c, hipSetDevice(c->device));
    CodeTable tab;
    std::memset(&tab, 0, sizeof(tab));
    uint64_t keys = 0;
    const int rc = table_alphabet(c, d_text, n, k, tab, *sigma, keys);
    std::memcpy(code, tab.c, sizeof(tab.c));
    PSACX_TRY(rc);
    *entries = keys + 1;
    if (!d_table) return PSACX_OK;                    // size query
    PSACX_TRY(lookup_table_fill<T>(c, d_text, n, k, *sigma + 1, keys, tab, d_table, d_ends));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// the table of a host-pointer form (staging.hpp)
template <typename T>
T* staged_lookup_table(Staging& s, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, uint32_t k, uint16_t code[256]) {
    if (s.rc != PSACX_OK || !k) return nullptr;
    CodeTable tab;
    uint32_t sigma = 0;
    uint64_t keys = 0;
    s.rc = table_alphabet(s.c, d_text, n, k, tab, sigma, keys);
    T* d_table = (T*)s.alloc((keys + 1) * sizeof(T));
    if (s.rc == PSACX_OK) s.rc = lookup_table_fill<T>(s.c, d_text, n, k, sigma + 1, keys, tab, d_table, d_ends);
    if (s.rc == PSACX_OK) std::memcpy(code, tab.c, sizeof(tab.c));
    return d_table;
}

template uint32_t* staged_lookup_table<uint32_t>(Staging&, const uint8_t*, uint64_t, const uint32_t*, uint32_t, uint16_t*);
template uint64_t* staged_lookup_table<uint64_t>(Staging&, const uint8_t*, uint64_t, const uint32_t*, uint32_t, uint16_t*);

// What a search takes of its table: (d_table, k, code[]) are all there or all absent (k == 0), and code[] gives tab and
// B = sigma + 1 with B^k inside LOCATE_MAX_KEYS; PSACX_EINVAL otherwise.
struct SearchTable { CodeTable tab; uint32_t B = 1; };

static int search_table_valid(const void* d_table, uint32_t k, const uint16_t* code) {
    return (d_table == nullptr) != (k == 0) || (code == nullptr) != (k == 0) ? PSACX_EINVAL : PSACX_OK;
}

static int search_table_of(uint32_t k, const uint16_t* code, SearchTable& t) {
    std::memset(&t.tab, 0, sizeof(t.tab));
    if (!k) return PSACX_OK;
    std::memcpy(t.tab.c, code, sizeof(t.tab.c));
    for (int ch = 0; ch < 256; ++ch) t.B = std::max<uint32_t>(t.B, (uint32_t)t.tab.c[ch] + 1);
    return t.B < 2 || key_space(t.B, k) == 0 ? PSACX_EINVAL : PSACX_OK;
}

// The three slab words around a search: [0] malformed offsets, [1], [2] the fetch counters.  They are zeroed, the offsets kernel
// runs (check_total: poff[q] must be total), search(bad, counters) queues the search kernel, and the words are read back: the
// call ends synchronised, PSACX_EINVAL if the offsets were malformed (the kernel wrote nothing then), else with
// stats.locate_fetches updated ([0, 0] unless the counting kernel ran).
template <typename Search>
static int search_with_slab_words(psacx_ctx* c, const uint64_t* d_poff, uint64_t q, bool check_total, uint64_t total, Search search) {
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(ensure_slab(c, 4096));
    unsigned long long* d_words = reinterpret_cast<unsigned long long*>(c->slab);
    PSACX_HIP(c, hipMemsetAsync(d_words, 0, 3 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(search_offsets_kernel, dim3(grid_for(c, q, 256, 8)), dim3(256), 0, c->stream, d_poff, q, check_total, total, d_words);
    PSACX_HIP(c, hipGetLastError());
    search((const unsigned long long*)d_words, d_words + 1);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long words[3] = {0, 0, 0};
    PSACX_HIP(c, hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (words[0]) return PSACX_EINVAL;
    c->stats.locate_fetches[0] = words[1];
    c->stats.locate_fetches[1] = words[2];
    return PSACX_OK;
}

// d_ends != nullptr: psacx_locate_gsa_dev_* (one pattern per lane whatever PSACX_OPT_LOCATE_SHAPE says).  Declared in query_calls.hpp:
// kmismatch.hip searches its pieces by it.
template <typename T>
int locate_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const T* d_SA, const T* d_table, uint32_t k, const uint16_t* code,
               const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, T* d_lb, T* d_ub, const uint32_t* d_ends) {
    if (!c) return PSACX_EINVAL;
    PSACX_TRY(search_table_valid(d_table, k, code));
    if (q == 0) return PSACX_OK;
    if (!d_text || !d_SA || !d_pat || !d_poff || !d_lb || !d_ub || n == 0) return PSACX_EINVAL;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    SearchTable t;
    PSACX_TRY(search_table_of(k, code, t));
    return search_with_slab_words(c, d_poff, q, false, 0, [&](const unsigned long long* d_bad, unsigned long long* d_counters) {
        auto launch = [&](auto kernel, int lanes) {
            hipLaunchKernelGGL(kernel, dim3(grid_for(c, q * lanes, 256, 8)), dim3(256), 0, c->stream, d_text, n, d_ends, d_SA, d_table, k, t.B, t.tab, d_pat,
                               d_poff, q, d_lb, d_ub, d_bad, d_counters);
        };
        with_flag(c->knobs.locate_count, [&](auto count) {
            constexpr bool COUNT = decltype(count)::value;
            if (d_ends) launch(locate_kernel<T, 1, true, COUNT>, 1);
            else if (c->knobs.locate_shape == 2) launch(locate_kernel<T, 8, false, COUNT>, 8);
            else launch(locate_kernel<T, 1, false, COUNT>, 1);
        });
    });
}

template int locate_dev<uint32_t>(psacx_ctx*, const uint8_t*, uint64_t, const uint32_t*, const uint32_t*, uint32_t, const uint16_t*, const uint8_t*, const uint64_t*,
                                  uint64_t, uint32_t*, uint32_t*, const uint32_t*);
template int locate_dev<uint64_t>(psacx_ctx*, const uint8_t*, uint64_t, const uint64_t*, const uint64_t*, uint32_t, const uint16_t*, const uint8_t*, const uint64_t*,
                                  uint64_t, uint64_t*, uint64_t*, const uint32_t*);

// psacx_match_dev_* / psacx_match_gsa_dev_* (set: the string-set form, which needs d_ends): the checks of locate_dev, the offsets
// kernel with the rule for out_entries, and one launch of match_kernel.
template <typename T>
int match_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, bool set, const T* d_SA, const T* d_table, uint32_t k,
              const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, uint32_t flags, uint64_t max_len, uint64_t out_entries,
              T* d_len, T* d_lb, T* d_ub) {
    if (!c) return PSACX_EINVAL;
    if (flags & ~(uint32_t)PSACX_MATCH_SUFFIXES) return PSACX_EINVAL;
    PSACX_TRY(search_table_valid(d_table, k, code));
    if (q == 0) return out_entries == 0 ? PSACX_OK : PSACX_EINVAL;
    const bool suffixes = (flags & PSACX_MATCH_SUFFIXES) != 0;
    if (!suffixes && out_entries != q) return PSACX_EINVAL;
    if (!d_text || !d_SA || !d_pat || !d_poff || n == 0 || (set && !d_ends)) return PSACX_EINVAL;
    if (out_entries && (!d_len || !d_lb || !d_ub)) return PSACX_EINVAL;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    SearchTable t;
    PSACX_TRY(search_table_of(k, code, t));
    return search_with_slab_words(c, d_poff, q, suffixes, out_entries, [&](const unsigned long long* d_bad, unsigned long long* d_counters) {
        if (!out_entries) return;                     // (a suffix batch of empty patterns has nothing to search)
        with_flag(set, [&](auto in_set) {
            with_flag(c->knobs.locate_count, [&](auto count) {
                hipLaunchKernelGGL((match_kernel<T, decltype(in_set)::value, decltype(count)::value>), dim3(grid_for(c, out_entries, 256, 8)), dim3(256), 0,
                                   c->stream, d_text, n, d_ends, d_SA, d_table, k, t.B, t.tab, d_pat, d_poff, q, suffixes ? MATCH_MODE_SUFFIXES : 0u, max_len,
                                   out_entries, d_len, d_lb, d_ub, d_bad, d_counters);
            });
        });
    });
}

template int match_dev<uint32_t>(psacx_ctx*, const uint8_t*, uint64_t, const uint32_t*, bool, const uint32_t*, const uint32_t*, uint32_t, const uint16_t*,
                                 const uint8_t*, const uint64_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint32_t*, uint32_t*, uint32_t*);
template int match_dev<uint64_t>(psacx_ctx*, const uint8_t*, uint64_t, const uint32_t*, bool, const uint64_t*, const uint64_t*, uint32_t, const uint16_t*,
                                 const uint8_t*, const uint64_t*, uint64_t, uint32_t, uint64_t, uint64_t, uint64_t*, uint64_t*, uint64_t*);

// The host-pointer forms of the two: everything is staged in device memory of its own for the time of the call, the table is built
// when k > 0, and the result arrays come back: lb and ub of q entries, or with longest (psacx_match_*) len, lb and ub of q
// entries, of poff[q] in the suffix mode.  offsets != nullptr: the text is the string set of those m + 1 offsets (psacx_*_gsa_*);
// they are checked and the bitmap of the string ends is built on the device.
template <typename T>
int search_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, const uint8_t* pat,
                const uint64_t* poff, uint64_t q, uint32_t k, bool longest, uint32_t flags, uint64_t max_len, T* len, T* lb, T* ub) {
    if (!c) return PSACX_EINVAL;
    if (flags & ~(uint32_t)PSACX_MATCH_SUFFIXES) return PSACX_EINVAL;
    if (q == 0) return PSACX_OK;
    if (!text || !SA || !poff || n == 0) return PSACX_EINVAL;
    if (offsets && (m == 0 || m > n)) return PSACX_EINVAL;
    uint64_t S = 0;
    PSACX_TRY(pattern_batch_valid(pat, poff, q, &S));
    const uint64_t entries = (flags & PSACX_MATCH_SUFFIXES) ? S : q;
    if (entries && ((longest && !len) || !lb || !ub)) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    Staging s(c, longest ? "match" : "locate");
    const uint8_t* d_text = (const uint8_t*)s.upload(text, n);
    const T* d_SA = (const T*)s.upload(SA, n * sizeof(T));
    const DeviceBatch b = s.upload_batch(pat, poff, q);
    T* d_len = longest ? (T*)s.alloc(entries * sizeof(T)) : nullptr;
    T* d_lb = (T*)s.alloc(entries * sizeof(T));
    T* d_ub = (T*)s.alloc(entries * sizeof(T));
    const uint32_t* d_ends = offsets ? s.string_ends(offsets, m, n) : nullptr;
    uint16_t codes[256];
    const T* d_table = staged_lookup_table<T>(s, d_text, n, d_ends, k, codes);
    const uint16_t* code = k ? codes : nullptr;
    if (s.rc == PSACX_OK)
        s.rc = longest ? match_dev<T>(c, d_text, n, d_ends, offsets != nullptr, d_SA, d_table, k, code, b.pat, b.poff, q, flags, max_len, entries, d_len,
                                      d_lb, d_ub)
                       : locate_dev<T>(c, d_text, n, d_SA, d_table, k, code, b.pat, b.poff, q, d_lb, d_ub, d_ends);
    s.download(len, d_len, entries * sizeof(T));
    s.download(lb, d_lb, entries * sizeof(T));
    s.download(ub, d_ub, entries * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// psacx_string_ends_dev: the bitmap check.hip builds for its own use, handed to the caller
static int string_ends_dev(psacx_ctx* c, const uint64_t* d_off, uint64_t m, uint64_t n, uint32_t* d_ends, uint64_t* words) {
    if (!c || !words || n == 0) return PSACX_EINVAL;
    *words = (n >> 5) + 1;
    if (!d_ends) return PSACX_OK;                     // size query
    if (!d_off || m == 0 || m > n) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(string_offsets_valid_dev(c, d_off, m, n));
    PSACX_TRY(string_ends_bitmap_dev(c, d_off, m, n, d_ends));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// psacx_occurrences_dev_*: the counts of the intervals, their scan over q + 1 entries, and the expansion
template <typename T>
int occurrences_dev(psacx_ctx* c, const T* d_SA, uint64_t n, const uint64_t* d_off, uint64_t m, const T* d_lb, const T* d_ub, uint64_t q,
                    uint64_t limit, uint64_t* d_start, T* d_pos, T* d_sid, uint64_t cap, uint64_t* total) {
    if (!c || !total) return PSACX_EINVAL;
    *total = 0;
    if ((d_sid && (!d_off || !d_pos)) || (d_off && (m == 0 || m > n))) return PSACX_EINVAL;
    if (q == 0) {
        if (d_start) { PSACX_HIP(c, hipSetDevice(c->device)); PSACX_HIP(c, hipMemsetAsync(d_start, 0, sizeof(uint64_t), c->stream)); PSACX_HIP(c, hipStreamSynchronize(c->stream)); }
        return PSACX_OK;
    }
    if (!d_SA || !d_lb || !d_ub || !d_start || n == 0) return PSACX_EINVAL;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    PSACX_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL((occ_counts_kernel<T>), dim3(grid_for(c, q + 1, 256, 8)), dim3(256), 0, c->stream, d_lb, d_ub, q, n, limit, d_start);
    PSACX_HIP(c, hipGetLastError());
    PSACX_TRY(scan_total_u64_dev(c, d_start, q + 1, total));
    if (!d_pos) return PSACX_OK;                      // size query
    if (*total > cap) return PSACX_ERANGE;
    if (*total == 0) return PSACX_OK;
    const uint64_t tiles = (*total + OCC_TILE - 1) / OCC_TILE;
    hipLaunchKernelGGL((occ_expand_kernel<T>), dim3(grid_for(c, tiles * 256, 256, 8)), dim3(256), 0, c->stream, d_SA, n, d_off, m, d_lb, q,
                       (const uint64_t*)d_start, *total, d_pos, d_sid);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// the scan for callers outside this file (query_calls.hpp)
int exclusive_scan_u64_dev(psacx_ctx* c, uint64_t* d_a, uint64_t len) { return exclusive_scan_dev<uint64_t>(c, d_a, len); }
int exclusive_scan_u32_dev(psacx_ctx* c, uint32_t* d_a, uint64_t len) { return exclusive_scan_dev<uint32_t>(c, d_a, len); }
int scan_total_u64_dev(psacx_ctx* c, uint64_t* d_a, uint64_t len, uint64_t* total) {
    PSACX_TRY(exclusive_scan_dev<uint64_t>(c, d_a, len));
    PSACX_HIP(c, hipMemcpyAsync(total, d_a + len - 1, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}
uint64_t exclusive_scan_slab_bytes(uint64_t len) {
    return (len + 256 * LOCATE_SCAN_ITEMS - 1) / (256 * LOCATE_SCAN_ITEMS) * sizeof(unsigned long long) + 4096;
}

} // namespace psacx

using namespace psacx;

extern "C" {

int psacx_string_ends_dev(psacx_ctx* c, const uint64_t* off, uint64_t m, uint64_t n, uint32_t* ends, uint64_t* words) { return string_ends_dev(c, off, m, n, ends, words); }

// The _gsa forms insist on what makes them so: the table needs the bitmap unless it is the size query, the search needs it
// where there is something to search, the host-pointer forms need the offsets.
#define PSACX_LOCATE_ABI(S, T)                                                                                                                 \
    int psacx_lookup_table_dev_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const T* sa, uint32_t k, T* table, uint16_t code[256],           \
                                   uint32_t* sigma, uint64_t* entries) {                                                                         \
        return lookup_table_dev<T>(c, t, n, sa, k, table, code, sigma, entries);                                                               \
    }                                                                                                                                            \
    int psacx_lookup_table_gsa_dev_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, uint32_t k, T* table,                   \
                                       uint16_t code[256], uint32_t* sigma, uint64_t* entries) {                                                 \
        return ends || !table ? lookup_table_dev<T>(c, t, n, nullptr, k, table, code, sigma, entries, ends) : PSACX_EINVAL;                     \
    }                                                                                                                                            \
    int psacx_locate_dev_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const T* sa, const T* table, uint32_t k, const uint16_t code[256],     \
                             const uint8_t* pat, const uint64_t* poff, uint64_t q, T* lb, T* ub) {                                               \
        return locate_dev<T>(c, t, n, sa, table, k, code, pat, poff, q, lb, ub);                                                                \
    }                                                                                                                                            \
    int psacx_locate_gsa_dev_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const T* sa, const T* table, uint32_t k,     \
                                 const uint16_t code[256], const uint8_t* pat, const uint64_t* poff, uint64_t q, T* lb, T* ub) {                 \
        return c && q && !ends ? PSACX_EINVAL : locate_dev<T>(c, t, n, sa, table, k, code, pat, poff, q, lb, ub, ends);                         \
    }                                                                                                                                            \
    int psacx_locate_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const T* sa, const uint8_t* pat, const uint64_t* poff, uint64_t q,         \
                         uint32_t k, T* lb, T* ub) {                                                                                             \
        return search_host<T>(c, t, n, nullptr, 0, sa, pat, poff, q, k, false, 0, 0, nullptr, lb, ub);                                          \
    }                                                                                                                                            \
    int psacx_locate_gsa_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const uint8_t* pat,      \
                             const uint64_t* poff, uint64_t q, uint32_t k, T* lb, T* ub) {                                                       \
        return off ? search_host<T>(c, t, n, off, m, sa, pat, poff, q, k, false, 0, 0, nullptr, lb, ub) : PSACX_EINVAL;                         \
    }                                                                                                                                            \
    int psacx_occurrences_dev_##S(psacx_ctx* c, const T* sa, uint64_t n, const uint64_t* off, uint64_t m, const T* lb, const T* ub, uint64_t q, \
                                  uint64_t limit, uint64_t* start, T* pos, T* sid, uint64_t cap, uint64_t* total) {                              \
        return occurrences_dev<T>(c, sa, n, off, m, lb, ub, q, limit, start, pos, sid, cap, total);                                             \
    }                                                                                                                                            \
    int psacx_match_dev_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const T* sa, const T* table, uint32_t k, const uint16_t code[256],      \
                            const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t flags, uint64_t max_len, uint64_t out_entries,        \
                            T* len, T* lb, T* ub) {                                                                                              \
        return match_dev<T>(c, t, n, nullptr, false, sa, table, k, code, pat, poff, q, flags, max_len, out_entries, len, lb, ub);               \
    }                                                                                                                                            \
    int psacx_match_gsa_dev_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const T* sa, const T* table, uint32_t k,      \
                                const uint16_t code[256], const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t flags,                  \
                                uint64_t max_len, uint64_t out_entries, T* len, T* lb, T* ub) {                                                  \
        return match_dev<T>(c, t, n, ends, true, sa, table, k, code, pat, poff, q, flags, max_len, out_entries, len, lb, ub);                   \
    }                                                                                                                                            \
    int psacx_match_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const T* sa, const uint8_t* pat, const uint64_t* poff, uint64_t q,          \
                        uint32_t k, uint32_t flags, uint64_t max_len, T* len, T* lb, T* ub) {                                                    \
        return search_host<T>(c, t, n, nullptr, 0, sa, pat, poff, q, k, true, flags, max_len, len, lb, ub);                                     \
    }                                                                                                                                            \
    int psacx_match_gsa_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const uint8_t* pat,       \
                            const uint64_t* poff, uint64_t q, uint32_t k, uint32_t flags, uint64_t max_len, T* len, T* lb, T* ub) {              \
        return off ? search_host<T>(c, t, n, off, m, sa, pat, poff, q, k, true, flags, max_len, len, lb, ub) : PSACX_EINVAL;                    \
    }
PSACX_LOCATE_ABI(u32, uint32_t)
PSACX_LOCATE_ABI(u64, uint64_t)
#undef PSACX_LOCATE_ABI

} // extern "C"
