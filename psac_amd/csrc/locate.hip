// locate.hip -- batched pattern search over a suffix array resident in HBM, and the k-mer lookup table in front of it
// (include/psacx.h: "pattern search"; kernels in locate.hpp); the same over string sets and the occurrence lists (locate_gsa.hpp); and
// the longest-match search on top of them (include/psacx.h: "longest match and matching statistics"; kernel in match.hpp).
//
// Stands in for sa_index::locate (the reference's include/seq_query.hpp:246-251) and lookup_index (lookup_table.hpp:36-149),
// which desa-main -c -q drives (src/desa_main.cpp).  One GPU; no LCP, Lc or RMQ is consulted: on one GPU the text is as near as
// they are.
#include "engine.hpp"
#include "locate.hpp"
#include "locate_gsa.hpp"
#include "match.hpp"

namespace psacx {

// check.hip: the offsets of a string set start at 0, end at n and ascend strictly (PSACX_EINVAL otherwise; waits); and the bitmap of
// the string ends of valid offsets, queued on the ctx stream
int string_offsets_valid_dev(psacx_ctx* c, const uint64_t* d_off, uint64_t m, uint64_t n);
int string_ends_bitmap_dev(psacx_ctx* c, const uint64_t* d_off, uint64_t m, uint64_t n, uint32_t* bits);

static const uint64_t LOCATE_MAX_KEYS = 1ull << 30;

// B^k, or 0 if that exceeds LOCATE_MAX_KEYS
static uint64_t key_space(uint32_t B, uint32_t k) {
    uint64_t e = 1;
    for (uint32_t i = 0; i < k; ++i) { e *= B; if (e > LOCATE_MAX_KEYS) return 0; }
    return e;
}

// The table by counting: every text position adds one to the bin of its key, then the bins become their exclusive prefix sums.
// The SA is not consulted -- the table is defined by the text alone and must not inherit a wrong SA.
// tab / B = sigma + 1 / keys = B^k as table_alphabet left them; d_table has keys + 1 entries.  Queued on the ctx stream.
// d_ends != nullptr: the text is a string set with that bitmap of its string ends, and the keys are cut there.
template <typename T>
static int lookup_table_fill(psacx_ctx* c, const uint8_t* d_text, uint64_t n, uint32_t k, uint32_t B, uint64_t keys, const CodeTable& tab, T* d_table,
                             const uint32_t* d_ends = nullptr) {
    const uint64_t E = keys + 1;
    const uint64_t nb = (E + 256 * LOCATE_SCAN_ITEMS - 1) / (256 * LOCATE_SCAN_ITEMS);
    PSACX_TRY(ensure_slab(c, nb * sizeof(unsigned long long) + 4096));
    unsigned long long* d_sums = reinterpret_cast<unsigned long long*>(c->slab);
    PSACX_HIP(c, hipMemsetAsync(d_table, 0, E * sizeof(T), c->stream));
    const int grid = grid_for(c, (n + LOCATE_STRIP - 1) / LOCATE_STRIP, 256, 8);
    if (d_ends && E <= LOCATE_LDS_BINS)
        hipLaunchKernelGGL((kmer_count_kernel<T, true, true>), dim3(grid), dim3(256), 0, c->stream, d_text, n, k, B, keys / B, tab, d_table, E, d_ends);
    else if (d_ends)
        hipLaunchKernelGGL((kmer_count_kernel<T, false, true>), dim3(grid), dim3(256), 0, c->stream, d_text, n, k, B, keys / B, tab, d_table, E, d_ends);
    else if (E <= LOCATE_LDS_BINS)
        hipLaunchKernelGGL((kmer_count_kernel<T, true, false>), dim3(grid), dim3(256), 0, c->stream, d_text, n, k, B, keys / B, tab, d_table, E, d_ends);
    else
        hipLaunchKernelGGL((kmer_count_kernel<T, false, false>), dim3(grid), dim3(256), 0, c->stream, d_text, n, k, B, keys / B, tab, d_table, E, d_ends);
    PSACX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL((scan_sums_kernel<T>), dim3((unsigned)nb), dim3(256), 0, c->stream, (const T*)d_table, E, d_sums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(256), 0, c->stream, d_sums, nb);
    hipLaunchKernelGGL((scan_apply_kernel<T>), dim3((unsigned)nb), dim3(256), 0, c->stream, d_table, E, (const unsigned long long*)d_sums);
    PSACX_HIP(c, hipGetLastError());
    return PSACX_OK;
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

template <typename T, int G>
static void launch_locate(psacx_ctx* c, bool count, const uint8_t* d_text, uint64_t n, const T* d_SA, const T* d_table, uint32_t k, uint32_t B,
                          const CodeTable& tab, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, T* d_lb, T* d_ub,
                          const unsigned long long* d_bad, unsigned long long* d_counters) {
    const int grid = grid_for(c, q * G, 256, 8);
    if (count)
        hipLaunchKernelGGL((locate_kernel<T, G, true>), dim3(grid), dim3(256), 0, c->stream, d_text, n, d_SA, d_table, k, B, tab, d_pat, d_poff, q,
                           d_lb, d_ub, d_bad, d_counters);
    else
        hipLaunchKernelGGL((locate_kernel<T, G, false>), dim3(grid), dim3(256), 0, c->stream, d_text, n, d_SA, d_table, k, B, tab, d_pat, d_poff, q,
                           d_lb, d_ub, d_bad, d_counters);
}

// d_ends != nullptr: psacx_locate_gsa_dev_* (one pattern per lane whatever PSACX_OPT_LOCATE_SHAPE says)
template <typename T>
int locate_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const T* d_SA, const T* d_table, uint32_t k, const uint16_t* code,
               const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, T* d_lb, T* d_ub, const uint32_t* d_ends = nullptr) {
    if (!c) return PSACX_EINVAL;
    if ((d_table == nullptr) != (k == 0) || (code == nullptr) != (k == 0)) return PSACX_EINVAL;
    if (q == 0) return PSACX_OK;
    if (!d_text || !d_SA || !d_pat || !d_poff || !d_lb || !d_ub || n == 0) return PSACX_EINVAL;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    CodeTable tab;
    std::memset(&tab, 0, sizeof(tab));
    uint32_t B = 1;
    if (k) {
        std::memcpy(tab.c, code, sizeof(tab.c));
        for (int ch = 0; ch < 256; ++ch) B = std::max<uint32_t>(B, (uint32_t)tab.c[ch] + 1);
        if (B < 2 || key_space(B, k) == 0) return PSACX_EINVAL;
    }
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(ensure_slab(c, 4096));
    unsigned long long* d_words = reinterpret_cast<unsigned long long*>(c->slab);      // [0] malformed offsets, [1], [2] the fetch counters
    PSACX_HIP(c, hipMemsetAsync(d_words, 0, 3 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(locate_offsets_kernel, dim3(grid_for(c, q, 256, 8)), dim3(256), 0, c->stream, d_poff, q, d_words);
    PSACX_HIP(c, hipGetLastError());
    const bool count = c->knobs.locate_count;
    if (d_ends) {
        const int grid = grid_for(c, q, 256, 8);
        if (count)
            hipLaunchKernelGGL((locate_gsa_kernel<T, true>), dim3(grid), dim3(256), 0, c->stream, d_text, n, d_ends, d_SA, d_table, k, B, tab, d_pat, d_poff,
                               q, d_lb, d_ub, (const unsigned long long*)d_words, d_words + 1);
        else
            hipLaunchKernelGGL((locate_gsa_kernel<T, false>), dim3(grid), dim3(256), 0, c->stream, d_text, n, d_ends, d_SA, d_table, k, B, tab, d_pat, d_poff,
                               q, d_lb, d_ub, (const unsigned long long*)d_words, d_words + 1);
    } else if (c->knobs.locate_shape == 2)
        launch_locate<T, 8>(c, count, d_text, n, d_SA, d_table, k, B, tab, d_pat, d_poff, q, d_lb, d_ub, d_words, d_words + 1);
    else
        launch_locate<T, 1>(c, count, d_text, n, d_SA, d_table, k, B, tab, d_pat, d_poff, q, d_lb, d_ub, d_words, d_words + 1);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long words[3] = {0, 0, 0};
    PSACX_HIP(c, hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (words[0]) return PSACX_EINVAL;                // poff[0] != 0 or a descending pair: the kernel wrote nothing
    c->stats.locate_fetches[0] = words[1];
    c->stats.locate_fetches[1] = words[2];
    return PSACX_OK;
}

// The host-pointer form: everything is staged in device memory of its own for the time of the call (the slab belongs to the calls
// above), the table is built when k > 0, and the two result arrays come back.  offsets != nullptr: the text is the string set
// of those m + 1 offsets (psacx_locate_gsa_*); they are checked and the bitmap of the string ends is built on the device.
template <typename T>
int locate_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, const uint8_t* pat,
                const uint64_t* poff, uint64_t q, uint32_t k, T* lb, T* ub) {
    if (!c) return PSACX_EINVAL;
    if (q == 0) return PSACX_OK;
    if (!text || !SA || !poff || !lb || !ub || n == 0) return PSACX_EINVAL;
    if (offsets && (m == 0 || m > n)) return PSACX_EINVAL;
    if (poff[0] != 0) return PSACX_EINVAL;
    for (uint64_t i = 0; i < q; ++i) if (poff[i + 1] < poff[i]) return PSACX_EINVAL;
    if (poff[q] && !pat) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    enum { TEXT, SA_, PAT, POFF, OFF, LB, UB, ENDS, TABLE, NBUF };
    size_t sizes[NBUF] = {n, n * sizeof(T), poff[q] ? poff[q] : 1, (q + 1) * sizeof(uint64_t), offsets ? (m + 1) * sizeof(uint64_t) : 0,
                          q * sizeof(T), q * sizeof(T), offsets ? ((n >> 5) + 1) * sizeof(uint32_t) : 0, 0};
    const void* src[5] = {text, SA, pat, poff, offsets};
    void* d[NBUF] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = PSACX_OK;
    auto alloc = [&](int b) {
        if (rc != PSACX_OK || sizes[b] == 0) return;
        const hipError_t e = hipMalloc(&d[b], sizes[b]);
        if (e != hipSuccess) { c->hip_err = std::string("hipMalloc(locate): ") + hipGetErrorString(e); (void)hipGetLastError(); rc = PSACX_ENOMEM; }
    };
    auto step = [&](hipError_t r) { if (rc == PSACX_OK && r != hipSuccess) { c->hip_err = hipGetErrorString(r); (void)hipGetLastError(); rc = PSACX_EHIP; } };
    for (int b = TEXT; b <= ENDS; ++b) alloc(b);
    for (int b = TEXT; b <= OFF && rc == PSACX_OK; ++b)
        if (src[b] && (b != PAT || poff[q])) step(hipMemcpyAsync(d[b], src[b], b == PAT ? (size_t)poff[q] : sizes[b], hipMemcpyHostToDevice, c->stream));
    if (rc == PSACX_OK && offsets) rc = string_offsets_valid_dev(c, (const uint64_t*)d[OFF], m, n);
    if (rc == PSACX_OK && offsets) rc = string_ends_bitmap_dev(c, (const uint64_t*)d[OFF], m, n, (uint32_t*)d[ENDS]);
    CodeTable tab;
    if (rc == PSACX_OK && k) {                        // one histogram for the alphabet, then the table sized by it
        uint32_t sigma = 0;
        uint64_t keys = 0;
        rc = table_alphabet(c, (const uint8_t*)d[TEXT], n, k, tab, sigma, keys);
        if (rc == PSACX_OK) { sizes[TABLE] = (keys + 1) * sizeof(T); alloc(TABLE); }
        if (rc == PSACX_OK) rc = lookup_table_fill<T>(c, (const uint8_t*)d[TEXT], n, k, sigma + 1, keys, tab, (T*)d[TABLE], (const uint32_t*)d[ENDS]);
    }
    if (rc == PSACX_OK)
        rc = locate_dev<T>(c, (const uint8_t*)d[TEXT], n, (const T*)d[SA_], (const T*)d[TABLE], k, k ? tab.c : nullptr, (const uint8_t*)d[PAT],
                           (const uint64_t*)d[POFF], q, (T*)d[LB], (T*)d[UB], (const uint32_t*)d[ENDS]);
    if (rc == PSACX_OK) {
        step(hipMemcpyAsync(lb, d[LB], sizes[LB], hipMemcpyDeviceToHost, c->stream));
        step(hipMemcpyAsync(ub, d[UB], sizes[UB], hipMemcpyDeviceToHost, c->stream));
    }
    step(hipStreamSynchronize(c->stream));
    for (int b = 0; b < NBUF; ++b) if (d[b]) (void)hipFree(d[b]);
    return rc;
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

template <typename T>
int locate_gsa_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, const T* d_table, uint32_t k,
                   const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, T* d_lb, T* d_ub) {
    if (c && q && !d_ends) return PSACX_EINVAL;
    return locate_dev<T>(c, d_text, n, d_SA, d_table, k, code, d_pat, d_poff, q, d_lb, d_ub, d_ends);
}

// psacx_match_dev_* / psacx_match_gsa_dev_* (set: the string-set form, which needs d_ends): the checks of locate_dev, the offsets
// kernel with the rule for out_entries, and one launch of match_kernel.
template <typename T>
int match_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, bool set, const T* d_SA, const T* d_table, uint32_t k,
              const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, uint32_t flags, uint64_t max_len, uint64_t out_entries,
              T* d_len, T* d_lb, T* d_ub) {
    if (!c) return PSACX_EINVAL;
    if (flags & ~(uint32_t)PSACX_MATCH_SUFFIXES) return PSACX_EINVAL;
    if ((d_table == nullptr) != (k == 0) || (code == nullptr) != (k == 0)) return PSACX_EINVAL;
    if (q == 0) return out_entries == 0 ? PSACX_OK : PSACX_EINVAL;
    const bool suffixes = (flags & PSACX_MATCH_SUFFIXES) != 0;
    if (!suffixes && out_entries != q) return PSACX_EINVAL;
    if (!d_text || !d_SA || !d_pat || !d_poff || n == 0 || (set && !d_ends)) return PSACX_EINVAL;
    if (out_entries && (!d_len || !d_lb || !d_ub)) return PSACX_EINVAL;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    CodeTable tab;
    std::memset(&tab, 0, sizeof(tab));
    uint32_t B = 1;
    if (k) {
        std::memcpy(tab.c, code, sizeof(tab.c));
        for (int ch = 0; ch < 256; ++ch) B = std::max<uint32_t>(B, (uint32_t)tab.c[ch] + 1);
        if (B < 2 || key_space(B, k) == 0) return PSACX_EINVAL;
    }
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(ensure_slab(c, 4096));
    unsigned long long* d_words = reinterpret_cast<unsigned long long*>(c->slab);      // [0] malformed offsets, [1], [2] the fetch counters
    PSACX_HIP(c, hipMemsetAsync(d_words, 0, 3 * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(match_offsets_kernel, dim3(grid_for(c, q, 256, 8)), dim3(256), 0, c->stream, d_poff, q, suffixes, out_entries, d_words);
    PSACX_HIP(c, hipGetLastError());
    const bool count = c->knobs.locate_count;
    if (out_entries) {                                // (a suffix batch of empty patterns has nothing to search)
        const int grid = grid_for(c, out_entries, 256, 8);
        const uint32_t mode = suffixes ? MATCH_MODE_SUFFIXES : 0u;
#define PSACX_MATCH_LAUNCH(SET, COUNT)                                                                                                        \
        hipLaunchKernelGGL((match_kernel<T, SET, COUNT>), dim3(grid), dim3(256), 0, c->stream, d_text, n, d_ends, d_SA, d_table, k, B, tab, d_pat,   \
                           d_poff, q, mode, max_len, out_entries, d_len, d_lb, d_ub, (const unsigned long long*)d_words, d_words + 1)
        if (set) { if (count) PSACX_MATCH_LAUNCH(true, true); else PSACX_MATCH_LAUNCH(true, false); }
        else { if (count) PSACX_MATCH_LAUNCH(false, true); else PSACX_MATCH_LAUNCH(false, false); }
#undef PSACX_MATCH_LAUNCH
        PSACX_HIP(c, hipGetLastError());
    }
    unsigned long long words[3] = {0, 0, 0};
    PSACX_HIP(c, hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (words[0]) return PSACX_EINVAL;                // malformed offsets, or poff[q] != out_entries: the kernel wrote nothing
    c->stats.locate_fetches[0] = words[1];
    c->stats.locate_fetches[1] = words[2];
    return PSACX_OK;
}

// The host-pointer forms of the above: locate_host with three result arrays of q entries, or of poff[q] in the suffix mode.
template <typename T>
int match_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, const uint8_t* pat,
               const uint64_t* poff, uint64_t q, uint32_t k, uint32_t flags, uint64_t max_len, T* len, T* lb, T* ub) {
    if (!c) return PSACX_EINVAL;
    if (flags & ~(uint32_t)PSACX_MATCH_SUFFIXES) return PSACX_EINVAL;
    if (q == 0) return PSACX_OK;
    if (!text || !SA || !poff || n == 0) return PSACX_EINVAL;
    if (offsets && (m == 0 || m > n)) return PSACX_EINVAL;
    if (poff[0] != 0) return PSACX_EINVAL;
    for (uint64_t i = 0; i < q; ++i) if (poff[i + 1] < poff[i]) return PSACX_EINVAL;
    if (poff[q] && !pat) return PSACX_EINVAL;
    const uint64_t entries = (flags & PSACX_MATCH_SUFFIXES) ? poff[q] : q;
    if (entries && (!len || !lb || !ub)) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    enum { TEXT, SA_, PAT, POFF, OFF, LEN, LB, UB, ENDS, TABLE, NBUF };
    size_t sizes[NBUF] = {n, n * sizeof(T), poff[q] ? poff[q] : 1, (q + 1) * sizeof(uint64_t), offsets ? (m + 1) * sizeof(uint64_t) : 0,
                          entries * sizeof(T), entries * sizeof(T), entries * sizeof(T), offsets ? ((n >> 5) + 1) * sizeof(uint32_t) : 0, 0};
    const void* src[5] = {text, SA, pat, poff, offsets};
    void* d[NBUF] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = PSACX_OK;
    auto alloc = [&](int b) {
        if (rc != PSACX_OK || sizes[b] == 0) return;
        const hipError_t e = hipMalloc(&d[b], sizes[b]);
        if (e != hipSuccess) { c->hip_err = std::string("hipMalloc(match): ") + hipGetErrorString(e); (void)hipGetLastError(); rc = PSACX_ENOMEM; }
    };
    auto step = [&](hipError_t r) { if (rc == PSACX_OK && r != hipSuccess) { c->hip_err = hipGetErrorString(r); (void)hipGetLastError(); rc = PSACX_EHIP; } };
    for (int b = TEXT; b <= ENDS; ++b) alloc(b);
    for (int b = TEXT; b <= OFF && rc == PSACX_OK; ++b)
        if (src[b] && (b != PAT || poff[q])) step(hipMemcpyAsync(d[b], src[b], b == PAT ? (size_t)poff[q] : sizes[b], hipMemcpyHostToDevice, c->stream));
    if (rc == PSACX_OK && offsets) rc = string_offsets_valid_dev(c, (const uint64_t*)d[OFF], m, n);
    if (rc == PSACX_OK && offsets) rc = string_ends_bitmap_dev(c, (const uint64_t*)d[OFF], m, n, (uint32_t*)d[ENDS]);
    CodeTable tab;
    if (rc == PSACX_OK && k) {
        uint32_t sigma = 0;
        uint64_t keys = 0;
        rc = table_alphabet(c, (const uint8_t*)d[TEXT], n, k, tab, sigma, keys);
        if (rc == PSACX_OK) { sizes[TABLE] = (keys + 1) * sizeof(T); alloc(TABLE); }
        if (rc == PSACX_OK) rc = lookup_table_fill<T>(c, (const uint8_t*)d[TEXT], n, k, sigma + 1, keys, tab, (T*)d[TABLE], (const uint32_t*)d[ENDS]);
    }
    if (rc == PSACX_OK)
        rc = match_dev<T>(c, (const uint8_t*)d[TEXT], n, (const uint32_t*)d[ENDS], offsets != nullptr, (const T*)d[SA_], (const T*)d[TABLE], k,
                          k ? tab.c : nullptr, (const uint8_t*)d[PAT], (const uint64_t*)d[POFF], q, flags, max_len, entries, (T*)d[LEN], (T*)d[LB],
                          (T*)d[UB]);
    if (rc == PSACX_OK && entries) {
        step(hipMemcpyAsync(len, d[LEN], sizes[LEN], hipMemcpyDeviceToHost, c->stream));
        step(hipMemcpyAsync(lb, d[LB], sizes[LB], hipMemcpyDeviceToHost, c->stream));
        step(hipMemcpyAsync(ub, d[UB], sizes[UB], hipMemcpyDeviceToHost, c->stream));
    }
    step(hipStreamSynchronize(c->stream));
    for (int b = 0; b < NBUF; ++b) if (d[b]) (void)hipFree(d[b]);
    return rc;
}

// psacx_occurrences_dev_*: the counts of the intervals, their scan (the kernels of the table's scan, over q + 1 entries), and
// the expansion.  The scan's block sums live in the slab, which grows with q as it does with the table's size.
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
    const uint64_t E = q + 1;
    const uint64_t nb = (E + 256 * LOCATE_SCAN_ITEMS - 1) / (256 * LOCATE_SCAN_ITEMS);
    PSACX_TRY(ensure_slab(c, nb * sizeof(unsigned long long) + 4096));
    unsigned long long* d_sums = reinterpret_cast<unsigned long long*>(c->slab);
    hipLaunchKernelGGL((occ_counts_kernel<T>), dim3(grid_for(c, E, 256, 8)), dim3(256), 0, c->stream, d_lb, d_ub, q, n, limit, d_start);
    PSACX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL((scan_sums_kernel<uint64_t>), dim3((unsigned)nb), dim3(256), 0, c->stream, (const uint64_t*)d_start, E, d_sums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(256), 0, c->stream, d_sums, nb);
    hipLaunchKernelGGL((scan_apply_kernel<uint64_t>), dim3((unsigned)nb), dim3(256), 0, c->stream, d_start, E, (const unsigned long long*)d_sums);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipMemcpyAsync(total, d_start + q, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
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

} // namespace psacx

using namespace psacx;

extern "C" {

int psacx_lookup_table_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, uint32_t k, uint32_t* table, uint16_t code[256],
                               uint32_t* sigma, uint64_t* entries) { return lookup_table_dev<uint32_t>(c, t, n, sa, k, table, code, sigma, entries); }
int psacx_lookup_table_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, uint32_t k, uint64_t* table, uint16_t code[256],
                               uint32_t* sigma, uint64_t* entries) { return lookup_table_dev<uint64_t>(c, t, n, sa, k, table, code, sigma, entries); }
int psacx_locate_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, const uint32_t* table, uint32_t k, const uint16_t code[256],
                         const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t* lb, uint32_t* ub) {
    return locate_dev<uint32_t>(c, t, n, sa, table, k, code, pat, poff, q, lb, ub);
}
int psacx_locate_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, const uint64_t* table, uint32_t k, const uint16_t code[256],
                         const uint8_t* pat, const uint64_t* poff, uint64_t q, uint64_t* lb, uint64_t* ub) {
    return locate_dev<uint64_t>(c, t, n, sa, table, k, code, pat, poff, q, lb, ub);
}
int psacx_locate_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k,
                     uint32_t* lb, uint32_t* ub) { return locate_host<uint32_t>(c, t, n, nullptr, 0, sa, pat, poff, q, k, lb, ub); }
int psacx_locate_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k,
                     uint64_t* lb, uint64_t* ub) { return locate_host<uint64_t>(c, t, n, nullptr, 0, sa, pat, poff, q, k, lb, ub); }

int psacx_string_ends_dev(psacx_ctx* c, const uint64_t* off, uint64_t m, uint64_t n, uint32_t* ends, uint64_t* words) { return string_ends_dev(c, off, m, n, ends, words); }
int psacx_lookup_table_gsa_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, uint32_t k, uint32_t* table, uint16_t code[256],
                                   uint32_t* sigma, uint64_t* entries) {
    return ends || !table ? lookup_table_dev<uint32_t>(c, t, n, nullptr, k, table, code, sigma, entries, ends) : PSACX_EINVAL;     // (the size query needs no bitmap)
}
int psacx_lookup_table_gsa_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, uint32_t k, uint64_t* table, uint16_t code[256],
                                   uint32_t* sigma, uint64_t* entries) {
    return ends || !table ? lookup_table_dev<uint64_t>(c, t, n, nullptr, k, table, code, sigma, entries, ends) : PSACX_EINVAL;
}
int psacx_locate_gsa_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint32_t* sa, const uint32_t* table, uint32_t k,
                             const uint16_t code[256], const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t* lb, uint32_t* ub) {
    return locate_gsa_dev<uint32_t>(c, t, n, ends, sa, table, k, code, pat, poff, q, lb, ub);
}
int psacx_locate_gsa_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint64_t* sa, const uint64_t* table, uint32_t k,
                             const uint16_t code[256], const uint8_t* pat, const uint64_t* poff, uint64_t q, uint64_t* lb, uint64_t* ub) {
    return locate_gsa_dev<uint64_t>(c, t, n, ends, sa, table, k, code, pat, poff, q, lb, ub);
}
int psacx_locate_gsa_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* sa, const uint8_t* pat,
                         const uint64_t* poff, uint64_t q, uint32_t k, uint32_t* lb, uint32_t* ub) {
    return off ? locate_host<uint32_t>(c, t, n, off, m, sa, pat, poff, q, k, lb, ub) : PSACX_EINVAL;
}
int psacx_locate_gsa_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* sa, const uint8_t* pat,
                         const uint64_t* poff, uint64_t q, uint32_t k, uint64_t* lb, uint64_t* ub) {
    return off ? locate_host<uint64_t>(c, t, n, off, m, sa, pat, poff, q, k, lb, ub) : PSACX_EINVAL;
}
int psacx_occurrences_dev_u32(psacx_ctx* c, const uint32_t* sa, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* lb, const uint32_t* ub,
                              uint64_t q, uint64_t limit, uint64_t* start, uint32_t* pos, uint32_t* sid, uint64_t cap, uint64_t* total) {
    return occurrences_dev<uint32_t>(c, sa, n, off, m, lb, ub, q, limit, start, pos, sid, cap, total);
}
int psacx_occurrences_dev_u64(psacx_ctx* c, const uint64_t* sa, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* lb, const uint64_t* ub,
                              uint64_t q, uint64_t limit, uint64_t* start, uint64_t* pos, uint64_t* sid, uint64_t cap, uint64_t* total) {
    return occurrences_dev<uint64_t>(c, sa, n, off, m, lb, ub, q, limit, start, pos, sid, cap, total);
}
int psacx_match_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, const uint32_t* table, uint32_t k, const uint16_t code[256],
                        const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t flags, uint64_t max_len, uint64_t out_entries, uint32_t* len,
                        uint32_t* lb, uint32_t* ub) {
    return match_dev<uint32_t>(c, t, n, nullptr, false, sa, table, k, code, pat, poff, q, flags, max_len, out_entries, len, lb, ub);
}
int psacx_match_gsa_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint32_t* sa, const uint32_t* table, uint32_t k,
                            const uint16_t code[256], const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t flags, uint64_t max_len,
                            uint64_t out_entries, uint32_t* len, uint32_t* lb, uint32_t* ub) {
    return match_dev<uint32_t>(c, t, n, ends, true, sa, table, k, code, pat, poff, q, flags, max_len, out_entries, len, lb, ub);
}
int psacx_match_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k,
                    uint32_t flags, uint64_t max_len, uint32_t* len, uint32_t* lb, uint32_t* ub) {
    return match_host<uint32_t>(c, t, n, nullptr, 0, sa, pat, poff, q, k, flags, max_len, len, lb, ub);
}
int psacx_match_gsa_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* sa, const uint8_t* pat,
                        const uint64_t* poff, uint64_t q, uint32_t k, uint32_t flags, uint64_t max_len, uint32_t* len, uint32_t* lb, uint32_t* ub) {
    return off ? match_host<uint32_t>(c, t, n, off, m, sa, pat, poff, q, k, flags, max_len, len, lb, ub) : PSACX_EINVAL;
}
int psacx_match_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, const uint64_t* table, uint32_t k, const uint16_t code[256],
                        const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t flags, uint64_t max_len, uint64_t out_entries, uint64_t* len,
                        uint64_t* lb, uint64_t* ub) {
    return match_dev<uint64_t>(c, t, n, nullptr, false, sa, table, k, code, pat, poff, q, flags, max_len, out_entries, len, lb, ub);
}
int psacx_match_gsa_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint64_t* sa, const uint64_t* table, uint32_t k,
                            const uint16_t code[256], const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t flags, uint64_t max_len,
                            uint64_t out_entries, uint64_t* len, uint64_t* lb, uint64_t* ub) {
    return match_dev<uint64_t>(c, t, n, ends, true, sa, table, k, code, pat, poff, q, flags, max_len, out_entries, len, lb, ub);
}
int psacx_match_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k,
                    uint32_t flags, uint64_t max_len, uint64_t* len, uint64_t* lb, uint64_t* ub) {
    return match_host<uint64_t>(c, t, n, nullptr, 0, sa, pat, poff, q, k, flags, max_len, len, lb, ub);
}
int psacx_match_gsa_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* sa, const uint8_t* pat,
                        const uint64_t* poff, uint64_t q, uint32_t k, uint32_t flags, uint64_t max_len, uint64_t* len, uint64_t* lb, uint64_t* ub) {
    return off ? match_host<uint64_t>(c, t, n, off, m, sa, pat, poff, q, k, flags, max_len, len, lb, ub) : PSACX_EINVAL;
}

} // extern "C"
