// fm.hip -- the FM-index in HBM: psacx_fm_index_dev_* builds the blob from the outputs of psacx_bwt_dev_*, psacx_fm_count_dev_* is the
// backward search, psacx_fm_occurrences_dev_* the occurrence lists through the sampled suffix array, psacx_fm_search_* the host-pointer
// form; psacx_fm_text_samples_dev_* samples the ranks of text positions and psacx_fm_extract_dev_* gives the bytes of the text back from
// them (include/psacx.h: "FM-index"; kernels and the layout of the blob in fm.hpp).  The reference has no counterpart.
#include "engine.hpp"
#include "fm.hpp"
#include "search.hpp"
#include "staging.hpp"

namespace psacx {

// The layout a descriptor stands for, or PSACX_EINVAL where its bits / words do not follow from n, sigma, sample and marks, or a code
// lies beyond sigma.
template <typename T>
static int fm_view(const psacx_fm_info* info, const uint64_t* d_fm, FmLayout& Y, CodeTable& code) {
    if (!info || !d_fm) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(info->n));
    if (info->sigma > 256 || info->bits != fm_bits_of(info->sigma) || info->marks > info->n || (info->sample == 0 && info->marks != 0))
        return PSACX_EINVAL;
    fm_layout(info->n, info->sigma, info->bits, info->sample, info->marks, sizeof(T), Y);
    if (Y.words != info->words) return PSACX_EINVAL;
    for (int ch = 0; ch < 256; ++ch) {
        if (info->code[ch] > info->sigma) return PSACX_EINVAL;
        code.c[ch] = info->code[ch];
    }
    Y.fm = d_fm;
    return PSACX_OK;
}

// psacx_fm_index_dev_*.  The histogram and the number of marks come first and serve the size query; nothing is written to d_fm or
// *info before the two code arrays are there.  Scratch in the ctx slab: the block sums of the scans at its base, then the histogram
// and one count per cell; beside the slab and for the time of the call the two arrays of n 16-bit codes.
// After psacx_profile(ctx, 1) the stages leave their times in psacx_stats, for tools/fm_time.py: ms_kmer the histogram, the mark counts
// and the codes, ms_sort_scatter the levels, ms_rebucket the marks and samples; events on the ctx stream around each.
template <typename T>
int fm_index_dev(psacx_ctx* c, uint64_t n, const uint8_t* d_bwt, const uint32_t* d_first, const T* d_SA, uint64_t sample, uint64_t* d_fm,
                 psacx_fm_info* info) {
    if (!c || !info) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (!d_first || (sample > 0 && !d_SA)) return PSACX_EINVAL;
    if (n && !d_bwt) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    const uint64_t cells = (n >> 6) + 1;
    const uint64_t mask = sample && (sample & (sample - 1)) == 0 ? sample - 1 : 0;
    unsigned long long* d_hist = nullptr;
    uint64_t* d_cnt = nullptr;
    auto layout = [&](Arena& a) {
        (void)a.take<unsigned char>(exclusive_scan_slab_bytes(cells + 1));
        d_hist = a.take<unsigned long long>(512);
        d_cnt = a.take<uint64_t>(cells + 1);
    };
    PSACX_TRY(slab_layout(c, layout));
    struct Marks {                                    // four events, made only under psacx_profile and destroyed on every path
        hipEvent_t e[4]; int made = 0;
        ~Marks() { for (int i = 0; i < made; ++i) (void)hipEventDestroy(e[i]); }
    } ev;
    if (c->profile_ops && d_fm) while (ev.made < 4 && hipEventCreate(&ev.e[ev.made]) == hipSuccess) ++ev.made;
    const bool timed = ev.made == 4;
    auto mark = [&](int i) { if (timed) (void)hipEventRecord(ev.e[i], c->stream); };
    const int lane_grid = grid_for(c, n, 256, 8), wave_grid = grid_for(c, n + 64, 256, 8);

    mark(0);
    unsigned long long hist[512];
    uint64_t marks = 0;
    PSACX_HIP(c, hipMemsetAsync(d_hist, 0, sizeof(hist), c->stream));
    if (n) {
        hipLaunchKernelGGL(fm_hist_kernel, dim3(lane_grid), dim3(256), 0, c->stream, n, d_bwt, d_first, d_hist);
        PSACX_HIP(c, hipGetLastError());
    }
    PSACX_HIP(c, hipMemcpyAsync(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost, c->stream));
    if (sample) {
        hipLaunchKernelGGL((fm_mark_count_kernel<T>), dim3(wave_grid), dim3(256), 0, c->stream, n, d_first, d_SA, sample, mask, d_cnt);
        PSACX_HIP(c, hipGetLastError());
        PSACX_TRY(exclusive_scan_u64_dev(c, d_cnt, cells + 1));
        PSACX_HIP(c, hipMemcpyAsync(&marks, d_cnt + cells, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (marks > n) marks = n;

    // codes, counts and the tables of the blob, on the host from 512 counts
    psacx_fm_info I;
    std::memset(&I, 0, sizeof(I));
    CodeTable code;
    uint64_t cnt[FM_SYMS] = {0}, E[FM_SYMS] = {0}, cw[FM_SYMS] = {0};
    uint32_t sigma = 0;
    for (int ch = 0; ch < 256; ++ch) {
        code.c[ch] = hist[ch] ? (uint16_t)++sigma : (uint16_t)0;
        I.code[ch] = code.c[ch];
        if (hist[ch]) { cnt[sigma] = hist[ch]; E[sigma] = std::min<uint64_t>(hist[256 + ch], hist[ch]); }
    }
    const uint32_t bits = fm_bits_of(sigma);
    FmLayout Y;
    fm_layout(n, sigma, bits, sample, marks, sizeof(T), Y);
    I.n = n; I.words = Y.words; I.sample = sample; I.marks = marks; I.sigma = sigma; I.bits = bits;
    if (!d_fm) { *info = I; return PSACX_OK; }       // size query

    std::vector<uint64_t> tab(FM_TAB_WORDS, 0);
    for (uint32_t s = 1; s <= sigma; ++s) { cw[s] = cnt[s] - E[s]; cw[0] += E[s]; }
    for (uint32_t s = 1; s <= sigma + 1; ++s) tab[FM_TAB_C + s] = tab[FM_TAB_C + s - 1] + cnt[s - 1];
    for (uint32_t l = 0; l < bits; ++l)
        for (uint32_t s = 0; s <= sigma; ++s) if (!((s >> (bits - 1 - l)) & 1u)) tab[FM_TAB_Z + l] += cw[s];
    {   // the start of every code behind the last level: the codes in the order of their reversed bits
        std::vector<uint64_t> startw(1u << bits, 0);
        uint64_t run = 0;
        for (uint32_t rev = 0; rev < (1u << bits); ++rev) {
            uint32_t s = 0;
            for (uint32_t b = 0; b < bits; ++b) if ((rev >> b) & 1u) s |= 1u << (bits - 1 - b);
            startw[s] = run;
            if (s <= sigma) run += cw[s];
        }
        for (uint32_t s = 1; s <= sigma; ++s) tab[FM_TAB_D + s] = tab[FM_TAB_C + s] + E[s] - startw[s];
    }

    Staging s(c, "fm index");
    uint16_t* wa = (uint16_t*)s.alloc(n * sizeof(uint16_t));
    uint16_t* wb = (uint16_t*)s.alloc(n * sizeof(uint16_t));
    if (s.rc != PSACX_OK) return s.rc;
    s.step(hipMemcpyAsync(d_fm + Y.tab, tab.data(), FM_TAB_WORDS * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    if (n) {
        hipLaunchKernelGGL(fm_codes_kernel, dim3(lane_grid), dim3(256), 0, c->stream, n, d_bwt, d_first, code, wa);
        s.step(hipGetLastError());
    }
    mark(1);
    for (uint32_t l = 0; l < bits && s.rc == PSACX_OK; ++l) {
        const unsigned shift = bits - 1 - l;
        const bool last = l + 1 == bits;
        hipLaunchKernelGGL(fm_level_count_kernel, dim3(wave_grid), dim3(256), 0, c->stream, n, (const uint16_t*)wa, shift, d_cnt);
        s.step(hipGetLastError());
        if (s.rc == PSACX_OK) s.rc = exclusive_scan_u64_dev(c, d_cnt, cells);
        if (s.rc != PSACX_OK) break;
        hipLaunchKernelGGL(fm_level_emit_kernel, dim3(wave_grid), dim3(256), 0, c->stream, n, (const uint16_t*)wa, shift, (const uint64_t*)d_cnt,
                           tab[FM_TAB_Z + l], reinterpret_cast<ulonglong2*>(d_fm + 2 * cells * l), last ? (uint16_t*)nullptr : wb);
        s.step(hipGetLastError());
        std::swap(wa, wb);
    }
    mark(2);
    if (sample && s.rc == PSACX_OK) {
        if (Y.words > Y.val_at) s.step(hipMemsetAsync(d_fm + Y.words - 1, 0, sizeof(uint64_t), c->stream));
        hipLaunchKernelGGL((fm_mark_count_kernel<T>), dim3(wave_grid), dim3(256), 0, c->stream, n, d_first, d_SA, sample, mask, d_cnt);
        s.step(hipGetLastError());
        if (s.rc == PSACX_OK) s.rc = exclusive_scan_u64_dev(c, d_cnt, cells + 1);
        if (s.rc == PSACX_OK) {
            hipLaunchKernelGGL((fm_mark_emit_kernel<T>), dim3(wave_grid), dim3(256), 0, c->stream, n, d_first, d_SA, sample, mask, (const uint64_t*)d_cnt,
                               marks, reinterpret_cast<ulonglong2*>(d_fm + Y.marks_at), reinterpret_cast<T*>(d_fm + Y.val_at));
            s.step(hipGetLastError());
        }
    }
    mark(3);
    s.step(hipStreamSynchronize(c->stream));
    if (s.rc != PSACX_OK) return s.rc;
    if (timed) {
        float ms[3] = {0, 0, 0};
        for (int i = 0; i < 3; ++i) (void)hipEventElapsedTime(&ms[i], ev.e[i], ev.e[i + 1]);
        c->stats.ms_kmer = ms[0]; c->stats.ms_sort_scatter = ms[1]; c->stats.ms_rebucket = ms[2];
    }
    *info = I;
    return PSACX_OK;
}

// psacx_fm_count_dev_*: the check of the offsets (search.hpp) through one word of the ctx slab, and one launch
template <typename T>
int fm_count_dev(psacx_ctx* c, const uint64_t* d_fm, const psacx_fm_info* info, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, T* d_lb,
                 T* d_ub) {
    if (!c) return PSACX_EINVAL;
    FmLayout Y;
    CodeTable code;
    PSACX_TRY(fm_view<T>(info, d_fm, Y, code));
    if (q == 0) return PSACX_OK;
    if (!d_pat || !d_poff || !d_lb || !d_ub) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(ensure_slab(c, 4096));
    unsigned long long* d_bad = reinterpret_cast<unsigned long long*>(c->slab);
    PSACX_HIP(c, hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), c->stream));
    const int grid = grid_for(c, q, 256, 8);
    hipLaunchKernelGGL(search_offsets_kernel, dim3(grid), dim3(256), 0, c->stream, d_poff, q, false, (uint64_t)0, d_bad);
    hipLaunchKernelGGL((fm_count_kernel<T>), dim3(grid), dim3(256), 0, c->stream, Y, code, d_pat, d_poff, q, d_lb, d_ub, (const unsigned long long*)d_bad);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long bad = 0;
    PSACX_HIP(c, hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return bad ? PSACX_EINVAL : PSACX_OK;
}

// psacx_fm_occurrences_dev_*: the counts and the scan of psacx_occurrences_dev_*, and the expansion through the walk
template <typename T>
int fm_occurrences_dev(psacx_ctx* c, const uint64_t* d_fm, const psacx_fm_info* info, const uint64_t* d_off, uint64_t m, const T* d_lb, const T* d_ub,
                       uint64_t q, uint64_t limit, uint64_t* d_start, T* d_pos, T* d_sid, uint64_t cap, uint64_t* total) {
    if (!c || !total) return PSACX_EINVAL;
    *total = 0;
    FmLayout Y;
    CodeTable code;
    PSACX_TRY(fm_view<T>(info, d_fm, Y, code));
    if (Y.sample == 0) return PSACX_EINVAL;
    if ((d_sid && (!d_off || !d_pos)) || (d_off && (m == 0 || m > Y.n))) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    if (q == 0) {
        if (d_start) { PSACX_HIP(c, hipMemsetAsync(d_start, 0, sizeof(uint64_t), c->stream)); PSACX_HIP(c, hipStreamSynchronize(c->stream)); }
        return PSACX_OK;
    }
    if (!d_lb || !d_ub || !d_start) return PSACX_EINVAL;
    hipLaunchKernelGGL((occ_counts_kernel<T>), dim3(grid_for(c, q + 1, 256, 8)), dim3(256), 0, c->stream, d_lb, d_ub, q, Y.n, limit, d_start);
    PSACX_HIP(c, hipGetLastError());
    PSACX_TRY(scan_total_u64_dev(c, d_start, q + 1, total));
    if (!d_pos) return PSACX_OK;                      // size query
    if (*total > cap) return PSACX_ERANGE;
    if (*total == 0) return PSACX_OK;
    const uint64_t tiles = (*total + OCC_TILE - 1) / OCC_TILE;
    hipLaunchKernelGGL((fm_occ_kernel<T>), dim3(grid_for(c, tiles * 256, 256, 8)), dim3(256), 0, c->stream, Y, d_off, m, d_lb, q,
                       (const uint64_t*)d_start, *total, d_pos, d_sid);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// the rate the kernels of the text samples work with, at most n + 1, and its shift (fm.hpp)
static uint64_t fm_rate_of(uint64_t rate, uint64_t n, unsigned& shift) {
    if (rate > n) rate = n + 1;
    shift = 64;
    if ((rate & (rate - 1)) == 0) { shift = 0; while ((1ull << shift) < rate) ++shift; }
    return rate;
}

// psacx_fm_text_samples_dev_*: one pass over SA.  Scratch in the ctx slab, for a string set only: the word of the offsets' check at its
// base (string_offsets_valid_dev) and behind it the bitmap of the string ends.
template <typename T>
int fm_text_samples_dev(psacx_ctx* c, uint64_t n, const T* d_SA, const uint64_t* d_off, uint64_t m, uint64_t rate, T* d_ts, uint64_t* entries) {
    if (!c || !entries || rate == 0) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (!d_off) m = 1;
    *entries = n / rate + std::max<uint64_t>(m, 1);
    if (n == 0 || !d_ts) return PSACX_OK;             // nothing to sample; the size query
    if (!d_SA || m == 0 || m > n) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    uint32_t* d_ends = nullptr;
    if (d_off) {
        auto layout = [&](Arena& a) {
            (void)a.take<unsigned char>(4096);
            d_ends = a.take<uint32_t>((n >> 5) + 1);
        };
        PSACX_TRY(slab_layout(c, layout));
        PSACX_TRY(string_offsets_valid_dev(c, d_off, m, n));
        PSACX_TRY(string_ends_bitmap_dev(c, d_off, m, n, d_ends));
    }
    unsigned shift;
    const uint64_t blocks = n / rate, use = fm_rate_of(rate, n, shift);
    hipLaunchKernelGGL((fm_text_samples_kernel<T>), dim3(grid_for(c, n, 256, 8)), dim3(256), 0, c->stream, n, d_SA, (const uint32_t*)d_ends, d_off, m, use,
                       shift, blocks, d_ts);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// psacx_fm_extract_dev_*: the clipped lengths and the segment counts, their two scans, and the walk over tiles of segments.  Scratch in
// the ctx slab: the block sums of the scans at its base (the word of the offsets' check before them), then the q + 1 segment starts.
template <typename T>
int fm_extract_dev(psacx_ctx* c, const uint64_t* d_fm, const psacx_fm_info* info, const T* d_ts, uint64_t rate, const uint64_t* d_off, uint64_t m,
                   const T* d_pos, const T* d_len, uint64_t q, uint64_t* d_start, uint8_t* d_out, uint64_t cap, uint64_t* total) {
    if (!c || !total) return PSACX_EINVAL;
    *total = 0;
    FmLayout Y;
    CodeTable code;
    PSACX_TRY(fm_view<T>(info, d_fm, Y, code));
    if (rate == 0 || !d_ts) return PSACX_EINVAL;
    if (!d_off) m = 1;
    else if (Y.n && (m == 0 || m > Y.n)) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    if (q == 0) {
        if (d_start) { PSACX_HIP(c, hipMemsetAsync(d_start, 0, sizeof(uint64_t), c->stream)); PSACX_HIP(c, hipStreamSynchronize(c->stream)); }
        return PSACX_OK;
    }
    if (!d_pos || !d_len || !d_start) return PSACX_EINVAL;
    uint64_t* d_segs = nullptr;
    auto layout = [&](Arena& a) {
        (void)a.take<unsigned char>(std::max<uint64_t>(exclusive_scan_slab_bytes(q + 1), 4096));
        d_segs = a.take<uint64_t>(q + 1);
    };
    PSACX_TRY(slab_layout(c, layout));
    if (d_off && Y.n) PSACX_TRY(string_offsets_valid_dev(c, d_off, m, Y.n));
    unsigned shift;
    const uint64_t blocks = Y.n / rate, use = fm_rate_of(rate, Y.n, shift);
    hipLaunchKernelGGL((fm_extract_counts_kernel<T>), dim3(grid_for(c, q + 1, 256, 8)), dim3(256), 0, c->stream, Y.n, d_off, m, use, shift, d_pos, d_len, q,
                       d_start, d_segs);
    PSACX_HIP(c, hipGetLastError());
    PSACX_TRY(exclusive_scan_u64_dev(c, d_start, q + 1));
    PSACX_TRY(exclusive_scan_u64_dev(c, d_segs, q + 1));
    uint64_t nsegs = 0;
    PSACX_HIP(c, hipMemcpyAsync(total, d_start + q, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipMemcpyAsync(&nsegs, d_segs + q, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (!d_out) return PSACX_OK;                      // size query
    if (*total > cap) return PSACX_ERANGE;
    if (*total == 0) return PSACX_OK;
    FmDecode dec;
    std::memset(&dec, 0, sizeof(dec));
    for (int ch = 0; ch < 256; ++ch) if (info->code[ch]) dec.b[info->code[ch]] = (uint8_t)ch;
    const uint64_t tiles = (nsegs + OCC_TILE - 1) / OCC_TILE;
    hipLaunchKernelGGL((fm_extract_kernel<T>), dim3(grid_for(c, tiles * 256, 256, 8)), dim3(256), 0, c->stream, Y, dec, d_ts, blocks, use, shift, d_off, m,
                       d_pos, q, (const uint64_t*)d_start, (const uint64_t*)d_segs, nsegs, d_out);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// psacx_fm_search_*: text and SA are staged, the bitmap of the string ends, the BWT and the index are built beside them, the patterns
// are counted and, with pos, listed.  Everything allocated is freed on every path.  Without pos the index carries no samples.
template <typename T>
int fm_search_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, uint64_t sample,
                   const uint8_t* pat, const uint64_t* poff, uint64_t q, T* lb, T* ub, uint64_t limit, uint64_t* start, T* pos, T* sid, uint64_t cap,
                   uint64_t* total) {
    if (!c) return PSACX_EINVAL;
    if (total) *total = 0;
    PSACX_TRY(index_check_n<T>(n));
    if (q == 0) { if (start) start[0] = 0; return PSACX_OK; }
    if (!poff || !lb || !ub) return PSACX_EINVAL;
    if (pos && (!start || !total || sample == 0)) return PSACX_EINVAL;
    if (sid && (!pos || !offsets)) return PSACX_EINVAL;
    if (n && (!text || !SA)) return PSACX_EINVAL;
    if (offsets && n && (m == 0 || m > n)) return PSACX_EINVAL;
    uint64_t S = 0;
    PSACX_TRY(pattern_batch_valid(pat, poff, q, &S));
    PSACX_HIP(c, hipSetDevice(c->device));
    const uint64_t use = pos ? sample : 0;
    Staging s(c, "fm search");
    uint8_t* d_text = (uint8_t*)s.upload(text, n);
    T* d_SA = (T*)s.upload(SA, n * sizeof(T));
    uint8_t* d_bwt = (uint8_t*)s.alloc(n);
    uint32_t* d_first = (uint32_t*)s.alloc(((n >> 5) + 1) * sizeof(uint32_t));
    const uint64_t* d_off = nullptr;
    const uint32_t* d_ends = offsets && n ? s.string_ends(offsets, m, n, &d_off) : nullptr;
    if (s.rc == PSACX_OK) s.rc = bwt_dev<T>(c, d_text, n, d_ends, (const T*)d_SA, d_bwt, d_first, (uint64_t*)nullptr);
    psacx_fm_info info;
    if (s.rc == PSACX_OK) s.rc = fm_index_dev<T>(c, n, d_bwt, d_first, use ? d_SA : (const T*)nullptr, use, (uint64_t*)nullptr, &info);
    if (s.rc != PSACX_OK) return s.rc;
    uint64_t* d_fm = (uint64_t*)s.alloc(info.words * sizeof(uint64_t));
    if (s.rc == PSACX_OK) s.rc = fm_index_dev<T>(c, n, d_bwt, d_first, use ? d_SA : (const T*)nullptr, use, d_fm, &info);
    const DeviceBatch b = s.upload_batch(pat, poff, q);
    T* d_lb = (T*)s.alloc(q * sizeof(T));
    T* d_ub = (T*)s.alloc(q * sizeof(T));
    if (s.rc == PSACX_OK) s.rc = fm_count_dev<T>(c, d_fm, &info, b.pat, b.poff, q, d_lb, d_ub);
    s.download(lb, d_lb, q * sizeof(T));
    s.download(ub, d_ub, q * sizeof(T));
    if (!pos || s.rc != PSACX_OK) { s.step(hipStreamSynchronize(c->stream)); return s.rc; }
    uint64_t* d_start = (uint64_t*)s.alloc((q + 1) * sizeof(uint64_t));
    if (s.rc == PSACX_OK) s.rc = fm_occurrences_dev<T>(c, d_fm, &info, d_off, m, d_lb, d_ub, q, limit, d_start, (T*)nullptr, (T*)nullptr, 0, total);
    s.download(start, d_start, (q + 1) * sizeof(uint64_t));
    s.step(hipStreamSynchronize(c->stream));
    if (s.rc != PSACX_OK) return s.rc;
    if (*total > cap) return PSACX_ERANGE;
    T* d_pos = (T*)s.alloc(*total * sizeof(T));
    T* d_sid = sid ? (T*)s.alloc(*total * sizeof(T)) : nullptr;
    if (s.rc == PSACX_OK) s.rc = fm_occurrences_dev<T>(c, d_fm, &info, d_off, m, d_lb, d_ub, q, limit, d_start, d_pos, d_sid, *total, total);
    s.download(pos, d_pos, *total * sizeof(T));
    if (sid) s.download(sid, d_sid, *total * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

} // namespace psacx

using namespace psacx;

extern "C" {

#define PSACX_FM_ABI(S, T)                                                                                                                      \
    int psacx_fm_index_dev_##S(psacx_ctx* c, uint64_t n, const uint8_t* bwt, const uint32_t* first, const T* sa, uint64_t sample, uint64_t* fm, \
                               psacx_fm_info* info) {                                                                                           \
        return fm_index_dev<T>(c, n, bwt, first, sa, sample, fm, info);                                                                         \
    }                                                                                                                                           \
    int psacx_fm_count_dev_##S(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* info, const uint8_t* pat, const uint64_t* poff,           \
                               uint64_t q, T* lb, T* ub) {                                                                                      \
        return fm_count_dev<T>(c, fm, info, pat, poff, q, lb, ub);                                                                              \
    }                                                                                                                                           \
    int psacx_fm_occurrences_dev_##S(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* info, const uint64_t* off, uint64_t m, const T* lb, \
                                     const T* ub, uint64_t q, uint64_t limit, uint64_t* start, T* pos, T* sid, uint64_t cap, uint64_t* total) { \
        return fm_occurrences_dev<T>(c, fm, info, off, m, lb, ub, q, limit, start, pos, sid, cap, total);                                       \
    }                                                                                                                                           \
    int psacx_fm_text_samples_dev_##S(psacx_ctx* c, uint64_t n, const T* sa, const uint64_t* off, uint64_t m, uint64_t rate, T* ts,            \
                                      uint64_t* entries) {                                                                                      \
        return fm_text_samples_dev<T>(c, n, sa, off, m, rate, ts, entries);                                                                     \
    }                                                                                                                                           \
    int psacx_fm_extract_dev_##S(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* info, const T* ts, uint64_t rate, const uint64_t* off,  \
                                 uint64_t m, const T* pos, const T* len, uint64_t q, uint64_t* start, uint8_t* out, uint64_t cap,               \
                                 uint64_t* total) {                                                                                             \
        return fm_extract_dev<T>(c, fm, info, ts, rate, off, m, pos, len, q, start, out, cap, total);                                           \
    }                                                                                                                                           \
    int psacx_fm_search_##S(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, uint64_t sample,       \
                            const uint8_t* pat, const uint64_t* poff, uint64_t q, T* lb, T* ub, uint64_t limit, uint64_t* start, T* pos,        \
                            T* sid, uint64_t cap, uint64_t* total) {                                                                            \
        return fm_search_host<T>(c, text, n, off, m, sa, sample, pat, poff, q, lb, ub, limit, start, pos, sid, cap, total);                     \
    }
PSACX_FM_ABI(u32, uint32_t)
PSACX_FM_ABI(u64, uint64_t)
#undef PSACX_FM_ABI

} // extern "C"
