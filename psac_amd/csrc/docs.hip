// docs.hip -- document counts and document lists over a string set: the index prev / dup from SA, LCP and its range-minimum index, the
// counts of intervals from dup and the lists of intervals from prev (include/psacx.h: "document counts and document lists"; kernels in
// docs.hpp).  The reference has no counterpart.
#include "engine.hpp"
#include "docs.hpp"
#include "staging.hpp"

namespace psacx {

// psacx_doc_index_dev_*: the keys, their sort, prev and h from the sorted keys, and the scan of h in the caller's dup.
// Scratch: the two key words, 2 n entries, are memory of the call's own, there before anything is written.  The ctx slab holds the
// buffers of the rank-pair sort and then the block sums of the scan (both lay themselves out from its base; the sort waits).
// After psacx_profile(ctx, 1) the stages leave their times in psacx_stats, for tools/doc_time.py: ms_kmer the keys, ms_sort_scatter the
// sort (its waits included), ms_rebucket prev and the pairs, ms_finalize the scan; events on the ctx stream around each.
template <typename T>
int doc_index_dev(psacx_ctx* c, uint64_t n, const uint64_t* d_off, uint64_t m, const T* d_SA, const T* d_LCP, const T* d_index, T* d_prev,
                  T* d_dup) {
    if (!c) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (!d_prev && !d_dup) return PSACX_EINVAL;
    if (n == 0) return PSACX_OK;
    if (m == 0 || m > n) return PSACX_EINVAL;
    if (!d_off || !d_SA || (d_dup && (!d_LCP || !d_index))) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    Staging s(c, "doc index");
    T* k1 = (T*)s.alloc(n * sizeof(T));
    T* k2 = (T*)s.alloc(n * sizeof(T));
    if (s.rc != PSACX_OK) return s.rc;
    struct Marks {                                    // five events, made only under psacx_profile and destroyed on every path
        hipEvent_t e[5]; int made = 0;
        ~Marks() { for (int i = 0; i < made; ++i) (void)hipEventDestroy(e[i]); }
    } ev;
    if (c->profile_ops) while (ev.made < 5 && hipEventCreate(&ev.e[ev.made]) == hipSuccess) ++ev.made;
    const bool timed = ev.made == 5;
    auto mark = [&](int i) { if (timed) (void)hipEventRecord(ev.e[i], c->stream); };
    const int lane_grid = grid_for(c, n, 256, 8);
    mark(0);
    hipLaunchKernelGGL((doc_keys_kernel<T>), dim3(lane_grid), dim3(256), 0, c->stream, d_SA, n, d_off, m, k1, k2);
    PSACX_HIP(c, hipGetLastError());
    mark(1);
    PSACX_TRY(pair_sort_first_dev_any(c, k1, k2, n, bits_of(m - 1)));
    mark(2);
    if (d_dup) PSACX_HIP(c, hipMemsetAsync(d_dup, 0, (n + 1) * sizeof(T), c->stream));
    hipLaunchKernelGGL((doc_prev_kernel<T>), dim3(lane_grid), dim3(256), 0, c->stream, (const T*)k1, (const T*)k2, n, d_prev, d_dup);
    PSACX_HIP(c, hipGetLastError());
    if (d_dup) {
        hipLaunchKernelGGL((doc_pairs_kernel<T>), dim3(grid_for(c, n * RMQ_LANES, 256, 8)), dim3(256), 0, c->stream, (const T*)k1, (const T*)k2, n,
                           d_LCP, d_index, d_dup);
        PSACX_HIP(c, hipGetLastError());
        mark(3);
        PSACX_TRY(exclusive_scan_dev_any(c, d_dup, n + 1));
    } else mark(3);
    mark(4);
    s.step(hipStreamSynchronize(c->stream));
    if (timed && s.rc == PSACX_OK) {
        float ms[4] = {0, 0, 0, 0};
        for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&ms[i], ev.e[i], ev.e[i + 1]);
        c->stats.ms_kmer = ms[0]; c->stats.ms_sort_scatter = ms[1]; c->stats.ms_rebucket = ms[2]; c->stats.ms_finalize = ms[3];
    }
    return s.rc;
}

// psacx_doc_count_dev_*: one launch, nothing allocated
template <typename T>
int doc_count_dev(psacx_ctx* c, uint64_t n, const T* d_dup, const T* d_lb, const T* d_ub, uint64_t q, T* d_docs) {
    if (!c) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (q == 0) return PSACX_OK;
    if (!d_lb || !d_ub || !d_docs || (n && !d_dup)) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL((doc_count_kernel<T>), dim3(grid_for(c, q, 256, 8)), dim3(256), 0, c->stream, n, d_dup, d_lb, d_ub, q, d_docs);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// psacx_doc_list_dev_*: the candidate numbers of the intervals, their marks, the marks per tile and per run, the starts and the lists.
// Scratch: the ctx slab holds the block sums of the scans only.  Memory of the call's own: the candidate starts, 8 (q + 1) bytes, and, once
// the number of candidates is known and has passed max_cand, a mark byte per candidate in whole tiles, 8 (t + 1) bytes of tile counts and
// 64 t bytes of run counts for t tiles.  Nothing is written to the outputs before all of it is there.
// late (the host-pointer form): the lists are not there yet; once the total is known and within cap they are taken from *late (sid, and pos
// where want_pos) and handed back through d_sid / d_pos, so that one run of the pipeline serves the size and the lists.
template <typename T>
int doc_list_run(psacx_ctx* c, const T* d_SA, uint64_t n, const uint64_t* d_off, uint64_t m, const T* d_prev, const T* d_lb, const T* d_ub,
                 uint64_t q, uint64_t max_cand, uint64_t* d_start, T*& d_sid, T*& d_pos, uint64_t cap, uint64_t* total, Staging* late, bool want_pos) {
    if (!c || !total) return PSACX_EINVAL;
    *total = 0;
    PSACX_TRY(index_check_n<T>(n));
    if (!d_sid && d_pos) return PSACX_EINVAL;
    if (n && (m == 0 || m > n)) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    if (q == 0 || n == 0) {                           // no candidates: every interval is empty or malformed
        if (q && !d_start) return PSACX_EINVAL;
        if (d_start) { PSACX_HIP(c, hipMemsetAsync(d_start, 0, (q + 1) * sizeof(uint64_t), c->stream)); PSACX_HIP(c, hipStreamSynchronize(c->stream)); }
        return PSACX_OK;
    }
    if (!d_SA || !d_off || !d_prev || !d_lb || !d_ub || !d_start) return PSACX_EINVAL;
    Staging s(c, "doc list");
    uint64_t* d_cstart = (uint64_t*)s.alloc((q + 1) * sizeof(uint64_t));
    if (s.rc != PSACX_OK) return s.rc;
    hipLaunchKernelGGL((occ_counts_kernel<T>), dim3(grid_for(c, q + 1, 256, 8)), dim3(256), 0, c->stream, d_lb, d_ub, q, n, (uint64_t)0, d_cstart);
    PSACX_HIP(c, hipGetLastError());
    uint64_t cand = 0;
    PSACX_TRY(scan_total_u64_dev(c, d_cstart, q + 1, &cand));
    if (max_cand && cand > max_cand) return PSACX_ERANGE;
    if (cand == 0) {
        PSACX_HIP(c, hipMemsetAsync(d_start, 0, (q + 1) * sizeof(uint64_t), c->stream));
        PSACX_HIP(c, hipStreamSynchronize(c->stream));
        return PSACX_OK;
    }
    const uint64_t ntiles = (cand + OCC_TILE - 1) / OCC_TILE;
    unsigned char* d_marks = nullptr;
    uint64_t* d_counts = nullptr;
    uint32_t* d_runs = nullptr;
    s.place([&](Arena& a) {
        d_marks = a.take<unsigned char>(ntiles * OCC_TILE);
        d_counts = a.take<uint64_t>(ntiles + 1);
        d_runs = a.take<uint32_t>(ntiles * (OCC_TILE / DOC_RUN));
    });
    if (s.rc != PSACX_OK) return s.rc;
    PSACX_HIP(c, hipMemsetAsync(d_marks + cand, 0, ntiles * OCC_TILE - cand, c->stream));
    const dim3 tile_grid(grid_for(c, ntiles * 256, 256, 8));
    hipLaunchKernelGGL((doc_mark_kernel<T>), tile_grid, dim3(256), 0, c->stream, d_prev, d_lb, (const uint64_t*)d_cstart, q, cand, d_marks);
    hipLaunchKernelGGL(doc_tile_kernel, tile_grid, dim3(256), 0, c->stream, (const unsigned char*)d_marks, ntiles, d_counts, d_runs);
    PSACX_HIP(c, hipGetLastError());
    PSACX_TRY(select_positions(c, d_counts, ntiles, true, total));
    hipLaunchKernelGGL(doc_start_kernel, dim3(grid_for(c, q + 1, 256, 8)), dim3(256), 0, c->stream, (const uint64_t*)d_cstart, q, cand,
                       (const unsigned char*)d_marks, ntiles, (const uint64_t*)d_counts, (const uint32_t*)d_runs, d_start);
    PSACX_HIP(c, hipGetLastError());
    if (late && *total <= cap) {
        d_sid = (T*)late->alloc(*total * sizeof(T));
        if (want_pos) d_pos = (T*)late->alloc(*total * sizeof(T));
        if (late->rc != PSACX_OK) return late->rc;
    }
    if (d_sid && *total <= cap)
        s.step(select_emit(c, d_marks, OCC_TILE, ntiles, d_counts, DocListEmit<T>{d_SA, n, d_off, m, d_lb, d_cstart, q, d_sid, d_pos}));
    s.step(hipStreamSynchronize(c->stream));
    if (s.rc != PSACX_OK) return s.rc;
    return (d_sid || late) && *total > cap ? PSACX_ERANGE : PSACX_OK;
}

template <typename T>
int doc_list_dev(psacx_ctx* c, const T* d_SA, uint64_t n, const uint64_t* d_off, uint64_t m, const T* d_prev, const T* d_lb, const T* d_ub,
                 uint64_t q, uint64_t max_cand, uint64_t* d_start, T* d_sid, T* d_pos, uint64_t cap, uint64_t* total) {
    return doc_list_run<T>(c, d_SA, n, d_off, m, d_prev, d_lb, d_ub, q, max_cand, d_start, d_sid, d_pos, cap, total, nullptr, false);
}

// The host-pointer forms: the arrays are staged (staging.hpp), the offsets checked on the device as for psacx_repeats_*, the range-minimum
// index and the doc index built beside them, and the results come back.  Everything allocated is freed on every path.
template <typename T>
int doc_count_host(psacx_ctx* c, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, const T* LCP, const T* lb, const T* ub, uint64_t q,
                   T* docs) {
    if (!c) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (q == 0) return PSACX_OK;
    if (!lb || !ub || !docs) return PSACX_EINVAL;
    if (n == 0) { std::memset(docs, 0, q * sizeof(T)); return PSACX_OK; }
    if (m == 0 || m > n || !offsets || !SA || !LCP) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    RmqLayout Y;
    rmq_layout(n, Y);
    uint64_t entries = 0;
    Staging s(c, "doc count");
    const uint64_t* d_off = (const uint64_t*)s.upload(offsets, (m + 1) * sizeof(uint64_t));
    if (s.rc == PSACX_OK) s.rc = string_offsets_valid_dev(c, d_off, m, n);
    T* d_SA = (T*)s.upload(SA, n * sizeof(T));
    T* d_LCP = (T*)s.upload(LCP, n * sizeof(T));
    T* d_index = (T*)s.alloc(Y.entries * sizeof(T));
    T* d_dup = (T*)s.alloc((n + 1) * sizeof(T));
    T* d_lb = (T*)s.upload(lb, q * sizeof(T));
    T* d_ub = (T*)s.upload(ub, q * sizeof(T));
    T* d_docs = (T*)s.alloc(q * sizeof(T));
    if (s.rc == PSACX_OK) s.rc = rmq_index_dev<T>(c, d_LCP, n, d_index, &entries);
    if (s.rc == PSACX_OK) s.rc = doc_index_dev<T>(c, n, d_off, m, d_SA, d_LCP, d_index, (T*)nullptr, d_dup);
    if (s.rc == PSACX_OK) s.rc = doc_count_dev<T>(c, n, d_dup, d_lb, d_ub, q, d_docs);
    s.download(docs, d_docs, q * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// sid == nullptr: the size query.  No LCP: the lists need prev alone.
template <typename T>
int doc_list_host(psacx_ctx* c, const T* SA, uint64_t n, const uint64_t* offsets, uint64_t m, const T* lb, const T* ub, uint64_t q,
                  uint64_t max_cand, uint64_t* start, T* sid, T* pos, uint64_t cap, uint64_t* total) {
    if (!c || !total) return PSACX_EINVAL;
    *total = 0;
    PSACX_TRY(index_check_n<T>(n));
    if (!sid && pos) return PSACX_EINVAL;
    if (q == 0) { if (start) start[0] = 0; return PSACX_OK; }
    if (!lb || !ub || !start) return PSACX_EINVAL;
    if (n == 0) { std::memset(start, 0, (q + 1) * sizeof(uint64_t)); return PSACX_OK; }
    if (m == 0 || m > n || !offsets || !SA) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    Staging s(c, "doc list");
    const uint64_t* d_off = (const uint64_t*)s.upload(offsets, (m + 1) * sizeof(uint64_t));
    if (s.rc == PSACX_OK) s.rc = string_offsets_valid_dev(c, d_off, m, n);
    T* d_SA = (T*)s.upload(SA, n * sizeof(T));
    T* d_prev = (T*)s.alloc(n * sizeof(T));
    T* d_lb = (T*)s.upload(lb, q * sizeof(T));
    T* d_ub = (T*)s.upload(ub, q * sizeof(T));
    uint64_t* d_start = (uint64_t*)s.alloc((q + 1) * sizeof(uint64_t));
    if (s.rc == PSACX_OK) s.rc = doc_index_dev<T>(c, n, d_off, m, d_SA, (const T*)nullptr, (const T*)nullptr, d_prev, (T*)nullptr);
    // one run: the lists are allocated inside it, once their size is known and within cap
    T *d_sid = nullptr, *d_pos = nullptr;
    int rc = s.rc;
    if (rc == PSACX_OK) rc = doc_list_run<T>(c, d_SA, n, d_off, m, d_prev, d_lb, d_ub, q, max_cand, d_start, d_sid, d_pos, cap, total, sid ? &s : nullptr, pos != nullptr);
    if (rc != PSACX_OK && !(rc == PSACX_ERANGE && *total > cap)) return rc;     // (more than cap: start and *total are valid; refused for max_cand: *total is 0)
    s.download(start, d_start, (q + 1) * sizeof(uint64_t));
    if (rc == PSACX_OK && d_sid) {
        s.download(sid, d_sid, *total * sizeof(T));
        if (pos) s.download(pos, d_pos, *total * sizeof(T));
    }
    s.step(hipStreamSynchronize(c->stream));
    return s.rc != PSACX_OK ? s.rc : rc;
}

} // namespace psacx

using namespace psacx;

extern "C" {

#define PSACX_DOCS_ABI(S, T)                                                                                                                    \
    int psacx_doc_index_dev_##S(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const T* lcp, const T* index, T* prev,  \
                                T* dup) {                                                                                                       \
        return doc_index_dev<T>(c, n, off, m, sa, lcp, index, prev, dup);                                                                       \
    }                                                                                                                                           \
    int psacx_doc_count_dev_##S(psacx_ctx* c, uint64_t n, const T* dup, const T* lb, const T* ub, uint64_t q, T* docs) {                        \
        return doc_count_dev<T>(c, n, dup, lb, ub, q, docs);                                                                                    \
    }                                                                                                                                           \
    int psacx_doc_list_dev_##S(psacx_ctx* c, const T* sa, uint64_t n, const uint64_t* off, uint64_t m, const T* prev, const T* lb, const T* ub, \
                               uint64_t q, uint64_t max_cand, uint64_t* start, T* sid, T* pos, uint64_t cap, uint64_t* total) {                 \
        return doc_list_dev<T>(c, sa, n, off, m, prev, lb, ub, q, max_cand, start, sid, pos, cap, total);                                       \
    }                                                                                                                                           \
    int psacx_doc_count_##S(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const T* lcp, const T* lb, const T* ub,     \
                            uint64_t q, T* docs) {                                                                                              \
        return doc_count_host<T>(c, n, off, m, sa, lcp, lb, ub, q, docs);                                                                       \
    }                                                                                                                                           \
    int psacx_doc_list_##S(psacx_ctx* c, const T* sa, uint64_t n, const uint64_t* off, uint64_t m, const T* lb, const T* ub, uint64_t q,        \
                           uint64_t max_cand, uint64_t* start, T* sid, T* pos, uint64_t cap, uint64_t* total) {                                 \
        return doc_list_host<T>(c, sa, n, off, m, lb, ub, q, max_cand, start, sid, pos, cap, total);                                            \
    }
PSACX_DOCS_ABI(u32, uint32_t)
PSACX_DOCS_ABI(u64, uint64_t)
#undef PSACX_DOCS_ABI

} // extern "C"
