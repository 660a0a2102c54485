// rmq.hip -- the range-minimum index of an array resident in HBM, batched range minima with their first positions, the
// longest common extension of text positions from ISA and LCP (include/psacx.h: "range minimum and longest common extension";
// kernels in rmq.hpp), and the suffix-prefix overlaps of a string set from the same arrays ("suffix-prefix overlaps";
// kernel in overlaps.hpp).
//
// Stands in for rmq<>::query (the reference's include/rmq.hpp:186) and, on one GPU, for what par_rmq.hpp answers across ranks.
// The text is no argument of any call here.
#include "engine.hpp"
#include "rmq.hpp"
#include "overlaps.hpp"
#include "staging.hpp"

namespace psacx {

// the levels >= 1 and their running minima, queued on the ctx stream (profile: an event pair around the kernel of level 1, the
// one pass over the values themselves)
template <typename T>
static int rmq_index_fill(psacx_ctx* c, const T* d_values, uint64_t n, T* d_index, bool profile = false) {
    RmqLayout Y;
    rmq_layout(n, Y);
    for (int L = 1; L < Y.nlev; ++L) {
        const T* below = L == 1 ? d_values : d_index + Y.lvl[L - 1];
        auto level = [&]() {
            hipLaunchKernelGGL((pyramid_level_kernel<T>), dim3(grid_for(c, Y.len[L] * 64, 256, 8)), dim3(256), 0, c->stream, below, Y.len[L - 1],
                               d_index + Y.lvl[L], Y.len[L]);
        };
        if (profile && L == 1) { ProfScope first(c, TC_RMQ_BUILD); level(); } else level();
        hipLaunchKernelGGL((pyramid_aux_kernel<T>), dim3(grid_for(c, Y.len[L], 256, 8)), dim3(256), 0, c->stream, (const T*)(d_index + Y.lvl[L]),
                           Y.len[L], d_index + Y.pre[L], d_index + Y.suf[L]);
    }
    PSACX_HIP(c, hipGetLastError());
    return PSACX_OK;
}

template <typename T>
int rmq_index_dev(psacx_ctx* c, const T* d_values, uint64_t n, T* d_index, uint64_t* entries) {
    if (!c || !entries) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    RmqLayout Y;
    rmq_layout(n, Y);
    *entries = Y.entries;
    if (!d_index) return PSACX_OK;                    // size query
    if (n == 0 || Y.nlev == 1) return PSACX_OK;       // level 0 is the index of up to 64 values
    if (!d_values) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    c->profile = c->profile_ops; c->ev_used = 0;     // psacx_profile: the level-1 kernel alone, for tools/lce_time.py
    int rc = rmq_index_fill<T>(c, d_values, n, d_index, c->profile);
    if (rc == PSACX_OK && hipStreamSynchronize(c->stream) != hipSuccess) { c->hip_err = "hipStreamSynchronize(rmq index)"; rc = PSACX_EHIP; }
    if (rc == PSACX_OK && c->profile && c->ev_used) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, c->ev_pool[0].a, c->ev_pool[0].b) == hipSuccess) c->stats.ms_rmq_build = ms;
    }
    c->profile = false; c->ev_used = 0;
    return rc;
}
template int rmq_index_dev<uint32_t>(psacx_ctx*, const uint32_t*, uint64_t, uint32_t*, uint64_t*);
template int rmq_index_dev<uint64_t>(psacx_ctx*, const uint64_t*, uint64_t, uint64_t*, uint64_t*);

template <typename T>
int rmq_dev(psacx_ctx* c, const T* d_values, uint64_t n, const T* d_index, const T* d_lo, const T* d_hi, uint64_t q, T* d_min, T* d_arg) {
    if (!c || (!d_min && !d_arg)) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (q == 0) return PSACX_OK;
    if (!d_lo || !d_hi || (n && (!d_values || !d_index))) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL((rmq_kernel<T>), dim3(grid_for(c, q * RMQ_LANES, 256, 8)), dim3(256), 0, c->stream, d_values, n, d_index, d_lo, d_hi, q,
                       d_min, d_arg);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

template <typename T>
int lce_dev(psacx_ctx* c, uint64_t n, const uint64_t* d_off, uint64_t m, const T* d_ISA, const T* d_LCP, const T* d_index, const T* d_a,
            const T* d_b, uint64_t q, uint64_t e, T* d_len) {
    if (!c) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (d_off && (m == 0 || m > n)) return PSACX_EINVAL;
    if (q == 0) return PSACX_OK;
    if (!d_a || !d_b || !d_len || (n && (!d_ISA || !d_LCP || !d_index))) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    const int grid = grid_for(c, q * RMQ_LANES, 256, 8);
    if (d_off)
        hipLaunchKernelGGL((lce_kernel<T, true>), dim3(grid), dim3(256), 0, c->stream, n, d_off, m, d_ISA, d_LCP, d_index, d_a, d_b, q, e, d_len);
    else
        hipLaunchKernelGGL((lce_kernel<T, false>), dim3(grid), dim3(256), 0, c->stream, n, d_off, m, d_ISA, d_LCP, d_index, d_a, d_b, q, e, d_len);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// The host-pointer forms: the arrays are staged (staging.hpp), the index is built and the results come back.
template <typename T>
int rmq_host(psacx_ctx* c, const T* values, uint64_t n, const T* lo, const T* hi, uint64_t q, T* mn, T* arg) {
    if (!c || (!mn && !arg)) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (q == 0) return PSACX_OK;
    if (!lo || !hi || (n && !values)) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    RmqLayout Y;
    rmq_layout(n, Y);
    Staging s(c, "rmq");
    T* d_values = (T*)s.upload(values, n * sizeof(T));
    T* d_lo = (T*)s.upload(lo, q * sizeof(T));
    T* d_hi = (T*)s.upload(hi, q * sizeof(T));
    T* d_index = (T*)s.alloc(Y.entries * sizeof(T));
    T* d_min = mn ? (T*)s.alloc(q * sizeof(T)) : nullptr;
    T* d_arg = arg ? (T*)s.alloc(q * sizeof(T)) : nullptr;
    if (s.rc == PSACX_OK) s.rc = rmq_index_fill<T>(c, d_values, n, d_index);
    if (s.rc == PSACX_OK) s.rc = rmq_dev<T>(c, d_values, n, d_index, d_lo, d_hi, q, d_min, d_arg);
    s.download(mn, d_min, q * sizeof(T));
    s.download(arg, d_arg, q * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

template <typename T>
int lce_host(psacx_ctx* c, uint64_t n, const uint64_t* offsets, uint64_t m, const T* ISA, const T* LCP, const T* a, const T* b, uint64_t q,
             uint64_t e, T* len) {
    if (!c) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (offsets && (m == 0 || m > n)) return PSACX_EINVAL;
    if (q == 0) return PSACX_OK;
    if (!a || !b || !len || (n && (!ISA || !LCP))) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    RmqLayout Y;
    rmq_layout(n, Y);
    Staging s(c, "rmq");
    T* d_ISA = (T*)s.upload(ISA, n * sizeof(T));
    T* d_LCP = (T*)s.upload(LCP, n * sizeof(T));
    T* d_a = (T*)s.upload(a, q * sizeof(T));
    T* d_b = (T*)s.upload(b, q * sizeof(T));
    uint64_t* d_off = offsets ? (uint64_t*)s.upload(offsets, (m + 1) * sizeof(uint64_t)) : nullptr;
    T* d_index = (T*)s.alloc(Y.entries * sizeof(T));
    T* d_len = (T*)s.alloc(q * sizeof(T));
    if (s.rc == PSACX_OK) s.rc = rmq_index_fill<T>(c, d_LCP, n, d_index);
    if (s.rc == PSACX_OK) s.rc = lce_dev<T>(c, n, d_off, m, d_ISA, d_LCP, d_index, d_a, d_b, q, e, d_len);
    s.download(len, d_len, q * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// psacx_overlaps_dev_*: the offsets are checked on the device before anything is written, the two outputs are cleared, and one
// launch walks every string.  Nothing is allocated beyond the slab word of the offsets check.
template <typename T>
int overlaps_dev(psacx_ctx* c, uint64_t n, const uint64_t* d_off, uint64_t m, const uint32_t* d_ends, const T* d_SA, const T* d_ISA, const T* d_LCP,
                 const T* d_index, uint64_t min_len, uint32_t flags, T* d_lb, T* d_ub) {
    if (!c || min_len == 0 || (flags & ~(uint32_t)PSACX_OVERLAP_WHOLE)) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (m == 0 || n == 0) return PSACX_OK;
    if (m > n || !d_off || !d_ends || !d_SA || !d_ISA || !d_LCP || !d_index || !d_lb || !d_ub) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(string_offsets_valid_dev(c, d_off, m, n));
    PSACX_HIP(c, hipMemsetAsync(d_lb, 0, n * sizeof(T), c->stream));
    PSACX_HIP(c, hipMemsetAsync(d_ub, 0, n * sizeof(T), c->stream));
    hipLaunchKernelGGL((overlaps_kernel<T>), dim3(grid_for(c, m * RMQ_LANES, 256, 8)), dim3(256), 0, c->stream, n, d_off, m, d_ends, d_SA, d_ISA,
                       d_LCP, d_index, min_len, flags, d_lb, d_ub);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

template <typename T>
int overlaps_host(psacx_ctx* c, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, const T* ISA, const T* LCP, uint64_t min_len,
                  uint32_t flags, T* lb, T* ub) {
    if (!c || min_len == 0 || (flags & ~(uint32_t)PSACX_OVERLAP_WHOLE)) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (m == 0 || n == 0) return PSACX_OK;
    if (m > n || !offsets || !SA || !ISA || !LCP || !lb || !ub) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    RmqLayout Y;
    rmq_layout(n, Y);
    Staging s(c, "overlaps");
    T* d_SA = (T*)s.upload(SA, n * sizeof(T));
    T* d_ISA = (T*)s.upload(ISA, n * sizeof(T));
    T* d_LCP = (T*)s.upload(LCP, n * sizeof(T));
    T* d_index = (T*)s.alloc(Y.entries * sizeof(T));
    T* d_lb = (T*)s.alloc(n * sizeof(T));
    T* d_ub = (T*)s.alloc(n * sizeof(T));
    const uint64_t* d_off = nullptr;
    const uint32_t* d_ends = s.string_ends(offsets, m, n, &d_off);
    if (s.rc == PSACX_OK) s.rc = rmq_index_fill<T>(c, d_LCP, n, d_index);
    if (s.rc == PSACX_OK) s.rc = overlaps_dev<T>(c, n, d_off, m, d_ends, d_SA, d_ISA, d_LCP, d_index, min_len, flags, d_lb, d_ub);
    s.download(lb, d_lb, n * sizeof(T));
    s.download(ub, d_ub, n * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

} // namespace psacx

using namespace psacx;

extern "C" {

#define PSACX_RMQ_ABI(S, T)                                                                                                                   \
    int psacx_rmq_index_dev_##S(psacx_ctx* c, const T* v, uint64_t n, T* index, uint64_t* entries) { return rmq_index_dev<T>(c, v, n, index, entries); } \
    int psacx_rmq_dev_##S(psacx_ctx* c, const T* v, uint64_t n, const T* index, const T* lo, const T* hi, uint64_t q, T* mn, T* arg) {           \
        return rmq_dev<T>(c, v, n, index, lo, hi, q, mn, arg);                                                                                  \
    }                                                                                                                                           \
    int psacx_lce_dev_##S(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const T* isa, const T* lcp, const T* index, const T* a,    \
                          const T* b, uint64_t q, uint64_t e, T* len) {                                                                         \
        return lce_dev<T>(c, n, off, m, isa, lcp, index, a, b, q, e, len);                                                                      \
    }                                                                                                                                           \
    int psacx_rmq_##S(psacx_ctx* c, const T* v, uint64_t n, const T* lo, const T* hi, uint64_t q, T* mn, T* arg) {                              \
        return rmq_host<T>(c, v, n, lo, hi, q, mn, arg);                                                                                        \
    }                                                                                                                                           \
    int psacx_lce_##S(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const T* isa, const T* lcp, const T* a, const T* b,            \
                      uint64_t q, uint64_t e, T* len) {                                                                                         \
        return lce_host<T>(c, n, off, m, isa, lcp, a, b, q, e, len);                                                                            \
    }
PSACX_RMQ_ABI(u32, uint32_t)
PSACX_RMQ_ABI(u64, uint64_t)
#undef PSACX_RMQ_ABI

#define PSACX_OVERLAPS_ABI(S, T)                                                                                                              \
    int psacx_overlaps_dev_##S(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* ends, const T* sa, const T* isa,      \
                               const T* lcp, const T* index, uint64_t min_len, uint32_t flags, T* lb, T* ub) {                                  \
        return overlaps_dev<T>(c, n, off, m, ends, sa, isa, lcp, index, min_len, flags, lb, ub);                                                \
    }                                                                                                                                           \
    int psacx_overlaps_##S(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const T* isa, const T* lcp,                  \
                           uint64_t min_len, uint32_t flags, T* lb, T* ub) {                                                                    \
        return overlaps_host<T>(c, n, off, m, sa, isa, lcp, min_len, flags, lb, ub);                                                            \
    }
PSACX_OVERLAPS_ABI(u32, uint32_t)
PSACX_OVERLAPS_ABI(u64, uint64_t)
#undef PSACX_OVERLAPS_ABI

} // extern "C"
