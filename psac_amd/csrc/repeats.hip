// repeats.hip -- the Burrows-Wheeler transform of a text or a string set from SA, and the right-maximal, maximal and supermaximal
// repeats from LCP, its range-minimum index, the BWT and the bitmap of the string starts (include/psacx.h: "BWT and repeats"; kernels in
// repeats.hpp).  The reference has no counterpart.
#include "engine.hpp"
#include "repeats.hpp"
#include "staging.hpp"

namespace psacx {

// psacx_bwt_dev_*: one launch over the ranks.  The primary travels through eight bytes of the ctx slab.
template <typename T>
int bwt_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, uint8_t* d_bwt, uint32_t* d_first,
            uint64_t* primary) {
    if (!c) return PSACX_EINVAL;
    if (primary) *primary = ~0ull;
    PSACX_TRY(index_check_n<T>(n));
    if (!d_bwt && !d_first) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    if (n == 0) {
        if (d_first) PSACX_HIP(c, hipMemsetAsync(d_first, 0, sizeof(uint32_t), c->stream));
        PSACX_HIP(c, hipStreamSynchronize(c->stream));
        return PSACX_OK;
    }
    if (!d_text || !d_SA) return PSACX_EINVAL;
    PSACX_TRY(ensure_slab(c, 4096));
    uint64_t* d_primary = reinterpret_cast<uint64_t*>(c->slab);
    PSACX_HIP(c, hipMemsetAsync(d_primary, 0xFF, sizeof(uint64_t), c->stream));
    hipLaunchKernelGGL((bwt_kernel<T>), dim3(grid_for(c, n + 64, 256, 8)), dim3(256), 0, c->stream, d_text, n, d_ends, d_SA, d_bwt, d_first,
                       primary ? d_primary : (uint64_t*)nullptr);
    PSACX_HIP(c, hipGetLastError());
    uint64_t p = ~0ull;
    PSACX_HIP(c, hipMemcpyAsync(&p, d_primary, sizeof(p), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (primary) *primary = p;
    return PSACX_OK;
}

template int bwt_dev<uint32_t>(psacx_ctx*, const uint8_t*, uint64_t, const uint32_t*, const uint32_t*, uint8_t*, uint32_t*, uint64_t*);
template int bwt_dev<uint64_t>(psacx_ctx*, const uint8_t*, uint64_t, const uint32_t*, const uint64_t*, uint8_t*, uint32_t*, uint64_t*);

// psacx_repeats_dev_*: the directories its kind needs, one launch over the ranks, the counts of the select bytes, their scan, and the
// three lists (repeats.hpp).  Scratch in the ctx slab: the block sums of the scans first (exclusive_scan_dev puts them at the slab's
// base), then bitmaps, directories, select bytes and tile counts.  The candidate intervals of a call that writes lists take 2 n
// entries of memory of their own for the time of the call; nothing is written before the memory is there.
template <typename T>
int repeats_dev(psacx_ctx* c, uint64_t n, const T* d_LCP, const T* d_index, const uint8_t* d_bwt, const uint32_t* d_first, uint32_t kind,
                uint64_t min_len, uint64_t min_occ, uint64_t max_occ, T* d_lb, T* d_ub, T* d_len, uint64_t cap, uint64_t* z) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    PSACX_TRY(index_check_n<T>(n));
    if (kind > (uint32_t)REPEATS_SUPERMAXIMAL) return PSACX_EINVAL;
    if (kind != (uint32_t)REPEATS_RIGHT && (!d_bwt || !d_first)) return PSACX_EINVAL;
    if ((d_lb == nullptr) != (d_ub == nullptr) || (!d_lb && d_len)) return PSACX_EINVAL;
    if (n <= 1) return PSACX_OK;
    if (!d_LCP || !d_index) return PSACX_EINVAL;
    if (min_occ < 2) min_occ = 2;
    PSACX_HIP(c, hipSetDevice(c->device));
    const uint64_t chunks = (n >> 6) + 1, ntiles = (n + REP_TILE - 1) / REP_TILE;
    const bool want_d = kind == (uint32_t)REPEATS_MAXIMAL, want_s = kind == (uint32_t)REPEATS_SUPERMAXIMAL;
    uint32_t *d_dbits = nullptr, *d_fbits = nullptr, *d_sbits = nullptr;
    uint64_t *d_dcnt = nullptr, *d_fcnt = nullptr, *d_scnt = nullptr, *d_counts = nullptr;
    unsigned char* d_sel = nullptr;
    auto layout = [&](Arena& a) {
        (void)a.take<unsigned char>(exclusive_scan_slab_bytes(std::max(chunks, ntiles + 1)));
        if (kind != (uint32_t)REPEATS_RIGHT) {
            d_dbits = a.take<uint32_t>(2 * chunks); d_dcnt = a.take<uint64_t>(chunks);
            d_fbits = a.take<uint32_t>(2 * chunks); d_fcnt = a.take<uint64_t>(chunks);
        }
        if (want_s) { d_sbits = a.take<uint32_t>(2 * chunks); d_scnt = a.take<uint64_t>(chunks); }
        d_sel = a.take<unsigned char>(ntiles * REP_TILE);
        d_counts = a.take<uint64_t>(ntiles + 1);
    };
    PSACX_TRY(slab_layout(c, layout));
    Staging s(c, "repeats");
    T *d_clb = nullptr, *d_cub = nullptr;
    if (d_lb) {
        d_clb = (T*)s.alloc(n * sizeof(T));
        d_cub = (T*)s.alloc(n * sizeof(T));
        if (s.rc != PSACX_OK) return s.rc;
    }
    const int wgrid = grid_for(c, n + 64, 256, 8);
    if (kind != (uint32_t)REPEATS_RIGHT) {
        hipLaunchKernelGGL(bwt_change_kernel, dim3(wgrid), dim3(256), 0, c->stream, n, d_bwt, d_first, d_dbits, d_dcnt, d_fbits, d_fcnt);
        PSACX_HIP(c, hipGetLastError());
        if (want_d) PSACX_TRY(exclusive_scan_u64_dev(c, d_dcnt, chunks));
        if (want_s) PSACX_TRY(exclusive_scan_u64_dev(c, d_fcnt, chunks));
    }
    if (want_s) {
        hipLaunchKernelGGL((lcp_step_kernel<T>), dim3(wgrid), dim3(256), 0, c->stream, n, d_LCP, d_sbits, d_scnt);
        PSACX_HIP(c, hipGetLastError());
        PSACX_TRY(exclusive_scan_u64_dev(c, d_scnt, chunks));
    }
    PSACX_HIP(c, hipMemsetAsync(d_sel + n, 0, ntiles * REP_TILE - n, c->stream));
    const RankDir D{reinterpret_cast<const uint64_t*>(d_dbits), d_dcnt}, F{reinterpret_cast<const uint64_t*>(d_fbits), d_fcnt},
        St{reinterpret_cast<const uint64_t*>(d_sbits), d_scnt};
    const dim3 grid(grid_for(c, n * RMQ_LANES, 256, 8));
#define PSACX_REPEATS_LAUNCH(K)                                                                                                          \
    hipLaunchKernelGGL((repeats_kernel<T, K>), grid, dim3(256), 0, c->stream, n, d_LCP, d_index, d_bwt, D, F, St, min_len, min_occ, max_occ, \
                       d_sel, d_clb, d_cub)
    if (want_s) PSACX_REPEATS_LAUNCH(REPEATS_SUPERMAXIMAL);
    else if (want_d) PSACX_REPEATS_LAUNCH(REPEATS_MAXIMAL);
    else PSACX_REPEATS_LAUNCH(REPEATS_RIGHT);
#undef PSACX_REPEATS_LAUNCH
    PSACX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(select_count_kernel<REP_TILE>, dim3(grid_for(c, ntiles * 256, 256, 8)), dim3(256), 0, c->stream, (const unsigned char*)d_sel, ntiles,
                       d_counts);
    PSACX_HIP(c, hipGetLastError());
    PSACX_TRY(select_positions(c, d_counts, ntiles, true, z));
    if (!d_lb) return PSACX_OK;                       // count query
    if (*z > cap) return PSACX_ERANGE;
    s.step(select_emit(c, d_sel, REP_TILE, ntiles, d_counts, RepeatsEmit<T>{d_LCP, d_clb, d_cub, d_lb, d_ub, d_len}));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// The host-pointer forms: text, SA and LCP are staged (staging.hpp), the bitmap of the string ends, the index and the BWT are built
// beside them, and the results come back.  Everything allocated is freed on every path.
template <typename T>
int bwt_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, uint8_t* bwt, uint64_t* primary) {
    if (!c) return PSACX_EINVAL;
    if (primary) *primary = ~0ull;
    PSACX_TRY(index_check_n<T>(n));
    if (n == 0) return PSACX_OK;
    if (!text || !SA || !bwt || (offsets && (m == 0 || m > n))) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    Staging s(c, "bwt");
    uint8_t* d_text = (uint8_t*)s.upload(text, n);
    T* d_SA = (T*)s.upload(SA, n * sizeof(T));
    uint8_t* d_bwt = (uint8_t*)s.alloc(n);
    const uint32_t* d_ends = offsets ? s.string_ends(offsets, m, n) : nullptr;
    if (s.rc == PSACX_OK) s.rc = bwt_dev<T>(c, d_text, n, d_ends, d_SA, d_bwt, (uint32_t*)nullptr, primary);
    s.download(bwt, d_bwt, n);
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// lb == NULL: the count query.  The right-maximal kind reads neither text nor SA.
template <typename T>
int repeats_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, const T* LCP, uint32_t kind,
                 uint64_t min_len, uint64_t min_occ, uint64_t max_occ, T* lb, T* ub, T* len, uint64_t cap, uint64_t* z) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    PSACX_TRY(index_check_n<T>(n));
    if (kind > (uint32_t)REPEATS_SUPERMAXIMAL) return PSACX_EINVAL;
    if ((lb == nullptr) != (ub == nullptr) || (!lb && len)) return PSACX_EINVAL;
    if (n <= 1) return PSACX_OK;
    const bool left = kind != (uint32_t)REPEATS_RIGHT;
    if (!LCP || (left && (!text || !SA)) || (offsets && (m == 0 || m > n))) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    RmqLayout Y;
    rmq_layout(n, Y);
    uint64_t entries = 0;
    Staging s(c, "repeats");
    T* d_LCP = (T*)s.upload(LCP, n * sizeof(T));
    T* d_index = (T*)s.alloc(Y.entries * sizeof(T));
    uint8_t* d_bwt = nullptr;
    uint32_t* d_first = nullptr;
    if (s.rc == PSACX_OK) s.rc = rmq_index_dev<T>(c, d_LCP, n, d_index, &entries);
    if (left) {
        uint8_t* d_text = (uint8_t*)s.upload(text, n);
        T* d_SA = (T*)s.upload(SA, n * sizeof(T));
        d_bwt = (uint8_t*)s.alloc(n);
        d_first = (uint32_t*)s.alloc(((n >> 5) + 1) * sizeof(uint32_t));
        const uint32_t* d_ends = offsets ? s.string_ends(offsets, m, n) : nullptr;
        if (s.rc == PSACX_OK) s.rc = bwt_dev<T>(c, d_text, n, d_ends, d_SA, d_bwt, d_first, (uint64_t*)nullptr);
    }
    if (s.rc == PSACX_OK)
        s.rc = repeats_dev<T>(c, n, d_LCP, d_index, d_bwt, d_first, kind, min_len, min_occ, max_occ, (T*)nullptr, (T*)nullptr, (T*)nullptr, 0, z);
    if (s.rc != PSACX_OK || !lb) return s.rc;
    if (*z > cap) return PSACX_ERANGE;
    const uint64_t room = *z ? *z : 1;
    T* d_lb = (T*)s.alloc(room * sizeof(T));
    T* d_ub = (T*)s.alloc(room * sizeof(T));
    T* d_len = len ? (T*)s.alloc(room * sizeof(T)) : nullptr;
    if (s.rc == PSACX_OK) s.rc = repeats_dev<T>(c, n, d_LCP, d_index, d_bwt, d_first, kind, min_len, min_occ, max_occ, d_lb, d_ub, d_len, *z, z);
    s.download(lb, d_lb, *z * sizeof(T));
    s.download(ub, d_ub, *z * sizeof(T));
    if (len) s.download(len, d_len, *z * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

} // namespace psacx

using namespace psacx;

extern "C" {

#define PSACX_REPEATS_ABI(S, T)                                                                                                                 \
    int psacx_bwt_dev_##S(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint32_t* ends, const T* sa, uint8_t* bwt, uint32_t* first,      \
                          uint64_t* primary) {                                                                                                \
        return bwt_dev<T>(c, text, n, ends, sa, bwt, first, primary);                                                                           \
    }                                                                                                                                           \
    int psacx_repeats_dev_##S(psacx_ctx* c, uint64_t n, const T* lcp, const T* index, const uint8_t* bwt, const uint32_t* first, uint32_t kind, \
                              uint64_t min_len, uint64_t min_occ, uint64_t max_occ, T* lb, T* ub, T* len, uint64_t cap, uint64_t* z) {          \
        return repeats_dev<T>(c, n, lcp, index, bwt, first, kind, min_len, min_occ, max_occ, lb, ub, len, cap, z);                              \
    }                                                                                                                                           \
    int psacx_bwt_##S(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, uint8_t* bwt,                \
                      uint64_t* primary) {                                                                                                    \
        return bwt_host<T>(c, text, n, off, m, sa, bwt, primary);                                                                               \
    }                                                                                                                                           \
    int psacx_repeats_##S(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const T* lcp,            \
                          uint32_t kind, uint64_t min_len, uint64_t min_occ, uint64_t max_occ, T* lb, T* ub, T* len, uint64_t cap,              \
                          uint64_t* z) {                                                                                                        \
        return repeats_host<T>(c, text, n, off, m, sa, lcp, kind, min_len, min_occ, max_occ, lb, ub, len, cap, z);                              \
    }
PSACX_REPEATS_ABI(u32, uint32_t)
PSACX_REPEATS_ABI(u64, uint64_t)
#undef PSACX_REPEATS_ABI

} // extern "C"
