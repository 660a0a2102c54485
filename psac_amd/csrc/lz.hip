// lz.hip -- the longest-previous-factor array of a text from SA, LCP and the range-minimum index of LCP, the greedy LZ77 parse cut
// from it, and the round-trip check of a parse (include/psacx.h: "LZ77 factorization"; kernels in lz.hpp).  The reference has no
// counterpart.  The text is an argument of the check alone.
#include "engine.hpp"
#include "lz.hpp"
#include "staging.hpp"

namespace psacx {

static int ansv_dev(psacx_ctx* c, const uint32_t* in, uint64_t n, uint64_t* l, uint64_t* r) { return ansv_dev_u32(c, in, n, 0, 0, ~0ull, l, r); }
static int ansv_dev(psacx_ctx* c, const uint64_t* in, uint64_t n, uint64_t* l, uint64_t* r) { return ansv_dev_u64(c, in, n, 0, 0, ~0ull, l, r); }

// psacx_lpf_dev_*: the neighbours of every rank (nearest smaller values of SA on both sides, 16 n bytes of memory of their own for
// the time of the call), then one launch over the ranks.  Nothing is written before the memory is there.
template <typename T>
int lpf_dev(psacx_ctx* c, uint64_t n, const T* d_SA, const T* d_LCP, const T* d_index, T* d_lpf, T* d_src) {
    if (!c) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (!d_lpf || !d_src) return PSACX_EINVAL;
    if (n == 0) return PSACX_OK;
    if (!d_SA || !d_LCP || !d_index) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    Staging s(c, "lpf");
    uint64_t* d_left = (uint64_t*)s.alloc(n * sizeof(uint64_t));
    uint64_t* d_right = (uint64_t*)s.alloc(n * sizeof(uint64_t));
    if (s.rc != PSACX_OK) return s.rc;
    PSACX_HIP(c, hipMemsetAsync(d_lpf, 0, n * sizeof(T), c->stream));
    PSACX_HIP(c, hipMemsetAsync(d_src, 0xFF, n * sizeof(T), c->stream));
    s.rc = ansv_dev(c, d_SA, n, d_left, d_right);
    if (s.rc == PSACX_OK) {
        hipLaunchKernelGGL((lpf_kernel<T>), dim3(grid_for(c, n * RMQ_LANES, 256, 8)), dim3(256), 0, c->stream, n, d_SA, d_LCP, d_index,
                           (const uint64_t*)d_left, (const uint64_t*)d_right, d_lpf, d_src);
        s.step(hipGetLastError());
    }
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// psacx_lz77_dev_*: exits, top walk, marks, the scan of the tile counts, and the two lists (lz.hpp).  Scratch in the ctx slab: the
// block sums of the scan first (exclusive_scan_dev puts them at the slab's base), then counts, group entries, marks and exits.
template <typename T>
int lz77_dev(psacx_ctx* c, uint64_t n, const T* d_lpf, const T* d_src, T* d_start, T* d_psrc, uint64_t cap, uint64_t* z) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    PSACX_TRY(index_check_n<T>(n));
    if (d_psrc && (!d_src || !d_start)) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    if (n == 0) {
        if (!d_start) return PSACX_OK;
        if (cap < 1) return PSACX_ERANGE;
        PSACX_HIP(c, hipMemsetAsync(d_start, 0, sizeof(T), c->stream));
        PSACX_HIP(c, hipStreamSynchronize(c->stream));
        return PSACX_OK;
    }
    if (!d_lpf) return PSACX_EINVAL;
    const LzGeometry geo = lz_geometry(c->knobs.lz_small_tiles);
    const uint64_t span = (uint64_t)geo.B * geo.G;
    const uint64_t ntiles = (n + geo.B - 1) / geo.B, ngroups = (n + span - 1) / span;
    uint64_t *d_counts = nullptr, *d_gentry = nullptr; unsigned char* d_marks = nullptr; T* d_gexit = nullptr;
    auto layout = [&](Arena& a) {
        (void)a.take<unsigned char>(exclusive_scan_slab_bytes(ntiles + 1));
        d_counts = a.take<uint64_t>(ntiles + 1);
        d_gentry = a.take<uint64_t>(ngroups);
        d_marks = a.take<unsigned char>(ntiles * geo.B);
        d_gexit = a.take<T>(n);
    };
    PSACX_TRY(slab_layout(c, layout));
    PSACX_HIP(c, hipMemsetAsync(d_counts, 0, (ntiles + 1) * sizeof(uint64_t), c->stream));
    PSACX_HIP(c, hipMemsetAsync(d_gentry, 0xFF, ngroups * sizeof(uint64_t), c->stream));
    PSACX_HIP(c, hipMemsetAsync(d_marks, 0, ntiles * geo.B, c->stream));
    const int grid = grid_for(c, ngroups * 256, 256, 8);
    hipLaunchKernelGGL((lz_exit_kernel<T>), dim3(grid), dim3(256), 0, c->stream, d_lpf, n, geo, ngroups, d_gexit);
    hipLaunchKernelGGL((lz_top_kernel<T>), dim3(1), dim3(64), 0, c->stream, (const T*)d_gexit, n, span, d_gentry);
    hipLaunchKernelGGL((lz_mark_kernel<T>), dim3(grid), dim3(256), 0, c->stream, d_lpf, n, geo, ngroups,
                       (const uint64_t*)d_gentry, d_marks, d_counts);
    PSACX_HIP(c, hipGetLastError());
    PSACX_TRY(select_positions(c, d_counts, ntiles, false, z));      // (cleared above with the counts)
    if (!d_start) return PSACX_OK;                    // count query
    if (*z + 1 > cap) return PSACX_ERANGE;
    PSACX_HIP(c, select_emit(c, d_marks, geo.B, ntiles, d_counts, LzEmit<T>{d_lpf, d_src, n, d_start, d_psrc}));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

template <typename T>
int check_lz77_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const T* d_start, const T* d_psrc, uint64_t z, uint64_t* errors) {
    if (!c || !errors) return PSACX_EINVAL;
    *errors = 0;
    PSACX_TRY(index_check_n<T>(n));
    if (!d_start || (z && !d_psrc) || (n && !d_text) || z > n) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(ensure_slab(c, 4096));
    unsigned long long* d_err = reinterpret_cast<unsigned long long*>(c->slab);
    PSACX_HIP(c, hipMemsetAsync(d_err, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL((check_lz77_kernel<T>), dim3(grid_for(c, n + 1, 256, 16)), dim3(256), 0, c->stream, d_text, n, d_start, d_psrc, z, d_err);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long bad = 0;
    PSACX_HIP(c, hipMemcpyAsync(&bad, d_err, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    *errors = bad;
    return PSACX_OK;
}

// The host-pointer forms: SA and LCP are staged (staging.hpp), the index is built, and the results come back.
template <typename T>
int lpf_host(psacx_ctx* c, uint64_t n, const T* SA, const T* LCP, T* lpf, T* src) {
    if (!c) return PSACX_EINVAL;
    PSACX_TRY(index_check_n<T>(n));
    if (!lpf || !src) return PSACX_EINVAL;
    if (n == 0) return PSACX_OK;
    if (!SA || !LCP) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    RmqLayout Y;
    rmq_layout(n, Y);
    uint64_t entries = 0;
    Staging s(c, "lpf");
    T* d_SA = (T*)s.upload(SA, n * sizeof(T));
    T* d_LCP = (T*)s.upload(LCP, n * sizeof(T));
    T* d_index = (T*)s.alloc(Y.entries * sizeof(T));
    T* d_lpf = (T*)s.alloc(n * sizeof(T));
    T* d_src = (T*)s.alloc(n * sizeof(T));
    if (s.rc == PSACX_OK) s.rc = rmq_index_dev<T>(c, d_LCP, n, d_index, &entries);
    if (s.rc == PSACX_OK) s.rc = lpf_dev<T>(c, n, d_SA, d_LCP, d_index, d_lpf, d_src);
    s.download(lpf, d_lpf, n * sizeof(T));
    s.download(src, d_src, n * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// start == NULL: the count query.  The factor array stays on the device.
template <typename T>
int lz77_host(psacx_ctx* c, uint64_t n, const T* SA, const T* LCP, T* start, T* src, uint64_t cap, uint64_t* z) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    PSACX_TRY(index_check_n<T>(n));
    if ((start == nullptr) != (src == nullptr)) return PSACX_EINVAL;
    if (n == 0) {
        if (start && cap < 1) return PSACX_ERANGE;
        if (start) start[0] = 0;
        return PSACX_OK;
    }
    if (!SA || !LCP) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    RmqLayout Y;
    rmq_layout(n, Y);
    uint64_t entries = 0;
    Staging s(c, "lz77");
    T* d_SA = (T*)s.upload(SA, n * sizeof(T));
    T* d_LCP = (T*)s.upload(LCP, n * sizeof(T));
    T* d_index = (T*)s.alloc(Y.entries * sizeof(T));
    T* d_lpf = (T*)s.alloc(n * sizeof(T));
    T* d_src = (T*)s.alloc(n * sizeof(T));
    if (s.rc == PSACX_OK) s.rc = rmq_index_dev<T>(c, d_LCP, n, d_index, &entries);
    if (s.rc == PSACX_OK) s.rc = lpf_dev<T>(c, n, d_SA, d_LCP, d_index, d_lpf, d_src);
    if (s.rc == PSACX_OK) s.rc = lz77_dev<T>(c, n, d_lpf, d_src, (T*)nullptr, (T*)nullptr, 0, z);
    if (s.rc != PSACX_OK || !start) return s.rc;
    if (*z + 1 > cap) return PSACX_ERANGE;
    T* d_start = (T*)s.alloc((*z + 1) * sizeof(T));
    T* d_psrc = (T*)s.alloc((*z + 1) * sizeof(T));
    if (s.rc == PSACX_OK) s.rc = lz77_dev<T>(c, n, d_lpf, d_src, d_start, d_psrc, *z + 1, z);
    s.download(start, d_start, (*z + 1) * sizeof(T));
    s.download(src, d_psrc, *z * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

} // namespace psacx

using namespace psacx;

extern "C" {

#define PSACX_LZ_ABI(S, T)                                                                                                                    \
    int psacx_lpf_dev_##S(psacx_ctx* c, uint64_t n, const T* sa, const T* lcp, const T* index, T* lpf, T* src) {                                \
        return lpf_dev<T>(c, n, sa, lcp, index, lpf, src);                                                                                      \
    }                                                                                                                                           \
    int psacx_lz77_dev_##S(psacx_ctx* c, uint64_t n, const T* lpf, const T* src, T* start, T* psrc, uint64_t cap, uint64_t* z) {                \
        return lz77_dev<T>(c, n, lpf, src, start, psrc, cap, z);                                                                                \
    }                                                                                                                                           \
    int psacx_check_lz77_dev_##S(psacx_ctx* c, const uint8_t* text, uint64_t n, const T* start, const T* psrc, uint64_t z, uint64_t* errors) {  \
        return check_lz77_dev<T>(c, text, n, start, psrc, z, errors);                                                                           \
    }                                                                                                                                           \
    int psacx_lpf_##S(psacx_ctx* c, uint64_t n, const T* sa, const T* lcp, T* lpf, T* src) { return lpf_host<T>(c, n, sa, lcp, lpf, src); }     \
    int psacx_lz77_##S(psacx_ctx* c, uint64_t n, const T* sa, const T* lcp, T* start, T* src, uint64_t cap, uint64_t* z) {                      \
        return lz77_host<T>(c, n, sa, lcp, start, src, cap, z);                                                                                 \
    }
PSACX_LZ_ABI(u32, uint32_t)
PSACX_LZ_ABI(u64, uint64_t)
#undef PSACX_LZ_ABI

} // extern "C"
