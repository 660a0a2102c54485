// mems.hip -- the maximal exact matches of a batch of patterns from the matching statistics, SA, LCP, the range-minimum index of LCP and
// the BWT (include/psacx.h: "maximal exact matches"; kernels in mems.hpp).  The reference has no counterpart.
#include "engine.hpp"
#include "mems.hpp"
#include "staging.hpp"

namespace psacx {

// psacx_mems_dev_*: the offsets check, then
//  - the walk that counts, the two scans, the walk that writes the shell records, the marks of the candidates, the counts of the mark
//    tiles, their scan and the triples; or
//  - PSACX_MEMS_SUPER: the counts of the kept slots, their scan and the expansion.
// Scratch in the ctx slab: the block sums of the scans first (exclusive_scan_dev puts them at the slab's base), then the two count
// arrays of poff[q] + 1 entries (one for PSACX_MEMS_SUPER, and one word for the kept slots).  Shell records, candidate starts, mark
// bytes and tile counts take memory of their own for the time of the call; nothing is written before the memory is there.
template <typename T>
int mems_dev(psacx_ctx* c, uint64_t n, const T* d_SA, const T* d_LCP, const T* d_index, const uint8_t* d_bwt, const uint32_t* d_first,
             const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, const T* d_mlen, const T* d_mlb, const T* d_mub, uint64_t min_len,
             uint64_t max_occ, uint32_t flags, uint64_t* d_qpos, T* d_tpos, T* d_len, uint64_t cap, uint64_t* z, uint64_t* work) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    if (work) work[0] = work[1] = 0;
    PSACX_TRY(index_check_n<T>(n));
    if (flags & ~MEMS_SUPER) return PSACX_EINVAL;
    if ((d_qpos == nullptr) != (d_tpos == nullptr) || (d_qpos == nullptr) != (d_len == nullptr)) return PSACX_EINVAL;
    if (q == 0 || n == 0) return PSACX_OK;
    if (!d_poff) return PSACX_EINVAL;
    if (min_len < 1) min_len = 1;
    const bool super = (flags & MEMS_SUPER) != 0;
    PSACX_HIP(c, hipSetDevice(c->device));

    // the offsets, checked on the device, and the number of slots
    PSACX_TRY(ensure_slab(c, 4096));
    unsigned long long* d_bad = reinterpret_cast<unsigned long long*>(c->slab);
    PSACX_HIP(c, hipMemsetAsync(d_bad, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(mems_offsets_kernel, dim3(grid_for(c, q, 256, 8)), dim3(256), 0, c->stream, d_poff, q, d_bad);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long bad = 0;
    uint64_t S = 0;
    PSACX_HIP(c, hipMemcpyAsync(&bad, d_bad, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipMemcpyAsync(&S, d_poff + q, sizeof(S), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (bad) return PSACX_EINVAL;
    if (S == 0) return PSACX_OK;
    if (!d_mlen || !d_mlb || !d_mub || (d_qpos && !d_SA)) return PSACX_EINVAL;
    if (!super && (!d_LCP || !d_index || !d_bwt || !d_first || !d_pat)) return PSACX_EINVAL;

    uint64_t *d_scnt = nullptr, *d_ccnt = nullptr;
    unsigned long long* d_kept = nullptr;
    auto layout = [&](Arena& a) {
        (void)a.take<unsigned char>(exclusive_scan_slab_bytes(S + 1));
        d_scnt = a.take<uint64_t>(S + 1);
        if (super) d_kept = a.take<unsigned long long>(1);
        else d_ccnt = a.take<uint64_t>(S + 1);
    };
    PSACX_TRY(slab_layout(c, layout));

    if (super) {
        PSACX_HIP(c, hipMemsetAsync(d_kept, 0, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL((mems_super_count_kernel<T>), dim3(grid_for(c, S + 1, 256, 8)), dim3(256), 0, c->stream, d_poff, q, S, d_mlen, d_mlb, d_mub, n,
                           min_len, max_occ, d_scnt, d_kept);
        PSACX_HIP(c, hipGetLastError());
        PSACX_TRY(exclusive_scan_u64_dev(c, d_scnt, S + 1));
        unsigned long long kept = 0;
        PSACX_HIP(c, hipMemcpyAsync(z, d_scnt + S, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        PSACX_HIP(c, hipMemcpyAsync(&kept, d_kept, sizeof(kept), hipMemcpyDeviceToHost, c->stream));
        PSACX_HIP(c, hipStreamSynchronize(c->stream));
        if (work) { work[0] = kept; work[1] = *z; }
        if (!d_qpos) return PSACX_OK;                 // count query
        if (*z > cap) return PSACX_ERANGE;
        if (*z == 0) return PSACX_OK;
        const uint64_t tiles = (*z + OCC_TILE - 1) / OCC_TILE;
        hipLaunchKernelGGL((mems_super_expand_kernel<T>), dim3(grid_for(c, tiles * 256, 256, 8)), dim3(256), 0, c->stream, d_SA, n, d_poff, q, S, d_mlen,
                           d_mlb, d_mub, (const uint64_t*)d_scnt, *z, d_qpos, d_tpos, d_len);
        PSACX_HIP(c, hipGetLastError());
        PSACX_HIP(c, hipStreamSynchronize(c->stream));
        return PSACX_OK;
    }

    const dim3 wgrid(grid_for(c, (S + 1) * RMQ_LANES, 256, 8));
    hipLaunchKernelGGL((mems_walk_kernel<T, false>), wgrid, dim3(256), 0, c->stream, n, d_LCP, d_index, d_poff, q, S, d_mlen, d_mlb, d_mub, min_len, max_occ,
                       d_scnt, d_ccnt, (uint64_t)0, (MemsShell<T>*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
    PSACX_HIP(c, hipGetLastError());
    PSACX_TRY(exclusive_scan_u64_dev(c, d_scnt, S + 1));
    PSACX_TRY(exclusive_scan_u64_dev(c, d_ccnt, S + 1));
    uint64_t nshells = 0, total = 0;
    PSACX_HIP(c, hipMemcpyAsync(&nshells, d_scnt + S, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipMemcpyAsync(&total, d_ccnt + S, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (work) { work[0] = nshells; work[1] = total; }
    if (total == 0 || c->knobs.mems_stop == 1) return PSACX_OK;

    const uint64_t ntiles = (total + OCC_TILE - 1) / OCC_TILE;
    Staging s(c, "mems");
    MemsShell<T>* d_shells = (MemsShell<T>*)s.alloc(nshells * sizeof(MemsShell<T>));
    uint64_t* d_slot = (uint64_t*)s.alloc(nshells * sizeof(uint64_t));
    uint64_t* d_cstart = (uint64_t*)s.alloc((nshells + 1) * sizeof(uint64_t));
    unsigned char* d_marks = (unsigned char*)s.alloc(ntiles * OCC_TILE);
    uint64_t* d_counts = (uint64_t*)s.alloc((ntiles + 1) * sizeof(uint64_t));
    if (s.rc != PSACX_OK) return s.rc;
    hipLaunchKernelGGL((mems_walk_kernel<T, true>), wgrid, dim3(256), 0, c->stream, n, d_LCP, d_index, d_poff, q, S, d_mlen, d_mlb, d_mub, min_len, max_occ,
                       d_scnt, d_ccnt, nshells, d_shells, d_slot, d_cstart);
    PSACX_HIP(c, hipGetLastError());
    if (c->knobs.mems_stop == 2) { s.step(hipStreamSynchronize(c->stream)); return s.rc; }
    PSACX_HIP(c, hipMemsetAsync(d_marks + total, 0, ntiles * OCC_TILE - total, c->stream));
    hipLaunchKernelGGL((mems_mark_kernel<T>), dim3(grid_for(c, ntiles * 256, 256, 8)), dim3(256), 0, c->stream, (const MemsShell<T>*)d_shells,
                       (const uint64_t*)d_slot, (const uint64_t*)d_cstart, nshells, total, d_bwt, d_first, d_pat, n, d_marks);
    PSACX_HIP(c, hipGetLastError());
    if (c->knobs.mems_stop == 3) { s.step(hipStreamSynchronize(c->stream)); return s.rc; }
    // (the scan of the tile counts may have to grow the slab, which the second walk still reads: it has to be through first)
    if (exclusive_scan_slab_bytes(ntiles + 1) > c->slab_bytes) PSACX_HIP(c, hipStreamSynchronize(c->stream));
    hipLaunchKernelGGL(select_count_kernel<OCC_TILE>, dim3(grid_for(c, ntiles * 256, 256, 8)), dim3(256), 0, c->stream, (const unsigned char*)d_marks, ntiles,
                       d_counts);
    PSACX_HIP(c, hipGetLastError());
    PSACX_TRY(select_positions(c, d_counts, ntiles, true, z));
    if (!d_qpos) return PSACX_OK;                     // count query
    if (*z > cap) return PSACX_ERANGE;
    s.step(select_emit(c, d_marks, OCC_TILE, ntiles, d_counts,
                       MemsEmit<T>{d_shells, d_slot, d_cstart, nshells, d_SA, n, d_qpos, d_tpos, d_len}));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// The host-pointer form: text, SA, LCP and patterns are staged (staging.hpp); the bitmap of the string ends, the table when k > 0, the
// statistics, the index and the BWT are built beside them; the count query sizes the lists and the triples come back.  Everything
// allocated is freed on every path.  qpos == nullptr: the count query.
template <typename T>
int mems_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, const T* LCP, const uint8_t* pat,
              const uint64_t* poff, uint64_t q, uint32_t k, uint64_t min_len, uint64_t max_occ, uint32_t flags, uint64_t* qpos, T* tpos, T* len,
              uint64_t cap, uint64_t* z) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    PSACX_TRY(index_check_n<T>(n));
    if (flags & ~MEMS_SUPER) return PSACX_EINVAL;
    if ((qpos == nullptr) != (tpos == nullptr) || (qpos == nullptr) != (len == nullptr)) return PSACX_EINVAL;
    if (q == 0 || n == 0) return PSACX_OK;
    if (!text || !SA || !LCP || !poff || (offsets && (m == 0 || m > n))) return PSACX_EINVAL;
    uint64_t S = 0;
    PSACX_TRY(pattern_batch_valid(pat, poff, q, &S));
    if (S == 0) return PSACX_OK;
    PSACX_HIP(c, hipSetDevice(c->device));
    RmqLayout Y;
    rmq_layout(n, Y);
    Staging s(c, "mems");
    const uint8_t* d_text = (const uint8_t*)s.upload(text, n);
    const T* d_SA = (const T*)s.upload(SA, n * sizeof(T));
    const T* d_LCP = (const T*)s.upload(LCP, n * sizeof(T));
    const DeviceBatch b = s.upload_batch(pat, poff, q);
    const uint8_t* d_pat = b.pat;
    const uint64_t* d_poff = b.poff;
    const uint32_t* d_ends = offsets ? s.string_ends(offsets, m, n) : nullptr;
    T* d_mlen = (T*)s.alloc(S * sizeof(T));
    T* d_mlb = (T*)s.alloc(S * sizeof(T));
    T* d_mub = (T*)s.alloc(S * sizeof(T));
    T* d_index = (T*)s.alloc(Y.entries * sizeof(T));
    uint8_t* d_bwt = (uint8_t*)s.alloc(n);
    uint32_t* d_first = (uint32_t*)s.alloc(((n >> 5) + 1) * sizeof(uint32_t));
    uint16_t code[256];
    const T* d_table = staged_lookup_table<T>(s, d_text, n, d_ends, k, code);
    if (s.rc == PSACX_OK)
        s.rc = match_dev<T>(c, d_text, n, d_ends, d_ends != nullptr, d_SA, d_table, k, k ? code : nullptr, d_pat, d_poff, q, PSACX_MATCH_SUFFIXES, 0, S, d_mlen,
                            d_mlb, d_mub);
    uint64_t entries = 0;
    if (s.rc == PSACX_OK) s.rc = rmq_index_dev<T>(c, d_LCP, n, d_index, &entries);
    if (s.rc == PSACX_OK) s.rc = bwt_dev<T>(c, d_text, n, d_ends, d_SA, d_bwt, d_first, (uint64_t*)nullptr);
    if (s.rc == PSACX_OK)
        s.rc = mems_dev<T>(c, n, d_SA, d_LCP, d_index, d_bwt, d_first, d_pat, d_poff, q, d_mlen, d_mlb, d_mub, min_len, max_occ, flags, (uint64_t*)nullptr,
                           (T*)nullptr, (T*)nullptr, 0, z, (uint64_t*)nullptr);
    if (s.rc != PSACX_OK || !qpos) return s.rc;
    if (*z > cap) return PSACX_ERANGE;
    const uint64_t room = *z ? *z : 1;
    uint64_t* d_qpos = (uint64_t*)s.alloc(room * sizeof(uint64_t));
    T* d_tpos = (T*)s.alloc(room * sizeof(T));
    T* d_len = (T*)s.alloc(room * sizeof(T));
    if (s.rc == PSACX_OK)
        s.rc = mems_dev<T>(c, n, d_SA, d_LCP, d_index, d_bwt, d_first, d_pat, d_poff, q, d_mlen, d_mlb, d_mub, min_len, max_occ, flags, d_qpos, d_tpos, d_len,
                           *z, z, (uint64_t*)nullptr);
    s.download(qpos, d_qpos, *z * sizeof(uint64_t));
    s.download(tpos, d_tpos, *z * sizeof(T));
    s.download(len, d_len, *z * sizeof(T));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

} // namespace psacx

using namespace psacx;

extern "C" {

#define PSACX_MEMS_ABI(S, T)                                                                                                                     \
    int psacx_mems_dev_##S(psacx_ctx* c, uint64_t n, const T* sa, const T* lcp, const T* index, const uint8_t* bwt, const uint32_t* first,        \
                           const uint8_t* pat, const uint64_t* poff, uint64_t q, const T* mlen, const T* mlb, const T* mub, uint64_t min_len,     \
                           uint64_t max_occ, uint32_t flags, uint64_t* qpos, T* tpos, T* len, uint64_t cap, uint64_t* z, uint64_t* work) {        \
        return mems_dev<T>(c, n, sa, lcp, index, bwt, first, pat, poff, q, mlen, mlb, mub, min_len, max_occ, flags, qpos, tpos, len, cap, z,      \
                           work);                                                                                                                \
    }                                                                                                                                            \
    int psacx_mems_##S(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const T* lcp,                 \
                       const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint64_t min_len, uint64_t max_occ, uint32_t flags,      \
                       uint64_t* qpos, T* tpos, T* len, uint64_t cap, uint64_t* z) {                                                              \
        return mems_host<T>(c, text, n, off, m, sa, lcp, pat, poff, q, k, min_len, max_occ, flags, qpos, tpos, len, cap, z);                      \
    }
PSACX_MEMS_ABI(u32, uint32_t)
PSACX_MEMS_ABI(u64, uint64_t)
#undef PSACX_MEMS_ABI

} // extern "C"
