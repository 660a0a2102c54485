// kedit.hip -- pattern search with up to e edits over text and SA resident in HBM (include/psacx.h: "pattern search with edits";
// kernels in kedit.hpp).  The reference has no counterpart.
#include "engine.hpp"
#include "kedit.hpp"
#include "staging.hpp"

namespace psacx {

// the kernels of kedit.hpp by the bucket of e and by text / set
#define KED_BY_BUCKET(e, CALL)                                                                                                      \
    do {                                                                                                                            \
        if ((e) <= 1) { CALL(1); } else if ((e) <= 2) { CALL(2); } else if ((e) <= 4) { CALL(4); } else if ((e) <= 8) { CALL(8); } else { CALL(15); } \
    } while (0)

template <typename T>
static void launch_verify(psacx_ctx* c, dim3 grid, uint32_t e, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, const uint8_t* d_pat,
                          const uint64_t* d_boff, const T* d_lb, const uint64_t* d_cstart, uint64_t Q, uint32_t E1, uint64_t total, uint32_t* d_mask,
                          uint64_t* d_cnt) {
#define KED_VERIFY(EB)                                                                                                                                   \
    if (d_ends) hipLaunchKernelGGL((ked_verify_kernel<T, true, EB>), grid, dim3(256), 0, c->stream, d_text, n, d_ends, d_SA, d_pat, d_boff, d_lb, d_cstart, Q, E1, \
                                   total, d_mask, d_cnt);                                                                                                \
    else hipLaunchKernelGGL((ked_verify_kernel<T, false, EB>), grid, dim3(256), 0, c->stream, d_text, n, d_ends, d_SA, d_pat, d_boff, d_lb, d_cstart, Q, E1, total, \
                            d_mask, d_cnt)
    KED_BY_BUCKET(e, KED_VERIFY);
#undef KED_VERIFY
}

template <typename T>
static void launch_align(psacx_ctx* c, dim3 grid, uint32_t e, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint8_t* d_pat,
                         const uint64_t* d_poff, uint64_t q, const uint64_t* d_qid, const T* d_tpos, uint64_t z, T* d_len, uint8_t* d_dist, uint32_t* d_best) {
#define KED_ALIGN(EB)                                                                                                                                   \
    if (d_ends) hipLaunchKernelGGL((ked_align_kernel<T, true, EB>), grid, dim3(256), 0, c->stream, d_text, n, d_ends, d_pat, d_poff, q, d_qid, d_tpos, z, d_len, \
                                   d_dist, d_best);                                                                                                     \
    else hipLaunchKernelGGL((ked_align_kernel<T, false, EB>), grid, dim3(256), 0, c->stream, d_text, n, d_ends, d_pat, d_poff, q, d_qid, d_tpos, z, d_len, d_dist, \
                            d_best)
    KED_BY_BUCKET(e, KED_ALIGN);
#undef KED_ALIGN
}

// psacx_kedit_dev_*: pieces, their search, the counts of their intervals and the scan by piece_candidates_dev; the masks of the candidates
// and the scan of their counts; the raw pairs, their sort and the unique; the forward pass over the distinct pairs; with
// PSACX_KEDIT_BEST the per-pattern minimum and a second compaction.
// Scratch.  The ctx slab: the three words of the searches and the block sums of the scans at its base, and, between
// the scan of the mask counts and the scan of the unique's tile counts, the buffers of the sort (pair_sort_keys_dev lays them out from the
// base and clears its error words itself; it copies the sorted keys back and waits, so the later scans may take the base again).
// Memory of the call's own: one block sized by the pieces, one by the candidates once they have passed max_cand, one by the raw hits
// once they are counted, one by the distinct hits.  Nothing is written to the outputs before all of it is there.
template <typename T>
int kedit_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, const T* d_table, uint32_t k,
              const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, uint32_t e, uint64_t max_cand, uint32_t flags,
              uint64_t* d_qid, T* d_tpos, T* d_len, uint8_t* d_dist, uint64_t cap, uint64_t* z, uint64_t* work) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    if (work) work[0] = work[1] = 0;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    if (e > KED_MAX_E || (flags & ~(uint32_t)PSACX_KEDIT_BEST)) return PSACX_EINVAL;
    if ((d_qid == nullptr) != (d_tpos == nullptr) || (d_qid == nullptr) != (d_len == nullptr) || (d_qid == nullptr) != (d_dist == nullptr)) return PSACX_EINVAL;
    if ((d_table == nullptr) != (k == 0) || (code == nullptr) != (k == 0)) return PSACX_EINVAL;
    if (q == 0 || n == 0) return PSACX_OK;
    if (sizeof(T) == 4 && q > 0xFFFFFFFFull) return PSACX_ERANGE;           // the pattern number is a key word of the sort
    if (!d_text || !d_SA || !d_poff) return PSACX_EINVAL;
    const uint32_t E1 = e + 1;
    if (q > (~0ull >> 8) / E1) return PSACX_ERANGE;
    const unsigned stop = c->knobs.kedit_stop;
    const bool best = (flags & PSACX_KEDIT_BEST) != 0;
    PSACX_HIP(c, hipSetDevice(c->device));

    Staging s(c, "kedit");
    PieceCandidates<T> pc;
    PSACX_TRY(piece_candidates_dev<T>(c, s, d_text, n, d_ends, d_SA, d_table, k, code, d_pat, d_poff, q, E1, 0, pc));
    uint64_t *const d_boff = pc.d_boff, *const d_cstart = pc.d_cstart;
    T* const d_lb = pc.d_lb;
    const uint64_t Q = pc.Q, total = pc.total;
    if (work) work[0] = total;
    if (max_cand && total > max_cand) return PSACX_ERANGE;
    if (total == 0 || stop == 1) return PSACX_OK;

    // the masks of the candidates and the raw hits
    uint32_t* d_mask = nullptr;
    uint64_t* d_cnt = nullptr;
    s.place([&](Arena& a) {
        d_mask = a.take<uint32_t>(total);
        d_cnt = a.take<uint64_t>(total + 1);
    });
    if (s.rc != PSACX_OK) return s.rc;
    PSACX_HIP(c, hipMemsetAsync(d_cnt + total, 0, sizeof(uint64_t), c->stream));
    const uint64_t ctiles = (total + OCC_TILE - 1) / OCC_TILE;
    launch_verify<T>(c, dim3(grid_for(c, ctiles * 256, 256, 8)), e, d_text, n, d_ends, d_SA, d_pat, (const uint64_t*)d_boff, (const T*)d_lb,
                     (const uint64_t*)d_cstart, Q, E1, total, d_mask, d_cnt);
    PSACX_HIP(c, hipGetLastError());
    uint64_t raw = 0;
    PSACX_TRY(scan_total_u64_dev(c, d_cnt, total + 1, &raw));
    if (work) work[1] = raw;
    if (raw == 0 || stop == 2) return PSACX_OK;

    // the raw pairs, sorted, and the marks of the unique
    const uint64_t rtiles = (raw + OCC_TILE - 1) / OCC_TILE;
    T *d_k1 = nullptr, *d_k2 = nullptr;
    unsigned char* d_marks = nullptr;
    uint64_t* d_counts = nullptr;
    s.place([&](Arena& a) {
        d_k1 = a.take<T>(raw);
        d_k2 = a.take<T>(raw);
        d_marks = a.take<unsigned char>(rtiles * OCC_TILE);
        d_counts = a.take<uint64_t>(rtiles + 1);
    });
    if (s.rc != PSACX_OK) return s.rc;
    hipLaunchKernelGGL((ked_emit_kernel<T>), dim3(grid_for(c, total, 256, 8)), dim3(256), 0, c->stream, (const uint32_t*)d_mask, (const uint64_t*)d_cnt, total,
                       (const uint64_t*)d_boff, (const T*)d_lb, (const uint64_t*)d_cstart, Q, E1, d_SA, n, d_k1, d_k2);
    PSACX_HIP(c, hipGetLastError());
    if (raw > 1) PSACX_TRY(pair_sort_keys_dev_any(c, d_k1, d_k2, raw, bits_of((q - 1) | (n - 1))));
    hipLaunchKernelGGL((ked_unique_kernel<T>), dim3(grid_for(c, rtiles * OCC_TILE, 256, 8)), dim3(256), 0, c->stream, (const T*)d_k1, (const T*)d_k2, raw,
                       rtiles * OCC_TILE, d_marks);
    hipLaunchKernelGGL(select_count_kernel<OCC_TILE>, dim3(grid_for(c, rtiles * 256, 256, 8)), dim3(256), 0, c->stream, (const unsigned char*)d_marks, rtiles,
                       d_counts);
    PSACX_HIP(c, hipGetLastError());
    uint64_t zu = 0;
    PSACX_TRY(select_positions(c, d_counts, rtiles, true, &zu));
    if (stop == 3) return PSACX_OK;
    if (!best) {
        *z = zu;
        if (!d_qid) return PSACX_OK;                  // count query
        if (zu > cap) return PSACX_ERANGE;
        s.step(select_emit(c, d_marks, OCC_TILE, rtiles, d_counts, KedPairEmit<T>{d_k1, d_k2, d_qid, d_tpos}));
        launch_align<T>(c, dim3(grid_for(c, zu, 256, 8)), e, d_text, n, d_ends, d_pat, d_poff, q, (const uint64_t*)d_qid, (const T*)d_tpos, zu, d_len, d_dist,
                        (uint32_t*)nullptr);
        s.step(hipGetLastError());
        s.step(hipStreamSynchronize(c->stream));
        return s.rc;
    }

    // PSACX_KEDIT_BEST: the distinct hits in lists of the call's own, the smallest distance of every pattern, the second compaction
    const uint64_t utiles = (zu + OCC_TILE - 1) / OCC_TILE;
    uint64_t *d_q0 = nullptr, *d_counts2 = nullptr;
    T *d_t0 = nullptr, *d_l0 = nullptr;
    uint8_t* d_d0 = nullptr;
    uint32_t* d_best = nullptr;
    unsigned char* d_marks2 = nullptr;
    s.place([&](Arena& a) {
        d_q0 = a.take<uint64_t>(zu);
        d_t0 = a.take<T>(zu);
        d_l0 = a.take<T>(zu);
        d_d0 = a.take<uint8_t>(zu);
        d_best = a.take<uint32_t>(q);
        d_marks2 = a.take<unsigned char>(utiles * OCC_TILE);
        d_counts2 = a.take<uint64_t>(utiles + 1);
    });
    if (s.rc != PSACX_OK) return s.rc;
    PSACX_HIP(c, hipMemsetAsync(d_best, 0xFF, q * sizeof(uint32_t), c->stream));
    s.step(select_emit(c, d_marks, OCC_TILE, rtiles, d_counts, KedPairEmit<T>{d_k1, d_k2, d_q0, d_t0}));
    launch_align<T>(c, dim3(grid_for(c, zu, 256, 8)), e, d_text, n, d_ends, d_pat, d_poff, q, (const uint64_t*)d_q0, (const T*)d_t0, zu, d_l0, d_d0, d_best);
    hipLaunchKernelGGL(ked_best_kernel, dim3(grid_for(c, utiles * OCC_TILE, 256, 8)), dim3(256), 0, c->stream, (const uint64_t*)d_q0, (const uint8_t*)d_d0,
                       (const uint32_t*)d_best, zu, utiles * OCC_TILE, d_marks2);
    hipLaunchKernelGGL(select_count_kernel<OCC_TILE>, dim3(grid_for(c, utiles * 256, 256, 8)), dim3(256), 0, c->stream, (const unsigned char*)d_marks2, utiles,
                       d_counts2);
    s.step(hipGetLastError());
    if (s.rc != PSACX_OK) return s.rc;
    PSACX_TRY(select_positions(c, d_counts2, utiles, true, z));
    if (!d_qid) return PSACX_OK;                      // count query
    if (*z > cap) return PSACX_ERANGE;
    s.step(select_emit(c, d_marks2, OCC_TILE, utiles, d_counts2, KedBestEmit<T>{d_q0, d_t0, d_l0, d_d0, d_qid, d_tpos, d_len, d_dist}));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// The host-pointer form: text, SA and patterns are staged (staging.hpp); the bitmap of the string ends and, when k > 0, the table
// are built beside them; the count query sizes the lists and the quadruples come back.  Everything allocated is freed on every
// path.  qid == nullptr: the count query.
template <typename T>
int kedit_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, const uint8_t* pat, const uint64_t* poff,
               uint64_t q, uint32_t k, uint32_t e, uint64_t max_cand, uint32_t flags, uint64_t* qid, T* tpos, T* len, uint8_t* dist, uint64_t cap,
               uint64_t* z) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    if (e > KED_MAX_E || (flags & ~(uint32_t)PSACX_KEDIT_BEST)) return PSACX_EINVAL;
    if ((qid == nullptr) != (tpos == nullptr) || (qid == nullptr) != (len == nullptr) || (qid == nullptr) != (dist == nullptr)) return PSACX_EINVAL;
    if (q == 0 || n == 0) return PSACX_OK;
    if (!text || !SA || !poff || (offsets && (m == 0 || m > n))) return PSACX_EINVAL;
    uint64_t S = 0;
    PSACX_TRY(pattern_batch_valid(pat, poff, q, &S));
    if (S == 0) return PSACX_OK;
    PSACX_HIP(c, hipSetDevice(c->device));
    Staging s(c, "kedit");
    const uint8_t* d_text = (const uint8_t*)s.upload(text, n);
    const T* d_SA = (const T*)s.upload(SA, n * sizeof(T));
    const DeviceBatch b = s.upload_batch(pat, poff, q);
    const uint8_t* d_pat = b.pat;
    const uint64_t* d_poff = b.poff;
    const uint32_t* d_ends = offsets ? s.string_ends(offsets, m, n) : nullptr;
    uint16_t code[256];
    const T* d_table = staged_lookup_table<T>(s, d_text, n, d_ends, k, code);
    const uint16_t* cd = k ? code : nullptr;
    if (s.rc == PSACX_OK)
        s.rc = kedit_dev<T>(c, d_text, n, d_ends, d_SA, d_table, k, cd, d_pat, d_poff, q, e, max_cand, flags, (uint64_t*)nullptr, (T*)nullptr, (T*)nullptr,
                            (uint8_t*)nullptr, 0, z, (uint64_t*)nullptr);
    if (s.rc != PSACX_OK || !qid) return s.rc;
    if (*z > cap) return PSACX_ERANGE;
    const uint64_t room = *z ? *z : 1;
    uint64_t* d_qid = (uint64_t*)s.alloc(room * sizeof(uint64_t));
    T* d_tpos = (T*)s.alloc(room * sizeof(T));
    T* d_len = (T*)s.alloc(room * sizeof(T));
    uint8_t* d_dist = (uint8_t*)s.alloc(room);
    if (s.rc == PSACX_OK)
        s.rc = kedit_dev<T>(c, d_text, n, d_ends, d_SA, d_table, k, cd, d_pat, d_poff, q, e, max_cand, flags, d_qid, d_tpos, d_len, d_dist, *z, z,
                            (uint64_t*)nullptr);
    s.download(qid, d_qid, *z * sizeof(uint64_t));
    s.download(tpos, d_tpos, *z * sizeof(T));
    s.download(len, d_len, *z * sizeof(T));
    s.download(dist, d_dist, *z);
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

} // namespace psacx

using namespace psacx;

extern "C" {

#define PSACX_KEDIT_ABI(S, T)                                                                                                                       \
    int psacx_kedit_dev_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const T* sa, const T* table, uint32_t k,               \
                            const uint16_t code[256], const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t e, uint64_t max_cand,          \
                            uint32_t flags, uint64_t* qid, T* tpos, T* len, uint8_t* dist, uint64_t cap, uint64_t* z, uint64_t* work) {             \
        return kedit_dev<T>(c, t, n, ends, sa, table, k, code, pat, poff, q, e, max_cand, flags, qid, tpos, len, dist, cap, z, work);               \
    }                                                                                                                                               \
    int psacx_kedit_##S(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const uint8_t* pat,             \
                        const uint64_t* poff, uint64_t q, uint32_t k, uint32_t e, uint64_t max_cand, uint32_t flags, uint64_t* qid, T* tpos, T* len, \
                        uint8_t* dist, uint64_t cap, uint64_t* z) {                                                                                 \
        return kedit_host<T>(c, text, n, off, m, sa, pat, poff, q, k, e, max_cand, flags, qid, tpos, len, dist, cap, z);                            \
    }
PSACX_KEDIT_ABI(u32, uint32_t)
PSACX_KEDIT_ABI(u64, uint64_t)
#undef PSACX_KEDIT_ABI

} // extern "C"
