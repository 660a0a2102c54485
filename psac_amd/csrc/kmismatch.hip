// kmismatch.hip -- pattern search with up to e mismatches over text and SA resident in HBM (include/psacx.h: "pattern search with
// mismatches"; kernels in kmismatch.hpp).  The reference has no counterpart.
#include "engine.hpp"
#include "kmismatch.hpp"
#include "staging.hpp"

namespace psacx {

// The front end of kmismatch_dev and kedit_dev (query_calls.hpp): the piece offsets, the locate call over them, the counts of the
// intervals and their scan.
template <typename T>
int piece_candidates_dev(psacx_ctx* c, Staging& s, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, const T* d_table,
                         uint32_t k, const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, uint32_t E1, size_t extra,
                         PieceCandidates<T>& pc) {
    if (!d_pat) {                                     // only a batch of empty patterns may come without a buffer
        uint64_t S = 0;
        PSACX_HIP(c, hipMemcpy(&S, d_poff + q, sizeof(S), hipMemcpyDeviceToHost));
        if (S) return PSACX_EINVAL;
    }
    const uint64_t Q = q * E1;
    pc.Q = Q;
    s.place([&](Arena& a) {
        pc.d_boff = a.take<uint64_t>(Q + 1);
        pc.d_cstart = a.take<uint64_t>(Q + 1);
        pc.d_extra = extra ? a.take<unsigned char>(extra) : nullptr;
        pc.d_lb = a.take<T>(Q);
        pc.d_ub = a.take<T>(Q);
    });
    if (s.rc != PSACX_OK) return s.rc;
    hipLaunchKernelGGL(kmm_pieces_kernel, dim3(grid_for(c, Q + 1, 256, 8)), dim3(256), 0, c->stream, d_poff, q, E1, pc.d_boff);
    PSACX_HIP(c, hipGetLastError());
    // (the offsets are checked by the search, on the piece offsets: boff[j (e + 1)] = poff[j], so a poff that does not start at 0 or
    // descends gives piece offsets that do neither, and the search returns PSACX_EINVAL before it writes)
    PSACX_TRY(locate_dev<T>(c, d_text, n, d_SA, d_table, k, code, d_pat ? d_pat : d_text, (const uint64_t*)pc.d_boff, Q, pc.d_lb, pc.d_ub, d_ends));
    hipLaunchKernelGGL((kmm_short_kernel<T>), dim3(grid_for(c, Q, 256, 8)), dim3(256), 0, c->stream, d_poff, q, E1, pc.d_lb, pc.d_ub);
    hipLaunchKernelGGL((occ_counts_kernel<T>), dim3(grid_for(c, Q + 1, 256, 8)), dim3(256), 0, c->stream, (const T*)pc.d_lb, (const T*)pc.d_ub, Q, n, (uint64_t)0,
                       pc.d_cstart);
    PSACX_HIP(c, hipGetLastError());
    return scan_total_u64_dev(c, pc.d_cstart, Q + 1, &pc.total);
}

template int piece_candidates_dev<uint32_t>(psacx_ctx*, Staging&, const uint8_t*, uint64_t, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t,
                                            const uint16_t*, const uint8_t*, const uint64_t*, uint64_t, uint32_t, size_t, PieceCandidates<uint32_t>&);
template int piece_candidates_dev<uint64_t>(psacx_ctx*, Staging&, const uint8_t*, uint64_t, const uint32_t*, const uint64_t*, const uint64_t*, uint32_t,
                                            const uint16_t*, const uint8_t*, const uint64_t*, uint64_t, uint32_t, size_t, PieceCandidates<uint64_t>&);

// psacx_kmismatch_dev_*: the front end above, the marks of the candidates, the counts of the mark tiles, their scan and the triples.
// Scratch.  The ctx slab holds the three words of the searches and the block sums of the scans only (both at its base, one after the
// other).  Two blocks of memory of the call's own: one sized by the pieces -- piece offsets, candidate starts, the word of the tested
// candidates and the piece intervals -- and, once the number of candidates is known and has passed max_cand, one sized by the
// candidates -- mark bytes and tile counts.  Nothing is written before the memory is there.
template <typename T>
int kmismatch_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, const T* d_table, uint32_t k,
                  const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, uint32_t e, uint64_t max_cand, uint64_t* d_qid,
                  T* d_tpos, uint8_t* d_dist, uint64_t cap, uint64_t* z, uint64_t* work) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    if (work) work[0] = work[1] = 0;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    if (e > KMM_MAX_E) return PSACX_EINVAL;
    if ((d_qid == nullptr) != (d_tpos == nullptr) || (d_qid == nullptr) != (d_dist == nullptr)) return PSACX_EINVAL;
    if ((d_table == nullptr) != (k == 0) || (code == nullptr) != (k == 0)) return PSACX_EINVAL;
    if (q == 0 || n == 0) return PSACX_OK;
    if (!d_text || !d_SA || !d_poff) return PSACX_EINVAL;
    const uint32_t E1 = e + 1;
    if (q > (~0ull >> 8) / E1) return PSACX_ERANGE;
    PSACX_HIP(c, hipSetDevice(c->device));

    Staging s(c, "kmismatch");
    PieceCandidates<T> pc;
    PSACX_TRY(piece_candidates_dev<T>(c, s, d_text, n, d_ends, d_SA, d_table, k, code, d_pat, d_poff, q, E1, sizeof(unsigned long long), pc));
    uint64_t *const d_boff = pc.d_boff, *const d_cstart = pc.d_cstart;
    unsigned long long* const d_tested = reinterpret_cast<unsigned long long*>(pc.d_extra);      // the word of the tested candidates
    T* const d_lb = pc.d_lb;
    const uint64_t Q = pc.Q, total = pc.total;
    if (work) work[0] = total;
    if (max_cand && total > max_cand) return PSACX_ERANGE;
    if (total == 0 || c->knobs.kmismatch_stop == 1) return PSACX_OK;

    const uint64_t ntiles = (total + OCC_TILE - 1) / OCC_TILE;
    unsigned char* d_marks = nullptr;
    uint64_t* d_counts = nullptr;
    s.place([&](Arena& a) {
        d_marks = a.take<unsigned char>(ntiles * OCC_TILE);
        d_counts = a.take<uint64_t>(ntiles + 1);
    });
    if (s.rc != PSACX_OK) return s.rc;
    PSACX_HIP(c, hipMemsetAsync(d_tested, 0, sizeof(unsigned long long), c->stream));
    PSACX_HIP(c, hipMemsetAsync(d_marks + total, 0, ntiles * OCC_TILE - total, c->stream));
    {
        const dim3 grid(grid_for(c, ntiles * 256, 256, 8));
        if (d_ends)
            hipLaunchKernelGGL((kmm_verify_kernel<T, true>), grid, dim3(256), 0, c->stream, d_text, n, d_ends, d_SA, d_pat, (const uint64_t*)d_boff, (const T*)d_lb,
                               (const uint64_t*)d_cstart, Q, E1, total, d_marks, d_tested);
        else
            hipLaunchKernelGGL((kmm_verify_kernel<T, false>), grid, dim3(256), 0, c->stream, d_text, n, d_ends, d_SA, d_pat, (const uint64_t*)d_boff, (const T*)d_lb,
                               (const uint64_t*)d_cstart, Q, E1, total, d_marks, d_tested);
    }
    PSACX_HIP(c, hipGetLastError());
    if (c->knobs.kmismatch_stop != 2) {
        hipLaunchKernelGGL(select_count_kernel<OCC_TILE>, dim3(grid_for(c, ntiles * 256, 256, 8)), dim3(256), 0, c->stream, (const unsigned char*)d_marks,
                           ntiles, d_counts);
        PSACX_HIP(c, hipGetLastError());
    }
    unsigned long long tested = 0;
    s.step(hipMemcpyAsync(&tested, d_tested, sizeof(tested), hipMemcpyDeviceToHost, c->stream));
    s.step(hipStreamSynchronize(c->stream));
    if (s.rc != PSACX_OK) return s.rc;
    if (work) work[1] = tested;
    if (c->knobs.kmismatch_stop == 2) return PSACX_OK;
    PSACX_TRY(select_positions(c, d_counts, ntiles, true, z));
    if (!d_qid) return PSACX_OK;                      // count query
    if (*z > cap) return PSACX_ERANGE;
    s.step(select_emit(c, d_marks, OCC_TILE, ntiles, d_counts,
                       KmmEmit<T>{d_boff, d_lb, d_cstart, Q, E1, d_SA, n, d_marks, d_qid, d_tpos, d_dist}));
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

// The host-pointer form: text, SA and patterns are staged (staging.hpp); the bitmap of the string ends and, when k > 0, the table
// are built beside them; the count query sizes the lists and the triples come back.  Everything allocated is freed on every path.
// qid == nullptr: the count query.
template <typename T>
int kmismatch_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const T* SA, const uint8_t* pat,
                   const uint64_t* poff, uint64_t q, uint32_t k, uint32_t e, uint64_t max_cand, uint64_t* qid, T* tpos, uint8_t* dist, uint64_t cap,
                   uint64_t* z) {
    if (!c || !z) return PSACX_EINVAL;
    *z = 0;
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    if (e > KMM_MAX_E) return PSACX_EINVAL;
    if ((qid == nullptr) != (tpos == nullptr) || (qid == nullptr) != (dist == nullptr)) return PSACX_EINVAL;
    if (q == 0 || n == 0) return PSACX_OK;
    if (!text || !SA || !poff || (offsets && (m == 0 || m > n))) return PSACX_EINVAL;
    uint64_t S = 0;
    PSACX_TRY(pattern_batch_valid(pat, poff, q, &S));
    if (S == 0) return PSACX_OK;
    PSACX_HIP(c, hipSetDevice(c->device));
    Staging s(c, "kmismatch");
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
        s.rc = kmismatch_dev<T>(c, d_text, n, d_ends, d_SA, d_table, k, cd, d_pat, d_poff, q, e, max_cand, (uint64_t*)nullptr, (T*)nullptr,
                                (uint8_t*)nullptr, 0, z, (uint64_t*)nullptr);
    if (s.rc != PSACX_OK || !qid) return s.rc;
    if (*z > cap) return PSACX_ERANGE;
    const uint64_t room = *z ? *z : 1;
    uint64_t* d_qid = (uint64_t*)s.alloc(room * sizeof(uint64_t));
    T* d_tpos = (T*)s.alloc(room * sizeof(T));
    uint8_t* d_dist = (uint8_t*)s.alloc(room);
    if (s.rc == PSACX_OK)
        s.rc = kmismatch_dev<T>(c, d_text, n, d_ends, d_SA, d_table, k, cd, d_pat, d_poff, q, e, max_cand, d_qid, d_tpos, d_dist, *z, z, (uint64_t*)nullptr);
    s.download(qid, d_qid, *z * sizeof(uint64_t));
    s.download(tpos, d_tpos, *z * sizeof(T));
    s.download(dist, d_dist, *z);
    s.step(hipStreamSynchronize(c->stream));
    return s.rc;
}

} // namespace psacx

using namespace psacx;

extern "C" {

#define PSACX_KMISMATCH_ABI(S, T)                                                                                                                \
    int psacx_kmismatch_dev_##S(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const T* sa, const T* table, uint32_t k,        \
                                const uint16_t code[256], const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t e, uint64_t max_cand,   \
                                uint64_t* qid, T* tpos, uint8_t* dist, uint64_t cap, uint64_t* z, uint64_t* work) {                              \
        return kmismatch_dev<T>(c, t, n, ends, sa, table, k, code, pat, poff, q, e, max_cand, qid, tpos, dist, cap, z, work);                    \
    }                                                                                                                                            \
    int psacx_kmismatch_##S(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const uint8_t* pat,      \
                            const uint64_t* poff, uint64_t q, uint32_t k, uint32_t e, uint64_t max_cand, uint64_t* qid, T* tpos, uint8_t* dist,  \
                            uint64_t cap, uint64_t* z) {                                                                                         \
        return kmismatch_host<T>(c, text, n, off, m, sa, pat, poff, q, k, e, max_cand, qid, tpos, dist, cap, z);                                 \
    }
PSACX_KMISMATCH_ABI(u32, uint32_t)
PSACX_KMISMATCH_ABI(u64, uint64_t)
#undef PSACX_KMISMATCH_ABI

} // extern "C"
