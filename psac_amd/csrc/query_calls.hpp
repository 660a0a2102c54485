// query_calls.hpp -- what the query layer calls across its .hip files (locate.hip, rmq.hip, lz.hip, repeats.hip, mems.hip, kmismatch.hip, kedit.hip, docs.hip, fm.hip, and check.hip and
// ansv.hip where they serve it), declared once.  Every file that defines one of these includes this header too, so a signature
// that moves in one place alone does not compile.  A template that another file calls is declared here and instantiated for both index
// widths where it is defined; the calls that exist per width only (the sorts of psacx_u32.hip / psacx_u64.hip, the two scans) have
// overloads by entry type here, so that no caller re-enters the C ABI or keeps width shims of its own.  What the host-pointer forms
// share beyond that is in staging.hpp.
#pragma once
#include "engine.hpp"

namespace psacx {

// check.hip: the m + 1 offsets of a string set on the device start at 0, end at n and ascend strictly (PSACX_EINVAL otherwise; uses the
// first bytes of the ctx slab and waits); and the bitmap of the string ends of valid offsets into bits[(n >> 5) + 1], queued on the
// ctx stream
int string_offsets_valid_dev(psacx_ctx* c, const uint64_t* d_off, uint64_t m, uint64_t n);
int string_ends_bitmap_dev(psacx_ctx* c, const uint64_t* d_off, uint64_t m, uint64_t n, uint32_t* bits);

// locate.hip: the scan of scan.hpp over 64-bit entries, queued on the ctx stream, and the bytes it takes at the base of the ctx slab:
// a caller that keeps scratch of its own in the slab leaves the first exclusive_scan_slab_bytes(len) bytes to the scan and sizes the
// slab before it places anything
int exclusive_scan_u64_dev(psacx_ctx* c, uint64_t* d_a, uint64_t len);
int exclusive_scan_u32_dev(psacx_ctx* c, uint32_t* d_a, uint64_t len);           // (32-bit entries whose sum stays below 2^32: docs.hip)
uint64_t exclusive_scan_slab_bytes(uint64_t len);
// the scan of d_a[0 .. len), len >= 1, and its last entry -- the sum of all but the last -- in *total: one copy, one wait
int scan_total_u64_dev(psacx_ctx* c, uint64_t* d_a, uint64_t len, uint64_t* total);

// locate.hip: psacx_locate_dev_* itself, and with d_ends psacx_locate_gsa_dev_* (uses the first words of the ctx slab; waits), instantiated
// there for both widths
template <typename T>
int locate_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const T* d_SA, const T* d_table, uint32_t k, const uint16_t* code,
               const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, T* d_lb, T* d_ub, const uint32_t* d_ends = nullptr);
// locate.hip: psacx_match_dev_* itself, and with set psacx_match_gsa_dev_*, which insists on d_ends (waits), instantiated there for both
// widths
template <typename T>
int match_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, bool set, const T* d_SA, const T* d_table, uint32_t k,
              const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, uint32_t flags, uint64_t max_len, uint64_t out_entries,
              T* d_len, T* d_lb, T* d_ub);

// repeats.hip: psacx_bwt_dev_* itself (uses the first word of the ctx slab; waits), instantiated there for both widths
template <typename T>
int bwt_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, uint8_t* d_bwt, uint32_t* d_first,
            uint64_t* primary);

// ansv.hip: all nearest smaller values of an array in HBM into two arrays of n 64-bit entries (pyramid in the ctx slab; waits)
int ansv_dev_u32(psacx_ctx* c, const uint32_t* in, uint64_t n, int lt, int rt, uint64_t nonsv, uint64_t* l, uint64_t* r);
int ansv_dev_u64(psacx_ctx* c, const uint64_t* in, uint64_t n, int lt, int rt, uint64_t nonsv, uint64_t* l, uint64_t* r);

// rmq.hip: psacx_rmq_index_dev_* itself (size query with d_index == nullptr; waits; keeps the psacx_profile bookkeeping), instantiated
// there for both widths
template <typename T>
int rmq_index_dev(psacx_ctx* c, const T* d_values, uint64_t n, T* d_index, uint64_t* entries);

// mems.hip: psacx_mems_dev_* itself (kernels in mems.hpp; waits), instantiated there for both widths
template <typename T>
int mems_dev(psacx_ctx* c, uint64_t n, const T* d_SA, const T* d_LCP, const T* d_index, const uint8_t* d_bwt, const uint32_t* d_first,
             const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, const T* d_mlen, const T* d_mlb, const T* d_mub, uint64_t min_len,
             uint64_t max_occ, uint32_t flags, uint64_t* d_qpos, T* d_tpos, T* d_len, uint64_t cap, uint64_t* z, uint64_t* work);

// kmismatch.hip: psacx_kmismatch_dev_* itself (kernels in kmismatch.hpp; waits), instantiated there for both widths
template <typename T>
int kmismatch_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, const T* d_table, uint32_t k,
                  const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, uint32_t e, uint64_t max_cand, uint64_t* d_qid,
                  T* d_tpos, uint8_t* d_dist, uint64_t cap, uint64_t* z, uint64_t* work);

// kmismatch.hip: the front end kmismatch_dev and kedit_dev share, after their own argument checks.  A batch without d_pat must be all
// empty (PSACX_EINVAL; one blocking copy of poff[q]).  One block of s holds the Q + 1 piece offsets, the Q + 1 candidate starts, `extra`
// bytes for the caller and the Q piece intervals, Q = q E1; the pieces are cut, searched by locate_dev (which refuses malformed
// offsets before anything is written), the pieces of patterns shorter than E1 are emptied, and the interval counts are scanned:
// total candidates.  Waits.  Instantiated there for both widths.
struct Staging;
template <typename T>
struct PieceCandidates { uint64_t *d_boff, *d_cstart; unsigned char* d_extra; T *d_lb, *d_ub; uint64_t Q, total; };
template <typename T>
int piece_candidates_dev(psacx_ctx* c, Staging& s, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, const T* d_table,
                         uint32_t k, const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, uint32_t E1, size_t extra,
                         PieceCandidates<T>& pc);

// kedit.hip: psacx_kedit_dev_* itself (kernels in kedit.hpp; waits), instantiated there for both widths
template <typename T>
int kedit_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const T* d_SA, const T* d_table, uint32_t k,
              const uint16_t* code, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, uint32_t e, uint64_t max_cand, uint32_t flags,
              uint64_t* d_qid, T* d_tpos, T* d_len, uint8_t* d_dist, uint64_t cap, uint64_t* z, uint64_t* work);

// fm.hip: psacx_fm_index_dev_* (size query with d_fm == nullptr), psacx_fm_count_dev_* and psacx_fm_occurrences_dev_* themselves (kernels and
// the layout of the blob in fm.hpp; all wait), instantiated there for both widths
template <typename T>
int fm_index_dev(psacx_ctx* c, uint64_t n, const uint8_t* d_bwt, const uint32_t* d_first, const T* d_SA, uint64_t sample, uint64_t* d_fm,
                 psacx_fm_info* info);
template <typename T>
int fm_count_dev(psacx_ctx* c, const uint64_t* d_fm, const psacx_fm_info* info, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q, T* d_lb,
                 T* d_ub);
template <typename T>
int fm_occurrences_dev(psacx_ctx* c, const uint64_t* d_fm, const psacx_fm_info* info, const uint64_t* d_off, uint64_t m, const T* d_lb, const T* d_ub,
                       uint64_t q, uint64_t limit, uint64_t* d_start, T* d_pos, T* d_sid, uint64_t cap, uint64_t* total);
// fm.hip: psacx_fm_text_samples_dev_* (size query with d_ts == nullptr) and psacx_fm_extract_dev_* themselves (both wait)
template <typename T>
int fm_text_samples_dev(psacx_ctx* c, uint64_t n, const T* d_SA, const uint64_t* d_off, uint64_t m, uint64_t rate, T* d_ts, uint64_t* entries);
template <typename T>
int fm_extract_dev(psacx_ctx* c, const uint64_t* d_fm, const psacx_fm_info* info, const T* d_ts, uint64_t rate, const uint64_t* d_off, uint64_t m,
                   const T* d_pos, const T* d_len, uint64_t q, uint64_t* d_start, uint8_t* d_out, uint64_t cap, uint64_t* total);

// psacx_u32.hip / psacx_u64.hip: pair_sort_keys_dev of construct.hpp: n >= 1 pairs (b1, b2) sorted in place on their low `bits` bits by the
// rank-pair sort, whose buffers it lays out from the base of the ctx slab; waits; leaves the statistics and the profiling state of the
// context as they were (kedit.hip sorts its raw hits by it)
int pair_sort_keys_dev_u32(psacx_ctx* c, uint32_t* b1, uint32_t* b2, uint64_t n, uint32_t bits);
int pair_sort_keys_dev_u64(psacx_ctx* c, uint64_t* b1, uint64_t* b2, uint64_t n, uint32_t bits);
// the same sort on the low `bits` bits of the first word alone: pairs of equal first words stay in the order they came in (docs.hip sorts
// the ranks by their string by it)
int pair_sort_first_dev_u32(psacx_ctx* c, uint32_t* b1, uint32_t* b2, uint64_t n, uint32_t bits);
int pair_sort_first_dev_u64(psacx_ctx* c, uint64_t* b1, uint64_t* b2, uint64_t n, uint32_t bits);

// the sorts and the scans above by the width of their entries, for the templates of the query layer
inline int pair_sort_keys_dev_any(psacx_ctx* c, uint32_t* b1, uint32_t* b2, uint64_t n, uint32_t bits) { return pair_sort_keys_dev_u32(c, b1, b2, n, bits); }
inline int pair_sort_keys_dev_any(psacx_ctx* c, uint64_t* b1, uint64_t* b2, uint64_t n, uint32_t bits) { return pair_sort_keys_dev_u64(c, b1, b2, n, bits); }
inline int pair_sort_first_dev_any(psacx_ctx* c, uint32_t* b1, uint32_t* b2, uint64_t n, uint32_t bits) { return pair_sort_first_dev_u32(c, b1, b2, n, bits); }
inline int pair_sort_first_dev_any(psacx_ctx* c, uint64_t* b1, uint64_t* b2, uint64_t n, uint32_t bits) { return pair_sort_first_dev_u64(c, b1, b2, n, bits); }
inline int exclusive_scan_dev_any(psacx_ctx* c, uint32_t* d_a, uint64_t len) { return exclusive_scan_u32_dev(c, d_a, len); }
inline int exclusive_scan_dev_any(psacx_ctx* c, uint64_t* d_a, uint64_t len) { return exclusive_scan_u64_dev(c, d_a, len); }

// the bits of x, at least 1: the key width of a sort whose largest key is x
inline uint32_t bits_of(uint64_t x) { uint32_t b = 1; while (b < 64 && (x >> b)) ++b; return b; }

constexpr uint64_t RMQ_MAX_N = 1ull << 48;             // 64^PYR_MAX: the top level of the range-minimum index is one group

// n of a call that takes (or builds) the range-minimum index, with entries of type T
template <typename T>
inline int index_check_n(uint64_t n) {
    if (sizeof(T) == 4 && n > 0xFFFFFFFEull) return PSACX_ERANGE;
    if (n > RMQ_MAX_N) return PSACX_ERANGE;
    return PSACX_OK;
}

} // namespace psacx
