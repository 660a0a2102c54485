// Shared by the query command lines (locate, lce, overlaps, lz77, repeats, mems, kmismatch, kedit, fmindex): the error rule, a wall clock, the readers of their
// inputs, the --index choice, the owner of the ctx and the device memory of a run, and the u32 / u64 overload pairs of the calls that
// more than one of them makes (construction, index, occurrences, the table over a text or a set, longest match, BWT, document counts and lists, the FM-index).  read_file is the one of bench_common.hpp.
#pragma once
#include <chrono>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/psacx.h"
#include "bench_common.hpp"

namespace query_cli {

using bench_cli::read_file;

inline void must(psacx_ctx* c, int rc) {
    if (rc == PSACX_OK) return;
    std::string msg = std::string("psacx: ") + psacx_strerror(rc);
    const char* detail = c ? psacx_last_hip_error(c) : "";
    if (detail && detail[0]) msg += std::string(" [") + detail + "]";
    throw std::runtime_error(msg);
}

inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

inline bool number(const char* w) {
    const std::string s = w;
    return !s.empty() && s.find_first_not_of("0123456789") == std::string::npos;
}

// the strings of a set are the runs of raw between '\n', laid back to back in text with their m + 1 offsets in soff (gsac); empty
// lines are dropped
inline void split_lines(const std::string& raw, std::string& text, std::vector<uint64_t>& soff) {
    text.clear();
    text.reserve(raw.size());
    soff.assign(1, 0);
    for (std::size_t b = 0; b < raw.size();) {
        std::size_t e = raw.find('\n', b);
        if (e == std::string::npos) e = raw.size();
        if (e > b) { text.append(raw, b, e - b); soff.push_back(text.size()); }
        b = e + 1;
    }
}

// --index 32|64|auto
inline bool index_known(const std::string& index) { return index == "32" || index == "64" || index == "auto"; }
inline bool use32(const std::string& index, uint64_t n) { return index == "32" || (index == "auto" && n < 0xFFFFFFFEull); }

// The ctx of a run and the device memory it holds: freed when the run ends or throws, the buffers first.
struct Session {
    psacx_ctx* c;
    std::vector<void*> held;
    explicit Session(int device) : c(nullptr) { must(nullptr, psacx_create(&c, device, nullptr)); }
    ~Session() { for (std::size_t i = 0; i < held.size(); ++i) (void)psacx_dev_free(c, held[i]); psacx_destroy(c); }
    void* dev(uint64_t bytes) { void* p = nullptr; must(c, psacx_dev_alloc(c, &p, bytes ? bytes : 1)); held.push_back(p); return p; }
    // gives one buffer back before the run ends (fmindex drops text and SA once its index stands)
    void release(void* p) {
        for (std::size_t i = 0; i < held.size(); ++i)
            if (held[i] == p) { held.erase(held.begin() + i); (void)psacx_dev_free(c, p); return; }
    }
private:
    Session(const Session&);
    Session& operator=(const Session&);
};

// off == nullptr: one text
inline int construct(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, uint32_t flags, uint32_t* sa, uint32_t* isa, uint32_t* lcp) {
    return off ? psacx_construct_gsa_dev_u32(c, t, n, off, m, 0, flags, sa, isa, lcp) : psacx_construct_dev_u32(c, t, n, 0, flags, sa, isa, lcp);
}
inline int construct(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, uint32_t flags, uint64_t* sa, uint64_t* isa, uint64_t* lcp) {
    return off ? psacx_construct_gsa_dev_u64(c, t, n, off, m, 0, flags, sa, isa, lcp) : psacx_construct_dev_u64(c, t, n, 0, flags, sa, isa, lcp);
}
inline int rmq_index(psacx_ctx* c, const uint32_t* v, uint64_t n, uint32_t* index, uint64_t* e) { return psacx_rmq_index_dev_u32(c, v, n, index, e); }
inline int rmq_index(psacx_ctx* c, const uint64_t* v, uint64_t n, uint64_t* index, uint64_t* e) { return psacx_rmq_index_dev_u64(c, v, n, index, e); }
inline int occurrences(psacx_ctx* c, const uint32_t* sa, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* lb, const uint32_t* ub, uint64_t q,
                       uint64_t limit, uint64_t* start, uint32_t* pos, uint32_t* sid, uint64_t cap, uint64_t* total) {
    return psacx_occurrences_dev_u32(c, sa, n, off, m, lb, ub, q, limit, start, pos, sid, cap, total);
}
inline int occurrences(psacx_ctx* c, const uint64_t* sa, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* lb, const uint64_t* ub, uint64_t q,
                       uint64_t limit, uint64_t* start, uint64_t* pos, uint64_t* sid, uint64_t cap, uint64_t* total) {
    return psacx_occurrences_dev_u64(c, sa, n, off, m, lb, ub, q, limit, start, pos, sid, cap, total);
}

// ends == nullptr: one text
inline int lookup_table(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, uint32_t k, uint32_t* tab, uint16_t* code, uint32_t* sg, uint64_t* e) {
    return ends ? psacx_lookup_table_gsa_dev_u32(c, t, n, ends, k, tab, code, sg, e) : psacx_lookup_table_dev_u32(c, t, n, nullptr, k, tab, code, sg, e);
}
inline int lookup_table(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, uint32_t k, uint64_t* tab, uint16_t* code, uint32_t* sg, uint64_t* e) {
    return ends ? psacx_lookup_table_gsa_dev_u64(c, t, n, ends, k, tab, code, sg, e) : psacx_lookup_table_dev_u64(c, t, n, nullptr, k, tab, code, sg, e);
}
inline int match(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint32_t* sa, const uint32_t* tab, uint32_t k, const uint16_t* code,
                 const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t flags, uint64_t max_len, uint64_t entries, uint32_t* len, uint32_t* lb,
                 uint32_t* ub) {
    return ends ? psacx_match_gsa_dev_u32(c, t, n, ends, sa, tab, k, code, pat, poff, q, flags, max_len, entries, len, lb, ub)
                : psacx_match_dev_u32(c, t, n, sa, tab, k, code, pat, poff, q, flags, max_len, entries, len, lb, ub);
}
inline int match(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint64_t* sa, const uint64_t* tab, uint32_t k, const uint16_t* code,
                 const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t flags, uint64_t max_len, uint64_t entries, uint64_t* len, uint64_t* lb,
                 uint64_t* ub) {
    return ends ? psacx_match_gsa_dev_u64(c, t, n, ends, sa, tab, k, code, pat, poff, q, flags, max_len, entries, len, lb, ub)
                : psacx_match_dev_u64(c, t, n, sa, tab, k, code, pat, poff, q, flags, max_len, entries, len, lb, ub);
}
inline int bwt(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint32_t* sa, uint8_t* b, uint32_t* f, uint64_t* p) {
    return psacx_bwt_dev_u32(c, t, n, ends, sa, b, f, p);
}
inline int bwt(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint64_t* sa, uint8_t* b, uint32_t* f, uint64_t* p) {
    return psacx_bwt_dev_u64(c, t, n, ends, sa, b, f, p);
}

inline int fm_build(psacx_ctx* c, uint64_t n, const uint8_t* b, const uint32_t* f, const uint32_t* sa, uint64_t s, uint64_t* fm, psacx_fm_info* i) {
    return psacx_fm_index_dev_u32(c, n, b, f, sa, s, fm, i);
}
inline int fm_build(psacx_ctx* c, uint64_t n, const uint8_t* b, const uint32_t* f, const uint64_t* sa, uint64_t s, uint64_t* fm, psacx_fm_info* i) {
    return psacx_fm_index_dev_u64(c, n, b, f, sa, s, fm, i);
}
inline int fm_count(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t* lb, uint32_t* ub) {
    return psacx_fm_count_dev_u32(c, fm, i, pat, poff, q, lb, ub);
}
inline int fm_count(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint64_t* lb, uint64_t* ub) {
    return psacx_fm_count_dev_u64(c, fm, i, pat, poff, q, lb, ub);
}
inline int fm_occurrences(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint64_t* off, uint64_t m, const uint32_t* lb, const uint32_t* ub,
                          uint64_t q, uint64_t limit, uint64_t* start, uint32_t* pos, uint32_t* sid, uint64_t cap, uint64_t* total) {
    return psacx_fm_occurrences_dev_u32(c, fm, i, off, m, lb, ub, q, limit, start, pos, sid, cap, total);
}
inline int fm_occurrences(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint64_t* off, uint64_t m, const uint64_t* lb, const uint64_t* ub,
                          uint64_t q, uint64_t limit, uint64_t* start, uint64_t* pos, uint64_t* sid, uint64_t cap, uint64_t* total) {
    return psacx_fm_occurrences_dev_u64(c, fm, i, off, m, lb, ub, q, limit, start, pos, sid, cap, total);
}

// the range-minimum index of d_values, in memory of the session: the size query, then the build
template <typename IT>
inline IT* rmq_index_of(Session& s, const IT* d_values, uint64_t n, uint64_t* entries) {
    must(s.c, rmq_index(s.c, (const IT*)nullptr, n, (IT*)nullptr, entries));
    IT* d_index = (IT*)s.dev(*entries * sizeof(IT));
    must(s.c, rmq_index(s.c, d_values, n, d_index, entries));
    return d_index;
}

inline int doc_index(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* sa, const uint32_t* lcp, const uint32_t* index, uint32_t* prev,
                     uint32_t* dup) { return psacx_doc_index_dev_u32(c, n, off, m, sa, lcp, index, prev, dup); }
inline int doc_index(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* sa, const uint64_t* lcp, const uint64_t* index, uint64_t* prev,
                     uint64_t* dup) { return psacx_doc_index_dev_u64(c, n, off, m, sa, lcp, index, prev, dup); }
inline int doc_count(psacx_ctx* c, uint64_t n, const uint32_t* dup, const uint32_t* lb, const uint32_t* ub, uint64_t q, uint32_t* docs) {
    return psacx_doc_count_dev_u32(c, n, dup, lb, ub, q, docs);
}
inline int doc_count(psacx_ctx* c, uint64_t n, const uint64_t* dup, const uint64_t* lb, const uint64_t* ub, uint64_t q, uint64_t* docs) {
    return psacx_doc_count_dev_u64(c, n, dup, lb, ub, q, docs);
}
inline int doc_list(psacx_ctx* c, const uint32_t* sa, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* prev, const uint32_t* lb, const uint32_t* ub,
                    uint64_t q, uint64_t max_cand, uint64_t* start, uint32_t* sid, uint32_t* pos, uint64_t cap, uint64_t* total) {
    return psacx_doc_list_dev_u32(c, sa, n, off, m, prev, lb, ub, q, max_cand, start, sid, pos, cap, total);
}
inline int doc_list(psacx_ctx* c, const uint64_t* sa, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* prev, const uint64_t* lb, const uint64_t* ub,
                    uint64_t q, uint64_t max_cand, uint64_t* start, uint64_t* sid, uint64_t* pos, uint64_t cap, uint64_t* total) {
    return psacx_doc_list_dev_u64(c, sa, n, off, m, prev, lb, ub, q, max_cand, start, sid, pos, cap, total);
}

// the doc counts of q intervals in HBM, from LCP and its index: dup in memory of the session, then one launch; docs comes back
template <typename IT>
inline void doc_counts_of(Session& s, uint64_t n, const uint64_t* d_soff, uint64_t m, const IT* d_sa, const IT* d_lcp, const IT* d_index, const IT* d_lb,
                          const IT* d_ub, uint64_t q, std::vector<IT>& docs) {
    IT* d_dup = (IT*)s.dev((n + 1) * sizeof(IT));
    IT* d_docs = (IT*)s.dev(q * sizeof(IT) + 1);
    must(s.c, doc_index(s.c, n, d_soff, m, d_sa, d_lcp, d_index, (IT*)nullptr, d_dup));
    must(s.c, doc_count(s.c, n, d_dup, d_lb, d_ub, q, d_docs));
    docs.assign(q, 0);
    if (q) must(s.c, psacx_copy_d2h(s.c, docs.data(), d_docs, q * sizeof(IT)));
}

} // namespace query_cli
