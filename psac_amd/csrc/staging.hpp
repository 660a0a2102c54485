// staging.hpp -- device memory of a host-pointer call (psacx_locate_*, psacx_match_*, psacx_rmq_*, psacx_lce_*, psacx_overlaps_*,
// psacx_lpf_*, psacx_lz77_*, psacx_bwt_*, psacx_repeats_*, psacx_mems_*, psacx_kmismatch_*, psacx_kedit_*, psacx_doc_count_*, psacx_doc_list_*, psacx_fm_search_*) and of the device forms that need arrays for the time of a
// call (psacx_lpf_dev_*, psacx_repeats_dev_*: n entries; psacx_mems_dev_*: shell records and mark bytes; psacx_kmismatch_dev_*: piece
// intervals and mark bytes; psacx_doc_index_dev_*: the key words; psacx_doc_list_dev_*: candidate starts and mark bytes; psacx_fm_index_dev_*: two arrays of 16-bit codes): the arrays are staged in
// memory of their own (the slab belongs to the device forms), and everything allocated is freed on every path.  rc is sticky: after
// the first failure every later step does nothing.
#pragma once
#include "query_calls.hpp"

namespace psacx {

struct Staging {
    psacx_ctx* c; const char* label; int rc = PSACX_OK; std::vector<void*> mem;
    Staging(psacx_ctx* ctx, const char* what) : c(ctx), label(what) {}             // what: names the call in the hipMalloc(...) error text
    ~Staging() { for (void* p : mem) (void)hipFree(p); }
    void* alloc(size_t bytes) {
        if (rc != PSACX_OK) return nullptr;
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e != hipSuccess) { c->hip_err = std::string("hipMalloc(") + label + "): " + hipGetErrorString(e); (void)hipGetLastError(); rc = PSACX_ENOMEM; return nullptr; }
        mem.push_back(p);
        return p;
    }
    void step(hipError_t r) { if (rc == PSACX_OK && r != hipSuccess) { c->hip_err = hipGetErrorString(r); (void)hipGetLastError(); rc = PSACX_EHIP; } }
    void* upload(const void* src, size_t bytes) {
        void* p = alloc(bytes);
        if (p && src && bytes) step(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, c->stream));
        return p;
    }
    void download(void* dst, const void* src, size_t bytes) { if (rc == PSACX_OK && dst && bytes) step(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); }
    // The string set of a call: its m + 1 offsets go up (*d_off: where they are), are checked on the device (PSACX_EINVAL; waits), and
    // give the bitmap of the string ends, (n >> 5) + 1 words, queued on the ctx stream.  1 <= m <= n is the caller's test.
    const uint32_t* string_ends(const uint64_t* offsets, uint64_t m, uint64_t n, const uint64_t** d_off = nullptr) {
        const uint64_t* d = (const uint64_t*)upload(offsets, (m + 1) * sizeof(uint64_t));
        uint32_t* bits = (uint32_t*)alloc(((n >> 5) + 1) * sizeof(uint32_t));
        if (rc == PSACX_OK) rc = string_offsets_valid_dev(c, d, m, n);
        if (rc == PSACX_OK) rc = string_ends_bitmap_dev(c, d, m, n, bits);
        if (d_off) *d_off = d;
        return bits;
    }
};

} // namespace psacx
