// staging.hpp -- device memory of a call beside the ctx slab (which belongs to the device forms), for the time of the call: the staged
// arrays of every host-pointer form, and the arrays a device form sizes by its input or by what it has counted so far (mark bytes,
// shell records, piece intervals, key words, code arrays).  Everything allocated is freed on every path.  rc is sticky: after the
// first failure every later step does nothing.  What the host forms with a pattern batch share sits here too: the check of the batch
// on the host, its upload, and the lookup table built beside the staged text.
#pragma once
#include "query_calls.hpp"

namespace psacx {

// The pattern batch of a host-pointer call: poff[0] == 0, poff ascends, and pat is there when poff[q] > 0 (PSACX_EINVAL otherwise).
// *S = poff[q].  poff != nullptr is the caller's test.
inline int pattern_batch_valid(const uint8_t* pat, const uint64_t* poff, uint64_t q, uint64_t* S) {
    if (poff[0] != 0) return PSACX_EINVAL;
    for (uint64_t i = 0; i < q; ++i) if (poff[i + 1] < poff[i]) return PSACX_EINVAL;
    *S = poff[q];
    return *S && !pat ? PSACX_EINVAL : PSACX_OK;
}

struct DeviceBatch { const uint8_t* pat; const uint64_t* poff; };

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
    // Several arrays in one allocation: layout(Arena&) takes them; it runs once dry to size the block and, if the block is there, once
    // on it.  The caller tests rc before it uses what layout set.
    template <typename Layout>
    void place(Layout layout) {
        Arena dry(nullptr);
        layout(dry);
        Arena ar((char*)alloc(dry.off));
        if (rc == PSACX_OK) layout(ar);
    }
    void step(hipError_t r) { if (rc == PSACX_OK && r != hipSuccess) { c->hip_err = hipGetErrorString(r); (void)hipGetLastError(); rc = PSACX_EHIP; } }
    void* upload(const void* src, size_t bytes) {
        void* p = alloc(bytes);
        if (p && src && bytes) step(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, c->stream));
        return p;
    }
    void download(void* dst, const void* src, size_t bytes) { if (rc == PSACX_OK && dst && bytes) step(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); }
    // a pattern batch that passed pattern_batch_valid: the poff[q] pattern bytes, then the q + 1 offsets
    DeviceBatch upload_batch(const uint8_t* pat, const uint64_t* poff, uint64_t q) {
        return DeviceBatch{(const uint8_t*)upload(pat, poff[q]), (const uint64_t*)upload(poff, (q + 1) * sizeof(uint64_t))};
    }
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

// locate.hip: the lookup table of a staged text (a string set with d_ends), in memory of s and queued on the ctx stream: one histogram
// for the alphabet, the table sized by it, the counts and their scan.  code[256] is filled; nullptr for k == 0 or once s.rc is set
// (PSACX_EINVAL where B^k is too large).  Instantiated there for both widths.
template <typename T>
T* staged_lookup_table(Staging& s, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, uint32_t k, uint16_t code[256]);

} // namespace psacx
