// staging.hpp -- device memory of a host-pointer call (psacx_locate_*, psacx_match_*, psacx_rmq_*, psacx_lce_*): the arrays are
// staged in memory of their own for the time of the call (the slab belongs to the device forms), and everything allocated is freed
// on every path.  rc is sticky: after the first failure every later step does nothing.
#pragma once
#include "engine.hpp"

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
};

} // namespace psacx
