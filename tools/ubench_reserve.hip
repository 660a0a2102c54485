// The tile reservations of the 512-way ISA levels alone (sa_kernels.hpp: rebucket_first_kernel's fused level, partition_packed_kernel):
// workgroups of 512 threads, thread t does one returning agent-scope 32-bit atomicAdd on cursor[row][t] -- 16 cache lines per row -- and
// nothing else.  What the reservations cost when every workgroup takes the same row, and when resident workgroups take different ones.
// hipcc --offload-arch=gfx950 -O3 -o tools/ubench_reserve tools/ubench_reserve.hip
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
constexpr unsigned NCLS = 512, ROWS = 512;
// MODE 0: row = block % p (p rows in turn; p = 1: the fused level today)
// MODE 1: row = block / 1024 (level 2 today: 1024 tiles of 8192 records per class of 2^23 positions)
// MODE 2: row = (block % p) * (512 / p) + block / (1024 * p) (level 2 with the tiles striped over p classes)
template <int MODE>
__global__ __launch_bounds__(512) void k(unsigned* cursor, unsigned p, unsigned* out) {
    const unsigned b = blockIdx.x;
    const unsigned row = MODE == 0 ? b % p : MODE == 1 ? b / 1024u : (b % p) * (ROWS / p) + b / (1024u * p);
    if (row >= ROWS) return;
    const unsigned at = atomicAdd(&cursor[(size_t)row * NCLS + threadIdx.x], 8u);
    if (at == 0xffffffffu) out[0] = at;
}
int main() {
    unsigned *cursor, *out;
    CK(hipMalloc(&cursor, (size_t)ROWS * NCLS * sizeof(unsigned))); CK(hipMalloc(&out, 64));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    struct { int mode; unsigned grid, p; const char* what; } runs[] = {
        {0, 1u << 20, 1, "2^20 workgroups, one row (fused level today)"},
        {0, 1u << 20, 8, "2^20 workgroups, row = block % 8"}, {0, 1u << 20, 16, "2^20 workgroups, row = block % 16"},
        {0, 1u << 20, 32, "2^20 workgroups, row = block % 32"}, {0, 1u << 20, 64, "2^20 workgroups, row = block % 64"},
        {1, 1u << 19, 1, "2^19 workgroups, row = block / 1024 (level 2 today)"},
        {2, 1u << 19, 8, "2^19 workgroups, striped over 8 classes"}, {2, 1u << 19, 16, "2^19 workgroups, striped over 16 classes"},
        {2, 1u << 19, 32, "2^19 workgroups, striped over 32 classes"}, {2, 1u << 19, 64, "2^19 workgroups, striped over 64 classes"}};
    for (const auto& r : runs) {
        auto fn = [&] {
            if (r.mode == 0) k<0><<<r.grid, 512>>>(cursor, r.p, out); else if (r.mode == 1) k<1><<<r.grid, 512>>>(cursor, r.p, out); else k<2><<<r.grid, 512>>>(cursor, r.p, out);
        };
        CK(hipMemset(cursor, 0, (size_t)ROWS * NCLS * sizeof(unsigned)));
        fn(); CK(hipDeviceSynchronize());
        CK(hipEventRecord(e0)); for (int i = 0; i < 3; ++i) fn(); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= 3;
        printf("%-52s %8.3f ms = %6.2f ns per workgroup\n", r.what, ms, ms * 1e6 / r.grid);
    }
    return 0;
}
