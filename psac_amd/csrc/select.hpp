// select.hpp -- the ordered compaction of the query layer: one mark byte (0 or 1) per element, in whole tiles; the number of marks per
// tile; the scan of scan.hpp over them (through locate.hip), whose last entry is the number z of marked elements; and one kernel that
// hands the k-th marked element and its place k to a functor.  The LZ77 parse (lz.hip) and the repeats (repeats.hip) are its callers:
// their Emit functors are beside their kernels (lz.hpp, repeats.hpp).
//
// A thread owns SELECT_PER = 4 marks, one 32-bit word; a tile is `tile` elements, a multiple of 4 and at most SELECT_TILE_MAX, so that
// one workgroup of 256 threads takes a tile per step and one block scan places its marks.
#pragma once
#include "query_calls.hpp"

namespace psacx {

constexpr int SELECT_PER = 4;                          // marks of a thread: one 32-bit word
constexpr unsigned SELECT_TILE_MAX = 256 * SELECT_PER;

// counts[t] = the marks set in tile t, for tiles of TILE = SELECT_TILE_MAX elements; sel holds whole tiles (the caller has cleared
// what lies behind its last element).  A caller whose own kernels leave the tile counts (lz_mark_kernel) does not need this.
template <int TILE>
__global__ __launch_bounds__(256) void select_count_kernel(const unsigned char* __restrict__ sel, uint64_t ntiles, uint64_t* __restrict__ counts) {
    static_assert(TILE == (int)SELECT_TILE_MAX, "every thread counts one word");
    __shared__ uint32_t sh[256 / WAVE];
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint32_t word = *reinterpret_cast<const uint32_t*>(sel + t * TILE + threadIdx.x * SELECT_PER);
        const uint32_t total = block_reduce<256, uint32_t>((uint32_t)__popc(word & 0x01010101u), OpSum(), sh);
        if (threadIdx.x == 0) counts[t] = total;
    }
}

// counts: the exclusive sums of the tile counts, ntiles + 1 entries.  emit(k, j) for the k-th marked element j, in the order of j (a
// tile whose two neighbouring counts agree is passed over); emit.finish(z) once, by one thread.  Emit: a few pointers, by value.
template <typename Emit>
__global__ __launch_bounds__(256) void select_emit_kernel(const unsigned char* __restrict__ marks, unsigned tile, uint64_t ntiles,
                                                          const uint64_t* __restrict__ counts, Emit emit) {
    __shared__ uint32_t sh[256 / WAVE + 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) emit.finish(counts[ntiles]);
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t base = counts[t];
        if (counts[t + 1] == base) continue;
        const uint64_t ts = t * tile;
        const unsigned j0 = threadIdx.x * SELECT_PER;
        uint32_t word = 0;
        if (j0 < tile) word = *reinterpret_cast<const uint32_t*>(marks + ts + j0) & 0x01010101u;     // (tile is a multiple of 4, marks holds whole tiles)
        uint32_t total;
        uint64_t at = base + block_scan_exclusive<256, uint32_t>((uint32_t)__popc(word), OpSum(), 0u, sh, &total);
#pragma unroll
        for (int d = 0; d < SELECT_PER; ++d) {
            if (!((word >> (8 * d)) & 1u)) continue;
            emit(at, ts + j0 + d);
            ++at;
        }
    }
}

// The tile counts d_counts[0 .. ntiles) become their exclusive sums over ntiles + 1 entries (the scan's block sums are at the base of
// the ctx slab: query_calls.hpp), and *z = the last of them, the number of marked elements.  clear_last: d_counts[ntiles] is not 0
// yet.  Waits.
inline int select_positions(psacx_ctx* c, uint64_t* d_counts, uint64_t ntiles, bool clear_last, uint64_t* z) {
    if (clear_last) PSACX_HIP(c, hipMemsetAsync(d_counts + ntiles, 0, sizeof(uint64_t), c->stream));
    PSACX_TRY(exclusive_scan_u64_dev(c, d_counts, ntiles + 1));
    PSACX_HIP(c, hipMemcpyAsync(z, d_counts + ntiles, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// select_emit_kernel over the tiles, queued on the ctx stream
template <typename Emit>
inline hipError_t select_emit(psacx_ctx* c, const unsigned char* d_marks, unsigned tile, uint64_t ntiles, const uint64_t* d_counts, Emit emit) {
    hipLaunchKernelGGL((select_emit_kernel<Emit>), dim3(grid_for(c, ntiles * 256, 256, 8)), dim3(256), 0, c->stream, d_marks, tile, ntiles, d_counts, emit);
    return hipGetLastError();
}

} // namespace psacx
