// mems.hpp -- the maximal exact matches of a batch of patterns against the index resident in HBM: SA, LCP, the range-minimum index of
// LCP, the BWT with the bitmap of the ranks that start a string, and the matching statistics of every pattern position
// (include/psacx.h: "maximal exact matches").  The reference has no counterpart; kernels only, the calls are in mems.hip.  The text
// is no argument.
//
// Walk.  mems_walk_kernel<T, WRITE>: RMQ_LANES = 16 lanes per slot, as overlaps_kernel.  The slot's pattern comes from a search in
// poff.  Shell 0 is the slot's own interval; each further shell asks L at both ends of the interval so far, takes the larger as
// its depth, and widens the side (or sides) that holds it by rmq_last / rmq_first to the nearest value below.  The first pass
// counts shells and candidates per slot; the call scans both; the second pass repeats the walk and writes a record per shell, its
// slot, and the exclusive start of its candidates.
//
// Mark.  mems_mark_kernel: balanced by candidates as occ_expand_kernel is by outputs.  A workgroup owns the OCC_TILE candidate
// numbers of its tile whatever the shells are: one binary search in the candidate starts for its first shell, OCC_CHUNK starts in
// LDS, one LDS search per candidate.  A candidate is rank r of its shell; it survives iff its slot starts a pattern, or rank r
// starts a string, or bwt[r] differs from the pattern byte in front of the slot.  One mark byte per candidate, stored to
// neighbouring addresses by neighbouring lanes.
//
// Compaction.  The mark bytes go through select.hpp in tiles of OCC_TILE; MemsEmit finds the shell of a survivor by a search over
// all candidate starts (one per MEM, not per candidate), fetches SA[r] and stores the triple.
//
// PSACX_MEMS_SUPER needs neither walk nor marks: mems_super_count_kernel keeps a slot whose statistic is not shorter than its left
// neighbour's, the scan gives the starts, and mems_super_expand_kernel is the expansion of occ_expand_kernel with three outputs.
//
// Whatever the arrays hold: a statistics entry with lb >= ub or ub > n gives no shell; len is cut to what is left of the pattern; a
// walk step either strictly lowers the depth (which is at least 1) or ends the walk, and never narrows the interval, which stays
// inside [0, n]; so every candidate is a rank below n.  The records and starts are this call's own scratch.
#pragma once
#include "occurrences.hpp"
#include "rmq.hpp"
#include "select.hpp"

namespace psacx {

constexpr uint32_t MEMS_SUPER = 1u;                    // PSACX_MEMS_SUPER
constexpr uint64_t MEMS_STARTS = 1ull << 63;           // in the slot word of a shell: the slot starts its pattern
static_assert(OCC_TILE == (int)SELECT_TILE_MAX, "a tile of candidates is a tile of the compaction");

// One shell: its ranks are [nlb, ilb) and [iub, nub) -- nub is not kept, the candidate starts give the count -- at depth len
template <typename T>
struct alignas(4 * sizeof(T)) MemsShell { T nlb, ilb, iub, len; };

// bit p of a bitmap of 32-bit words
__device__ __forceinline__ bool mems_bit(const uint32_t* __restrict__ bits, uint64_t p) { return (bits[p >> 5] >> (p & 31)) & 1u; }

// poff[0] == 0 and poff[i] <= poff[i + 1] for the q + 1 offsets -- or *bad becomes nonzero (the rule of search_offsets_kernel)
__global__ __launch_bounds__(256) void mems_offsets_kernel(const uint64_t* __restrict__ poff, uint64_t q, unsigned long long* bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    bool wrong = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < q; i += stride) {
        if (i == 0 && poff[0] != 0) wrong = true;
        if (poff[i + 1] < poff[i]) wrong = true;
    }
    if (wrong) atomicOr(bad, 1ull);
}

template <typename T>
__device__ __forceinline__ uint64_t mems_L(const T* __restrict__ LCP, uint64_t x, uint64_t n) {
    return (x == 0 || x >= n) ? 0ull : (uint64_t)LCP[x];
}

// The statistics of slot p < S = poff[q] as the walk takes them: the pattern j that holds p, len cut to poff[j+1] - p; false where
// they give no shell.  starts: p == poff[j].
template <typename T>
__device__ __forceinline__ bool mems_slot(const uint64_t* __restrict__ poff, uint64_t q, const T* __restrict__ mlen, const T* __restrict__ mlb,
                                          const T* __restrict__ mub, uint64_t n, uint64_t p, uint64_t& l, uint64_t& lb, uint64_t& ub,
                                          bool& starts, uint64_t& room) {
    const uint64_t j = occ_last_le(poff, q + 1, p);
    if (j >= q) return false;
    const uint64_t p0 = poff[j], p1 = poff[j + 1];
    if (p0 > p || p1 <= p) return false;
    l = (uint64_t)mlen[p]; lb = (uint64_t)mlb[p]; ub = (uint64_t)mub[p];
    room = p1 - p;
    if (l > room) l = room;
    starts = p == p0;
    return lb < ub && ub <= n;
}

// !WRITE: shell_cnt[p], cand_cnt[p] = the shells and candidates of slot p for p < S, 0 for p == S.
// WRITE: both hold their exclusive sums; shell number shell_cnt[p] + k of slot p gets its record, its slot word and the start of its
// candidates, and cand_start[nshells] = the number of candidates.
template <typename T, bool WRITE>
__global__ __launch_bounds__(256) void mems_walk_kernel(uint64_t n, const T* __restrict__ LCP, const T* __restrict__ index,
                                                        const uint64_t* __restrict__ poff, uint64_t q, uint64_t S, const T* __restrict__ mlen,
                                                        const T* __restrict__ mlb, const T* __restrict__ mub, uint64_t min_len, uint64_t max_occ,
                                                        uint64_t* __restrict__ shell_cnt, uint64_t* __restrict__ cand_cnt, uint64_t nshells,
                                                        MemsShell<T>* __restrict__ shells, uint64_t* __restrict__ shell_slot,
                                                        uint64_t* __restrict__ cand_start) {
    RmqLayout Y;
    rmq_layout(n, Y);
    const unsigned sub = threadIdx.x % RMQ_LANES;
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / RMQ_LANES;
    const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / RMQ_LANES;
    for (uint64_t p = group; p <= S; p += ngroups) {
        uint64_t ns = 0, nc = 0;
        const uint64_t s0 = WRITE ? shell_cnt[p] : 0, c0 = WRITE ? cand_cnt[p] : 0;
        uint64_t l = 0, lb = 0, ub = 0, room = 0;
        bool starts = false;
        if (p < S && mems_slot<T>(poff, q, mlen, mlb, mub, n, p, l, lb, ub, starts, room)) {
            uint64_t ilb = lb, iub = lb;               // the interval so far: empty, shell 0 gains all of [lb, ub)
            uint64_t nlb = lb, nub = ub, nl = l;
            for (;;) {
                if (nl < min_len || (max_occ && nub - nlb > max_occ)) break;
                if (WRITE && sub == 0 && s0 + ns < nshells) {
                    shells[s0 + ns] = MemsShell<T>{(T)nlb, (T)ilb, (T)iub, (T)nl};
                    shell_slot[s0 + ns] = p | (starts ? MEMS_STARTS : 0ull);
                    cand_start[s0 + ns] = c0 + nc;
                }
                ++ns;
                nc += (ilb - nlb) + (nub - iub);
                ilb = nlb; iub = nub; l = nl;
                const uint64_t a = mems_L<T>(LCP, ilb, n), b = mems_L<T>(LCP, iub, n);
                nl = a > b ? a : b;
                if (nl >= l || nl < min_len) break;    // (the depth falls strictly; min_len >= 1)
                if (a >= nl) {                         // (then ilb >= 1)
                    const uint64_t h = rmq_last<T>(LCP, index, Y, sub, ilb, (T)(nl - 1), n);
                    nlb = h < ilb ? h : 0;             // nothing found: L[0] is 0 whatever is stored
                }
                if (b >= nl) {                         // (then iub < n)
                    const uint64_t e = iub + 1 < n ? rmq_first<T>(LCP, index, Y, sub, iub + 1, n, (T)(nl - 1), n) : n;
                    nub = (e > iub && e <= n) ? e : n;
                }
                if (nlb == ilb && nub == iub) break;   // (no index of these values)
            }
        }
        if (sub != 0) continue;
        if (!WRITE) { shell_cnt[p] = ns; cand_cnt[p] = nc; }
        else if (p == S) cand_start[nshells] = c0;
    }
}

// rank number k of a shell
template <typename T>
__device__ __forceinline__ uint64_t mems_rank(const MemsShell<T>& sh, uint64_t k) {
    const uint64_t left = (uint64_t)sh.ilb - (uint64_t)sh.nlb;
    return k < left ? (uint64_t)sh.nlb + k : (uint64_t)sh.iub + (k - left);
}

// marks[o] = 1 iff candidate o is a MEM, for o < total; the structure of occ_expand_kernel over cand_start[0 .. nshells], whose
// entries ascend strictly (every shell has a rank) and end with total.  So a tile meets at most OCC_TILE = OCC_CHUNK shells and the chunk
// loop takes one trip; it is kept in the shape of occ_expand_kernel, where empty intervals make it take more.
template <typename T>
__global__ __launch_bounds__(256) void mems_mark_kernel(const MemsShell<T>* __restrict__ shells, const uint64_t* __restrict__ shell_slot,
                                                        const uint64_t* __restrict__ cand_start, uint64_t nshells, uint64_t total,
                                                        const uint8_t* __restrict__ bwt, const uint32_t* __restrict__ first,
                                                        const uint8_t* __restrict__ pat, uint64_t n, unsigned char* __restrict__ marks) {
    __shared__ uint64_t s_start[OCC_CHUNK + 1];
    for (uint64_t o0 = (uint64_t)blockIdx.x * OCC_TILE; o0 < total; o0 += (uint64_t)gridDim.x * OCC_TILE) {
        const uint64_t o1 = o0 + OCC_TILE < total ? o0 + OCC_TILE : total;
        uint64_t open = o0;                                                  // the first candidate not marked yet (the same in every thread)
        while (open < o1) {
            const uint64_t j0 = occ_last_le(cand_start, nshells + 1, open);  // (cand_start[nshells] = total > open, so j0 < nshells)
            if (j0 >= nshells) break;
            const uint64_t cnt = nshells - j0 < OCC_CHUNK ? nshells - j0 : OCC_CHUNK;
            __syncthreads();
            for (uint64_t i = threadIdx.x; i <= cnt; i += blockDim.x) s_start[i] = cand_start[j0 + i];
            __syncthreads();
            const uint64_t upto = s_start[cnt] < o1 ? s_start[cnt] : o1;
            if (upto <= open) break;                                         // (starts that do not ascend: not this call's scan)
            for (uint64_t o = o0 + threadIdx.x; o < upto; o += blockDim.x) {
                if (o < open) continue;
                const uint64_t i = occ_last_le(s_start, cnt, o);
                const MemsShell<T> sh = shells[j0 + i];
                const uint64_t slot = shell_slot[j0 + i];
                const uint64_t r = mems_rank<T>(sh, o - s_start[i]);
                bool keep = (slot & MEMS_STARTS) != 0;
                if (!keep && r < n) keep = mems_bit(first, r) || bwt[r] != pat[(slot & ~MEMS_STARTS) - 1];
                marks[o] = keep ? 1 : 0;
            }
            open = upto;
        }
    }
}

// The functor of select_emit_kernel: the k-th surviving candidate o gives the triple (slot, SA[r], depth of its shell)
template <typename T>
struct MemsEmit {
    const MemsShell<T>* __restrict__ shells;
    const uint64_t* __restrict__ shell_slot;
    const uint64_t* __restrict__ cand_start;
    uint64_t nshells;
    const T* __restrict__ SA;
    uint64_t n;
    uint64_t* __restrict__ qpos;
    T* __restrict__ tpos;
    T* __restrict__ len;
    __device__ __forceinline__ void operator()(uint64_t at, uint64_t o) const {
        const uint64_t j = occ_last_le(cand_start, nshells + 1, o);
        if (j >= nshells) return;
        const MemsShell<T> sh = shells[j];
        const uint64_t slot = shell_slot[j] & ~MEMS_STARTS;
        const uint64_t r = mems_rank<T>(sh, o - cand_start[j]);
        const T t = r < n ? SA[r] : (T)0;
        qpos[at] = slot;
        tpos[at] = t;
        len[at] = sh.len;
    }
    __device__ __forceinline__ void finish(uint64_t) const {}
};

// PSACX_MEMS_SUPER.  start[p] = ub - lb of a kept slot p < S, else 0, and start[S] = 0; *kept counts the kept slots.
template <typename T>
__global__ __launch_bounds__(256) void mems_super_count_kernel(const uint64_t* __restrict__ poff, uint64_t q, uint64_t S, const T* __restrict__ mlen,
                                                               const T* __restrict__ mlb, const T* __restrict__ mub, uint64_t n, uint64_t min_len,
                                                               uint64_t max_occ, uint64_t* __restrict__ start, unsigned long long* __restrict__ kept) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p0 = (uint64_t)blockIdx.x * blockDim.x; p0 <= S; p0 += stride) {
        const uint64_t p = p0 + threadIdx.x;
        uint64_t cnt = 0;
        uint64_t l = 0, lb = 0, ub = 0, room = 0;
        bool starts = false;
        if (p < S && mems_slot<T>(poff, q, mlen, mlb, mub, n, p, l, lb, ub, starts, room) && l >= min_len) {
            bool keep = starts;
            if (!keep) {                               // the left neighbour lies in the same pattern, with one byte more of room
                uint64_t before = (uint64_t)mlen[p - 1];
                if (before > room + 1) before = room + 1;
                keep = before <= l;
            }
            if (keep && (max_occ == 0 || ub - lb <= max_occ)) cnt = ub - lb;
        }
        if (p <= S) start[p] = cnt;
        const uint64_t any = __ballot(cnt != 0);
        if (lane_id() == 0 && any) atomicAdd(kept, (unsigned long long)__popcll(any));
    }
}

// qpos / tpos / len [start[p] + t] = (p, SA[lb_p + t], len_p) for t < start[p + 1] - start[p]: occ_expand_kernel with three outputs
template <typename T>
__global__ __launch_bounds__(256) void mems_super_expand_kernel(const T* __restrict__ SA, uint64_t n, const uint64_t* __restrict__ poff, uint64_t q,
                                                                uint64_t S, const T* __restrict__ mlen, const T* __restrict__ mlb,
                                                                const T* __restrict__ mub, const uint64_t* __restrict__ start, uint64_t total, uint64_t* __restrict__ qpos,
                                                                T* __restrict__ tpos, T* __restrict__ len) {
    __shared__ uint64_t s_start[OCC_CHUNK + 1];
    for (uint64_t o0 = (uint64_t)blockIdx.x * OCC_TILE; o0 < total; o0 += (uint64_t)gridDim.x * OCC_TILE) {
        const uint64_t o1 = o0 + OCC_TILE < total ? o0 + OCC_TILE : total;
        uint64_t open = o0;
        while (open < o1) {
            const uint64_t j0 = occ_last_le(start, S + 1, open);             // (start[S] = total > open, so j0 < S and slot j0 holds `open`)
            if (j0 >= S) break;
            const uint64_t cnt = S - j0 < OCC_CHUNK ? S - j0 : OCC_CHUNK;
            __syncthreads();
            for (uint64_t i = threadIdx.x; i <= cnt; i += blockDim.x) s_start[i] = start[j0 + i];
            __syncthreads();
            const uint64_t upto = s_start[cnt] < o1 ? s_start[cnt] : o1;
            if (upto <= open) break;
            for (uint64_t o = o0 + threadIdx.x; o < upto; o += blockDim.x) {
                if (o < open) continue;
                const uint64_t i = occ_last_le(s_start, cnt, o), p = j0 + i;
                uint64_t l = 0, lb = 0, ub = 0, room = 0;
                bool starts = false;
                (void)mems_slot<T>(poff, q, mlen, mlb, mub, n, p, l, lb, ub, starts, room);
                const uint64_t r = lb + (o - s_start[i]);                    // < ub_p <= n: the counts came from these entries
                const T t = r < n ? SA[r] : (T)0;
                qpos[o] = p;
                tpos[o] = t;
                len[o] = (T)l;
            }
            open = upto;
        }
    }
}

} // namespace psacx
