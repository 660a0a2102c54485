// repeats.hpp -- the Burrows-Wheeler transform of a text or a string set from SA, and its right-maximal, maximal and supermaximal
// repeats from LCP, the range-minimum index of LCP, the BWT and the bitmap of the ranks that start a string, all resident in HBM
// (include/psacx.h: "BWT and repeats").  The reference has no counterpart; kernels only, the calls are in repeats.hip.
//
// BWT.  bwt_kernel: one rank per lane, a wave owns 64 consecutive ranks.  One SA entry (streamed), one gathered byte.  The bit "this
// rank starts a string" goes through one ballot per wave; lanes 0 and 1 store its halves as two 32-bit words.  The few ranks that
// start a string of a set need the end of that string: the wave takes them one after another and scans the bitmap of the string
// ends 64 words at a time.
//
// Directories.  Three bit arrays over the ranks, 64 ranks per word, built by one ballot per wave as above, each with the number of
// its bits per word, which the scan of scan.hpp turns into "bits in front of this word":
//     D[x]  = first[x] | first[x-1] | bwt[x] != bwt[x-1]        (1 <= x < n)       bwt_change_kernel
//     F[x]  = first[x]                                           (x < n)            (the same kernel: the caller's bitmap, cut at n)
//     St[x] = L[x] != L[x-1], L[0] = 0                            (1 <= x < n)       lcp_step_kernel
// rank_bits(x) = dir[x >> 6] + popcount(word[x >> 6] below bit x & 63): one directory entry and one word; a count over [a, b) is two.
//
// Enumeration.  repeats_kernel<T, KIND>: RMQ_LANES = 16 lanes per rank j, as lpf_kernel.  l = L[j]; h = rmq_last(j, l) is the
// previous value <= l; j is the head of its interval iff L[h] < l.  Most ranks end there.  A head asks rmq_first for the next value
// below l, applies the filters, and then the tests of its kind from the directories.  The supermaximal kind then goes through the
// bwt bytes of its interval: every lane keeps a set of 256 bits in eight registers (no array is indexed at run time), tests its own
// bytes against it, and the sixteen sets are merged by xor-shuffles, where two sets that share a bit are a collision.  Lane 0 stores
// one select byte per rank and the interval of a selected head at slot j.
//
// Compaction.  The select bytes go through select.hpp in tiles of REP_TILE ranks: counts per tile, their scan (the last entry is z),
// and the functor RepeatsEmit writes lb, ub and L[j] in the order of j.
#pragma once
#include "rmq.hpp"
#include "select.hpp"

namespace psacx {

constexpr int REP_TILE = 1024;                         // ranks of a tile of the compaction (select.hpp: 4 per thread)
constexpr unsigned REP_MAX_DISTINCT = 256;             // byte values: an interval with more ranks that do not start a string repeats one

enum { REPEATS_RIGHT = 0, REPEATS_MAXIMAL = 1, REPEATS_SUPERMAXIMAL = 2 };

// bit p of a bitmap of 32-bit words
__device__ __forceinline__ bool rep_bit(const uint32_t* __restrict__ bits, uint64_t p) { return (bits[p >> 5] >> (p & 31)) & 1u; }

// lanes 0 and 1 store the ballot of the wave that owns ranks [64 w, 64 w + 64) as the 32-bit words 2 w and 2 w + 1 of `bits`
// (words at and beyond `words` do not exist); lane 0 also stores its number of bits where counts are kept
__device__ __forceinline__ void rep_store_ballot(uint64_t ballot, uint64_t w, uint32_t* __restrict__ bits, uint64_t words,
                                                 uint64_t* __restrict__ counts) {
    const unsigned lane = lane_id();
    if (lane < 2 && 2 * w + lane < words) bits[2 * w + lane] = (uint32_t)(ballot >> (32 * lane));
    if (counts && lane == 0) counts[w] = (uint64_t)__popcll(ballot);
}

// the end of the string that holds position p < n: the smallest set bit above p of the bitmap of the string ends, at most n.
// The 64 lanes of a wave scan 64 words per step (all of them call this with the same p).
__device__ __forceinline__ uint64_t rep_string_end(const uint32_t* __restrict__ ends, uint64_t p, uint64_t n) {
    const unsigned lane = lane_id();
    const uint64_t from = p + 1, last = n >> 5;         // bit n lies in word `last`, the last one of the bitmap
    for (uint64_t w0 = from >> 5; w0 <= last; w0 += WAVE) {
        const uint64_t w = w0 + lane;
        uint32_t word = w <= last ? ends[w] : 0u;
        if (w == (from >> 5)) word &= ~0u << (from & 31);
        const uint64_t any = __ballot(word != 0);
        if (any) {
            const int src = __builtin_ctzll(any);
            const uint64_t e = ((w0 + src) << 5) + (uint64_t)(__ffs((int)shfl<uint32_t>(word, src)) - 1);
            return e < n ? e : n;
        }
    }
    return n;
}

// bwt[r] = S[SA[r] - 1], or the last byte of its string where SA[r] starts one; first: the bitmap of those ranks, (n >> 5) + 1 words;
// primary: the rank of position 0 (the call has set it to all ones).  ends == nullptr: one text.  Any output may be nullptr.
template <typename T>
__global__ __launch_bounds__(256) void bwt_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ ends,
                                                  const T* __restrict__ SA, uint8_t* __restrict__ bwt, uint32_t* __restrict__ first,
                                                  uint64_t* __restrict__ primary) {
    const unsigned lane = lane_id();
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
    const uint64_t chunks = (n >> 6) + 1, words = (n >> 5) + 1;
    for (uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; w < chunks; w += nwaves) {
        const uint64_t r = (w << 6) + lane;
        const uint64_t s = r < n ? (uint64_t)SA[r] : n;
        const bool in = s < n;                          // (an SA entry >= n: byte 0, bit clear)
        const bool start = in && (ends ? rep_bit(ends, s) : s == 0);
        uint8_t b = 0;
        if (in && !start) b = text[s - 1];
        if (bwt) {
            if (ends) {
                uint64_t todo = __ballot(start);
                while (todo) {                          // one string start after another, the whole wave on each
                    const int src = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const uint64_t e = rep_string_end(ends, shfl<uint64_t>(s, src), n);      // in (s, n]
                    if (lane == (unsigned)src) b = text[e - 1];
                }
            } else if (start) b = text[n - 1];
            if (r < n) bwt[r] = b;
        }
        if (first) rep_store_ballot(__ballot(start), w, first, words, nullptr);
        if (primary && in && s == 0) *primary = r;
    }
}

// D and F of the header comment: two 32-bit words and one count per 64 ranks each.  `first` is the caller's bitmap, read inside its
// (n >> 5) + 1 words and below bit n only.  dbits / fbits hold 2 * chunks words, dcnt / fcnt chunks entries, chunks = (n >> 6) + 1.
__global__ __launch_bounds__(256) void bwt_change_kernel(uint64_t n, const uint8_t* __restrict__ bwt, const uint32_t* __restrict__ first,
                                                         uint32_t* __restrict__ dbits, uint64_t* __restrict__ dcnt,
                                                         uint32_t* __restrict__ fbits, uint64_t* __restrict__ fcnt) {
    const unsigned lane = lane_id();
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
    const uint64_t chunks = (n >> 6) + 1;
    for (uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; w < chunks; w += nwaves) {
        const uint64_t x = (w << 6) + lane;
        bool f = false, d = false;
        if (x < n) {
            f = rep_bit(first, x);
            if (x >= 1) d = f || rep_bit(first, x - 1) || bwt[x] != bwt[x - 1];
        }
        rep_store_ballot(__ballot(d), w, dbits, 2 * chunks, dcnt);
        rep_store_ballot(__ballot(f), w, fbits, 2 * chunks, fcnt);
    }
}

// St of the header comment
template <typename T>
__global__ __launch_bounds__(256) void lcp_step_kernel(uint64_t n, const T* __restrict__ LCP, uint32_t* __restrict__ sbits,
                                                       uint64_t* __restrict__ scnt) {
    const unsigned lane = lane_id();
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
    const uint64_t chunks = (n >> 6) + 1;
    for (uint64_t w = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; w < chunks; w += nwaves) {
        const uint64_t x = (w << 6) + lane;
        bool st = false;
        if (x >= 1 && x < n) st = LCP[x] != (x == 1 ? (T)0 : LCP[x - 1]);
        rep_store_ballot(__ballot(st), w, sbits, 2 * chunks, scnt);
    }
}

// A bitmap of 64-bit words with its directory: dir[w] = the bits of the words in front of word w.  Positions up to n.
struct RankDir {
    const uint64_t* __restrict__ bits;
    const uint64_t* __restrict__ dir;
};

__device__ __forceinline__ uint64_t rank_bits(const RankDir& R, uint64_t x) {
    const uint64_t w = x >> 6;
    return R.dir[w] + (uint64_t)__popcll(R.bits[w] & ((1ull << (x & 63)) - 1ull));
}

// the set bits in [a, b); 0 for an empty range
__device__ __forceinline__ uint64_t count_bits(const RankDir& R, uint64_t a, uint64_t b) {
    if (a >= b) return 0;
    const uint64_t ra = rank_bits(R, a), rb = rank_bits(R, b);
    return rb > ra ? rb - ra : 0;
}

// byte b into the set m[8] of 256 bits; true if it was there.  Unrolled with guards: m stays in registers.
__device__ __forceinline__ bool rep_set_add(uint32_t (&m)[8], unsigned b) {
    const uint32_t bit = 1u << (b & 31);
    bool hit = false;
#pragma unroll
    for (unsigned k = 0; k < 8; ++k) {
        if ((b >> 5) == k) { hit = (m[k] & bit) != 0; m[k] |= bit; }
    }
    return hit;
}

// are the bwt bytes of the ranks of [lb, ub) that do not start a string pairwise different?  The 16 lanes of a group call this
// together.  One rank per lane and turn; the turns end with the first collision a lane sees in its own set, and the sets of the
// lanes are merged at the end.
__device__ __forceinline__ bool rep_bytes_distinct(const uint8_t* __restrict__ bwt, const uint64_t* __restrict__ fbits, unsigned sub, uint64_t lb,
                                                   uint64_t ub) {
    uint32_t m[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned shift = lane_id() & ~(unsigned)(RMQ_LANES - 1);
    bool coll = false;
    for (uint64_t x0 = lb; x0 < ub; x0 += RMQ_LANES) {
        const uint64_t x = x0 + sub;
        if (x < ub && !((fbits[x >> 6] >> (x & 63)) & 1ull)) coll = rep_set_add(m, bwt[x]);
        if ((__ballot(coll) >> shift) & 0xFFFFull) return false;
    }
    uint32_t both = 0;
#pragma unroll
    for (int d = 1; d < RMQ_LANES; d <<= 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t o = shfl_xor<uint32_t>(m[k], d);
            both |= m[k] & o;
            m[k] |= o;
        }
    }
    return ((__ballot(both != 0) >> shift) & 0xFFFFull) == 0;
}

// sel[j] = 1 and cand_lb[j], cand_ub[j] = the interval, for every head j that passes kind and filters; sel[j] = 0 otherwise.
// cand_lb == nullptr (the count query) stores the select bytes alone.  min_occ >= 2; max_occ == 0: no upper bound.
template <typename T, int KIND>
__global__ __launch_bounds__(256) void repeats_kernel(uint64_t n, const T* __restrict__ LCP, const T* __restrict__ index,
                                                      const uint8_t* __restrict__ bwt, RankDir D, RankDir F, RankDir St, uint64_t min_len,
                                                      uint64_t min_occ, uint64_t max_occ, unsigned char* __restrict__ sel,
                                                      T* __restrict__ cand_lb, T* __restrict__ cand_ub) {
    RmqLayout Y;
    rmq_layout(n, Y);
    const unsigned sub = threadIdx.x % RMQ_LANES;
    const uint64_t group = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / RMQ_LANES;
    const uint64_t ngroups = ((uint64_t)gridDim.x * blockDim.x) / RMQ_LANES;
    for (uint64_t j = group; j < n; j += ngroups) {
        bool take = false;
        uint64_t lb = 0, ub = n;
        const T l = j >= 1 ? LCP[j] : (T)0;            // (rank 0 is never a head)
        if (l != 0) {
            uint64_t h = rmq_last<T>(LCP, index, Y, sub, j, l, n);
            if (h >= j) h = 0;                          // nothing found: the interval starts at rank 0
            const T lh = h ? LCP[h] : (T)0;             // (L[0] is 0 whatever is stored)
            if (lh < l) {                               // a head: the interval is [h, ub)
                lb = h;
                if (j + 1 < n) ub = rmq_first<T>(LCP, index, Y, sub, j + 1, n, (T)(l - 1), n);
                if (ub <= j || ub > n) ub = n;
                const uint64_t occ = ub - lb;           // >= 2: lb < j < ub
                take = (uint64_t)l >= min_len && occ >= min_occ && (max_occ == 0 || occ <= max_occ);
                if (KIND == REPEATS_MAXIMAL) take = take && count_bits(D, lb + 1, ub) != 0;
                if (KIND == REPEATS_SUPERMAXIMAL) {
                    take = take && count_bits(St, lb + 2, ub) == 0;
                    if (take) {
                        const uint64_t starts = count_bits(F, lb, ub);
                        take = starts <= occ && occ - starts <= REP_MAX_DISTINCT;
                    }
                    if (take) take = rep_bytes_distinct(bwt, F.bits, sub, lb, ub);
                }
            }
        }
        if (sub != 0) continue;
        sel[j] = take ? 1 : 0;
        if (take && cand_lb) { cand_lb[j] = (T)lb; cand_ub[j] = (T)ub; }
    }
}

// The functor of select_emit_kernel: the k-th selected head j gives lb[k], ub[k] and, where asked for, len[k] = L[j]
// (j < n: nothing behind n is selected).
template <typename T>
struct RepeatsEmit {
    const T* __restrict__ LCP;
    const T* __restrict__ cand_lb;
    const T* __restrict__ cand_ub;
    T* __restrict__ lb;
    T* __restrict__ ub;
    T* __restrict__ len;
    __device__ __forceinline__ void operator()(uint64_t at, uint64_t j) const {
        const T l = cand_lb[j], u = cand_ub[j];         // both loads in flight before the first store (restrict does not reach a member)
        lb[at] = l;
        ub[at] = u;
        if (len) len[at] = LCP[j];
    }
    __device__ __forceinline__ void finish(uint64_t) const {}
};

} // namespace psacx
