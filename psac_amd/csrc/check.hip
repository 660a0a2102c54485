// check.hip -- device-side verification of SA / ISA / LCP (the CLI's -c at sizes where a host
// check is impractical).  Follows check_SA (/root/reference/include/check_suffix_array.hpp:56-88:
// range, ISA[SA[i]] == i, order through the first character and the ranks of the suffixes one
// further) and d_check_sa's idea of a scalable checker (:207-267).  LCP entries are verified by
// direct character comparison, which is linear in sum(LCP): meant for texts with short repeats.
#include "engine.hpp"
#include "query_calls.hpp"
#include "nsv.hpp"     // nsv_pyramid_layout only: the suffix-tree checker below must not use the searches declared there

namespace psacx {

// err[0]: SA out of range / not inverse of ISA, err[1]: order violations, err[2]: LCP mismatches,
// err[3]: LCP[0] != 0
template <typename T>
__global__ void check_kernel(const uint8_t* __restrict__ text, uint64_t n, const T* __restrict__ SA,
                             const T* __restrict__ ISA, const T* __restrict__ LCP, unsigned long long* __restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned e0 = 0, e1 = 0, e2 = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t b = SA[i];
        if (b >= n || (uint64_t)ISA[b] != i) { ++e0; continue; }
        if (i == 0) { if (LCP && LCP[0] != 0) atomicAdd(&err[3], 1ull); continue; }
        const uint64_t a = SA[i - 1];
        if (a >= n) continue;                       // counted by the thread that owns i - 1
        const uint8_t ca = text[a], cb = text[b];
        bool ok = ca < cb;
        if (ca == cb) ok = (a + 1 == n) || (b + 1 < n && ISA[a + 1] < ISA[b + 1]);
        if (!ok) ++e1;
        if (LCP) {
            const uint64_t l = LCP[i];
            uint64_t h = 0;
            while (h < l && a + h < n && b + h < n && text[a + h] == text[b + h]) ++h;
            const bool more = (a + h < n && b + h < n && text[a + h] == text[b + h]);
            if (h != l || more) ++e2;
        }
    }
    e0 = wave_reduce<uint32_t>(e0, OpSum()); e1 = wave_reduce<uint32_t>(e1, OpSum()); e2 = wave_reduce<uint32_t>(e2, OpSum());
    if (lane_id() == 0) {
        if (e0) atomicAdd(&err[0], (unsigned long long)e0);
        if (e1) atomicAdd(&err[1], (unsigned long long)e1);
        if (e2) atomicAdd(&err[2], (unsigned long long)e2);
    }
}

template <typename T>
int check_dev(psacx_ctx* c, const uint8_t* text, uint64_t n, const T* sa, const T* isa, const T* lcp, uint64_t* errors) {
    if (!c || !text || !sa || !isa || !errors || n == 0) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(ensure_slab(c, 4096));
    unsigned long long* d = reinterpret_cast<unsigned long long*>(c->slab);
    PSACX_HIP(c, hipMemsetAsync(d, 0, 32, c->stream));
    hipLaunchKernelGGL((check_kernel<T>), dim3(grid_for(c, n, 256, 16)), dim3(256), 0, c->stream, text, n, sa, isa, lcp, d);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipMemcpyAsync(errors, d, 32, hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// ---- string sets: the generalized suffix array of psacx_construct_gsa_* (gl_check_gsa, src/gsac.cpp:85-135, gathers everything on one
// rank and tolerates swapped equal suffixes; here the arrays stay in HBM and equal suffixes must stand in text order, as the engine
// builds them).  The string ends are a bitmap of n + 1 bits, bit p = "a string starts at p, or p == n": the suffix at a ends after one
// character iff bit a + 1 is set, and the characters two suffixes can share end at the first set bit past either position.
//
// One thread per offset whose word no smaller offset shares writes that word whole (the offsets ascend, so the others of the word
// follow it directly): plain stores, no atomics.  The words without an offset were zeroed before.
__global__ void string_ends_bitmap_kernel(const uint64_t* __restrict__ off, uint64_t m, uint32_t* __restrict__ bits) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= m; t += stride) {
        const uint64_t w = off[t] >> 5;
        if (t && (off[t - 1] >> 5) == w) continue;
        uint32_t x = 0;
        for (uint64_t u = t; u <= m && (off[u] >> 5) == w; ++u) x |= 1u << (off[u] & 31);
        bits[w] = x;
    }
}

__device__ __forceinline__ bool ends_at(const uint32_t* __restrict__ bits, uint64_t p) { return (bits[p >> 5] >> (p & 31)) & 1u; }

// characters from p (< n) to the end of its string, or cap (1 <= cap <= n) if there are more: bit n is set, so the scan stays inside
// the bitmap whatever cap is
__device__ __forceinline__ uint64_t to_string_end(const uint32_t* __restrict__ bits, uint64_t n, uint64_t p, uint64_t cap) {
    uint64_t w = (p + 1) >> 5;
    const uint64_t last = min(p + cap, n) >> 5;
    uint32_t x = bits[w] & (~0u << ((p + 1) & 31));
    while (!x && w < last) x = bits[++w];
    if (!x) return cap;
    return min((w << 5) + (uint64_t)(__ffs((int)x) - 1) - p, cap);
}

// err as check_kernel; the rules are those of include/psacx.h (psacx_check_gsa_dev_*)
template <typename T>
__global__ void check_gsa_kernel(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ bits, const T* __restrict__ SA,
                                 const T* __restrict__ ISA, const T* __restrict__ LCP, unsigned long long* __restrict__ err) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned e0 = 0, e1 = 0, e2 = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t b = SA[i];
        if (b >= n || (uint64_t)ISA[b] != i) { ++e0; continue; }
        if (i == 0) { if (LCP && LCP[0] != 0) atomicAdd(&err[3], 1ull); continue; }
        const uint64_t a = SA[i - 1];
        if (a >= n) continue;                       // counted by the thread that owns i - 1
        const uint8_t ca = text[a], cb = text[b];
        bool ok = ca < cb;
        if (ca == cb) {
            const bool ea = ends_at(bits, a + 1), eb = ends_at(bits, b + 1);
            ok = ea ? (!eb || a < b) : (!eb && ISA[a + 1] < ISA[b + 1]);        // (neither ends: a + 1 < n and b + 1 < n)
        }
        if (!ok) ++e1;
        if (LCP) {
            const uint64_t l = LCP[i], cap = l < n ? l + 1 : n;
            const uint64_t room = min(to_string_end(bits, n, a, cap), to_string_end(bits, n, b, cap)), lim = min(l, room);
            uint64_t h = 0;
            while (h < lim && text[a + h] == text[b + h]) ++h;
            const bool more = h == l && room > l && text[a + h] == text[b + h];
            if (h != l || more) ++e2;
        }
    }
    e0 = wave_reduce<uint32_t>(e0, OpSum()); e1 = wave_reduce<uint32_t>(e1, OpSum()); e2 = wave_reduce<uint32_t>(e2, OpSum());
    if (lane_id() == 0) {
        if (e0) atomicAdd(&err[0], (unsigned long long)e0);
        if (e1) atomicAdd(&err[1], (unsigned long long)e1);
        if (e2) atomicAdd(&err[2], (unsigned long long)e2);
    }
}

template <typename T>
int check_gsa_dev(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* d_off, uint64_t m, const T* sa, const T* isa, const T* lcp,
                  uint64_t* errors) {
    if (!c || !text || !d_off || !sa || !isa || !errors || n == 0 || m == 0 || m > n) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(ensure_slab(c, 4096));
    unsigned long long* d = reinterpret_cast<unsigned long long*>(c->slab);
    // d[0..3]: the counters, d[4]: malformed offsets (a set that does not cover [0, n) with non-empty strings would send the
    // bitmap's stores out of bounds)
    PSACX_HIP(c, hipMemsetAsync(d, 0, 40, c->stream));
    hipLaunchKernelGGL(check_offsets_kernel<0>, dim3(grid_for(c, m + 1, 256, 8)), dim3(256), 0, c->stream, d_off, m, n, d + 4);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long bad = 0;
    PSACX_HIP(c, hipMemcpyAsync(&bad, d + 4, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (bad) return PSACX_EINVAL;
    const uint64_t words = (n >> 5) + 1;
    uint32_t* bits = nullptr;
    hipError_t e = hipMalloc((void**)&bits, words * sizeof(uint32_t));
    if (e != hipSuccess) { c->hip_err = std::string("hipMalloc(string ends): ") + hipGetErrorString(e); (void)hipGetLastError(); return PSACX_ENOMEM; }
    int rc = PSACX_OK;
    auto step = [&](hipError_t r) { if (rc == PSACX_OK && r != hipSuccess) { c->hip_err = hipGetErrorString(r); (void)hipGetLastError(); rc = PSACX_EHIP; } };
    step(hipMemsetAsync(bits, 0, words * sizeof(uint32_t), c->stream));
    if (rc == PSACX_OK) {
        hipLaunchKernelGGL(string_ends_bitmap_kernel, dim3(grid_for(c, m + 1, 256, 8)), dim3(256), 0, c->stream, d_off, m, bits);
        step(hipGetLastError());
    }
    if (rc == PSACX_OK) {
        hipLaunchKernelGGL((check_gsa_kernel<T>), dim3(grid_for(c, n, 256, 16)), dim3(256), 0, c->stream, text, n, (const uint32_t*)bits, sa, isa, lcp, d);
        step(hipGetLastError());
    }
    if (rc == PSACX_OK) step(hipMemcpyAsync(errors, d, 32, hipMemcpyDeviceToHost, c->stream));
    step(hipStreamSynchronize(c->stream));
    (void)hipFree(bits);
    return rc;
}

// The two steps of check_gsa_dev for the callers that keep the bitmap in their own workspace (the suffix tree of a string set, here and
// in ansv.hip).  PSACX_EINVAL unless the m + 1 offsets start at 0, end at n and ascend strictly; uses the first bytes of the slab and waits.
int string_offsets_valid_dev(psacx_ctx* c, const uint64_t* d_off, uint64_t m, uint64_t n) {
    PSACX_TRY(ensure_slab(c, 4096));
    unsigned long long* d = reinterpret_cast<unsigned long long*>(c->slab);
    PSACX_HIP(c, hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(check_offsets_kernel<0>, dim3(grid_for(c, m + 1, 256, 8)), dim3(256), 0, c->stream, d_off, m, n, d);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long bad = 0;
    PSACX_HIP(c, hipMemcpyAsync(&bad, d, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return bad ? PSACX_EINVAL : PSACX_OK;
}

// bits[(n >> 5) + 1] = the bitmap of the string ends of VALID offsets, queued on the ctx stream
int string_ends_bitmap_dev(psacx_ctx* c, const uint64_t* d_off, uint64_t m, uint64_t n, uint32_t* bits) {
    PSACX_HIP(c, hipMemsetAsync(bits, 0, ((n >> 5) + 1) * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(string_ends_bitmap_kernel, dim3(grid_for(c, m + 1, 256, 8)), dim3(256), 0, c->stream, d_off, m, bits);
    PSACX_HIP(c, hipGetLastError());
    return PSACX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Suffix-tree node table: is `nodes` the table of text / SA / LCP as given?  The rules are those of include/psacx.h
// (psacx_check_suffix_tree_dev_*): head(), the leaf and the internal records are restated there without ANSV, and nothing
// here is shared with the builder (ansv.hip) but the min-pyramid's shape.  L = LCP with L[0] read as 0: st_at() does that
// on level 0, and entry 0 of every level above -- the minimum of a group that holds L[0] -- is set to 0 after the build.
//
// One wave takes 64 consecutive entries with one coalesced load.  Lane k learns which lanes hold a value < / <= its own
// (64 broadcasts, two ballots each); every search that ends inside the group is then bit arithmetic on those two masks.  Only
// a search that leaves the group walks the pyramid, and the whole wave walks with it: one coalesced load and one ballot per level
// (st_walk; one thread on its own took a load per entry, and the checker spent most of its time waiting for those).
// ---------------------------------------------------------------------------------------------------------------
constexpr uint64_t ST_NONE = ~0ull;

template <typename T>
__device__ __forceinline__ T st_at(const Pyramid<T>& P, int L, uint64_t idx) { return (L == 0 && idx == 0) ? (T)0 : P.lvl[L][idx]; }

template <typename T>
__global__ void st_first_is_zero_kernel(Pyramid<T> P) {
    const int L = 1 + (int)threadIdx.x;
    if (L < P.nlev) P.lvl[L][0] = 0;
}

// Deliberately NOT nsv_search_wave (nsv.hpp), which it resembles: the checker's verdict must not rest on the code the builder's
// ANSV uses, so the walk is written a second time here (with L[0] read as 0, the direction a run-time argument and a way to skip the
// group already searched).  Do not merge.
// All 64 lanes work on ONE search, its arguments wave-uniform: nearest j < pos (left) or j > pos with L[j] < v (strict) or
// L[j] <= v; ST_NONE if there is none.  One step looks at a whole 64-entry group with one coalesced load and one ballot.
// skip: the caller has already looked through the level-0 group of pos.
template <typename T>
__device__ uint64_t st_walk_one(const Pyramid<T>& P, uint64_t pos, T v, bool strict, bool skip, bool left) {
    const unsigned lane = lane_id();
    uint64_t p = pos, j = 0;
    int L = 0;
    if (skip) {
        if (P.nlev < 2) return ST_NONE;              // one group is the whole array
        p >>= 6; L = 1;
    }
    for (;;) {                                      // upwards: the rest of p's group on every level
        const uint64_t len = P.len[L], g0 = p & ~63ull, idx = g0 + lane;
        const bool inr = idx < len && (left ? idx < p : idx > p);
        const T x = inr ? st_at(P, L, idx) : (T)0;
        const uint64_t m = __ballot(inr && (strict ? x < v : x <= v));
        if (m) { j = g0 + (uint64_t)(left ? 63 - __builtin_clzll(m) : __builtin_ctzll(m)); break; }
        if (left ? g0 == 0 : g0 + 64 >= len) return ST_NONE;       // (the top level is one group, so L stays below nlev)
        p >>= 6; ++L;
    }
    while (L > 0) {                                 // downwards: the nearest qualifying child, which exists because its minimum qualified
        --L;
        const uint64_t lo = j << 6, idx = lo + lane;
        const bool inr = idx < P.len[L];
        const T x = inr ? st_at(P, L, idx) : (T)0;
        const uint64_t m = __ballot(inr && (strict ? x < v : x <= v));
        j = m ? lo + (uint64_t)(left ? 63 - __builtin_clzll(m) : __builtin_ctzll(m)) : lo;
    }
    return j;
}

// The searches of the lanes that `want` one, one after the other, each by the whole wave; the others get ST_NONE.  Every lane of the
// wave must call this (the arguments of a lane that wants nothing are ignored).
template <typename T>
__device__ uint64_t st_walk(const Pyramid<T>& P, bool want, uint64_t pos, T v, bool strict, bool skip, bool left) {
    uint64_t res = ST_NONE;
    for (uint64_t pending = __ballot(want); pending; pending &= pending - 1) {
        const int src = __builtin_ctzll(pending);
        const uint64_t r = st_walk_one<T>(P, shfl<uint64_t>(pos, src), shfl<T>(v, src), strict, skip, left);
        if ((int)lane_id() == src) res = r;
    }
    return res;
}

__device__ __forceinline__ uint64_t st_cell(const uint8_t* __restrict__ text, uint64_t n, const CodeTable& tab, uint64_t s, uint64_t d) {
    return (s < n && d < n - s) ? (uint64_t)tab.c[text[s + d]] : 0;
}

// The table of a string set (psacx_check_suffix_tree_gsa_dev_*): 0 where the string of the suffix at s has ended d characters on
// (bits as above), and nothing is read unless s < n and s + d < n
__device__ __forceinline__ uint64_t gst_cell(const uint8_t* __restrict__ text, uint64_t n, const uint32_t* __restrict__ bits, const CodeTable& tab,
                                             uint64_t s, uint64_t d) {
    if (s >= n || d >= n - s || (d > 0 && ends_at(bits, s + d))) return 0;
    return (uint64_t)tab.c[text[s + d]];
}

// One record of a string set's table (a row of sigma + 2 cells) against the table: through a character it is matched iff cell 1 + c
// holds its id; through the $ iff cells 0 and 1 hold a range lo <= id <= hi with lo != 0, and it then accounts for either cell that
// holds its very id.  acc: the nonzero cells the matched records account for.
__device__ __forceinline__ void gst_match(const unsigned long long* __restrict__ cells, uint64_t c, uint64_t id, unsigned& hit, unsigned& acc) {
    if (c) { if (cells[1 + c] == id) { ++hit; ++acc; } return; }
    const uint64_t lo = cells[0], hi = cells[1];
    if (lo != 0 && lo <= id && id <= hi) { ++hit; acc += (unsigned)(id == lo) + (unsigned)(id == hi); }
}

// cnt[0]: records, cnt[1]: records whose cell holds their id; GSA (the table of a string set, bits = its string ends): cnt[1] the
// matched records, cnt[3] the cells they account for
template <typename T, bool GSA>
__global__ __launch_bounds__(256) void st_check_kernel(Pyramid<T> P, uint64_t n, const T* __restrict__ SA, const uint8_t* __restrict__ text,
                                                       CodeTable tab, uint64_t row, const unsigned long long* __restrict__ nodes,
                                                       unsigned long long* __restrict__ cnt, const uint32_t* __restrict__ bits) {
    const uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) / WAVE;
    const unsigned lane = lane_id();
    const uint64_t ngroups = (n + 63) >> 6;
    const uint64_t below = (1ull << lane) - 1ull;
    unsigned rec = 0, hit = 0, acc = 0;
    for (uint64_t g = wave_id; g < ngroups; g += nwaves) {
        const uint64_t base = g << 6, i = base + lane;
        const bool in = i < n;
        const T v = in ? st_at(P, 0, i) : (T)0;
        uint64_t lt = 0, le = 0;                     // the lanes of this group whose value is < / <= this lane's
        for (int k = 0; k < WAVE; ++k) {
            const T vk = shfl<T>(v, k);
            const uint64_t a = __ballot(in && v < vk), b = __ballot(in && v <= vk);
            if (lane == (unsigned)k) { lt = a; le = b; }
        }
        T nxt = shfl<T>(v, (int)((lane + 1) & 63u));  // L[i + 1]
        if (lane == 63 && i + 1 < n) nxt = P.lvl[0][i + 1];
        // l = the nearest smaller value on the left (v > 0: it exists, L[0] reads as 0), head = head(i): inside the group from the
        // masks, else by the wave (every st_walk below is called by all 64 lanes)
        uint64_t l = ST_NONE, head = 0;
        int l_lane = -1;
        const bool pos_v = in && v > 0;
        const uint64_t ml = lt & below;
        if (pos_v && ml) {
            l_lane = 63 - __builtin_clzll(ml);
            l = base + (uint64_t)l_lane;
            head = base + (uint64_t)__builtin_ctzll(le & (~0ull << (l_lane + 1)));      // (never empty: this lane's own bit is in le)
        }
        const bool far_l = pos_v && !ml;
        {
            const uint64_t wl = st_walk<T>(P, far_l, i, v, true, true, true);
            const uint64_t wh = st_walk<T>(P, far_l && wl != ST_NONE, wl, v, false, false, false);
            if (far_l) { l = wl; head = wh == ST_NONE || wh > i ? i : wh; }
        }
        const uint64_t head_of_l = shfl<uint64_t>(head, l_lane < 0 ? 0 : l_lane);          // head(l) where l is in the group
        // ---- the internal node i: r, and head(l) where l lies outside the group
        const bool node = in && i != 0 && v > 0 && head == i && l != ST_NONE;
        const T lv = node ? st_at(P, 0, l) : (T)0;
        const uint64_t mr = lane == 63 ? 0ull : lt & (~0ull << (lane + 1));
        uint64_t r = node && mr ? base + (uint64_t)__builtin_ctzll(mr) : ST_NONE;
        {
            const uint64_t wr = st_walk<T>(P, node && !mr, i, v, true, true, false);
            if (node && !mr) r = wr;
        }
        const T rv = r != ST_NONE ? st_at(P, 0, r) : (T)0;
        const bool by_r = node && r != ST_NONE && rv > lv;
        uint64_t hl = l_lane >= 0 ? head_of_l : 0;                                          // head(l); 0 where L[l] == 0
        {
            const bool far_h = node && !by_r && l_lane < 0 && lv > 0;
            const uint64_t s = st_walk<T>(P, far_h, l, lv, true, false, true);
            const uint64_t h = st_walk<T>(P, far_h && s != ST_NONE, s, lv, false, false, false);
            if (far_h) hl = s == ST_NONE ? 0 : (h == ST_NONE || h > l ? l : h);              // (l itself qualifies)
        }
        if (!in) continue;
        const uint64_t sa = SA[i];
        // ---- the leaf n + i
        {
            uint64_t p = head, d = v;
            if (i + 1 < n && nxt > v) { p = i + 1; d = nxt; }
            ++rec;
            if (GSA) gst_match(nodes + p * row, gst_cell(text, n, bits, tab, sa, d), n + i, hit, acc);
            else if (nodes[p * row + st_cell(text, n, tab, sa, d)] == n + i) ++hit;
        }
        if (!node) continue;
        const uint64_t p = by_r ? r : hl, d = by_r ? (uint64_t)rv : (uint64_t)lv;
        ++rec;
        if (GSA) gst_match(nodes + p * row, gst_cell(text, n, bits, tab, sa, d), i, hit, acc);
        else if (nodes[p * row + st_cell(text, n, tab, sa, d)] == i) ++hit;
    }
    rec = wave_reduce<uint32_t>(rec, OpSum()); hit = wave_reduce<uint32_t>(hit, OpSum());
    if (GSA) acc = wave_reduce<uint32_t>(acc, OpSum());
    if (lane == 0) {
        if (rec) atomicAdd(&cnt[0], (unsigned long long)rec);
        if (hit) atomicAdd(&cnt[1], (unsigned long long)hit);
        if (GSA && acc) atomicAdd(&cnt[3], (unsigned long long)acc);
    }
}

// one streaming pass: how many of the m words are not zero (16 bytes per load where the table is aligned for it)
__global__ void count_nonzero_kernel(const unsigned long long* __restrict__ a, uint64_t m, unsigned long long* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t pairs = (reinterpret_cast<uintptr_t>(a) & 15u) == 0 ? m / 2 : 0;
    const ulonglong2* a2 = reinterpret_cast<const ulonglong2*>(a);
    unsigned c = 0;
    for (uint64_t i = t; i < pairs; i += stride) { const ulonglong2 w = a2[i]; c += (w.x != 0) + (w.y != 0); }
    for (uint64_t i = pairs * 2 + t; i < m; i += stride) c += a[i] != 0;
    c = wave_reduce<uint32_t>(c, OpSum());
    if (lane_id() == 0 && c) atomicAdd(out, (unsigned long long)c);
}

template <typename T>
int check_suffix_tree_dev(psacx_ctx* c, const uint8_t* text, uint64_t n, const T* sa, const T* lcp, const uint64_t* nodes, uint64_t* out) {
    if (!c || !text || !sa || !lcp || !nodes || !out || n == 0) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    Pyramid<T> P;
    unsigned long long* d = nullptr;                 // 256 character counts, then records / matched / nonzero cells
    auto layout = [&](Arena& a) {
        d = a.take<unsigned long long>(256 + 4);
        nsv_pyramid_layout<T>(a, lcp, n, P);
    };
    PSACX_TRY(slab_layout(c, layout));
    CodeTable tab;
    uint32_t sigma = 0;
    PSACX_TRY(tree_alphabet_dev(c, text, n, d, tab, sigma));
    const uint64_t row = (uint64_t)sigma + 1;
    unsigned long long* cnt = d + 256;
    PSACX_HIP(c, hipMemsetAsync(cnt, 0, 4 * sizeof(unsigned long long), c->stream));
    for (int L = 1; L < P.nlev; ++L) {
        hipLaunchKernelGGL((pyramid_level_kernel<T>), dim3(grid_for(c, P.len[L] * 64, 256, 8)), dim3(256), 0, c->stream,
                           P.lvl[L - 1], P.len[L - 1], P.lvl[L], P.len[L]);
        PSACX_HIP(c, hipGetLastError());
    }
    if (P.nlev > 1) {
        hipLaunchKernelGGL((st_first_is_zero_kernel<T>), dim3(1), dim3(64), 0, c->stream, P);
        PSACX_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL((st_check_kernel<T, false>), dim3(grid_for(c, n, 256, 16)), dim3(256), 0, c->stream, P, n, sa, text, tab, row,
                       reinterpret_cast<const unsigned long long*>(nodes), cnt, (const uint32_t*)nullptr);
    PSACX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(count_nonzero_kernel, dim3(grid_for(c, n * row / 2 + 1, 256, 16)), dim3(256), 0, c->stream,
                       reinterpret_cast<const unsigned long long*>(nodes), n * row, cnt + 2);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    PSACX_HIP(c, hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = h[0] - h[1]; out[1] = h[2] - h[1]; out[2] = h[0]; out[3] = h[2];
    return PSACX_OK;
}

// The same for the table of a string set: check_suffix_tree_dev with the bitmap of the string ends beside the pyramid in the slab.
template <typename T>
int check_suffix_tree_gsa_dev(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* d_off, uint64_t m, const T* sa, const T* lcp,
                              const uint64_t* nodes, uint64_t* out) {
    if (!c || !text || !d_off || !sa || !lcp || !nodes || !out || n == 0 || m == 0 || m > n) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    PSACX_TRY(string_offsets_valid_dev(c, d_off, m, n));
    Pyramid<T> P;
    unsigned long long* d = nullptr;                 // 256 character counts, then records / matched / nonzero cells / cells accounted for
    uint32_t* bits = nullptr;
    auto layout = [&](Arena& a) {
        d = a.take<unsigned long long>(256 + 4);
        bits = a.take<uint32_t>((n >> 5) + 1);
        nsv_pyramid_layout<T>(a, lcp, n, P);
    };
    PSACX_TRY(slab_layout(c, layout));
    CodeTable tab;
    uint32_t sigma = 0;
    PSACX_TRY(tree_alphabet_dev(c, text, n, d, tab, sigma));
    const uint64_t row = (uint64_t)sigma + 2;
    unsigned long long* cnt = d + 256;
    PSACX_HIP(c, hipMemsetAsync(cnt, 0, 4 * sizeof(unsigned long long), c->stream));
    PSACX_TRY(string_ends_bitmap_dev(c, d_off, m, n, bits));
    for (int L = 1; L < P.nlev; ++L) {
        hipLaunchKernelGGL((pyramid_level_kernel<T>), dim3(grid_for(c, P.len[L] * 64, 256, 8)), dim3(256), 0, c->stream,
                           P.lvl[L - 1], P.len[L - 1], P.lvl[L], P.len[L]);
        PSACX_HIP(c, hipGetLastError());
    }
    if (P.nlev > 1) {
        hipLaunchKernelGGL((st_first_is_zero_kernel<T>), dim3(1), dim3(64), 0, c->stream, P);
        PSACX_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL((st_check_kernel<T, true>), dim3(grid_for(c, n, 256, 16)), dim3(256), 0, c->stream, P, n, sa, text, tab, row,
                       reinterpret_cast<const unsigned long long*>(nodes), cnt, (const uint32_t*)bits);
    PSACX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(count_nonzero_kernel, dim3(grid_for(c, n * row / 2 + 1, 256, 16)), dim3(256), 0, c->stream,
                       reinterpret_cast<const unsigned long long*>(nodes), n * row, cnt + 2);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long h[4] = {0, 0, 0, 0};
    PSACX_HIP(c, hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = h[0] - h[1]; out[1] = h[2] - h[3]; out[2] = h[0]; out[3] = h[2];
    return PSACX_OK;
}

// Synthetic benchmark texts of SURVEY.md section 8(d), generated where they are used: character g of
// DNA(n, seed) is "ACGT"[z & 3], of ASCII128(n, seed) z & 127, with z the g-th output (counting from 1) of
// splitmix64 started at `seed`; TANDEM repeats the first `period` characters of DNA(period, seed); MUTATED is that repeat with one
// position in 200 (chosen by a second stream over the absolute position) given a character of its own: repeated reads with mutations.
// tests/inputs.py defines the same streams on the host.
__device__ __forceinline__ uint64_t splitmix64_at(uint64_t seed, uint64_t g) {
    uint64_t z = seed + (g + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void synth_text_kernel(uint8_t* __restrict__ out, uint64_t n, uint64_t first, int kind, uint64_t seed, uint64_t period) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 16;
    for (uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; i0 < n; i0 += stride) {
        uint8_t b[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            uint64_t g = first + i0 + j;
            const uint64_t g_abs = g;
            if (kind == 2 || kind == 3) g %= period;
            uint64_t z = splitmix64_at(seed, g);
            if (kind == 3) {           // one position in 200 carries its own character instead of the repeat's
                const uint64_t m = splitmix64_at(seed ^ 0xA5A5A5A5A5A5A5A5ull, g_abs);
                if (m % 200 == 0) z = m >> 8;
            }
            b[j] = kind == 1 ? (uint8_t)(z & 127) : (uint8_t)"ACGT"[z & 3];
        }
        if (i0 + 16 <= n && ((uintptr_t)(out + i0) & 15) == 0) {
            uint4 v;
            v.x = b[0] | (b[1] << 8) | (b[2] << 16) | ((unsigned)b[3] << 24);
            v.y = b[4] | (b[5] << 8) | (b[6] << 16) | ((unsigned)b[7] << 24);
            v.z = b[8] | (b[9] << 8) | (b[10] << 16) | ((unsigned)b[11] << 24);
            v.w = b[12] | (b[13] << 8) | (b[14] << 16) | ((unsigned)b[15] << 24);
            *reinterpret_cast<uint4*>(out + i0) = v;
        } else {
            for (int j = 0; j < 16 && i0 + j < n; ++j) out[i0 + j] = b[j];
        }
    }
}

int synth_text_dev(psacx_ctx* c, uint8_t* d_text, uint64_t n, uint64_t first, int kind, uint64_t seed, uint64_t period) {
    if (!c || !d_text || kind < 0 || kind > 3 || (kind >= 2 && period == 0)) return PSACX_EINVAL;
    if (n == 0) return PSACX_OK;
    PSACX_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(synth_text_kernel, dim3(grid_for(c, n / 16 + 1, 256, 16)), dim3(256), 0, c->stream, d_text, n, first, kind, seed, period);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

int check_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, const uint32_t* isa, const uint32_t* lcp, uint64_t* e) {
    return check_dev<uint32_t>(c, t, n, sa, isa, lcp, e);
}
int check_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, const uint64_t* isa, const uint64_t* lcp, uint64_t* e) {
    return check_dev<uint64_t>(c, t, n, sa, isa, lcp, e);
}

int check_suffix_tree_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, const uint32_t* lcp, const uint64_t* nodes, uint64_t* o) {
    return check_suffix_tree_dev<uint32_t>(c, t, n, sa, lcp, nodes, o);
}
int check_suffix_tree_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, const uint64_t* lcp, const uint64_t* nodes, uint64_t* o) {
    return check_suffix_tree_dev<uint64_t>(c, t, n, sa, lcp, nodes, o);
}

int check_suffix_tree_gsa_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* sa, const uint32_t* lcp,
                                  const uint64_t* nodes, uint64_t* o) { return check_suffix_tree_gsa_dev<uint32_t>(c, t, n, off, m, sa, lcp, nodes, o); }
int check_suffix_tree_gsa_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* sa, const uint64_t* lcp,
                                  const uint64_t* nodes, uint64_t* o) { return check_suffix_tree_gsa_dev<uint64_t>(c, t, n, off, m, sa, lcp, nodes, o); }

int check_gsa_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* sa, const uint32_t* isa,
                      const uint32_t* lcp, uint64_t* e) { return check_gsa_dev<uint32_t>(c, t, n, off, m, sa, isa, lcp, e); }
int check_gsa_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* sa, const uint64_t* isa,
                      const uint64_t* lcp, uint64_t* e) { return check_gsa_dev<uint64_t>(c, t, n, off, m, sa, isa, lcp, e); }

} // namespace psacx
