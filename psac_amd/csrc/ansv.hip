// ansv.hip -- all nearest smaller values over an integer array (the LCP array).
//
// Stands in for ansv<T,left_type,right_type,global_indexing>() (/root/reference/include/
// ansv.hpp:2042-2051; sequential semantics ansv.hpp:48-65; tie rules ansv_common.hpp:20-22;
// caller suffix_tree.hpp:43-63 with left = furthest_eq, right = nearest_sm).
//
// The reference walks a monotone stack per rank and exchanges unmatched prefix minima.  On the
// GPU the array is cut into tiles; inside a tile every search is a binary descent over window
// minima held in registers and LDS, and the few searches that leave a tile share one walk of a
// global 64-ary min-pyramid per distinct value (ansv_tile.hpp).
#include "engine.hpp"
#include "query_calls.hpp"
#include "nsv.hpp"
#include "ansv_wave.hpp"

namespace psacx {

// type 0 nearest_sm, 1 nearest_eq, 2 furthest_eq
template <typename T, bool LEFT>
__device__ __forceinline__ uint64_t nsv_typed(const Pyramid<T>& P, uint64_t n, uint64_t i, int type) {
    const T v = P.lvl[0][i];
    if (type == 0) return nsv_search<T, LEFT>(P, i, v, true);
    const uint64_t j = nsv_search<T, LEFT>(P, i, v, false);
    if (type == 1 || j == NSV_NONE) return j;
    // furthest_eq: the far end of the run of values equal to in[j] that nothing smaller interrupts
    const T u = P.lvl[0][j];
    const uint64_t s = nsv_search<T, LEFT>(P, j, u, true);         // first strictly smaller beyond j
    if (LEFT) {
        // leftmost element <= u in (s, j]: search rightwards from s (or from before index 0)
        if (s == NSV_NONE) { if (P.lvl[0][0] <= u) return 0; return nsv_search<T, false>(P, 0, u, false); }
        return nsv_search<T, false>(P, s, u, false);
    } else {
        if (s == NSV_NONE) { if (P.lvl[0][n - 1] <= u) return n - 1; return nsv_search<T, true>(P, n - 1, u, false); }
        return nsv_search<T, true>(P, s, u, false);
    }
}

// dev: in / left / right are device pointers (results stay in HBM); otherwise host pointers, staged here
template <typename T>
int ansv_run(psacx_ctx* c, const T* in, uint64_t n, int lt, int rt, uint64_t nonsv, uint64_t* left, uint64_t* right, bool dev) {
    if (!c || !in || !left || !right || n == 0 || lt < 0 || lt > 2 || rt < 0 || rt > 2) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    Pyramid<T> P;
    T* d_in = nullptr; uint64_t *d_l = nullptr, *d_r = nullptr;
    auto layout = [&](Arena& a) {
        if (dev) { d_in = const_cast<T*>(in); d_l = left; d_r = right; }
        else { d_in = a.take<T>(n); d_l = a.take<uint64_t>(n); d_r = a.take<uint64_t>(n); }
        nsv_pyramid_layout<T>(a, d_in, n, P);
    };
    PSACX_TRY(slab_layout(c, layout));
    if (!dev) PSACX_HIP(c, hipMemcpyAsync(d_in, in, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    ProfScope* ps = new ProfScope(c, TC_TOTAL);
    for (int L = 1; L < P.nlev; ++L) {
        hipLaunchKernelGGL((pyramid_level_kernel<T>), dim3(grid_for(c, P.len[L] * 64, 256, 8)), dim3(256), 0, c->stream,
                           P.lvl[L - 1], P.len[L - 1], P.lvl[L], P.len[L]);
    }
    launch_ansv_tiles<T>(c, P, n, lt, rt, nonsv, d_l, d_r);
    delete ps;
    PSACX_HIP(c, hipGetLastError());
    if (!dev) {
        PSACX_HIP(c, hipMemcpyAsync(left, d_l, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        PSACX_HIP(c, hipMemcpyAsync(right, d_r, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->profile) prof_collect(c);
    return PSACX_OK;
}

// ---------------------------------------------------------------------------------------------
// Suffix-tree node table (/root/reference/include/suffix_tree.hpp:43-223 for_each_parent and
// :440-499 construct_suffix_tree, one rank): one row of sigma + 1 cells per LCP index (= internal
// node); cell c holds the child reached through the character with alphabet code c (0 = end of
// text).  Leaves are numbered n + i.  Parents come from the ANSV of LCP: left = furthest_eq,
// right = nearest_sm (suffix_tree.hpp:62).
// ---------------------------------------------------------------------------------------------
//
// GSA = true: the table of a string set (include/psacx.h, psacx_suffix_tree_gsa_dev_*).  The parents are the same function of LCP; a
// row has sigma + 2 cells, the character with code c leads to cell 1 + c, and a suffix whose string has ended at the parent's depth
// (bits: bit p = "a string starts at p, or p == n") is a $-leaf.  The $-leaves of a node are equal suffixes, neighbours in SA: the
// one whose left neighbour is no $-leaf of the node writes cell 0, the one whose right neighbour is none writes cell 1.

// has the string of the suffix at s ended d characters on?  Nothing is read unless s < n and s + d < n.
__device__ __forceinline__ bool gst_ended(const uint32_t* __restrict__ bits, uint64_t n, uint64_t s, uint64_t d) {
    if (s >= n || d >= n - s) return true;
    const uint64_t p = s + d;
    return d > 0 && ((bits[p >> 5] >> (p & 31)) & 1u);
}

template <typename T, bool GSA>
__global__ void st_nodes_kernel(const T* __restrict__ LCP, uint64_t n, const T* __restrict__ SA, const uint8_t* __restrict__ text,
                                CodeTable tab, uint64_t row, const uint64_t* __restrict__ lnsv, const uint64_t* __restrict__ rnsv,
                                unsigned long long* __restrict__ nodes, unsigned long long* __restrict__ edges,
                                const uint32_t* __restrict__ bits) {
    // lnsv / rnsv: ANSV of LCP with left = furthest_eq, right = nearest_sm (suffix_tree.hpp:62), NSV_NONE where none.
    // The stored LCP[0] is expected to be 0.  Where it is not, it still never serves as an index or as a depth: a left result of "none"
    // (only possible then) stands for parent 0 at depth 0, a left result of 0 is read as depth 0, and a parent at depth 0 is row 0
    // whichever zero the search stopped at (with LCP[0] = 0 the furthest equal of a zero IS entry 0, so nothing changes for valid input).
    // The table is then that of LCP[0] = 0, provided the stored value equals no other entry (an equal entry can end a furthest_eq
    // search early).
    // edges (optional): the number of records written, one atomic per wave.
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    unsigned written = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t ln = lnsv[i], rn = rnsv[i];
        const uint64_t sa = SA[i];
        const uint64_t li = LCP[i];
        const uint64_t lv = (ln != NSV_NONE && ln != 0) ? (uint64_t)LCP[ln] : 0;    // the left parent's depth and its row
        const uint64_t lp = lv != 0 ? ln : 0;
        // ---- the leaf n + i (suffix_tree.hpp:72-143)
        uint64_t parent, lcp_val;
        if (i == 0) {
            lcp_val = n > 1 ? (uint64_t)LCP[1] : 0;
            parent = lcp_val > 0 ? 1 : 0;
        } else if (i == n - 1 || li >= (uint64_t)LCP[i + 1]) {
            if (lv == li) { parent = lp; lcp_val = lv; }
            else { parent = i; lcp_val = li; }
        } else {
            parent = i + 1; lcp_val = LCP[i + 1];
        }
        uint64_t ci = sa + lcp_val;
        if (!GSA) {
            nodes[parent * row + (ci < n ? tab.c[text[ci]] : 0)] = n + i;
        } else if (!gst_ended(bits, n, sa, lcp_val)) {
            nodes[parent * row + 1 + tab.c[text[ci]]] = n + i;
        } else {
            // a $-leaf at depth lcp_val: its neighbour is one of the same node iff they share exactly lcp_val characters and it ends there too
            const bool first = i == 0 || !(li == lcp_val && gst_ended(bits, n, SA[i - 1], lcp_val));
            const bool last = i == n - 1 || !((uint64_t)LCP[i + 1] == lcp_val && gst_ended(bits, n, SA[i + 1], lcp_val));
            if (first) nodes[parent * row] = n + i;
            if (last) nodes[parent * row + 1] = n + i;
        }
        ++written;
        // ---- the internal node i (suffix_tree.hpp:146-222)
        if (i == 0 || li == 0) continue;
        if (rn == NSV_NONE) {
            if (lv == li) continue;                   // duplicate of the node further left
            parent = lp; lcp_val = lv;
        } else {
            const uint64_t rv = LCP[rn];
            if (lv >= rv) { if (lv == li) continue; parent = lp; lcp_val = lv; }
            else { parent = rn; lcp_val = rv; }
        }
        ci = sa + lcp_val;
        if (!GSA) {
            nodes[parent * row + (ci < n ? tab.c[text[ci]] : 0)] = i;
        } else if (!gst_ended(bits, n, sa, lcp_val)) {
            nodes[parent * row + 1 + tab.c[text[ci]]] = i;
        } else {
            // (no generalized suffix array has such a node: the arrays are wrong, and so will this row be)
            nodes[parent * row] = i; nodes[parent * row + 1] = i;
        }
        ++written;
    }
    if (edges) {
        written = wave_reduce<uint32_t>(written, OpSum());
        if (lane_id() == 0 && written) atomicAdd(edges, (unsigned long long)written);
    }
}

template <typename T>
int suffix_tree_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const T* sa, const T* lcp, uint64_t* nodes, uint32_t* sigma) {
    if (!c || !text || !sigma || n == 0) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    // alphabet on the host (alphabet.hpp:147-164): codes 1..sigma in byte order
    unsigned long long hist[256] = {0};
    for (uint64_t i = 0; i < n; ++i) ++hist[text[i]];
    CodeTable tab;
    tree_code_table(hist, tab, *sigma);
    if (!nodes) return PSACX_OK;                      // size query
    if (!sa || !lcp) return PSACX_EINVAL;
    const uint64_t row = (uint64_t)*sigma + 1;
    Pyramid<T> P;
    T* d_lcp = nullptr; T* d_sa = nullptr; uint8_t* d_text = nullptr; unsigned long long* d_nodes = nullptr;
    uint64_t *d_ln = nullptr, *d_rn = nullptr;
    auto layout = [&](Arena& a) {
        d_lcp = a.take<T>(n); d_sa = a.take<T>(n); d_text = a.take<uint8_t>(n); d_nodes = a.take<unsigned long long>(n * row);
        d_ln = a.take<uint64_t>(n); d_rn = a.take<uint64_t>(n);
        P.lvl[0] = d_lcp; P.len[0] = n; P.nlev = 1;
        uint64_t len = n;
        while (len > 64 && P.nlev < PYR_MAX) { len = (len + 63) / 64; P.lvl[P.nlev] = a.take<T>(len); P.len[P.nlev] = len; P.nlev++; }
    };
    PSACX_TRY(slab_layout(c, layout));
    PSACX_HIP(c, hipMemcpyAsync(d_lcp, lcp, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    PSACX_HIP(c, hipMemcpyAsync(d_sa, sa, n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    PSACX_HIP(c, hipMemcpyAsync(d_text, text, n, hipMemcpyHostToDevice, c->stream));
    PSACX_HIP(c, hipMemsetAsync(d_nodes, 0, n * row * sizeof(unsigned long long), c->stream));
    for (int L = 1; L < P.nlev; ++L) {
        hipLaunchKernelGGL((pyramid_level_kernel<T>), dim3(grid_for(c, P.len[L] * 64, 256, 8)), dim3(256), 0, c->stream,
                           P.lvl[L - 1], P.len[L - 1], P.lvl[L], P.len[L]);
        PSACX_HIP(c, hipGetLastError());
    }
    launch_ansv_tiles<T>(c, P, n, 2, 0, NSV_NONE, d_ln, d_rn);
    PSACX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL((st_nodes_kernel<T, false>), dim3(grid_for(c, n, 256, 16)), dim3(256), 0, c->stream, d_lcp, n, d_sa, d_text, tab, row,
                       d_ln, d_rn, d_nodes, (unsigned long long*)nullptr, (const uint32_t*)nullptr);
    PSACX_HIP(c, hipGetLastError());
    PSACX_HIP(c, hipMemcpyAsync(nodes, d_nodes, n * row * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    return PSACX_OK;
}

// The same over arrays resident in HBM: the alphabet from a device histogram, the ANSV results and the pyramid in the ctx slab, the
// table written where the caller wants it and counted by the kernel that writes it.  Nothing but 256 character counts and the edge
// count comes back to the host.
template <typename T>
int suffix_tree_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const T* d_sa, const T* d_lcp, uint64_t* d_nodes, uint32_t* sigma, uint64_t* edges) {
    if (!c || !d_text || !sigma || n == 0) return PSACX_EINVAL;
    if (d_nodes && (!d_sa || !d_lcp)) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    Pyramid<T> P;
    unsigned long long* d_hist = nullptr; uint64_t *d_ln = nullptr, *d_rn = nullptr;
    auto layout = [&](Arena& a) {
        d_hist = a.take<unsigned long long>(256 + 1);          // the character counts, then the edge counter
        if (!d_nodes) return;
        d_ln = a.take<uint64_t>(n); d_rn = a.take<uint64_t>(n);
        nsv_pyramid_layout<T>(a, d_lcp, n, P);
    };
    PSACX_TRY(slab_layout(c, layout));
    CodeTable tab;
    PSACX_TRY(tree_alphabet_dev(c, d_text, n, d_hist, tab, *sigma));
    if (!d_nodes) return PSACX_OK;                    // size query
    const uint64_t row = (uint64_t)*sigma + 1;
    unsigned long long* d_edges = d_hist + 256;
    PSACX_HIP(c, hipMemsetAsync(d_edges, 0, sizeof(unsigned long long), c->stream));
    PSACX_HIP(c, hipMemsetAsync(d_nodes, 0, n * row * sizeof(unsigned long long), c->stream));
    for (int L = 1; L < P.nlev; ++L) {
        hipLaunchKernelGGL((pyramid_level_kernel<T>), dim3(grid_for(c, P.len[L] * 64, 256, 8)), dim3(256), 0, c->stream,
                           P.lvl[L - 1], P.len[L - 1], P.lvl[L], P.len[L]);
        PSACX_HIP(c, hipGetLastError());
    }
    launch_ansv_tiles<T>(c, P, n, 2, 0, NSV_NONE, d_ln, d_rn);
    PSACX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL((st_nodes_kernel<T, false>), dim3(grid_for(c, n, 256, 16)), dim3(256), 0, c->stream, d_lcp, n, d_sa, d_text, tab, row,
                       d_ln, d_rn, reinterpret_cast<unsigned long long*>(d_nodes), d_edges, (const uint32_t*)nullptr);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long cnt = 0;
    PSACX_HIP(c, hipMemcpyAsync(&cnt, d_edges, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (edges) *edges = cnt;
    return PSACX_OK;
}

template <typename T>
__global__ void gst_clear_first_kernel(T* lcp) { lcp[0] = 0; }

// The table of a string set (psacx_suffix_tree_gsa_dev_*): suffix_tree_dev with the bitmap of the string ends beside the ANSV results
// in the slab.  The ANSV takes the stored LCP[0] for a value, so where it is not 0 -- psacx_construct_gsa_* always stores 0 -- the
// call works on a copy of LCP whose entry 0 is.
template <typename T>
int suffix_tree_gsa_dev(psacx_ctx* c, const uint8_t* d_text, uint64_t n, const uint64_t* d_off, uint64_t m, const T* d_sa, const T* d_lcp,
                        uint64_t* d_nodes, uint32_t* sigma, uint64_t* edges) {
    if (!c || !d_text || !sigma || n == 0) return PSACX_EINVAL;
    if (d_nodes && (!d_sa || !d_lcp || !d_off)) return PSACX_EINVAL;
    if (d_off && (m == 0 || m > n)) return PSACX_EINVAL;
    PSACX_HIP(c, hipSetDevice(c->device));
    if (d_off) PSACX_TRY(string_offsets_valid_dev(c, d_off, m, n));
    T lcp0 = 0;
    if (d_nodes) {
        PSACX_HIP(c, hipMemcpyAsync(&lcp0, d_lcp, sizeof(T), hipMemcpyDeviceToHost, c->stream));
        PSACX_HIP(c, hipStreamSynchronize(c->stream));
    }
    Pyramid<T> P;
    unsigned long long* d_hist = nullptr; uint64_t *d_ln = nullptr, *d_rn = nullptr; uint32_t* bits = nullptr; T* lcp_copy = nullptr;
    auto layout = [&](Arena& a) {
        d_hist = a.take<unsigned long long>(256 + 1);          // the character counts, then the edge counter
        if (!d_nodes) return;
        bits = a.take<uint32_t>((n >> 5) + 1);
        d_ln = a.take<uint64_t>(n); d_rn = a.take<uint64_t>(n);
        if (lcp0 != 0) lcp_copy = a.take<T>(n);
        nsv_pyramid_layout<T>(a, lcp_copy ? lcp_copy : d_lcp, n, P);
    };
    PSACX_TRY(slab_layout(c, layout));
    CodeTable tab;
    PSACX_TRY(tree_alphabet_dev(c, d_text, n, d_hist, tab, *sigma));
    if (!d_nodes) return PSACX_OK;                    // size query
    const uint64_t row = (uint64_t)*sigma + 2;
    unsigned long long* d_edges = d_hist + 256;
    PSACX_HIP(c, hipMemsetAsync(d_edges, 0, sizeof(unsigned long long), c->stream));
    PSACX_HIP(c, hipMemsetAsync(d_nodes, 0, n * row * sizeof(unsigned long long), c->stream));
    PSACX_TRY(string_ends_bitmap_dev(c, d_off, m, n, bits));
    if (lcp_copy) {
        PSACX_HIP(c, hipMemcpyAsync(lcp_copy, d_lcp, n * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL((gst_clear_first_kernel<T>), dim3(1), dim3(1), 0, c->stream, lcp_copy);
        PSACX_HIP(c, hipGetLastError());
    }
    for (int L = 1; L < P.nlev; ++L) {
        hipLaunchKernelGGL((pyramid_level_kernel<T>), dim3(grid_for(c, P.len[L] * 64, 256, 8)), dim3(256), 0, c->stream,
                           P.lvl[L - 1], P.len[L - 1], P.lvl[L], P.len[L]);
        PSACX_HIP(c, hipGetLastError());
    }
    launch_ansv_tiles<T>(c, P, n, 2, 0, NSV_NONE, d_ln, d_rn);
    PSACX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL((st_nodes_kernel<T, true>), dim3(grid_for(c, n, 256, 16)), dim3(256), 0, c->stream, (const T*)P.lvl[0], n, d_sa, d_text, tab,
                       row, d_ln, d_rn, reinterpret_cast<unsigned long long*>(d_nodes), d_edges, (const uint32_t*)bits);
    PSACX_HIP(c, hipGetLastError());
    unsigned long long cnt = 0;
    PSACX_HIP(c, hipMemcpyAsync(&cnt, d_edges, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if (edges) *edges = cnt;
    return PSACX_OK;
}

// The host-pointer form: the arrays are staged in device memory of their own (the slab belongs to the call above) and the table comes back.
template <typename T>
int suffix_tree_gsa_host(psacx_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* off, uint64_t m, const T* sa, const T* lcp,
                         uint64_t* nodes, uint32_t* sigma) {
    if (!c || !text || !sigma || n == 0) return PSACX_EINVAL;
    if (nodes && (!sa || !lcp || !off)) return PSACX_EINVAL;
    if (off) {
        if (m == 0 || m > n || off[0] != 0 || off[m] != n) return PSACX_EINVAL;
        for (uint64_t t = 1; t <= m; ++t) if (off[t] <= off[t - 1]) return PSACX_EINVAL;
    }
    PSACX_HIP(c, hipSetDevice(c->device));
    unsigned long long hist[256] = {0};
    for (uint64_t i = 0; i < n; ++i) ++hist[text[i]];
    CodeTable tab;
    tree_code_table(hist, tab, *sigma);
    if (!nodes) return PSACX_OK;                      // size query
    const uint64_t row = (uint64_t)*sigma + 2;
    const size_t sizes[5] = {n, (m + 1) * sizeof(uint64_t), n * sizeof(T), n * sizeof(T), n * row * sizeof(uint64_t)};
    const void* src[4] = {text, off, sa, lcp};
    void* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = PSACX_OK;
    for (int k = 0; k < 5 && rc == PSACX_OK; ++k) {
        const hipError_t e = hipMalloc(&d[k], sizes[k]);
        if (e != hipSuccess) { c->hip_err = std::string("hipMalloc(string set): ") + hipGetErrorString(e); (void)hipGetLastError(); rc = PSACX_ENOMEM; }
    }
    auto step = [&](hipError_t r) { if (rc == PSACX_OK && r != hipSuccess) { c->hip_err = hipGetErrorString(r); (void)hipGetLastError(); rc = PSACX_EHIP; } };
    for (int k = 0; k < 4 && rc == PSACX_OK; ++k) step(hipMemcpyAsync(d[k], src[k], sizes[k], hipMemcpyHostToDevice, c->stream));
    if (rc == PSACX_OK) {
        uint32_t sg = 0;
        rc = suffix_tree_gsa_dev<T>(c, (const uint8_t*)d[0], n, (const uint64_t*)d[1], m, (const T*)d[2], (const T*)d[3], (uint64_t*)d[4], &sg, nullptr);
    }
    if (rc == PSACX_OK) step(hipMemcpyAsync(nodes, d[4], sizes[4], hipMemcpyDeviceToHost, c->stream));
    step(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 5; ++k) if (d[k]) (void)hipFree(d[k]);
    return rc;
}

int suffix_tree_gsa_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* sa, const uint32_t* lcp,
                            uint64_t* nodes, uint32_t* sg, uint64_t* e) { return suffix_tree_gsa_dev<uint32_t>(c, t, n, off, m, sa, lcp, nodes, sg, e); }
int suffix_tree_gsa_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* sa, const uint64_t* lcp,
                            uint64_t* nodes, uint32_t* sg, uint64_t* e) { return suffix_tree_gsa_dev<uint64_t>(c, t, n, off, m, sa, lcp, nodes, sg, e); }
int suffix_tree_gsa_host_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* sa, const uint32_t* lcp,
                             uint64_t* nodes, uint32_t* sg) { return suffix_tree_gsa_host<uint32_t>(c, t, n, off, m, sa, lcp, nodes, sg); }
int suffix_tree_gsa_host_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* sa, const uint64_t* lcp,
                             uint64_t* nodes, uint32_t* sg) { return suffix_tree_gsa_host<uint64_t>(c, t, n, off, m, sa, lcp, nodes, sg); }

int suffix_tree_dev_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, const uint32_t* lcp, uint64_t* nodes, uint32_t* sg, uint64_t* e) {
    return suffix_tree_dev<uint32_t>(c, t, n, sa, lcp, nodes, sg, e);
}
int suffix_tree_dev_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, const uint64_t* lcp, uint64_t* nodes, uint32_t* sg, uint64_t* e) {
    return suffix_tree_dev<uint64_t>(c, t, n, sa, lcp, nodes, sg, e);
}

int suffix_tree_host_u32(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, const uint32_t* lcp, uint64_t* nodes, uint32_t* sg) {
    return suffix_tree_host<uint32_t>(c, t, n, sa, lcp, nodes, sg);
}
int suffix_tree_host_u64(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, const uint64_t* lcp, uint64_t* nodes, uint32_t* sg) {
    return suffix_tree_host<uint64_t>(c, t, n, sa, lcp, nodes, sg);
}

int ansv_host_u32(psacx_ctx* c, const uint32_t* in, uint64_t n, int lt, int rt, uint64_t nonsv, uint64_t* l, uint64_t* r) {
    return ansv_run<uint32_t>(c, in, n, lt, rt, nonsv, l, r, false);
}
int ansv_host_u64(psacx_ctx* c, const uint64_t* in, uint64_t n, int lt, int rt, uint64_t nonsv, uint64_t* l, uint64_t* r) {
    return ansv_run<uint64_t>(c, in, n, lt, rt, nonsv, l, r, false);
}
int ansv_dev_u32(psacx_ctx* c, const uint32_t* in, uint64_t n, int lt, int rt, uint64_t nonsv, uint64_t* l, uint64_t* r) {
    return ansv_run<uint32_t>(c, in, n, lt, rt, nonsv, l, r, true);
}
int ansv_dev_u64(psacx_ctx* c, const uint64_t* in, uint64_t n, int lt, int rt, uint64_t nonsv, uint64_t* l, uint64_t* r) {
    return ansv_run<uint64_t>(c, in, n, lt, rt, nonsv, l, r, true);
}

} // namespace psacx
