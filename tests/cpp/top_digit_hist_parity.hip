// top_digit_hist_waves_kernel against top_digit_hist_kernel (psac_amd/csrc/sa_kernels.hpp): both fill tile_hist[tile][256] from the same
// device text and the tables are compared on the host, entry by entry.  A wrong table makes key_scatter1w_kernel write outside its
// buckets, so this runs before any construction that scatters by the new kernel's table (tests/test_gpu_side_kernels.py).
// One line per case; exit status 1 at the first difference.  Nothing but the two kernels is launched.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../psac_amd/csrc/radix.hpp"
#include "../../psac_amd/csrc/sa_kernels.hpp"

using namespace psacx;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); std::exit(2); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {          // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Case {
    std::string name;
    uint64_t n;
    unsigned lc, symbols;       // bits per character, distinct characters of the text
    uint64_t spec;              // short suffixes in front of the records
    uint64_t extra;             // n_text = n + extra
    unsigned ptr_off;           // text pointer: this many bytes past a 16-byte boundary
    int shape;                  // 0 random, 1 one symbol, 2 one symbol and the last nch characters another
};

static constexpr int BLOCK = 512, ITEMS = 8, TILE = BLOCK * ITEMS, NEW_BLOCK = 256, NEW_NW = NEW_BLOCK / WAVE;
static constexpr uint64_t MAX_N = 64ull * TILE + 1, SLACK = 256;

static uint8_t* d_raw = nullptr;
static unsigned *d_old = nullptr, *d_new = nullptr;

static bool run_case(const Case& cs) {
    const uint64_t n = cs.n, n_text = cs.n + cs.extra;
    const unsigned nch_full = (8 + cs.lc - 1) / cs.lc;
    CodeTable tab;
    for (int i = 0; i < 256; ++i) tab.c[i] = 0;
    // the symbols are bytes spread over the byte range, their codes 0 .. symbols - 1 in byte order (engine.hpp: build_alphabet)
    std::vector<uint8_t> sym(cs.symbols);
    for (unsigned s = 0; s < cs.symbols; ++s) { sym[s] = (uint8_t)(cs.symbols == 256 ? s : 33 + s * (222 / cs.symbols)); tab.c[sym[s]] = (uint16_t)s; }
    // the bytes around the text are another symbol's: a read outside [0, n_text) that counts shows in the table
    std::vector<uint8_t> host(SLACK + n_text + SLACK, sym[cs.symbols - 1]);
    uint8_t* t = host.data() + SLACK + cs.ptr_off;
    for (uint64_t i = 0; i < n_text; ++i) t[i] = cs.shape == 0 ? sym[rng() % cs.symbols] : sym[0];
    if (cs.shape == 2) for (uint64_t i = n_text - std::min<uint64_t>(n_text, nch_full); i < n_text; ++i) t[i] = sym[cs.symbols - 1];
    HIP_OK(hipMemcpy(d_raw, host.data(), host.size(), hipMemcpyHostToDevice));
    const uint8_t* d_text = d_raw + SLACK + cs.ptr_off;
    KeyShape ks;
    ks.lc = cs.lc; ks.c1 = 64 / cs.lc; ks.c2 = 64 / cs.lc; ks.spec = cs.spec;
    const uint64_t ntiles = (n + TILE - 1) / TILE;
    const size_t tab_bytes = ntiles * RADIX * sizeof(unsigned);
    std::vector<unsigned> h_old(ntiles * RADIX), h_new(ntiles * RADIX);
    HIP_OK(hipMemset(d_old, 0xA5, tab_bytes));
    hipLaunchKernelGGL((top_digit_hist_kernel<uint64_t, BLOCK, ITEMS>), dim3((unsigned)ntiles), dim3(BLOCK), 0, 0, d_text, n, n_text, tab, ks, d_old);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h_old.data(), d_old, tab_bytes, hipMemcpyDeviceToHost));
    uint64_t total = 0;
    for (unsigned v : h_old) total += v;
    bool ok = total == n;          // (the parent's table counts every record once)
    // a grid that gives every wave one tile, and one workgroup alone: its four waves loop over all tiles
    const unsigned grids[2] = {(unsigned)((ntiles + NEW_NW - 1) / NEW_NW), 1u};
    for (int g = 0; g < 2 && ok; ++g) {
        HIP_OK(hipMemset(d_new, 0x5A, tab_bytes));
        hipLaunchKernelGGL((top_digit_hist_waves_kernel<NEW_BLOCK>), dim3(grids[g]), dim3(NEW_BLOCK), 0, 0, d_text, n, n_text, tab, ks, ntiles, d_new);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(h_new.data(), d_new, tab_bytes, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < h_old.size(); ++i)
            if (h_old[i] != h_new[i]) {
                std::printf("DIFF %s grid %u: tile %llu digit %llu: %u (top_digit_hist_kernel) against %u\n", cs.name.c_str(), grids[g],
                            (unsigned long long)(i / RADIX), (unsigned long long)(i % RADIX), h_old[i], h_new[i]);
                ok = false;
                break;
            }
    }
    std::printf("%s %s: n %llu n_text %llu lc %u symbols %u spec %llu pointer +%u tiles %llu\n", ok ? "ok  " : "FAIL", cs.name.c_str(), (unsigned long long)n,
                (unsigned long long)n_text, cs.lc, cs.symbols, (unsigned long long)cs.spec, cs.ptr_off, (unsigned long long)ntiles);
    return ok;
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { std::printf("no HIP device\n"); return 2; }
    HIP_OK(hipMalloc(&d_raw, 2 * SLACK + MAX_N + 100 + 16));
    HIP_OK(hipMalloc(&d_old, 65 * RADIX * sizeof(unsigned)));
    HIP_OK(hipMalloc(&d_new, 65 * RADIX * sizeof(unsigned)));
    const uint64_t N3 = 3ull * TILE + 3;
    const unsigned lcs[6] = {1, 2, 3, 5, 7, 8}, syms[6] = {2, 4, 5, 20, 128, 256};
    std::vector<Case> cases;
    // the sizes: one record, one short of a lane's run, a run, around a tile, a last tile of three records, more tiles than the waves of a small grid
    for (uint64_t n : std::vector<uint64_t>{1, 63, 64, 4095, 4096, 4097, N3, MAX_N})
        for (uint64_t spec : {0ull, 41ull})
            cases.push_back({"size", n, 2, 4, std::min(spec, n), 0, 0, 0});
    // every width of the top digit in characters (lc 1, 2, 3, 5, 7, 8: nch 8, 4, 3, 2, 2, 1), with and without short suffixes in front, the text ending
    // with the records or 100 characters later, every alignment class of the text pointer
    for (int a = 0; a < 6; ++a)
        for (uint64_t spec : {0ull, 41ull})
            for (uint64_t extra : {0ull, 100ull})
                for (unsigned off : {0u, 1u, 8u, 15u})
                    cases.push_back({"shape", N3, lcs[a], syms[a], spec, extra, off, 0});
    for (int a = 0; a < 6; ++a) {
        cases.push_back({"one_symbol", N3, lcs[a], syms[a], 0, 0, 0, 1});
        cases.push_back({"one_symbol", N3, lcs[a], syms[a], 41, 100, 1, 1});
        cases.push_back({"last_characters_differ", N3, lcs[a], syms[a], 0, 0, 0, 2});
        cases.push_back({"last_characters_differ", N3, lcs[a], syms[a], 41, 0, 15, 2});
    }
    // the long text at the other alignments and widths: whole tiles on the fast path in several trips of a wave
    for (int a = 0; a < 6; ++a) cases.push_back({"trips", MAX_N, lcs[a], syms[a], a & 1 ? 41ull : 0ull, a & 2 ? 100ull : 0ull, (unsigned)(5 * a) & 15u, 0});
    for (const Case& cs : cases)
        if (!run_case(cs)) return 1;
    std::printf("all %zu cases agree\n", cases.size());
    HIP_OK(hipFree(d_raw)); HIP_OK(hipFree(d_old)); HIP_OK(hipFree(d_new));
    return 0;
}
