// prefix_sort_1w (psac_amd/csrc/engine.hpp) in its two forms on the same device text: the LSD passes on every digit inside the 256 buckets
// (PSACX_OPT_LSD_BUCKET_PASSES) against the group form -- upper digits most significant first, the last 16 prefix bits ordered on chip
// (radix.hpp: group_sort16_kernel).  The record arrays and the tie bytes are compared BIT FOR BIT: the constructions of
// tests/test_gpu_group_sort.py cannot see the order among records that tie on the prefix, because the tie stage reorders them; the stable
// order of the sort is what the short suffixes rely on.  Every case runs without and with the padded output of the pass on the top digit, and
// must report the psacx_stats.group_sort it is named for.  One line per case; the first difference is printed; exit status 1 on a difference.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../psac_amd/csrc/engine.hpp"

using namespace psacx;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); std::exit(2); } } while (0)

static std::vector<uint64_t> stream64(uint64_t n, uint64_t seed) {          // tests/inputs.py: splitmix64_stream
    std::vector<uint64_t> v(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        v[i] = z ^ (z >> 31);
    }
    return v;
}
static std::vector<uint8_t> dna(uint64_t n, uint64_t seed) {
    const std::vector<uint64_t> s = stream64(n, seed);
    std::vector<uint8_t> t(n);
    for (uint64_t i = 0; i < n; ++i) t[i] = (uint8_t)"ACGT"[s[i] & 3];
    return t;
}
static std::vector<uint8_t> ascii128(uint64_t n, uint64_t seed) {
    const std::vector<uint64_t> s = stream64(n, seed);
    std::vector<uint8_t> t(n);
    for (uint64_t i = 0; i < n; ++i) t[i] = (uint8_t)(s[i] & 127);
    return t;
}
// random DNA with `motif` at so many places that exactly `want` suffixes begin with it (counted)
static std::vector<uint8_t> plant(uint64_t n, uint64_t seed, const char* motif, uint64_t want) {
    std::vector<uint8_t> t = dna(n, seed);
    const size_t k = std::strlen(motif);
    auto count = [&]() { uint64_t c = 0; for (uint64_t i = 0; i + k <= n; ++i) c += std::memcmp(&t[i], motif, k) == 0; return c; };
    uint64_t at = 4099, have = count();
    while (have < want) {
        for (uint64_t j = have; j < want; ++j) { std::memcpy(&t[at], motif, k); at += 397; }
        have = count();
    }
    if (have != want || at + 4096 >= n) { std::printf("plant: %llu of %llu\n", (unsigned long long)have, (unsigned long long)want); std::exit(2); }
    return t;
}
static std::vector<uint8_t> short_tail_pairs(uint64_t n, uint64_t seed) {          // tests/test_gpu_group_sort.py: _dna_short_tail_pairs
    std::vector<uint8_t> t = dna(n, seed);
    const uint64_t p = 1000003, m = 40, r = 22;
    t[p + m - 1] = 'C';
    for (uint64_t i = 0; i < r; ++i) t[p + m + i] = 'A';
    t[p + m + r] = 'C';
    for (uint64_t i = 0; i < m; ++i) t[n - m + i] = t[p + i];
    return t;
}

struct Case { std::string name; std::vector<uint8_t> text; unsigned lc, lead; int expect; };

static bool run_case(const Case& cs, uint64_t pad) {
    const uint64_t n = cs.text.size();
    psacx_ctx ctx;
    std::memset(&ctx.stats, 0, sizeof(ctx.stats));
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, 0));
    ctx.n_cu = prop.multiProcessorCount;
    CodeTable tab;
    bool present[256] = {false};
    for (uint8_t ch : cs.text) present[ch] = true;
    uint16_t next = 0;
    for (int ch = 0; ch < 256; ++ch) tab.c[ch] = present[ch] ? next++ : (uint16_t)0;          // (engine.hpp: build_alphabet)
    KeyShape ks;
    ks.lc = cs.lc; ks.c1 = 64 / cs.lc; ks.c2 = 64 / cs.lc; ks.spec = std::min<uint64_t>(ks.c1 + ks.c2 - 1, n);
    const unsigned lo1 = ks.c1 * cs.lc - cs.lead;
    uint8_t* d_text = nullptr;
    uint64_t *d_k0 = nullptr, *d_a = nullptr;
    uint8_t *d_dig = nullptr, *d_tie = nullptr;
    SortScratch sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.desc_bytes = sort_desc_bytes(n) + onew_sub_bucket_supplement(n);
    HIP_OK(hipMalloc(&d_text, n + 64));
    HIP_OK(hipMemset(d_text, 0, n + 64));
    HIP_OK(hipMemcpy(d_text, cs.text.data(), n, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&d_k0, (n + RADIX * pad) * 8));
    HIP_OK(hipMalloc(&d_a, n * 8));
    HIP_OK(hipMalloc(&d_dig, n + 256));
    HIP_OK(hipMalloc(&d_tie, n + 256));
    HIP_OK(hipMalloc(&sc.d_desc, sc.desc_bytes));
    HIP_OK(hipMalloc(&sc.d_base, (size_t)MAX_PASSES * RADIX * 8));
    HIP_OK(hipHostMalloc((void**)&sc.h_base, (size_t)MAX_PASSES * RADIX * 8, hipHostMallocDefault));
    std::vector<uint64_t> rec[2];
    std::vector<uint8_t> tie[2];
    const uint64_t* where[2] = {nullptr, nullptr};
    uint64_t form[2] = {0, 0};
    bool ok = true;
    for (int f = 0; f < 2 && ok; ++f) {          // 0: the LSD passes, 1: the default
        ctx.knobs = Knobs();
        ctx.knobs.lsd_bucket_passes = f == 0;
        ctx.stats.group_sort = 0;
        HIP_OK(hipMemset(d_k0, 0xA5, (n + RADIX * pad) * 8));
        HIP_OK(hipMemset(d_a, 0x5A, n * 8));
        HIP_OK(hipMemset(d_tie, 0xEE, n + 256));
        uint64_t* s1 = nullptr;
        OneWordView view = OneWordView();
        const int rc = prefix_sort_1w(&ctx, sc, d_k0, d_a, (uint64_t*)nullptr, n, lo1, cs.lead, (psacx_round*)nullptr, &s1, d_text, n, tab, ks, /*probe=*/false, &view, d_dig, pad, d_tie);
        HIP_OK(hipDeviceSynchronize());
        if (rc != PSACX_OK) { std::printf("FAIL %s: prefix_sort_1w returned %d (%s)\n", cs.name.c_str(), rc, ctx.hip_err.c_str()); ok = false; break; }
        rec[f].resize(n); tie[f].resize(n);
        HIP_OK(hipMemcpy(rec[f].data(), s1, n * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(tie[f].data(), d_tie, n, hipMemcpyDeviceToHost));
        where[f] = s1;
        form[f] = ctx.stats.group_sort;
    }
    if (ok && (form[0] != 0 || form[1] != (uint64_t)cs.expect)) {
        std::printf("FAIL %s: group_sort %llu (pinned) and %llu, expected 0 and %d\n", cs.name.c_str(), (unsigned long long)form[0], (unsigned long long)form[1], cs.expect);
        ok = false;
    }
    if (ok && where[0] != where[1]) { std::printf("FAIL %s: the sorted records end up in different arrays\n", cs.name.c_str()); ok = false; }
    for (uint64_t i = 0; ok && i < n; ++i)
        if (rec[0][i] != rec[1][i] || tie[0][i] != tie[1][i]) {
            std::printf("DIFF %s at place %llu: record %016llx tie byte %02x (LSD passes) against %016llx %02x\n", cs.name.c_str(), (unsigned long long)i,
                        (unsigned long long)rec[0][i], tie[0][i], (unsigned long long)rec[1][i], tie[1][i]);
            ok = false;
        }
    std::printf("%s %s: n %llu lead %u pad %llu group_sort %llu\n", ok ? "ok  " : "FAIL", cs.name.c_str(), (unsigned long long)n, cs.lead, (unsigned long long)pad,
                (unsigned long long)form[1]);
    HIP_OK(hipFree(d_text)); HIP_OK(hipFree(d_k0)); HIP_OK(hipFree(d_a)); HIP_OK(hipFree(d_dig)); HIP_OK(hipFree(d_tie));
    HIP_OK(hipFree(sc.d_desc)); HIP_OK(hipFree(sc.d_base)); HIP_OK(hipHostFree(sc.h_base));
    return ok;
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { std::printf("no HIP device\n"); return 2; }
    const uint64_t N1 = (1ull << 23) + 4097 + 3, N6 = (1ull << 22) + 1234, N7 = (1ull << 23) + 1234;
    std::vector<Case> cases;
    cases.push_back({"dna_last_tile_of_3", dna(N1, 21), 2, 32, 1});
    cases.push_back({"dna_last_tile_of_3_lead40", dna(N1, 21), 2, 40, 1});
    cases.push_back({"ascii128_lc7_lead40", ascii128((1ull << 23) + 1, 23), 7, 40, 1});
    cases.push_back({"planted_sub_bucket_lead40", plant(N6, 31, "CGTTGCAT", 10000), 2, 40, 1});
    cases.push_back({"planted_group_cap_lead40", plant(N6, 32, "CGTTGCATTACG", GROUP_CAP), 2, 40, 1});
    cases.push_back({"planted_group_cap_plus_1_lead40", plant(N6, 32, "CGTTGCATTACG", GROUP_CAP + 1), 2, 40, 2});
    cases.push_back({"planted_group_cap_lead32", plant(N7, 33, "CGTTGCAT", GROUP_CAP), 2, 32, 1});
    cases.push_back({"planted_group_cap_plus_1_lead32", plant(N7, 33, "CGTTGCAT", GROUP_CAP + 1), 2, 32, 2});
    cases.push_back({"dna_short_tail_pairs", short_tail_pairs(1ull << 23, 25), 2, 32, 1});
    cases.push_back({"dna_short_tail_pairs_lead40", short_tail_pairs(1ull << 23, 25), 2, 40, 1});
    for (const Case& cs : cases)
        for (uint64_t pad : {0ull, 20480ull})
            if (!run_case(cs, pad)) return 1;
    std::printf("all %zu cases agree\n", 2 * cases.size());
    return 0;
}
