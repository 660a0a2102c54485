// group_sort16_kernel<.., BITS> (psac_amd/csrc/radix.hpp) launched directly on record arrays and group starts made on the host, in the form with one
// counting round and in the form of counting rounds only.  The records it leaves are compared place by place with std::stable_sort by the 16 bits
// inside every group (tests/cpp/group_rank_model.hpp), and the words of tie bits, entry by entry, with the definition on those records
// (tests/cpp/tie_bits_model.hpp: words_brute): bit p set iff the places p - 1 and p lie in one batch and agree above the suffix field.  What the kernel
// must leave alone (a group above GROUP_CAP, a chunk whose starts are not monotone) must come back as it went in, with no bit.  The tables are those of
// tests/cpp/group_sort16_direct.hip at 1024 groups plus tables made for the bits:
//   - one key per group, groups of 200 .. 300: every place but the first of a batch has its bit -- across the places 63 | 64 of a batch, across word
//     borders, at the last record of a batch; batches start and end inside words;
//   - groups of 64 with ONE key in all of them: six groups per batch, the same 16 bits at the end of one group and the start of the next -- no bit there;
//   - groups of 300 with a run of 20 equal keys among random ones: 19 bits in a row, and a bucket of the one counting round above GROUP_RANK_MAX,
//     so the counting rounds order the batch;
//   - single groups of 385 .. 512 records with keys from a small set (many ties), empty groups between them;
//   - keys from a set of 64 in groups of Poisson-like sizes (a quarter of the places tie), a record count that is no multiple of 64;
//   - first places from 2^31 and 2^32 on that are no multiple of 64: bit indices beyond 32 bits, every batch shifted inside its words.
// One line per table; the first difference is printed; exit status 1 on a difference.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../psac_amd/csrc/dev_common.hpp"
#include "../../psac_amd/csrc/sort_scratch.hpp"
#include "../../psac_amd/csrc/radix.hpp"
#include "group_rank_model.hpp"
#include "tie_bits_model.hpp"

using namespace group_rank_model;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); std::exit(2); } } while (0)

static_assert(CAP == (unsigned)psacx::GROUP_CAP && CHUNK == (unsigned)psacx::WAVE, "the model cuts the batches the kernel cuts");

// sizes[g] records in group g, the 16 bits of record i of group g from key(g, i)
template <typename F>
static Table make_keyed(const char* name, int sfield, const std::vector<unsigned>& sizes, F key, uint64_t seed) {
    Table t{name, sfield, {}, {}, -1};
    uint64_t at = 0;
    for (uint64_t g = 0; g < sizes.size(); ++g) {
        t.starts.push_back(at);
        for (unsigned i = 0; i < sizes[g]; ++i, ++at) t.rec.push_back(make_rec(g, key(g, i, mix(seed)) & 0xFFFF, sfield, at * 2654435761ull + 12345, mix(seed) & 0xFF));
    }
    return t;
}

// base: the table lies `base` records into arrays that begin before the allocation (any base: the words of the bits begin with the word of place `base`)
static bool run_table(const Table& t, uint64_t base, uint64_t* bits_total) {
    const uint64_t nrec = t.rec.size(), ngroups = t.starts.size();
    const uint64_t nwords = (base + nrec + 63) / 64 - base / 64 + 1;
    bool ok = true;
    uint64_t* d_rec = nullptr;
    unsigned long long* d_starts = nullptr;
    unsigned long long* d_words = nullptr;
    HIP_OK(hipMalloc(&d_rec, (nrec + 1) * 8));
    HIP_OK(hipMalloc(&d_starts, ngroups * 8));
    HIP_OK(hipMalloc(&d_words, nwords * 8));
    std::vector<uint64_t> starts = t.starts;
    for (uint64_t& x : starts) x += base;
    HIP_OK(hipMemcpy(d_starts, starts.data(), ngroups * 8, hipMemcpyHostToDevice));
    uint64_t* const rec0 = reinterpret_cast<uint64_t*>(reinterpret_cast<uintptr_t>(d_rec) - base * 8);
    uint8_t* const words0 = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(d_words) - (base / 64) * 8);
    uint64_t set = 0;
    for (int form = 0; form < 2 && ok; ++form) {          // 0: one counting round and ranks, 1: counting rounds only
        // what the form must leave: its batches in stable order, everything else as it was; the bits of those batches
        std::vector<uint64_t> want = t.rec;
        std::vector<tie_bits_model::Span> spans;
        for (const Batch& b : cut(t.starts, nrec, form == 0 ? psacx::GROUP_RANK_BATCH : (unsigned)psacx::GROUP_CAP)) {
            const std::vector<uint64_t> exp = expected(&t.rec[b.a], t.starts, nrec, b, t.sfield);
            for (unsigned i = 0; i < b.count; ++i) want[b.a + i] = exp[i];
            spans.push_back({base + b.a, b.count});
        }
        const std::vector<uint64_t> want_words = tie_bits_model::words_brute(want, base, spans, t.sfield);
        if (want_words.size() != nwords) { std::printf("FAIL %s: the model has %zu words\n", t.name, want_words.size()); ok = false; break; }
        std::vector<uint64_t> got(nrec), got_words(nwords);
        HIP_OK(hipMemcpy(d_rec, t.rec.data(), nrec * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_words, 0, nwords * 8));
        // (3 workgroups of four waves for 16 chunks of 64 groups: the waves' stride loop is taken twice, and neighbouring batches belong to different workgroups)
        if (form == 0) hipLaunchKernelGGL((psacx::group_sort16_kernel<256, true, true>), dim3(3), dim3(256), 0, 0, rec0, d_starts, ngroups, base + nrec, t.sfield, words0);
        else hipLaunchKernelGGL((psacx::group_sort16_kernel<256, false, true>), dim3(3), dim3(256), 0, 0, rec0, d_starts, ngroups, base + nrec, t.sfield, words0);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got.data(), d_rec, nrec * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_words.data(), d_words, nwords * 8, hipMemcpyDeviceToHost));
        const char* const fname = form == 0 ? "one counting round" : "counting rounds only";
        for (uint64_t i = 0; i < nrec && ok; ++i)
            if (got[i] != want[i]) {
                std::printf("DIFF %s, %s, at place %llu: record %016llx, std::stable_sort gives %016llx\n", t.name, fname, (unsigned long long)i,
                            (unsigned long long)got[i], (unsigned long long)want[i]);
                ok = false;
            }
        for (uint64_t i = 0; i < nwords && ok; ++i)
            if (got_words[i] != want_words[i]) {
                std::printf("DIFF %s, %s, word %llu (places from %llu): %016llx, the definition gives %016llx\n", t.name, fname, (unsigned long long)i,
                            (unsigned long long)((base / 64 + i) * 64 - base), (unsigned long long)got_words[i], (unsigned long long)want_words[i]);
                ok = false;
            }
        set = 0;
        for (uint64_t w : want_words) set += (uint64_t)__builtin_popcountll(w);
    }
    *bits_total += set;
    std::printf("%s %-28s sfield %d first record %llu groups %llu records %llu bits %llu\n", ok ? "ok  " : "FAIL", t.name, t.sfield, (unsigned long long)base,
                (unsigned long long)ngroups, (unsigned long long)nrec, (unsigned long long)set);
    HIP_OK(hipFree(d_rec)); HIP_OK(hipFree(d_starts)); HIP_OK(hipFree(d_words));
    return ok;
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { std::printf("no HIP device\n"); return 2; }
    constexpr unsigned NG = 1024;
    std::vector<Table> all = tables(NG);
    all.push_back(make_keyed("bits_one_key_per_group", 32, poisson_like(NG, 256, 21), [](uint64_t g, unsigned, uint64_t) { return (unsigned)(g * 2654435761ull >> 7); }, 201));
    all.push_back(make_keyed("bits_one_key_groups_of_64", 32, std::vector<unsigned>(NG, 64), [](uint64_t, unsigned, uint64_t) { return 0x1234u; }, 202));
    all.push_back(make_keyed("bits_run_of_20", 32, std::vector<unsigned>(NG, 300),
                             [](uint64_t, unsigned i, uint64_t r) { return i >= 140 && i < 160 ? 0x4242u : (unsigned)r | (i < 140 ? 0u : 0x8000u) | 1u; }, 203));
    {
        std::vector<unsigned> sizes(NG);
        for (unsigned g = 0; g < NG; ++g) sizes[g] = g % 3 == 1 ? 0u : 385u + (g * 37u) % 128u;          // 385 .. 512, an empty group after every second
        sizes[5] = 512; sizes[8] = 385;
        all.push_back(make_keyed("bits_single_groups_385_512", 40, sizes, [](uint64_t, unsigned, uint64_t r) { return (unsigned)(r % 97) * 601u; }, 204));
    }
    {
        std::vector<unsigned> sizes = poisson_like(NG, 256, 25);
        uint64_t total = 0;
        for (unsigned x : sizes) total += x;
        sizes[NG - 1] += 64 - (unsigned)(total % 64) + 29;          // (the records: 29 above a multiple of 64)
        all.push_back(make_keyed("bits_keys_of_64_values", 32, sizes, [](uint64_t, unsigned, uint64_t r) { return (unsigned)(r & 63) << 9; }, 205));
    }
    uint64_t bits = 0;
    for (const Table& t : all)
        if (!run_table(t, 0, &bits)) return 1;
    const size_t k = all.size();
    if (!run_table(all[k - 1], (1ull << 31) + 17, &bits) || !run_table(all[k - 5], (1ull << 32) + 63, &bits) || !run_table(all[1], (3ull << 31) - 300000 + 5, &bits)) return 1;
    if (bits == 0) { std::printf("FAIL: no table has a bit\n"); return 1; }
    std::printf("all %zu tables agree\n", all.size() + 3);
    return 0;
}
