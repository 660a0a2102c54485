// group_sort16_kernel (psac_amd/csrc/radix.hpp) launched directly on record arrays and group starts made on the host (tests/cpp/group_rank_model.hpp:
// the tables tests/cpp/test_group_rank.cpp runs through the host model), once in the form with one counting round and once pinned to the counting
// rounds only (PSACX_OPT_GROUP_COUNTING_ROUNDS).  The records AND the tie bytes both leave are compared place by place with std::stable_sort by the
// 16 bits inside every group; the records carry distinct low 32 bits, so a broken order among equal keys shows.  What the kernel must leave alone
// (a group above GROUP_CAP, a chunk whose starts are not monotone) must come back as it went in, tie bytes included.  The host counts the batches
// that take the way back to the counting rounds and checks that count against what the table is named for.  One line per table; the first
// difference is printed; exit status 1 on a difference.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../psac_amd/csrc/dev_common.hpp"
#include "../../psac_amd/csrc/sort_scratch.hpp"
#include "../../psac_amd/csrc/radix.hpp"
#include "group_rank_model.hpp"

using namespace group_rank_model;

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); std::exit(2); } } while (0)

static_assert(CAP == (unsigned)psacx::GROUP_CAP && CHUNK == (unsigned)psacx::WAVE, "the model cuts the batches the kernel cuts");

// base: the table lies `base` records into arrays that begin before the allocation -- the starts count from there, as in a text whose records
// do not fit 31 or 32 bits of index; the kernel touches nothing below the first start
static bool run_table(const Table& t, uint64_t base) {
    const uint64_t nrec = t.rec.size(), ngroups = t.starts.size();
    constexpr uint8_t UNTOUCHED = 0xEE;
    // what both forms must leave, and the batches that take the way back in the form with one round
    std::vector<uint64_t> want = t.rec;
    std::vector<uint8_t> want_tie(nrec, UNTOUCHED);
    uint64_t back = 0, two_or_more = 0, batches = 0;
    for (const Batch& b : cut(t.starts, nrec, psacx::GROUP_RANK_BATCH)) {
        const std::vector<uint64_t> exp = expected(&t.rec[b.a], t.starts, nrec, b, t.sfield);
        for (unsigned i = 0; i < b.count; ++i) { want[b.a + i] = exp[i]; want_tie[b.a + i] = (uint8_t)(exp[i] >> t.sfield); }
        ++batches; two_or_more += b.count >= 2; back += way_back(&t.rec[b.a], b, t.sfield);
    }
    bool ok = true;
    if ((t.expect_back == 0 && back != 0) || (t.expect_back == 1 && (back != two_or_more || back == 0))) {
        std::printf("FAIL %s: %llu of %llu batches take the way back\n", t.name, (unsigned long long)back, (unsigned long long)two_or_more);
        ok = false;
    }
    uint64_t* d_rec = nullptr;
    unsigned long long* d_starts = nullptr;
    uint8_t* d_tie = nullptr;
    HIP_OK(hipMalloc(&d_rec, (nrec + 1) * 8));
    HIP_OK(hipMalloc(&d_starts, ngroups * 8));
    HIP_OK(hipMalloc(&d_tie, nrec + 1));
    std::vector<uint64_t> starts = t.starts;
    for (uint64_t& x : starts) x += base;
    HIP_OK(hipMemcpy(d_starts, starts.data(), ngroups * 8, hipMemcpyHostToDevice));
    uint64_t* const rec0 = reinterpret_cast<uint64_t*>(reinterpret_cast<uintptr_t>(d_rec) - base * 8);
    uint8_t* const tie0 = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(d_tie) - base);
    for (int form = 0; form < 2 && ok; ++form) {          // 0: one counting round and ranks, 1: counting rounds only
        std::vector<uint64_t> got(nrec);
        std::vector<uint8_t> got_tie(nrec);
        HIP_OK(hipMemcpy(d_rec, t.rec.data(), nrec * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(d_tie, UNTOUCHED, nrec + 1));
        // (7 workgroups of four waves: the 64 chunks of 4096 groups take the waves' stride loop to its third trip)
        if (form == 0) hipLaunchKernelGGL((psacx::group_sort16_kernel<256, true>), dim3(7), dim3(256), 0, 0, rec0, d_starts, ngroups, base + nrec, t.sfield, tie0);
        else hipLaunchKernelGGL((psacx::group_sort16_kernel<256, false>), dim3(7), dim3(256), 0, 0, rec0, d_starts, ngroups, base + nrec, t.sfield, tie0);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got.data(), d_rec, nrec * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got_tie.data(), d_tie, nrec, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < nrec; ++i)
            if (got[i] != want[i] || got_tie[i] != want_tie[i]) {
                std::printf("DIFF %s, %s, at place %llu: record %016llx tie byte %02x, std::stable_sort gives %016llx %02x\n", t.name,
                            form == 0 ? "one counting round" : "counting rounds only", (unsigned long long)i, (unsigned long long)got[i], got_tie[i],
                            (unsigned long long)want[i], want_tie[i]);
                ok = false;
                break;
            }
    }
    std::printf("%s %-28s sfield %d first record %llu groups %llu records %llu batches %llu way back %llu\n", ok ? "ok  " : "FAIL", t.name, t.sfield,
                (unsigned long long)base, (unsigned long long)ngroups, (unsigned long long)nrec, (unsigned long long)batches, (unsigned long long)back);
    HIP_OK(hipFree(d_rec)); HIP_OK(hipFree(d_starts)); HIP_OK(hipFree(d_tie));
    return ok;
}

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { std::printf("no HIP device\n"); return 2; }
    const std::vector<Table> all = tables(4096);
    for (const Table& t : all)
        if (!run_table(t, 0)) return 1;
    // record numbers whose low halves lie from 2^31 on, below and above 2^32 (2^32 characters: the upper half of the records)
    if (!run_table(all[0], 1ull << 31) || !run_table(all[0], 3ull << 31) || !run_table(all[1], (3ull << 31) - 300000)) return 1;
    std::printf("all %zu tables agree\n", all.size() + 3);
    return 0;
}
