// lce(sa, a, b, max_mismatch), lce(sa, ss, a, b, max_mismatch) and range_min(sa, lo, hi) of include/suffix_array.hpp on
// "mississippi" (LCP 0 1 1 4 0 0 1 0 2 1 3) and on the set {"missis", "sippi"}: lengths, minima and positions stated here by hand,
// for both index types; and the refusal on a communicator of several ranks.
// Built by tests/test_rmq_lce_model_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_lce.py.
#include <iostream>
#include <limits>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank() {
    typedef std::vector<index_t> v;
    const std::string text = "mississippi";
    suffix_array<char, index_t, true> sa((psacx::comm(0)));
    sa.verbose = false;
    sa.construct(text.begin(), text.end(), true);
    // ississippi / issippi, ssissippi / ssippi, mississippi / ississippi, sissippi / sippi, a == b, i / ippi, the empty suffix
    const v a({1, 2, 0, 3, 4, 10, 11}), b({4, 5, 1, 6, 4, 7, 3});
    CHECK(lce(sa, a, b) == v({4, 3, 0, 2, 7, 1, 0}));
    CHECK(lce(sa, a, b, 1) == v({5, 4, 1, 3, 7, 1, 0}));
    CHECK(lce(sa, v({1}), v({4}), 2) == v({7}));
    CHECK(lce(sa, a, b, 100) == v({7, 6, 10, 5, 7, 1, 0}));
    CHECK(lce(sa, v(), v()).empty());
    bool threw = false;
    try { lce(sa, a, v({1})); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);

    const index_t ones = std::numeric_limits<index_t>::max();
    const range_minima<index_t> r = range_min(sa, v({0, 1, 3, 5, 8, 1}), v({11, 4, 4, 5, 20, 11}));
    CHECK(r.min == v({0, 1, 4, ones, 1, 0}));
    CHECK(r.arg == v({0, 1, 3, 11, 9, 4}));

    const std::string flat = "missis$sippi$";
    simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
    suffix_array<char, index_t, true> gsa((psacx::comm(0)));
    gsa.verbose = false;
    gsa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("mississippi")));
    // issis / ippi, ssis / sippi, sis / sippi, ssis / s (the text goes on with "sippi": not across the seam), a == b, s / sippi
    const v sa_({1, 2, 3, 2, 4, 5, 6}), sb({7, 6, 6, 5, 4, 6, 11});
    CHECK(lce(gsa, ss, sa_, sb) == v({1, 1, 2, 1, 2, 1, 0}));
    CHECK(lce(gsa, ss, sa_, sb, 1) == v({2, 2, 3, 1, 2, 1, 0}));
    threw = false;
    try { simple_dstringset shorter(flat.begin(), flat.end() - 2, psacx::comm(0)); lce(gsa, shorter, sa_, sb); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    return 0;
}

int main() {
    if (one_rank<uint64_t>() || one_rank<uint32_t>()) return 1;
    {
        // two ranks (on one device): no distributed form, and none emulated
        const std::string text = "mississippi";
        suffix_array<char, uint64_t, true> sa((psacx::comm(std::vector<int>(2, 0))));
        sa.verbose = false;
        sa.construct(text.begin(), text.end(), true);
        bool threw = false;
        try { lce(sa, std::vector<uint64_t>(1, 1), std::vector<uint64_t>(1, 4)); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
        threw = false;
        try { range_min(sa, std::vector<uint64_t>(1, 1), std::vector<uint64_t>(1, 4)); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "lce header tests passed" << std::endl;
    return 0;
}
