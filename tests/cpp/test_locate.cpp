// locate(sa, begin, end, patterns, k) of include/suffix_array.hpp on "mississippi": intervals stated here by hand from its suffix
// array (10 7 4 1 0 9 8 6 3 5 2), insertion points of absent patterns included, for both index types, without and with a lookup
// table; and its refusal on a communicator of several ranks.
// Built by tests/test_locate_model_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_locate.py.
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank() {
    const std::string text = "mississippi";
    suffix_array<char, index_t, false> sa((psacx::comm(0)));
    sa.verbose = false;
    sa.construct(text.begin(), text.end(), true);
    typedef std::pair<index_t, index_t> r;
    const std::vector<std::string> pats = {"i", "ssi", "mississippi", "", "misx", "a", "z", "ississippii", "pi", "ippi"};
    const std::vector<r> want = {r(0, 4), r(9, 11), r(4, 5), r(0, 11), r(5, 5), r(0, 0), r(11, 11), r(4, 4), r(5, 6), r(1, 2)};
    for (unsigned int k = 0; k <= 3; ++k) CHECK(locate(sa, text.begin(), text.end(), pats, k) == want);
    CHECK(locate(sa, text.begin(), text.end(), std::vector<std::string>()).empty());
    suffix_array<char, index_t, true> with_lcp((psacx::comm(0)));
    with_lcp.verbose = false;
    with_lcp.construct(text.begin(), text.end(), true);
    CHECK(locate(with_lcp, text.begin(), text.end(), pats, 2) == want);
    bool threw = false;
    try { locate(sa, text.begin(), text.end() - 1, pats); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    return 0;
}

int main() {
    if (one_rank<uint64_t>() || one_rank<uint32_t>()) return 1;
    {
        // two ranks (on one device): no distributed form, and none emulated
        const std::string text = "mississippi";
        suffix_array<char, uint64_t, false> sa((psacx::comm(std::vector<int>(2, 0))));
        sa.verbose = false;
        sa.construct(text.begin(), text.end(), true);
        bool threw = false;
        try { locate(sa, text.begin(), text.end(), std::vector<std::string>(1, "ssi")); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "locate header tests passed" << std::endl;
    return 0;
}
