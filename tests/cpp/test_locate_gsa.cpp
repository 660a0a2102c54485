// locate(sa, ss, patterns, k) and occurrences(...) of include/suffix_array.hpp on the set {"missis", "sippi"}: intervals stated
// here by hand from its generalized suffix array (10 7 4 1 0 9 8 5 6 3 2 over "mississippi" without a separator: the suffixes
// at 1 .. 5 end with "missis", so "s" at 5 comes before "sippi" at 6), for both index types, without and with a lookup table; the
// occurrence lists with and without the set; and the refusal of both on a communicator of several ranks.
// Built by tests/test_locate_gsa_model_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_locate_gsa.py.
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank() {
    const std::string flat = "missis$sippi$";
    simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
    suffix_array<char, index_t, false> sa((psacx::comm(0)));
    sa.verbose = false;
    sa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("mississippi")));
    const index_t gsa[11] = {10, 7, 4, 1, 0, 9, 8, 5, 6, 3, 2};
    CHECK(sa.local_SA == std::vector<index_t>(gsa, gsa + 11));
    typedef std::pair<index_t, index_t> r;
    // the suffixes in order: i ippi is issis missis pi ppi s sippi sis ssis
    const std::vector<std::string> pats = {"i", "ssi", "missis", "", "sis", "siss", "issi", "sissi", "a", "z", "s", "ssip", "pi", "mississippi"};
    const std::vector<r> want = {r(0, 4), r(10, 11), r(4, 5), r(0, 11), r(9, 10), r(10, 10), r(3, 4), r(10, 10), r(0, 0), r(11, 11), r(7, 11),
                                 r(10, 10), r(5, 6), r(5, 5)};
    for (unsigned int k = 0; k <= 3; ++k) CHECK(locate(sa, ss, pats, k) == want);
    CHECK(locate(sa, ss, std::vector<std::string>()).empty());
    std::vector<index_t> lb, ub;
    for (std::size_t i = 0; i < want.size(); ++i) { lb.push_back(want[i].first); ub.push_back(want[i].second); }
    const occurrence_lists<index_t> all = occurrences(sa, ss, lb, ub);
    CHECK(all.start.size() == pats.size() + 1 && all.start[0] == 0 && all.start[1] == 4 && all.start.back() == all.pos.size());
    CHECK(all.pos.size() == 4 + 1 + 1 + 11 + 1 + 0 + 1 + 0 + 0 + 0 + 4 + 0 + 1 + 0 && all.sid.size() == all.pos.size());
    CHECK(all.pos[0] == 10 && all.pos[1] == 7 && all.pos[2] == 4 && all.pos[3] == 1);          // "i", in SA order
    CHECK(all.sid[0] == 1 && all.sid[1] == 1 && all.sid[2] == 0 && all.sid[3] == 0);
    CHECK(all.pos[4] == 2 && all.sid[4] == 0);                                                   // "ssi" only inside "missis"
    const occurrence_lists<index_t> two = occurrences(sa, lb, ub, 2);
    CHECK(two.sid.empty() && two.start[1] == 2 && two.start[4] == 2 + 1 + 1 + 2 && two.pos[0] == 10 && two.pos[1] == 7);
    bool threw = false;
    try { simple_dstringset shorter(flat.begin(), flat.end() - 2, psacx::comm(0)); locate(sa, shorter, pats); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    return 0;
}

int main() {
    if (one_rank<uint64_t>() || one_rank<uint32_t>()) return 1;
    {
        // two ranks (on one device): no distributed form, and none emulated
        const std::string flat = "missis$sippi$";
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        suffix_array<char, uint64_t, false> sa((psacx::comm(std::vector<int>(2, 0))));
        sa.verbose = false;
        sa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("mississippi")));
        bool threw = false;
        try { locate(sa, ss, std::vector<std::string>(1, "ssi")); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
        threw = false;
        try { occurrences(sa, std::vector<uint64_t>(1, 0), std::vector<uint64_t>(1, 1)); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "locate_gsa header tests passed" << std::endl;
    return 0;
}
