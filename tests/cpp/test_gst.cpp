// construct_gst(sa, ss) of include/suffix_array.hpp on the set {"ab", "ab", "b"}, whose table tests/test_gst_model_cpu.py
// states cell by cell, for both index types; and its refusal on a communicator of several ranks.
// Built by tests/test_gst_model_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_gst.py.
#include <iostream>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank(const std::vector<std::size_t>& want) {
    std::vector<std::string> strs = {"ab", "ab", "b"};
    std::string flat = flatten_strings(strs);
    simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
    psacx::alphabet<char> a = psacx::alphabet<char>::from_string("ab", psacx::comm(0));
    suffix_array<char, index_t, true> sa((psacx::comm(0)));
    sa.verbose = false;
    sa.construct_ss(ss, a);
    CHECK(construct_gst(sa, ss, psacx::comm(0)) == want);
    CHECK(construct_gst(sa, ss) == want);
    return 0;
}

int main() {
    //                                      $lo $hi a  b
    const std::vector<std::size_t> want = {0, 0, 1, 3,      // root: "ab.." is node 1, "b.." node 3
                                           5, 6, 0, 0,      // node 1 = "ab": the two equal suffixes, leaves 5 and 6
                                           0, 0, 0, 0,
                                           7, 9, 0, 0,      // node 3 = "b": leaves 7, 8, 9
                                           0, 0, 0, 0};
    if (one_rank<uint64_t>(want) || one_rank<uint32_t>(want)) return 1;
    {
        // two ranks (on one device): no distributed form, and none emulated
        std::vector<std::string> strs = {"ab", "ab", "b"};
        std::string flat = flatten_strings(strs);
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        suffix_array<char, uint64_t, true> sa((psacx::comm(std::vector<int>(2, 0))));
        sa.verbose = false;
        sa.construct_ss(ss, psacx::alphabet<char>::from_string("ab", psacx::comm(0)));
        bool threw = false;
        try { construct_gst(sa, ss); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "gst header tests passed" << std::endl;
    return 0;
}
