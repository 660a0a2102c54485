// match(sa, begin, end, patterns, k, suffixes, max_len) and match(sa, ss, patterns, ...) of include/suffix_array.hpp on
// "mississippi" (suffix array 10 7 4 1 0 9 8 6 3 5 2) and on the set {"missis", "sippi"} (10 7 4 1 0 9 8 5 6 3 2): lengths and
// intervals stated here by hand, for both index types, without and with a lookup table, both modes and a cap; and the refusal on
// a communicator of several ranks.
// Built by tests/test_match_model_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_match.py.
#include <iostream>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static bool equal(const match_lists<index_t>& got, const std::vector<index_t>& len, const std::vector<index_t>& lb, const std::vector<index_t>& ub) {
    return got.len == len && got.lb == lb && got.ub == ub;
}

template <typename index_t>
static int one_rank() {
    typedef std::vector<index_t> v;
    const std::string text = "mississippi";
    suffix_array<char, index_t, false> sa((psacx::comm(0)));
    sa.verbose = false;
    sa.construct(text.begin(), text.end(), true);
    // the suffixes in order: i ippi issippi ississippi mississippi pi ppi sippi sissippi ssippi ssissippi
    const std::vector<std::string> pats = {"misx", "issississi", "piss", "x", "ssi", "", "issix"};
    for (unsigned int k = 0; k <= 3; ++k) {
        CHECK(equal(match(sa, text.begin(), text.end(), pats, k), v({3, 7, 2, 0, 3, 0, 4}), v({4, 3, 5, 0, 9, 0, 2}), v({5, 4, 6, 11, 11, 11, 4})));
        // every suffix of "misx" and of "pi", the empty pattern between them owning no slot: misx isx sx x pi i
        CHECK(equal(match(sa, text.begin(), text.end(), std::vector<std::string>({"misx", "", "pi"}), k, true), v({3, 2, 1, 0, 2, 1}),
                    v({4, 2, 7, 0, 5, 0}), v({5, 4, 11, 11, 6, 4})));
        // cut to two bytes: mi is pi x ss "" is
        CHECK(equal(match(sa, text.begin(), text.end(), pats, k, false, 2), v({2, 2, 2, 0, 2, 0, 2}), v({4, 2, 5, 0, 9, 0, 2}), v({5, 4, 6, 11, 11, 11, 4})));
    }
    CHECK(match(sa, text.begin(), text.end(), std::vector<std::string>()).len.empty());
    CHECK(match(sa, text.begin(), text.end(), std::vector<std::string>(3, ""), 0, true).lb.empty());
    bool threw = false;
    try { match(sa, text.begin(), text.end() - 1, pats); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);

    const std::string flat = "missis$sippi$";
    simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
    suffix_array<char, index_t, false> gsa((psacx::comm(0)));
    gsa.verbose = false;
    gsa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("mississippi")));
    // the suffixes in order: i ippi is issis missis pi ppi s sippi sis ssis; "ssip", "mississippi" and "sissi" match across the seam only
    const std::vector<std::string> spats = {"ssip", "mississippi", "sissi", "z", "is", "ssi", "", "issip"};
    for (unsigned int k = 0; k <= 3; ++k) {
        CHECK(equal(match(gsa, ss, spats, k), v({3, 6, 3, 0, 2, 3, 0, 4}), v({10, 4, 9, 0, 2, 10, 0, 3}), v({11, 5, 10, 11, 4, 11, 11, 4})));
        // ssip sip ip p
        CHECK(equal(match(gsa, ss, std::vector<std::string>(1, "ssip"), k, true), v({3, 3, 2, 1}), v({10, 8, 1, 5}), v({11, 9, 2, 7})));
    }
    threw = false;
    try { simple_dstringset shorter(flat.begin(), flat.end() - 2, psacx::comm(0)); match(gsa, shorter, spats); } catch (const std::runtime_error&) { threw = true; }
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
        try { match(sa, text.begin(), text.end(), std::vector<std::string>(1, "ssi")); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "match header tests passed" << std::endl;
    return 0;
}
