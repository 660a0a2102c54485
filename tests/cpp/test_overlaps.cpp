// overlaps(sa, ss, min_len, whole) of include/suffix_array.hpp on the set {"abab", "babab", "ab", "abab"} (offsets 0 4 9 11 15;
// SA 2 7 9 13 0 5 11 3 8 10 14 1 6 12 4): the intervals stated here by hand, for both index types, the lists behind them through
// occurrences(sa, ss, lb, ub), and the refusals.
// Built by tests/test_overlaps_build_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_overlaps.py.
#include <iostream>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank() {
    typedef std::vector<index_t> v;
    const std::string flat = "abab$babab$ab$abab$";
    simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
    suffix_array<char, index_t, true> gsa((psacx::comm(0)));
    gsa.verbose = false;
    gsa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("ab")));
    // slot 1: "ab" onto string 0 -- its own border at 2, the end of babab, string 2 whole, the end of the other abab;
    // slot 4: "b" onto babab; slot 6: "bab" onto babab, itself a border; slot 12: "ab" onto string 3; "a", "aba", "ba", "baba" end nothing
    overlap_intervals<index_t> r = overlaps(gsa, ss, 1);
    CHECK(r.lb == v({0, 0, 0, 0, 7, 0, 11, 0, 0, 0, 0, 0, 0, 0, 0}));
    CHECK(r.ub == v({0, 4, 0, 0, 11, 0, 14, 0, 0, 0, 0, 0, 4, 0, 0}));
    // with the whole strings: abab ends abab, babab and abab (slots 3 and 14), babab ends itself (8), ab ends four strings (10)
    r = overlaps(gsa, ss, 1, true);
    CHECK(r.lb == v({0, 0, 0, 4, 7, 0, 11, 0, 14, 0, 0, 0, 0, 0, 4}));
    CHECK(r.ub == v({0, 4, 0, 7, 11, 0, 14, 0, 15, 0, 4, 0, 4, 0, 7}));
    r = overlaps(gsa, ss, 2, true);
    CHECK(r.lb == v({0, 0, 0, 4, 0, 0, 11, 0, 14, 0, 0, 0, 0, 0, 4}));
    CHECK(r.ub == v({0, 4, 0, 7, 0, 0, 14, 0, 15, 0, 4, 0, 4, 0, 7}));
    const occurrence_lists<index_t> occ = occurrences(gsa, ss, r.lb, r.ub);
    CHECK(occ.start.size() == 16 && occ.start[1] == 0 && occ.start[2] == 4 && occ.start[4] == 7 && occ.start[15] == 22);
    CHECK(v(occ.pos.begin(), occ.pos.begin() + 7) == v({2, 7, 9, 13, 0, 5, 11}));
    CHECK(v(occ.sid.begin(), occ.sid.begin() + 7) == v({0, 1, 2, 3, 0, 1, 3}));
    r = overlaps(gsa, ss, 6, true);
    CHECK(r.lb == v(15, 0) && r.ub == v(15, 0));
    bool threw = false;
    try { overlaps(gsa, ss, 0); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    threw = false;
    try { simple_dstringset shorter(flat.begin(), flat.end() - 2, psacx::comm(0)); overlaps(gsa, shorter, 1); } catch (const std::runtime_error&) { threw = true; }
    CHECK(threw);
    return 0;
}

int main() {
    if (one_rank<uint64_t>() || one_rank<uint32_t>()) return 1;
    {
        // two ranks (on one device): no distributed form, and none emulated
        const std::string flat = "abab$babab$";
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        suffix_array<char, uint64_t, true> sa((psacx::comm(std::vector<int>(2, 0))));
        sa.verbose = false;
        sa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("ab")));
        bool threw = false;
        try { overlaps(sa, ss, 1); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "overlaps header tests passed" << std::endl;
    return 0;
}
