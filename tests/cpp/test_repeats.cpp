// bwt(...) and repeats(...) of include/suffix_array.hpp on "mississippi", "banana" and the set {abcab, cab}: the lists stated here by
// hand (tests/test_repeats_model_cpu.py holds the same ones to the model), for both index types, and the refusals.
// Built by tests/test_repeats_build_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_repeats.py.
#include <iostream>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank() {
    typedef std::vector<index_t> v;
    suffix_array<char, index_t, true> sa((psacx::comm(0)));
    sa.verbose = false;
    {
        const std::string text = "mississippi";
        bool threw = false;                                         // nothing constructed
        try { repeats(sa, text.begin(), text.end()); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
        sa.construct(text.begin(), text.end());
        // SA 10 7 4 1 0 9 8 6 3 5 2, LCP 0 1 1 4 0 0 1 0 2 1 3
        const bwt_result b = bwt(sa, text.begin(), text.end());
        CHECK(b.bwt == "pssmipissii" && b.primary == 4);            // rank 4 is the whole text: the byte in front is the last one
        repeat_intervals<index_t> r = repeats(sa, text.begin(), text.end(), repeats_right);
        // i x4, issi x2, p x2, si x2, s x4, ssi x2: heads 1 3 6 8 9 10
        CHECK(r.lb == v({0, 2, 5, 7, 7, 9}) && r.ub == v({4, 4, 7, 9, 11, 11}) && r.len == v({1, 4, 1, 2, 1, 3}));
        r = repeats(sa, text.begin(), text.end());
        CHECK(r.lb == v({0, 2, 5, 7}) && r.ub == v({4, 4, 7, 11}) && r.len == v({1, 4, 1, 1}));
        r = repeats(sa, text.begin(), text.end(), repeats_supermaximal);
        CHECK(r.lb == v({2, 5}) && r.ub == v({4, 7}) && r.len == v({4, 1}));                 // issi, p
        r = repeats(sa, text.begin(), text.end(), repeats_right, 2, 2, 2);
        CHECK(r.lb == v({2, 7, 9}) && r.len == v({4, 2, 3}));
        r = repeats(sa, text.begin(), text.end(), repeats_maximal, 1, 3);
        CHECK(r.lb == v({0, 7}) && r.ub == v({4, 11}));
        bool refused = false;                                       // a text of another length
        const std::string other = "mississipp";
        try { repeats(sa, other.begin(), other.end()); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
    }
    {
        const std::string text = "banana";                          // SA 5 3 1 0 4 2, LCP 0 1 3 0 0 2
        sa.construct(text.begin(), text.end());
        const bwt_result b = bwt(sa, text.begin(), text.end());
        CHECK(b.bwt == "nnbaaa" && b.primary == 3);
        repeat_intervals<index_t> r = repeats(sa, text.begin(), text.end());
        CHECK(r.lb == v({0, 1}) && r.ub == v({3, 3}) && r.len == v({1, 3}));                 // a x3, ana x2
        r = repeats(sa, text.begin(), text.end(), repeats_supermaximal);
        CHECK(r.lb == v({1}) && r.ub == v({3}) && r.len == v({3}));                          // ana
    }
    {
        const std::string flat = "abcab$cab";                       // suffixes ab(3) ab(6) abcab(0) b(4) b(7) bcab(1) cab(2) cab(5)
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        sa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("abc")));
        const bwt_result b = bwt(sa, ss);
        CHECK(b.bwt == "ccbaaabb" && b.primary == 2);
        repeat_intervals<index_t> r = repeats(sa, ss, repeats_right);
        CHECK(r.lb == v({0, 3, 6}) && r.ub == v({3, 6, 8}) && r.len == v({2, 1, 3}));        // ab x3, b x3, cab x2
        r = repeats(sa, ss);
        CHECK(r.lb == v({0, 6}) && r.ub == v({3, 8}) && r.len == v({2, 3}));                 // ab, cab
        r = repeats(sa, ss, repeats_supermaximal);
        CHECK(r.lb == v({6}) && r.ub == v({8}) && r.len == v({3}));                          // cab
    }
    return 0;
}

int main() {
    if (one_rank<uint64_t>() || one_rank<uint32_t>()) return 1;
    {
        // two ranks (on one device): no distributed form, and none emulated
        const std::string text = "mississippi";
        suffix_array<char, uint64_t, true> sa((psacx::comm(std::vector<int>(2, 0))));
        sa.verbose = false;
        sa.construct(text.begin(), text.end());
        bool threw = false;
        try { repeats(sa, text.begin(), text.end()); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "repeats header tests passed" << std::endl;
    return 0;
}
