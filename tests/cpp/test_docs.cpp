// doc_count(...), doc_list(...) and common_repeats(...) of include/suffix_array.hpp on the sets {mississippi, missouri, miss} and
// {abab, ab}: the counts and lists stated here by hand (tests/golden/docs_named.json and tests/test_docs_model_cpu.py hold the same ones to
// the model), for both index types, and the refusals.
// Built by tests/test_docs_build_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_docs.py.
#include <iostream>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank() {
    typedef std::vector<index_t> v;
    typedef std::vector<std::size_t> vs;
    suffix_array<char, index_t, true> sa((psacx::comm(0)));
    sa.verbose = false;
    {
        // SA 10 18 7 20 4 1 12 19 0 11 15 9 8 17 22 6 3 14 21 5 2 13 16 (positions count the strings back to back)
        const std::string flat = "mississippi$missouri$miss";
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        sa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("imoprsu")));
        // the locate intervals of miss, ss, i, ssi, ouri, s, and one that is empty
        const v lb({7, 18, 0, 19, 10, 14, 0}), ub({10, 22, 7, 21, 11, 22, 0});
        CHECK(doc_count(sa, ss, lb, ub) == v({3, 3, 3, 1, 1, 3, 0}));                        // ssi occurs twice, in one string
        const doc_lists<index_t> l = doc_list(sa, ss, lb, ub);
        CHECK(l.start == vs({0, 3, 6, 9, 10, 11, 14, 14}));
        CHECK(l.sid == v({2, 0, 1, 2, 0, 1, 0, 1, 2, 0, 1, 2, 0, 1}));
        CHECK(l.pos == v({19, 0, 11, 21, 5, 13, 10, 18, 20, 5, 15, 22, 6, 14}));
        // singletons, the whole array, and an arbitrary interval through the list
        CHECK(doc_count(sa, ss, v({0, 22, 0}), v({1, 23, 23})) == v({1, 1, 3}));
        const doc_lists<index_t> a = doc_list(sa, ss, v({3, 9}), v({9, 3}));
        CHECK(a.start == vs({0, 3, 3}) && a.sid == v({2, 0, 1}) && a.pos == v({20, 4, 12}));   // ranks 3, 4, 6; lb > ub counts 0
        // the right-maximal repeats common to all three strings: i, iss, miss, s, ss; the longest is miss
        const common_repeat_intervals<index_t> c = common_repeats(sa, ss, 3);
        CHECK(c.lb == v({0, 3, 7, 14, 18}) && c.ub == v({7, 7, 10, 22, 22}) && c.len == v({1, 3, 4, 1, 2}) && c.docs == v({3, 3, 3, 3, 3}));
        const common_repeat_intervals<index_t> one = common_repeats(sa, ss, 1, 1);
        CHECK(one.lb == v({4, 11, 15, 19}) && one.len == v({4, 1, 2, 3}) && one.docs == v({1, 1, 1, 1}));      // issi, p, si, ssi
        CHECK(common_repeats(sa, ss, 3, 0, repeats_right, 4).len == v({4}));
        bool refused = false;                                       // more ranks than max_cand
        try { doc_list(sa, ss, lb, ub, 5); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
        refused = false;                                            // lb and ub of different lengths
        try { doc_count(sa, ss, v({0}), v({1, 2})); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
        const std::string other = "ab$ab";                          // another set
        simple_dstringset ss2(other.begin(), other.end(), psacx::comm(0));
        refused = false;
        try { doc_count(sa, ss2, v({0}), v({1})); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
    }
    {
        // {abab, ab}: SA 2 4 0 3 5 1, LCP 0 2 2 0 1 1.  [0, 2) holds the suffixes that ARE ab (an interval of overlaps()): no LCP-interval,
        // the count formula gives 1 there and the list gives both strings
        const std::string flat = "abab$ab";
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        sa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("ab")));
        CHECK(doc_count(sa, ss, v({0, 0}), v({3, 2})) == v({2, 1}));
        const doc_lists<index_t> l = doc_list(sa, ss, v({0}), v({2}));
        CHECK(l.start == vs({0, 2}) && l.sid == v({0, 1}) && l.pos == v({2, 4}));
    }
    {
        suffix_array<char, index_t, false> plain((psacx::comm(0)));  // no LCP: the lists alone
        plain.verbose = false;
        const std::string flat = "abab$ab";
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        plain.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("ab")));
        const doc_lists<index_t> l = doc_list(plain, ss, v({0, 3}), v({6, 6}));
        CHECK(l.start == vs({0, 2, 4}) && l.sid == v({0, 1, 0, 1}) && l.pos == v({2, 4, 3, 5}));
    }
    return 0;
}

int main() {
    if (one_rank<uint64_t>() || one_rank<uint32_t>()) return 1;
    std::cout << "docs header tests passed" << std::endl;
    return 0;
}
