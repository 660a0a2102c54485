// kedit(...) of include/suffix_array.hpp on "mississippi" and the set {abcab, cab}: the lists stated here by hand
// (tests/test_kedit_build_cpu.py holds the same ones to the model), for both index types, and the refusals.
// Built by tests/test_kedit_build_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_kedit.py.
#include <iostream>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank() {
    typedef std::vector<index_t> v;
    typedef std::vector<uint64_t> q;
    typedef std::vector<uint8_t> d;
    suffix_array<char, index_t, true> sa((psacx::comm(0)));
    sa.verbose = false;
    {
        const std::string text = "mississippi";
        std::vector<std::string> pats;
        pats.push_back("issi"); pats.push_back("ssippx"); pats.push_back("m"); pats.push_back(""); pats.push_back("sip");
        bool threw = false;                                         // nothing constructed
        try { kedit(sa, text.begin(), text.end(), pats, 1); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
        sa.construct(text.begin(), text.end());
        edit_lists<index_t> r = kedit(sa, text.begin(), text.end(), pats, 0);
        // no edits: the occurrences by position; issi at 1 and 4, m at 0, sip at 6
        CHECK(r.qid == q({0, 0, 2, 4}) && r.tpos == v({1, 4, 0, 6}) && r.len == v({4, 4, 1, 3}) && r.dist == d({0, 0, 0, 0}));
        r = kedit(sa, text.begin(), text.end(), pats, 1);
        // issi: missi at 0, ssi at 2 and 5, sissi at 3 beside the exact ones; ssippx is ssipp at 5; sip: si at 3 and 7, ssip at 5;
        // m and the empty pattern have at most e bytes
        CHECK(r.qid == q({0, 0, 0, 0, 0, 0, 1, 4, 4, 4, 4}) && r.tpos == v({0, 1, 2, 3, 4, 5, 5, 3, 5, 6, 7}));
        CHECK(r.len == v({5, 4, 3, 5, 4, 3, 5, 2, 4, 3, 2}) && r.dist == d({1, 0, 1, 1, 0, 1, 1, 1, 1, 0, 1}));
        edit_lists<index_t> t2 = kedit(sa, text.begin(), text.end(), pats, 1, 2);   // the same behind a table of 2-mers
        CHECK(t2.qid == r.qid && t2.tpos == r.tpos && t2.len == r.len && t2.dist == r.dist);
        r = kedit(sa, text.begin(), text.end(), pats, 1, 0, true);  // the best of every pattern
        CHECK(r.qid == q({0, 0, 1, 4}) && r.tpos == v({1, 4, 5, 6}) && r.len == v({4, 4, 5, 3}) && r.dist == d({0, 0, 1, 0}));
        CHECK(kedit(sa, text.begin(), text.end(), pats, 2).qid.size() == 22);
        CHECK(kedit(sa, text.begin(), text.end(), std::vector<std::string>(), 1).qid.empty());
        bool refused = false;                                       // more than 15 edits
        try { kedit(sa, text.begin(), text.end(), pats, 16); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
        refused = false;                                            // a text of another length
        const std::string other = "mississipp";
        try { kedit(sa, other.begin(), other.end(), pats, 1); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
    }
    {
        const std::string flat = "abcab$cab";                       // the strings abcab at 0 and cab at 5
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        sa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("abc")));
        std::vector<std::string> pats;
        pats.push_back("cab"); pats.push_back("abc"); pats.push_back("bc"); pats.push_back("cb"); pats.push_back("abcabc");
        edit_lists<index_t> r = kedit(sa, ss, pats, 0);
        // bc at 1 only: the bytes at 4 and 5 belong to two strings; abcabc would be the two strings laid together
        CHECK(r.qid == q({0, 0, 1, 2}) && r.tpos == v({2, 5, 0, 1}) && r.len == v({3, 3, 3, 2}) && r.dist == d({0, 0, 0, 0}));
        r = kedit(sa, ss, pats, 1, 0, true);
        // one edit, the best: cb is c or b or ca or ab from every start (all at distance 1); abcabc is the first string whole
        CHECK(r.qid == q({0, 0, 1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4}) && r.tpos == v({2, 5, 0, 1, 0, 1, 2, 3, 4, 5, 6, 7, 0}));
        CHECK(r.len == v({3, 3, 3, 2, 2, 1, 1, 2, 1, 1, 2, 1, 5}) && r.dist == d({0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1}));
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
        try { kedit(sa, text.begin(), text.end(), std::vector<std::string>(1, "sip"), 1); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "kedit header tests passed" << std::endl;
    return 0;
}
