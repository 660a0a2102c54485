// kmismatch(...) of include/suffix_array.hpp on "mississippi" and the set {abcab, cab}: the lists stated here by hand
// (tests/test_kmismatch_model_cpu.py holds the same ones to the model), for both index types, and the refusals.
// Built by tests/test_kmismatch_build_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_kmismatch.py.
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
        try { kmismatch(sa, text.begin(), text.end(), pats, 1); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
        sa.construct(text.begin(), text.end());
        mismatch_lists<index_t> r = kmismatch(sa, text.begin(), text.end(), pats, 0);
        // issi at 4 and 1 (issippi sorts before ississippi), m at 0, sip at 6
        CHECK(r.qid == q({0, 0, 2, 4}) && r.tpos == v({4, 1, 0, 6}) && r.dist == d({0, 0, 0, 0}));
        r = kmismatch(sa, text.begin(), text.end(), pats, 1);
        // ssippx is ssippi at 5; sip is sis at 3, found from its piece s after the exact one; m is shorter than e + 1
        CHECK(r.qid == q({0, 0, 1, 4, 4}) && r.tpos == v({4, 1, 5, 6, 3}) && r.dist == d({0, 0, 1, 0, 1}));
        r = kmismatch(sa, text.begin(), text.end(), pats, 1, 2);    // the same behind a table of 2-mers
        CHECK(r.qid == q({0, 0, 1, 4, 4}) && r.tpos == v({4, 1, 5, 6, 3}) && r.dist == d({0, 0, 1, 0, 1}));
        CHECK(kmismatch(sa, text.begin(), text.end(), pats, 2).qid.size() == 10);
        CHECK(kmismatch(sa, text.begin(), text.end(), std::vector<std::string>(), 1).qid.empty());
        bool refused = false;                                       // more than 15 mismatches
        try { kmismatch(sa, text.begin(), text.end(), pats, 16); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
        refused = false;                                            // a text of another length
        const std::string other = "mississipp";
        try { kmismatch(sa, other.begin(), other.end(), pats, 1); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
    }
    {
        const std::string flat = "abcab$cab";                       // suffixes ab(3) ab(6) abcab(0) b(4) b(7) bcab(1) cab(2) cab(5)
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        sa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("abc")));
        std::vector<std::string> pats;
        pats.push_back("cab"); pats.push_back("abc"); pats.push_back("bc"); pats.push_back("cb"); pats.push_back("abcabc");
        mismatch_lists<index_t> r = kmismatch(sa, ss, pats, 0);
        // bc at 1 only: the bytes at 4 and 5 belong to two strings; abcabc would be the two strings laid together
        CHECK(r.qid == q({0, 0, 1, 2}) && r.tpos == v({2, 5, 0, 1}) && r.dist == d({0, 0, 0, 0}));
        r = kmismatch(sa, ss, pats, 1);
        // cb: ca at 2 and 5 from the piece c, then ab at 3, 6 and 0 from the piece b
        CHECK(r.qid == q({0, 0, 1, 2, 3, 3, 3, 3, 3}) && r.tpos == v({2, 5, 0, 1, 2, 5, 3, 6, 0}) && r.dist == d({0, 0, 0, 0, 1, 1, 1, 1, 1}));
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
        try { kmismatch(sa, text.begin(), text.end(), std::vector<std::string>(1, "sip"), 1); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "kmismatch header tests passed" << std::endl;
    return 0;
}
