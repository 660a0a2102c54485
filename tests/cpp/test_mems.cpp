// mems(...) of include/suffix_array.hpp on "mississippi" and the set {abcab, cab}: the lists stated here by hand
// (tests/test_mems_model_cpu.py holds the same ones to the model), for both index types, and the refusals.
// Built by tests/test_mems_build_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_mems.py.
#include <iostream>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank() {
    typedef std::vector<index_t> v;
    typedef std::vector<uint64_t> q;
    suffix_array<char, index_t, true> sa((psacx::comm(0)));
    sa.verbose = false;
    {
        const std::string text = "mississippi";
        std::vector<std::string> pats;
        pats.push_back("ississim"); pats.push_back("sip");         // slots 0-7 and 8-10
        bool threw = false;                                         // nothing constructed
        try { mems(sa, text.begin(), text.end(), pats, 3); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
        sa.construct(text.begin(), text.end());
        mem_lists<index_t> r = mems(sa, text.begin(), text.end(), pats, 3);
        // ississi at 1, issi at 4 (left of it s, in the pattern nothing), issi of slot 3 at 1 (left m against s), sip at 6
        CHECK(r.qpos == q({0, 0, 3, 8}) && r.tpos == v({1, 4, 1, 6}) && r.len == v({7, 4, 4, 3}));
        r = mems(sa, text.begin(), text.end(), pats, 3, 2);         // the same behind a table of 2-mers
        CHECK(r.qpos == q({0, 0, 3, 8}) && r.tpos == v({1, 4, 1, 6}) && r.len == v({7, 4, 4, 3}));
        r = mems(sa, text.begin(), text.end(), pats, 2);
        CHECK(r.qpos == q({0, 0, 3, 8, 8}) && r.tpos == v({1, 4, 1, 6, 3}) && r.len == v({7, 4, 4, 3, 2}));
        CHECK(mems(sa, text.begin(), text.end(), pats, 1).qpos.size() == 24);
        CHECK(mems(sa, text.begin(), text.end(), pats, 0).qpos.size() == 24);
        r = mems(sa, text.begin(), text.end(), pats, 3, 0, 1);      // unique in the text: issi occurs twice
        CHECK(r.qpos == q({0, 8}) && r.tpos == v({1, 6}) && r.len == v({7, 3}));
        r = mems(sa, text.begin(), text.end(), pats, 1, 0, 0, true);
        CHECK(r.qpos == q({0, 7, 8}) && r.tpos == v({1, 0, 6}) && r.len == v({7, 1, 3}));
        CHECK(mems(sa, text.begin(), text.end(), std::vector<std::string>(), 1).qpos.empty());
        bool refused = false;                                       // a text of another length
        const std::string other = "mississipp";
        try { mems(sa, other.begin(), other.end(), pats, 1); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
    }
    {
        const std::string flat = "abcab$cab";                       // suffixes ab(3) ab(6) abcab(0) b(4) b(7) bcab(1) cab(2) cab(5)
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        sa.construct_ss(ss, psacx::alphabet<char>::from_string(std::string("abc")));
        std::vector<std::string> pats;
        pats.push_back("bcabc"); pats.push_back(""); pats.push_back("ca");
        mem_lists<index_t> r = mems(sa, ss, pats, 2);
        // bcab at 1; cab of slot 1 at 5, where a string starts; abc at 0; ca at 2 and at 5
        CHECK(r.qpos == q({0, 1, 2, 5, 5}) && r.tpos == v({1, 5, 0, 2, 5}) && r.len == v({4, 3, 3, 2, 2}));
        r = mems(sa, ss, pats, 2, 0, 0, true);
        CHECK(r.qpos == q({0, 2, 5, 5}) && r.tpos == v({1, 0, 2, 5}) && r.len == v({4, 3, 2, 2}));
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
        try { mems(sa, text.begin(), text.end(), std::vector<std::string>(1, "sip"), 1); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "mems header tests passed" << std::endl;
    return 0;
}
