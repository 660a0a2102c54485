// fm_index<index_t> of include/suffix_array.hpp on mississippi and on the set {mississippi, missouri, miss}: the intervals and positions
// stated here by hand (tests/golden/fm_named.json and tests/test_fm_model_cpu.py hold the same ones to the model), for both index types,
// after the suffix array the index came from is gone, and the refusals.
// Built by tests/test_fm_model_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_fm.py.
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static int one_rank() {
    typedef std::vector<index_t> v;
    typedef std::vector<std::size_t> vs;
    typedef std::pair<index_t, index_t> iv;
    std::vector<std::string> pats;
    pats.push_back("iss"); pats.push_back("ippi"); pats.push_back("i"); pats.push_back("x"); pats.push_back(""); pats.push_back("mississippi");
    pats.push_back("im");
    {
        // SA 10 7 4 1 0 9 8 6 3 5 2
        const std::string text = "mississippi";
        std::unique_ptr<suffix_array<char, index_t, false> > sa(new suffix_array<char, index_t, false>(psacx::comm(0)));
        sa->verbose = false;
        sa->construct(text.begin(), text.end());
        fm_index<index_t> fm(*sa, text.begin(), text.end(), 2);
        fm_index<index_t> counting(*sa, text.begin(), text.end(), 0);
        sa.reset();                                                 // the index answers without the suffix array
        const std::vector<iv> c = fm.count(pats);
        CHECK(c[0] == iv(2, 4) && c[1] == iv(1, 2) && c[2] == iv(0, 4) && c[3] == iv(0, 0) && c[4] == iv(0, 11) && c[5] == iv(4, 5) && c[6] == iv(0, 0));
        CHECK(counting.count(pats) == c);
        CHECK(counting.bytes() < fm.bytes() && fm.size() == 11);
        const occurrence_lists<index_t> l = fm.locate(pats);
        CHECK(l.start == vs({0, 2, 3, 7, 7, 18, 19, 19}));
        CHECK(l.pos == v({4, 1, 7, 10, 7, 4, 1, 10, 7, 4, 1, 0, 9, 8, 6, 3, 5, 2, 0}));
        CHECK(l.sid.empty());
        const occurrence_lists<index_t> two = fm.locate(pats, 2);
        CHECK(two.start == vs({0, 2, 3, 5, 5, 7, 8, 8}) && two.pos == v({4, 1, 7, 10, 7, 10, 7, 0}));
        bool refused = false;                                       // no samples: counts only
        try { counting.locate(pats); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
    }
    {
        // SA 10 18 7 20 4 1 12 19 0 11 15 9 8 17 22 6 3 14 21 5 2 13 16 (positions count the strings back to back)
        const std::string flat = "mississippi$missouri$miss";
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        std::unique_ptr<suffix_array<char, index_t, false> > sa(new suffix_array<char, index_t, false>(psacx::comm(0)));
        sa->verbose = false;
        sa->construct_ss(ss, psacx::alphabet<char>::from_string(std::string("imoprsu")));
        fm_index<index_t> fm(*sa, ss, 3);
        sa.reset();
        std::vector<std::string> p;
        p.push_back("miss"); p.push_back("ss"); p.push_back("ssi"); p.push_back("ouri"); p.push_back("im"); p.push_back("ssm"); p.push_back("missouri");
        const std::vector<iv> c = fm.count(p);                      // im and ssm would match only across two strings
        CHECK(c[0] == iv(7, 10) && c[1] == iv(18, 22) && c[2] == iv(19, 21) && c[3] == iv(10, 11) && c[4] == iv(0, 0) && c[5] == iv(0, 0) && c[6] == iv(9, 10));
        const occurrence_lists<index_t> l = fm.locate(p);
        CHECK(l.start == vs({0, 3, 7, 9, 10, 10, 10, 11}));
        CHECK(l.pos == v({19, 0, 11, 21, 5, 2, 13, 5, 2, 15, 11}));
        CHECK(l.sid == v({2, 0, 1, 2, 0, 0, 1, 0, 0, 1, 1}));
    }
    return 0;
}

int main() {
    if (one_rank<uint64_t>() || one_rank<uint32_t>()) return 1;
    std::cout << "fm header tests passed" << std::endl;
    return 0;
}
