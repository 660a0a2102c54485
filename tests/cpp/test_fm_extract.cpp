// fm_index<index_t> of include/suffix_array.hpp with text samples, on mississippi and on the set {mississippi, missouri, miss}: the text
// back from the index after the suffix array is gone, windows clipped at their string's end, for both index types and three rates, and
// the refusal of an index built without text samples.
// Built by tests/test_fm_extract_model_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_fm_extract.py.
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

static std::string str(const std::vector<uint8_t>& v) { return std::string(v.begin(), v.end()); }

template <typename index_t>
static int one_rank(std::size_t rate) {
    typedef std::vector<index_t> v;
    typedef std::vector<std::size_t> vs;
    {
        const std::string text = "mississippi";
        std::unique_ptr<suffix_array<char, index_t, false> > sa(new suffix_array<char, index_t, false>(psacx::comm(0)));
        sa->verbose = false;
        sa->construct(text.begin(), text.end());
        fm_index<index_t> fm(*sa, text.begin(), text.end(), 2, rate);
        fm_index<index_t> plain(*sa, text.begin(), text.end(), 2);
        sa.reset();                                                 // the index answers without the suffix array and the text
        CHECK(fm.bytes() == plain.bytes() + (11 / rate + 1) * sizeof(index_t));
        CHECK(fm.text() == std::vector<std::string>(1, text));
        vs start;
        const std::vector<uint8_t> out = fm.extract(v({0, 4, 10, 9, 11, 3}), v({4, 3, 5, 0, 2, 100}), start);
        CHECK(start == vs({0, 4, 7, 8, 8, 8, 16}));
        CHECK(str(out) == "mississi" "sissippi");
        bool refused = false;                                       // no text samples
        try { plain.text(); } catch (const std::runtime_error&) { refused = true; }
        CHECK(refused);
    }
    {
        const std::string flat = "mississippi$missouri$miss";
        simple_dstringset ss(flat.begin(), flat.end(), psacx::comm(0));
        std::unique_ptr<suffix_array<char, index_t, false> > sa(new suffix_array<char, index_t, false>(psacx::comm(0)));
        sa->verbose = false;
        sa->construct_ss(ss, psacx::alphabet<char>::from_string(std::string("imoprsu")));
        fm_index<index_t> fm(*sa, ss, 3, rate);
        sa.reset();
        std::vector<std::string> want;
        want.push_back("mississippi"); want.push_back("missouri"); want.push_back("miss");
        CHECK(fm.text() == want);
        vs start;                                                   // positions count the strings back to back; every window ends with its string
        const std::vector<uint8_t> out = fm.extract(v({8, 10, 11, 15, 19, 22, 23}), v({9, 1, 8, 100, 2, 7, 1}), start);
        CHECK(start == vs({0, 3, 4, 12, 16, 18, 19, 19}));
        CHECK(str(out) == "ppi" "i" "missouri" "ouri" "mi" "s");
    }
    return 0;
}

int main() {
    for (std::size_t rate = 1; rate <= 4; rate += (rate == 1 ? 2 : 1))          // 1, 3, 4
        if (one_rank<uint64_t>(rate) || one_rank<uint32_t>(rate)) return 1;
    if (one_rank<uint32_t>(40)) return 1;                            // above n: the end samples alone
    std::cout << "fm extract header tests passed" << std::endl;
    return 0;
}
