// lz77(sa) of include/suffix_array.hpp on "mississippi", 300 times 'a' and ("ab" x 50) "c" ("ab" x 50): the phrases stated here by
// hand (tests/test_lz_build_cpu.py holds them to the model), for both index types, decoded again, and the refusals.
// Built by tests/test_lz_build_cpu.py (no GPU: it must end with the library's error) and run by tests/test_gpu_lz77.py.
#include <iostream>
#include <string>
#include <vector>

#include "../../include/suffix_array.hpp"

#define CHECK(x) do { if (!(x)) { std::cerr << "FAILED: " #x " at line " << __LINE__ << std::endl; return 1; } } while (0)

template <typename index_t>
static std::string decode(const lz_factors<index_t>& f, const std::string& text) {
    std::string out;
    for (std::size_t k = 0; k + 1 < f.start.size(); ++k) {
        const std::size_t len = (std::size_t)(f.start[k + 1] - f.start[k]);
        if (f.src[k] == (index_t)~(index_t)0) out.push_back(text[(std::size_t)f.start[k]]);
        else for (std::size_t t = 0; t < len; ++t) out.push_back(out[(std::size_t)f.src[k] + t]);
    }
    return out;
}

template <typename index_t>
static int one_rank() {
    typedef std::vector<index_t> v;
    const index_t lit = (index_t)~(index_t)0;
    suffix_array<char, index_t, true> sa((psacx::comm(0)));
    sa.verbose = false;
    {
        bool threw = false;                                         // nothing constructed: no LCP to parse from
        try { lz77(sa); } catch (const std::runtime_error&) { threw = true; }
        CHECK(threw);
    }
    {
        const std::string text = "mississippi";
        sa.construct(text.begin(), text.end());
        const lz_factors<index_t> f = lz77(sa);
        // m i s (s from 2) (issi from 1) p (p from 8) (i from 7)
        CHECK(f.start == v({0, 1, 2, 3, 4, 8, 9, 10, 11}));
        CHECK(f.src == v({lit, lit, lit, 2, 1, lit, 8, 7}));
        CHECK(decode(f, text) == text);
    }
    {
        const std::string text(300, 'a');                           // (a second construct on the same object, as the reference's tests do)
        sa.construct(text.begin(), text.end());
        const lz_factors<index_t> f = lz77(sa);
        CHECK(f.start == v({0, 1, 300}));                           // the second phrase copies 299 bytes from 0: it overlaps itself
        CHECK(f.src == v({lit, 0}));
        CHECK(decode(f, text) == text);
    }
    {
        std::string half;
        for (int i = 0; i < 50; ++i) half += "ab";
        const std::string text = half + "c" + half;
        sa.construct(text.begin(), text.end());
        const lz_factors<index_t> f = lz77(sa);
        CHECK(f.start == v({0, 1, 2, 100, 101, 201}));
        CHECK(f.src == v({lit, lit, 0, lit, 0}));
        CHECK(decode(f, text) == text);
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
        try { lz77(sa); }
        catch (const std::runtime_error& e) { threw = std::string(e.what()).find("single-rank") != std::string::npos; }
        CHECK(threw);
    }
    std::cout << "lz77 header tests passed" << std::endl;
    return 0;
}
