// lz77 -- the greedy LZ77 factorization of a text on the MI355X engine:
//   lz77 -f <text> [--index 32|64|auto] [-c] [--list] [--device N]
// The text goes up once; SA and LCP are constructed in HBM (psacx_construct_dev_* with PSACX_LCP), the range-minimum index of LCP is
// built beside them (psacx_rmq_index_dev_*), the longest previous factors are found from the three (psacx_lpf_dev_*) and the parse is
// cut from them (psacx_lz77_dev_*).  Prints "z: <phrases> n/z: <mean phrase length>" to stdout and "SA time:" / "Index time:" /
// "LPF time:" / "Parse time: <ms> ms" to stderr.  -c runs the device verdict (psacx_check_lz77_dev_*: the parse decodes to the text),
// prints "errors: <count>" and exits non-zero unless the count is 0.  --list prints one line "start len src" per phrase, "-" as the
// source of a literal.
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "query_cli.hpp"

using namespace query_cli;

static void usage() {
    std::cerr << "USAGE: lz77 -f <text> [--index 32|64|auto] [-c] [--list] [--device N]\n"
                 "Prints the number of phrases z of the greedy LZ77 parse and n / z (MI355X engine).\n"
                 "-c checks on the device that the parse decodes to the text; --list prints \"start len src\" per phrase.\n";
}

static int lpf(psacx_ctx* c, uint64_t n, const uint32_t* sa, const uint32_t* lcp, const uint32_t* index, uint32_t* l, uint32_t* s) { return psacx_lpf_dev_u32(c, n, sa, lcp, index, l, s); }
static int lpf(psacx_ctx* c, uint64_t n, const uint64_t* sa, const uint64_t* lcp, const uint64_t* index, uint64_t* l, uint64_t* s) { return psacx_lpf_dev_u64(c, n, sa, lcp, index, l, s); }
static int parse(psacx_ctx* c, uint64_t n, const uint32_t* l, const uint32_t* s, uint32_t* start, uint32_t* psrc, uint64_t cap, uint64_t* z) { return psacx_lz77_dev_u32(c, n, l, s, start, psrc, cap, z); }
static int parse(psacx_ctx* c, uint64_t n, const uint64_t* l, const uint64_t* s, uint64_t* start, uint64_t* psrc, uint64_t cap, uint64_t* z) { return psacx_lz77_dev_u64(c, n, l, s, start, psrc, cap, z); }
static int verdict(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* start, const uint32_t* psrc, uint64_t z, uint64_t* e) { return psacx_check_lz77_dev_u32(c, t, n, start, psrc, z, e); }
static int verdict(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* start, const uint64_t* psrc, uint64_t z, uint64_t* e) { return psacx_check_lz77_dev_u64(c, t, n, start, psrc, z, e); }

template <typename IT>
static int run(const std::string& text, bool check, bool list, int device) {
    const uint64_t n = text.size();
    Session s(device);
    psacx_ctx* const c = s.c;
    int rc = 0;
    auto t0 = std::chrono::steady_clock::now();
    uint8_t* d_text = (uint8_t*)s.dev(n);
    IT* d_sa = (IT*)s.dev(n * sizeof(IT));
    IT* d_isa = (IT*)s.dev(n * sizeof(IT));
    IT* d_lcp = (IT*)s.dev(n * sizeof(IT));
    must(c, psacx_copy_h2d(c, d_text, text.data(), n));
    must(c, construct(c, d_text, n, nullptr, 0, PSACX_LCP, d_sa, d_isa, d_lcp));
    std::cerr << "SA time: " << ms_since(t0) << " ms" << std::endl;
    auto t1 = std::chrono::steady_clock::now();
    uint64_t entries = 0;
    IT* d_index = rmq_index_of<IT>(s, d_lcp, n, &entries);
    std::cerr << "Index time: " << ms_since(t1) << " ms" << std::endl;
    IT* d_lpf = d_isa;                                             // ISA is not needed any more
    IT* d_src = (IT*)s.dev(n * sizeof(IT));
    auto t2 = std::chrono::steady_clock::now();
    must(c, lpf(c, n, d_sa, d_lcp, d_index, d_lpf, d_src));
    std::cerr << "LPF time: " << ms_since(t2) << " ms" << std::endl;
    auto t3 = std::chrono::steady_clock::now();
    uint64_t z = 0;
    must(c, parse(c, n, d_lpf, d_src, (IT*)nullptr, (IT*)nullptr, 0, &z));
    IT* d_start = (IT*)s.dev((z + 1) * sizeof(IT));
    IT* d_psrc = (IT*)s.dev((z + 1) * sizeof(IT));
    must(c, parse(c, n, d_lpf, d_src, d_start, d_psrc, z + 1, &z));
    std::cerr << "Parse time: " << ms_since(t3) << " ms" << std::endl;
    std::cout << "z: " << z << " n/z: " << (double)n / (double)z << '\n';
    if (check) {
        uint64_t errors = 0;
        must(c, verdict(c, d_text, n, d_start, d_psrc, z, &errors));
        std::cout << "errors: " << errors << '\n';
        if (errors) rc = EXIT_FAILURE;
    }
    if (list) {
        std::vector<IT> start(z + 1), psrc(z + 1);
        must(c, psacx_copy_d2h(c, start.data(), d_start, (z + 1) * sizeof(IT)));
        must(c, psacx_copy_d2h(c, psrc.data(), d_psrc, z * sizeof(IT)));
        for (uint64_t k = 0; k < z; ++k) {
            std::cout << (uint64_t)start[k] << ' ' << (uint64_t)(start[k + 1] - start[k]) << ' ';
            if (psrc[k] == (IT)~(IT)0) std::cout << "-\n"; else std::cout << (uint64_t)psrc[k] << '\n';
        }
    }
    return rc;
}

int main(int argc, char** argv) {
    std::string file, index = "auto";
    int device = 0;
    bool check = false, list = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { std::cerr << "error: missing value for " << name << std::endl; usage(); exit(EXIT_FAILURE); }
            return argv[++i];
        };
        if (a == "-f" || a == "--file") file = need("-f");
        else if (a == "-c" || a == "--check") check = true;
        else if (a == "--list") list = true;
        else if (a == "--device") device = atoi(need("--device"));
        else if (a == "--index") index = need("--index");
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { std::cerr << "error: unknown argument " << a << std::endl; usage(); return EXIT_FAILURE; }
    }
    if (file.empty() || !index_known(index)) { usage(); return EXIT_FAILURE; }
    std::string text;
    if (!read_file(file, text)) { std::cerr << "error: cannot open " << file << std::endl; return EXIT_FAILURE; }
    if (text.empty()) { std::cerr << "error: empty input" << std::endl; return EXIT_FAILURE; }
    const bool narrow = use32(index, text.size());
    try {
        const int rc = narrow ? run<uint32_t>(text, check, list, device) : run<uint64_t>(text, check, list, device);
        std::cout.flush();
        if (!std::cout) { std::cerr << "error: cannot write the results" << std::endl; return EXIT_FAILURE; }
        return rc;
    } catch (const std::exception& ex) {
        std::cerr << "error: " << ex.what() << std::endl;
        return EXIT_FAILURE;
    }
}
