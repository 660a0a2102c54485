// overlaps -- the suffix-prefix overlaps of a set of reads on the MI355X engine:
//   overlaps -f <reads> [-l MINLEN] [--whole] [--list [LIMIT]] [--index 32|64|auto] [--device N] [-o file]
// The strings are the lines of -f, as gsac reads them.  They go up once; SA, ISA and LCP are constructed in HBM
// (psacx_construct_gsa_dev_* with PSACX_LCP), the range-minimum index of LCP and the bitmap of the string ends are built beside
// them (psacx_rmq_index_dev_*, psacx_string_ends_dev), and one call walks every string (psacx_overlaps_dev_*).  Prints
// "slots: <non-empty slots> pairs: <overlaps>" and "SA time:" / "Index time:" / "Overlaps time: <ms> ms" to stderr.
// --list runs psacx_occurrences_dev_* over the result (at most LIMIT sources per target and length) and prints one line
// "target source length" per overlap to stdout or the file of -o: the last `length` bytes of string `source` are the first
// `length` bytes of string `target`.  A string overlaps itself where it has a border.  --whole also asks for length = the
// whole target: the strings that end with it, itself among them.
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
    std::cerr << "USAGE: overlaps -f <reads, one per line> [-l MINLEN] [--whole] [--list [LIMIT]] [--index 32|64|auto] [--device N] [-o <file>]\n"
                 "Finds every suffix of a read that is a prefix of a read, MINLEN bytes (default 1) or longer (MI355X engine).\n"
                 "--list prints \"target source length\" per overlap; --whole includes overlaps as long as the whole target.\n";
}

static int overlaps(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* ends, const uint32_t* sa, const uint32_t* isa, const uint32_t* lcp,
                    const uint32_t* index, uint64_t l, uint32_t f, uint32_t* lb, uint32_t* ub) {
    return psacx_overlaps_dev_u32(c, n, off, m, ends, sa, isa, lcp, index, l, f, lb, ub);
}
static int overlaps(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* ends, const uint64_t* sa, const uint64_t* isa, const uint64_t* lcp,
                    const uint64_t* index, uint64_t l, uint32_t f, uint64_t* lb, uint64_t* ub) {
    return psacx_overlaps_dev_u64(c, n, off, m, ends, sa, isa, lcp, index, l, f, lb, ub);
}

template <typename IT>
static int run(const std::string& text, const std::vector<uint64_t>& soff, uint64_t min_len, bool whole, bool list, uint64_t limit, int device,
               std::ostream& out) {
    const uint64_t n = text.size(), m = soff.size() - 1;
    Session s(device);
    psacx_ctx* const c = s.c;
    auto t0 = std::chrono::steady_clock::now();
    uint8_t* d_text = (uint8_t*)s.dev(n);
    IT* d_sa = (IT*)s.dev(n * sizeof(IT));
    IT* d_isa = (IT*)s.dev(n * sizeof(IT));
    IT* d_lcp = (IT*)s.dev(n * sizeof(IT));
    uint64_t* d_soff = (uint64_t*)s.dev((m + 1) * sizeof(uint64_t));
    must(c, psacx_copy_h2d(c, d_text, text.data(), n));
    must(c, psacx_copy_h2d(c, d_soff, soff.data(), (m + 1) * sizeof(uint64_t)));
    must(c, construct(c, d_text, n, d_soff, m, PSACX_LCP, d_sa, d_isa, d_lcp));
    std::cerr << "SA time: " << ms_since(t0) << " ms" << std::endl;
    auto t1 = std::chrono::steady_clock::now();
    uint64_t entries = 0, words = 0;
    IT* d_index = rmq_index_of<IT>(s, d_lcp, n, &entries);
    must(c, psacx_string_ends_dev(c, nullptr, m, n, nullptr, &words));
    uint32_t* d_ends = (uint32_t*)s.dev(words * sizeof(uint32_t));
    must(c, psacx_string_ends_dev(c, d_soff, m, n, d_ends, &words));
    std::cerr << "Index time: " << ms_since(t1) << " ms" << std::endl;
    IT* d_lb = (IT*)s.dev(n * sizeof(IT));
    IT* d_ub = (IT*)s.dev(n * sizeof(IT));
    auto t2 = std::chrono::steady_clock::now();
    must(c, overlaps(c, n, d_soff, m, d_ends, d_sa, d_isa, d_lcp, d_index, min_len, whole ? PSACX_OVERLAP_WHOLE : 0u, d_lb, d_ub));
    std::cerr << "Overlaps time: " << ms_since(t2) << " ms" << std::endl;
    std::vector<IT> lb(n), ub(n);
    must(c, psacx_copy_d2h(c, lb.data(), d_lb, n * sizeof(IT)));
    must(c, psacx_copy_d2h(c, ub.data(), d_ub, n * sizeof(IT)));
    uint64_t slots = 0, pairs = 0;
    for (uint64_t p = 0; p < n; ++p) if (ub[p] > lb[p]) { ++slots; pairs += (uint64_t)(ub[p] - lb[p]); }
    std::cerr << "slots: " << slots << " pairs: " << pairs << std::endl;
    if (list) {
        auto t3 = std::chrono::steady_clock::now();
        uint64_t* d_start = (uint64_t*)s.dev((n + 1) * sizeof(uint64_t));
        uint64_t total = 0;
        must(c, occurrences(c, d_sa, n, d_soff, m, d_lb, d_ub, n, limit, d_start, (IT*)nullptr, (IT*)nullptr, 0, &total));
        IT* d_pos = (IT*)s.dev(total * sizeof(IT));
        IT* d_sid = (IT*)s.dev(total * sizeof(IT));
        must(c, occurrences(c, d_sa, n, d_soff, m, d_lb, d_ub, n, limit, d_start, d_pos, d_sid, total, &total));
        std::cerr << "List time: " << ms_since(t3) << " ms" << std::endl;
        std::vector<uint64_t> start(n + 1);
        std::vector<IT> sid(total);
        must(c, psacx_copy_d2h(c, start.data(), d_start, (n + 1) * sizeof(uint64_t)));
        if (total) must(c, psacx_copy_d2h(c, sid.data(), d_sid, total * sizeof(IT)));
        uint64_t j = 0;
        for (uint64_t p = 0; p < n; ++p) {                         // slot p = o_j + d - 1
            while (soff[j + 1] <= p) ++j;
            for (uint64_t t = start[p]; t < start[p + 1]; ++t) out << j << ' ' << (uint64_t)sid[t] << ' ' << (p - soff[j] + 1) << '\n';
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    std::string file, outfile, index = "auto";
    int device = 0;
    bool whole = false, list = false;
    unsigned long long min_len = 1, limit = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { std::cerr << "error: missing value for " << name << std::endl; usage(); exit(EXIT_FAILURE); }
            return argv[++i];
        };
        if (a == "-f" || a == "--file") file = need("-f");
        else if (a == "-l" || a == "--min-len") {
            const char* w = need("-l");
            if (!number(w)) { std::cerr << "error: " << w << " is no length" << std::endl; return EXIT_FAILURE; }
            min_len = strtoull(w, nullptr, 10);
        }
        else if (a == "--whole") whole = true;
        else if (a == "--list") { list = true; if (i + 1 < argc && number(argv[i + 1])) limit = strtoull(argv[++i], nullptr, 10); }
        else if (a == "-o" || a == "--outfile") outfile = need("-o");
        else if (a == "--device") device = atoi(need("--device"));
        else if (a == "--index") index = need("--index");
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { std::cerr << "error: unknown argument " << a << std::endl; usage(); return EXIT_FAILURE; }
    }
    if (file.empty() || !index_known(index)) { usage(); return EXIT_FAILURE; }
    if (min_len == 0) { std::cerr << "error: the minimum length must be at least 1" << std::endl; return EXIT_FAILURE; }
    std::string raw, text;
    if (!read_file(file, raw)) { std::cerr << "error: cannot open " << file << std::endl; return EXIT_FAILURE; }
    std::vector<uint64_t> soff;
    split_lines(raw, text, soff);
    if (text.empty()) { std::cerr << "error: empty input" << std::endl; return EXIT_FAILURE; }
    const bool narrow = use32(index, text.size());
    try {
        std::ofstream f;
        if (!outfile.empty()) {
            f.open(outfile.c_str(), std::ios::trunc);
            if (!f) { std::cerr << "error: cannot write " << outfile << std::endl; return EXIT_FAILURE; }
        }
        std::ostream& out = outfile.empty() ? std::cout : f;
        const int rc = narrow ? run<uint32_t>(text, soff, min_len, whole, list, limit, device, out) : run<uint64_t>(text, soff, min_len, whole, list, limit, device, out);
        out.flush();
        if (!out) { std::cerr << "error: cannot write the results" << std::endl; return EXIT_FAILURE; }
        return rc;
    } catch (const std::exception& ex) {
        std::cerr << "error: " << ex.what() << std::endl;
        return EXIT_FAILURE;
    }
}
