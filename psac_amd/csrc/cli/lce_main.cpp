// lce -- longest common extensions of pairs of text positions on the MI355X engine:
//   lce -f <text> -p <pairs: "a b" per line> [-e E] [--set] [--index 32|64|auto] [--device N] [-o file]
// The text goes up once; SA, ISA and LCP are constructed in HBM (psacx_construct_dev_* with PSACX_LCP), the range-minimum index
// of LCP is built beside them (psacx_rmq_index_dev_*) and the pairs are answered there (psacx_lce_dev_*).  Prints one length per
// pair -- how far the two positions agree when up to E differing characters are stepped over -- to stdout or the file of -o, and
// "SA time:" / "Index time:" / "LCE time: <ms> ms" to stderr.
// --set reads -f as gsac does: the strings are the runs between '\n' (psacx_construct_gsa_dev_*), and an extension ends where
// either string does.  A position may then also be written string:offset-in-string.
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
    std::cerr << "USAGE: lce -f <text> -p <pairs, \"a b\" per line> [-e E] [--set] [--index 32|64|auto] [--device N] [-o <file>]\n"
                 "Prints for every pair of text positions how far they agree when up to E mismatches are stepped over (MI355X engine).\n"
                 "--set: the strings of -f are its lines, an extension ends with either string, and a position may be string:offset.\n";
}

static int lce(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const uint32_t* isa, const uint32_t* lcp, const uint32_t* index, const uint32_t* a,
               const uint32_t* b, uint64_t q, uint64_t e, uint32_t* len) { return psacx_lce_dev_u32(c, n, off, m, isa, lcp, index, a, b, q, e, len); }
static int lce(psacx_ctx* c, uint64_t n, const uint64_t* off, uint64_t m, const uint64_t* isa, const uint64_t* lcp, const uint64_t* index, const uint64_t* a,
               const uint64_t* b, uint64_t q, uint64_t e, uint64_t* len) { return psacx_lce_dev_u64(c, n, off, m, isa, lcp, index, a, b, q, e, len); }

template <typename IT>
static int run(const std::string& text, const std::vector<uint64_t>& soff, const std::vector<uint64_t>& pa, const std::vector<uint64_t>& pb, uint64_t e,
               int device, std::ostream& out) {
    const uint64_t n = text.size(), q = pa.size(), m = soff.empty() ? 0 : soff.size() - 1;
    const bool set = m != 0;
    const uint64_t top = (uint64_t)(IT)~(IT)0;
    std::vector<IT> a(q), b(q), len(q);
    for (uint64_t i = 0; i < q; ++i) { a[i] = (IT)(pa[i] < top ? pa[i] : top); b[i] = (IT)(pb[i] < top ? pb[i] : top); }     // (beyond n is beyond n)
    Session s(device);
    psacx_ctx* const c = s.c;
    auto t0 = std::chrono::steady_clock::now();
    uint8_t* d_text = (uint8_t*)s.dev(n);
    IT* d_sa = (IT*)s.dev(n * sizeof(IT));
    IT* d_isa = (IT*)s.dev(n * sizeof(IT));
    IT* d_lcp = (IT*)s.dev(n * sizeof(IT));
    uint64_t* d_soff = set ? (uint64_t*)s.dev((m + 1) * sizeof(uint64_t)) : nullptr;
    must(c, psacx_copy_h2d(c, d_text, text.data(), n));
    if (set) must(c, psacx_copy_h2d(c, d_soff, soff.data(), (m + 1) * sizeof(uint64_t)));
    must(c, construct(c, d_text, n, d_soff, m, PSACX_LCP, d_sa, d_isa, d_lcp));
    std::cerr << "SA time: " << ms_since(t0) << " ms" << std::endl;
    auto t1 = std::chrono::steady_clock::now();
    uint64_t entries = 0;
    IT* d_index = rmq_index_of<IT>(s, d_lcp, n, &entries);
    std::cerr << "Index time: " << ms_since(t1) << " ms" << std::endl;
    std::cerr << "Index entries: " << entries << std::endl;
    if (q) {
        IT* d_a = (IT*)s.dev(q * sizeof(IT));
        IT* d_b = (IT*)s.dev(q * sizeof(IT));
        IT* d_len = (IT*)s.dev(q * sizeof(IT));
        must(c, psacx_copy_h2d(c, d_a, a.data(), q * sizeof(IT)));
        must(c, psacx_copy_h2d(c, d_b, b.data(), q * sizeof(IT)));
        auto t2 = std::chrono::steady_clock::now();
        must(c, lce(c, n, d_soff, m, d_isa, d_lcp, d_index, d_a, d_b, q, e, d_len));
        std::cerr << "LCE time: " << ms_since(t2) << " ms" << std::endl;
        must(c, psacx_copy_d2h(c, len.data(), d_len, q * sizeof(IT)));
    }
    for (uint64_t i = 0; i < q; ++i) out << (uint64_t)len[i] << '\n';
    return 0;
}

// "123", or with a set "s:o" = offset o in string s; false if it is neither
static bool position(const std::string& w, const std::vector<uint64_t>& soff, uint64_t& p) {
    if (w.empty()) return false;
    const std::size_t colon = w.find(':');
    const std::string head = w.substr(0, colon), tail = colon == std::string::npos ? std::string() : w.substr(colon + 1);
    if (head.empty() || head.find_first_not_of("0123456789") != std::string::npos) return false;
    if (colon == std::string::npos) { p = strtoull(head.c_str(), nullptr, 10); return true; }
    if (soff.empty() || tail.empty() || tail.find_first_not_of("0123456789") != std::string::npos) return false;
    const uint64_t s = strtoull(head.c_str(), nullptr, 10), o = strtoull(tail.c_str(), nullptr, 10);
    if (s + 1 >= soff.size()) return false;
    p = soff[(std::size_t)s] + o;
    return true;
}

int main(int argc, char** argv) {
    std::string file, pairs, outfile, index = "auto";
    int device = 0;
    bool set = false;
    unsigned long long e = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { std::cerr << "error: missing value for " << name << std::endl; usage(); exit(EXIT_FAILURE); }
            return argv[++i];
        };
        if (a == "-f" || a == "--file") file = need("-f");
        else if (a == "-p" || a == "--pairs") pairs = need("-p");
        else if (a == "-e") e = strtoull(need("-e"), nullptr, 10);
        else if (a == "-o" || a == "--outfile") outfile = need("-o");
        else if (a == "--device") device = atoi(need("--device"));
        else if (a == "--index") index = need("--index");
        else if (a == "--set") set = true;
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { std::cerr << "error: unknown argument " << a << std::endl; usage(); return EXIT_FAILURE; }
    }
    if (file.empty() || pairs.empty() || !index_known(index)) { usage(); return EXIT_FAILURE; }
    std::string text, lines;
    if (!read_file(file, text)) { std::cerr << "error: cannot open " << file << std::endl; return EXIT_FAILURE; }
    if (!read_file(pairs, lines)) { std::cerr << "error: cannot open " << pairs << std::endl; return EXIT_FAILURE; }
    std::vector<uint64_t> soff;
    if (set) { std::string flat; split_lines(text, flat, soff); text.swap(flat); }
    if (text.empty()) { std::cerr << "error: empty input" << std::endl; return EXIT_FAILURE; }
    // one pair per line, two positions separated by blanks; empty lines are skipped
    std::vector<uint64_t> pa, pb;
    uint64_t line_no = 0;
    for (std::size_t b = 0; b < lines.size();) {
        std::size_t en = lines.find('\n', b);
        if (en == std::string::npos) en = lines.size();
        const std::string line = lines.substr(b, en - b);
        b = en + 1;
        ++line_no;
        const std::size_t w0 = line.find_first_not_of(" \t\r");
        if (w0 == std::string::npos) continue;
        const std::size_t w0e = line.find_first_of(" \t", w0);
        const std::size_t w1 = w0e == std::string::npos ? std::string::npos : line.find_first_not_of(" \t", w0e);
        const std::size_t w1e = w1 == std::string::npos ? std::string::npos : line.find_first_of(" \t\r", w1);
        uint64_t x = 0, y = 0;
        if (w1 == std::string::npos || !position(line.substr(w0, w0e - w0), soff, x) ||
            !position(line.substr(w1, w1e == std::string::npos ? std::string::npos : w1e - w1), soff, y)) {
            std::cerr << "error: line " << line_no << " of " << pairs << " is no pair of positions" << std::endl;
            return EXIT_FAILURE;
        }
        pa.push_back(x);
        pb.push_back(y);
    }
    const bool narrow = use32(index, text.size());
    try {
        std::ofstream f;
        if (!outfile.empty()) {
            f.open(outfile.c_str(), std::ios::trunc);
            if (!f) { std::cerr << "error: cannot write " << outfile << std::endl; return EXIT_FAILURE; }
        }
        std::ostream& out = outfile.empty() ? std::cout : f;
        const int rc = narrow ? run<uint32_t>(text, soff, pa, pb, e, device, out) : run<uint64_t>(text, soff, pa, pb, e, device, out);
        out.flush();
        if (!out) { std::cerr << "error: cannot write the results" << std::endl; return EXIT_FAILURE; }
        return rc;
    } catch (const std::exception& ex) {
        std::cerr << "error: " << ex.what() << std::endl;
        return EXIT_FAILURE;
    }
}
