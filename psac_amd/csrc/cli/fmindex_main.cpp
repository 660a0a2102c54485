// fmindex -- counts and locates patterns in a text or a set of strings through an FM-index, on the MI355X engine:
//   fmindex -f <text> -q <patterns, one per line> [--set] [-s SAMPLE] [--occ [LIMIT]] [--index 32|64|auto] [--device N]
// The text goes up once; with --set its lines are the strings of a set (laid back to back, as gsac reads them).  The suffix array is
// constructed in HBM, the BWT and the index (psacx_fm_index_dev_*) beside it; then text, suffix array and BWT are FREED and the
// patterns are answered from the index alone (psacx_fm_count_dev_*, psacx_fm_occurrences_dev_*).  Prints "lb ub" per pattern to stdout
// -- lb = ub = 0 where it does not occur -- and with --occ its occurrences behind them (at most LIMIT each): positions, or
// string:offset-in-string for a set.  "Index bytes: <b> (text + SA: <t>)" and "SA time:" / "Index time:" / "Search time: <ms> ms" go to
// stderr.  -s 0 builds an index that counts only.
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "query_cli.hpp"

using namespace query_cli;

static void usage() {
    std::cerr << "USAGE: fmindex -f <text> -q <patterns, one per line> [--set] [-s SAMPLE] [--occ [LIMIT]] [--index 32|64|auto] [--device N]\n"
                 "Prints the suffix-array interval \"lb ub\" of every pattern (0 0 where it does not occur) from an FM-index in HBM, after text\n"
                 "and suffix array are freed (MI355X engine).  --set reads one string per line.  -s is the sample rate of the suffix array\n"
                 "(default 32; 0: counts only).  --occ prints the occurrences of every pattern behind its interval.\n";
}

struct Options {
    uint64_t sample, limit;
    bool occ;
    int device;
};

template <typename IT>
static int run(const std::string& text, const std::vector<uint64_t>& soff, const std::string& pat, const std::vector<uint64_t>& poff, const Options& o) {
    const uint64_t n = text.size(), m = soff.empty() ? 0 : soff.size() - 1, q = poff.size() - 1;
    Session s(o.device);
    psacx_ctx* const c = s.c;
    auto t0 = std::chrono::steady_clock::now();
    uint8_t* d_text = (uint8_t*)s.dev(n);
    IT* d_sa = (IT*)s.dev(n * sizeof(IT));
    IT* d_isa = (IT*)s.dev(n * sizeof(IT));
    uint64_t* d_soff = nullptr;
    must(c, psacx_copy_h2d(c, d_text, text.data(), n));
    if (m) {
        d_soff = (uint64_t*)s.dev((m + 1) * sizeof(uint64_t));
        must(c, psacx_copy_h2d(c, d_soff, soff.data(), (m + 1) * sizeof(uint64_t)));
    }
    must(c, construct(c, d_text, n, d_soff, m, 0, d_sa, d_isa, (IT*)nullptr));
    s.release(d_isa);
    std::cerr << "SA time: " << ms_since(t0) << " ms" << std::endl;
    auto t1 = std::chrono::steady_clock::now();
    uint64_t words = (n >> 5) + 1;
    uint32_t* d_ends = nullptr;
    if (m) {
        d_ends = (uint32_t*)s.dev(words * sizeof(uint32_t));
        must(c, psacx_string_ends_dev(c, d_soff, m, n, d_ends, &words));
    }
    uint8_t* d_bwt = (uint8_t*)s.dev(n);
    uint32_t* d_first = (uint32_t*)s.dev(((n >> 5) + 1) * sizeof(uint32_t));
    must(c, bwt(c, d_text, n, d_ends, d_sa, d_bwt, d_first, (uint64_t*)nullptr));
    psacx_fm_info info;
    const IT* sa_in = o.sample ? d_sa : (const IT*)nullptr;
    must(c, fm_build(c, n, d_bwt, d_first, sa_in, o.sample, (uint64_t*)nullptr, &info));
    uint64_t* d_fm = (uint64_t*)s.dev(info.words * sizeof(uint64_t));
    must(c, fm_build(c, n, d_bwt, d_first, sa_in, o.sample, d_fm, &info));
    s.release(d_text); s.release(d_sa); s.release(d_bwt); s.release(d_first);       // the index answers alone from here on
    if (d_ends) s.release(d_ends);
    must(c, psacx_trim(c));
    std::cerr << "Index time: " << ms_since(t1) << " ms" << std::endl;
    std::cerr << "Index bytes: " << info.words * sizeof(uint64_t) << " (text + SA: " << n * (1 + sizeof(IT)) << ")" << std::endl;
    auto t2 = std::chrono::steady_clock::now();
    uint8_t* d_pat = (uint8_t*)s.dev(pat.size() + 1);
    uint64_t* d_poff = (uint64_t*)s.dev((q + 1) * sizeof(uint64_t));
    IT* d_lb = (IT*)s.dev(q * sizeof(IT));
    IT* d_ub = (IT*)s.dev(q * sizeof(IT));
    if (!pat.empty()) must(c, psacx_copy_h2d(c, d_pat, pat.data(), pat.size()));
    must(c, psacx_copy_h2d(c, d_poff, poff.data(), (q + 1) * sizeof(uint64_t)));
    must(c, fm_count(c, d_fm, &info, d_pat, d_poff, q, d_lb, d_ub));
    std::vector<IT> lb(q), ub(q), pos, sid;
    std::vector<uint64_t> start(q + 1, 0);
    if (q) {
        must(c, psacx_copy_d2h(c, lb.data(), d_lb, q * sizeof(IT)));
        must(c, psacx_copy_d2h(c, ub.data(), d_ub, q * sizeof(IT)));
    }
    if (o.occ) {
        uint64_t* d_start = (uint64_t*)s.dev((q + 1) * sizeof(uint64_t));
        uint64_t total = 0;
        must(c, fm_occurrences(c, d_fm, &info, d_soff, m, d_lb, d_ub, q, o.limit, d_start, (IT*)nullptr, (IT*)nullptr, 0, &total));
        IT* d_pos = (IT*)s.dev(total * sizeof(IT));
        IT* d_sid = m ? (IT*)s.dev(total * sizeof(IT)) : nullptr;
        must(c, fm_occurrences(c, d_fm, &info, d_soff, m, d_lb, d_ub, q, o.limit, d_start, d_pos, d_sid, total, &total));
        pos.assign(total, 0);
        if (m) sid.assign(total, 0);
        must(c, psacx_copy_d2h(c, start.data(), d_start, (q + 1) * sizeof(uint64_t)));
        if (total) must(c, psacx_copy_d2h(c, pos.data(), d_pos, total * sizeof(IT)));
        if (total && m) must(c, psacx_copy_d2h(c, sid.data(), d_sid, total * sizeof(IT)));
    }
    std::cerr << "Search time: " << ms_since(t2) << " ms" << std::endl;
    for (uint64_t i = 0; i < q; ++i) {
        std::cout << (uint64_t)lb[i] << ' ' << (uint64_t)ub[i];
        if (o.occ)
            for (uint64_t t = start[i]; t < start[i + 1]; ++t) {
                if (m && (uint64_t)sid[t] < m) std::cout << ' ' << (uint64_t)sid[t] << ':' << (uint64_t)pos[t] - soff[(std::size_t)sid[t]];
                else std::cout << ' ' << (uint64_t)pos[t];
            }
        std::cout << '\n';
    }
    return 0;
}

int main(int argc, char** argv) {
    std::string file, queries, index = "auto";
    Options o;
    o.sample = 32; o.limit = 0; o.occ = false; o.device = 0;
    bool set = false;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { std::cerr << "error: missing value for " << name << std::endl; usage(); exit(EXIT_FAILURE); }
            return argv[++i];
        };
        auto count = [&](const char* name) -> uint64_t {
            const char* w = need(name);
            if (!number(w)) { std::cerr << "error: " << w << " is no number" << std::endl; usage(); exit(EXIT_FAILURE); }
            return strtoull(w, nullptr, 10);
        };
        if (a == "-f" || a == "--file") file = need("-f");
        else if (a == "-q" || a == "--queries") queries = need("-q");
        else if (a == "--set") set = true;
        else if (a == "-s" || a == "--sample") o.sample = count("-s");
        else if (a == "--occ") { o.occ = true; if (i + 1 < argc && number(argv[i + 1])) o.limit = strtoull(argv[++i], nullptr, 10); }
        else if (a == "--device") o.device = atoi(need("--device"));
        else if (a == "--index") index = need("--index");
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { std::cerr << "error: unknown argument " << a << std::endl; usage(); return EXIT_FAILURE; }
    }
    if (file.empty() || queries.empty() || !index_known(index)) { usage(); return EXIT_FAILURE; }
    if (o.occ && o.sample == 0) { std::cerr << "error: --occ needs a sample rate above 0" << std::endl; usage(); return EXIT_FAILURE; }
    std::string raw, text, lines;
    if (!read_file(file, raw)) { std::cerr << "error: cannot open " << file << std::endl; return EXIT_FAILURE; }
    if (!read_file(queries, lines)) { std::cerr << "error: cannot open " << queries << std::endl; return EXIT_FAILURE; }
    std::vector<uint64_t> soff;
    if (set) split_lines(raw, text, soff); else text.swap(raw);
    if (text.empty()) { std::cerr << "error: empty input" << std::endl; return EXIT_FAILURE; }
    // one pattern per line; a last line without its newline counts
    std::string pat;
    std::vector<uint64_t> poff(1, 0);
    for (std::size_t b = 0; b < lines.size();) {
        std::size_t e = lines.find('\n', b);
        if (e == std::string::npos) e = lines.size();
        pat.append(lines, b, e - b);
        poff.push_back(pat.size());
        b = e + 1;
    }
    const bool narrow = use32(index, text.size());
    try {
        const int rc = narrow ? run<uint32_t>(text, soff, pat, poff, o) : run<uint64_t>(text, soff, pat, poff, o);
        std::cout.flush();
        if (!std::cout) { std::cerr << "error: cannot write the results" << std::endl; return EXIT_FAILURE; }
        return rc;
    } catch (const std::exception& ex) {
        std::cerr << "error: " << ex.what() << std::endl;
        return EXIT_FAILURE;
    }
}
