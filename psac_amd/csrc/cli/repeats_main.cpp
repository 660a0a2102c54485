// repeats -- the right-maximal, maximal or supermaximal repeats of a text or a set of strings, and its BWT, on the MI355X engine:
//   repeats -f <text> [--set] [--index 32|64|auto] [--kind right|maximal|super] [-l MINLEN] [--min-occ K] [--max-occ K]
//           [--list [LIMIT]] [--bwt OUT] [--min-docs D [--max-docs D]] [--device N]
// The text goes up once; with --set its lines are the strings of a set (laid back to back, as gsac reads them).  SA and LCP are
// constructed in HBM (psacx_construct_dev_* / psacx_construct_gsa_dev_* with PSACX_LCP), the range-minimum index of LCP and the BWT
// are built beside them (psacx_rmq_index_dev_*, psacx_bwt_dev_*), and one call enumerates the repeats (psacx_repeats_dev_*).  Prints
// "z: <repeats>" to stdout and "SA time:" / "Index time:" / "BWT time:" / "Repeats time: <ms> ms" to stderr.  --list prints one line
// "lb ub len first-occurrence" per repeat (at most LIMIT of them), --bwt writes the n bytes of the BWT to OUT and prints
// "primary: <rank>".
// --set --min-docs D [--max-docs D] keeps the repeats that occur in at least D (and at most --max-docs) strings of the set
// (psacx_doc_index_dev_*, psacx_doc_count_dev_*, "Docs time:"; the filter runs on the host): z counts those, --list prints them with a fifth
// column, the number of strings, and a last line "longest: lb ub len pos docs" names the longest repeat kept (the first of them in the
// order of the list; "longest: none" if none is kept).
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
    std::cerr << "USAGE: repeats -f <text> [--set] [--index 32|64|auto] [--kind right|maximal|super] [-l MINLEN] [--min-occ K] [--max-occ K]\n"
                 "               [--list [LIMIT]] [--bwt OUT] [--min-docs D [--max-docs D]] [--device N]\n"
                 "Prints the number z of repeats of the kind (default maximal) that are at least MINLEN long and occur between\n"
                 "--min-occ and --max-occ times (MI355X engine).  --set reads one string per line.  --list prints \"lb ub len pos\" per\n"
                 "repeat: it is the len bytes at pos and occurs at SA[lb .. ub).  --bwt writes the SA-aligned BWT and prints the primary.\n"
                 "--set --min-docs D [--max-docs D]: only the repeats that occur in D or more (and at most --max-docs) strings, with that\n"
                 "number as a fifth column, and a line \"longest: lb ub len pos docs\" for the longest of them.\n";
}

static int repeats(psacx_ctx* c, uint64_t n, const uint32_t* lcp, const uint32_t* index, const uint8_t* b, const uint32_t* f, uint32_t kind, uint64_t l,
                   uint64_t lo, uint64_t hi, uint32_t* lb, uint32_t* ub, uint32_t* len, uint64_t cap, uint64_t* z) {
    return psacx_repeats_dev_u32(c, n, lcp, index, b, f, kind, l, lo, hi, lb, ub, len, cap, z);
}
static int repeats(psacx_ctx* c, uint64_t n, const uint64_t* lcp, const uint64_t* index, const uint8_t* b, const uint32_t* f, uint32_t kind, uint64_t l,
                   uint64_t lo, uint64_t hi, uint64_t* lb, uint64_t* ub, uint64_t* len, uint64_t cap, uint64_t* z) {
    return psacx_repeats_dev_u64(c, n, lcp, index, b, f, kind, l, lo, hi, lb, ub, len, cap, z);
}

struct Options {
    uint32_t kind;
    uint64_t min_len, min_occ, max_occ, limit, min_docs, max_docs;
    bool list;
    std::string bwt_out;
    int device;
};

template <typename IT>
static int run(const std::string& text, const std::vector<uint64_t>& soff, const Options& o) {
    const uint64_t n = text.size(), m = soff.empty() ? 0 : soff.size() - 1;
    Session s(o.device);
    psacx_ctx* const c = s.c;
    auto t0 = std::chrono::steady_clock::now();
    uint8_t* d_text = (uint8_t*)s.dev(n);
    IT* d_sa = (IT*)s.dev(n * sizeof(IT));
    IT* d_isa = (IT*)s.dev(n * sizeof(IT));
    IT* d_lcp = (IT*)s.dev(n * sizeof(IT));
    uint64_t* d_soff = nullptr;
    must(c, psacx_copy_h2d(c, d_text, text.data(), n));
    if (m) {
        d_soff = (uint64_t*)s.dev((m + 1) * sizeof(uint64_t));
        must(c, psacx_copy_h2d(c, d_soff, soff.data(), (m + 1) * sizeof(uint64_t)));
    }
    must(c, construct(c, d_text, n, d_soff, m, PSACX_LCP, d_sa, d_isa, d_lcp));
    std::cerr << "SA time: " << ms_since(t0) << " ms" << std::endl;
    auto t1 = std::chrono::steady_clock::now();
    uint64_t entries = 0, words = (n >> 5) + 1;
    IT* d_index = rmq_index_of<IT>(s, d_lcp, n, &entries);
    uint32_t* d_ends = nullptr;
    if (m) {
        d_ends = (uint32_t*)s.dev(words * sizeof(uint32_t));
        must(c, psacx_string_ends_dev(c, d_soff, m, n, d_ends, &words));
    }
    std::cerr << "Index time: " << ms_since(t1) << " ms" << std::endl;
    auto t2 = std::chrono::steady_clock::now();
    uint8_t* d_bwt = (uint8_t*)s.dev(n);
    uint32_t* d_first = (uint32_t*)s.dev(words * sizeof(uint32_t));
    uint64_t primary = 0;
    must(c, bwt(c, d_text, n, d_ends, d_sa, d_bwt, d_first, &primary));
    std::cerr << "BWT time: " << ms_since(t2) << " ms" << std::endl;
    auto t3 = std::chrono::steady_clock::now();
    uint64_t z = 0;
    must(c, repeats(c, n, d_lcp, d_index, d_bwt, d_first, o.kind, o.min_len, o.min_occ, o.max_occ, (IT*)nullptr, (IT*)nullptr, (IT*)nullptr, 0, &z));
    IT *d_lb = nullptr, *d_ub = nullptr, *d_len = nullptr;
    const bool by_docs = o.min_docs != 0;
    if (o.list || by_docs) {
        d_lb = (IT*)s.dev(z * sizeof(IT)); d_ub = (IT*)s.dev(z * sizeof(IT)); d_len = (IT*)s.dev(z * sizeof(IT));
        must(c, repeats(c, n, d_lcp, d_index, d_bwt, d_first, o.kind, o.min_len, o.min_occ, o.max_occ, d_lb, d_ub, d_len, z, &z));
    }
    std::cerr << "Repeats time: " << ms_since(t3) << " ms" << std::endl;
    std::vector<IT> docs;
    std::vector<uint64_t> kept;                            // with --min-docs: the repeats that pass, in the order of the list
    if (by_docs) {
        auto t4 = std::chrono::steady_clock::now();
        doc_counts_of<IT>(s, n, d_soff, m, d_sa, d_lcp, d_index, d_lb, d_ub, z, docs);
        std::cerr << "Docs time: " << ms_since(t4) << " ms" << std::endl;
        for (uint64_t k = 0; k < z; ++k)
            if ((uint64_t)docs[k] >= o.min_docs && (o.max_docs == 0 || (uint64_t)docs[k] <= o.max_docs)) kept.push_back(k);
    }
    std::cout << "z: " << (by_docs ? (uint64_t)kept.size() : z) << '\n';
    if (!o.bwt_out.empty()) {
        std::string b(n, '\0');
        must(c, psacx_copy_d2h(c, &b[0], d_bwt, n));
        std::ofstream f(o.bwt_out.c_str(), std::ios::binary | std::ios::trunc);
        f.write(b.data(), (std::streamsize)n);
        f.flush();
        if (!f) throw std::runtime_error("cannot write " + o.bwt_out);
        std::cout << "primary: " << primary << '\n';
    }
    if ((o.list || by_docs) && z) {
        std::vector<IT> lb(z), ub(z), len(z), sa(n);
        must(c, psacx_copy_d2h(c, lb.data(), d_lb, z * sizeof(IT)));
        must(c, psacx_copy_d2h(c, ub.data(), d_ub, z * sizeof(IT)));
        must(c, psacx_copy_d2h(c, len.data(), d_len, z * sizeof(IT)));
        must(c, psacx_copy_d2h(c, sa.data(), d_sa, n * sizeof(IT)));
        auto line = [&](uint64_t k) {
            uint64_t pos = (uint64_t)sa[lb[k]];                 // the first occurrence in the text
            for (uint64_t r = (uint64_t)lb[k]; r < (uint64_t)ub[k]; ++r) if ((uint64_t)sa[r] < pos) pos = (uint64_t)sa[r];
            std::cout << (uint64_t)lb[k] << ' ' << (uint64_t)ub[k] << ' ' << (uint64_t)len[k] << ' ' << pos;
            if (by_docs) std::cout << ' ' << (uint64_t)docs[k];
            std::cout << '\n';
        };
        const uint64_t have = by_docs ? (uint64_t)kept.size() : z;
        const uint64_t shown = o.limit && o.limit < have ? o.limit : have;
        if (o.list)
            for (uint64_t k = 0; k < shown; ++k) line(by_docs ? kept[k] : k);
        if (by_docs && !kept.empty()) {
            uint64_t best = kept[0];
            for (std::size_t i = 1; i < kept.size(); ++i) if ((uint64_t)len[kept[i]] > (uint64_t)len[best]) best = kept[i];
            std::cout << "longest: ";
            line(best);
        }
    }
    if (by_docs && kept.empty()) std::cout << "longest: none\n";
    return 0;
}

int main(int argc, char** argv) {
    std::string file, index = "auto", kind = "maximal";
    Options o;
    o.kind = PSACX_REPEATS_MAXIMAL; o.min_len = 1; o.min_occ = 2; o.max_occ = 0; o.limit = 0; o.list = false; o.device = 0; o.min_docs = o.max_docs = 0;
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
        else if (a == "--set") set = true;
        else if (a == "--kind") kind = need("--kind");
        else if (a == "-l" || a == "--min-len") o.min_len = count("-l");
        else if (a == "--min-occ") o.min_occ = count("--min-occ");
        else if (a == "--max-occ") o.max_occ = count("--max-occ");
        else if (a == "--list") { o.list = true; if (i + 1 < argc && number(argv[i + 1])) o.limit = strtoull(argv[++i], nullptr, 10); }
        else if (a == "--bwt") o.bwt_out = need("--bwt");
        else if (a == "--min-docs") o.min_docs = count("--min-docs");
        else if (a == "--max-docs") o.max_docs = count("--max-docs");
        else if (a == "--device") o.device = atoi(need("--device"));
        else if (a == "--index") index = need("--index");
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { std::cerr << "error: unknown argument " << a << std::endl; usage(); return EXIT_FAILURE; }
    }
    if (kind == "right") o.kind = PSACX_REPEATS_RIGHT;
    else if (kind == "maximal") o.kind = PSACX_REPEATS_MAXIMAL;
    else if (kind == "super" || kind == "supermaximal") o.kind = PSACX_REPEATS_SUPERMAXIMAL;
    else { usage(); return EXIT_FAILURE; }
    if (file.empty() || !index_known(index)) { usage(); return EXIT_FAILURE; }
    if ((o.min_docs || o.max_docs) && (!set || !o.min_docs)) { std::cerr << "error: --min-docs belongs to --set, --max-docs to --min-docs" << std::endl; usage(); return EXIT_FAILURE; }
    std::string raw, text;
    if (!read_file(file, raw)) { std::cerr << "error: cannot open " << file << std::endl; return EXIT_FAILURE; }
    std::vector<uint64_t> soff;
    if (set) split_lines(raw, text, soff); else text.swap(raw);
    if (text.empty()) { std::cerr << "error: empty input" << std::endl; return EXIT_FAILURE; }
    const bool narrow = use32(index, text.size());
    try {
        const int rc = narrow ? run<uint32_t>(text, soff, o) : run<uint64_t>(text, soff, o);
        std::cout.flush();
        if (!std::cout) { std::cerr << "error: cannot write the results" << std::endl; return EXIT_FAILURE; }
        return rc;
    } catch (const std::exception& ex) {
        std::cerr << "error: " << ex.what() << std::endl;
        return EXIT_FAILURE;
    }
}
