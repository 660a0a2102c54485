// kedit -- where the patterns occur in a text or a set of strings within edit distance E, on the MI355X engine:
//   kedit -f <text> -q <patterns, one per line> -e E [--set] [--best] [-k K] [--index 32|64|auto] [--max-cand C] [--list [LIMIT]] [--device N]
// The text goes up once; with --set its lines are the strings of a set (laid back to back, as gsac reads them).  The suffix array
// is constructed in HBM (psacx_construct_dev_* / psacx_construct_gsa_dev_*), with -k the k-mer lookup table beside it, and one call
// gives the hits (psacx_kedit_dev_*).  Prints "z: <hits>", "candidates: <c>" and "raw hits: <r>" to stdout and "SA time:" /
// "Index time:" / "Search time: <ms> ms" to stderr.  --list prints one line "pattern string position-in-string length distance" per
// hit (at most LIMIT of them) in the order of the call: ascending pattern, then ascending position.  --best keeps the hits of the
// smallest distance of every pattern (PSACX_KEDIT_BEST).
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "query_cli.hpp"

using namespace query_cli;

static void usage() {
    std::cerr << "USAGE: kedit -f <text> -q <patterns, one per line> -e E [--set] [--best] [-k K] [--index 32|64|auto] [--max-cand C]\n"
                 "             [--list [LIMIT]] [--device N]\n"
                 "Prints the number z of starts from which a pattern occurs in the text within edit distance E (0..15) (MI355X engine).\n"
                 "--set reads one string per line.  --best keeps the hits of the smallest distance of every pattern.  --max-cand refuses a\n"
                 "batch whose pieces occur more than C times in all.  --list prints \"pattern string position length distance\" per hit.\n";
}

static int kedit(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint32_t* sa, const uint32_t* tab, uint32_t k,
                 const uint16_t* code, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t e, uint64_t max_cand, uint32_t flags, uint64_t* qid,
                 uint32_t* tpos, uint32_t* len, uint8_t* dist, uint64_t cap, uint64_t* z, uint64_t* work) {
    return psacx_kedit_dev_u32(c, t, n, ends, sa, tab, k, code, pat, poff, q, e, max_cand, flags, qid, tpos, len, dist, cap, z, work);
}
static int kedit(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint64_t* sa, const uint64_t* tab, uint32_t k,
                 const uint16_t* code, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t e, uint64_t max_cand, uint32_t flags, uint64_t* qid,
                 uint64_t* tpos, uint64_t* len, uint8_t* dist, uint64_t cap, uint64_t* z, uint64_t* work) {
    return psacx_kedit_dev_u64(c, t, n, ends, sa, tab, k, code, pat, poff, q, e, max_cand, flags, qid, tpos, len, dist, cap, z, work);
}

struct Options {
    uint64_t max_cand, limit;
    uint32_t k, e, flags;
    bool list;
    int device;
};

// the last j with off[j] <= p
static std::size_t holder(const std::vector<uint64_t>& off, uint64_t p) {
    std::size_t lo = 0, hi = off.size();
    while (hi - lo > 1) { const std::size_t mid = lo + (hi - lo) / 2; if (off[mid] <= p) lo = mid; else hi = mid; }
    return lo;
}

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
    std::cerr << "SA time: " << ms_since(t0) << " ms" << std::endl;
    auto t1 = std::chrono::steady_clock::now();
    uint64_t words = (n >> 5) + 1;
    uint32_t* d_ends = nullptr;
    if (m) {
        d_ends = (uint32_t*)s.dev(words * sizeof(uint32_t));
        must(c, psacx_string_ends_dev(c, d_soff, m, n, d_ends, &words));
    }
    uint16_t code[256];
    IT* d_table = nullptr;
    if (o.k) {
        uint32_t sigma = 0;
        uint64_t te = 0;
        must(c, lookup_table(c, d_text, n, d_ends, o.k, (IT*)nullptr, code, &sigma, &te));
        d_table = (IT*)s.dev(te * sizeof(IT));
        must(c, lookup_table(c, d_text, n, d_ends, o.k, d_table, code, &sigma, &te));
    }
    std::cerr << "Index time: " << ms_since(t1) << " ms" << std::endl;
    auto t2 = std::chrono::steady_clock::now();
    uint8_t* d_pat = (uint8_t*)s.dev(pat.size() + 1);
    uint64_t* d_poff = (uint64_t*)s.dev((q + 1) * sizeof(uint64_t));
    if (!pat.empty()) must(c, psacx_copy_h2d(c, d_pat, pat.data(), pat.size()));
    must(c, psacx_copy_h2d(c, d_poff, poff.data(), (q + 1) * sizeof(uint64_t)));
    uint64_t z = 0, work[2] = {0, 0};
    must(c, kedit(c, d_text, n, d_ends, d_sa, d_table, o.k, o.k ? code : nullptr, d_pat, d_poff, q, o.e, o.max_cand, o.flags, (uint64_t*)nullptr, (IT*)nullptr,
                  (IT*)nullptr, (uint8_t*)nullptr, 0, &z, work));
    uint64_t* d_qid = nullptr;
    IT *d_tpos = nullptr, *d_len = nullptr;
    uint8_t* d_dist = nullptr;
    if (o.list) {
        d_qid = (uint64_t*)s.dev(z * sizeof(uint64_t)); d_tpos = (IT*)s.dev(z * sizeof(IT)); d_len = (IT*)s.dev(z * sizeof(IT)); d_dist = (uint8_t*)s.dev(z);
        must(c, kedit(c, d_text, n, d_ends, d_sa, d_table, o.k, o.k ? code : nullptr, d_pat, d_poff, q, o.e, o.max_cand, o.flags, d_qid, d_tpos, d_len, d_dist,
                      z, &z, work));
    }
    std::cerr << "Search time: " << ms_since(t2) << " ms" << std::endl;
    std::cout << "z: " << z << "\ncandidates: " << work[0] << "\nraw hits: " << work[1] << '\n';
    if (o.list && z) {
        std::vector<uint64_t> qid(z);
        std::vector<IT> tpos(z), len(z);
        std::vector<uint8_t> dist(z);
        must(c, psacx_copy_d2h(c, qid.data(), d_qid, z * sizeof(uint64_t)));
        must(c, psacx_copy_d2h(c, tpos.data(), d_tpos, z * sizeof(IT)));
        must(c, psacx_copy_d2h(c, len.data(), d_len, z * sizeof(IT)));
        must(c, psacx_copy_d2h(c, dist.data(), d_dist, z));
        const uint64_t shown = o.limit && o.limit < z ? o.limit : z;
        for (uint64_t i = 0; i < shown; ++i) {
            const std::size_t sid = m ? holder(soff, (uint64_t)tpos[i]) : 0;
            std::cout << qid[i] << ' ' << sid << ' ' << (uint64_t)tpos[i] - (m ? soff[sid] : 0) << ' ' << (uint64_t)len[i] << ' '
                      << (unsigned)dist[i] << '\n';
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    std::string file, queries, index = "auto";
    Options o;
    o.max_cand = 0; o.limit = 0; o.k = 0; o.e = 0; o.flags = 0; o.list = false; o.device = 0;
    bool set = false, have_e = false;
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
        else if (a == "--best") o.flags |= PSACX_KEDIT_BEST;
        else if (a == "-e" || a == "--edits") {
            const uint64_t v = count("-e");
            if (v > 15) { std::cerr << "error: -e takes 0..15" << std::endl; usage(); return EXIT_FAILURE; }
            o.e = (uint32_t)v; have_e = true;
        }
        else if (a == "--max-cand") o.max_cand = count("--max-cand");
        else if (a == "-k") o.k = (uint32_t)count("-k");
        else if (a == "--list") { o.list = true; if (i + 1 < argc && number(argv[i + 1])) o.limit = strtoull(argv[++i], nullptr, 10); }
        else if (a == "--device") o.device = atoi(need("--device"));
        else if (a == "--index") index = need("--index");
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { std::cerr << "error: unknown argument " << a << std::endl; usage(); return EXIT_FAILURE; }
    }
    if (file.empty() || queries.empty() || !have_e || !index_known(index)) { usage(); return EXIT_FAILURE; }
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
