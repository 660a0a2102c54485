// mems -- the maximal exact matches of a batch of patterns against a text or a set of strings on the MI355X engine:
//   mems -f <text> -q <patterns, one per line> -l MINLEN [--set] [--super] [--max-occ K] [-k K] [--index 32|64|auto]
//        [--list [LIMIT]] [--device N]
// The text goes up once; with --set its lines are the strings of a set (laid back to back, as gsac reads them).  SA and LCP are
// constructed in HBM (psacx_construct_dev_* / psacx_construct_gsa_dev_* with PSACX_LCP); the range-minimum index of LCP, the BWT and
// -- with -k -- the k-mer lookup table are built beside them; one call gives the matching statistics of every pattern position
// (psacx_match_dev_* with PSACX_MATCH_SUFFIXES) and one the matches (psacx_mems_dev_*).  Prints "z: <matches>" to stdout and "SA
// time:" / "Index time:" / "BWT time:" / "Match time:" / "MEMs time: <ms> ms" to stderr.  --list prints one line
// "pattern offset-in-pattern string position-in-string length" per match (at most LIMIT of them) in the order of the call:
// ascending pattern position, then descending length, then suffix-array rank.
#include <chrono>
#include <cstdlib>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "query_cli.hpp"

using namespace query_cli;

static void usage() {
    std::cerr << "USAGE: mems -f <text> -q <patterns, one per line> -l MINLEN [--set] [--super] [--max-occ K] [-k K] [--index 32|64|auto]\n"
                 "            [--list [LIMIT]] [--device N]\n"
                 "Prints the number z of maximal exact matches of at least MINLEN bytes between the patterns and the text (MI355X engine).\n"
                 "--set reads one string per line.  --max-occ keeps matches whose bytes occur at most K times in the text, --super those\n"
                 "contained in no other match of their pattern.  --list prints \"pattern offset string position length\" per match.\n";
}

static int mems(psacx_ctx* c, uint64_t n, const uint32_t* sa, const uint32_t* lcp, const uint32_t* index, const uint8_t* b, const uint32_t* f,
                const uint8_t* pat, const uint64_t* poff, uint64_t q, const uint32_t* ml, const uint32_t* mlb, const uint32_t* mub, uint64_t l,
                uint64_t hi, uint32_t flags, uint64_t* qpos, uint32_t* tpos, uint32_t* len, uint64_t cap, uint64_t* z) {
    return psacx_mems_dev_u32(c, n, sa, lcp, index, b, f, pat, poff, q, ml, mlb, mub, l, hi, flags, qpos, tpos, len, cap, z, nullptr);
}
static int mems(psacx_ctx* c, uint64_t n, const uint64_t* sa, const uint64_t* lcp, const uint64_t* index, const uint8_t* b, const uint32_t* f,
                const uint8_t* pat, const uint64_t* poff, uint64_t q, const uint64_t* ml, const uint64_t* mlb, const uint64_t* mub, uint64_t l,
                uint64_t hi, uint32_t flags, uint64_t* qpos, uint64_t* tpos, uint64_t* len, uint64_t cap, uint64_t* z) {
    return psacx_mems_dev_u64(c, n, sa, lcp, index, b, f, pat, poff, q, ml, mlb, mub, l, hi, flags, qpos, tpos, len, cap, z, nullptr);
}

struct Options {
    uint64_t min_len, max_occ, limit;
    uint32_t k, flags;
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
    const uint64_t n = text.size(), m = soff.empty() ? 0 : soff.size() - 1, q = poff.size() - 1, e = poff[q];
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
    uint8_t* d_bwt = (uint8_t*)s.dev(n);
    uint32_t* d_first = (uint32_t*)s.dev(words * sizeof(uint32_t));
    must(c, bwt(c, d_text, n, d_ends, d_sa, d_bwt, d_first, (uint64_t*)nullptr));
    std::cerr << "BWT time: " << ms_since(t2) << " ms" << std::endl;
    auto t3 = std::chrono::steady_clock::now();
    uint8_t* d_pat = (uint8_t*)s.dev(pat.size() + 1);
    uint64_t* d_poff = (uint64_t*)s.dev((q + 1) * sizeof(uint64_t));
    IT* d_ml = (IT*)s.dev(e * sizeof(IT) + 1);
    IT* d_mlb = (IT*)s.dev(e * sizeof(IT) + 1);
    IT* d_mub = (IT*)s.dev(e * sizeof(IT) + 1);
    if (!pat.empty()) must(c, psacx_copy_h2d(c, d_pat, pat.data(), pat.size()));
    must(c, psacx_copy_h2d(c, d_poff, poff.data(), (q + 1) * sizeof(uint64_t)));
    if (q) must(c, match(c, d_text, n, d_ends, d_sa, d_table, o.k, o.k ? code : nullptr, d_pat, d_poff, q, PSACX_MATCH_SUFFIXES, 0, e, d_ml, d_mlb, d_mub));
    std::cerr << "Match time: " << ms_since(t3) << " ms" << std::endl;
    auto t4 = std::chrono::steady_clock::now();
    uint64_t z = 0;
    must(c, mems(c, n, d_sa, d_lcp, d_index, d_bwt, d_first, d_pat, d_poff, q, d_ml, d_mlb, d_mub, o.min_len, o.max_occ, o.flags, (uint64_t*)nullptr,
                 (IT*)nullptr, (IT*)nullptr, 0, &z));
    uint64_t* d_qpos = nullptr;
    IT *d_tpos = nullptr, *d_len = nullptr;
    if (o.list) {
        d_qpos = (uint64_t*)s.dev(z * sizeof(uint64_t)); d_tpos = (IT*)s.dev(z * sizeof(IT)); d_len = (IT*)s.dev(z * sizeof(IT));
        must(c, mems(c, n, d_sa, d_lcp, d_index, d_bwt, d_first, d_pat, d_poff, q, d_ml, d_mlb, d_mub, o.min_len, o.max_occ, o.flags, d_qpos, d_tpos,
                     d_len, z, &z));
    }
    std::cerr << "MEMs time: " << ms_since(t4) << " ms" << std::endl;
    std::cout << "z: " << z << '\n';
    if (o.list && z) {
        std::vector<uint64_t> qpos(z);
        std::vector<IT> tpos(z), len(z);
        must(c, psacx_copy_d2h(c, qpos.data(), d_qpos, z * sizeof(uint64_t)));
        must(c, psacx_copy_d2h(c, tpos.data(), d_tpos, z * sizeof(IT)));
        must(c, psacx_copy_d2h(c, len.data(), d_len, z * sizeof(IT)));
        const uint64_t shown = o.limit && o.limit < z ? o.limit : z;
        for (uint64_t i = 0; i < shown; ++i) {
            const std::size_t j = holder(poff, qpos[i]), sid = m ? holder(soff, (uint64_t)tpos[i]) : 0;
            std::cout << j << ' ' << qpos[i] - poff[j] << ' ' << sid << ' ' << (uint64_t)tpos[i] - (m ? soff[sid] : 0) << ' ' << (uint64_t)len[i] << '\n';
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    std::string file, queries, index = "auto";
    Options o;
    o.min_len = 0; o.max_occ = 0; o.limit = 0; o.k = 0; o.flags = 0; o.list = false; o.device = 0;
    bool set = false, have_len = false;
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
        else if (a == "--super") o.flags |= PSACX_MEMS_SUPER;
        else if (a == "-l" || a == "--min-len") { o.min_len = count("-l"); have_len = true; }
        else if (a == "--max-occ") o.max_occ = count("--max-occ");
        else if (a == "-k") o.k = (uint32_t)count("-k");
        else if (a == "--list") { o.list = true; if (i + 1 < argc && number(argv[i + 1])) o.limit = strtoull(argv[++i], nullptr, 10); }
        else if (a == "--device") o.device = atoi(need("--device"));
        else if (a == "--index") index = need("--index");
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { std::cerr << "error: unknown argument " << a << std::endl; usage(); return EXIT_FAILURE; }
    }
    if (file.empty() || queries.empty() || !have_len || !index_known(index)) { usage(); return EXIT_FAILURE; }
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
