// locate -- batched pattern search on the MI355X engine, the counterpart of the reference's
// `desa-main -f <text> -c -q <patterns>` (the reference's src/desa_main.cpp):
//   locate -f <text> -q <patterns, one per line> [-k K] [--set] [--occ [LIMIT]] [--longest [--suffixes] [--max-len L]]
//          [--docs] [--doc-list [LIMIT]] [--index 32|64|auto] [--device N] [-o file]
// The text goes up once; the suffix array is constructed in HBM (psacx_construct_dev_*), the lookup table for -k K > 0 is built
// there (psacx_lookup_table_dev_*) and the patterns are located there (psacx_locate_dev_*).  Prints "lb ub" per pattern -- the
// occurrences are SA[lb..ub) -- to stdout or the file of -o, and "SA time:" / "Table time:" / "Locate time: <ms> ms" to stderr.
// An empty line is the empty pattern.
// --set reads -f as gsac does: the strings are the runs between '\n'.  The generalized suffix array is constructed in HBM
// (psacx_construct_gsa_dev_*), the bitmap of the string ends beside it (psacx_string_ends_dev, "Ends time:"), and table and search
// are those of a string set (psacx_lookup_table_gsa_dev_*, psacx_locate_gsa_dev_*): no pattern matches across two strings.
// --occ [LIMIT] prints the occurrences of every pattern after its "lb ub", on the same line (psacx_occurrences_dev_*,
// "Occurrences time:"), at most LIMIT each if LIMIT > 0: text positions, or string:offset-in-string with --set.
// --longest answers every pattern with its longest prefix that occurs (psacx_match_dev_* / psacx_match_gsa_dev_*): prints
// "len lb ub" per query -- the prefix of len bytes occurs at SA[lb..ub) -- and "Match time:" instead of "Locate time:".
// --suffixes makes every byte of every pattern a query (the rest of its pattern from there on: the matching statistics, one line
// per byte in the order of the patterns), --max-len L cuts every query to L bytes.  --occ lists the occurrences of the prefixes.
// --set --docs prints, behind "lb ub", in how many strings the pattern occurs (the LCP comes with the construction, then
// psacx_rmq_index_dev_*, psacx_doc_index_dev_*, psacx_doc_count_dev_*; "Docs time:").  --set --doc-list [LIMIT] prints behind that each such
// string once, as string:offset-in-string of its first suffix in SA order, at most LIMIT per pattern if LIMIT > 0 (psacx_doc_list_dev_*).
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
    std::cerr << "USAGE: locate -f <text> -q <patterns, one per line> [-k K] [--set] [--occ [LIMIT]] [--longest [--suffixes] [--max-len L]]\n"
                 "              [--docs] [--doc-list [LIMIT]] [--index 32|64|auto] [--device N] [-o <file>]\n"
                 "Locates every pattern in the suffix array of the text (MI355X engine): prints lb ub per pattern, the occurrences are SA[lb..ub).\n"
                 "--set: the strings of -f are its lines, and no pattern matches across two of them.  --occ [LIMIT]: print the occurrences too.\n"
                 "--longest: print len lb ub of the longest prefix of every pattern that occurs; --suffixes: of every suffix of every pattern;\n"
                 "--max-len L: of at most L bytes of each.\n"
                 "--set --docs: print in how many strings each pattern occurs; --set --doc-list [LIMIT]: print each of them once.\n";
}

static int table(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, uint32_t k, uint32_t* tab, uint16_t* code, uint32_t* sg, uint64_t* e) {
    return psacx_lookup_table_dev_u32(c, t, n, sa, k, tab, code, sg, e);
}
static int table(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, uint32_t k, uint64_t* tab, uint16_t* code, uint32_t* sg, uint64_t* e) {
    return psacx_lookup_table_dev_u64(c, t, n, sa, k, tab, code, sg, e);
}
static int locate(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* sa, const uint32_t* tab, uint32_t k, const uint16_t* code, const uint8_t* pat,
                  const uint64_t* poff, uint64_t q, uint32_t* lb, uint32_t* ub) { return psacx_locate_dev_u32(c, t, n, sa, tab, k, code, pat, poff, q, lb, ub); }
static int locate(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* sa, const uint64_t* tab, uint32_t k, const uint16_t* code, const uint8_t* pat,
                  const uint64_t* poff, uint64_t q, uint64_t* lb, uint64_t* ub) { return psacx_locate_dev_u64(c, t, n, sa, tab, k, code, pat, poff, q, lb, ub); }

static int table(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint32_t*, uint32_t k, uint32_t* tab, uint16_t* code, uint32_t* sg,
                 uint64_t* e) { return psacx_lookup_table_gsa_dev_u32(c, t, n, ends, k, tab, code, sg, e); }
static int table(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint64_t*, uint32_t k, uint64_t* tab, uint16_t* code, uint32_t* sg,
                 uint64_t* e) { return psacx_lookup_table_gsa_dev_u64(c, t, n, ends, k, tab, code, sg, e); }
static int locate(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint32_t* sa, const uint32_t* tab, uint32_t k, const uint16_t* code,
                  const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t* lb, uint32_t* ub) {
    return psacx_locate_gsa_dev_u32(c, t, n, ends, sa, tab, k, code, pat, poff, q, lb, ub);
}
static int locate(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* ends, const uint64_t* sa, const uint64_t* tab, uint32_t k, const uint16_t* code,
                  const uint8_t* pat, const uint64_t* poff, uint64_t q, uint64_t* lb, uint64_t* ub) {
    return psacx_locate_gsa_dev_u64(c, t, n, ends, sa, tab, k, code, pat, poff, q, lb, ub);
}
// soff: the offsets of the strings of --set (empty without it); occ: print the occurrences, at most limit each if limit > 0;
// longest: --longest, with mflags (PSACX_MATCH_SUFFIXES for --suffixes) and max_len
template <typename IT>
static int run(const std::string& text, const std::vector<uint64_t>& soff, const std::string& pat, const std::vector<uint64_t>& poff, uint32_t k,
               bool occ, uint64_t limit, bool longest, uint32_t mflags, uint64_t max_len, bool docs, bool doc_lists, uint64_t dlimit, int device,
               std::ostream& out) {
    const uint64_t n = text.size(), q = poff.size() - 1, m = soff.empty() ? 0 : soff.size() - 1;
    const uint64_t e = longest && (mflags & PSACX_MATCH_SUFFIXES) ? poff[q] : q;      // results: one per pattern, or one per byte of the patterns
    const bool set = m != 0;
    Session s(device);
    psacx_ctx* const c = s.c;
    auto t0 = std::chrono::steady_clock::now();
    uint8_t* d_text = (uint8_t*)s.dev(n);
    IT* d_sa = (IT*)s.dev(n * sizeof(IT));
    IT* d_isa = (IT*)s.dev(n * sizeof(IT));
    uint64_t* d_soff = set ? (uint64_t*)s.dev((m + 1) * sizeof(uint64_t)) : nullptr;
    must(c, psacx_copy_h2d(c, d_text, text.data(), n));
    if (set) must(c, psacx_copy_h2d(c, d_soff, soff.data(), (m + 1) * sizeof(uint64_t)));
    IT* d_lcp = docs ? (IT*)s.dev(n * sizeof(IT)) : nullptr;
    must(c, construct(c, d_text, n, d_soff, m, docs ? PSACX_LCP : 0, d_sa, d_isa, d_lcp));
    std::cerr << "SA time: " << ms_since(t0) << " ms" << std::endl;
    uint32_t* d_ends = nullptr;
    if (set) {
        auto te = std::chrono::steady_clock::now();
        uint64_t words = 0;
        must(c, psacx_string_ends_dev(c, nullptr, m, n, nullptr, &words));
        d_ends = (uint32_t*)s.dev(words * sizeof(uint32_t));
        must(c, psacx_string_ends_dev(c, d_soff, m, n, d_ends, &words));
        std::cerr << "Ends time: " << ms_since(te) << " ms" << std::endl;
    }
    uint16_t code[256];
    IT* d_table = nullptr;
    if (k) {
        auto t1 = std::chrono::steady_clock::now();
        uint32_t sigma = 0;
        uint64_t entries = 0;
        must(c, set ? table(c, d_text, n, d_ends, (const IT*)nullptr, k, (IT*)nullptr, code, &sigma, &entries)
                    : table(c, d_text, n, (const IT*)nullptr, k, (IT*)nullptr, code, &sigma, &entries));
        d_table = (IT*)s.dev(entries * sizeof(IT));
        must(c, set ? table(c, d_text, n, d_ends, d_sa, k, d_table, code, &sigma, &entries) : table(c, d_text, n, d_sa, k, d_table, code, &sigma, &entries));
        std::cerr << "Table time: " << ms_since(t1) << " ms" << std::endl;
        std::cerr << "Table entries: " << entries << std::endl;
    }
    std::vector<IT> len(longest ? e : 0), lb(e), ub(e), pos, sid, ndocs(docs ? e : 0), dsid, dpos;
    std::vector<uint64_t> start(e + 1, 0), dstart(e + 1, 0);
    if (q) {
        uint8_t* d_pat = (uint8_t*)s.dev(pat.size() + 1);
        uint64_t* d_poff = (uint64_t*)s.dev((q + 1) * sizeof(uint64_t));
        IT* d_len = longest ? (IT*)s.dev(e * sizeof(IT) + 1) : nullptr;
        IT* d_lb = (IT*)s.dev(e * sizeof(IT) + 1);
        IT* d_ub = (IT*)s.dev(e * sizeof(IT) + 1);
        if (!pat.empty()) must(c, psacx_copy_h2d(c, d_pat, pat.data(), pat.size()));
        must(c, psacx_copy_h2d(c, d_poff, poff.data(), (q + 1) * sizeof(uint64_t)));
        auto t2 = std::chrono::steady_clock::now();
        if (longest) {
            must(c, match(c, d_text, n, d_ends, d_sa, d_table, k, k ? code : nullptr, d_pat, d_poff, q, mflags, max_len, e, d_len, d_lb, d_ub));
            std::cerr << "Match time: " << ms_since(t2) << " ms" << std::endl;
            if (e) must(c, psacx_copy_d2h(c, len.data(), d_len, e * sizeof(IT)));
        } else {
            must(c, set ? locate(c, d_text, n, d_ends, d_sa, d_table, k, k ? code : nullptr, d_pat, d_poff, q, d_lb, d_ub)
                        : locate(c, d_text, n, d_sa, d_table, k, k ? code : nullptr, d_pat, d_poff, q, d_lb, d_ub));
            std::cerr << "Locate time: " << ms_since(t2) << " ms" << std::endl;
        }
        if (e) must(c, psacx_copy_d2h(c, lb.data(), d_lb, e * sizeof(IT)));
        if (e) must(c, psacx_copy_d2h(c, ub.data(), d_ub, e * sizeof(IT)));
        if (occ) {
            auto t3 = std::chrono::steady_clock::now();
            uint64_t* d_start = (uint64_t*)s.dev((e + 1) * sizeof(uint64_t));
            uint64_t total = 0;
            must(c, occurrences(c, d_sa, n, d_soff, m, d_lb, d_ub, e, limit, d_start, (IT*)nullptr, (IT*)nullptr, 0, &total));
            IT* d_pos = (IT*)s.dev(total * sizeof(IT) + 1);
            IT* d_sid = set ? (IT*)s.dev(total * sizeof(IT) + 1) : nullptr;
            must(c, occurrences(c, d_sa, n, d_soff, m, d_lb, d_ub, e, limit, d_start, d_pos, d_sid, total, &total));
            std::cerr << "Occurrences time: " << ms_since(t3) << " ms" << std::endl;
            pos.resize(total);
            must(c, psacx_copy_d2h(c, start.data(), d_start, (e + 1) * sizeof(uint64_t)));
            if (total) must(c, psacx_copy_d2h(c, pos.data(), d_pos, total * sizeof(IT)));
            if (set) { sid.resize(total); if (total) must(c, psacx_copy_d2h(c, sid.data(), d_sid, total * sizeof(IT))); }
        }
        if (docs || doc_lists) {
            auto t4 = std::chrono::steady_clock::now();
            // one build of the doc index: dup for the counts, prev for the lists, whichever are asked for
            IT* d_index = nullptr;
            if (docs) { uint64_t entries = 0; d_index = rmq_index_of<IT>(s, d_lcp, n, &entries); }
            IT* d_dup = docs ? (IT*)s.dev((n + 1) * sizeof(IT)) : nullptr;
            IT* d_prev = doc_lists ? (IT*)s.dev(n * sizeof(IT)) : nullptr;
            must(c, doc_index(c, n, d_soff, m, d_sa, d_lcp, d_index, d_prev, d_dup));
            if (docs) {
                IT* d_docs = (IT*)s.dev(e * sizeof(IT) + 1);
                must(c, doc_count(c, n, d_dup, d_lb, d_ub, e, d_docs));
                if (e) must(c, psacx_copy_d2h(c, ndocs.data(), d_docs, e * sizeof(IT)));
            }
            if (doc_lists) {
                uint64_t* d_dstart = (uint64_t*)s.dev((e + 1) * sizeof(uint64_t));
                uint64_t total = 0;
                must(c, doc_list(c, d_sa, n, d_soff, m, d_prev, d_lb, d_ub, e, 0, d_dstart, (IT*)nullptr, (IT*)nullptr, 0, &total));
                IT* d_dsid = (IT*)s.dev(total * sizeof(IT) + 1);
                IT* d_dpos = (IT*)s.dev(total * sizeof(IT) + 1);
                must(c, doc_list(c, d_sa, n, d_soff, m, d_prev, d_lb, d_ub, e, 0, d_dstart, d_dsid, d_dpos, total, &total));
                dsid.resize(total); dpos.resize(total);
                must(c, psacx_copy_d2h(c, dstart.data(), d_dstart, (e + 1) * sizeof(uint64_t)));
                if (total) must(c, psacx_copy_d2h(c, dsid.data(), d_dsid, total * sizeof(IT)));
                if (total) must(c, psacx_copy_d2h(c, dpos.data(), d_dpos, total * sizeof(IT)));
            }
            std::cerr << "Docs time: " << ms_since(t4) << " ms" << std::endl;
        }
    }
    for (uint64_t i = 0; i < e; ++i) {
        if (longest) out << (uint64_t)len[i] << ' ';
        out << (uint64_t)lb[i] << ' ' << (uint64_t)ub[i];
        if (docs) out << ' ' << (uint64_t)ndocs[i];
        if (doc_lists) {
            const uint64_t upto = dlimit && dstart[i] + dlimit < dstart[i + 1] ? dstart[i] + dlimit : dstart[i + 1];
            for (uint64_t t = dstart[i]; t < upto; ++t) {
                const std::size_t sd = (std::size_t)dsid[t];
                out << ' ' << (uint64_t)dsid[t] << ':' << (uint64_t)dpos[t] - (sd < soff.size() ? soff[sd] : 0);
            }
        }
        if (occ)
            for (uint64_t t = start[i]; t < start[i + 1]; ++t) {
                out << ' ';
                if (set) out << (uint64_t)sid[t] << ':' << (uint64_t)pos[t] - soff[(std::size_t)sid[t]]; else out << (uint64_t)pos[t];
            }
        out << '\n';
    }
    return 0;
}

int main(int argc, char** argv) {
    std::string file, queries, outfile, index = "auto";
    int device = 0;
    long k = 0;
    bool set = false, occ = false, longest = false, suffixes = false, docs = false, doc_lists = false;
    unsigned long long limit = 0, max_len = 0, dlimit = 0;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto need = [&](const char* name) -> const char* {
            if (i + 1 >= argc) { std::cerr << "error: missing value for " << name << std::endl; usage(); exit(EXIT_FAILURE); }
            return argv[++i];
        };
        if (a == "-f" || a == "--file") file = need("-f");
        else if (a == "-q" || a == "--queries") queries = need("-q");
        else if (a == "-k") k = atol(need("-k"));
        else if (a == "-o" || a == "--outfile") outfile = need("-o");
        else if (a == "--device") device = atoi(need("--device"));
        else if (a == "--index") index = need("--index");
        else if (a == "--set") set = true;
        else if (a == "--longest") longest = true;
        else if (a == "--suffixes") suffixes = true;
        else if (a == "--max-len") max_len = strtoull(need("--max-len"), nullptr, 10);
        else if (a == "--occ") {
            occ = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') limit = strtoull(argv[++i], nullptr, 10);
        }
        else if (a == "--docs") docs = true;
        else if (a == "--doc-list") {
            doc_lists = true;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') dlimit = strtoull(argv[++i], nullptr, 10);
        }
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { std::cerr << "error: unknown argument " << a << std::endl; usage(); return EXIT_FAILURE; }
    }
    if (file.empty() || queries.empty() || k < 0 || !index_known(index)) { usage(); return EXIT_FAILURE; }
    if ((docs || doc_lists) && !set) { std::cerr << "error: --docs and --doc-list belong to --set" << std::endl; usage(); return EXIT_FAILURE; }
    if (!longest && (suffixes || max_len)) { std::cerr << "error: --suffixes and --max-len belong to --longest" << std::endl; usage(); return EXIT_FAILURE; }
    std::string text, lines;
    if (!read_file(file, text)) { std::cerr << "error: cannot open " << file << std::endl; return EXIT_FAILURE; }
    if (!read_file(queries, lines)) { std::cerr << "error: cannot open " << queries << std::endl; return EXIT_FAILURE; }
    std::vector<uint64_t> soff;
    if (set) { std::string flat; split_lines(text, flat, soff); text.swap(flat); }
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
        std::ofstream f;
        if (!outfile.empty()) {
            f.open(outfile.c_str(), std::ios::trunc);
            if (!f) { std::cerr << "error: cannot write " << outfile << std::endl; return EXIT_FAILURE; }
        }
        std::ostream& out = outfile.empty() ? std::cout : f;
        const int rc = narrow ? run<uint32_t>(text, soff, pat, poff, (uint32_t)k, occ, limit, longest, suffixes ? PSACX_MATCH_SUFFIXES : 0u, max_len, docs, doc_lists, dlimit, device, out)
                             : run<uint64_t>(text, soff, pat, poff, (uint32_t)k, occ, limit, longest, suffixes ? PSACX_MATCH_SUFFIXES : 0u, max_len, docs, doc_lists, dlimit, device, out);
        out.flush();
        if (!out) { std::cerr << "error: cannot write the results" << std::endl; return EXIT_FAILURE; }
        return rc;
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return EXIT_FAILURE;
    }
}
