// fmindex -- counts and locates patterns in a text or a set of strings through an FM-index, on the MI355X engine:
//   fmindex -f <text> -q <patterns, one per line> [--set] [-s SAMPLE] [--occ [LIMIT]] [--text-rate R] [--context W] [--restore OUT]
//           [--index 32|64|auto] [--device N]
// The text goes up once; with --set its lines are the strings of a set (laid back to back, as gsac reads them).  The suffix array is
// constructed in HBM, the BWT and the index (psacx_fm_index_dev_*) beside it; then text, suffix array and BWT are FREED and the
// patterns are answered from the index alone (psacx_fm_count_dev_*, psacx_fm_occurrences_dev_*).  Prints "lb ub" per pattern to stdout
// -- lb = ub = 0 where it does not occur -- and with --occ its occurrences behind them (at most LIMIT each): positions, or
// string:offset-in-string for a set.  "Index bytes: <b> (text + SA: <t>)" and "SA time:" / "Index time:" / "Search time: <ms> ms" go to
// stderr.  -s 0 builds an index that counts only.
// --text-rate R builds the text samples beside the index (psacx_fm_text_samples_dev_*), before the suffix array goes; the index bytes
// count them.  With them, --context W (with --occ) prints under the line of a pattern one line per listed occurrence: a tab, the
// occurrence as above, a tab, and the occurrence with W bytes on either side, clipped to its string (psacx_fm_extract_dev_*); and
// --restore OUT writes the text back from the index alone: the bytes of the text, or with --set every string and a newline.
#include <algorithm>
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
    std::cerr << "USAGE: fmindex -f <text> -q <patterns, one per line> [--set] [-s SAMPLE] [--occ [LIMIT]] [--text-rate R] [--context W]\n"
                 "               [--restore OUT] [--index 32|64|auto] [--device N]\n"
                 "Prints the suffix-array interval \"lb ub\" of every pattern (0 0 where it does not occur) from an FM-index in HBM, after text\n"
                 "and suffix array are freed (MI355X engine).  --set reads one string per line.  -s is the sample rate of the suffix array\n"
                 "(default 32; 0: counts only).  --occ prints the occurrences of every pattern behind its interval.\n"
                 "--text-rate R keeps one rank per R positions and per string, so that the index gives the text back: --context W (with --occ)\n"
                 "prints every listed occurrence with W bytes on either side, --restore OUT writes the whole text to OUT from the index.\n";
}

struct Options {
    uint64_t sample, limit, text_rate, width;
    bool occ, context;
    int device;
    std::string restore;
};

static int text_samples(psacx_ctx* c, uint64_t n, const uint32_t* sa, const uint64_t* off, uint64_t m, uint64_t rate, uint32_t* ts, uint64_t* e) {
    return psacx_fm_text_samples_dev_u32(c, n, sa, off, m, rate, ts, e);
}
static int text_samples(psacx_ctx* c, uint64_t n, const uint64_t* sa, const uint64_t* off, uint64_t m, uint64_t rate, uint64_t* ts, uint64_t* e) {
    return psacx_fm_text_samples_dev_u64(c, n, sa, off, m, rate, ts, e);
}
static int fm_extract(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint32_t* ts, uint64_t rate, const uint64_t* off, uint64_t m,
                      const uint32_t* pos, const uint32_t* len, uint64_t q, uint64_t* start, uint8_t* out, uint64_t cap, uint64_t* total) {
    return psacx_fm_extract_dev_u32(c, fm, i, ts, rate, off, m, pos, len, q, start, out, cap, total);
}
static int fm_extract(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint64_t* ts, uint64_t rate, const uint64_t* off, uint64_t m,
                      const uint64_t* pos, const uint64_t* len, uint64_t q, uint64_t* start, uint8_t* out, uint64_t cap, uint64_t* total) {
    return psacx_fm_extract_dev_u64(c, fm, i, ts, rate, off, m, pos, len, q, start, out, cap, total);
}

// the bytes of the queries (pos[i], len[i]) from the index, back to back, and where each begins: the size query, then the fill
template <typename IT>
static void extract(Session& s, const uint64_t* d_fm, const psacx_fm_info& info, const IT* d_ts, uint64_t rate, const uint64_t* d_soff, uint64_t m,
                    const std::vector<IT>& pos, const std::vector<IT>& len, std::vector<uint64_t>& start, std::string& out) {
    psacx_ctx* const c = s.c;
    const uint64_t q = pos.size();
    IT* d_pos = (IT*)s.dev(q * sizeof(IT));
    IT* d_len = (IT*)s.dev(q * sizeof(IT));
    uint64_t* d_start = (uint64_t*)s.dev((q + 1) * sizeof(uint64_t));
    if (q) {
        must(c, psacx_copy_h2d(c, d_pos, pos.data(), q * sizeof(IT)));
        must(c, psacx_copy_h2d(c, d_len, len.data(), q * sizeof(IT)));
    }
    uint64_t total = 0;
    must(c, fm_extract(c, d_fm, &info, d_ts, rate, d_soff, m, d_pos, d_len, q, d_start, (uint8_t*)nullptr, 0, &total));
    uint8_t* d_out = (uint8_t*)s.dev(total);
    must(c, fm_extract(c, d_fm, &info, d_ts, rate, d_soff, m, d_pos, d_len, q, d_start, d_out, total, &total));
    start.assign(q + 1, 0);
    out.assign(total, '\0');
    must(c, psacx_copy_d2h(c, start.data(), d_start, (q + 1) * sizeof(uint64_t)));
    if (total) must(c, psacx_copy_d2h(c, &out[0], d_out, total));
    s.release(d_pos); s.release(d_len); s.release(d_start); s.release(d_out);
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
    IT* d_ts = nullptr;
    uint64_t entries = 0;
    if (o.text_rate) {
        must(c, text_samples(c, n, (const IT*)nullptr, d_soff, m, o.text_rate, (IT*)nullptr, &entries));
        d_ts = (IT*)s.dev(entries * sizeof(IT));
        must(c, text_samples(c, n, d_sa, d_soff, m, o.text_rate, d_ts, &entries));
    }
    s.release(d_text); s.release(d_sa); s.release(d_bwt); s.release(d_first);       // the index answers alone from here on
    if (d_ends) s.release(d_ends);
    must(c, psacx_trim(c));
    std::cerr << "Index time: " << ms_since(t1) << " ms" << std::endl;
    std::cerr << "Index bytes: " << info.words * sizeof(uint64_t) + entries * sizeof(IT) << " (text + SA: " << n * (1 + sizeof(IT)) << ")" << std::endl;
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
    std::vector<uint64_t> wstart;
    std::string windows;
    if (o.context) {                                   // [pos - W, pos + pattern + W), cut at the start of its string here and at its end by the call
        std::vector<IT> wpos(pos.size()), wlen(pos.size());
        for (uint64_t i = 0; i < q; ++i)
            for (uint64_t t = start[i]; t < start[i + 1]; ++t) {
                const uint64_t p = (uint64_t)pos[t], lo = m && (uint64_t)sid[t] < m ? soff[(std::size_t)sid[t]] : 0;
                const uint64_t a = p >= n ? p : (p - lo > o.width ? p - o.width : lo);
                wpos[t] = (IT)a;
                wlen[t] = (IT)std::min<uint64_t>(n, p - a + (poff[i + 1] - poff[i]) + std::min<uint64_t>(o.width, n));
            }
        extract<IT>(s, d_fm, info, d_ts, o.text_rate, d_soff, m, wpos, wlen, wstart, windows);
    }
    std::cerr << "Search time: " << ms_since(t2) << " ms" << std::endl;
    auto place = [&](uint64_t t) {
        if (m && (uint64_t)sid[t] < m) std::cout << (uint64_t)sid[t] << ':' << (uint64_t)pos[t] - soff[(std::size_t)sid[t]];
        else std::cout << (uint64_t)pos[t];
    };
    for (uint64_t i = 0; i < q; ++i) {
        std::cout << (uint64_t)lb[i] << ' ' << (uint64_t)ub[i];
        if (o.occ)
            for (uint64_t t = start[i]; t < start[i + 1]; ++t) { std::cout << ' '; place(t); }
        std::cout << '\n';
        if (o.context)
            for (uint64_t t = start[i]; t < start[i + 1]; ++t) {
                std::cout << '\t'; place(t); std::cout << '\t';
                std::cout.write(windows.data() + wstart[t], (std::streamsize)(wstart[t + 1] - wstart[t]));
                std::cout << '\n';
            }
    }
    if (!o.restore.empty()) {
        auto t3 = std::chrono::steady_clock::now();
        std::vector<IT> rpos, rlen;
        if (!m) { rpos.push_back(0); rlen.push_back((IT)n); }
        for (uint64_t j = 0; j < m; ++j) { rpos.push_back((IT)soff[j]); rlen.push_back((IT)(soff[j + 1] - soff[j])); }
        std::vector<uint64_t> rstart;
        std::string bytes;
        extract<IT>(s, d_fm, info, d_ts, o.text_rate, d_soff, m, rpos, rlen, rstart, bytes);
        std::cerr << "Restore time: " << ms_since(t3) << " ms" << std::endl;
        std::ofstream f(o.restore.c_str(), std::ios::binary);
        for (std::size_t j = 0; j + 1 < rstart.size(); ++j) {
            f.write(bytes.data() + rstart[j], (std::streamsize)(rstart[j + 1] - rstart[j]));
            if (m) f.put('\n');
        }
        f.close();
        if (!f) throw std::runtime_error("cannot write " + o.restore);
    }
    return 0;
}

int main(int argc, char** argv) {
    std::string file, queries, index = "auto";
    Options o;
    o.sample = 32; o.limit = 0; o.occ = false; o.device = 0; o.text_rate = 0; o.width = 0; o.context = false;
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
        else if (a == "--text-rate") o.text_rate = count("--text-rate");
        else if (a == "--context") { o.context = true; o.width = count("--context"); }
        else if (a == "--restore") o.restore = need("--restore");
        else if (a == "--device") o.device = atoi(need("--device"));
        else if (a == "--index") index = need("--index");
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else { std::cerr << "error: unknown argument " << a << std::endl; usage(); return EXIT_FAILURE; }
    }
    if (file.empty() || queries.empty() || !index_known(index)) { usage(); return EXIT_FAILURE; }
    if (o.occ && o.sample == 0) { std::cerr << "error: --occ needs a sample rate above 0" << std::endl; usage(); return EXIT_FAILURE; }
    if ((o.context || !o.restore.empty()) && o.text_rate == 0) { std::cerr << "error: --context and --restore need --text-rate above 0" << std::endl; usage(); return EXIT_FAILURE; }
    if (o.context && !o.occ) { std::cerr << "error: --context needs --occ" << std::endl; usage(); return EXIT_FAILURE; }
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
