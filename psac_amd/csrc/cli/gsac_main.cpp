// gsac -- generalized suffix array of the lines of a file, the command line of
// /root/reference/src/gsac.cpp:139-204:  gsac -f <file> [-l] [-t] [-c] [--check-device] [-o <basename>] [--device N]
// Strings are the runs between '\n' (src/gsac.cpp:170); positions count the characters with the
// separators left out.  -o (extra) writes <basename>.sa64 / .lcp64 as psac does.
//
// -c: the reference compares with libdivsufsort on the separator-joined text and tolerates
// swapped equal suffixes (src/gsac.cpp:85-135).  Here neighbouring suffixes are compared
// directly, which also pins the order of equal suffixes (text order) and the LCP values.
// --check-device (extra): the arrays go back to HBM and the device checker gives the verdict (psacx_check_gsa_dev_u64; with
// --gpus / --gpus-on-device the distributed one, psacx_multi_check_gsa_dev_u64, on the ranks that built them): the same rules at sizes
// the walk below does not reach.
// -t (extra; implies -l): the generalized suffix tree's node table is built in HBM from the arrays (psacx_suffix_tree_gsa_dev_u64) and
// its edge count and time are printed as psac -t prints them; with --check-device psacx_check_suffix_tree_gsa_dev_u64 gives a verdict on
// the table too.  One GPU: with --gpus / --gpus-on-device it is an error.
#include <cstring>
#include <vector>

#include "../../../include/suffix_array.hpp"
#include "bench_common.hpp"

typedef uint64_t index_t;      // src/gsac.cpp:36

template <bool LCP>
static bool check_gsa(const suffix_array<char, index_t, LCP>& sa, const simple_dstringset& ss) {
    const std::size_t n = sa.n;
    std::string cat; cat.reserve(n);
    std::vector<std::size_t> end_of(n);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) {
        cat.append(ss.str_begins[s], ss.sizes[s]);
        for (std::size_t i = cat.size() - ss.sizes[s]; i < cat.size(); ++i) end_of[i] = cat.size();
    }
    if (sa.local_SA.size() != n) { std::cerr << "[ERROR] GSA has the wrong size" << std::endl; return false; }
    std::vector<bool> seen(n, false);
    for (std::size_t i = 0; i < n; ++i) {
        const std::size_t p = sa.local_SA[i];
        if (p >= n || seen[p]) { std::cerr << "[ERROR] gsa[" << i << "] is not part of a permutation" << std::endl; return false; }
        seen[p] = true;
        if (sa.local_B[p] != i) { std::cerr << "[ERROR] ISA[gsa[" << i << "]] != " << i << std::endl; return false; }
    }
    for (std::size_t i = 1; i < n; ++i) {
        std::size_t a = sa.local_SA[i - 1], b = sa.local_SA[i], c = 0;
        const std::size_t ea = end_of[a], eb = end_of[b];
        while (a + c < ea && b + c < eb && cat[a + c] == cat[b + c]) ++c;
        const bool a_end = a + c == ea, b_end = b + c == eb;
        bool ok;
        if (a_end && b_end) ok = a < b;                      // equal suffixes: text order
        else if (a_end) ok = true;
        else if (b_end) ok = false;
        else ok = (unsigned char)cat[a + c] < (unsigned char)cat[b + c];
        if (!ok) { std::cerr << "[ERROR] gsa[" << i - 1 << "] and gsa[" << i << "] are out of order" << std::endl; return false; }
        if (LCP && sa.local_LCP[i] != c) { std::cerr << "[ERROR] lcp[" << i << "] = " << sa.local_LCP[i] << ", expected " << c << std::endl; return false; }
    }
    if (LCP && n && sa.local_LCP[0] != 0) { std::cerr << "[ERROR] lcp[0] != 0" << std::endl; return false; }
    std::cout << "[SUCCESS] GSA correct" << std::endl;       // src/gsac.cpp:132-134
    return true;
}

// one device buffer per call of get(); freed with the object
struct DevBufs {
    psacx_ctx* c;
    std::vector<void*> held;
    explicit DevBufs(psacx_ctx* c_) : c(c_) {}
    ~DevBufs() { for (std::size_t i = 0; i < held.size(); ++i) psacx_dev_free(c, held[i]); }
    void* get(const void* src, uint64_t bytes) {
        void* p = nullptr;
        psacx::check(c, psacx_dev_alloc(c, &p, bytes));
        held.push_back(p);
        if (bytes) psacx::check(c, psacx_copy_h2d(c, p, src, bytes));
        return p;
    }
};

template <bool LCP>
static bool check_gsa_on_device(suffix_array<char, index_t, LCP>& sa, const simple_dstringset& ss) {
    static_assert(sizeof(index_t) == 8, "the 64-bit entry points are called");
    const uint64_t n = sa.n;
    std::vector<uint8_t> cat; cat.reserve(n);
    std::vector<uint64_t> off(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) {
        cat.insert(cat.end(), reinterpret_cast<const uint8_t*>(ss.str_begins[s]), reinterpret_cast<const uint8_t*>(ss.str_begins[s]) + ss.sizes[s]);
        off.push_back(cat.size());
    }
    if (sa.local_SA.size() != n || sa.local_B.size() != n) { std::cerr << "[ERROR] GSA has the wrong size" << std::endl; return false; }
    const uint64_t* SA = reinterpret_cast<const uint64_t*>(sa.local_SA.data());
    const uint64_t* ISA = reinterpret_cast<const uint64_t*>(sa.local_B.data());
    const uint64_t* L = LCP ? reinterpret_cast<const uint64_t*>(sa.local_LCP.data()) : nullptr;
    uint64_t err[4] = {0, 0, 0, 0};
    if (psacx_multi* mg = sa.multi_context()) {
        const int P = psacx_multi_nlocal(mg);
        std::vector<DevBufs*> bufs;
        std::vector<const uint8_t*> t(P); std::vector<const uint64_t*> a(P), b(P), c(P); std::vector<uint64_t> m(P);
        uint64_t first = 0;
        int rc = PSACX_OK;
        try {
            for (int r = 0; r < P; ++r) {                   // mxx::blk_dist: the first n % P ranks hold one character more
                m[r] = n / P + ((uint64_t)r < n % P ? 1 : 0);
                bufs.push_back(new DevBufs(psacx_multi_ctx(mg, r)));
                t[r] = (const uint8_t*)bufs[r]->get(cat.data() + first, m[r]);
                a[r] = (const uint64_t*)bufs[r]->get(SA + first, m[r] * 8);
                b[r] = (const uint64_t*)bufs[r]->get(ISA + first, m[r] * 8);
                c[r] = LCP ? (const uint64_t*)bufs[r]->get(L + first, m[r] * 8) : nullptr;
                first += m[r];
            }
            rc = psacx_multi_check_gsa_dev_u64(mg, t.data(), m.data(), off.data(), (uint64_t)ss.sizes.size(), a.data(), b.data(), LCP ? c.data() : nullptr, err);
        } catch (...) { for (std::size_t i = 0; i < bufs.size(); ++i) delete bufs[i]; throw; }
        for (std::size_t i = 0; i < bufs.size(); ++i) delete bufs[i];
        if (rc != PSACX_OK) throw std::runtime_error(std::string("psacx: ") + psacx_strerror(rc) + " [" + psacx_multi_last_error(mg) + "]");
    } else {
        psacx_ctx* cx = sa.context();
        DevBufs d(cx);
        const uint8_t* t = (const uint8_t*)d.get(cat.data(), n);
        const uint64_t* o = (const uint64_t*)d.get(off.data(), off.size() * 8);
        const uint64_t* a = (const uint64_t*)d.get(SA, n * 8);
        const uint64_t* b = (const uint64_t*)d.get(ISA, n * 8);
        const uint64_t* c = LCP ? (const uint64_t*)d.get(L, n * 8) : nullptr;
        psacx::check(cx, psacx_check_gsa_dev_u64(cx, t, n, o, (uint64_t)ss.sizes.size(), a, b, c, err));
    }
    if (err[0] | err[1] | err[2] | err[3]) {
        std::cerr << "[ERROR] GSA wrong: " << err[0] << " entries out of range or not inverse to ISA, " << err[1] << " out of order, " << err[2]
                  << " LCP values wrong, LCP[0] != 0: " << err[3] << std::endl;
        return false;
    }
    std::cout << "[SUCCESS] GSA correct" << std::endl;
    return true;
}

// gsac -t: text, offsets, SA and LCP go (back) to HBM, the table is built and stays there
static bool tree_on_device(suffix_array<char, index_t, true>& sa, const simple_dstringset& ss, bool check_device) {
    static_assert(sizeof(index_t) == 8, "the 64-bit entry points are called");
    const uint64_t n = sa.n, m = ss.sizes.size();
    std::vector<uint8_t> cat; cat.reserve(n);
    std::vector<uint64_t> off(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) {
        cat.insert(cat.end(), reinterpret_cast<const uint8_t*>(ss.str_begins[s]), reinterpret_cast<const uint8_t*>(ss.str_begins[s]) + ss.sizes[s]);
        off.push_back(cat.size());
    }
    psacx_ctx* cx = sa.context();
    DevBufs d(cx);
    const uint8_t* t = (const uint8_t*)d.get(cat.data(), n);
    const uint64_t* o = (const uint64_t*)d.get(off.data(), off.size() * 8);
    const uint64_t* a = (const uint64_t*)d.get(sa.local_SA.data(), n * 8);
    const uint64_t* l = (const uint64_t*)d.get(sa.local_LCP.data(), n * 8);
    bench_cli::Clock clk;
    uint32_t sigma = 0;
    uint64_t edges = 0;
    psacx::check(cx, psacx_suffix_tree_gsa_dev_u64(cx, t, n, o, m, nullptr, nullptr, nullptr, &sigma, nullptr));
    void* p = nullptr;
    psacx::check(cx, psacx_dev_alloc(cx, &p, n * ((uint64_t)sigma + 2) * sizeof(uint64_t)));
    d.held.push_back(p);
    psacx::check(cx, psacx_suffix_tree_gsa_dev_u64(cx, t, n, o, m, a, l, (uint64_t*)p, &sigma, &edges));
    std::cerr << "ST time: " << clk.elapsed() << " ms" << std::endl;
    std::cerr << "ST edges: " << edges << std::endl;
    if (!check_device) return true;
    uint64_t out[4] = {0, 0, 0, 0};
    psacx::check(cx, psacx_check_suffix_tree_gsa_dev_u64(cx, t, n, o, m, a, l, (const uint64_t*)p, out));
    if (out[0] | out[1] | (out[2] != edges)) {
        std::cerr << "[ERROR] Suffix Tree is wrong: " << out[0] << " records not in their cell, " << out[1] << " cells without a record" << std::endl;
        return false;
    }
    std::cout << "[SUCCESS] Suffix Tree is correct" << std::endl;
    return true;
}
static bool tree_on_device(suffix_array<char, index_t, false>&, const simple_dstringset&, bool) { return true; }

template <typename V> static void write_u64(const std::string& fn, const std::vector<V>& v) {
    std::ofstream f(fn.c_str(), std::ios::binary | std::ios::trunc);
    for (std::size_t i = 0; i < v.size(); ++i) { const uint64_t x = (uint64_t)v[i]; f.write(reinterpret_cast<const char*>(&x), 8); }
    if (!f) { std::cerr << "error: cannot write " << fn << std::endl; exit(EXIT_FAILURE); }
}

template <bool LCP>
static int run(const std::string& str, bool check, bool check_device, bool tree, const std::string& out, int device, const std::vector<int>& devices) {
    simple_dstringset ss(str.begin(), str.end(), psacx::comm(device), '\n');
    if (ss.sum_sizes == 0) { std::cerr << "error: no strings in the input" << std::endl; return EXIT_FAILURE; }
    psacx::alphabet<char> alpha = psacx::alphabet<char>::from_stringset(ss, psacx::comm(device));
    bench_cli::Clock t;
    // --gpus N / --gpus-on-device D,N: the string set is block-distributed over the ranks of the communicator
    suffix_array<char, index_t, LCP> sa(devices.empty() ? psacx::comm(device) : psacx::comm(devices));
    sa.construct_ss(ss, alpha);
    std::cerr << "PSAC time: " << t.elapsed() << " ms" << std::endl;
    if (check && !check_gsa<LCP>(sa, ss)) return 1;
    if (check_device && !check_gsa_on_device<LCP>(sa, ss)) return 1;
    if (tree && !tree_on_device(sa, ss, check_device)) return 1;
    if (!out.empty()) {
        write_u64(out + ".sa64", sa.local_SA);
        if (LCP) write_u64(out + ".lcp64", sa.local_LCP);
    }
    return 0;
}

int main(int argc, char** argv) {
    bool check_device = false;              // the one long switch: taken out before the shared parser sees the line
    for (int i = 1; i < argc; ) {
        if (std::string(argv[i]) != "--check-device") { ++i; continue; }
        check_device = true;
        for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
        --argc;
    }
    bench_cli::Args a(argc, argv, "fo", "lct");
    if (!a.ok || !a.has("-f")) {
        std::cerr << "USAGE: gsac -f <filename> [-l] [-t] [-c] [--check-device] [-o <basename>] [--device N] [--gpus N] [--gpus-on-device D,N]\n"
                     "Parallel distributed generalized suffix array and LCP construction (MI355X engine)." << std::endl;
        return EXIT_FAILURE;
    }
    std::string str;
    if (!bench_cli::read_file(a.str("-f"), str)) { std::cerr << "error: cannot open " << a.str("-f") << std::endl; return EXIT_FAILURE; }
    const int device = (int)a.num("--device", 0);
    std::vector<int> devices;
    for (int i = 1; i + 1 < argc; ++i) {
        const std::string f = argv[i], v = argv[i + 1];
        if (f == "--gpus") for (int d = 0; d < atoi(v.c_str()); ++d) devices.push_back(d);
        if (f == "--gpus-on-device") {
            const std::size_t c = v.find(',');
            devices.assign((std::size_t)std::max(c == std::string::npos ? 1 : atoi(v.substr(c + 1).c_str()), 1), atoi(v.substr(0, c).c_str()));
        }
    }
    const bool tree = a.has("-t");
    if (tree && !devices.empty()) { std::cerr << "error: -t builds the tree on one GPU; it does not go with --gpus / --gpus-on-device" << std::endl; return EXIT_FAILURE; }
    try {
        return a.has("-l") || tree ? run<true>(str, a.has("-c"), check_device, tree, a.str("-o"), device, devices)
                                   : run<false>(str, a.has("-c"), check_device, false, a.str("-o"), device, devices);
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return EXIT_FAILURE;
    }
}
