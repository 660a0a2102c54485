// suffix_array.hpp -- C++11 host mirror of psac's suffix_array<> class over libpsacx.so.
//
// Same class name, template parameters, public fields and construct() signatures as
// /root/reference/include/suffix_array.hpp:170-228, :365-486, so that a caller such as
// src/psac.cpp:117-128 compiles against this header unchanged apart from the communicator
// type: the reference takes an mxx::comm (one MPI rank per text block); this engine takes a
// psacx::comm naming the HIP device(s): one device = one rank; several devices = that many ranks,
// one GPU each, all driven by this process (the text is block-decomposed over them exactly as
// src/psac.cpp:85-93 decomposes it over MPI ranks, the exchanges run over RCCL).  All compute happens in the
// HIP engine behind the C ABI of psacx.h; this header only moves data and re-throws errors
// (std::runtime_error, as suffix_array.hpp:226-227 does).
#ifndef PSACX_SUFFIX_ARRAY_HPP
#define PSACX_SUFFIX_ARRAY_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <fstream>
#include <limits>
#include <iostream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "psacx.h"

namespace psacx {

// Stand-in for mxx::comm (Appendix A of SURVEY.md lists the surface psac uses).  One process holds every rank:
// rank() is 0, size() the number of GPUs (ranks) the communicator spans.
class comm {
public:
    explicit comm(int device = 0) : devices_(1, device) {}
    explicit comm(const std::vector<int>& devices) : devices_(devices.empty() ? std::vector<int>(1, 0) : devices) {}
    int rank() const { return 0; }
    int size() const { return (int)devices_.size(); }
    bool is_first() const { return true; }
    int device() const { return devices_[0]; }
    const std::vector<int>& devices() const { return devices_; }
    comm copy() const { return comm(devices_); }
private:
    std::vector<int> devices_;
};

// mxx::blk_dist at one rank (suffix_array.hpp:194, bulk_permute.hpp:23)
struct blk_dist {
    std::size_t n;
    blk_dist() : n(0) {}
    explicit blk_dist(std::size_t n_) : n(n_) {}
    std::size_t global_size() const { return n; }
    std::size_t local_size() const { return n; }
    std::size_t eprefix_size() const { return 0; }
    std::size_t iprefix_size() const { return n; }
    int rank_of(std::size_t) const { return 0; }
};

// characters compare by their unsigned value (alphabet.hpp:205-236)
template <typename char_t> struct unsigned_less {
    bool operator()(char_t a, char_t b) const { typedef typename std::make_unsigned<char_t>::type u; return (u)a < (u)b; }
};

// the part of alphabet<char> callers read (alphabet.hpp:147-164, :224-262, :296-300)
template <typename char_t> class alphabet {
public:
    alphabet() : m_sigma(0), m_bits(0) {}
    unsigned int sigma() const { return m_sigma; }
    unsigned int size() const { return m_sigma; }
    unsigned int bits_per_char() const { return m_bits; }
    template <typename word_type> unsigned int chars_per_word() const {
        unsigned int b = sizeof(word_type) * 8;
        if (std::is_signed<word_type>::value) --b;
        return b / m_bits;
    }
    const std::vector<char_t>& unique_chars() const { return m_chars; }
    void write(const std::string& filename) const {
        std::ofstream f(filename.c_str(), std::ios::binary);
        for (std::size_t i = 0; i < m_chars.size(); ++i) f.write(reinterpret_cast<const char*>(&m_chars[i]), sizeof(char_t));
    }
    // alphabet.hpp:205-236: the characters that occur, ascending by unsigned value
    template <typename Iterator>
    static alphabet from_sequence(Iterator begin, Iterator end) {
        typedef typename std::make_unsigned<char_t>::type uchar_t;
        std::vector<uchar_t> u;
        for (Iterator it = begin; it != end; ++it) u.push_back((uchar_t)*it);
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        std::vector<char_t> chars;
        for (std::size_t i = 0; i < u.size(); ++i) chars.push_back((char_t)u[i]);
        alphabet a; a.set(chars); return a;
    }
    template <typename Iterator, typename Comm>
    static alphabet from_sequence(Iterator begin, Iterator end, const Comm&) { return from_sequence(begin, end); }
    static alphabet from_string(const std::basic_string<char_t>& str) { return from_sequence(str.begin(), str.end()); }
    template <typename Comm>
    static alphabet from_string(const std::basic_string<char_t>& str, const Comm&) { return from_sequence(str.begin(), str.end()); }
    template <typename StringSet, typename Comm>
    static alphabet from_stringset(const StringSet& ss, const Comm&) {
        std::basic_string<char_t> all;
        for (std::size_t s = 0; s < ss.sizes.size(); ++s) all.append(ss.str_begins[s], ss.str_begins[s] + ss.sizes[s]);
        return from_string(all);
    }
    // alphabet.hpp:303-311, :328-331: the used characters, ascending
    void read(const std::string& filename) {
        std::ifstream f(filename.c_str(), std::ios::binary);
        if (!f) throw std::runtime_error("cannot read " + filename);
        std::vector<char_t> chars; char_t c;
        while (f.read(reinterpret_cast<char*>(&c), sizeof(char_t))) chars.push_back(c);
        set(chars);
    }
    bool operator==(const alphabet& o) const { return m_chars == o.m_chars; }     // alphabet.hpp:286-288
    bool operator!=(const alphabet& o) const { return !(*this == o); }
    void set(const std::vector<char_t>& chars) {
        m_chars = chars; m_sigma = (unsigned int)chars.size();
        m_bits = 0; while ((1u << m_bits) < m_sigma + 1u) ++m_bits;
    }
private:
    std::vector<char_t> m_chars;
    unsigned int m_sigma, m_bits;
};

template <typename char_t> std::ostream& operator<<(std::ostream& os, const alphabet<char_t>& a) {
    os << "{sigma=" << a.sigma() << ", l=" << a.bits_per_char() << ", A=[";
    for (std::size_t i = 0; i < a.unique_chars().size(); ++i) os << (i ? ", " : "") << a.unique_chars()[i];
    return os << "]}";
}

inline void check(psacx_ctx* ctx, int rc) {
    if (rc == PSACX_OK) return;
    std::string msg = std::string("psacx: ") + psacx_strerror(rc);
    const char* d = ctx ? psacx_last_hip_error(ctx) : "";
    if (d && *d) msg += std::string(" [") + d + "]";
    throw std::runtime_error(msg);
}

} // namespace psacx

// simple_dstringset of /root/reference/include/stringset.hpp:33-151 on one rank: the strings of a
// flat buffer, cut at runs of the separator; empty strings do not exist.
class simple_dstringset {
public:
    bool first_split, last_split;              // never set on one rank (stringset.hpp:74-80)
    std::vector<const char*> str_begins;
    std::vector<std::size_t> sizes;
    std::size_t sum_sizes;

    template <typename Iterator>
    simple_dstringset(Iterator begin, Iterator end, const psacx::comm&, char sep = '$')
        : first_split(false), last_split(false), sum_sizes(0) {
        Iterator it = begin;
        while (it != end && *it == sep) ++it;
        while (it != end) {
            Iterator e = it;
            while (e != end && *e != sep) ++e;
            sizes.push_back((std::size_t)std::distance(it, e));
            sum_sizes += sizes.back();
            str_begins.push_back(&(*it));
            it = e;
            while (it != end && *it == sep) ++it;
        }
    }
};

// stringset.hpp:586-600: every string followed by the separator
inline std::string flatten_strings(const std::vector<std::string>& strs, char sep = '$') {
    std::string out;
    for (std::size_t i = 0; i < strs.size(); ++i) { out += strs[i]; out.push_back(sep); }
    return out;
}

#ifndef PSACX_INFO
#define PSACX_INFO(msg) { std::cerr << msg << std::endl; }
#endif

template <typename char_t, typename index_t = std::size_t, bool _CONSTRUCT_LCP = false, bool _CONSTRUCT_LC = false>
class suffix_array {
    static_assert(sizeof(index_t) == 4 || sizeof(index_t) == 8, "index_t must be a 32 or 64 bit unsigned integer");
    static_assert(!_CONSTRUCT_LC || _CONSTRUCT_LCP, "_CONSTRUCT_LC needs _CONSTRUCT_LCP (the reference fills Lc inside its LCP code)");
public:
    explicit suffix_array(const psacx::comm& _comm)
        : n(0), local_size(0), comm(_comm.copy()), p(_comm.size()), verbose(true), ctx_(nullptr), multi_(nullptr) {
        psacx::check(nullptr, psacx_create(&ctx_, comm.device(), nullptr));
        if (p > 1) {
            const int rc = psacx_multi_create(&multi_, p, comm.devices().data());
            if (rc != PSACX_OK) { psacx_destroy(ctx_); ctx_ = nullptr; psacx::check(nullptr, rc); }
        }
    }
    virtual ~suffix_array() { if (multi_) psacx_multi_destroy(multi_); if (ctx_) psacx_destroy(ctx_); }
    suffix_array(const suffix_array&) = delete;
    suffix_array& operator=(const suffix_array&) = delete;

    /// The global size of the input string and suffix array (suffix_array.hpp:180)
    std::size_t n;
    /// The local size (== n: this process holds the blocks of all p ranks, in rank order) (suffix_array.hpp:185)
    std::size_t local_size;
    psacx::comm comm;
    /// number of ranks = GPUs the construction is distributed over (suffix_array.hpp:191)
    int p;
    psacx::blk_dist part;
    using char_type = char_t;
    using alphabet_type = psacx::alphabet<char_t>;
    alphabet_type alpha;
    /// The suffix array, the inverse suffix array (0-based) and the LCP array
    /// (suffix_array.hpp:204-209); local_LCP stays empty unless _CONSTRUCT_LCP.
    std::vector<index_t> local_SA;
    std::vector<index_t> local_B;
    std::vector<index_t> local_LCP;
    /// left-branching characters Lc[i] = S[SA[i-1] + LCP[i]] (suffix_array.hpp:211-212), '\0' past
    /// the end; stays empty unless _CONSTRUCT_LC
    std::vector<char_t> local_Lc;
    bool verbose;                     // print the reference's stderr lines

    void init_size(std::size_t lsize) {      // suffix_array.hpp:217-228
        local_size = lsize; n = lsize; part = psacx::blk_dist(n);
    }

    // suffix_array.hpp:469-486
    template <typename Iterator>
    void construct(Iterator begin, Iterator end, bool fast_resolval = true, unsigned int k = 0) {
        construct_with(begin, end, fast_resolval, k, nullptr);
    }
    // suffix_array.hpp:365-366: the alphabet and k come from the caller (an alphabet that covers more characters than occur is
    // fine: SA, ISA and LCP do not depend on the coding, which only has to keep the order of the characters; a character
    // outside it is an error).  `alpha` is the caller's afterwards, as in the reference.
    template <typename Iterator>
    void construct(Iterator begin, Iterator end, bool fast_resolval, const alphabet_type& a, unsigned int k) {
        construct_with(begin, end, fast_resolval, k, &a);
    }

private:
    template <typename Iterator>
    void construct_with(Iterator begin, Iterator end, bool fast_resolval, unsigned int k, const alphabet_type* given) {
        init_size((std::size_t)std::distance(begin, end));
        if (n == 0) throw std::runtime_error("psacx: empty input");
        std::vector<uint8_t> bytes(n);
        std::vector<char_t> chars;
        const unsigned w = densify(begin, end, bytes, chars);
        if (given) {
            const std::vector<char_t>& have = given->unique_chars();
            for (std::size_t i = 0; i < chars.size(); ++i)
                if (!std::binary_search(have.begin(), have.end(), chars[i], psacx::unsigned_less<char_t>()))
                    throw std::runtime_error("psacx: the text holds a character that is not in the given alphabet");
            if (k == 0) throw std::runtime_error("psacx: construct with an explicit alphabet needs k > 0");
            const unsigned int kmax = given->template chars_per_word<index_t>();
            if (k > kmax) k = kmax;
        }
        local_SA.assign(n, 0); local_B.assign(n, 0);
        if (_CONSTRUCT_LCP) local_LCP.assign(n, 0); else local_LCP.clear();
        uint32_t flags = (_CONSTRUCT_LCP ? PSACX_LCP : 0u) | (fast_resolval ? 0u : PSACX_NO_FAST);
        std::vector<uint8_t> lc;
        if (_CONSTRUCT_LC) lc.assign(n, 0);
        int rc;
        if (w > 1) {
            // more than 256 distinct symbols: the engine builds the arrays of the text of w bytes per symbol, reduce_wide keeps the
            // suffixes that start on a symbol boundary
            if ((uint64_t)n * w > (uint64_t)std::numeric_limits<index_t>::max())
                throw std::runtime_error("psacx: the text of this many distinct symbols needs a wider index type");
            if (multi_ && !fast_resolval) throw std::runtime_error("psacx: fast_resolval = false needs a single-rank communicator");
            struct length_guard {                       // run() and run_multi() read the length from the object
                std::size_t& n; std::size_t n0;
                length_guard(std::size_t& n_, std::size_t bytes_) : n(n_), n0(n_) { n = bytes_; }
                ~length_guard() { n = n0; }
            };
            std::vector<index_t> sa((std::size_t)n * w), isa((std::size_t)n * w), lcp;
            if (_CONSTRUCT_LCP) lcp.assign((std::size_t)n * w, 0);
            {
                length_guard g(n, (std::size_t)n * w);
                rc = multi_ ? run_multi(bytes.data(), k * w, flags, sa.data(), isa.data(), _CONSTRUCT_LCP ? lcp.data() : nullptr, nullptr)
                            : run(bytes.data(), k * w, flags, sa.data(), isa.data(), _CONSTRUCT_LCP ? lcp.data() : nullptr, nullptr);
            }
            if (multi_) {
                if (rc != PSACX_OK) throw std::runtime_error(std::string("psacx: ") + (rc > -7 ? psacx_strerror(rc) : "RCCL failure") + " [" +
                                                             psacx_multi_last_error(multi_) + "]");
            } else psacx::check(ctx_, rc);
            reduce_wide(w, sa, lcp);
        } else if (multi_) {
            // p ranks, one GPU each: blocks of n / p characters (mxx::blk_dist), results gathered in rank order
            if (!fast_resolval) throw std::runtime_error("psacx: fast_resolval = false needs a single-rank communicator");
            rc = run_multi(bytes.data(), k, flags, local_SA.data(), local_B.data(), _CONSTRUCT_LCP ? local_LCP.data() : nullptr,
                           _CONSTRUCT_LC ? lc.data() : nullptr);
            if (rc != PSACX_OK) throw std::runtime_error(std::string("psacx: ") + (rc > -7 ? psacx_strerror(rc) : "RCCL failure") + " [" +
                                                         psacx_multi_last_error(multi_) + "]");
        } else {
            rc = run(bytes.data(), k, flags, local_SA.data(), local_B.data(), _CONSTRUCT_LCP ? local_LCP.data() : nullptr,
                     _CONSTRUCT_LC ? lc.data() : nullptr);
            psacx::check(ctx_, rc);
        }
        local_Lc.clear();
        if (_CONSTRUCT_LC) {
            // positions past the end carry '\0' (alphabet.hpp:168); they are exactly those with SA[i-1] + LCP[i] == n
            local_Lc.assign(n, (char_t)0);
            std::vector<char_t> sym;
            if (w > 1) sym.assign(begin, end);          // (wide symbols: the character itself, read from the caller's text)
            for (std::size_t i = 1; i < n; ++i) {
                const std::size_t at = (std::size_t)local_SA[i - 1] + (std::size_t)local_LCP[i];
                if (at >= n) continue;
                local_Lc[i] = w > 1 ? sym[at] : sizeof(char_t) == 1 ? (char_t)lc[i] : chars[lc[i]];
            }
        }
        psacx_stats st;
        if (multi_) psacx::check(nullptr, psacx_multi_get_stats(multi_, &st, nullptr, nullptr, nullptr));
        else psacx::check(ctx_, psacx_get_stats(ctx_, &st));
        if (given) alpha = *given; else alpha.set(chars);
        if (verbose) {
            PSACX_INFO("Alphabet: " << alpha);                       // suffix_array.hpp:481
            for (uint32_t r = 0; r < st.n_rounds; ++r)                // suffix_array.hpp:416
                PSACX_INFO("iteration " << st.rounds[r].h << ": unfinished buckets = " << st.rounds[r].unfinished_buckets
                           << ", unfinished elements = " << st.rounds[r].unfinished_elements);
        }
    }

public:
    // suffix_array.hpp:267-363: generalized suffix array of a string set.  local_SA counts positions
    // in the strings laid back to back without separators; equal suffixes come in that order.
    void construct_ss(simple_dstringset& ss, const alphabet_type& a) {
        static_assert(sizeof(char_t) == 1, "string sets hold bytes");
        static_assert(!_CONSTRUCT_LC, "left-branching characters are not defined for string sets");
        init_size(ss.sum_sizes);
        if (n == 0) throw std::runtime_error("psacx: empty input");
        std::vector<uint8_t> bytes; bytes.reserve(n);
        std::vector<uint64_t> off(1, 0);
        for (std::size_t s = 0; s < ss.sizes.size(); ++s) {
            bytes.insert(bytes.end(), reinterpret_cast<const uint8_t*>(ss.str_begins[s]),
                         reinterpret_cast<const uint8_t*>(ss.str_begins[s]) + ss.sizes[s]);
            off.push_back(bytes.size());
        }
        local_SA.assign(n, 0); local_B.assign(n, 0);
        if (_CONSTRUCT_LCP) local_LCP.assign(n, 0); else local_LCP.clear();
        const uint32_t flags = _CONSTRUCT_LCP ? PSACX_LCP : 0u;
        psacx_stats st;
        if (multi_) {
            // p > 1: the strings lie back to back in the block-distributed text (psacx_multi_construct_gsa_*)
            const int rc = run_gsa_multi(bytes.data(), off.data(), (uint64_t)ss.sizes.size(), flags, local_SA.data(), local_B.data(),
                                         _CONSTRUCT_LCP ? local_LCP.data() : nullptr);
            if (rc != PSACX_OK) throw std::runtime_error(std::string("psacx: ") + psacx_strerror(rc) + " [" + psacx_multi_last_error(multi_) + "]");
            psacx::check(nullptr, psacx_multi_get_stats(multi_, &st, nullptr, nullptr, nullptr));
        } else {
            psacx::check(ctx_, run_gsa(bytes.data(), off.data(), (uint64_t)ss.sizes.size(), flags, local_SA.data(), local_B.data(),
                                       _CONSTRUCT_LCP ? local_LCP.data() : nullptr));
            psacx::check(ctx_, psacx_get_stats(ctx_, &st));
        }
        alpha = a;
        if (verbose) {
            PSACX_INFO("Alphabet: " << alpha);                       // suffix_array.hpp:273-275
            for (uint32_t r = 0; r < st.n_rounds; ++r)                // suffix_array.hpp:317
                PSACX_INFO("iteration " << st.rounds[r].h << ": unfinished buckets = " << st.rounds[r].unfinished_buckets
                           << ", unfinished elements = " << st.rounds[r].unfinished_elements);
        }
    }

    // suffix_array.hpp:232-242: raw little-endian arrays, no header
    void write(const std::string& basename) const {
        dump(basename + ".sa", local_SA);
        if (_CONSTRUCT_LCP) dump(basename + ".lcp", local_LCP);
        if (_CONSTRUCT_LC) dump(basename + ".lc", local_Lc);
        alpha.write(basename + ".alpha");
    }
    // suffix_array.hpp:245-265
    void read(const std::string& basename) {
        slurp(basename + ".sa", local_SA);
        if (_CONSTRUCT_LCP) {
            slurp(basename + ".lcp", local_LCP);
            if (local_SA.size() != local_LCP.size()) throw std::runtime_error("SA and LCP have to have same size");
        }
        if (_CONSTRUCT_LC) {
            slurp(basename + ".lc", local_Lc);
            if (local_SA.size() != local_Lc.size()) throw std::runtime_error("SA and Lc have to have same size");
        }
        alpha.read(basename + ".alpha");
        init_size(local_SA.size());
    }

    psacx_ctx* context() { return ctx_; }
    psacx_multi* multi_context() { return multi_; }

private:
    psacx_ctx* ctx_;
    psacx_multi* multi_;

    // (lc != nullptr: also the left-branching characters, psacx_multi_construct_lc_*)
    int run_multi(const uint8_t* t, unsigned int k, uint32_t flags, uint32_t* sa, uint32_t* isa, uint32_t* lcp, uint8_t* lc) {
        return lc ? psacx_multi_construct_lc_u32(multi_, t, n, k, flags, sa, isa, lcp, lc) : psacx_multi_construct_u32(multi_, t, n, k, flags, sa, isa, lcp);
    }
    int run_multi(const uint8_t* t, unsigned int k, uint32_t flags, uint64_t* sa, uint64_t* isa, uint64_t* lcp, uint8_t* lc) {
        return lc ? psacx_multi_construct_lc_u64(multi_, t, n, k, flags, sa, isa, lcp, lc) : psacx_multi_construct_u64(multi_, t, n, k, flags, sa, isa, lcp);
    }
    template <typename U>
    typename std::enable_if<!std::is_same<U, uint32_t>::value && !std::is_same<U, uint64_t>::value, int>::type
    run_multi(const uint8_t* t, unsigned int k, uint32_t flags, U* sa, U* isa, U* lcp, uint8_t* lc) {
        typedef typename std::conditional<sizeof(U) == 4, uint32_t, uint64_t>::type W;
        return run_multi(t, k, flags, reinterpret_cast<W*>(sa), reinterpret_cast<W*>(isa), reinterpret_cast<W*>(lcp), lc);
    }

    int run(const uint8_t* t, unsigned int k, uint32_t flags, uint32_t* sa, uint32_t* isa, uint32_t* lcp, uint8_t* lc) {
        return lc ? psacx_construct_lc_u32(ctx_, t, n, k, flags, sa, isa, lcp, lc) : psacx_construct_u32(ctx_, t, n, k, flags, sa, isa, lcp);
    }
    int run(const uint8_t* t, unsigned int k, uint32_t flags, uint64_t* sa, uint64_t* isa, uint64_t* lcp, uint8_t* lc) {
        return lc ? psacx_construct_lc_u64(ctx_, t, n, k, flags, sa, isa, lcp, lc) : psacx_construct_u64(ctx_, t, n, k, flags, sa, isa, lcp);
    }
    int run_gsa(const uint8_t* t, const uint64_t* off, uint64_t m, uint32_t flags, uint32_t* sa, uint32_t* isa, uint32_t* lcp) {
        return psacx_construct_gsa_u32(ctx_, t, n, off, m, 0, flags, sa, isa, lcp);
    }
    int run_gsa(const uint8_t* t, const uint64_t* off, uint64_t m, uint32_t flags, uint64_t* sa, uint64_t* isa, uint64_t* lcp) {
        return psacx_construct_gsa_u64(ctx_, t, n, off, m, 0, flags, sa, isa, lcp);
    }
    int run_gsa_multi(const uint8_t* t, const uint64_t* off, uint64_t m, uint32_t flags, uint32_t* sa, uint32_t* isa, uint32_t* lcp) {
        return psacx_multi_construct_gsa_u32(multi_, t, n, off, m, 0, flags, sa, isa, lcp);
    }
    int run_gsa_multi(const uint8_t* t, const uint64_t* off, uint64_t m, uint32_t flags, uint64_t* sa, uint64_t* isa, uint64_t* lcp) {
        return psacx_multi_construct_gsa_u64(multi_, t, n, off, m, 0, flags, sa, isa, lcp);
    }
    template <typename U>
    typename std::enable_if<!std::is_same<U, uint32_t>::value && !std::is_same<U, uint64_t>::value, int>::type
    run_gsa_multi(const uint8_t* t, const uint64_t* off, uint64_t m, uint32_t flags, U* sa, U* isa, U* lcp) {
        typedef typename std::conditional<sizeof(U) == 4, uint32_t, uint64_t>::type W;
        return run_gsa_multi(t, off, m, flags, reinterpret_cast<W*>(sa), reinterpret_cast<W*>(isa), reinterpret_cast<W*>(lcp));
    }
    template <typename U>
    typename std::enable_if<!std::is_same<U, uint32_t>::value && !std::is_same<U, uint64_t>::value, int>::type
    run_gsa(const uint8_t* t, const uint64_t* off, uint64_t m, uint32_t flags, U* sa, U* isa, U* lcp) {
        typedef typename std::conditional<sizeof(U) == 4, uint32_t, uint64_t>::type W;
        return run_gsa(t, off, m, flags, reinterpret_cast<W*>(sa), reinterpret_cast<W*>(isa), reinterpret_cast<W*>(lcp));
    }
    template <typename U>
    typename std::enable_if<!std::is_same<U, uint32_t>::value && !std::is_same<U, uint64_t>::value, int>::type
    run(const uint8_t* t, unsigned int k, uint32_t flags, U* sa, U* isa, U* lcp, uint8_t* lc) {
        typedef typename std::conditional<sizeof(U) == 4, uint32_t, uint64_t>::type W;
        return run(t, k, flags, reinterpret_cast<W*>(sa), reinterpret_cast<W*>(isa), reinterpret_cast<W*>(lcp), lc);
    }

    // bytes pass through; wider symbols (int alphabets, test/test_psac.cpp:277-304) are ranked among the distinct symbols that occur,
    // which keeps their order.  At most 256 of them: one byte per symbol.  More (the reference's alphabet<int> is unbounded,
    // alphabet.hpp:205-236): the rank as w = 2, 3 or 4 bytes, most significant first -- fixed-width big-endian codes compare as the
    // symbols do, so the suffixes of the byte text that start on a symbol boundary stand in the order of the symbol text's suffixes
    // (reduce_wide below).  Returns w.
    template <typename Iterator>
    unsigned densify(Iterator begin, Iterator end, std::vector<uint8_t>& bytes, std::vector<char_t>& chars) {
        typedef typename std::make_unsigned<char_t>::type uchar_t;
        chars.clear();
        if (sizeof(char_t) == 1) {
            bool used[256] = {false};
            std::size_t i = 0;
            for (Iterator it = begin; it != end; ++it, ++i) { const uint8_t b = (uint8_t)(uchar_t)*it; bytes[i] = b; used[b] = true; }
            for (int ch = 0; ch < 256; ++ch) if (used[ch]) chars.push_back((char_t)(uchar_t)ch);
            return 1;
        }
        std::vector<uchar_t> u; u.reserve(n);
        for (Iterator it = begin; it != end; ++it) u.push_back((uchar_t)*it);
        std::vector<uchar_t> uniq(u);                   // distinct symbols, ascending by unsigned value
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        for (std::size_t i = 0; i < uniq.size(); ++i) chars.push_back((char_t)uniq[i]);
        unsigned w = 1;
        while (w < 4 && (uniq.size() - 1) >> (8 * w)) ++w;
        if ((uint64_t)(uniq.size() - 1) >> 32) throw std::runtime_error("psacx: more than 2^32 distinct symbols");
        bytes.resize(n * w);
        for (std::size_t i = 0; i < n; ++i) {
            const uint64_t r = (uint64_t)(std::lower_bound(uniq.begin(), uniq.end(), u[i]) - uniq.begin());
            for (unsigned b = 0; b < w; ++b) bytes[i * w + b] = (uint8_t)(r >> (8 * (w - 1 - b)));
        }
        return w;
    }
    // Results over the byte text of w bytes per symbol -> results over the symbols.  The suffixes that start on a symbol boundary, in
    // the order they have in SA', are SA; the rank among them is ISA; the common prefix of two neighbours among them is the minimum of
    // LCP' over the entries between them, in whole symbols.
    void reduce_wide(unsigned w, const std::vector<index_t>& sa, const std::vector<index_t>& lcp) {
        std::size_t r = 0;
        uint64_t run = ~(uint64_t)0;                    // minimum of LCP' since the last kept entry
        for (std::size_t j = 0; j < sa.size(); ++j) {
            if (!lcp.empty() && j && (uint64_t)lcp[j] < run) run = (uint64_t)lcp[j];
            if ((uint64_t)sa[j] % w) continue;
            const std::size_t i = (std::size_t)((uint64_t)sa[j] / w);
            local_SA[r] = (index_t)i; local_B[i] = (index_t)r;
            if (!lcp.empty()) local_LCP[r] = r ? (index_t)(run / w) : (index_t)0;
            run = ~(uint64_t)0;
            ++r;
        }
    }
    template <typename V> static void dump(const std::string& fn, const std::vector<V>& v) {
        std::ofstream f(fn.c_str(), std::ios::binary | std::ios::trunc);
        f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(V)));
        if (!f) throw std::runtime_error("cannot write " + fn);
    }
    template <typename V> static void slurp(const std::string& fn, std::vector<V>& v) {
        std::ifstream f(fn.c_str(), std::ios::binary | std::ios::ate);
        if (!f) throw std::runtime_error("cannot read " + fn);
        std::size_t bytes = (std::size_t)f.tellg();
        v.resize(bytes / sizeof(V));
        f.seekg(0); f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(V)));
    }
};

// construct_suffix_tree(sa, begin, end, comm) of /root/reference/include/suffix_tree.hpp:413-438:
// the (sigma + 1) * n node table (row i = internal node of LCP index i, cell c = child through the
// character with alphabet code c, leaves are n + i, 0 = none).  The text must be bytes.
template <typename Iterator, typename index_t>
std::vector<std::size_t> construct_suffix_tree(suffix_array<char, index_t, true>& sa, Iterator str_begin, Iterator str_end,
                                               const psacx::comm&) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    std::vector<uint8_t> text(str_begin, str_end);
    if (text.size() != sa.n) throw std::runtime_error("construct_suffix_tree: text does not match the suffix array");
    uint32_t sigma = 0;
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    const W* p_sa = reinterpret_cast<const W*>(sa.local_SA.data());
    const W* p_lcp = reinterpret_cast<const W*>(sa.local_LCP.data());
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* a, const uint32_t* l, uint64_t* o, uint32_t* s) {
            return psacx_suffix_tree_u32(c, t, n, a, l, o, s);
        }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* a, const uint64_t* l, uint64_t* o, uint32_t* s) {
            return psacx_suffix_tree_u64(c, t, n, a, l, o, s);
        }
        // p > 1: the table is built by the ranks of the suffix array's communicator (suffix_tree.hpp:440-499)
        static int run(psacx_multi* g, const uint8_t* t, uint64_t n, const uint32_t* a, const uint32_t* l, uint64_t* o, uint32_t* s) {
            return psacx_multi_suffix_tree_u32(g, t, n, a, l, o, s);
        }
        static int run(psacx_multi* g, const uint8_t* t, uint64_t n, const uint64_t* a, const uint64_t* l, uint64_t* o, uint32_t* s) {
            return psacx_multi_suffix_tree_u64(g, t, n, a, l, o, s);
        }
    };
    if (psacx_multi* mg = sa.multi_context()) {
        auto must = [&](int rc) { if (rc != PSACX_OK) throw std::runtime_error(std::string("psacx: ") + psacx_strerror(rc) + " [" + psacx_multi_last_error(mg) + "]"); };
        must(Call::run(mg, text.data(), sa.n, (const W*)nullptr, (const W*)nullptr, nullptr, &sigma));
        std::vector<std::size_t> nodes((std::size_t)(sigma + 1) * sa.n, 0);
        must(Call::run(mg, text.data(), sa.n, p_sa, p_lcp, reinterpret_cast<uint64_t*>(nodes.data()), &sigma));
        return nodes;
    }
    psacx::check(sa.context(), Call::run(sa.context(), text.data(), sa.n, (const W*)nullptr, (const W*)nullptr, nullptr, &sigma));
    std::vector<std::size_t> nodes((std::size_t)(sigma + 1) * sa.n, 0);
    psacx::check(sa.context(), Call::run(sa.context(), text.data(), sa.n, p_sa, p_lcp, reinterpret_cast<uint64_t*>(nodes.data()), &sigma));
    return nodes;
}

// construct_gst(sa, ss, comm) of the reference (include/suffix_tree.hpp:521-608): the (sigma + 2) * n node table of the
// string set `sa.construct_ss(ss, ...)` was built from (row i = internal node of LCP index i, cells 0 and 1 = first and last
// $-leaf, cell c + 1 = child through the character with alphabet code c, leaves are n + i, 0 = none; psacx_suffix_tree_gsa_* in
// psacx.h defines it and names the two points where the reference's code, which nothing calls, would differ).  One rank only:
// there is no distributed form, and none is emulated by gathering.
template <typename index_t>
std::vector<std::size_t> construct_gst(suffix_array<char, index_t, true>& sa, simple_dstringset& ss, const psacx::comm& = psacx::comm(0)) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    if (sa.multi_context()) throw std::runtime_error("psacx: construct_gst needs a single-rank communicator (the tree of a string set is built on one GPU)");
    if (ss.sum_sizes != sa.n) throw std::runtime_error("construct_gst: string set does not match the suffix array");
    std::vector<uint8_t> text; text.reserve(sa.n);
    std::vector<uint64_t> off(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) {
        text.insert(text.end(), reinterpret_cast<const uint8_t*>(ss.str_begins[s]), reinterpret_cast<const uint8_t*>(ss.str_begins[s]) + ss.sizes[s]);
        off.push_back(text.size());
    }
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* f, uint64_t m, const uint32_t* a, const uint32_t* l, uint64_t* o, uint32_t* s) {
            return psacx_suffix_tree_gsa_u32(c, t, n, f, m, a, l, o, s);
        }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* f, uint64_t m, const uint64_t* a, const uint64_t* l, uint64_t* o, uint32_t* s) {
            return psacx_suffix_tree_gsa_u64(c, t, n, f, m, a, l, o, s);
        }
    };
    uint32_t sigma = 0;
    const uint64_t m = (uint64_t)ss.sizes.size();
    psacx::check(sa.context(), Call::run(sa.context(), text.data(), sa.n, off.data(), m, (const W*)nullptr, (const W*)nullptr, nullptr, &sigma));
    std::vector<std::size_t> nodes((std::size_t)(sigma + 2) * sa.n, 0);
    psacx::check(sa.context(), Call::run(sa.context(), text.data(), sa.n, off.data(), m, reinterpret_cast<const W*>(sa.local_SA.data()),
                                         reinterpret_cast<const W*>(sa.local_LCP.data()), reinterpret_cast<uint64_t*>(nodes.data()), &sigma));
    return nodes;
}

// sa_index::locate (seq_query.hpp:246-251 of the reference) for a batch of patterns: element i = [lb, ub) of patterns[i] in
// sa.local_SA -- it occurs at local_SA[lb .. ub); where it does not occur, lb == ub is its insertion point (psacx.h: "pattern
// search").  The text [begin, end) must be the bytes `sa` was constructed from.  k > 0 puts the k-mer lookup table of
// lookup_table.hpp:36-149 in front of the searches; the answers are the same.  One rank only: there is no distributed form, and
// none is emulated by gathering.
template <typename index_t, bool LCP, bool LC, typename Iterator>
std::vector<std::pair<index_t, index_t> > locate(suffix_array<char, index_t, LCP, LC>& sa, Iterator begin, Iterator end,
                                                 const std::vector<std::string>& patterns, unsigned int k = 0) {
    if (sa.multi_context()) throw std::runtime_error("psacx: locate needs a single-rank communicator (the search runs on one GPU)");
    std::vector<uint8_t> text(begin, end);
    if (text.size() != sa.n) throw std::runtime_error("locate: text does not match the suffix array");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* a, const uint8_t* p, const uint64_t* f, uint64_t q, uint32_t k,
                       uint32_t* l, uint32_t* u) { return psacx_locate_u32(c, t, n, a, p, f, q, k, l, u); }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* a, const uint8_t* p, const uint64_t* f, uint64_t q, uint32_t k,
                       uint64_t* l, uint64_t* u) { return psacx_locate_u64(c, t, n, a, p, f, q, k, l, u); }
    };
    std::vector<uint8_t> pat;
    std::vector<uint64_t> off(1, 0);
    for (std::size_t i = 0; i < patterns.size(); ++i) {
        pat.insert(pat.end(), patterns[i].begin(), patterns[i].end());
        off.push_back(pat.size());
    }
    const uint64_t q = (uint64_t)patterns.size();
    std::vector<W> lb(patterns.size()), ub(patterns.size());
    psacx::check(sa.context(), Call::run(sa.context(), text.data(), sa.n, reinterpret_cast<const W*>(sa.local_SA.data()), pat.data(), off.data(), q,
                                         (uint32_t)k, lb.data(), ub.data()));
    std::vector<std::pair<index_t, index_t> > out(patterns.size());
    for (std::size_t i = 0; i < patterns.size(); ++i) out[i] = std::make_pair((index_t)lb[i], (index_t)ub[i]);
    return out;
}

// The same over the generalized suffix array of a string set: `ss` is the set `sa.construct_ss(ss, ...)` was built from.  Suffix i
// ends where its string ends, so no pattern matches across two strings (psacx.h: "pattern search over string sets").
template <typename index_t, bool LCP>
std::vector<std::pair<index_t, index_t> > locate(suffix_array<char, index_t, LCP, false>& sa, simple_dstringset& ss,
                                                 const std::vector<std::string>& patterns, unsigned int k = 0) {
    if (sa.multi_context()) throw std::runtime_error("psacx: locate needs a single-rank communicator (the search runs on one GPU)");
    if (ss.sum_sizes != sa.n) throw std::runtime_error("locate: string set does not match the suffix array");
    std::vector<uint8_t> text; text.reserve(sa.n);
    std::vector<uint64_t> soff(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) {
        text.insert(text.end(), reinterpret_cast<const uint8_t*>(ss.str_begins[s]), reinterpret_cast<const uint8_t*>(ss.str_begins[s]) + ss.sizes[s]);
        soff.push_back(text.size());
    }
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* a, const uint8_t* p, const uint64_t* f,
                       uint64_t q, uint32_t k, uint32_t* l, uint32_t* u) { return psacx_locate_gsa_u32(c, t, n, o, m, a, p, f, q, k, l, u); }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* a, const uint8_t* p, const uint64_t* f,
                       uint64_t q, uint32_t k, uint64_t* l, uint64_t* u) { return psacx_locate_gsa_u64(c, t, n, o, m, a, p, f, q, k, l, u); }
    };
    std::vector<uint8_t> pat;
    std::vector<uint64_t> off(1, 0);
    for (std::size_t i = 0; i < patterns.size(); ++i) {
        pat.insert(pat.end(), patterns[i].begin(), patterns[i].end());
        off.push_back(pat.size());
    }
    const uint64_t q = (uint64_t)patterns.size();
    std::vector<W> lb(patterns.size()), ub(patterns.size());
    psacx::check(sa.context(), Call::run(sa.context(), text.data(), sa.n, soff.data(), (uint64_t)ss.sizes.size(),
                                         reinterpret_cast<const W*>(sa.local_SA.data()), pat.data(), off.data(), q, (uint32_t)k, lb.data(), ub.data()));
    std::vector<std::pair<index_t, index_t> > out(patterns.size());
    for (std::size_t i = 0; i < patterns.size(); ++i) out[i] = std::make_pair((index_t)lb[i], (index_t)ub[i]);
    return out;
}

// The occurrence lists of a batch of intervals [lb[j], ub[j]) of locate (psacx.h: "occurrence lists"): the occurrences of pattern j
// are pos[start[j] .. start[j + 1]) = local_SA[lb[j] .. ub[j]), in that order, at most `limit` of them where limit > 0; sid, filled
// by the form that takes the string set, names the string holding each.  The lists are made on the GPU (psacx_occurrences_dev_*).
template <typename index_t>
struct occurrence_lists {
    std::vector<std::size_t> start;
    std::vector<index_t> pos, sid;
};

namespace psacx {
template <typename index_t, bool LCP, bool LC>
occurrence_lists<index_t> occurrences_of(suffix_array<char, index_t, LCP, LC>& sa, const std::vector<uint64_t>* soff, const std::vector<index_t>& lb,
                                         const std::vector<index_t>& ub, std::size_t limit) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    if (sa.multi_context()) throw std::runtime_error("psacx: occurrences needs a single-rank communicator (the lists are made on one GPU)");
    if (lb.size() != ub.size()) throw std::runtime_error("occurrences: lb and ub differ in length");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint32_t* a, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* l, const uint32_t* u, uint64_t q, uint64_t lim,
                       uint64_t* st, uint32_t* p, uint32_t* s, uint64_t cap, uint64_t* tot) { return psacx_occurrences_dev_u32(c, a, n, o, m, l, u, q, lim, st, p, s, cap, tot); }
        static int run(psacx_ctx* c, const uint64_t* a, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* l, const uint64_t* u, uint64_t q, uint64_t lim,
                       uint64_t* st, uint64_t* p, uint64_t* s, uint64_t cap, uint64_t* tot) { return psacx_occurrences_dev_u64(c, a, n, o, m, l, u, q, lim, st, p, s, cap, tot); }
    };
    psacx_ctx* c = sa.context();
    const uint64_t q = (uint64_t)lb.size(), n = (uint64_t)sa.n, m = soff ? (uint64_t)soff->size() - 1 : 0;
    occurrence_lists<index_t> out;
    out.start.assign(q + 1, 0);
    std::vector<void*> held;
    struct Free {                                            // the device buffers go on every path
        psacx_ctx* c; std::vector<void*>& v;
        ~Free() { for (std::size_t i = 0; i < v.size(); ++i) (void)psacx_dev_free(c, v[i]); }
    } guard = {c, held};
    (void)guard;
    auto dev = [&](const void* src, uint64_t bytes) -> void* {
        void* p = nullptr;
        check(c, psacx_dev_alloc(c, &p, bytes ? bytes : 1));
        held.push_back(p);
        if (src && bytes) check(c, psacx_copy_h2d(c, p, src, bytes));
        return p;
    };
    const W* d_sa = (const W*)dev(sa.local_SA.data(), n * sizeof(W));
    const W* d_lb = (const W*)dev(lb.data(), q * sizeof(W));
    const W* d_ub = (const W*)dev(ub.data(), q * sizeof(W));
    const uint64_t* d_off = soff ? (const uint64_t*)dev(soff->data(), (m + 1) * sizeof(uint64_t)) : nullptr;
    uint64_t* d_start = (uint64_t*)dev(nullptr, (q + 1) * sizeof(uint64_t));
    uint64_t total = 0;
    check(c, Call::run(c, d_sa, n, d_off, m, d_lb, d_ub, q, (uint64_t)limit, d_start, (W*)nullptr, (W*)nullptr, 0, &total));
    out.pos.assign(total, 0);
    if (soff) out.sid.assign(total, 0);
    W* d_pos = (W*)dev(nullptr, total * sizeof(W));
    W* d_sid = soff ? (W*)dev(nullptr, total * sizeof(W)) : nullptr;
    check(c, Call::run(c, d_sa, n, d_off, m, d_lb, d_ub, q, (uint64_t)limit, d_start, d_pos, d_sid, total, &total));
    check(c, psacx_copy_d2h(c, out.start.data(), d_start, (q + 1) * sizeof(uint64_t)));
    if (total) check(c, psacx_copy_d2h(c, out.pos.data(), d_pos, total * sizeof(W)));
    if (total && soff) check(c, psacx_copy_d2h(c, out.sid.data(), d_sid, total * sizeof(W)));
    return out;
}
} // namespace psacx

template <typename index_t, bool LCP, bool LC>
occurrence_lists<index_t> occurrences(suffix_array<char, index_t, LCP, LC>& sa, const std::vector<index_t>& lb, const std::vector<index_t>& ub,
                                      std::size_t limit = 0) {
    return psacx::occurrences_of(sa, (const std::vector<uint64_t>*)nullptr, lb, ub, limit);
}

template <typename index_t, bool LCP>
occurrence_lists<index_t> occurrences(suffix_array<char, index_t, LCP, false>& sa, simple_dstringset& ss, const std::vector<index_t>& lb,
                                      const std::vector<index_t>& ub, std::size_t limit = 0) {
    if (ss.sum_sizes != sa.n) throw std::runtime_error("occurrences: string set does not match the suffix array");
    std::vector<uint64_t> soff(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) soff.push_back(soff.back() + ss.sizes[s]);
    return psacx::occurrences_of(sa, &soff, lb, ub, limit);
}

// Longest match (psacx.h: "longest match and matching statistics"): for every query the length of its longest prefix that occurs
// and the locate interval of that prefix -- it occurs at local_SA[lb[i] .. ub[i]); len[i] == 0 gives [0, n).  One query per
// pattern, or with suffixes = true one per byte of the patterns laid back to back (the query at byte p is the rest of its pattern
// from p on: the matching statistics of every pattern), in that order.  max_len > 0 cuts every query to that many bytes.  k > 0
// puts the k-mer lookup table in front; the answers are the same.  One rank only, as locate.
template <typename index_t>
struct match_lists {
    std::vector<index_t> len, lb, ub;
};

namespace psacx {
// soff: the offsets of a string set, or nullptr for one text
template <typename index_t, bool LCP, bool LC>
match_lists<index_t> match_of(suffix_array<char, index_t, LCP, LC>& sa, const std::vector<uint8_t>& text, const std::vector<uint64_t>* soff,
                              const std::vector<std::string>& patterns, unsigned int k, bool suffixes, std::size_t max_len) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* a, const uint8_t* p, const uint64_t* f,
                       uint64_t q, uint32_t k, uint32_t fl, uint64_t ml, uint32_t* d, uint32_t* l, uint32_t* u) {
            return o ? psacx_match_gsa_u32(c, t, n, o, m, a, p, f, q, k, fl, ml, d, l, u) : psacx_match_u32(c, t, n, a, p, f, q, k, fl, ml, d, l, u);
        }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* a, const uint8_t* p, const uint64_t* f,
                       uint64_t q, uint32_t k, uint32_t fl, uint64_t ml, uint64_t* d, uint64_t* l, uint64_t* u) {
            return o ? psacx_match_gsa_u64(c, t, n, o, m, a, p, f, q, k, fl, ml, d, l, u) : psacx_match_u64(c, t, n, a, p, f, q, k, fl, ml, d, l, u);
        }
    };
    std::vector<uint8_t> pat;
    std::vector<uint64_t> off(1, 0);
    for (std::size_t i = 0; i < patterns.size(); ++i) {
        pat.insert(pat.end(), patterns[i].begin(), patterns[i].end());
        off.push_back(pat.size());
    }
    const uint64_t q = (uint64_t)patterns.size();
    const std::size_t entries = suffixes ? pat.size() : patterns.size();
    std::vector<W> len(entries), lb(entries), ub(entries);
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, soff ? soff->data() : (const uint64_t*)nullptr, soff ? (uint64_t)soff->size() - 1 : 0,
                                  reinterpret_cast<const W*>(sa.local_SA.data()), pat.data(), off.data(), q, (uint32_t)k,
                                  suffixes ? PSACX_MATCH_SUFFIXES : 0u, (uint64_t)max_len, len.data(), lb.data(), ub.data()));
    match_lists<index_t> out;
    out.len.assign(len.begin(), len.end());
    out.lb.assign(lb.begin(), lb.end());
    out.ub.assign(ub.begin(), ub.end());
    return out;
}
} // namespace psacx

template <typename index_t, bool LCP, bool LC, typename Iterator>
match_lists<index_t> match(suffix_array<char, index_t, LCP, LC>& sa, Iterator begin, Iterator end, const std::vector<std::string>& patterns,
                           unsigned int k = 0, bool suffixes = false, std::size_t max_len = 0) {
    if (sa.multi_context()) throw std::runtime_error("psacx: match needs a single-rank communicator (the search runs on one GPU)");
    std::vector<uint8_t> text(begin, end);
    if (text.size() != sa.n) throw std::runtime_error("match: text does not match the suffix array");
    return psacx::match_of(sa, text, (const std::vector<uint64_t>*)nullptr, patterns, k, suffixes, max_len);
}

// The same over the generalized suffix array of a string set: a match never crosses a string end.
template <typename index_t, bool LCP>
match_lists<index_t> match(suffix_array<char, index_t, LCP, false>& sa, simple_dstringset& ss, const std::vector<std::string>& patterns,
                           unsigned int k = 0, bool suffixes = false, std::size_t max_len = 0) {
    if (sa.multi_context()) throw std::runtime_error("psacx: match needs a single-rank communicator (the search runs on one GPU)");
    if (ss.sum_sizes != sa.n) throw std::runtime_error("match: string set does not match the suffix array");
    std::vector<uint8_t> text; text.reserve(sa.n);
    std::vector<uint64_t> soff(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) {
        text.insert(text.end(), reinterpret_cast<const uint8_t*>(ss.str_begins[s]), reinterpret_cast<const uint8_t*>(ss.str_begins[s]) + ss.sizes[s]);
        soff.push_back(text.size());
    }
    return psacx::match_of(sa, text, &soff, patterns, k, suffixes, max_len);
}

// Longest common extension (psacx.h: "range minimum and longest common extension"): len[i] = how far the text positions a[i]
// and b[i] agree when up to max_mismatch differing characters are stepped over, from local_B (the inverse suffix array) and
// local_LCP alone -- the text is not needed.  A position at or beyond n is the empty suffix.  The suffix array must have been
// constructed with its LCP.  One rank only, as match.
namespace psacx {
template <typename index_t, bool LC>
std::vector<index_t> lce_of(suffix_array<char, index_t, true, LC>& sa, const std::vector<uint64_t>* soff, const std::vector<index_t>& a,
                            const std::vector<index_t>& b, std::size_t max_mismatch) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* isa, const uint32_t* lcp, const uint32_t* x, const uint32_t* y,
                       uint64_t q, uint64_t e, uint32_t* len) { return psacx_lce_u32(c, n, o, m, isa, lcp, x, y, q, e, len); }
        static int run(psacx_ctx* c, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* isa, const uint64_t* lcp, const uint64_t* x, const uint64_t* y,
                       uint64_t q, uint64_t e, uint64_t* len) { return psacx_lce_u64(c, n, o, m, isa, lcp, x, y, q, e, len); }
    };
    if (a.size() != b.size()) throw std::runtime_error("lce: a and b differ in length");
    if (sa.local_B.size() != sa.n || sa.local_LCP.size() != sa.n) throw std::runtime_error("lce: the suffix array holds no ISA and LCP of its text");
    std::vector<W> x(a.begin(), a.end()), y(b.begin(), b.end()), len(a.size());
    check(sa.context(), Call::run(sa.context(), sa.n, soff ? soff->data() : (const uint64_t*)nullptr, soff ? (uint64_t)soff->size() - 1 : 0,
                                  reinterpret_cast<const W*>(sa.local_B.data()), reinterpret_cast<const W*>(sa.local_LCP.data()), x.data(), y.data(),
                                  (uint64_t)x.size(), (uint64_t)max_mismatch, len.data()));
    return std::vector<index_t>(len.begin(), len.end());
}
} // namespace psacx

template <typename index_t, bool LC>
std::vector<index_t> lce(suffix_array<char, index_t, true, LC>& sa, const std::vector<index_t>& a, const std::vector<index_t>& b,
                         std::size_t max_mismatch = 0) {
    if (sa.multi_context()) throw std::runtime_error("psacx: lce needs a single-rank communicator (the queries run on one GPU)");
    return psacx::lce_of(sa, (const std::vector<uint64_t>*)nullptr, a, b, max_mismatch);
}

// The same over the arrays of a string set: an extension ends where either string does.
template <typename index_t>
std::vector<index_t> lce(suffix_array<char, index_t, true, false>& sa, simple_dstringset& ss, const std::vector<index_t>& a,
                         const std::vector<index_t>& b, std::size_t max_mismatch = 0) {
    if (sa.multi_context()) throw std::runtime_error("psacx: lce needs a single-rank communicator (the queries run on one GPU)");
    if (ss.sum_sizes != sa.n) throw std::runtime_error("lce: string set does not match the suffix array");
    std::vector<uint64_t> soff(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) soff.push_back(soff.back() + ss.sizes[s]);
    return psacx::lce_of(sa, &soff, a, b, max_mismatch);
}

// Range minima over local_LCP: min[i] is the minimum of local_LCP[lo[i] .. min(hi[i], n)) and arg[i] the smallest position that
// holds it (the first minimum, as the reference's rmq<>::query returns it); an empty range gives all ones and n.
template <typename index_t>
struct range_minima {
    std::vector<index_t> min, arg;
};

template <typename index_t, bool LC>
range_minima<index_t> range_min(suffix_array<char, index_t, true, LC>& sa, const std::vector<index_t>& lo, const std::vector<index_t>& hi) {
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint32_t* v, uint64_t n, const uint32_t* l, const uint32_t* h, uint64_t q, uint32_t* m, uint32_t* a) {
            return psacx_rmq_u32(c, v, n, l, h, q, m, a);
        }
        static int run(psacx_ctx* c, const uint64_t* v, uint64_t n, const uint64_t* l, const uint64_t* h, uint64_t q, uint64_t* m, uint64_t* a) {
            return psacx_rmq_u64(c, v, n, l, h, q, m, a);
        }
    };
    if (sa.multi_context()) throw std::runtime_error("psacx: range_min needs a single-rank communicator (the queries run on one GPU)");
    if (lo.size() != hi.size()) throw std::runtime_error("range_min: lo and hi differ in length");
    if (sa.local_LCP.size() != sa.n) throw std::runtime_error("range_min: the suffix array holds no LCP of its text");
    std::vector<W> l(lo.begin(), lo.end()), h(hi.begin(), hi.end()), mn(lo.size()), at(lo.size());
    psacx::check(sa.context(), Call::run(sa.context(), reinterpret_cast<const W*>(sa.local_LCP.data()), sa.n, l.data(), h.data(), (uint64_t)l.size(),
                                         mn.data(), at.data()));
    range_minima<index_t> out;
    out.min.assign(mn.begin(), mn.end());
    out.arg.assign(at.begin(), at.end());
    return out;
}

// Suffix-prefix overlaps of a string set (psacx.h: "suffix-prefix overlaps"): for string j, which starts at offset o_j, and a
// length d in [min_len, L_j - 1] (whole: up to L_j) the suffixes that are exactly the first d bytes of string j are
// local_SA[lb[p] .. ub[p]) with p = o_j + d - 1; every other slot holds 0, 0.  Borders of string j and whole strings that are its
// prefixes are among them.  n entries each; occurrences(sa, ss, lb, ub) lists positions and source strings.  The suffix array
// must have been constructed from ss with its LCP.  One rank only, as lce.
template <typename index_t>
struct overlap_intervals {
    std::vector<index_t> lb, ub;
};

template <typename index_t>
overlap_intervals<index_t> overlaps(suffix_array<char, index_t, true, false>& sa, simple_dstringset& ss, std::size_t min_len, bool whole = false) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* s, const uint32_t* isa, const uint32_t* lcp, uint64_t l,
                       uint32_t f, uint32_t* lb, uint32_t* ub) { return psacx_overlaps_u32(c, n, o, m, s, isa, lcp, l, f, lb, ub); }
        static int run(psacx_ctx* c, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* s, const uint64_t* isa, const uint64_t* lcp, uint64_t l,
                       uint32_t f, uint64_t* lb, uint64_t* ub) { return psacx_overlaps_u64(c, n, o, m, s, isa, lcp, l, f, lb, ub); }
    };
    if (sa.multi_context()) throw std::runtime_error("psacx: overlaps needs a single-rank communicator (the queries run on one GPU)");
    if (ss.sum_sizes != sa.n) throw std::runtime_error("overlaps: string set does not match the suffix array");
    if (sa.local_SA.size() != sa.n || sa.local_B.size() != sa.n || sa.local_LCP.size() != sa.n)
        throw std::runtime_error("overlaps: the suffix array holds no SA, ISA and LCP of its strings");
    std::vector<uint64_t> soff(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) soff.push_back(soff.back() + ss.sizes[s]);
    std::vector<W> lb(sa.n), ub(sa.n);
    psacx::check(sa.context(), Call::run(sa.context(), sa.n, soff.data(), (uint64_t)soff.size() - 1, reinterpret_cast<const W*>(sa.local_SA.data()),
                                         reinterpret_cast<const W*>(sa.local_B.data()), reinterpret_cast<const W*>(sa.local_LCP.data()),
                                         (uint64_t)min_len, whole ? PSACX_OVERLAP_WHOLE : 0u, lb.data(), ub.data()));
    overlap_intervals<index_t> out;
    out.lb.assign(lb.begin(), lb.end());
    out.ub.assign(ub.begin(), ub.end());
    return out;
}

// The greedy LZ77 parse of the text (psacx.h: "LZ77 factorization"): phrase k is the text from start[k] to start[k + 1], a copy of
// as many bytes from src[k] -- which may run into the phrase itself -- or one literal byte where src[k] is all ones of index_t.
// start has z + 1 entries and ends with n, src has z.  The suffix array must have been constructed from one text with its LCP.
// One rank only, as overlaps.
template <typename index_t>
struct lz_factors {
    std::vector<index_t> start, src;
};

template <typename index_t>
lz_factors<index_t> lz77(suffix_array<char, index_t, true, false>& sa) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, uint64_t n, const uint32_t* s, const uint32_t* lcp, uint32_t* start, uint32_t* src, uint64_t cap, uint64_t* z) {
            return psacx_lz77_u32(c, n, s, lcp, start, src, cap, z);
        }
        static int run(psacx_ctx* c, uint64_t n, const uint64_t* s, const uint64_t* lcp, uint64_t* start, uint64_t* src, uint64_t cap, uint64_t* z) {
            return psacx_lz77_u64(c, n, s, lcp, start, src, cap, z);
        }
    };
    if (sa.multi_context()) throw std::runtime_error("psacx: lz77 needs a single-rank communicator (the parse runs on one GPU)");
    if (sa.n == 0 || sa.local_SA.size() != sa.n || sa.local_LCP.size() != sa.n)
        throw std::runtime_error("lz77: the suffix array holds no SA and LCP of a text");
    const W* s = reinterpret_cast<const W*>(sa.local_SA.data());
    const W* l = reinterpret_cast<const W*>(sa.local_LCP.data());
    uint64_t z = 0;
    psacx::check(sa.context(), Call::run(sa.context(), sa.n, s, l, (W*)0, (W*)0, 0, &z));
    std::vector<W> start(z + 1), src(z + 1);
    psacx::check(sa.context(), Call::run(sa.context(), sa.n, s, l, start.data(), src.data(), z + 1, &z));
    lz_factors<index_t> out;
    out.start.assign(start.begin(), start.end());
    out.src.assign(src.begin(), src.begin() + z);
    return out;
}

// The Burrows-Wheeler transform aligned with local_SA (psacx.h: "BWT and repeats"): bwt[r] is the byte in front of suffix local_SA[r],
// and where that suffix starts a string (the text) the last byte of that string -- not libdivsufsort's divbwt layout.  primary is
// the rank of position 0.  The text [begin, end) must be the bytes `sa` was constructed from (the object does not keep them), `ss`
// the set of construct_ss.  One rank only, as lz77.
struct bwt_result {
    std::string bwt;
    std::size_t primary;
};

// The repeats of one kind as LCP-intervals: repeat k is the len[k] bytes at local_SA[lb[k]] and occurs exactly at
// local_SA[lb[k] .. ub[k]), in ascending order of the interval heads.  occurrences(sa, lb, ub) / occurrences(sa, ss, lb, ub) list
// positions and strings.  The suffix array must have been constructed with its LCP.
template <typename index_t>
struct repeat_intervals {
    std::vector<index_t> lb, ub, len;
};

enum repeat_kind { repeats_right = 0, repeats_maximal = 1, repeats_supermaximal = 2 };

namespace psacx {

inline void flatten_set(simple_dstringset& ss, std::vector<uint8_t>& text, std::vector<uint64_t>& soff) {
    text.clear(); soff.assign(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) {
        text.insert(text.end(), reinterpret_cast<const uint8_t*>(ss.str_begins[s]), reinterpret_cast<const uint8_t*>(ss.str_begins[s]) + ss.sizes[s]);
        soff.push_back(text.size());
    }
}

template <typename index_t, bool LCP, bool LC>
bwt_result bwt_of(suffix_array<char, index_t, LCP, LC>& sa, const std::vector<uint8_t>& text, const std::vector<uint64_t>* soff) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* s, uint8_t* b, uint64_t* p) {
            return psacx_bwt_u32(c, t, n, o, m, s, b, p);
        }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* s, uint8_t* b, uint64_t* p) {
            return psacx_bwt_u64(c, t, n, o, m, s, b, p);
        }
    };
    if (sa.multi_context()) throw std::runtime_error("psacx: bwt needs a single-rank communicator (the transform runs on one GPU)");
    if (sa.n == 0 || text.size() != sa.n || sa.local_SA.size() != sa.n) throw std::runtime_error("bwt: text does not match the suffix array");
    std::vector<uint8_t> out(sa.n);
    uint64_t primary = 0;
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, soff ? soff->data() : (const uint64_t*)0, soff ? (uint64_t)soff->size() - 1 : 0,
                                  reinterpret_cast<const W*>(sa.local_SA.data()), out.data(), &primary));
    bwt_result r;
    r.bwt.assign(out.begin(), out.end());
    r.primary = (std::size_t)primary;
    return r;
}

template <typename index_t>
repeat_intervals<index_t> repeats_of(suffix_array<char, index_t, true, false>& sa, const std::vector<uint8_t>& text, const std::vector<uint64_t>* soff,
                                     repeat_kind kind, std::size_t min_len, std::size_t min_occ, std::size_t max_occ) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* s, const uint32_t* l, uint32_t k,
                       uint64_t a, uint64_t b, uint64_t d, uint32_t* lb, uint32_t* ub, uint32_t* len, uint64_t cap, uint64_t* z) {
            return psacx_repeats_u32(c, t, n, o, m, s, l, k, a, b, d, lb, ub, len, cap, z);
        }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* s, const uint64_t* l, uint32_t k,
                       uint64_t a, uint64_t b, uint64_t d, uint64_t* lb, uint64_t* ub, uint64_t* len, uint64_t cap, uint64_t* z) {
            return psacx_repeats_u64(c, t, n, o, m, s, l, k, a, b, d, lb, ub, len, cap, z);
        }
    };
    if (sa.multi_context()) throw std::runtime_error("psacx: repeats needs a single-rank communicator (the enumeration runs on one GPU)");
    if (sa.n == 0 || text.size() != sa.n || sa.local_SA.size() != sa.n || sa.local_LCP.size() != sa.n)
        throw std::runtime_error("repeats: the suffix array holds no SA and LCP of this text");
    const W* s = reinterpret_cast<const W*>(sa.local_SA.data());
    const W* l = reinterpret_cast<const W*>(sa.local_LCP.data());
    const uint64_t* o = soff ? soff->data() : (const uint64_t*)0;
    const uint64_t m = soff ? (uint64_t)soff->size() - 1 : 0;
    uint64_t z = 0;
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, o, m, s, l, (uint32_t)kind, min_len, min_occ, max_occ, (W*)0, (W*)0, (W*)0, 0, &z));
    std::vector<W> lb(z + 1), ub(z + 1), len(z + 1);
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, o, m, s, l, (uint32_t)kind, min_len, min_occ, max_occ, lb.data(), ub.data(),
                                  len.data(), z, &z));
    repeat_intervals<index_t> out;
    out.lb.assign(lb.begin(), lb.begin() + z);
    out.ub.assign(ub.begin(), ub.begin() + z);
    out.len.assign(len.begin(), len.begin() + z);
    return out;
}

} // namespace psacx

template <typename index_t, bool LCP, bool LC, typename Iterator>
bwt_result bwt(suffix_array<char, index_t, LCP, LC>& sa, Iterator begin, Iterator end) {
    return psacx::bwt_of(sa, std::vector<uint8_t>(begin, end), (const std::vector<uint64_t>*)0);
}

template <typename index_t, bool LCP>
bwt_result bwt(suffix_array<char, index_t, LCP, false>& sa, simple_dstringset& ss) {
    std::vector<uint8_t> text; std::vector<uint64_t> soff;
    psacx::flatten_set(ss, text, soff);
    return psacx::bwt_of(sa, text, &soff);
}

template <typename index_t, typename Iterator>
repeat_intervals<index_t> repeats(suffix_array<char, index_t, true, false>& sa, Iterator begin, Iterator end, repeat_kind kind = repeats_maximal,
                                  std::size_t min_len = 1, std::size_t min_occ = 2, std::size_t max_occ = 0) {
    return psacx::repeats_of(sa, std::vector<uint8_t>(begin, end), (const std::vector<uint64_t>*)0, kind, min_len, min_occ, max_occ);
}

template <typename index_t>
repeat_intervals<index_t> repeats(suffix_array<char, index_t, true, false>& sa, simple_dstringset& ss, repeat_kind kind = repeats_maximal,
                                  std::size_t min_len = 1, std::size_t min_occ = 2, std::size_t max_occ = 0) {
    std::vector<uint8_t> text; std::vector<uint64_t> soff;
    psacx::flatten_set(ss, text, soff);
    return psacx::repeats_of(sa, text, &soff, kind, min_len, min_occ, max_occ);
}

// Document counts and document lists (psacx.h: "document counts and document lists") over the set of construct_ss.
// doc_count: the number of distinct strings among the suffixes local_SA[lb[j] .. ub[j]), for LCP-intervals: what locate / match /
// repeats / mems return, singletons and [0, n); the intervals of overlaps() are none, doc_list serves them.  Needs the LCP.
// doc_list: each of those strings once, for ANY interval: sid[start[j] .. start[j + 1]) in the order of their first rank, pos where
// that suffix starts.  max_cand > 0 refuses a batch whose intervals hold more ranks.
// common_repeats: repeats(), then doc_count(), then a filter on the host (the repeats are not filtered on the device): the repeats
// that occur in at least min_docs strings, and in at most max_docs where max_docs > 0, with their counts.  The longest substring
// common to at least min_docs strings is the row of the largest len.  One rank only, as repeats.
template <typename index_t>
struct doc_lists {
    std::vector<std::size_t> start;
    std::vector<index_t> sid, pos;
};

template <typename index_t>
struct common_repeat_intervals {
    std::vector<index_t> lb, ub, len, docs;
};

namespace psacx {

template <typename index_t, bool LCP>
std::vector<uint64_t> doc_offsets(suffix_array<char, index_t, LCP, false>& sa, simple_dstringset& ss, const char* what, std::size_t lbs, std::size_t ubs) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    if (sa.multi_context()) throw std::runtime_error(std::string("psacx: ") + what + " needs a single-rank communicator (the index is built on one GPU)");
    if (sa.n == 0 || ss.sum_sizes != sa.n || sa.local_SA.size() != sa.n) throw std::runtime_error(std::string(what) + ": string set does not match the suffix array");
    if (lbs != ubs) throw std::runtime_error(std::string(what) + ": lb and ub differ in length");
    std::vector<uint64_t> soff(1, 0);
    for (std::size_t s = 0; s < ss.sizes.size(); ++s) soff.push_back(soff.back() + ss.sizes[s]);
    return soff;
}

} // namespace psacx

template <typename index_t>
std::vector<index_t> doc_count(suffix_array<char, index_t, true, false>& sa, simple_dstringset& ss, const std::vector<index_t>& lb,
                               const std::vector<index_t>& ub) {
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* s, const uint32_t* l, const uint32_t* a, const uint32_t* b,
                       uint64_t q, uint32_t* d) { return psacx_doc_count_u32(c, n, o, m, s, l, a, b, q, d); }
        static int run(psacx_ctx* c, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* s, const uint64_t* l, const uint64_t* a, const uint64_t* b,
                       uint64_t q, uint64_t* d) { return psacx_doc_count_u64(c, n, o, m, s, l, a, b, q, d); }
    };
    const std::vector<uint64_t> soff = psacx::doc_offsets(sa, ss, "doc_count", lb.size(), ub.size());
    if (sa.local_LCP.size() != sa.n) throw std::runtime_error("doc_count: the suffix array holds no LCP");
    std::vector<index_t> docs(lb.size(), 0);
    psacx::check(sa.context(), Call::run(sa.context(), sa.n, soff.data(), (uint64_t)soff.size() - 1, reinterpret_cast<const W*>(sa.local_SA.data()),
                                         reinterpret_cast<const W*>(sa.local_LCP.data()), reinterpret_cast<const W*>(lb.data()),
                                         reinterpret_cast<const W*>(ub.data()), (uint64_t)lb.size(), reinterpret_cast<W*>(docs.data())));
    return docs;
}

template <typename index_t, bool LCP>
doc_lists<index_t> doc_list(suffix_array<char, index_t, LCP, false>& sa, simple_dstringset& ss, const std::vector<index_t>& lb,
                            const std::vector<index_t>& ub, std::size_t max_cand = 0) {
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint32_t* s, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* a, const uint32_t* b, uint64_t q, uint64_t mc,
                       uint64_t* st, uint32_t* sid, uint32_t* pos, uint64_t cap, uint64_t* tot) { return psacx_doc_list_u32(c, s, n, o, m, a, b, q, mc, st, sid, pos, cap, tot); }
        static int run(psacx_ctx* c, const uint64_t* s, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* a, const uint64_t* b, uint64_t q, uint64_t mc,
                       uint64_t* st, uint64_t* sid, uint64_t* pos, uint64_t cap, uint64_t* tot) { return psacx_doc_list_u64(c, s, n, o, m, a, b, q, mc, st, sid, pos, cap, tot); }
    };
    const std::vector<uint64_t> soff = psacx::doc_offsets(sa, ss, "doc_list", lb.size(), ub.size());
    const W* s = reinterpret_cast<const W*>(sa.local_SA.data());
    const W* a = reinterpret_cast<const W*>(lb.data());
    const W* b = reinterpret_cast<const W*>(ub.data());
    const uint64_t q = (uint64_t)lb.size(), m = (uint64_t)soff.size() - 1;
    std::vector<uint64_t> start(q + 1, 0);
    uint64_t total = 0;
    psacx::check(sa.context(), Call::run(sa.context(), s, sa.n, soff.data(), m, a, b, q, (uint64_t)max_cand, start.data(), (W*)0, (W*)0, 0, &total));
    std::vector<W> sid(total + 1), pos(total + 1);
    psacx::check(sa.context(), Call::run(sa.context(), s, sa.n, soff.data(), m, a, b, q, (uint64_t)max_cand, start.data(), sid.data(), pos.data(), total, &total));
    doc_lists<index_t> out;
    out.start.assign(start.begin(), start.end());
    out.sid.assign(sid.begin(), sid.begin() + total);
    out.pos.assign(pos.begin(), pos.begin() + total);
    return out;
}

template <typename index_t>
common_repeat_intervals<index_t> common_repeats(suffix_array<char, index_t, true, false>& sa, simple_dstringset& ss, std::size_t min_docs,
                                                std::size_t max_docs = 0, repeat_kind kind = repeats_right, std::size_t min_len = 1) {
    const repeat_intervals<index_t> r = repeats(sa, ss, kind, min_len);
    const std::vector<index_t> docs = doc_count(sa, ss, r.lb, r.ub);
    common_repeat_intervals<index_t> out;
    for (std::size_t k = 0; k < docs.size(); ++k) {
        if ((std::size_t)docs[k] < min_docs || (max_docs && (std::size_t)docs[k] > max_docs)) continue;
        out.lb.push_back(r.lb[k]); out.ub.push_back(r.ub[k]); out.len.push_back(r.len[k]); out.docs.push_back(docs[k]);
    }
    return out;
}

// The maximal exact matches of a batch of patterns against the text (psacx.h: "maximal exact matches"): match i is
// pattern bytes [qpos[i], qpos[i] + len[i]) -- qpos counts the bytes of the patterns laid back to back -- equal to the text at
// tpos[i], at least min_len long and extensible on neither side inside its pattern and its string.  max_occ > 0 keeps matches whose
// bytes occur at most that often, super those contained in no other match of their pattern.  Order: ascending qpos, then
// descending len, then rank in local_SA.  The suffix array must have been constructed with its LCP.  One rank only, as match.
template <typename index_t>
struct mem_lists {
    std::vector<uint64_t> qpos;
    std::vector<index_t> tpos, len;
};

namespace psacx {

template <typename index_t>
mem_lists<index_t> mems_of(suffix_array<char, index_t, true, false>& sa, const std::vector<uint8_t>& text, const std::vector<uint64_t>* soff,
                           const std::vector<std::string>& patterns, std::size_t min_len, unsigned int k, std::size_t max_occ, bool super) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* s, const uint32_t* l, const uint8_t* p,
                       const uint64_t* po, uint64_t q, uint32_t k, uint64_t a, uint64_t b, uint32_t f, uint64_t* qp, uint32_t* tp, uint32_t* len,
                       uint64_t cap, uint64_t* z) {
            return psacx_mems_u32(c, t, n, o, m, s, l, p, po, q, k, a, b, f, qp, tp, len, cap, z);
        }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* s, const uint64_t* l, const uint8_t* p,
                       const uint64_t* po, uint64_t q, uint32_t k, uint64_t a, uint64_t b, uint32_t f, uint64_t* qp, uint64_t* tp, uint64_t* len,
                       uint64_t cap, uint64_t* z) {
            return psacx_mems_u64(c, t, n, o, m, s, l, p, po, q, k, a, b, f, qp, tp, len, cap, z);
        }
    };
    if (sa.multi_context()) throw std::runtime_error("psacx: mems needs a single-rank communicator (the search runs on one GPU)");
    if (sa.n == 0 || text.size() != sa.n || sa.local_SA.size() != sa.n || sa.local_LCP.size() != sa.n)
        throw std::runtime_error("mems: the suffix array holds no SA and LCP of this text");
    std::vector<uint8_t> pat;
    std::vector<uint64_t> poff(1, 0);
    for (std::size_t i = 0; i < patterns.size(); ++i) {
        pat.insert(pat.end(), patterns[i].begin(), patterns[i].end());
        poff.push_back((uint64_t)pat.size());
    }
    const W* s = reinterpret_cast<const W*>(sa.local_SA.data());
    const W* l = reinterpret_cast<const W*>(sa.local_LCP.data());
    const uint64_t* o = soff ? soff->data() : (const uint64_t*)0;
    const uint64_t m = soff ? (uint64_t)soff->size() - 1 : 0, q = (uint64_t)patterns.size();
    const uint32_t flags = super ? PSACX_MEMS_SUPER : 0u;
    uint64_t z = 0;
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, o, m, s, l, pat.data(), poff.data(), q, k, min_len, max_occ, flags, (uint64_t*)0,
                                  (W*)0, (W*)0, 0, &z));
    std::vector<uint64_t> qpos(z + 1);
    std::vector<W> tpos(z + 1), len(z + 1);
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, o, m, s, l, pat.data(), poff.data(), q, k, min_len, max_occ, flags, qpos.data(),
                                  tpos.data(), len.data(), z, &z));
    mem_lists<index_t> out;
    out.qpos.assign(qpos.begin(), qpos.begin() + z);
    out.tpos.assign(tpos.begin(), tpos.begin() + z);
    out.len.assign(len.begin(), len.begin() + z);
    return out;
}

} // namespace psacx

template <typename index_t, typename Iterator>
mem_lists<index_t> mems(suffix_array<char, index_t, true, false>& sa, Iterator begin, Iterator end, const std::vector<std::string>& patterns,
                        std::size_t min_len, unsigned int k = 0, std::size_t max_occ = 0, bool super = false) {
    return psacx::mems_of(sa, std::vector<uint8_t>(begin, end), (const std::vector<uint64_t>*)0, patterns, min_len, k, max_occ, super);
}

template <typename index_t>
mem_lists<index_t> mems(suffix_array<char, index_t, true, false>& sa, simple_dstringset& ss, const std::vector<std::string>& patterns,
                        std::size_t min_len, unsigned int k = 0, std::size_t max_occ = 0, bool super = false) {
    std::vector<uint8_t> text; std::vector<uint64_t> soff;
    psacx::flatten_set(ss, text, soff);
    return psacx::mems_of(sa, text, &soff, patterns, min_len, k, max_occ, super);
}

// Where the patterns occur in the text with at most e substituted bytes (psacx.h: "pattern search with mismatches"): hit i is pattern
// qid[i] at text position tpos[i] (a position of the strings laid back to back, for a set), inside one string, with dist[i] <= e
// differing bytes.  Patterns shorter than e + 1 bytes have no hits.  Order: ascending pattern, then the first piece of the pattern
// that occurs exactly there, then rank in local_SA.  k > 0 puts the k-mer lookup table in front of the piece searches.  One rank
// only, as locate.
template <typename index_t>
struct mismatch_lists {
    std::vector<uint64_t> qid;
    std::vector<index_t> tpos;
    std::vector<uint8_t> dist;
};

namespace psacx {

template <typename index_t>
mismatch_lists<index_t> kmismatch_of(suffix_array<char, index_t, true, false>& sa, const std::vector<uint8_t>& text, const std::vector<uint64_t>* soff,
                                     const std::vector<std::string>& patterns, unsigned int e, unsigned int k) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* s, const uint8_t* p, const uint64_t* po,
                       uint64_t q, uint32_t k, uint32_t e, uint64_t* qi, uint32_t* tp, uint8_t* d, uint64_t cap, uint64_t* z) {
            return psacx_kmismatch_u32(c, t, n, o, m, s, p, po, q, k, e, 0, qi, tp, d, cap, z);
        }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* s, const uint8_t* p, const uint64_t* po,
                       uint64_t q, uint32_t k, uint32_t e, uint64_t* qi, uint64_t* tp, uint8_t* d, uint64_t cap, uint64_t* z) {
            return psacx_kmismatch_u64(c, t, n, o, m, s, p, po, q, k, e, 0, qi, tp, d, cap, z);
        }
    };
    if (sa.multi_context()) throw std::runtime_error("psacx: kmismatch needs a single-rank communicator (the search runs on one GPU)");
    if (sa.n == 0 || text.size() != sa.n || sa.local_SA.size() != sa.n)
        throw std::runtime_error("kmismatch: the suffix array holds no SA of this text");
    std::vector<uint8_t> pat;
    std::vector<uint64_t> poff(1, 0);
    for (std::size_t i = 0; i < patterns.size(); ++i) {
        pat.insert(pat.end(), patterns[i].begin(), patterns[i].end());
        poff.push_back((uint64_t)pat.size());
    }
    const W* s = reinterpret_cast<const W*>(sa.local_SA.data());
    const uint64_t* o = soff ? soff->data() : (const uint64_t*)0;
    const uint64_t m = soff ? (uint64_t)soff->size() - 1 : 0, q = (uint64_t)patterns.size();
    uint64_t z = 0;
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, o, m, s, pat.data(), poff.data(), q, k, e, (uint64_t*)0, (W*)0, (uint8_t*)0, 0, &z));
    std::vector<uint64_t> qid(z + 1);
    std::vector<W> tpos(z + 1);
    std::vector<uint8_t> dist(z + 1);
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, o, m, s, pat.data(), poff.data(), q, k, e, qid.data(), tpos.data(), dist.data(), z, &z));
    mismatch_lists<index_t> out;
    out.qid.assign(qid.begin(), qid.begin() + z);
    out.tpos.assign(tpos.begin(), tpos.begin() + z);
    out.dist.assign(dist.begin(), dist.begin() + z);
    return out;
}

} // namespace psacx

template <typename index_t, typename Iterator>
mismatch_lists<index_t> kmismatch(suffix_array<char, index_t, true, false>& sa, Iterator begin, Iterator end, const std::vector<std::string>& patterns,
                                  unsigned int e, unsigned int k = 0) {
    return psacx::kmismatch_of(sa, std::vector<uint8_t>(begin, end), (const std::vector<uint64_t>*)0, patterns, e, k);
}

template <typename index_t>
mismatch_lists<index_t> kmismatch(suffix_array<char, index_t, true, false>& sa, simple_dstringset& ss, const std::vector<std::string>& patterns,
                                  unsigned int e, unsigned int k = 0) {
    std::vector<uint8_t> text; std::vector<uint64_t> soff;
    psacx::flatten_set(ss, text, soff);
    return psacx::kmismatch_of(sa, text, &soff, patterns, e, k);
}

// Where the patterns occur in the text within edit distance e (psacx.h: "pattern search with edits"): hit i is pattern qid[i] against
// the len[i] bytes from text position tpos[i] (a position of the strings laid back to back, for a set), inside one string, at
// unit-cost Levenshtein distance dist[i] <= e: the smallest over all lengths from that start, and len[i] the shortest length that
// attains it.  Patterns of at most e bytes have no hits.  Order: ascending pattern, then ascending position.  best: only the hits
// of the smallest distance of every pattern.  k > 0 puts the k-mer lookup table in front of the piece searches.  One rank only, as
// kmismatch.
template <typename index_t>
struct edit_lists {
    std::vector<uint64_t> qid;
    std::vector<index_t> tpos;
    std::vector<index_t> len;
    std::vector<uint8_t> dist;
};

namespace psacx {

template <typename index_t>
edit_lists<index_t> kedit_of(suffix_array<char, index_t, true, false>& sa, const std::vector<uint8_t>& text, const std::vector<uint64_t>* soff,
                             const std::vector<std::string>& patterns, unsigned int e, unsigned int k, bool best) {
    static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    struct Call {
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint32_t* s, const uint8_t* p, const uint64_t* po,
                       uint64_t q, uint32_t k, uint32_t e, uint32_t f, uint64_t* qi, uint32_t* tp, uint32_t* l, uint8_t* d, uint64_t cap, uint64_t* z) {
            return psacx_kedit_u32(c, t, n, o, m, s, p, po, q, k, e, 0, f, qi, tp, l, d, cap, z);
        }
        static int run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint64_t* o, uint64_t m, const uint64_t* s, const uint8_t* p, const uint64_t* po,
                       uint64_t q, uint32_t k, uint32_t e, uint32_t f, uint64_t* qi, uint64_t* tp, uint64_t* l, uint8_t* d, uint64_t cap, uint64_t* z) {
            return psacx_kedit_u64(c, t, n, o, m, s, p, po, q, k, e, 0, f, qi, tp, l, d, cap, z);
        }
    };
    if (sa.multi_context()) throw std::runtime_error("psacx: kedit needs a single-rank communicator (the search runs on one GPU)");
    if (sa.n == 0 || text.size() != sa.n || sa.local_SA.size() != sa.n)
        throw std::runtime_error("kedit: the suffix array holds no SA of this text");
    std::vector<uint8_t> pat;
    std::vector<uint64_t> poff(1, 0);
    for (std::size_t i = 0; i < patterns.size(); ++i) {
        pat.insert(pat.end(), patterns[i].begin(), patterns[i].end());
        poff.push_back((uint64_t)pat.size());
    }
    const W* s = reinterpret_cast<const W*>(sa.local_SA.data());
    const uint64_t* o = soff ? soff->data() : (const uint64_t*)0;
    const uint64_t m = soff ? (uint64_t)soff->size() - 1 : 0, q = (uint64_t)patterns.size();
    const uint32_t f = best ? PSACX_KEDIT_BEST : 0u;
    uint64_t z = 0;
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, o, m, s, pat.data(), poff.data(), q, k, e, f, (uint64_t*)0, (W*)0, (W*)0, (uint8_t*)0, 0, &z));
    std::vector<uint64_t> qid(z + 1);
    std::vector<W> tpos(z + 1), len(z + 1);
    std::vector<uint8_t> dist(z + 1);
    check(sa.context(), Call::run(sa.context(), text.data(), sa.n, o, m, s, pat.data(), poff.data(), q, k, e, f, qid.data(), tpos.data(), len.data(), dist.data(), z,
                                  &z));
    edit_lists<index_t> out;
    out.qid.assign(qid.begin(), qid.begin() + z);
    out.tpos.assign(tpos.begin(), tpos.begin() + z);
    out.len.assign(len.begin(), len.begin() + z);
    out.dist.assign(dist.begin(), dist.begin() + z);
    return out;
}

} // namespace psacx

template <typename index_t, typename Iterator>
edit_lists<index_t> kedit(suffix_array<char, index_t, true, false>& sa, Iterator begin, Iterator end, const std::vector<std::string>& patterns,
                          unsigned int e, unsigned int k = 0, bool best = false) {
    return psacx::kedit_of(sa, std::vector<uint8_t>(begin, end), (const std::vector<uint64_t>*)0, patterns, e, k, best);
}

template <typename index_t>
edit_lists<index_t> kedit(suffix_array<char, index_t, true, false>& sa, simple_dstringset& ss, const std::vector<std::string>& patterns,
                          unsigned int e, unsigned int k = 0, bool best = false) {
    std::vector<uint8_t> text; std::vector<uint64_t> soff;
    psacx::flatten_set(ss, text, soff);
    return psacx::kedit_of(sa, text, &soff, patterns, e, k, best);
}

// The FM-index of the text or string set of a suffix array (psacx.h: "FM-index"), resident in HBM.  It is built from the suffix array
// and the bytes it was constructed from -- fm_index(sa, begin, end) for one text, fm_index(sa, ss) for a string set -- and owns nothing
// but its blob, its descriptor, the string offsets and a context of its own on the device of `sa`: text and suffix array may go once it stands.
// count: element i = [lb, ub) of patterns[i], the interval of locate where it occurs and (0, 0) where it does not.  locate: the
// occurrence lists of occurrences(), from the sampled suffix array (sample > 0; sample == 0 builds an index that counts only).
// With text_rate > 0 the index carries the text samples too and gives the bytes back: extract(pos, len) returns the slices
// S[pos[i] .. pos[i] + len[i]) back to back, each clipped at the end of its string, with start[i] where slice i begins; text() the
// strings of the set (one for a text).  Without text samples both throw.
template <typename index_t>
class fm_index {
    typedef typename std::conditional<sizeof(index_t) == 4, uint32_t, uint64_t>::type W;
    static int build(psacx_ctx* c, uint64_t n, const uint8_t* b, const uint32_t* f, const uint32_t* s, uint64_t r, uint64_t* fm, psacx_fm_info* i) { return psacx_fm_index_dev_u32(c, n, b, f, s, r, fm, i); }
    static int build(psacx_ctx* c, uint64_t n, const uint8_t* b, const uint32_t* f, const uint64_t* s, uint64_t r, uint64_t* fm, psacx_fm_info* i) { return psacx_fm_index_dev_u64(c, n, b, f, s, r, fm, i); }
    static int bwt_run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* e, const uint32_t* s, uint8_t* b, uint32_t* f) { return psacx_bwt_dev_u32(c, t, n, e, s, b, f, 0); }
    static int bwt_run(psacx_ctx* c, const uint8_t* t, uint64_t n, const uint32_t* e, const uint64_t* s, uint8_t* b, uint32_t* f) { return psacx_bwt_dev_u64(c, t, n, e, s, b, f, 0); }
    static int count_run(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint8_t* p, const uint64_t* o, uint64_t q, uint32_t* l, uint32_t* u) { return psacx_fm_count_dev_u32(c, fm, i, p, o, q, l, u); }
    static int count_run(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint8_t* p, const uint64_t* o, uint64_t q, uint64_t* l, uint64_t* u) { return psacx_fm_count_dev_u64(c, fm, i, p, o, q, l, u); }
    static int occ_run(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint64_t* o, uint64_t m, const uint32_t* l, const uint32_t* u, uint64_t q, uint64_t lim,
                       uint64_t* st, uint32_t* p, uint32_t* s, uint64_t cap, uint64_t* tot) { return psacx_fm_occurrences_dev_u32(c, fm, i, o, m, l, u, q, lim, st, p, s, cap, tot); }
    static int occ_run(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint64_t* o, uint64_t m, const uint64_t* l, const uint64_t* u, uint64_t q, uint64_t lim,
                       uint64_t* st, uint64_t* p, uint64_t* s, uint64_t cap, uint64_t* tot) { return psacx_fm_occurrences_dev_u64(c, fm, i, o, m, l, u, q, lim, st, p, s, cap, tot); }

    static int ts_run(psacx_ctx* c, uint64_t n, const uint32_t* s, const uint64_t* o, uint64_t m, uint64_t r, uint32_t* ts, uint64_t* e) { return psacx_fm_text_samples_dev_u32(c, n, s, o, m, r, ts, e); }
    static int ts_run(psacx_ctx* c, uint64_t n, const uint64_t* s, const uint64_t* o, uint64_t m, uint64_t r, uint64_t* ts, uint64_t* e) { return psacx_fm_text_samples_dev_u64(c, n, s, o, m, r, ts, e); }
    static int ext_run(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint32_t* ts, uint64_t r, const uint64_t* o, uint64_t m, const uint32_t* p, const uint32_t* l,
                       uint64_t q, uint64_t* st, uint8_t* out, uint64_t cap, uint64_t* tot) { return psacx_fm_extract_dev_u32(c, fm, i, ts, r, o, m, p, l, q, st, out, cap, tot); }
    static int ext_run(psacx_ctx* c, const uint64_t* fm, const psacx_fm_info* i, const uint64_t* ts, uint64_t r, const uint64_t* o, uint64_t m, const uint64_t* p, const uint64_t* l,
                       uint64_t q, uint64_t* st, uint8_t* out, uint64_t cap, uint64_t* tot) { return psacx_fm_extract_dev_u64(c, fm, i, ts, r, o, m, p, l, q, st, out, cap, tot); }

    struct held {                                                // device buffers that go on every path
        psacx_ctx* c; std::vector<void*> v;
        explicit held(psacx_ctx* ctx) : c(ctx) {}
        ~held() { for (std::size_t i = 0; i < v.size(); ++i) (void)psacx_dev_free(c, v[i]); }
        void* dev(const void* src, uint64_t bytes) {
            void* p = 0;
            psacx::check(c, psacx_dev_alloc(c, &p, bytes ? bytes : 1));
            v.push_back(p);
            if (src && bytes) psacx::check(c, psacx_copy_h2d(c, p, src, bytes));
            return p;
        }
    };

    psacx_ctx* c_;
    uint64_t* d_fm_;
    uint64_t* d_off_;
    uint64_t m_;
    psacx_fm_info info_;
    W* d_ts_;                                                    // the text samples (text_rate > 0)
    uint64_t text_rate_, text_entries_;
    std::vector<uint64_t> soff_;                                 // the offsets on the host: text() asks for every string by them

    template <bool LCP, bool LC>
    void make(suffix_array<char, index_t, LCP, LC>& sa, const std::vector<uint8_t>& text, const std::vector<uint64_t>* soff, std::size_t sample,
              std::size_t text_rate) {
        static_assert(sizeof(std::size_t) == 8, "size_t must be 64 bit");
        if (sa.multi_context()) throw std::runtime_error("psacx: fm_index needs a single-rank communicator (the index is built on one GPU)");
        if (sa.n == 0 || text.size() != sa.n || sa.local_SA.size() != sa.n) throw std::runtime_error("fm_index: text does not match the suffix array");
        psacx::check(0, psacx_create(&c_, sa.comm.device(), 0));     // a context of its own: the index outlives `sa`
        const uint64_t n = (uint64_t)sa.n;
        held h(c_);
        const uint8_t* d_text = (const uint8_t*)h.dev(text.data(), n);
        const W* d_sa = (const W*)h.dev(sa.local_SA.data(), n * sizeof(W));
        uint8_t* d_bwt = (uint8_t*)h.dev(0, n);
        uint32_t* d_first = (uint32_t*)h.dev(0, ((n >> 5) + 1) * 4);
        uint32_t* d_ends = 0;
        if (soff) {
            m_ = (uint64_t)soff->size() - 1;
            void* p = 0;
            psacx::check(c_, psacx_dev_alloc(c_, &p, (m_ + 1) * 8));
            d_off_ = (uint64_t*)p;                               // (kept: the lists name the string of a position by it)
            psacx::check(c_, psacx_copy_h2d(c_, d_off_, soff->data(), (m_ + 1) * 8));
            d_ends = (uint32_t*)h.dev(0, ((n >> 5) + 1) * 4);
            uint64_t words = 0;
            psacx::check(c_, psacx_string_ends_dev(c_, d_off_, m_, n, d_ends, &words));
        }
        psacx::check(c_, bwt_run(c_, d_text, n, d_ends, d_sa, d_bwt, d_first));
        const W* sa_in = sample ? d_sa : (const W*)0;
        psacx::check(c_, build(c_, n, d_bwt, d_first, sa_in, (uint64_t)sample, (uint64_t*)0, &info_));
        void* p = 0;
        psacx::check(c_, psacx_dev_alloc(c_, &p, info_.words * 8));
        d_fm_ = (uint64_t*)p;
        psacx::check(c_, build(c_, n, d_bwt, d_first, sa_in, (uint64_t)sample, d_fm_, &info_));
        if (soff) soff_ = *soff;
        if (text_rate) {
            text_rate_ = (uint64_t)text_rate;
            psacx::check(c_, ts_run(c_, n, (const W*)0, d_off_, m_, text_rate_, (W*)0, &text_entries_));
            psacx::check(c_, psacx_dev_alloc(c_, &p, text_entries_ * sizeof(W)));
            d_ts_ = (W*)p;
            psacx::check(c_, ts_run(c_, n, d_sa, d_off_, m_, text_rate_, d_ts_, &text_entries_));
        }
    }
    void drop() {
        if (d_fm_) (void)psacx_dev_free(c_, d_fm_);
        if (d_off_) (void)psacx_dev_free(c_, d_off_);
        if (d_ts_) (void)psacx_dev_free(c_, d_ts_);
        d_fm_ = 0; d_off_ = 0; d_ts_ = 0;
        if (c_) psacx_destroy(c_);
        c_ = 0;
    }
    fm_index(const fm_index&);                                   // (one owner of the blob)
    fm_index& operator=(const fm_index&);

public:
    template <bool LCP, bool LC, typename Iterator>
    fm_index(suffix_array<char, index_t, LCP, LC>& sa, Iterator begin, Iterator end, std::size_t sample = 32, std::size_t text_rate = 0)
        : c_(0), d_fm_(0), d_off_(0), m_(0), d_ts_(0), text_rate_(0), text_entries_(0) {
        try { make(sa, std::vector<uint8_t>(begin, end), (const std::vector<uint64_t>*)0, sample, text_rate); } catch (...) { drop(); throw; }
    }
    template <bool LCP>
    fm_index(suffix_array<char, index_t, LCP, false>& sa, simple_dstringset& ss, std::size_t sample = 32, std::size_t text_rate = 0)
        : c_(0), d_fm_(0), d_off_(0), m_(0), d_ts_(0), text_rate_(0), text_entries_(0) {
        std::vector<uint8_t> text; std::vector<uint64_t> soff;
        psacx::flatten_set(ss, text, soff);
        try { make(sa, text, &soff, sample, text_rate); } catch (...) { drop(); throw; }
    }
    ~fm_index() { drop(); }

    std::size_t bytes() const { return (std::size_t)info_.words * 8 + (std::size_t)text_entries_ * sizeof(W); }          // the index in HBM, text samples included
    std::size_t size() const { return (std::size_t)info_.n; }
    const psacx_fm_info& info() const { return info_; }

    std::vector<std::pair<index_t, index_t> > count(const std::vector<std::string>& patterns) const {
        std::vector<uint8_t> pat;
        std::vector<uint64_t> off(1, 0);
        for (std::size_t i = 0; i < patterns.size(); ++i) {
            pat.insert(pat.end(), patterns[i].begin(), patterns[i].end());
            off.push_back(pat.size());
        }
        const uint64_t q = (uint64_t)patterns.size();
        std::vector<W> lb(q), ub(q);
        held h(c_);
        const uint8_t* d_pat = (const uint8_t*)h.dev(pat.data(), pat.size());
        const uint64_t* d_poff = (const uint64_t*)h.dev(off.data(), (q + 1) * 8);
        W* d_lb = (W*)h.dev(0, q * sizeof(W));
        W* d_ub = (W*)h.dev(0, q * sizeof(W));
        psacx::check(c_, count_run(c_, d_fm_, &info_, d_pat, d_poff, q, d_lb, d_ub));
        if (q) {
            psacx::check(c_, psacx_copy_d2h(c_, lb.data(), d_lb, q * sizeof(W)));
            psacx::check(c_, psacx_copy_d2h(c_, ub.data(), d_ub, q * sizeof(W)));
        }
        std::vector<std::pair<index_t, index_t> > out(patterns.size());
        for (std::size_t i = 0; i < patterns.size(); ++i) out[i] = std::make_pair((index_t)lb[i], (index_t)ub[i]);
        return out;
    }

    occurrence_lists<index_t> locate(const std::vector<std::string>& patterns, std::size_t limit = 0) const {
        const std::vector<std::pair<index_t, index_t> > iv = count(patterns);
        const uint64_t q = (uint64_t)iv.size();
        std::vector<W> lb(q), ub(q);
        for (std::size_t i = 0; i < iv.size(); ++i) { lb[i] = (W)iv[i].first; ub[i] = (W)iv[i].second; }
        occurrence_lists<index_t> out;
        out.start.assign(q + 1, 0);
        held h(c_);
        const W* d_lb = (const W*)h.dev(lb.data(), q * sizeof(W));
        const W* d_ub = (const W*)h.dev(ub.data(), q * sizeof(W));
        uint64_t* d_start = (uint64_t*)h.dev(0, (q + 1) * 8);
        uint64_t total = 0;
        psacx::check(c_, occ_run(c_, d_fm_, &info_, d_off_, m_, d_lb, d_ub, q, (uint64_t)limit, d_start, (W*)0, (W*)0, 0, &total));
        out.pos.assign(total, 0);
        if (d_off_) out.sid.assign(total, 0);
        W* d_pos = (W*)h.dev(0, total * sizeof(W));
        W* d_sid = d_off_ ? (W*)h.dev(0, total * sizeof(W)) : (W*)0;
        psacx::check(c_, occ_run(c_, d_fm_, &info_, d_off_, m_, d_lb, d_ub, q, (uint64_t)limit, d_start, d_pos, d_sid, total, &total));
        psacx::check(c_, psacx_copy_d2h(c_, out.start.data(), d_start, (q + 1) * 8));
        if (total) psacx::check(c_, psacx_copy_d2h(c_, out.pos.data(), d_pos, total * sizeof(W)));
        if (total && d_off_) psacx::check(c_, psacx_copy_d2h(c_, out.sid.data(), d_sid, total * sizeof(W)));
        return out;
    }

    std::vector<uint8_t> extract(const std::vector<index_t>& pos, const std::vector<index_t>& len, std::vector<std::size_t>& start) const {
        if (!d_ts_) throw std::runtime_error("fm_index: the index has no text samples (text_rate == 0)");
        if (pos.size() != len.size()) throw std::runtime_error("fm_index: extract needs one length per position");
        const uint64_t q = (uint64_t)pos.size();
        std::vector<W> p(pos.begin(), pos.end()), l(len.begin(), len.end());
        start.assign(q + 1, 0);
        held h(c_);
        const W* d_pos = (const W*)h.dev(p.data(), q * sizeof(W));
        const W* d_len = (const W*)h.dev(l.data(), q * sizeof(W));
        uint64_t* d_start = (uint64_t*)h.dev(0, (q + 1) * 8);
        uint64_t total = 0;
        psacx::check(c_, ext_run(c_, d_fm_, &info_, d_ts_, text_rate_, d_off_, m_, d_pos, d_len, q, d_start, (uint8_t*)0, 0, &total));
        std::vector<uint8_t> out(total);
        uint8_t* d_out = (uint8_t*)h.dev(0, total);
        psacx::check(c_, ext_run(c_, d_fm_, &info_, d_ts_, text_rate_, d_off_, m_, d_pos, d_len, q, d_start, d_out, total, &total));
        std::vector<uint64_t> st(q + 1, 0);
        psacx::check(c_, psacx_copy_d2h(c_, st.data(), d_start, (q + 1) * 8));
        start.assign(st.begin(), st.end());
        if (total) psacx::check(c_, psacx_copy_d2h(c_, out.data(), d_out, total));
        return out;
    }

    std::vector<std::string> text() const {
        std::vector<index_t> pos, len;
        if (soff_.empty()) { pos.push_back(0); len.push_back((index_t)info_.n); }
        for (std::size_t j = 0; j + 1 < soff_.size(); ++j) { pos.push_back((index_t)soff_[j]); len.push_back((index_t)(soff_[j + 1] - soff_[j])); }
        std::vector<std::size_t> start;
        const std::vector<uint8_t> out = extract(pos, len, start);
        std::vector<std::string> strings;
        for (std::size_t j = 0; j + 1 < start.size(); ++j) strings.push_back(std::string(out.begin() + start[j], out.begin() + start[j + 1]));
        return strings;
    }
};

#endif // PSACX_SUFFIX_ARRAY_HPP
