// first_round.hpp -- the first round of the construction on one MI355X: alphabet and k, the sort on the 2k-character window (two stages,
// or one sort over both words), LCP and bucket ids, SA -> ISA, the first list of unresolved suffixes.  Included by construct.hpp behind the
// helpers it uses (Work, carve, run_carries, run_compact, invert_permutation, finish_inversion32, the isa_* shapes); construct_dev calls
// first_round and goes on with the refinement rounds.
#pragma once

namespace psacx {

// What first_round_shape decides: the code table, the window, k, the bits of the two key words, the leading bits stage 1 sorts on
struct FirstShape {
    CodeTable tab; KeyShape ks; uint32_t k;
    unsigned bits_w1, bits_w2, lead;
    bool two_stage;
};
// The sorted records of the first round as the rebucket kernel takes them
template <typename T> struct FirstSorted {
    SortBufs<T> rec;
    bool onew;               // the sorted records of the first round are still one-word (sa_kernels.hpp: OneWordView); rec.k1 holds them
    OneWordView view;
    T* onew_w1;              // ... and word 1 of the suffixes that tie on the leading bits is here
    bool packed1;            // the one-word sort ran: word 1 comes back without its bits below the prefix
    uint8_t* tie_bytes;      // ... and left the lowest byte of every record's prefix bits here (engine.hpp: onew_bucket_passes)
    bool tie_bits;           // ... or, from the group sort, a bit per place in its first n / 8 bytes: the places p - 1 and p tie (tie_bits.hpp)
};

// (64-bit words, at most 2^32 characters: the list comes with its entries' bucket numbers counted from 0, in the idle upper half of the
//  payload array -- the one-word sort keys of the refinement rounds then need only as many bits as there are buckets)
// (ALIAS: ord_arr is the upper half of w.x.v.  x.v is also written in full by the last pass of a v32 sort, by shift_keys_kernel in whole
//  rounds at n = 2^32, by three-word sorts and as level-1 ISA pairs by the fused rebucket kernel.  Every reader of ord_arr --
//  gather_keys_kernel with by_ord -- runs directly after the run_compact that wrote it and before the round's sort touches x.v; keep it so.)
template <typename T> inline uint32_t* ord_array(const Work<T>& w, uint64_t n) {
    return (sizeof(T) == 8 && n <= (1ull << 32)) ? reinterpret_cast<uint32_t*>(w.x.v) + n : (uint32_t*)nullptr;
}

// ---- alphabet (alphabet.hpp:213-218) and k (kmer.hpp:26-40), the window, the leading bits, one stage or two
template <typename T>
int first_round_shape(psacx_ctx* c, Work<T>& w, const uint8_t* d_text, uint64_t n, uint32_t k_req, bool gsa, FirstShape& sh) {
    const Knobs& kn = c->knobs;
    psacx_stats& st = c->stats;
    {
        ProfScope ps(c, TC_ALPHABET);
        PSACX_HIP(c, hipMemsetAsync(w.d_hist256, 0, 256 * sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL((char_hist_kernel<256>), dim3(grid_for(c, n / 16 + 1, 256, 8)), dim3(256), 0, c->stream,
                           d_text, n, w.d_hist256);
        PSACX_HIP(c, hipGetLastError());
    }
    unsigned long long* h_hist = w.sc.h_hist;          // (free until the first sort)
    PSACX_HIP(c, hipMemcpyAsync(h_hist, w.d_hist256, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t lc = 1;
    build_alphabet(h_hist, sh.tab, st.sigma, st.bits_per_char, lc);
    const uint32_t l = st.bits_per_char;
    const uint32_t k = choose_k((uint32_t)sizeof(T) * 8, l, n, k_req);
    st.k = sh.k = k;
    // the 2k-character window of the first round, packed with lc bits per character
    KeyShape& ks = sh.ks;
    if (gsa) {
        // string ends need their own code in the key: psac's codes 1..sigma with l bits, 0 = end
        for (int ch = 0; ch < 256; ++ch) if (h_hist[ch]) sh.tab.c[ch] = (uint16_t)(sh.tab.c[ch] + 1);
        lc = l;
    }
    ks.lc = lc;
    ks.c1 = std::min<uint32_t>(2 * k, (uint32_t)(sizeof(T) * 8) / lc);
    ks.c2 = 2 * k - ks.c1;
    ks.spec = gsa ? 0 : std::min<uint64_t>(2ull * k - 1, n);

    // ---- first rank-pair sort (idxsort.hpp:23-83); payload = text position -> SA.
    // Two stages when the leading bits of word 1 already separate almost every suffix (random DNA,
    // 32-bit words: 4^16 windows for 2^28 suffixes; 64-bit words: the top 40 bits for 2^32): stage 1
    // sorts (word 1, suffix) pairs on those bits only -- two thirds of the bytes per pass and far
    // fewer passes -- and stage 2 orders the suffixes that still tie by the full window.
    const unsigned bits_w1 = ks.c1 * lc, bits_w2 = ks.c2 * lc;
    unsigned lead = bits_for(n - 1) + 3;                      // leading bits stage 1 sorts on (ties: ~ n / 2^lead)
    lead = (lead + RADIX_BITS - 1) / RADIX_BITS * RADIX_BITS;
    // word 1 slightly too short for that (DNA, 32-bit words, 2^29 < n <= 2^30): all of word 1 still leaves
    // fewer than a quarter of the suffixes tied, which is cheaper than carrying word 2 through five passes
    const unsigned slack = 2;
    if (lead > bits_w1 && bits_for(n - 1) + slack <= bits_w1 && bits_w1 % RADIX_BITS == 0) lead = bits_w1;
    // PSACX_OPT_FIRST_LEAD (tests): more leading bits than the text needs, e.g. the 40 of a text of 2^32 characters
    if (kn.first_lead && kn.first_lead % RADIX_BITS == 0 && kn.first_lead >= bits_for(n - 1) + 3 && kn.first_lead <= 32 + RADIX_BITS && kn.first_lead <= bits_w1)
        lead = kn.first_lead;
    sh.bits_w1 = bits_w1; sh.bits_w2 = bits_w2; sh.lead = lead;
    sh.two_stage = !gsa && n >= (1ull << 21) && !kn.one_stage && lead <= bits_w1 &&
                   lead + RADIX_BITS <= bits_w1 + bits_w2;     // at least one pass less
    return PSACX_OK;
}

// ---- first-round keys: the 2k-character window at every position, packed (kmer.hpp:119-177,
//      shifting.hpp:33-122; see key_pairs_kernel for the packing)
// (the one-word prefix sort computes word 1 inside its pass on the top digit: no keys in memory unless it has to give up)
// k2rec == nullptr: word 2 is not kept; with_hist: the pass-1 histograms of the stage-1 sort on the bits above lo1 ride along
template <typename T>
int make_first_keys(psacx_ctx* c, Work<T>& w, const uint8_t* d_text, uint64_t n, const T* d_slen, const FirstShape& sh, T* k1, T* k2rec,
                    bool with_hist, unsigned lo1) {
    ProfScope ps(c, TC_KMER);
    constexpr int KB = 256, KI = 8;
    uint64_t nb = (n + KB * KI - 1) / (KB * KI);
    if (d_slen)
        hipLaunchKernelGGL((key_pairs_kernel<T, KB, KI, true>), dim3((unsigned)nb), dim3(KB), 0, c->stream, d_text, n, n,
                           sh.tab, sh.ks, k1, k2rec, w.sc.d_partials, d_slen);
    else if (with_hist) {
        // tile shape of the stage-1 sort, pass-1 histograms written on the way
        constexpr int HB = ScatterCfg<T>::BLOCK, HI = ScatterCfg<T>::ITEMS;
        nb = (n + HB * HI - 1) / (HB * HI);
        hipLaunchKernelGGL((key_pairs_kernel<T, HB, HI, false, true>), dim3((unsigned)nb), dim3(HB), 0, c->stream, d_text, n, n,
                           sh.tab, sh.ks, k1, k2rec, w.sc.d_partials, (const T*)nullptr,
                           pass_scratch(w.sc.d_desc, nb).tile_hist, (int)lo1);
    } else
        hipLaunchKernelGGL((key_pairs_kernel<T, KB, KI>), dim3((unsigned)nb), dim3(KB), 0, c->stream, d_text, n, n,
                           sh.tab, sh.ks, k1, k2rec, w.sc.d_partials, (const T*)nullptr);
    PSACX_HIP(c, hipGetLastError());
    PSACX_TRY(summary_finish(c, w.sc, (unsigned)nb));
    return PSACX_OK;
}

// Stage 2 of the two-stage sort: s.rec.k1 / d_sa are sorted on the leading bits; the suffixes that tie on them are ordered by their full
// windows.  first_in / first_alt: the record sets stage 1 started from and sorted into.  PSACX_RETRY_1STAGE: more ties than the
// reduced-memory layout has room for.
template <typename T>
int resolve_prefix_ties(psacx_ctx* c, Work<T>& w, const uint8_t* d_text, uint64_t n, T* d_sa, T* d_isa, const FirstShape& sh,
                        const SortBufs<T>& first_in, const SortBufs<T>& first_alt, FirstSorted<T>& s) {
    const Knobs& kn = c->knobs;
    const CodeTable& tab = sh.tab;
    const KeyShape& ks = sh.ks;
    const unsigned lo1 = sh.bits_w1 - sh.lead, bits_w1 = sh.bits_w1, bits_w2 = sh.bits_w2;
    psacx_round* r0 = &c->stats.rounds[0];
    T* S1 = s.rec.k1;
    T* const S2 = w.diet ? w.x.k2 : first_alt.k2;        // word 2 in sorted order, filled for the ties only
    T* free_k1 = (S1 == w.x.k1) ? w.y.k1 : w.x.k1;
    // stage 2, common case: all tie groups are tiny and get ordered in place
    // (tile shapes measured: 64-bit words 256 x 32: 10.7 ms at 2^32, 128 x 32: 11.1, 256 x 16: 13.0, 512 x 8: 16.6;
    //  32-bit words 256 x 16: 1.2-1.3 ms at 2^28, 128 x 32: 1.4)
    constexpr int TB = 256, TI = sizeof(T) == 8 ? 32 : 16, TG = 8;
    unsigned long long* d_big = reinterpret_cast<unsigned long long*>(w.d_totals + 2);
    unsigned long long* h_big = reinterpret_cast<unsigned long long*>(c->pinned + PIN_TIE_BIG);
    {
        ProfScope ps(c, TC_GATHER);
        PSACX_HIP(c, hipMemsetAsync(d_big, 0, sizeof(unsigned long long), c->stream));
        const uint64_t nb = (n + (uint64_t)TB * TI - 1) / ((uint64_t)TB * TI);
        if constexpr (sizeof(T) == 8) {
            // S1: the one-word records; the array the last pass did not write takes word 1 of the tied suffixes.  With the bytes of the
            // last pass: persistent waves, a tile of 64 x 32 places each per trip, four workgroups per CU (sa_kernels.hpp;
            // PSACX_OPT_PLAIN_SIDE_KERNELS pins the workgroup-per-tile kernel)
            const uint64_t nwt = (n + (uint64_t)WAVE * TI - 1) / ((uint64_t)WAVE * TI);
            const uint64_t nbt = (n + (uint64_t)WAVE * 64 - 1) / ((uint64_t)WAVE * 64);          // (with the tie bits: a word per lane)
            c->stats.tie_form = !s.onew ? 0 : s.tie_bits ? 2 : s.tie_bytes ? 1 : 0;
            if (s.onew && s.tie_bytes && s.tie_bits)
                hipLaunchKernelGGL((tie_resolve_1w_waves_kernel<TB, TI, TG, true>), dim3((unsigned)grid_for(c, nbt * WAVE, TB, 4)), dim3(TB), 0, c->stream,
                                   reinterpret_cast<uint64_t*>(S1), reinterpret_cast<uint64_t*>(free_k1), reinterpret_cast<uint64_t*>(S2), n, s.view, d_text, n,
                                   tab, ks, d_big, (const uint8_t*)s.tie_bytes, nbt);
            else if (s.onew && s.tie_bytes && !kn.plain_side_kernels)
                hipLaunchKernelGGL((tie_resolve_1w_waves_kernel<TB, TI, TG>), dim3((unsigned)grid_for(c, nwt * WAVE, TB, 4)), dim3(TB), 0, c->stream,
                                   reinterpret_cast<uint64_t*>(S1), reinterpret_cast<uint64_t*>(free_k1), reinterpret_cast<uint64_t*>(S2), n, s.view, d_text, n,
                                   tab, ks, d_big, (const uint8_t*)s.tie_bytes, nwt);
            else if (s.onew)
                hipLaunchKernelGGL((tie_resolve_1w_kernel<TB, TI, TG>), dim3((unsigned)nb), dim3(TB), 0, c->stream, reinterpret_cast<uint64_t*>(S1),
                                   reinterpret_cast<uint64_t*>(free_k1), reinterpret_cast<uint64_t*>(S2), n, s.view, d_text, n, tab, ks, d_big,
                                   (const uint8_t*)s.tie_bytes);
        }
        if (!kn.ties_radix && !s.onew)
            hipLaunchKernelGGL((tie_resolve_kernel<T, TB, TI, TG>), dim3((unsigned)nb), dim3(TB), 0, c->stream, S1, d_sa, S2, n, lo1,
                               d_text, n, tab, ks, d_big, s.packed1);
        PSACX_HIP(c, hipGetLastError());
    }
    PSACX_HIP(c, hipMemcpyAsync(h_big, d_big, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    PSACX_HIP(c, hipStreamSynchronize(c->stream));
    if constexpr (sizeof(T) == 8) {
        if (s.onew && *h_big) {
            // a long group: the radix path below works on word 1 and the suffixes as arrays -- written now, as the last pass would have
            ProfScope ps(c, TC_GATHER);
            hipLaunchKernelGGL(onew_widen_kernel<0>, dim3(grid_for(c, n, 256, 8)), dim3(256), 0, c->stream, reinterpret_cast<const uint64_t*>(S1), n, s.view,
                               reinterpret_cast<uint64_t*>(free_k1), reinterpret_cast<uint64_t*>(d_sa));
            PSACX_HIP(c, hipGetLastError());
            std::swap(S1, free_k1);
            s.rec.k1 = S1;
            s.onew = false;
        }
    }
    if (*h_big || kn.ties_radix) {
        // some group is long (repetitive text): compact all ties and radix-sort them by the full window
        const uint64_t ntiles = (n + ScanCfg<T>::TILE - 1) / ScanCfg<T>::TILE;
        {
            ProfScope ps(c, TC_COMPACT);
            hipLaunchKernelGGL((count_active_kernel<T, ScanCfg<T>::BLOCK, SCAN_ITEMS>), dim3((unsigned)ntiles), dim3(ScanCfg<T>::BLOCK), 0,
                               c->stream, S1, n, (T)0, (T)0, w.d_nact, lo1, w.d_nunf);
            PSACX_HIP(c, hipGetLastError());
        }
        // two record sets for the ties out of buffers that are idle until the rebucket step; the
        // compaction already fills word 1 and the suffix of set a
        SortBufs<T> a, b, s2;
        if (w.diet) { a = w.ry; b.k1 = w.bsa; b.k2 = w.x.v; b.v = free_k1; }
        else { a.k1 = free_k1; a.k2 = first_alt.v; a.v = first_in.v; b.k1 = w.bsa; b.k2 = w.pos_b; b.v = d_isa; }
        // (the tie groups counted from 0 beside the list, in the idle second key array of set b: the sort below takes the group's
        //  number in place of the sorted prefix)
        uint32_t* const tie_ord = reinterpret_cast<uint32_t*>(b.k2);
        uint64_t ties = 0, tie_groups = 0;
        bool tie_v32 = sizeof(T) == 8 && n <= (1ull << 32);         // (the suffixes of the ties as 32-bit entries through the sort)
        PSACX_TRY(run_compact<T>(c, w, S1, nullptr, n, w.pos_a, &ties, &tie_groups, w.cap_active, lo1, d_sa, a.k1, a.v, 0, false, tie_ord, &tie_v32));
        const unsigned ord_bits = bits_for(tie_groups > 1 ? tie_groups - 1 : 1);
        const bool by_ord = lo1 > 0 && ties > 0 && tie_groups > 0 && tie_groups < (1ull << 32) && lo1 + ord_bits + RADIX_BITS <= bits_w1;
        // repetitive text in the reduced-memory layout: there is no room to sort all ties at once, so the
        // first round is run again as one sort over both words (the keys were sorted in place: rebuilt)
        if (ties > w.cap_active) return PSACX_RETRY_1STAGE;
        if (ties) {
            {
                ProfScope ps(c, TC_GATHER);
                const int gg = grid_for(c, ties, 256, 16);
                hipLaunchKernelGGL((gather_prefix_ties_kernel<T, 256>), dim3(gg), dim3(256), 0, c->stream, ties, a.k1, a.v,
                                   d_text, n, tab, ks, a.k2, w.sc.d_partials, s.packed1, by_ord ? (const uint32_t*)tie_ord : (const uint32_t*)nullptr, lo1, tie_v32 ? 1 : 0);
                PSACX_HIP(c, hipGetLastError());
                PSACX_TRY(summary_finish(c, w.sc, (unsigned)gg));
            }
            psacx_round r1;
            std::memset(&r1, 0, sizeof(r1));
            PSACX_TRY(pair_sort<T>(c, w.sc, a, b, ties, /*iota=*/false, by_ord ? lo1 + ord_bits : bits_w1, bits_w2, nullptr, &s2, &r1, 0, 0,
                                   /*summary_ready=*/true, 0, -1, /*v32_in=*/tie_v32));
            r0->sort_passes += r1.sort_passes; r0->sort_passes_skipped += r1.sort_passes_skipped;
            ProfScope ps(c, TC_GATHER);
            hipLaunchKernelGGL((scatter_prefix_ties_kernel<T>), dim3(grid_for(c, ties, 256, 16)), dim3(256), 0, c->stream,
                               w.pos_a, ties, lo1 ? s2.k1 : (const T*)nullptr, s2.k2, s2.v, S1, S2, d_sa, by_ord ? lo1 : 0u);
            PSACX_HIP(c, hipGetLastError());
        }
    }
    s.rec.k2 = S2; s.rec.v = d_sa;
    s.onew_w1 = s.onew ? free_k1 : (T*)nullptr;
    return PSACX_OK;
}

// The two-stage sort: (word 1, suffix) on the leading bits -- in one-word records where they fit -- then the ties.
// PSACX_RETRY_1STAGE: one sort over both words instead (the probe of the one-word sort, or resolve_prefix_ties)
template <typename T>
int first_sort_two_stage(psacx_ctx* c, Work<T>& w, const uint8_t* d_text, uint64_t n, T* d_sa, T* d_isa, const FirstShape& sh, FirstSorted<T>& s) {
    const Knobs& kn = c->knobs;
    psacx_round* r0 = &c->stats.rounds[0];
    const unsigned lo1 = sh.bits_w1 - sh.lead, lead = sh.lead;
    // one-word records, most significant digit first (engine.hpp: prefix_sort_1w): 64-bit words, suffixes below 2^32, the
    // prefix without its top digit in 32 bits
    bool one_word = sizeof(T) == 8 && n <= (1ull << 32) && n >= (1ull << kn.one_word_min) && lead >= 3 * RADIX_BITS &&
                    lead <= 32 + RADIX_BITS && lead % RADIX_BITS == 0 && !kn.no_one_word;

    // In the diet layout the second record set is the output buffers (y = ISA, LCP, SA).  Two stages: only word 1 and the suffix are sorted;
    // word 1 may just as well end up in the ISA buffer (it is dead before the inversion writes ISA), and then the suffixes
    // land in the SA buffer itself instead of being copied there (n w bytes read + written: 13 ms of a 4 GiB / uint64
    // construction) -- so an even number of passes starts from y.
    const unsigned planned = lead / RADIX_BITS;
    const bool start_y = w.diet && !(planned & 1u);
    SortBufs<T> first_in = start_y ? w.y : w.x, first_alt = start_y ? w.x : w.y;
    // with two stages word 2 is not kept at all (the few suffixes that need it read it from the text)
    if (!one_word) PSACX_TRY(make_first_keys<T>(c, w, d_text, n, nullptr, sh, first_in.k1, nullptr, true, lo1));

    std::memset(r0, 0, sizeof(*r0));
    SortBufs<T> in1{first_in.k1, nullptr, first_in.v}, alt1{first_alt.k1, nullptr, first_alt.v};
    if constexpr (sizeof(T) == 8) {
        if (one_word) {
            uint64_t* s1 = nullptr;
            // the records stay one-word through the tie stage and the rebucket kernel when that kernel runs in its fused form
            const bool keep = !kn.widen_last && !kn.ties_radix && isa_narrow_levels<T>(n, kn) > 0;
            // (the digit bytes between the passes live in the array that takes word 2 of the tied suffixes after the sort: idle until then)
            uint8_t* const dig = kn.no_digit_bytes ? (uint8_t*)nullptr : reinterpret_cast<uint8_t*>(w.diet ? w.x.k2 : first_alt.k2);
            // (... and the bytes the tie stage looks for its groups in live in the other second-word array, which nobody writes before the rebucket kernel)
            s.tie_bytes = (keep && !kn.no_digit_bytes) ? reinterpret_cast<uint8_t*>(w.diet ? w.y.k2 : first_in.k2) : (uint8_t*)nullptr;
            const int rc1 = prefix_sort_1w(c, w.sc, reinterpret_cast<uint64_t*>(in1.k1), reinterpret_cast<uint64_t*>(alt1.k1),
                                           reinterpret_cast<uint64_t*>(d_sa), n, lo1, lead, r0, &s1, d_text, n, sh.tab, sh.ks, !kn.one_word_always,
                                           keep ? &s.view : nullptr, dig,
                                           (in1.k1 == w.x.k1 && onew_pad_total<T>(n)) ? ONEW_PAD : (uint64_t)0, s.tie_bytes, &s.tie_bits);
            if (rc1 == PSACX_RETRY_1STAGE) return rc1;          // (nearly every suffix ties on the prefix: one sort over both words; nothing was written)
            if (rc1 == PSACX_RETRY_1W) {          // (a repetitive text, or no room for the bucket tables: nothing was written)
                one_word = false;
                PSACX_TRY(make_first_keys<T>(c, w, d_text, n, nullptr, sh, first_in.k1, nullptr, true, lo1));
            }
            else {
                PSACX_TRY(rc1);
                s.rec.k1 = reinterpret_cast<T*>(s1); s.rec.k2 = nullptr; s.rec.v = d_sa;
                s.packed1 = true;          // (the bits of word 1 below the prefix are gone: ties read word 1 from the text)
                s.onew = keep;
            }
        }
    }
    if (!one_word)
        PSACX_TRY(pair_sort<T>(c, w.sc, in1, alt1, n, /*iota=*/true, sh.bits_w1, 0, w.diet ? (T*)nullptr : d_sa, &s.rec, r0,
                               sh.ks.spec, n, /*summary_ready=*/true, lo1, (int)lo1));
    if (w.diet && s.rec.v != d_sa)          // (a skipped pass changed the parity)
        PSACX_HIP(c, hipMemcpyAsync(d_sa, s.rec.v, n * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    return resolve_prefix_ties<T>(c, w, d_text, n, d_sa, d_isa, sh, first_in, first_alt, s);
}

// One sort over both words of the window
template <typename T>
int first_sort_one_stage(psacx_ctx* c, Work<T>& w, const uint8_t* d_text, uint64_t n, T* d_sa, const T* d_slen, const FirstShape& sh, FirstSorted<T>& s) {
    psacx_round* r0 = &c->stats.rounds[0];
    s = FirstSorted<T>();
    // In the diet layout the second record set is the output buffers (y = ISA, LCP, SA).  One stage: both sorted key
    // words must end up in the workspace set x (word 2 in the LCP buffer would be overwritten while its neighbours are
    // still being read), so an odd number of passes starts from y.
    const unsigned planned = (sh.bits_w1 + RADIX_BITS - 1) / RADIX_BITS + (sh.bits_w2 + RADIX_BITS - 1) / RADIX_BITS;
    const bool start_y = w.diet && (planned & 1u) != 0;
    SortBufs<T> first_in = start_y ? w.y : w.x, first_alt = start_y ? w.x : w.y;
    // word 2 of every record is sorted along in one stage
    PSACX_TRY(make_first_keys<T>(c, w, d_text, n, d_slen, sh, first_in.k1, first_in.k2, false, 0));

    std::memset(r0, 0, sizeof(*r0));
    PSACX_TRY(pair_sort<T>(c, w.sc, first_in, first_alt, n, /*iota=*/true, sh.bits_w1, sh.bits_w2, w.diet ? (T*)nullptr : d_sa,
                           &s.rec, r0, sh.ks.spec, n, /*summary_ready=*/true));
    if (w.diet) {
        // keys into the workspace set if a skipped pass changed the parity; SA out of the scratch payload
        if (s.rec.k1 != w.x.k1) {
            PSACX_HIP(c, hipMemcpyAsync(w.x.k1, s.rec.k1, n * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
            PSACX_HIP(c, hipMemcpyAsync(w.x.k2, s.rec.k2, n * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
            s.rec.k1 = w.x.k1; s.rec.k2 = w.x.k2;
        }
        if (s.rec.v != d_sa) PSACX_HIP(c, hipMemcpyAsync(d_sa, s.rec.v, n * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
        s.rec.v = d_sa;
    }
    return PSACX_OK;
}

// rebucket_first_kernel with the first level of the inversion fused in
template <typename T, bool WITH_LCP>
inline void launch_rebucket_first_fused(psacx_ctx* c, unsigned ntiles, const T* s1, const T* s2, const T* sa, uint64_t n, KeyShape ks,
                                        T* bsa, T* lcp, uint64_t* carry, uint64_t* nact, uint64_t* nunf, T* pyr1,
                                        uint32_t* pk, uint32_t* pv, unsigned shift, unsigned* cursors, int lazy_ids = 0) {
    // pv == nullptr: packed pairs (64-bit words: one array of (position | rank << 32) entries at pk)
    if (pv)
        hipLaunchKernelGGL((rebucket_first_kernel<T, ScanCfg<T>::BLOCK, SCAN_ITEMS, WITH_LCP, false, ISA_NARROW_CB>), dim3(ntiles),
                           dim3(ScanCfg<T>::BLOCK), 0, c->stream, s1, s2, sa, n, ks, bsa, lcp, carry, nact, nunf, n, Boundary<T>(), pyr1,
                           (unsigned*)nullptr, 0, pk, pv, shift, cursors, (T*)nullptr, lazy_ids);
    else
        hipLaunchKernelGGL((rebucket_first_kernel<T, ScanCfg<T>::BLOCK, SCAN_ITEMS, WITH_LCP, false, ISA_NARROW_CB, true>), dim3(ntiles),
                           dim3(ScanCfg<T>::BLOCK), 0, c->stream, s1, s2, sa, n, ks, bsa, lcp, carry, nact, nunf, n, Boundary<T>(), pyr1,
                           (unsigned*)nullptr, 0, pk, pv, shift, cursors, (T*)nullptr, lazy_ids);
}

// ---- LCP of the 2k-mers + new bucket ids (suffix_array.hpp:1353-1396, bucketing.hpp:57-123), the early-out hook, SA -> ISA
// (the inversion stays with the rebucket kernel because three of that kernel's launch forms decide how it runs)
// *lazy_ids: the rebucket kernel left out the ids of tiles without unresolved suffixes (filled in by run_compact if needed)
template <typename T, bool WITH_LCP>
int rebucket_first_round(psacx_ctx* c, Work<T>& w, uint64_t n, T* d_sa, T* d_isa, T* d_lcp, bool gsa, const KeyShape& ks, const FirstSorted<T>& s,
                         bool* lazy_ids) {
    const Knobs& kn = c->knobs;
    const SortBufs<T>& sorted = s.rec;
    bool isa_hist_ready = false;
    const bool fuse_l1 = !gsa && isa_narrow_levels<T>(n, kn) > 0;
    *lazy_ids = false;
    // 32-bit words, normal layout: the same fusion; the pairs use two payload scratch arrays of the sort, the second level
    // the two position lists (all idle between the sort and the first compaction)
    const bool fuse32 = sizeof(T) == 4 && !gsa && !w.diet && isa_levels32(n) > 0;
    const uint64_t ntiles = (n + ScanCfg<T>::TILE - 1) / ScanCfg<T>::TILE;
    {
        ProfScope ps(c, TC_REBUCKET);
        T* const pyr1 = (WITH_LCP && w.pyr.nlev > 1) ? w.pyr.lvl[1] : (T*)nullptr;   // level 1 comes out of the rebucket kernel
        // ... and so do the tile histograms of the inversion's first radix level when the tiles agree
        isa_hist_ready = !fuse32 && isa_radix_levels<T>(n, kn) && (uint64_t)ScanCfg<T>::TILE == (uint64_t)ScatterCfg<T>::TILE;
        unsigned* const sa_hist = isa_hist_ready ? pass_scratch(w.sc.d_desc, ntiles).tile_hist : (unsigned*)nullptr;
        if (gsa) {
            PSACX_TRY((run_carries<T, false, true>(c, w, sorted.k1, sorted.k2, nullptr, n, d_sa, ks)));
            hipLaunchKernelGGL((rebucket_first_kernel<T, ScanCfg<T>::BLOCK, SCAN_ITEMS, WITH_LCP, true>), dim3((unsigned)ntiles),
                               dim3(ScanCfg<T>::BLOCK), 0, c->stream, sorted.k1, sorted.k2, d_sa, n, ks, w.bsa, d_lcp,
                               w.d_carry, w.d_nact, w.d_nunf, n, Boundary<T>(), pyr1, sa_hist, (int)INV_WINDOW_BITS);
        } else if (fuse32) {
            PSACX_TRY((run_carries<T, false>(c, w, sorted.k1, sorted.k2, nullptr, n, d_sa, ks)));
            PSACX_HIP(c, hipMemsetAsync(w.d_cursors, 0, ((size_t)1 << ISA_NARROW_CB) * sizeof(unsigned) + sizeof(unsigned), c->stream));
            launch_rebucket_first_fused<T, WITH_LCP>(c, (unsigned)ntiles, sorted.k1, sorted.k2, d_sa, n, ks, w.bsa, d_lcp, w.d_carry, w.d_nact,
                                                     w.d_nunf, pyr1, reinterpret_cast<uint32_t*>(w.x.v), reinterpret_cast<uint32_t*>(w.y.v),
                                                     isa_narrow_shift(isa_levels32(n), 0), w.d_cursors);
        } else if (fuse_l1 && s.onew) {
            // ... on the one-word records of the prefix sort: the kernel takes word 1 and the suffixes out of them and writes the suffix array
            if constexpr (sizeof(T) == 8) {
                hipLaunchKernelGGL(last_head_1w_kernel<0>, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, c->stream, reinterpret_cast<const uint64_t*>(sorted.k1),
                                   reinterpret_cast<const uint64_t*>(s.onew_w1), reinterpret_cast<const uint64_t*>(sorted.k2), n, (unsigned)ScanCfg<T>::TILE, ntiles,
                                   w.d_carry, ks, s.view);
                PSACX_HIP(c, hipGetLastError());
                PSACX_TRY(scan_carries<T>(c, w, ntiles));
                PSACX_HIP(c, hipMemsetAsync(w.d_cursors, 0, ((size_t)1 << ISA_NARROW_CB) * sizeof(unsigned) + sizeof(unsigned), c->stream));
                *lazy_ids = n >= (1ull << 22);
                // the lean 32-bit kernel where its assumptions hold (rebucket_1w_math.hpp: rb1w_fits); PSACX_OPT_GENERIC_REBUCKET pins the generic one.
                // Its gain is its third workgroup per CU: 80 VGPRs and no scratch, which the compiler reaches only with the two opaque values of
                // rb1w_fresh (sa_kernels.hpp).  After a change of the kernel or of the compiler, look at the resource remark of the gfx950 build
                // (-Rpass-analysis=kernel-resource-usage; figures in DESIGN.md 3.3) and at the A/B of profiles/rebucket_1w_ab.txt.
                if (!kn.generic_rebucket && rb1w_fits(ks.lc, ks.c1, ks.c2, s.view.low, s.view.sfield, n)) {
                    c->stats.rebucket_1w = 1;
                    hipLaunchKernelGGL((rebucket_first_1w_kernel<RB1W_BLOCK, ScanCfg<T>::TILE / RB1W_BLOCK, WITH_LCP, ISA_NARROW_CB>), dim3((unsigned)ntiles), dim3(RB1W_BLOCK), 0,
                                       c->stream, reinterpret_cast<const uint64_t*>(sorted.k1), reinterpret_cast<const uint64_t*>(s.onew_w1),
                                       reinterpret_cast<const uint64_t*>(sorted.k2), n, s.view, rb1w_shape(ks.lc, ks.c1, ks.c2, s.view.low, s.view.sfield, n),
                                       reinterpret_cast<uint64_t*>(w.bsa), reinterpret_cast<uint64_t*>(d_lcp), w.d_carry, w.d_nact, w.d_nunf,
                                       reinterpret_cast<uint64_t*>(pyr1), reinterpret_cast<uint64_t*>(w.x.v),
                                       isa_narrow_shift(isa_narrow_levels<T>(n, kn), 0), w.d_cursors, reinterpret_cast<uint64_t*>(d_sa), *lazy_ids ? 1 : 0);
                } else
                hipLaunchKernelGGL((rebucket_first_kernel<T, RB1W_BLOCK, ScanCfg<T>::TILE / RB1W_BLOCK, WITH_LCP, false, ISA_NARROW_CB, true, true>), dim3((unsigned)ntiles),
                                   dim3(RB1W_BLOCK), 0, c->stream, sorted.k1, sorted.k2, (const T*)nullptr, n, ks, w.bsa, d_lcp, w.d_carry, w.d_nact, w.d_nunf, n,
                                   Boundary<T>(), pyr1, (unsigned*)nullptr, 0, reinterpret_cast<uint32_t*>(w.x.v), (uint32_t*)nullptr,
                                   isa_narrow_shift(isa_narrow_levels<T>(n, kn), 0), w.d_cursors, d_sa, *lazy_ids ? 1 : 0, s.view, (const T*)s.onew_w1);
            }
        } else if (fuse_l1) {
            // the first level of the SA -> ISA inversion rides along: its (position, rank) pairs go to the payload scratch
            // array of the sort, which nobody reads any more (word 1 / word 2 / SA are read from other arrays)
            PSACX_TRY((run_carries<T, false>(c, w, sorted.k1, sorted.k2, nullptr, n, d_sa, ks)));
            PSACX_HIP(c, hipMemsetAsync(w.d_cursors, 0, ((size_t)1 << ISA_NARROW_CB) * sizeof(unsigned) + sizeof(unsigned), c->stream));
            uint32_t* const pk = reinterpret_cast<uint32_t*>(w.x.v);
            *lazy_ids = n >= (1ull << 22);
            launch_rebucket_first_fused<T, WITH_LCP>(c, (unsigned)ntiles, sorted.k1, sorted.k2, d_sa, n, ks, w.bsa, d_lcp, w.d_carry, w.d_nact,
                                                     w.d_nunf, pyr1, pk, (uint32_t*)nullptr,
                                                     isa_narrow_shift(isa_narrow_levels<T>(n, kn), 0), w.d_cursors, *lazy_ids ? 1 : 0);
        } else {
            PSACX_TRY((run_carries<T, false>(c, w, sorted.k1, sorted.k2, nullptr, n, d_sa, ks)));
            hipLaunchKernelGGL((rebucket_first_kernel<T, ScanCfg<T>::BLOCK, SCAN_ITEMS, WITH_LCP>), dim3((unsigned)ntiles),
                               dim3(ScanCfg<T>::BLOCK), 0, c->stream, sorted.k1, sorted.k2, d_sa, n, ks, w.bsa, d_lcp,
                               w.d_carry, w.d_nact, w.d_nunf, n, Boundary<T>(), pyr1, sa_hist, (int)INV_WINDOW_BITS);
        }
        PSACX_HIP(c, hipGetLastError());
    }
    // (a host-pointer call starts SA and LCP on their way out from here: they are final unless refinement rounds follow)
    if (c->first_round_hook && !gsa && c->early_word) {
        hipLaunchKernelGGL(sum_counts_kernel<0>, dim3(1), dim3(1024), 0, c->stream, (const uint64_t*)w.d_nunf, ntiles, c->early_word);
        PSACX_HIP(c, hipGetLastError());
        void (*hook)(void*) = c->first_round_hook; c->first_round_hook = nullptr; hook(c->first_round_hook_arg);
    }
    // ---- SA -> ISA (bulk_permute.hpp:14-73)
    ProfScope ps(c, TC_ISA_SCATTER);
    SortBufs<T> t1 = w.x, t2 = w.y;
    if (w.diet) { t2.k1 = w.x.v; t2.k2 = d_isa; }       // the last partition level may write the values into ISA itself
    if (fuse_l1) { t1.k1 = w.x.v; t2.k1 = w.x.k1; }     // level 1 is in x.v; level 2 writes over word 1 (or its twin), dead by now
    if (fuse32)
        PSACX_TRY(finish_inversion32<T>(c, w.d_cursors, reinterpret_cast<uint32_t*>(w.x.v), reinterpret_cast<uint32_t*>(w.y.v),
                                        reinterpret_cast<uint32_t*>(w.pos_a), reinterpret_cast<uint32_t*>(w.pos_b), n, isa_levels32(n), d_isa));
    else
        PSACX_TRY(invert_permutation<T>(c, w.d_cursors, d_sa, w.bsa, n, d_isa, t1, t2, kn, 0, &w.sc, isa_hist_ready, fuse_l1));
    return PSACX_OK;
}

// The first round.  *k: the characters it sorted on (half the window); *active, *unf_b: the suffixes that still share a bucket -- their list
// is at w.pos_a when it fits the workspace -- and the buckets they share
template <typename T, bool WITH_LCP>
int first_round(psacx_ctx* c, Work<T>& w, const uint8_t* d_text, uint64_t n, uint32_t k_req, T* d_sa, T* d_isa, T* d_lcp, const T* d_slen,
                uint32_t* k, uint64_t* active, uint64_t* unf_b) {
    const bool gsa = d_slen != nullptr;
    FirstShape sh;
    PSACX_TRY(first_round_shape<T>(c, w, d_text, n, k_req, gsa, sh));
    FirstSorted<T> s = FirstSorted<T>();
    int rc = sh.two_stage ? first_sort_two_stage<T>(c, w, d_text, n, d_sa, d_isa, sh, s) : PSACX_RETRY_1STAGE;
    if (rc == PSACX_RETRY_1STAGE) rc = first_sort_one_stage<T>(c, w, d_text, n, d_sa, d_slen, sh, s);
    PSACX_TRY(rc);
    bool lazy_ids = false;
    PSACX_TRY((rebucket_first_round<T, WITH_LCP>(c, w, n, d_sa, d_isa, d_lcp, gsa, sh.ks, s, &lazy_ids)));
    if (WITH_LCP) {
        ProfScope ps(c, TC_RMQ_BUILD);
        for (int L = 2; L < w.pyr.nlev; ++L) {
            hipLaunchKernelGGL((pyramid_level_kernel<T>), dim3(grid_for(c, w.pyr.len[L] * 64, 256, 8)), dim3(256), 0,
                               c->stream, w.pyr.lvl[L - 1], w.pyr.len[L - 1], w.pyr.lvl[L], w.pyr.len[L]);
            PSACX_HIP(c, hipGetLastError());
        }
    }

    // ---- which suffixes still share a bucket (suffix_array.hpp:925-965)
    *active = 0; *unf_b = 0;
    PSACX_TRY(run_compact<T>(c, w, w.bsa, nullptr, n, w.pos_a, active, unf_b, w.cap_active, 0, nullptr, nullptr, nullptr, 0, lazy_ids, ord_array(w, n)));
    psacx_round* r0 = &c->stats.rounds[0];
    r0->h = sh.k; r0->active = n; r0->unfinished_buckets = *unf_b; r0->unfinished_elements = *active;
    c->stats.n_rounds = 1;
    *k = sh.k;
    return PSACX_OK;
}

} // namespace psacx
