/* psacx.h -- C ABI of the MI355X-native suffix-array / ISA / LCP engine.
 *
 * This is the drop-in boundary for the SA+LCP path of patflick/psac.  Each
 * entry point names the reference interface (file:line under /root/reference)
 * it stands in for.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *   - every function returns 0 on success or a negative PSACX_E* code;
 *     psacx_strerror() turns a code into text.  Nothing throws across the ABI
 *     (the reference throws std::runtime_error, suffix_array.hpp:226-227; the
 *     C++ mirror in include/suffix_array.hpp re-throws from these codes).
 *   - a psacx_ctx owns one HIP device, one stream and a reusable HBM
 *     workspace.  It is not re-entrant; use one ctx per host thread / per GPU.
 *   - "_dev" entry points take DEVICE pointers (text resident in HBM, results
 *     left in HBM); the plain ones take HOST pointers and stage over PCIe.
 *   - index type: _u32 needs n <= 2^32 - 2 (idxsort.hpp:39), _u64 needs n < 2^62.
 */
#ifndef PSACX_H
#define PSACX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct psacx_ctx psacx_ctx;

enum {
    PSACX_OK = 0,
    PSACX_EINVAL = -1,     /* bad argument (null pointer, n == 0, k too large ...) */
    PSACX_ERANGE = -2,     /* n does not fit the index type */
    PSACX_ENOMEM = -3,     /* HBM workspace allocation failed */
    PSACX_EHIP = -4,       /* a HIP runtime call failed (psacx_last_hip_error) */
    PSACX_EDEVICE = -5,    /* a kernel reported an internal error (look-back timeout) */
    PSACX_ENOGPU = -6      /* no usable HIP device */
};

/* flags for psacx_construct_* */
enum {
    PSACX_LCP = 1u,        /* also build the LCP array (template flag _CONSTRUCT_LCP,
                              suffix_array.hpp:170) */
    PSACX_NO_FAST = 2u,    /* fast_resolval = false (suffix_array.hpp:470): keep sorting
                              every suffix each round instead of only unresolved buckets */
    PSACX_PROFILE = 4u     /* bracket every kernel class with HIP events (psacx_get_stats) */
};

#define PSACX_MAX_ROUNDS 72

typedef struct psacx_round {
    uint64_t h;                    /* prefix length already sorted when the round started */
    uint64_t active;               /* suffixes that took part in this round's sort */
    uint64_t unfinished_buckets;   /* as printed by suffix_array.hpp:416 / :961 */
    uint64_t unfinished_elements;
    uint32_t sort_passes;          /* radix passes executed */
    uint32_t sort_passes_skipped;  /* digits found constant by the histogram */
} psacx_round;

typedef struct psacx_stats {
    uint32_t sigma;                /* alphabet.hpp:147-155 */
    uint32_t bits_per_char;        /* alphabet.hpp:154 */
    uint32_t k;                    /* kmer.hpp:26-40 */
    uint32_t n_rounds;
    psacx_round rounds[PSACX_MAX_ROUNDS];
    /* event timers, milliseconds, filled when PSACX_PROFILE was set */
    double ms_total;               /* whole construct call, device side */
    double ms_alphabet, ms_kmer, ms_sort_hist, ms_sort_scatter, ms_rebucket, ms_isa_scatter,
           ms_gather, ms_compact, ms_rmq_build, ms_finalize;
    /* the radix scatter-pass kernel, counted per form: [0] = single-sweep look-back form
       (radix_scatter_kernel, small inputs), [1] = three-kernel form (radix_scatter3_kernel,
       large inputs; ms_sort_scatter3 times only that kernel, its per-tile histogram and
       offset scans are in ms_sort_tilehist), [2] = three-kernel form over two-word records
       (B1, idx): the prefix sort that opens the first round (ms_sort_scatter2) */
    double ms_sort_scatter3, ms_sort_tilehist, ms_sort_scatter2;
    uint64_t scatter_launches[3];  /* kernels launched */
    uint64_t scatter_records[3];   /* records moved by them (sum over launches) */
    uint64_t scatter_bytes[3];     /* algorithmic bytes: read + write of the record, 2 * 3w ([2]: 2 * 2w) per record */
    uint64_t hist_bytes;           /* algorithmic bytes of the histogram kernels: 2w per record */
    uint64_t workspace_bytes;      /* HBM held by the ctx */
    uint64_t onew_passes;          /* bucket passes run over one-word records (the MSD-first prefix sort of the first round); 0: that sort ran
                                      in the two-array form, whose passes are counted in scatter_*[2] alone */
    uint64_t heavy_rounds;         /* refinement rounds (or slabs of one) whose records were split into heavy and light ones (psac_amd/csrc/heavy_keys.hpp) */
    uint64_t heavy_records;        /* ... records that carried their bucket's heavy rank and skipped the sort */
    uint64_t light_records;        /* ... records that were sorted */
    uint64_t level_gathers;        /* refinement rounds (or slabs) whose ranks h further came through partition levels (construct.hpp: gather_by_levels) */
    /* host-pointer calls (psacx_construct_u32 / _u64), host wall clock, milliseconds: [0] text to the device, [1] the construction,
       [2] what was left of SA and LCP on their early way out when the construction returned (below), [3] ISA (and SA, LCP if they did not
       leave early) into the caller's arrays, [4] Lc, [5] the call; SA and LCP leaving early (from the end of the first round):
       [6] when that began, [7] = [8] when both were through, since the call began */
    double ms_host[9];
    /* psacx_locate_dev_* with PSACX_OPT_LOCATE_COUNT set, last call: [0] SA entries fetched, [1] text words fetched (8 bytes or less each, counted per load in either kernel shape);
       a bisection step is one of the first and at least one of the second, each waiting for the one before it.  0 without the option. */
    uint64_t locate_fetches[2];
    uint64_t rebucket_1w;          /* 1 when the first round of the last construction ran rebucket_first_1w_kernel, the 32-bit form of the rebucket kernel on
                                      one-word records, 0 when it ran the generic rebucket_first_kernel */
    uint64_t group_sort;           /* the one-word prefix sort of the last construction: 0 = LSD passes on every digit inside the 256 buckets, 1 = upper digits most
                                      significant first and the groups of the last 16 prefix bits sorted on chip, 2 = that form entered, a group longer
                                      than its cap found, the remaining digits sorted LSD inside the partition reached */
    uint64_t tie_form;             /* the side stream the tie stage of the last construction's one-word first round looked for its groups in: 0 = none (it compared
                                      the records, or the first round did not keep one-word records), 1 = a tie byte per record, 2 = the tie bits of the group sort
                                      (PSACX_OPT_PLAIN_SIDE_KERNELS = 2 pins the bytes) */
    uint64_t grid_cuts;            /* launches of grid-stride kernels since the context was created whose grid came out smaller than the workgroups their items
                                      asked for, by the default bound of a few workgroups per CU or by PSACX_OPT_GRID_CAP: some workgroup of such a launch takes a
                                      second trip through its loop.  Never cleared; filled by psacx_get_stats. */
} psacx_stats;

/* life cycle ------------------------------------------------------------- */

/* Replaces suffix_array(const mxx::comm&) (suffix_array.hpp:174): binds the
 * engine to HIP device `device` (>= 0).  `stream` may be NULL (the ctx makes
 * its own), an existing hipStream_t passed as void*, or PSACX_STREAM_DEFAULT for
 * the device's default (null) stream, e.g. when sharing PyTorch's current stream. */
#define PSACX_STREAM_DEFAULT ((void*)(intptr_t)-1)
int psacx_create(psacx_ctx** out, int device, void* stream);
void psacx_destroy(psacx_ctx* ctx);
const char* psacx_strerror(int code);
/* text of the last HIP error seen by this ctx ("" if none) */
const char* psacx_last_hip_error(const psacx_ctx* ctx);
/* release the cached HBM workspace and the host-side staging of the host-pointer path: pinned ring, widening threads (all re-made on the next call that needs them) */
int psacx_trim(psacx_ctx* ctx);

/* Options of a context.  Every stage of the construction has one or more forms; the engine picks by text size, free
 * HBM and what it finds in the text.  An option pins the choice of one stage -- for the parity suite, which runs every form, and for A/B
 * timings.  None changes SA / ISA / LCP.  Values: 0 = the engine decides (default), 1 = on, or as listed.  An option stays set until it
 * is set again; psacx_configure(ctx, PSACX_OPT_RESET, 0) restores all defaults.  (The reference has no counterpart: its forms are
 * template parameters and #defines, e.g. suffix_array.hpp:170, :470.)
 *   FORCE_DIET        reduced-memory layout although the normal one fits
 *   DIET_CAP          at most this many records of room for the refinement rounds of the reduced layout (0 = what fits)
 *   ONE_STAGE         first round as one sort over both key words
 *   TIES_RADIX        ties of the two-stage first round through compaction + radix sort
 *   NO_ONE_WORD       the prefix sort of the first round in (word 1, suffix) passes, not one-word records
 *   ONE_WORD_ALWAYS   no repetition probe before the one-word prefix sort
 *   ONE_WORD_MIN      log2 of the smallest text that takes the one-word form (0 = 24)
 *   WIDEN_LAST        the last pass of the one-word prefix sort writes two arrays
 *   NO_DIGIT_BYTES    tile histograms of the bucket passes from the records
 *   NO_BUCKET_SORT    refinement rounds never sort inside LDS
 *   ISA_UPDATE        1 = one store per record, 2 = partition levels
 *   GATHER            ranks h further of a refinement round: 1 = one fetch per record, 2 = partition levels
 *   NO_HEAVY          no split of a round's records into heavy and light ones
 *   NO_WHOLE          no text-order rounds
 *   NO_LAZY_RANKS     the heavy runs of a split round always take the rank of their head and store it
 *   NO_EARLY_OUT      host-pointer calls: SA and LCP leave the device only when the construction has returned (default: from the moment the
 *                     first round has written them, under the SA -> ISA inversion; copied again if refinement rounds follow)
 *   NO_SPREAD_CURSORS the partition levels of the SA -> ISA path run their tiles in order (default: striped over several destination classes,
 *                     so that the workgroups running together do not all reserve and write inside one of them)
 *   LOCATE_SHAPE      psacx_locate_*: 1 = one pattern per lane (the default), 2 = eight lanes per pattern, 64 characters per step (A/B runs);
 *                     no effect on psacx_locate_gsa_*, which has the first shape only
 *   LOCATE_COUNT      psacx_locate_*: the kernel counts its fetches into psacx_stats.locate_fetches (slower; tools/locate_time.py)
 *   GENERIC_REBUCKET  the first round on one-word records runs the generic rebucket kernel, not its 32-bit form (A/B runs)
 *   PLAIN_SIDE_KERNELS the tile histograms of the top digit and the tie scan of the one-word first round run their one-tile-per-workgroup
 *                     kernels (top_digit_hist_kernel, tie_resolve_1w_kernel), not the persistent ones (parity tests, A/B runs)
 *                     2 = TIE_BYTES: the persistent kernels, but the group form of the prefix sort leaves a tie byte per record and the tie scan reads
 *                     those, not the tie bits (psacx_stats.tie_form; parity tests, A/B runs; PSACX_TIE_BYTES in the debug shim); larger values are refused
 *   LSD_BUCKET_PASSES the one-word prefix sort of the first round sorts every digit below the top one by LSD passes inside the 256 buckets, not the
 *                     upper digits most significant first and the last 16 bits on chip (psacx_stats.group_sort; parity tests, A/B runs)
 *   GROUP_COUNTING_ROUNDS the group form orders the last 16 prefix bits of every batch by two or three stable counting rounds, not by one round and the
 *                     ranks inside its buckets (radix.hpp: group_sort16_kernel; the records it leaves are the same; parity tests, A/B runs)
 *   FIRST_LEAD        test option: leading bits the two-stage first round sorts on; honoured when a multiple of 8, at least bits(n - 1) + 3, at most 40
 *                     and at most the bits of the first key word, ignored otherwise (40 reaches the sub-bucket passes on small texts)
 *   LZ_SMALL_TILES    test option: psacx_lz77_dev_* parses on tiles of 64 positions in groups of 4 tiles, not 1024 in groups of 128, so that every
 *                     level of the parse, the walk over the groups included, is taken at a few hundred positions; the parse is the same
 *   GRID_CAP          test option: 1..65535 = every grid-stride kernel is launched on at most this many workgroups, not on the default bound of a few
 *                     workgroups per CU, so that the second and later trips of its loop are taken at a few thousand items (psacx_stats.grid_cuts counts
 *                     the launches that were cut); 0 = the default bound; larger values are refused; no result changes
 *   MEMS_STOP         timing option (tools/mems_time.py): 1..3 = psacx_mems_dev_* without PSACX_MEMS_SUPER returns PSACX_OK with z = 0 after its
 *                     counting walk and the two scans (1), after the writing walk (2), after the marks (3), synchronised; work is set as usual; the
 *                     differences of the times are the times of the stages.  0 = the whole call; larger values are refused
 *   KMISMATCH_STOP    timing option (tools/kmismatch_time.py): 1..2 = psacx_kmismatch_dev_* returns PSACX_OK with z = 0 after the piece searches
 *                     and the scan of their counts (1), after the marks (2), synchronised; work is set as far as it is known; the count query is
 *                     the stage after them.  0 = the whole call; larger values are refused
 *   KEDIT_STOP        timing option (tools/kedit_time.py): 1..3 = psacx_kedit_dev_* returns PSACX_OK with z = 0 after the piece searches and
 *                     the scan of their counts (1), after the verification and the scan of the raw hits (2), after the sort and the unique
 *                     (3), synchronised; work is set as far as it is known.  0 = the whole call; larger values are refused                     */
enum {
    PSACX_OPT_RESET = 0, PSACX_OPT_FORCE_DIET, PSACX_OPT_DIET_CAP, PSACX_OPT_ONE_STAGE, PSACX_OPT_TIES_RADIX, PSACX_OPT_NO_ONE_WORD,
    PSACX_OPT_ONE_WORD_ALWAYS, PSACX_OPT_ONE_WORD_MIN, PSACX_OPT_WIDEN_LAST, PSACX_OPT_NO_DIGIT_BYTES, PSACX_OPT_NO_BUCKET_SORT,
    PSACX_OPT_ISA_UPDATE, PSACX_OPT_GATHER, PSACX_OPT_NO_HEAVY, PSACX_OPT_NO_WHOLE, PSACX_OPT_NO_LAZY_RANKS, PSACX_OPT_NO_EARLY_OUT,
    PSACX_OPT_NO_SPREAD_CURSORS, PSACX_OPT_LOCATE_SHAPE, PSACX_OPT_LOCATE_COUNT, PSACX_OPT_GENERIC_REBUCKET,
    PSACX_OPT_PLAIN_SIDE_KERNELS, PSACX_OPT_LSD_BUCKET_PASSES, PSACX_OPT_FIRST_LEAD, PSACX_OPT_LZ_SMALL_TILES,
    PSACX_OPT_GRID_CAP, PSACX_OPT_GROUP_COUNTING_ROUNDS, PSACX_OPT_MEMS_STOP, PSACX_OPT_KMISMATCH_STOP,
    PSACX_OPT_KEDIT_STOP,
    PSACX_OPT_COUNT
};
int psacx_configure(psacx_ctx* ctx, int option, uint64_t value);
/* Debug shim, the ONLY place where the library looks at the environment, and only when called: resets the options of ctx and sets those
 * named by PSACX_<OPTION> variables (PSACX_FORCE_DIET=1, PSACX_DIET_CAP=<records>, PSACX_ISA_UPDATE=stores|levels, PSACX_GATHER=fetch|levels, ...).
 * The Python tests call it before every construction (psac_amd.ENV_KNOBS); products call psacx_configure. */
int psacx_configure_from_env(psacx_ctx* ctx);
/* value of environment variable `name` as the shim sees it (NULL if unset): shared with psacx_multi_configure_from_env */
const char* psacx_debug_env(const char* name);

/* construction ------------------------------------------------------------
 * Replace suffix_array<char,index_t,LCP>::construct(begin, end, fast_resolval, k)
 * (suffix_array.hpp:469-486 -> :365-466) for one rank holding the whole text.
 *   text  n bytes (any byte values; the alphabet is detected, alphabet.hpp:213-218)
 *   k     0 = auto (kmer.hpp:26-40), else upper bound on the k-mer length
 *   SA    out, n entries: local_SA        (suffix_array.hpp:204)
 *   ISA   out, n entries: local_B, 0-based inverse SA (suffix_array.hpp:206, :460-464)
 *   LCP   out, n entries or NULL: local_LCP (suffix_array.hpp:209); LCP[0] = 0
 */
int psacx_construct_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t k,
                        uint32_t flags, uint32_t* SA, uint32_t* ISA, uint32_t* LCP);
int psacx_construct_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t k,
                        uint32_t flags, uint64_t* SA, uint64_t* ISA, uint64_t* LCP);
int psacx_construct_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, uint32_t k,
                            uint32_t flags, uint32_t* d_SA, uint32_t* d_ISA, uint32_t* d_LCP);
int psacx_construct_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, uint32_t k,
                            uint32_t flags, uint64_t* d_SA, uint64_t* d_ISA, uint64_t* d_LCP);

/* suffix_array<char_t, index_t, true, true>::construct (suffix_array.hpp:170, :469-486): SA, ISA
 * and LCP as above (PSACX_LCP is implied) plus the left-branching characters local_Lc
 * (suffix_array.hpp:211-212; built at :1365-1383 and par_rmq.hpp:334-481; consumed by
 * desa.hpp:408, tldt.hpp:437):
 *   Lc    out, n bytes: Lc[i] = text[SA[i-1] + LCP[i]], 0 when that position is past the end
 *         (alphabet.hpp:168 decodes the end marker to '\0') and for i = 0.
 */
int psacx_construct_lc_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t k, uint32_t flags,
                           uint32_t* SA, uint32_t* ISA, uint32_t* LCP, uint8_t* Lc);
int psacx_construct_lc_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, uint32_t k, uint32_t flags,
                           uint64_t* SA, uint64_t* ISA, uint64_t* LCP, uint8_t* Lc);
int psacx_construct_lc_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, uint32_t k, uint32_t flags,
                               uint32_t* d_SA, uint32_t* d_ISA, uint32_t* d_LCP, uint8_t* d_Lc);
int psacx_construct_lc_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, uint32_t k, uint32_t flags,
                               uint64_t* d_SA, uint64_t* d_ISA, uint64_t* d_LCP, uint8_t* d_Lc);

/* Generalized suffix array of a set of strings: suffix_array<>::construct_ss(simple_dstringset&,
 * alphabet) (suffix_array.hpp:267-363; string set stringset.hpp:33-81; k-mers kmer.hpp:269-355; shifts
 * shifting.hpp:374-418; bucket rules bucketing.hpp:130-143; tests test/test_gsa.cpp).
 *   text     the m strings back to back WITHOUT separators, n bytes in total
 *   offsets  m + 1 ascending offsets, offsets[0] = 0, offsets[m] = n, no empty string
 *   SA       every suffix of every string, positions counted in `text`; a suffix ends with its
 *            string, an end sorts below every character, equal suffixes come in text order
 *   ISA      inverse of SA;  LCP (with PSACX_LCP): common prefix inside the strings
 */
int psacx_construct_gsa_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m,
                            uint32_t k, uint32_t flags, uint32_t* SA, uint32_t* ISA, uint32_t* LCP);
int psacx_construct_gsa_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m,
                            uint32_t k, uint32_t flags, uint64_t* SA, uint64_t* ISA, uint64_t* LCP);
int psacx_construct_gsa_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                                uint32_t k, uint32_t flags, uint32_t* d_SA, uint32_t* d_ISA, uint32_t* d_LCP);
int psacx_construct_gsa_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                                uint32_t k, uint32_t flags, uint64_t* d_SA, uint64_t* d_ISA, uint64_t* d_LCP);

/* psacx_profile(ctx, 1): zero the statistics and let the step-level ops of psacx_ops.h add their
 * radix-pass event times and byte counts to them (psacx_get_stats reads the running totals);
 * psacx_profile(ctx, 0) stops it. */
int psacx_profile(psacx_ctx* ctx, int on);

/* statistics of the last construct call on this ctx (iteration log of
 * suffix_array.hpp:416, section timers of suffix_array.hpp:52-63) */
int psacx_get_stats(const psacx_ctx* ctx, psacx_stats* out);

/* verification on the device ---------------------------------------------------
 * Replaces check_SA / check_lcp / d_check_sa (check_suffix_array.hpp:56-88, :106-126, :207-267)
 * for buffers resident in HBM.  errors[0] = SA entries out of range or ISA[SA[i]] != i,
 * errors[1] = suffix-order violations, errors[2] = LCP entries that differ from a direct
 * character comparison (d_LCP may be NULL), errors[3] = LCP[0] != 0.  All zero = correct.
 * The LCP check costs sum(LCP) character reads: use it on texts without long repeats.
 * How entries are counted (tests/checker_model.py states the same rules on the host):
 *  - an entry i with SA[i] >= n or ISA[SA[i]] != i counts in errors[0] and is examined no further;
 *  - entry 0 is only asked for LCP[0] == 0; an entry i > 0 is compared with its predecessor only if
 *    SA[i-1] < n (a predecessor out of range is counted at its own entry);
 *  - order, with a = SA[i-1], b = SA[i]: fine iff S[a] < S[b], or S[a] == S[b] and (a + 1 == n, or
 *    b + 1 < n and ISA[a+1] < ISA[b+1]); ISA values are only compared, never used as indices;
 *  - LCP[i] is compared with the characters the two suffixes share whether or not the order test
 *    passed, so one wrong LCP entry counts once. */
int psacx_check_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_SA,
                        const uint32_t* d_ISA, const uint32_t* d_LCP, uint64_t errors[4]);
int psacx_check_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_SA,
                        const uint64_t* d_ISA, const uint64_t* d_LCP, uint64_t errors[4]);

/* The same for a generalized suffix array (psacx_construct_gsa_*): d_text holds the m strings back to back without separators,
 * d_offsets (device memory) their m + 1 offsets as psacx_construct_gsa_dev_* takes them.  The reference's counterpart is
 * gl_check_gsa (src/gsac.cpp:85-135), which gathers the arrays on rank 0, compares with libdivsufsort and tolerates swapped equal
 * suffixes; this is the scalable form (check_suffix_array.hpp:207-267) for string sets, and it pins the order of equal suffixes
 * as the engine builds them (text order).  Offsets that do not start at 0, do not end at n, hold an empty string or do not ascend
 * return PSACX_EINVAL before anything else is read.  Beside the 4 KiB slab of the ctx the call allocates a bitmap of n + 1 bits
 * ("a string starts here / end of text") for the time of the call; no array of n index words.
 * The counting rules are those of psacx_check_dev_* with "end of text" replaced by "end of the suffix's string"; end(p) is the
 * offset at which the string holding position p ends:
 *  - errors[0]: SA[i] >= n or ISA[SA[i]] != i; such an entry is examined no further;
 *  - errors[3]: LCP[0] != 0;
 *  - an entry i > 0 that passed is compared with its predecessor only if SA[i-1] < n;
 *  - errors[1], with a = SA[i-1], b = SA[i]: the entry is fine iff S[a] < S[b], or S[a] == S[b] and one of: a + 1 == end(a) and
 *    b + 1 == end(b) and a < b (equal suffixes in text order); a + 1 == end(a) and b + 1 < end(b); neither suffix ends after one
 *    character and ISA[a+1] < ISA[b+1].  (a + 1 < end(a) with b + 1 == end(b) is wrong.)  ISA values are only compared, never used
 *    as indices;
 *  - errors[2]: LCP[i] != the number of characters the two suffixes share before either string ends, counted whether or not the
 *    order test passed (sum(LCP) character reads).
 * With m = 1 the verdict on correct arrays equals psacx_check_dev_*'s; on corrupt arrays it may differ, because a one-character
 * suffix that appears twice in a row now fails the a < b rule. */
int psacx_check_gsa_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                            const uint32_t* d_SA, const uint32_t* d_ISA, const uint32_t* d_LCP, uint64_t errors[4]);
int psacx_check_gsa_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                            const uint64_t* d_SA, const uint64_t* d_ISA, const uint64_t* d_LCP, uint64_t errors[4]);

/* benchmark inputs ----------------------------------------------------------------
 * psacx_rand_dna: the reference's generator rand_dna(size, seed) (alphabet.hpp:32-45, used by psac -r,
 * src/psac.cpp:89-93): srand(1337 * seed), then "ACGT"[rand() % 4] per character (glibc rand; host memory).
 * psacx_synth_text_dev: the synthetic texts of the benchmark configurations written straight
 * into HBM: characters first .. first + n of kind 0 = DNA(seed), 1 = ASCII128(seed) (splitmix64 streams, the same
 * definition as tests/inputs.py), 2 = TANDEM: DNA(seed) repeated with `period`, 3 = MUTATED: that repeat with one position in
 * 200 replaced (long shared prefixes that end somewhere: the repeated reads of a sequencing run, the human genome of pbs_run.sh:36). */
int psacx_rand_dna(uint8_t* out, uint64_t n, int seed);
int psacx_synth_text_dev(psacx_ctx* ctx, uint8_t* d_text, uint64_t n, uint64_t first, int kind, uint64_t seed,
                         uint64_t period);

/* the rank-pair sort on its own -------------------------------------------
 * Replaces idxsort_vectors(vec1, vec2, comm) (idxsort.hpp:23-83) at one rank:
 * sorts records (b1[i], b2[i], i) by (b1, b2); on return b1/b2 hold the sorted
 * keys and idx the permutation.  Device pointers, n entries each.  key_bits =
 * number of significant low bits in each key word (0, or more than the word has = all);
 * the keys must be zero above them (a pass takes a whole 8-bit digit).  The sort is
 * stable: equal pairs keep index order.
 * psacx_get_stats then reports in rounds[0] the radix passes run (sort_passes) and the
 * 8-bit digits of the key_bits found constant and skipped (sort_passes_skipped). */
int psacx_pair_sort_dev_u32(psacx_ctx* ctx, uint32_t* d_b1, uint32_t* d_b2, uint32_t* d_idx,
                            uint64_t n, uint32_t key_bits);
int psacx_pair_sort_dev_u64(psacx_ctx* ctx, uint64_t* d_b1, uint64_t* d_b2, uint64_t* d_idx,
                            uint64_t n, uint32_t key_bits);

/* all nearest smaller values ----------------------------------------------
 * Replaces ansv<T,left_type,right_type,global_indexing>(in, left, right, comm)
 * (ansv.hpp:2042-2051) at one rank.  type: 0 nearest_sm, 1 nearest_eq,
 * 2 furthest_eq (ansv_common.hpp:20-22).  Results are global indices, `nonsv`
 * where no such element exists.  Any value of T is a legal input, its largest included,
 * and any 64-bit word a legal nonsv.  Host pointers. */
int psacx_ansv_u32(psacx_ctx* ctx, const uint32_t* in, uint64_t n, int left_type, int right_type,
                   uint64_t nonsv, uint64_t* left_nsv, uint64_t* right_nsv);
int psacx_ansv_u64(psacx_ctx* ctx, const uint64_t* in, uint64_t n, int left_type, int right_type,
                   uint64_t nonsv, uint64_t* left_nsv, uint64_t* right_nsv);
/* same with the input (e.g. the LCP array psacx_construct_dev_* left in HBM) and both results in device memory */
int psacx_ansv_dev_u32(psacx_ctx* ctx, const uint32_t* d_in, uint64_t n, int left_type, int right_type,
                       uint64_t nonsv, uint64_t* d_left_nsv, uint64_t* d_right_nsv);
int psacx_ansv_dev_u64(psacx_ctx* ctx, const uint64_t* d_in, uint64_t n, int left_type, int right_type,
                       uint64_t nonsv, uint64_t* d_left_nsv, uint64_t* d_right_nsv);

/* suffix tree topology -------------------------------------------------------
 * Replaces construct_suffix_tree(sa, begin, end, comm) (suffix_tree.hpp:413-499, parents by
 * for_each_parent :43-223) at one rank.  nodes: n x (sigma + 1) table, row i = internal node of LCP
 * index i, cell c = child through the character with alphabet code c (0 = end of text), leaves are
 * n + i, 0 = no child.  Host pointers.  Call with nodes == NULL first to learn sigma. */
int psacx_suffix_tree_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint32_t* SA,
                          const uint32_t* LCP, uint64_t* nodes, uint32_t* sigma);
int psacx_suffix_tree_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* SA,
                          const uint64_t* LCP, uint64_t* nodes, uint32_t* sigma);
/* The same with every array resident in HBM (the arrays psacx_construct_dev_* left there): d_nodes receives the
 * n x (sigma + 1) table, which never visits the host; no input is written.  d_nodes == NULL: only *sigma is computed
 * (d_SA / d_LCP may be NULL then).  The alphabet comes from a histogram taken on the device.  edges (may be NULL)
 * receives the number of records written = nonzero cells = n + internal nodes, counted by the kernel that writes them.
 * d_LCP[0] is expected to be 0, as psacx_construct_dev_* stores it.  Another value there never serves as an index or as a depth: a
 * search that finds nothing, or finds entry 0, means parent 0 at depth 0; the table is that of LCP[0] = 0 provided the stored value
 * equals no other entry. */
int psacx_suffix_tree_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_SA,
                              const uint32_t* d_LCP, uint64_t* d_nodes, uint32_t* sigma, uint64_t* edges);
int psacx_suffix_tree_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_SA,
                              const uint64_t* d_LCP, uint64_t* d_nodes, uint32_t* sigma, uint64_t* edges);

/* Is d_nodes the node table of the text / SA / LCP as given?  (The reference's check_suffix_tree.hpp is a sequential
 * host walk; this one runs in HBM.)  SA and LCP themselves are NOT verified here: that is psacx_check_dev_*'s job, and
 * a table is "correct" relative to whatever arrays it is handed.  It shares no code and no intermediate array with the
 * builder (no ANSV): the table is restated as follows.  L = LCP with L[0] read as 0 whatever is stored, row = sigma + 1,
 * code() = alphabet code (1..sigma in byte order of the characters of d_text).
 *   head(x)    = the smallest j <= x with L[j] == L[x] and min(L[j..x]) == L[x];
 *   cell(s, d) = code(text[s + d]) if s < n and d < n - s, else 0 (no wrapping, no out-of-range read);
 *   leaf record of every i in [0, n): x = i + 1 if i + 1 < n and L[i+1] > L[i], else x = i; id n + i in cell
 *     (head(x), cell(SA[i], L[x]));
 *   internal record of every i >= 1 with L[i] > 0 and head(i) == i: l / r = the nearest j < i / j > i with L[j] < L[i]
 *     (r may not exist); (p, d) = (r, L[r]) if r exists and L[r] > L[l], else (head(l), L[l]); id i in cell
 *     (p, cell(SA[i], d)).
 * The correct table holds every record's id in its cell and 0 everywhere else.  Counting rules, total for any input:
 *  - out[2] = records (leaf + internal) of the arrays as given; out[3] = nonzero cells of the table;
 *  - a record is matched iff the cell it names holds its id (each record on its own, even if corrupt inputs send two
 *    records to one cell);
 *  - out[0] = records not matched; out[1] = out[3] - matched records = nonzero cells no record accounts for (never
 *    negative: ids are distinct and nonzero);
 *  - correct <=> out[0] == out[1] == 0.
 * Table values are only compared, never used as indices.  Workspace: the ctx slab (a min-pyramid over LCP, n / 63 words). */
int psacx_check_suffix_tree_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_SA,
                                    const uint32_t* d_LCP, const uint64_t* d_nodes, uint64_t out[4]);
int psacx_check_suffix_tree_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_SA,
                                    const uint64_t* d_LCP, const uint64_t* d_nodes, uint64_t out[4]);

/* The suffix tree of a string set (construct_gst with gst_edgechars, suffix_tree.hpp:501-608, one rank) from the arrays
 * psacx_construct_gsa_* leaves: text[0..n) holds the m strings back to back, offsets[0..m] ascend with offsets[0] = 0,
 * offsets[m] = n and no empty string (anything else: PSACX_EINVAL before any other array is read).  One row of sigma + 2 cells per
 * LCP index: cells 0 and 1 hold the first and the last $-leaf (a suffix whose string ends at the node's depth), cell c + 1 the
 * child through the character with alphabet code c; leaves are numbered n + i, 0 = none.  Two things differ from the reference,
 * whose code for this is never called: the root's edges are stored (it collects them and drops them), and a suffix that starts a
 * string hangs under the root by its first character (its test for "string begins here" would take it for an ended one).
 * Defined as the one-string table above is: L = LCP with L[0] read as 0 whatever is stored, head(), l, r and code() as there,
 * row = sigma + 2, start[p] = a string starts at p, or p == n.
 *   gcell(s, d) = 0 (the $) if s >= n, or d >= n - s, or (d > 0 and start[s + d]); else code(text[s + d]) (no out-of-range read);
 *   leaf record of every i in [0, n): x = i + 1 if i + 1 < n and L[i+1] > L[i], else x = i; id n + i, row head(x),
 *     c = gcell(SA[i], L[x]);
 *   internal record of every i >= 1 with L[i] > 0 and head(i) == i: (p, d) = (r, L[r]) if r exists and L[r] > L[l], else
 *     (head(l), L[l]); id i, row p, c = gcell(SA[i], d);
 *   a record with c >= 1 puts its id in cell (row, 1 + c); the records of a row with c == 0 put their smallest id in cell (row, 0)
 *   and their largest in cell (row, 1); every other cell is 0.
 * On a correct generalized suffix array the c == 0 records of a row are leaves only, neighbours in SA (the equal suffixes, first in
 * the node's interval), and row 0 has none; with m = 1, columns 2.. are columns 1.. of the one-string table and columns 0 and 1
 * both its column 0.
 * psacx_suffix_tree_gsa_dev_*: everything resident in HBM, no input written; d_nodes == NULL only computes *sigma (d_offsets, d_SA
 * and d_LCP may be NULL then); edges (may be NULL) receives the number of records written, leaf + internal, counted by the kernel
 * that writes them.  The $ cells are written without atomics: a $-leaf i at depth d writes cell 0 iff i == 0 or not (L[i] == d
 * and the suffix at SA[i-1] ends d characters on), and cell 1 iff i == n - 1 or not (L[i+1] == d and the suffix at SA[i+1] ends
 * d characters on).  On arrays that are no generalized suffix array nothing is read or written out of range (SA >= n and
 * SA + d >= n are turned away before the bitmap and the text are touched; parents are LCP indices), and the $ cells of a row hold
 * ids of $ records of that row, not necessarily the extremes.  The stored LCP[0] is never used as a value: where it is not 0
 * the call works on a copy of LCP.  Workspace: the ctx slab (the ANSV of LCP, 16 n bytes, and the bitmap of n + 1 bits).
 * psacx_suffix_tree_gsa_*: the host-pointer form, nodes[n x (sigma + 2)]; nodes == NULL only computes *sigma. */
int psacx_suffix_tree_gsa_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m,
                              const uint32_t* SA, const uint32_t* LCP, uint64_t* nodes, uint32_t* sigma);
int psacx_suffix_tree_gsa_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m,
                              const uint64_t* SA, const uint64_t* LCP, uint64_t* nodes, uint32_t* sigma);
int psacx_suffix_tree_gsa_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                                  const uint32_t* d_SA, const uint32_t* d_LCP, uint64_t* d_nodes, uint32_t* sigma, uint64_t* edges);
int psacx_suffix_tree_gsa_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                                  const uint64_t* d_SA, const uint64_t* d_LCP, uint64_t* d_nodes, uint32_t* sigma, uint64_t* edges);
/* Is d_nodes that table for the text / offsets / SA / LCP as given?  As psacx_check_suffix_tree_dev_*: the same searches, no ANSV,
 * no code of the builder's; malformed offsets return PSACX_EINVAL.  Counting rules, total for any SA, LCP and table:
 *  - out[2] = records of the arrays as given; out[3] = nonzero cells of the table;
 *  - a record with c >= 1 is matched iff cell (row, 1 + c) holds its id;
 *  - a record with c == 0 and id v is matched iff lo != 0 and lo <= v <= hi, lo and hi being cells (row, 0) and (row, 1); it is then
 *    also a witness of lo if v == lo and of hi if v == hi (a single $-leaf witnesses both);
 *  - out[0] = records not matched; out[1] = out[3] - matched records with c >= 1 - witnesses (never negative: ids are distinct
 *    and a record witnesses only its own row);
 *  - correct <=> out[0] == out[1] == 0.
 * Table values are only compared, never used as indices. */
int psacx_check_suffix_tree_gsa_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                                        const uint32_t* d_SA, const uint32_t* d_LCP, const uint64_t* d_nodes, uint64_t out[4]);
int psacx_check_suffix_tree_gsa_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                                        const uint64_t* d_SA, const uint64_t* d_LCP, const uint64_t* d_nodes, uint64_t out[4]);

/* pattern search ------------------------------------------------------------------
 * Replaces sa_index::locate (seq_query.hpp:246-251) and the top-level lookup table lookup_index (lookup_table.hpp:36-149) for a
 * text and its suffix array resident in HBM; desa-main -f ... -c -q ... (src/desa_main.cpp) is the reference's tool on top of them.
 * One GPU.  The Lc-guided search of desa.hpp exists to avoid remote text reads and belongs with a distributed index.
 *
 * Definitions.  Text S[0..n), bytes compared as unsigned values.  Suffix i is S[i..n).  A pattern P has m >= 0 bytes.  Order is
 * lexicographic, and a proper prefix is smaller.
 *
 *     lb(P) = #{ i : S[i..n) < P }
 *     ub(P) = lb(P) + #{ i : P is a prefix of S[i..n) }
 *
 *  - For a correct SA, SA[lb..ub) are the occurrences of P.
 *  - For the found cases this is what the reference's sa_index::locate returns (seq_query.hpp:246-251).
 *  - If P does not occur, lb == ub == the insertion point.  The reference's faster indexes only promise first == second there.
 *    This project pins the value, as it pins everything else.
 *  - m == 0 gives [0, n).
 *
 * Lookup table.  code() is the alphabet code: 1..sigma in byte order of the bytes that occur in the text, and 0 for an absent byte
 * and for positions past the end.  B = sigma + 1.
 *
 *     key_k(i) = sum over j < k of code(S[i+j]) * B^(k-1-j).
 *
 * The table has B^k + 1 entries of the index type.  table[v] = #{ i : key_k(i) < v }, so table[0] = 0, table[B^k] = n, and bucket
 * v is SA[table[v] .. table[v+1]).
 *  - This is lookup_index::table (lookup_table.hpp:36-149) with two changes.  The keys are dense: the reference packs bits_per_char
 *    bits, which wastes 5/8 of a DNA table.  The sum is exclusive, with one entry more.
 *  - k >= 1.  B^k > 2^30 returns PSACX_EINVAL.
 *
 * Use of the table by a pattern.  Let j = min(m, k).
 *  - If any of P[0..j) has code 0, the table is not used for that pattern.  It is searched over [0, n).
 *  - Otherwise v is the key of P[0..j) padded with zeros, and w = v + B^(k-j).
 *     - For m <= k the answer is [table[v], table[w]) with no search.
 *     - For m > k both bounds are searched inside [table[v], table[v+1]).  Comparisons may start at character k, because every
 *       suffix in that bucket has at least k characters and shares them with P.
 *
 * Totality.
 *  - Whatever SA and table hold, nothing is read out of range.  An SA entry >= n is compared as the empty suffix.  Table entries are
 *    clamped to n, and a bucket with lo > hi is treated as empty.
 *  - Every search terminates.
 *  - On arrays that are no suffix array or table of the text, the answers are unspecified except lb <= ub <= n.
 *
 * psacx_lookup_table_dev_*: code[256] (host memory) receives code(), *sigma the alphabet size, *entries = B^k + 1; d_table == NULL
 * only computes these three (the size query, as psacx_suffix_tree_dev_* has one; d_SA may be NULL then).  The alphabet comes from a
 * histogram taken on the device.  The table is counted from the text -- a histogram of key_k over all positions and an exclusive
 * scan, as lookup_table.hpp:60-140 -- so d_SA is not consulted and a wrong SA cannot leak into it.
 * psacx_locate_dev_*: d_pat holds the q patterns back to back, d_poff (device memory) their q + 1 offsets; d_lb / d_ub receive q
 * entries each.  d_table == NULL with k == 0 and code == NULL is the form without a table; any other mix of the three is
 * PSACX_EINVAL.  poff[0] != 0 or a descending pair returns PSACX_EINVAL, checked on the device before any result is written; equal
 * neighbours are empty patterns and legal.  q == 0 returns PSACX_OK.  Nothing is allocated per call beyond the 4 KiB of the ctx slab.
 * psacx_locate_*: the host-pointer form; k == 0 means no table.  It stages text, SA and patterns, builds the table when k > 0,
 * and copies the two result arrays back. */
int psacx_lookup_table_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_SA, uint32_t k,
                               uint32_t* d_table, uint16_t code[256], uint32_t* sigma, uint64_t* entries);
int psacx_lookup_table_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_SA, uint32_t k,
                               uint64_t* d_table, uint16_t code[256], uint32_t* sigma, uint64_t* entries);
int psacx_locate_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_SA,
                         const uint32_t* d_table, uint32_t k, const uint16_t code[256],
                         const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                         uint32_t* d_lb, uint32_t* d_ub);
int psacx_locate_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_SA,
                         const uint64_t* d_table, uint32_t k, const uint16_t code[256],
                         const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                         uint64_t* d_lb, uint64_t* d_ub);
int psacx_locate_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint32_t* SA, const uint8_t* pat, const uint64_t* poff,
                     uint64_t q, uint32_t k, uint32_t* lb, uint32_t* ub);
int psacx_locate_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* SA, const uint8_t* pat, const uint64_t* poff,
                     uint64_t q, uint32_t k, uint64_t* lb, uint64_t* ub);

/* pattern search over string sets -------------------------------------------------
 * The query side of psacx_construct_gsa_*: the same search over the generalized suffix array of a string set.  The reference has
 * the pieces -- sa_index::locate (seq_query.hpp:246-251), lookup_index (lookup_table.hpp:36-149) and the string set
 * (stringset.hpp:33-81) -- but no query over a set; psacx_locate_dev_* cannot stand in for one, because it compares up to the end of
 * the text and a pattern would match across the seam of two strings.  One GPU.
 *
 * Definitions.  The m strings lie back to back in text[0..n); offsets[0..m] ascends strictly from 0 to n (no empty string).
 * end(p) is the offset at which the string holding position p ends.  Suffix i is S[i..end(i)).  Bytes compare as unsigned
 * values, and a proper prefix is smaller.
 *
 *     lb(P) = #{ i : S[i..end(i)) < P }
 *     ub(P) = lb(P) + #{ i : P is a prefix of S[i..end(i)) }
 *
 *  - On a correct generalized suffix array the occurrences of P are exactly SA[lb..ub).  Equal suffixes lie in text order there, so
 *    nothing is ambiguous.
 *  - A pattern never matches across a string end.
 *  - If P does not occur, lb == ub == the insertion point.  m_P == 0 gives [0, n).
 *  - With m == 1 everything here equals the plain form above.
 *
 * String ends.  The index carries a bitmap of n + 1 bits, (n >> 5) + 1 words of 32: bit p = "a string starts at p, or p == n".
 * psacx_string_ends_dev builds it from the offsets: *words = (n >> 5) + 1, and d_ends == NULL only computes that (the size query;
 * d_offsets is not read then).  Offsets that do not start at 0, end at n and ascend strictly return PSACX_EINVAL before anything
 * is written (the rules of psacx_check_gsa_dev_*).  It is built once per index and handed to the calls below, as the lookup table
 * is: no query call does O(n) work for it.
 *
 * Lookup table.  code() and B as above (the alphabet of the whole text).  The keys are cut at string ends:
 *
 *     key_k(i) = sum over j < k of c_j * B^(k-1-j),   c_j = code(S[i+j]) if i + j < end(i), else 0.
 *
 * The table has B^k + 1 entries, table[v] = #{ i : key_k(i) < v }; k >= 1, and B^k > 2^30 returns PSACX_EINVAL.  It is counted from
 * the text and the bitmap, never from the SA.  d_table == NULL is the size query (d_ends may be NULL then).
 *
 * Use of the table by a pattern: the rule of the plain form, word for word.  Let j = min(m_P, k).
 *  - If any of P[0..j) has code 0, the table is not used for that pattern.  It is searched over [0, n).
 *  - Otherwise v is the key of P[0..j) padded with zeros, and w = v + B^(k-j).
 *     - For m_P <= k the answer is [table[v], table[w]) with no search.
 *     - For m_P > k both bounds are searched inside [table[v], table[v+1]).  Comparisons may start at character k, because every
 *       suffix in that bucket has at least k characters before its string ends and shares them with P.
 *
 * Totality, as for the plain form.
 *  - Whatever SA, table and bitmap hold, nothing is read at or beyond n, in the text or in the pattern buffer, and the bitmap is
 *    not read beyond bit n.  An SA entry >= n is the empty suffix.  Table entries are clamped to n, and an inverted bucket is empty.
 *  - Every search terminates, and lb <= ub <= n.
 *
 * psacx_locate_gsa_dev_*: arguments as psacx_locate_dev_*, with d_ends after n.  The mix rules for d_table, k and code, the check of
 * poff on the device before any result is written, and q == 0 are those of the plain form.  Nothing is allocated per call beyond
 * the 4 KiB of the ctx slab.  The kernel is one pattern per lane.  PSACX_OPT_LOCATE_SHAPE = 2 has no effect here: there is no
 * eight-lane form for string sets.  A bisection step is still two dependent fetches: when SA[mid] has arrived, the bitmap words of
 * the next 8 characters and the text word are fetched together and the text word is cut at the first set bit; a comparison reads
 * at most ceil(m_P / 32) + 1 bitmap words.  With PSACX_OPT_LOCATE_COUNT, psacx_stats.locate_fetches counts SA entries and text
 * words as for the plain form.  Bitmap words are not counted.
 * psacx_locate_gsa_*: the host-pointer form; k == 0 means no table.  It stages text, offsets, SA and patterns, builds the bitmap
 * (malformed offsets: PSACX_EINVAL), builds the table when k > 0, copies the two result arrays back, and frees what it allocated
 * on every path. */
int psacx_string_ends_dev(psacx_ctx* ctx, const uint64_t* d_offsets, uint64_t m, uint64_t n, uint32_t* d_ends, uint64_t* words);
int psacx_lookup_table_gsa_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, uint32_t k,
                                   uint32_t* d_table, uint16_t code[256], uint32_t* sigma, uint64_t* entries);
int psacx_lookup_table_gsa_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, uint32_t k,
                                   uint64_t* d_table, uint16_t code[256], uint32_t* sigma, uint64_t* entries);
int psacx_locate_gsa_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint32_t* d_SA,
                             const uint32_t* d_table, uint32_t k, const uint16_t code[256],
                             const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                             uint32_t* d_lb, uint32_t* d_ub);
int psacx_locate_gsa_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint64_t* d_SA,
                             const uint64_t* d_table, uint32_t k, const uint16_t code[256],
                             const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                             uint64_t* d_lb, uint64_t* d_ub);
int psacx_locate_gsa_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA,
                         const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint32_t* lb, uint32_t* ub);
int psacx_locate_gsa_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA,
                         const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint64_t* lb, uint64_t* ub);

/* longest match and matching statistics ---------------------------------------------
 * The question one level above locate: how long is the longest prefix of a query that occurs, and where?  psacx_locate_*
 * answers a pattern that does not occur with a bare insertion point; these calls answer it with the length of its longest
 * matching prefix and that prefix's interval, and can do so for every suffix of every pattern in one launch (the matching
 * statistics of the patterns).  The reference has no counterpart.  One GPU.
 *
 * Definitions.  Text, suffixes, byte order, lb(), ub(), code(), the table and the bitmap of the string ends are exactly those of
 * the two blocks above: in the plain form suffix i is S[i..n), in the set form it is S[i..end(i)).  For a query Q of m bytes:
 *
 *     len(Q)   = max { d <= m : Q[0..d) is a prefix of some suffix }         (d = 0 always qualifies)
 *     [lb, ub) = [ lb(Q[0..len)), ub(Q[0..len)) )                             (the locate interval of the matched prefix)
 *
 *  - len == m means Q occurs, and [lb, ub) is what locate returns.  len == 0 gives [0, n).
 *  - On a correct SA the interval is never empty for n >= 1.
 *  - Nothing is ambiguous: all three values are functions of the text (and the offsets) alone.
 *  - In the set form a match never crosses a string end.
 *
 * Which queries.  flags == 0: one query per pattern, Q_j = pat[poff[j] .. poff[j+1]), and q results.
 * flags & PSACX_MATCH_SUFFIXES: one query per byte of the pattern buffer.  Slot p in [0, poff[q]) belongs to the pattern j with
 * poff[j] <= p < poff[j+1]; its query is pat[p .. poff[j+1]); there are poff[q] results, in buffer order.  Empty patterns own no
 * slot.  These are the matching statistics of every pattern.
 *
 * Cap.  max_len > 0 truncates every query to its first max_len bytes before anything else, so len <= max_len.  max_len == 0
 * means no cap.
 *
 * Table.  With a correct table the three results equal those without one, for every query.  Non-emptiness of the bucket of
 * Q[0..j) is monotone in j, so the longest prefix of at most min(m, k) bytes that occurs is found from table entries alone;
 * only a query whose first k bytes occur, with m > k, is searched, inside its bucket.  A byte with code 0 (absent from the
 * text) at position i of Q bounds len <= i: unlike locate, this form never falls back to a search over [0, n) because of such
 * a byte.
 *
 * Totality, as for locate.  Whatever SA, table and bitmap hold, nothing is read out of range: text and pattern buffer never at
 * or beyond their ends, the bitmap never beyond bit n, the table only inside its B^k + 1 entries.  Every loop terminates.
 * len <= m (and <= max_len), and lb <= ub <= n.  On arrays that are no suffix array, table or bitmap of the text the values are
 * otherwise unspecified.
 *
 * psacx_match_dev_* / psacx_match_gsa_dev_*: arguments as psacx_locate_dev_* / psacx_locate_gsa_dev_*; d_len, d_lb and d_ub
 * (index type) receive out_entries results each.  out_entries is the room the caller has: it must equal q, or poff[q] in the
 * suffix mode.  A mismatch, poff[0] != 0 or a descending pair returns PSACX_EINVAL, found on the device before any result is
 * written.  The mix rules for d_table / k / code are those of locate; unknown flag bits return PSACX_EINVAL; q == 0 returns
 * PSACX_OK (out_entries must be 0).  Nothing is allocated per call beyond the 4 KiB of the ctx slab.  With
 * PSACX_OPT_LOCATE_COUNT, psacx_stats.locate_fetches counts SA entries and text words as for locate; for a batch of patterns
 * that all occur the counts equal those of the locate call.
 * psacx_match_* / psacx_match_gsa_*: the host-pointer forms; k == 0 means no table.  They stage text, (offsets,) SA and
 * patterns, build the bitmap and the table when k > 0, copy the three result arrays back -- q entries each, or poff[q] in the
 * suffix mode -- and free what they allocated on every path. */
#define PSACX_MATCH_SUFFIXES 1u
int psacx_match_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_SA,
                        const uint32_t* d_table, uint32_t k, const uint16_t code[256],
                        const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                        uint32_t flags, uint64_t max_len, uint64_t out_entries, uint32_t* d_len, uint32_t* d_lb, uint32_t* d_ub);
int psacx_match_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_SA,
                        const uint64_t* d_table, uint32_t k, const uint16_t code[256],
                        const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                        uint32_t flags, uint64_t max_len, uint64_t out_entries, uint64_t* d_len, uint64_t* d_lb, uint64_t* d_ub);
int psacx_match_gsa_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint32_t* d_SA,
                            const uint32_t* d_table, uint32_t k, const uint16_t code[256],
                            const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                            uint32_t flags, uint64_t max_len, uint64_t out_entries, uint32_t* d_len, uint32_t* d_lb, uint32_t* d_ub);
int psacx_match_gsa_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint64_t* d_SA,
                            const uint64_t* d_table, uint32_t k, const uint16_t code[256],
                            const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                            uint32_t flags, uint64_t max_len, uint64_t out_entries, uint64_t* d_len, uint64_t* d_lb, uint64_t* d_ub);
int psacx_match_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint32_t* SA, const uint8_t* pat, const uint64_t* poff,
                    uint64_t q, uint32_t k, uint32_t flags, uint64_t max_len, uint32_t* len, uint32_t* lb, uint32_t* ub);
int psacx_match_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* SA, const uint8_t* pat, const uint64_t* poff,
                    uint64_t q, uint32_t k, uint32_t flags, uint64_t max_len, uint64_t* len, uint64_t* lb, uint64_t* ub);
int psacx_match_gsa_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA,
                        const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint32_t flags, uint64_t max_len,
                        uint32_t* len, uint32_t* lb, uint32_t* ub);
int psacx_match_gsa_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA,
                        const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint32_t flags, uint64_t max_len,
                        uint64_t* len, uint64_t* lb, uint64_t* ub);

/* occurrence lists ------------------------------------------------------------------
 * The positions behind a batch of intervals [lb_j, ub_j) of either search, in HBM.
 *
 *     c_j = ub_j - lb_j if lb_j <= ub_j <= n, else 0; with limit > 0, c_j is capped at limit.
 *     start = the exclusive prefix sums of c (q + 1 entries of 64 bits), start[q] = *total.
 *     pos[start_j + t] = SA[lb_j + t] for t < c_j: SA order, which is pinned.  Sorting by position is not part of this.
 *     sid[start_j + t] = the string holding that position: the largest s with offsets[s] <= pos, and m for a pos >= n.
 *
 *  - d_offsets == NULL: one text (m is ignored).  d_sid, where not NULL, needs d_offsets and d_pos (PSACX_EINVAL otherwise).  The
 *    offsets are only searched, never trusted: any m + 1 values give some s in [0, m).
 *  - d_pos == NULL is the size query: start and *total only.
 *  - *total > cap returns PSACX_ERANGE; start and *total are valid, and nothing is written to d_pos or d_sid.
 *  - q == 0 gives *total = 0 and PSACX_OK.  No input is written.  SA entries are copied as they are, entries >= n included.
 *  - The expansion is balanced by output: a workgroup owns a fixed tile of output slots, finds its first pattern by one binary
 *    search in start, and walks forward from there, so the cost per output does not depend on how the counts are spread.  The
 *    scan's block sums live in the ctx slab, 8 bytes per 4096 patterns beyond its 4 KiB. */
int psacx_occurrences_dev_u32(psacx_ctx* ctx, const uint32_t* d_SA, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                              const uint32_t* d_lb, const uint32_t* d_ub, uint64_t q, uint64_t limit,
                              uint64_t* d_start, uint32_t* d_pos, uint32_t* d_sid, uint64_t cap, uint64_t* total);
int psacx_occurrences_dev_u64(psacx_ctx* ctx, const uint64_t* d_SA, uint64_t n, const uint64_t* d_offsets, uint64_t m,
                              const uint64_t* d_lb, const uint64_t* d_ub, uint64_t q, uint64_t limit,
                              uint64_t* d_start, uint64_t* d_pos, uint64_t* d_sid, uint64_t cap, uint64_t* total);

/* range minimum and longest common extension -------------------------------------------
 * The two questions that need ISA and LCP: what is the minimum of LCP[l..r) and where does it first occur, and how far do two
 * text positions agree.  The reference has the sequential structure (rmq<>::query, rmq.hpp:186, returns the first minimum of a
 * range; par_rmq.hpp spreads it over ranks); nothing of it queries positions of the text.  One GPU.  The text is no argument
 * of any call here.
 *
 * Definitions.  V[0..n) is an array of the index type T, "all ones" is the largest value of T.
 *
 *     range_j = [lo_j, min(hi_j, n))
 *     min_j   = min V[range_j]
 *     arg_j   = the smallest position in range_j that holds min_j        (the first minimum, as std::min_element)
 *
 *  - An empty range (lo_j >= min(hi_j, n)) gives min_j = all ones and arg_j = n.
 *  - A value of all ones is legal in V; arg_j still lies inside the range.
 *
 * Index.  The 64-ary min-pyramid of V from level 1 upwards -- level[L][i] = min V[64^L i .. 64^L (i + 1)) -- and, for every
 * such level, the running minima of each group of 64 entries from its left end and from its right end.  Level 0 is V itself:
 * a second copy would not fit the bound.  *entries counts entries of T: 3 (n / 63) and a few per level, at least 1 and at most
 * n / 16 + 4096.  The index holds values only, never positions a query would use as an address; it is opaque otherwise and
 * valid for as long as V does not change.
 *
 * Longest common extension.  Text S[0..n) with its ISA and LCP (LCP[i] = the common prefix of the suffixes of ranks i - 1 and
 * i), or a string set with the arrays of psacx_construct_gsa_* and its m + 1 offsets.
 *
 *     end(p) = n in the plain form (d_offsets == NULL, m ignored); in the set form the end of the string that holds p: the
 *              smallest offset above p, clamped to (p, n].  A position >= n is the empty suffix and its end is itself.
 *     L      = min(end(a) - a, end(b) - b)
 *     lce_e(a, b) = max { d <= L : #{ j < d : S[a+j] != S[b+j] } <= e },   e = max_mismatch; e = 0 is the plain LCE.
 *
 * From the arrays, for a != b and both below n, with r = ISA[a] and s = ISA[b]:
 *
 *     lce_0(a, b) = min LCP[min(r, s) + 1 .. max(r, s) + 1);           lce_0(a, a) = end(a) - a.
 *
 * For e > 0 the kangaroo walk: add lce_0(a + d, b + d) to d; stop when d >= L; otherwise the byte at d differs by definition,
 * and while the budget lasts it is stepped over and the walk goes on.  At most e + 1 range minima per pair.
 *  - The offsets are only searched (one binary search per side), never trusted, as in psacx_occurrences_dev_*.
 *  - The set form with e = 0 and a != b searches no offsets: the generalized LCP is cut at string ends already.
 *
 * Totality.  Whatever V, ISA, LCP, index and offsets hold, nothing is read out of range: every address follows from lo, hi, a,
 * b and n, an ISA entry >= n is clamped to n - 1, and offsets are read inside their m + 1 entries.  Every loop ends.
 * arg_j lies in range_j or equals n.  len <= n - max(a, b), and 0 for a position >= n.  On arrays that are not the ISA, LCP and
 * index of one text, the values are otherwise unspecified.
 *
 * psacx_rmq_index_dev_*: builds the index of d_values into d_index; d_index == NULL is the size query (d_values may be NULL
 * then).  n == 0 is legal.  It is built once per array and handed to the calls below, as the lookup table is: no query call
 * does O(n) work.  n beyond the index type, or beyond 2^48, returns PSACX_ERANGE.  After psacx_profile(ctx, 1),
 * psacx_stats.ms_rmq_build receives the time of the level-1 kernel alone, the one pass over the values (tools/lce_time.py).
 * psacx_rmq_dev_*: d_lo / d_hi hold q range ends each; d_min / d_arg receive q entries each.  Either may be NULL (the first
 * minimum is then not searched for); both NULL returns PSACX_EINVAL.  q == 0 returns PSACX_OK.  Nothing is allocated per call,
 * and no input is written.  Sixteen lanes answer one range: two 64-entry groups of V at most, one entry of the index per lane
 * above them, one wait; the position costs a second walk of at most 2 levels - 1 groups.
 * psacx_lce_dev_*: d_index is the range-minimum index of d_LCP; d_a / d_b hold q positions each, d_len receives q lengths.
 * d_offsets != NULL with m == 0 or m > n returns PSACX_EINVAL.
 * psacx_rmq_* / psacx_lce_*: the host-pointer forms.  They stage the arrays, build the index, copy the results back, and free
 * what they allocated on every path. */
int psacx_rmq_index_dev_u32(psacx_ctx* ctx, const uint32_t* d_values, uint64_t n, uint32_t* d_index, uint64_t* entries);
int psacx_rmq_index_dev_u64(psacx_ctx* ctx, const uint64_t* d_values, uint64_t n, uint64_t* d_index, uint64_t* entries);
int psacx_rmq_dev_u32(psacx_ctx* ctx, const uint32_t* d_values, uint64_t n, const uint32_t* d_index,
                      const uint32_t* d_lo, const uint32_t* d_hi, uint64_t q, uint32_t* d_min, uint32_t* d_arg);
int psacx_rmq_dev_u64(psacx_ctx* ctx, const uint64_t* d_values, uint64_t n, const uint64_t* d_index,
                      const uint64_t* d_lo, const uint64_t* d_hi, uint64_t q, uint64_t* d_min, uint64_t* d_arg);
int psacx_lce_dev_u32(psacx_ctx* ctx, uint64_t n, const uint64_t* d_offsets, uint64_t m, const uint32_t* d_ISA, const uint32_t* d_LCP,
                      const uint32_t* d_index, const uint32_t* d_a, const uint32_t* d_b, uint64_t q, uint64_t max_mismatch,
                      uint32_t* d_len);
int psacx_lce_dev_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* d_offsets, uint64_t m, const uint64_t* d_ISA, const uint64_t* d_LCP,
                      const uint64_t* d_index, const uint64_t* d_a, const uint64_t* d_b, uint64_t q, uint64_t max_mismatch,
                      uint64_t* d_len);
int psacx_rmq_u32(psacx_ctx* ctx, const uint32_t* values, uint64_t n, const uint32_t* lo, const uint32_t* hi, uint64_t q,
                  uint32_t* min, uint32_t* arg);
int psacx_rmq_u64(psacx_ctx* ctx, const uint64_t* values, uint64_t n, const uint64_t* lo, const uint64_t* hi, uint64_t q,
                  uint64_t* min, uint64_t* arg);
int psacx_lce_u32(psacx_ctx* ctx, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* ISA, const uint32_t* LCP,
                  const uint32_t* a, const uint32_t* b, uint64_t q, uint64_t max_mismatch, uint32_t* len);
int psacx_lce_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* ISA, const uint64_t* LCP,
                  const uint64_t* a, const uint64_t* b, uint64_t q, uint64_t max_mismatch, uint64_t* len);

/* suffix-prefix overlaps --------------------------------------------------------------
 * The question a generalized suffix array of reads is built for: which suffixes of which strings are prefixes of which other
 * strings -- the all-pairs suffix-prefix problem, whose answers are the edges of an overlap graph.  psacx_locate_gsa_* of a
 * prefix returns every occurrence, not the ones that end their string.  The reference has no counterpart.  One GPU.  The text
 * is no argument of any call here: ISA, LCP, the range-minimum index of LCP and the bitmap of the string ends answer it.
 *
 * Definitions.  Text, offsets o_0 .. o_m, end(p), suffix i = S[i..end(i)), the byte order and the bitmap are exactly those of
 * "pattern search over string sets".  String j is S[o_j..o_{j+1}) with L_j bytes, X(j, d) its first d bytes.
 *
 *     T(j, d)   = { i : S[i..end(i)) == X(j, d) }          the suffixes that ARE X(j, d): they end their string after d bytes
 *     olb(j, d) = #{ i : S[i..end(i)) < X(j, d) }          (= lb(X(j, d)) of locate)
 *     oub(j, d) = olb(j, d) + |T(j, d)|
 *
 *  - On a correct generalized suffix array SA[olb..oub) is exactly T(j, d): an end sorts below every character, so the suffixes
 *    equal to X(j, d) come first among those that start with it, and equal suffixes lie in text order.
 *  - A member of T(j, d) may lie in string j itself: a border of j.  A member may be a whole string: that string is a prefix of
 *    j.  Both are overlaps by the definition and both are reported.
 *
 * Depths asked.  d runs over [min_len, L_j - 1]; with PSACX_OVERLAP_WHOLE over [min_len, L_j].  The interval of d == L_j holds
 * every string that ends with string j, string j itself (position o_j) among them.  min_len == 0 and unknown flag bits return
 * PSACX_EINVAL.
 *
 * Output.  One slot per byte of the text, as in the suffix mode of match: slot p = o_j + d - 1 belongs to (j, d).
 * lb[p], ub[p] = olb(j, d), oub(j, d) where d is asked and T(j, d) is not empty; every other slot holds 0, 0.  n entries of the
 * index type each.  psacx_occurrences_dev_* takes the two arrays as they are, with q = n and the offsets: pos is where the
 * overlap of length d onto string j starts, sid the string it comes from.
 *
 * The walk.  The overlaps of string j sit on the path from its leaf to the root of the suffix tree, which in LCP is a chain of
 * previous-smaller-value steps from r = ISA[o_j].  With i = r and d = L_j - 1 (L_j with PSACX_OVERLAP_WHOLE), while d >= min_len:
 *  1. if LCP[i] >= d, i becomes the largest x < i with LCP[x] <= d - 1 (none: stop).  Now i = olb(j, d).
 *  2. T(j, d) is not empty iff the suffix SA[i] ends after d bytes: SA[i] + d <= n and that bit of the bitmap is set.
 *  3. Then oub is the first x in (i, hi) whose bit SA[x] + d is clear, or hi; the bits are monotone there.  hi = r for d < L_j
 *     (entry r is string j and longer than d); for d == L_j it is the first x > r with LCP[x] <= d - 1, or n.
 *  4. d becomes LCP[i].  For the depths in between olb is still i and SA[i] is longer than they are: those slots are empty by
 *     definition and are not searched.
 * A few steps per string instead of one search per prefix.
 *
 * Totality.  Whatever SA, ISA, LCP, index, bitmap and offsets hold, nothing is read out of range: SA, ISA and LCP inside
 * [0, n), the bitmap never beyond bit n, the index by its layout only.  Every loop ends: the depth falls strictly per step,
 * and a step that would not lower it ends the walk.  lb <= ub <= n in every slot.  Offsets that do not start at 0, end at n
 * and ascend strictly return PSACX_EINVAL before anything is written (the device check of psacx_string_ends_dev).  m == 0 or
 * n == 0 returns PSACX_OK.  On arrays that are no index of one string set the values are otherwise unspecified.
 *
 * psacx_overlaps_dev_*: d_ends is the bitmap of psacx_string_ends_dev, d_index the index of psacx_rmq_index_dev_* over d_LCP.
 * The call clears d_lb and d_ub itself and allocates nothing beyond the ctx slab.  No input is written.  Sixteen lanes walk
 * one string; the end of a run is found by a 16-way partition, one probe per lane and round.
 * psacx_overlaps_*: the host-pointer form.  It stages offsets, SA, ISA and LCP, builds the bitmap and the index, copies the 2 n
 * entries back, and frees what it allocated on every path. */
#define PSACX_OVERLAP_WHOLE 1u
int psacx_overlaps_dev_u32(psacx_ctx* ctx, uint64_t n, const uint64_t* d_offsets, uint64_t m, const uint32_t* d_ends,
                           const uint32_t* d_SA, const uint32_t* d_ISA, const uint32_t* d_LCP, const uint32_t* d_index,
                           uint64_t min_len, uint32_t flags, uint32_t* d_lb, uint32_t* d_ub);
int psacx_overlaps_dev_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* d_offsets, uint64_t m, const uint32_t* d_ends,
                           const uint64_t* d_SA, const uint64_t* d_ISA, const uint64_t* d_LCP, const uint64_t* d_index,
                           uint64_t min_len, uint32_t flags, uint64_t* d_lb, uint64_t* d_ub);
int psacx_overlaps_u32(psacx_ctx* ctx, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA, const uint32_t* ISA,
                       const uint32_t* LCP, uint64_t min_len, uint32_t flags, uint32_t* lb, uint32_t* ub);
int psacx_overlaps_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA, const uint64_t* ISA,
                       const uint64_t* LCP, uint64_t min_len, uint32_t flags, uint64_t* lb, uint64_t* ub);

/* LZ77 factorization ------------------------------------------------------------------
 * The first question asked of the index about the text itself: the longest previous factor of every position and the greedy
 * Lempel-Ziv parse cut from it -- for compression, for the repetitiveness measure z, as input to an LZ-index.  The reference has
 * no counterpart.  One text, one GPU.  The text is no argument of the two building calls: SA, LCP and the range-minimum index of
 * LCP (psacx_rmq_index_dev_*) answer them.
 *
 * Definitions.  Text S[0..n), "all ones" the largest value of the index type.  SA and LCP as psacx_construct_dev_* leaves them,
 * LCP[r] the common prefix of the suffixes of ranks r - 1 and r.  For rank r with i = SA[r]:
 *
 *     p = the largest rank below r with SA[p] < i          (none: lp = 0)
 *     q = the smallest rank above r with SA[q] < i         (none: lq = 0)
 *     lp = min LCP[p+1 .. r+1)        lq = min LCP[r+1 .. q+1)
 *     if lp >= lq and lp > 0:   LPF[i] = lp,  SRC[i] = SA[p]
 *     else if lq > 0:           LPF[i] = lq,  SRC[i] = SA[q]
 *     else:                     LPF[i] = 0,   SRC[i] = all ones
 *
 *  - On the arrays of one text LPF[i] = max over j < i of lcp(S[i..), S[j..)): the longest previous factor.  The predecessor
 *    wins ties, which pins SRC.
 *  - p and q are nearest smaller values of SA itself, on both sides; lp and lq are two range minima.
 *
 * Parse.  s_0 = 0; len_k = min(max(1, LPF[s_k]), n - s_k); s_{k+1} = s_k + len_k, until s_z = n.  A phrase with LPF[s_k] = 0 is a
 * literal of one byte and its source is all ones; every other phrase copies len_k bytes from SRC[s_k].  A source may overlap its
 * phrase (src + len > start), as in LZ77: a decoder copies byte by byte.
 *
 * Totality.  Whatever SA, LCP and index hold, nothing is read or written out of range; SA entries >= n write nothing; both
 * outputs are cleared first, to 0 and to all ones; every slot ends as either (LPF = 0, SRC = all ones) or (SRC < i and
 * 1 <= LPF <= n - i).  The parse takes any n values as LPF, clamps them as above and always ends with s_z = n.
 *
 * psacx_lpf_dev_*: d_lpf and d_src receive n entries each.  n == 0 is legal; n beyond the index type returns PSACX_ERANGE; a NULL
 * output PSACX_EINVAL.  Scratch: 16 n bytes of device memory for the two neighbour arrays, allocated for the time of the call
 * beside the ctx slab (which holds the search pyramid over SA); where that fails the call returns PSACX_ENOMEM and the outputs are
 * as they were.  Sixteen lanes per rank; no input is written.
 * psacx_lz77_dev_*: d_start receives z + 1 entries, start[z] = n; d_psrc receives z entries, all ones for a literal.  *z is
 * always set.  d_start == NULL is the count query.  z + 1 > cap returns PSACX_ERANGE with *z valid and nothing written to the two
 * lists (the convention of psacx_occurrences_dev_*).  d_src may be NULL (any n values as LPF, no sources); d_psrc must then be
 * NULL too.  Scratch in the ctx slab: n entries of the index type, n bytes, and a word per 1024 positions.  No kernel of the parse
 * follows a chain of dependent loads that grows with n beyond one load per 2^17 positions.
 * psacx_check_lz77_dev_*: the round-trip verdict -- the parse decodes to the text.  *errors counts
 *   - start[0] != 0, and start[z] != n                                         (one each);
 *   - per phrase k: start[k+1] <= start[k]; else a literal (source all ones) longer than 1; and a source >= start[k];
 *   - per text position x, whose phrase k is found by a bisection of start: x outside [start[k], start[k+1]); else, for a phrase
 *     with a source below its start, S[src + x - start[k]] != S[x].
 * 0 means that start / psrc decode to S byte by byte.  It does not prove the parse greedy: any parse into literals and earlier
 * copies passes.  (Greediness is held by the host model of the tests at small sizes.)  z > n returns PSACX_EINVAL.  Nothing is
 * read out of range whatever the lists hold.
 * psacx_lpf_* / psacx_lz77_*: the host-pointer forms.  They stage SA and LCP, build the index, and free what they allocated on
 * every path.  psacx_lz77_* returns start (z + 1 entries) and src (z entries) without handing out LPF; start == NULL and
 * src == NULL is the count query, z + 1 > cap returns PSACX_ERANGE with *z valid. */
int psacx_lpf_dev_u32(psacx_ctx* ctx, uint64_t n, const uint32_t* d_SA, const uint32_t* d_LCP, const uint32_t* d_index, uint32_t* d_lpf,
                      uint32_t* d_src);
int psacx_lpf_dev_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* d_SA, const uint64_t* d_LCP, const uint64_t* d_index, uint64_t* d_lpf,
                      uint64_t* d_src);
int psacx_lz77_dev_u32(psacx_ctx* ctx, uint64_t n, const uint32_t* d_lpf, const uint32_t* d_src, uint32_t* d_start, uint32_t* d_psrc,
                       uint64_t cap, uint64_t* z);
int psacx_lz77_dev_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* d_lpf, const uint64_t* d_src, uint64_t* d_start, uint64_t* d_psrc,
                       uint64_t cap, uint64_t* z);
int psacx_check_lz77_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_start, const uint32_t* d_psrc, uint64_t z,
                             uint64_t* errors);
int psacx_check_lz77_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint64_t* d_start, const uint64_t* d_psrc, uint64_t z,
                             uint64_t* errors);
int psacx_lpf_u32(psacx_ctx* ctx, uint64_t n, const uint32_t* SA, const uint32_t* LCP, uint32_t* lpf, uint32_t* src);
int psacx_lpf_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* SA, const uint64_t* LCP, uint64_t* lpf, uint64_t* src);
int psacx_lz77_u32(psacx_ctx* ctx, uint64_t n, const uint32_t* SA, const uint32_t* LCP, uint32_t* start, uint32_t* src, uint64_t cap,
                   uint64_t* z);
int psacx_lz77_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* SA, const uint64_t* LCP, uint64_t* start, uint64_t* src, uint64_t cap,
                   uint64_t* z);

/* BWT and repeats ---------------------------------------------------------------------
 * The Burrows-Wheeler transform of the text, and the repeats of a text or a read set as the inner nodes of its suffix tree
 * filtered by what stands to their left: right-maximal, maximal and supermaximal repeats from SA + LCP + BWT (Abouelhoda, Kurtz,
 * Ohlebusch 2004).  psacx_suffix_tree_dev_* reaches the same nodes through a table of n x (sigma + 1) words; nothing here needs
 * it, and no ANSV is used.  The reference has no counterpart.  One GPU.
 *
 * Setting.  One text S[0..n), or a string set as for psacx_locate_gsa_dev_*: the m strings lie back to back and d_ends is the
 * bitmap of psacx_string_ends_dev (bit p = "a string starts at p, or p == n").  SA and LCP as psacx_construct_dev_* /
 * psacx_construct_gsa_dev_* leave them.  L[r] = LCP[r], with L[0] read as 0 whatever is stored.  Ranks are SA indices.  "All ones"
 * is the largest value of the index type.
 *
 * BWT.
 *     bwt[r]   = S[SA[r] - 1] if SA[r] is not the start of a string; otherwise the last byte of that string (S[n-1] for one text):
 *                the cyclic convention per string.  The array is aligned with SA.  It is NOT libdivsufsort's divbwt layout, which
 *                drops the primary entry and shifts the entries in front of it.
 *     first    = a bitmap of (n >> 5) + 1 words of 32: bit r is set iff SA[r] starts a string (one text: iff SA[r] == 0).  Bits at
 *                and beyond n are 0.
 *     *primary = the rank r with SA[r] == 0; all ones of 64 bits if no entry is 0; any one of them if several are.
 *  - d_ends == NULL: one text.  d_first and primary may each be NULL; d_bwt may be NULL if d_first is not.
 *  - Totality: an SA entry >= n gives bwt 0 and a clear bit.  Nothing is read outside the text [0, n) and the bitmap [0, n].  No
 *    input is written.  n == 0 is PSACX_OK; n beyond the index type returns PSACX_ERANGE.
 *  - One rank per lane, one gathered byte per rank.  A wave owns 64 consecutive ranks and its two words of `first` come from one
 *    ballot, stored by two of its lanes: no atomics and no read-modify-write of bitmap words.  The primary is written by the lane
 *    that sees it.  A rank that starts a string of a set needs the end of that string; the wave scans d_ends for it 64 words a step,
 *    n / 32 words over all strings.  Scratch: 8 bytes of the ctx slab.
 *
 * Repeats.  A repeat is named by its LCP-interval.  Rank j >= 1 with l = L[j] > 0 is a HEAD iff the largest h < j with L[h] <= l
 * has L[h] < l: the head(x) == x of the suffix-tree checker above, one head per inner node.  Its interval is lb = h and ub = the
 * smallest e > j with L[e] < l, or n.  The repeat is S[SA[lb] .. SA[lb] + l); it has ub - lb >= 2 occurrences, exactly SA[lb..ub).
 * In a set a string end counts as a right character different from everything and a string start as a left character different
 * from everything: one unique sentinel on each side of each string.
 *
 * Three bit arrays over the ranks 1 .. n - 1:
 *     D[x]  = first[x] or first[x-1] or bwt[x] != bwt[x-1]
 *     F[x]  = first[x]                                                    (also at rank 0)
 *     St[x] = L[x] != L[x-1]
 * The kinds:
 *     PSACX_REPEATS_RIGHT         every head: the right-maximal repeats, all inner nodes below the root.
 *     PSACX_REPEATS_MAXIMAL       heads whose interval is left-diverse: D[x] == 1 for some lb < x < ub.
 *     PSACX_REPEATS_SUPERMAXIMAL  heads whose interval is flat (no x in [lb + 2, ub) has St[x] == 1: all children are leaves), holds
 *                                 at most 256 ranks that do not start a string, and whose bwt bytes of those ranks are pairwise
 *                                 different.  The same as "a maximal repeat that is a substring of no other maximal repeat".
 * Filters, applied after the kind: l >= min_len (0 and 1 mean the same); ub - lb >= min_occ (values below 2 mean 2); with
 * max_occ > 0, ub - lb <= max_occ.
 *
 * psacx_repeats_dev_*: d_index is the index of psacx_rmq_index_dev_* over d_LCP; d_bwt and d_first are the outputs of
 * psacx_bwt_dev_*.
 *  - Output: z triples (lb, ub, len = l) in ascending order of the head j, which is pinned.  d_len may be NULL.
 *  - d_lb == NULL (then d_ub and d_len must be NULL too, PSACX_EINVAL otherwise) is the count query.
 *  - z > cap returns PSACX_ERANGE with *z valid and nothing written to the lists (the convention of psacx_lz77_dev_* and
 *    psacx_occurrences_dev_*).  *z is always set.
 *  - Kind 0 reads neither d_bwt nor d_first, and both may be NULL.  Kinds 1 and 2 need both (PSACX_EINVAL otherwise).  An unknown
 *    kind returns PSACX_EINVAL.  n <= 1 gives z = 0.  n beyond the index type, or beyond 2^48, returns PSACX_ERANGE.
 *  - d_lb and d_ub are, as they are, the interval lists psacx_occurrences_dev_* takes (q = z): pos lists where each repeat occurs,
 *    sid in which string.
 *  - Totality, whatever LCP, index, bwt and first hold: nothing is read or written out of range (first inside its (n >> 5) + 1
 *    words and below bit n), every search ends, every triple has 0 <= lb < ub <= n, ub - lb >= 2 and len >= 1, rank 0 is never a
 *    head, and a left search that finds nothing means lb = 0.  No input is written.
 *  - Sixteen lanes per rank.  A rank costs one search to the left (one or two groups of 64 LCP entries where the answer is near) and
 *    one fetch of L[h]; most ranks end there.  A head adds one search to the right and, per kind, two directory entries and two
 *    bitmap words for each of its tests.  The supermaximal kind then walks the bwt bytes of its interval, 16 per step, and leaves at
 *    the first collision.  Flat intervals are disjoint, so the walks of a whole call touch at most n ranks; only a run of identical
 *    whole strings makes a single walk long.
 *  - Scratch.  In the ctx slab, with c = (n >> 6) + 1 and t = ceil(n / 1024): for kinds 1 and 2 the bit arrays D and F with their
 *    directories, 2 * (8 c + 8 c) bytes; for kind 2 the same for St, 16 c bytes; the select bytes, 1024 t; the tile counts,
 *    8 (t + 1); the block sums of the scans, 8 bytes per 4096 of max(c, t + 1) beyond 4 KiB; each part rounded up to 256 bytes.
 *    Kind 1 scans D alone and kind 2 F and St.  A call that writes lists also allocates 2 n entries of the index type for the
 *    candidate intervals, beside the slab and for the time of the call; where that fails it returns PSACX_ENOMEM and the outputs
 *    are untouched.  The count query allocates nothing.  It runs everything but the last kernel, so a caller that counts first and
 *    asks for the lists afterwards pays the walk over the ranks twice.
 * psacx_bwt_* / psacx_repeats_*: the host-pointer forms.  offsets == NULL means one text (m is ignored); otherwise the m + 1
 * offsets of the strings, which must start at 0, end at n and ascend strictly (PSACX_EINVAL).  They stage the arrays, build the
 * bitmap of the string ends, the index and the BWT, and free what they allocated on every path.  psacx_bwt_* needs bwt;
 * psacx_repeats_* with lb == NULL is the count query, z > cap returns PSACX_ERANGE with *z valid; kind 0 reads neither text nor SA. */
#define PSACX_REPEATS_RIGHT 0u
#define PSACX_REPEATS_MAXIMAL 1u
#define PSACX_REPEATS_SUPERMAXIMAL 2u
int psacx_bwt_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint32_t* d_SA, uint8_t* d_bwt,
                      uint32_t* d_first, uint64_t* primary);
int psacx_bwt_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint64_t* d_SA, uint8_t* d_bwt,
                      uint32_t* d_first, uint64_t* primary);
int psacx_repeats_dev_u32(psacx_ctx* ctx, uint64_t n, const uint32_t* d_LCP, const uint32_t* d_index, const uint8_t* d_bwt,
                          const uint32_t* d_first, uint32_t kind, uint64_t min_len, uint64_t min_occ, uint64_t max_occ, uint32_t* d_lb,
                          uint32_t* d_ub, uint32_t* d_len, uint64_t cap, uint64_t* z);
int psacx_repeats_dev_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* d_LCP, const uint64_t* d_index, const uint8_t* d_bwt,
                          const uint32_t* d_first, uint32_t kind, uint64_t min_len, uint64_t min_occ, uint64_t max_occ, uint64_t* d_lb,
                          uint64_t* d_ub, uint64_t* d_len, uint64_t cap, uint64_t* z);
int psacx_bwt_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA, uint8_t* bwt,
                  uint64_t* primary);
int psacx_bwt_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA, uint8_t* bwt,
                  uint64_t* primary);
int psacx_repeats_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA,
                      const uint32_t* LCP, uint32_t kind, uint64_t min_len, uint64_t min_occ, uint64_t max_occ, uint32_t* lb, uint32_t* ub,
                      uint32_t* len, uint64_t cap, uint64_t* z);
int psacx_repeats_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA,
                      const uint64_t* LCP, uint32_t kind, uint64_t min_len, uint64_t min_occ, uint64_t max_occ, uint64_t* lb, uint64_t* ub,
                      uint64_t* len, uint64_t cap, uint64_t* z);

/* maximal exact matches ------------------------------------------------------------------
 * The maximal exact matches (MEMs) of a batch of patterns against the indexed text: the seeds of read mapping and the anchors of
 * genome alignment (MUMmer, essaMEM, BWA-MEM).  They follow from the matching statistics of psacx_match_dev_* by walking the
 * LCP-intervals that enclose each slot's interval, with the BWT for the left side.  No text is read.  The reference has no
 * counterpart.  One GPU.
 *
 * Setting, as for the repeats above.  One text S[0..n), or a string set whose suffix i is S[i..end(i)).  L[r] = LCP[r], with L[0]
 * and L[n] read as 0.  Ranks are SA indices.  Patterns are pat / poff as for psacx_match_dev_*; a slot p in [0, poff[q]) is a byte
 * of the pattern buffer and belongs to the pattern j with poff[j] <= p < poff[j+1].
 *
 * A MEM is a triple (p, t, l) with l >= max(min_len, 1) and pat[p..p+l) == S[t..t+l), where
 *  - the match lies inside pattern j and inside the string of t;
 *  - it is not right-extensible: p + l == poff[j+1], or t + l == end(t), or the next bytes differ;
 *  - it is not left-extensible: p == poff[j], or t starts a string, or pat[p-1] != S[t-1];
 *  - with max_occ > 0, pat[p..p+l) has at most max_occ occurrences (the size of its locate interval); max_occ == 1 gives the matches
 *    that are unique in the indexed text;
 *  - with PSACX_MEMS_SUPER, only MEMs whose pattern range [p, p+l) is contained in no other MEM's range of the same pattern are kept
 *    (SMEMs).  These are exactly the triples (p, SA[r], len_p) for r in [lb_p, ub_p) of the slots with p == poff[j] or
 *    len_{p-1} <= len_p, under the same min_len / max_occ filters; they need no left-character test.
 *
 * From the statistics (len_p, lb_p, ub_p) of slot p, uncapped (max_len == 0):
 *  - Shell 0 is [lb_p, ub_p) with l = len_p.
 *  - The next shell has l' = max(L[lb], L[ub]), which is < l.  Its interval is lb' = the largest x <= lb with L[x] < l' and
 *    ub' = the smallest y >= ub with L[y] < l', or n.  Its ranks are [lb', lb) and [ub, ub').
 *  - Every rank of a shell matches pat[p..] in exactly that shell's l bytes and is right-maximal.
 *  - The walk ends at the first shell with l < max(min_len, 1), or with max_occ > 0 and ub' - lb' > max_occ.  That shell is not
 *    counted as walked.
 *  - A rank r of a shell is a candidate.  It is a MEM iff p == poff[j], or bit r of `first` is set, or bwt[r] != pat[p-1].
 *
 * Output order, pinned: ascending slot; inside a slot descending l; inside a shell ascending rank.
 *
 * psacx_mems_dev_*: d_index is the index of psacx_rmq_index_dev_* over d_LCP; d_bwt / d_first are the outputs of psacx_bwt_dev_*;
 * d_mlen / d_mlb / d_mub are the three outputs of psacx_match_dev_* or psacx_match_gsa_dev_* with PSACX_MATCH_SUFFIXES and
 * max_len == 0, poff[q] entries each.
 *  - Output: z triples, d_qpos (the slot), d_tpos = SA[r] and d_len (index type).
 *  - d_qpos == NULL is the count query; d_tpos and d_len must then be NULL too, and none of them otherwise (PSACX_EINVAL).
 *  - z > cap returns PSACX_ERANGE with *z valid and nothing written to the lists.  *z is always set.
 *  - Unknown flag bits return PSACX_EINVAL.  poff[0] != 0 or a descending pair returns PSACX_EINVAL, found on the device before any
 *    result is written.  q == 0 or n == 0 gives z = 0.  n beyond the index type, or beyond 2^48, returns PSACX_ERANGE.
 *  - min_len 0 and 1 mean the same.
 *  - work may be NULL.  Otherwise work[0] is the number of shells walked and work[1] the number of candidates tested; with
 *    PSACX_MEMS_SUPER, the slots kept and their ranks.  Both are functions of the inputs alone: max_occ bounds the work, not only
 *    the output.
 *  - With PSACX_MEMS_SUPER neither d_LCP, d_index, d_bwt, d_first nor d_pat is read, and each may be NULL.  The count query does not
 *    read d_SA.
 *  - Totality, whatever the arrays hold: nothing is read or written out of range (d_first inside its (n >> 5) + 1 words); every walk
 *    ends, since a step that does not strictly lower l ends it; a statistics entry with lb >= ub or ub > n gives no shell; d_mlen is
 *    cut to the rest of the pattern, so every triple has l >= 1 and p + l <= poff[j+1]; tpos is the SA entry as it is.  No input is
 *    written.
 *  - Sixteen lanes per slot walk the shells, twice: once to count, once to write the shell records.  The candidates are then tested
 *    by workgroups that own 1024 candidate numbers each, whatever the shells are, so a slot with millions of candidates is spread
 *    over as many workgroups as it fills; one bwt byte and one bit of `first` per candidate, one SA entry per MEM.
 *  - Scratch.  In the ctx slab, with s = poff[q] + 1: the shell and candidate counts per slot, 2 * 8 s bytes (8 s + 8 with
 *    PSACX_MEMS_SUPER), behind the block sums of the scans, 8 bytes per 4096 of s beyond 4 KiB; each part rounded up to 256 bytes.
 *    Beside the slab and for the time of the call, with h shells, c candidates and t = ceil(c / 1024): the shell records,
 *    4 h entries of the index type and 8 h bytes; their candidate starts, 8 (h + 1); the mark bytes, 1024 t; the tile counts,
 *    8 (t + 1).  Where that fails the call returns PSACX_ENOMEM and the outputs are untouched.  PSACX_MEMS_SUPER allocates nothing
 *    beside the slab.  The count query runs everything but the last kernel.
 * psacx_mems_*: the host-pointer form.  offsets == NULL means one text (m is ignored); otherwise the m + 1 offsets of the strings,
 * which must start at 0, end at n and ascend strictly (PSACX_EINVAL).  It stages the arrays, builds the bitmap of the string ends,
 * the table when k > 0, the statistics, the index and the BWT, calls the device form and frees what it allocated on every path.
 * qpos == NULL is the count query, z > cap returns PSACX_ERANGE with *z valid. */
#define PSACX_MEMS_SUPER 1u
int psacx_mems_dev_u32(psacx_ctx* ctx, uint64_t n, const uint32_t* d_SA, const uint32_t* d_LCP, const uint32_t* d_index,
                       const uint8_t* d_bwt, const uint32_t* d_first, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                       const uint32_t* d_mlen, const uint32_t* d_mlb, const uint32_t* d_mub, uint64_t min_len, uint64_t max_occ,
                       uint32_t flags, uint64_t* d_qpos, uint32_t* d_tpos, uint32_t* d_len, uint64_t cap, uint64_t* z, uint64_t* work);
int psacx_mems_dev_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* d_SA, const uint64_t* d_LCP, const uint64_t* d_index,
                       const uint8_t* d_bwt, const uint32_t* d_first, const uint8_t* d_pat, const uint64_t* d_poff, uint64_t q,
                       const uint64_t* d_mlen, const uint64_t* d_mlb, const uint64_t* d_mub, uint64_t min_len, uint64_t max_occ,
                       uint32_t flags, uint64_t* d_qpos, uint64_t* d_tpos, uint64_t* d_len, uint64_t cap, uint64_t* z, uint64_t* work);
int psacx_mems_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA,
                   const uint32_t* LCP, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint64_t min_len,
                   uint64_t max_occ, uint32_t flags, uint64_t* qpos, uint32_t* tpos, uint32_t* len, uint64_t cap, uint64_t* z);
int psacx_mems_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA,
                   const uint64_t* LCP, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint64_t min_len,
                   uint64_t max_occ, uint32_t flags, uint64_t* qpos, uint64_t* tpos, uint64_t* len, uint64_t cap, uint64_t* z);

/* pattern search with mismatches ----------------------------------------------------------
 * Where a pattern occurs in the indexed text with at most e substituted bytes (Hamming distance): what a read mapper does with the
 * seeds of the calls above.  The pattern is cut into e + 1 pieces, one of which must occur exactly (pigeonhole); the pieces are
 * searched by the pattern search, and every occurrence of a piece is verified against the text.  No insertions or deletions.  The
 * reference has no counterpart.  One GPU.
 *
 * Setting, as for psacx_locate_dev_* and psacx_locate_gsa_dev_*.  One text S[0..n), or a string set whose suffix i is S[i..end(i));
 * for a set, d_ends is the bitmap of psacx_string_ends_dev.  Patterns are pat / poff as for psacx_locate_dev_*.  e is the number of
 * mismatches allowed, 0 <= e <= 15 (PSACX_EINVAL above).
 *
 * A hit is a triple (j, t, d) where
 *  - pattern j has m_j bytes and t + m_j <= n;
 *  - the window [t, t + m_j) lies inside one string: for a set, no bit of d_ends is set at t + 1 .. t + m_j - 1;
 *  - d = #{ x < m_j : pat[poff[j] + x] != S[t + x] } <= e.
 * A pattern with m_j < e + 1 has no hits (every window would be one) and owns no candidate.
 *
 * Pieces.  Pattern j is cut at b_i = floor(i m_j / (e + 1)), i = 0 .. e + 1: e + 1 non-empty pieces that tile it.  The boundaries of
 * all patterns are a valid offset array of q (e + 1) patterns over the same pattern buffer, and the pieces are searched as
 * psacx_locate_dev_* (with d_ends: psacx_locate_gsa_dev_*) searches them; with a table, a piece of at most k bytes takes no search.
 *
 * Candidates.  Every rank r of the interval of piece i of pattern j is a candidate, with s = SA[r] and t = s - b_i.  It is tested iff
 * s >= b_i, s < n, t + m_j <= n and the window lies inside one string.  It is a hit iff d <= e and each of the pieces 0 .. i - 1 has
 * at least one mismatch at this alignment: every hit has an exact piece, and it is reported from its first one, exactly once.
 *
 * Output order, pinned: ascending pattern; inside a pattern ascending piece; inside a piece ascending rank.
 *
 * psacx_kmismatch_dev_*: d_table / k / code as for psacx_locate_dev_*: the table of psacx_lookup_table_dev_*, or with d_ends that of
 * psacx_lookup_table_gsa_dev_*, with its k and code[], or NULL, 0, NULL; any other mix returns PSACX_EINVAL.
 *  - Output: z triples, d_qid (the pattern, uint64), d_tpos = t (index type) and d_dist = d (uint8).
 *  - d_qid == NULL is the count query; d_tpos and d_dist must then be NULL too, and none of them otherwise (PSACX_EINVAL).
 *  - z > cap returns PSACX_ERANGE with *z valid and nothing written to the lists.  *z is always set.
 *  - work may be NULL.  Otherwise work[0] is the number of candidates and work[1] the number tested.  Both are functions of the
 *    inputs alone.
 *  - With max_cand > 0 and work[0] > max_cand the call returns PSACX_ERANGE before anything sized by the candidates is allocated;
 *    *z = 0 and work[0] is valid.  A pattern of a repeat can own n candidates per piece: this is the guard.
 *  - poff[0] != 0 or a descending pair returns PSACX_EINVAL, found on the device before any result is written.  q == 0 or n == 0
 *    gives z = 0.  n beyond the index type returns PSACX_ERANGE.
 *  - Totality, whatever SA and table hold: nothing is read or written out of range (d_ends inside its (n >> 5) + 1 words); every
 *    triple reported is a true hit with exactly that d, because the verification reads the text and not the index; completeness
 *    and the pinned order need a correct SA (and table).  No input is written.
 *  - Workgroups own 1024 candidate numbers each, whatever the pieces are, so a piece with millions of occurrences is spread over as
 *    many workgroups as it fills; one lane per candidate fetches SA[r] and compares 8 bytes per step until a piece before its own
 *    is exact or d exceeds e; one mark byte per candidate carries the hit and its d into the ordered compaction.
 *  - Scratch.  The ctx slab holds only the three words of the searches and the block sums of the scans, 8 bytes per 4096 entries
 *    beyond 4 KiB.  Beside the slab and for the time of the call, with Q = q (e + 1), c candidates and t = ceil(c / 1024): one block
 *    of the piece offsets, 8 (Q + 1) bytes, the candidate starts, 8 (Q + 1), one word for work[1] and the piece intervals, 2 Q
 *    entries of the index type; and, once c is known and has passed max_cand, one block of the mark bytes, 1024 t, and the tile
 *    counts, 8 (t + 1); each part rounded up to 256 bytes.  Where that fails the call returns PSACX_ENOMEM and the outputs are
 *    untouched.  The count query runs everything but the last kernel.
 * psacx_kmismatch_*: the host-pointer form.  offsets == NULL means one text (m is ignored); otherwise the m + 1 offsets of the
 * strings, which must start at 0, end at n and ascend strictly (PSACX_EINVAL).  It stages the arrays, builds the bitmap of the string
 * ends and the table when k > 0, calls the device form and frees what it allocated on every path.  qid == NULL is the count query,
 * z > cap returns PSACX_ERANGE with *z valid. */
int psacx_kmismatch_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint32_t* d_SA,
                            const uint32_t* d_table, uint32_t k, const uint16_t code[256], const uint8_t* d_pat, const uint64_t* d_poff,
                            uint64_t q, uint32_t e, uint64_t max_cand, uint64_t* d_qid, uint32_t* d_tpos, uint8_t* d_dist, uint64_t cap,
                            uint64_t* z, uint64_t* work);
int psacx_kmismatch_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint64_t* d_SA,
                            const uint64_t* d_table, uint32_t k, const uint16_t code[256], const uint8_t* d_pat, const uint64_t* d_poff,
                            uint64_t q, uint32_t e, uint64_t max_cand, uint64_t* d_qid, uint64_t* d_tpos, uint8_t* d_dist, uint64_t cap,
                            uint64_t* z, uint64_t* work);
int psacx_kmismatch_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA,
                        const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint32_t e, uint64_t max_cand, uint64_t* qid,
                        uint32_t* tpos, uint8_t* dist, uint64_t cap, uint64_t* z);
int psacx_kmismatch_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA,
                        const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint32_t e, uint64_t max_cand, uint64_t* qid,
                        uint64_t* tpos, uint8_t* dist, uint64_t cap, uint64_t* z);

/* pattern search with edits ---------------------------------------------------------------
 * Where a pattern occurs in the indexed text within edit distance e (unit-cost Levenshtein distance: substitutions, insertions and
 * deletions), which psacx_kmismatch_* does not answer: one inserted or deleted byte costs it every hit behind it.  The reference
 * has no counterpart.  One GPU.
 *
 * Setting, as for psacx_kmismatch_dev_*.  One text S[0..n), or a string set whose suffix i is S[i..end(i)); for a set, d_ends is the
 * bitmap of psacx_string_ends_dev.  Patterns are pat / poff.  0 <= e <= 15 (PSACX_EINVAL above).
 *
 * For pattern j (m_j bytes) and a start t < n let
 *     D(j, t) = min over 0 <= L <= end(t) - t of ed(P_j, S[t .. t + L))   and   L(j, t) = the smallest L that attains it.
 * A hit is a quadruple (j, t, L(j, t), D(j, t)) with D(j, t) <= e.  The match lies inside one string: L never passes end(t).  A
 * pattern with m_j <= e has no hits (every start would be one) and owns no candidate, as for psacx_kmismatch_*.  Every hit is
 * reported exactly once, in ascending pattern, then ascending t.  With e = 0 the hits are the occurrences of the pattern, sorted by
 * position.  An exact occurrence at t brings the neighbouring starts along at distances 1 .. e: PSACX_KEDIT_BEST in flags keeps,
 * for every pattern, only the hits whose distance is the smallest among that pattern's hits, in the same order.  Unknown flag bits
 * return PSACX_EINVAL.
 *
 * Pieces and candidates are those of psacx_kmismatch_dev_*: pattern j is cut at b_i = floor(i m_j / (e + 1)), the pieces are searched
 * exactly, and rank r of piece i is a candidate with s = SA[r] and diagonal t0 = s - b_i.  An alignment with at most e edits leaves
 * one piece unedited (pigeonhole), and that piece lies off its diagonal by at most the number of insertions and deletions before it,
 * so the starts examined for a candidate are t in [max(start of s's string, t0 - e), min(s, t0 + e)], at most 2e + 1.  D <= e
 * implies L <= m_j + e, so the text up to min(end(t), t + m_j + e) decides D and L whenever D <= e: two candidates that reach the same
 * (j, t) agree, and the raw hits (candidate, start) become the hits by a plain unique.
 *
 * psacx_kedit_dev_*: d_table / k / code as for psacx_kmismatch_dev_*; any other mix returns PSACX_EINVAL.
 *  - Output: z quadruples, d_qid (the pattern, uint64), d_tpos = t and d_len = L (index type) and d_dist = D (uint8).
 *  - d_qid == NULL is the count query; all four lists must be NULL, or none of them (PSACX_EINVAL).
 *  - z > cap returns PSACX_ERANGE with *z valid and nothing written to the lists.  *z is always set.
 *  - work may be NULL.  Otherwise work[0] is the number of candidates and work[1] the number of raw hits before the unique.  Both
 *    are functions of the inputs alone.
 *  - With max_cand > 0 and work[0] > max_cand the call returns PSACX_ERANGE before anything sized by the candidates is allocated;
 *    *z = 0 and work[0] is valid.  Memory sized by the raw hits is allocated only once they are counted.
 *  - poff[0] != 0 or a descending pair returns PSACX_EINVAL, found on the device before any result is written.  q == 0 or n == 0
 *    gives z = 0.  n beyond the index type returns PSACX_ERANGE, and so does q >= 2^32 with the 32-bit index type (the pattern
 *    number is a key word of the sort).
 *  - Totality, whatever SA and table hold: nothing is read or written out of range (d_ends inside its (n >> 5) + 1 words); every
 *    quadruple reported is a true hit with exactly that L and D, because the verification reads the text and not the index;
 *    completeness and the order need a correct SA (and table); every hit is reported once regardless.  No input is written.
 *  - Workgroups own 1024 candidate numbers each, whatever the pieces are.  One lane per candidate fetches SA[r] and runs one
 *    right-to-left pass of the edit-distance recurrence with a free end over the band of the 4 EB + 1 diagonals around t0, EB >= e
 *    one of 1, 2, 4, 8, 15 at compile time, so the band is registers; the lane leaves when every cell of its row exceeds e.  The
 *    result is a mask of the starts with D <= e.  The raw pairs (j, t) are sorted by the rank-pair sort, equal neighbours dropped by
 *    the ordered compaction, and a forward pass over the distinct pairs alone gives L and D.
 *  - Scratch.  The ctx slab holds the three words of the searches and the block sums of the scans at its base and, between two of
 *    the scans, the buffers of the rank-pair sort over the raw hits (the statistics of the context are not touched by it).  Beside the slab and for the time of the call, with
 *    Q = q (e + 1), c candidates, r raw hits and u distinct hits: the piece offsets and candidate starts, 16 (Q + 1) bytes, and the
 *    piece intervals, 2 Q entries; once c has passed max_cand, a mask and a count per candidate, 12 c + 8; once r is counted, two
 *    entries, a mark byte and 8 / 1024 bytes of tile counts per raw hit; with PSACX_KEDIT_BEST 9 bytes, two entries and a mark byte
 *    per distinct hit and 4 q.  Each part is rounded up to 256 bytes.  Where that fails the call returns PSACX_ENOMEM and the
 *    outputs are untouched.
 * psacx_kedit_*: the host-pointer form, as psacx_kmismatch_* is that of psacx_kmismatch_dev_*: offsets == NULL means one text (m is
 * ignored); it stages the arrays, builds the bitmap and the table when k > 0, calls the device form and frees what it allocated on
 * every path.  qid == NULL is the count query, z > cap returns PSACX_ERANGE with *z valid. */
#define PSACX_KEDIT_BEST 1u
int psacx_kedit_dev_u32(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint32_t* d_SA,
                        const uint32_t* d_table, uint32_t k, const uint16_t code[256], const uint8_t* d_pat, const uint64_t* d_poff,
                        uint64_t q, uint32_t e, uint64_t max_cand, uint32_t flags, uint64_t* d_qid, uint32_t* d_tpos, uint32_t* d_len,
                        uint8_t* d_dist, uint64_t cap, uint64_t* z, uint64_t* work);
int psacx_kedit_dev_u64(psacx_ctx* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_ends, const uint64_t* d_SA,
                        const uint64_t* d_table, uint32_t k, const uint16_t code[256], const uint8_t* d_pat, const uint64_t* d_poff,
                        uint64_t q, uint32_t e, uint64_t max_cand, uint32_t flags, uint64_t* d_qid, uint64_t* d_tpos, uint64_t* d_len,
                        uint8_t* d_dist, uint64_t cap, uint64_t* z, uint64_t* work);
int psacx_kedit_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA,
                    const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint32_t e, uint64_t max_cand, uint32_t flags,
                    uint64_t* qid, uint32_t* tpos, uint32_t* len, uint8_t* dist, uint64_t cap, uint64_t* z);
int psacx_kedit_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA,
                    const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t k, uint32_t e, uint64_t max_cand, uint32_t flags,
                    uint64_t* qid, uint64_t* tpos, uint64_t* len, uint8_t* dist, uint64_t cap, uint64_t* z);

/* document counts and document lists ------------------------------------------------------
 * In how many strings of a set, and in which, the suffixes of an interval [lb, ub) of the generalized suffix array start: the
 * document frequency of a pattern, a repeat or a seed, and each string once however often it repeats the pattern, which
 * psacx_occurrences_dev_* (one entry per occurrence) does not give.  The reference has no counterpart.  One GPU.
 *
 * Setting, as for psacx_repeats_dev_* over a set: m strings back to back, offsets[0..m], SA and LCP as psacx_construct_gsa_dev_*
 * leaves them: suffixes end with their strings, equal suffixes stand in text order, LCP is cut at string ends.  L[r] = LCP[r] with
 * L[0] read as 0.  doc(r) is the string that holds SA[r]: the largest s < m with offsets[s] <= SA[r], searched and never trusted, as
 * in psacx_occurrences_dev_*.  "All ones" is the largest value of the index type.
 *
 * Index, two arrays:
 *     prev[r], n entries: the largest p < r with doc(p) == doc(r), or all ones if there is none;
 *     dup[i], n + 1 entries: dup[i] = sum over x < i of h[x], where h[x] counts the ranks r with p = prev[r] not all ones whose FIRST
 *     minimum of L[p+1 .. r] (both ends included) lies at x: the arg rule of psacx_rmq_dev_*.  h[0] = 0 and dup[n] = n - (the number of
 *     strings that own a rank).
 *
 * Counts.  For an LCP-interval the number of distinct strings is
 *     docs(lb, ub) = (ub - lb) - (dup[ub] - dup[lb + 1]).
 * An LCP-interval has lb < ub <= n and, with l = min L[lb+1 .. ub-1] (all ones if ub == lb + 1), (lb == 0 or L[lb] < l) and (ub == n or
 * L[ub] < l).  This is Hui's counting of duplicate pairs at their lowest common ancestor: a pair (p, r) with both ends inside has its
 * minimum strictly inside (lb, ub), a pair with one end outside crosses a boundary value that is strictly smaller, so its first minimum
 * lies at or outside a boundary.  Every singleton and [0, n) are LCP-intervals, and so is every non-empty interval that psacx_locate_gsa_* /
 * psacx_match_gsa_* / psacx_repeats_* / psacx_mems_* return.  The intervals of psacx_overlaps_dev_* are NOT: their right boundary
 * equals the inner value, and the formula may count a pair that crosses it.  Callers with such intervals, or with arbitrary ones, use
 * the list call, whose total is exact for any interval.
 *
 * Lists.  For ANY interval [lb, ub) with lb <= ub <= n, the ranks r in it with prev[r] < lb or prev[r] all ones are the first
 * occurrence of each string in the interval; the list holds them in ascending r.
 *
 * psacx_doc_index_dev_*: d_index is the index of psacx_rmq_index_dev_* over d_LCP.
 *  - d_prev or d_dup may be NULL (d_LCP and d_index are not read without d_dup); both NULL returns PSACX_EINVAL.
 *  - n == 0 is PSACX_OK; otherwise m == 0 or m > n returns PSACX_EINVAL.  n beyond the index type or beyond 2^48 returns PSACX_ERANGE.
 *  - No input is written.  An SA entry >= n counts for the last string (the search of the offsets decides, nothing is read out of range).
 *  - Stages: one key (doc(r), r) per rank, one lane each, by a binary search over the offsets; the rank-pair sort on the bits of m - 1 of
 *    the first word (stable; the ranks of a string stay in order); prev scattered from neighbours of equal doc, where an adjacent pair
 *    (p = r - 1) adds to h[r] without a search; every other pair runs the range-minimum search over L[p+1 .. r] on sixteen lanes and one
 *    lane adds to h[x] by an atomic; the exclusive scan of h in d_dup.
 *  - Scratch.  The ctx slab holds the buffers of the rank-pair sort and then the block sums of the scan.  Beside the slab and for the
 *    time of the call: the two key words, 2 n entries.  Where that fails the call returns PSACX_ENOMEM and the outputs are untouched.
 *  - After psacx_profile(ctx, 1) the call leaves the times of its stages in psacx_stats: ms_kmer the keys, ms_sort_scatter the sort,
 *    ms_rebucket prev and the pairs, ms_finalize the scan (tools/doc_time.py).
 * psacx_doc_count_dev_*: one interval per lane, two fetches.  docs_j = 0 unless lb_j < ub_j <= n; otherwise
 *     docs_j = (ub - lb) - min(sat(dup[ub] - dup[lb+1]), ub - lb - 1),   sat = the difference, or 0 if it is negative.
 *  - Totality: whatever dup holds, 1 <= docs_j <= ub - lb, and nothing is read outside its n + 1 entries.
 *  - Nothing is allocated.  q == 0 is PSACX_OK.
 * psacx_doc_list_dev_*: d_start receives q + 1 exclusive prefix sums (64 bits) of the list lengths, start[q] = *total;
 * sid[start_j + t] = doc(r_t) and pos[start_j + t] = SA[r_t] for the t-th listed rank of interval j.
 *  - d_sid == NULL (then d_pos must be NULL, PSACX_EINVAL otherwise) is the size query.  d_pos may be NULL on its own.
 *  - *total > cap returns PSACX_ERANGE with start and *total valid and nothing written to the lists.  *total is always set.
 *  - Intervals that are not lb_j <= ub_j <= n count 0.
 *  - Candidates are the ranks of all intervals.  With max_cand > 0 and more candidates the call returns PSACX_ERANGE before anything sized
 *    by them is allocated, with *total = 0 and start untouched (the convention of psacx_kmismatch_dev_*).
 *  - Workgroups own 1024 candidates each, whatever the intervals are: one prev fetch and one mark byte per candidate, then the ordered
 *    compaction; the listed ranks fetch SA and search the offsets.
 *  - Totality: a prev entry that is garbage only changes which ranks are listed.  SA entries >= n give sid = m, as in
 *    psacx_occurrences_dev_*.  Nothing is read or written out of range; no input is written.
 *  - Scratch.  The ctx slab holds the block sums of the scans.  Beside the slab and for the time of the call: 8 (q + 1) bytes of candidate
 *    starts and, once the candidates have passed max_cand, per tile of 1024 candidates 1024 mark bytes, 8 bytes of tile counts and 64 of
 *    run counts.  Where that fails the call returns PSACX_ENOMEM and the outputs are untouched.
 * psacx_doc_count_* / psacx_doc_list_*: the host-pointer forms.  They stage the arrays, check the offsets as psacx_repeats_* does
 * (PSACX_EINVAL), build the range-minimum index (the count) and the doc index, call the device forms and free what they allocated on
 * every path.  psacx_doc_list_* needs no LCP; sid == NULL is the size query, *total > cap returns PSACX_ERANGE with start and *total
 * valid. */
int psacx_doc_index_dev_u32(psacx_ctx* ctx, uint64_t n, const uint64_t* d_offsets, uint64_t m, const uint32_t* d_SA, const uint32_t* d_LCP,
                            const uint32_t* d_index, uint32_t* d_prev, uint32_t* d_dup);
int psacx_doc_index_dev_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* d_offsets, uint64_t m, const uint64_t* d_SA, const uint64_t* d_LCP,
                            const uint64_t* d_index, uint64_t* d_prev, uint64_t* d_dup);
int psacx_doc_count_dev_u32(psacx_ctx* ctx, uint64_t n, const uint32_t* d_dup, const uint32_t* d_lb, const uint32_t* d_ub, uint64_t q,
                            uint32_t* d_docs);
int psacx_doc_count_dev_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* d_dup, const uint64_t* d_lb, const uint64_t* d_ub, uint64_t q,
                            uint64_t* d_docs);
int psacx_doc_list_dev_u32(psacx_ctx* ctx, const uint32_t* d_SA, uint64_t n, const uint64_t* d_offsets, uint64_t m, const uint32_t* d_prev,
                           const uint32_t* d_lb, const uint32_t* d_ub, uint64_t q, uint64_t max_cand, uint64_t* d_start, uint32_t* d_sid,
                           uint32_t* d_pos, uint64_t cap, uint64_t* total);
int psacx_doc_list_dev_u64(psacx_ctx* ctx, const uint64_t* d_SA, uint64_t n, const uint64_t* d_offsets, uint64_t m, const uint64_t* d_prev,
                           const uint64_t* d_lb, const uint64_t* d_ub, uint64_t q, uint64_t max_cand, uint64_t* d_start, uint64_t* d_sid,
                           uint64_t* d_pos, uint64_t cap, uint64_t* total);
int psacx_doc_count_u32(psacx_ctx* ctx, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA, const uint32_t* LCP,
                        const uint32_t* lb, const uint32_t* ub, uint64_t q, uint32_t* docs);
int psacx_doc_count_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA, const uint64_t* LCP,
                        const uint64_t* lb, const uint64_t* ub, uint64_t q, uint64_t* docs);
int psacx_doc_list_u32(psacx_ctx* ctx, const uint32_t* SA, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* lb,
                       const uint32_t* ub, uint64_t q, uint64_t max_cand, uint64_t* start, uint32_t* sid, uint32_t* pos, uint64_t cap,
                       uint64_t* total);
int psacx_doc_list_u64(psacx_ctx* ctx, const uint64_t* SA, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* lb,
                       const uint64_t* ub, uint64_t q, uint64_t max_cand, uint64_t* start, uint64_t* sid, uint64_t* pos, uint64_t cap,
                       uint64_t* total);

/* FM-index ---------------------------------------------------------------------------------
 * A compressed full-text index: backward search on the Burrows-Wheeler transform counts patterns without text or suffix array, and a
 * sampled suffix array gives their positions.  After the build the caller may free text and SA and keep the index, a fraction of
 * their size.  The reference has no counterpart.  One GPU.
 *
 * Setting, as for psacx_bwt_dev_*: one text S[0..n), or m strings back to back.  bwt and first are exactly what psacx_bwt_dev_* writes:
 * cyclic per string, first[r] set iff SA[r] starts a string.  One text is a set of one string and passes its first bitmap too.
 *
 * Symbols.  code[256] maps the bytes that occur to 1 .. sigma in byte order; bytes that do not occur are coded 0.  Code 0 is also the
 * STOP symbol: w[r] = 0 if first[r], else code[bwt[r]].  bits = ceil(log2(sigma + 1)), from 1 to 9: with sigma = 256 the codes need 9
 * bits and do not fit a byte.
 * Counts.  cnt[c] = the ranks r with code[S[SA[r]]] == c (the text bytes of code c); C[c] = the sum of cnt[d] over d < c;
 * E[c] = the strings whose last byte has code c = #{r : first[r] and code[bwt[r]] == c}.
 * LF.  For a rank r with w[r] = c != 0: LF(r) = C[c] + E[c] + rank_c(r), rank_c(r) = #{x < r : w[x] == c}; then SA[LF(r)] = SA[r] - 1.
 * The E[c] suffixes that are the last byte of a string alone have no predecessor rank and are the smallest suffixes that start with c;
 * without E[c], "iss" in mississippi comes out as [1, 3) instead of [2, 4).
 * Backward search of P[0..L).  L == 0 gives [0, n).  A byte coded 0 gives a miss.  The FIRST step, on the last byte c, is
 * [C[c], C[c] + cnt[c]): pushing [0, n) through LF would lose the E[c] one-byte suffixes ("ippi" would miss).  Every further step maps
 * both bounds by C[c] + E[c] + rank_c(.).  An empty interval ends the search.
 * Result.  For a pattern that occurs (inside one string) the result is exactly the interval of psacx_locate_dev_* /
 * psacx_locate_gsa_dev_*.  A miss is pinned to lb = ub = 0: this is NOT locate's insertion point.  STOP makes matches across two
 * strings impossible without any bitmap test.
 * Samples.  With a sample rate s >= 1, rank r is marked iff first[r] or SA[r] % s == 0, and val[rank_marks(r)] = SA[r], entries of the
 * index type.  From any rank fewer than s LF steps reach a marked rank x, and SA[r] = val[rank_marks(x)] + steps.  s == 0: no samples,
 * the index counts only.
 *
 * The index is one opaque array of 64-bit words in HBM and a host descriptor, psacx_fm_info, which the build fills and every query
 * takes back (the convention of code[256] / sigma of the lookup table).  With cells = (n >> 6) + 1 the blob holds, in this order: a
 * binary wavelet matrix over w, bits levels of cells cells of 16 bytes {ones in front of this cell, 64 bits}, most significant bit
 * first, so that one rank is one 16-byte load; 544 words of tables (the zeros per level, C, and C + E - the start of the symbol behind
 * the last level, so that a bound costs `bits` dependent cells and one add); with s > 0 the marks, cells cells of the same form, and val:
 *     words = 2 * bits * cells + 544 + (s ? 2 * cells : 0) + ceil(sizeof(T) * marks / 8),
 * at most 16 * bits * cells + 16 * cells [if s] + sizeof(T) * marks + 16 KiB bytes: 0.75 bytes per character for DNA counting (sigma 4
 * and STOP give 3 bits).  The layout may change between versions of the library; a blob is not a file format.
 *
 * psacx_fm_index_dev_*: d_SA is read only with sample > 0.  d_fm == NULL is the size query: it fills *info (words among it) and writes
 * nothing else; it reads d_bwt, d_first and, with sample > 0, d_SA.
 *  - n == 0 is PSACX_OK (an index whose every search misses).  n beyond the index type or beyond 2^48 returns PSACX_ERANGE.
 *  - d_first == NULL, info == NULL, d_bwt == NULL with n > 0, or sample > 0 with d_SA == NULL return PSACX_EINVAL.
 *  - Stages, all streaming: a histogram of the bytes and of the last bytes of the strings gives the codes and the tables; the codes w as
 *    16 bits; per level one ballot per wave gives the cell word and its count, the scan gives the directory, and a stable partition sends
 *    each code to bit ? Z + rank1(r) : r - rank1(r) of the next level's order; marks and val the same way.
 *  - Scratch.  The ctx slab holds the block sums of the scans, the histogram and one count per cell.  Beside the slab and for the time of
 *    the call: two arrays of n 16-bit codes.  Where that fails the call returns PSACX_ENOMEM with d_fm and *info untouched.
 *  - After psacx_profile(ctx, 1) the build leaves the times of its stages in psacx_stats: ms_kmer the histogram, the mark count and the
 *    codes, ms_sort_scatter the levels, ms_rebucket the marks and samples (tools/fm_time.py).
 * psacx_fm_count_dev_*: one pattern per lane, d_pat / d_poff as psacx_locate_dev_* takes them (malformed offsets: PSACX_EINVAL, nothing
 * written).  lb_j, ub_j as under "Result".  A descriptor whose bits / words do not follow from its n, sigma, sample and marks for this
 * index type, or with a code beyond sigma, returns PSACX_EINVAL.  q == 0 is PSACX_OK.
 * psacx_fm_occurrences_dev_*: the contract of psacx_occurrences_dev_* (limit; d_pos == NULL is the size query; *total > cap returns
 * PSACX_ERANGE with start and *total valid and the lists untouched; d_sid optional, with d_offsets), where SA[r] is replaced by the LF
 * walk from r to a marked rank.  An index built with sample == 0 returns PSACX_EINVAL.
 * Totality, whatever the blob holds: nothing is read outside its `words` words; every search ends after L steps; every walk ends after
 * at most min(sample, n) steps, and a walk that met no mark gives all ones (sid = m); every interval has 0 <= lb <= ub <= n; no input
 * is written.
 * psacx_fm_search_*: the host-pointer form.  It stages text and SA, builds the bitmap of the string ends (offsets == NULL: one text), the
 * BWT and the index, answers and frees what it allocated on every path.  lb / ub receive the intervals.  pos == NULL counts only (no
 * samples are built; start, sid, cap and total are not used).  With pos: start (q + 1 entries), total and sample > 0 are required,
 * *total > cap returns PSACX_ERANGE with lb, ub, start and *total valid.
 *
 * Text samples and extraction.  The blob replaces the suffix array; with the text samples beside it the index replaces the text too.
 * The samples are a second array and the blob is what it was without them.  With a rate t >= 1 and blocks = n / t:
 *     ts[k], k < blocks      = the rank of the suffix at position (k + 1) * t - 1 (the last position of block [k * t, (k + 1) * t));
 *     ts[blocks + j], j < m  = the rank of the suffix at the last byte of string j,
 * entries of the index type, blocks + max(m, 1) of them.  From the rank x of the suffix at position p the text to its left comes out
 * under LF: S[p] is the symbol c with C[c] <= x < C[c + 1], and then S[p - 1] = w[x], x = LF(x), and so on.  w is STOP at the ranks of
 * string starts, so a walk can not be entered from the next string: hence one sample per string end.
 * psacx_fm_text_samples_dev_*: one streaming pass over d_SA.  d_offsets == NULL means one text: m is read as 1, its end is n - 1.
 *  - d_ts == NULL is the size query: it sets *entries and reads nothing.  n == 0 is PSACX_OK and writes nothing.
 *  - rate == 0, entries == NULL, or with n > 0 and d_ts: d_SA == NULL, m == 0 or m > n return PSACX_EINVAL; offsets that do not start at
 *    0, end at n and ascend strictly return PSACX_EINVAL before anything is written (psacx_string_ends_dev); n beyond the index type
 *    returns PSACX_ERANGE.
 *  - An SA entry at or beyond n is skipped.  No input is written.  Scratch, for a string set only: the bitmap of the string ends in the
 *    ctx slab.
 * psacx_fm_extract_dev_*: query i asks for S[pos_i .. pos_i + len_i), clipped at the end of the string that holds pos_i; pos_i >= n
 * gives length 0.  d_start receives q + 1 entries, the prefix sums of the clipped lengths, d_out[d_start[i] ..) the bytes.  The contract
 * is that of psacx_fm_occurrences_dev_*: d_out == NULL is the size query; *total > cap returns PSACX_ERANGE with d_start and *total
 * valid and d_out untouched; q == 0 is PSACX_OK.  d_ts, rate, d_offsets and m are those of psacx_fm_text_samples_dev_*.
 *  - The descriptor is checked as by every query (PSACX_EINVAL); rate == 0, d_ts == NULL, or with q > 0 a NULL d_pos, d_len or d_start
 *    return PSACX_EINVAL; so do malformed offsets, before anything is written.
 *  - Work is balanced by output.  The unit is a segment, the part of one query's range inside one block [k * t, (k + 1) * t): a lane
 *    starts at the sample of the block's last position, or at the end sample of its string where that comes first, takes the head symbol
 *    from C and walks fewer than t LF steps to the left, storing the bytes whose position lies inside the query.  One query for a
 *    whole text runs as wide as a million short ones.
 *  - Scratch in the ctx slab: the block sums of the scans and q + 1 segment starts.
 *  - Totality, whatever the blob and d_ts hold: every sample is clamped to n before use; every walk ends after fewer than min(t, n)
 *    steps; nothing is read outside the `words` words of the blob or outside the `entries` entries of d_ts; nothing is written outside
 *    d_out[0 .. *total); a segment whose sample is n or heads no symbol, or that meets STOP, a code beyond sigma or a rank of n early,
 *    writes byte 0 for the positions it did not reach.  No input is written.
 * There is no host-pointer psacx_fm_extract_*: a call that takes the text in order to return it has no user. */
typedef struct psacx_fm_info {
    uint64_t n;            /* ranks */
    uint64_t words;        /* 64-bit words of the blob */
    uint64_t sample;       /* the sample rate s, 0 = counts only */
    uint64_t marks;        /* marked ranks = entries of val */
    uint32_t sigma;        /* distinct bytes */
    uint32_t bits;         /* levels of the wavelet matrix */
    uint16_t code[256];    /* byte -> 1 .. sigma, 0 = does not occur */
} psacx_fm_info;
int psacx_fm_index_dev_u32(psacx_ctx* ctx, uint64_t n, const uint8_t* d_bwt, const uint32_t* d_first, const uint32_t* d_SA, uint64_t sample,
                           uint64_t* d_fm, psacx_fm_info* info);
int psacx_fm_index_dev_u64(psacx_ctx* ctx, uint64_t n, const uint8_t* d_bwt, const uint32_t* d_first, const uint64_t* d_SA, uint64_t sample,
                           uint64_t* d_fm, psacx_fm_info* info);
int psacx_fm_count_dev_u32(psacx_ctx* ctx, const uint64_t* d_fm, const psacx_fm_info* info, const uint8_t* d_pat, const uint64_t* d_poff,
                           uint64_t q, uint32_t* d_lb, uint32_t* d_ub);
int psacx_fm_count_dev_u64(psacx_ctx* ctx, const uint64_t* d_fm, const psacx_fm_info* info, const uint8_t* d_pat, const uint64_t* d_poff,
                           uint64_t q, uint64_t* d_lb, uint64_t* d_ub);
int psacx_fm_occurrences_dev_u32(psacx_ctx* ctx, const uint64_t* d_fm, const psacx_fm_info* info, const uint64_t* d_offsets, uint64_t m,
                                 const uint32_t* d_lb, const uint32_t* d_ub, uint64_t q, uint64_t limit, uint64_t* d_start, uint32_t* d_pos,
                                 uint32_t* d_sid, uint64_t cap, uint64_t* total);
int psacx_fm_occurrences_dev_u64(psacx_ctx* ctx, const uint64_t* d_fm, const psacx_fm_info* info, const uint64_t* d_offsets, uint64_t m,
                                 const uint64_t* d_lb, const uint64_t* d_ub, uint64_t q, uint64_t limit, uint64_t* d_start, uint64_t* d_pos,
                                 uint64_t* d_sid, uint64_t cap, uint64_t* total);
int psacx_fm_text_samples_dev_u32(psacx_ctx* ctx, uint64_t n, const uint32_t* d_SA, const uint64_t* d_offsets, uint64_t m, uint64_t rate,
                                  uint32_t* d_ts, uint64_t* entries);
int psacx_fm_text_samples_dev_u64(psacx_ctx* ctx, uint64_t n, const uint64_t* d_SA, const uint64_t* d_offsets, uint64_t m, uint64_t rate,
                                  uint64_t* d_ts, uint64_t* entries);
int psacx_fm_extract_dev_u32(psacx_ctx* ctx, const uint64_t* d_fm, const psacx_fm_info* info, const uint32_t* d_ts, uint64_t rate,
                             const uint64_t* d_offsets, uint64_t m, const uint32_t* d_pos, const uint32_t* d_len, uint64_t q,
                             uint64_t* d_start, uint8_t* d_out, uint64_t cap, uint64_t* total);
int psacx_fm_extract_dev_u64(psacx_ctx* ctx, const uint64_t* d_fm, const psacx_fm_info* info, const uint64_t* d_ts, uint64_t rate,
                             const uint64_t* d_offsets, uint64_t m, const uint64_t* d_pos, const uint64_t* d_len, uint64_t q,
                             uint64_t* d_start, uint8_t* d_out, uint64_t cap, uint64_t* total);
int psacx_fm_search_u32(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint32_t* SA,
                        uint64_t sample, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint32_t* lb, uint32_t* ub, uint64_t limit,
                        uint64_t* start, uint32_t* pos, uint32_t* sid, uint64_t cap, uint64_t* total);
int psacx_fm_search_u64(psacx_ctx* ctx, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t m, const uint64_t* SA,
                        uint64_t sample, const uint8_t* pat, const uint64_t* poff, uint64_t q, uint64_t* lb, uint64_t* ub, uint64_t limit,
                        uint64_t* start, uint64_t* pos, uint64_t* sid, uint64_t cap, uint64_t* total);

/* several GPUs -------------------------------------------------------------------
 * The reference's suffix_array<> IS distributed: every MPI rank holds one block of the text and of SA / ISA / LCP
 * (suffix_array.hpp:183-194, :217-228; src/psac.cpp:85-93 block-decomposes the input).  A psacx_multi stands for the
 * communicator: nranks ranks, one GPU each, of which nlocal live in this process.
 *   psacx_multi_create       one process (one host thread) drives ndev GPUs: ranks 0..ndev-1 = dev_ids[0..ndev-1]
 *                            (NULL: devices 0..ndev-1).  Distinct devices share one RCCL communicator
 *                            (ncclCommInitAll); a device listed more than once carries several ranks that exchange
 *                            by device-to-device copies (how the tests run P ranks on a one-GPU box).
 *   psacx_multi_create_rank  one process per GPU, psac's own deployment (one MPI rank per device): every process
 *                            passes the same 128-byte id, made by psacx_multi_unique_id on one of them and
 *                            broadcast by the host (MPI_Bcast in psac, torch.distributed in bench.py).
 * Exchanges replace mxx's collectives: grouped ncclSend / ncclRecv for MPI_Alltoallv (idxsort.hpp:60-62 via
 * mxx::sort, bulk_permute.hpp:60-61, bulk_rma.hpp:20-49, par_rmq.hpp:273-293), one small all-gather for the
 * scalars (bucketing.hpp:39,70,117), on a second stream per GPU.
 * psacx_multi_construct_dev_*: d_text[i] / m[i] / d_SA[i] ... are the block of local rank i (device pointers on that
 * rank's GPU); the blocks must follow mxx::blk_dist (the first n mod p ranks hold one character more,
 * suffix_array.hpp:226-227: PSACX_EINVAL otherwise).  psacx_multi_construct_*: the whole text and results on the
 * host of the single process that owns every rank (psac --gpus N).
 * Errors: the codes above, -7 for an RCCL failure; psacx_multi_last_error gives the text. */
typedef struct psacx_multi psacx_multi;
int psacx_multi_create(psacx_multi** out, int ndev, const int* dev_ids);
int psacx_multi_unique_id(void* id128);
int psacx_multi_create_rank(psacx_multi** out, int rank, int nranks, int device, const void* id128);
void psacx_multi_destroy(psacx_multi* mg);
int psacx_multi_nranks(const psacx_multi* mg);
int psacx_multi_nlocal(const psacx_multi* mg);
int psacx_multi_uses_rccl(const psacx_multi* mg);
/* How the ranks reach each other: 0 = device-to-device copies inside one process (ranks may share a device), 1 = RCCL
 * (grouped ncclSend / ncclRecv + ncclAllGather, the replacement of mxx's MPI_Alltoallv / MPI_Allgather, idxsort.hpp:60-62,
 * bucketing.hpp:39), 2 = one process per rank on one host staged through POSIX shared memory: psacx_multi_create_rank
 * with PSACX_MULTI_TRANSPORT=shm in the environment -- psac's own deployment without a GPU-aware MPI (src/psac.cpp:85-93),
 * and the way two processes can share one GPU, which RCCL refuses.  id128 is then any 128 bytes all ranks agree on.
 * A communicator that cannot be built makes psacx_multi_create / _create_rank fail with -7; nothing falls back silently.
 * PSACX_MULTI_FORCE_WIRE=1 (test switch): data a rank addresses to itself and scalars that are already on this host still
 * travel through ncclSend / ncclRecv / ncclAllGather. */
int psacx_multi_transport(const psacx_multi* mg);
/* after a call: ncclSend / ncclRecv / ncclAllGather calls this process really issued, and exchange_ms[i] = time the
 * exchanges occupied local rank i's second stream (HIP events).  Any pointer may be null. */
int psacx_multi_get_wire(const psacx_multi* mg, uint64_t* sends, uint64_t* recvs, uint64_t* allgathers, double* exchange_ms);
/* host wall time of the phases of the last construction as "name=ms;name=ms;..." (the section timers of
 * suffix_array.hpp:52-63 for this engine); PSACX_ERANGE if buf is too small */
int psacx_multi_get_phases(const psacx_multi* mg, char* buf, uint64_t cap);
/* which forms the last construction took: bit 0 = first round in two-word form (records (B1, idx), ties repaired from the
 * text owners; idxsort.hpp:23-83 moves (B1, B2, idx)), bit 1 = reduced-memory layout, bit 2 = SA -> ISA slice by slice
 * through the destination-partition levels (bulk_permute.hpp:14-73),
 * bit 4 = first round in one-word records dealt to the ranks by the top digit of the prefix (8 bytes per record on the wire),
 * bits 8..15 = slabs beyond the first in which the ties of that round were ordered (reduced-memory layout, repetitive text: the
 * records of one slab at a time take the place of idxsort.hpp:41-45's whole second record set) */
int psacx_multi_last_form(const psacx_multi* mg);
const char* psacx_multi_last_error(const psacx_multi* mg);
psacx_ctx* psacx_multi_ctx(psacx_multi* mg, int local_rank);
int psacx_multi_construct_dev_u32(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, uint32_t k, uint32_t flags,
                                  uint32_t* const* d_SA, uint32_t* const* d_ISA, uint32_t* const* d_LCP);
int psacx_multi_construct_dev_u64(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, uint32_t k, uint32_t flags,
                                  uint64_t* const* d_SA, uint64_t* const* d_ISA, uint64_t* const* d_LCP);
int psacx_multi_construct_u32(psacx_multi* mg, const uint8_t* text, uint64_t n, uint32_t k, uint32_t flags, uint32_t* SA,
                              uint32_t* ISA, uint32_t* LCP);
int psacx_multi_construct_u64(psacx_multi* mg, const uint8_t* text, uint64_t n, uint32_t k, uint32_t flags, uint64_t* SA,
                              uint64_t* ISA, uint64_t* LCP);
/* Distributed verification of block-distributed results without gathering them on one rank: d_check_sa
 * (check_suffix_array.hpp:207-267: SA a permutation with inverse ISA, S[SA[i-1]] <= S[SA[i]], ties decided by the
 * ranks of the suffixes one further) through the engine's own exchanges, plus -- beyond the reference, whose
 * distributed checker leaves LCP out -- every LCP entry through the recurrence LCP[i] = 0 | 1 | 1 + min(LCP[ISA[SA[i-1]
 * +1]+1 .. ISA[SA[i]+1]]).  errors[0..3] as psacx_check_dev_*, summed over all ranks (every rank gets the totals).
 * d_LCP may be NULL.
 * Counted as by psacx_check_dev_* (errors[0] ends the examination of an entry; predecessor only if in range; the same
 * order test), with two differences: LCP is not examined at an entry that fails the order test, and errors[2] counts
 * the entries that break the recurrence over the arrays as given -- 0 if the first characters differ, 1 if
 * SA[i-1] + 1 == n, else 1 + the range minimum -- so one wrong LCP entry is usually counted at itself and at every
 * entry whose range minimum it was, and an LCP array raised everywhere is caught only where the recurrence is
 * anchored (the 0s and 1s).  An entry that passes the order test with ISA[SA[i]+1] >= n (two numbers that are no
 * ranks compared) counts in errors[2]; no range minimum is asked for it, so an ISA holding anything is safe to pass. */
int psacx_multi_check_dev_u32(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint32_t* const* d_SA,
                              const uint32_t* const* d_ISA, const uint32_t* const* d_LCP, uint64_t errors[4]);
int psacx_multi_check_dev_u64(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint64_t* const* d_SA,
                              const uint64_t* const* d_ISA, const uint64_t* const* d_LCP, uint64_t errors[4]);
/* The distributed checker for a generalized suffix array (psacx_multi_construct_gsa_dev_*: the strings back to back in the
 * block-distributed text, offsets = the nstr + 1 global string offsets on the host of every process).  Same exchanges, pieces and
 * range minima as psacx_multi_check_dev_*: the string ends travel in a spare bit of the text words.  Malformed offsets (not
 * starting at 0, not ending at n, an empty string, not ascending) return PSACX_EINVAL.  errors[0], errors[1] and errors[3] as
 * psacx_check_gsa_dev_* (src/gsac.cpp:85-135 is the reference's gathered counterpart, check_suffix_array.hpp:207-267 the scheme);
 * errors[2] is examined only where the order test passed and expects, with a = SA[i-1], b = SA[i]: 0 if S[a] != S[b]; 1 if
 * a + 1 == end(a) or b + 1 == end(b); otherwise 1 + min(LCP[ISA[a+1]+1 .. ISA[b+1]]) over the arrays as given.  An entry whose
 * order test passed with ISA[b+1] >= n counts in errors[2] and no range minimum is asked for it.  With nstr = 1 the verdict on
 * correct arrays equals psacx_multi_check_dev_*'s; on corrupt arrays it may differ (a repeated one-character suffix fails a < b). */
int psacx_multi_check_gsa_dev_u32(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint64_t* offsets, uint64_t nstr,
                                  const uint32_t* const* d_SA, const uint32_t* const* d_ISA, const uint32_t* const* d_LCP, uint64_t errors[4]);
int psacx_multi_check_gsa_dev_u64(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint64_t* offsets, uint64_t nstr,
                                  const uint64_t* const* d_SA, const uint64_t* const* d_ISA, const uint64_t* const* d_LCP, uint64_t errors[4]);
/* Left-branching characters of block-distributed results (suffix_array<char_t, index_t, true, true>::local_Lc on p ranks,
 * suffix_array.hpp:211-212; filled by :1365-1383 and par_rmq.hpp:334-481 in the reference; by definition
 * Lc[i] = S[SA[i-1] + LCP[i]], desa.hpp:262-264, '\0' past the end and at i = 0): d_Lc[i] receives m[i] bytes for the
 * block of local rank i.  SA and LCP as psacx_multi_construct_dev_* left them. */
/* the host-pointer form (psacx_multi_construct_* + Lc[0..n)): flags must carry PSACX_LCP */
int psacx_multi_construct_lc_u32(psacx_multi* mg, const uint8_t* text, uint64_t n, uint32_t k, uint32_t flags, uint32_t* SA,
                                 uint32_t* ISA, uint32_t* LCP, uint8_t* Lc);
int psacx_multi_construct_lc_u64(psacx_multi* mg, const uint8_t* text, uint64_t n, uint32_t k, uint32_t flags, uint64_t* SA,
                                 uint64_t* ISA, uint64_t* LCP, uint8_t* Lc);
int psacx_multi_left_chars_dev_u32(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint32_t* const* d_SA,
                                   const uint32_t* const* d_LCP, uint8_t* const* d_Lc);
int psacx_multi_left_chars_dev_u64(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint64_t* const* d_SA,
                                   const uint64_t* const* d_LCP, uint8_t* const* d_Lc);
/* ansv<T, left_type, right_type, global_indexing>(in, left_nsv, right_nsv, comm) (ansv.hpp:2042-2051) over a
 * block-distributed array (blocks as mxx::blk_dist, e.g. the LCP blocks psacx_multi_construct_dev_* left in HBM):
 * d_left[i] / d_right[i] receive, per element of local rank i's block, the GLOBAL index of its nearest smaller value on
 * that side (types as psacx_ansv_*), nonsv where there is none.  Device pointers; results are uint64. */
int psacx_multi_ansv_dev_u32(psacx_multi* mg, const uint32_t* const* d_in, const uint64_t* m, int left_type, int right_type,
                             uint64_t nonsv, uint64_t* const* d_left, uint64_t* const* d_right);
int psacx_multi_ansv_dev_u64(psacx_multi* mg, const uint64_t* const* d_in, const uint64_t* m, int left_type, int right_type,
                             uint64_t nonsv, uint64_t* const* d_left, uint64_t* const* d_right);
/* construct_ss (suffix_array.hpp:267-363: the generalized suffix array of a string set) on p ranks: the strings lie back to
 * back without separators in the block-distributed text (kmer.hpp:269-355 cuts every k-mer at its string's end,
 * shifting.hpp:374-418 answers "the suffix h further" with 0 beyond it, bucketing.hpp:130-143 the bucket rules); offsets =
 * the nstr + 1 ascending GLOBAL offsets of the strings (host array, the same on every rank; offsets[0] = 0,
 * offsets[nstr] = n, no empty string).  Results as psacx_construct_gsa_*, block-distributed as psacx_multi_construct_dev_*. */
int psacx_multi_construct_gsa_dev_u32(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint64_t* offsets, uint64_t nstr,
                                      uint32_t k, uint32_t flags, uint32_t* const* d_SA, uint32_t* const* d_ISA, uint32_t* const* d_LCP);
int psacx_multi_construct_gsa_dev_u64(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint64_t* offsets, uint64_t nstr,
                                      uint32_t k, uint32_t flags, uint64_t* const* d_SA, uint64_t* const* d_ISA, uint64_t* const* d_LCP);
/* the host-pointer form (every rank in this process): the signature of psacx_construct_gsa_* */
int psacx_multi_construct_gsa_u32(psacx_multi* mg, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t nstr, uint32_t k,
                                  uint32_t flags, uint32_t* SA, uint32_t* ISA, uint32_t* LCP);
int psacx_multi_construct_gsa_u64(psacx_multi* mg, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t nstr, uint32_t k,
                                  uint32_t flags, uint64_t* SA, uint64_t* ISA, uint64_t* LCP);
/* construct_suffix_tree(sa, begin, end, comm) on p ranks (suffix_tree.hpp:413-499; parents by for_each_parent :43-223 from
 * the ANSV of LCP :62, cells sent to the owners of their rows like bulk_permute's pairs): d_nodes[i] receives the rows of the
 * LCP indices of local rank i's block, m[i] x (sigma + 1) cells of 64 bits, row-major; cell (j, c) = the child of internal
 * node off_i + j through the character with alphabet code c (0 = end of text), leaves numbered n + index, 0 = none -- the
 * table psacx_suffix_tree_* builds on one rank, block-distributed by rows.  *sigma = number of distinct characters of the
 * whole text; d_nodes == NULL only queries it.  SA and LCP as psacx_multi_construct_dev_* left them. */
int psacx_multi_suffix_tree_dev_u32(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint32_t* const* d_SA,
                                    const uint32_t* const* d_LCP, uint64_t* const* d_nodes, uint32_t* sigma);
int psacx_multi_suffix_tree_dev_u64(psacx_multi* mg, const uint8_t* const* d_text, const uint64_t* m, const uint64_t* const* d_SA,
                                    const uint64_t* const* d_LCP, uint64_t* const* d_nodes, uint32_t* sigma);
/* the host-pointer form (the signature of psacx_suffix_tree_*; needs every rank in this process): nodes[n x (sigma + 1)] */
int psacx_multi_suffix_tree_u32(psacx_multi* mg, const uint8_t* text, uint64_t n, const uint32_t* SA, const uint32_t* LCP,
                                uint64_t* nodes, uint32_t* sigma);
int psacx_multi_suffix_tree_u64(psacx_multi* mg, const uint8_t* text, uint64_t n, const uint64_t* SA, const uint64_t* LCP,
                                uint64_t* nodes, uint32_t* sigma);
/* statistics of the last call (sigma, k, the per-round log) and what this process moved: payload bytes sent to other
 * ranks, number of all-to-all exchanges and of scalar all-gathers */
int psacx_multi_get_stats(const psacx_multi* mg, psacx_stats* out, uint64_t* bytes_sent, uint64_t* exchanges, uint64_t* gathers);
/* Memory layout of the distributed construction.  psac plans "6 words per character" for its distributed sort
 * (idxsort.hpp:43, suffix_array.hpp:751).  The normal layout here keeps every intermediate array of a phase at once
 * (fastest; up to ~14 words per character beside the three result arrays).  The reduced-memory layout lets the records of
 * the first round alternate between the rank's three result arrays and ONE allocated set of three arrays, runs SA -> ISA in
 * chunks, and works a refinement round with more unresolved suffixes than SLAB on some rank off in slabs of whole buckets
 * (results identical; the per-round counters of such a round may run ahead of the one-step log).
 *   PSACX_MULTI_OPT_LAYOUT        0 = choose by the free device memory of every rank (default), 1 = normal, 2 = reduced
 *   PSACX_MULTI_OPT_SLAB          unresolved suffixes per slab and rank (0 = block size / 16)
 *   PSACX_MULTI_OPT_OUTPUT_SLACK  the d_SA / d_ISA / d_LCP arrays handed to psacx_multi_construct_dev_* hold this many
 *                                 elements MORE than the block (m / 8 + 256 lets every rank use them as record arrays
 *                                 despite the sample sort's imbalance; without slack a rank falls back to allocating)
 * Forms of single stages (tests, A/B runs, traces; none changes the result; 0 = the engine decides unless listed):
 *   PSACX_MULTI_OPT_TRACE          1 = wall time of every phase on stderr (all local streams drained at each mark)
 *   PSACX_MULTI_OPT_WIRE_PIECE     largest message in bytes (0 = 2^28; a single 2^31-byte ncclSend arrives damaged on this stack)
 *   PSACX_MULTI_OPT_PIECES         ranges per destination of the first round's shuffle
 *   PSACX_MULTI_OPT_CHECK_CHUNKS   chunks of the distributed checker
 *   PSACX_MULTI_OPT_GLOBAL_REFINE_SORT  1 = refinement rounds sort all their records across the ranks
 *   PSACX_MULTI_OPT_ONE_STAGE      1 = first round as one sort over both key words
 *   PSACX_MULTI_OPT_TWO_WORD       first round in two-word records: 1 = never, 2 = also below 2^21 records per rank, 3 = additionally whatever the samples say
 *   PSACX_MULTI_OPT_ONE_WORD       first round in one-word records dealt by top digit: 1 = never, 2 = also for small blocks
 *   PSACX_MULTI_OPT_NO_SLICES      1 = SA -> ISA without destination slices
 *   PSACX_MULTI_OPT_SLICE_WIDE     1 = slice inversion on full words although 32-bit entries would do
 *   PSACX_MULTI_OPT_SLICE_SHAPE    window bits | slice bits << 8 | slices per step << 16 of the slice inversion (0 = by size)
 * psacx_multi_configure_from_env: the debug shim of psacx_configure_from_env for these options (PSACX_MULTI_DIET, PSACX_MULTI_SLAB,
 * PSACX_MULTI_TRACE, PSACX_MULTI_WIRE_PIECE, PSACX_MULTI_PIECES, PSACX_MULTI_CHECK_CHUNKS, PSACX_MULTI_GLOBAL_REFINE_SORT, PSACX_ONE_STAGE,
 * PSACX_MULTI_TWO_WORD, PSACX_MULTI_ONE_WORD, PSACX_MULTI_NO_SLICES, PSACX_SLICE_WIDE, PSACX_SLICE_SHAPE=wb,s1,step); options set through
 * psacx_multi_configure before it (layout, slab, slack) are kept unless a variable names them.  It also forwards to
 * psacx_configure_from_env for the rank contexts. */
#define PSACX_MULTI_OPT_LAYOUT 1
#define PSACX_MULTI_OPT_SLAB 2
#define PSACX_MULTI_OPT_OUTPUT_SLACK 3
#define PSACX_MULTI_OPT_TRACE 4
#define PSACX_MULTI_OPT_WIRE_PIECE 5
#define PSACX_MULTI_OPT_PIECES 6
#define PSACX_MULTI_OPT_CHECK_CHUNKS 7
#define PSACX_MULTI_OPT_GLOBAL_REFINE_SORT 8
#define PSACX_MULTI_OPT_ONE_STAGE 9
#define PSACX_MULTI_OPT_TWO_WORD 10
#define PSACX_MULTI_OPT_ONE_WORD 11
#define PSACX_MULTI_OPT_NO_SLICES 12
#define PSACX_MULTI_OPT_SLICE_WIDE 13
#define PSACX_MULTI_OPT_SLICE_SHAPE 14
int psacx_multi_configure_from_env(psacx_multi* mg);
/* Creation with explicit transport choices (psacx_multi_create / psacx_multi_create_rank = flags 0, shm_box_bytes 0):
 *   PSACX_MULTI_FORCE_WIRE  no shortcut for data a rank sends to itself or for scalars already on this host: every ncclSend / ncclRecv /
 *                           ncclAllGather is really issued (a single rank then drives RCCL too)
 *   PSACX_MULTI_NO_RCCL     peer copies between distinct devices of one process instead of a communicator
 *   PSACX_MULTI_SHM         (create_rank) one process per rank on one host, exchanges staged through POSIX shared memory: ranks may share a device;
 *                           shm_box_bytes = size of a rank's mailbox (0 = 32 MiB) */
#define PSACX_MULTI_FORCE_WIRE 1u
#define PSACX_MULTI_NO_RCCL 2u
#define PSACX_MULTI_SHM 4u
int psacx_multi_create_ex(psacx_multi** out, int ndev, const int* dev_ids, uint32_t flags);
int psacx_multi_create_rank_ex(psacx_multi** out, int rank, int nranks, int device, const void* id128, uint32_t flags, uint64_t shm_box_bytes);
int psacx_multi_configure(psacx_multi* mg, int option, uint64_t value);
/* after a construction: peak_bytes[i] = high-water mark of the device memory local rank i's engine had in use at once
 * (every array it allocated; the caller's text and result arrays are not in it; free blocks the rank keeps cached for
 * reuse beyond that are returned to the device whenever an allocation does not fit), *reduced = 1 if the reduced-memory
 * layout ran, *slab_rounds = refinement rounds worked off in more than one slab.  Any pointer may be null. */
int psacx_multi_get_memory(const psacx_multi* mg, uint64_t* peak_bytes, int* reduced, uint32_t* slab_rounds);

/* device memory helpers for hosts without their own HIP bindings ------------ */
int psacx_dev_alloc(psacx_ctx* ctx, void** out, uint64_t bytes);
int psacx_dev_free(psacx_ctx* ctx, void* p);
int psacx_copy_h2d(psacx_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int psacx_copy_d2h(psacx_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int psacx_sync(psacx_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* PSACX_H */
