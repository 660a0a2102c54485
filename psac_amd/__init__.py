"""psac_amd -- MI355X-native suffix array / inverse SA / LCP construction.

Host-side mirror of psac's `suffix_array<char_t, index_t, LCP>` class
(/root/reference/include/suffix_array.hpp:170-228, :469-486) over the C-ABI of
libpsacx.so (include/psacx.h).  The compute path is HIP only.
"""
from .suffix_array import Context, SuffixArray, parse_stringset, ansv, ansv_device, check_device, check_gsa_device, suffix_tree, suffix_tree_device, check_suffix_tree_device, suffix_tree_gsa, suffix_tree_gsa_device, check_suffix_tree_gsa_device, lookup_table_device, locate_device, locate, pattern_buffer, string_ends_device, lookup_table_gsa_device, locate_gsa_device, occurrences_device, occurrences, match_device, match_gsa_device, match, rmq_index_device, rmq_device, lce_device, rmq, lce, overlaps_device, overlaps, lpf_device, lz77_device, check_lz77_device, lpf, lz77, lz77_decode, bwt_device, repeats_device, bwt, bwt_decode, repeats, mems_device, mems, MEMS_SUPER, kmismatch_device, kmismatch, kedit_device, kedit, KEDIT_BEST, REPEATS_KINDS, MATCH_SUFFIXES, OVERLAP_WHOLE, NEAREST_SM, NEAREST_EQ, FURTHEST_EQ  # noqa: F401
from ._lib import PsacxError, LIB_PATH  # noqa: F401
from .multi import MultiContext, unique_id  # noqa: F401

__all__ = ["Context", "SuffixArray", "parse_stringset", "suffix_tree", "suffix_tree_device", "check_suffix_tree_device", "suffix_tree_gsa", "suffix_tree_gsa_device", "check_suffix_tree_gsa_device", "lookup_table_device", "locate_device", "locate", "pattern_buffer", "string_ends_device", "lookup_table_gsa_device", "locate_gsa_device", "occurrences_device", "occurrences", "match_device", "match_gsa_device", "match", "rmq_index_device", "rmq_device", "lce_device", "rmq", "lce", "overlaps_device", "overlaps", "lpf_device", "lz77_device", "check_lz77_device", "lpf", "lz77", "lz77_decode", "bwt_device", "repeats_device", "bwt", "bwt_decode", "repeats", "mems_device", "mems", "MEMS_SUPER", "kmismatch_device", "kmismatch", "kedit_device", "kedit", "KEDIT_BEST", "REPEATS_KINDS", "MATCH_SUFFIXES", "OVERLAP_WHOLE", "check_device", "check_gsa_device", "ansv", "PsacxError", "MultiContext", "unique_id", "NEAREST_SM", "NEAREST_EQ", "FURTHEST_EQ"]
