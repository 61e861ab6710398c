"""ctypes binding of the C ABI in include/sbwtgpu.h (libsbwtgpu.so).

Plumbing only: tests and bench.py call the HIP path through this exactly as a C/C++ host
would.  There is no Python or CPU implementation of any query behind these calls -- if the
shared library is missing, importing/using this module fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SBWTGPU_LIB", os.path.join(_HERE, "lib", "libsbwtgpu.so"))   # override: A/B builds only

OK = 0
ERR_INVALID_ARG = -1
ERR_NO_DEVICE = -2
ERR_HIP = -3
ERR_NO_STREAMING = -4
ERR_PRECALC_TOO_LONG = -5
ERR_PRECALC_GT_K = -6
ERR_NOT_SINGLETON = -7
ERR_OOM = -8
ERR_READ_TOO_LONG = -9
ERR_STALLED = -10
UNITIGS_LINKS = 1               # SBWTGPU_UNITIGS_* (sbwtgpu_unitigs_create_graph)
UNITIGS_COLUMN_MAP = 2
# sbwtgpu_walk_step: one step of a read through the unitig graph (Unitigs.walks)
WALK_STEP = np.dtype([("unitig", np.uint32), ("offset", np.uint32), ("read_pos", np.int32), ("n_kmers", np.int32)])
# sbwtgpu_bubble: one variant site of the plain unitig graph (Unitigs.bubbles)
BUBBLE = np.dtype([("source", np.uint32), ("branch", np.uint32, (2,)), ("sink", np.uint32), ("n_kmers", np.uint32, (2,)),
                   ("kind", np.uint32), ("reserved", np.uint32)])
BUBBLE_OTHER, BUBBLE_SNP = 0, 1

# every symbol include/sbwtgpu.h declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "sbwtgpu_version", "sbwtgpu_last_error", "sbwtgpu_device_count", "sbwtgpu_set_tuning",
    "sbwtgpu_index_create", "sbwtgpu_index_destroy", "sbwtgpu_index_get_info", "sbwtgpu_index_get_precalc",
    "sbwtgpu_index_export_header", "sbwtgpu_index_blob", "sbwtgpu_index_copy_blob", "sbwtgpu_index_adopt", "sbwtgpu_index_bcast",
    "sbwtgpu_rank_batch", "sbwtgpu_streaming_search_batch", "sbwtgpu_search_batch",
    "sbwtgpu_streaming_search_batch_i32", "sbwtgpu_search_batch_i32",
    "sbwtgpu_update_interval_batch", "sbwtgpu_forward_batch",
    "sbwtgpu_build_plain_matrix", "sbwtgpu_free_plain_matrix",
    "sbwtgpu_partial_search_batch", "sbwtgpu_get_kmer_batch", "sbwtgpu_select_batch",
    "sbwtgpu_search_workspace_bytes", "sbwtgpu_streaming_search_dev", "sbwtgpu_search_dev",
    "sbwtgpu_streaming_search_dev_i32", "sbwtgpu_search_dev_i32",
    "sbwtgpu_rank_dev", "sbwtgpu_encode_bases_dev", "sbwtgpu_search_encoded_dev",
    "sbwtgpu_workspace_status", "sbwtgpu_workspace_stats", "sbwtgpu_kernel_times",
    "sbwtgpu_format_text_bound", "sbwtgpu_format_scratch_bytes", "sbwtgpu_format_results_dev",
    "sbwtgpu_search_text_batch", "sbwtgpu_search_text_stream", "sbwtgpu_free_host", "sbwtgpu_release_cached_buffers",
    "sbwtgpu_index_build_lcs", "sbwtgpu_index_get_lcs", "sbwtgpu_matching_statistics_batch", "sbwtgpu_ms_workspace_bytes",
    "sbwtgpu_matching_statistics_dev", "sbwtgpu_ms_workspace_stats",
    "sbwtgpu_unitigs_create", "sbwtgpu_unitigs_info", "sbwtgpu_unitigs_dev", "sbwtgpu_unitigs_copy", "sbwtgpu_unitigs_stats",
    "sbwtgpu_unitigs_destroy", "sbwtgpu_unitigs_create_colored", "sbwtgpu_unitigs_set_ids_dev", "sbwtgpu_unitigs_set_ids_copy",
    "sbwtgpu_unitigs_color_info", "sbwtgpu_unitigs_create_graph", "sbwtgpu_unitigs_links_info", "sbwtgpu_unitigs_links_dev",
    "sbwtgpu_unitigs_links_copy", "sbwtgpu_unitigs_column_map_dev", "sbwtgpu_unitigs_column_map_copy",
    "sbwtgpu_unitigs_locate_dev", "sbwtgpu_unitigs_locate_batch", "sbwtgpu_unitigs_graph_stats",
    "sbwtgpu_unitigs_walks_prepare", "sbwtgpu_unitigs_walks_workspace_bytes", "sbwtgpu_unitigs_walks_dev", "sbwtgpu_unitigs_walks_batch",
    "sbwtgpu_index_setop", "sbwtgpu_index_setop_counts", "sbwtgpu_index_kmer_keys",
    "sbwtgpu_read_hits_batch", "sbwtgpu_read_hits_workspace_bytes", "sbwtgpu_read_hits_dev",
    "sbwtgpu_colors_create", "sbwtgpu_colors_destroy", "sbwtgpu_colors_add_batch", "sbwtgpu_colors_info", "sbwtgpu_colors_copy",
    "sbwtgpu_colors_dev", "sbwtgpu_pseudoalign_batch", "sbwtgpu_pseudoalign_workspace_bytes", "sbwtgpu_pseudoalign_dev",
    "sbwtgpu_colors_create_wide", "sbwtgpu_colors_words", "sbwtgpu_colors_info_wide", "sbwtgpu_pseudoalign_wide_batch",
    "sbwtgpu_pseudoalign_wide_dev",
    "sbwtgpu_colorsets_compress", "sbwtgpu_colorsets_create", "sbwtgpu_colorsets_expand", "sbwtgpu_colorsets_destroy",
    "sbwtgpu_colorsets_info", "sbwtgpu_colorsets_copy", "sbwtgpu_colorsets_dev", "sbwtgpu_pseudoalign_sets_batch",
    "sbwtgpu_pseudoalign_sets_dev",
    "sbwtgpu_colorsets_builder_create", "sbwtgpu_colorsets_builder_add_batch", "sbwtgpu_colorsets_builder_info",
    "sbwtgpu_colorsets_builder_finish", "sbwtgpu_colorsets_builder_destroy",
    "sbwtgpu_colorsets_merge",
    "sbwtgpu_colorsets_set_sizes", "sbwtgpu_colorsets_shared_kmers", "sbwtgpu_colorsets_shared_workspace_bytes",
    "sbwtgpu_colorsets_shared_kmers_dev",
    "sbwtgpu_colorsets_match_sets", "sbwtgpu_colorsets_select_counts", "sbwtgpu_colorsets_select",
    "sbwtgpu_screen_create", "sbwtgpu_screen_reset", "sbwtgpu_screen_destroy", "sbwtgpu_screen_workspace_bytes",
    "sbwtgpu_screen_add_dev", "sbwtgpu_screen_add_batch", "sbwtgpu_screen_info", "sbwtgpu_screen_sets", "sbwtgpu_screen_colors",
    "sbwtgpu_screen_seen_dev", "sbwtgpu_screen_seen_copy",
    "sbwtgpu_bubbles_create", "sbwtgpu_bubbles_info", "sbwtgpu_bubbles_dev", "sbwtgpu_bubbles_copy",
    "sbwtgpu_bubbles_in_degrees_copy", "sbwtgpu_bubbles_stats", "sbwtgpu_bubbles_destroy",
    "sbwtgpu_genotype_create", "sbwtgpu_genotype_reset", "sbwtgpu_genotype_destroy", "sbwtgpu_genotype_workspace_bytes",
    "sbwtgpu_genotype_add_dev", "sbwtgpu_genotype_add_batch", "sbwtgpu_genotype_info", "sbwtgpu_genotype_branches",
    "sbwtgpu_genotype_kmer_hits_copy", "sbwtgpu_genotype_calls",
    "sbwtgpu_positions_create", "sbwtgpu_positions_upload", "sbwtgpu_positions_reset", "sbwtgpu_positions_destroy",
    "sbwtgpu_positions_add_batch", "sbwtgpu_positions_info", "sbwtgpu_positions_first_copy", "sbwtgpu_positions_first_dev",
    "sbwtgpu_positions_map_workspace_bytes", "sbwtgpu_positions_map_dev", "sbwtgpu_positions_map_batch",
    "sbwtgpu_occurrences_builder_create", "sbwtgpu_occurrences_builder_add_batch", "sbwtgpu_occurrences_builder_finish",
    "sbwtgpu_occurrences_builder_destroy", "sbwtgpu_occurrences_upload", "sbwtgpu_occurrences_destroy", "sbwtgpu_occurrences_info",
    "sbwtgpu_occurrences_offsets_copy", "sbwtgpu_occurrences_keys_copy", "sbwtgpu_occurrences_offsets_dev",
    "sbwtgpu_occurrences_keys_dev", "sbwtgpu_occurrences_to_positions", "sbwtgpu_occurrences_map_workspace_bytes",
    "sbwtgpu_occurrences_map_dev", "sbwtgpu_occurrences_map_batch",
    "sbwtgpu_refseqs_create", "sbwtgpu_refseqs_destroy", "sbwtgpu_refseqs_add_batch", "sbwtgpu_refseqs_info",
    "sbwtgpu_refseqs_lengths_copy", "sbwtgpu_refseqs_get", "sbwtgpu_refseqs_verify_workspace_bytes", "sbwtgpu_refseqs_verify_dev",
    "sbwtgpu_refseqs_verify_batch",
    "sbwtgpu_align_workspace_bytes", "sbwtgpu_align_dev", "sbwtgpu_align_batch",
    "sbwtgpu_pileup_create", "sbwtgpu_pileup_reset", "sbwtgpu_pileup_destroy", "sbwtgpu_pileup_add_aligned_dev",
    "sbwtgpu_pileup_workspace_bytes", "sbwtgpu_pileup_add_dev", "sbwtgpu_pileup_add_batch", "sbwtgpu_pileup_info",
    "sbwtgpu_pileup_counts_copy", "sbwtgpu_pileup_counts_dev", "sbwtgpu_pileup_calls",
]

SETOP_UNION, SETOP_INTERSECTION, SETOP_DIFFERENCE, SETOP_SYMMETRIC_DIFFERENCE = 0, 1, 2, 3
SETOPS = {"union": SETOP_UNION, "intersection": SETOP_INTERSECTION, "difference": SETOP_DIFFERENCE,
          "symmetric-difference": SETOP_SYMMETRIC_DIFFERENCE}


class SbwtGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"sbwtgpu error {code}: {msg}")
        self.code = code
        self.msg = msg


class IndexDesc(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int64),
        ("A_bits", C.c_void_p), ("C_bits", C.c_void_p), ("G_bits", C.c_void_p), ("T_bits", C.c_void_p),
        ("suffix_group_starts", C.c_void_p),
        ("k", C.c_int64), ("n_kmers", C.c_int64), ("precalc_k", C.c_int64),
        ("precalc", C.c_void_p),
    ]


class IndexInfo(C.Structure):
    _fields_ = [
        ("n_nodes", C.c_int64), ("n_kmers", C.c_int64), ("k", C.c_int64), ("precalc_k", C.c_int64),
        ("C", C.c_int64 * 4),
        ("has_streaming_support", C.c_int32), ("device", C.c_int32),
        ("device_precalc_k", C.c_int64), ("blob_bytes", C.c_int64), ("image_level", C.c_int64),
        ("n_paths", C.c_int64), ("n_branch", C.c_int64), ("default_search_variant", C.c_int64),
    ]


class ImageHeader(C.Structure):
    """SbwtBlobHeader (csrc/sbwt_device.h): what sbwtgpu_index_export_header hands out, field for field.  Read-only view for
    tests and tools that need to know which structures an image holds (Index.image_header())."""
    _fields_ = [
        ("magic", C.c_uint64),
        ("n_nodes", C.c_int64), ("n_kmers", C.c_int64), ("k", C.c_int64), ("p_file", C.c_int64), ("p_dev", C.c_int64),
        ("C", C.c_int64 * 4),
        ("n_blocks", C.c_int64), ("n_mega", C.c_int64),
        ("off_blocks", C.c_int64), ("off_ptab", C.c_int64), ("off_ftab", C.c_int64), ("off_mega", C.c_int64),
        ("blob_bytes", C.c_int64),
        ("has_ssup", C.c_int32), ("rank_only", C.c_int32), ("ssup_derived", C.c_int32), ("p_sparse", C.c_int32),
        ("off_stab", C.c_int64),
        ("big_layout", C.c_int32), ("has_path", C.c_int32),
        ("off_col", C.c_int64), ("off_pos", C.c_int64), ("off_pq", C.c_int64), ("off_trans", C.c_int64),
        ("stab_pos", C.c_int32), ("p_filter", C.c_int32),
        ("off_pfil", C.c_int64),
        ("log2f", C.c_int32), ("has_safe", C.c_int32), ("force_mega", C.c_int32),
        ("n_tslots", C.c_int64), ("n_sb", C.c_int64), ("n_pos", C.c_int64), ("n_trans", C.c_int64),
        ("n_paths", C.c_int64), ("n_branch", C.c_int64), ("image_level", C.c_int64),
        ("row_ones", C.c_int64 * 4),
        ("log2b2_unused", C.c_int32),
        ("n_sb2", C.c_int64), ("off_stab2", C.c_int64), ("path_lookahead", C.c_int64),
    ]


class PlainMatrixBitsC(C.Structure):
    _fields_ = [("n_nodes", C.c_int64), ("n_kmers", C.c_int64), ("k", C.c_int64),
                ("A_bits", C.c_void_p), ("C_bits", C.c_void_p), ("G_bits", C.c_void_p), ("T_bits", C.c_void_p),
                ("suffix_group_starts", C.c_void_p)]


class SetopInfoC(C.Structure):
    _fields_ = [("n_a", C.c_int64), ("n_b", C.c_int64), ("n_both", C.c_int64), ("n_either", C.c_int64),
                ("n_result", C.c_int64), ("n_nopred", C.c_int64), ("pass_ms", C.c_double * 4)]

    def as_dict(self) -> dict:
        d = {f: int(getattr(self, f)) for f in ("n_a", "n_b", "n_both", "n_either", "n_result", "n_nopred")}
        d["pass_ms"] = dict(zip(("keys_a", "keys_b", "merge_select", "tail_columns"), (float(x) for x in self.pass_ms)))
        return d


class ColorsetsMergeInfoC(C.Structure):
    _fields_ = [("n_real_u", C.c_int64), ("n_from_a", C.c_int64), ("n_from_b", C.c_int64), ("n_from_both", C.c_int64),
                ("n_pairs", C.c_int64), ("n_sets", C.c_int64), ("pass_ms", C.c_double * 4)]

    def as_dict(self) -> dict:
        d = {f: int(getattr(self, f)) for f in ("n_real_u", "n_from_a", "n_from_b", "n_from_both", "n_pairs", "n_sets")}
        d["pass_ms"] = dict(zip(("keys", "locate_gather", "pairs_rows", "canonical"), (float(x) for x in self.pass_ms)))
        return d


class SharedInfoC(C.Structure):
    """sbwtgpu_shared_info: what one shared-k-mers call did."""
    _fields_ = [("n_sets_used", C.c_int64), ("n_colors", C.c_int32), ("words", C.c_int32), ("used_mfma", C.c_int32),
                ("n_limbs", C.c_int32), ("pass_ms", C.c_double * 4)]

    def as_dict(self) -> dict:
        d = {f: int(getattr(self, f)) for f in ("n_sets_used", "n_colors", "words", "used_mfma", "n_limbs")}
        d["pass_ms"] = dict(zip(("sizes", "transpose_compact", "product", "mirror_copy"), (float(x) for x in self.pass_ms)))
        return d


class ColorPredicateC(C.Structure):
    """sbwtgpu_color_predicate: W-word include and exclude masks (exclude may be NULL) and the two bounds."""
    _fields_ = [("include", C.c_void_p), ("exclude_or_null", C.c_void_p), ("min_in", C.c_int32), ("max_in", C.c_int32)]


class ColorSelectInfoC(C.Structure):
    """sbwtgpu_color_select_info: what one colour-select call counted."""
    _fields_ = [("n_real", C.c_int64), ("n_selected", C.c_int64), ("n_sets_matched", C.c_int64), ("n_nopred", C.c_int64),
                ("pass_ms", C.c_double * 3)]

    def as_dict(self) -> dict:
        d = {f: int(getattr(self, f)) for f in ("n_real", "n_selected", "n_sets_matched", "n_nopred")}
        d["pass_ms"] = dict(zip(("keys", "verdict_select", "tail_columns"), (float(x) for x in self.pass_ms)))
        return d


class ColorsInfoC(C.Structure):
    _fields_ = [("n_columns", C.c_int64), ("k", C.c_int64), ("n_colors", C.c_int32), ("n_colored_columns", C.c_int64),
                ("per_color", C.c_int64 * 64)]


# a read's pseudoalignment record (sbwtgpu_pseudoalignment): 16 bytes
PSEUDOALIGNMENT_DTYPE = np.dtype([("colors", np.uint64), ("n_kmers", np.int32), ("n_found", np.int32)])
# a read's record over a wide colour matrix (sbwtgpu_read_found): 8 bytes, its colours are W words of their own
READ_FOUND_DTYPE = np.dtype([("n_kmers", np.int32), ("n_found", np.int32)])
# sbwtgpu_read_map: a read's placement on the references (32 bytes)
READ_MAP_DTYPE = np.dtype([("start", np.int64), ("seq", np.int32), ("strand", np.int32), ("votes", np.int32), ("votes2", np.int32),
                           ("n_found", np.int32), ("n_anchored", np.int32)])
POSITIONS_MAP_TABLE = 256       # SBWTGPU_POSITIONS_MAP_TABLE
POS_NONE = 0xFFFFFFFFFFFFFFFF   # first[v]: no position
OCCURRENCES_MAP_TABLE = 256     # SBWTGPU_OCCURRENCES_MAP_TABLE
OCCURRENCES_MAX_OCC = 1 << 20   # SBWTGPU_OCCURRENCES_MAX_OCC
# sbwtgpu_read_verify: what the verification of a mapped read against the reference sequences gives
READ_VERIFY_DTYPE = np.dtype([("ref_end", np.int64), ("mismatches", np.int32), ("edit", np.int32)])
# sbwtgpu_read_align: where the best alignment of a verified read begins, its number of runs and of = columns
READ_ALIGN_DTYPE = np.dtype([("ref_begin", np.int64), ("n_ops", np.int32), ("n_eq", np.int32)])
CIGAR_LETTERS = {1: "I", 2: "D", 7: "=", 8: "X"}       # the codes of a run, as in BAM
# the pileup of aligned reads: sbwtgpu_pileup_base (one per reference base), sbwtgpu_pileup_call, sbwtgpu_pileup_filter
PILEUP_BASE_DTYPE = np.dtype([("depth", np.uint32), ("n", np.uint32, (4,)), ("n_del", np.uint32), ("n_ins", np.uint32),
                              ("n_other", np.uint32)])
PILEUP_CALL_DTYPE = np.dtype([("pos", np.int64), ("seq", np.int32), ("allele", np.int32), ("ref", np.int32), ("depth", np.int32),
                              ("count", np.int32), ("ref_count", np.int32)])
PILEUP_FILTER_DTYPE = np.dtype([("min_votes", np.int32), ("require_unique", np.int32), ("max_edit", np.int32), ("reserved", np.int32)])
PILEUP_DEL, PILEUP_INS = 4, 5   # SBWTGPU_PILEUP_DEL, SBWTGPU_PILEUP_INS: the alleles of a call beside the base codes 0 .. 3

VERIFY_MAX_BAND = 256           # SBWTGPU_VERIFY_MAX_BAND
VERIFY_MAX_READ = 1024          # SBWTGPU_VERIFY_MAX_READ
MAX_COLORS = 4096

_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """Loads libsbwtgpu.so (built by `python -m sbwt_amd.build` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m sbwt_amd.build` "
                          "(there is no CPU fallback for the GPU search path)")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    L.sbwtgpu_version.restype = C.c_char_p
    L.sbwtgpu_last_error.restype = C.c_char_p
    L.sbwtgpu_device_count.argtypes = [C.POINTER(ci)]
    L.sbwtgpu_set_tuning.argtypes = [C.c_char_p, i64]
    L.sbwtgpu_index_create.argtypes = [C.POINTER(IndexDesc), ci, C.POINTER(vp)]
    L.sbwtgpu_index_destroy.argtypes = [vp]
    L.sbwtgpu_index_destroy.restype = None
    L.sbwtgpu_index_get_info.argtypes = [vp, C.POINTER(IndexInfo)]
    L.sbwtgpu_index_get_precalc.argtypes = [vp, vp]
    L.sbwtgpu_index_export_header.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.sbwtgpu_index_blob.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.sbwtgpu_index_copy_blob.argtypes = [vp, vp, i64, vp]
    L.sbwtgpu_index_adopt.argtypes = [vp, i64, vp, i64, ci, C.POINTER(vp)]
    L.sbwtgpu_index_bcast.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(vp)]
    L.sbwtgpu_rank_batch.argtypes = [vp, vp, vp, i64, vp]
    L.sbwtgpu_streaming_search_batch.argtypes = [vp, vp, vp, i64, vp, vp]
    L.sbwtgpu_search_batch.argtypes = [vp, vp, vp, i64, vp, vp]
    try:                                    # (absent from older builds loaded through SBWTGPU_LIB for A/B runs)
        L.sbwtgpu_streaming_search_batch_i32.argtypes = [vp, vp, vp, i64, vp, vp]
        L.sbwtgpu_search_batch_i32.argtypes = [vp, vp, vp, i64, vp, vp]
    except AttributeError:
        if "SBWTGPU_LIB" not in os.environ:
            raise
    L.sbwtgpu_update_interval_batch.argtypes = [vp, vp, vp, i64, vp, vp]
    L.sbwtgpu_forward_batch.argtypes = [vp, vp, vp, i64, vp]
    L.sbwtgpu_build_plain_matrix.argtypes = [C.POINTER(C.c_char_p), vp, i64, i64, ci, ci, ci, C.POINTER(PlainMatrixBitsC)]
    L.sbwtgpu_free_plain_matrix.argtypes = [C.POINTER(PlainMatrixBitsC)]
    L.sbwtgpu_free_plain_matrix.restype = None
    L.sbwtgpu_partial_search_batch.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    L.sbwtgpu_get_kmer_batch.argtypes = [vp, vp, i64, vp]
    L.sbwtgpu_select_batch.argtypes = [vp, vp, vp, i64, vp]
    L.sbwtgpu_search_workspace_bytes.argtypes = [i64]
    L.sbwtgpu_search_workspace_bytes.restype = i64
    L.sbwtgpu_streaming_search_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, i64, vp]
    L.sbwtgpu_search_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, i64, vp]
    try:
        L.sbwtgpu_streaming_search_dev_i32.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, i64, vp]
        L.sbwtgpu_search_dev_i32.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, i64, vp]
    except AttributeError:                      # an older A/B build named by SBWTGPU_LIB
        if not os.environ.get("SBWTGPU_LIB"):
            raise
    L.sbwtgpu_rank_dev.argtypes = [vp, vp, vp, i64, vp, vp]
    L.sbwtgpu_workspace_status.argtypes = [vp, vp, C.POINTER(ci)]
    L.sbwtgpu_encode_bases_dev.argtypes = [vp, vp, i64, vp, i64, vp]
    L.sbwtgpu_search_encoded_dev.argtypes = [vp, i64, vp, i64, vp, vp, vp, i64, ci, vp]
    L.sbwtgpu_workspace_stats.argtypes = [vp, vp, C.POINTER(i64)]
    L.sbwtgpu_kernel_times.argtypes = [vp, i64, C.POINTER(i64)]
    L.sbwtgpu_format_text_bound.argtypes = [vp, i64, i64]
    L.sbwtgpu_format_text_bound.restype = i64
    L.sbwtgpu_format_scratch_bytes.argtypes = [i64]
    L.sbwtgpu_format_scratch_bytes.restype = i64
    L.sbwtgpu_format_results_dev.argtypes = [vp, vp, vp, i64, i64, vp, i64, vp, vp, i64, vp]
    L.sbwtgpu_search_text_batch.argtypes = [vp, vp, vp, i64, ci, C.POINTER(vp), C.POINTER(i64), C.POINTER(i64)]
    L.sbwtgpu_free_host.argtypes = [vp]
    L.sbwtgpu_free_host.restype = None
    L.sbwtgpu_release_cached_buffers.restype = None
    try:                                        # (absent from older builds loaded through SBWTGPU_LIB for A/B runs)
        L.sbwtgpu_index_build_lcs.argtypes = [vp]
        L.sbwtgpu_index_get_lcs.argtypes = [vp, vp]
        L.sbwtgpu_matching_statistics_batch.argtypes = [vp, vp, vp, i64, vp, vp, vp]
        L.sbwtgpu_ms_workspace_bytes.argtypes = [i64]
        L.sbwtgpu_ms_workspace_bytes.restype = i64
        L.sbwtgpu_matching_statistics_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, vp]
        L.sbwtgpu_ms_workspace_stats.argtypes = [vp, vp, C.POINTER(i64)]
        L.sbwtgpu_unitigs_create.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_unitigs_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
        L.sbwtgpu_unitigs_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.sbwtgpu_unitigs_copy.argtypes = [vp, vp, vp, vp]
        L.sbwtgpu_unitigs_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(i64)]
        L.sbwtgpu_unitigs_destroy.argtypes = [vp]
        L.sbwtgpu_unitigs_destroy.restype = None
        L.sbwtgpu_unitigs_create_colored.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_unitigs_set_ids_dev.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_unitigs_set_ids_copy.argtypes = [vp, vp]
        L.sbwtgpu_unitigs_color_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int32)]
        L.sbwtgpu_index_setop.argtypes = [vp, vp, ci, ci, C.POINTER(PlainMatrixBitsC), C.POINTER(SetopInfoC)]
        L.sbwtgpu_index_setop_counts.argtypes = [vp, vp, C.POINTER(SetopInfoC)]
        L.sbwtgpu_index_kmer_keys.argtypes = [vp, vp, i64, C.POINTER(i64), C.POINTER(ci)]
        L.sbwtgpu_read_hits_batch.argtypes = [vp, vp, vp, i64, ci, vp]
        L.sbwtgpu_read_hits_workspace_bytes.argtypes = [i64, i64, ci]
        L.sbwtgpu_read_hits_workspace_bytes.restype = i64
        L.sbwtgpu_read_hits_dev.argtypes = [vp, vp, i64, vp, i64, ci, vp, vp, i64, vp]
        L.sbwtgpu_colors_create.argtypes = [vp, ci, vp, C.POINTER(vp)]
        L.sbwtgpu_colors_destroy.argtypes = [vp]
        L.sbwtgpu_colors_destroy.restype = None
        L.sbwtgpu_colors_add_batch.argtypes = [vp, ci, vp, vp, i64, ci, C.POINTER(i64), C.POINTER(i64)]
        L.sbwtgpu_colors_info.argtypes = [vp, C.POINTER(ColorsInfoC)]
        L.sbwtgpu_colors_copy.argtypes = [vp, vp]
        L.sbwtgpu_colors_dev.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_pseudoalign_batch.argtypes = [vp, vp, vp, i64, ci, ci, ci, vp, vp]
        L.sbwtgpu_pseudoalign_workspace_bytes.argtypes = [i64, i64, ci]
        L.sbwtgpu_pseudoalign_workspace_bytes.restype = i64
        L.sbwtgpu_pseudoalign_dev.argtypes = [vp, vp, i64, vp, i64, ci, ci, ci, vp, vp, vp, i64, vp]
        L.sbwtgpu_colors_create_wide.argtypes = [vp, ci, vp, C.POINTER(vp)]
        L.sbwtgpu_colors_words.argtypes = [vp]
        L.sbwtgpu_colors_info_wide.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int32), C.POINTER(i64), vp]
        L.sbwtgpu_pseudoalign_wide_batch.argtypes = [vp, vp, vp, i64, ci, ci, ci, vp, vp, vp]
        L.sbwtgpu_pseudoalign_wide_dev.argtypes = [vp, vp, i64, vp, i64, ci, ci, ci, vp, vp, vp, vp, i64, vp]
        L.sbwtgpu_colorsets_compress.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_colorsets_create.argtypes = [vp, ci, vp, i64, vp, C.POINTER(vp)]
        L.sbwtgpu_colorsets_expand.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_colorsets_destroy.argtypes = [vp]
        L.sbwtgpu_colorsets_destroy.restype = None
        L.sbwtgpu_colorsets_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(i64),
                                             C.POINTER(i64), C.POINTER(i64)]
        L.sbwtgpu_colorsets_copy.argtypes = [vp, vp, vp]
        L.sbwtgpu_colorsets_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.sbwtgpu_pseudoalign_sets_batch.argtypes = [vp, vp, vp, i64, ci, ci, ci, vp, vp, vp]
        L.sbwtgpu_pseudoalign_sets_dev.argtypes = [vp, vp, i64, vp, i64, ci, ci, ci, vp, vp, vp, vp, i64, vp]
        L.sbwtgpu_colorsets_builder_create.argtypes = [vp, ci, C.POINTER(vp)]
        L.sbwtgpu_colorsets_builder_add_batch.argtypes = [vp, ci, vp, vp, i64, ci, C.POINTER(i64), C.POINTER(i64)]
        L.sbwtgpu_colorsets_builder_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                     C.POINTER(i64), C.POINTER(i64), vp, C.POINTER(i64)]
        L.sbwtgpu_colorsets_builder_finish.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_colorsets_builder_destroy.argtypes = [vp]
        L.sbwtgpu_colorsets_builder_destroy.restype = None
        L.sbwtgpu_colorsets_merge.argtypes = [vp, vp, vp, ci, C.POINTER(vp), C.POINTER(ColorsetsMergeInfoC)]
        L.sbwtgpu_colorsets_set_sizes.argtypes = [vp, vp]
        L.sbwtgpu_colorsets_shared_kmers.argtypes = [vp, vp, vp, C.POINTER(SharedInfoC)]
        L.sbwtgpu_colorsets_shared_workspace_bytes.argtypes = [vp]
        L.sbwtgpu_colorsets_shared_workspace_bytes.restype = i64
        L.sbwtgpu_colorsets_shared_kmers_dev.argtypes = [vp, vp, vp, vp, i64, vp]
        L.sbwtgpu_colorsets_match_sets.argtypes = [vp, C.POINTER(ColorPredicateC), vp]
        L.sbwtgpu_colorsets_select_counts.argtypes = [vp, C.POINTER(ColorPredicateC), C.POINTER(ColorSelectInfoC)]
        L.sbwtgpu_colorsets_select.argtypes = [vp, C.POINTER(ColorPredicateC), ci, C.POINTER(PlainMatrixBitsC), C.POINTER(ColorSelectInfoC)]
        # (the newest last: an older build stops here with every binding it has)
        L.sbwtgpu_unitigs_create_graph.argtypes = [vp, vp, C.c_uint, C.POINTER(vp)]
        L.sbwtgpu_unitigs_links_info.argtypes = [vp, C.POINTER(i64)]
        L.sbwtgpu_unitigs_links_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.sbwtgpu_unitigs_links_copy.argtypes = [vp, vp, vp]
        L.sbwtgpu_unitigs_column_map_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.sbwtgpu_unitigs_column_map_copy.argtypes = [vp, vp, vp]
        L.sbwtgpu_unitigs_locate_dev.argtypes = [vp, vp, i64, vp, vp, vp]
        L.sbwtgpu_unitigs_locate_batch.argtypes = [vp, vp, i64, vp, vp]
        L.sbwtgpu_unitigs_graph_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.sbwtgpu_unitigs_walks_prepare.argtypes = [vp]
        L.sbwtgpu_unitigs_walks_workspace_bytes.argtypes = [i64, i64]
        L.sbwtgpu_unitigs_walks_workspace_bytes.restype = i64
        L.sbwtgpu_unitigs_walks_dev.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, i64, vp, vp, i64, vp]
        L.sbwtgpu_unitigs_walks_batch.argtypes = [vp, vp, vp, vp, i64, vp, C.POINTER(vp), C.POINTER(i64), vp]
        L.sbwtgpu_screen_create.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_screen_reset.argtypes = [vp]
        L.sbwtgpu_screen_destroy.argtypes = [vp]
        L.sbwtgpu_screen_destroy.restype = None
        L.sbwtgpu_screen_workspace_bytes.argtypes = [i64, i64, ci]
        L.sbwtgpu_screen_workspace_bytes.restype = i64
        L.sbwtgpu_screen_add_dev.argtypes = [vp, vp, i64, vp, i64, ci, vp, i64, vp]
        L.sbwtgpu_screen_add_batch.argtypes = [vp, vp, vp, i64, ci]
        L.sbwtgpu_screen_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int32)]
        L.sbwtgpu_screen_sets.argtypes = [vp, vp, vp, vp]
        L.sbwtgpu_screen_colors.argtypes = [vp, vp, vp, vp]
        L.sbwtgpu_screen_seen_dev.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_screen_seen_copy.argtypes = [vp, vp]
        L.sbwtgpu_bubbles_create.argtypes = [vp, vp, C.POINTER(vp)]
        L.sbwtgpu_bubbles_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.sbwtgpu_bubbles_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.sbwtgpu_bubbles_copy.argtypes = [vp, vp, vp, vp]
        L.sbwtgpu_bubbles_in_degrees_copy.argtypes = [vp, vp]
        L.sbwtgpu_bubbles_stats.argtypes = [vp, C.POINTER(C.c_double)]
        L.sbwtgpu_bubbles_destroy.argtypes = [vp]
        L.sbwtgpu_bubbles_destroy.restype = None
        L.sbwtgpu_genotype_create.argtypes = [vp, vp, vp, C.POINTER(vp)]
        L.sbwtgpu_genotype_reset.argtypes = [vp]
        L.sbwtgpu_genotype_destroy.argtypes = [vp]
        L.sbwtgpu_genotype_destroy.restype = None
        L.sbwtgpu_genotype_workspace_bytes.argtypes = [i64, i64, ci]
        L.sbwtgpu_genotype_workspace_bytes.restype = i64
        L.sbwtgpu_genotype_add_dev.argtypes = [vp, vp, i64, vp, i64, ci, vp, i64, vp]
        L.sbwtgpu_genotype_add_batch.argtypes = [vp, vp, vp, i64, ci]
        L.sbwtgpu_genotype_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64),
                                            C.POINTER(C.c_int32)]
        L.sbwtgpu_genotype_branches.argtypes = [vp, vp, vp, vp]
        L.sbwtgpu_genotype_kmer_hits_copy.argtypes = [vp, vp, vp]
        L.sbwtgpu_genotype_calls.argtypes = [vp, C.c_int32, i64, vp, vp, vp, vp]
        L.sbwtgpu_positions_create.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_positions_upload.argtypes = [vp, vp, C.POINTER(vp)]
        L.sbwtgpu_positions_reset.argtypes = [vp]
        L.sbwtgpu_positions_destroy.argtypes = [vp]
        L.sbwtgpu_positions_destroy.restype = None
        L.sbwtgpu_positions_add_batch.argtypes = [vp, i64, vp, vp, i64, ci, C.POINTER(i64), C.POINTER(i64)]
        L.sbwtgpu_positions_info.argtypes = [vp] + [C.POINTER(i64)] * 6
        L.sbwtgpu_positions_first_copy.argtypes = [vp, vp]
        L.sbwtgpu_positions_first_dev.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_positions_map_workspace_bytes.argtypes = [i64, i64, ci]
        L.sbwtgpu_positions_map_workspace_bytes.restype = i64
        L.sbwtgpu_positions_map_dev.argtypes = [vp, vp, i64, vp, i64, ci, vp, vp, i64, vp]
        L.sbwtgpu_positions_map_batch.argtypes = [vp, vp, vp, i64, ci, vp]
        L.sbwtgpu_occurrences_builder_create.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_occurrences_builder_add_batch.argtypes = [vp, i64, vp, vp, i64, ci, C.POINTER(i64), C.POINTER(i64)]
        L.sbwtgpu_occurrences_builder_finish.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_occurrences_builder_destroy.argtypes = [vp]
        L.sbwtgpu_occurrences_builder_destroy.restype = None
        L.sbwtgpu_occurrences_upload.argtypes = [vp, vp, vp, i64, C.POINTER(vp)]
        L.sbwtgpu_occurrences_destroy.argtypes = [vp]
        L.sbwtgpu_occurrences_destroy.restype = None
        L.sbwtgpu_occurrences_info.argtypes = [vp] + [C.POINTER(i64)] * 8
        L.sbwtgpu_occurrences_offsets_copy.argtypes = [vp, vp]
        L.sbwtgpu_occurrences_keys_copy.argtypes = [vp, vp]
        L.sbwtgpu_occurrences_offsets_dev.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_occurrences_keys_dev.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_occurrences_to_positions.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_occurrences_map_workspace_bytes.argtypes = [i64, i64, ci]
        L.sbwtgpu_occurrences_map_workspace_bytes.restype = i64
        L.sbwtgpu_occurrences_map_dev.argtypes = [vp, vp, i64, vp, i64, ci, ci, vp, vp, i64, vp]
        L.sbwtgpu_occurrences_map_batch.argtypes = [vp, vp, vp, i64, ci, ci, vp]
        L.sbwtgpu_refseqs_create.argtypes = [ci, C.POINTER(vp)]
        L.sbwtgpu_refseqs_destroy.argtypes = [vp]
        L.sbwtgpu_refseqs_destroy.restype = None
        L.sbwtgpu_refseqs_add_batch.argtypes = [vp, i64, vp, vp, i64]
        L.sbwtgpu_refseqs_info.argtypes = [vp] + [C.POINTER(i64)] * 4
        L.sbwtgpu_refseqs_lengths_copy.argtypes = [vp, vp]
        L.sbwtgpu_refseqs_get.argtypes = [vp, i64, i64, i64, vp]
        L.sbwtgpu_refseqs_verify_workspace_bytes.argtypes = [i64, i64]
        L.sbwtgpu_refseqs_verify_workspace_bytes.restype = i64
        L.sbwtgpu_refseqs_verify_dev.argtypes = [vp, vp, i64, vp, i64, vp, ci, vp, vp, i64, vp]
        L.sbwtgpu_refseqs_verify_batch.argtypes = [vp, vp, vp, i64, vp, ci, vp]
        L.sbwtgpu_align_workspace_bytes.argtypes = [i64, i64]
        L.sbwtgpu_align_workspace_bytes.restype = i64
        L.sbwtgpu_align_dev.argtypes = [vp, vp, i64, vp, i64, vp, ci, vp, vp, vp, vp, i64, vp, i64, vp]
        L.sbwtgpu_align_batch.argtypes = [vp, vp, vp, i64, vp, ci, vp, vp, vp, C.POINTER(vp), C.POINTER(i64)]
        L.sbwtgpu_pileup_create.argtypes = [vp, C.POINTER(vp)]
        L.sbwtgpu_pileup_reset.argtypes = [vp]
        L.sbwtgpu_pileup_destroy.argtypes = [vp]
        L.sbwtgpu_pileup_destroy.restype = None
        L.sbwtgpu_pileup_add_aligned_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp]
        L.sbwtgpu_pileup_workspace_bytes.argtypes = [i64, i64]
        L.sbwtgpu_pileup_workspace_bytes.restype = i64
        L.sbwtgpu_pileup_add_dev.argtypes = [vp, vp, i64, vp, i64, vp, ci, vp, vp, i64, vp]
        L.sbwtgpu_pileup_add_batch.argtypes = [vp, vp, vp, i64, vp, ci, vp]
        L.sbwtgpu_pileup_info.argtypes = [vp] + [C.POINTER(i64)] * 8
        L.sbwtgpu_pileup_counts_copy.argtypes = [vp, i64, i64, i64, vp]
        L.sbwtgpu_pileup_counts_dev.argtypes = [vp, i64, i64, i64, vp, vp]
        L.sbwtgpu_pileup_calls.argtypes = [vp, ci, ci, ci, C.POINTER(vp), C.POINTER(i64)]
    except AttributeError:
        if not os.environ.get("SBWTGPU_LIB"):
            raise
    _lib = L
    return L


def cigar_string(ops) -> str:
    """The runs of one read (uint32: length << 4 | code) as a CIGAR string, 57=1X92=; * for no runs."""
    ops = np.asarray(ops, dtype=np.uint32)
    if len(ops) == 0:
        return "*"
    return "".join("%d%s" % (int(o) >> 4, CIGAR_LETTERS[int(o) & 15]) for o in ops)


def _check(rc: int) -> None:
    if rc != OK:
        raise SbwtGpuError(rc, lib().sbwtgpu_last_error().decode(errors="replace"))


def set_tuning(key: str, value: int) -> None:
    _check(lib().sbwtgpu_set_tuning(key.encode(), value))


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().sbwtgpu_device_count(C.byref(n))
    return n.value if rc == OK else 0


def _words(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a


def concat_reads(reads: Sequence[bytes]):
    """bases / read_off arrays for a list of byte strings."""
    lens = np.fromiter((len(r) for r in reads), dtype=np.int64, count=len(reads))
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    bases = np.frombuffer(b"".join(reads), dtype=np.uint8).copy() if len(reads) else np.zeros(0, np.uint8)
    return bases, off


def out_offsets(read_off: np.ndarray, k: int) -> np.ndarray:
    lens = np.diff(read_off)
    m = np.maximum(lens - k + 1, 0)
    off = np.zeros(len(read_off), dtype=np.int64)
    np.cumsum(m, out=off[1:])
    return off


class BuiltBits:
    """What the builders return: the four rows + suffix_group_starts as uint64 word arrays (numpy copies)."""

    def __init__(self, cols, ssup, n_nodes, n_kmers, k):
        self.cols, self.ssup, self.n_nodes, self.n_kmers, self.k = cols, ssup, n_nodes, n_kmers, k


def _take_bits(out: PlainMatrixBitsC) -> BuiltBits:
    """numpy copies of a sbwtgpu_plain_matrix_bits, which is released."""
    try:
        nw = (out.n_nodes + 63) // 64

        def words(p):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(nw,)).copy()
        cols = [words(out.A_bits), words(out.C_bits), words(out.G_bits), words(out.T_bits)]
        ssup = words(out.suffix_group_starts) if out.suffix_group_starts else None
        return BuiltBits(cols, ssup, out.n_nodes, out.n_kmers, out.k)
    finally:
        lib().sbwtgpu_free_plain_matrix(C.byref(out))


def build_bits_gpu(seqs: Sequence[bytes], k: int, add_revcomp: bool = False, streaming_support: bool = True,
                   device: int = 0) -> BuiltBits:
    """sbwtgpu_build_plain_matrix: the plain-matrix SBWT columns of `seqs`, built on the GPU (2 <= k <= 64)."""
    arr = (C.c_char_p * len(seqs))(*[bytes(s) for s in seqs])
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    out = PlainMatrixBitsC()
    _check(lib().sbwtgpu_build_plain_matrix(arr, lens.ctypes.data, len(seqs), k, int(add_revcomp), int(streaming_support),
                                            device, C.byref(out)))
    return _take_bits(out)


class _Owner:
    """What every handle-owning class shares: the handle in `_h`, and `_destroy`, the name of the library call that frees it."""

    _destroy = ""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h


class Index(_Owner):
    """Owning wrapper of a `sbwtgpu_index*` (one GPU)."""

    def __init__(self, handle: int, keepalive=None):
        self._h = C.c_void_p(handle)
        self._keep = keepalive
        info = IndexInfo()
        _check(lib().sbwtgpu_index_get_info(self._h, C.byref(info)))
        self.n_nodes, self.n_kmers, self.k = info.n_nodes, info.n_kmers, info.k
        self.precalc_k = info.precalc_k
        self.C = [info.C[i] for i in range(4)]
        self.has_streaming_support = bool(info.has_streaming_support)
        self.device = info.device
        self.device_precalc_k = info.device_precalc_k
        self.blob_bytes = info.blob_bytes
        self.image_level = info.image_level
        self.n_paths, self.n_branch, self.default_search_variant = info.n_paths, info.n_branch, info.default_search_variant

    @classmethod
    def create(cls, A, Cb, G, T, ssup, n_nodes: int, k: int, n_kmers: int = 0, precalc_k: int = 0,
               precalc=None, device: int = 0) -> "Index":
        A, Cb, G, T = _words(A), _words(Cb), _words(G), _words(T)
        s = _words(ssup) if ssup is not None else None
        pc = np.ascontiguousarray(precalc, dtype=np.int64) if precalc is not None else None
        d = IndexDesc(n_nodes, A.ctypes.data, Cb.ctypes.data, G.ctypes.data, T.ctypes.data,
                      s.ctypes.data if s is not None else None, k, n_kmers, precalc_k,
                      pc.ctypes.data if pc is not None else None)
        h = C.c_void_p()
        _check(lib().sbwtgpu_index_create(C.byref(d), device, C.byref(h)))
        return cls(h.value)

    @classmethod
    def adopt(cls, header: bytes, dev_ptr: int, blob_bytes: int, device: int, keepalive=None) -> "Index":
        h = C.c_void_p()
        buf = C.create_string_buffer(header, len(header))
        _check(lib().sbwtgpu_index_adopt(buf, len(header), C.c_void_p(dev_ptr), blob_bytes, device, C.byref(h)))
        return cls(h.value, keepalive=keepalive)

    def close(self) -> None:                   # (its own: the handle stays a c_void_p, and `_keep` lives as long as the object)
        if self._h:
            lib().sbwtgpu_index_destroy(self._h)
            self._h = C.c_void_p()

    # ---- replication helpers ----
    def export_header(self) -> bytes:
        n = C.c_int64(0)
        _check(lib().sbwtgpu_index_export_header(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().sbwtgpu_index_export_header(self._h, buf, n.value, C.byref(n)))
        return buf.raw[: n.value]

    def image_header(self) -> ImageHeader:
        """The exported header as a structure: has_path, p_sparse, n_sb2 (0 = no second-level table), p_dev, p_file, ..."""
        raw = self.export_header()
        if len(raw) != C.sizeof(ImageHeader):
            raise SbwtGpuError(ERR_INVALID_ARG, "ImageHeader has %d bytes, the library's header %d" % (C.sizeof(ImageHeader), len(raw)))
        return ImageHeader.from_buffer_copy(raw)

    def blob(self):
        p, n = C.c_void_p(), C.c_int64(0)
        _check(lib().sbwtgpu_index_blob(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def blob_tensor(self):
        """The device image as a uint8 torch tensor that ALIASES it (no copy): what rank 0 hands to the broadcast.  The
        tensor is valid while this Index is."""
        import torch
        ptr, n = self.blob()

        class _Alias:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}
        t = torch.as_tensor(_Alias(), device=torch.device("cuda", self.device))
        t._sbwt_owner = self          # keeps the image alive as long as the tensor
        return t

    def copy_blob(self, dst_dev_ptr: int, nbytes: int, stream: int = 0) -> None:
        _check(lib().sbwtgpu_index_copy_blob(self._h, dst_dev_ptr, nbytes, stream))

    def get_precalc(self) -> np.ndarray:
        out = np.zeros((4 ** self.precalc_k if self.precalc_k else 0, 2), dtype=np.int64)
        if self.precalc_k:
            _check(lib().sbwtgpu_index_get_precalc(self._h, out.ctypes.data))
        return out

    # ---- host-buffer queries ----
    def rank(self, pos, sym) -> np.ndarray:
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        sym = np.ascontiguousarray(sym, dtype=np.uint8)
        out = np.empty(len(pos), dtype=np.int64)
        _check(lib().sbwtgpu_rank_batch(self._h, pos.ctypes.data, sym.ctypes.data, len(pos), out.ctypes.data))
        return out

    def _search(self, fn, bases, read_off, out_off=None):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        if out_off is None:
            out_off = out_offsets(read_off, self.k)
        out_off = np.ascontiguousarray(out_off, dtype=np.int64)
        out = np.full(int(out_off[-1]) if len(out_off) else 0, -12345, dtype=np.int64)
        _check(fn(self._h, bases.ctypes.data, read_off.ctypes.data, len(read_off) - 1, out.ctypes.data,
                  out_off.ctypes.data))
        return out, out_off

    def streaming_search(self, bases, read_off, out_off=None):
        return self._search(lib().sbwtgpu_streaming_search_batch, bases, read_off, out_off)

    def search(self, bases, read_off, out_off=None):
        return self._search(lib().sbwtgpu_search_batch, bases, read_off, out_off)

    def search_i32(self, bases, read_off, streaming: bool = True, out_off=None):
        """The same with int32 results (sbwtgpu_*_batch_i32: half the bytes over PCIe; indexes of fewer than 2^31 columns)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        if out_off is None:
            out_off = out_offsets(read_off, self.k)
        out_off = np.ascontiguousarray(out_off, dtype=np.int64)
        out = np.full(int(out_off[-1]) if len(out_off) else 0, -12345, dtype=np.int32)
        fn = lib().sbwtgpu_streaming_search_batch_i32 if streaming else lib().sbwtgpu_search_batch_i32
        _check(fn(self._h, bases.ctypes.data, read_off.ctypes.data, len(read_off) - 1, out.ctypes.data, out_off.ctypes.data))
        return out, out_off

    def streaming_search_reads(self, reads: Sequence[bytes]):
        bases, off = concat_reads(reads)
        out, oo = self.streaming_search(bases, off)
        return [out[oo[i]:oo[i + 1]] for i in range(len(reads))]

    def search_reads(self, reads: Sequence[bytes]):
        bases, off = concat_reads(reads)
        out, oo = self.search(bases, off)
        return [out[oo[i]:oo[i + 1]] for i in range(len(reads))]

    def search_text(self, bases, read_off, streaming: bool = True):
        """The formatted `sbwt search` output of a batch (device-side print_vector, pipelined host path):
        returns (text bytes, number of k-mers searched)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        p, n, q = C.c_void_p(), C.c_int64(0), C.c_int64(0)
        _check(lib().sbwtgpu_search_text_batch(self._h, bases.ctypes.data, read_off.ctypes.data, len(read_off) - 1,
                                               int(streaming), C.byref(p), C.byref(n), C.byref(q)))
        try:
            return C.string_at(p.value, n.value), q.value
        finally:
            lib().sbwtgpu_free_host(p)

    def update_interval(self, bases, off, first, second):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        first = np.array(first, dtype=np.int64)
        second = np.array(second, dtype=np.int64)
        _check(lib().sbwtgpu_update_interval_batch(self._h, bases.ctypes.data, off.ctypes.data, len(first),
                                                   first.ctypes.data, second.ctypes.data))
        return first, second

    def forward(self, node, sym) -> np.ndarray:
        node = np.ascontiguousarray(node, dtype=np.int64)
        sym = np.ascontiguousarray(sym, dtype=np.uint8)
        out = np.empty(len(node), dtype=np.int64)
        _check(lib().sbwtgpu_forward_batch(self._h, node.ctypes.data, sym.ctypes.data, len(node), out.ctypes.data))
        return out

    def partial_search(self, bases, off):
        """SBWT::partial_search for every query: (first, second, matched_len) arrays."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        first, second, matched = (np.empty(n, dtype=np.int64) for _ in range(3))
        _check(lib().sbwtgpu_partial_search_batch(self._h, bases.ctypes.data, off.ctypes.data, n, first.ctypes.data,
                                                  second.ctypes.data, matched.ctypes.data))
        return first, second, matched

    def get_kmers(self, colex_ranks) -> np.ndarray:
        """SBWT::get_kmer for every column: an (n, k) uint8 array of ASCII chars ('$' = dummy prefix)."""
        cr = np.ascontiguousarray(colex_ranks, dtype=np.int64)
        out = np.empty((len(cr), self.k), dtype=np.uint8)
        _check(lib().sbwtgpu_get_kmer_batch(self._h, cr.ctypes.data, len(cr), out.ctypes.data))
        return out

    def select(self, j, sym) -> np.ndarray:
        j = np.ascontiguousarray(j, dtype=np.int64)
        sym = np.ascontiguousarray(sym, dtype=np.uint8)
        out = np.empty(len(j), dtype=np.int64)
        _check(lib().sbwtgpu_select_batch(self._h, j.ctypes.data, sym.ctypes.data, len(j), out.ctypes.data))
        return out

    # ---- device-buffer queries (raw pointers; torch tensors' data_ptr() go here) ----
    def streaming_search_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_out: int,
                             d_out_off: int, d_ws: int, ws_bytes: int, stream: int = 0, streaming: bool = True):
        fn = lib().sbwtgpu_streaming_search_dev if streaming else lib().sbwtgpu_search_dev
        _check(fn(self._h, d_bases, total_bases, d_read_off, n_reads, d_out, d_out_off, d_ws, ws_bytes, stream))

    def streaming_search_dev_i32(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_out32: int,
                                 d_out_off: int, d_ws: int, ws_bytes: int, stream: int = 0, streaming: bool = True):
        """The same with an int32 result array on the device (sbwtgpu_*_dev_i32)."""
        fn = lib().sbwtgpu_streaming_search_dev_i32 if streaming else lib().sbwtgpu_search_dev_i32
        _check(fn(self._h, d_bases, total_bases, d_read_off, n_reads, d_out32, d_out_off, d_ws, ws_bytes, stream))

    def encode_bases_dev(self, d_bases: int, total_bases: int, d_ws: int, ws_bytes: int, stream: int = 0):
        _check(lib().sbwtgpu_encode_bases_dev(self._h, d_bases, total_bases, d_ws, ws_bytes, stream))

    def search_encoded_dev(self, total_bases: int, d_read_off: int, n_reads: int, d_out: int, d_out_off: int,
                           d_ws: int, ws_bytes: int, streaming: bool = True, stream: int = 0):
        _check(lib().sbwtgpu_search_encoded_dev(self._h, total_bases, d_read_off, n_reads, d_out, d_out_off, d_ws,
                                                ws_bytes, int(streaming), stream))

    def workspace_stats(self, d_ws: int, stream: int = 0):
        """(n_stream, n_search, n_lf, n_tab_hit, n_ext) of the last search on this workspace."""
        st = (C.c_int64 * 8)()
        _check(lib().sbwtgpu_workspace_stats(d_ws, stream, st))
        return tuple(int(x) for x in st[:5])

    def workspace_bridges(self, d_ws: int, stream: int = 0) -> int:
        """Substitutions bridged along a path (M_BRIDGE) by the last search on this workspace."""
        st = (C.c_int64 * 8)()
        _check(lib().sbwtgpu_workspace_stats(d_ws, stream, st))
        return int(st[5])

    # ---- k-bounded matching statistics (include/sbwtgpu.h) ----
    def build_lcs(self) -> None:
        """Builds the LCS array on the device (idempotent; every MS call does it when needed)."""
        _check(lib().sbwtgpu_index_build_lcs(self._h))

    def lcs(self) -> np.ndarray:
        """The LCS array: lcs[j] = longest common suffix of the labels of columns j-1 and j ('$' never counts), lcs[0] = 0."""
        out = np.empty(self.n_nodes, dtype=np.uint8)
        _check(lib().sbwtgpu_index_get_lcs(self._h, out.ctypes.data))
        return out

    def matching_statistics(self, bases, read_off, intervals: bool = True):
        """k-bounded matching statistics of every base: len (uint8), and with intervals=True also first, second (int64)
        -- slot b answers bases[b] (arrays of read_off[-1] entries).  Returns len, or (len, first, second)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = int(read_off[-1]) if len(read_off) else 0
        ln = np.zeros(n, dtype=np.uint8)
        first = np.full(n, -12345, dtype=np.int64) if intervals else None
        second = np.full(n, -12345, dtype=np.int64) if intervals else None
        _check(lib().sbwtgpu_matching_statistics_batch(self._h, bases.ctypes.data, read_off.ctypes.data, max(len(read_off) - 1, 0),
                                                       ln.ctypes.data, first.ctypes.data if intervals else None,
                                                       second.ctypes.data if intervals else None))
        return (ln, first, second) if intervals else ln

    def matching_statistics_reads(self, reads: Sequence[bytes], intervals: bool = True):
        """Per-read lists of the batch results of a list of byte strings."""
        bases, off = concat_reads(reads)
        res = self.matching_statistics(bases, off, intervals)
        if not intervals:
            return [res[off[i]:off[i + 1]] for i in range(len(reads))]
        return [tuple(a[off[i]:off[i + 1]] for a in res) for i in range(len(reads))]

    def matching_statistics_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_len: int,
                                d_first: int, d_second: int, d_ws: int, ws_bytes: int, stream: int = 0):
        """sbwtgpu_matching_statistics_dev (raw device pointers; d_first = d_second = 0: lengths only)."""
        _check(lib().sbwtgpu_matching_statistics_dev(self._h, d_bases, total_bases, d_read_off, n_reads, d_len,
                                                     d_first or None, d_second or None, d_ws, ws_bytes, stream))

    def ms_workspace_stats(self, d_ws: int, stream: int = 0) -> dict:
        """Counters of the last MS launch on a workspace."""
        st = (C.c_int64 * 5)()
        _check(lib().sbwtgpu_ms_workspace_stats(d_ws, stream, st))
        return dict(zip(("positions", "walked", "full", "contractions", "recomputes"), (int(x) for x in st)))

    # ---- unitigs (include/sbwtgpu.h) ----
    def unitigs_dev(self) -> "Unitigs":
        """The unitigs of the index as a device-resident result (close() it, or let it go)."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_unitigs_create(self._h, C.byref(h)))
        return Unitigs(h)

    def unitigs(self):
        """(bases: uint8[total], off: int64[n + 1], first_col: int64[n]): unitig i is bases[off[i]:off[i + 1]] and starts
        with the label of column first_col[i]; ascending first_col."""
        with self.unitigs_dev() as u:
            return u.copy()

    def unitig_graph_dev(self, links: bool = True, column_map: bool = False) -> "Unitigs":
        """sbwtgpu_unitigs_create_graph: the unitigs with their links (Unitigs.links) and / or the column map
        (Unitigs.column_map, Unitigs.locate), device-resident."""
        h = C.c_void_p()
        flags = (UNITIGS_LINKS if links else 0) | (UNITIGS_COLUMN_MAP if column_map else 0)
        _check(lib().sbwtgpu_unitigs_create_graph(self._h, None, flags, C.byref(h)))
        return Unitigs(h, self.n_nodes)

    # ---- set operations on two indexes (include/sbwtgpu.h) ----
    def setop(self, other: "Index", op, streaming_support: bool = True):
        """sbwtgpu_index_setop: (BuiltBits, info) of self `op` other; op is a SETOP_* value or a name of SETOPS.  A failed
        call raises SbwtGpuError with the counts the call got to (n_nopred at the dummy limit) as its `info`."""
        out, info = PlainMatrixBitsC(), SetopInfoC()
        rc = lib().sbwtgpu_index_setop(self._h, other._h, SETOPS.get(op, op), int(streaming_support), C.byref(out), C.byref(info))
        if rc != OK:
            err = SbwtGpuError(rc, lib().sbwtgpu_last_error().decode(errors="replace"))
            err.info = info.as_dict()
            raise err
        return _take_bits(out), info.as_dict()

    def setop_counts(self, other: "Index") -> dict:
        """|A|, |B|, |A and B|, |A or B| of the two indexes' k-mer sets, and jaccard / containment (of self in other)."""
        info = SetopInfoC()
        _check(lib().sbwtgpu_index_setop_counts(self._h, other._h, C.byref(info)))
        d = info.as_dict()
        d["jaccard"] = d["n_both"] / d["n_either"] if d["n_either"] else 1.0
        d["containment"] = d["n_both"] / d["n_a"] if d["n_a"] else 1.0
        return d

    def kmer_keys(self) -> np.ndarray:
        """The k-mers of the index as the builder's sorted keys (character i at bits 2i): uint64[n_kmers] for k <= 32, an
        (n_kmers, 2) uint64 array of (low, high) words for 32 < k <= 64."""
        n, kb = C.c_int64(0), C.c_int(0)
        cap = max(self.n_kmers, 0) * (8 if self.k <= 32 else 16)
        out = np.empty(cap // 8, dtype=np.uint64)
        rc = lib().sbwtgpu_index_kmer_keys(self._h, out.ctypes.data if cap else None, cap, C.byref(n), C.byref(kb))
        if rc in (OK, ERR_INVALID_ARG) and n.value * kb.value > cap:               # (an index made with n_kmers = 0: unknown)
            cap = n.value * kb.value
            out = np.empty(cap // 8, dtype=np.uint64)
            rc = lib().sbwtgpu_index_kmer_keys(self._h, out.ctypes.data, cap, C.byref(n), C.byref(kb))
        _check(rc)
        out = out[: n.value * kb.value // 8]
        return out if kb.value == 8 else out.reshape(n.value, 2)

    # ---- per-read hit profiles (include/sbwtgpu.h) ----
    def read_hits(self, bases, read_off, both_strands: bool = False) -> np.ndarray:
        """sbwtgpu_read_hits_batch: an (n_reads, 4) int32 array of (n_kmers, n_found, covered_bases, longest_run) per read."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = max(len(read_off) - 1, 0)
        out = np.full((n, 4), -12345, dtype=np.int32)
        _check(lib().sbwtgpu_read_hits_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n, 2 if both_strands else 1,
                                             out.ctypes.data))
        return out

    def read_hits_reads(self, reads: Sequence[bytes], both_strands: bool = False) -> np.ndarray:
        """The same for a list of byte strings."""
        bases, off = concat_reads(reads)
        return self.read_hits(bases, off, both_strands)

    def read_hits_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_out: int, d_ws: int, ws_bytes: int,
                      both_strands: bool = False, stream: int = 0):
        """sbwtgpu_read_hits_dev (raw device pointers; d_out: n_reads records of four int32)."""
        _check(lib().sbwtgpu_read_hits_dev(self._h, d_bases, total_bases, d_read_off, n_reads, 2 if both_strands else 1, d_out,
                                           d_ws, ws_bytes, stream))

    def workspace_status(self, d_ws: int, stream: int = 0) -> int:
        st = C.c_int(0)
        _check(lib().sbwtgpu_workspace_status(d_ws, stream, C.byref(st)))
        return st.value

    # ---- reference positions and read mapping (include/sbwtgpu.h, "positions") ----
    def positions(self) -> "Positions":
        """sbwtgpu_positions_create: an empty position table bound to this index."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_positions_create(self._h, C.byref(h)))
        return Positions(h, self)

    def occurrences_builder(self) -> "OccurrencesBuilder":
        """sbwtgpu_occurrences_builder_create: an empty builder of an occurrence table bound to this index."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_occurrences_builder_create(self._h, C.byref(h)))
        return OccurrencesBuilder(h, self)


class Unitigs(_Owner):
    """Owns an sbwtgpu_unitigs handle."""

    _destroy = "sbwtgpu_unitigs_destroy"

    def __init__(self, handle, n_nodes: int = 0):
        self._h = handle
        self.n_nodes = n_nodes                  # (a graph handle: the length of the column map)
        n, total, nk = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(lib().sbwtgpu_unitigs_info(self._h, C.byref(n), C.byref(total), C.byref(nk)))
        self.n_unitigs, self.total_bases, self.n_kmers = n.value, total.value, nk.value

    def dev_ptrs(self):
        """(d_bases, d_off, d_first_col) as integers; valid until close()."""
        b, o, f = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().sbwtgpu_unitigs_dev(self._h, C.byref(b), C.byref(o), C.byref(f)))
        return b.value or 0, o.value or 0, f.value or 0

    def copy(self):
        bases = np.empty(self.total_bases, dtype=np.uint8)
        off = np.empty(self.n_unitigs + 1, dtype=np.int64)
        first_col = np.empty(self.n_unitigs, dtype=np.int64)
        _check(lib().sbwtgpu_unitigs_copy(self._h, bases.ctypes.data, off.ctypes.data, first_col.ctypes.data))
        return bases, off, first_col

    def stats(self) -> dict:
        """Device-event times of the passes (ms) and the number of pointer-jumping rounds."""
        ms = (C.c_double * 6)()
        r = C.c_int64(0)
        _check(lib().sbwtgpu_unitigs_stats(self._h, ms, C.byref(r)))
        names = ("pred_marks", "real_flags", "internal_edges", "pointer_jumping", "ids_offsets", "bases")
        return {"pass_ms": dict(zip(names, (float(x) for x in ms))), "jump_rounds": int(r.value)}


    # ---- a graph handle only (Index.unitig_graph_dev, ColorSets.unitig_graph_dev) ----
    def n_links(self) -> int:
        n = C.c_int64(0)
        _check(lib().sbwtgpu_unitigs_links_info(self._h, C.byref(n)))
        return int(n.value)

    def links_dev(self):
        """(d_link_off, d_link_to) as integers; valid until close()."""
        o, t = C.c_void_p(), C.c_void_p()
        _check(lib().sbwtgpu_unitigs_links_dev(self._h, C.byref(o), C.byref(t)))
        return o.value or 0, t.value or 0

    def links(self):
        """(link_off: int64[n_unitigs + 1], link_to: uint32[n_links]): unitig i links to link_to[link_off[i]:link_off[i + 1]],
        in the order of the edge character."""
        link_off = np.empty(self.n_unitigs + 1, dtype=np.int64)
        link_to = np.empty(self.n_links(), dtype=np.uint32)
        _check(lib().sbwtgpu_unitigs_links_copy(self._h, link_off.ctypes.data, link_to.ctypes.data if len(link_to) else None))
        return link_off, link_to

    def column_map_dev(self):
        """(d_col_unitig, d_col_offset) as integers; valid until close()."""
        a, b = C.c_void_p(), C.c_void_p()
        _check(lib().sbwtgpu_unitigs_column_map_dev(self._h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def column_map(self):
        """(col_unitig, col_offset): uint32[n_nodes] each, the unitig of every column and the position of its k-mer on it;
        0xFFFFFFFF in both for a dummy column."""
        col_unitig = np.empty(self.n_nodes, dtype=np.uint32)
        col_offset = np.empty(self.n_nodes, dtype=np.uint32)
        _check(lib().sbwtgpu_unitigs_column_map_copy(self._h, col_unitig.ctypes.data, col_offset.ctypes.data))
        return col_unitig, col_offset

    def locate(self, cols):
        """sbwtgpu_unitigs_locate_batch: (unitig, offset), uint32 each, of int64 search results; 0xFFFFFFFF for no column."""
        cols = np.ascontiguousarray(cols, dtype=np.int64)
        unitig = np.empty(len(cols), dtype=np.uint32)
        offset = np.empty(len(cols), dtype=np.uint32)
        _check(lib().sbwtgpu_unitigs_locate_batch(self._h, cols.ctypes.data, len(cols), unitig.ctypes.data, offset.ctypes.data))
        return unitig, offset

    def locate_dev(self, d_cols: int, n: int, d_unitig: int, d_offset: int, stream: int = 0) -> None:
        """sbwtgpu_unitigs_locate_dev (raw device pointers)."""
        _check(lib().sbwtgpu_unitigs_locate_dev(self._h, d_cols, n, d_unitig, d_offset, stream))

    def graph_stats(self) -> dict:
        """Device-event times (ms) of the link passes and of the map pass of the create call."""
        a, b = C.c_double(0), C.c_double(0)
        _check(lib().sbwtgpu_unitigs_graph_stats(self._h, C.byref(a), C.byref(b)))
        return {"links_ms": float(a.value), "map_ms": float(b.value)}

    # ---- reads threaded through the graph (a handle with the column map) ----
    def walks_prepare(self) -> None:
        """sbwtgpu_unitigs_walks_prepare: builds the handle's start bitmap (idempotent)."""
        _check(lib().sbwtgpu_unitigs_walks_prepare(self._h))

    def walks(self, index: "Index", bases, read_off, coverage: bool = False):
        """sbwtgpu_unitigs_walks_batch: (step_off: int64[n_reads + 1], steps: WALK_STEP[n_steps]) -- read r's steps are
        steps[step_off[r]:step_off[r + 1]] -- and with coverage=True also int64[n_unitigs], the k-mer hits per unitig."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = max(len(read_off) - 1, 0)
        step_off = np.full(n + 1, -12345, dtype=np.int64)
        cov = np.full(self.n_unitigs, -12345, dtype=np.int64) if coverage else None
        p, ns = C.c_void_p(), C.c_int64(0)
        _check(lib().sbwtgpu_unitigs_walks_batch(index._h, self._h, bases.ctypes.data, read_off.ctypes.data, n, step_off.ctypes.data,
                                                 C.byref(p), C.byref(ns), cov.ctypes.data if coverage else None))
        try:
            steps = np.empty(ns.value, dtype=WALK_STEP)
            if ns.value:
                C.memmove(steps.ctypes.data, p.value, ns.value * WALK_STEP.itemsize)
        finally:
            if p.value:
                lib().sbwtgpu_free_host(p)
        return (step_off, steps, cov) if coverage else (step_off, steps)

    def walks_reads(self, index: "Index", reads: Sequence[bytes], coverage: bool = False):
        """The same for a list of byte strings."""
        bases, off = concat_reads(reads)
        return self.walks(index, bases, off, coverage)

    def walks_dev(self, index: "Index", d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_step_off: int, d_steps: int,
                  steps_cap: int, d_unitig_kmers: int, d_ws: int, ws_bytes: int, stream: int = 0) -> None:
        """sbwtgpu_unitigs_walks_dev (raw device pointers; d_unitig_kmers 0 = no coverage); needs walks_prepare()."""
        _check(lib().sbwtgpu_unitigs_walks_dev(index._h, self._h, d_bases, total_bases, d_read_off, n_reads, d_step_off, d_steps,
                                               steps_cap, d_unitig_kmers or None, d_ws, ws_bytes, stream))

    # ---- bubbles (a plain handle with the links) ----
    def in_degrees(self) -> np.ndarray:
        """sbwtgpu_bubbles_in_degrees_copy: uint32[n_unitigs], the number of links that end at every unitig."""
        indeg = np.empty(self.n_unitigs, dtype=np.uint32)
        _check(lib().sbwtgpu_bubbles_in_degrees_copy(self._h, indeg.ctypes.data if self.n_unitigs else None))
        return indeg

    def bubbles(self, colorsets: Optional["ColorSets"] = None) -> "Bubbles":
        """sbwtgpu_bubbles_create: the bubbles of the graph and, with a colour-set object of the same index (the handle then
        needs the column map), the colours of every branch."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_bubbles_create(self._h, colorsets._h if colorsets is not None else None, C.byref(h)))
        return Bubbles(h)

    def genotype(self, index: "Index", bubbles: "Bubbles") -> "Genotype":
        """sbwtgpu_genotype_create: an accumulator of per-allele k-mer depth over the bubbles of this handle (made from `index`
        with the links and the column map).  The object copies what it needs of `bubbles`."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_genotype_create(index._h, self._h, bubbles._h, C.byref(h)))
        return Genotype(h, index, self)

    # ---- a coloured handle only (ColorSets.unitigs_dev) ----
    def set_ids_dev(self) -> int:
        """d_set_id (n_unitigs uint32) as an integer; valid until close()."""
        p = C.c_void_p()
        _check(lib().sbwtgpu_unitigs_set_ids_dev(self._h, C.byref(p)))
        return p.value or 0

    def set_ids(self) -> np.ndarray:
        """uint32[n_unitigs]: the colour-set id of every unitig (the id of its first column)."""
        set_id = np.empty(self.n_unitigs, dtype=np.uint32)
        _check(lib().sbwtgpu_unitigs_set_ids_copy(self._h, set_id.ctypes.data))
        return set_id

    def color_info(self) -> dict:
        nb, ns, nc = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        _check(lib().sbwtgpu_unitigs_color_info(self._h, C.byref(nb), C.byref(ns), C.byref(nc)))
        return {"n_color_breaks": int(nb.value), "n_sets": int(ns.value), "n_colors": int(nc.value)}


class Bubbles(_Owner):
    """Owns an sbwtgpu_bubbles handle: the variant sites of a plain unitig graph (Unitigs.bubbles)."""

    _destroy = "sbwtgpu_bubbles_destroy"

    def __init__(self, handle):
        self._h = handle
        i = self.info()
        self.n_bubbles, self.n_snps, self.n_colors, self.words = i["n_bubbles"], i["n_snps"], i["n_colors"], i["words"]

    def info(self) -> dict:
        nb, ns, nc, w = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0)
        _check(lib().sbwtgpu_bubbles_info(self._h, C.byref(nb), C.byref(ns), C.byref(nc), C.byref(w)))
        return {"n_bubbles": int(nb.value), "n_snps": int(ns.value), "n_colors": int(nc.value), "words": int(w.value)}

    def _copy(self):
        rec = np.zeros(self.n_bubbles, dtype=BUBBLE)
        inter = np.zeros((self.n_bubbles, 2, self.words), dtype=np.uint64)
        uni = np.zeros((self.n_bubbles, 2, self.words), dtype=np.uint64)
        rows = self.n_bubbles > 0 and self.words > 0
        _check(lib().sbwtgpu_bubbles_copy(self._h, rec.ctypes.data if self.n_bubbles else None, inter.ctypes.data if rows else None,
                                          uni.ctypes.data if rows else None))
        return rec, inter, uni

    def records(self) -> np.ndarray:
        """BUBBLE[n_bubbles], ascending by source: source, branch[2], sink, n_kmers[2], kind, reserved."""
        return self._copy()[0]

    def branch_colors(self):
        """(inter, uni): uint64[n_bubbles, 2, W] each -- the references that hold the whole allele of a branch, and those that
        hold any of its k-mers.  W = 0 for an object made without colour sets."""
        return self._copy()[1:]

    def dev_ptrs(self):
        """(d_rec, d_inter, d_union) as integers (0 where there is nothing); valid until close()."""
        r, a, b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().sbwtgpu_bubbles_dev(self._h, C.byref(r), C.byref(a), C.byref(b)))
        return r.value or 0, a.value or 0, b.value or 0

    def stats(self) -> dict:
        """Device-event times of the passes (ms)."""
        ms = (C.c_double * 4)()
        _check(lib().sbwtgpu_bubbles_stats(self._h, ms))
        return {"pass_ms": dict(zip(("in_degrees", "detect", "compact", "branch_colors"), (float(x) for x in ms)))}


class Genotype(_Owner):
    """Owns an sbwtgpu_genotype handle: the accumulator of a read set genotyped at the bubbles of a plain unitig graph
    (include/sbwtgpu.h, "genotype") -- per k-mer of every branch its hits, per branch seen / hits / min_hits, per bubble a call
    and per colour how often the sample follows it.  Everything is exact int64.  The index and the handle are kept referenced."""

    _destroy = "sbwtgpu_genotype_destroy"

    def __init__(self, handle, index: "Index", unitigs: "Unitigs"):
        self._h = handle
        self.index, self.unitigs = index, unitigs
        i = self.info()
        self.n_bubbles, self.n_branch_kmers, self.n_colors = i["n_bubbles"], i["n_branch_kmers"], i["n_colors"]

    def add(self, bases, read_off, strands: int = 1) -> None:
        """sbwtgpu_genotype_add_batch: the reads (uint8 bases, int64 offsets) join the sample; strands = 2 adds the reverse
        complement of every window too."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        _check(lib().sbwtgpu_genotype_add_batch(self._h, bases.ctypes.data, read_off.ctypes.data, len(read_off) - 1, strands))

    def add_reads(self, reads: Sequence[bytes], strands: int = 1) -> None:
        bases, off = concat_reads(reads)
        self.add(bases, off, strands)

    def add_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_ws: int, ws_bytes: int, strands: int = 1,
                stream: int = 0) -> None:
        """sbwtgpu_genotype_add_dev (raw device pointers; workspace of genotype_workspace_bytes): asynchronous on stream."""
        _check(lib().sbwtgpu_genotype_add_dev(self._h, d_bases or None, total_bases, d_read_off or None, n_reads, strands, d_ws or None,
                                              ws_bytes, stream or None))

    def reset(self) -> None:
        _check(lib().sbwtgpu_genotype_reset(self._h))

    def info(self) -> dict:
        """n_bubbles, n_branch_kmers (P), n_windows, n_hits, n_site_hits and n_colors."""
        v = [C.c_int64() for _ in range(5)]
        nc = C.c_int32()
        _check(lib().sbwtgpu_genotype_info(self._h, *[C.byref(x) for x in v], C.byref(nc)))
        return dict(zip(("n_bubbles", "n_branch_kmers", "n_windows", "n_hits", "n_site_hits"), (int(x.value) for x in v)),
                    n_colors=int(nc.value))

    def branches(self):
        """(seen, hits, min_hits): int64[2 n_bubbles] each, slot 2 i + j = branch j of bubble i."""
        out = [np.full(2 * self.n_bubbles, -12345, dtype=np.int64) for _ in range(3)]
        _check(lib().sbwtgpu_genotype_branches(self._h, *[x.ctypes.data if x.size else None for x in out]))
        return tuple(out)

    def kmer_hits(self):
        """(branch_off, kmer_hits): int64[2 n_bubbles + 1] and uint64[P]; branch s holds kmer_hits[branch_off[s] : branch_off[s + 1]]."""
        off = np.full(2 * self.n_bubbles + 1, -12345, dtype=np.int64)
        hits = np.full(self.n_branch_kmers, 12345, dtype=np.uint64)
        _check(lib().sbwtgpu_genotype_kmer_hits_copy(self._h, off.ctypes.data, hits.ctypes.data if hits.size else None))
        return off, hits

    def calls(self, breadth_ppm: int = 1_000_000, min_depth: int = 1):
        """(call, ref_sites, ref_match, ref_only): uint8[n_bubbles] (bit 0: allele a present, bit 1: allele b) and, for an
        object made from bubbles with colours, int64[n_colors] each (None otherwise)."""
        call = np.full(self.n_bubbles, 0xA5, dtype=np.uint8)
        ref = [np.full(self.n_colors, -12345, dtype=np.int64) for _ in range(3)] if self.n_colors else [None] * 3
        _check(lib().sbwtgpu_genotype_calls(self._h, breadth_ppm, min_depth, call.ctypes.data if call.size else None,
                                            *[x.ctypes.data if x is not None else None for x in ref]))
        return (call,) + tuple(ref)


class Colors(_Owner):
    """Owns an sbwtgpu_colors handle: the colour matrix of an index (one uint64 row per column, bit c = reference c holds the
    column's k-mer) and pseudoalignment over it.  The index must stay alive as long as the object (it is kept referenced)."""

    _destroy = "sbwtgpu_colors_destroy"

    def __init__(self, handle, index: Index, n_colors: int):
        self._h = handle
        self.index, self.n_colors = index, n_colors

    @classmethod
    def create(cls, index: Index, n_colors: int) -> "Colors":
        """An empty matrix of n_colors colours (1 .. 64)."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_colors_create(index.handle, n_colors, None, C.byref(h)))
        return cls(h, index, n_colors)

    @classmethod
    def from_rows(cls, index: Index, rows, n_colors: int, k: Optional[int] = None) -> "Colors":
        """A matrix from its rows (Colors.rows(), or hostlib.colors_read with its k): bits >= n_colors and the rows of dummy
        columns are cleared.  Rows of another index -- another number of columns, another k -- are refused."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        if rows.ndim != 1 or len(rows) != index.n_nodes or (k is not None and k != index.k):
            raise SbwtGpuError(ERR_INVALID_ARG, "colours of %d columns at k = %s used with an index of %d columns at k = %d"
                               % (rows.size, "?" if k is None else k, index.n_nodes, index.k))
        h = C.c_void_p()
        _check(lib().sbwtgpu_colors_create(index.handle, n_colors, rows.ctypes.data, C.byref(h)))
        return cls(h, index, n_colors)

    def add_sequences(self, color: int, bases, read_off, both_strands: bool = False):
        """sbwtgpu_colors_add_batch: colours every k-mer of the sequences that the index holds; (n_windows, n_hit_windows).
        Not to be run concurrently with anything else on this object."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        nw, nh = C.c_int64(0), C.c_int64(0)
        _check(lib().sbwtgpu_colors_add_batch(self._h, color, bases.ctypes.data, read_off.ctypes.data, max(len(read_off) - 1, 0),
                                              2 if both_strands else 1, C.byref(nw), C.byref(nh)))
        return nw.value, nh.value

    def add_reads(self, color: int, reads: Sequence[bytes], both_strands: bool = False):
        """The same for a list of byte strings."""
        bases, off = concat_reads(reads)
        return self.add_sequences(color, bases, off, both_strands)

    def rows(self) -> np.ndarray:
        out = np.empty(self.index.n_nodes, dtype=np.uint64)
        _check(lib().sbwtgpu_colors_copy(self._h, out.ctypes.data))
        return out

    def rows_dev(self) -> int:
        p = C.c_void_p()
        _check(lib().sbwtgpu_colors_dev(self._h, C.byref(p)))
        return p.value or 0

    def info(self) -> dict:
        """n_columns, k, n_colors, n_colored_columns and per_color (n_colors counts of coloured columns)."""
        ci = ColorsInfoC()
        _check(lib().sbwtgpu_colors_info(self._h, C.byref(ci)))
        return {"n_columns": ci.n_columns, "k": ci.k, "n_colors": ci.n_colors, "n_colored_columns": ci.n_colored_columns,
                "per_color": [int(ci.per_color[c]) for c in range(ci.n_colors)]}

    def pseudoalign(self, bases, read_off, both_strands: bool = False, threshold_ppm: int = 1_000_000, denominator: int = 0,
                    counts: bool = False):
        """sbwtgpu_pseudoalign_batch: a record array (PSEUDOALIGNMENT_DTYPE: colors, n_kmers, n_found) of n_reads entries;
        with counts=True also the (n_reads, n_colors) int32 array of count_c."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = max(len(read_off) - 1, 0)
        out = np.zeros(n, dtype=PSEUDOALIGNMENT_DTYPE)
        out["n_kmers"] = -12345
        cnt = np.full((n, self.n_colors), -12345, dtype=np.int32) if counts else None
        _check(lib().sbwtgpu_pseudoalign_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n, 2 if both_strands else 1,
                                               threshold_ppm, denominator, out.ctypes.data, cnt.ctypes.data if counts else None))
        return (out, cnt) if counts else out

    def pseudoalign_reads(self, reads: Sequence[bytes], both_strands: bool = False, threshold_ppm: int = 1_000_000,
                          denominator: int = 0, counts: bool = False):
        """The same for a list of byte strings."""
        bases, off = concat_reads(reads)
        return self.pseudoalign(bases, off, both_strands, threshold_ppm, denominator, counts)

    def pseudoalign_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_out: int, d_counts: int, d_ws: int,
                        ws_bytes: int, both_strands: bool = False, threshold_ppm: int = 1_000_000, denominator: int = 0,
                        stream: int = 0):
        """sbwtgpu_pseudoalign_dev (raw device pointers; d_out: n_reads records of 16 bytes; d_counts = 0: no counts)."""
        _check(lib().sbwtgpu_pseudoalign_dev(self._h, d_bases, total_bases, d_read_off, n_reads, 2 if both_strands else 1,
                                             threshold_ppm, denominator, d_out, d_counts or None, d_ws, ws_bytes, stream))


class WideColors(Colors):
    """A colour matrix of up to MAX_COLORS colours: W = ceil(n_colors / 64) uint64 words per column, colour c is bit c & 63 of
    word c >> 6 (include/sbwtgpu.h, "wide colour matrices").  Colouring (add_sequences, add_reads), rows_dev and close are
    Colors'; rows, info and the queries are the wide calls, which give for n_colors <= 64 what Colors gives."""

    def __init__(self, handle, index: Index, n_colors: int):
        super().__init__(handle, index, n_colors)
        self.words = int(lib().sbwtgpu_colors_words(handle))

    @classmethod
    def create(cls, index: Index, n_colors: int) -> "WideColors":
        """An empty matrix of n_colors colours (1 .. MAX_COLORS)."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_colors_create_wide(index.handle, n_colors, None, C.byref(h)))
        return cls(h, index, n_colors)

    @classmethod
    def from_rows(cls, index: Index, rows, n_colors: int, k: Optional[int] = None) -> "WideColors":
        """A matrix from its (n_nodes, W) words (WideColors.rows(), or hostlib.colors_read_wide with its k): bits >= n_colors
        and the rows of dummy columns are cleared.  Rows of another shape, another index or another k are refused."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        if not 1 <= n_colors <= MAX_COLORS:
            raise SbwtGpuError(ERR_INVALID_ARG, "n_colors must be in 1 .. %d, not %d" % (MAX_COLORS, n_colors))
        words = (n_colors + 63) // 64
        if rows.ndim != 2 or rows.shape != (index.n_nodes, words) or (k is not None and k != index.k):
            raise SbwtGpuError(ERR_INVALID_ARG, "colours of shape %s at k = %s used with an index of %d columns at k = %d, %d words a row"
                               % (rows.shape, "?" if k is None else k, index.n_nodes, index.k, words))
        h = C.c_void_p()
        _check(lib().sbwtgpu_colors_create_wide(index.handle, n_colors, rows.ctypes.data, C.byref(h)))
        return cls(h, index, n_colors)

    add = Colors.add_sequences

    def rows(self) -> np.ndarray:
        """(n_nodes, W) uint64"""
        out = np.empty((self.index.n_nodes, self.words), dtype=np.uint64)
        _check(lib().sbwtgpu_colors_copy(self._h, out.ctypes.data))
        return out

    def info(self) -> dict:
        """n_columns, k, n_colors, words, n_colored_columns and per_color (n_colors counts of coloured columns)."""
        n, k, nc, ncc = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int64()
        per = np.zeros(self.n_colors, dtype=np.int64)
        _check(lib().sbwtgpu_colors_info_wide(self._h, C.byref(n), C.byref(k), C.byref(nc), C.byref(ncc), per.ctypes.data))
        return {"n_columns": n.value, "k": k.value, "n_colors": nc.value, "words": self.words, "n_colored_columns": ncc.value,
                "per_color": [int(x) for x in per]}

    def pseudoalign(self, bases, read_off, both_strands: bool = False, threshold_ppm: int = 1_000_000, denominator: int = 0,
                    counts: bool = False):
        """sbwtgpu_pseudoalign_wide_batch: (records, colors) -- a READ_FOUND_DTYPE array of n_reads entries and the (n_reads, W)
        uint64 colour words; with counts=True also the (n_reads, n_colors) int32 array of count_c."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = max(len(read_off) - 1, 0)
        out = np.zeros(n, dtype=READ_FOUND_DTYPE)
        out["n_kmers"] = -12345
        col = np.zeros((n, self.words), dtype=np.uint64)
        cnt = np.full((n, self.n_colors), -12345, dtype=np.int32) if counts else None
        _check(lib().sbwtgpu_pseudoalign_wide_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n, 2 if both_strands else 1,
                                                    threshold_ppm, denominator, out.ctypes.data, col.ctypes.data,
                                                    cnt.ctypes.data if counts else None))
        return (out, col, cnt) if counts else (out, col)

    def pseudoalign_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_out: int, d_colors: int, d_counts: int,
                        d_ws: int, ws_bytes: int, both_strands: bool = False, threshold_ppm: int = 1_000_000, denominator: int = 0,
                        stream: int = 0):
        """sbwtgpu_pseudoalign_wide_dev (raw device pointers; d_out: n_reads records of 8 bytes; d_colors: n_reads x W words;
        d_counts = 0: no counts)."""
        _check(lib().sbwtgpu_pseudoalign_wide_dev(self._h, d_bases, total_bases, d_read_off, n_reads, 2 if both_strands else 1,
                                                  threshold_ppm, denominator, d_out, d_colors, d_counts or None, d_ws, ws_bytes, stream))


class ColorSets(_Owner):
    """Owns an sbwtgpu_colorsets handle: the deduplicated colour sets of an index -- one uint32 id per column and a table of the
    distinct rows of W = ceil(n_colors / 64) words (include/sbwtgpu.h, "colour sets").  It means the wide matrix
    table[ids[j]]; the queries return what WideColors' return on that matrix.  The index is kept referenced."""

    _destroy = "sbwtgpu_colorsets_destroy"

    def __init__(self, handle, index: Index):
        self._h = handle
        self.index = index
        info = self.info()
        self.n_colors, self.words, self.n_sets = info["n_colors"], info["words"], info["n_sets"]

    @classmethod
    def from_colors(cls, colors: Colors) -> "ColorSets":
        """sbwtgpu_colorsets_compress: the canonical form of any colours object, which stays as it is."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_colorsets_compress(colors.handle, C.byref(h)))
        return cls(h, colors.index)

    @classmethod
    def from_arrays(cls, index: Index, n_colors: int, ids, table, k: Optional[int] = None) -> "ColorSets":
        """sbwtgpu_colorsets_create from ids (n_nodes uint32) and table ((n_sets, W) uint64; ColorSets.copy(), or
        hostlib.colorsets_read with its k): the ids of dummy columns are set to 0, every other broken invariant is refused."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        table = np.ascontiguousarray(table, dtype=np.uint64)
        if not 1 <= n_colors <= MAX_COLORS:
            raise SbwtGpuError(ERR_INVALID_ARG, "n_colors must be in 1 .. %d, not %d" % (MAX_COLORS, n_colors))
        words = (n_colors + 63) // 64
        if ids.ndim != 1 or len(ids) != index.n_nodes or (k is not None and k != index.k):
            raise SbwtGpuError(ERR_INVALID_ARG, "colour sets of %d columns at k = %s used with an index of %d columns at k = %d"
                               % (ids.size, "?" if k is None else k, index.n_nodes, index.k))
        if table.ndim != 2 or table.shape[1] != words or table.shape[0] < 1:
            raise SbwtGpuError(ERR_INVALID_ARG, "a table of shape %s, %d colours need at least one row of %d words"
                               % (table.shape, n_colors, words))
        h = C.c_void_p()
        _check(lib().sbwtgpu_colorsets_create(index.handle, n_colors, ids.ctypes.data, table.shape[0], table.ctypes.data, C.byref(h)))
        return cls(h, index)

    @classmethod
    def merge(cls, u: Index, sa: "ColorSets", sb: Optional["ColorSets"] = None, color_offset: Optional[int] = None) -> "ColorSets":
        """sbwtgpu_colorsets_merge: the canonical colour-set object of index u whose column of k-mer x carries what sa says
        about x in its index, plus what sb says about it in its own with color_offset added to every colour (default: sa's
        n_colors, the two colour spaces one after the other; 0 without sb).  The counts and pass times of the call are the
        result's merge_info."""
        if color_offset is None:
            color_offset = sa.n_colors if sb is not None else 0
        h, info = C.c_void_p(), ColorsetsMergeInfoC()
        _check(lib().sbwtgpu_colorsets_merge(u.handle, sa.handle, sb.handle if sb is not None else None, color_offset, C.byref(h),
                                             C.byref(info)))
        out = cls(h, u)
        out.merge_info = info.as_dict()
        return out

    def info(self) -> dict:
        """n_columns, k, n_colors, words, n_sets, n_colored_columns and device_bytes."""
        n, k, ns, ncc, db = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        nc, w = C.c_int32(), C.c_int32()
        _check(lib().sbwtgpu_colorsets_info(self._h, C.byref(n), C.byref(k), C.byref(nc), C.byref(w), C.byref(ns), C.byref(ncc),
                                            C.byref(db)))
        return {"n_columns": n.value, "k": k.value, "n_colors": nc.value, "words": w.value, "n_sets": ns.value,
                "n_colored_columns": ncc.value, "device_bytes": db.value}

    def copy(self):
        """(ids uint32[n_nodes], table uint64[n_sets, W])"""
        ids = np.empty(self.index.n_nodes, dtype=np.uint32)
        table = np.empty((self.n_sets, self.words), dtype=np.uint64)
        _check(lib().sbwtgpu_colorsets_copy(self._h, ids.ctypes.data, table.ctypes.data))
        return ids, table

    def dev_ptrs(self):
        """(d_ids, d_table) raw device pointers"""
        a, b = C.c_void_p(), C.c_void_p()
        _check(lib().sbwtgpu_colorsets_dev(self._h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def unitigs_dev(self) -> "Unitigs":
        """sbwtgpu_unitigs_create_colored: the unitigs of the index cut where the colour set changes, device-resident."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_unitigs_create_colored(self._h, C.byref(h)))
        return Unitigs(h)

    def unitig_graph_dev(self, links: bool = True, column_map: bool = False) -> "Unitigs":
        """sbwtgpu_unitigs_create_graph on the object: the coloured unitigs with their links and / or the column map."""
        h = C.c_void_p()
        flags = (UNITIGS_LINKS if links else 0) | (UNITIGS_COLUMN_MAP if column_map else 0)
        _check(lib().sbwtgpu_unitigs_create_graph(None, self._h, flags, C.byref(h)))
        return Unitigs(h, self.index.n_nodes)

    def unitigs(self):
        """(bases, off, first_col, set_id): Index.unitigs() of the coloured unitigs, and uint32[n] the set id of each."""
        with self.unitigs_dev() as u:
            return u.copy() + (u.set_ids(),)

    def expand(self) -> "WideColors":
        """sbwtgpu_colorsets_expand: the wide colours object this one means."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_colorsets_expand(self._h, C.byref(h)))
        return WideColors(h, self.index, self.n_colors)

    def set_sizes(self) -> np.ndarray:
        """sbwtgpu_colorsets_set_sizes: int64[n_sets], the columns that carry each set (entry 0: dummy and uncoloured columns)."""
        out = np.full(self.n_sets, -12345, dtype=np.int64)
        _check(lib().sbwtgpu_colorsets_set_sizes(self._h, out.ctypes.data))
        return out

    def shared_kmers(self, weights=None) -> np.ndarray:
        """sbwtgpu_colorsets_shared_kmers: int64[n_colors, n_colors], G[a][b] = the sum over the sets that hold colours a and
        b of the set's weight -- by default its size, so that G[a][b] is the number of index k-mers references a and b share;
        or weights, n_sets integers in 0 .. 2^31 - 1 (entry 0 is ignored).  The call's info is left in self.shared_info."""
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.int64)
            if w.shape != (self.n_sets,):
                raise SbwtGpuError(ERR_INVALID_ARG, "weights of shape %s, the object has %d sets" % (w.shape, self.n_sets))
        out = np.full((self.n_colors, self.n_colors), -12345, dtype=np.int64)
        info = SharedInfoC()
        _check(lib().sbwtgpu_colorsets_shared_kmers(self._h, w.ctypes.data if w is not None else None, out.ctypes.data, C.byref(info)))
        self.shared_info = info.as_dict()
        return out

    def shared_workspace_bytes(self) -> int:
        """sbwtgpu_colorsets_shared_workspace_bytes: the workspace shared_kmers_dev needs for this object."""
        return int(lib().sbwtgpu_colorsets_shared_workspace_bytes(self._h))

    def shared_kmers_dev(self, d_weights: int, d_matrix: int, d_ws: int, ws_bytes: int, stream: int = 0) -> None:
        """sbwtgpu_colorsets_shared_kmers_dev (raw device pointers; d_weights 0 = the set sizes): asynchronous on stream.  The
        first int64 of the workspace is -1 afterwards unless a weight was out of range (then: the smallest such set)."""
        _check(lib().sbwtgpu_colorsets_shared_kmers_dev(self._h, d_weights or None, d_matrix or None, d_ws or None, ws_bytes,
                                                        stream or None))

    # ---- colour select: k-mers by a predicate over their colour sets (include/sbwtgpu.h) ----
    def screen(self) -> "Screen":
        """sbwtgpu_screen_create: an empty accumulator for screening read sets against this object's references."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_screen_create(self._h, C.byref(h)))
        return Screen(h, self)

    def color_mask(self, colors) -> np.ndarray:
        """uint64[W] with the bits of `colors`: an iterable of colour numbers, or a ready array of W uint64 words (taken as it
        is; the library refuses bits at or above n_colors)."""
        if isinstance(colors, np.ndarray) and colors.dtype == np.uint64:
            if colors.shape != (self.words,):
                raise SbwtGpuError(ERR_INVALID_ARG, "a colour mask of shape %s, %d colours need %d words"
                                   % (colors.shape, self.n_colors, self.words))
            return np.ascontiguousarray(colors)
        mask = np.zeros(self.words, dtype=np.uint64)
        for c in colors:
            c = int(c)
            if not 0 <= c < self.n_colors:
                raise SbwtGpuError(ERR_INVALID_ARG, "colour %d in a mask, the object has %d colours" % (c, self.n_colors))
            mask[c >> 6] |= np.uint64(1) << np.uint64(c & 63)
        return mask

    def _predicate(self, include, exclude, min_in, max_in):
        inc = self.color_mask(include)
        exc = self.color_mask(exclude) if exclude is not None else None
        if max_in is None:
            max_in = sum(bin(int(x)).count("1") for x in inc)
            max_in = max(max_in, min_in)                    # (a min_in above popcount(include) is legal and selects nothing)
        p = ColorPredicateC(inc.ctypes.data, exc.ctypes.data if exc is not None else None, int(min_in), int(max_in))
        return p, (inc, exc)

    def match_sets(self, include, exclude=None, min_in: int = 1, max_in: Optional[int] = None) -> np.ndarray:
        """sbwtgpu_colorsets_match_sets: uint8[n_sets], 1 where the table row has no colour of `exclude` and between min_in
        and max_in (default: all) colours of `include`."""
        p, keep = self._predicate(include, exclude, min_in, max_in)
        out = np.full(self.n_sets, 0xA5, dtype=np.uint8)
        _check(lib().sbwtgpu_colorsets_match_sets(self._h, C.byref(p), out.ctypes.data))
        return out

    def select_counts(self, include, exclude=None, min_in: int = 1, max_in: Optional[int] = None) -> dict:
        """sbwtgpu_colorsets_select_counts: n_real, n_selected and n_sets_matched of the predicate, nothing is built."""
        p, keep = self._predicate(include, exclude, min_in, max_in)
        info = ColorSelectInfoC()
        _check(lib().sbwtgpu_colorsets_select_counts(self._h, C.byref(p), C.byref(info)))
        return info.as_dict()

    def select(self, include, exclude=None, min_in: int = 1, max_in: Optional[int] = None, streaming_support: bool = True):
        """sbwtgpu_colorsets_select: (BuiltBits, info) of the index of the k-mers whose colour set matches.  A failed call
        raises SbwtGpuError with the counts the call got to as its `info`."""
        p, keep = self._predicate(include, exclude, min_in, max_in)
        out, info = PlainMatrixBitsC(), ColorSelectInfoC()
        rc = lib().sbwtgpu_colorsets_select(self._h, C.byref(p), int(streaming_support), C.byref(out), C.byref(info))
        if rc != OK:
            err = SbwtGpuError(rc, lib().sbwtgpu_last_error().decode(errors="replace"))
            err.info = info.as_dict()
            raise err
        return _take_bits(out), info.as_dict()

    def pseudoalign(self, bases, read_off, both_strands: bool = False, threshold_ppm: int = 1_000_000, denominator: int = 0,
                    counts: bool = False):
        """sbwtgpu_pseudoalign_sets_batch: what WideColors.pseudoalign returns -- (records, colors[, counts])."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = max(len(read_off) - 1, 0)
        out = np.zeros(n, dtype=READ_FOUND_DTYPE)
        out["n_kmers"] = -12345
        col = np.zeros((n, self.words), dtype=np.uint64)
        cnt = np.full((n, self.n_colors), -12345, dtype=np.int32) if counts else None
        _check(lib().sbwtgpu_pseudoalign_sets_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n, 2 if both_strands else 1,
                                                    threshold_ppm, denominator, out.ctypes.data, col.ctypes.data,
                                                    cnt.ctypes.data if counts else None))
        return (out, col, cnt) if counts else (out, col)

    def pseudoalign_reads(self, reads: Sequence[bytes], both_strands: bool = False, threshold_ppm: int = 1_000_000,
                          denominator: int = 0, counts: bool = False):
        """The same for a list of byte strings."""
        bases, off = concat_reads(reads)
        return self.pseudoalign(bases, off, both_strands, threshold_ppm, denominator, counts)

    def pseudoalign_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_out: int, d_colors: int, d_counts: int,
                        d_ws: int, ws_bytes: int, both_strands: bool = False, threshold_ppm: int = 1_000_000, denominator: int = 0,
                        stream: int = 0):
        """sbwtgpu_pseudoalign_sets_dev (raw device pointers, as WideColors.pseudoalign_dev)."""
        _check(lib().sbwtgpu_pseudoalign_sets_dev(self._h, d_bases, total_bases, d_read_off, n_reads, 2 if both_strands else 1,
                                                  threshold_ppm, denominator, d_out, d_colors, d_counts or None, d_ws, ws_bytes, stream))


class Screen(_Owner):
    """Owns an sbwtgpu_screen handle: the accumulator of a read set screened against the references of a colour-set object
    (include/sbwtgpu.h, "screen") -- per set and per colour the index k-mers, the distinct ones the sample holds and the hits.
    Everything is exact int64.  The colour sets (and through them the index) are kept referenced."""

    _destroy = "sbwtgpu_screen_destroy"

    def __init__(self, handle, sets: "ColorSets"):
        self._h = handle
        self.sets_object = sets
        self.n_sets, self.n_colors = sets.n_sets, sets.n_colors

    def add(self, bases, read_off, strands: int = 1) -> None:
        """sbwtgpu_screen_add_batch: the reads (uint8 bases, int64 offsets) join the sample; strands = 2 adds the reverse
        complement of every window too."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        _check(lib().sbwtgpu_screen_add_batch(self._h, bases.ctypes.data, read_off.ctypes.data, len(read_off) - 1, strands))

    def add_reads(self, reads: Sequence[bytes], strands: int = 1) -> None:
        bases, off = concat_reads(reads)
        self.add(bases, off, strands)

    def add_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_ws: int, ws_bytes: int, strands: int = 1,
                stream: int = 0) -> None:
        """sbwtgpu_screen_add_dev (raw device pointers; workspace of screen_workspace_bytes): asynchronous on stream."""
        _check(lib().sbwtgpu_screen_add_dev(self._h, d_bases or None, total_bases, d_read_off or None, n_reads, strands, d_ws or None,
                                            ws_bytes, stream or None))

    def info(self) -> dict:
        """n_windows, n_hits, n_seen, n_sets and n_colors."""
        nw, nh, ns, nt = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        nc = C.c_int32()
        _check(lib().sbwtgpu_screen_info(self._h, C.byref(nw), C.byref(nh), C.byref(ns), C.byref(nt), C.byref(nc)))
        return {"n_windows": nw.value, "n_hits": nh.value, "n_seen": ns.value, "n_sets": nt.value, "n_colors": nc.value}

    def sets(self):
        """(set_kmers, set_seen, set_hits): int64[n_sets] each."""
        out = [np.full(self.n_sets, -12345, dtype=np.int64) for _ in range(3)]
        _check(lib().sbwtgpu_screen_sets(self._h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
        return tuple(out)

    def colors(self):
        """(ref_kmers, ref_seen, ref_hits): int64[n_colors] each."""
        out = [np.full(self.n_colors, -12345, dtype=np.int64) for _ in range(3)]
        _check(lib().sbwtgpu_screen_colors(self._h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
        return tuple(out)

    def seen(self) -> np.ndarray:
        """uint64[ceil(n / 64)]: bit v % 64 of word v // 64 says whether column v has a hit."""
        out = np.zeros((self.sets_object.index.n_nodes + 63) // 64, dtype=np.uint64)
        _check(lib().sbwtgpu_screen_seen_copy(self._h, out.ctypes.data))
        return out

    def seen_dev(self) -> int:
        p = C.c_void_p()
        _check(lib().sbwtgpu_screen_seen_dev(self._h, C.byref(p)))
        return p.value or 0

    def reset(self) -> None:
        _check(lib().sbwtgpu_screen_reset(self._h))


class _Placement(_Owner):
    """What Positions, OccurrencesBuilder and Occurrences share: a handle bound to its index (kept referenced), and the add and
    map calls, which differ between the classes in `_abi`, the prefix of their library functions, and in the arguments that
    the occurrence maps put behind `strands` (max_occ)."""

    _abi = ""

    def __init__(self, handle, index: Index):
        self._h = handle
        self.index = index
        self._destroy = self._abi + "_destroy"

    def _call(self, name: str, *args) -> None:
        _check(getattr(lib(), self._abi + name)(self._h, *args))

    def _add_batch(self, bases, read_off, first_seq: int, strands: int):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        nw, nh = C.c_int64(), C.c_int64()
        self._call("_add_batch", first_seq, bases.ctypes.data, read_off.ctypes.data, len(read_off) - 1, strands, C.byref(nw), C.byref(nh))
        return nw.value, nh.value

    def _map_batch(self, bases, read_off, strands: int, *extra) -> np.ndarray:
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = max(len(read_off) - 1, 0)
        out = np.zeros(n, dtype=READ_MAP_DTYPE)
        self._call("_map_batch", bases.ctypes.data, read_off.ctypes.data, n, strands, *extra, out.ctypes.data)
        return out

    def _map_dev(self, d_bases, total_bases, d_read_off, n_reads, d_out, d_ws, ws_bytes, stream, strands: int, *extra) -> None:
        self._call("_map_dev", d_bases or None, total_bases, d_read_off or None, n_reads, strands, *extra, d_out or None, d_ws or None,
                   ws_bytes, stream or None)

    @classmethod
    def _map_workspace_bytes(cls, total_bases: int, n_reads: int, strands: int) -> int:
        return getattr(lib(), cls._abi + "_map_workspace_bytes")(total_bases, n_reads, strands)


class Positions(_Placement):
    """Owns an sbwtgpu_positions handle: per column the smallest reference coordinate of its k-mer, and the reads placed on the
    references by diagonal voting (include/sbwtgpu.h, "positions").  Everything is exact integers.  The index is kept
    referenced."""

    _abi = "sbwtgpu_positions"

    @classmethod
    def upload(cls, index: Index, first) -> "Positions":
        """sbwtgpu_positions_upload: an object from a copied table (uint64[n_nodes])."""
        first = np.ascontiguousarray(first, dtype=np.uint64)
        if first.shape != (index.n_nodes,):
            raise ValueError("first must have one uint64 per column (%d), not shape %r" % (index.n_nodes, first.shape))
        h = C.c_void_p()
        _check(lib().sbwtgpu_positions_upload(index.handle, first.ctypes.data, C.byref(h)))
        return cls(h, index)

    def add_sequences(self, bases, read_off, first_seq: int, strands: int = 1):
        """sbwtgpu_positions_add_batch: sequence i of the batch gets the number first_seq + i.  Returns (n_windows,
        n_hit_windows) of the batch."""
        return self._add_batch(bases, read_off, first_seq, strands)

    def add(self, seqs: Sequence[bytes], first_seq: int, strands: int = 1):
        """The same for a list of byte strings."""
        return self._add_batch(*concat_reads(seqs), first_seq, strands)

    def info(self) -> dict:
        """n_columns, k, n_windows, n_hits, n_positioned and device_bytes."""
        v = [C.c_int64() for _ in range(6)]
        self._call("_info", *[C.byref(x) for x in v])
        return dict(zip(("n_columns", "k", "n_windows", "n_hits", "n_positioned", "device_bytes"), (x.value for x in v)))

    def first(self) -> np.ndarray:
        """uint64[n_nodes]: (seq << 32) | (pos << 1) | t per column, POS_NONE where the column has no position."""
        out = np.zeros(self.index.n_nodes, dtype=np.uint64)
        self._call("_first_copy", out.ctypes.data)
        return out

    def first_dev(self) -> int:
        p = C.c_void_p()
        self._call("_first_dev", C.byref(p))
        return p.value or 0

    def reset(self) -> None:
        self._call("_reset")

    def map(self, bases, read_off, strands: int = 1) -> np.ndarray:
        """sbwtgpu_positions_map_batch: one READ_MAP_DTYPE record per read."""
        return self._map_batch(bases, read_off, strands)

    def map_reads(self, reads: Sequence[bytes], strands: int = 1) -> np.ndarray:
        """The same for a list of byte strings."""
        return self._map_batch(*concat_reads(reads), strands)

    def map_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_out: int, d_ws: int, ws_bytes: int,
                strands: int = 1, stream: int = 0) -> None:
        """sbwtgpu_positions_map_dev (raw device pointers; d_out: n_reads records of 32 bytes; workspace of workspace_bytes):
        asynchronous on stream."""
        self._map_dev(d_bases, total_bases, d_read_off, n_reads, d_out, d_ws, ws_bytes, stream, strands)

    @staticmethod
    def workspace_bytes(total_bases: int, n_reads: int, strands: int = 1) -> int:
        return Positions._map_workspace_bytes(total_bases, n_reads, strands)


class OccurrencesBuilder(_Placement):
    """Owns an sbwtgpu_occurrences_builder handle: the log of (column, key) hits that finish() turns into an Occurrences object
    (include/sbwtgpu.h, "occurrences").  Adds from several threads are safe; they are serialised.  The index is kept
    referenced."""

    _abi = "sbwtgpu_occurrences_builder"

    def add_sequences(self, bases, read_off, first_seq: int, strands: int = 1):
        """sbwtgpu_occurrences_builder_add_batch: sequence i of the batch gets the number first_seq + i.  Returns (n_windows,
        n_hit_windows) of the batch."""
        return self._add_batch(bases, read_off, first_seq, strands)

    def add(self, seqs: Sequence[bytes], first_seq: int, strands: int = 1):
        """The same for a list of byte strings."""
        return self._add_batch(*concat_reads(seqs), first_seq, strands)

    def finish(self) -> "Occurrences":
        """sbwtgpu_occurrences_builder_finish: the object; the builder is consumed."""
        h = C.c_void_p()
        self._call("_finish", C.byref(h))
        self._h = None
        return Occurrences(h, self.index)


class Occurrences(_Placement):
    """Owns an sbwtgpu_occurrences handle: every reference coordinate of every column's k-mer as CSR arrays (off, occ), and the
    reads placed on the references by diagonal voting over all of them (include/sbwtgpu.h, "occurrences").  Everything is exact
    integers.  The index is kept referenced."""

    _abi = "sbwtgpu_occurrences"

    @classmethod
    def upload(cls, index: Index, off, occ) -> "Occurrences":
        """sbwtgpu_occurrences_upload: an object from copied arrays (off uint64[n_nodes + 1], occ uint64[off[-1]])."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        occ = np.ascontiguousarray(occ, dtype=np.uint64)
        if off.shape != (index.n_nodes + 1,):
            raise ValueError("off must have n_nodes + 1 = %d entries, not shape %r" % (index.n_nodes + 1, off.shape))
        h = C.c_void_p()
        _check(lib().sbwtgpu_occurrences_upload(index.handle, off.ctypes.data, occ.ctypes.data if len(occ) else None, len(occ), C.byref(h)))
        return cls(h, index)

    def info(self) -> dict:
        """n_columns, k, n_windows, n_hits, n_occurrences, n_positioned, max_count and device_bytes."""
        v = [C.c_int64() for _ in range(8)]
        self._call("_info", *[C.byref(x) for x in v])
        return dict(zip(("n_columns", "k", "n_windows", "n_hits", "n_occurrences", "n_positioned", "max_count", "device_bytes"),
                        (x.value for x in v)))

    def offsets(self) -> np.ndarray:
        """uint64[n_nodes + 1]: column v's keys are keys()[off[v]:off[v + 1]]."""
        out = np.zeros(self.index.n_nodes + 1, dtype=np.uint64)
        self._call("_offsets_copy", out.ctypes.data)
        return out

    def keys(self) -> np.ndarray:
        """uint64[n_occurrences]: (seq << 32) | (pos << 1) | t, strictly ascending within a column."""
        out = np.zeros(self.info()["n_occurrences"], dtype=np.uint64)
        self._call("_keys_copy", out.ctypes.data if len(out) else None)
        return out

    def offsets_dev(self) -> int:
        p = C.c_void_p()
        self._call("_offsets_dev", C.byref(p))
        return p.value or 0

    def keys_dev(self) -> int:
        p = C.c_void_p()
        self._call("_keys_dev", C.byref(p))
        return p.value or 0

    def positions(self) -> "Positions":
        """sbwtgpu_occurrences_to_positions: the Positions object with first[v] = the smallest key of column v."""
        h = C.c_void_p()
        self._call("_to_positions", C.byref(h))
        return Positions(h, self.index)

    def map(self, bases, read_off, strands: int = 1, max_occ: int = 1024) -> np.ndarray:
        """sbwtgpu_occurrences_map_batch: one READ_MAP_DTYPE record per read."""
        return self._map_batch(bases, read_off, strands, max_occ)

    def map_reads(self, reads: Sequence[bytes], strands: int = 1, max_occ: int = 1024) -> np.ndarray:
        """The same for a list of byte strings."""
        return self._map_batch(*concat_reads(reads), strands, max_occ)

    def map_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_out: int, d_ws: int, ws_bytes: int,
                strands: int = 1, max_occ: int = 1024, stream: int = 0) -> None:
        """sbwtgpu_occurrences_map_dev (raw device pointers; d_out: n_reads records of 32 bytes; workspace of workspace_bytes):
        asynchronous on stream."""
        self._map_dev(d_bases, total_bases, d_read_off, n_reads, d_out, d_ws, ws_bytes, stream, strands, max_occ)

    @staticmethod
    def workspace_bytes(total_bases: int, n_reads: int, strands: int = 1) -> int:
        return Occurrences._map_workspace_bytes(total_bases, n_reads, strands)


class RefSeqs(_Owner):
    """Owns an sbwtgpu_refseqs handle: the reference sequences packed on the device (2 bits and one validity bit per base), and
    the verification of mapped reads against them: per read the mismatches on the voted diagonal and the best edit distance in
    a window around it (include/sbwtgpu.h, "reference sequences and verification").  Everything is exact integers.  Needs no
    index.  The verify calls must not run while an add does."""

    _destroy = "sbwtgpu_refseqs_destroy"

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def create(cls, device: int = 0) -> "RefSeqs":
        h = C.c_void_p()
        _check(lib().sbwtgpu_refseqs_create(device, C.byref(h)))
        return cls(h)

    def add_sequences(self, bases, read_off, first_seq: Optional[int] = None) -> None:
        """sbwtgpu_refseqs_add_batch: sequence i of the batch gets the number first_seq + i, which must be the next number
        (None: whatever it is)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        if first_seq is None:
            first_seq = self.info()["n_seqs"]
        _check(lib().sbwtgpu_refseqs_add_batch(self._h, first_seq, bases.ctypes.data, read_off.ctypes.data, max(len(read_off) - 1, 0)))

    def add(self, seqs: Sequence[bytes], first_seq: Optional[int] = None) -> None:
        """The same for a list of byte strings."""
        self.add_sequences(*concat_reads(seqs), first_seq)

    def info(self) -> dict:
        """n_seqs, total_bases, n_invalid (bases that are not upper-case ACGT) and device_bytes."""
        v = [C.c_int64() for _ in range(4)]
        _check(lib().sbwtgpu_refseqs_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("n_seqs", "total_bases", "n_invalid", "device_bytes"), (x.value for x in v)))

    def lengths(self) -> np.ndarray:
        out = np.zeros(self.info()["n_seqs"], dtype=np.int64)
        _check(lib().sbwtgpu_refseqs_lengths_copy(self._h, out.ctypes.data if len(out) else None))
        return out

    def get(self, seq: int, pos: int = 0, length: Optional[int] = None) -> bytes:
        """sbwtgpu_refseqs_get: bases pos .. pos + length of sequence seq as ASCII, N for an invalid base (None: to its end)."""
        if length is None:
            lens = self.lengths()
            length = int(lens[seq]) - pos if 0 <= seq < len(lens) else 0
        out = np.zeros(max(length, 0), dtype=np.uint8)
        _check(lib().sbwtgpu_refseqs_get(self._h, seq, pos, length, out.ctypes.data if len(out) else None))
        return out.tobytes()

    def verify(self, bases, read_off, records, band: int = 8) -> np.ndarray:
        """sbwtgpu_refseqs_verify_batch: one READ_VERIFY_DTYPE record per read from its READ_MAP_DTYPE record (seq, strand and
        start are read)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        records = np.ascontiguousarray(records, dtype=READ_MAP_DTYPE)
        n = max(len(read_off) - 1, 0)
        if len(records) != n:
            raise ValueError("%d map records for %d reads" % (len(records), n))
        out = np.zeros(n, dtype=READ_VERIFY_DTYPE)
        _check(lib().sbwtgpu_refseqs_verify_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n, records.ctypes.data if n else None,
                                                  band, out.ctypes.data if n else None))
        return out

    def verify_reads(self, reads: Sequence[bytes], records, band: int = 8) -> np.ndarray:
        """The same for a list of byte strings."""
        return self.verify(*concat_reads(reads), records, band)

    def verify_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_map: int, d_out: int, d_ws: int, ws_bytes: int,
                   band: int = 8, stream: int = 0) -> None:
        """sbwtgpu_refseqs_verify_dev (raw device pointers; d_map: n_reads records of 32 bytes; d_out: n_reads records of 16 bytes;
        workspace of workspace_bytes): asynchronous on stream."""
        _check(lib().sbwtgpu_refseqs_verify_dev(self._h, d_bases or None, total_bases, d_read_off or None, n_reads, d_map or None, band,
                                                d_out or None, d_ws or None, ws_bytes, stream or None))

    @staticmethod
    def workspace_bytes(total_bases: int, n_reads: int) -> int:
        return int(lib().sbwtgpu_refseqs_verify_workspace_bytes(total_bases, n_reads))

    def align(self, bases, read_off, records, band: int = 8):
        """sbwtgpu_align_batch: (verify, align, op_off, ops).  verify is what verify() gives; align holds one READ_ALIGN_DTYPE
        record per read; read i's runs are ops[op_off[i]:op_off[i + 1]] (uint32, length << 4 | code; cigar_string)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        records = np.ascontiguousarray(records, dtype=READ_MAP_DTYPE)
        n = max(len(read_off) - 1, 0)
        if len(records) != n:
            raise ValueError("%d map records for %d reads" % (len(records), n))
        verify = np.zeros(n, dtype=READ_VERIFY_DTYPE)
        out = np.zeros(n, dtype=READ_ALIGN_DTYPE)
        op_off = np.zeros(n + 1, dtype=np.int64)
        p, total = C.c_void_p(), C.c_int64(0)
        _check(lib().sbwtgpu_align_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n, records.ctypes.data if n else None, band,
                                         verify.ctypes.data if n else None, out.ctypes.data if n else None, op_off.ctypes.data,
                                         C.byref(p), C.byref(total)))
        try:
            ops = np.empty(total.value, dtype=np.uint32)
            if total.value:
                C.memmove(ops.ctypes.data, p.value, total.value * 4)
        finally:
            if p.value:
                lib().sbwtgpu_free_host(p)
        return verify, out, op_off, ops

    def align_reads(self, reads: Sequence[bytes], records, band: int = 8):
        """The same for a list of byte strings."""
        return self.align(*concat_reads(reads), records, band)

    def align_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_map: int, d_verify_out: int, d_out: int,
                  d_op_off: int, d_ops: int, ops_cap: int, d_ws: int, ws_bytes: int, band: int = 8, stream: int = 0) -> None:
        """sbwtgpu_align_dev (raw device pointers; d_verify_out and d_out: n_reads records of 16 bytes; d_op_off: n_reads + 1
        int64; d_ops: ops_cap uint32; workspace of align_workspace_bytes): asynchronous on stream."""
        _check(lib().sbwtgpu_align_dev(self._h, d_bases or None, total_bases, d_read_off or None, n_reads, d_map or None, band,
                                       d_verify_out or None, d_out or None, d_op_off or None, d_ops or None, ops_cap, d_ws or None,
                                       ws_bytes, stream or None))

    @staticmethod
    def align_workspace_bytes(total_bases: int, n_reads: int) -> int:
        return int(lib().sbwtgpu_align_workspace_bytes(total_bases, n_reads))

    def pileup(self) -> "Pileup":
        """sbwtgpu_pileup_create: an empty pileup over the sequences the object holds now."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_pileup_create(self._h, C.byref(h)))
        return Pileup(h, self)


def pileup_filter(min_votes: int = 0, unique: bool = False, max_edit: int = -1, reserved: int = 0) -> np.ndarray:
    """One PILEUP_FILTER_DTYPE record."""
    f = np.zeros(1, dtype=PILEUP_FILTER_DTYPE)
    f[0] = (min_votes, 1 if unique else 0, max_edit, reserved)
    return f


class Pileup(_Owner):
    """Owns an sbwtgpu_pileup handle: the per-base counters of a read set's alignments on the sequences of a RefSeqs object,
    which live on the device across adds (include/sbwtgpu.h, "pileup of aligned reads").  Everything is exact integers.  The
    RefSeqs object is kept referenced and must not be added to while a call on the pileup runs."""

    _destroy = "sbwtgpu_pileup_destroy"

    def __init__(self, handle, refseqs: "RefSeqs"):
        self._h = handle
        self.refseqs = refseqs

    def add(self, bases, read_off, records, band: int = 8, min_votes: int = 0, unique: bool = False, max_edit: int = -1) -> None:
        """sbwtgpu_pileup_add_batch: the reads (uint8 bases, int64 offsets) with their READ_MAP_DTYPE records are verified,
        aligned and, where the filter passes, piled."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        records = np.ascontiguousarray(records, dtype=READ_MAP_DTYPE)
        n = max(len(read_off) - 1, 0)
        if len(records) != n:
            raise ValueError("%d map records for %d reads" % (len(records), n))
        f = pileup_filter(min_votes, unique, max_edit)
        _check(lib().sbwtgpu_pileup_add_batch(self._h, bases.ctypes.data, read_off.ctypes.data, n, records.ctypes.data if n else None, band,
                                              f.ctypes.data))

    def add_reads(self, reads: Sequence[bytes], records, band: int = 8, min_votes: int = 0, unique: bool = False, max_edit: int = -1) -> None:
        """The same for a list of byte strings."""
        self.add(*concat_reads(reads), records, band, min_votes, unique, max_edit)

    def add_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_map: int, d_ws: int, ws_bytes: int, band: int = 8,
                min_votes: int = 0, unique: bool = False, max_edit: int = -1, stream: int = 0) -> None:
        """sbwtgpu_pileup_add_dev (raw device pointers; d_map: n_reads records of 32 bytes; workspace of workspace_bytes):
        asynchronous on stream."""
        f = pileup_filter(min_votes, unique, max_edit)
        _check(lib().sbwtgpu_pileup_add_dev(self._h, d_bases or None, total_bases, d_read_off or None, n_reads, d_map or None, band,
                                            f.ctypes.data, d_ws or None, ws_bytes, stream or None))

    def add_aligned_dev(self, d_bases: int, total_bases: int, d_read_off: int, n_reads: int, d_map: int, d_verify: int, d_align: int,
                        d_op_off: int, d_ops: int, min_votes: int = 0, unique: bool = False, max_edit: int = -1, stream: int = 0) -> None:
        """sbwtgpu_pileup_add_aligned_dev (raw device pointers: what align_dev took and wrote, every run stored): asynchronous on
        stream."""
        f = pileup_filter(min_votes, unique, max_edit)
        _check(lib().sbwtgpu_pileup_add_aligned_dev(self._h, d_bases or None, total_bases, d_read_off or None, n_reads, d_map or None,
                                                    d_verify or None, d_align or None, d_op_off or None, d_ops or None, f.ctypes.data,
                                                    stream or None))

    @staticmethod
    def workspace_bytes(total_bases: int, n_reads: int) -> int:
        return int(lib().sbwtgpu_pileup_workspace_bytes(total_bases, n_reads))

    def info(self) -> dict:
        """n_seqs, total_bases, n_offered, n_piled, n_columns (the sum of depth), n_clipped, n_overhang and device_bytes."""
        v = [C.c_int64() for _ in range(8)]
        _check(lib().sbwtgpu_pileup_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("n_seqs", "total_bases", "n_offered", "n_piled", "n_columns", "n_clipped", "n_overhang", "device_bytes"),
                        (x.value for x in v)))

    def counts(self, seq: int, pos: int = 0, length: Optional[int] = None) -> np.ndarray:
        """sbwtgpu_pileup_counts_copy: the PILEUP_BASE_DTYPE records of bases pos .. pos + length of sequence seq (None: to its
        end)."""
        if length is None:
            lens = self.refseqs.lengths()
            length = int(lens[seq]) - pos if 0 <= seq < len(lens) else 0
        out = np.zeros(max(length, 0), dtype=PILEUP_BASE_DTYPE)
        _check(lib().sbwtgpu_pileup_counts_copy(self._h, seq, pos, length, out.ctypes.data if len(out) else None))
        return out

    def counts_dev(self, seq: int, pos: int, length: int, d_out: int, stream: int = 0) -> None:
        """sbwtgpu_pileup_counts_dev (d_out: length records of 32 bytes on the device): asynchronous on stream."""
        _check(lib().sbwtgpu_pileup_counts_dev(self._h, seq, pos, length, d_out or None, stream or None))

    def calls(self, min_depth: int = 1, min_alt: int = 1, min_frac_ppm: int = 0) -> np.ndarray:
        """sbwtgpu_pileup_calls: the PILEUP_CALL_DTYPE records in ascending (seq, pos, allele)."""
        p, n = C.c_void_p(), C.c_int64(0)
        _check(lib().sbwtgpu_pileup_calls(self._h, min_depth, min_alt, min_frac_ppm, C.byref(p), C.byref(n)))
        try:
            out = np.empty(n.value, dtype=PILEUP_CALL_DTYPE)
            if n.value:
                C.memmove(out.ctypes.data, p.value, n.value * PILEUP_CALL_DTYPE.itemsize)
        finally:
            if p.value:
                lib().sbwtgpu_free_host(p)
        return out

    def reset(self) -> None:
        _check(lib().sbwtgpu_pileup_reset(self._h))


class ColorSetsBuilder(_Owner):
    """Owns an sbwtgpu_colorsets_builder handle: colour sets made one colour at a time, without the wide matrix
    (include/sbwtgpu.h, "the builder").  The sequences of one colour come in consecutive add calls; finish() gives the
    ColorSets that ColorSets.from_colors gives for a WideColors coloured by the same adds, and consumes the builder.  Not
    thread-safe.  The index is kept referenced."""

    _destroy = "sbwtgpu_colorsets_builder_destroy"

    def __init__(self, handle, index: Index, n_colors: int):
        self._h = handle
        self.index, self.n_colors = index, n_colors
        self.words = (n_colors + 63) // 64

    @classmethod
    def create(cls, index: Index, n_colors: int) -> "ColorSetsBuilder":
        """An empty builder of n_colors colours (1 .. MAX_COLORS)."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_colorsets_builder_create(index.handle, n_colors, C.byref(h)))
        return cls(h, index, n_colors)

    def add_sequences(self, color: int, bases, read_off, both_strands: bool = False):
        """sbwtgpu_colorsets_builder_add_batch: marks every k-mer of the sequences that the index holds for `color`, which
        opens (closing the colour that was open); (n_windows, n_hit_windows)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        nw, nh = C.c_int64(0), C.c_int64(0)
        _check(lib().sbwtgpu_colorsets_builder_add_batch(self._h, color, bases.ctypes.data, read_off.ctypes.data,
                                                         max(len(read_off) - 1, 0), 2 if both_strands else 1, C.byref(nw), C.byref(nh)))
        return nw.value, nh.value

    def add_reads(self, color: int, reads: Sequence[bytes], both_strands: bool = False):
        """The same for a list of byte strings."""
        bases, off = concat_reads(reads)
        return self.add_sequences(color, bases, off, both_strands)

    def info(self) -> dict:
        """The state as of the last closed colour: n_columns, k, n_colors, words, n_sets, n_colored_columns, per_color (the
        columns marked when a colour was closed; 0 for new and open colours) and device_bytes."""
        n, k, ns, ncc, db = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        nc, w = C.c_int32(), C.c_int32()
        per = np.zeros(self.n_colors, dtype=np.int64)
        _check(lib().sbwtgpu_colorsets_builder_info(self._h, C.byref(n), C.byref(k), C.byref(nc), C.byref(w), C.byref(ns), C.byref(ncc),
                                                    per.ctypes.data, C.byref(db)))
        return {"n_columns": n.value, "k": k.value, "n_colors": nc.value, "words": w.value, "n_sets": ns.value,
                "n_colored_columns": ncc.value, "per_color": [int(x) for x in per], "device_bytes": db.value}

    def finish(self) -> ColorSets:
        """sbwtgpu_colorsets_builder_finish: closes the open colour and returns the canonical colour-set object."""
        h = C.c_void_p()
        _check(lib().sbwtgpu_colorsets_builder_finish(self._h, C.byref(h)))
        return ColorSets(h, self.index)


def kernel_times() -> list:
    """Durations (ms) of the dominant kernel of the search calls since set_tuning("kernel_events", 1)."""
    buf = (C.c_double * 256)()
    n = C.c_int64(0)
    _check(lib().sbwtgpu_kernel_times(buf, 256, C.byref(n)))
    return [float(buf[i]) for i in range(n.value)]


def search_workspace_bytes(total_bases: int) -> int:
    return int(lib().sbwtgpu_search_workspace_bytes(total_bases))


def ms_workspace_bytes(total_bases: int) -> int:
    return int(lib().sbwtgpu_ms_workspace_bytes(total_bases))


def read_hits_workspace_bytes(total_bases: int, n_reads: int, both_strands: bool = False) -> int:
    return int(lib().sbwtgpu_read_hits_workspace_bytes(total_bases, n_reads, 2 if both_strands else 1))


def walks_workspace_bytes(total_bases: int, n_reads: int) -> int:
    return int(lib().sbwtgpu_unitigs_walks_workspace_bytes(total_bases, n_reads))


def genotype_workspace_bytes(total_bases: int, n_reads: int, strands: int = 1) -> int:
    return int(lib().sbwtgpu_genotype_workspace_bytes(total_bases, n_reads, strands))


def screen_workspace_bytes(total_bases: int, n_reads: int, strands: int = 1) -> int:
    return int(lib().sbwtgpu_screen_workspace_bytes(total_bases, n_reads, strands))


def pseudoalign_workspace_bytes(total_bases: int, n_reads: int, both_strands: bool = False) -> int:
    return int(lib().sbwtgpu_pseudoalign_workspace_bytes(total_bases, n_reads, 2 if both_strands else 1))
