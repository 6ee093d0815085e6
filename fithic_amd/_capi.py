"""ctypes binding of libfithic_mi355x.so (the C ABI declared in include/fithic_mi355x.h).

The product path has NO CPU fallback: if the shared library is missing this module raises at import of
the symbols, and every kernel entry point fails loudly (FHX_ERR_NO_DEVICE) without a GPU.
"""
import ctypes
import os
import subprocess

import numpy as np

from . import _loader

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = _loader.LIB_PATH
CSRC = os.path.join(_PKG, "csrc")

FHX_OK = 0
FHX_ERR_ARG, FHX_ERR_NO_DEVICE, FHX_ERR_HIP, FHX_ERR_UNSUPPORTED, FHX_ERR_REFERENCE_EXIT, FHX_ERR_NOMEM, FHX_ERR_INTERNAL = -1, -2, -3, -4, -5, -6, -7
MODE_INTRA_ONLY, MODE_INTER_ONLY, MODE_ALL = 0, 1, 2
# FHX_TOTALS_*: how bdtrc sees a total of counts that does not fit a C int (include/fithic_mi355x.h; fithic.py:1070, 1101)
TOTALS_REFERENCE, TOTALS_WIDE = 0, 1
INT64_MAX = (1 << 63) - 1

# enum fhx_array
(A_HIST_SUMCC, A_HIST_NPAIRS, A_BIN_LB, A_BIN_UB, A_BIN_POSS, A_BIN_SUMCC, A_BIN_SUMDIST, A_BIN_POSS7, A_X, A_Y,
 A_KNOTS, A_COEFFS, A_TABLE_X, A_TABLE_Y0, A_TABLE_Y, A_OUTLIER_DIST_HIST, A_FDR_COUNTS, A_BIN_POSS0, A_DIST_KEYS,
 A_OUTLIER_DISTS) = range(20)
_ARRAY_DTYPE = {A_BIN_SUMDIST: np.float64, A_X: np.float64, A_Y: np.float64, A_KNOTS: np.float64,
                A_COEFFS: np.float64, A_TABLE_Y0: np.float64, A_TABLE_Y: np.float64}


class FhxParams(ctypes.Structure):
    _fields_ = [("resolution", ctypes.c_int64), ("dist_low", ctypes.c_int64), ("dist_up", ctypes.c_int64),
                ("n_bins", ctypes.c_int32), ("mapp_thres", ctypes.c_int32), ("mode", ctypes.c_int32),
                ("totals", ctypes.c_int32), ("bias_low", ctypes.c_double), ("bias_up", ctypes.c_double)]


class FhxStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("n_rows", "inter_count", "inter_sum", "intra_all_count", "intra_all_sum",
                                              "in_range_count", "in_range_sum", "max_count", "n_dist", "n_skipped")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class FhxFitInfo(ctypes.Structure):
    _fields_ = [("n_bins_made", ctypes.c_int32), ("n_knots", ctypes.c_int32), ("spline_ier", ctypes.c_int32),
                ("spline_restarted", ctypes.c_int32), ("n_table", ctypes.c_int64), ("n_frags", ctypes.c_int64),
                ("possible_intra_in_range", ctypes.c_int64), ("possible_inter_all", ctypes.c_double),
                ("possible_intra_all", ctypes.c_double), ("max_possible_dist", ctypes.c_double),
                ("inter_chr_prob", ctypes.c_double), ("baseline_intra_prob", ctypes.c_double),
                ("spline_s", ctypes.c_double), ("spline_fp", ctypes.c_double), ("residual", ctypes.c_double),
                ("bh_total_tests", ctypes.c_double), ("outlier_thres", ctypes.c_double),
                ("totals", ctypes.c_int32), ("totals_narrowed", ctypes.c_int32), ("bdtrc_n_intra", ctypes.c_int64),
                ("bdtrc_n_inter", ctypes.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# every symbol include/fithic_mi355x.h declares: name -> (restype, argtypes)
_P = ctypes.c_void_p
_I32P = ctypes.POINTER(ctypes.c_int32)
_I64P = ctypes.POINTER(ctypes.c_int64)
_F64P = ctypes.POINTER(ctypes.c_double)
SYMBOLS = {
    "fhx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_P)]),
    "fhx_destroy": (None, [_P]),
    "fhx_last_error": (ctypes.c_char_p, [_P]),
    "fhx_version": (ctypes.c_char_p, []),
    "fhx_warmup": (ctypes.c_int, [ctypes.c_int]),
    "fhx_set_params": (ctypes.c_int, [_P, ctypes.POINTER(FhxParams)]),
    "fhx_run_pass": (ctypes.c_int, [_P, ctypes.POINTER(FhxStats), ctypes.POINTER(FhxFitInfo)]),
    "fhx_load_fragments": (ctypes.c_int, [_P, _I32P, _I32P, _I32P, ctypes.c_int64, _I32P, ctypes.c_int32]),
    "fhx_host_inflate": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.POINTER(_P)]),
    "fhx_text_bytes": (ctypes.c_int64, [_P]),
    "fhx_text_copy": (ctypes.c_int, [_P, _P, ctypes.c_int64]),
    "fhx_text_error": (ctypes.c_char_p, [_P]),
    "fhx_host_parse_text": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_P)]),
    "fhx_text_free": (None, [_P]),
    "fhx_ingest_contacts_text": (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)]),
    "fhx_ingest_contacts_name": (ctypes.c_char_p, [_P, ctypes.c_int32]),
    "fhx_ingest_contacts_file": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
                                                ctypes.POINTER(ctypes.c_int32)]),
    "fhx_debug_inflate_file": (ctypes.c_int, [_P, ctypes.c_char_p, _P, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "fhx_ingest_contacts_commit": (ctypes.c_int, [_P, _I32P, ctypes.c_int32]),
    "fhx_ingest_contacts_discard": (None, [_P]),
    "fhx_fetch_pairs": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, _I32P, _I32P, _I32P, _I32P, _I32P]),
    "fhx_load_bias": (ctypes.c_int, [_P, _I32P, _I32P, _F64P, ctypes.c_int64]),
    "fhx_load_pairs": (ctypes.c_int, [_P, _I32P, _I32P, _I32P, _I32P, _I32P, ctypes.c_int64]),
    "fhx_load_pairs_device": (ctypes.c_int, [_P, _P, _P, _P, _P, _P, ctypes.c_int64, _P]),
    "fhx_pass_stats": (ctypes.c_int, [_P, ctypes.POINTER(FhxStats)]),
    "fhx_set_global_stats": (ctypes.c_int, [_P, ctypes.POINTER(FhxStats), _I64P, _I64P, ctypes.c_int64]),
    "fhx_set_dist_keys": (ctypes.c_int, [_P, _I64P, ctypes.c_int64]),
    "fhx_set_outlier_dists": (ctypes.c_int, [_P, _I64P, ctypes.c_int64]),
    "fhx_set_outlier_dist_hist": (ctypes.c_int, [_P, _I64P, ctypes.c_int64]),
    "fhx_make_bins": (ctypes.c_int, [_P, _I32P]),
    "fhx_fit": (ctypes.c_int, [_P, ctypes.POINTER(FhxFitInfo)]),
    "fhx_pvalues": (ctypes.c_int, [_P]),
    "fhx_bh": (ctypes.c_int, [_P, ctypes.c_double]),
    "fhx_sync": (ctypes.c_int, [_P]),
    "fhx_set_global_rows": (ctypes.c_int, [_P, _I64P, ctypes.c_int64]),
    "fhx_get_skip_limit": (ctypes.c_int64, [_P]),
    "fhx_set_skip_limit": (ctypes.c_int, [_P, ctypes.c_int64]),
    "fhx_next_pass": (ctypes.c_int, [_P, _I64P]),
    "fhx_reset_passes": (ctypes.c_int, [_P]),
    "fhx_get_stats": (ctypes.c_int, [_P, ctypes.POINTER(FhxStats)]),
    "fhx_fetch": (ctypes.c_int, [_P, _F64P, _F64P, _F64P, _F64P, _F64P]),
    "fhx_fetch_flags": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8)]),
    "fhx_fetch_outlier_rows": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    "fhx_get_array": (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_int64, _I64P]),
    "fhx_device_ptr": (_P, [_P, ctypes.c_int]),
    "fhx_n_sorted": (ctypes.c_int64, [_P]),
    "fhx_bh_sort_stats": (ctypes.c_int, [_P, _I64P]),
    "fhx_k3_pass_info": (ctypes.c_int, [_P, _I64P]),
    "fhx_debug_k3_tiles_per_group": (ctypes.c_int, [_P, ctypes.c_int]),
    "fhx_debug_device_blocks": (ctypes.c_int, [_I64P, _I64P]),
    "fhx_debug_k1_wide": (ctypes.c_int, [_P, ctypes.c_int]),
    "fhx_k3_compact_variant": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int32)]),
    "fhx_kernel_seconds": (ctypes.c_int, [_P, _F64P, _F64P, _F64P]),
    "fhx_kernel_seconds_total": (ctypes.c_int, [_P, _F64P, _I64P, ctypes.c_int]),
    "fhx_kernel_events_dropped": (ctypes.c_int, [_P, _I64P]),
    "fhx_k2_heavy_launch": (ctypes.c_int, [_P, _F64P, _I64P]),
    "fhx_k2_heavy_clock": (ctypes.c_int, [_P, _F64P]),
    "fhx_k2_class_rows": (ctypes.c_int, [_P, _I64P]),
    "fhx_bdtrc_array": (ctypes.c_int, [_P, ctypes.c_double, _I32P, _F64P, ctypes.c_int64, _F64P]),
    "fhx_debug_format": (ctypes.c_int, [_P, _F64P, ctypes.c_int64, ctypes.c_int32, ctypes.c_char_p, _I32P]),
    "fhx_debug_contfrac": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _F64P, _F64P, _F64P, ctypes.c_int64, _F64P]),
    "fhx_debug_lean_div": (ctypes.c_int, [_P, _F64P, _F64P, ctypes.c_int64, _F64P]),
    "fhx_debug_table_div": (ctypes.c_int, [_P, ctypes.c_int, _F64P, ctypes.c_int64, _F64P, _I32P]),
    "fhx_debug_classify": (ctypes.c_int, [_P, ctypes.c_double, _I32P, _F64P, ctypes.c_int64, _I32P, _I32P, _F64P]),
    "fhx_debug_k2_rows": (ctypes.c_int, [_P, ctypes.c_double, ctypes.c_double, _I32P, _F64P, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int64,
                                         ctypes.c_int32, _F64P, _I64P, _I64P, _I64P, ctypes.c_int64]),
    "fhx_bh_array": (ctypes.c_int, [_P, _F64P, ctypes.c_int64, ctypes.c_double, _F64P]),
    "fhx_bh_top_hist": (ctypes.c_int, [_P, _I64P, ctypes.c_int64]),
    "fhx_bh_set_cutoff": (ctypes.c_int, [_P, _I64P, ctypes.c_int64, ctypes.c_double]),
    "fhx_bh_top_hist_device": (ctypes.c_int, [_P]),
    "fhx_bh_set_cutoff_device": (ctypes.c_int, [_P, ctypes.c_double]),
    "fhx_bh_local_sort": (ctypes.c_int, [_P]),
    "fhx_bh_apply_sorted": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P, _F64P]),
    "fhx_sort_u64": (ctypes.c_int, [_P, _P, ctypes.c_int64, _P, _P]),
    "fhx_bh_scatter": (ctypes.c_int, [_P, _P]),
    "fhx_memcpy_d2d": (ctypes.c_int, [_P, _P, _P, ctypes.c_int64]),
    "fhx_comm_unique_id": (ctypes.c_int, [_P, ctypes.c_int64]),
    "fhx_comm_init": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int]),
    "fhx_comm_init_custom": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int]),
    "fhx_comm_destroy": (ctypes.c_int, [_P]),
    "fhx_comm_info": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "fhx_run_pass_distributed": (ctypes.c_int, [_P, ctypes.POINTER(FhxFitInfo)]),
    "fhx_next_pass_distributed": (ctypes.c_int, [_P, _I64P]),
    "fhx_pass_stats_distributed": (ctypes.c_int, [_P, ctypes.POINTER(FhxStats)]),
    "fhx_bh_distributed": (ctypes.c_int, [_P, ctypes.c_double]),
    "fhx_dist_stage_seconds": (ctypes.c_int, [_P, _F64P]),
    "fhx_dist_trace": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_int64, _I64P, ctypes.c_int]),
    "fhx_copy": (ctypes.c_int, [_P, _P, _P, ctypes.c_int64, ctypes.c_int]),
    "fhx_host_read_table": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_P)]),
    "fhx_table_rows": (ctypes.c_int64, [_P]),
    "fhx_table_n_names": (ctypes.c_int32, [_P]),
    "fhx_table_name": (ctypes.c_char_p, [_P, ctypes.c_int32]),
    "fhx_table_error": (ctypes.c_char_p, [_P]),
    "fhx_table_copy": (ctypes.c_int, [_P, ctypes.c_int32, _P]),
    "fhx_table_map_names": (ctypes.c_int, [_P, _I32P, ctypes.c_int32]),
    "fhx_table_free": (None, [_P]),
    "fhx_host_write_contacts": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, _I32P, _I32P, _I32P, _I32P,
                                               _I32P, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "fhx_host_write_significances": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, _I32P, _I32P, _I32P,
                                                    _I32P, _I32P, _F64P, _F64P, _F64P, _F64P, _F64P, ctypes.c_int64, ctypes.c_int32,
                                                    ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, _I64P]),
    "fhx_write_significances_device": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, _I32P, _I32P,
                                                      _I32P, _I32P, _I32P, ctypes.c_int64, _I64P, _I64P]),
    "fhx_write_significances_device_range": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, ctypes.c_int64,
                                                            ctypes.c_int64, ctypes.c_int32, _I64P, _I64P]),
    # the FDR subset of a pass from its resident columns (csrc/fhx_sigresident.hip)
    "fhx_significant_select": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint64,
                                              ctypes.c_int32, ctypes.c_int32, _I64P, _I64P, _I64P, _I32P, _I64P]),
    "fhx_significant_copy_text": (ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_int64]),
    "fhx_significant_copy_rows": (ctypes.c_int, [_P, _I64P, ctypes.c_int64]),
    # the interact track and the per-chromosome subsets from the same columns (csrc/fhx_sigresident_track.inc, fhx_sigresident_split.inc, both part of that unit)
    "fhx_significant_track": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint64,
                                             ctypes.c_int32, _I64P, _I64P, _I64P, _I64P, _I32P, _I64P]),
    "fhx_significant_copy_track": (ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_int64]),
    "fhx_significant_split": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint64,
                                             ctypes.c_int32, _I64P, _I32P, _I32P, _I64P]),
    "fhx_significant_split_counts": (ctypes.c_int, [_P, _I64P, _I64P, ctypes.c_int32]),
    "fhx_significant_split_names": (ctypes.c_int, [_P, ctypes.c_void_p, ctypes.c_int32]),
    "fhx_significant_copy_split": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]),
    "fhx_ingest_contacts_file_slice": (ctypes.c_int, [_P, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _I64P, _I32P, _I32P, _I32P]),
    "fhx_set_global_rows_range": (ctypes.c_int, [_P, ctypes.c_int64]),
    "fhx_text_part_bounds": (ctypes.c_int, [_P, ctypes.c_int32, ctypes.c_int32, _I64P, _I64P]),
    "fhx_ingest_contacts_text_slice": (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _I64P, _I32P]),
    "fhx_host_inflate_part": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(_P)]),
    "fhx_text_part_bytes": (ctypes.c_int64, [_P]),
    "fhx_text_part_is_last": (ctypes.c_int32, [_P]),
    "fhx_text_part_tail": (ctypes.c_int, [_P, _P, ctypes.c_int64]),
    "fhx_text_part_resolve": (ctypes.c_int, [_P, _P, ctypes.c_int64, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_uint32)]),
    "fhx_text_part_error": (ctypes.c_char_p, [_P]),
    "fhx_text_part_free": (None, [_P]),
    "fhx_crc32_combine": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int64]),
    "fhx_text_first_row_end": (ctypes.c_int64, [_P, _P, ctypes.c_int64]),
    "fhx_text_ends_with_newline": (ctypes.c_int32, [_P]),
    "fhx_ingest_contacts_text_own": (ctypes.c_int, [_P, _P, ctypes.c_int32, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int64, _I64P, _I32P]),
    "fhx_ingest_contacts_chr_counts": (ctypes.c_int, [_P, _I64P, ctypes.c_int32]),
    "fhx_ingest_contacts_commit_shard": (ctypes.c_int, [_P, _I32P, ctypes.POINTER(ctypes.c_uint8), ctypes.c_int32, _I64P]),
    "fhx_shard_segments": (ctypes.c_int, [_P, _I64P, _I64P, _I64P, ctypes.c_int64, _I64P]),
    "fhx_host_spline_fit": (ctypes.c_int, [_F64P, _F64P, ctypes.c_int32, ctypes.c_double, _F64P, _F64P, _I32P, _F64P, _I32P, _I32P]),
    "fhx_host_spline_eval": (ctypes.c_int, [_F64P, _F64P, ctypes.c_int32, _F64P, ctypes.c_int64, _F64P]),
    "fhx_host_pava_decreasing": (ctypes.c_int, [_F64P, ctypes.c_int64, _F64P]),
    "fhx_host_lbeta_table": (ctypes.c_int, [ctypes.c_double, ctypes.c_int64, _F64P, _F64P]),
    # Knight-Ruiz bias vectors (fithic/utils/HiCKRy.py)
    "fhx_kr_load_loci": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I32P, ctypes.c_int64]),
    "fhx_kr_load_pairs": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I32P, _I32P, _I32P, _F64P, ctypes.c_int64, _I64P]),
    "fhx_kr_load_pairs_resident": (ctypes.c_int, [ctypes.c_void_p, _P, _I64P]),
    "fhx_kr_shape": (ctypes.c_int, [ctypes.c_void_p, _I64P, _I64P, _I64P, _I64P]),
    "fhx_kr_get_csr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _I64P, _I32P, _F64P]),
    "fhx_kr_row_sums": (ctypes.c_int, [ctypes.c_void_p, _F64P]),
    "fhx_kr_remove_sparse": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, _I64P, _F64P, _I64P]),
    "fhx_kr_get_removed": (ctypes.c_int, [ctypes.c_void_p, _I64P, ctypes.c_int64, _I64P]),
    "fhx_kr_balance": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]),
    "fhx_kr_get_x": (ctypes.c_int, [ctypes.c_void_p, _F64P]),
    "fhx_kr_bias": (ctypes.c_int, [ctypes.c_void_p, _F64P]),
    "fhx_kr_spmv": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _F64P, _F64P, ctypes.c_int32, _F64P]),
    "fhx_kr_dot": (ctypes.c_int, [ctypes.c_void_p, _F64P, _F64P, ctypes.c_int64, _F64P]),
    # merging of nearby significant contacts (fithic/utils/CombineNearbyInteraction.py)
    "fhx_cni_load": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I64P, _I64P, _I64P, _F64P, _F64P, ctypes.c_int64, ctypes.c_int64, _I64P]),
    "fhx_cni_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p]),
    "fhx_cni_get_records": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _I64P]),
    # HiC-Pro matrix -> contact columns and per-bin totals (fithic/utils/HiCPro2FitHiC.py)
    "fhx_hp_load_bins": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _I32P, _I32P, ctypes.c_int64]),
    "fhx_hp_parse_matrix": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, _I64P, _I32P, _I64P, _I64P]),
    "fhx_hp_totals": (ctypes.c_int, [ctypes.c_void_p, _I64P]),
    "fhx_hp_fetch_rows": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I32P, _I32P, _I32P, _I32P]),
    # HiC-Pro allValidPairs -> contact counts (fithic/utils/validPairs2FitHiC-fixedSize.sh)
    "fhx_vp_bin_file": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, _I64P, _I32P, _I64P]),
    "fhx_vp_counts": (ctypes.c_int, [ctypes.c_void_p, _I64P, _I64P, _I64P, _I32P]),
    "fhx_vp_name": (ctypes.c_char_p, [ctypes.c_void_p, ctypes.c_int32]),
    "fhx_vp_fetch_cells": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I32P, _I32P, _I32P, _I32P]),
    "fhx_vp_write_contacts": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int32, _I32P, _I32P, _I32P, _I32P,
                                             _I32P, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    # the FDR subset of a significances file (fithic/utils/merge-filter.sh)
    "fhx_ms_select_file": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32,
                                          ctypes.c_int32, ctypes.c_int32, _I64P, _I32P, _I64P]),
    "fhx_ms_counts": (ctypes.c_int, [ctypes.c_void_p, _I64P, _I64P, _I64P]),
    "fhx_ms_copy_subset": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    # the UCSC interact track of the same selection (fithic/utils/visualize-UCSC.sh)
    "fhx_ms_track_file": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32,
                                         _I64P, _I32P, _I64P]),
    "fhx_ms_track_counts": (ctypes.c_int, [ctypes.c_void_p, _I64P, _I64P, _I64P, _I64P]),
    "fhx_ms_track_stage_seconds": (ctypes.c_int, [ctypes.c_void_p, _F64P]),
    "fhx_ms_copy_track": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "fhx_ms_score_text": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]),
    # the per-chromosome FDR subsets on the same handle
    "fhx_ms_split_file": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32,
                                         ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), _I64P]),
    "fhx_ms_split_counts": (ctypes.c_int, [ctypes.c_void_p, _I64P, ctypes.POINTER(ctypes.c_int32), _I64P, _I64P, ctypes.c_int32]),
    "fhx_ms_split_names": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "fhx_ms_split_stage_seconds": (ctypes.c_int, [ctypes.c_void_p, _F64P]),
    "fhx_ms_copy_split": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64]),
    # Juicer dump text -> contact counts (fithic/utils/createFitHiCContacts-hic_old.sh, createFitHiCContacts-hic.py)
    "fhx_jc_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fhx_jc_convert_file": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int32,
                                           ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _I64P, _I32P, _I64P]),
    "fhx_jc_counts": (ctypes.c_int, [ctypes.c_void_p, _I64P, _I64P, _I64P]),
    "fhx_jc_copy_text": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]),
    "fhx_jc_fetch_rows": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I32P, _I32P, _I32P, _I32P]),
    "fhx_dg_digest_file": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, _I32P, _I32P, ctypes.c_int32, _I32P, _I64P]),
    "fhx_dg_counts": (ctypes.c_int, [ctypes.c_void_p, _I64P, _I64P, _I64P, _I64P]),
    "fhx_dg_name": (ctypes.c_char_p, [ctypes.c_void_p, ctypes.c_int64]),
    "fhx_dg_contig_length": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64]),
    "fhx_dg_fetch_sites": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I32P]),
    "fhx_dg_write_fragments": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int64, _I64P, _I32P, _I32P, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]),
    "fhx_dg_write_bed": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int64, _I64P, _I32P, _I32P, ctypes.c_int64,
                                        ctypes.c_int32]),
    # HiC-Pro allValidPairs -> contact counts between the restriction fragments of a digest (no reference script)
    "fhx_fp_load_table": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, _I32P, ctypes.c_int32, _I64P, ctypes.c_int32, _I32P, ctypes.c_int64]),
    "fhx_fp_bin_file": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, _I64P, _I32P, _I64P]),
    "fhx_fp_counts": (ctypes.c_int, [ctypes.c_void_p, _I64P, _I64P, _I64P, _I64P, _I64P]),
    "fhx_fp_fetch_cells": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I32P, _I32P, _I32P, _I32P]),
    # contact rows in HBM summed onto N-fold coarser loci (no reference script)
    "fhx_cz_reset": (ctypes.c_int, [ctypes.c_void_p]),
    "fhx_cz_load_plan": (ctypes.c_int, [ctypes.c_void_p, _I64P, ctypes.c_int32, _I32P, _I32P, ctypes.c_int64, _I32P, _I32P, ctypes.c_int64]),
    "fhx_cz_coarsen_device": (ctypes.c_int, [ctypes.c_void_p, _P, _P, _P, _P, _P, ctypes.c_int64, _P, ctypes.c_int32, _I64P, _I32P, _I64P]),
    "fhx_cz_coarsen_host": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I32P, _I32P, _I32P, _I32P, ctypes.c_int64, ctypes.c_int32, _I64P, _I32P, _I64P]),
    "fhx_cz_counts": (ctypes.c_int, [ctypes.c_void_p, _I64P, _I64P, _I64P]),
    "fhx_cz_fetch_cells": (ctypes.c_int, [ctypes.c_void_p, _I32P, _I32P, _I32P, _I32P, _I32P]),
}
# the rows every handle beside the engine's repeats, per prefix
for _p in ("kr", "cni", "hp", "vp", "ms", "jc", "dg", "fp", "cz"):
    SYMBOLS.update({"fhx_%s_create" % _p: (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_P)]), "fhx_%s_destroy" % _p: (None, [_P]),
                    "fhx_%s_last_error" % _p: (ctypes.c_char_p, [_P])})
for _p in ("vp", "ms", "jc", "dg", "fp", "cz"):
    SYMBOLS["fhx_%s_stage_seconds" % _p] = (ctypes.c_int, [_P, _F64P])
for _p in ("hp", "vp", "jc", "fp", "cz"):
    SYMBOLS.update({"fhx_%s_device_ptr" % _p: (_P, [_P, ctypes.c_int32]), "fhx_%s_stream" % _p: (_P, [_P])})

# One object per translation unit (fithic_amd/csrc/_obj/, git-ignored), compiled in parallel, then one link: a change in K2 does
# not recompile K1, K3, the Knight-Ruiz path or the host stages.  Flags are the same for every unit - -ffp-contract=off matters
# for bit-exactness on the host (FITPACK, lgamma tables) as much as on the device (fhx_bdtrc.hpp).
SOURCES = ["fhx_device.hip", "fhx_k1.hip", "fhx_k2.hip", "fhx_k3.hip", "fhx_kr.hip", "fhx_cni.hip", "fhx_hicpro.hip", "fhx_validpairs.hip", "fhx_sigselect.hip", "fhx_sigresident.hip", "fhx_juicer.hip", "fhx_digest.hip", "fhx_fragpairs.hip", "fhx_coarsen.hip", "fhx_host.cpp", "fhx_io.cpp", "fhx_gunzip.cpp"]
COMPILE_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread"]
LINK_FLAGS = ["--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-lz", "-ldl"]
OBJ_DIR = os.path.join(CSRC, "_obj")


def build_commands():
    """[(compile command per unit)], link command - what build() runs (INTEGRATION.md quotes it)"""
    objs = [os.path.join(OBJ_DIR, os.path.splitext(f)[0] + ".o") for f in SOURCES]
    compiles = [["hipcc"] + COMPILE_FLAGS + ["-c", "-o", o, os.path.join(CSRC, f)] for f, o in zip(SOURCES, objs)]
    link = ["hipcc"] + objs + LINK_FLAGS + ["-o", LIB_PATH]
    return compiles, link


def build(force=False):
    """Compile the HIP kernels + host stages for gfx950 into the in-tree shared library."""
    from concurrent.futures import ThreadPoolExecutor
    shared = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc", ".def", ".h"))]
    header = os.path.join(os.path.dirname(_PKG), "include", "fithic_mi355x.h")
    if os.path.exists(header):                         # an installed package ships csrc/ but not include/
        shared.append(header)
    newest_shared = max(os.path.getmtime(p) for p in shared)
    compiles, link = build_commands()
    # a library newer than every source and header is current whatever csrc/_obj holds: the objects are git- and gpurun-ignored,
    # so a fresh checkout or the GPU box has the .so without them and must not recompile ten units to find that out
    newest_src = max([newest_shared] + [os.path.getmtime(os.path.join(CSRC, f)) for f in SOURCES])
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= newest_src:
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    stale = []
    for f, cmd in zip(SOURCES, compiles):
        obj, src = cmd[-2], cmd[-1]
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), newest_shared):
            stale.append(cmd)
    if stale:
        def run(cmd):
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError("%s failed:\n%s" % (" ".join(cmd[-4:]), r.stderr[-4000:]))
        with ThreadPoolExecutor(max_workers=min(len(stale), os.cpu_count() or 4)) as ex:
            list(ex.map(run, stale))
    objs = [cmd[-2] for cmd in compiles]
    if stale or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call(link)
    return LIB_PATH


_lib = None


def _share_torch_rccl():
    """One RCCL per process, for the same reason: PyTorch ships a librccl.so built against its own HIP runtime.  When torch is
    installed its copy is loaded (globally) before the first communicator is made and the library's run-time lookup finds it;
    without torch the system's librccl.so.1 is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return None
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "librccl.so")
    if not os.path.exists(cand):
        return None
    try:
        return ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except OSError:
        return None


UNIQUE_ID_BYTES = 128
STAGE_NAMES = ("k1_and_stats_exchange", "host_fit", "k2_launch", "cutoff_sort_splitters", "exchange_slice_bh_return")


def comm_unique_id():
    """ncclGetUniqueId as 128 bytes (rank 0 makes it, every rank passes it to Context.comm_init)."""
    _share_torch_rccl()
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    rc = lib().fhx_comm_unique_id(ctypes.cast(buf, _P), UNIQUE_ID_BYTES)
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_comm_unique_id: RCCL is not available")
    return bytes(buf.raw)


class FhxTransport(ctypes.Structure):
    """Caller-provided collectives on device pointers (include/fithic_mi355x.h: fhx_transport)."""
    ALL_REDUCE = ctypes.CFUNCTYPE(ctypes.c_int, _P, _P, ctypes.c_int64, ctypes.c_int)
    ALL_GATHER = ctypes.CFUNCTYPE(ctypes.c_int, _P, _P, _P, ctypes.c_int64)
    ALL_TO_ALL_V = ctypes.CFUNCTYPE(ctypes.c_int, _P, _P, _I64P, _I64P, _P, _I64P, _I64P, ctypes.c_int)
    _fields_ = [("user", _P), ("all_reduce_i64", ALL_REDUCE), ("all_gather", ALL_GATHER), ("all_to_all_v", ALL_TO_ALL_V)]


def lib():
    """The loaded library; raises (loudly) when it has not been built - there is no fallback."""
    global _lib
    if _lib is None:
        L = _loader.load()
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)        # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


class FhxError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("fhx error %d: %s" % (code, message))
        self.code = code


def device_blocks():
    """test hook (fhx_debug_device_blocks): (live device blocks, their bytes) of this process, over every handle"""
    blocks, nbytes = ctypes.c_int64(0), ctypes.c_int64(0)
    lib().fhx_debug_device_blocks(ctypes.byref(blocks), ctypes.byref(nbytes))
    return blocks.value, nbytes.value


def _ptr(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def _i32(a):
    a = np.ascontiguousarray(a)
    if a.dtype != np.int32:
        if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
            raise ValueError("value does not fit int32")
        a = a.astype(np.int32)
    return a


class Context:
    """One engine context = one GPU (device >= 0) or host-only (device = -1)."""

    def __init__(self, device=0):
        self._L = lib()
        h = _P()
        rc = self._L.fhx_create(int(device), ctypes.byref(h))
        if rc != FHX_OK:
            raise FhxError(rc, "fhx_create(device=%d) failed%s" % (device, " - no usable MI355X" if rc == FHX_ERR_NO_DEVICE else ""))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._L.fhx_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc):
        if rc != FHX_OK:
            raise FhxError(rc, (self._L.fhx_last_error(self._h) or b"").decode())

    # ---- setup ----
    def set_params(self, resolution, dist_low=0, dist_up=None, n_bins=100, mapp_thres=1, mode=MODE_INTRA_ONLY,
                   bias_low=0.5, bias_up=2.0, totals=TOTALS_REFERENCE):
        up = INT64_MAX if dist_up is None or dist_up == float("inf") else int(dist_up)
        p = FhxParams(int(resolution), int(dist_low), up, int(n_bins), int(mapp_thres), int(mode), int(totals), float(bias_low),
                      float(bias_up))
        self._check(self._L.fhx_set_params(self._h, ctypes.byref(p)))

    def load_fragments(self, chr_ids, mids, hits, chr_sort_rank):
        c, m, h, r = _i32(chr_ids), _i32(mids), _i32(hits), _i32(chr_sort_rank)
        self._check(self._L.fhx_load_fragments(self._h, _ptr(c, ctypes.c_int32), _ptr(m, ctypes.c_int32), _ptr(h, ctypes.c_int32),
                                               len(c), _ptr(r, ctypes.c_int32), len(r)))

    def load_bias(self, chr_ids, mids, bias):
        c, m = _i32(chr_ids), _i32(mids)
        b = np.ascontiguousarray(bias, np.float64)
        self._check(self._L.fhx_load_bias(self._h, _ptr(c, ctypes.c_int32), _ptr(m, ctypes.c_int32), _ptr(b, ctypes.c_double), len(c)))

    def load_pairs(self, chr1, mid1, chr2, mid2, count):
        a = [_i32(v) for v in (chr1, mid1, chr2, mid2, count)]
        self._check(self._L.fhx_load_pairs(self._h, *[_ptr(v, ctypes.c_int32) for v in a], len(a[0])))

    def load_pairs_device(self, ptrs, n, stream=None):
        self._check(self._L.fhx_load_pairs_device(self._h, *[_P(int(p)) for p in ptrs], int(n), _P(stream or 0)))

    def ingest_contacts_text(self, text, threads=0):
        """The inflated contacts file (host_inflate) parsed on the GPU -> (rows, names in order of first appearance).  Raises
        FhxError(FHX_ERR_UNSUPPORTED) for a file the device parser does not take: host_parse_text(text, ...) then."""
        n, k = ctypes.c_int64(0), ctypes.c_int32(0)
        self._check(self._L.fhx_ingest_contacts_text(self._h, text._h, int(threads), ctypes.byref(n), ctypes.byref(k)))
        return n.value, [self._L.fhx_ingest_contacts_name(self._h, i).decode() for i in range(k.value)]

    def ingest_contacts_file(self, path, threads=0):
        """The contacts FILE inflated and parsed on the GPU -> (rows, names).  Raises FhxError(FHX_ERR_UNSUPPORTED) with
        .refused = 1 (container / stream not taken: inflate on the host, the device parser may still take the text) or
        2 (text outside the device grammar: the host parser)."""
        n, k, why = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0)
        rc = self._L.fhx_ingest_contacts_file(self._h, os.fsencode(path), int(threads), ctypes.byref(n), ctypes.byref(k), ctypes.byref(why))
        if rc != FHX_OK:
            e = FhxError(rc, (self._L.fhx_last_error(self._h) or b"").decode())
            e.refused = why.value
            raise e
        return n.value, [self._L.fhx_ingest_contacts_name(self._h, i).decode() for i in range(k.value)]

    def debug_inflate_file(self, path, cap):
        out = np.empty(int(cap), np.uint8)
        n = ctypes.c_int64(0)
        self._check(self._L.fhx_debug_inflate_file(self._h, os.fsencode(path), out.ctypes.data_as(_P), int(cap), ctypes.byref(n)))
        return out[:n.value].tobytes()

    def ingest_contacts_commit(self, ids):
        """ids[i] = the run's chromosome id of name i: the parsed rows become the context's contact rows"""
        ids = np.ascontiguousarray(ids, np.int32)
        self._check(self._L.fhx_ingest_contacts_commit(self._h, _ptr(ids, ctypes.c_int32), len(ids)))

    def ingest_contacts_file_slice(self, path, part, n_parts, threads=0):
        """part `part` of `n_parts` of the contacts FILE inflated and parsed on the GPU -> (rows, names, ends with a newline); raises
        FhxError(FHX_ERR_UNSUPPORTED) with .refused as ingest_contacts_file"""
        n, k, why, nl = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        rc = self._L.fhx_ingest_contacts_file_slice(self._h, os.fsencode(path), int(threads), int(part), int(n_parts), ctypes.byref(n),
                                                    ctypes.byref(k), ctypes.byref(why), ctypes.byref(nl))
        if rc != FHX_OK:
            e = FhxError(rc, (self._L.fhx_last_error(self._h) or b"").decode())
            e.refused = why.value
            raise e
        return n.value, [self._L.fhx_ingest_contacts_name(self._h, i).decode() for i in range(k.value)], bool(nl.value)

    def ingest_contacts_text_slice(self, text, part, n_parts, threads=0):
        """the rows that start in part `part` of `n_parts` of an inflated text (HostText) parsed on the GPU -> (rows, names)"""
        n, k = ctypes.c_int64(0), ctypes.c_int32(0)
        self._check(self._L.fhx_ingest_contacts_text_slice(self._h, text._h, int(threads), int(part), int(n_parts), ctypes.byref(n), ctypes.byref(k)))
        return n.value, [self._L.fhx_ingest_contacts_name(self._h, i).decode() for i in range(k.value)]

    def ingest_contacts_text_own(self, text, skip, extra=b"", threads=0):
        """the rows whose first byte lies in `text` (a part of a stream: HostText of TextPart.resolve) from byte `skip` on, the last one
        completed by `extra`, parsed on the GPU -> (rows, names)"""
        n, k = ctypes.c_int64(0), ctypes.c_int32(0)
        self._keep_extra = bytes(extra)                       # (referenced until the call returns)
        self._check(self._L.fhx_ingest_contacts_text_own(self._h, text._h, int(threads), int(skip), self._keep_extra, len(self._keep_extra),
                                                         ctypes.byref(n), ctypes.byref(k)))
        return n.value, [self._L.fhx_ingest_contacts_name(self._h, i).decode() for i in range(k.value)]

    def set_global_rows_range(self, first):
        self._check(self._L.fhx_set_global_rows_range(self._h, int(first)))

    def ingest_contacts_chr_counts(self, n_names):
        """rows of the parsed text per name, by the chromosome of the first locus"""
        out = np.zeros(int(n_names), np.int64)
        self._check(self._L.fhx_ingest_contacts_chr_counts(self._h, _ptr(out, ctypes.c_int64), int(n_names)))
        return out

    def ingest_contacts_commit_shard(self, ids, mine):
        """as ingest_contacts_commit, keeping only the rows whose first chromosome has mine[i] set -> rows kept"""
        ids = np.ascontiguousarray(ids, np.int32)
        mine = np.ascontiguousarray(mine, np.uint8)
        n = ctypes.c_int64(0)
        self._check(self._L.fhx_ingest_contacts_commit_shard(self._h, _ptr(ids, ctypes.c_int32), _ptr(mine, ctypes.c_uint8), len(ids), ctypes.byref(n)))
        return n.value

    def shard_segments(self, cap=1 << 10):
        """[(local start, file position, length)] of the stretches of consecutive file positions this rank holds, or None (> cap)"""
        a, b, c = (np.zeros(int(cap), np.int64) for _ in range(3))
        n = ctypes.c_int64(0)
        self._check(self._L.fhx_shard_segments(self._h, _ptr(a, ctypes.c_int64), _ptr(b, ctypes.c_int64), _ptr(c, ctypes.c_int64), int(cap), ctypes.byref(n)))
        if n.value > cap:
            return None
        return [(int(a[i]), int(b[i]), int(c[i])) for i in range(n.value)]

    def write_significances_range(self, path, chr_names, row_begin, row_end, with_header):
        """rows [row_begin, row_end) of this context as gzip members (header member in front if asked) -> (rows written, bytes)"""
        arr = (ctypes.c_char_p * len(chr_names))(*[os.fsencode(n) for n in chr_names])
        rows, nbytes = ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self._L.fhx_write_significances_device_range(self._h, os.fsencode(path), arr, len(chr_names), int(row_begin), int(row_end),
                                                                 1 if with_header else 0, ctypes.byref(rows), ctypes.byref(nbytes)))
        return rows.value, nbytes.value

    def ingest_contacts_discard(self):
        self._L.fhx_ingest_contacts_discard(self._h)

    def fetch_pairs(self, rows=None, n=None):
        """(chr1, mid1, chr2, mid2, count) of the given loaded rows (all n of them when rows is None), rebuilt on the device"""
        if rows is not None:
            rows = np.ascontiguousarray(rows, np.int64)
            n = len(rows)
        out = [np.empty(int(n), np.int32) for _ in range(5)]
        self._check(self._L.fhx_fetch_pairs(self._h, _ptr(rows, ctypes.c_int64) if rows is not None else None, int(n),
                                            *[_ptr(v, ctypes.c_int32) for v in out]))
        return out

    # ---- one pass ----
    def pass_stats(self):
        st = FhxStats()
        self._check(self._L.fhx_pass_stats(self._h, ctypes.byref(st)))
        return st

    def set_global_stats(self, stats, hist_sumcc, hist_npairs):
        a = np.ascontiguousarray(hist_sumcc, np.int64)
        b = np.ascontiguousarray(hist_npairs, np.int64)
        self._check(self._L.fhx_set_global_stats(self._h, ctypes.byref(stats), _ptr(a, ctypes.c_int64), _ptr(b, ctypes.c_int64), len(a)))

    def set_dist_keys(self, keys):
        a = np.ascontiguousarray(keys, np.int64)
        self._check(self._L.fhx_set_dist_keys(self._h, _ptr(a, ctypes.c_int64), len(a)))

    def set_outlier_dists(self, dists):
        a = np.ascontiguousarray(dists, np.int64)
        self._check(self._L.fhx_set_outlier_dists(self._h, _ptr(a, ctypes.c_int64), len(a)))

    def set_outlier_dist_hist(self, hist):
        a = np.ascontiguousarray(hist, np.int64)
        self._check(self._L.fhx_set_outlier_dist_hist(self._h, _ptr(a, ctypes.c_int64), len(a)))

    def make_bins(self):
        n = ctypes.c_int32(0)
        self._check(self._L.fhx_make_bins(self._h, ctypes.byref(n)))
        return n.value

    def fit(self):
        info = FhxFitInfo()
        self._check(self._L.fhx_fit(self._h, ctypes.byref(info)))
        return info

    def run_pass(self):
        """pass_stats -> fit -> pvalues -> bh in one call (fhx_run_pass) -> (FhxStats, FhxFitInfo)"""
        st, info = FhxStats(), FhxFitInfo()
        self._check(self._L.fhx_run_pass(self._h, ctypes.byref(st), ctypes.byref(info)))
        return st, info

    def pvalues(self):
        self._check(self._L.fhx_pvalues(self._h))

    def bh(self, n_total_tests):
        self._check(self._L.fhx_bh(self._h, float(n_total_tests)))

    def sync(self):
        self._check(self._L.fhx_sync(self._h))

    def set_global_rows(self, rows):
        r = np.ascontiguousarray(rows, np.int64)
        self._check(self._L.fhx_set_global_rows(self._h, _ptr(r, ctypes.c_int64), len(r)))

    def get_skip_limit(self):
        return self._L.fhx_get_skip_limit(self._h)

    def set_skip_limit(self, limit):
        self._check(self._L.fhx_set_skip_limit(self._h, int(limit)))

    def next_pass(self):
        n = ctypes.c_int64(0)
        self._check(self._L.fhx_next_pass(self._h, ctypes.byref(n)))
        return n.value

    def reset_passes(self):
        self._check(self._L.fhx_reset_passes(self._h))

    # ---- sharded runs (one context per GPU / rank) ----
    def comm_init(self, unique_id, rank, world):
        """RCCL communicator on this context's GPU (blocks until every rank has called it)."""
        _share_torch_rccl()
        buf = ctypes.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES)
        self._check(self._L.fhx_comm_init(self._h, ctypes.cast(buf, _P), int(rank), int(world)))

    def comm_init_custom(self, transport, rank, world):
        self._transport = transport                      # keeps the callbacks alive
        self._check(self._L.fhx_comm_init_custom(self._h, ctypes.cast(ctypes.pointer(transport), _P), int(rank), int(world)))

    def comm_destroy(self):
        self._check(self._L.fhx_comm_destroy(self._h))

    def comm_info(self):
        r, w, v = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._L.fhx_comm_info(self._h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(v)))
        return r.value, w.value, v.value

    def run_pass_distributed(self):
        info = FhxFitInfo()
        self._check(self._L.fhx_run_pass_distributed(self._h, ctypes.byref(info)))
        return info

    def pass_stats_distributed(self):
        st = FhxStats()
        self._check(self._L.fhx_pass_stats_distributed(self._h, ctypes.byref(st)))
        return st

    def bh_distributed(self, n_total_tests):
        self._check(self._L.fhx_bh_distributed(self._h, float(n_total_tests)))

    def next_pass_distributed(self):
        n = ctypes.c_int64(0)
        self._check(self._L.fhx_next_pass_distributed(self._h, ctypes.byref(n)))
        return n.value

    def dist_stage_seconds(self):
        out = np.zeros(5, np.float64)
        self._check(self._L.fhx_dist_stage_seconds(self._h, _ptr(out, ctypes.c_double)))
        return dict(zip(STAGE_NAMES, out.tolist()))

    def dist_trace(self, clear=True):
        """[(step, kind, size)] of the collectives issued so far (FHX_DIST_TRACE=1 at comm_init time), in the vocabulary of
        csrc/fhx_dist_schedule.def"""
        n = ctypes.c_int64(0)
        self._check(self._L.fhx_dist_trace(self._h, None, 0, ctypes.byref(n), 0))
        buf = ctypes.create_string_buffer(max(int(n.value), 1))
        self._check(self._L.fhx_dist_trace(self._h, buf, int(n.value), ctypes.byref(n), 1 if clear else 0))
        rows = []
        for line in buf.raw[:n.value].decode().splitlines():
            step, kind, size = line.split()
            rows.append((step, kind, int(size)))
        return rows

    def copy(self, dst, src, nbytes, kind):
        """kind 0 = host to device, 1 = device to host, 2 = device to device (addresses as ints)."""
        self._check(self._L.fhx_copy(self._h, _P(int(dst)), _P(int(src)), int(nbytes), int(kind)))

    def stats(self):
        """fhx_stats of the last pass as the context holds them (global ones after a sharded pass)."""
        st = FhxStats()
        self._check(self._L.fhx_get_stats(self._h, ctypes.byref(st)))
        return st

    def fetch(self, n_rows, p=True, q=True, expcc=False, bias=False):
        out = {}
        bufs = []
        for key, want in (("p", p), ("q", q), ("expcc", expcc), ("b1", bias), ("b2", bias)):
            if want:
                out[key] = np.empty(n_rows, np.float64)
                bufs.append(_ptr(out[key], ctypes.c_double))
            else:
                bufs.append(None)
        self._check(self._L.fhx_fetch(self._h, *bufs))
        return out

    def fetch_outlier_rows(self):
        """row numbers of the outlier lines, ascending (int64), compacted on the device"""
        n = ctypes.c_int64(0)
        self._check(self._L.fhx_fetch_outlier_rows(self._h, None, 0, ctypes.byref(n)))
        rows = np.empty(n.value, np.int64)
        if n.value:
            self._check(self._L.fhx_fetch_outlier_rows(self._h, _ptr(rows, ctypes.c_int64), len(rows), ctypes.byref(n)))
        return rows

    def fetch_flags(self, n_rows, outlier=True, skip=False):
        o = np.empty(n_rows, np.uint8) if outlier else None
        k = np.empty(n_rows, np.uint8) if skip else None
        self._check(self._L.fhx_fetch_flags(self._h, _ptr(o, ctypes.c_uint8) if outlier else None,
                                            _ptr(k, ctypes.c_uint8) if skip else None))
        return o, k

    def write_significances_device(self, path, names, chr1=None, mid1=None, chr2=None, mid2=None, count=None):
        """The significances file formatted and deflated by the GPU from the resident p and q; returns (rows, bytes).  Without
        the five identity columns they are rebuilt on the device from the rows fhx_load_pairs stored (nothing is uploaded).
        Raises FhxError with code FHX_ERR_UNSUPPORTED when a row does not fit the device formatter (use host_write_significances)."""
        arr_names = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
        rows, nbytes = ctypes.c_int64(0), ctypes.c_int64(0)
        if chr1 is None:
            ptrs, n = [None] * 5, self.stats().n_rows
        else:
            i32 = [_i32(v) for v in (chr1, mid1, chr2, mid2, count)]
            ptrs, n = [_ptr(v, ctypes.c_int32) for v in i32], len(i32[0])
        self._check(self._L.fhx_write_significances_device(self._h, os.fsencode(path), arr_names, len(names), *ptrs, n, ctypes.byref(rows),
                                                           ctypes.byref(nbytes)))
        return rows.value, nbytes.value

    def significant_select(self, names, fdr_text, key_bound, zero_kept, strict=False):
        """fhx_significant_select: the FDR subset of the pass from its resident columns -> (n_emitted, n_kept, text, rows).  A q
        outside the grammar raises MsRefused (why, the line the row has in the file the pass writes); a kept row the device
        formatter does not cover raises FhxError with code FHX_ERR_UNSUPPORTED."""
        arr_names = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
        emitted, kept, nbytes = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        why, line = ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self._L.fhx_significant_select(self._h, arr_names, len(names), fdr_text, len(fdr_text), int(key_bound), 1 if zero_kept else 0,
                                            1 if strict else 0, ctypes.byref(emitted), ctypes.byref(kept), ctypes.byref(nbytes),
                                            ctypes.byref(why), ctypes.byref(line))
        if rc != FHX_OK and why.value:
            raise MsRefused(rc, (self._L.fhx_last_error(self._h) or b"").decode(), why.value, line.value)
        self._check(rc)
        return emitted.value, kept.value, self.significant_text(nbytes.value), self.significant_rows(kept.value)

    def significant_text(self, n_bytes):
        buf = np.empty(max(int(n_bytes), 1), np.uint8)
        self._check(self._L.fhx_significant_copy_text(self._h, buf.ctypes.data_as(_P), int(n_bytes)))
        return buf[:int(n_bytes)].tobytes()

    def significant_rows(self, n_kept):
        rows = np.empty(max(int(n_kept), 1), np.int64)
        self._check(self._L.fhx_significant_copy_rows(self._h, _ptr(rows, ctypes.c_int64), int(n_kept)))
        return rows[:int(n_kept)]

    def significant_track(self, names, fdr_text, key_bound, zero_kept):
        """fhx_significant_track: the interact track of the pass from its resident columns -> (n_emitted, n_kept, n_deferred, text).
        Refusals as for significant_select, plus MS_MIDPOINT and MS_NAME on any emitted row."""
        arr_names = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
        emitted, kept, deferred, nbytes = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        why, line = ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self._L.fhx_significant_track(self._h, arr_names, len(names), fdr_text, len(fdr_text), int(key_bound), 1 if zero_kept else 0,
                                           ctypes.byref(emitted), ctypes.byref(kept), ctypes.byref(deferred), ctypes.byref(nbytes),
                                           ctypes.byref(why), ctypes.byref(line))
        if rc != FHX_OK and why.value:
            raise MsRefused(rc, (self._L.fhx_last_error(self._h) or b"").decode(), why.value, line.value)
        self._check(rc)
        return emitted.value, kept.value, deferred.value, self.significant_track_text(nbytes.value)

    def significant_track_text(self, n_bytes):
        buf = np.empty(max(int(n_bytes), 1), np.uint8)
        self._check(self._L.fhx_significant_copy_track(self._h, buf.ctypes.data_as(_P), int(n_bytes)))
        return buf[:int(n_bytes)].tobytes()

    def significant_split(self, names, fdr_text, key_bound, zero_kept):
        """fhx_significant_split: the per-chromosome FDR subsets of the pass from its resident columns ->
        (n_emitted, [(name, kept rows, text)] in bytewise order of the names).  Refusals as for significant_select, plus the name
        rules on any emitted row and MS_NAMES."""
        arr_names = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
        emitted, listed = ctypes.c_int64(0), ctypes.c_int32(0)
        why, line = ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self._L.fhx_significant_split(self._h, arr_names, len(names), fdr_text, len(fdr_text), int(key_bound), 1 if zero_kept else 0,
                                           ctypes.byref(emitted), ctypes.byref(listed), ctypes.byref(why), ctypes.byref(line))
        if rc != FHX_OK and why.value:
            raise MsRefused(rc, (self._L.fhx_last_error(self._h) or b"").decode(), why.value, line.value)
        self._check(rc)
        return emitted.value, self.significant_split_parts(listed.value)

    def significant_split_parts(self, n_listed):
        n = int(n_listed)
        kept, nbytes = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        self._check(self._L.fhx_significant_split_counts(self._h, _ptr(kept, ctypes.c_int64), _ptr(nbytes, ctypes.c_int64), n))
        raw = np.zeros(max(n, 1) * MS_SPLIT_NAME_BYTES, np.uint8)
        self._check(self._L.fhx_significant_split_names(self._h, raw.ctypes.data_as(_P), n))
        raw = raw.tobytes()
        parts = []
        for k in range(n):
            buf = np.empty(max(int(nbytes[k]), 1), np.uint8)
            self._check(self._L.fhx_significant_copy_split(self._h, k, buf.ctypes.data_as(_P), int(nbytes[k])))
            parts.append((raw[k * MS_SPLIT_NAME_BYTES:(k + 1) * MS_SPLIT_NAME_BYTES].rstrip(b"\0"), int(kept[k]), buf[:int(nbytes[k])].tobytes()))
        return parts

    def get_array(self, which):
        n = ctypes.c_int64(0)
        self._check(self._L.fhx_get_array(self._h, which, None, 0, ctypes.byref(n)))
        a = np.empty(n.value, _ARRAY_DTYPE.get(which, np.int64))
        self._check(self._L.fhx_get_array(self._h, which, a.ctypes.data_as(_P), n.value, ctypes.byref(n)))
        return a

    def kernel_seconds(self):
        k = [ctypes.c_double(0) for _ in range(3)]
        self._check(self._L.fhx_kernel_seconds(self._h, *[ctypes.byref(v) for v in k]))
        return tuple(v.value for v in k)

    def kernel_seconds_total(self, reset=False):
        """(seconds[4], passes[4]) of K1, K2, K3 and the heavy K2 launch summed since the last reset (waits for the stream once)."""
        s = (ctypes.c_double * 4)()
        n = (ctypes.c_int64 * 4)()
        self._check(self._L.fhx_kernel_seconds_total(self._h, s, n, 1 if reset else 0))
        return list(s), list(n)

    def bh_sort_stats(self):
        """how the last BH call sorted its survivors (include/fithic_mi355x.h: fhx_bh_sort_stats)"""
        n = (ctypes.c_int64 * 8)()
        self._check(self._L.fhx_bh_sort_stats(self._h, n))
        return dict(zip(("passes", "low_bit", "beyond_lists", "inversions", "runs_by_thread", "long_run_inversions", "segments", "segment_keys"),
                        [int(v) for v in n]))

    def k3_pass_info(self):
        """which path the last bh() took through K3: the eight slots of fhx_k3_pass_info and, as a ninth, fhx_k3_compact_variant
        (include/fithic_mi355x.h)"""
        n = (ctypes.c_int64 * 8)()
        self._check(self._L.fhx_k3_pass_info(self._h, n))
        v = ctypes.c_int32(0)
        self._check(self._L.fhx_k3_compact_variant(self._h, ctypes.byref(v)))       # [8]: 0 / 1 / 2, the sparse compaction
        return [int(x) for x in n] + [v.value]

    def debug_k3_tiles_per_group(self, per):
        """test hook (fhx_debug_k3_tiles_per_group): 1..4 tiles per workgroup in the scattered compaction, 0: the library's choice"""
        self._check(self._L.fhx_debug_k3_tiles_per_group(self._h, int(per)))

    def debug_k1_wide(self, on):
        """test hook (fhx_debug_k1_wide): True makes pass_stats read the three int32 columns instead of the key column"""
        self._check(self._L.fhx_debug_k1_wide(self._h, 1 if on else 0))

    def kernel_events_dropped(self):
        """passes of K1, K2, K3, heavy launch whose events were overwritten unread since the last reset (0 = the sums are complete)"""
        n = (ctypes.c_int64 * 4)()
        self._check(self._L.fhx_kernel_events_dropped(self._h, n))
        return list(n)

    def k2_heavy_launch(self):
        sec, rows = ctypes.c_double(0), ctypes.c_int64(0)
        self._check(self._L.fhx_k2_heavy_launch(self._h, ctypes.byref(sec), ctypes.byref(rows)))
        return sec.value, rows.value

    def k2_heavy_clock(self):
        """GHz the last heavy launch ran at (0.0: it held no task)"""
        ghz = ctypes.c_double(0)
        self._check(self._L.fhx_k2_heavy_clock(self._h, ctypes.byref(ghz)))
        return ghz.value

    def k2_class_rows(self):
        """rows the last pvalues() queued per class: power series, incbcf, incbd, swapped incbcf (300 iterations), closed form >= 0.01"""
        out = (ctypes.c_int64 * 5)()
        self._check(self._L.fhx_k2_class_rows(self._h, out))
        return dict(zip(("pseries", "cf_bcf", "cf_bd", "cf_swapped", "closed_pow"), [int(v) for v in out]))

    def device_ptr(self, which):
        return self._L.fhx_device_ptr(self._h, which)

    def bdtrc_array(self, n_total, count, prior):
        c = _i32(count)
        pr = np.ascontiguousarray(prior, np.float64)
        out = np.empty(len(c), np.float64)
        self._check(self._L.fhx_bdtrc_array(self._h, float(n_total), _ptr(c, ctypes.c_int32), _ptr(pr, ctypes.c_double), len(c),
                                            _ptr(out, ctypes.c_double)))
        return out

    def debug_classify(self, n_total, count, prior, thresholds=False):
        """(class by the threshold table, class by incbet's predicates[, thresholds n x 5]) for integer counts and priors"""
        c = _i32(count)
        pr = np.ascontiguousarray(prior, np.float64)
        t, a = np.empty(len(c), np.int32), np.empty(len(c), np.int32)
        thr = np.empty((len(c), 5), np.float64) if thresholds else None
        self._check(self._L.fhx_debug_classify(self._h, float(n_total), _ptr(c, ctypes.c_int32), _ptr(pr, ctypes.c_double), len(c),
                                               _ptr(t, ctypes.c_int32), _ptr(a, ctypes.c_int32),
                                               _ptr(thr, ctypes.c_double) if thresholds else None))
        return (t, a, thr) if thresholds else (t, a)

    def debug_k2_rows(self, n_intra, n_inter, count, prior, is_inter, nonfixed=False):
        """The K2 launches of a pass on chosen rows (fhx_debug_k2_rows; the context's contact rows are discarded): returns
        (p, rows per class as k2_class_rows, rows the heavy kernel handed back, the fused key histogram of 4096 bins)."""
        c = _i32(count)
        pr = np.ascontiguousarray(prior, np.float64)
        it = np.ascontiguousarray(is_inter, np.uint8)
        if not (len(c) == len(pr) == len(it)):
            raise ValueError("count, prior and is_inter must have one entry per row")
        p = np.empty(len(c), np.float64)
        cls = (ctypes.c_int64 * 5)()
        redo = ctypes.c_int64(0)
        hist = np.zeros(4096, np.int64)
        self._check(self._L.fhx_debug_k2_rows(self._h, float(n_intra), float(n_inter), _ptr(c, ctypes.c_int32), _ptr(pr, ctypes.c_double),
                                              _ptr(it, ctypes.c_uint8), len(c), int(bool(nonfixed)), _ptr(p, ctypes.c_double), cls,
                                              ctypes.byref(redo), _ptr(hist, ctypes.c_int64), len(hist)))
        by_class = dict(zip(("pseries", "cf_bcf", "cf_bd", "cf_swapped", "closed_pow"), [int(v) for v in cls]))
        return p, by_class, redo.value, hist

    def debug_contfrac(self, kind, lazy, a, b, x):
        a, b, x = (np.ascontiguousarray(v, np.float64) for v in (a, b, x))
        out = np.empty(len(a), np.float64)
        self._check(self._L.fhx_debug_contfrac(self._h, int(kind), int(lazy), _ptr(a, ctypes.c_double), _ptr(b, ctypes.c_double),
                                               _ptr(x, ctypes.c_double), len(a), _ptr(out, ctypes.c_double)))
        return out

    def debug_format(self, values, kind):
        """The device writer's "%e" (kind 0) / "%f" (kind 1) of every value: list of bytes, None where the device does not cover it."""
        v = np.ascontiguousarray(values, np.float64)
        text = ctypes.create_string_buffer(len(v) * 32)
        ln = np.empty(len(v), np.int32)
        self._check(self._L.fhx_debug_format(self._h, _ptr(v, ctypes.c_double), len(v), int(kind), text, _ptr(ln, ctypes.c_int32)))
        raw = text.raw
        return [raw[32 * i:32 * i + ln[i]] if ln[i] > 0 else None for i in range(len(v))]

    def debug_lean_div(self, n, d):
        n, d = (np.ascontiguousarray(v, np.float64) for v in (n, d))
        out = np.empty(len(n), np.float64)
        self._check(self._L.fhx_debug_lean_div(self._h, _ptr(n, ctypes.c_double), _ptr(d, ctypes.c_double), len(n), _ptr(out, ctypes.c_double)))
        return out

    def debug_table_div(self, kind, num):
        """num[i] / j (j + 1) (kind 0) or num[i] / j (kind 1) by the class kernels' tabulated reciprocals: (J - 1, len(num)) for j = 1 .. J - 1"""
        num = np.ascontiguousarray(num, np.float64)
        length = ctypes.c_int32(0)
        dummy = np.empty(1, np.float64)
        self._check(self._L.fhx_debug_table_div(self._h, int(kind), _ptr(dummy, ctypes.c_double), 0, _ptr(dummy, ctypes.c_double), ctypes.byref(length)))
        out = np.empty((length.value - 1, len(num)), np.float64)
        if len(num):
            self._check(self._L.fhx_debug_table_div(self._h, int(kind), _ptr(num, ctypes.c_double), len(num), _ptr(out, ctypes.c_double),
                                                    ctypes.byref(length)))
        return out

    def bh_array(self, p, n_total_tests):
        p = np.ascontiguousarray(p, np.float64)
        q = np.empty(len(p), np.float64)
        self._check(self._L.fhx_bh_array(self._h, _ptr(p, ctypes.c_double), len(p), float(n_total_tests), _ptr(q, ctypes.c_double)))
        return q

    def bh_top_hist(self):
        h = np.zeros(8192, np.int64)
        self._check(self._L.fhx_bh_top_hist(self._h, _ptr(h, ctypes.c_int64), len(h)))
        return h

    def bh_set_cutoff(self, global_hist, n_total_tests):
        h = np.ascontiguousarray(global_hist, np.int64)
        self._check(self._L.fhx_bh_set_cutoff(self._h, _ptr(h, ctypes.c_int64), len(h), float(n_total_tests)))

    def bh_top_hist_device(self):
        """Histogram left on the device; returns its address (8192 x uint64) for an in-place all-reduce."""
        self._check(self._L.fhx_bh_top_hist_device(self._h))
        return self.device_ptr(4)

    def bh_set_cutoff_device(self, n_total_tests):
        self._check(self._L.fhx_bh_set_cutoff_device(self._h, float(n_total_tests)))

    def bh_local_sort(self):
        self._check(self._L.fhx_bh_local_sort(self._h))

    def n_sorted(self):
        return self._L.fhx_n_sorted(self._h)

    def bh_apply_sorted(self, d_keys, n, rank0, carry_in, n_total_tests, d_q_sorted):
        mx = ctypes.c_double(0)
        self._check(self._L.fhx_bh_apply_sorted(self._h, _P(int(d_keys) if d_keys else 0), int(n), int(rank0), float(carry_in),
                                                float(n_total_tests), _P(int(d_q_sorted) if d_q_sorted else 0), ctypes.byref(mx)))
        return mx.value


    def sort_u64(self, d_keys_in, n, d_keys_out, d_perm_out):
        self._check(self._L.fhx_sort_u64(self._h, _P(int(d_keys_in)), int(n), _P(int(d_keys_out)), _P(int(d_perm_out))))

    def bh_scatter(self, d_q_sorted_local):
        self._check(self._L.fhx_bh_scatter(self._h, _P(int(d_q_sorted_local)) if d_q_sorted_local else None))

    def memcpy_d2d(self, dst, src, nbytes):
        self._check(self._L.fhx_memcpy_d2d(self._h, _P(int(dst)), _P(int(src)), int(nbytes)))


# ---- native text I/O (no context needed) ---------------------------------------------------------------
class HostText:
    """An inflated file (fhx_host_inflate): input of Ctx.ingest_contacts_text and of host_parse_text."""

    def __init__(self, path, threads=0):
        L = lib()
        self._L, self._h = L, _P()
        rc = L.fhx_host_inflate(os.fsencode(path), int(threads), ctypes.byref(self._h))
        if rc != FHX_OK:
            msg = (L.fhx_text_error(self._h) or b"").decode() if self._h else "fhx_host_inflate"
            self.close()
            raise FhxError(rc, msg)

    def __len__(self):
        return int(self._L.fhx_text_bytes(self._h))

    def bytes(self):
        """the inflated text (tests)"""
        out = np.empty(len(self), np.uint8)
        rc = self._L.fhx_text_copy(self._h, out.ctypes.data_as(_P), len(out))
        if rc != FHX_OK:
            raise FhxError(rc, "fhx_text_copy")
        return out.tobytes()

    def first_row_end(self):
        """(length of the first row with its newline, the row) - (-1, b"") when the text holds no newline"""
        n = int(self._L.fhx_text_first_row_end(self._h, None, 0))
        if n < 0:
            return -1, b""
        buf = ctypes.create_string_buffer(n)
        self._L.fhx_text_first_row_end(self._h, buf, n)
        return n, buf.raw

    def ends_with_newline(self):
        return bool(self._L.fhx_text_ends_with_newline(self._h))

    def part_bounds(self, part, n_parts):
        """bytes [lo, hi) of the text that part `part` of `n_parts` takes (Ctx.ingest_contacts_text_slice): the rows that start in its
        N-th of the bytes"""
        lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = self._L.fhx_text_part_bounds(self._h, int(part), int(n_parts), ctypes.byref(lo), ctypes.byref(hi))
        if rc != FHX_OK:
            raise FhxError(rc, "fhx_text_part_bounds")
        return lo.value, hi.value

    def close(self):
        if self._h:
            self._L.fhx_text_free(self._h)
            self._h = _P()

    __del__ = close


class TextPart:
    """Part `part` of `n_parts` of one plain gzip stream, decoded without the 32 KB of text before it (fhx_host_inflate_part).
    tail(): its last 32768 symbols in terms of that window; resolve(window) -> (HostText of the part, CRC-32)."""

    WINDOW = 32768

    def __init__(self, path, part, n_parts, threads=0):
        L = lib()
        self._L, self._h = L, _P()
        rc = L.fhx_host_inflate_part(os.fsencode(path), int(threads), int(part), int(n_parts), ctypes.byref(self._h))
        if rc != FHX_OK:
            msg = (L.fhx_text_part_error(self._h) or b"").decode() if self._h else "fhx_host_inflate_part"
            self.close()
            raise FhxError(rc, msg)

    def __len__(self):
        return int(self._L.fhx_text_part_bytes(self._h))

    def is_last(self):
        return bool(self._L.fhx_text_part_is_last(self._h))

    def tail(self):
        out = np.empty(self.WINDOW, np.uint16)
        rc = self._L.fhx_text_part_tail(self._h, out.ctypes.data_as(_P), len(out))
        if rc != FHX_OK:
            raise FhxError(rc, "fhx_text_part_tail")
        return out

    def resolve(self, window):
        w = np.ascontiguousarray(window, np.uint8)
        h, crc = _P(), ctypes.c_uint32(0)
        rc = self._L.fhx_text_part_resolve(self._h, w.ctypes.data_as(_P), len(w), ctypes.byref(h), ctypes.byref(crc))
        if rc != FHX_OK:
            raise FhxError(rc, "fhx_text_part_resolve")
        text = HostText.__new__(HostText)
        text._L, text._h = self._L, h
        return text, int(crc.value)

    def close(self):
        if self._h:
            self._L.fhx_text_part_free(self._h)
            self._h = _P()

    __del__ = close


def chain_windows(tails):
    """tails[r] = TextPart.tail() of part r -> the 32 KB of text before every part (part 0: zeros; nothing refers to them)"""
    windows = [np.zeros(TextPart.WINDOW, np.uint8)]
    for t in tails[:-1]:
        t = np.asarray(t, np.uint16)
        ref = t >= 256
        w = t.astype(np.uint8)
        w[ref] = windows[-1][t[ref] - 256]
        windows.append(w)
    return windows


def crc32_combine(crc_a, crc_b, len_b):
    return int(lib().fhx_crc32_combine(int(crc_a), int(crc_b), int(len_b)))


def _table_out(L, rc, h, kind, name_ids, want_float, what):
    try:
        if rc != FHX_OK:
            raise FhxError(rc, (L.fhx_table_error(h) or b"").decode() if h else what)
        n = L.fhx_table_rows(h)
        names = [L.fhx_table_name(h, i).decode() for i in range(L.fhx_table_n_names(h))]
        if name_ids is not None and names:
            ids = np.ascontiguousarray(name_ids(names), np.int32)
            rc = L.fhx_table_map_names(h, _ptr(ids, ctypes.c_int32), len(ids))
            if rc != FHX_OK:
                raise FhxError(rc, "fhx_table_map_names")
        cols = {}
        want = {0: (0, 1, 2, 3, 4), 1: (0, 1, 4), 2: (0, 1)}[kind]
        for c in want:
            a = np.empty(n, np.int32)
            L.fhx_table_copy(h, c, a.ctypes.data_as(_P))
            cols[c] = a
        dv = None
        if kind == 2 or (kind == 0 and want_float):
            dv = np.empty(n, np.float64)
            L.fhx_table_copy(h, 5, dv.ctypes.data_as(_P))
        return names, cols, dv
    finally:
        if h:
            L.fhx_table_free(h)


def host_read_table(path, kind, threads=0, name_ids=None, want_float=True):
    """-> (names, int32 columns dict, float64 column or None).  kind: 0 contacts, 1 fragments, 2 bias.
    name_ids(names) -> the caller's ids of the file's names: the chromosome columns then come out in that id space (mapped inside
    the parallel copy, not per row in numpy).  want_float=False skips the 8 B/row float column of a contacts file."""
    L = lib()
    h = _P()
    flags = 0x100 if (kind == 0 and not want_float) else 0          # FHX_TABLE_NO_FLOAT
    rc = L.fhx_host_read_table(os.fsencode(path), int(kind) | flags, int(threads), ctypes.byref(h))
    return _table_out(L, rc, h, kind, name_ids, want_float, "fhx_host_read_table")


def host_parse_text(text, kind, threads=0, name_ids=None, want_float=True):
    """host_read_table's parse stage on an already inflated file (a HostText)"""
    L = lib()
    h = _P()
    flags = 0x100 if (kind == 0 and not want_float) else 0
    rc = L.fhx_host_parse_text(text._h, int(kind) | flags, int(threads), ctypes.byref(h))
    return _table_out(L, rc, h, kind, name_ids, want_float, "fhx_host_parse_text")


def host_write_contacts(path, names, chr1, mid1, chr2, mid2, count, gzip_level=1, threads=0):
    """chr1 mid1 chr2 mid2 count as the reference reads it, size-tagged gzip members written on all cores (tooling)."""
    arr_names = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
    i32 = [_i32(v) for v in (chr1, mid1, chr2, mid2, count)]
    rc = lib().fhx_host_write_contacts(os.fsencode(path), arr_names, len(names), *[_ptr(v, ctypes.c_int32) for v in i32], len(i32[0]),
                                       int(gzip_level), int(threads))
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_host_write_contacts(%s)" % path)


def host_write_significances(path, names, chr1, mid1, chr2, mid2, count, p, q, b1, b2, expcc, mode, dist_low, dist_up,
                             gzip_level=None, threads=0):
    """gzip level: 1 unless FHX_GZIP_LEVEL says otherwise - the decompressed bytes are what the reference writes; its own
    files are level 9 (Python's gzip default).  Measured on the output text (one core): level 1 compresses 0.38 M rows/s into
    39 B/row, level 3 0.28 M rows/s into 36 B/row, level 6 0.14 M rows/s into 33 B/row; formatting alone runs at 1.1 M rows/s."""
    if gzip_level is None:
        gzip_level = int(os.environ.get("FHX_GZIP_LEVEL", "1"))
    arr_names = (ctypes.c_char_p * len(names))(*[n.encode() for n in names])
    i32 = [_i32(v) for v in (chr1, mid1, chr2, mid2, count)]
    f64 = [np.ascontiguousarray(v, np.float64) for v in (p, q, b1, b2, expcc)]
    up = INT64_MAX if dist_up is None or dist_up == float("inf") else int(dist_up)
    written = ctypes.c_int64(0)
    rc = lib().fhx_host_write_significances(os.fsencode(path), arr_names, len(names), *[_ptr(v, ctypes.c_int32) for v in i32],
                                            *[_ptr(v, ctypes.c_double) for v in f64], len(i32[0]), int(mode), int(dist_low), up,
                                            int(gzip_level), int(threads), ctypes.byref(written))
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_host_write_significances(%s)" % path)
    return written.value


# ---- host numerics (no context needed) -------------------------------------------------------------
def host_spline_fit(x, y, s):
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    m = len(x)
    t = np.empty(m + 8, np.float64)
    c = np.empty(m + 8, np.float64)
    n = ctypes.c_int32(0)
    fp = ctypes.c_double(0)
    ier = ctypes.c_int32(0)
    rs = ctypes.c_int32(0)
    rc = lib().fhx_host_spline_fit(_ptr(x, ctypes.c_double), _ptr(y, ctypes.c_double), m, float(s), _ptr(t, ctypes.c_double),
                                   _ptr(c, ctypes.c_double), ctypes.byref(n), ctypes.byref(fp), ctypes.byref(ier), ctypes.byref(rs))
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_host_spline_fit")
    return t[:n.value].copy(), c[:n.value - 4].copy(), fp.value, ier.value, bool(rs.value)


def host_spline_eval(t, c, xs):
    t = np.ascontiguousarray(t, np.float64)
    c = np.ascontiguousarray(c, np.float64)
    xs = np.ascontiguousarray(xs, np.float64)
    out = np.empty(len(xs), np.float64)
    rc = lib().fhx_host_spline_eval(_ptr(t, ctypes.c_double), _ptr(c, ctypes.c_double), len(t), _ptr(xs, ctypes.c_double), len(xs),
                                    _ptr(out, ctypes.c_double))
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_host_spline_eval")
    return out


def host_pava_decreasing(y):
    y = np.ascontiguousarray(y, np.float64)
    out = np.empty(len(y), np.float64)
    rc = lib().fhx_host_pava_decreasing(_ptr(y, ctypes.c_double), len(y), _ptr(out, ctypes.c_double))
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_host_pava_decreasing")
    return out


def host_lbeta_table(n_total, max_count):
    lb = np.empty(max_count + 1, np.float64)
    ib = np.empty(max_count + 1, np.float64)
    rc = lib().fhx_host_lbeta_table(float(n_total), int(max_count), _ptr(lb, ctypes.c_double), _ptr(ib, ctypes.c_double))
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_host_lbeta_table")
    return lb, ib


# ---- the contexts beside Context: one native handle each, made by fhx_<prefix>_create -------------------------------------
class _Handle:
    """A native context on one GPU: fhx_<PREFIX>_create / _destroy / _last_error.  Raises without the built library or a GPU."""
    PREFIX = None
    REFUSED = None                   # the text paths: what _chk raises when the call named a reason
    STAGE_NAMES = None               # stage_seconds(): the slots of fhx_<PREFIX>_stage_seconds
    COUNTS = None                    # counts(): ((key, ctype), ...), the outputs of fhx_<PREFIX>_counts

    def __init__(self, device=0):
        self.L = lib()
        self.h = ctypes.c_void_p()
        rc = self._fn("create")(int(device), ctypes.byref(self.h))
        if rc != FHX_OK:
            self.h = None
            raise FhxError(rc, "fhx_%s_create(device=%d) failed: no usable MI355X / HIP runtime" % (self.PREFIX, device))

    def _fn(self, name):
        return getattr(self.L, "fhx_%s_%s" % (self.PREFIX, name))

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    __del__ = close

    def _last_error(self):
        return (self._fn("last_error")(self.h) or b"").decode()

    def _chk(self, rc, why=0, *where):
        """why, where: the reason (not 0: the file was refused) and the line (and index) a text path's call reported"""
        if rc != FHX_OK and why:
            raise self.REFUSED(rc, self._last_error(), why, *where)
        if rc != FHX_OK:
            raise FhxError(rc, self._last_error())

    def _stage_seconds(self, names, fn="stage_seconds"):
        out = np.zeros(len(names), np.float64)
        self._chk(self._fn(fn)(self.h, _ptr(out, ctypes.c_double)))
        return dict(zip(names, out.tolist()))

    def stage_seconds(self):
        return self._stage_seconds(self.STAGE_NAMES)

    def _counts(self, spec, fn="counts"):
        v = [t(0) for _, t in spec]
        self._chk(self._fn(fn)(self.h, *[ctypes.byref(x) for x in v]))
        return {k: x.value for (k, _), x in zip(spec, v)}

    def counts(self):
        return self._counts(self.COUNTS)

    # the handles that hold five resident int32 columns: fhx_<PREFIX>_fetch_<what>, _device_ptr and _stream
    def _fetch_columns(self, what, n):
        cols = [np.zeros(n, np.int32) for _ in range(5)]
        self._chk(self._fn("fetch_" + what)(self.h, *[_ptr(v, ctypes.c_int32) for v in cols]))
        return cols

    def device_ptrs(self):
        return [self._fn("device_ptr")(self.h, k) or 0 for k in range(5)]

    def stream(self):
        return self._fn("stream")(self.h) or 0


class _LineRefused(FhxError):
    """a text path refused its file: why = one of the path's reasons, line = the smallest offending 1-based line"""

    def __init__(self, code, message, why, line):
        super().__init__(code, message)
        self.why, self.line = int(why), int(line)


def _i64s(*keys):
    return tuple((k, ctypes.c_int64) for k in keys)


# ---- Knight-Ruiz (fhx_kr_*) ------------------------------------------------------------------------------------------
class KrInfo(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("nnz", ctypes.c_int64), ("outer_iterations", ctypes.c_int32),
                ("inner_iterations", ctypes.c_int32), ("matvecs", ctypes.c_int64), ("boundary_steps", ctypes.c_int64),
                ("residual", ctypes.c_double), ("spmv_seconds", ctypes.c_double), ("spmv_timed", ctypes.c_int64),
                ("value_bytes", ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class KrContext(_Handle):
    """One Knight-Ruiz balancing context on one GPU (fhx_kr_*).  Raises without the built library or without a GPU."""
    PREFIX = "kr"

    def load_loci(self, chr_ids, mids):
        c, m = _i32(chr_ids), _i32(mids)
        self._chk(self.L.fhx_kr_load_loci(self.h, _ptr(c, ctypes.c_int32), _ptr(m, ctypes.c_int32), len(c)))

    def load_pairs(self, chr1, mid1, chr2, mid2, value):
        a = [_i32(v) for v in (chr1, mid1, chr2, mid2)]
        z = np.ascontiguousarray(value, np.float64)
        bad = ctypes.c_int64(-1)
        rc = self.L.fhx_kr_load_pairs(self.h, *[_ptr(v, ctypes.c_int32) for v in a], _ptr(z, ctypes.c_double), len(z), ctypes.byref(bad))
        if rc == FHX_ERR_REFERENCE_EXIT and bad.value >= 0:
            raise KeyError(bad.value)
        self._chk(rc)

    def load_pairs_resident(self, engine_ctx):
        """The same matrix from the contact rows `engine_ctx` (a Context on this GPU) holds, loaded with the chromosome ids of
        load_loci: KeyError(row) as load_pairs; FhxError(FHX_ERR_UNSUPPORTED) when a count of its text was not an integer as
        written - load_pairs with the file's float counts then."""
        bad = ctypes.c_int64(-1)
        rc = self.L.fhx_kr_load_pairs_resident(self.h, engine_ctx._h, ctypes.byref(bad))
        if rc == FHX_ERR_REFERENCE_EXIT and bad.value >= 0:
            raise KeyError(bad.value)
        self._chk(rc)

    def shape(self):
        v = [ctypes.c_int64() for _ in range(4)]
        self._chk(self.L.fhx_kr_shape(self.h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def get_csr(self, which=0):
        n_full, nnz_full, n_red, nnz_red = self.shape()
        n, nnz = (n_red, nnz_red) if which else (n_full, nnz_full)
        indptr, col, val = np.zeros(n + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, np.float64)
        self._chk(self.L.fhx_kr_get_csr(self.h, which, _ptr(indptr, ctypes.c_int64), _ptr(col, ctypes.c_int32), _ptr(val, ctypes.c_double)))
        return indptr, col, val

    def row_sums(self):
        out = np.zeros(self.shape()[0], np.float64)
        self._chk(self.L.fhx_kr_row_sums(self.h, _ptr(out, ctypes.c_double)))
        return out

    def remove_sparse(self, perc):
        nrem, val, rem = ctypes.c_int64(), ctypes.c_double(), ctypes.c_int64()
        rc = self.L.fhx_kr_remove_sparse(self.h, float(perc), ctypes.byref(nrem), ctypes.byref(val), ctypes.byref(rem))
        if rc == FHX_ERR_REFERENCE_EXIT:
            raise IndexError(self._last_error())
        self._chk(rc)
        idx = np.zeros(nrem.value, np.int64)
        self._chk(self.L.fhx_kr_get_removed(self.h, _ptr(idx, ctypes.c_int64), len(idx), None))
        return idx, val.value, rem.value

    def balance(self, tol=1e-6):
        info = KrInfo()
        rc = self.L.fhx_kr_balance(self.h, float(tol), ctypes.byref(info))
        if rc == FHX_ERR_REFERENCE_EXIT:
            raise ValueError(self._last_error())
        self._chk(rc)
        x = np.zeros(info.n, np.float64)
        if info.n:
            self._chk(self.L.fhx_kr_get_x(self.h, _ptr(x, ctypes.c_double)))
        return x, info

    def bias(self):
        out = np.zeros(self.shape()[0], np.float64)
        self._chk(self.L.fhx_kr_bias(self.h, _ptr(out, ctypes.c_double)))
        return out

    def spmv(self, x, which=0, repeats=1):
        x = np.ascontiguousarray(x, np.float64)
        y = np.zeros_like(x)
        sec = ctypes.c_double()
        self._chk(self.L.fhx_kr_spmv(self.h, which, _ptr(x, ctypes.c_double), _ptr(y, ctypes.c_double), int(repeats), ctypes.byref(sec)))
        return y, sec.value

    def dot(self, a, b=None):
        a = np.ascontiguousarray(a, np.float64)
        out = ctypes.c_double()
        bb = np.ascontiguousarray(b, np.float64) if b is not None else None
        self._chk(self.L.fhx_kr_dot(self.h, _ptr(a, ctypes.c_double), _ptr(bb, ctypes.c_double) if bb is not None else None, len(a), ctypes.byref(out)))
        return out.value


# ---- merging of nearby contacts (fhx_cni_*) --------------------------------------------------------------------------
class CniInfo(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int64) for k in ("rows", "nodes", "components", "selected", "pick_rounds", "largest_component")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


CNI_RECORD = np.dtype([("chr", np.int32), ("reserved", np.int32), ("n_lo", np.int64), ("n_hi", np.int64), ("cc", np.int64),
                       ("p", np.float64), ("q", np.float64), ("box_min_lo", np.int64), ("box_max_lo", np.int64),
                       ("box_min_hi", np.int64), ("box_max_hi", np.int64), ("sum_cc", np.int64), ("box_cells", np.int64),
                       ("component_size", np.int64), ("first_row", np.int64)])


class CniContext(_Handle):
    """Connected-component merging of significant contacts on one GPU (fhx_cni_*).  Raises without the library or a GPU."""
    PREFIX = "cni"

    def load(self, chr_ids, n1, n2, cc, p, q, bin_size):
        c = _i32(chr_ids)
        a = [np.ascontiguousarray(v, np.int64) for v in (n1, n2, cc)]
        f = [np.ascontiguousarray(v, np.float64) for v in (p, q)]
        nodes = ctypes.c_int64()
        self._chk(self.L.fhx_cni_load(self.h, _ptr(c, ctypes.c_int32), *[_ptr(v, ctypes.c_int64) for v in a],
                                      *[_ptr(v, ctypes.c_double) for v in f], len(c), int(bin_size), ctypes.byref(nodes)))
        return nodes.value

    def run(self, connectivity=8, top_percent=100, neighborhood=2, sort_order=0):
        info = CniInfo()
        self._chk(self.L.fhx_cni_run(self.h, connectivity, top_percent, neighborhood, sort_order, ctypes.byref(info)))
        out = np.zeros(info.selected, CNI_RECORD)
        if info.selected:
            self._chk(self.L.fhx_cni_get_records(self.h, out.ctypes.data_as(ctypes.c_void_p), len(out), None))
        return out, info


# ---- HiC-Pro matrix -> contact columns and per-bin totals (fhx_hp_*) ------------------------------------------------------
(HP_OK, HP_TOKENS, HP_INDEX, HP_COUNT, HP_FRACTION, HP_ABSENT, HP_BYTES, HP_LONG_LINE, HP_TOTAL, HP_INTERNAL) = range(10)


class HpRefused(FhxError):
    """fhx_hp_parse_matrix refused the file: why = one of HP_*, line = the smallest offending 1-based line (0: none), index = the
    absent index for HP_ABSENT"""

    def __init__(self, code, message, why, line, index):
        super().__init__(code, message)
        self.why, self.line, self.index = int(why), int(line), int(index)


class HpContext(_Handle):
    """A HiC-Pro matrix parsed and accumulated on one GPU (fhx_hp_*).  Raises without the library or a GPU."""
    PREFIX = "hp"
    REFUSED = HpRefused

    def __init__(self, device=0):
        self.n_slots = self.n_rows = 0
        super().__init__(device)

    def load_bins(self, index_base, chr_ids, mids):
        """dense table over [index_base, index_base + len(chr_ids)); chr id -1 = index absent from the bed"""
        c, m = _i32(chr_ids), _i32(mids)
        if len(c) != len(m):
            raise ValueError("chr_ids and mids differ in length")
        self._chk(self.L.fhx_hp_load_bins(self.h, int(index_base), _ptr(c, ctypes.c_int32), _ptr(m, ctypes.c_int32), len(c)))
        self.n_slots, self.n_rows = len(c), 0

    def parse_matrix(self, path):
        """-> number of rows; HpRefused for a file outside the device grammar or with an index the bed does not list"""
        n, why, line, index = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self.n_rows = 0
        rc = self.L.fhx_hp_parse_matrix(self.h, os.fsencode(path), ctypes.byref(n), ctypes.byref(why), ctypes.byref(line), ctypes.byref(index))
        self._chk(rc, why.value, line.value, index.value)
        self.n_rows = n.value
        return self.n_rows

    def totals(self):
        out = np.zeros(self.n_slots, np.int64)
        self._chk(self.L.fhx_hp_totals(self.h, _ptr(out, ctypes.c_int64)))
        return out

    def fetch_rows(self):
        """(chr1, mid1, chr2, mid2, count), int32, file order"""
        return self._fetch_columns("rows", self.n_rows)


(VP_OK, VP_TOKENS, VP_NAME, VP_POSITION, VP_RANGE, VP_BYTES, VP_LONG_LINE, VP_NAMES, VP_COUNT, VP_RES, VP_INTERNAL, VP_PAIRS) = range(12)
VP_STAGE_NAMES = ("read_upload", "newline_scan", "parse", "names_keys", "sort", "cells")


class VpRefused(_LineRefused):
    """fhx_vp_bin_file refused the file: why = one of VP_*, line = the smallest offending 1-based line (0: the reason belongs to
    no line)"""


class VpContext(_Handle):
    """A validPairs file binned, sorted and counted on one GPU (fhx_vp_*).  Raises without the library or a GPU."""
    PREFIX = "vp"
    REFUSED = VpRefused
    STAGE_NAMES = VP_STAGE_NAMES
    COUNTS = _i64s("lines", "pairs", "cells") + (("names", ctypes.c_int32),)     # lines read, pairs kept by the filters, cells, distinct names

    def __init__(self, device=0):
        self.n_cells = 0
        super().__init__(device)

    def bin_file(self, path, res):
        """-> number of cells; VpRefused for a file outside the device grammar"""
        n, why, line = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        self.n_cells = 0
        rc = self.L.fhx_vp_bin_file(self.h, os.fsencode(path), int(res), ctypes.byref(n), ctypes.byref(why), ctypes.byref(line))
        self._chk(rc, why.value, line.value)
        self.n_cells = n.value
        return self.n_cells

    def names(self):
        """the chromosome names in bytewise order: the chr columns index this list"""
        return [self.L.fhx_vp_name(self.h, k).decode() for k in range(self.counts()["names"])]

    def fetch_cells(self):
        """(chr1, mid1, chr2, mid2, count), int32, in the script's text order"""
        return self._fetch_columns("cells", self.n_cells)


def vp_write_contacts(path, names, chr1, mid1, chr2, mid2, count, gzip_level=1, threads=0):
    """the cells as validPairs2FitHiC-fixedSize.sh writes them (the count right-justified to width 7), size-tagged gzip members"""
    arr_names = (ctypes.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    i32 = [_i32(v) for v in (chr1, mid1, chr2, mid2, count)]
    rc = lib().fhx_vp_write_contacts(os.fsencode(path), arr_names, len(names), *[_ptr(v, ctypes.c_int32) for v in i32], len(i32[0]),
                                     int(gzip_level), int(threads))
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_vp_write_contacts(%s)" % path)


(MS_OK, MS_TOKENS, MS_FIELD, MS_BYTES, MS_LONG_LINE, MS_FDR, MS_INTERNAL) = range(7)
MS_MIDPOINT, MS_NAME, MS_KEPT = 7, 8, 9                             # refusals of the interact track alone
MS_NAME_TAB, MS_NAME_BYTES, MS_NAME_NUMERIC, MS_NAMES = 10, 11, 12, 13     # refusals of the per-chromosome split alone
MS_SPLIT_NAMES, MS_SPLIT_NAME_BYTES = 4096, 64
MS_FDR_BYTES = 32
MS_STAGE_NAMES = ("read_upload", "newline_scan", "select", "gather", "copy_out")
MS_TRACK_STAGE_NAMES = ("read_upload", "newline_scan", "select", "deferred_round_trip", "format", "copy_out")
MS_SPLIT_STAGE_NAMES = ("read_upload", "newline_scan", "names_select", "sort_gather", "copy_out")


class MsRefused(_LineRefused):
    """fhx_ms_select_file refused the file: why = one of MS_*, line = the smallest offending 1-based line (0: the reason belongs
    to no line)"""


class MsContext(_Handle):
    """The FDR subset of a significances file made on one GPU (fhx_ms_*).  Raises without the library or a GPU."""
    PREFIX = "ms"
    REFUSED = MsRefused
    STAGE_NAMES = MS_STAGE_NAMES
    COUNTS = _i64s("lines", "kept", "bytes")                         # lines read, lines kept, bytes of the subset

    def select_file(self, path, fdr_text, key_bound, zero_kept, strict=False, skip_first_line=True):
        """-> bytes of the subset; MsRefused for a file outside the device grammar"""
        n, why, line = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self.L.fhx_ms_select_file(self.h, os.fsencode(path), fdr_text, len(fdr_text), int(key_bound), int(bool(zero_kept)),
                                       int(bool(strict)), int(bool(skip_first_line)), ctypes.byref(n), ctypes.byref(why), ctypes.byref(line))
        self._chk(rc, why.value, line.value)
        return n.value

    def subset(self):
        """the kept lines, verbatim and in file order, each ending in a newline"""
        buf = np.empty(self.counts()["bytes"], np.uint8)
        self._chk(self.L.fhx_ms_copy_subset(self.h, buf.ctypes.data_as(ctypes.c_void_p), len(buf)))
        return buf.tobytes()

    def track_file(self, path, fdr_text, key_bound, zero_kept):
        """the interact track of the rows with field 7 < fdr -> its bytes; MsRefused for a file outside the device grammar"""
        n, why, line = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self.L.fhx_ms_track_file(self.h, os.fsencode(path), fdr_text, len(fdr_text), int(key_bound), int(bool(zero_kept)),
                                      ctypes.byref(n), ctypes.byref(why), ctypes.byref(line))
        self._chk(rc, why.value, line.value)
        return n.value

    def track_counts(self):
        """lines read, lines kept, kept lines whose score the host made, bytes of the track"""
        return self._counts(_i64s("lines", "kept", "deferred", "bytes"), "track_counts")

    def track_stage_seconds(self):
        return self._stage_seconds(MS_TRACK_STAGE_NAMES, "track_stage_seconds")

    def track(self):
        """the script's two fixed lines and one line per kept row, in file order"""
        buf = np.empty(self.track_counts()["bytes"], np.uint8)
        self._chk(self.L.fhx_ms_copy_track(self.h, buf.ctypes.data_as(ctypes.c_void_p), len(buf)))
        return buf.tobytes()

    def split_file(self, path, fdr_text, key_bound, zero_kept):
        """the subsets of the rows with field 1 == field 3 and field 7 <= fdr, one per name of field 1 -> the number of names;
        MsRefused for a file outside the device grammar"""
        n, why, line = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self.L.fhx_ms_split_file(self.h, os.fsencode(path), fdr_text, len(fdr_text), int(key_bound), int(bool(zero_kept)),
                                      ctypes.byref(n), ctypes.byref(why), ctypes.byref(line))
        self._chk(rc, why.value, line.value)
        return n.value

    def split_counts(self):
        """lines read, and per name (in the order of split_names) its kept lines and their bytes"""
        a, n = ctypes.c_int64(0), ctypes.c_int32(0)
        self._chk(self.L.fhx_ms_split_counts(self.h, ctypes.byref(a), ctypes.byref(n), None, None, 0))
        kept, nbytes = np.zeros(max(n.value, 1), np.int64), np.zeros(max(n.value, 1), np.int64)
        self._chk(self.L.fhx_ms_split_counts(self.h, None, None, _ptr(kept, ctypes.c_int64), _ptr(nbytes, ctypes.c_int64), n.value))
        return dict(lines=a.value, kept=kept[:n.value].tolist(), bytes=nbytes[:n.value].tolist())

    def split_names(self):
        """the names of field 1 as bytes, in no particular order; split_text(k) is the subset of the k-th"""
        n = len(self.split_counts()["kept"])
        buf = np.zeros(max(n, 1) * MS_SPLIT_NAME_BYTES, np.uint8)
        self._chk(self.L.fhx_ms_split_names(self.h, buf.ctypes.data_as(ctypes.c_void_p), n))
        raw = buf.tobytes()
        return [raw[k * MS_SPLIT_NAME_BYTES:(k + 1) * MS_SPLIT_NAME_BYTES].rstrip(b"\0") for k in range(n)]

    def split_stage_seconds(self):
        return self._stage_seconds(MS_SPLIT_STAGE_NAMES, "split_stage_seconds")

    def split_text(self, index, n_bytes):
        """the kept lines of one name, verbatim and in file order, each ending in a newline"""
        buf = np.empty(int(n_bytes), np.uint8)
        self._chk(self.L.fhx_ms_copy_split(self.h, int(index), buf.ctypes.data_as(ctypes.c_void_p), len(buf)))
        return buf.tobytes()


def ms_score_text(field, certify=False):
    """The two score fields of an interact line for one field 7, as bytes: the deferred route (the host's strtod, log and awk's number
    printing), or with certify the kernel's route run on the host - b"" where it would defer.  Needs no GPU."""
    out = ctypes.create_string_buffer(32)
    n = lib().fhx_ms_score_text(field, len(field), int(bool(certify)), out, 32)
    if n < 0:
        raise FhxError(n, "fhx_ms_score_text(%r)" % (field,))
    return out.raw[:n]


# ---- Juicer dump text -> contact counts (fhx_jc_*) -------------------------------------------------------------------------
(JC_OK, JC_BYTES, JC_LONG_LINE, JC_TOKENS, JC_BIN, JC_GRID, JC_RANGE, JC_COUNT, JC_FRACTION, JC_INTERNAL) = range(10)
JC_STAGE_NAMES = ("read_upload", "newline_scan", "parse", "format", "copy_out")


class JcRefused(_LineRefused):
    """fhx_jc_convert_file refused the file: why = one of JC_*, line = the smallest offending 1-based line"""


class JcContext(_Handle):
    """Juicer dump files converted on one GPU (fhx_jc_*): their output text and, in midpoint mode, their rows in HBM.  Raises
    without the library or a GPU."""
    PREFIX = "jc"
    REFUSED = JcRefused
    STAGE_NAMES = JC_STAGE_NAMES
    COUNTS = _i64s("lines", "rows", "bytes")                         # lines read, rows kept, bytes of text kept

    def reset(self):
        self._chk(self.L.fhx_jc_reset(self.h))

    def convert_file(self, path, name1, name2, resolution=0, ids=(0, 0), keep_text=True, keep_rows=False):
        """one dump appended to the handle's text and / or rows -> its number of lines; resolution 0 is verbatim mode.  JcRefused
        for a file outside the device grammar: the handle is then empty."""
        n, why, line = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self.L.fhx_jc_convert_file(self.h, os.fsencode(path), name1.encode(), name2.encode(), int(resolution), int(ids[0]), int(ids[1]),
                                        int(bool(keep_text)), int(bool(keep_rows)), ctypes.byref(n), ctypes.byref(why), ctypes.byref(line))
        self._chk(rc, why.value, line.value)
        return n.value

    def text(self):
        """the output lines kept so far, in the order of the calls and of the lines"""
        buf = np.empty(self.counts()["bytes"], np.uint8)
        self._chk(self.L.fhx_jc_copy_text(self.h, buf.ctypes.data_as(ctypes.c_void_p), len(buf)))
        return buf.tobytes()

    def fetch_rows(self):
        """(chr1, mid1, chr2, mid2, count), int32, in the order of the calls and of the lines"""
        return self._fetch_columns("rows", self.counts()["rows"])


# ---- FASTA -> cut sites -> the fragments of `fithic -r 0` (fhx_dg_*) ---------------------------------------------------------
(DG_OK, DG_BYTES, DG_BLANK, DG_LONG_LINE, DG_CONTIG_LENGTH, DG_EMPTY_NAME, DG_NAME_CHARS, DG_DUPLICATE, DG_NO_HEADER, DG_INTERNAL) = range(10)
DG_MAX_MOTIF, DG_MAX_MOTIFS = 16, 64
DG_STAGE_NAMES = ("read_upload", "newline_scan", "class_pass", "sites", "sort", "fetch")


class DgRefused(_LineRefused):
    """fhx_dg_digest_file refused the file: why = one of DG_*, line = the smallest offending 1-based line"""


class DgContext(_Handle):
    """One FASTA digested on one GPU (fhx_dg_*): contig names and lengths on the host, the sorted cut sites in HBM.  Raises without
    the library or a GPU."""
    PREFIX = "dg"
    REFUSED = DgRefused
    STAGE_NAMES = DG_STAGE_NAMES
    COUNTS = _i64s("lines", "contigs", "bases", "sites")             # lines read, contigs, their bases in all, cut sites

    def digest_file(self, path, motifs):
        """motifs = [(letters of acgt, offset of the cut), ...], an N of the site expanded.  DgRefused for a file outside the
        device grammar: the handle is then empty."""
        buf = np.zeros((len(motifs), DG_MAX_MOTIF), np.uint8)
        for k, (m, _) in enumerate(motifs):
            buf[k, :len(m)] = np.frombuffer(m.encode("ascii"), np.uint8)
        lengths = np.array([len(m) for m, _ in motifs], np.int32)
        offsets = np.array([o for _, o in motifs], np.int32)
        why, line = ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self.L.fhx_dg_digest_file(self.h, os.fsencode(path), buf.ctypes.data_as(ctypes.c_char_p), _ptr(lengths, ctypes.c_int32),
                                       _ptr(offsets, ctypes.c_int32), len(motifs), ctypes.byref(why), ctypes.byref(line))
        self._chk(rc, why.value, line.value)

    def names(self):
        return [self.L.fhx_dg_name(self.h, k) for k in range(self.counts()["contigs"])]

    def lengths(self):
        return np.array([self.L.fhx_dg_contig_length(self.h, k) for k in range(self.counts()["contigs"])], np.int64)

    def fetch_sites(self):
        """(contig, position), int32, ordered by contig, then position; equal sites are kept"""
        n = self.counts()["sites"]
        contig, position = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._chk(self.L.fhx_dg_fetch_sites(self.h, _ptr(contig, ctypes.c_int32), _ptr(position, ctypes.c_int32)))
        return contig, position


def dg_write_fragments(path, lengths, site_contig, site_position, gzip_level=6, threads=0):
    """the fragments file of `fithic -r 0` (gzip): `chr<k> \\t 0 \\t end \\t 1 \\t 1` per fragment of the digest.  Host side, no GPU."""
    lengths = np.ascontiguousarray(lengths, np.int64)
    c, p = _i32(site_contig), _i32(site_position)
    rc = lib().fhx_dg_write_fragments(os.fsencode(path), len(lengths), _ptr(lengths, ctypes.c_int64), _ptr(c, ctypes.c_int32),
                                      _ptr(p, ctypes.c_int32), len(c), int(gzip_level), int(threads))
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_dg_write_fragments(%s)" % path)


def dg_write_bed(path, names, lengths, site_contig, site_position, threads=0):
    """HiC-Pro's fragment bed of the digest (plain text); names are bytes.  Host side, no GPU."""
    lengths = np.ascontiguousarray(lengths, np.int64)
    c, p = _i32(site_contig), _i32(site_position)
    arr = (ctypes.c_char_p * max(len(names), 1))(*names)
    rc = lib().fhx_dg_write_bed(os.fsencode(path), arr, len(lengths), _ptr(lengths, ctypes.c_int64), _ptr(c, ctypes.c_int32),
                                _ptr(p, ctypes.c_int32), len(c), int(threads))
    if rc != FHX_OK:
        raise FhxError(rc, "fhx_dg_write_bed(%s)" % path)


# ---- allValidPairs -> contact counts between restriction fragments (fhx_fp_*) -------------------------------------------------
(FP_OK, FP_TOKENS, FP_NAME, FP_POSITION, FP_RANGE, FP_BYTES, FP_LONG_LINE, FP_COUNT, FP_INTERNAL, FP_PAIRS) = range(10)
FP_MAX_CONTIGS, FP_NAME_BYTES = 4096, 64
FP_STAGE_NAMES = ("read_upload", "newline_scan", "parse", "sort", "cells", "table")


class FpRefused(_LineRefused):
    """fhx_fp_bin_file refused the file: why = one of FP_*, line = the smallest offending 1-based line (0: the reason belongs to
    no line)"""


class FpContext(_Handle):
    """A validPairs file binned to the fragments of a digest, sorted and counted on one GPU (fhx_fp_*).  Raises without the library
    or a GPU."""
    PREFIX = "fp"
    REFUSED = FpRefused
    STAGE_NAMES = FP_STAGE_NAMES
    # lines read, pairs kept, lines dropped for a name, lines dropped as same-fragment, cells
    COUNTS = _i64s("lines", "pairs", "dropped_name", "same_fragment", "cells")

    def __init__(self, device=0):
        self.n_cells = 0
        super().__init__(device)

    def load_table(self, names, name_contig, first, ends):
        """names: bytes of 1 to 63 bytes each; name_contig[k] = the contig name k stands for, -1 = its lines are dropped; first:
        n_contigs + 1 row offsets into ends, the ascending fragment ends of every contig"""
        text = np.zeros((len(names), FP_NAME_BYTES), np.uint8)
        for k, n in enumerate(names):
            if not 1 <= len(n) < FP_NAME_BYTES:
                raise ValueError("name %r: 1 to %d bytes are expected" % (n, FP_NAME_BYTES - 1))
            text[k, :len(n)] = np.frombuffer(n, np.uint8)
        which, ends = _i32(name_contig), _i32(ends)
        first = np.ascontiguousarray(first, np.int64)
        self.n_cells = 0
        self._chk(self.L.fhx_fp_load_table(self.h, text.ctypes.data_as(ctypes.c_char_p), _ptr(which, ctypes.c_int32), len(names),
                                           _ptr(first, ctypes.c_int64), len(first) - 1, _ptr(ends, ctypes.c_int32), len(ends)))

    def bin_file(self, path):
        """-> number of cells; FpRefused for a file outside the device grammar"""
        n, why, line = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        self.n_cells = 0
        rc = self.L.fhx_fp_bin_file(self.h, os.fsencode(path), ctypes.byref(n), ctypes.byref(why), ctypes.byref(line))
        self._chk(rc, why.value, line.value)
        self.n_cells = n.value
        return self.n_cells

    def fetch_cells(self):
        """(contig1, end1, contig2, end2, count), int32, in ascending (fragment row 1, fragment row 2)"""
        return self._fetch_columns("cells", self.n_cells)


# ---- contact rows in HBM summed onto N-fold coarser loci (fhx_cz_*) -----------------------------------------------------------
(CZ_OK, CZ_LOCUS, CZ_COUNT, CZ_SUM, CZ_INTERNAL) = range(5)
CZ_STAGE_NAMES = ("upload", "keys", "sort", "heads_sums", "cells", "plan")


class CzRefused(FhxError):
    """fhx_cz_coarsen_* refused the rows: why = one of CZ_*, row = the smallest offending 0-based row; for CZ_SUM, which belongs to
    no row, the first cell above 2^31 - 1 as coarse row 1 << 32 | coarse row 2"""

    def __init__(self, code, message, why, row):
        super().__init__(code, message)
        self.why, self.row = int(why), int(row)


class CzContext(_Handle):
    """Contact rows re-keyed to the coarse loci of a plan, sorted and summed on one GPU (fhx_cz_*).  Raises without the library or a
    GPU."""
    PREFIX = "cz"
    REFUSED = CzRefused
    STAGE_NAMES = CZ_STAGE_NAMES
    COUNTS = _i64s("rows", "diagonal", "cells")                      # rows given, rows dropped as diagonal, cells

    def __init__(self, device=0):
        self.n_cells = 0
        super().__init__(device)

    def reset(self):
        self.n_cells = 0
        self._chk(self.L.fhx_cz_reset(self.h))

    def load_plan(self, first, fine_mid, group_of, coarse_chr, coarse_mid):
        """first: n_chr + 1 row offsets into fine_mid by chromosome id, the strictly ascending mids of every id; group_of: the coarse
        row of every fine row; (coarse_chr, coarse_mid): the coarse loci"""
        first = np.ascontiguousarray(first, np.int64)
        a = [_i32(v) for v in (fine_mid, group_of, coarse_chr, coarse_mid)]
        self.n_cells = 0
        self._chk(self.L.fhx_cz_load_plan(self.h, _ptr(first, ctypes.c_int64), len(first) - 1, _ptr(a[0], ctypes.c_int32), _ptr(a[1], ctypes.c_int32),
                                          len(a[0]), _ptr(a[2], ctypes.c_int32), _ptr(a[3], ctypes.c_int32), len(a[2])))

    def _done(self, rc, n, why, row):
        self.n_cells = 0
        self._chk(rc, why.value, row.value)
        self.n_cells = n.value
        return self.n_cells

    def coarsen_device(self, ptrs, n, stream=0, diagonal=True):
        """five device pointers (chr1, mid1, chr2, mid2, count: int32), n rows, the producer's stream -> number of cells; CzRefused
        for rows outside the plan"""
        cells, why, row = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self.L.fhx_cz_coarsen_device(self.h, *[_P(int(p)) if p else None for p in ptrs], int(n), _P(int(stream)) if stream else None,
                                          int(bool(diagonal)), ctypes.byref(cells), ctypes.byref(why), ctypes.byref(row))
        return self._done(rc, cells, why, row)

    def coarsen_host(self, chr1, mid1, chr2, mid2, count, diagonal=True):
        """the same on five host columns, uploaded first"""
        cols = [_i32(v) for v in (chr1, mid1, chr2, mid2, count)]
        cells, why, row = ctypes.c_int64(0), ctypes.c_int32(0), ctypes.c_int64(0)
        rc = self.L.fhx_cz_coarsen_host(self.h, *[_ptr(v, ctypes.c_int32) for v in cols], len(cols[0]), int(bool(diagonal)),
                                        ctypes.byref(cells), ctypes.byref(why), ctypes.byref(row))
        return self._done(rc, cells, why, row)

    def fetch_cells(self):
        """(chr1, mid1, chr2, mid2, count), int32, in ascending (coarse row 1, coarse row 2)"""
        return self._fetch_columns("cells", self.n_cells)
