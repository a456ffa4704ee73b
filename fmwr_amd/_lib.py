"""ctypes binding of libfmx.so (include/fmx.h).  This is the same binding a reference-side
maintainer would write (INTEGRATION.md shows the Rcpp form); Python is only the test/bench driver.

There is no fallback: if the library is missing, or no GPU is visible, calls raise.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMX_LIB_PATH") or os.path.join(_PKG, "libfmx.so")  # FMX_LIB_PATH: A/B builds of the library (tuning only)

OK, ERR_INVALID, ERR_HIP, ERR_NOGPU, ERR_STATE = 0, 1, 2, 3, 4
TASK_CLASSIFICATION, TASK_REGRESSION, TASK_RANKING = 10, 20, 30
SOLVER_MCMC, SOLVER_ALS, SOLVER_SGD, SOLVER_FTRL, SOLVER_TDAP = 100, 200, 300, 500, 600
MODE_SEQUENTIAL, MODE_MINIBATCH = 0, 1
LINK_NONE, LINK_LOGISTIC, LINK_CLAMP, LINK_PROBIT = 0, 1, 2, 3
DIV_REL_SCORE, DIV_REL_MINMAX = 0, 1
SIM_COSINE, SIM_DOT = 0, 1
REDUCE_MEAN, REDUCE_SUM = 0, 1
COLUMNS_UNIFORM, COLUMNS_ZIPF = 1, 2
EVAL_LL, EVAL_AUC, EVAL_ACC, EVAL_RMSE, EVAL_MSE, EVAL_MAE = 0, 111, 222, 333, 444, 555
EVAL_PAIR_ACC, EVAL_BPR = 666, 777  # ranking engines only
KERNEL_ROWS_FORWARD, KERNEL_COLS_UPDATE, KERNEL_SCALAR, KERNEL_SEQ, KERNEL_ALS_SWEEP = 0, 1, 2, 3, 4

# every symbol include/fmx.h declares (tests/test_abi.py checks the library exports all of them)
SYMBOLS = [
    "fmx_last_error", "fmx_device_count", "fmx_config_default", "fmx_engine_create", "fmx_engine_destroy", "fmx_set_params",
    "fmx_get_params", "fmx_engine_save", "fmx_engine_load", "fmx_matrix_from_rlist", "fmx_matrix_from_dgc", "fmx_matrix_from_csr", "fmx_matrix_synthetic", "fmx_matrix_synthetic_fields", "fmx_matrix_synthetic_iid", "fmx_matrix_synthetic_ragged", "fmx_matrix_synthetic_values", "fmx_train_stream", "fmx_matrix_set_labels", "fmx_matrix_set_fields", "fmx_matrix_destroy",
    "fmx_matrix_info", "fmx_matrix_export", "fmx_matrix_scales", "fmx_matrix_normalize", "fmx_predict", "fmx_train", "fmx_train_grid", "fmx_train_order", "fmx_num_batches",
    "fmx_step", "fmx_grad", "fmx_grad_buffer", "fmx_grad_elem_bytes", "fmx_grad_layout", "fmx_grad_begin", "fmx_grad_chunk", "fmx_apply_chunk", "fmx_apply", "fmx_sync", "fmx_stream", "fmx_predict_device",
    "fmx_als_plan_info", "fmx_als_tiled_info", "fmx_als_order_info", "fmx_als_carry_q", "fmx_als_vsweep", "fmx_mcmc_vsweep", "fmx_als_train", "fmx_mcmc_train", "fmx_mcmc_train_from", "fmx_mcmc_v_hyper", "fmx_evaluate", "fmx_train_tracked", "fmx_trace_size", "fmx_trace_get", "fmx_trace_params",
    "fmx_profile_enable", "fmx_profile_get", "fmx_profile_reset", "fmx_rows_tune_info", "fmx_matrix_rows_form", "fmx_measure_gather", "fmx_measure_gather_occ", "fmx_measure_gather_matrix", "fmx_rccl_selftest",
    "fmx_get_rows", "fmx_set_rows", "fmx_init_normal", "fmx_compact_info", "fmx_compact_count", "fmx_compact_reserve", "fmx_grad_compact", "fmx_compact_records", "fmx_apply_compact",
    "fmx_vsweep_device", "fmx_group_info", "fmx_source_open", "fmx_source_next", "fmx_source_close",
    "fmx_apply_compact_parts", "fmx_layout_info", "fmx_owner_configure", "fmx_owner_info", "fmx_rows_pack", "fmx_rows_unpack",
    "fmx_topk", "fmx_topk_device", "fmx_contrib", "fmx_contrib_device", "fmx_contrib_summary",
    "fmx_matrix_pairs", "fmx_matrix_pairs_hard",
    "fmx_heldout_rank", "fmx_heldout_rank_device", "fmx_heldout_metrics",
    "fmx_rank_lists", "fmx_rank_lists_device", "fmx_topk_lists", "fmx_topk_lists_device", "fmx_project", "fmx_project_device",
    "fmx_fold_in", "fmx_fold_in_pairs",
    "fmx_diversify", "fmx_diversify_device",
    "fmx_neighbors", "fmx_neighbors_device",
    "fmx_index_build", "fmx_index_from_assign", "fmx_index_info", "fmx_index_export", "fmx_index_free", "fmx_topk_index", "fmx_topk_index_device",
    "fmx_interactions", "fmx_interactions_device", "fmx_interactions_summary",
    "fmx_metrics", "fmx_metrics_device",
    "fmx_predict_calibrated", "fmx_predict_calibrated_device", "fmx_reliability", "fmx_reliability_device",
    "fmx_calibrate_platt", "fmx_calibrate_platt_device", "fmx_calibrate_isotonic", "fmx_calibrate_isotonic_device",
    "fmx_matrix_take", "fmx_matrix_take_device", "fmx_split_assign", "fmx_split_assign_device", "fmx_matrix_select", "fmx_matrix_select_device",
    "fmx_free_device", "fmx_matrix_split_entries", "fmx_row_permutation", "fmx_row_permutation_device",
    "fmx_matrix_column_stats", "fmx_matrix_column_stats_device", "fmx_column_map_select", "fmx_column_map_select_device",
    "fmx_column_map_hash", "fmx_column_map_hash_device", "fmx_matrix_remap_columns", "fmx_matrix_remap_columns_device",
    "fmx_matrix_join", "fmx_matrix_join_device", "fmx_matrix_stack",
    "fmx_matrix_column_quantiles", "fmx_matrix_bin_columns",
    "fmx_matrix_cross",
    "fmx_target_stats", "fmx_target_stats_device", "fmx_target_table_from_arrays", "fmx_target_table_info", "fmx_target_table_export",
    "fmx_target_table_free", "fmx_matrix_encode_targets", "fmx_matrix_encode_targets_device",
]
# include/fmx.h: the targets of fmx_target_stats, the kinds of fmx_matrix_encode_targets, the most terms and parts of a table
TARGET_POSITIVE, TARGET_LABEL = 0, 1
ENCODE_MEAN, ENCODE_COUNT = 1, 2
TARGET_MAX_TERMS = 64
TARGET_MAX_PARTS = 64
# include/fmx.h: the most segments and terms of one fmx_matrix_cross, and the first stream of its hash
CROSS_MAX_SEGMENTS = 4096
CROSS_MAX_TERMS = 64
CROSS_STREAM0 = 128
# include/fmx.h: the most bins of one fmx_matrix_column_quantiles, the most edges of one column of fmx_matrix_bin_columns
BINS_MAX_BINS = 65536
BINS_MAX_EDGES = 65535
# include/fmx.h: the most blocks of one fmx_matrix_join, the most parts of one fmx_matrix_stack
JOIN_MAX_BLOCKS = 16
STACK_MAX_PARTS = 1024
# include/fmx.h: fmx_column_rule's counts and rare modes, fmx_matrix_remap_columns' combine modes and the map value that removes a column
COLUMNS_BY_ROWS, COLUMNS_BY_ENTRIES = 0, 1
RARE_DROP, RARE_BUCKET = 0, 1
COMBINE_KEEP, COMBINE_SUM, COMBINE_FIRST = 0, 1, 2
COLUMN_DROP = 0xFFFFFFFF
# include/fmx.h: fmx_split_spec's scopes and orders, and the part of a row that belongs to no segment
SPLIT_ROWS, SPLIT_WITHIN_GROUPS, SPLIT_GROUPS = 0, 1, 2
SPLIT_ORDER_HASH, SPLIT_ORDER_TAIL = 0, 1
SPLIT_NO_PART = 0xFFFFFFFF
# include/fmx.h: the columns of fmx_metrics' value rows (CLASSIFICATION | REGRESSION) and count rows, and their widths
MET_VALUES, MET_COUNTS = 6, 4
MET_AUC, MET_LOGLOSS, MET_ACCURACY, MET_BRIER, MET_MEAN_PRED, MET_MEAN_LABEL = 0, 1, 2, 3, 4, 5
MET_MSE, MET_RMSE, MET_MAE, MET_MEAN_ERR = 0, 1, 2, 3
MET_ROWS, MET_POSITIVES, MET_PAIRS2, MET_CORRECT = 0, 1, 2, 3
# include/fmx.h: the calibrator's kinds, the binnings of fmx_reliability and the columns of its value rows
CAL_NONE, CAL_PLATT, CAL_STEPS = 0, 1, 2
BINS_WIDTH, BINS_MASS = 0, 1
CAL_VALUES = 4
CAL_ECE, CAL_MCE, CAL_BRIER, CAL_LOGLOSS = 0, 1, 2, 3


# fmwr_amd/csrc/fmx_test_hooks.h: exported for the GPU tests, not part of the C ABI
TEST_HOOKS = ["fmx_debug_fail_next_plan_build", "fmx_debug_fail_next_comm_init", "fmx_debug_lose_next_seq_multiplier", "fmx_debug_stall_next_persistent_sweep",
              "fmx_debug_contrib_summary_chunk", "fmx_debug_foldin_slab", "fmx_debug_heldout_limits", "fmx_debug_pairs_hard_chunk", "fmx_debug_lists_limits", "fmx_debug_diversify_limits", "fmx_debug_neighbors_limits", "fmx_debug_index_limits", "fmx_debug_interactions_limits", "fmx_debug_metrics_limits", "fmx_debug_take_limits", "fmx_debug_calibrate_limits", "fmx_debug_columns_limits", "fmx_debug_join_limits", "fmx_debug_bins_limits", "fmx_debug_cross_limits", "fmx_debug_target_limits", "fmx_debug_matrix_flags", "fmx_debug_matrix_layout", "fmx_debug_cols_launches",
              "fmx_debug_long_launches", "fmx_debug_rows_launches", "fmx_debug_rows_forward_launches", "fmx_debug_rows_merged_launches",
              "fmx_debug_rows_sched_launches", "fmx_debug_rows_sched_id_limit", "fmx_debug_rows_sched_export",
              "fmx_debug_rows_pace_launches", "fmx_debug_rows_pace_trace", "fmx_debug_rows_ahead_launches",
              "fmx_debug_rows_clock_launches", "fmx_debug_rows_clock_records_of", "fmx_debug_rows_clock_poison"]


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("task", C.c_int32), ("solver", C.c_int32), ("num_factor", C.c_int32),
        ("keep_w0", C.c_int32), ("keep_w1", C.c_int32),
        ("l2_w0", C.c_double), ("l1_w1", C.c_double), ("l2_w1", C.c_double), ("l1_v", C.c_double), ("l2_v", C.c_double),
        ("learn_rate", C.c_double),
        ("alpha_w", C.c_double), ("alpha_v", C.c_double), ("beta_w", C.c_double), ("beta_v", C.c_double),
        ("random_step", C.c_int32), ("mode", C.c_int32), ("batch_rows", C.c_int64),
        ("min_target", C.c_double), ("max_target", C.c_double),
        ("device", C.c_int32), ("batch_reduce", C.c_int32), ("gamma", C.c_double), ("tile_rows", C.c_int64),
        ("state_fp64", C.c_int32), ("exchange_chunks", C.c_int32), ("n_gpus", C.c_int32), ("als_max_levels", C.c_int32), ("seq_reassociate", C.c_int32), ("gpus_share_device", C.c_int32),
    ]


class FieldsSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_dense", C.c_int32), ("n_fields", C.c_int32), ("reserved", C.c_int32),
                ("field_vocab", C.c_void_p), ("skew", C.c_double), ("seed", C.c_uint64)]


class TrackConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("metric", C.c_int32), ("step_size", C.c_int64), ("convergence", C.c_double),
                ("keep_params", C.c_int32), ("reserved", C.c_int32)]


class SplitSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("scope", C.c_int32), ("order", C.c_int32), ("n_folds", C.c_int32), ("hold_count", C.c_int64),
                ("hold_fraction", C.c_double), ("min_keep", C.c_int64), ("seed", C.c_uint64), ("salt", C.c_uint64)]


class ColumnRule(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("by", C.c_int32), ("min_count", C.c_int64), ("max_count", C.c_int64), ("max_features", C.c_int64),
                ("keep_prefix", C.c_uint32), ("rare", C.c_int32), ("n_segments", C.c_int32), ("reserved", C.c_int32), ("segment_base", C.c_void_p)]


class JoinBlock(C.Structure):
    _fields_ = [("m", C.c_void_p), ("rows", C.c_void_p), ("n_ids", C.c_int64), ("col_base", C.c_uint32)]


class BinSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_cols", C.c_int32), ("cols", C.c_void_p), ("edge_offset", C.c_void_p), ("edges", C.c_void_p),
                ("reserved", C.c_int64)]


class CrossTerm(C.Structure):
    _fields_ = [("seg_a", C.c_uint32), ("seg_b", C.c_uint32), ("n_buckets", C.c_uint32), ("reserved", C.c_uint32)]


class CrossSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_segments", C.c_int32), ("segment_base", C.c_void_p), ("n_terms", C.c_int32), ("keep_source", C.c_int32),
                ("terms", C.c_void_p), ("seed", C.c_uint64), ("salt", C.c_uint64), ("reserved", C.c_int64)]


class TargetSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_segments", C.c_int32), ("segment_base", C.c_void_p), ("n_terms", C.c_int32), ("term_segment", C.c_void_p),
                ("n_parts", C.c_int32), ("target", C.c_int32), ("reserved", C.c_int64)]


class EncodeSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("keep_source", C.c_int32), ("kinds", C.c_void_p), ("prior", C.c_double), ("strength", C.c_double),
                ("reserved", C.c_int64)]


class Calibrator(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("n_groups", C.c_int64), ("max_steps", C.c_int32), ("link", C.c_int32),
                ("platt", C.c_void_p), ("n_steps", C.c_void_p), ("thr", C.c_void_p), ("val", C.c_void_p)]


class FmxError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


_lib = None


def lib():
    """Load libfmx.so; raises if it has not been built (python -m fmwr_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build the HIP library first (python -m fmwr_amd.build). "
                              "fmwr_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.fmx_last_error.restype = C.c_char_p
        for name in SYMBOLS + TEST_HOOKS:
            if name != "fmx_last_error":
                getattr(L, name).restype = C.c_int
        # int fmx_matrix_pairs_hard(fmx_engine*, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* positives, int32_t n_neg,
        #                           int32_t n_cand, uint64_t seed, int64_t epoch, fmx_matrix** out)
        L.fmx_matrix_pairs_hard.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int64,
                                            C.POINTER(C.c_void_p)]
        # int fmx_fold_in(fmx_engine*, const fmx_matrix*, const uint32_t* ids, int64_t n_ids, double lambda_w, double lambda_v, int32_t n_newton,
        #                 int32_t apply, double* out_w, double* out_v, int64_t* out_rows, int32_t* out_status)
        L.fmx_fold_in.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]
        # int fmx_fold_in_pairs(fmx_engine*, const fmx_matrix*, const uint32_t* ids, int64_t n_ids, double lambda_w, double lambda_v, int32_t n_newton,
        #                       int32_t apply, double* out_w, double* out_v, int64_t* out_pairs, int32_t* out_status)
        L.fmx_fold_in_pairs.argtypes = L.fmx_fold_in.argtypes
        # int fmx_diversify(fmx_engine*, const fmx_matrix* items, int64_t n, int32_t pool, const int64_t* index, const double* score, int32_t top_k,
        #                   double lambda, int32_t relevance, int64_t* out_index, double* out_score, double* out_margin)   (and the _device form)
        L.fmx_diversify.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
        L.fmx_diversify_device.argtypes = L.fmx_diversify.argtypes
        # int fmx_neighbors(fmx_engine*, const fmx_matrix* queries, const fmx_matrix* items, int32_t top_k, int32_t metric, int32_t skip_self,
        #                   int64_t* out_index, double* out_score)
        L.fmx_neighbors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        # int fmx_neighbors_device(fmx_engine*, const fmx_matrix* queries, int64_t r0, int64_t r1, const fmx_matrix* items, int32_t top_k,
        #                          int32_t metric, int32_t skip_self, void* dev_index_i64, void* dev_score_f64)
        L.fmx_neighbors_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.fmx_debug_neighbors_limits.argtypes = [C.c_int64, C.c_int64]
        # int fmx_index_build(fmx_engine*, const fmx_matrix* items, int32_t n_lists, int32_t n_iter, uint64_t seed, fmx_item_index** out)
        L.fmx_index_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(C.c_void_p)]
        # int fmx_index_from_assign(fmx_engine*, int64_t n_items, int32_t n_lists, const uint32_t* assign, const double* centroid, fmx_item_index** out)
        L.fmx_index_from_assign.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        # int fmx_index_info(const fmx_item_index*, int64_t* n_items, int32_t* n_lists, int32_t* k, int64_t* non_empty)
        L.fmx_index_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # int fmx_index_export(const fmx_item_index*, double* centroid, uint32_t* assign, int64_t* list_ptr, int32_t* list_item)
        L.fmx_index_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmx_index_free.argtypes = [C.c_void_p]
        # int fmx_topk_index(fmx_engine*, const fmx_item_index*, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* exclude,
        #                    int32_t top_k, int32_t n_probe, int link, int64_t* out_index, double* out_score, int64_t* out_scanned)
        L.fmx_topk_index.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        # int fmx_topk_index_device(fmx_engine*, const fmx_item_index*, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items,
        #                           const fmx_matrix* exclude, int32_t top_k, int32_t n_probe, int link, void* dev_index_i64, void* dev_score_f64,
        #                           void* dev_scanned_i64)
        L.fmx_topk_index_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmx_debug_index_limits.argtypes = [C.c_int32, C.c_int64, C.c_int32]
        # int fmx_interactions(fmx_engine*, const fmx_matrix*, int32_t top_m, int64_t* out_a, int64_t* out_b, double* out_value)
        L.fmx_interactions.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        # int fmx_interactions_device(fmx_engine*, const fmx_matrix*, int64_t r0, int64_t r1, int32_t top_m, void* dev_a_i64, void* dev_b_i64,
        #                             void* dev_value_f64)
        L.fmx_interactions_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        # int fmx_interactions_summary(fmx_engine*, const fmx_matrix*, const uint32_t* group_of_feature, int32_t n_groups, double* sum,
        #                              double* abs_sum, int64_t* count)
        L.fmx_interactions_summary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmx_debug_interactions_limits.argtypes = [C.c_int32, C.c_int32, C.c_int64]
        # int fmx_metrics(fmx_engine*, const fmx_matrix*, const uint32_t* group_of_row, int64_t n_groups, int link, double* out_value, int64_t* out_count)
        L.fmx_metrics.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        # int fmx_metrics_device(fmx_engine*, const fmx_matrix*, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, int link,
        #                        void* dev_value_f64, void* dev_count_i64)
        L.fmx_metrics_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        L.fmx_debug_metrics_limits.argtypes = [C.c_int32, C.c_int32, C.c_int64]
        # int fmx_predict_calibrated(fmx_engine*, const fmx_matrix*, const uint32_t* group_of_row, int64_t n_groups, const fmx_calibrator*, int link, double* out)
        L.fmx_predict_calibrated.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Calibrator), C.c_int, C.c_void_p]
        # int fmx_predict_calibrated_device(fmx_engine*, const fmx_matrix*, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups,
        #                                   const fmx_calibrator*, int link, void* dev_out_f64)
        L.fmx_predict_calibrated_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(Calibrator), C.c_int, C.c_void_p]
        # int fmx_reliability(fmx_engine*, const fmx_matrix*, const uint32_t* group_of_row, int64_t n_groups, int32_t n_bins, int32_t binning,
        #                     const fmx_calibrator*, int link, int64_t* count, double* sum_p, double* lo_z, double* hi_z, int64_t* nan_rows, double* value)
        L.fmx_reliability.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(Calibrator), C.c_int] + [C.c_void_p] * 6
        # int fmx_reliability_device(fmx_engine*, const fmx_matrix*, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, int32_t n_bins,
        #                            int32_t binning, const fmx_calibrator*, int link, six device outputs)
        L.fmx_reliability_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.POINTER(Calibrator),
                                             C.c_int] + [C.c_void_p] * 6
        # int fmx_calibrate_platt(fmx_engine*, const fmx_matrix*, const uint32_t* group_of_row, int64_t n_groups, double lambda, int32_t n_newton,
        #                         double* ab, int64_t* rows, int32_t* status)
        L.fmx_calibrate_platt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmx_calibrate_platt_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        # int fmx_calibrate_isotonic(fmx_engine*, const fmx_matrix*, const uint32_t* group_of_row, int64_t n_groups, int32_t n_bins, int32_t* n_steps,
        #                            double* thr, double* val)
        L.fmx_calibrate_isotonic.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmx_calibrate_isotonic_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmx_debug_calibrate_limits.argtypes = [C.c_int64]
        # int fmx_matrix_take(const fmx_matrix*, const int64_t* rows, int64_t n_take, fmx_matrix** out)   (and the _device form)
        L.fmx_matrix_take.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
        L.fmx_matrix_take_device.argtypes = L.fmx_matrix_take.argtypes
        # int fmx_split_assign(int device, int64_t n, const uint32_t* group_of_row, int64_t n_groups, const fmx_split_spec*, uint32_t* out_part)
        L.fmx_split_assign.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(SplitSpec), C.c_void_p]
        L.fmx_split_assign_device.argtypes = L.fmx_split_assign.argtypes
        # int fmx_matrix_select(const fmx_matrix*, const uint32_t* part_of_row, uint32_t which, int32_t complement, fmx_matrix** out, int64_t* out_rows)
        L.fmx_matrix_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p]
        # int fmx_matrix_select_device(const fmx_matrix*, const void* dev_part_u32, uint32_t which, int32_t complement, fmx_matrix** out, void** dev_rows_i64)
        L.fmx_matrix_select_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.fmx_free_device.argtypes = [C.c_void_p]
        # int fmx_matrix_split_entries(const fmx_matrix*, int32_t order, int64_t hold_count, double hold_fraction, int64_t min_keep, uint64_t seed,
        #                              uint64_t salt, fmx_matrix** out_kept, fmx_matrix** out_held)
        L.fmx_matrix_split_entries.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_void_p)]
        # int fmx_row_permutation(int device, int64_t n, uint64_t seed, uint64_t epoch, int64_t* out_rows)   (and the _device form)
        L.fmx_row_permutation.argtypes = [C.c_int, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p]
        L.fmx_row_permutation_device.argtypes = L.fmx_row_permutation.argtypes
        L.fmx_debug_take_limits.argtypes = [C.c_int32, C.c_int32, C.c_int64]
        # int fmx_matrix_column_stats(const fmx_matrix*, int64_t* count, double* value)   (and the _device form)
        L.fmx_matrix_column_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmx_matrix_column_stats_device.argtypes = L.fmx_matrix_column_stats.argtypes
        # int fmx_column_map_select(int device, uint32_t p, const int64_t* count, const fmx_column_rule*, uint32_t* map, uint32_t* new_p,
        #                           uint32_t* new_segment_base)   (and the _device form)
        L.fmx_column_map_select.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.POINTER(ColumnRule), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
        L.fmx_column_map_select_device.argtypes = L.fmx_column_map_select.argtypes
        # int fmx_column_map_hash(int device, uint32_t p, uint32_t n_buckets, uint64_t seed, uint64_t salt, uint32_t keep_prefix, uint32_t* map,
        #                         uint32_t* new_p)   (and the _device form)
        L.fmx_column_map_hash.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        L.fmx_column_map_hash_device.argtypes = L.fmx_column_map_hash.argtypes
        # int fmx_matrix_remap_columns(const fmx_matrix*, const uint32_t* map, uint32_t new_p, int32_t combine, fmx_matrix** out)   (and the _device form)
        L.fmx_matrix_remap_columns.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]
        L.fmx_matrix_remap_columns_device.argtypes = L.fmx_matrix_remap_columns.argtypes
        L.fmx_debug_columns_limits.argtypes = [C.c_int32, C.c_int64, C.c_int64]
        L.fmx_debug_matrix_flags.argtypes = [C.c_void_p, C.c_void_p]
        # int fmx_debug_matrix_layout(const fmx_matrix*, int32_t* dense_prefix, int32_t* n_fields, uint32_t* base /* [FMX_MAX_FIELDS + 1] */)
        L.fmx_debug_matrix_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
        # int fmx_matrix_join(int device, const fmx_join_block* blocks, int32_t n_blocks, int64_t n_out, uint32_t out_p, int32_t labels_from,
        #                     fmx_matrix** out)   (and the _device form)
        L.fmx_matrix_join.argtypes = [C.c_int, C.POINTER(JoinBlock), C.c_int32, C.c_int64, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]
        L.fmx_matrix_join_device.argtypes = L.fmx_matrix_join.argtypes
        # int fmx_matrix_stack(const fmx_matrix* const* parts, int32_t n_parts, fmx_matrix** out)
        L.fmx_matrix_stack.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p)]
        L.fmx_debug_join_limits.argtypes = [C.c_int32, C.c_int32, C.c_int64]
        # int fmx_matrix_column_quantiles(const fmx_matrix*, const uint32_t* cols, int32_t n_cols, int32_t n_bins, float* edges, int32_t* n_edges,
        #                                 int64_t* count, float* range)
        L.fmx_matrix_column_quantiles.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # int fmx_matrix_bin_columns(const fmx_matrix*, const fmx_bin_spec*, uint32_t* new_base, fmx_matrix** out)
        L.fmx_matrix_bin_columns.argtypes = [C.c_void_p, C.POINTER(BinSpec), C.c_void_p, C.POINTER(C.c_void_p)]
        L.fmx_debug_bins_limits.argtypes = [C.c_int32, C.c_int64]
        # int fmx_matrix_cross(const fmx_matrix*, const fmx_cross_spec*, uint32_t* cross_base, fmx_matrix** out)
        L.fmx_matrix_cross.argtypes = [C.c_void_p, C.POINTER(CrossSpec), C.c_void_p, C.POINTER(C.c_void_p)]
        L.fmx_debug_cross_limits.argtypes = [C.c_int32, C.c_int32, C.c_int64]
        # int fmx_target_stats(const fmx_matrix*, const uint32_t* part, const fmx_target_spec*, fmx_target_table** out)   (and the _device form)
        L.fmx_target_stats.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(TargetSpec), C.POINTER(C.c_void_p)]
        L.fmx_target_stats_device.argtypes = L.fmx_target_stats.argtypes
        # int fmx_target_table_from_arrays(int device, const fmx_target_spec* layout, const int64_t* count, const double* sum, fmx_target_table** out)
        L.fmx_target_table_from_arrays.argtypes = [C.c_int, C.POINTER(TargetSpec), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        # int fmx_target_table_info(const fmx_target_table*, int64_t* info /* [8] */)
        L.fmx_target_table_info.argtypes = [C.c_void_p, C.c_void_p]
        # int fmx_target_table_export(const fmx_target_table*, uint32_t* segment_base, uint32_t* term_segment, int64_t* count, double* sum)
        L.fmx_target_table_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmx_target_table_free.argtypes = [C.c_void_p]
        # int fmx_matrix_encode_targets(const fmx_matrix*, const fmx_target_table*, const uint32_t* part, const fmx_encode_spec*, uint32_t* enc_base,
        #                               fmx_matrix** out)   (and the _device form)
        L.fmx_matrix_encode_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(EncodeSpec), C.c_void_p, C.POINTER(C.c_void_p)]
        L.fmx_matrix_encode_targets_device.argtypes = L.fmx_matrix_encode_targets.argtypes
        L.fmx_debug_target_limits.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int64]
        _lib = L
    return _lib


def check(status):
    if status != OK:
        raise FmxError(status, lib().fmx_last_error().decode("utf-8", "replace"))


def default_config():
    cfg = Config()
    check(lib().fmx_config_default(C.byref(cfg)))
    return cfg
