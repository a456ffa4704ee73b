"""fmwr_amd -- MI355X-native engine for the hot path of evanwang1990/FMwR (FM forward, SGD / FTRL-Proximal step,
ALS V sweep) behind the C ABI of include/fmx.h.  Build the library first: python -m fmwr_amd.build"""
from .api import (ALS_solver, FTRL_solver, FmMatrix, MCMC_solver, SGD_solver, TDAP_solver, fm_diversify, fm_embed, fm_explain, fm_fold_in, fm_fold_in_rank, fm_folds, fm_holdout, fm_calibrate, fm_interactions, fm_matrix, fm_metrics, fm_predict_calibrated, fm_prior_correction, fm_reliability, fm_recommend, fm_recommend_metrics, fm_rerank, fm_select, fm_similar, fm_split, fm_track,  # noqa: F401
                  Binning, fm_apply_bins, fm_bin_features, Crossing, fm_apply_crosses, fm_cross_candidates, fm_cross_features, TargetEncoding, fm_apply_targets, fm_encode_targets, ColumnMap, fm_apply_columns, fm_design, fm_stack, fm_feature_stats, fm_hash_features, fm_prune_features, fm_remap_model,
                  fm_index, fm_index_recall, fm_recommend_indexed, fm_rank_evaluate, fm_train, fm_train_rank, fm_update, model_control, predict, solver_control, track_control)
from .engine import Engine, ItemIndex, Matrix, TargetTable  # noqa: F401
