/* Test hooks of libfmx.so -- NOT part of the C ABI (include/fmx.h).  The library exports them so that the GPU tests can arm a fault through ctypes;
 * nothing in the library or its drivers calls them, each is one-shot, and none changes a result.  Kept out of the public header on purpose. */
#ifndef FMX_TEST_HOOKS_H_
#define FMX_TEST_HOOKS_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* the next per-tile plan build of this process fails once with FMX_ERR_HIP, as an allocation failure halfway would (tests/test_gpu_api.py:
 * a failed build leaves no half-built cache behind) */
int fmx_debug_fail_next_plan_build(void);
/* the next fmx_engine_create with cfg.n_gpus > 1 fails where the communicator is initialised -- after the other replicas were created -- as
 * ncclCommInitAll failing on a later device would (tests/test_gpu_group.py: the error path tears everything down, the next create works) */
int fmx_debug_fail_next_comm_init(void);
/* the next launch of the reassociated reference-order learner (cfg.seq_reassociate) never sees the multiplier of its example 7: that worker's bounded wait gives up, every
 * other wait follows, and fmx_get_params / fmx_sync must report FMX_ERR_HIP instead of handing out the NaN (tests/test_gpu_seq_reassoc.py) */
int fmx_debug_lose_next_seq_multiplier(void);
/* in the next persistent exact sweep the plan's first feature does not hand its rows on (als_exact_flow_k: their tags stay where they were; als_exact_persist_k: it is
 * never counted): the features after it never become ready, the bounded waits give up, and the sweep must fail with FMX_ERR_HIP (tests/test_gpu_configs4.py).
 * Takes a few seconds: the waits are bounded generously */
int fmx_debug_stall_next_persistent_sweep(void);
/* the next fmx_contrib_summary cuts the matrix into row chunks of at most `entries` entries instead of its default (tests/test_gpu_contrib.py: the
 * sums do not depend on the chunking beyond rounding); a row longer than that is a chunk of its own */
int fmx_debug_contrib_summary_chunk(int64_t entries);
/* the next fmx_fold_in or fmx_fold_in_pairs works its groups off in slabs of at most `rows` participating rows -- pairs, for the pair call -- (a larger
 * group is a slab of its own) and `groups` groups (tests/test_gpu_foldin.py, tests/test_gpu_foldin_pairs.py: the multi-slab path on small data gives the
 * same bits); 0 keeps a default */
int fmx_debug_foldin_slab(int64_t rows, int64_t groups);
/* the next fmx_heldout_* call holds at most `window` sorted positives per context in a count pass (at most 256) and ranks at most `chunk` context
 * rows per chunk (tests/test_gpu_heldout.py: the multi-window and multi-chunk paths on small data give the same bits); 0 keeps a default */
int fmx_debug_heldout_limits(int32_t window, int64_t chunk);
/* the next fmx_matrix_pairs_hard projects and scores at most `contexts` context rows per chunk (tests/test_gpu_hardneg.py: the chunked path on
 * small data gives the same bits); 0 keeps the default */
int fmx_debug_pairs_hard_chunk(int64_t contexts);
/* from now on (sticky, unlike the hooks above: a call of the list entry points may run in several pieces) fmx_rank_lists* / fmx_topk_lists* take
 * a list through the fused LDS path only if it holds at most `lds_entries` entries (at most 1024), the longer ones through the general path, and
 * rank at most `chunk` context rows per chunk (tests/test_gpu_lists.py: both paths and the multi-chunk path on small data give the same bits);
 * 0 restores a default */
int fmx_debug_lists_limits(int32_t lds_entries, int64_t chunk);
/* from now on (sticky, as the hook above) fmx_diversify* gathers a pool into LDS only if it holds at most `lds_rows` slots -- a negative value: never, every
 * pool takes the global form -- and selects at most `chunk` context rows per launch (tests/test_gpu_diversify.py: both forms and the multi-chunk path
 * give the same bits); 0 restores a default */
int fmx_debug_diversify_limits(int32_t lds_rows, int64_t chunk);
/* from now on (sticky, as the two hooks above) fmx_neighbors* cuts the items into slices of `slice_items` rows (rounded up to a multiple of 256) and
 * ranks at most `chunk_rows` query rows per chunk (tests/test_gpu_neighbors.py: the multi-slice and multi-chunk paths on a few hundred rows give the
 * same bits); 0 restores a default */
int fmx_debug_neighbors_limits(int64_t slice_items, int64_t chunk_rows);
/* from now on (sticky, as the hook above) fmx_topk_index* takes the fine form `fine_form` -- 0 the rule, 1 the context form, 2 the list form; any
 * other value is refused --, ranks at most `chunk_rows` context rows per chunk, and fmx_index_build stages at most `assign_slice_lists` centroids
 * in LDS at a time (tests/test_gpu_index.py: both forms, the multi-chunk path and the carried (best, list) of the multi-slice assign on small
 * data give the same bits); 0 restores a default */
int fmx_debug_index_limits(int32_t fine_form /* 0 rule, 1 context, 2 list */, int64_t chunk_rows, int32_t assign_slice_lists);
/* the next fmx_interactions* call (one-shot: a call takes its limits once, for every piece it runs) sends rows of at most `wave_entries` entries (at
 * most 32) through the wave form and the longer ones through the workgroup form in tiles of `tile_entries` entries (2 .. 32), and the next
 * fmx_interactions_summary gives every workgroup `summary_rows_per_group` rows (tests/test_gpu_interactions.py: every form and boundary at tiny
 * shapes gives the same bits; another row cut moves the summary only by rounding); 0 keeps a default */
int fmx_debug_interactions_limits(int32_t wave_entries, int32_t tile_entries, int64_t summary_rows_per_group);
/* from now on (sticky, as the list, diversify and neighbour hooks) fmx_metrics* counts a group's pairs in the wave form only if it holds at most
 * `wave_rows` rows (at most 64) and in the workgroup form only if it holds at most `lds_rows` rows (at most 1024) -- a negative value: never, the
 * groups go on to the next form; both negative: every group takes the global form -- and runs the forward in calls of `chunk_rows` rows
 * (tests/test_gpu_metrics.py: every form and boundary on a few dozen rows gives the same bits); 0 restores a default */
int fmx_debug_metrics_limits(int32_t wave_rows, int32_t lds_rows, int64_t chunk_rows);
/* from now on (sticky, as the list, diversify and metrics hooks) fmx_matrix_take* -- and with it fmx_matrix_select* -- copies a source of fixed row
 * length through the fixed form only if its rows hold at most `fixed_entries` entries, a take whose longest OUTPUT row holds at most `group_entries` (at
 * most 512) through the lane-group form and everything else through the flat form -- a negative value: never, the take goes on to the next form -- and
 * covers `rows_per_launch` output rows (flat form: 16-byte pieces of the output) per launch (tests/test_gpu_select.py: every form, boundary and the
 * multi-launch path on rows of a few dozen entries give the same bits: it is a copy); 0 restores a default */
int fmx_debug_take_limits(int32_t fixed_entries, int32_t group_entries, int64_t rows_per_launch);
/* from now on (sticky, as the metrics hook) the calibration calls -- fmx_predict_calibrated*, fmx_reliability*, fmx_calibrate_platt*,
 * fmx_calibrate_isotonic* -- run the forward in calls of `chunk_rows` rows (tests/test_gpu_calibrate.py: the multi-call forward on a few dozen rows
 * gives the same bits; the kernels have one form for every group and bin size); 0 restores the default */
int fmx_debug_calibrate_limits(int64_t chunk_rows);
/* from now on (sticky, as the take hook) the column calls -- fmx_matrix_column_stats*, fmx_matrix_remap_columns* -- send a row through the lane-group
 * form of SUM / FIRST only if it holds at most `group_entries` source entries (at most 64; the lane groups are 16, 32 or 64 wide, the narrowest that
 * holds min(group_entries, the longest row)) and the longer ones through the segmented sort -- a negative value: never, every row takes the long
 * form, and the stats never take the unit-value shortcut --, launch the per-entry kernels over `chunk_entries` entries and the per-row, per-column
 * and per-chunk kernels over `rows_per_launch` items (tests/test_gpu_columns.py: every form and boundary on rows of a few entries gives the same
 * bits); 0 restores a default */
int fmx_debug_columns_limits(int32_t group_entries, int64_t chunk_entries, int64_t rows_per_launch);
/* from now on (sticky, as the take hook) fmx_matrix_join* copies a join whose blocks all have a fixed row length through the fixed form only if a
 * joined row holds at most `fixed_entries` entries, a join whose longest row holds at most `group_entries` (at most 512) through the lane-group form
 * and everything else through the flat form -- a negative value: never, the join goes on to the next form -- and covers `rows_per_launch` output rows
 * (flat form: 16-byte pieces of the output) per launch (tests/test_gpu_join.py: every form, boundary and the multi-launch path on rows of a few
 * entries give the same bits: it is a copy); 0 restores a default */
int fmx_debug_join_limits(int32_t fixed_entries, int32_t group_entries, int64_t rows_per_launch);
/* from now on (sticky, as the join hook) fmx_matrix_bin_columns stages the packed edge table in LDS only if it holds at most `lds_edges` edges over
 * all binned columns (at most 12 288) -- a negative value: never, the table is read from global memory -- and both fmx_matrix_column_quantiles and
 * fmx_matrix_bin_columns launch their per-entry kernels over `chunk_entries` entries, rounded down to a multiple of 4 and at least 4
 * (tests/test_gpu_bins.py: both forms, the boundary and the multi-launch path on a few dozen entries give the same bits); 0 restores a default */
int fmx_debug_bins_limits(int32_t lds_edges, int64_t chunk_entries);
/* from now on (sticky, as the join hook) fmx_matrix_cross never takes its single form if `single` is negative, sends rows of more than
 * `group_entries` (at most 64) source entries to the long form -- a negative value: every row -- and launches its per-row kernels over
 * `rows_per_launch` rows (tests/test_gpu_cross.py: the three forms, the boundary between the group and the long form and the multi-launch path
 * give the same bits); 0 restores a default */
int fmx_debug_cross_limits(int32_t single, int32_t group_entries, int64_t rows_per_launch);
/* from now on (sticky, as the cross hook) fmx_matrix_encode_targets* never takes its single form if `single` is negative and sends rows of more than
 * `group_entries` (at most 64) source entries to the long form -- a negative value: every row, and fmx_target_stats* then never takes its unit form:
 * it sorts --; the per-entry kernels of both calls launch over `chunk_entries` entries and the per-row, per-cell and per-chunk kernels over
 * `rows_per_launch` items (tests/test_gpu_target.py: both forms of the fit, the three of the apply, the boundary between the group and the long form
 * and the multi-launch paths give the same bits); 0 restores a default */
int fmx_debug_target_limits(int32_t single, int32_t group_entries, int64_t chunk_entries, int64_t rows_per_launch);
/* a reader, not a fault: what the detector found on a matrix -- out[0] rows_sorted, [1] unit_values, [2] fixed_row_len, [3] max_row_len, [4] the fields
 * of its layout (0: none) -- (tests/test_gpu_columns.py: a remapped matrix carries the flags of its own entries, not the source's) */
int fmx_debug_matrix_flags(const fmx_matrix* m, int32_t* out /* [5] */);
/* a reader beside it: the layout itself -- the dense prefix, the number of fields C (0: none) and base[0 .. C] (the rest of the array is zeroed)
 * (tests/test_gpu_flags.py: flags and layout of every producer against tests/flags_model.py, which restates them from the exported rows) */
int fmx_debug_matrix_layout(const fmx_matrix* m, int32_t* dense_prefix, int32_t* n_fields, uint32_t* base /* [FMX_MAX_FIELDS + 1] */);
/* a counter, not a fault: how many list-by-list phase-2 launches of this process went to out[0] the general kernel, out[1] the specialised kernel,
 * out[2] the specialised kernel with the row ids one round ahead (tests/test_gpu_cols_lean.py: the cases reach the kernels they are meant for) */
int fmx_debug_cols_launches(int64_t* out);
/* a counter beside it: how many launch pairs of the long-list kernels (fm_cols_long_partial_k + fm_cols_long_finish_k) of this process ran on out[0] the
 * engine's main stream, out[1] its side stream (tests/test_gpu_step_forms.py: the long lists and the side-stream placement are really reached) */
int fmx_debug_long_launches(int64_t* out);
/* and one for the step's first half: how many phase-1 TRAINING launches of this process took out[0] one-wave workgroups with four lane groups per row,
 * out[1] one-wave workgroups with one lane group per row, out[2] 256-thread workgroups on the serial request schedule, out[3] the same with four
 * entries in flight, out[4] the pull kernel (FMX_ROWS_PULL=1), out[5] the flat kernel (FMX_ROWS_FLAT=1); a ranking step counts under the workgroup
 * width and split it ran with (tests/test_gpu_rows_forms.py: every form is reached by the cases that are meant for it) */
int fmx_debug_rows_launches(int64_t* out /* [6] */);
/* the same six slots for the FORWARD-ONLY launches of phase 1 (the TRAIN = false instances: fmx_predict and everything that evaluates a model, the
 * projection behind every ranking call, the ALS q tables), one count per launch of more than zero rows; a call of more than 2^18 rows counts once per
 * slab (tests/test_gpu_forward_forms.py: every form and instance is reached by the calls that are meant for it) */
int fmx_debug_rows_forward_launches(int64_t* out /* [6] */);
/* beside it, and in none of its slots: how many phase-1 launches of this process, training and forward-only, out[0] took the merged form (fm_rows_merged_k:
 * a lane group walks four rows as one column-ordered stream), out[1] met every condition of that form but the stage size -- some 256-row block holds
 * more entries than the workgroup stages -- and took the per-row form (tests/test_gpu_rows_merged.py: every case runs the form it is meant for) */
int fmx_debug_rows_merged_launches(int64_t* out /* [2] */);
/* and for the scheduled form (fm_rows_sched_k: the merged form's walk along a table made once per matrix): out[0] launches that took it, out[1] launches
 * that met its rule and whose tile had a schedule built, but with a block of more steps than the workgroup stages, out[2] schedule builds
 * (tests/test_gpu_rows_sched.py) */
int fmx_debug_rows_sched_launches(int64_t* out /* [3] */);
/* from now on (sticky) schedules are built only for matrices of at most `limit` features instead of 2^30 - 1 -- a schedule word keeps the column in 30
 * bits -- so that the refusal can be tested on a small table; 0 restores the default */
int fmx_debug_rows_sched_id_limit(uint32_t limit);
/* a copy of the schedule of one 256-row block of one tile as the device builder wrote it: *steps its steps (-1: the matrix, or this tile, has no
 * schedule), out[64 * steps] its words, step-major (word g of a step: lane group g's; col | slot << 30, 0xFFFFFFFF a bubble); info, if not NULL:
 * [0] bytes the matrix's schedule takes, [1] microseconds its build took, [2] its policy (0 MERGE, 3 DEAL), [3] 0 (tests/test_gpu_rows_sched.py:
 * the device builder against tests/rows_sched_model.py, word for word) */
/* A DEAL schedule (policy 3) goes through the same hook, header + steps: *steps is still the block's steps T_b, and out[] holds the block's 64 header words
 * (word g = the rows of lane group g, slot s in byte s) FOLLOWED by its 64 * steps words, so cap_words must cover 64 * (steps + 1)
 * (tests/test_gpu_rows_deal.py: the device builder against tests/rows_deal_model.py, header and words) */
int fmx_debug_rows_sched_export(const fmx_matrix* m, int64_t tile, int64_t block, uint32_t* out, int64_t cap_words, int64_t* steps, int64_t* info /* [4] */);
/* the pace of the scheduled form (fm_rows_sched_k, FMX_ROWS_PACE; tests/test_gpu_rows_clock_pace.py).  A counter: how many scheduled-form
 * launches of this process out[0] were paced, out[1] were not */
int fmx_debug_rows_pace_launches(int64_t* out /* [2] */);
/* the look-ahead depth of the scheduled form's walk (fm_rows_sched_k<.., AHEAD>, FMX_ROWS_AHEAD; tests/test_gpu_rows_ahead.py): out[d - 1] = how many
 * scheduled-form launches of this process ran the instance of depth d, d = 1 .. 4; their sum is out[0] of fmx_debug_rows_sched_launches */
int fmx_debug_rows_ahead_launches(int64_t* out /* [4] */);
/* the clock pace (FMX_ROWS_PACE=3, 4; tests/test_gpu_rows_clock_pace.py).  How many clock-paced launches of this process out[0] had a target, out[1] had none
 * (both also count as paced in fmx_debug_rows_pace_launches) */
int fmx_debug_rows_clock_launches(int64_t* out /* [2] */);
/* a copy of replica `replica`'s records, three sets of eight labels: out[2 * (8 * set + label)] = ticks of the 100 MHz counter (low 40 bits) | steps << 40, summed
 * over the label's workgroups by the launch that wrote the set (clock-paced launch n of the engine: set n % 3; it read set (n + 2) % 3 and cleared set (n + 1) % 3);
 * out[.. + 1] = the target planted by the poison hook (0: none) */
int fmx_debug_rows_clock_records_of(fmx_engine* e, int32_t replica, uint64_t* out /* [48] */);
/* from now on (sticky; every replica of a group handle) every record's planted target is `value` (ticks per step, Q8; not 0) before every clock-paced launch of the
 * engine, every such launch takes it in place of gain x ticks / steps whatever came before, and no launch clears a set.  1: every wave finds itself far behind at every
 * check and none sleeps; 0xFFFFFFFF: far ahead, every wave takes the longest sleep at every check.  The same bits either way */
int fmx_debug_rows_clock_poison(fmx_engine* e, uint32_t value);
/* FMX_ROWS_PACE_TRACE=1: the stamps of the engine's last MERGE or DEAL launch, *waves waves (workgroup-major, four per workgroup) of 16 words: [0] = XCC id
 * | steps << 8 | sleeps taken << 32 | the sum of their levels (1, 2, 3) << 48, [1 + t / 16] = s_memrealtime (100 MHz) at step t for t = 0, 16, ..., [1 + (steps + 15) / 16] = behind the last step,
 * [15] = at kernel entry, before the schedule is staged, [14] = behind the epilogue's last store.
 * out may be NULL to ask for *waves alone (profiles/rows_pace_trace.py) */
int fmx_debug_rows_pace_trace(fmx_engine* e, uint64_t* out, int64_t cap_words, int64_t* waves);
#ifdef __cplusplus
}
#endif
#endif /* FMX_TEST_HOOKS_H_ */
