/*
 * fmx.h -- C ABI of the MI355X-native Factorization Machine engine (libfmx.so).
 *
 * This is the drop-in boundary for ONE path of evanwang1990/FMwR: the degree-2 FM forward and the
 * SGD / FTRL-Proximal / TDAP training step, plus the ALS / MCMC learners (V-column sweep, w0 / w loops,
 * probit tables) and the tracker that call the same forward.  It replaces what the Rcpp entry
 * points FM() / FMPredict() do between unmarshalling the R lists and marshalling the result
 * (reference src/FM.cpp:7-173, :177-214), i.e. the seam
 *
 *     learner->init(); learner->learn(data);        src/FM.cpp:145,153   (core/Learner.h:49-51)
 *     fm.predict_batch(..) / fm.predict_prob(..)    src/FM.cpp:199-203   (core/Model.h:106-180)
 *
 * Plain pointers and sizes only; no C++/torch types; nothing throws across the boundary: every call
 * returns an int status (FMX_OK == 0) and fmx_last_error() gives the message (the glue turns a
 * non-zero status into Rcpp::stop(msg), as END_RCPP does for the reference, src/RcppExports.cpp:11,22).
 * The caller keeps ownership of every host pointer it passes; no pointer is retained after return
 * (the reference deep-copies too: util/Smatrix.h:53-60, util/Dvector.h:89-99).
 *
 * A handle is used from one host thread at a time (R is single-threaded; Model::predict is not
 * re-entrant either, core/Model.h:26-27).
 */
#ifndef FMX_H_
#define FMX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMX_OK 0
#define FMX_ERR_INVALID 1  /* bad argument / unsupported configuration */
#define FMX_ERR_HIP 2      /* HIP runtime error (message holds hipGetErrorString) */
#define FMX_ERR_NOGPU 3    /* no usable device: the engine has NO CPU fallback */
#define FMX_ERR_STATE 4    /* call order / handle state */

/* task and solver ids are the reference's (util/Macros.h:11-21) */
#define FMX_TASK_CLASSIFICATION 10
#define FMX_TASK_REGRESSION 20
/* Pairwise ranking (BPR; the reference reserves the id, util/Macros.h:13, and never builds it).  The matrix is a PAIR
 * matrix: an even number of rows, rows 2t and 2t + 1 one preference pair, row 2t the preferred one (fmx_matrix_pairs samples such rows).
 * With d_t = y(2t) - y(2t + 1) the loss is log(1 + exp(-d_t)); labels are ignored.  w0 cancels in every pair and stays bit for bit as set
 * (FTRL's z0 / n0 too).  Only FMX_MODE_MINIBATCH with FMX_SOLVER_SGD or FMX_SOLVER_FTRL; batch_rows even, tile_rows 0 or even.  fmx_train,
 * fmx_step, fmx_grad*, fmx_grad_compact and fmx_num_batches refuse a matrix of odd row count, an odd max_iter / rows_limit and any step whose
 * row range starts on an odd row; fmx_train_tracked and fmx_train_grid refuse ranking engines.  fmx_predict, fmx_topk and fmx_contrib work as
 * for any engine; the natural link is FMX_LINK_NONE.  SGD's L1 rates act as L1 (as for CLASSIFICATION). */
#define FMX_TASK_RANKING 30
#define FMX_SOLVER_MCMC 100  /* util/Macros.h:17; trains through fmx_mcmc_train */
#define FMX_SOLVER_ALS 200
#define FMX_SOLVER_SGD 300
#define FMX_SOLVER_FTRL 500
#define FMX_SOLVER_TDAP 600

/* FMX_MODE_SEQUENTIAL: the reference's algorithm as is -- one example per update, visited in the
 *   reference's order (solver/SGD_Learner.h:86-88), fp64 state.  The parity mode.
 * FMX_MODE_MINIBATCH : synchronous mini-batches of batch_rows examples, fp32 state, gradient sums per
 *   coordinate.  The throughput mode; equals the reference step at batch_rows == 1. */
#define FMX_MODE_SEQUENTIAL 0
#define FMX_MODE_MINIBATCH 1

/* How a mini-batch combines the per-example gradients of one coordinate (c = its occurrences in the batch):
 * FMX_REDUCE_MEAN: one reference step with the MEAN gradient G/c (and one lazy-L2 / L1 / FTRL update) per touched
 *   coordinate per batch -- stable for any batch size with the reference's learning rates; the default.
 * FMX_REDUCE_SUM : the SUM G with c-fold decay -- what processing the c examples one after the other with frozen
 *   gradients does; first-order equal to the reference's pass, but dense coordinates (w0!) overshoot once
 *   learn_rate * c is not small.  Both are the reference's example step at batch_rows == 1. */
#define FMX_REDUCE_MEAN 0
#define FMX_REDUCE_SUM 1

/* output transform of fmx_predict */
#define FMX_LINK_NONE 0      /* raw y_hat: Model::predict_batch, core/Model.h:106-161 */
#define FMX_LINK_LOGISTIC 1  /* 1/(1+exp(-y_hat)): Model::predict_prob, core/Model.h:173-178 */
#define FMX_LINK_CLAMP 2     /* clamp to [min_target, max_target]: src/FM.cpp:202-210 */
#define FMX_LINK_PROBIT 3    /* fast_pnorm(y_hat), the table-driven Phi of MCMC / ALS models: core/Model.h:166-171 */

/* Mirrors the three R control lists (R/fm_control.R:52-66 model.control, R/fm_solver_control.R:91-115
 * SGD.solver / FTRL.solver) as FM() reads them by key (src/FM.cpp:48-63, :97-144). */
typedef struct fmx_config {
  uint32_t struct_size;    /* = sizeof(fmx_config); ABI guard */
  int32_t task;            /* model.control(task)                       */
  int32_t solver;          /* attr(solver, "solver")                    */
  int32_t num_factor;      /* hyper.params$factor.number   (default 2)  */
  int32_t keep_w0;         /* hyper.params$keep.w0                      */
  int32_t keep_w1;         /* hyper.params$keep.w1                      */
  double l2_w0;            /* hyper.params$L2.w0                        */
  double l1_w1, l2_w1;     /* hyper.params$L1.w1, L2.w1                 */
  double l1_v, l2_v;       /* hyper.params$L1.v, L2.v                   */
  double learn_rate;       /* SGD.solver(learn_rate = 0.01)             */
  double alpha_w, alpha_v; /* FTRL.solver(alpha_w = .1, alpha_v = .1)   */
  double beta_w, beta_v;   /* FTRL.solver(beta_w = 1, beta_v = 1)       */
  int32_t random_step;     /* SGD/FTRL.solver(random_step = 1L)         */
  int32_t mode;            /* FMX_MODE_*                                */
  int64_t batch_rows;      /* mini-batch rows per step per GPU          */
  double min_target;       /* learner->min_target, src/FM.cpp:89-96     */
  double max_target;       /* learner->max_target                       */
  int32_t device;          /* HIP device ordinal                        */
  int32_t batch_reduce;    /* FMX_REDUCE_* (mini-batch mode)            */
  double gamma;            /* TDAP.solver(gamma = 1e-4): decay rate (alpha_w, alpha_v shared with FTRL) */
  int64_t tile_rows;       /* 0: default.  A step of batch_rows rows is processed in tiles of at most this many
                              rows (parameters frozen across the tiles, sums accumulated): keeps the per-tile
                              tables cache resident for large batches.  Same result up to the rounding of the
                              partial sums to the state type between tiles (fp32 unless state_fp64).           */
  int32_t state_fp64;      /* mini-batch mode: 0 = fp32 parameter/optimizer tables (default, half the HBM traffic),
                              1 = the fp64 tables of the sequential mode (the reference's precision, core/Model.h:26-42;
                              per-row sums and the exchange buffer become fp64 too).
                              WHICH MODES GUARANTEE north_star's "1e-5 relative on V" against the CPU restatement of the same
                              algorithm: FMX_MODE_SEQUENTIAL (measured <= 1e-11, prediction signs exact) and FMX_MODE_MINIBATCH with
                              state_fp64 = 1 (<= 6e-7 on every case tried, 1 650 fuzz seeds incl. diverging runs).  With fp32 state
                              the bar holds on runs that do not amplify rounding -- all targeted tests and 1 641 of the 1 650 seeds --
                              and NOT in general: on nine seeds the dynamics amplify the fp32 storage rounding beyond 1e-4, two of
                              them short and tame (41 steps, |V| <= 286: w off by 1.8e-4; 10 steps, |V| <= 8.9: V off by 2.9e-4;
                              profiles/r04_fuzz_more.txt; kept as fp64-state regression cases in tests/test_gpu_fuzz.py).  bench.py's
                              headline is the fp32 mode (BASELINE.json configs[1] asks for fp32); the fp64-state figure and its
                              roofline are printed beside it (other_configs."configs[1]_fp64_state").                          */
  int32_t exchange_chunks; /* 0/1: the exchange buffer is one block.  n > 1: it is laid out in n blocks of consecutive
                              features so that a multi-GPU driver can pipeline the exchange (fmx_grad_begin/_chunk/
                              _apply_chunk): the all-reduce of one block overlaps the gradient sums of the next.   */
  int32_t n_gpus;          /* 0/1: one GPU.  N > 1 (FMX_MODE_MINIBATCH): fmx_train shards the matrix's rows over the devices
                              device .. device+N-1, one replica each, and all-reduces the gradient sums between steps with
                              RCCL -- what the reference's `nthreads` (options("FM.threads"), src/FM.cpp:59,97) becomes
                              here.  batch_rows stays "rows per step per GPU".  fmx_get_params / fmx_predict use replica 0. */
  int32_t als_max_levels;  /* ALS / MCMC sweeps: the ORDER of the coordinate steps (history and measurements: DESIGN.md section 6; no further values will be added).
                               0  the exact schedule: levels of row-disjoint features, the reference's index-order Gauss-Seidel reproduced (its numbers).
                                  Deep plans (columns without field structure: thousands of dependent levels) sweep a factor in ONE launch (als_exact_persist_k).
                              L>0 a matrix that needs more than L levels is swept in the reference's own approximate parallel form instead
                                  (solver/MCMC_ALS_Learner.h:200-268: the features of a group step against one snapshot of the residual), under a guard that
                                  falls back to 0 if the residual rises.  For one-column-per-field data both forms coincide.
                              -1  the COLOURED order: every step exact, the features visited in (colour, index) order of a deterministic colouring of the
                                  "share a row" graph -- the reference's numbers on the matrix relabelled in that order (fmx_als_plan_info's level_of gives it),
                                  not on the matrix as given.  A matrix whose exact schedule is shallow (<= ~128 levels) keeps those levels as its colours:
                                  -1 is then bit for bit 0.
                              -2  the coloured order nested FEATURE-MAJOR: all k factors of a feature stepped together, coordinates in (colour, feature, factor)
                                  order (the reference nests factor outer); every step exact.  Applies to plans of light lists of at most 1 024 rows whose rows'
                                  lines fit the LDS at this k (577 rows at k = 17..32, 296 at k <= 64); other plans run as -1 (fmx_als_plan_info: kind 2).        */
  int32_t seq_reassociate; /* FMX_MODE_SEQUENTIAL, SGD (L2 or cumulative L1) on rows of at most 32 (64 at k <= 32) ascending columns.  0 (default): the forward's sum in
                              the reference's association, y_hat = ((w0 + w_j1 x_j1) + ...) + 0.5 (s_1^2 - q_1) + ... (core/Model.h:77-100) -- the oracle's
                              bits up to the device exp().  1: the same formula summed as w0 + (row part), the row part a fixed tree; only w0 then
                              chains one example to the next (solver/SGD_Learner.h:100-112).  The reference's algorithm, visiting order and
                              precision; the last bits of y_hat differ (<= 1e-10 on V against the oracle, prediction signs exact on every parity
                              case; the same bits from run to run).  4.0 M examples/s against 1.65 M at configs[1]'s shape.  FTRL, TDAP and other row
                              shapes ignore the flag (they run the bitwise kernels).                                                              */
  int32_t gpus_share_device; /* 1: all N replicas live on `device` and exchange through a device kernel instead of RCCL
                              (rehearsals and tests on a one-GPU box; same sums, same order of ranks)                  */
} fmx_config;

typedef struct fmx_engine fmx_engine; /* parameters + optimizer state on one GPU */
typedef struct fmx_matrix fmx_matrix; /* a device-resident fm.matrix (CSR + labels [+ per-batch CSC]) */

/* Message of the last failing call on this thread ("" if none). */
const char* fmx_last_error(void);

/* Number of HIP devices this process sees (what cfg.n_gpus may count up to); FMX_ERR_NOGPU without one. */
int fmx_device_count(int32_t* count);

/* Fill *cfg with the reference's defaults (R/fm_control.R:52-66, R/fm_solver_control.R:91-115). */
int fmx_config_default(fmx_config* cfg);

/* ---- engine: replaces `Model fm; fm.init(); learner = new XXX_Learner(); learner->init()`
 *      (src/FM.cpp:47-64, :78-145).  Parameters start at w0 = 0, w = 0, V = 0: V0 is an INPUT
 *      (fmx_set_params), because the reference draws it from R's RNG (util/Dmatrix.h:143-146). */
int fmx_engine_create(const fmx_config* cfg, uint64_t num_features, fmx_engine** out);
int fmx_engine_destroy(fmx_engine* e);

/* w: [p] or NULL (zeros); v: the R NumericMatrix k x p, column-major, i.e. v[f + j*k] (what
 * Model::save_model / load_model exchange, core/Model.h:182-227) or NULL (zeros).
 * Warm start of fm.update(): src/FM.cpp:66-72.  Optimizer state is reset, as learner->init() does. */
int fmx_set_params(fmx_engine* e, double w0, const double* w, const double* v);
int fmx_get_params(fmx_engine* e, double* w0, double* w, double* v);

/* Sparse access to the parameters (p = 33 M, k = 32 is 8.4 GB of doubles: a full fmx_get_params is the wrong tool there):
 * rows of the features ids[0..n): w -> w[i], V -> v[f + i*k] (the same k x n column-major shape as fmx_set_params).
 * fmx_set_rows leaves every other row and the optimizer state alone; a NULL w or v keeps that part of the rows. */
int fmx_get_rows(fmx_engine* e, const uint32_t* ids, int64_t n, double* w, double* v);
int fmx_set_rows(fmx_engine* e, const uint32_t* ids, int64_t n, const double* w, const double* v);
/* w0 = 0, w = 0, V ~ N(mean, stdev) drawn ON THE DEVICE (Philox4x32-10 keyed by seed, feature and factor pair; Box-Muller):
 * the shape of Model::init (core/Model.h:63-72) for synthetic workloads too large to stage through the host.  It is not R's
 * generator: runs that must reproduce the reference draw V0 in the glue and pass it to fmx_set_params. */
int fmx_init_normal(fmx_engine* e, uint64_t seed, double mean, double stdev);

/* ---- checkpoint (the reference keeps a model only as an R list and drops the optimizer state on fm.update):
 * parameters AND optimizer state (SGD-L1 q/u, FTRL z/n, TDAP u/nu/delta/h/z) to a file and back.  The loading engine must
 * have the same feature count, factor count, solver kind and mode.  Format: 64-byte header ("FMX1", version, shape),
 * the device scalars, then the tables as stored on the device (little endian). */
int fmx_engine_save(fmx_engine* e, const char* path);
int fmx_engine_load(fmx_engine* e, const char* path);

/* ---- data: replaces `SMatrix<float> m; m.assign(X); DVector<float> tg; tg.assign(target)`
 *      (src/FM.cpp:31-44).  All inputs are host pointers; the matrix is copied to HBM. */

/* R's fm.matrix layout (R/fm_matrix.R:25-34): value f64[nnz], col_idx i32[nnz] 0-based, row_size i32[n];
 * narrowed to f32 / u32 like util/Smatrix.h:44-61.  labels may be NULL (prediction). */
int fmx_matrix_from_rlist(int device, int64_t n, uint32_t p, int64_t nnz, const double* value,
                          const int32_t* col_idx, const int32_t* row_size, const double* labels,
                          fmx_matrix** out);
/* A dgCMatrix as it lies in R (Matrix package slots: x f64[nnz], i i32[nnz] 0-based ROW indices, p i32[ncol + 1] column pointers, Dim = (nrow, ncol)).
 * R/fm_matrix.R:26-33 transposes it on the host first (`Matrix::t(data)`, then the list above); here the slots go over as they are and the transposition
 * is a device sort by row (stable: the columns of a row come out ascending).  Row indices out of range, decreasing pointers and a pointer total other than nnz
 * are refused; nrow and nnz must be below 2^32 (one sort over all entries).  labels may be NULL. */
int fmx_matrix_from_dgc(int device, int64_t nrow, uint32_t ncol, int64_t nnz, const double* x, const int32_t* i, const int32_t* p, const double* labels,
                        fmx_matrix** out);
/* Plain CSR: row_ptr i64[n+1], col u32[nnz], val f32[nnz], y f32[n] or NULL. */
int fmx_matrix_from_csr(int device, int64_t n, uint32_t p, const int64_t* row_ptr, const uint32_t* col,
                        const float* val, const float* y, fmx_matrix** out);
/* Synthetic workload generated on the device: rows [row_offset, row_offset+n) of a
 * stream keyed by (seed, global row id): nnz_per_row stratified-uniform sorted distinct columns, value 1,
 * label +-1.  Shard-independent: a rank asks for its own row range. */
int fmx_matrix_synthetic(int device, int64_t n, uint32_t p, int32_t nnz_per_row, uint64_t seed,
                         int64_t row_offset, fmx_matrix** out);
/* Criteo-shaped synthetic rows (BASELINE.json configs[3]): n_dense always-present features (ids
 * 0..n_dense-1, value in [0,1)) followed by one one-hot feature from each of n_fields categorical fields (<= 64); field f owns
 * the next field_vocab[f] ids, the id inside a field is floor(vocab * u^skew) with u uniform (skew = 1: uniform; larger: a
 * power-law head, as in click logs).  Number of features = n_dense + sum(field_vocab); every row holds n_dense + n_fields
 * entries, ascending.  Keyed by (seed, global row id) like fmx_matrix_synthetic. */
typedef struct fmx_fields_spec {
  uint32_t struct_size;  /* = sizeof(fmx_fields_spec) */
  int32_t n_dense;
  int32_t n_fields;
  int32_t reserved;
  const uint32_t* field_vocab; /* [n_fields] */
  double skew;
  uint64_t seed;
} fmx_fields_spec;
int fmx_matrix_synthetic_fields(int device, int64_t n, const fmx_fields_spec* spec, int64_t row_offset, fmx_matrix** out);
/* Field-structured rows -- what fm.matrix makes of a data frame whose factor columns are one-hot encoded (R/fm_matrix.R: model.matrix keeps a
 * factor's dummy columns together): every row holds the n_dense always-present columns 0 .. n_dense-1 (any values), then exactly ONE id of each of
 * n_fields (<= 64) categorical fields, field c's ids lying in [field_base[c], field_base[c + 1]) with value 1 (field_base[0] = n_dense,
 * field_base[n_fields] = the feature count).  The layout is checked on the device (FMX_ERR_INVALID if a row differs); the inverted index of a step is
 * then built field by field -- a column's ids inside its field are sorted on ceil(log2 vocabulary) bits, the dense columns are not sorted at all --
 * instead of by one sort of all column ids: same plan, same results, about twice the planning rate.  The generators set it themselves,
 * and every uploaded matrix is looked at for it (rows of one length whose entry positions have disjoint ascending column ranges, values 1 outside a
 * leading run of always-present columns): this call is for a caller who knows the vocabularies to be wider than the ids that occur, or wants the check. */
int fmx_matrix_set_fields(fmx_matrix* m, int32_t n_dense, int32_t n_fields, const uint32_t* field_base);
/* Replace the labels of a device-resident matrix (y: f32[n] on the host): e.g. labels planted from a known model. */
int fmx_matrix_set_labels(fmx_matrix* m, const float* y);
/* SURVEY 8(d)'s other column laws (fmx_matrix_synthetic draws one column per stratum of [0, p)): nnz_per_row (<= 64) columns
 * i.i.d. over [0, p), sorted inside the row, repeats bumped to the next id.  law = FMX_COLUMNS_UNIFORM, or FMX_COLUMNS_ZIPF with
 * exponent `zipf_s` > 1 (1.05: a few features occur in most rows). */
#define FMX_COLUMNS_UNIFORM 1
#define FMX_COLUMNS_ZIPF 2
int fmx_matrix_synthetic_iid(int device, int64_t n, uint32_t p, int32_t nnz_per_row, uint64_t seed, int64_t row_offset, int32_t law,
                             double zipf_s, fmx_matrix** out);
/* SURVEY 8(d)'s ragged variant: row lengths Poisson(mean_nnz) clipped to [min_nnz, max_nnz] (the survey's "Poisson(30) clipped to [1, 64]"), columns
 * i.i.d. uniform over [0, p), sorted inside the row, repeats bumped; values 1, labels +-1; shard independent (keyed by the global row). */
int fmx_matrix_synthetic_ragged(int device, int64_t n, uint32_t p, double mean_nnz, int32_t min_nnz, int32_t max_nnz, uint64_t seed, int64_t row_offset,
                                fmx_matrix** out);
/* SURVEY 8(d)'s value variant: every stored value of a resident matrix redrawn uniform in (0, 1), keyed by (seed, global row = row_offset + r, entry) like the
 * generators above (a shard draws what the whole matrix would).  The matrix stops being one-hot: its plans are dropped and the kernels read the value arrays
 * from here on (util/Smatrix.h:44-61: the reference's values are real floats). */
int fmx_matrix_synthetic_values(fmx_matrix* m, uint64_t seed, int64_t row_offset);
int fmx_matrix_destroy(fmx_matrix* m);
int fmx_matrix_info(const fmx_matrix* m, int64_t* n, uint32_t* p, int64_t* nnz);
/* Copy rows [r0, r1) back to the host (row_ptr is rebased to 0); any pointer may be NULL. */
int fmx_matrix_export(const fmx_matrix* m, int64_t r0, int64_t r1, int64_t* row_ptr, uint32_t* col,
                      float* val, float* y);

/* ---- preprocessing on the device
 * SMatrix::scales (util/Smatrix.h:98-135, called at src/FM.cpp:36-38): z-score the stored entries of the listed columns
 * (ascending 0-based ids, as R passes `normalize - 1`) in place; mean/std: f64[p] outputs = Scales$mean / Scales$std. */
int fmx_matrix_scales(fmx_matrix* m, const int32_t* norm_columns, int64_t n_norm, double* mean, double* std);
/* SMatrix::normalize (util/Smatrix.h:137-153, src/FM.cpp:183-186): apply a fitted model's Scales to new data. */
int fmx_matrix_normalize(fmx_matrix* m, const double* mean, const double* std);

/* ---- the hot path */

/* Model::predict_batch / predict_prob (+ clamp) for every row; out: f64[n] on the host. */
int fmx_predict(fmx_engine* e, const fmx_matrix* m, double* out, int link);

/* Learner::learn(data): run max_iter EXAMPLES (the reference counts examples, solver/SGD_Learner.h:168-173).
 * SEQUENTIAL: rows visited as the reference visits them (libc rand() strides when random_step > 1).
 * MINIBATCH : consecutive batches of batch_rows rows, wrapping at the end of the matrix.
 * examples_done (may be NULL) receives the number actually processed. */
int fmx_train(fmx_engine* e, fmx_matrix* m, int64_t max_iter, int64_t* examples_done);
/* A GRID of models trained side by side in the reference's own algorithm (SGD_Learner::learn / FTRL_Learner::learn, one update per example in the reference's
 * visiting order).  NO COUNTERPART IN THE REFERENCE: its R/fm_select.R:22-66 picks the best SNAPSHOT of one fit's trace, it does not train a grid; this entry is
 * what a user's own loop of fm.train() calls over hyper-parameters becomes -- ONE launch per 65 536 examples with one workgroup per model (the reference-order
 * learner is a single workgroup bound by its scalar chain, DESIGN.md section 4: one model cannot use more of the chip, 64 or 256 models can).  An extension, not
 * a row of SURVEY section 8.  Every engine keeps its own parameters, optimizer state and hyper-parameters (learn_rate, regularisers, alpha / beta ...);
 * the engines share the feature count, factor.number, solver, task, device and random_step = 1 (ONE visiting order), and the matrix.  Each model's result is bit for
 * bit what fmx_train(engine, m, max_iter) alone gives it.  SGD (L1 / L2), FTRL and TDAP (the reference's default solver); rows of at most 32 entries (64 at k <= 32) with
 * ascending columns -- the shapes the windowed learners take. */
int fmx_train_grid(fmx_engine* const* engines, int32_t n_engines, fmx_matrix* m, int64_t max_iter, int64_t* examples_done);
/* Same, but with an explicit visiting order (row ids, SEQUENTIAL mode only). */
int fmx_train_order(fmx_engine* e, fmx_matrix* m, const int64_t* order, int64_t count);

/* Streamed training (BASELINE.json configs[3]: 4e9 rows x 33 M features do not fit the reference's uint32 offsets,
 * util/Smatrix.h:10-17, nor any memory): the rows [row_offset, row_offset + total_rows) of a synthetic stream are produced
 * step by step -- batch_rows rows are generated and their inverted index is built two steps ahead of the step that trains on
 * them (on a second stream beside the running step; FMX_STREAM_OVERLAP=0: behind it on the engine's stream -- DESIGN.md 6.5, 6.7); each step is trained
 * on once and dropped.  spec == NULL: the uniform generator of fmx_matrix_synthetic with nnz_per_row entries; otherwise the
 * Criteo-shaped one (nnz_per_row ignored).  Needs batch_rows <= the tile size (one tile per step).  ingest_wait_s (may be
 * NULL): host seconds spent waiting for a tile's counts.  On a cfg.n_gpus > 1 handle replica r streams rows
 * [r T / N, (r + 1) T / N) of the range on its own device and the replicas exchange per step (records of the occurring features
 * for sparse tiles, the dense buffer otherwise). */
int fmx_train_stream(fmx_engine* e, const fmx_fields_spec* spec, int32_t nnz_per_row, uint64_t seed, int64_t row_offset,
                     int64_t total_rows, int64_t* examples_done, double* ingest_wait_s);

/* The same stream step by step, for a driver that exchanges between the gradient sums and the update of every step (one process
 * per GPU: fmwr_amd/distributed.py; rank r opens rows [r T / N, (r + 1) T / N) -- the generators are keyed by the global row id).
 *   fmx_source_open   generates and plans the first two steps (enqueued on the engine's stream)
 *   fmx_source_next   hands out the next step as a matrix of ONE batch (step index 0 for fmx_step / fmx_grad / fmx_grad_compact /
 *                     fmx_owner_info ...), valid until the call after the next one; waits (host) only for that tile's counts, and
 *                     enqueues the generation and planning of the step after the next.  *step_matrix == NULL at the end.
 *   fmx_source_close  waits for the engine's stream and frees the stream; ingest_wait_s as above. */
typedef struct fmx_source fmx_source;
int fmx_source_open(fmx_engine* e, const fmx_fields_spec* spec, int32_t nnz_per_row, uint64_t seed, int64_t row_offset, int64_t total_rows,
                    fmx_source** out);
int fmx_source_next(fmx_source* s, fmx_matrix** step_matrix, int64_t* rows);
int fmx_source_close(fmx_source* s, double* ingest_wait_s);

/* ---- tracker (core/Tracker.h, the evaluation blocks of solver/SGD_Learner.h:140-176 and FTRL_Learner.h:118-154) */

/* metric ids are the reference's (util/Macros.h:24-29); evaluates() picks by task (core/Evaluation.h:20-41) */
#define FMX_EVAL_LL 0
#define FMX_EVAL_AUC 111
#define FMX_EVAL_ACC 222
#define FMX_EVAL_RMSE 333
#define FMX_EVAL_MSE 444
#define FMX_EVAL_MAE 555
/* ranking engines only (and only these there), on a pair matrix, from the raw scores: the mean over pairs of [d > 0] + 1/2 [d == 0], and the
 * mean BPR loss log(1 + exp(-d)) computed stably for any d.  Fixed-order reductions: the same bits every call. */
#define FMX_EVAL_PAIR_ACC 666
#define FMX_EVAL_BPR 777

/* track.control() (R/fm_track_control.R:20-26) as FM() plumbs it (src/FM.cpp:99-103) */
typedef struct fmx_track_config {
  uint32_t struct_size;  /* = sizeof(fmx_track_config) */
  int32_t metric;        /* FMX_EVAL_*: evaluate.metric */
  int64_t step_size;     /* evaluate + snapshot every step_size examples (> 0) */
  double convergence;    /* stop after 3 consecutive relative changes <= this (conv_condition) */
  int32_t keep_params;   /* 1: snapshot (w0, w, V) at every record like Tracker::record (core/Tracker.h:54-63); 0: metrics only */
  int32_t reserved;
} fmx_track_config;

/* Metric of the engine's current parameters on a data set: forward + link (probability for CLASSIFICATION, clamp to
 * the target range for REGRESSION) + evaluates().  What Tracker::report computes per snapshot (core/Tracker.h:70-94).
 * It keeps the reference's definitions, quirks included; the standard AUC, log loss and error metrics, also per row group, are fmx_metrics. */
int fmx_evaluate(fmx_engine* e, const fmx_matrix* m, int metric, double* out);

/* Learner::learn with the tracker on: as fmx_train, plus an evaluation on the training matrix after example 0,
 * step_size, 2*step_size, ... and after the last one; stops early when converged.  The trace stays in the engine
 * until the next fmx_train_tracked / fmx_set_params.  cfg.n_gpus > 1 (mini-batch learners): the record rule is applied to the
 * example indices a GLOBAL step covers (n_gpus * batch_rows of them) and the model is looked at on replica 0, over all of m. */
int fmx_train_tracked(fmx_engine* e, fmx_matrix* m, int64_t max_iter, const fmx_track_config* track,
                      int64_t* examples_done, int32_t* convergent);
int fmx_trace_size(fmx_engine* e, int64_t* n_records);
/* iters: the example index of each record (Trace$trace[[1]]), evals: Trace$evaluation.train */
int fmx_trace_get(fmx_engine* e, int64_t* iters, double* evals);
/* snapshot `record` (needs keep_params): same layouts as fmx_get_params */
int fmx_trace_params(fmx_engine* e, int64_t record, double* w0, double* w, double* v);

/* ---- step-level interface (what fmx_train loops over; used by bench.py and the multi-GPU driver).
 * All of these enqueue on the engine's stream and return without waiting; fmx_sync waits. */

/* number of steps (batches of batch_rows rows) the matrix splits into (builds the per-tile CSC on first use) */
int fmx_num_batches(fmx_engine* e, fmx_matrix* m, int64_t* n_batches);
/* one full mini-batch step on this GPU: forward -> gradient sums -> update, rows of batch `batch`
 * (rows_limit > 0 truncates the batch to its first rows_limit rows). */
int fmx_step(fmx_engine* e, fmx_matrix* m, int64_t batch, int64_t rows_limit);
/* multi-GPU split of the same step: local gradient sums into the exchange buffer ... */
int fmx_grad(fmx_engine* e, fmx_matrix* m, int64_t batch, int64_t rows_limit);
/* ... device pointer / element count of that buffer, for an in-place all-reduce(sum); elements are fp32, or fp64
 * with cfg.state_fp64 (fmx_grad_elem_bytes says which: 4 or 8) ... */
int fmx_grad_buffer(fmx_engine* e, void** dev_ptr, int64_t* n_floats);
int fmx_grad_elem_bytes(const fmx_engine* e, int32_t* bytes);
/* Pipelined form of the same split (cfg.exchange_chunks > 1).  The buffer is n_chunks blocks of chunk_elems elements,
 * block c holding the sums of features [c*chunk_features, (c+1)*chunk_features), followed at tail_offset by 4 elements
 * {sum of multipliers, sum of their squares, rows / 4096, rows % 4096} (two parts so that an fp32 sum over the ranks stays exact):
 *   fmx_grad_begin          forward of the whole step (all its tiles), writes the tail        -> all-reduce the tail
 *   fmx_grad_chunk(c)       gradient sums of block c over all tiles                            -> all-reduce block c (async)
 *   fmx_apply_chunk(c,..)   update of block c's features from the reduced block; `last` != 0 on the final call of the
 *                           step also applies the w0 / penalty-level update (every block reads the step's start scalars).
 * Results are identical to fmx_grad + fmx_apply (same sums in the same order). */
int fmx_grad_layout(fmx_engine* e, int64_t* n_chunks, int64_t* chunk_features, int64_t* chunk_elems, int64_t* tail_offset);
int fmx_grad_begin(fmx_engine* e, fmx_matrix* m, int64_t batch, int64_t rows_limit);
int fmx_grad_chunk(fmx_engine* e, fmx_matrix* m, int64_t chunk);
int fmx_apply_chunk(fmx_engine* e, int64_t chunk, int64_t global_rows, int32_t last);
/* ... and the update from the (reduced) buffer; global_rows = rows of the whole global batch, or <= 0 to take the
 * count that travelled in the buffer's tail (each rank's fmx_grad wrote its own row count there; the all-reduce summed them). */
int fmx_apply(fmx_engine* e, int64_t global_rows);
/* ---- compact exchange (SURVEY 8(e) "collective sizing", BASELINE.json configs[3]: p = 33 M, k = 32 -> a dense buffer of 4.5 GB
 * per step).  When a step is one tile holding fewer entries than there are features (fmx_compact_info says `usable`), the
 * gradient sums of the features that OCCUR in the step are published as records instead:
 *     record = G[kp] | (Q[kp]: FTRL with FMX_REDUCE_SUM) | Gw | Qw | cnt | feature id      (record_elems elements, fp32 or fp64)
 * in ascending feature order, plus a 4-element tail {sum of multipliers, sum of squares, rows / 4096, rows % 4096}.
 *   fmx_grad_compact      forward + gradient sums of the step -> this rank's records and tail (enqueued)
 *   fmx_compact_records   device pointers of the records / the tail, and the record count (known on the host from ingest)
 *   -- the driver all-reduces the tail (sum) and all-gathers the records (padded to the largest count) --
 *   fmx_apply_compact     the gathered parts (part r: counts[r] records starting at record r * stride_records) are merged by
 *                         feature id, a feature's parts added in rank order, and the update is applied once per feature.
 * Two ranks give bitwise the result of the dense fmx_grad / all-reduce / fmx_apply step (tests/test_gpu_distributed.py). */
int fmx_compact_info(fmx_engine* e, fmx_matrix* m, int64_t* record_elems, int64_t* capacity, int32_t* usable);
int fmx_compact_count(fmx_engine* e, fmx_matrix* m, int64_t batch, int64_t* n_records); /* records step `batch` publishes */
int fmx_compact_reserve(fmx_engine* e, int64_t capacity); /* room for `capacity` records (>= every rank's own capacity) */
int fmx_grad_compact(fmx_engine* e, fmx_matrix* m, int64_t batch, int64_t rows_limit);
int fmx_compact_records(fmx_engine* e, void** dev_records, int64_t* n_records, void** dev_tail);
int fmx_apply_compact(fmx_engine* e, const void* dev_records, const int64_t* counts, int32_t n_parts, int64_t stride_records,
                      int64_t global_rows);
/* The parts of fmx_apply_compact at explicit positions: part r holds counts[r] records starting at record starts[r] of the buffer
 * (what an all-to-all with uneven splits leaves behind). */
int fmx_apply_compact_parts(fmx_engine* e, const void* dev_records, const int64_t* counts, const int64_t* starts, int32_t n_parts,
                            int64_t global_rows);

/* ---- owner-sharded exchange (SURVEY 8(e) option (ii), BASELINE.json configs[3] on N GPUs).  Feature j BELONGS to rank j mod N: the
 * owner holds its current (V row, w) and its optimizer state; the other ranks hold copies that are refreshed when a step needs
 * them.  Per step, on every rank (the collectives are the driver's: fmwr_amd/distributed.py):
 *     ids    = the step's occurring features in owner-major order, counts[o] of them owned by rank o     (fmx_owner_info)
 *     pull   : all-to-all of the ids to their owners; an owner packs the rows asked for (fmx_rows_pack), all-to-all back,
 *              the asking rank stores them (fmx_rows_unpack): every row the step reads is the owner's current one
 *     sums   : fmx_grad_compact -- with fmx_owner_configure(N > 1) its records come out in the same owner-major order, so the
 *              part for owner o is one contiguous slice
 *     push   : all-to-all of the record slices to their owners (+ all-reduce of the 4-element tail)
 *     update : fmx_apply_compact_parts on the received parts: a feature's parts are added in rank order and the update is applied
 *              once, by its owner.
 * Per rank and step this moves about 2 x (N-1)/N x records instead of the all-gather's N x records, and equals it bit for bit
 * (the same additions in the same order).  w0 and the other scalars stay replicated (the tail is all-reduced).  After training,
 * a rank's copy of a feature it does not own is as old as the last step of its own that used it. */
int fmx_owner_configure(fmx_engine* e, int32_t n_owners, int32_t rank);
/* counts: i64[n_owners] records of step `batch` per owner; *dev_ids: u32[sum(counts)] the ids in owner-major order (device; valid
 * until the matrix's plans change, for a streamed step until the call after the next fmx_source_next) */
int fmx_owner_info(fmx_engine* e, fmx_matrix* m, int64_t batch, int64_t* counts, void** dev_ids);
/* (V row | w 0 0 0) of n features in the state's element type: row_elems = kp + 4 elements per feature (device buffers) */
int fmx_rows_pack(fmx_engine* e, const void* dev_ids_u32, int64_t n, void* dev_rows, int64_t* row_elems);
int fmx_rows_unpack(fmx_engine* e, const void* dev_ids_u32, int64_t n, const void* dev_rows);

int fmx_sync(fmx_engine* e);
/* the hipStream_t the engine launches on (as void*), so a caller can order its own work after it */
int fmx_stream(fmx_engine* e, void** stream);
/* device-side forward: y_hat (f64) for rows [r0, r1) into a device buffer the caller owns */
int fmx_predict_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, void* dev_out_f64, int link);

/* ---- recommendation: the K best item rows for every context row under the FM score of the concatenated row c (+) i
 *      (the entries of context row c followed by those of item row i), computed without forming c (+) i:
 *          score(c, i) = (base_c + base_i) + <s_c, s_i>,   s_r = sum_{j in r} x_j v_j,
 *      base_c the forward of row c (w0 included, keep_w0 / keep_w1 honoured), base_i the forward of row i without w0, the dot a fixed-order
 *      sum over the factors in the state precision (fp64 tables: fp64; fp32 tables: fp32 s and an fp32 dot).  A pair's score is the same
 *      bits however contexts and items are tiled, sliced or batched.
 * Order: a higher raw score first; equal scores by the lower item index; NaN below every number -- strict and total, so the top-K set is
 * unique.  The link (FMX_LINK_*) is applied to the K returned values only.  context and items must have p == the engine's p and live on its
 * device; items has fewer than 2^31 - 1 rows.  exclude: NULL, or a matrix with n == context rows and p == item rows whose column ids of row c
 * are items context c never receives (values ignored; duplicates and any order accepted).  1 <= top_k <= 1024; slots beyond a context's
 * eligible items hold index -1 and score NaN.  Multi-GPU engines run on their primary device. */
/* out_index i64[n_ctx][top_k], out_score f64[n_ctx][top_k]: host, row-major */
int fmx_topk(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* exclude,
             int32_t top_k, int link, int64_t* out_index, double* out_score);
/* the same for context rows [r0, r1), outputs [r1 - r0][top_k] on the device (mirrors fmx_predict_device) */
int fmx_topk_device(fmx_engine* e, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items,
                    const fmx_matrix* exclude, int32_t top_k, int link, void* dev_index_i64, void* dev_score_f64);

/* ---- negative sampling for FMX_TASK_RANKING: a pair matrix built on the device.
 *      positives: n == context rows, p == item rows; the column ids of row c are the items context c prefers (values ignored, any order,
 *      duplicates count once).  For every distinct positive i of context c, n_neg negatives j are drawn EXACTLY uniformly from the items
 *      that are not positives of c (no rejection: r = mulhi(hash(seed, epoch, pair), items - |P_c|), and j is the r-th non-positive, found
 *      by a binary search on P[idx] - idx over c's sorted positives), then the pairs are shuffled by a stable sort on a 64-bit hash key.
 *      Output rows 2t = context(c) entries followed by item(i) entries, 2t + 1 = context(c) entries followed by item(j) entries (the
 *      concatenation of fmx_topk); 2 * n_neg * (distinct positives) rows, labels 1, on the context matrix's device, p = context p.  Contexts
 *      without positives give no pair; a context whose positives cover every item is FMX_ERR_INVALID.  Deterministic: the same inputs, seed
 *      and epoch give the same bits; another epoch gives other negatives and another order.  context and items must share p and a device. */
int fmx_matrix_pairs(const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* positives, int32_t n_neg, uint64_t seed, int64_t epoch,
                     fmx_matrix** out);
/* Hard negatives (dynamic negative sampling): the pair matrix of fmx_matrix_pairs(context, items, positives, n_neg, seed,
 * epoch) -- the same rows, row order, positives, shuffle and flags -- in which only the negative item of a pair may differ.  Pair t (distinct
 * positive t / n_neg, draw t % n_neg) draws n_cand candidates with replacement from c's non-positives by the uniform sampler's rule on hash
 * stream 0 (candidate 0: exactly fmx_matrix_pairs' negative) and streams q + 1 (candidate q >= 1); stream 1 stays the shuffle key.  Its
 * negative is the candidate that comes first in fmx_topk's order under e's parameters at the time of the call (a higher raw score first,
 * equal scores by the lower item index, NaN below every number), the raw score formed bit for bit as fmx_topk forms it.  So n_cand = 1 gives
 * fmx_matrix_pairs' bits, and no chosen negative comes after the uniform one in that order.  1 <= n_cand <= 64.  e: any engine fmx_topk
 * accepts (p == context p == items p, on the matrices' device, fmx_topk's factor limit); its parameters and optimiser state are not
 * modified; multi-GPU engines read their primary replica.  Every refusal (those of fmx_matrix_pairs and fmx_topk, a NULL engine, n_cand
 * out of range) is FMX_ERR_INVALID with *out cleared, before any launch; a context whose positives cover every item is refused as
 * fmx_matrix_pairs refuses it, before the negatives are drawn. */
int fmx_matrix_pairs_hard(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* positives, int32_t n_neg,
                          int32_t n_cand, uint64_t seed, int64_t epoch, fmx_matrix** out);

/* ---- contributions: the exact Shapley value of every stored entry of a row for the raw score (link NONE), the empty row as baseline:
 *      phi_e = keep_w1 x_e w_c(e) + 1/2 x_e sum_f v_c(e),f (s_f - x_e v_c(e),f),  s = sum_e x_e v_c(e);  keep_w0 w0 + sum_e phi_e = y_hat.
 * The players are the stored entries (a column stored twice in a row is two players), in the matrix's entry order.  Arithmetic is fp64 for
 * either table type; a row's values depend on that row alone (not on the range or the chunking of a call), and a row of one entry gets
 * exactly x w (0 with keep_w1 = 0).  Multi-GPU engines read their primary replica. */
int fmx_contrib(fmx_engine* e, const fmx_matrix* m, double* out /* f64[nnz], in the matrix's entry order */);
int fmx_contrib_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1,
                       void* dev_out_f64 /* f64[row_ptr[r1] - row_ptr[r0]]: entry row_ptr[r0] at index 0 */);
/* per feature j over every row of m: sum[j] = sum of phi_e, abs_sum[j] = sum of |phi_e|, count[j] = entries with c(e) = j.  fp64 sums in a
 * fixed order (no floating-point atomics): the same matrix and engine give the same bits every call. */
int fmx_contrib_summary(fmx_engine* e, const fmx_matrix* m, double* sum /* [p] */, double* abs_sum /* [p] */,
                        int64_t* count /* [p] or NULL */);

/* ---- pairwise interactions: the pair terms fmx_contrib splits in half.  A row has stored entries e_0 .. e_{m-1} in the matrix's entry order
 *      (column c(e), value x_e; a column stored twice is two players, as in fmx_contrib).  With the scaled factor row
 *          t_e[f] = (double) v[c(e)][f] * (double) x_e          (one rounded fp64 product; exact for fp32 tables)
 *      the pair value of entries a < b is
 *          I(a, b) = ((..(0.0 + t_a[0] * t_b[0]) + t_a[1] * t_b[1]) ..) + t_a[k-1] * t_b[k-1]
 *      one fp64 accumulator starting at +0.0, f ascending over the k factors, every product rounded, then every sum (no fma), for both table
 *      types; k = 0 gives +0.0 for every pair; a NaN value is reported as the canonical quiet NaN (0x7ff8000000000000).  I(a, b) is the
 *      Shapley interaction index of the two entries for the raw score, the empty row as baseline, and up to rounding
 *          keep_w0 w0 + sum_e keep_w1 x_e w_c(e) + sum_{a<b} I(a, b) = y_hat,     sum_{b != a} I(a, b) = 2 (phi_a - keep_w1 x_a w_c(a)).
 *      Order of a row's pairs ("strongest first"): a larger |I| first (-0 = +0); equal magnitudes, whatever their signs, by the lower a, then
 *      the lower b; a NaN value after every number, in (a, b) order among NaNs.  The order is strict and total: the result is unique.
 *      Guarantees: a row's result is a function of that row and the parameters alone (never of the range, the chunking or the kernel form a
 *      call takes); the result for a smaller top_m is a prefix of the result for a larger one; nothing is ordered or summed by atomics.
 *      1 <= top_m <= 64; any row length and factor count; every engine fmx_contrib accepts (both table precisions, the w-in-row layout,
 *      every task, multi-GPU engines read their primary replica); parameters and optimiser state are never modified.  Every refusal (a NULL
 *      engine, matrix or required output, a p or device mismatch, top_m or n_groups out of range, a group id >= n_groups, NULL groups with
 *      p > n_groups, a bad row range) is FMX_ERR_INVALID before any launch and before any output is written; n == 0 or an empty range is
 *      FMX_OK with nothing written. */
/* per row the top_m strongest pairs: out_a / out_b i64[n][top_m] = the two entries' 0-based positions INSIDE the row (a < b),
   out_value f64[n][top_m] = I(a, b), bits as defined; slots beyond the row's m(m-1)/2 pairs hold -1 / -1 / NaN */
int fmx_interactions(fmx_engine* e, const fmx_matrix* m, int32_t top_m, int64_t* out_a, int64_t* out_b, double* out_value);
/* rows [r0, r1), device outputs [r1 - r0][top_m] (mirrors fmx_contrib_device) */
int fmx_interactions_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, int32_t top_m,
                            void* dev_a_i64, void* dev_b_i64, void* dev_value_f64);
/* over every row of m and every pair a < b, with g = group_of_feature[c(a)], h = group_of_feature[c(b)]:
   sum[g][h] += I, abs_sum[g][h] += |I|, count[g][h] += 1, and the same into [h][g] when g != h (symmetric G x G tables, row-major;
   the diagonal holds the pairs inside one group).  group_of_feature: u32[p] on the host, every value < n_groups; NULL = identity, needs
   p <= n_groups.  1 <= n_groups <= 64.  count may be NULL.  The sums are fp64, added in an order that is a function of the matrix, the group
   map and the row cut alone (no floating-point atomics): the same inputs give the same bits on every call.  Counts are exact. */
int fmx_interactions_summary(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_feature, int32_t n_groups,
                             double* sum, double* abs_sum, int64_t* count);

/* ---- pointwise metrics with the standard definitions, per row group (per user, per day, per campaign): what fmx_evaluate, which keeps the
 *      reference's definitions, does not give.  For a CLASSIFICATION or REGRESSION engine, a labelled matrix m of its feature count on its
 *      device, rows [r0, r1), a group id per row (or none: one group) and a link:
 *          z_r = the raw forward of row r (fmx_predict_device over the same range with FMX_LINK_NONE, bit for bit),
 *          p_r = link(z_r), fmx_predict's own transform.
 *      Per group g, over the rows of the range whose group id is g:
 *      count i64[G][FMX_MET_COUNTS] = rows, positives, pairs2, correct (REGRESSION: positives = pairs2 = correct = 0).
 *          A row is positive iff its label is > 0 (core/Evaluation.h:49,61); every other row is negative.
 *          pairs2  = sum over (positive i, negative j) of 2 [z_i > z_j] + [z_i == z_j]: twice the Mann-Whitney U with ties as 1/2, an exact
 *                    integer.  The comparison is the ranking order's: -0 == +0, NaN below every number, NaN equal to NaN.
 *          correct = rows whose predicted class is the label's; predicted positive iff p_r >= 0.5; a NaN p_r is never correct.
 *      value f64[G][FMX_MET_VALUES], CLASSIFICATION (link FMX_LINK_LOGISTIC or FMX_LINK_PROBIT):
 *          AUC        = (double) pairs2 / (double) (2 P N): both integers converted round-to-nearest, one IEEE divide; NaN when P or N is 0
 *          LOGLOSS    = mean of l_r.  LOGISTIC: l_r = max(-t, 0) + log1p(exp(-|t|)), t = z_r for a positive row, -z_r for a negative one (stable
 *                       for any z).  PROBIT: l_r = -log(q_r), q_r = p_r for a positive row, 1 - p_r for a negative one: +inf where the probit
 *                       table saturates to 0 or 1 on the wrong side, and then the group's LOGLOSS is +inf
 *          ACCURACY   = correct / rows,   BRIER = mean of (p_r - [positive])^2,   MEAN_PRED = mean of p_r,   MEAN_LABEL = P / rows
 *      value, REGRESSION (link FMX_LINK_NONE or FMX_LINK_CLAMP), y_r the label:
 *          MSE = mean of (p_r - y_r)^2, RMSE = sqrt(MSE) (the IEEE square root of MSE's bits), MAE = mean of |p_r - y_r| (a true mean absolute
 *          error), MEAN_ERR = mean of p_r - y_r, MEAN_PRED = mean of p_r, MEAN_LABEL = mean of y_r
 *      Every term is formed in fp64 from individually rounded operations (subtract, multiply, fabs: no fma), and every mean is a fixed-order
 *      sum divided once by (double) rows.  An empty group has zero counts and NaN in every value.
 *      Guarantees: the integers are exact, so AUC, ACCURACY, the CLASSIFICATION MEAN_LABEL and RMSE-given-MSE are unique bits.  No floating-point
 *      value is summed by atomics; a group's sums are added in an order that is a function of that group's ascending row list alone, so a
 *      group's bits do not depend on the other groups, on n_groups, on how the group ids are numbered, on the internal form that counted its
 *      pairs, or on the call.  Parameters and optimiser state are never modified.  Both table precisions, the w-in-row layout and sequential
 *      engines are accepted; multi-GPU engines read their primary replica.  r1 - r0 <= 2^31 - 1 (pairs2 then fits 64 bits);
 *      1 <= n_groups <= 2^31 - 1.  Every refusal (a NULL handle, a RANKING engine, a matrix without labels, a p or device mismatch, a link of the
 *      other task's family, n_groups out of range, a host group id >= n_groups, NULL groups with n_groups != 1, a bad row range, a NULL
 *      out_value) is FMX_ERR_INVALID before any launch and before any output is written; an empty range is FMX_OK with nothing written. */
#define FMX_MET_VALUES 6      /* width of a value row */
#define FMX_MET_COUNTS 4      /* width of a count row */
#define FMX_MET_AUC 0         /* value columns, CLASSIFICATION */
#define FMX_MET_LOGLOSS 1
#define FMX_MET_ACCURACY 2
#define FMX_MET_BRIER 3
#define FMX_MET_MSE 0         /* value columns, REGRESSION */
#define FMX_MET_RMSE 1
#define FMX_MET_MAE 2
#define FMX_MET_MEAN_ERR 3
#define FMX_MET_MEAN_PRED 4   /* both tasks */
#define FMX_MET_MEAN_LABEL 5
#define FMX_MET_ROWS 0        /* count columns */
#define FMX_MET_POSITIVES 1
#define FMX_MET_PAIRS2 2
#define FMX_MET_CORRECT 3
/* every row of m.  The group ids are checked on the host (an id >= n_groups is refused) and uploaded once. */
int fmx_metrics(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row /* host u32[n] or NULL: one group, needs n_groups == 1 */,
                int64_t n_groups, int link, double* out_value /* [n_groups][6] */, int64_t* out_count /* [n_groups][4] or NULL */);
/* rows [r0, r1), device inputs and outputs.  The device form cannot check the ids: a row whose id is >= n_groups is ignored (it belongs to no
   group), as fmx_diversify_device treats a bad index. */
int fmx_metrics_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32 /* indexed from row r0; or NULL */,
                       int64_t n_groups, int link, void* dev_value_f64, void* dev_count_i64 /* may be NULL */);

/* ---- calibration of a CLASSIFICATION engine's probabilities, per row group: measure (a reliability table, ECE), fit (Platt scaling, isotonic
 *      steps), apply.  Common to every call below: a CLASSIFICATION engine (REGRESSION and RANKING are refused), a labelled matrix m of its
 *      feature count on its device, rows [r0, r1) with r1 - r0 <= 2^31 - 1, a group id per row or none (one group, n_groups == 1),
 *      1 <= n_groups <= 2^31 - 1.  The host forms refuse an id >= n_groups; the device forms ignore such a row (it belongs to no group; its
 *      calibrated prediction is NaN).  z_r is the raw forward of row r (fmx_predict_device with FMX_LINK_NONE, bit for bit); a row is positive iff
 *      its label is > 0.  Scores are compared by the ranking order's key, so -0 == +0.  Both table precisions, the w-in-row layout and sequential
 *      engines are accepted; multi-GPU engines read their primary replica; parameters and optimiser state are never modified.  Every refusal is
 *      FMX_ERR_INVALID with a message, before any launch and before any output is written; an empty range is FMX_OK with nothing written.
 *
 *      The calibrator is plain data behind host pointers; a call copies it and retains nothing. */
#define FMX_CAL_NONE  0   /* p = link(z), fmx_predict's transform */
#define FMX_CAL_PLATT 1   /* p = logistic(a z + b) */
#define FMX_CAL_STEPS 2   /* p = val[s], s the last step with thr[s] <= z */
typedef struct fmx_calibrator {
  uint32_t struct_size; int32_t kind;
  int64_t n_groups;            /* 1: one map for every row; else the call's n_groups */
  int32_t max_steps, link;     /* STEPS: row width of thr / val (>= 1); NONE: the FMX_LINK_* used (LOGISTIC or PROBIT) */
  const double* platt;         /* f64[n_groups][2] = a, b */
  const int32_t* n_steps;      /* i32[n_groups], each in 0..max_steps */
  const double* thr;           /* f64[n_groups][max_steps], ascending; thr[g][0] = -inf */
  const double* val;           /* f64[n_groups][max_steps] */
} fmx_calibrator;
/*      A NULL calibrator is FMX_CAL_NONE under the call's `link` argument (LOGISTIC or PROBIT); with a calibrator `link` is not read.
 *      p_r, the calibrated probability of a row with score z in group g (the map of group g, or the one map):
 *          NONE   p = link(z), fmx_predict's own transform.
 *          PLATT  t = __dadd_rn(__dmul_rn(a, z), b) (two rounded operations, no fma), p = 1 / (1 + exp(-t)), exactly fmx_predict's LOGISTIC
 *                 transform of t: (a, b) = (1, 0) is fmx_predict(FMX_LINK_LOGISTIC) bit for bit.  NaN in a or b gives NaN.
 *          STEPS  s = the last step of the group's first n_steps with key(thr[s]) <= key(z), found by binary search (thr ascending is the
 *                 caller's promise); p = the bits of val[s].  n_steps == 0, or no such step (thr[0] is not -inf), gives NaN.
 *          A NaN z gives NaN under every kind.
 *      fmx_predict_calibrated*: out f64[rows] = p_r.  A calibrator with n_groups == 1 (or NULL) needs no ids: they may be NULL whatever n_groups
 *      is, and the device form does not read them; one with n_groups > 1 needs ids and n_groups equal to its own. */
int fmx_predict_calibrated(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row /* host u32[n] or NULL */, int64_t n_groups,
                           const fmx_calibrator* cal, int link, double* out /* [n] */);
int fmx_predict_calibrated_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32 /* indexed from row r0; or NULL */,
                                  int64_t n_groups, const fmx_calibrator* cal, int link, void* dev_out_f64);

/* ---- the reliability table.  n_bins = B in 1..1024, n_groups * B <= 2^28.  A row of group g is VALID iff p_r is a number (so a row whose z is
 *      NaN, or whose map is empty, is not); the others belong to no bin and are counted in nan_rows[g].  s = the group's valid rows.
 *          FMX_BINS_WIDTH  bin = min(B - 1, (int) floor(__dmul_rn(p_r, (double) B))), and 0 where that is negative (a step map may hold any value).
 *          FMX_BINS_MASS   the group's valid rows ascending by (key of z, row); head = the 0-based position of the first row of the row's run of
 *                          equal keys; bin = floor(head * B / s) in exact integers (fmx_split_assign's fold formula on the run head).  Equal
 *                          scores share a bin, bins may be empty, the bin is non-decreasing in z, and with B >= s every run has its own bin.
 *      count i64[G][B][2] = rows, positives: exact.  sum_p f64[G][B] = sum of p_r.  lo_z, hi_z f64[G][B] = the bits of the smallest and largest
 *      raw score of the bin, of two zeros -0 being the smaller (order-free); NaN for an empty bin.  nan_rows i64[G].
 *      value f64[G][FMX_CAL_VALUES], formed from the table b ascending over the non-empty bins, from +0.0, every operation rounded, no fma:
 *          gap_b = |sum_p_b / (double) rows_b - (double) pos_b / (double) rows_b|
 *          ECE   = ECE + ((double) rows_b / (double) s) * gap_b,      MCE = gap_b where gap_b > MCE
 *      so, given the table's bits, ECE and MCE are unique bits.  BRIER = mean over the valid rows of (p_r - [positive])^2; LOGLOSS = mean of
 *      -log(q_r), q_r = p_r for a positive row and 1 - p_r otherwise (fmx_metrics' PROBIT form under every map: a step map can return 0 or 1,
 *      and then the value is +inf).  A group with s == 0 has zero counts and NaN values.
 *      No floating-point value is summed by atomics.  A bin's rows are added in chunks of 1 024 along the bin's ascending row list (WIDTH) or
 *      (key, row) list (MASS), each chunk in a fixed tree, the chunks ascending; BRIER and LOGLOSS add the group's non-empty bins' sums b
 *      ascending and divide once.  The order is a function of the group's own rows, B, the binning and the map alone: a group's bits do not
 *      depend on the other groups, on n_groups, on how the ids are numbered, or on the call.  Every output may be NULL. */
#define FMX_BINS_WIDTH 0
#define FMX_BINS_MASS 1
#define FMX_CAL_VALUES 4      /* width of a value row */
#define FMX_CAL_ECE 0
#define FMX_CAL_MCE 1
#define FMX_CAL_BRIER 2
#define FMX_CAL_LOGLOSS 3
int fmx_reliability(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row, int64_t n_groups, int32_t n_bins, int32_t binning,
                    const fmx_calibrator* cal, int link, int64_t* out_count, double* out_sum_p, double* out_lo_z, double* out_hi_z, int64_t* out_nan_rows,
                    double* out_value);
int fmx_reliability_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, int32_t n_bins,
                           int32_t binning, const fmx_calibrator* cal, int link, void* dev_count_i64, void* dev_sum_p_f64, void* dev_lo_z_f64,
                           void* dev_hi_z_f64, void* dev_nan_rows_i64, void* dev_value_f64);

/* ---- Platt scaling.  Per group, (a, b) minimises  sum_r logloss([positive_r], sigma(a z_r + b)) + lambda / 2 ((a - 1)^2 + b^2)  -- the ridge
 *      pulls towards the identity map -- by n_newton >= 1 full Newton steps from (1, 0): no line search and no early exit, fmx_fold_in's
 *      convention.  lambda >= 0 (NaN is refused).  A row takes part iff it has a group and its z is finite.  Per step, with y = +-1 the row's
 *      class, m = y (a z + b), sigma = 1 / (1 + exp(-m)), nu = 1 / (1 + exp(m)) (fold-in's forms), w = sigma nu, d = -y nu (= sigma(a z + b) - t):
 *          g = (sum d z + lambda (a - 1),  sum d + lambda b),   H = [[sum w z^2 + lambda, sum w z], [sum w z, sum w + lambda]],
 *      (a, b) += the solution of H x = -g by a 2 x 2 Cholesky.  The five sums are fp64 in a fixed order (chunks of 1 024 of the group's ascending
 *      participating rows, a fixed tree per chunk, the chunks ascending): no atomics, a function of the group's own rows alone.
 *      status i32[G]: 0 solved; 1 a pivot was not positive or not finite in some step, and then a, b are NaN.  A group without rows gets (1, 0)
 *      with lambda > 0 and status 1 with lambda == 0.  status 0 does not promise convergence or a lower loss: on a separable or one-class group
 *      the undamped steps overshoot (40 rows of one class with scores spread over -6 .. 8 end near a = 930 after 8 steps at lambda 0.1).
 *      ab f64[G][2], rows i64[G] (the rows that took part), status: each may be NULL. */
int fmx_calibrate_platt(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row, int64_t n_groups, double lambda, int32_t n_newton,
                        double* out_ab, int64_t* out_rows, int32_t* out_status);
int fmx_calibrate_platt_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, double lambda,
                               int32_t n_newton, void* dev_ab_f64, void* dev_rows_i64, void* dev_status_i32);

/* ---- isotonic calibration over equal-mass bins: the FMX_BINS_MASS table of the raw scores for n_bins = B (1..1024, n_groups * B <= 2^28; the
 *      valid rows are those whose z is not NaN), then adjacent violators pooled over the non-empty bins, b ascending, on the integer pairs
 *      (positives, rows): a bin joins the block before it while pos_prev * rows_cur >= pos_cur * rows_prev (64-bit products, at most 2^62;
 *      equal pools too, so the block values rise strictly and the blocks are unique).
 *      n_steps i32[G] = the blocks; thr f64[G][B]: -inf for the first block, else the lo_z of the block's first bin; val f64[G][B] =
 *      (double) pos / (double) rows, one IEEE divide; unused slots hold NaN.  Everything is exact.  With B >= s this is the exact isotonic
 *      regression of the group.  The three outputs are a FMX_CAL_STEPS calibrator with max_steps = B.  Each may be NULL. */
int fmx_calibrate_isotonic(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row, int64_t n_groups, int32_t n_bins, int32_t* out_n_steps,
                           double* out_thr, double* out_val);
int fmx_calibrate_isotonic_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, int32_t n_bins,
                                  void* dev_n_steps_i32, void* dev_thr_f64, void* dev_val_f64);

/* ---- full-ranking evaluation on held-out items.  context, items and exclude as for fmx_topk.  heldout: n == context rows, p == item rows;
 *      the column ids of row c are H_c, context c's held-out positives (values ignored, any order, duplicates count once).  X_c = exclude's
 *      row c (NULL: empty); an id both in H_c and in X_c is FMX_ERR_INVALID, detected before any output is written.
 *      score(c, j) is the raw score fmx_topk computes for the pair, bit for bit, and the order is fmx_topk's (a higher score first, equal
 *      scores by the lower item index, NaN below every number).  The eligible items of c are all items but X_c, and
 *          rank(c, h)     = |{j eligible : j before h}|  (0-based; h itself and excluded items never count)
 *          neg_rank(c, h) = rank(c, h) - |{h' in H_c : h' before h}|,   N_c = items - |X_c| - |H_c| (distinct ids)
 *      so h is in fmx_topk(c, K, exclude) iff rank(c, h) < K, at position rank(c, h).
 * Metrics per context with |H_c| >= 1, in fp64 (hits_K = |{h : rank < K}|):
 *      precision@K = hits_K / K, recall@K = hits_K / |H_c|, hit@K = [hits_K > 0],
 *      ndcg@K = sum_{h: rank < K} 1 / log2(rank + 2)  /  sum_{t < min(K, |H_c|)} 1 / log2(t + 2)   (binary relevance),
 *      mrr = 1 / (1 + min_h rank),  auc = mean over h of (N_c - neg_rank) / N_c  (NaN when N_c = 0).
 * AUC breaks ties of equal scores by the item index, as the order does; FMX_EVAL_PAIR_ACC counts a tie as 1/2 instead.  A context without
 * held-out items gets NaN and is not counted; a context with N_c = 0 is left out of the AUC mean only.  The means are over contexts in
 * ascending order by a fixed reduction tree: the same inputs give the same bits every call, whatever the chunking, slicing or row range.
 * Multi-GPU engines read their primary replica; both table precisions, with fmx_topk's factor limit. */
/* ranks of held-out items: out_rank i64[heldout nnz], out_score f64[heldout nnz] (raw score, may be NULL), in heldout's entry order;
   duplicate entries get the same values */
int fmx_heldout_rank(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* heldout,
                     const fmx_matrix* exclude, int64_t* out_rank, double* out_score);
/* the same for context rows [r0, r1): device outputs indexed from heldout->row_ptr[r0] (mirrors fmx_contrib_device) */
int fmx_heldout_rank_device(fmx_engine* e, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items,
                            const fmx_matrix* heldout, const fmx_matrix* exclude, void* dev_rank_i64, void* dev_score_f64);
/* ks: n_ks values (1 <= n_ks <= 32, every K >= 1, no upper bound); out f64[4 n_ks + 2] = per K (precision, recall, ndcg, hit), then mrr, auc;
   per_context NULL or f64[n_ctx][4 n_ks + 2]; counted NULL or i64[2] = contexts with a held-out item, contexts with auc defined */
int fmx_heldout_metrics(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* heldout,
                        const fmx_matrix* exclude, const int32_t* ks, int32_t n_ks, double* out, double* per_context,
                        int64_t* counted);

/* ---- re-ranking of candidate lists.  context and items as for fmx_topk.  lists: n == context rows, p == item rows; the column ids of row c
 *      are L_c, the candidates of context c (values ignored, any order, duplicates allowed; an empty row is allowed).
 *      score(c, j) is the raw score fmx_topk computes for the pair, bit for bit, and the order is fmx_topk's (a higher score first, equal
 *      scores -- -0 = +0 -- by the lower item index, NaN below every number): strict and total on distinct items.
 *          pos(c, j) = |{j' in distinct(L_c) : j' before j}|   (0-based; duplicate entries of one list get the same score and the same
 *                                                               position and count once)
 *      so fmx_topk(c, K, exclude = every item not in L_c) lists exactly the candidates with pos < K, candidate j in slot pos(c, j); and if
 *      L_c is every item outside an exclusion list X_c, pos(c, h) = rank(c, h) of fmx_heldout_rank(exclude = X).  The work is O(entries of
 *      lists) after one projection of the items (the host forms stage their results in pieces and project once per piece of 2^22 entries
 *      or result slots; the _device forms once per call); results are the same bits for any chunking, row range, list order or internal path, and on
 *      every call (nothing is ordered by atomics, no floating-point value is summed by them).
 * Accepted engines and limits are fmx_topk's (both table precisions, its factor limit; multi-GPU engines read their primary replica;
 * parameters and optimiser state are not modified).  lists must be context->n x items->n on the engine's device.  A single list holds at most
 * 2^32 - 1 entries; lists->nnz is bounded by memory only (the calls work in chunks).  Every refusal is FMX_ERR_INVALID before any launch and
 * before any output is written; context->n == 0 or an empty range is FMX_OK with nothing written. */
/* out_score f64[lists nnz] (link applied), out_pos i64[lists nnz] or NULL, in lists' entry order; positions always follow the raw score */
int fmx_rank_lists(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* lists, int link,
                   double* out_score, int64_t* out_pos);
/* the same for context rows [r0, r1): device outputs indexed from lists->row_ptr[r0] (mirrors fmx_heldout_rank_device); dev_pos_i64 may be NULL */
int fmx_rank_lists_device(fmx_engine* e, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items,
                          const fmx_matrix* lists, int link, void* dev_score_f64, void* dev_pos_i64);
/* [n_ctx][top_k] as fmx_topk: slot t of context c holds the distinct candidate with pos == t (its index and the linked score); slots beyond
   the number of distinct candidates hold index -1 and score NaN (every slot when lists holds nothing).  1 <= top_k <= 1024; a caller who
   wants a whole longer list in order uses fmx_rank_lists' out_pos */
int fmx_topk_lists(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* lists, int32_t top_k, int link,
                   int64_t* out_index, double* out_score);
int fmx_topk_lists_device(fmx_engine* e, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items,
                          const fmx_matrix* lists, int32_t top_k, int link, void* dev_index_i64, void* dev_score_f64);
/* the two sides of the score: out_base[r] = the forward of row r of m (keep_w0 / keep_w1 honoured; w0 added only if with_w0 != 0),
 * out_s[r][f] = the factor sum  sum_j x_j v_j,f  as fmx_topk holds it: rounded to the state type (float for fp32 tables) and widened exactly
 * to double; f < k only.  For a context row c and an item row i, with bc, s_c from with_w0 = 1 and bi, s_i from with_w0 = 0,
 *      raw fmx_topk score(c, i) == (bc + bi) + (double) chain,   chain = fma(s_c[k-1], s_i[k-1], ... fma(s_c[0], s_i[0], 0))
 * evaluated in the state type.  (The kernels run the chain over zero-padded factors; fma(0, 0, acc) returns acc for every value but -0,
 * which it turns into +0, so the two forms can differ only in the sign of a zero dot product added to a zero base.)  A row's values do not
 * depend on the range or the chunking of the call.  No limit on the factor count; multi-GPU engines read their primary replica. */
int fmx_project(fmx_engine* e, const fmx_matrix* m, int32_t with_w0, double* out_base /* f64[n] */,
                double* out_s /* f64[n][k] row-major; may be NULL when k == 0 */);
int fmx_project_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, int32_t with_w0, void* dev_base_f64,
                       void* dev_s_f64);

/* ---- diversified re-ranking: greedy maximal marginal relevance (MMR) over ranked pools.  The input is what fmx_topk /
 *      fmx_topk_lists write: per context row a pool of `pool` slots, index i64[n][pool] and score f64[n][pool].  The call returns top_k of them in
 *      the order greedy MMR picks them; it needs the items, not the contexts.  T is the engine's state type (float for fp32 tables, double for fp64).
 *   1. Empty slots.  A slot whose index is outside [0, items->n) is empty and never selected.  The host form refuses any index other than -1 that
 *      is out of range; the device form cannot check, treats every such index as empty and reads no row for it.  Duplicate items in a row are
 *      allowed: every slot is a candidate of its own.
 *   2. Projections.  s_i is item i's projection, fmx_project(with_w0 = 0)'s values;  d(i, j) = (double) fma(s_i[ks-1], s_j[ks-1], ... fma(s_i[0],
 *      s_j[0], 0)): one accumulator in T, f ascending over the zero-padded factors -- fmx_topk's chain without the bases.
 *   3. Norms.  nrm(i) = d(i, i);  inv(i) = 1.0 / sqrt(nrm(i)) in fp64 (IEEE sqrt, then IEEE divide) if nrm(i) is finite and > 0, else 0.0.
 *   4. Similarity of candidate slot u and selected slot v: 0.0 if inv of either item is 0, else (d(i_u, i_v) * inv(i_u)) * inv(i_v), two rounded
 *      fp64 products.  A zero or overflowed row is similar to nothing.
 *   5. Relevance.  FMX_DIV_REL_SCORE: rel(u) = score(u).  FMX_DIV_REL_MINMAX: hi, lo = the largest and smallest non-NaN score among the row's
 *      non-empty slots (a zero bound taken as +0); rel(u) = (score(u) - lo) / (hi - lo) when both are finite and hi > lo, else +0.0; a NaN score
 *      stays NaN.
 *   6. mu = 1.0 - lambda, computed once on the host.
 *   7. Selection.  Step t = 0, 1, ... until top_k slots are selected or none is left.  For every slot not yet selected
 *          margin(u) = lambda * rel(u) - mu * pen(u)      (two products and a difference: three fp64 roundings; every NaN margin is the one
 *                                                          quiet NaN 0x7ff8000000000000)
 *      pen(u) = +0.0 at t = 0; at t >= 1 the largest sim(u, v) over the slots v selected so far (the earlier one of equal values).  The step
 *      selects the first slot under fmx_topk's order on the margin -- a higher margin first, -0 = +0, NaN below every number -- ties by the
 *      lower item index, then by the lower slot number.
 *   8. Outputs.  out_index[c][t], out_score[c][t]: the item and the GIVEN score of the slot selected at step t, bits copied; out_margin[c][t]: its
 *      margin at that step.  Slots beyond the number selected hold -1 / NaN / NaN.
 * So lambda = 1 with FMX_DIV_REL_SCORE returns the pool's non-empty slots in fmx_topk's order: fed with fmx_topk(K = pool)'s output it equals
 * fmx_topk(top_k), bit for bit.  A row's result does not depend on the other rows, the chunking, the internal form (pool in LDS or in global
 * memory) or, for rows of distinct items, the order of the slots; the result for a smaller top_k is a prefix of the result for a larger one; the same
 * bits on every call (nothing is ordered or summed by atomics); parameters and optimiser state are not modified.
 * Limits: 1 <= pool <= 1024, 1 <= top_k <= pool, lambda in [0, 1] (NaN refused), relevance one of the two constants; engines and the factor limit
 * are fmx_topk's; items on the engine's device with its feature count; multi-GPU engines read their primary replica.  Every refusal is
 * FMX_ERR_INVALID with a message, before any launch and before any output is written; n == 0 is FMX_OK with nothing written. */
#define FMX_DIV_REL_SCORE  0   /* relevance = the score as given */
#define FMX_DIV_REL_MINMAX 1   /* relevance = the score rescaled to [0, 1] over the row's pool */
int fmx_diversify(fmx_engine* e, const fmx_matrix* items, int64_t n, int32_t pool, const int64_t* index /* [n][pool] */,
                  const double* score /* [n][pool] */, int32_t top_k, double lambda, int32_t relevance, int64_t* out_index /* [n][top_k] */,
                  double* out_score /* [n][top_k] */, double* out_margin /* [n][top_k] or NULL */);
/* the same on device buffers (items projected once per call) */
int fmx_diversify_device(fmx_engine* e, const fmx_matrix* items, int64_t n, int32_t pool, const void* dev_index_i64,
                         const void* dev_score_f64, int32_t top_k, double lambda, int32_t relevance, void* dev_out_index_i64,
                         void* dev_out_score_f64, void* dev_out_margin_f64 /* may be NULL */);

/* ---- nearest neighbours: the top_k item rows most similar to each query row by the cosine (or the dot product) of their
 *      factor projections -- "more like this".  queries and items are any two matrices with the engine's feature count (the same matrix twice
 *      for item-to-item neighbours).  T is the engine's state type (float for fp32 tables, double for fp64).
 *   1. Projections.  s_r is row r's projection, fmx_project(with_w0 = 0)'s values; queries and items are projected the same way.  The base plays no
 *      part, and neither do w0 or w.
 *   2. Dot.  d(q, i) = (double) fma(s_q[ks-1], s_i[ks-1], ... fma(s_q[0], s_i[0], 0)): one accumulator in T, f ascending over the zero-padded
 *      factors -- fmx_diversify's step 2.
 *   3. Norms.  nrm(r) = d(r, r);  inv(r) = 1.0 / sqrt(nrm(r)) in fp64 (IEEE sqrt, then IEEE divide) if nrm(r) is finite and > 0, else 0.0 --
 *      fmx_diversify's step 3.
 *   4. Score.  FMX_SIM_COSINE: 0.0 if inv(q) or inv(i) is 0.0, else (d(q, i) * inv(q)) * inv(i), two rounded fp64 products, the query's inverse
 *      norm first: fmx_diversify's step 4 with (candidate = q, selected = i) gives the same bits.  A zero or overflowed row is similar to nothing.
 *      FMX_SIM_DOT: d(q, i); no norm is computed.  The rounded cosine is NOT exactly symmetric in (q, i): the two products associate differently,
 *      so score(q, i) and score(i, q) may differ in the last bit.
 *   5. Order and outputs.  The order is fmx_topk's: a higher score first, -0 = +0, equal scores by the lower item index, NaN below every number
 *      but still eligible.  Slot t of query row q holds the item at position t and its score (no link is applied); slots beyond the eligible
 *      items hold -1 / NaN.
 *   6. skip_self != 0: query row r -- its absolute row index in `queries`, also in the _device form -- never receives item index r.  This is the
 *      call with queries == items.  Nothing else is excluded; there is no exclusion matrix in this call.
 *   7. Guarantees.  A (query, item) score is the same bits whatever the tiling, slicing, chunking, row range or call; a query's result does not
 *      depend on the other queries; the result for a smaller top_k is a prefix of the result for a larger one; nothing is ordered or summed by
 *      atomics; parameters and optimiser state are not modified.
 *   8. Limits.  1 <= top_k <= 1024; metric one of the two constants; items->n < 2^31 - 1; engines and the factor limit are fmx_topk's (both table
 *      precisions, the w-in-row layout); both matrices on the engine's device with its feature count; multi-GPU engines read their primary
 *      replica.  Every refusal is FMX_ERR_INVALID with a message, before any launch and before any output is written; queries->n == 0 or an
 *      empty range is FMX_OK with nothing written; items->n == 0 writes -1 / NaN everywhere. */
#define FMX_SIM_COSINE 0   /* the cosine of the two projections */
#define FMX_SIM_DOT    1   /* their dot product */
int fmx_neighbors(fmx_engine* e, const fmx_matrix* queries, const fmx_matrix* items, int32_t top_k, int32_t metric, int32_t skip_self,
                  int64_t* out_index /* [n_q][top_k] */, double* out_score /* [n_q][top_k] */);
/* the same for query rows [r0, r1): device outputs [r1 - r0][top_k] (items projected once per call) */
int fmx_neighbors_device(fmx_engine* e, const fmx_matrix* queries, int64_t r0, int64_t r1, const fmx_matrix* items, int32_t top_k,
                         int32_t metric, int32_t skip_self, void* dev_index_i64, void* dev_score_f64);

/* ---- clustered item index: an inverted-file index over the items' projections, and fmx_topk over the n_probe lists closest
 *      to each context instead of over every item.  Nothing about a pair's score changes: a candidate's score is fmx_topk's bit for bit and the
 *      order is fmx_topk's; with every list probed the call IS fmx_topk.  The approximation is only in which lists are looked at, and that choice
 *      is the exactly stated function of the index below.
 *   The index.  An opaque fmx_item_index on the engine's device; plain data, it holds no parameters and no projections: n_items, n_lists, k (the
 *      engine's factor count at build time), centroid f64[n_lists][k + 1], assign u32[n_items], and the lists as list_ptr i64[n_lists + 1],
 *      list_item i32[n_items] -- the items of list l in ascending item index.  The augmented vector of item i is
 *          a_i = (s_i[0 .. k-1] widened to double, base_i),   s_i and base_i fmx_project(items, with_w0 = 0)'s values,
 *      so that the item side of score(c, i) = base_c + base_i + <s_c, s_i> is the inner product of (s_c, 1) with a_i.  An item is FINITE if all
 *      k + 1 components are finite.
 *   Build.  fmx_index_build(e, items, n_lists, n_iter, seed, &out): 1 <= n_lists <= min(finite items, 65 536), 0 <= n_iter <= 100, otherwise
 *      FMX_ERR_INVALID with *out = NULL.
 *      1. Seeds.  The finite items ordered by (pair_hash(seed, 0, i, 5), i) -- the counter hash of fmx_matrix_pairs, stream 5; centroid l is a
 *         bit copy of a of the l-th item of that order.
 *      2. Assign, against the current centroids.  d(i, l): acc = 0; for f = 0 .. k ascending: t = a_i[f] - mu_l[f], acc = fma(t, t, acc), all in
 *         fp64.  Item i goes to the first l (ascending) whose distance is strictly below the best so far, the best starting at +inf; if none
 *         is, to list 0.  Non-finite items go to list 0.
 *      3. Update.  A list with at least one finite member: mu_l[f] = sum / (double) cnt over its finite members, the sum in one order that
 *         depends on the list's ascending member list alone -- fmx_matrix_column_stats' order: chunks of 1 024 positions of the list; within a
 *         chunk lane l of 64 adds the terms at positions l, l + 64, ... in that order from +0.0 (a non-finite member adds nothing), the lanes
 *         meet in an xor butterfly (strides 32, 16, ..., 1); the chunk sums are added ascending from +0.0.  No floating-point atomics.  A list
 *         without finite members keeps its centroid's bits.
 *      4. n_iter times (assign, update), then one final assign: the exported assign is the exact arg-min against the exported centroids.  The
 *         lists follow from assign by a stable sort.
 *      The result is a function of (the items' projections, n_lists, n_iter, seed) alone: the same bits on every call.
 *   fmx_index_from_assign(e, n_items, n_lists, assign, centroid, &out) (host arrays; 1 <= n_lists <= 65 536, 0 <= n_items < 2^31 - 1) builds the
 *      same object from a caller's clustering with k = the engine's: hand-made indexes, reloading, tests.  Any centroid bits are accepted; an
 *      assign[i] >= n_lists is refused, naming the lowest such i.
 *   fmx_index_info: any output may be NULL.  fmx_index_export: host arrays, any may be NULL.  fmx_index_free(NULL) is a no-op.
 *   Search.  fmx_topk_index(e, index, context, items, exclude, top_k, n_probe, link, ...): context, items, exclude, top_k, link, the factor limit
 *      and the accepted engines are fmx_topk's; items->n must equal the index's n_items, the engine's k the index's k, the index must live on the
 *      engine's device, and 1 <= n_probe <= n_lists.  The items are projected once per call, as fmx_topk does, so the call always scores under
 *      the engine's CURRENT parameters: a stale index costs recall, never the correctness of a score.
 *      1. Coarse score.  g(c, l) = mu_l[k] + acc with acc = 0; for f = 0 .. k-1 ascending: acc = fma((double) s_c[f], mu_l[f], acc) -- fp64 for
 *         both table types.
 *      2. Probe set.  P_c = the first min(n_probe, non_empty) NON-EMPTY lists under fmx_topk's order on (g, l): a higher g first, equal g by the
 *         lower list id, NaN below every number, -0 = +0.
 *      3. Result.  The first top_k candidates of P_c in fmx_topk's order; the candidates are the items of the lists of P_c that are not in
 *         exclude's row c, each with fmx_topk's raw score bit for bit.  Missing slots hold index -1 and score NaN.  The link is applied to the
 *         returned values only.
 *      4. out_scanned[c] (i64, may be NULL) = the number of items in the lists of P_c, before exclusion.
 *      Consequences.  n_probe >= non_empty gives fmx_topk's outputs bit for bit.  Probe sets are nested in n_probe, so slot t at n_probe + 1
 *      never comes after slot t at n_probe in the order.  A row's result does not depend on the other rows, the chunking, the host or device
 *      entry point or the call.  Every refusal is FMX_ERR_INVALID with a message, before any launch and before any output is written;
 *      context->n == 0 or an empty range is FMX_OK with nothing written.  Parameters and optimiser state are not modified. */
typedef struct fmx_item_index fmx_item_index;
#define FMX_INDEX_MAX_LISTS 65536
#define FMX_INDEX_MAX_ITER  100
int fmx_index_build(fmx_engine* e, const fmx_matrix* items, int32_t n_lists, int32_t n_iter, uint64_t seed, fmx_item_index** out);
int fmx_index_from_assign(fmx_engine* e, int64_t n_items, int32_t n_lists, const uint32_t* assign /* [n_items] */,
                          const double* centroid /* [n_lists][k + 1] */, fmx_item_index** out);
int fmx_index_info(const fmx_item_index* index, int64_t* n_items, int32_t* n_lists, int32_t* k, int64_t* non_empty);
int fmx_index_export(const fmx_item_index* index, double* centroid /* [n_lists][k + 1] */, uint32_t* assign /* [n_items] */,
                     int64_t* list_ptr /* [n_lists + 1] */, int32_t* list_item /* [n_items] */);
int fmx_index_free(fmx_item_index* index);
/* out_index i64[n_ctx][top_k], out_score f64[n_ctx][top_k], out_scanned i64[n_ctx] or NULL: host, row-major */
int fmx_topk_index(fmx_engine* e, const fmx_item_index* index, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* exclude,
                   int32_t top_k, int32_t n_probe, int link, int64_t* out_index, double* out_score, int64_t* out_scanned);
/* the same for context rows [r0, r1), outputs [r1 - r0][top_k] and [r1 - r0] on the device (mirrors fmx_topk_device) */
int fmx_topk_index_device(fmx_engine* e, const fmx_item_index* index, const fmx_matrix* context, int64_t r0, int64_t r1,
                          const fmx_matrix* items, const fmx_matrix* exclude, int32_t top_k, int32_t n_probe, int link, void* dev_index_i64,
                          void* dev_score_f64, void* dev_scanned_i64 /* may be NULL */);

/* ---- fold-in: the rows (w_u, v_u) of features the model has not seen, solved against the frozen model from the rows of
 *      m that mention them.  For a fold feature u and a row r that stores u exactly once, with value x,
 *          y(r) = b_r + <z_r, theta_u>,   theta_u = (w_u, v_u),   z_r = x (keep_w1, t_r),   t_r = sum_{j != u} x_j v_j,
 *      b_r the forward of the row without that entry (keep_w0 / keep_w1 honoured).  With Lambda = diag(lambda_w, lambda_v, ..., lambda_v) and
 *      R_u the rows that hold u:
 *        REGRESSION      theta_u minimises sum_{R_u} (y_r - b_r - <z_r, theta>)^2 + theta' Lambda theta: (Z'Z + Lambda) theta = Z'(y - b), one
 *                        Cholesky solve; targets and predictions are NOT clamped to [min_target, max_target]; n_newton is ignored.
 *        CLASSIFICATION  labels +-1, the logistic loss whatever solver trained the model: n_newton full Newton steps from theta = 0 (no line
 *                        search, no early exit): y^_r = b_r + <z_r, theta>, sigma_r = 1 / (1 + exp(-y_r y^_r)),
 *                        g = sum -y_r (1 - sigma_r) z_r + Lambda theta, H = sum sigma_r (1 - sigma_r) z_r z_r' + Lambda, theta -= H^-1 g.
 *      With keep_w1 = 0, w_u is not a variable and is returned as 0.
 * m: a labelled matrix on the engine's device with the engine's p.  A row that stores no fold feature is ignored; a row that stores two entries
 * whose columns are fold features (the same column twice included) is FMX_ERR_INVALID.
 * out_status: 0 solved; 1 a Cholesky pivot was not positive or not finite -- out_w / out_v are then NaN and, with apply, the engine's row stays
 * untouched.  A feature without rows gets theta = 0 with positive lambdas (status 0) and status 1 with a zero lambda.  Status 0 says only
 * that every pivot was positive and finite, NOT that the problem was well-posed: with a zero lambda a rank-deficient group (fewer than 1 + k
 * rows, or dependent rows) can leave a tiny positive pivot in floating point and return status 0 with a meaningless theta -- callers with few
 * rows per feature keep lambda positive, or compare out_rows with 1 + k.  apply != 0 writes the
 * solved rows exactly as fmx_set_rows would (rounded to the state type, every other row and all optimiser state left alone, every replica of a
 * multi-GPU engine); apply == 0 modifies nothing.
 * Refusals, all FMX_ERR_INVALID before any launch that writes a result and before any output or parameter is touched: a NULL engine or matrix,
 * a p or device mismatch, m without labels, an id >= p, an id listed twice, a negative or NaN lambda, a RANKING engine, num_factor > 64, one fold feature stored in more than
 * 2^24 rows (a group's rows are held together: 8.7 GB at 64 factors), and for
 * CLASSIFICATION n_newton < 1 or a label other than +-1 in a participating row.  n_ids == 0 is FMX_OK with nothing written.
 * Guarantees: (1) all arithmetic is fp64 for both table types, as in fmx_contrib.  (2) The current parameters of the fold features are never
 * read: the results are the same bits whatever those rows hold, NaN included.  (3) A feature's result depends only on its own rows taken in
 * ascending row order: the same bits whether it is folded alone or with any other ids, in any order of ids, and on every call (no
 * floating-point atomics; a group cut over several workgroups adds its partial sums in ascending chunk order).  (4) Both table precisions and
 * the w-in-row layout; multi-GPU engines read their primary replica. */
int fmx_fold_in(fmx_engine* e, const fmx_matrix* m, const uint32_t* ids, int64_t n_ids, double lambda_w, double lambda_v, int32_t n_newton,
                int32_t apply, double* out_w /* f64[n_ids] or NULL */, double* out_v /* f64 k x n_ids, v[f + i*k], as fmx_get_rows; or NULL */,
                int64_t* out_rows /* i64[n_ids] or NULL: |R_u| */, int32_t* out_status /* i32[n_ids] or NULL */);

/* ---- pairwise fold-in: the same solve for FMX_TASK_RANKING engines, on difference vectors.  m is a pair matrix as the
 *      task defines it: an even row count, rows 2t and 2t + 1 are pair t, row 2t the preferred one; labels are ignored and may be absent.
 *      Per row, b_r and z_r are fmx_fold_in's (a row stores at most one entry of the fold features), except that b_r never includes w0 (it
 *      cancels in every pair) and that a row WITHOUT a fold entry has b_r = its whole forward and z_r = 0 exactly (by selection, never by a
 *      product with zero).  A pair takes part if at least one of its rows stores a fold feature u -- its group; two rows that store different
 *      fold features are refused -- with
 *          d_t(theta) = B_t + <Z_t, theta_u>,   B_t = b_2t - b_2t+1,   Z_t = z_2t - z_2t+1,
 *      and theta_u minimises sum_{T_u} log(1 + exp(-d_t)) + theta' Lambda theta / 2 by n_newton full Newton steps from theta = 0 (no line search,
 *      no early exit): fmx_fold_in's CLASSIFICATION loop with every label +1,
 *          sigma_t = 1 / (1 + exp(-d_t)),  H = sum sigma_t (1 - sigma_t) Z_t Z_t' + Lambda,  rhs = sum (1 - sigma_t) Z_t - Lambda theta,  theta += H^-1 rhs.
 *      With keep_w1 = 0, w_u is not a variable and is returned as 0.  This covers a new item seen as a positive (u in row 2t only), a new item
 *      seen as a sampled negative (u in row 2t + 1 only) and a new user (u in both rows).  For a new user with equal values in both rows Z_t[0]
 *      is exactly 0: a pair says nothing about w_u, which comes out exactly 0 with lambda_w > 0, while with lambda_w = 0 the first pivot is
 *      exactly 0 and the feature gets status 1 -- A USER-SIDE FOLD-IN NEEDS lambda_w > 0 OR keep_w1 = 0.  A new user and a new item that meet
 *      in one row are refused (two fold entries in a row): fold them in separate calls.
 * out_pairs: |T_u|, the pairs of every feature.  out_status, NaN outputs on a failed pivot, apply (through fmx_set_rows, solved features only)
 * and n_ids == 0 (FMX_OK, nothing written) are fmx_fold_in's, as is what status 0 does and does not say.
 * Refusals, all FMX_ERR_INVALID before any launch that writes a result and before any output or parameter is touched: a NULL engine or matrix,
 * a p or device mismatch, an odd row count, an engine that is not RANKING (fmx_fold_in solves those), num_factor > 64, an id >= p, an id listed
 * twice, a negative or NaN lambda, n_newton < 1, a row with two fold entries, a pair whose rows hold different fold features, one feature
 * in more than 2^24 pairs.
 * Guarantees: (1) all arithmetic is fp64 for both table types.  (2) The fold features' current rows are never read: the same bits whatever
 * they hold, NaN included; w0 is never read either.  (3) A feature's bits depend only on its own pairs taken in ascending pair order: not on
 * which other ids the call holds, on the order of ids, on the slab a group falls in, or on the call (no floating-point atomics).  (4) Both
 * table precisions and the w-in-row layout; multi-GPU engines read their primary replica, apply writes every replica.  (5) Consistency with
 * fmx_fold_in: if every row 2t + 1 of m is empty and m' holds m's rows 2t with labels +1, fmx_fold_in_pairs(m) returns bit for bit what
 * fmx_fold_in(m') returns on a CLASSIFICATION engine with the same tables, keep_w0 = 0 and the same lambdas and n_newton; if the rows 2t are
 * the empty ones and m' holds the rows 2t + 1 with labels -1, likewise (every operation involved is sign-symmetric).  The two calls share
 * the row arithmetic, the Gram kernel and the solve. */
int fmx_fold_in_pairs(fmx_engine* e, const fmx_matrix* m, const uint32_t* ids, int64_t n_ids, double lambda_w, double lambda_v, int32_t n_newton,
                      int32_t apply, double* out_w /* f64[n_ids] or NULL */, double* out_v /* f64 k x n_ids, as fmx_fold_in; or NULL */,
                      int64_t* out_pairs /* i64[n_ids] or NULL: |T_u| */, int32_t* out_status /* i32[n_ids] or NULL */);

/* ---- ALS V-column sweep (solver/MCMC_ALS_Learner.h:272-354, ALS branch, one attribute group):
 * error: f64[n] residual on entry (y_hat - y, :520-527), updated in place; v_lambda, v_mu: f64[k] or NULL (zeros). */
int fmx_als_vsweep(fmx_engine* e, fmx_matrix* m, double* error, double alpha, const double* v_lambda,
                   const double* v_mu);
/* The MCMC (Gibbs) form of the same sweep (do_sample, :329-331): every coordinate is drawn from N(mean, var) instead of set
 * to the mean.  The reference draws with R's Rf_rnorm inside the loop; here the caller pre-draws the standard normals in the
 * same order -- std_normals: f64[k][p], element (f, j) at f*p + j, e.g. rnorm(k*p) under the same seed -- so the engine
 * needs no RNG and reproduces the reference's chain.  The hyper-prior draws (update_v_lambda / update_v_mu) stay with the
 * caller, who passes their current values in v_lambda / v_mu. */
int fmx_mcmc_vsweep(fmx_engine* e, fmx_matrix* m, double* error, double alpha, const double* v_lambda,
                    const double* v_mu, const double* std_normals);

/* Both sweeps with the residual RESIDENT on the engine's device (what a learner's loop and bench.py --solver als / mcmc use: no
 * host transfer per sweep): dev_error_f64 f64[n], updated in place; dev_std_normals_f64 f64[k][p] (element (f, j) at f*p + j) or
 * NULL for the ALS form.  v_lambda / v_mu stay host pointers (k scalars).  Returns when the sweep has finished. */
int fmx_vsweep_device(fmx_engine* e, fmx_matrix* m, void* dev_error_f64, double alpha, const double* v_lambda, const double* v_mu,
                      const void* dev_std_normals_f64);

/* The exact sweeps process the features in LEVELS (features of a level share no row, levels in ascending order reproduce the
 * reference's index-order Gauss-Seidel): how many levels (or, with cfg.als_max_levels exceeded, groups of the approximate
 * form: `approximate` = 1; with cfg.als_max_levels = -1 or -2, colours of the coloured order: `approximate` = 2, or 3 when the V sweep of a -2 plan nests feature-major -- light lists of at most 1 024 rows; 2 there means it nests factor outer, as -1) this matrix needs, the size of the largest, and every
 * feature's level / group / colour. */
int fmx_als_plan_info(fmx_engine* e, fmx_matrix* m, int64_t* levels, int64_t* largest_level, int32_t* approximate,
                      int32_t* level_of_feature /* [p] or NULL */);
/* Wide levels of an exact plan (every feature of the level holds at most 4096 entries, at least 2048 features: the fields of one-column-per-
 * field data) are swept in a ROW-TILED form on matrices of 2 M rows or more (fm_als_tiled.hip: per-tile sums against an L2-resident slice of
 * the (q, e) pairs, the coordinate steps, a row-major correction pass) instead of walking CSC columns against the whole table.  Same
 * arithmetic per entry; the two sums of a coordinate step associate differently (1e-10 against the column-walking form).  Reports how many
 * levels take that form (0: none), the rows per tile and the number of tiles; builds the plan if need be.  FMX_ALS_TILED=0 / 1 in the
 * environment forbids / forces the form wherever a level qualifies (1: any size, any width -- tests), FMX_ALS_TILE_ROWS sets the tile. */
int fmx_als_tiled_info(fmx_engine* e, fmx_matrix* m, int32_t* levels_tiled, int64_t* tile_rows, int32_t* n_tiles);
/* A COMPLETE tiled plan -- every level of the plan is a tiled one and every row holds exactly one feature of every level: one-column-per-field data, BASELINE.json
 * configs[4]'s shape -- lets the V sweep keep the (q, e) pairs physically in the list order of the level that consumes them next (the LEVEL-ORDER form,
 * fm_als_tiled.hip): per level one kernel streams the pairs, sums the lists and takes the coordinate steps (no per-tile partial sums), one kernel applies the
 * corrections and writes every pair to its place in the next level's order (a permutation inside the tile's L2-resident slice: the one random 16-byte access
 * per stored nonzero that is left).  Same arithmetic per entry as the other forms, sums associated in (tile, entry) order: 1e-10 against them and the oracle,
 * bitwise run to run.  Where, in addition, every feature's list fits a block of 8 192 rows (6 144 with real values), the sweep takes the BLOCK form
 * (fm_als_blocks.hip): the level's array is feature-block-major and ONE kernel per level streams a block's pairs into LDS, sums its lists, takes the coordinate
 * steps, corrects the pairs there and stores them as contiguous runs into the next level's blocks -- the pairs are read once per level and nothing waits for
 * another workgroup (202 against 120 M examples/s at configs[4]).  *level_order = 2: the block form (V sweep and w sweep), 1: the tile form (V sweep; the w sweep keeps the three-pass form), 0: neither.  FMX_ALS_ORDER=1 keeps the tile form, 0 forbids both. */
int fmx_als_order_info(fmx_engine* e, fmx_matrix* m, int32_t* level_order);
/* Opt-in (default off): carry q = X v_f from one V sweep to the next.  The reference recomputes q_f from scratch for every factor of every sweep
 * (solver/MCMC_ALS_Learner.h:283-300); here one forward pass builds it for all factors (38 GB of V-row gathers at configs[4]: 7 of a sweep's 49 ms).  But a sweep
 * itself keeps q current -- every correction of v_fj is applied to the rows' q (:341-350) -- so when a factor's last level is done its pairs hold X v_f for the NEW
 * v_f.  With on = 1 the block form writes that back into the table as the pairs move on, and the next V sweep on the same plan skips the forward pass if the V
 * table is bit for bit what the sweep left (a 64-bit fingerprint; set_params, training steps, another matrix or a rebuilt plan all force the rebuild, as does every
 * 64th sweep, against rounding drift: each carried sweep adds ~1e-16 relative per level).  Results agree with the rebuilt form to ~1e-13: within the 1e-10 of the
 * oracle tests, not bit for bit (the carried q keeps an ABSOLUTE rounding floor of ~1e-16 x the largest |q| since the last rebuild: a sweep that drives q towards zero by
 * many orders of magnitude sees it; ten sweeps at configs[4]: 1e-15 from the rebuilt form, profiles/r05_block_soak.txt).  The feature-major sweep
 * (cfg.als_max_levels = -2) keeps its row-major table current by construction and honours the switch the same way (the key also holds the matrix's value
 * generation: redrawn or rescaled values force the rebuild): 10 M x 1 M, k = 16: 223 -> 259 M examples/s on i.i.d. columns, 334 -> 404 M on field data.  Other
 * forms of the sweep ignore the switch. */
int fmx_als_carry_q(fmx_engine* e, int32_t on);

/* The ALS learner's training loop (MCMC_ALS_Learner::learn, :91-156; REGRESSION): max_iter times { forward; residual;
 * w0 update (:162-188); w sweep (:190-270, the exact one-thread form) }.  As shipped the reference never sweeps V (its
 * update_v call is commented out, :151-155): with_v = 0 reproduces that, with_v = 1 adds the V sweep after the w sweep.
 * The R-side ALS.solver parameters are overridden by learner->init() in the reference and do not enter (alpha = 1,
 * lambdas = 0).  Needs an FMX_MODE_SEQUENTIAL engine (fp64 tables). */
int fmx_als_train(fmx_engine* e, fmx_matrix* m, int32_t max_iter, int32_t with_v);
/* MCMC_ALS_Learner::learn for the MCMC learner (solver/MCMC_ALS_Learner.h:91-156, hyper-parameter draws :359-445), one
 * attribute group, REGRESSION and CLASSIFICATION.  The reference draws from R's generator inside the loop; a library has
 * no access to it, so the CALLER pre-draws, in the reference's call order, per iteration:
 *   std_gammas [max_iter][2]     standard (scale 1) Gamma variates of shape (1 + n)/2 and (1 + p + 1)/2
 *                                (update_alpha, update_w_lambda: Rf_rgamma(a, s) == s * such a variate),
 *   std_normals[max_iter][2 + p] standard normals for w0, w_mu and w[0..p)  (Rf_rnorm(m, s) == m + s * z).
 * Under R:  set.seed(s); for (it in 1:max_iter) { g1 <- rgamma(1, (1+n)/2); z0 <- rnorm(1); g2 <- rgamma(1, (2+p)/2);
 * zmu <- rnorm(1); zw <- rnorm(p) }  reproduces the reference's chain (slots of switched-off updates are not drawn).
 * The CLASSIFICATION residual subtracts truncated normals drawn from libc rand() row by row, as the reference does
 * (util/Random.h:20-93; one host thread).  V is never updated, as shipped (SURVEY A-1).  state_out[3]: alpha, w_lambda, w_mu. */
int fmx_mcmc_train(fmx_engine* e, fmx_matrix* m, int32_t max_iter, const double* std_gammas, const double* std_normals, double* state_out);

/* The same chain continued: state_io[3] = {alpha, w_lambda, w_mu} on entry (what an earlier call returned) and on return.  Lets the
 * caller interleave evaluations with iterations -- the tracker block of MCMC_ALS_Learner::learn (:96-125) is, per record point,
 * fmx_evaluate(...) followed by fmx_mcmc_train_from(e, m, 1, gammas + 2*it, normals + (2+p)*it, state). */
int fmx_mcmc_train_from(fmx_engine* e, fmx_matrix* m, int32_t max_iter, const double* std_gammas, const double* std_normals, double* state_io);
/* V hyper-priors of the MCMC / ALS learners: update_v_lambda then update_v_mu (solver/MCMC_ALS_Learner.h:448-517; in the shipped
 * code their caller is commented out together with the V sweep, :151-155), one attribute group.  v_lambda, v_mu: f64[k] in/out
 * (what fmx_mcmc_vsweep / fmx_als_vsweep take).  sample != 0 (MCMC): std_gammas[k] standard Gamma variates of shape (2 + p)/2,
 * std_normals[k] standard normals, in factor order -- under R: g <- rgamma(k, (2+p)/2); z <- rnorm(k).  sample == 0 (ALS): the
 * means, no variates.  The shipped update_v_mu sums v(f, attr_group[i]) instead of v(f, i) (:462): kept. */
int fmx_mcmc_v_hyper(fmx_engine* e, const double* std_gammas, const double* std_normals, double* v_lambda, double* v_mu, int32_t sample);

/* ---- row selection on the device: one matrix derived from another -- a row gather, hold-out and k-fold assignment, the rows
 * of one part, a hold-out of entries inside rows, an epoch shuffle.  All of it is integer work and copied bits: tests/split_model.py restates every
 * call in numpy and the outputs are equal to it bit for bit.
 *
 * The keys.  mix64 is splitmix64's finaliser; in wrapping 64-bit arithmetic
 *     H(seed, salt, t, stream) = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15) ^ (salt * 0xD6E8FEB86659FD93 + stream)) ^ (t + 0x632BE59BD9B4E019))
 * (the pair sampler's construction).  key_row(r) = H(seed, salt, r, 0) with r the absolute row index, key_group(g) = H(seed, salt, g, 1),
 * key_entry(r, c) = H(seed, salt, (r << 32) | c, 2) with c the column id; the epoch permutation uses H(seed, epoch, r, 3). */

/* Row t of *out is row rows[t] of m: its entries in the source's order, column ids, value bits and label bits copied.  Any order, repeats allowed
 * (bootstrap), n_take may exceed the source's rows, n_take == 0 gives a valid matrix of no rows.  *out has m's feature count and device, labels iff m
 * has them, a new identity and no plans.  An id outside [0, rows of m) is refused with FMX_ERR_INVALID and *out = NULL (the device form finds it in the
 * pass that reads the row lengths; the flag comes back with the entry count in one read).  A source with a field layout (the field generators,
 * fmx_matrix_set_fields) hands it and its flags on -- every multiset of its rows satisfies it --, any other output goes through the detector every
 * upload goes through.  Flags never change a result.  dev_rows_i64: i64[n_take] on m's device. */
int fmx_matrix_take(const fmx_matrix* m, const int64_t* rows /* host i64[n_take] */, int64_t n_take, fmx_matrix** out);
int fmx_matrix_take_device(const fmx_matrix* m, const void* dev_rows_i64, int64_t n_take, fmx_matrix** out);

/* A part id per row, from n, the rows' groups and the spec alone (no matrix is involved).
 *   scope   FMX_SPLIT_ROWS            the items are the rows, in one segment
 *           FMX_SPLIT_WITHIN_GROUPS   the items are the rows, a segment is a group's rows (stratified splits; leave-k-out per user)
 *           FMX_SPLIT_GROUPS          the items are the group ids 0 .. n_groups-1 in one segment, empty groups included; a row takes its group's part
 *                                     (no user on both sides)
 *   order   FMX_SPLIT_ORDER_HASH      items ascend by (key_row(r), r) -- scope GROUPS: (key_group(g), g) -- inside their segment
 *           FMX_SPLIT_ORDER_TAIL      by the item index DESCENDING: the last rows of a segment come first (temporal hold-out)
 * An item of 0-based rank rho in a segment of s items gets
 *   hold-out (n_folds == 0)   c = hold_count > 0 ? hold_count : (int64) floor(hold_fraction * (double) s)   (one rounded fp64 product),
 *                             q = min(c, max(s - min_keep, 0)), part = rho < q ? 1 (held) : 0 (kept)
 *   folds (2 .. 65536)        part = floor(rho * n_folds / s) in exact integers: fold sizes inside a segment differ by at most one.
 * The parts are a function of (n, groups, spec) alone.  Under WITHIN_GROUPS a row's part depends only on its own group's set of row indices -- not on the
 * other groups, n_groups or the numbering of the ids; under hold-out the held set of a smaller hold_count is a subset of a larger one's; under GROUPS
 * the groups' parts depend on (n_groups, spec) only.
 * group_of_row NULL needs scope ROWS (n_groups is then ignored; with scope ROWS given groups are not read beyond the host form's range check).  The host
 * form refuses an id >= n_groups; the device form cannot: such a row gets part 0xFFFFFFFF and belongs to no segment, as fmx_metrics_device treats it.
 * 0 <= n <= 2^31 - 1, 1 <= n_groups <= 2^31 - 1.  Every refusal -- a NULL spec or output, a wrong struct_size, a scope or order out of range, n_folds
 * of 1 or above 65536, a negative count or min_keep, a fraction outside [0, 1] or NaN -- is FMX_ERR_INVALID before any device is touched and before
 * any output is written. */
#define FMX_SPLIT_ROWS 0
#define FMX_SPLIT_WITHIN_GROUPS 1
#define FMX_SPLIT_GROUPS 2
#define FMX_SPLIT_ORDER_HASH 0
#define FMX_SPLIT_ORDER_TAIL 1
typedef struct fmx_split_spec {
  uint32_t struct_size;   /* sizeof(fmx_split_spec) */
  int32_t scope;
  int32_t order;
  int32_t n_folds;        /* 0: hold-out (parts 0 = kept, 1 = held); 2 .. 65536: folds 0 .. n_folds-1 */
  int64_t hold_count;     /* > 0: items held per segment; 0: use hold_fraction */
  double hold_fraction;   /* in [0, 1]; NaN refused */
  int64_t min_keep;       /* >= 0: items a segment always keeps */
  uint64_t seed, salt;
} fmx_split_spec;
int fmx_split_assign(int device, int64_t n, const uint32_t* group_of_row /* host u32[n] or NULL */, int64_t n_groups, const fmx_split_spec* spec,
                     uint32_t* out_part /* host u32[n] */);
int fmx_split_assign_device(int device, int64_t n, const void* dev_group_u32, int64_t n_groups, const fmx_split_spec* spec, void* dev_part_u32);

/* The rows r of m with part[r] == which, in ascending r; with complement != 0 the rows with part[r] != which and part[r] != 0xFFFFFFFF.  A stream
 * compaction into a row list, then fmx_matrix_take's gather: fold f's test set is (which = f, complement = 0), its train set (f, 1).
 * The source rows of *out.  The device form hands them back as a device buffer of i64[rows of *out] in *dev_rows_i64 (pass NULL if not wanted), which
 * the caller releases with fmx_free_device -- the only buffer this library allocates for a caller.  The host form copies them into out_rows (NULL: not
 * wanted), which needs room for the rows of *out: at most the rows of m, so a caller who does not know the count passes i64[rows of m] and reads the
 * count from fmx_matrix_info(*out). */
int fmx_matrix_select(const fmx_matrix* m, const uint32_t* part_of_row /* host u32[rows of m] */, uint32_t which, int32_t complement, fmx_matrix** out,
                      int64_t* out_rows);
int fmx_matrix_select_device(const fmx_matrix* m, const void* dev_part_u32, uint32_t which, int32_t complement, fmx_matrix** out, void** dev_rows_i64);
/* releases a device buffer that fmx_matrix_select_device returned (NULL: nothing to do) */
int fmx_free_device(void* dev_ptr);

/* Hold out entries INSIDE rows -- for positives-shaped matrices (contexts x items).  A segment is a row, the items its stored entries at positions i;
 * the order is (key_entry(r, c_i), i) ascending, with FMX_SPLIT_ORDER_TAIL i descending; the quota is fmx_split_assign's hold-out quota with s = the
 * row's stored entries.  Both outputs have m's rows and feature count, and its labels if any; every entry of m goes to exactly one of them, in source
 * order inside its row, value bits copied.  A column stored twice in a row has equal keys: position decides.  At most 2^31 - 1 rows and entries. */
int fmx_matrix_split_entries(const fmx_matrix* m, int32_t order, int64_t hold_count, double hold_fraction, int64_t min_keep, uint64_t seed, uint64_t salt,
                             fmx_matrix** out_kept, fmx_matrix** out_held);

/* out[t] = the row at position t when 0 .. n-1 ascend by (H(seed, epoch, r, 3), r): a permutation, another epoch another order.  Feed it to
 * fmx_matrix_take for an epoch shuffle.  0 <= n <= 2^31 - 1. */
int fmx_row_permutation(int device, int64_t n, uint64_t seed, uint64_t epoch, int64_t* out_rows /* host i64[n] */);
int fmx_row_permutation_device(int device, int64_t n, uint64_t seed, uint64_t epoch, void* dev_rows_i64);

/* ---- column selection on the device: one matrix derived from another along the COLUMNS -- how often every feature occurs,
 * a map from old to new feature ids (pruning with an optional rare-value bucket per segment, or hashing), and the matrix under such a map.
 * tests/columns_model.py restates every call in numpy; counts, maps and the remapped matrix are equal to it bit for bit, and so are the two sums,
 * whose order is fixed below.  No call uses a floating-point atomic.  At most 2^31 - 1 rows and stored entries per call.  Every refusal named
 * below is FMX_ERR_INVALID before any device is touched and before any output is written; a matrix output is *out = NULL on every refusal. */

/* Per column j of m:
 *   count[3 j + 0]  entries        the stored entries with column j
 *   count[3 j + 1]  rows           the rows that store j at least once (a column stored twice in a row counts once)
 *   count[3 j + 2]  positive rows  those rows whose label is > 0; all zero for a matrix without labels
 *   value[2 j + 0]  sum            of (double) x over the column's entries
 *   value[2 j + 1]  sum_sq         of (double) x * (double) x (one rounded fp64 product each)
 * value may be NULL.  THE ORDER OF THE SUMS.  The column's entries in ascending (row, position in the row) order form a list; it is cut into
 * chunks of 1 024 positions.  Inside a chunk, lane l of 64 adds the terms at positions l, l + 64, l + 128, ... in that order from +0.0; the 64 lane
 * sums meet in an xor butterfly, v[l] = v[l] + v[l ^ s] for s = 32, 16, 8, 4, 2, 1; the chunk sums are added in ascending order from +0.0.  Every
 * step is one rounded fp64 addition.  A column's sums therefore depend on its own entry list alone -- not on the other columns, the launch cuts or
 * the call -- and on one-hot data (every value 1.0f) both are exactly (double) entries.  A one-hot source with strictly ascending rows is counted
 * without a sort; everything else goes through a stable sort of (column, entry index).  Both give the same bits on the same data. */
int fmx_matrix_column_stats(const fmx_matrix* m, int64_t* count /* host i64[p][3] */, double* value /* host f64[p][2] or NULL */);
int fmx_matrix_column_stats_device(const fmx_matrix* m, void* dev_count_i64, void* dev_value_f64);

/* A map from old to new feature ids out of a count table (fmx_matrix_column_stats') and a rule, in integers alone: the map is a function of
 * (count, rule).  c_j is count[3 j + 1] under FMX_COLUMNS_BY_ROWS, count[3 j + 0] under FMX_COLUMNS_BY_ENTRIES.
 *   survivors   a column j >= keep_prefix survives iff min_count <= c_j and (max_count == 0 or c_j <= max_count).  If max_features > 0 and more
 *               columns than that survive, only the max_features with the largest c_j do, ties to the lower id (c_j is clamped to 0 .. 2^32 - 1 for
 *               this order alone).  Columns below keep_prefix (the dense columns) always survive and are outside the cap.
 *   numbering   segment by segment (segment s = [segment_base[s], segment_base[s + 1]); n_segments == 0: one segment [0, p)): the segment's
 *               survivors take consecutive new ids in ascending old id; under FMX_RARE_BUCKET the segment then gets exactly one further id, its
 *               bucket, whether or not anything maps to it, and every other column of the segment maps to it; under FMX_RARE_DROP every other
 *               column maps to 0xFFFFFFFF.
 *   outputs     map u32[p]; *new_p the new feature count; new_segment_base u32[max(n_segments, 1) + 1] (NULL: not wanted) the segments' new
 *               ranges -- with a matrix's field bases as segments a field-layout matrix keeps one id per field under BUCKET, and
 *               new_segment_base is what fmx_matrix_set_fields takes for the remapped matrix.
 * segment_base is a host array in both forms, ascending (an empty segment is allowed) from 0 to p.  Refused: a NULL rule, count, map or new_p, a
 * wrong struct_size, by or rare out of range, a negative bound, reserved != 0, keep_prefix > p, a segment_base that does not start at 0, end at p
 * or ascend, p + max(n_segments, 1) above 2^32 - 2.  new_p and new_segment_base are host outputs in both forms. */
#define FMX_COLUMNS_BY_ROWS 0
#define FMX_COLUMNS_BY_ENTRIES 1
#define FMX_RARE_DROP 0
#define FMX_RARE_BUCKET 1
typedef struct fmx_column_rule {
  uint32_t struct_size;    /* sizeof(fmx_column_rule) */
  int32_t by;
  int64_t min_count;
  int64_t max_count;       /* 0: no upper bound */
  int64_t max_features;    /* 0: no cap */
  uint32_t keep_prefix;
  int32_t rare;
  int32_t n_segments;      /* 0: one segment [0, p) */
  int32_t reserved;        /* 0 */
  const uint32_t* segment_base;   /* host u32[n_segments + 1], or NULL with n_segments == 0 */
} fmx_column_rule;
int fmx_column_map_select(int device, uint32_t p, const int64_t* count /* host i64[p][3] */, const fmx_column_rule* rule, uint32_t* map /* host u32[p] */,
                          uint32_t* new_p, uint32_t* new_segment_base);
int fmx_column_map_select_device(int device, uint32_t p, const void* dev_count_i64, const fmx_column_rule* rule, void* dev_map_u32, uint32_t* new_p,
                                 uint32_t* new_segment_base);

/* The hashing trick: map[j] = j for j < keep_prefix, otherwise keep_prefix + mulhi64(H(seed, salt, j, 4), n_buckets) with the row selection's H
 * (stream 4) and mulhi64(a, b) = floor(a b / 2^64), the pair sampler's rule.  *new_p = keep_prefix + n_buckets.  Refused: n_buckets == 0,
 * keep_prefix > p, keep_prefix + n_buckets above 2^32 - 2, a NULL map or new_p.  Unsigned: there is no sign hash. */
int fmx_column_map_hash(int device, uint32_t p, uint32_t n_buckets, uint64_t seed, uint64_t salt, uint32_t keep_prefix, uint32_t* map /* host u32[p] */,
                        uint32_t* new_p);
int fmx_column_map_hash_device(int device, uint32_t p, uint32_t n_buckets, uint64_t seed, uint64_t salt, uint32_t keep_prefix, void* dev_map_u32, uint32_t* new_p);

/* m under a map u32[m's feature count]: *out has m's rows, device and label bits (labels iff m has them), feature count new_p, a new identity and
 * no plans.  An entry of column c gets the id map[c]; 0xFFFFFFFF removes it.  A map value that is neither below new_p nor 0xFFFFFFFF is refused
 * whether or not its column occurs (the device form finds the lowest such column in its first pass; the flag comes back with the entry total in
 * one read).
 *   FMX_COMBINE_KEEP    the remaining entries stay in source order, id relabelled, value bits copied; duplicates stay two entries.
 *   FMX_COMBINE_SUM     a row's remaining entries ascend strictly by new id; entries of equal new id become one entry whose value is
 *                       (float) (((double) x_1 + (double) x_2) + ...) in source order: every fp64 addition rounded, then one rounding to fp32.
 *   FMX_COMBINE_FIRST   the same order and merge; the value is the bits of the first entry in source order (a one-hot matrix stays one-hot).
 * SUM and FIRST sort (new id << 32 | position in the row) inside every row; short rows take a lane-group form and long rows a segmented sort,
 * with the same bits.  The output goes through the detector every upload goes through: no flag is copied from the source. */
#define FMX_COMBINE_KEEP 0
#define FMX_COMBINE_SUM 1
#define FMX_COMBINE_FIRST 2
#define FMX_COLUMN_DROP 0xFFFFFFFFu
int fmx_matrix_remap_columns(const fmx_matrix* m, const uint32_t* map /* host u32[features of m] */, uint32_t new_p, int32_t combine, fmx_matrix** out);
int fmx_matrix_remap_columns_device(const fmx_matrix* m, const void* dev_map_u32, uint32_t new_p, int32_t combine, fmx_matrix** out);

/* ---- matrix composition on the device: one matrix built out of several -- blocks joined side by side by row index, parts
 * stacked one under the other.  An interaction table (user, item, label) and two side tables, one row per user and one per item, become FM rows
 * [onehot(user) | onehot(item) | U[user] | I[item]] without a trip through the host.  All of it is integer work and copied bits:
 * tests/join_model.py restates both calls in numpy and the outputs are equal to it bit for bit. */

/* JOIN.  Row t of *out holds, for b = 0 .. n_blocks-1 in that order, the entries of row rows_b[t] of block b: in the source's order, every column
 * id + col_base_b, value bits copied.  An INDICATOR block (m == NULL) contributes the single entry (col_base_b + rows_b[t], 1.0f).  Repeats and any
 * order of ids are allowed; a column that two blocks both store appears twice (col_base = 0 on a shared feature count is the concatenation
 * fmx_topk scores and fmx_matrix_pairs forms); n_out == 0 gives a valid matrix of no rows.  *out has out_p features, lives on `device`, has a new
 * identity and no plans, and has labels iff labels_from >= 0: the label bits of row rows_b[t] of block b = labels_from.
 * Refused with FMX_ERR_INVALID and *out = NULL -- before any device is touched: a NULL argument, n_blocks outside 1 .. FMX_JOIN_MAX_BLOCKS, a
 * negative n_out or n_ids, a block without a row list (the identity) whose source does not hold exactly n_out rows or that is an indicator block,
 * labels_from outside -1 .. n_blocks-1 or naming an indicator block or a source without labels; before any launch: col_base_b + the features of
 * block b (an indicator: n_ids) above out_p, in 64 bits, and a source on another device than `device`.  An id outside its block's range -- [0,
 * rows of the source), an indicator's [0, n_ids) -- is found, in both forms, by the pass that reads the row lengths: the message names the lowest
 * position t and, at that position, the lowest block; the flag comes back with the entry count in one read, as in fmx_matrix_take.  A joined row of
 * more than 2^31 - 1 entries is refused.
 * FLAGS.  When every block is an indicator block or has a field layout (the field generators, fmx_matrix_set_fields, the detector), the shifted
 * ranges [col_base_b, col_base_b + features of b) ascend with b without overlap, and only block 0 has a dense prefix, and only with col_base 0,
 * the output is handed a field layout without going through the detector: the blocks' field bases concatenated, an indicator block being one field
 * (the first base is the dense prefix, the last out_p), the row length the sum, rows_sorted / unit_values the conjunction.  Every other output goes
 * through the detector every upload goes through.  Flags never change a result. */
#define FMX_JOIN_MAX_BLOCKS 16
typedef struct fmx_join_block {
  const fmx_matrix* m;   /* source matrix, or NULL: an INDICATOR block (one entry per row: column col_base + rows[t], value 1.0f) */
  const void* rows;      /* i64[n_out]: host in fmx_matrix_join, device in fmx_matrix_join_device; NULL = identity (needs a source of exactly n_out rows; refused for an indicator block) */
  int64_t n_ids;         /* indicator blocks: ids lie in [0, n_ids); ignored when m != NULL */
  uint32_t col_base;     /* added to every column id the block contributes */
} fmx_join_block;
int fmx_matrix_join(int device, const fmx_join_block* blocks, int32_t n_blocks, int64_t n_out, uint32_t out_p, int32_t labels_from, fmx_matrix** out);
int fmx_matrix_join_device(int device, const fmx_join_block* blocks, int32_t n_blocks, int64_t n_out, uint32_t out_p, int32_t labels_from, fmx_matrix** out);

/* STACK.  The rows of part 0, then part 1, and so on: row pointers rebased, column ids, value bits and label bits copied.  1 <= n_parts <= 1024;
 * all parts share the feature count and the device.  *out has labels iff every part has them.  A field layout is handed on iff all parts carry the
 * identical one; every other output goes through the detector.  Refused with FMX_ERR_INVALID and *out = NULL before any device is touched: a NULL
 * argument or part, n_parts out of range, differing feature counts or devices, parts with and without labels. */
int fmx_matrix_stack(const fmx_matrix* const* parts, int32_t n_parts, fmx_matrix** out);

/* ---- value binning on the device: dense columns become one-hot buckets.  A factorization machine sees a numeric feature x
 * only as w x and x <v, .>; binned, the feature is one id per bucket with its own w and v.  The fit finds equal-mass (quantile) edges, the apply
 * replaces the chosen columns by bucket ids.  Values are only ever compared, through one 32-bit order key: no floating-point arithmetic anywhere.
 * tests/bins_model.py restates both calls in numpy and the outputs are equal to it bit for bit.
 *
 * THE ORDER OF VALUES.  vkey(x): the float's bits with -0 taken as +0; a set sign bit gives the complement, otherwise the bits with the top bit
 * set; every NaN of either sign gives 0xFFFFFFFF, above +inf's 0xFF800000.  Ascending in vkey is ascending in x, NaN last. */

/* FIT.  For column slot s (column cols[s]): L = the non-NaN STORED values of the column, -0 read as +0, ascending by vkey; cnt = |L|.  The candidates
 * are L[floor(b cnt / n_bins)] for b = 1 .. n_bins-1, in 64-bit integers; the edges are the distinct candidates that are > L[0], ascending.
 * lo = L[0], hi = L[cnt - 1]; with cnt == 0 there are no edges and lo = hi = +0.0.  Absent entries are not zeros: only stored entries are binned.  A
 * unit_values source is read as 1.0f.
 *   cols     host u32[n_cols], strictly ascending, each below m's feature count
 *   edges    host f32[n_cols][n_bins - 1], row s padded with +0.0 behind n_edges[s]
 *   n_edges  host i32[n_cols]
 *   count    host i64[n_cols][2] = {non-NaN stored entries, NaN entries}
 *   range    host f32[n_cols][2] = {lo, hi}
 * What follows from the definition: at most n_bins - 1 edges, strictly ascending, none NaN; under bin(x) = #{e : e <= x} every bin holds at least
 * one fitting entry, equal values share a bin, and the bin is monotone in x; without ties no bin holds more than ceil(cnt / n_bins) entries; the
 * assignment is unchanged by any strictly increasing map of the values (no log transform is needed before quantile bins); a column's outputs depend
 * on its own multiset of values alone -- not on the other columns, the row order, the launch cuts or the call.
 * 1 <= n_bins <= 65 536; at most 2^31 - 1 stored entries.  Refused with FMX_ERR_INVALID before any device is touched, every output untouched: a NULL
 * argument (edges may be NULL only with n_bins == 1), n_cols < 0, n_bins out of range, cols not strictly ascending or out of range.
 * There is no _device form: every input and output besides the matrix is a few kilobytes of host data. */
int fmx_matrix_column_quantiles(const fmx_matrix* m, const uint32_t* cols, int32_t n_cols, int32_t n_bins, float* edges, int32_t* n_edges, int64_t* count,
                                float* range);

/* APPLY.  Edges from the fit or from the caller (width, log-spaced, hand-made bins).  An unbinned column j has width 1, the binned column of slot s
 * width n_edges_s + 2: n_edges_s + 1 bins and one id for NaN, which exists whether or not anything maps to it (as the rare-value bucket of
 * fmx_column_map_select does).  new_base u32[p + 1] is the exclusive prefix sum of the widths, new_base[p] the output's feature count: binned columns
 * expand in place.  *out has m's rows, row pointers, label bits, device and entry order; entry (c, x) becomes
 *   unbinned c             (new_base[c], x) with x's bits copied
 *   binned c, x not NaN    (new_base[c] + #{e : e <= x}, 1.0f)
 *   binned c, x NaN        (new_base[c] + n_edges_c + 1, 1.0f)
 * A column stored twice in a row gives two entries (fmx_matrix_remap_columns(..., FMX_COMBINE_FIRST) merges them).  *out has a new identity and no
 * plans and goes through the detector every upload goes through: no flag is copied.  new_base restricted to the binned columns and the field bases is
 * what fmx_matrix_set_fields takes.
 * Refused with FMX_ERR_INVALID before any device is touched, *out = NULL and new_base untouched: a NULL argument, a wrong struct_size, reserved != 0,
 * cols not strictly ascending or out of range, an edge_offset that does not start at 0 or does not ascend, an edge that is NaN, edges not strictly
 * ascending, more than 65 535 edges in a column, the widths summing above 2^32 - 2.  There is no _device form, for the fit's reason. */
typedef struct fmx_bin_spec {
  uint32_t struct_size;         /* sizeof(fmx_bin_spec) */
  int32_t n_cols;
  const uint32_t* cols;         /* host u32[n_cols], strictly ascending */
  const int64_t* edge_offset;   /* host i64[n_cols + 1], from 0, ascending */
  const float* edges;           /* host f32[edge_offset[n_cols]]: per column strictly ascending under <, no NaN; +-inf allowed */
  int64_t reserved;             /* 0 */
} fmx_bin_spec;
int fmx_matrix_bin_columns(const fmx_matrix* m, const fmx_bin_spec* spec, uint32_t* new_base /* host u32[p + 1] */, fmx_matrix** out);

/* ---- feature crosses on the device: pairs of entries of two column segments get ids of their own.  A degree-2 FM gives the
 * pair (a, b) only the rank-k term <v_a, v_b>; crossed, the pair is a feature with its own w and v -- a full-rank correction for the field pairs that
 * need one, and third-order effects through <v_ab, v_c>.  Ids are integer work and the value is the IEEE binary32 product, so tests/cross_model.py
 * restates the call in numpy and the output is equal to it bit for bit.
 *
 * SEGMENTS.  segment_base u32[n_segments + 1] cuts the columns [0, p) into segments [base[s], base[s + 1]), empty ones allowed: the fields of one-hot
 * data, a dense column each, the columns fmx_matrix_bin_columns made of one.  width(s) = base[s + 1] - base[s].
 * ENTRIES.  For row r and segment s, E_s = the row's stored entries whose column lies in the segment, in source order.  A column stored twice is two
 * entries; rows need not be sorted.
 * PAIRS.  Term t = (a, b), a < b, emits one entry per (i, j) in E_a x E_b, i-major: i ascending, then j ascending.  A self-cross (a == b) emits one
 * entry per pair of positions i < j of E_a, i-major.
 * IDS.  u = col_i - base[a], v = col_j - base[b]; a self-cross takes (u, v) := (min, max), so the id does not depend on the storage order.  The
 * term's width W_t is n_buckets if that is > 0, otherwise width(a) * width(b) in 64 bits.  The exact id is cross_base[t] + u * width(b) + v, the
 * hashed id cross_base[t] + mulhi64(H(seed, salt, u << 32 | v, 128 + t), n_buckets) with the H and mulhi64 of fmx_column_map_hash.
 * VALUE.  The IEEE binary32 product x_i * x_j, rounded once, subnormals kept; every NaN result is 0x7FC00000.  A unit_values source reads as 1.0f, so
 * a one-hot source gives a one-hot output.
 * OUTPUT.  cross_base[0] = keep_source ? p : 0, cross_base[t + 1] = cross_base[t] + W_t, and cross_base[n_terms] is the output's feature count.  A
 * row of *out is the source row (bits copied; only with keep_source), then the terms in order.  *out has m's rows, device and label bits, a new
 * identity and no plans, and goes through the detector every upload goes through: no flag is copied.  segment_base followed by cross_base[1 ..] is a
 * valid segment list of the output (with keep_source): what a second cross -- a triple is a cross of a crossed segment --, fmx_column_map_select and
 * fmx_matrix_set_fields take.  A row's output depends on that row and the spec alone: not on other rows, the launch cuts or the call.
 * Refused with FMX_ERR_INVALID before any device is touched, *out = NULL and cross_base untouched: a NULL argument, a wrong struct_size, reserved != 0
 * in the spec or a term, n_segments outside 1 .. 4096, n_terms outside 1 .. 64, keep_source neither 0 nor 1, a segment_base that does not start at
 * 0, end at m's feature count or ascend, a term with seg_a > seg_b or a segment index out of range, the widths (p under keep_source, and every W_t)
 * summing above 2^32 - 2, counted in 64 bits.  An output row or an output of more than 2^31 - 1 entries is found by the pass that reads the row
 * lengths -- the flag comes back with the total in one read, as in fmx_matrix_take -- and the message names the lowest such row.
 * There is no _device form, for the reason fmx_matrix_bin_columns has none. */
typedef struct fmx_cross_term {
  uint32_t seg_a, seg_b;        /* seg_a <= seg_b; equal: a self-cross */
  uint32_t n_buckets;           /* 0: exact ids; > 0: hashed into that many */
  uint32_t reserved;            /* 0 */
} fmx_cross_term;
typedef struct fmx_cross_spec {
  uint32_t struct_size;         /* sizeof(fmx_cross_spec) */
  int32_t n_segments;           /* 1 .. 4096 */
  const uint32_t* segment_base; /* host u32[n_segments + 1], ascending from 0 to p, empty segments allowed */
  int32_t n_terms;              /* 1 .. 64 */
  int32_t keep_source;          /* 1: source entries first, then the crosses; 0: crosses only */
  const fmx_cross_term* terms;  /* host [n_terms] */
  uint64_t seed, salt;
  int64_t reserved;             /* 0 */
} fmx_cross_spec;
int fmx_matrix_cross(const fmx_matrix* m, const fmx_cross_spec* spec, uint32_t* cross_base /* host u32[n_terms + 1] */, fmx_matrix** out);

/* ---- target and count encoding on the device: a high-cardinality field becomes one or two dense columns -- MEAN, the smoothed
 * target rate of the id a row carries, and COUNT, how often that id was seen.  Fitted on the rows it is applied to, MEAN leaks the label; the fit
 * therefore keeps its statistics per PART (the folds of fmx_split_assign) and the apply leaves a row's own part out.  Every output is integers, copied
 * bits or floating-point arithmetic in one stated order, so tests/target_model.py restates both calls in numpy and the device is equal to it bit for bit.
 *
 * SEGMENTS as in fmx_matrix_cross.  TERMS: term_segment u32[n_terms], strictly ascending segment indices -- the encoded fields.
 * SLOTS.  term_base[0] = 0, term_base[t + 1] = term_base[t] + width(term_segment[t]); the slot of column c of term t is
 * term_base[t] + c - segment_base[term_segment[t]], and W = term_base[n_terms].  W * n_parts <= 2^31 - 1.
 *
 * ---- the fit: fmx_target_stats.  part: u32[rows], or NULL -- every row is part 0.  A row whose part is >= n_parts (FMX_SPLIT_NO_PART among them) is
 * counted nowhere.  A CELL is one (slot, part).  rows = the rows of the part that store the column at least once (a column stored twice in a row counts
 * once), positive rows = those of them with label > 0, and under FMX_TARGET_LABEL sum = the (double) labels of the cell's rows added in ascending row
 * order in the order of fmx_matrix_column_stats -- chunks of 1 024 positions of the cell's row list, lane strides of 64 from +0.0, the xor butterfly
 * 32 .. 1, the chunk sums ascending from +0.0.  A sum that is a NaN is stored as 0x7FF8000000000000.  A cell's bits depend on its own row list alone:
 * not on the other cells, the launch cuts or the form the call took (a one-hot source with strictly ascending rows under FMX_TARGET_POSITIVE is counted
 * with 64-bit integer atomics, everything else by a sort of (slot * n_parts + part, entry index); no floating-point atomic anywhere).
 * The table is an opaque fmx_target_table on m's device (for 33 M ids and 5 parts it is gigabytes: it does not pass through the host between the
 * fit and the apply).  It keeps its layout: segment_base, term_segment, n_parts, target.
 * EXPORT AND IMPORT, one layout both ways: count i64[W][n_parts][2] = {rows, positive rows}; sum f64[W][n_parts] (FMX_TARGET_LABEL only: export
 * leaves it untouched and from_arrays ignores it under FMX_TARGET_POSITIVE).  from_arrays copies the bits it is given; fmx_target_table_export takes
 * NULL for what is not wanted.
 * Refused with FMX_ERR_INVALID before any device is touched, *out = NULL: a NULL argument, a wrong struct_size, reserved != 0, n_segments outside
 * 1 .. 4096, n_terms or n_parts outside 1 .. 64, a segment_base that does not start at 0, end at m's feature count or ascend, a term_segment that does
 * not ascend strictly or names no segment, an unknown target, a matrix without labels, W * n_parts above 2^31 - 1, in from_arrays a NULL count, or a
 * NULL sum under FMX_TARGET_LABEL.
 *
 * ---- the apply: fmx_matrix_encode_targets.  For row r and term t, E = the row's stored entries whose column lies in the term's segment, in source
 * order (a column stored twice is two entries); an empty E emits nothing.  own := a part array is given and f = part[r] < n_parts.  Per column c:
 * N_c = sum_g rows[c][g], A_c = sum_g positive[c][g] (int64), T_c = the chain of sum[c][g], g ascending, from +0.0 (a NaN: 0x7FF8000000000000).
 *   n   = sum_{e in E} (N_c - (own ? rows[c][f] : 0))                                     int64
 *   a   = (double) sum_{e in E} (A_c - (own ? positive[c][f] : 0))                        FMX_TARGET_POSITIVE: the integer sum first
 *   a   = the chain from +0.0 over E, in source order, of (own ? T_c - sum[c][f] : T_c)   FMX_TARGET_LABEL: the subtraction is one rounded operation
 *   den = (double) n + strength        (the conversion rounds to nearest, the addition once)          pm = prior * strength, one rounded product
 *   MEAN  = den == 0 ? (float) prior : (float) ((a + pm) / den)     one rounded addition, one IEEE fp64 division, one narrowing; a NaN is 0x7FC00000
 *   COUNT = (float) n                                               rounded once from the integer
 * OUTPUT.  enc_base[0] = keep_source ? p : 0, enc_base[t + 1] = enc_base[t] + popcount(kinds[t]); enc_base[n_terms] is the output's feature count.  A
 * row of *out is the source row (bits copied; only with keep_source), then the terms in order, MEAN (column enc_base[t]) before COUNT.  *out has m's
 * rows, device and label bits, a new identity and no plans, and goes through the detector every upload goes through: no flag is copied.  With
 * keep_source, segment_base followed by enc_base[1 ..] is a segment list of the output: what fmx_matrix_set_fields, fmx_matrix_bin_columns and
 * fmx_matrix_cross take.  A row's output depends on that row, its part, the table and the spec alone.  A row without a valid part -- and every row of
 * part == NULL -- is encoded with the totals: the form for validation and serving data.
 * Refused as above, *out = NULL and enc_base untouched: a NULL argument, a wrong struct_size, reserved != 0, keep_source neither 0 nor 1, m's feature
 * count or device different from the table's, a kinds[t] that is 0 or has a bit above FMX_ENCODE_COUNT, a strength that is negative or not finite, a
 * prior that is not finite, the widths (p under keep_source, and the new columns) summing above 2^32 - 2.  An output of more than 2^31 - 1 entries is
 * found by the pass that reads the row lengths (an output row is at most 128 entries longer than its source row). */
#define FMX_TARGET_POSITIVE 0 /* the target of a row is [label > 0] */
#define FMX_TARGET_LABEL 1    /* ... the label itself */
#define FMX_ENCODE_MEAN 1u
#define FMX_ENCODE_COUNT 2u
typedef struct fmx_target_table fmx_target_table;
typedef struct fmx_target_spec {
  uint32_t struct_size;         /* sizeof(fmx_target_spec) */
  int32_t n_segments;           /* 1 .. 4096 */
  const uint32_t* segment_base; /* host u32[n_segments + 1], ascending from 0 to p, empty segments allowed */
  int32_t n_terms;              /* 1 .. 64 */
  const uint32_t* term_segment; /* host u32[n_terms], strictly ascending segment indices: the encoded fields */
  int32_t n_parts;              /* 1 .. 64 */
  int32_t target;               /* FMX_TARGET_POSITIVE or FMX_TARGET_LABEL */
  int64_t reserved;             /* 0 */
} fmx_target_spec;
typedef struct fmx_encode_spec {
  uint32_t struct_size;         /* sizeof(fmx_encode_spec) */
  int32_t keep_source;          /* 1: source entries first, then the encodings; 0: encodings only */
  const uint32_t* kinds;        /* host u32[n_terms]: FMX_ENCODE_MEAN | FMX_ENCODE_COUNT, not 0 */
  double prior, strength;       /* both finite, strength >= 0 */
  int64_t reserved;             /* 0 */
} fmx_encode_spec;
int fmx_target_stats(const fmx_matrix* m, const uint32_t* part /* host u32[rows] or NULL */, const fmx_target_spec* spec, fmx_target_table** out);
int fmx_target_stats_device(const fmx_matrix* m, const void* dev_part_u32 /* or NULL */, const fmx_target_spec* spec, fmx_target_table** out);
int fmx_target_table_from_arrays(int device, const fmx_target_spec* layout, const int64_t* count /* [W][n_parts][2] */,
                                 const double* sum /* [W][n_parts]; NULL under FMX_TARGET_POSITIVE */, fmx_target_table** out);
/* info[8] = device, p, n_segments, n_terms, n_parts, target, W, the bytes of the table on the device */
int fmx_target_table_info(const fmx_target_table* table, int64_t* info /* [8] */);
int fmx_target_table_export(const fmx_target_table* table, uint32_t* segment_base /* [n_segments + 1] */, uint32_t* term_segment /* [n_terms] */,
                            int64_t* count /* [W][n_parts][2] */, double* sum /* [W][n_parts] */);
int fmx_target_table_free(fmx_target_table* table);
int fmx_matrix_encode_targets(const fmx_matrix* m, const fmx_target_table* table, const uint32_t* part /* host u32[rows] or NULL */,
                              const fmx_encode_spec* spec, uint32_t* enc_base /* host u32[n_terms + 1] */, fmx_matrix** out);
int fmx_matrix_encode_targets_device(const fmx_matrix* m, const fmx_target_table* table, const void* dev_part_u32 /* or NULL */,
                                     const fmx_encode_spec* spec, uint32_t* enc_base /* host u32[n_terms + 1] */, fmx_matrix** out);

/* ---- measurement: HIP-event timing of each kernel on the engine's stream (bench.py roofline leg). */
#define FMX_KERNEL_ROWS_FORWARD 0 /* phase 1: V-row gather + forward + grad multiplier */
#define FMX_KERNEL_COLS_UPDATE 1  /* phase 2: per-feature gradient sums + update */
#define FMX_KERNEL_SCALAR 2       /* w0 reduction/update */
#define FMX_KERNEL_SEQ 3          /* sequential-exact learner */
#define FMX_KERNEL_ALS_SWEEP 4    /* one level (or group) of one factor of an ALS / MCMC sweep: als_level_k and its heavy-column forms */
#define FMX_KERNEL_COUNT 8
/* on == 0: off; on == n > 0: time every n-th launch of each kernel (n = 1: all; sampling keeps the events' own cost,
 * a few microseconds of stream time per timed launch, out of the measured throughput). */
int fmx_profile_enable(fmx_engine* e, int on);
int fmx_profile_get(fmx_engine* e, int kernel, double* total_ms, int64_t* launches);
int fmx_profile_reset(fmx_engine* e);
/* Phase 1's request schedule for large steps (>= 65536 rows per launch), which the engine picks by timing its own first 14
 * such launches: *serial = 1 one entry's requests outstanding per lane group, 0 four entries', -1 not decided yet;
 * ms_serial / ms_pipelined = the six timed launches of each.  The choice never changes a result.  FMX_ROWS_SERIAL=0/1 pins it. */
int fmx_rows_tune_info(fmx_engine* e, int32_t* serial, double* ms_serial, double* ms_pipelined);
/* Which form of phase 1 large steps (and large forward passes) take on this matrix: 0 one lane group per row (the product form), 1 the flat form
 * (FMX_ROWS_FLAT=1 on rows of differing lengths: the entries of a block of rows as one stream cut evenly over the lane groups, a row's pieces combined in
 * entry order; replaces the per-row loop of core/Model.h:83-97), 2 lane groups pulling rows (FMX_ROWS_PULL=1).  Forms 1 and 2 are measurement records
 * (both slower, profiles/r04_ragged_forms.txt); form 1 associates a row's sums differently from forms 0 and 2 (same parity bars, other last bits).  Under it a
 * row's bits depend on the matrix it is launched on: the shards of a cfg.n_gpus handle are re-based copies whose blocks of rows are cut elsewhere, so an N-GPU run
 * and a one-GPU run of the same data differ in last bits under FMX_ROWS_FLAT=1 (they are bitwise equal under the product form), and the switch is read at every
 * launch -- set it before the first call and leave it. */
int fmx_matrix_rows_form(const fmx_matrix* m, int32_t* form);
/* How the engine laid out its parameter tables: elements between consecutive features' V rows, and whether a feature's linear weight
 * sits inside its V row (fp32 mini-batch tables of at most 16 padded factors, from 3 M features up: out of the caches a nonzero then
 * costs one memory request instead of two; FMX_W_IN_ROW=0/1 in the environment overrides).  Never changes a result. */
int fmx_layout_info(fmx_engine* e, int32_t* v_row_stride, int32_t* w_in_row);
/* A cfg.n_gpus > 1 handle: replicas, whether they share one device (rehearsal), the ordered device pairs (a, b), a != b, and for how many of them
 * direct peer access could be enabled at creation (hipDeviceCanAccessPeer / hipDeviceEnablePeerAccess: the shards, fmx_set_params and the
 * owner-sharded exchange move data with peer copies, which go over xGMI only then), and the exchange a step of one sparse tile takes unless
 * FMX_GROUP_EXCHANGE says otherwise (1: all-gather of the occurring features' records; 2: owner-sharded -- the default only where the replicas share
 * a device until a run on two or more devices has confirmed it bitwise).  A one-GPU handle reports n = 1 and zeros. */
int fmx_group_info(fmx_engine* e, int32_t* n_replicas, int32_t* share_device, int32_t* peer_pairs, int32_t* peer_pairs_direct, int32_t* sparse_exchange);
/* RCCL smoke test for cfg.n_gpus > 1: loads librccl, ncclCommInitAll over devices 0..n-1, one grouped fp32 and fp64
 * all-reduce(sum) of 1000 elements per rank on per-device streams, checked against the closed form; max_err = largest deviation. */
int fmx_rccl_selftest(int32_t n, double* max_err);
/* What the memory system gives the hot kernels' access pattern and nothing else: uniformly random rows of row_bytes bytes
 * (16..256, a power of two) from a table of table_bytes bytes; ids are generated in registers, row_bytes / 16 lanes fetch a row,
 * in_flight (1, 2, 4 or 8) rows outstanding per lane, n_groups lane groups each summing per_group rows, `reps` launches timed with
 * HIP events.  bench.py reports kernel rows/s divided by this figure as "ceiling_frac".  Environment switches of the probe (measurement only; profiles/
 * r04_gather_granularity.txt, r04_phase1_l2.txt): FMX_PROBE_STRATA=1 fetch j of every lane group comes from stratum j of the table (the order in which phase 1 walks
 * rows of one column per stratum); FMX_PROBE_SIDE=1 a 4-byte word of a second table under the same id beside every row (phase 1's w); FMX_PROBE_LOAD=1/2/3 non-temporal /
 * system-scope / both buffer loads; FMX_PROBE_UNCACHED=1 the table in hipDeviceMallocUncached memory. */
int fmx_measure_gather(int device, int64_t table_bytes, int32_t row_bytes, int64_t n_groups, int32_t per_group, int32_t in_flight,
                       int32_t reps, double* rows_per_s);
/* the same probe held to at most 160 KiB / lds_bytes workgroups per CU: how many requests in flight the ceiling needs */
int fmx_measure_gather_occ(int device, int64_t table_bytes, int32_t row_bytes, int64_t n_groups, int32_t per_group, int32_t in_flight,
                           int32_t reps, int32_t lds_bytes, double* rows_per_s);

/* the same gather driven by a MATRIX: lane group g fetches the table row of every column id of row r0 + g (rows [r0, r0 + nrows) of m) from
 * a scratch table of table_rows rows -- phase 1's own access stream with the arithmetic stripped away.  For skewed columns (most fetches
 * served on-die) this, not the uniformly random probe, is the ceiling bench.py divides by. */
int fmx_measure_gather_matrix(fmx_matrix* m, int64_t r0, int64_t nrows, int64_t table_rows, int32_t row_bytes, int32_t in_flight,
                              int32_t reps, double* rows_per_s);

#ifdef __cplusplus
}
#endif
#endif /* FMX_H_ */
