// The query side of libfmx.so: the extern "C" entry points of include/fmx.h that read a trained engine -- predictions, top-K, neighbours, pair
// sampling, contributions, interactions, pointwise metrics, calibration, fold-in, held-out ranks and metrics, candidate lists, projections, diversification.  Host code only: an
// entry point checks its arguments (nothing is written on a refusal), makes the engine's state current (query_begin) and hands the rows to the
// *_run function of its kernel file; a host form stages the results on the device in bounded pieces (staged) and copies each piece down.
#include <algorithm>
#include <cmath>
#include <vector>

#include "fmx_internal.h"
#include "fm_rank.h"

using namespace fmx;

// the engine's device, its stream drained, and the parameters a valid state
static int query_begin(fmx_engine* e) {
  FMX_TRY(use_device(e->cfg.device));
  FMX_HIP(hipStreamSynchronize(e->stream));
  return seq_abort_check(e);
}

// rows [r0, r1) of a matrix of n rows; `what` ("", "context ", "query ") names the matrix in the message
static int check_rows(int64_t r0, int64_t r1, int64_t n, const char* what) {
  FMX_CHECK(r0 >= 0 && r0 <= r1 && r1 <= n, FMX_ERR_INVALID, "%srow range [%lld,%lld) out of bounds", what, (long long)r0, (long long)r1);
  return FMX_OK;
}

// fmx_topk's factor limit: a context's padded factors fit the kernels' LDS row
static int check_topk_factors(const fmx_engine* e) {
  const int esz = wide_state(e) ? (int)sizeof(double) : (int)sizeof(float), fb = wide_state(e) ? 8 : 16;
  FMX_CHECK((e->k + fb - 1) / fb * fb * esz <= TK_KS_BYTES, FMX_ERR_INVALID, "top-K scoring holds at most %d factors", TK_KS_BYTES / esz);
  return FMX_OK;
}

// one output of a host form: the caller's array (NULL: not asked for, nothing is staged) of `width` elements of `esz` bytes per row
struct Out {
  void* host;
  size_t esz;
  int64_t width;
};

static int stage(const char* what, DevBuf* b, size_t bytes) {
  if (dev_buf(b, bytes) == FMX_OK) return FMX_OK;
  set_error("%s: could not allocate the result staging", what);
  return FMX_ERR_HIP;
}

// the finished piece down: `bytes` from each staging d[i] that is in use to host[i]
template <size_t N>
static int copy_down(fmx_engine* e, const char* what, void* const (&host)[N], void* const (&d)[N], const size_t (&bytes)[N]) {
  bool ok = hipStreamSynchronize(e->stream) == hipSuccess;
  for (size_t i = 0; i < N && ok; ++i)
    if (d[i] && bytes[i]) ok = hipMemcpy(host[i], d[i], bytes[i], hipMemcpyDeviceToHost) == hipSuccess;
  FMX_CHECK(ok, FMX_ERR_HIP, "%s: the kernels or the copy of the results failed", what);
  return FMX_OK;
}

// The host forms' staging: rows [0, n) in pieces of at most `piece` rows, so that the device memory of a call stays bounded whatever n is.
// run(a, b, d) fills d[i], the staging of output i (null where the output is), with rows [a, b); then the stream is drained and every output
// copied down at host + a * width.  One allocation per output for the whole call, freed on every exit.
template <size_t N, typename Run>
static int staged(fmx_engine* e, const char* what, int64_t n, int64_t piece, const Out (&out)[N], Run run) {
  const int64_t rows = std::min(n, piece);
  DevBuf buf[N];
  void* d[N] = {};
  for (size_t i = 0; i < N; ++i) {
    if (!out[i].host) continue;
    FMX_TRY(stage(what, &buf[i], (size_t)(rows * out[i].width) * out[i].esz));
    d[i] = buf[i].get();
  }
  for (int64_t a = 0; a < n; a += rows) {
    const int64_t b = std::min(n, a + rows);
    FMX_TRY(run(a, b, d));
    void* host[N];
    size_t bytes[N];
    for (size_t i = 0; i < N; ++i) {
      const size_t row = (size_t)out[i].width * out[i].esz;
      host[i] = (char*)out[i].host + (size_t)a * row;
      bytes[i] = (size_t)(b - a) * row;
    }
    FMX_TRY(copy_down(e, what, host, d, bytes));
  }
  return FMX_OK;
}

// rows per piece of at most 2^22 result slots: the staging of the top-K forms stays at 64 MB
static int64_t slot_rows(int32_t per_row) { return std::max<int64_t>(1, (1LL << 22) / per_row); }

extern "C" {

int fmx_predict(fmx_engine* e, const fmx_matrix* m, double* out, int link) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(out != nullptr || m->n == 0, FMX_ERR_INVALID, "out is NULL");
  FMX_CHECK(link >= FMX_LINK_NONE && link <= FMX_LINK_PROBIT, FMX_ERR_INVALID, "unknown link %d", link);
  FMX_TRY(use_device(e->cfg.device));
  if (m->n == 0) return FMX_OK;
  return staged(e, "fmx_predict", m->n, m->n, {Out{out, sizeof(double), 1}},
                [&](int64_t a, int64_t b, void* const* d) { return forward_rows(e, m, a, b, (double*)d[0], link); });
}

int fmx_predict_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, void* dev_out_f64, int link) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(r0 >= 0 && r0 <= r1 && r1 <= m->n && dev_out_f64, FMX_ERR_INVALID, "bad row range or NULL output");  // (one refusal, its own text)
  FMX_TRY(use_device(e->cfg.device));
  return forward_rows(e, m, r0, r1, (double*)dev_out_f64, link);
}

static int check_topk(const fmx_engine* e, const fmx_matrix* c, const fmx_matrix* items, const fmx_matrix* x, int32_t top_k, int link) {
  FMX_TRY(check_pair(e, c));
  FMX_TRY(check_pair(e, items));
  FMX_CHECK(top_k >= 1 && top_k <= 1024, FMX_ERR_INVALID, "top_k must be in 1..1024 (got %d)", (int)top_k);
  FMX_CHECK(link >= FMX_LINK_NONE && link <= FMX_LINK_PROBIT, FMX_ERR_INVALID, "unknown link %d", link);
  FMX_CHECK(items->n < INT32_MAX, FMX_ERR_INVALID, "at most 2^31 - 2 item rows (got %lld)", (long long)items->n);
  if (x) {
    FMX_CHECK(x->n == c->n && (int64_t)x->p == items->n, FMX_ERR_INVALID, "exclude must be %lld x %lld (got %lld x %u)", (long long)c->n,
              (long long)items->n, (long long)x->n, x->p);
    FMX_CHECK(x->device == e->cfg.device, FMX_ERR_INVALID, "exclude lives on device %d, engine on %d", x->device, e->cfg.device);
  }
  return FMX_OK;
}

int fmx_topk(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* exclude, int32_t top_k, int link, int64_t* out_index,
             double* out_score) {
  FMX_TRY(check_topk(e, context, items, exclude, top_k, link));
  FMX_CHECK((out_index && out_score) || context->n == 0, FMX_ERR_INVALID, "out_index / out_score is NULL");
  FMX_TRY(query_begin(e));
  if (context->n == 0) return FMX_OK;
  return staged(e, "fmx_topk", context->n, slot_rows(top_k), {Out{out_index, sizeof(int64_t), top_k}, Out{out_score, sizeof(double), top_k}},
                [&](int64_t a, int64_t b, void* const* d) { return topk_run(e, context, a, b, items, exclude, top_k, link, (int64_t*)d[0], (double*)d[1]); });
}

int fmx_topk_device(fmx_engine* e, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items, const fmx_matrix* exclude, int32_t top_k,
                    int link, void* dev_index_i64, void* dev_score_f64) {
  FMX_TRY(check_topk(e, context, items, exclude, top_k, link));
  FMX_TRY(check_rows(r0, r1, context->n, "context "));
  FMX_CHECK((dev_index_i64 && dev_score_f64) || r0 == r1, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  return topk_run(e, context, r0, r1, items, exclude, top_k, link, (int64_t*)dev_index_i64, (double*)dev_score_f64);
}

static int check_neighbors(const fmx_engine* e, const fmx_matrix* q, const fmx_matrix* items, int32_t top_k, int32_t metric) {
  FMX_TRY(check_topk(e, q, items, nullptr, top_k, FMX_LINK_NONE));
  FMX_CHECK(metric == FMX_SIM_COSINE || metric == FMX_SIM_DOT, FMX_ERR_INVALID, "unknown similarity metric %d", (int)metric);
  return check_topk_factors(e);
}

int fmx_neighbors(fmx_engine* e, const fmx_matrix* queries, const fmx_matrix* items, int32_t top_k, int32_t metric, int32_t skip_self, int64_t* out_index,
                  double* out_score) {
  FMX_TRY(check_neighbors(e, queries, items, top_k, metric));
  FMX_CHECK((out_index && out_score) || queries->n == 0, FMX_ERR_INVALID, "out_index / out_score is NULL");
  FMX_TRY(query_begin(e));
  if (queries->n == 0) return FMX_OK;
  return staged(e, "fmx_neighbors", queries->n, slot_rows(top_k), {Out{out_index, sizeof(int64_t), top_k}, Out{out_score, sizeof(double), top_k}},
                [&](int64_t a, int64_t b, void* const* d) {
                  return neighbors_run(e, queries, a, b, items, top_k, metric, skip_self != 0, (int64_t*)d[0], (double*)d[1]);
                });
}

int fmx_neighbors_device(fmx_engine* e, const fmx_matrix* queries, int64_t r0, int64_t r1, const fmx_matrix* items, int32_t top_k, int32_t metric,
                         int32_t skip_self, void* dev_index_i64, void* dev_score_f64) {
  FMX_TRY(check_neighbors(e, queries, items, top_k, metric));
  FMX_TRY(check_rows(r0, r1, queries->n, "query "));
  FMX_CHECK((dev_index_i64 && dev_score_f64) || r0 == r1, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  return neighbors_run(e, queries, r0, r1, items, top_k, metric, skip_self != 0, (int64_t*)dev_index_i64, (double*)dev_score_f64);
}

int fmx_index_build(fmx_engine* e, const fmx_matrix* items, int32_t n_lists, int32_t n_iter, uint64_t seed, fmx_item_index** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(n_lists >= 1 && n_lists <= FMX_INDEX_MAX_LISTS, FMX_ERR_INVALID, "n_lists must be in 1..min(finite items, %d) (got %d)", FMX_INDEX_MAX_LISTS, (int)n_lists);
  FMX_CHECK(n_iter >= 0 && n_iter <= FMX_INDEX_MAX_ITER, FMX_ERR_INVALID, "n_iter must be in 0..%d (got %d)", FMX_INDEX_MAX_ITER, (int)n_iter);
  FMX_TRY(check_topk(e, items, items, nullptr, 1, FMX_LINK_NONE));
  FMX_CHECK((int64_t)n_lists <= items->n, FMX_ERR_INVALID, "n_lists must be at most the number of finite items (got %d for %lld items)", (int)n_lists,
            (long long)items->n);
  FMX_TRY(query_begin(e));
  return index_build_run(e, items, n_lists, n_iter, seed, out);
}

int fmx_index_from_assign(fmx_engine* e, int64_t n_items, int32_t n_lists, const uint32_t* assign, const double* centroid, fmx_item_index** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(n_items >= 0 && n_items < INT32_MAX, FMX_ERR_INVALID, "n_items must be in 0..2^31 - 2 (got %lld)", (long long)n_items);
  FMX_CHECK(n_lists >= 1 && n_lists <= FMX_INDEX_MAX_LISTS, FMX_ERR_INVALID, "n_lists must be in 1..%d (got %d)", FMX_INDEX_MAX_LISTS, (int)n_lists);
  FMX_CHECK(e != nullptr, FMX_ERR_INVALID, "NULL engine");
  FMX_CHECK(centroid != nullptr && (assign != nullptr || n_items == 0), FMX_ERR_INVALID, "assign / centroid is NULL");
  for (int64_t i = 0; i < n_items; ++i)
    FMX_CHECK(assign[i] < (uint32_t)n_lists, FMX_ERR_INVALID, "assign[%lld] = %u, but there are %d lists", (long long)i, assign[i], (int)n_lists);
  FMX_TRY(query_begin(e));
  return index_from_assign_run(e, n_items, n_lists, assign, centroid, out);
}

int fmx_index_info(const fmx_item_index* index, int64_t* n_items, int32_t* n_lists, int32_t* k, int64_t* non_empty) {
  FMX_CHECK(index != nullptr, FMX_ERR_INVALID, "NULL index");
  if (n_items) *n_items = index->n_items;
  if (n_lists) *n_lists = index->n_lists;
  if (k) *k = index->k;
  if (non_empty) *non_empty = index->non_empty;
  return FMX_OK;
}

int fmx_index_export(const fmx_item_index* index, double* centroid, uint32_t* assign, int64_t* list_ptr, int32_t* list_item) {
  FMX_CHECK(index != nullptr, FMX_ERR_INVALID, "NULL index");
  FMX_TRY(use_device(index->device));
  return index_export_run(index, centroid, assign, list_ptr, list_item);
}

int fmx_index_free(fmx_item_index* index) {
  if (!index) return FMX_OK;
  FMX_TRY(use_device(index->device));
  index_free(index);
  return FMX_OK;
}

static int check_topk_index(const fmx_engine* e, const fmx_item_index* ix, const fmx_matrix* c, const fmx_matrix* items, const fmx_matrix* x, int32_t top_k,
                            int32_t n_probe, int link) {
  FMX_CHECK(n_probe >= 1, FMX_ERR_INVALID, "n_probe must be at least 1 (got %d)", (int)n_probe);
  FMX_TRY(check_topk(e, c, items, x, top_k, link));
  FMX_CHECK(ix != nullptr, FMX_ERR_INVALID, "NULL index");
  FMX_CHECK(ix->device == e->cfg.device, FMX_ERR_INVALID, "the index lives on device %d, engine on %d", ix->device, e->cfg.device);
  FMX_CHECK(items->n == ix->n_items, FMX_ERR_INVALID, "the index holds %lld items, items has %lld rows", (long long)ix->n_items, (long long)items->n);
  FMX_CHECK(e->k == ix->k, FMX_ERR_INVALID, "the index was built for %d factors, the engine has %d", ix->k, e->k);
  FMX_CHECK(n_probe >= 1 && n_probe <= ix->n_lists, FMX_ERR_INVALID, "n_probe must be in 1..n_lists = %d (got %d)", ix->n_lists, (int)n_probe);
  return check_topk_factors(e);
}

int fmx_topk_index(fmx_engine* e, const fmx_item_index* index, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* exclude, int32_t top_k,
                   int32_t n_probe, int link, int64_t* out_index, double* out_score, int64_t* out_scanned) {
  FMX_TRY(check_topk_index(e, index, context, items, exclude, top_k, n_probe, link));
  FMX_CHECK((out_index && out_score) || context->n == 0, FMX_ERR_INVALID, "out_index / out_score is NULL");
  FMX_TRY(query_begin(e));
  if (context->n == 0) return FMX_OK;
  return staged(e, "fmx_topk_index", context->n, slot_rows(top_k),
                {Out{out_index, sizeof(int64_t), top_k}, Out{out_score, sizeof(double), top_k}, Out{out_scanned, sizeof(int64_t), 1}},
                [&](int64_t a, int64_t b, void* const* d) {
                  return topk_index_run(e, index, context, a, b, items, exclude, top_k, n_probe, link, (int64_t*)d[0], (double*)d[1], (int64_t*)d[2]);
                });
}

int fmx_topk_index_device(fmx_engine* e, const fmx_item_index* index, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items,
                          const fmx_matrix* exclude, int32_t top_k, int32_t n_probe, int link, void* dev_index_i64, void* dev_score_f64, void* dev_scanned_i64) {
  FMX_TRY(check_topk_index(e, index, context, items, exclude, top_k, n_probe, link));
  FMX_TRY(check_rows(r0, r1, context->n, "context "));
  FMX_CHECK((dev_index_i64 && dev_score_f64) || r0 == r1, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  return topk_index_run(e, index, context, r0, r1, items, exclude, top_k, n_probe, link, (int64_t*)dev_index_i64, (double*)dev_score_f64,
                        (int64_t*)dev_scanned_i64);
}

static int check_sampling(const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* positives, int32_t n_neg, int64_t epoch) {
  FMX_CHECK(context && items && positives, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(context->p == items->p, FMX_ERR_INVALID, "context and items must share the feature count (%u vs %u)", context->p, items->p);
  FMX_CHECK(context->device == items->device && positives->device == context->device, FMX_ERR_INVALID, "context, items and positives must live on one device");
  FMX_CHECK(positives->n == context->n, FMX_ERR_INVALID, "positives must hold one row per context row (%lld vs %lld)", (long long)positives->n, (long long)context->n);
  FMX_CHECK((int64_t)positives->p == items->n, FMX_ERR_INVALID, "positives' column count must be the item count (%u vs %lld)", positives->p, (long long)items->n);
  FMX_CHECK(items->n >= 1 && items->n < (1LL << 32) - 1, FMX_ERR_INVALID, "items must hold 1 .. 2^32 - 2 rows");
  FMX_CHECK(context->n < (1LL << 31), FMX_ERR_INVALID, "at most 2^31 - 1 context rows");
  FMX_CHECK(n_neg >= 1, FMX_ERR_INVALID, "n_neg must be >= 1 (got %d)", n_neg);
  FMX_CHECK(epoch >= 0, FMX_ERR_INVALID, "epoch must be >= 0");
  return FMX_OK;
}

int fmx_matrix_pairs_hard(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* positives, int32_t n_neg, int32_t n_cand,
                          uint64_t seed, int64_t epoch, fmx_matrix** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_TRY(check_sampling(context, items, positives, n_neg, epoch));
  FMX_CHECK(e != nullptr, FMX_ERR_INVALID, "NULL engine");
  FMX_CHECK(n_cand >= 1 && n_cand <= 64, FMX_ERR_INVALID, "n_cand must be in 1..64 (got %d)", (int)n_cand);
  FMX_TRY(check_topk(e, context, items, nullptr, 1, FMX_LINK_NONE));
  FMX_TRY(check_topk_factors(e));
  FMX_TRY(query_begin(e));
  return pairs_build(context, items, positives, n_neg, seed, epoch, out, e, n_cand);
}

int fmx_matrix_pairs(const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* positives, int32_t n_neg, uint64_t seed, int64_t epoch,
                     fmx_matrix** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_TRY(check_sampling(context, items, positives, n_neg, epoch));
  FMX_TRY(use_device(context->device));
  return pairs_build(context, items, positives, n_neg, seed, epoch, out);
}

int fmx_contrib(fmx_engine* e, const fmx_matrix* m, double* out) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(out != nullptr || m->nnz == 0, FMX_ERR_INVALID, "out is NULL");
  FMX_TRY(query_begin(e));
  if (m->nnz == 0) return FMX_OK;
  // one piece of nnz one-element "rows": the entries of the whole matrix
  return staged(e, "fmx_contrib", m->nnz, m->nnz, {Out{out, sizeof(double), 1}},
                [&](int64_t, int64_t, void* const* d) { return contrib_run(e, m, 0, m->n, (double*)d[0]); });
}

int fmx_contrib_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, void* dev_out_f64) {
  FMX_TRY(check_pair(e, m));
  FMX_TRY(check_rows(r0, r1, m->n, ""));
  FMX_CHECK(dev_out_f64 != nullptr || r0 == r1, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(use_device(e->cfg.device));
  return contrib_run(e, m, r0, r1, (double*)dev_out_f64);
}

int fmx_contrib_summary(fmx_engine* e, const fmx_matrix* m, double* sum, double* abs_sum, int64_t* count) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(sum != nullptr && abs_sum != nullptr, FMX_ERR_INVALID, "sum / abs_sum is NULL");
  FMX_TRY(query_begin(e));
  return contrib_summary_run(e, m, sum, abs_sum, count);
}

static int check_interactions(const fmx_engine* e, const fmx_matrix* m, int32_t top_m) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(top_m >= 1 && top_m <= 64, FMX_ERR_INVALID, "top_m must be in 1..64 (got %d)", (int)top_m);
  return FMX_OK;
}

int fmx_interactions(fmx_engine* e, const fmx_matrix* m, int32_t top_m, int64_t* out_a, int64_t* out_b, double* out_value) {
  FMX_TRY(check_interactions(e, m, top_m));
  FMX_CHECK((out_a && out_b && out_value) || m->n == 0, FMX_ERR_INVALID, "out_a / out_b / out_value is NULL");
  FMX_TRY(query_begin(e));
  if (m->n == 0) return FMX_OK;
  const InterLimits lim = interactions_take_limits();  // once per call: every piece runs under the same limits
  return staged(e, "fmx_interactions", m->n, slot_rows(top_m),
                {Out{out_a, sizeof(int64_t), top_m}, Out{out_b, sizeof(int64_t), top_m}, Out{out_value, sizeof(double), top_m}},
                [&](int64_t a, int64_t b, void* const* d) { return interactions_run(e, m, a, b, top_m, lim, (int64_t*)d[0], (int64_t*)d[1], (double*)d[2]); });
}

int fmx_interactions_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, int32_t top_m, void* dev_a_i64, void* dev_b_i64, void* dev_value_f64) {
  FMX_TRY(check_interactions(e, m, top_m));
  FMX_TRY(check_rows(r0, r1, m->n, ""));
  FMX_CHECK((dev_a_i64 && dev_b_i64 && dev_value_f64) || r0 == r1, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  if (r0 == r1) return FMX_OK;
  return interactions_run(e, m, r0, r1, top_m, interactions_take_limits(), (int64_t*)dev_a_i64, (int64_t*)dev_b_i64, (double*)dev_value_f64);
}

int fmx_interactions_summary(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_feature, int32_t n_groups, double* sum, double* abs_sum,
                             int64_t* count) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(sum != nullptr && abs_sum != nullptr, FMX_ERR_INVALID, "sum / abs_sum is NULL");
  FMX_CHECK(n_groups >= 1 && n_groups <= 64, FMX_ERR_INVALID, "n_groups must be in 1..64 (got %d)", (int)n_groups);
  if (group_of_feature) {
    for (uint32_t j = 0; j < m->p; ++j)
      FMX_CHECK(group_of_feature[j] < (uint32_t)n_groups, FMX_ERR_INVALID, "feature %u is in group %u, but there are %d groups", j, group_of_feature[j], (int)n_groups);
  } else {
    FMX_CHECK(m->p <= (uint32_t)n_groups, FMX_ERR_INVALID, "without a group map every feature is its own group: %u features need p <= n_groups (%d)", m->p, (int)n_groups);
  }
  FMX_TRY(query_begin(e));
  return interactions_summary_run(e, m, group_of_feature, n_groups, interactions_take_limits(), sum, abs_sum, count);
}

static int check_metrics(const fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, int64_t n_groups, int link) {
  FMX_TRY(check_pair(e, m));
  const int task = e->hyper.task;
  FMX_CHECK(task == FMX_TASK_CLASSIFICATION || task == FMX_TASK_REGRESSION, FMX_ERR_INVALID,
            "fmx_metrics evaluates CLASSIFICATION and REGRESSION engines (a RANKING engine has FMX_EVAL_PAIR_ACC / FMX_EVAL_BPR and fmx_heldout_metrics)");
  FMX_CHECK(m->has_labels && m->y != nullptr, FMX_ERR_INVALID, "fmx_metrics needs a matrix with labels");
  if (task == FMX_TASK_CLASSIFICATION)
    FMX_CHECK(link == FMX_LINK_LOGISTIC || link == FMX_LINK_PROBIT, FMX_ERR_INVALID, "a CLASSIFICATION engine is measured under FMX_LINK_LOGISTIC or FMX_LINK_PROBIT (got %d)", link);
  else
    FMX_CHECK(link == FMX_LINK_NONE || link == FMX_LINK_CLAMP, FMX_ERR_INVALID, "a REGRESSION engine is measured under FMX_LINK_NONE or FMX_LINK_CLAMP (got %d)", link);
  FMX_CHECK(n_groups >= 1 && n_groups <= INT32_MAX, FMX_ERR_INVALID, "n_groups must be in 1..2^31 - 1 (got %lld)", (long long)n_groups);
  FMX_TRY(check_rows(r0, r1, m->n, ""));
  FMX_CHECK(r1 - r0 <= INT32_MAX, FMX_ERR_INVALID, "at most 2^31 - 1 rows per call (got %lld)", (long long)(r1 - r0));
  return FMX_OK;
}

int fmx_metrics(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row, int64_t n_groups, int link, double* out_value, int64_t* out_count) {
  FMX_TRY(check_metrics(e, m, 0, m ? m->n : 0, n_groups, link));
  const int64_t n = m->n;
  FMX_CHECK(group_of_row != nullptr || n_groups == 1, FMX_ERR_INVALID, "without group ids there is one group: n_groups must be 1 (got %lld)", (long long)n_groups);
  FMX_CHECK(out_value != nullptr || n == 0, FMX_ERR_INVALID, "out_value is NULL");
  if (group_of_row)
    for (int64_t r = 0; r < n; ++r)
      FMX_CHECK((int64_t)group_of_row[r] < n_groups, FMX_ERR_INVALID, "row %lld is in group %u, but there are %lld groups", (long long)r, group_of_row[r], (long long)n_groups);
  FMX_TRY(query_begin(e));
  if (n == 0) return FMX_OK;
  const size_t G = (size_t)n_groups;
  DevBuf dg, dv, dc;
  if (group_of_row) {
    FMX_TRY(stage("fmx_metrics", &dg, (size_t)n * sizeof(uint32_t)));
    FMX_HIP(hipMemcpy(dg.get(), group_of_row, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  FMX_TRY(stage("fmx_metrics", &dv, G * FMX_MET_VALUES * sizeof(double)));
  if (out_count) FMX_TRY(stage("fmx_metrics", &dc, G * FMX_MET_COUNTS * sizeof(int64_t)));
  FMX_TRY(metrics_run(e, m, 0, n, group_of_row ? (const uint32_t*)dg.get() : nullptr, n_groups, link, metrics_limits(), (double*)dv.get(), (int64_t*)dc.get()));
  return copy_down(e, "fmx_metrics", {(void*)out_value, (void*)out_count}, {dv.get(), dc.get()},
                   {G * FMX_MET_VALUES * sizeof(double), G * FMX_MET_COUNTS * sizeof(int64_t)});
}

int fmx_metrics_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, int link, void* dev_value_f64,
                       void* dev_count_i64) {
  FMX_TRY(check_metrics(e, m, r0, r1, n_groups, link));
  FMX_CHECK(dev_group_u32 != nullptr || n_groups == 1, FMX_ERR_INVALID, "without group ids there is one group: n_groups must be 1 (got %lld)", (long long)n_groups);
  FMX_CHECK(dev_value_f64 != nullptr || r0 == r1, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  if (r0 == r1) return FMX_OK;
  return metrics_run(e, m, r0, r1, (const uint32_t*)dev_group_u32, n_groups, link, metrics_limits(), (double*)dev_value_f64, (int64_t*)dev_count_i64);
}

// what every calibration call checks first; `what` names the call in the messages
static int check_calibrate(const fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, int64_t n_groups, const char* what) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(e->hyper.task == FMX_TASK_CLASSIFICATION, FMX_ERR_INVALID, "%s calibrates CLASSIFICATION engines only", what);
  FMX_CHECK(m->has_labels && m->y != nullptr, FMX_ERR_INVALID, "%s needs a matrix with labels", what);
  FMX_CHECK(n_groups >= 1 && n_groups <= INT32_MAX, FMX_ERR_INVALID, "n_groups must be in 1..2^31 - 1 (got %lld)", (long long)n_groups);
  FMX_TRY(check_rows(r0, r1, m->n, ""));
  FMX_CHECK(r1 - r0 <= INT32_MAX, FMX_ERR_INVALID, "at most 2^31 - 1 rows per call (got %lld)", (long long)(r1 - r0));
  return FMX_OK;
}

// the group ids of a host form (every id < n_groups) or none (one group)
static int check_group_ids(const uint32_t* group_of_row, int64_t n, int64_t n_groups, bool needed) {
  FMX_CHECK(group_of_row != nullptr || n_groups == 1 || !needed, FMX_ERR_INVALID, "without group ids there is one group: n_groups must be 1 (got %lld)",
            (long long)n_groups);
  if (group_of_row)
    for (int64_t r = 0; r < n; ++r)
      FMX_CHECK((int64_t)group_of_row[r] < n_groups, FMX_ERR_INVALID, "row %lld is in group %u, but there are %lld groups", (long long)r, group_of_row[r], (long long)n_groups);
  return FMX_OK;
}

// a calibrator (NULL: FMX_CAL_NONE under `link`) for a call of n_groups groups
static int check_calibrator(const fmx_calibrator* c, int link, int64_t n_groups) {
  if (!c) {
    FMX_CHECK(link == FMX_LINK_LOGISTIC || link == FMX_LINK_PROBIT, FMX_ERR_INVALID, "without a calibrator the link must be FMX_LINK_LOGISTIC or FMX_LINK_PROBIT (got %d)", link);
    return FMX_OK;
  }
  FMX_CHECK(c->struct_size == sizeof(fmx_calibrator), FMX_ERR_INVALID, "fmx_calibrator.struct_size is %u, this library's is %u", c->struct_size, (unsigned)sizeof(fmx_calibrator));
  FMX_CHECK(c->kind >= FMX_CAL_NONE && c->kind <= FMX_CAL_STEPS, FMX_ERR_INVALID, "unknown calibrator kind %d", (int)c->kind);
  if (c->kind == FMX_CAL_NONE) {
    FMX_CHECK(c->link == FMX_LINK_LOGISTIC || c->link == FMX_LINK_PROBIT, FMX_ERR_INVALID, "a FMX_CAL_NONE calibrator's link must be FMX_LINK_LOGISTIC or FMX_LINK_PROBIT (got %d)",
              (int)c->link);
    return FMX_OK;
  }
  FMX_CHECK(c->n_groups == 1 || c->n_groups == n_groups, FMX_ERR_INVALID, "the calibrator holds %lld maps: it must hold 1 or the call's n_groups (%lld)", (long long)c->n_groups,
            (long long)n_groups);
  if (c->kind == FMX_CAL_PLATT) {
    FMX_CHECK(c->platt != nullptr, FMX_ERR_INVALID, "a FMX_CAL_PLATT calibrator needs platt");
    return FMX_OK;
  }
  FMX_CHECK(c->max_steps >= 1 && c->n_steps && c->thr && c->val, FMX_ERR_INVALID, "a FMX_CAL_STEPS calibrator needs max_steps >= 1, n_steps, thr and val");
  FMX_CHECK(c->n_groups <= (1LL << 28) / c->max_steps, FMX_ERR_INVALID, "a calibrator holds at most 2^28 steps in all");
  for (int64_t g = 0; g < c->n_groups; ++g)
    FMX_CHECK(c->n_steps[g] >= 0 && c->n_steps[g] <= c->max_steps, FMX_ERR_INVALID, "n_steps[%lld] = %d is outside 0..max_steps = %d", (long long)g, (int)c->n_steps[g],
              (int)c->max_steps);
  return FMX_OK;
}

// does the call read the group ids?  (one map for every row needs none)
static bool calibrator_needs_ids(const fmx_calibrator* c) { return c && c->kind != FMX_CAL_NONE && c->n_groups > 1; }

static int check_bins(int64_t n_groups, int32_t n_bins) {
  FMX_CHECK(n_bins >= 1 && n_bins <= 1024, FMX_ERR_INVALID, "n_bins must be in 1..1024 (got %d)", (int)n_bins);
  FMX_CHECK(n_groups * n_bins <= (1LL << 28), FMX_ERR_INVALID, "n_groups * n_bins must be at most 2^28 (got %lld)", (long long)(n_groups * n_bins));
  return FMX_OK;
}

// the host group ids on the device (none: dg stays empty)
static int stage_groups(const char* what, DevBuf* dg, const uint32_t* group_of_row, int64_t n) {
  if (!group_of_row) return FMX_OK;
  FMX_TRY(stage(what, dg, (size_t)n * sizeof(uint32_t)));
  FMX_HIP(hipMemcpy(dg->get(), group_of_row, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
  return FMX_OK;
}

int fmx_predict_calibrated(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row, int64_t n_groups, const fmx_calibrator* cal, int link, double* out) {
  FMX_TRY(check_calibrate(e, m, 0, m ? m->n : 0, n_groups, "fmx_predict_calibrated"));
  const int64_t n = m->n;
  FMX_TRY(check_calibrator(cal, link, n_groups));
  FMX_TRY(check_group_ids(group_of_row, n, n_groups, calibrator_needs_ids(cal)));
  FMX_CHECK(out != nullptr || n == 0, FMX_ERR_INVALID, "out is NULL");
  FMX_TRY(query_begin(e));
  if (n == 0) return FMX_OK;
  DevBuf dg, dout;
  FMX_TRY(stage_groups("fmx_predict_calibrated", &dg, group_of_row, n));
  FMX_TRY(stage("fmx_predict_calibrated", &dout, (size_t)n * sizeof(double)));
  FMX_TRY(predict_calibrated_run(e, m, 0, n, (const uint32_t*)dg.get(), n_groups, cal, link, (double*)dout.get()));
  return copy_down(e, "fmx_predict_calibrated", {(void*)out}, {dout.get()}, {(size_t)n * sizeof(double)});
}

int fmx_predict_calibrated_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, const fmx_calibrator* cal,
                                  int link, void* dev_out_f64) {
  FMX_TRY(check_calibrate(e, m, r0, r1, n_groups, "fmx_predict_calibrated_device"));
  FMX_TRY(check_calibrator(cal, link, n_groups));
  FMX_CHECK(dev_group_u32 != nullptr || n_groups == 1 || !calibrator_needs_ids(cal), FMX_ERR_INVALID, "without group ids there is one group: n_groups must be 1 (got %lld)",
            (long long)n_groups);
  FMX_CHECK(dev_out_f64 != nullptr || r0 == r1, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  if (r0 == r1) return FMX_OK;
  return predict_calibrated_run(e, m, r0, r1, (const uint32_t*)dev_group_u32, n_groups, cal, link, (double*)dev_out_f64);
}

int fmx_reliability(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row, int64_t n_groups, int32_t n_bins, int32_t binning, const fmx_calibrator* cal, int link,
                    int64_t* out_count, double* out_sum_p, double* out_lo_z, double* out_hi_z, int64_t* out_nan_rows, double* out_value) {
  FMX_TRY(check_calibrate(e, m, 0, m ? m->n : 0, n_groups, "fmx_reliability"));
  const int64_t n = m->n;
  FMX_TRY(check_bins(n_groups, n_bins));
  FMX_CHECK(binning == FMX_BINS_WIDTH || binning == FMX_BINS_MASS, FMX_ERR_INVALID, "unknown binning %d", (int)binning);
  FMX_TRY(check_calibrator(cal, link, n_groups));
  FMX_TRY(check_group_ids(group_of_row, n, n_groups, true));
  FMX_TRY(query_begin(e));
  if (n == 0) return FMX_OK;
  const size_t G = (size_t)n_groups, cells = G * (size_t)n_bins;
  void* const host[6] = {out_count, out_sum_p, out_lo_z, out_hi_z, out_nan_rows, out_value};
  const size_t bytes[6] = {cells * 2 * sizeof(int64_t), cells * sizeof(double), cells * sizeof(double), cells * sizeof(double), G * sizeof(int64_t),
                           G * FMX_CAL_VALUES * sizeof(double)};
  DevBuf dg, buf[6];
  void* d[6] = {};
  FMX_TRY(stage_groups("fmx_reliability", &dg, group_of_row, n));
  for (int i = 0; i < 6; ++i) {
    if (!host[i]) continue;
    FMX_TRY(stage("fmx_reliability", &buf[i], bytes[i]));
    d[i] = buf[i].get();
  }
  FMX_TRY(reliability_run(e, m, 0, n, (const uint32_t*)dg.get(), n_groups, n_bins, binning, cal, link, (int64_t*)d[0], (double*)d[1], (double*)d[2], (double*)d[3],
                          (int64_t*)d[4], (double*)d[5]));
  return copy_down(e, "fmx_reliability", host, d, bytes);
}

int fmx_reliability_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, int32_t n_bins, int32_t binning,
                           const fmx_calibrator* cal, int link, void* dev_count_i64, void* dev_sum_p_f64, void* dev_lo_z_f64, void* dev_hi_z_f64, void* dev_nan_rows_i64,
                           void* dev_value_f64) {
  FMX_TRY(check_calibrate(e, m, r0, r1, n_groups, "fmx_reliability_device"));
  FMX_TRY(check_bins(n_groups, n_bins));
  FMX_CHECK(binning == FMX_BINS_WIDTH || binning == FMX_BINS_MASS, FMX_ERR_INVALID, "unknown binning %d", (int)binning);
  FMX_TRY(check_calibrator(cal, link, n_groups));
  FMX_CHECK(dev_group_u32 != nullptr || n_groups == 1, FMX_ERR_INVALID, "without group ids there is one group: n_groups must be 1 (got %lld)", (long long)n_groups);
  FMX_TRY(query_begin(e));
  if (r0 == r1) return FMX_OK;
  return reliability_run(e, m, r0, r1, (const uint32_t*)dev_group_u32, n_groups, n_bins, binning, cal, link, (int64_t*)dev_count_i64, (double*)dev_sum_p_f64,
                         (double*)dev_lo_z_f64, (double*)dev_hi_z_f64, (int64_t*)dev_nan_rows_i64, (double*)dev_value_f64);
}

static int check_platt(double lambda, int32_t n_newton) {
  FMX_CHECK(lambda >= 0.0, FMX_ERR_INVALID, "lambda must be a number >= 0");   // (a NaN fails the comparison)
  FMX_CHECK(n_newton >= 1, FMX_ERR_INVALID, "n_newton must be at least 1 (got %d)", (int)n_newton);
  return FMX_OK;
}

int fmx_calibrate_platt(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row, int64_t n_groups, double lambda, int32_t n_newton, double* out_ab,
                        int64_t* out_rows, int32_t* out_status) {
  FMX_TRY(check_calibrate(e, m, 0, m ? m->n : 0, n_groups, "fmx_calibrate_platt"));
  const int64_t n = m->n;
  FMX_TRY(check_platt(lambda, n_newton));
  FMX_TRY(check_group_ids(group_of_row, n, n_groups, true));
  FMX_TRY(query_begin(e));
  if (n == 0) return FMX_OK;
  const size_t G = (size_t)n_groups;
  void* const host[3] = {out_ab, out_rows, out_status};
  const size_t bytes[3] = {G * 2 * sizeof(double), G * sizeof(int64_t), G * sizeof(int32_t)};
  DevBuf dg, buf[3];
  void* d[3] = {};
  FMX_TRY(stage_groups("fmx_calibrate_platt", &dg, group_of_row, n));
  for (int i = 0; i < 3; ++i) {
    if (!host[i]) continue;
    FMX_TRY(stage("fmx_calibrate_platt", &buf[i], bytes[i]));
    d[i] = buf[i].get();
  }
  FMX_TRY(platt_run(e, m, 0, n, (const uint32_t*)dg.get(), n_groups, lambda, n_newton, (double*)d[0], (int64_t*)d[1], (int32_t*)d[2]));
  return copy_down(e, "fmx_calibrate_platt", host, d, bytes);
}

int fmx_calibrate_platt_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, double lambda, int32_t n_newton,
                               void* dev_ab_f64, void* dev_rows_i64, void* dev_status_i32) {
  FMX_TRY(check_calibrate(e, m, r0, r1, n_groups, "fmx_calibrate_platt_device"));
  FMX_TRY(check_platt(lambda, n_newton));
  FMX_CHECK(dev_group_u32 != nullptr || n_groups == 1, FMX_ERR_INVALID, "without group ids there is one group: n_groups must be 1 (got %lld)", (long long)n_groups);
  FMX_TRY(query_begin(e));
  if (r0 == r1) return FMX_OK;
  return platt_run(e, m, r0, r1, (const uint32_t*)dev_group_u32, n_groups, lambda, n_newton, (double*)dev_ab_f64, (int64_t*)dev_rows_i64, (int32_t*)dev_status_i32);
}

int fmx_calibrate_isotonic(fmx_engine* e, const fmx_matrix* m, const uint32_t* group_of_row, int64_t n_groups, int32_t n_bins, int32_t* out_n_steps, double* out_thr,
                           double* out_val) {
  FMX_TRY(check_calibrate(e, m, 0, m ? m->n : 0, n_groups, "fmx_calibrate_isotonic"));
  const int64_t n = m->n;
  FMX_TRY(check_bins(n_groups, n_bins));
  FMX_TRY(check_group_ids(group_of_row, n, n_groups, true));
  FMX_TRY(query_begin(e));
  if (n == 0) return FMX_OK;
  const size_t G = (size_t)n_groups, cells = G * (size_t)n_bins;
  void* const host[3] = {out_n_steps, out_thr, out_val};
  const size_t bytes[3] = {G * sizeof(int32_t), cells * sizeof(double), cells * sizeof(double)};
  DevBuf dg, buf[3];
  void* d[3] = {};
  FMX_TRY(stage_groups("fmx_calibrate_isotonic", &dg, group_of_row, n));
  for (int i = 0; i < 3; ++i) {
    if (!host[i]) continue;
    FMX_TRY(stage("fmx_calibrate_isotonic", &buf[i], bytes[i]));
    d[i] = buf[i].get();
  }
  FMX_TRY(isotonic_run(e, m, 0, n, (const uint32_t*)dg.get(), n_groups, n_bins, (int32_t*)d[0], (double*)d[1], (double*)d[2]));
  return copy_down(e, "fmx_calibrate_isotonic", host, d, bytes);
}

int fmx_calibrate_isotonic_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const void* dev_group_u32, int64_t n_groups, int32_t n_bins,
                                  void* dev_n_steps_i32, void* dev_thr_f64, void* dev_val_f64) {
  FMX_TRY(check_calibrate(e, m, r0, r1, n_groups, "fmx_calibrate_isotonic_device"));
  FMX_TRY(check_bins(n_groups, n_bins));
  FMX_CHECK(dev_group_u32 != nullptr || n_groups == 1, FMX_ERR_INVALID, "without group ids there is one group: n_groups must be 1 (got %lld)", (long long)n_groups);
  FMX_TRY(query_begin(e));
  if (r0 == r1) return FMX_OK;
  return isotonic_run(e, m, r0, r1, (const uint32_t*)dev_group_u32, n_groups, n_bins, (int32_t*)dev_n_steps_i32, (double*)dev_thr_f64, (double*)dev_val_f64);
}

// what fmx_fold_in and fmx_fold_in_pairs share once the engine / matrix pair is accepted: the checks of the ids and the lambdas, the solve, apply, the outputs
static int fold_in_checked(fmx_engine* e, const fmx_matrix* m, const uint32_t* ids, int64_t n_ids, double lambda_w, double lambda_v, int32_t n_newton, int32_t apply,
                           bool pairs, double* out_w, double* out_v, int64_t* out_count, int32_t* out_status) {
  FMX_CHECK(n_ids >= 0 && (n_ids == 0 || ids != nullptr), FMX_ERR_INVALID, "bad id list");
  FMX_CHECK(n_ids < (1LL << 31), FMX_ERR_INVALID, "too many fold features (%lld)", (long long)n_ids);
  FMX_CHECK(e->k <= 64, FMX_ERR_INVALID, "fold-in holds at most 64 factors (engine: %d)", e->k);
  FMX_CHECK(lambda_w >= 0.0 && lambda_v >= 0.0, FMX_ERR_INVALID, "lambda_w and lambda_v must be numbers >= 0");   // (a NaN fails both comparisons)
  FMX_CHECK(!(pairs || e->hyper.task == FMX_TASK_CLASSIFICATION) || n_newton >= 1, FMX_ERR_INVALID, "n_newton must be at least 1 (got %d)", n_newton);
  {
    std::vector<uint32_t> s(ids, ids + n_ids);
    std::sort(s.begin(), s.end());
    for (int64_t i = 0; i < n_ids; ++i) {
      FMX_CHECK((uint64_t)s[(size_t)i] < e->p, FMX_ERR_INVALID, "feature id %u out of range", s[(size_t)i]);
      FMX_CHECK(i == 0 || s[(size_t)i] != s[(size_t)i - 1], FMX_ERR_INVALID, "feature id %u is listed twice", s[(size_t)i]);
    }
  }
  FMX_TRY(use_device(e->cfg.device));
  if (n_ids == 0) return FMX_OK;   // (before the drain: an empty id list waits for nothing)
  FMX_TRY(query_begin(e));
  std::vector<double> theta;
  std::vector<int64_t> rows;
  std::vector<int32_t> status;
  FMX_TRY(foldin_run(e, m, ids, n_ids, lambda_w, lambda_v, n_newton, pairs, &theta, &rows, &status));
  const int k = e->k, D = 1 + k;
  if (apply) {
    // the solved rows only, through fmx_set_rows itself (rounding, replicas, the carried q of the ALS sweeps)
    std::vector<uint32_t> sid;
    std::vector<double> sw, sv;
    for (int64_t i = 0; i < n_ids; ++i) {
      if (status[(size_t)i] != 0) continue;
      sid.push_back(ids[i]);
      sw.push_back(theta[(size_t)i * D]);
      sv.insert(sv.end(), theta.begin() + (size_t)i * D + 1, theta.begin() + (size_t)(i + 1) * D);
    }
    if (!sid.empty()) FMX_TRY(fmx_set_rows(e, sid.data(), (int64_t)sid.size(), sw.data(), k > 0 ? sv.data() : nullptr));
  }
  for (int64_t i = 0; i < n_ids; ++i) {
    if (out_w) out_w[i] = theta[(size_t)i * D];
    if (out_v) for (int f = 0; f < k; ++f) out_v[f + i * k] = theta[(size_t)i * D + 1 + f];
    if (out_count) out_count[i] = rows[(size_t)i];
    if (out_status) out_status[i] = status[(size_t)i];
  }
  return FMX_OK;
}

int fmx_fold_in(fmx_engine* e, const fmx_matrix* m, const uint32_t* ids, int64_t n_ids, double lambda_w, double lambda_v, int32_t n_newton, int32_t apply,
                double* out_w, double* out_v, int64_t* out_rows, int32_t* out_status) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(m->has_labels && m->y != nullptr, FMX_ERR_INVALID, "fold-in needs a matrix with labels");
  FMX_CHECK(e->hyper.task == FMX_TASK_REGRESSION || e->hyper.task == FMX_TASK_CLASSIFICATION, FMX_ERR_INVALID,
            "fold-in solves REGRESSION and CLASSIFICATION engines only");
  return fold_in_checked(e, m, ids, n_ids, lambda_w, lambda_v, n_newton, apply, false, out_w, out_v, out_rows, out_status);
}

int fmx_fold_in_pairs(fmx_engine* e, const fmx_matrix* m, const uint32_t* ids, int64_t n_ids, double lambda_w, double lambda_v, int32_t n_newton, int32_t apply,
                      double* out_w, double* out_v, int64_t* out_pairs, int32_t* out_status) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(m->n % 2 == 0, FMX_ERR_INVALID, "a pair matrix holds rows 2t, 2t + 1: this matrix has an odd row count (%lld)", (long long)m->n);
  FMX_CHECK(e->hyper.task == FMX_TASK_RANKING, FMX_ERR_INVALID, "the pairwise fold-in solves RANKING engines only (fmx_fold_in solves the others)");
  return fold_in_checked(e, m, ids, n_ids, lambda_w, lambda_v, n_newton, apply, true, out_w, out_v, out_pairs, out_status);
}

static int check_heldout(const fmx_engine* e, const fmx_matrix* c, const fmx_matrix* items, const fmx_matrix* h, const fmx_matrix* x) {
  FMX_TRY(check_topk(e, c, items, x, 1, FMX_LINK_NONE));
  FMX_CHECK(h != nullptr, FMX_ERR_INVALID, "heldout is NULL");
  FMX_CHECK(h->n == c->n && (int64_t)h->p == items->n, FMX_ERR_INVALID, "heldout must be %lld x %lld (got %lld x %u)", (long long)c->n,
            (long long)items->n, (long long)h->n, h->p);
  FMX_CHECK(h->device == e->cfg.device, FMX_ERR_INVALID, "heldout lives on device %d, engine on %d", h->device, e->cfg.device);
  return FMX_OK;
}

int fmx_heldout_rank(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* heldout, const fmx_matrix* exclude,
                     int64_t* out_rank, double* out_score) {
  FMX_TRY(check_heldout(e, context, items, heldout, exclude));
  FMX_CHECK(out_rank != nullptr || heldout->nnz == 0, FMX_ERR_INVALID, "out_rank is NULL");
  FMX_TRY(query_begin(e));
  const int64_t nnz = heldout->nnz;
  if (nnz == 0) return FMX_OK;
  // one piece of nnz one-element "rows": the held-out entries of every context
  return staged(e, "fmx_heldout_rank", nnz, nnz, {Out{out_rank, sizeof(int64_t), 1}, Out{out_score, sizeof(double), 1}},
                [&](int64_t, int64_t, void* const* d) {
                  return heldout_run(e, context, 0, context->n, items, heldout, exclude, (int64_t*)d[0], (double*)d[1], nullptr, 0, nullptr);
                });
}

int fmx_heldout_rank_device(fmx_engine* e, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items, const fmx_matrix* heldout,
                            const fmx_matrix* exclude, void* dev_rank_i64, void* dev_score_f64) {
  FMX_TRY(check_heldout(e, context, items, heldout, exclude));
  FMX_TRY(check_rows(r0, r1, context->n, "context "));
  FMX_CHECK(dev_rank_i64 != nullptr || r0 == r1, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  return heldout_run(e, context, r0, r1, items, heldout, exclude, (int64_t*)dev_rank_i64, (double*)dev_score_f64, nullptr, 0, nullptr);
}

int fmx_heldout_metrics(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* heldout, const fmx_matrix* exclude,
                        const int32_t* ks, int32_t n_ks, double* out, double* per_context, int64_t* counted) {
  FMX_TRY(check_heldout(e, context, items, heldout, exclude));
  FMX_CHECK(ks != nullptr && n_ks >= 1 && n_ks <= 32, FMX_ERR_INVALID, "ks must hold 1..32 cut-offs (got %d)", (int)n_ks);
  for (int32_t q = 0; q < n_ks; ++q) FMX_CHECK(ks[q] >= 1, FMX_ERR_INVALID, "ks[%d] = %d: every K must be >= 1", (int)q, (int)ks[q]);
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  FMX_TRY(query_begin(e));
  const int cols = 4 * n_ks + 2;
  const int64_t n = context->n;
  if (n == 0) {
    for (int q = 0; q < cols; ++q) out[q] = std::nan("");
    if (counted) { counted[0] = 0; counted[1] = 0; }
    return FMX_OK;
  }
  // the per-context table stays on the device for the means; it is copied down whole only where the caller asks for it
  DevBuf pc;
  FMX_TRY(stage("fmx_heldout_metrics", &pc, (size_t)n * cols * sizeof(double)));
  std::vector<double> h_out((size_t)cols);
  int64_t h_cnt[2] = {0, 0};
  FMX_TRY(heldout_run(e, context, 0, n, items, heldout, exclude, nullptr, nullptr, ks, n_ks, (double*)pc.get()));
  FMX_TRY(heldout_means(e, (const double*)pc.get(), n, cols, h_out.data(), h_cnt));
  if (per_context) FMX_TRY(copy_down(e, "fmx_heldout_metrics", {(void*)per_context}, {pc.get()}, {(size_t)n * cols * sizeof(double)}));
  std::copy(h_out.begin(), h_out.end(), out);
  if (counted) { counted[0] = h_cnt[0]; counted[1] = h_cnt[1]; }
  return FMX_OK;
}

static int check_lists(const fmx_engine* e, const fmx_matrix* c, const fmx_matrix* items, const fmx_matrix* lists, int32_t top_k, int link) {
  FMX_TRY(check_topk(e, c, items, nullptr, top_k, link));
  FMX_CHECK(lists != nullptr, FMX_ERR_INVALID, "lists is NULL");
  FMX_CHECK(lists->n == c->n && (int64_t)lists->p == items->n, FMX_ERR_INVALID, "lists must be %lld x %lld (got %lld x %u)", (long long)c->n,
            (long long)items->n, (long long)lists->n, lists->p);
  FMX_CHECK(lists->device == e->cfg.device, FMX_ERR_INVALID, "lists lives on device %d, engine on %d", lists->device, e->cfg.device);
  return check_topk_factors(e);
}

// lists' row offsets on the host, and the context rows cut into pieces of at most `budget` entries (a longer list is a piece of its own)
static int lists_pieces(const fmx_matrix* lists, int64_t budget, std::vector<int64_t>* rp, std::vector<int64_t>* cut) {
  const int64_t n = lists->n;
  rp->resize((size_t)n + 1);
  FMX_HIP(hipMemcpy(rp->data(), lists->row_ptr, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  cut->assign(1, 0);
  while (cut->back() < n) {
    const int64_t a = cut->back();
    int64_t b = a + 1;
    while (b < n && (*rp)[b + 1] - (*rp)[a] <= budget) ++b;
    cut->push_back(b);
  }
  return FMX_OK;
}

int fmx_rank_lists(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* lists, int link, double* out_score,
                   int64_t* out_pos) {
  FMX_TRY(check_lists(e, context, items, lists, 1, link));
  FMX_CHECK(out_score != nullptr || lists->nnz == 0, FMX_ERR_INVALID, "out_score is NULL");
  FMX_TRY(query_begin(e));
  if (context->n == 0 || lists->nnz == 0) return FMX_OK;
  // contexts in pieces of at most 2^22 entries (the cut is by entries, not by rows: not staged()'s): the device staging stays at 64 MB unless
  // one list is longer
  std::vector<int64_t> rp, cut;
  FMX_TRY(lists_pieces(lists, 1LL << 22, &rp, &cut));
  int64_t most = 0;
  for (size_t i = 0; i + 1 < cut.size(); ++i) most = std::max(most, rp[cut[i + 1]] - rp[cut[i]]);
  DevBuf ds, dp;
  FMX_TRY(stage("fmx_rank_lists", &ds, (size_t)most * sizeof(double)));
  if (out_pos) FMX_TRY(stage("fmx_rank_lists", &dp, (size_t)most * sizeof(int64_t)));
  for (size_t i = 0; i + 1 < cut.size(); ++i) {
    const int64_t a = rp[cut[i]] - rp[0], cnt = rp[cut[i + 1]] - rp[cut[i]];
    if (cnt == 0) continue;
    FMX_TRY(lists_run(e, context, cut[i], cut[i + 1], items, lists, link, 0, (double*)ds.get(), (int64_t*)dp.get(), nullptr, nullptr));
    FMX_TRY(copy_down(e, "fmx_rank_lists", {(void*)(out_score + a), (void*)(out_pos ? out_pos + a : nullptr)}, {ds.get(), dp.get()},
                      {(size_t)cnt * sizeof(double), (size_t)cnt * sizeof(int64_t)}));
  }
  return FMX_OK;
}

int fmx_rank_lists_device(fmx_engine* e, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items, const fmx_matrix* lists, int link,
                          void* dev_score_f64, void* dev_pos_i64) {
  FMX_TRY(check_lists(e, context, items, lists, 1, link));
  FMX_TRY(check_rows(r0, r1, context->n, "context "));
  FMX_CHECK(dev_score_f64 != nullptr || r0 == r1 || lists->nnz == 0, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  if (lists->nnz == 0) return FMX_OK;
  return lists_run(e, context, r0, r1, items, lists, link, 0, (double*)dev_score_f64, (int64_t*)dev_pos_i64, nullptr, nullptr);
}

int fmx_topk_lists(fmx_engine* e, const fmx_matrix* context, const fmx_matrix* items, const fmx_matrix* lists, int32_t top_k, int link,
                   int64_t* out_index, double* out_score) {
  FMX_TRY(check_lists(e, context, items, lists, top_k, link));
  FMX_CHECK((out_index && out_score) || context->n == 0, FMX_ERR_INVALID, "out_index / out_score is NULL");
  FMX_TRY(query_begin(e));
  if (context->n == 0) return FMX_OK;
  return staged(e, "fmx_topk_lists", context->n, slot_rows(top_k), {Out{out_index, sizeof(int64_t), top_k}, Out{out_score, sizeof(double), top_k}},
                [&](int64_t a, int64_t b, void* const* d) {
                  return lists_run(e, context, a, b, items, lists, link, top_k, nullptr, nullptr, (int64_t*)d[0], (double*)d[1]);
                });
}

int fmx_topk_lists_device(fmx_engine* e, const fmx_matrix* context, int64_t r0, int64_t r1, const fmx_matrix* items, const fmx_matrix* lists,
                          int32_t top_k, int link, void* dev_index_i64, void* dev_score_f64) {
  FMX_TRY(check_lists(e, context, items, lists, top_k, link));
  FMX_TRY(check_rows(r0, r1, context->n, "context "));
  FMX_CHECK((dev_index_i64 && dev_score_f64) || r0 == r1, FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  return lists_run(e, context, r0, r1, items, lists, link, top_k, nullptr, nullptr, (int64_t*)dev_index_i64, (double*)dev_score_f64);
}

int fmx_project(fmx_engine* e, const fmx_matrix* m, int32_t with_w0, double* out_base, double* out_s) {
  FMX_TRY(check_pair(e, m));
  FMX_CHECK(m->n == 0 || (out_base != nullptr && (out_s != nullptr || e->k == 0)), FMX_ERR_INVALID, "out_base / out_s is NULL");
  FMX_TRY(query_begin(e));
  if (m->n == 0) return FMX_OK;
  // rows in pieces of 2^16, the chunk of project_run itself
  return staged(e, "fmx_project", m->n, 1 << 16, {Out{out_base, sizeof(double), 1}, Out{out_s, sizeof(double), e->k}},
                [&](int64_t a, int64_t b, void* const* d) { return project_run(e, m, a, b, with_w0 != 0, (double*)d[0], (double*)d[1]); });
}

int fmx_project_device(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, int32_t with_w0, void* dev_base_f64, void* dev_s_f64) {
  FMX_TRY(check_pair(e, m));
  FMX_TRY(check_rows(r0, r1, m->n, ""));
  FMX_CHECK(r0 == r1 || (dev_base_f64 != nullptr && (dev_s_f64 != nullptr || e->k == 0)), FMX_ERR_INVALID, "NULL output");
  FMX_TRY(query_begin(e));
  return project_run(e, m, r0, r1, with_w0 != 0, (double*)dev_base_f64, (double*)dev_s_f64);
}

static int check_diversify(const fmx_engine* e, const fmx_matrix* items, int64_t n, int32_t pool, int32_t top_k, double lambda, int32_t relevance) {
  FMX_TRY(check_topk(e, items, items, nullptr, 1, FMX_LINK_NONE));
  FMX_CHECK(n >= 0, FMX_ERR_INVALID, "n must be >= 0 (got %lld)", (long long)n);
  FMX_CHECK(pool >= 1 && pool <= 1024, FMX_ERR_INVALID, "pool must be in 1..1024 (got %d)", (int)pool);
  FMX_CHECK(top_k >= 1 && top_k <= pool, FMX_ERR_INVALID, "top_k must be in 1..pool = %d (got %d)", (int)pool, (int)top_k);
  FMX_CHECK(lambda >= 0.0 && lambda <= 1.0, FMX_ERR_INVALID, "lambda must be in [0, 1] (got %g)", lambda);  // (NaN fails both comparisons)
  FMX_CHECK(relevance == FMX_DIV_REL_SCORE || relevance == FMX_DIV_REL_MINMAX, FMX_ERR_INVALID, "unknown relevance mode %d", (int)relevance);
  return check_topk_factors(e);
}

// (the host form is staged inside diversify_run: it projects the items once per call, not once per piece)
int fmx_diversify(fmx_engine* e, const fmx_matrix* items, int64_t n, int32_t pool, const int64_t* index, const double* score, int32_t top_k, double lambda,
                  int32_t relevance, int64_t* out_index, double* out_score, double* out_margin) {
  FMX_TRY(check_diversify(e, items, n, pool, top_k, lambda, relevance));
  FMX_CHECK((index && score && out_index && out_score) || n == 0, FMX_ERR_INVALID, "index / score / out_index / out_score is NULL");
  for (int64_t t = 0; t < n * pool; ++t)
    FMX_CHECK(index[t] == -1 || (index[t] >= 0 && index[t] < items->n), FMX_ERR_INVALID, "index[%lld][%lld] = %lld is neither -1 nor an item row (0..%lld)",
              (long long)(t / pool), (long long)(t % pool), (long long)index[t], (long long)items->n - 1);
  FMX_TRY(query_begin(e));
  if (n == 0) return FMX_OK;
  return diversify_run(e, items, n, pool, index, score, top_k, lambda, relevance, out_index, out_score, out_margin, true);
}

int fmx_diversify_device(fmx_engine* e, const fmx_matrix* items, int64_t n, int32_t pool, const void* dev_index_i64, const void* dev_score_f64, int32_t top_k,
                         double lambda, int32_t relevance, void* dev_out_index_i64, void* dev_out_score_f64, void* dev_out_margin_f64) {
  FMX_TRY(check_diversify(e, items, n, pool, top_k, lambda, relevance));
  FMX_CHECK((dev_index_i64 && dev_score_f64 && dev_out_index_i64 && dev_out_score_f64) || n == 0, FMX_ERR_INVALID, "NULL input or output");
  FMX_TRY(query_begin(e));
  if (n == 0) return FMX_OK;
  return diversify_run(e, items, n, pool, (const int64_t*)dev_index_i64, (const double*)dev_score_f64, top_k, lambda, relevance, (int64_t*)dev_out_index_i64,
                       (double*)dev_out_score_f64, (double*)dev_out_margin_f64, false);
}

}  // extern "C"
