/*
 * ref_harness.cpp -- drives the reference's own classes on one case file and writes one result file.
 *
 * TEST INFRASTRUCTURE ONLY, and only where the reference tree is present: `make -C oracle ref` compiles this single
 * translation unit against the reference's unmodified FM.h (through the stand-in Rcpp.h beside this file) into
 * oracle/_ref/ref_harness.  tests/golden/make_ref_golden.py runs it once per case (one process per case, so libc
 * rand() is always in the state of srand(1)) and freezes what it writes under tests/golden/.
 *
 *   ref_harness CASE_FILE RESULT_FILE
 *
 * Both files are a flat list of named arrays (see read_pack / write_pack): u32 name length, name, one type byte
 * ('d' f64, 'f' f32, 'i' i32, 'u' u32, 'l' i64), u64 count, the raw little-endian elements.  Scalars are arrays of
 * one element.  The array "op" picks what runs:
 *   1 learn     SGD / FTRL / TDAP / ALS / MCMC learner, tracker on or off
 *   2 forward   Model::predict per row, predict_batch, predict_prob, and Tracker::report (the clamp) on one snapshot
 *   3 evaluate  evaluates() on a given y_hat, y for a list of (task, metric)
 *   4 matrix    SMatrix::scales, normalize, transpose
 *   5 als_v     update_v_lambda / update_v_mu / update_v of the ALS or MCMC learner, reached through a subclass
 *   6 order     the row visiting order of the learners' loop, from the reference's random_select
 *
 * Rf_rnorm / Rf_rgamma are defined here: deterministic, and every draw's STANDARD variate is logged ("norm_z",
 * "gamma_z") so that code taking caller-drawn variates can be fed exactly what the reference consumed.
 */
#include "FM.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>

namespace {

/* ------------------------------------------------------------------ the case / result container */
struct Arr {
  char type;
  std::vector<char> bytes;
  uint64_t count;
};
typedef std::map<std::string, Arr> Pack;
std::vector<std::string> g_out_order;

size_t elem_size(char t) { return (t == 'd' || t == 'l') ? 8 : 4; }

Pack read_pack(const char* path) {
  Pack pk;
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  for (;;) {
    uint32_t nl;
    if (!f.read((char*)&nl, 4)) break;
    std::string name(nl, ' ');
    f.read(&name[0], nl);
    Arr a;
    f.read(&a.type, 1);
    f.read((char*)&a.count, 8);
    a.bytes.resize(a.count * elem_size(a.type));
    f.read(a.bytes.data(), (std::streamsize)a.bytes.size());
    if (!f) throw std::runtime_error("truncated case file at " + name);
    pk[name] = a;
  }
  return pk;
}

void write_pack(const char* path, const Pack& pk) {
  std::ofstream f(path, std::ios::binary);
  for (size_t i = 0; i < g_out_order.size(); ++i) {
    const std::string& name = g_out_order[i];
    const Arr& a = pk.at(name);
    uint32_t nl = (uint32_t)name.size();
    f.write((const char*)&nl, 4);
    f.write(name.data(), nl);
    f.write(&a.type, 1);
    f.write((const char*)&a.count, 8);
    f.write(a.bytes.data(), (std::streamsize)a.bytes.size());
  }
  if (!f) throw std::runtime_error(std::string("cannot write ") + path);
}

template <typename T>
void put(Pack& pk, const std::string& name, char type, const T* p, size_t n) {
  Arr a;
  a.type = type;
  a.count = n;
  a.bytes.resize(n * sizeof(T));
  if (n) std::memcpy(a.bytes.data(), p, n * sizeof(T));
  if (!pk.count(name)) g_out_order.push_back(name);
  pk[name] = a;
}
void put_d(Pack& pk, const std::string& name, const std::vector<double>& v) { put(pk, name, 'd', v.data(), v.size()); }
void put_d(Pack& pk, const std::string& name, double v) { put(pk, name, 'd', &v, 1); }
void put_l(Pack& pk, const std::string& name, const std::vector<int64_t>& v) { put(pk, name, 'l', v.data(), v.size()); }

bool has(const Pack& pk, const std::string& name) { return pk.count(name) != 0; }

/* any numeric array as doubles */
std::vector<double> get(const Pack& pk, const std::string& name) {
  if (!has(pk, name)) throw std::runtime_error("case lacks " + name);
  const Arr& a = pk.at(name);
  std::vector<double> r(a.count);
  for (uint64_t i = 0; i < a.count; ++i) {
    const char* p = a.bytes.data() + i * elem_size(a.type);
    switch (a.type) {
      case 'd': { double x; std::memcpy(&x, p, 8); r[i] = x; break; }
      case 'f': { float x; std::memcpy(&x, p, 4); r[i] = x; break; }
      case 'i': { int32_t x; std::memcpy(&x, p, 4); r[i] = x; break; }
      case 'u': { uint32_t x; std::memcpy(&x, p, 4); r[i] = x; break; }
      case 'l': { int64_t x; std::memcpy(&x, p, 8); r[i] = (double)x; break; }
      default: throw std::runtime_error("unknown type in " + name);
    }
  }
  return r;
}
double num(const Pack& pk, const std::string& name) { return get(pk, name).at(0); }
double num(const Pack& pk, const std::string& name, double dflt) { return has(pk, name) ? num(pk, name) : dflt; }

/* ------------------------------------------------------------------ the random entry points of R's C API */
uint64_t g_lcg = 12345;
std::vector<double> g_norm_z, g_gamma_z;

double lcg_unif() { /* Knuth's MMIX multiplier; 53 bits, never 0 or 1 */
  g_lcg = g_lcg * 6364136223846793005ULL + 1442695040888963407ULL;
  return ((double)(g_lcg >> 11) + 0.5) / 9007199254740992.0;
}
bool g_init_draw = false; /* inside Model::init() of a case that asks for a drawn V */
double std_normal() { /* Box-Muller, cosine branch */
  double a = lcg_unif();
  double b = lcg_unif();
  return std::sqrt(-2.0 * std::log(a)) * std::cos(2.0 * M_PI * b);
}
double std_gamma(double shape) { /* Marsaglia & Tsang 2000; shape < 1 by the usual boost */
  if (shape < 1.0) {
    double u = lcg_unif();
    return std_gamma(shape + 1.0) * std::pow(u, 1.0 / shape);
  }
  const double d = shape - 1.0 / 3.0, c = 1.0 / std::sqrt(9.0 * d);
  for (;;) {
    double x, v;
    do {
      x = std_normal();
      v = 1.0 + c * x;
    } while (v <= 0.0);
    v = v * v * v;
    double u = lcg_unif();
    if (u < 1.0 - 0.0331 * x * x * x * x) return d * v;
    if (std::log(u) < 0.5 * x * x + d * (1.0 - v + std::log(v))) return d * v;
  }
}

}  // namespace

double Rf_rnorm(double mean, double sd) {
  if (g_init_draw) { /* SURVEY.md Appendix B writes its V0 as mu + sd*sqrt(-2 ln a)*cos(2 pi b): that association, not mean + sd*z */
    double a = lcg_unif();
    double b = lcg_unif();
    return mean + sd * std::sqrt(-2.0 * std::log(a)) * std::cos(2.0 * M_PI * b);
  }
  double z = std_normal();
  g_norm_z.push_back(z);
  return mean + sd * z;
}
double Rf_rgamma(double shape, double scale) {
  double z = std_gamma(shape);
  g_gamma_z.push_back(z);
  return scale * z;
}

namespace {

/* ------------------------------------------------------------------ inputs into the reference's own containers */
/* col_idx / value get one spare element: the Iterator reads one past a row's end before it tests for the end */
void fill_matrix(const Pack& pk, SMatrix<float>& X) {
  std::vector<double> rp = get(pk, "row_ptr"), col = get(pk, "col"), val = get(pk, "val");
  X.dim1 = (uint)rp.size() - 1;
  X.dim2 = (uint)num(pk, "p");
  X.size = (uint)col.size();
  X.transposed = false;
  X.row_idx.setSize(X.dim1 + 1);
  for (uint i = 0; i <= X.dim1; ++i) X.row_idx[i] = (uint)rp[i];
  X.col_idx.setSize(X.size + 1);
  X.value.setSize(X.size + 1);
  for (uint i = 0; i < X.size; ++i) { X.col_idx[i] = (uint)col[i]; X.value[i] = (float)val[i]; }
  X.col_idx[X.size] = 0;
  X.value[X.size] = 0.0f;
}

void fill_target(const Pack& pk, DVector<float>& y) {
  std::vector<double> v = get(pk, "y");
  y.setSize((uint)v.size());
  for (uint i = 0; i < y.size(); ++i) y[i] = (float)v[i];
}

void fill_model(const Pack& pk, Model& model, uint p) {
  model.SOLVER = (int)num(pk, "solver");
  model.TASK = (int)num(pk, "task");
  model.num_attribute = p;
  model.num_factor = (uint)num(pk, "k");
  model.k0 = num(pk, "k0", 1) != 0;
  model.k1 = num(pk, "k1", 1) != 0;
  model.l1_regw = num(pk, "l1_regw", 0);
  model.l1_regv = num(pk, "l1_regv", 0);
  model.l2_reg0 = num(pk, "l2_reg0", 0);
  model.l2_regw = num(pk, "l2_regw", 0);
  model.l2_regv = num(pk, "l2_regv", 0);
  model.init_mean = num(pk, "init_mean", 0);
  model.init_stdev = num(pk, "init_stdev", 0.01);
  model.nthreads = 1;
  g_init_draw = num(pk, "draw_v", 0) != 0;
  model.init(); /* sizes w, v and the scratch sums; draws V from Rf_rnorm */
  g_init_draw = false;
  if (num(pk, "draw_v", 0) == 0) {
    g_norm_z.clear(); /* V is an input: the draws of init() are not part of the case */
    model.w0 = num(pk, "w0_in", 0);
    std::vector<double> w = get(pk, "w_in"), v = get(pk, "v_in");
    if (w.size() != p || v.size() != (size_t)model.num_factor * p) throw std::runtime_error("w_in / v_in have the wrong size");
    for (uint j = 0; j < p; ++j) model.w[j] = w[j];
    for (uint f = 0; f < model.num_factor; ++f)
      for (uint j = 0; j < p; ++j) model.v(f, j) = v[(size_t)f * p + j];
  }
}

std::vector<double> flat_v(const DMatrix<double>& v, uint k, uint p) {
  std::vector<double> r((size_t)k * p);
  for (uint f = 0; f < k; ++f)
    for (uint j = 0; j < p; ++j) r[(size_t)f * p + j] = v(f, j);
  return r;
}
std::vector<double> flat(const DVector<double>& w) { return std::vector<double>(w.begin(), w.end()); }

void put_model(Pack& out, Model& model) {
  put_d(out, "w0", model.w0);
  put_d(out, "w", flat(model.w));
  put_d(out, "v", flat_v(model.v, model.num_factor, model.num_attribute));
}

void put_tracker(Pack& out, Learner& L, Model& model) {
  Tracker& t = L.tracker;
  if (t.step_size <= 0) return;
  std::vector<int64_t> idx;
  std::vector<double> ev, sw0, sw, sv;
  for (int r = 0; r < t.record_cnter; ++r) {
    idx.push_back(t.record_index[r]);
    ev.push_back(t.evaluations_of_train[r]);
    Params& P = t.parameters[r];
    sw0.push_back(model.k0 ? P.w0 : 0.0);
    if (model.k1) { std::vector<double> w = flat(P.w); sw.insert(sw.end(), w.begin(), w.end()); }
    if (model.num_factor > 0) { std::vector<double> v = flat_v(P.v, model.num_factor, model.num_attribute); sv.insert(sv.end(), v.begin(), v.end()); }
  }
  put_l(out, "rec_index", idx);
  put_d(out, "rec_eval", ev);
  put_d(out, "snap_w0", sw0);
  put_d(out, "snap_w", sw);
  put_d(out, "snap_v", sv);
  put_d(out, "step_size_used", t.step_size);
}

/* the protected updates of the ALS / MCMC learner */
template <typename Base>
class Opened : public Base {
 public:
  using Base::update_v;
  using Base::update_v_lambda;
  using Base::update_v_mu;
};

void common_learner(const Pack& pk, Learner& L, Model& model, DataMetaInfo& groups, Data& train) {
  L.meta = &groups;
  L.fm = &model;
  L.min_target = num(pk, "min_target", train.min_target);
  L.max_target = num(pk, "max_target", train.max_target);
  L.nthreads = 1;
  L.max_iter = (int)num(pk, "max_iter");
  L.tracker.step_size = (int)num(pk, "trace_step", -1);
  L.tracker.max_iter = L.max_iter;
  L.type = (int)num(pk, "eval_type", LL);
  L.tracker.type = L.type;
  L.conv_condition = num(pk, "conv_condition", 1e-4);
}

template <typename LearnerT>
void mcmc_als_hyper(const Pack& pk, LearnerT& L) { /* after init(): the shipped driver assigns them before it and loses them */
  L.alpha_0 = num(pk, "alpha_0", L.alpha_0);
  L.gamma_0 = num(pk, "gamma_0", L.gamma_0);
  L.beta_0 = num(pk, "beta_0", L.beta_0);
  L.mu_0 = num(pk, "mu_0", L.mu_0);
  L.alpha = num(pk, "alpha", L.alpha);
  L.w0_mean_0 = num(pk, "w0_mean_0", L.w0_mean_0);
}

/* ------------------------------------------------------------------ op 1 */
void op_learn(const Pack& pk, Pack& out) {
  SMatrix<float> X, Xt;
  fill_matrix(pk, X);
  DVector<float> y;
  fill_target(pk, y);
  Data train;
  train.add_data(&X);
  train.add_target(&y);
  Model model;
  fill_model(pk, model, X.ncol());
  if (num(pk, "draw_v", 0) != 0) put_d(out, "v_init", flat_v(model.v, model.num_factor, model.num_attribute));
  DataMetaInfo groups(train.num_features);
  Learner* base = NULL;
  SGD_Learner sgd;
  FTRL_Learner ftrl;
  TDAP_Learner tdap;
  ALS_Learner als;
  MCMC_Learner mcmc;
  switch (model.SOLVER) {
    case SGD:
      base = &sgd;
      common_learner(pk, sgd, model, groups, train);
      sgd.learn_rate = num(pk, "learn_rate");
      sgd.random_step = (int)num(pk, "random_step", 1);
      sgd.init();
      break;
    case FTRL:
      base = &ftrl;
      common_learner(pk, ftrl, model, groups, train);
      ftrl.alpha_w = num(pk, "alpha_w", ftrl.alpha_w);
      ftrl.alpha_v = num(pk, "alpha_v", ftrl.alpha_v);
      ftrl.beta_w = num(pk, "beta_w", ftrl.beta_w);
      ftrl.beta_v = num(pk, "beta_v", ftrl.beta_v);
      ftrl.random_step = (int)num(pk, "random_step", 1);
      ftrl.init();
      break;
    case TDAP:
      base = &tdap;
      common_learner(pk, tdap, model, groups, train);
      tdap.gamma = num(pk, "gamma", tdap.gamma);
      tdap.alpha_w = num(pk, "alpha_w", tdap.alpha_w);
      tdap.alpha_v = num(pk, "alpha_v", tdap.alpha_v);
      tdap.random_step = (int)num(pk, "random_step", 1);
      tdap.init();
      break;
    case ALS:
      base = &als;
      common_learner(pk, als, model, groups, train);
      als.init();
      mcmc_als_hyper(pk, als);
      break;
    case MCMC:
      base = &mcmc;
      common_learner(pk, mcmc, model, groups, train);
      mcmc.init();
      mcmc_als_hyper(pk, mcmc);
      break;
    default:
      throw std::runtime_error("unknown solver");
  }
  if (model.SOLVER <= ALS) {
    X.transpose(Xt);
    train.add_data(&Xt);
  }
  base->learn(train);
  put_model(out, model);
  if (num(pk, "with_pred", 0) != 0) { /* the final model's raw predictions, for the sign check of the device paths */
    DVector<double> o(train.num_cases);
    model.predict_batch(train, o);
    put_d(out, "pred", flat(o));
  }
  put_d(out, "convergent", base->convergent ? 1.0 : 0.0);
  put_tracker(out, *base, model);
  if (model.SOLVER == MCMC) {
    put_d(out, "alpha", mcmc.alpha);
    put_d(out, "w_lambda", mcmc.w_lambda[0]);
    put_d(out, "w_mu", mcmc.w_mu[0]);
  }
}

/* ------------------------------------------------------------------ op 2 */
void op_forward(const Pack& pk, Pack& out) {
  SMatrix<float> X;
  fill_matrix(pk, X);
  DVector<float> y;
  fill_target(pk, y);
  Data train;
  train.add_data(&X);
  train.add_target(&y);
  Model model;
  fill_model(pk, model, X.ncol());
  uint n = X.nrow();
  std::vector<double> row(n);
  for (uint i = 0; i < n; ++i) {
    SMatrix<float>::Iterator it(X, i);
    row[i] = model.predict(it);
  }
  put_d(out, "pred_row", row);
  DVector<double> o(n);
  model.predict_batch(train, o);
  put_d(out, "pred_batch", flat(o));
  model.predict_prob(train, o);
  put_d(out, "prob", flat(o));
  /* Tracker::report on one snapshot: the regression clamp (or the link) followed by the metric */
  std::vector<double> types = get(pk, "eval_types"), rep;
  for (size_t t = 0; t < types.size(); ++t) {
    Tracker tr;
    tr.type = (int)types[t];
    tr.step_size = 1;
    tr.max_iter = 1;
    tr.init();
    tr.record(&model, 0, 0.0);
    tr.record_times = 1;
    tr.report(&model, train, num(pk, "min_target", train.min_target), num(pk, "max_target", train.max_target));
    rep.push_back(tr.evaluations_of_test[0]);
  }
  put_d(out, "report_eval", rep);
}

/* ------------------------------------------------------------------ op 3 */
void op_evaluate(const Pack& pk, Pack& out) {
  std::vector<double> yh = get(pk, "y_hat"), tasks = get(pk, "tasks"), types = get(pk, "types"), r;
  DVector<double> y_hat((uint)yh.size());
  for (uint i = 0; i < y_hat.size(); ++i) y_hat[i] = yh[i];
  DVector<float> y;
  fill_target(pk, y);
  Model model;
  for (size_t t = 0; t < types.size(); ++t) {
    model.TASK = (int)tasks[t];
    r.push_back(evaluates(&model, y_hat, y, (int)types[t]));
  }
  put_d(out, "eval", r);
}

/* ------------------------------------------------------------------ op 4 */
std::vector<double> values_of(const SMatrix<float>& X) {
  std::vector<double> r(X.size);
  for (uint i = 0; i < X.size; ++i) r[i] = X.value[i];
  return r;
}
void op_matrix(const Pack& pk, Pack& out) {
  {
    SMatrix<float> X;
    fill_matrix(pk, X);
    std::vector<double> nc = get(pk, "norm_columns");
    IntegerVector cols((int)nc.size() + 1); /* scales() looks one past the last listed column */
    for (size_t i = 0; i < nc.size(); ++i) cols[i] = (int)nc[i];
    cols[nc.size()] = -1;
    List s = X.scales(cols);
    NumericVector mean = as<NumericVector>(s["mean"]), sd = as<NumericVector>(s["std"]);
    put_d(out, "scaled_val", values_of(X));
    put_d(out, "mean", std::vector<double>(mean.begin(), mean.end()));
    put_d(out, "std", std::vector<double>(sd.begin(), sd.end()));
  }
  {
    SMatrix<float> X;
    fill_matrix(pk, X);
    X.value.resetSize(X.size); /* normalize() walks value.size() entries */
    List s = List::create(_["mean"] = get(pk, "norm_mean"), _["std"] = get(pk, "norm_std"));
    X.normalize(s);
    put_d(out, "normalized_val", values_of(X));
  }
  if (num(pk, "do_transpose", 1) != 0) {
    SMatrix<float> X, Xt;
    fill_matrix(pk, X);
    X.transpose(Xt);
    std::vector<int64_t> rp(Xt.row_idx.begin(), Xt.row_idx.end()), ci(Xt.col_idx.begin(), Xt.col_idx.end());
    put_l(out, "t_row_ptr", rp);
    put_l(out, "t_col", ci);
    put_d(out, "t_val", values_of(Xt));
  }
}

/* ------------------------------------------------------------------ op 5 */
template <typename LearnerT>
void run_als_v(const Pack& pk, Pack& out) {
  SMatrix<float> X, Xt;
  fill_matrix(pk, X);
  DVector<float> y;
  fill_target(pk, y);
  Data train;
  train.add_data(&X);
  train.add_target(&y);
  X.transpose(Xt);
  train.add_data(&Xt);
  Model model;
  fill_model(pk, model, X.ncol());
  DataMetaInfo groups(train.num_features);
  Opened<LearnerT> L;
  common_learner(pk, L, model, groups, train);
  L.init();
  mcmc_als_hyper(pk, L);
  uint k = model.num_factor;
  if (has(pk, "v_lambda")) {
    std::vector<double> lam = get(pk, "v_lambda"), mu = get(pk, "v_mu");
    for (uint f = 0; f < k; ++f) { L.v_lambda(0, f) = lam[f]; L.v_mu(0, f) = mu[f]; }
  }
  if (num(pk, "do_hyper", 0) != 0) { /* the order of the block that update_all keeps commented out */
    L.update_v_lambda();
    L.update_v_mu();
  }
  std::vector<double> lam(k), mu(k);
  for (uint f = 0; f < k; ++f) { lam[f] = L.v_lambda(0, f); mu[f] = L.v_mu(0, f); }
  put_d(out, "v_lambda_out", lam);
  put_d(out, "v_mu_out", mu);
  if (num(pk, "do_sweep", 1) != 0) {
    std::vector<double> e = get(pk, "err_in");
    DVector<double> err((uint)e.size()), vq((uint)e.size());
    for (uint i = 0; i < err.size(); ++i) err[i] = e[i];
    vq.init(0.0);
    L.update_v(train, err, vq);
  }
  put_model(out, model);
}
void op_als_v(const Pack& pk, Pack& out) {
  if ((int)num(pk, "solver") == MCMC) run_als_v<MCMC_Learner>(pk, out);
  else run_als_v<ALS_Learner>(pk, out);
}

/* ------------------------------------------------------------------ op 6 */
void op_order(const Pack& pk, Pack& out) {
  uint n = (uint)num(pk, "n");
  int step = (int)num(pk, "random_step"), max_iter = (int)num(pk, "max_iter");
  std::vector<int64_t> order;
  while ((int)order.size() < max_iter && n > 1) {
    for (uint i = random_select(step); i < n; i += random_select(step)) {
      order.push_back(i);
      if ((int)order.size() >= max_iter) break;
    }
  }
  put_l(out, "order", order);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s CASE_FILE RESULT_FILE\n", argv[0]);
    return 2;
  }
  try {
    Pack pk = read_pack(argv[1]), out;
    switch ((int)num(pk, "op")) {
      case 1: op_learn(pk, out); break;
      case 2: op_forward(pk, out); break;
      case 3: op_evaluate(pk, out); break;
      case 4: op_matrix(pk, out); break;
      case 5: op_als_v(pk, out); break;
      case 6: op_order(pk, out); break;
      default: throw std::runtime_error("unknown op");
    }
    put_d(out, "norm_z", g_norm_z);
    put_d(out, "gamma_z", g_gamma_z);
    write_pack(argv[2], out);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "ref_harness: %s\n", e.what());
    return 1;
  }
  return 0;
}
