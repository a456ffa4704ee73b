// Calibration of a CLASSIFICATION engine's probabilities per row group (fmx_predict_calibrated*, fmx_reliability*, fmx_calibrate_platt*,
// fmx_calibrate_isotonic*): measure, fit, apply.  include/fmx.h has the definitions to the bit; tests/calibrate_model.py
// restates them in numpy.
//
// For the rows [r0, r1) of a labelled matrix: z_r is the raw forward (forward_rows, FMX_LINK_NONE), g_r the row's group (a row whose id is >= G
// belongs to no group), p_r = cal_apply(z_r, g_r) the calibrated probability.  Scores are compared under mt_key's order (rank_order_key read
// upwards: -0 == +0).  A row is `valid` iff it has a group and p_r is a number (a NaN z gives a NaN p under every kind).
//
//   table      one forward, then cal_rows_k: p_r, the valid flag, the NaN rows per group (64-bit integer atomics) and the sort keys.
//              WIDTH: the cell c = g B + bin is known per row; one stable radix sort by c (an invalid row: c = G B, a bucket nobody reads)
//              leaves a cell's rows contiguous and ascending.  MASS: a 64-bit radix sort by mt_key(z), a stable one by group ((group, key, row)
//              order), the tie-run heads by a max-scan (as mt_long_flags_k), bin = floor((head - first of the group) B / s): the cell is again
//              ascending along the sorted rows.  cell offsets by binary search (group_offsets over G B + 1 cells).
//   sums       THE ORDER OF EVERY FLOATING-POINT SUM.  A cell's row list (ascending rows under WIDTH, ascending (key, row) under MASS) is cut
//              into chunks of CAL_CHUNK = 1 024 rows.  A workgroup sums one chunk (cal_sums_k, mt_sums_k's scheme): thread t adds the terms of
//              positions t, t + 256, t + 512, t + 768 in that order from +0.0, the 64 lanes of a wave by an xor butterfly (every lane holds the
//              same bits), the four waves in wave order.  cal_cells_k adds a cell's chunk sums in ascending order from +0.0: sum_p and the
//              cell's Brier and log-loss sums.  cal_groups_k (one thread per group) adds the group's non-empty cells' Brier and log-loss sums
//              b ascending from +0.0 and divides once by (double) s; ECE and MCE from the table as include/fmx.h writes them.  Every term and
//              every step is an individually rounded fp64 operation; nothing is added by floating-point atomics.  The order is a function of
//              the group's own rows (and B, the binning and the map) alone.  Positives are integer sums; lo_z / hi_z are the minimum and
//              maximum of a total order on the bits (-0 below +0), so they are order-free.
//   platt      rows with a group and a finite z, stably sorted by group; a group's ascending row list in chunks of CAL_CHUNK rows.  Per
//              Newton step platt_sums_k writes the five sums of every (group, chunk) in the order above; platt_solve_k (one thread per group)
//              adds a group's chunks ascending from +0.0, adds the ridge, solves the 2 x 2 system by Cholesky and writes (a, b).
//              status 0 says that every pivot of every step was positive and finite.  It does NOT say that the steps converged, that the loss
//              went down (there is no line search) or that (a, b) is small: on a separable or one-class group the undamped steps overshoot
//              (40 rows of one class with scores spread over -6 .. 8 end near a = 930 after 8 steps at lambda 0.1).
//   isotonic   the MASS table without the sums, then one thread per group pools adjacent violators over the non-empty bins in place (the
//              block stack never runs ahead of the bin being read, so it lives in the count table itself): no per-thread array, no scratch.
#include <algorithm>
#include <atomic>
#include <vector>

#include "fm_prims.h"

namespace fmx {
namespace {

constexpr int CAL_THREADS = 256;
constexpr int CAL_WAVES = CAL_THREADS / 64;
constexpr int CAL_CHUNK = 4 * CAL_THREADS;    // rows per chunk of the sums
constexpr int64_t CAL_FWD_ROWS = 1LL << 24;   // rows per forward call

std::atomic<int64_t> g_cal_chunk_rows{0};

// ascending in this key = ascending in z; NaN is 0, below every number; -0 and +0 share a key (fm_metrics.hip's mt_key)
__device__ __forceinline__ uint64_t cal_key(double z) { return ~rank_order_key(z); }
// a total order on the bits of the numbers, -0 below +0: what lo_z / hi_z are the minimum / maximum of
__device__ __forceinline__ uint64_t cal_bits_key(double z) {
  const uint64_t u = (uint64_t)__double_as_longlong(z);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double cal_bits_unkey(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
__device__ __forceinline__ double cal_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// the calibrator on the device
struct CalDev {
  int kind, link, max_steps;
  int64_t G;                 // 1: one map for every row
  const double* platt;
  const int32_t* n_steps;
  const double *thr, *val;
  Hyper h;
  const double* pn_y;
};

// p of a row with score z in group g (g < the call's n_groups)
__device__ __forceinline__ double cal_apply(const CalDev& c, double z, int64_t g) {
  if (z != z) return z;
  if (c.kind == FMX_CAL_NONE) return rank_link(c.h, z, c.link, c.pn_y);
  const int64_t gi = c.G == 1 ? 0 : g;
  if (c.kind == FMX_CAL_PLATT) {
    const double a = c.platt[2 * gi], b = c.platt[2 * gi + 1];
    if (a != a || b != b) return cal_nan();
    return rank_link(c.h, __dadd_rn(__dmul_rn(a, z), b), FMX_LINK_LOGISTIC, nullptr);
  }
  // STEPS: the last step whose threshold is <= z under the key order
  const int ns = c.n_steps[gi];
  const double* thr = c.thr + (size_t)gi * c.max_steps;
  const uint64_t kz = cal_key(z);
  int lo = 0, hi = ns;   // the first step with thr > z
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cal_key(thr[mid]) <= kz) lo = mid + 1; else hi = mid;
  }
  return lo == 0 ? cal_nan() : c.val[(size_t)gi * c.max_steps + lo - 1];
}

__global__ __launch_bounds__(CAL_THREADS) void cal_predict_k(CalDev c, const double* __restrict__ z, const uint32_t* __restrict__ grp, int64_t n, int64_t G,
                                                            double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t g = grp ? (int64_t)grp[i] : 0;
  out[i] = g < G ? cal_apply(c, z[i], g) : cal_nan();
}

// per row: p, the NaN rows of its group, and the sort keys.  WIDTH (k64 == nullptr): k32 = the cell.  MASS: k64 = the score's key, k32 = the group.
// An invalid row takes the key past the last cell / group.
__global__ __launch_bounds__(CAL_THREADS) void cal_rows_k(CalDev c, const double* __restrict__ z, const uint32_t* __restrict__ grp, int64_t n, int64_t G, int B,
                                                         double* __restrict__ p, unsigned long long* __restrict__ nan_rows, uint32_t* __restrict__ k32,
                                                         uint64_t* __restrict__ k64, uint32_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t g = grp ? (int64_t)grp[i] : 0;
  const double zi = z[i];
  double pi = cal_nan();
  bool valid = false;
  if (g < G) {
    pi = cal_apply(c, zi, g);
    valid = pi == pi;
    if (!valid) atomicAdd(&nan_rows[g], 1ull);
  }
  p[i] = pi;
  val[i] = (uint32_t)i;
  if (k64) {
    k64[i] = cal_key(zi);
    k32[i] = (uint32_t)(valid ? g : G);
  } else {
    int bin = 0;
    if (valid) {
      const double t = floor(__dmul_rn(pi, (double)B));
      bin = !(t >= 0.0) ? 0 : (!(t < (double)B) ? B - 1 : (int)t);   // (a step map may hold values outside [0, 1])
    }
    k32[i] = (uint32_t)(valid ? g * B + bin : G * B);
  }
}

__global__ __launch_bounds__(CAL_THREADS) void cal_gather_k(const uint32_t* __restrict__ src, const uint32_t* __restrict__ row, int64_t n, uint32_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (i < n) dst[i] = src[row[i]];
}

// MASS, on the rows in (group, key, row) order: a tie-run head holds its own position, every other slot 0
__global__ __launch_bounds__(CAL_THREADS) void cal_heads_k(const double* __restrict__ z, const uint32_t* __restrict__ gs, const uint32_t* __restrict__ row, int64_t n,
                                                          uint32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (i >= n) return;
  const bool hd = i == 0 || gs[i] != gs[i - 1] || cal_key(z[row[i]]) != cal_key(z[row[i - 1]]);
  head[i] = hd ? (uint32_t)i : 0u;
}

// MASS: the cell of every sorted position, bin = floor((head - the group's first position) B / s) in exact integers
__global__ __launch_bounds__(CAL_THREADS) void cal_mass_cells_k(const uint32_t* __restrict__ gs, const uint32_t* __restrict__ rh, const int64_t* __restrict__ goff, int64_t n,
                                                               int64_t G, int B, uint32_t* __restrict__ cell) {
  const int64_t i = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t g = gs[i];
  if (g >= G) { cell[i] = (uint32_t)(G * B); return; }
  const int64_t first = goff[g], s = goff[g + 1] - first;   // s >= 1: position i is in the group
  cell[i] = (uint32_t)(g * B + ((int64_t)rh[i] - first) * B / s);
}

// chunks per run of a CSR of `cnt` runs (slot cnt: 0, so that a scan over cnt + 1 slots ends in the total)
__global__ __launch_bounds__(CAL_THREADS) void cal_plan_k(const int64_t* __restrict__ off, int64_t cnt, int64_t* __restrict__ nch) {
  const int64_t c = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (c > cnt) return;
  nch[c] = c < cnt ? (off[c + 1] - off[c] + CAL_CHUNK - 1) / CAL_CHUNK : 0;
}

// the run of an item: the last c with ioff[c] <= item (ioff[cnt] = items > item)
__device__ __forceinline__ int64_t cal_item_run(const int64_t* __restrict__ ioff, int64_t cnt, int64_t item) {
  int64_t lo = 0, hi = cnt;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ioff[mid] <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

constexpr int CAL_SUMS = 3;   // p, (p - [positive])^2, -log(q)

struct CalSumArgs {
  const double *z, *p;
  const float* y;
  const uint32_t* row;     // the sorted rows
  const int64_t *boff, *ioff;
  int64_t cells;
  int sums;                // 0: positives and lo / hi only (the isotonic fit)
  double* part;            // [items][CAL_SUMS]
  int64_t* ipart;          // [items] positives
  uint64_t* kpart;         // [items][2] min, max of cal_bits_key(z)
};

// one workgroup per (cell, chunk): the chunk's sums in the fixed order, its positives, its smallest and largest score
__global__ __launch_bounds__(CAL_THREADS) void cal_sums_k(CalSumArgs a) {
  __shared__ double ws[CAL_WAVES][CAL_SUMS];
  __shared__ int wi[CAL_WAVES];
  __shared__ uint64_t wk[CAL_WAVES][2];
  const int64_t item = blockIdx.x;
  const int64_t c = cal_item_run(a.ioff, a.cells, item);
  const int64_t base = a.boff[c] + (item - a.ioff[c]) * CAL_CHUNK;
  const int64_t left = a.boff[c + 1] - base;
  const int cnt = (int)(left < CAL_CHUNK ? left : CAL_CHUNK);
  double s[CAL_SUMS];
#pragma unroll
  for (int q = 0; q < CAL_SUMS; ++q) s[q] = 0.0;
  int np = 0;
  uint64_t kmin = ~0ull, kmax = 0ull;
  for (int j = threadIdx.x; j < cnt; j += CAL_THREADS) {
    const int64_t r = a.row[base + j];
    const bool ps = a.y[r] > 0.0f;
    const uint64_t k = cal_bits_key(a.z[r]);
    kmin = k < kmin ? k : kmin;
    kmax = k > kmax ? k : kmax;
    np += ps ? 1 : 0;
    if (a.sums) {
      const double p = a.p[r];
      const double d = __dsub_rn(p, ps ? 1.0 : 0.0);
      const double q = ps ? p : __dsub_rn(1.0, p);
      s[0] = __dadd_rn(s[0], p);
      s[1] = __dadd_rn(s[1], __dmul_rn(d, d));
      s[2] = __dadd_rn(s[2], -log(q));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int q = 0; q < CAL_SUMS; ++q) s[q] = __dadd_rn(s[q], __shfl_xor(s[q], o));
    np += __shfl_xor(np, o);
    const uint64_t omin = __shfl_xor((unsigned long long)kmin, o), omax = __shfl_xor((unsigned long long)kmax, o);
    kmin = omin < kmin ? omin : kmin;
    kmax = omax > kmax ? omax : kmax;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < CAL_SUMS; ++q) ws[wv][q] = s[q];
    wi[wv] = np;
    wk[wv][0] = kmin; wk[wv][1] = kmax;
  }
  __syncthreads();
  if (threadIdx.x < CAL_SUMS) {
    double v = ws[0][threadIdx.x];
    for (int w = 1; w < CAL_WAVES; ++w) v = __dadd_rn(v, ws[w][threadIdx.x]);
    a.part[(size_t)item * CAL_SUMS + threadIdx.x] = v;
  } else if (threadIdx.x == CAL_SUMS) {
    int v = 0;
    uint64_t mn = ~0ull, mx = 0ull;
    for (int w = 0; w < CAL_WAVES; ++w) {
      v += wi[w];
      mn = wk[w][0] < mn ? wk[w][0] : mn;
      mx = wk[w][1] > mx ? wk[w][1] : mx;
    }
    a.ipart[item] = v;
    a.kpart[(size_t)item * 2] = mn; a.kpart[(size_t)item * 2 + 1] = mx;
  }
}

// per cell: its chunks in ascending order
__global__ __launch_bounds__(CAL_THREADS) void cal_cells_k(CalSumArgs a, int64_t* __restrict__ count, double* __restrict__ sum_p, double* __restrict__ lo_z,
                                                          double* __restrict__ hi_z, double* __restrict__ cell_sums) {
  const int64_t c = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (c >= a.cells) return;
  const int64_t rows = a.boff[c + 1] - a.boff[c];
  double s[CAL_SUMS];
#pragma unroll
  for (int q = 0; q < CAL_SUMS; ++q) s[q] = 0.0;
  int64_t P = 0;
  uint64_t mn = ~0ull, mx = 0ull;
  for (int64_t it = a.ioff[c]; it < a.ioff[c + 1]; ++it) {
#pragma unroll
    for (int q = 0; q < CAL_SUMS; ++q) s[q] = __dadd_rn(s[q], a.part[(size_t)it * CAL_SUMS + q]);
    P += a.ipart[it];
    const uint64_t k0 = a.kpart[(size_t)it * 2], k1 = a.kpart[(size_t)it * 2 + 1];
    mn = k0 < mn ? k0 : mn;
    mx = k1 > mx ? k1 : mx;
  }
  count[2 * c] = rows; count[2 * c + 1] = P;
  sum_p[c] = s[0];
  lo_z[c] = rows ? cal_bits_unkey(mn) : cal_nan();
  if (hi_z) hi_z[c] = rows ? cal_bits_unkey(mx) : cal_nan();
  if (cell_sums) { cell_sums[2 * c] = s[1]; cell_sums[2 * c + 1] = s[2]; }
}

// per group, from the table: ECE, MCE, BRIER, LOGLOSS
__global__ __launch_bounds__(CAL_THREADS) void cal_groups_k(const int64_t* __restrict__ count, const double* __restrict__ sum_p, const double* __restrict__ cell_sums,
                                                           int64_t G, int B, double* __restrict__ value) {
  const int64_t g = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (g >= G) return;
  const int64_t* cnt = count + (size_t)g * B * 2;
  int64_t s = 0;
  for (int b = 0; b < B; ++b) s += cnt[2 * b];
  double* v = value + (size_t)g * FMX_CAL_VALUES;
  if (s == 0) {
#pragma unroll
    for (int q = 0; q < FMX_CAL_VALUES; ++q) v[q] = cal_nan();
    return;
  }
  const double ds = (double)s;
  double ece = 0.0, mce = 0.0, br = 0.0, ll = 0.0;
  for (int b = 0; b < B; ++b) {
    const int64_t rows = cnt[2 * b];
    if (rows == 0) continue;
    const double dr = (double)rows;
    const double gap = fabs(__dsub_rn(__ddiv_rn(sum_p[(size_t)g * B + b], dr), __ddiv_rn((double)cnt[2 * b + 1], dr)));
    ece = __dadd_rn(ece, __dmul_rn(__ddiv_rn(dr, ds), gap));
    mce = gap > mce ? gap : mce;
    br = __dadd_rn(br, cell_sums[2 * ((size_t)g * B + b)]);
    ll = __dadd_rn(ll, cell_sums[2 * ((size_t)g * B + b) + 1]);
  }
  v[FMX_CAL_ECE] = ece; v[FMX_CAL_MCE] = mce;
  v[FMX_CAL_BRIER] = __ddiv_rn(br, ds); v[FMX_CAL_LOGLOSS] = __ddiv_rn(ll, ds);
}

// one thread per group: pool adjacent violators over the non-empty bins, b ascending, on the integer pairs (positives, rows).  The block stack is
// kept in the count table itself (block t at slot t <= the bin being read) and in thr.
__global__ __launch_bounds__(CAL_THREADS) void cal_pav_k(int64_t* __restrict__ count, const double* __restrict__ lo_z, int64_t G, int B, int32_t* __restrict__ n_steps,
                                                        double* __restrict__ thr, double* __restrict__ val) {
  const int64_t g = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (g >= G) return;
  int64_t* cnt = count + (size_t)g * B * 2;
  const double* lo = lo_z + (size_t)g * B;
  double* th = thr + (size_t)g * B;
  double* vl = val + (size_t)g * B;
  int top = 0;   // blocks on the stack
  for (int b = 0; b < B; ++b) {
    int64_t rows = cnt[2 * b], pos = cnt[2 * b + 1];
    if (rows == 0) continue;
    double t0 = lo[b];
    while (top > 0) {
      const int64_t prow = cnt[2 * (top - 1)], ppos = cnt[2 * (top - 1) + 1];
      if (ppos * rows < pos * prow) break;   // the block before is strictly lower: both stay
      rows += prow; pos += ppos;
      t0 = th[top - 1];
      --top;
    }
    cnt[2 * top] = rows; cnt[2 * top + 1] = pos;
    th[top] = t0;
    ++top;
  }
  for (int t = 0; t < B; ++t) {
    if (t < top) {
      vl[t] = __ddiv_rn((double)cnt[2 * t + 1], (double)cnt[2 * t]);
      if (t == 0) th[0] = -__builtin_inf();
    } else {
      vl[t] = cal_nan(); th[t] = cal_nan();
    }
  }
  n_steps[g] = top;
}

// ---------------------------------------------------------------------------------------------------------------- Platt scaling

constexpr int PL_SUMS = 5;   // sum (sigma - t) z, sum (sigma - t), sum w z^2, sum w z, sum w

__global__ __launch_bounds__(CAL_THREADS) void platt_keys_k(const double* __restrict__ z, const uint32_t* __restrict__ grp, int64_t n, int64_t G, uint32_t* __restrict__ key,
                                                           uint32_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t g = grp ? (int64_t)grp[i] : 0;
  key[i] = (uint32_t)((g < G && isfinite(z[i])) ? g : G);
  val[i] = (uint32_t)i;
}

__global__ __launch_bounds__(CAL_THREADS) void platt_init_k(int64_t G, const int64_t* __restrict__ off, double* __restrict__ ab, int32_t* __restrict__ status,
                                                           int64_t* __restrict__ rows) {
  const int64_t g = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (g >= G) return;
  ab[2 * g] = 1.0; ab[2 * g + 1] = 0.0;
  status[g] = 0;
  if (rows) rows[g] = off[g + 1] - off[g];
}

// one workgroup per (group, chunk): the five sums of the chunk at the group's current (a, b), in the fixed order
__global__ __launch_bounds__(CAL_THREADS) void platt_sums_k(const double* __restrict__ z, const float* __restrict__ y, const uint32_t* __restrict__ row,
                                                           const int64_t* __restrict__ off, const int64_t* __restrict__ ioff, int64_t G, const double* __restrict__ ab,
                                                           double* __restrict__ part) {
  __shared__ double ws[CAL_WAVES][PL_SUMS];
  const int64_t item = blockIdx.x;
  const int64_t g = cal_item_run(ioff, G, item);
  const int64_t base = off[g] + (item - ioff[g]) * CAL_CHUNK;
  const int64_t left = off[g + 1] - base;
  const int cnt = (int)(left < CAL_CHUNK ? left : CAL_CHUNK);
  const double a = ab[2 * g], b = ab[2 * g + 1];
  double s[PL_SUMS];
#pragma unroll
  for (int q = 0; q < PL_SUMS; ++q) s[q] = 0.0;
  for (int j = threadIdx.x; j < cnt; j += CAL_THREADS) {
    const int64_t r = row[base + j];
    const double zr = z[r];
    const double yr = y[r] > 0.0f ? 1.0 : -1.0;
    const double m = __dmul_rn(yr, __dadd_rn(__dmul_rn(a, zr), b));
    const double sg = 1.0 / (1.0 + exp(-m));   // sigma of the margin, as fold-in's logistic loop forms it
    const double ng = 1.0 / (1.0 + exp(m));    // 1 - sigma, without the cancellation
    const double w = __dmul_rn(sg, ng);
    const double d = __dmul_rn(-yr, ng);       // sigma(a z + b) - [positive]
    const double wz = __dmul_rn(w, zr);
    s[0] = __dadd_rn(s[0], __dmul_rn(d, zr));
    s[1] = __dadd_rn(s[1], d);
    s[2] = __dadd_rn(s[2], __dmul_rn(wz, zr));
    s[3] = __dadd_rn(s[3], wz);
    s[4] = __dadd_rn(s[4], w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int q = 0; q < PL_SUMS; ++q) s[q] = __dadd_rn(s[q], __shfl_xor(s[q], o));
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < PL_SUMS; ++q) ws[wv][q] = s[q];
  }
  __syncthreads();
  if (threadIdx.x < PL_SUMS) {
    double v = ws[0][threadIdx.x];
    for (int w = 1; w < CAL_WAVES; ++w) v = __dadd_rn(v, ws[w][threadIdx.x]);
    part[(size_t)item * PL_SUMS + threadIdx.x] = v;
  }
}

// one thread per group: the chunks ascending, the ridge, the 2 x 2 Cholesky solve, the step
__global__ __launch_bounds__(CAL_THREADS) void platt_solve_k(const int64_t* __restrict__ ioff, const double* __restrict__ part, int64_t G, double lambda,
                                                            double* __restrict__ ab, int32_t* __restrict__ status) {
  const int64_t g = (int64_t)blockIdx.x * CAL_THREADS + threadIdx.x;
  if (g >= G) return;
  double s[PL_SUMS];
#pragma unroll
  for (int q = 0; q < PL_SUMS; ++q) s[q] = 0.0;
  for (int64_t it = ioff[g]; it < ioff[g + 1]; ++it) {
#pragma unroll
    for (int q = 0; q < PL_SUMS; ++q) s[q] = __dadd_rn(s[q], part[(size_t)it * PL_SUMS + q]);
  }
  const double a = ab[2 * g], b = ab[2 * g + 1];
  const double g0 = __dadd_rn(s[0], __dmul_rn(lambda, __dsub_rn(a, 1.0))), g1 = __dadd_rn(s[1], __dmul_rn(lambda, b));
  const double h00 = __dadd_rn(s[2], lambda), h01 = s[3], h11 = __dadd_rn(s[4], lambda);
  bool bad = !(h00 > 0.0) || !isfinite(h00);
  double l00 = 0.0, l10 = 0.0, d1 = 0.0;
  if (!bad) {
    l00 = __dsqrt_rn(h00);
    l10 = __ddiv_rn(h01, l00);
    d1 = __dsub_rn(h11, __dmul_rn(l10, l10));
    bad = !(d1 > 0.0) || !isfinite(d1);
  }
  if (bad) {
    ab[2 * g] = cal_nan(); ab[2 * g + 1] = cal_nan();
    status[g] = 1;
    return;
  }
  const double l11 = __dsqrt_rn(d1);
  // L y = -g, then L' x = y
  const double y0 = __ddiv_rn(-g0, l00);
  const double y1 = __ddiv_rn(__dsub_rn(-g1, __dmul_rn(l10, y0)), l11);
  const double x1 = __ddiv_rn(y1, l11);
  const double x0 = __ddiv_rn(__dsub_rn(y0, __dmul_rn(l10, x1)), l00);
  ab[2 * g] = __dadd_rn(a, x0); ab[2 * g + 1] = __dadd_rn(b, x1);
}

// ---------------------------------------------------------------------------------------------------------------- host side

int64_t cal_chunk_rows() {
  const int64_t c = g_cal_chunk_rows.load();
  return c > 0 ? c : CAL_FWD_ROWS;
}

// the raw scores, in forward calls of chunk rows (a short tail joins the call before it)
int cal_forward(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t n, double* z) {
  const int64_t chunk = cal_chunk_rows();
  for (int64_t a = 0; a < n;) {
    int64_t b = std::min(n, a + chunk);
    if (n - b < chunk / 16) b = n;
    FMX_TRY(forward_rows(e, m, r0 + a, r0 + b, z + a, FMX_LINK_NONE));
    a = b;
  }
  return FMX_OK;
}

template <typename T>
int cal_up(Scratch& S, const T* host, size_t count, const T** dev) {
  T* d = nullptr;
  FMX_TRY(S.get(&d, count));
  FMX_HIP(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
  *dev = d;
  return FMX_OK;
}

// the calibrator's tables to the device (cal == nullptr: FMX_CAL_NONE under `link`); checked by the entry points
int cal_upload(fmx_engine* e, Scratch& S, const fmx_calibrator* cal, int link, CalDev* c) {
  *c = CalDev{};
  c->h = e->hyper;
  c->kind = cal ? cal->kind : FMX_CAL_NONE;
  c->link = cal ? cal->link : link;
  c->G = cal ? cal->n_groups : 1;
  c->max_steps = cal ? cal->max_steps : 0;
  if (c->kind == FMX_CAL_NONE) {
    c->G = 1;
    if (c->link == FMX_LINK_PROBIT) FMX_TRY(ensure_probit(e));
    c->pn_y = e->probit;
  } else if (c->kind == FMX_CAL_PLATT) {
    FMX_TRY(cal_up(S, cal->platt, (size_t)c->G * 2, &c->platt));
  } else {
    const size_t cells = (size_t)c->G * (size_t)c->max_steps;
    FMX_TRY(cal_up(S, cal->n_steps, (size_t)c->G, &c->n_steps));
    FMX_TRY(cal_up(S, cal->thr, cells, &c->thr));
    FMX_TRY(cal_up(S, cal->val, cells, &c->val));
  }
  return FMX_OK;
}

// the chunk plan of a CSR of cnt runs: ioff [cnt + 1] and the number of items
int cal_plan(Scratch& S, const int64_t* off, int64_t cnt, int64_t** ioff, int64_t* items, const char* what) {
  hipStream_t st = S.st;
  int64_t* nch = nullptr;
  FMX_TRY(S.get(&nch, (size_t)cnt + 1)); FMX_TRY(S.get(ioff, (size_t)cnt + 1));
  hipLaunchKernelGGL(cal_plan_k, dim3(blocks(cnt + 1, CAL_THREADS)), dim3(CAL_THREADS), 0, st, off, cnt, nch);
  FMX_HIP(hipGetLastError());
  FMX_TRY(exclusive_sum(S, (const int64_t*)nch, *ioff, cnt + 1));
  FMX_HIP(hipMemcpyAsync(items, *ioff + cnt, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  FMX_CHECK(*items >= 0 && *items < (1LL << 31), FMX_ERR_HIP, "%s: the chunk plan is inconsistent (%lld chunks)", what, (long long)*items);
  return FMX_OK;
}

// the table of rows [r0, r0 + n): count [G][B][2], sum_p / lo_z / hi_z [G][B], nan_rows [G], value [G][4] (each may be null; without value
// the floating-point sums are not formed)
int cal_table(fmx_engine* e, Scratch& S, const fmx_matrix* m, int64_t r0, int64_t n, const uint32_t* d_group, int64_t G, int B, int binning, const CalDev& c,
              int64_t* count, double* sum_p, double* lo_z, double* hi_z, int64_t* nan_rows, double* value) {
  hipStream_t st = S.st;
  const int64_t cells = G * B;
  double *z = nullptr, *p = nullptr;
  FMX_TRY(S.get(&z, (size_t)n)); FMX_TRY(S.get(&p, (size_t)n));
  FMX_TRY(cal_forward(e, m, r0, n, z));
  if (!count) FMX_TRY(S.get(&count, (size_t)cells * 2));
  if (!sum_p) FMX_TRY(S.get(&sum_p, (size_t)cells));
  if (!lo_z) FMX_TRY(S.get(&lo_z, (size_t)cells));
  if (!nan_rows) FMX_TRY(S.get(&nan_rows, (size_t)G));
  FMX_HIP(hipMemsetAsync(nan_rows, 0, (size_t)G * sizeof(int64_t), st));

  const bool mass = binning == FMX_BINS_MASS;
  uint32_t *k_in = nullptr, *k_out = nullptr, *v_in = nullptr, *v_out = nullptr;
  FMX_TRY(S.get(&k_in, (size_t)n)); FMX_TRY(S.get(&k_out, (size_t)n));
  FMX_TRY(S.get(&v_in, (size_t)n)); FMX_TRY(S.get(&v_out, (size_t)n));
  uint64_t *lk = nullptr, *sk = nullptr;
  if (mass) { FMX_TRY(S.get(&lk, (size_t)n)); FMX_TRY(S.get(&sk, (size_t)n)); }
  hipLaunchKernelGGL(cal_rows_k, dim3(blocks(n, CAL_THREADS)), dim3(CAL_THREADS), 0, st, c, (const double*)z, d_group, n, G, B, p, (unsigned long long*)nan_rows, k_in,
                     lk, v_in);
  FMX_HIP(hipGetLastError());
  const uint32_t *cell = nullptr, *row = nullptr;   // per sorted position
  if (!mass) {
    FMX_TRY(sort_pairs(S, k_in, k_out, v_in, v_out, n, key_bits((uint64_t)cells)));
    cell = k_out; row = v_out;
  } else {
    FMX_TRY(sort_pairs(S, lk, sk, v_in, v_out, n, 64));   // (key, row) order
    uint32_t* gk = (uint32_t*)lk;                         // lk is free again: 2 n u32
    hipLaunchKernelGGL(cal_gather_k, dim3(blocks(n, CAL_THREADS)), dim3(CAL_THREADS), 0, st, (const uint32_t*)k_in, (const uint32_t*)v_out, n, gk);
    FMX_HIP(hipGetLastError());
    FMX_TRY(sort_pairs(S, gk, k_out, v_out, v_in, n, key_bits((uint64_t)G)));   // (group, key, row) order: groups k_out, rows v_in
    int64_t* goff = nullptr;
    FMX_TRY(S.get(&goff, (size_t)G + 1));
    FMX_TRY(group_offsets(k_out, n, G, goff, st));
    uint32_t *head = gk, *rh = gk + n;
    hipLaunchKernelGGL(cal_heads_k, dim3(blocks(n, CAL_THREADS)), dim3(CAL_THREADS), 0, st, (const double*)z, (const uint32_t*)k_out, (const uint32_t*)v_in, n, head);
    FMX_HIP(hipGetLastError());
    FMX_TRY(inclusive_max(S, (const uint32_t*)head, rh, n));
    hipLaunchKernelGGL(cal_mass_cells_k, dim3(blocks(n, CAL_THREADS)), dim3(CAL_THREADS), 0, st, (const uint32_t*)k_out, (const uint32_t*)rh, (const int64_t*)goff, n, G, B,
                       k_in);
    FMX_HIP(hipGetLastError());
    cell = k_in; row = v_in;
  }
  int64_t *boff = nullptr, *ioff = nullptr;
  FMX_TRY(S.get(&boff, (size_t)cells + 1));
  FMX_TRY(group_offsets(cell, n, cells, boff, st));
  int64_t items = 0;
  FMX_TRY(cal_plan(S, boff, cells, &ioff, &items, "calibration"));

  CalSumArgs a{};
  a.z = z; a.p = p; a.y = m->y + r0; a.row = row;
  a.boff = boff; a.ioff = ioff; a.cells = cells;
  a.sums = value ? 1 : 0;
  FMX_TRY(S.get(&a.part, (size_t)items * CAL_SUMS)); FMX_TRY(S.get(&a.ipart, (size_t)items)); FMX_TRY(S.get(&a.kpart, (size_t)items * 2));
  if (items > 0) {
    hipLaunchKernelGGL(cal_sums_k, dim3((unsigned)items), dim3(CAL_THREADS), 0, st, a);
    FMX_HIP(hipGetLastError());
  }
  double* cell_sums = nullptr;
  if (value) FMX_TRY(S.get(&cell_sums, (size_t)cells * 2));
  hipLaunchKernelGGL(cal_cells_k, dim3(blocks(cells, CAL_THREADS)), dim3(CAL_THREADS), 0, st, a, count, sum_p, lo_z, hi_z, cell_sums);
  FMX_HIP(hipGetLastError());
  if (value) {
    hipLaunchKernelGGL(cal_groups_k, dim3(blocks(G, CAL_THREADS)), dim3(CAL_THREADS), 0, st, (const int64_t*)count, (const double*)sum_p, (const double*)cell_sums, G, B,
                       value);
    FMX_HIP(hipGetLastError());
  }
  return FMX_OK;
}

}  // namespace

void debug_calibrate_limits(int64_t chunk_rows) { g_cal_chunk_rows.store(chunk_rows > 0 ? chunk_rows : 0); }

int predict_calibrated_run(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const uint32_t* d_group, int64_t G, const fmx_calibrator* cal, int link,
                           double* d_out) {
  const int64_t n = r1 - r0;
  if (n <= 0) return FMX_OK;
  hipStream_t st = e->stream;
  Scratch S(st);
  CalDev c;
  FMX_TRY(cal_upload(e, S, cal, link, &c));
  double* z = nullptr;
  FMX_TRY(S.get(&z, (size_t)n));
  FMX_TRY(cal_forward(e, m, r0, n, z));
  if (c.G == 1) { d_group = nullptr; G = 1; }   // one map for every row: the ids are not read
  hipLaunchKernelGGL(cal_predict_k, dim3(blocks(n, CAL_THREADS)), dim3(CAL_THREADS), 0, st, c, (const double*)z, d_group, n, G, d_out);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

int reliability_run(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const uint32_t* d_group, int64_t G, int B, int binning, const fmx_calibrator* cal,
                    int link, int64_t* d_count, double* d_sum_p, double* d_lo_z, double* d_hi_z, int64_t* d_nan_rows, double* d_value) {
  const int64_t n = r1 - r0;
  if (n <= 0) return FMX_OK;
  Scratch S(e->stream);
  CalDev c;
  FMX_TRY(cal_upload(e, S, cal, link, &c));
  double* value = d_value;
  if (!value) FMX_TRY(S.get(&value, (size_t)G * FMX_CAL_VALUES));   // (sum_p needs the sums pass)
  return cal_table(e, S, m, r0, n, d_group, G, B, binning, c, d_count, d_sum_p, d_lo_z, d_hi_z, d_nan_rows, value);
}

int isotonic_run(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const uint32_t* d_group, int64_t G, int B, int32_t* d_n_steps, double* d_thr,
                 double* d_val) {
  const int64_t n = r1 - r0;
  if (n <= 0) return FMX_OK;
  hipStream_t st = e->stream;
  Scratch S(st);
  CalDev c;
  FMX_TRY(cal_upload(e, S, nullptr, FMX_LINK_LOGISTIC, &c));   // (the bins are cut by z: the map only says which rows are NaN rows)
  int64_t* count = nullptr;
  double* lo = nullptr;
  FMX_TRY(S.get(&count, (size_t)G * B * 2)); FMX_TRY(S.get(&lo, (size_t)G * B));
  if (!d_n_steps) FMX_TRY(S.get(&d_n_steps, (size_t)G));
  if (!d_thr) FMX_TRY(S.get(&d_thr, (size_t)G * B));
  if (!d_val) FMX_TRY(S.get(&d_val, (size_t)G * B));
  FMX_TRY(cal_table(e, S, m, r0, n, d_group, G, B, FMX_BINS_MASS, c, count, nullptr, lo, nullptr, nullptr, nullptr));
  hipLaunchKernelGGL(cal_pav_k, dim3(blocks(G, CAL_THREADS)), dim3(CAL_THREADS), 0, st, count, (const double*)lo, G, B, d_n_steps, d_thr, d_val);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

int platt_run(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const uint32_t* d_group, int64_t G, double lambda, int n_newton, double* d_ab,
              int64_t* d_rows, int32_t* d_status) {
  const int64_t n = r1 - r0;
  if (n <= 0) return FMX_OK;
  hipStream_t st = e->stream;
  Scratch S(st);
  double* z = nullptr;
  FMX_TRY(S.get(&z, (size_t)n));
  FMX_TRY(cal_forward(e, m, r0, n, z));
  uint32_t *k_in = nullptr, *k_out = nullptr, *v_in = nullptr, *row = nullptr;
  FMX_TRY(S.get(&k_in, (size_t)n)); FMX_TRY(S.get(&k_out, (size_t)n));
  FMX_TRY(S.get(&v_in, (size_t)n)); FMX_TRY(S.get(&row, (size_t)n));
  hipLaunchKernelGGL(platt_keys_k, dim3(blocks(n, CAL_THREADS)), dim3(CAL_THREADS), 0, st, (const double*)z, d_group, n, G, k_in, v_in);
  FMX_HIP(hipGetLastError());
  FMX_TRY(sort_pairs(S, k_in, k_out, v_in, row, n, key_bits((uint64_t)G)));
  int64_t *off = nullptr, *ioff = nullptr;
  FMX_TRY(S.get(&off, (size_t)G + 1));
  FMX_TRY(group_offsets(k_out, n, G, off, st));
  int64_t items = 0;
  FMX_TRY(cal_plan(S, off, G, &ioff, &items, "Platt scaling"));
  if (!d_ab) FMX_TRY(S.get(&d_ab, (size_t)G * 2));
  if (!d_status) FMX_TRY(S.get(&d_status, (size_t)G));
  double* part = nullptr;
  FMX_TRY(S.get(&part, (size_t)items * PL_SUMS));
  hipLaunchKernelGGL(platt_init_k, dim3(blocks(G, CAL_THREADS)), dim3(CAL_THREADS), 0, st, G, (const int64_t*)off, d_ab, d_status, d_rows);
  FMX_HIP(hipGetLastError());
  for (int it = 0; it < n_newton; ++it) {
    if (items > 0) {
      hipLaunchKernelGGL(platt_sums_k, dim3((unsigned)items), dim3(CAL_THREADS), 0, st, (const double*)z, (const float*)(m->y + r0), (const uint32_t*)row,
                         (const int64_t*)off, (const int64_t*)ioff, G, (const double*)d_ab, part);
      FMX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(platt_solve_k, dim3(blocks(G, CAL_THREADS)), dim3(CAL_THREADS), 0, st, (const int64_t*)ioff, (const double*)part, G, lambda, d_ab, d_status);
    FMX_HIP(hipGetLastError());
  }
  return FMX_OK;
}

}  // namespace fmx
