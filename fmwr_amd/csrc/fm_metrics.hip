// Exact pointwise metrics per row group (fmx_metrics*): AUC, log loss, accuracy, Brier score for CLASSIFICATION engines,
// MSE, RMSE, MAE, mean error for REGRESSION engines, and the mean prediction and label for both.
//
// For the rows [r0, r1) of a labelled matrix: z_r is the raw forward (forward_rows, FMX_LINK_NONE), p_r = rank_link(z_r), and per group g
//     count[g] = {rows, positives, pairs2, correct},   pairs2 = sum over (positive i, negative j) of 2 [z_i > z_j] + [z_i == z_j]
// (twice the Mann-Whitney U with ties as 1/2: an integer), compared under mt_key -- rank_order_key's order read upwards: -0 == +0, NaN below
// every number and equal to NaN.  The integers are exact, whichever way they are counted; the floating-point sums are formed by ONE kernel in
// ONE order for every group size, so the form that counts a group's pairs cannot move a bit of its values.
//
//   grouping   a stable radix sort of the row ids by group id (an id >= n_groups sorts into a bucket nobody reads): a CSR of groups, the rows
//              ascending inside each.  Without group ids the one group is the range itself and nothing is sorted.
//   sums       a group's row list is cut into chunks of MT_CHUNK rows.  A workgroup sums one chunk: thread t adds the terms of rows t, t + 256,
//              t + 512, t + 768 in that order from +0.0, the 64 lanes of a wave are added by an xor butterfly (commutative steps: every lane
//              holds the same bits), the four waves' sums are added in wave order.  The finishing kernel adds a group's chunk sums in
//              ascending order and divides once.  Every term is made of individually rounded fp64 operations (__dsub_rn / __dmul_rn /
//              __dadd_rn); nothing is added by floating-point atomics.  The order is a function of the group's ascending row list alone.
//   pairs2     wave form       groups of at most 64 rows: one wave per group, four groups per workgroup, no workgroup barrier.  A lane holds
//                              one row's key and label and counts against the group's rows by lane broadcasts; the wave's total by __shfl_xor.
//              workgroup form  65 .. 1 024 rows: keys and labels in LDS, every thread counts its positives against the tile by broadcast
//                              reads (all lanes read one address).
//              global form     longer groups: their rows sorted by (group, key) -- a 64-bit radix sort by key, then a stable one by group --,
//                              an exclusive scan of the negative flags, a max-scan of the tie-run heads, and per row
//                                  positive: 2 (negatives before its run, inside the group) + (negatives before it inside its run)
//                                  negative: positives before it inside its run
//                              which counts every tied pair once.  The per-row integers are added per group by 64-bit integer atomics.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

#include "fm_prims.h"

namespace fmx {
namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_WAVE_ROWS = 64;            // most rows of a wave-form group: one per lane
constexpr int MT_LDS_ROWS = 1024;           // most rows of a workgroup-form group: 8 KiB of keys + 1 KiB of labels
constexpr int MT_CHUNK = 4 * MT_THREADS;    // rows per chunk of the sums
constexpr int MT_SUMS = 5;                  // floating-point sums per group
constexpr int64_t MT_FWD_ROWS = 1LL << 24;  // rows per forward call

std::atomic<int> g_wave_rows{0}, g_lds_rows{0};
std::atomic<int64_t> g_chunk_rows{0};

// ascending in this key = ascending in z; NaN is 0, below every number; -0 and +0 share a key
__device__ __forceinline__ uint64_t mt_key(double z) { return ~rank_order_key(z); }

struct MtArgs {
  const double* z;       // [n] raw scores, indexed from the range's first row
  const float* y;        // [n] labels, likewise
  const uint32_t* rows;  // [n] the rows grouped (ascending inside a group), or null: the identity
  const int64_t* off;    // [G + 1] group g's rows are positions [off[g], off[g + 1])
  int64_t G;
  int cls;               // CLASSIFICATION
  int link;
  Hyper h;
  const double* pn_y;
  int wave_rows, lds_rows;   // the forms' limits (<= 0: the form is off)
};

// 0 wave, 1 workgroup, 2 global
__device__ __forceinline__ int mt_form(const MtArgs& a, int64_t len) {
  if (a.wave_rows > 0 && len <= a.wave_rows) return 0;
  if (a.lds_rows > 0 && len <= a.lds_rows) return 1;
  return 2;
}

__device__ __forceinline__ int64_t mt_row(const MtArgs& a, int64_t pos) { return a.rows ? (int64_t)a.rows[pos] : pos; }

__global__ __launch_bounds__(MT_THREADS) void mt_group_keys_k(const uint32_t* __restrict__ grp, int64_t n, int64_t G, uint32_t* __restrict__ key,
                                                             uint32_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (i >= n) return;
  const uint32_t g = grp[i];
  key[i] = (int64_t)g < G ? g : (uint32_t)G;   // G <= 2^31 - 1
  val[i] = (uint32_t)i;
}

// per group its chunk count and, for a global-form group, its row count (slot G of both: 0, so that a scan over G + 1 slots ends in the total)
__global__ __launch_bounds__(MT_THREADS) void mt_plan_k(MtArgs a, int64_t* __restrict__ nch, int64_t* __restrict__ llen) {
  const int64_t g = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (g > a.G) return;
  int64_t len = 0;
  if (g < a.G) len = a.off[g + 1] - a.off[g];
  nch[g] = (len + MT_CHUNK - 1) / MT_CHUNK;
  llen[g] = (a.cls && len > 0 && mt_form(a, len) == 2) ? len : 0;
}

// the terms of one row
__device__ __forceinline__ void mt_terms(const MtArgs& a, double z, float yf, double t[MT_SUMS], int* pos, int* correct) {
  const double p = z != z ? z : rank_link(a.h, z, a.link, a.pn_y);   // (a NaN score stays out of the probit table's index arithmetic)
  if (a.cls) {
    const bool ps = yf > 0.0f;
    double l;
    if (a.link == FMX_LINK_LOGISTIC) {
      const double tt = ps ? z : -z;
      l = __dadd_rn(fmax(-tt, 0.0), log1p(exp(-fabs(tt))));
    } else {
      const double q = ps ? p : __dsub_rn(1.0, p);
      l = -log(q);
    }
    const double d = __dsub_rn(p, ps ? 1.0 : 0.0);
    t[0] = l; t[1] = __dmul_rn(d, d); t[2] = p; t[3] = 0.0; t[4] = 0.0;
    *pos = ps ? 1 : 0;
    *correct = (p == p && (p >= 0.5) == ps) ? 1 : 0;   // a NaN p is never correct
  } else {
    const double y = (double)yf;
    const double d = __dsub_rn(p, y);
    t[0] = __dmul_rn(d, d); t[1] = fabs(d); t[2] = d; t[3] = p; t[4] = y;
    *pos = 0; *correct = 0;
  }
}

// one workgroup per (group, chunk): the chunk's sums in the fixed order into part[item][MT_SUMS], its positives and correct rows into ipart[item][2]
__global__ __launch_bounds__(MT_THREADS) void mt_sums_k(MtArgs a, const int64_t* __restrict__ ioff, double* __restrict__ part, int64_t* __restrict__ ipart) {
  __shared__ double ws[MT_WAVES][MT_SUMS];
  __shared__ int wi[MT_WAVES][2];
  const int64_t item = blockIdx.x;
  int64_t lo = 0, hi = a.G;   // the group of the item: the last g with ioff[g] <= item (ioff[G] = items > item)
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (ioff[mid] <= item) lo = mid; else hi = mid - 1;
  }
  const int64_t g = lo;
  const int64_t base = a.off[g] + (item - ioff[g]) * MT_CHUNK;
  const int64_t left = a.off[g + 1] - base;
  const int cnt = (int)(left < MT_CHUNK ? left : MT_CHUNK);
  double s[MT_SUMS];
#pragma unroll
  for (int q = 0; q < MT_SUMS; ++q) s[q] = 0.0;
  int np = 0, nc = 0;
  for (int j = threadIdx.x; j < cnt; j += MT_THREADS) {
    const int64_t r = mt_row(a, base + j);
    double t[MT_SUMS];
    int ps, co;
    mt_terms(a, a.z[r], a.y[r], t, &ps, &co);
#pragma unroll
    for (int q = 0; q < MT_SUMS; ++q) s[q] = __dadd_rn(s[q], t[q]);
    np += ps; nc += co;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int q = 0; q < MT_SUMS; ++q) s[q] = __dadd_rn(s[q], __shfl_xor(s[q], o));
    np += __shfl_xor(np, o); nc += __shfl_xor(nc, o);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < MT_SUMS; ++q) ws[wv][q] = s[q];
    wi[wv][0] = np; wi[wv][1] = nc;
  }
  __syncthreads();
  if (threadIdx.x < MT_SUMS) {
    double v = ws[0][threadIdx.x];
    for (int w = 1; w < MT_WAVES; ++w) v = __dadd_rn(v, ws[w][threadIdx.x]);
    part[(size_t)item * MT_SUMS + threadIdx.x] = v;
  } else if (threadIdx.x < MT_SUMS + 2) {
    const int q = threadIdx.x - MT_SUMS;
    int v = 0;
    for (int w = 0; w < MT_WAVES; ++w) v += wi[w][q];
    ipart[(size_t)item * 2 + q] = v;
  }
}

// 2 [ki > kj] + [ki == kj]
__device__ __forceinline__ int mt_cmp2(uint64_t ki, uint64_t kj) { return ki > kj ? 2 : (ki == kj ? 1 : 0); }

// wave form: one wave per group, four groups per workgroup; the kernel has no workgroup barrier
__global__ __launch_bounds__(MT_THREADS) void mt_pairs_wave_k(MtArgs a, unsigned long long* __restrict__ pairs2) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * MT_WAVES + (threadIdx.x >> 6);
  if (g >= a.G) return;   // (uniform over the wave)
  const int64_t b = a.off[g];
  const int64_t len = a.off[g + 1] - b;
  if (mt_form(a, len) != 0) return;
  uint64_t key = 0;
  int flag = 2;            // 1 positive, 0 negative, 2 no row
  if (lane < len) {        // len <= wave_rows <= 64
    const int64_t r = mt_row(a, b + lane);
    key = mt_key(a.z[r]);
    flag = a.y[r] > 0.0f ? 1 : 0;
  }
  int c = 0;
  for (int j = 0; j < (int)len; ++j) {
    const uint64_t kj = __shfl((unsigned long long)key, j);
    const int fj = __shfl(flag, j);
    c += (flag == 1 && fj == 0) ? mt_cmp2(key, kj) : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) pairs2[g] = (unsigned long long)c;
}

// workgroup form: the group's keys and labels in LDS, every thread counts its positives against all of them
__global__ __launch_bounds__(MT_THREADS) void mt_pairs_wg_k(MtArgs a, unsigned long long* __restrict__ pairs2) {
  __shared__ uint64_t keys[MT_LDS_ROWS];
  __shared__ unsigned char flags[MT_LDS_ROWS];
  __shared__ long long wsum[MT_WAVES];
  const int64_t g = blockIdx.x;
  const int64_t b = a.off[g];
  const int64_t len64 = a.off[g + 1] - b;
  if (mt_form(a, len64) != 1) return;   // (uniform over the workgroup)
  const int len = (int)len64;           // <= lds_rows <= MT_LDS_ROWS
  for (int j = threadIdx.x; j < len; j += MT_THREADS) {
    const int64_t r = mt_row(a, b + j);
    keys[j] = mt_key(a.z[r]);
    flags[j] = a.y[r] > 0.0f ? 1 : 0;
  }
  __syncthreads();
  long long c = 0;
  for (int i = threadIdx.x; i < len; i += MT_THREADS) {
    if (!flags[i]) continue;
    const uint64_t ki = keys[i];
    int ci = 0;
    for (int j = 0; j < len; ++j) ci += flags[j] ? 0 : mt_cmp2(ki, keys[j]);
    c += ci;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t = 0;
    for (int w = 0; w < MT_WAVES; ++w) t += wsum[w];
    pairs2[g] = (unsigned long long)t;
  }
}

// global form, step 1: the rows of the global-form groups, group by group, with their keys
__global__ __launch_bounds__(MT_THREADS) void mt_long_fill_k(MtArgs a, int64_t n, const uint32_t* __restrict__ gsorted, const int64_t* __restrict__ loff,
                                                            uint64_t* __restrict__ lkey, uint32_t* __restrict__ lval) {
  const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t g = gsorted ? (int64_t)gsorted[i] : 0;
  if (g >= a.G) return;   // an id out of range: the row belongs to no group
  const int64_t len = a.off[g + 1] - a.off[g];
  if (mt_form(a, len) != 2) return;
  const int64_t dst = loff[g] + (i - a.off[g]);
  const int64_t r = mt_row(a, i);
  lkey[dst] = mt_key(a.z[r]);
  lval[dst] = (uint32_t)r;
}

__global__ __launch_bounds__(MT_THREADS) void mt_long_groups_k(const uint32_t* __restrict__ grp, const uint32_t* __restrict__ row, int64_t nl, uint32_t* __restrict__ gkey) {
  const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (i < nl) gkey[i] = grp[row[i]];
}

// step 2, on the rows in (group, key) order: the negative flags and the tie-run heads (a head holds its own position, every other slot 0)
__global__ __launch_bounds__(MT_THREADS) void mt_long_flags_k(MtArgs a, const uint32_t* __restrict__ grp, const uint32_t* __restrict__ row, int64_t nl,
                                                             uint32_t* __restrict__ negf, uint32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (i >= nl) return;
  const uint32_t r = row[i];
  bool hd = i == 0;
  if (!hd) {
    const uint32_t rp = row[i - 1];
    hd = (grp && grp[r] != grp[rp]) || mt_key(a.z[r]) != mt_key(a.z[rp]);
  }
  negf[i] = a.y[r] > 0.0f ? 0u : 1u;
  head[i] = hd ? (uint32_t)i : 0u;
}

// step 3: every row's integer, added per group (a workgroup whose rows share a group adds once)
__global__ __launch_bounds__(MT_THREADS) void mt_long_acc_k(const uint32_t* __restrict__ grp, const uint32_t* __restrict__ row, int64_t nl,
                                                           const uint32_t* __restrict__ negf, const uint32_t* __restrict__ ns, const uint32_t* __restrict__ rh,
                                                           const int64_t* __restrict__ loff, unsigned long long* __restrict__ pairs2) {
  __shared__ unsigned long long wsum[MT_WAVES];
  const int64_t b0 = (int64_t)blockIdx.x * MT_THREADS;
  const int64_t i = b0 + threadIdx.x;
  const int64_t last = b0 + MT_THREADS - 1 < nl ? b0 + MT_THREADS - 1 : nl - 1;
  const uint32_t gfirst = grp ? grp[row[b0]] : 0u, glast = grp ? grp[row[last]] : 0u;   // (b0 < nl: the grid covers nl)
  unsigned long long c = 0;
  uint32_t g = gfirst;
  if (i < nl) {
    if (grp) g = grp[row[i]];
    const uint32_t h = rh[i];
    const uint32_t nh = ns[h], ni = ns[i];
    if (negf[i]) c = (unsigned long long)(((uint32_t)i - ni) - (h - nh));
    else c = 2ull * (unsigned long long)(nh - ns[loff[g]]) + (unsigned long long)(ni - nh);
  }
  if (gfirst == glast) {   // the rows are in group order: every row of the workgroup is in that group (uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = 0;
      for (int w = 0; w < MT_WAVES; ++w) t += wsum[w];
      if (t) atomicAdd(&pairs2[gfirst], t);
    }
  } else if (c) {
    atomicAdd(&pairs2[g], c);
  }
}

__device__ __forceinline__ double mt_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// per group: the chunk sums in ascending order, one division each, the counts
__global__ __launch_bounds__(MT_THREADS) void mt_finish_k(MtArgs a, const int64_t* __restrict__ ioff, const double* __restrict__ part, const int64_t* __restrict__ ipart,
                                                         const unsigned long long* __restrict__ pairs2, double* __restrict__ value, int64_t* __restrict__ count) {
  const int64_t g = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
  if (g >= a.G) return;
  const int64_t rows = a.off[g + 1] - a.off[g];
  double s[MT_SUMS];
#pragma unroll
  for (int q = 0; q < MT_SUMS; ++q) s[q] = 0.0;
  int64_t P = 0, C = 0;
  for (int64_t it = ioff[g]; it < ioff[g + 1]; ++it) {
#pragma unroll
    for (int q = 0; q < MT_SUMS; ++q) s[q] = __dadd_rn(s[q], part[(size_t)it * MT_SUMS + q]);
    P += ipart[(size_t)it * 2]; C += ipart[(size_t)it * 2 + 1];
  }
  const unsigned long long p2 = a.cls ? pairs2[g] : 0ull;
  double* v = value + (size_t)g * FMX_MET_VALUES;
  if (rows == 0) {
#pragma unroll
    for (int q = 0; q < FMX_MET_VALUES; ++q) v[q] = mt_nan();
  } else {
    const double dn = (double)rows;
    if (a.cls) {
      const int64_t N = rows - P;
      v[FMX_MET_AUC] = (P == 0 || N == 0) ? mt_nan() : __ddiv_rn(__ull2double_rn(p2), __ull2double_rn(2ull * (unsigned long long)P * (unsigned long long)N));
      v[FMX_MET_LOGLOSS] = __ddiv_rn(s[0], dn);
      v[FMX_MET_ACCURACY] = __ddiv_rn((double)C, dn);
      v[FMX_MET_BRIER] = __ddiv_rn(s[1], dn);
      v[FMX_MET_MEAN_PRED] = __ddiv_rn(s[2], dn);
      v[FMX_MET_MEAN_LABEL] = __ddiv_rn((double)P, dn);
    } else {
      const double mse = __ddiv_rn(s[0], dn);
      v[FMX_MET_MSE] = mse;
      v[FMX_MET_RMSE] = __dsqrt_rn(mse);
      v[FMX_MET_MAE] = __ddiv_rn(s[1], dn);
      v[FMX_MET_MEAN_ERR] = __ddiv_rn(s[2], dn);
      v[FMX_MET_MEAN_PRED] = __ddiv_rn(s[3], dn);
      v[FMX_MET_MEAN_LABEL] = __ddiv_rn(s[4], dn);
    }
  }
  if (count) {
    int64_t* c = count + (size_t)g * FMX_MET_COUNTS;
    c[FMX_MET_ROWS] = rows; c[FMX_MET_POSITIVES] = P; c[FMX_MET_PAIRS2] = (int64_t)p2; c[FMX_MET_CORRECT] = C;
  }
}

}  // namespace

MetLimits metrics_limits() {
  MetLimits l;
  l.wave_rows = g_wave_rows.load();
  l.lds_rows = g_lds_rows.load();
  l.chunk_rows = g_chunk_rows.load();
  if (l.wave_rows == 0 || l.wave_rows > MT_WAVE_ROWS) l.wave_rows = MT_WAVE_ROWS;   // (a negative value: the form is off)
  if (l.lds_rows == 0 || l.lds_rows > MT_LDS_ROWS) l.lds_rows = MT_LDS_ROWS;
  if (l.chunk_rows <= 0) l.chunk_rows = MT_FWD_ROWS;
  return l;
}

void debug_metrics_limits(int wave_rows, int lds_rows, int64_t chunk_rows) {
  g_wave_rows.store(wave_rows);
  g_lds_rows.store(lds_rows);
  g_chunk_rows.store(chunk_rows > 0 ? chunk_rows : 0);
}

int metrics_run(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, const uint32_t* d_group, int64_t G, int link, const MetLimits& lim, double* d_value,
                int64_t* d_count) {
  const int64_t n = r1 - r0;
  if (n <= 0) return FMX_OK;
  hipStream_t st = e->stream;
  if (link == FMX_LINK_PROBIT) FMX_TRY(ensure_probit(e));
  Scratch S(st);

  // the raw scores, in forward calls of chunk_rows rows (a short tail joins the call before it)
  double* z = nullptr;
  FMX_TRY(S.get(&z, (size_t)n));
  for (int64_t a = 0; a < n;) {
    int64_t b = std::min(n, a + lim.chunk_rows);
    if (n - b < lim.chunk_rows / 16) b = n;
    FMX_TRY(forward_rows(e, m, r0 + a, r0 + b, z + a, FMX_LINK_NONE));
    a = b;
  }

  MtArgs a{};
  a.z = z; a.y = m->y + r0;
  a.G = G;
  a.cls = e->hyper.task == FMX_TASK_CLASSIFICATION ? 1 : 0;
  a.link = link;
  a.h = e->hyper;
  a.pn_y = e->probit;
  a.wave_rows = lim.wave_rows; a.lds_rows = lim.lds_rows;

  // the groups' CSR
  int64_t* off = nullptr;
  FMX_TRY(S.get(&off, (size_t)G + 1));
  uint32_t* gsorted = nullptr;
  if (d_group) {
    uint32_t *k_in = nullptr, *v_in = nullptr, *rows = nullptr;
    FMX_TRY(S.get(&k_in, (size_t)n)); FMX_TRY(S.get(&v_in, (size_t)n));
    FMX_TRY(S.get(&gsorted, (size_t)n)); FMX_TRY(S.get(&rows, (size_t)n));
    hipLaunchKernelGGL(mt_group_keys_k, dim3(blocks(n, MT_THREADS)), dim3(MT_THREADS), 0, st, d_group, n, G, k_in, v_in);
    FMX_HIP(hipGetLastError());
    FMX_TRY(sort_pairs(S, k_in, gsorted, v_in, rows, n, key_bits((uint64_t)G)));
    FMX_TRY(group_offsets(gsorted, n, G, off, st));
    a.rows = rows;
  } else {
    const int64_t h_off[2] = {0, n};   // G == 1
    FMX_HIP(hipMemcpy(off, h_off, sizeof(h_off), hipMemcpyHostToDevice));
  }
  a.off = off;

  // chunks of the sums and rows of the global form, per group and in all
  int64_t *nch = nullptr, *llen = nullptr, *ioff = nullptr, *loff = nullptr;
  FMX_TRY(S.get(&nch, (size_t)G + 1)); FMX_TRY(S.get(&llen, (size_t)G + 1));
  FMX_TRY(S.get(&ioff, (size_t)G + 1)); FMX_TRY(S.get(&loff, (size_t)G + 1));
  hipLaunchKernelGGL(mt_plan_k, dim3(blocks(G + 1, MT_THREADS)), dim3(MT_THREADS), 0, st, a, nch, llen);
  FMX_HIP(hipGetLastError());
  FMX_TRY(exclusive_sum(S, (const int64_t*)nch, ioff, G + 1));
  FMX_TRY(exclusive_sum(S, (const int64_t*)llen, loff, G + 1));
  int64_t items = 0, nl = 0;
  FMX_HIP(hipMemcpyAsync(&items, ioff + G, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipMemcpyAsync(&nl, loff + G, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  FMX_CHECK(items >= 0 && items < (1LL << 31) && nl >= 0 && nl <= n, FMX_ERR_HIP, "metrics: the group plan is inconsistent (%lld chunks, %lld rows)", (long long)items,
            (long long)nl);

  double* part = nullptr;
  int64_t* ipart = nullptr;
  FMX_TRY(S.get(&part, (size_t)items * MT_SUMS)); FMX_TRY(S.get(&ipart, (size_t)items * 2));
  if (items > 0) {
    hipLaunchKernelGGL(mt_sums_k, dim3((unsigned)items), dim3(MT_THREADS), 0, st, a, (const int64_t*)ioff, part, ipart);
    FMX_HIP(hipGetLastError());
  }

  unsigned long long* pairs2 = nullptr;
  if (a.cls) {
    FMX_TRY(S.get(&pairs2, (size_t)G));
    FMX_HIP(hipMemsetAsync(pairs2, 0, (size_t)G * sizeof(unsigned long long), st));
    if (a.wave_rows > 0) {
      hipLaunchKernelGGL(mt_pairs_wave_k, dim3(blocks(G, MT_WAVES)), dim3(MT_THREADS), 0, st, a, pairs2);
      FMX_HIP(hipGetLastError());
    }
    if (a.lds_rows > 0 && n > (a.wave_rows > 0 ? a.wave_rows : 0)) {   // some group may be longer than the wave form takes
      hipLaunchKernelGGL(mt_pairs_wg_k, dim3((unsigned)G), dim3(MT_THREADS), 0, st, a, pairs2);
      FMX_HIP(hipGetLastError());
    }
    if (nl > 0) {
      uint64_t *lkey = nullptr, *skey = nullptr;
      uint32_t *lval = nullptr, *sval = nullptr, *negf = nullptr, *head = nullptr, *ns = nullptr, *rh = nullptr;
      FMX_TRY(S.get(&lkey, (size_t)nl)); FMX_TRY(S.get(&skey, (size_t)nl));
      FMX_TRY(S.get(&lval, (size_t)nl)); FMX_TRY(S.get(&sval, (size_t)nl));
      hipLaunchKernelGGL(mt_long_fill_k, dim3(blocks(n, MT_THREADS)), dim3(MT_THREADS), 0, st, a, n, (const uint32_t*)gsorted, (const int64_t*)loff, lkey, lval);
      FMX_HIP(hipGetLastError());
      FMX_TRY(sort_pairs(S, lkey, skey, lval, sval, nl, 64));
      const uint32_t* row = sval;
      if (d_group) {   // then by group, stably: (group, key) order
        uint32_t* gk = (uint32_t*)lkey;   // lkey is free again: 2 nl u32
        hipLaunchKernelGGL(mt_long_groups_k, dim3(blocks(nl, MT_THREADS)), dim3(MT_THREADS), 0, st, d_group, (const uint32_t*)sval, nl, gk);
        FMX_HIP(hipGetLastError());
        FMX_TRY(sort_pairs(S, gk, gk + nl, sval, lval, nl, key_bits((uint64_t)G)));
        row = lval;
      }
      FMX_TRY(S.get(&negf, (size_t)nl)); FMX_TRY(S.get(&head, (size_t)nl));
      FMX_TRY(S.get(&ns, (size_t)nl)); FMX_TRY(S.get(&rh, (size_t)nl));
      hipLaunchKernelGGL(mt_long_flags_k, dim3(blocks(nl, MT_THREADS)), dim3(MT_THREADS), 0, st, a, d_group, row, nl, negf, head);
      FMX_HIP(hipGetLastError());
      FMX_TRY(exclusive_sum(S, (const uint32_t*)negf, ns, nl));
      FMX_TRY(inclusive_max(S, (const uint32_t*)head, rh, nl));
      hipLaunchKernelGGL(mt_long_acc_k, dim3(blocks(nl, MT_THREADS)), dim3(MT_THREADS), 0, st, d_group, row, nl, (const uint32_t*)negf, (const uint32_t*)ns,
                         (const uint32_t*)rh, (const int64_t*)loff, pairs2);
      FMX_HIP(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(mt_finish_k, dim3(blocks(G, MT_THREADS)), dim3(MT_THREADS), 0, st, a, (const int64_t*)ioff, (const double*)part, (const int64_t*)ipart,
                     (const unsigned long long*)pairs2, d_value, d_count);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

}  // namespace fmx
