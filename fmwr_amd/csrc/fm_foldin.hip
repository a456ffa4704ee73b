// Fold-in (fmx_fold_in): the rows (w_u, v_u) of features the model has not seen, solved against the frozen model.
//
// A row r that stores fold feature u exactly once, with value x, predicts
//     y(r) = b_r + <z_r, theta_u>,   theta_u = (w_u, v_u),   z_r = x (keep_w1, t_r),   t_r = sum_{j != u} x_j v_j,
// b_r the forward of the row without that entry.  Squared loss: (Z'Z + Lambda) theta = Z'(y - b), one Cholesky solve.  Logistic loss: n_newton
// full Newton steps from theta = 0.  Both are the same loop here: H = sum c_r z_r z_r' + Lambda, rhs = sum d_r z_r - Lambda theta,
// theta += H^-1 rhs, with c = 1, d = y - b (squared, one step) or c = sigma (1 - sigma), d = y (1 - sigma) (logistic).
//
//   fold_find_k   one thread per row: the row's fold entry through a p-bit membership map, its group (the rank of the column among the
//                 sorted ids) as sort key, its position; a second fold entry or a label other than +-1 raises an integer flag
//   (fm_prims)    stable radix sort of (group, row): rows ascending inside a group; the groups' offsets by binary search
//   fold_rows_k   one lane group per participating row (a 16-byte slice of the factor row per lane, as the forward): b_r and z_r in fp64,
//                 the fold entry skipped by POSITION -- the fold features' current parameters are never read
//   fold_gram_k   one workgroup per (group, chunk of FI_CHUNK rows): the upper triangle of sum c z z' as 4 x 4 register blocks, z broadcast
//                 from LDS (VALU fp64 fma), and sum d z; every sum runs over the chunk's rows in ascending order
//   fold_solve_k  one workgroup per group: the chunks' partial sums added in ascending chunk order, + Lambda, in-LDS Cholesky with the pivot
//                 check, two triangular solves, theta += delta
// The pairwise form (fmx_fold_in_pairs) is the logistic loop with every label +1 on difference vectors: the units that are
// keyed, sorted, counted and summed over are the PAIRS (rows 2t, 2t + 1) of a pair matrix.
//   fold_pair_key_k  one thread per pair: the pair's key from its rows' keys; rows that name different groups raise a flag
//   fold_pairs_k     two neighbouring lane groups per participating pair, one per row, the rows' sums by the device function fold_rows_k
//                    uses; B_t = b_2t - b_2t+1 and Z_t = z_2t - z_2t+1 taken in registers across the wave
// and the Gram kernel, the solve and the slab loop run on (B, Z) as they do on (b, z).
// Every floating-point sum has a fixed order that depends on the group's own rows alone (no floating-point atomics): a feature's bits do not
// depend on what else the call folds.  Groups are worked off in slabs of bounded rows, and one group holds at most FI_GROUP_ROWS_MAX rows (refused beyond,
// before anything is written), so the kept (b, z) rows stay bounded.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "fm_prims.h"

namespace fmx {
namespace {

constexpr int FI_THREADS = 256;
constexpr int FI_CHUNK = 256;      // rows per (group, chunk) workgroup of the Gram kernel
constexpr int FI_RT = 32;          // rows staged in LDS at a time
constexpr int FI_DMAX = 65;        // 1 + 64 factors
constexpr int FI_DPMAX = 68;       // padded to the 4 x 4 blocks
constexpr int FI_RHS_T0 = 160;     // first thread of the right-hand side (the blocks take at most 153 threads)
constexpr int64_t FI_SLAB_ROWS = 1 << 22;    // participating rows per slab (about 2.2 GB of z at 64 factors)
constexpr int64_t FI_SLAB_GROUPS = 1 << 15;  // groups per slab
constexpr int64_t FI_GROUP_ROWS_MAX = 1 << 24;  // rows of ONE fold feature: a group is never cut, so this bounds the (b, z) workspace (8.7 GB at 64 factors)
constexpr uint32_t FI_NONE = 0xffffffffu;

enum : int { FI_FLAG_TWO = 1, FI_FLAG_LABEL = 2, FI_FLAG_MIXED = 4 };

std::atomic<int64_t> g_slab_rows_once{0}, g_slab_groups_once{0};  // test hook: the next call's slab limits

// ------------------------------------------------------------------------------------------------------------ select and group

__global__ __launch_bounds__(FI_THREADS) void fold_find_k(const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, const float* __restrict__ y, int64_t n,
                                                         const uint32_t* __restrict__ bits, const uint32_t* __restrict__ sorted_ids, int n_ids, int check_labels,
                                                         uint32_t* __restrict__ key, uint32_t* __restrict__ pos, int64_t* __restrict__ rows, int* __restrict__ flag) {
  const int64_t r = (int64_t)blockIdx.x * FI_THREADS + threadIdx.x;
  if (r >= n) return;
  const int64_t a = row_ptr[r], b = row_ptr[r + 1];
  int found = 0;
  int64_t at = 0;
  uint32_t c_at = 0;
  for (int64_t t = a; t < b; ++t) {
    const uint32_t c = col[t];
    if ((bits[c >> 5] >> (c & 31)) & 1u) {
      if (found == 0) { at = t; c_at = c; }
      ++found;
    }
  }
  uint32_t g = FI_NONE, off = 0;
  if (found == 1) {
    int lo = 0, hi = n_ids;  // the rank of c_at among the sorted ids (it is one of them)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sorted_ids[mid] < c_at) lo = mid + 1; else hi = mid;
    }
    g = (uint32_t)lo;
    off = (uint32_t)(at - a);
    if (check_labels) {
      const float l = y[r];
      if (!(l == 1.0f || l == -1.0f)) atomicOr(flag, FI_FLAG_LABEL);
    }
  } else if (found > 1) {
    atomicOr(flag, FI_FLAG_TWO);
  }
  key[r] = g == FI_NONE ? (uint32_t)n_ids : g;  // rows without a fold entry sort behind every group
  pos[r] = off;
  rows[r] = r;
}

// pairs (fmx_fold_in_pairs): rows 2t and 2t + 1 form pair t.  Its key is the group either row names (n_ids: neither does); two different groups
// in one pair raise FI_FLAG_MIXED
__global__ __launch_bounds__(FI_THREADS) void fold_pair_key_k(const uint32_t* __restrict__ row_key, int64_t n_pairs, int n_ids, uint32_t* __restrict__ pair_key,
                                                             int* __restrict__ flag) {
  const int64_t t = (int64_t)blockIdx.x * FI_THREADS + threadIdx.x;
  if (t >= n_pairs) return;
  const uint32_t none = (uint32_t)n_ids;
  const uint32_t ka = row_key[2 * t], kb = row_key[2 * t + 1];
  if (ka != none && kb != none && ka != kb) atomicOr(flag, FI_FLAG_MIXED);
  pair_key[t] = ka != none ? ka : kb;
}

// ------------------------------------------------------------------------------------------------------------ row pass

__device__ __forceinline__ void fi_get(const float4& v, double* o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
__device__ __forceinline__ void fi_get(const double2& v, double* o) { o[0] = v.x; o[1] = v.y; }

struct FoldRowsArgs {
  const int64_t* row_ptr;
  const uint32_t* col;
  const float* val;
  const int64_t* rows;   // sorted (group, row) order -- fold_pairs_k: sorted (group, pair) order
  const uint32_t* pos;   // per ROW: the fold entry's offset inside the row
  const uint32_t* row_key;  // fold_pairs_k only, per ROW: its group, or n_ids when it stores no fold entry
  uint32_t n_ids;
  int64_t i0, count;     // sorted positions [i0, i0 + count)
  const void* V;
  const void* w;
  int64_t vs, ws;
  const double* scal;
  int k, D, lpr, k0, k1, unit;
  double* B;             // [count]
  double* Z;             // [count][D]
};

// The sums of one row over the entries [ta, tb) without the one at `skip` (-1: none), by one lane group of a.lpr lanes -- the arithmetic that
// fold_rows_k and fold_pairs_k share: s[f] = sum x_j v_j,f of this lane's factors, and b = w0term + sum w_j x_j + the pairwise term.  The
// linear sum lives in lane 0 of the group, so b is the row's b there (and only there).  Every lane of a wave must call it (butterfly).
template <typename T>
__device__ __forceinline__ double fold_row_sums(const FoldRowsArgs& a, int64_t ta, int64_t tb, int64_t skip, int lig, double w0term, double* s) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VEC = StateVec<T>::N;
  const T* __restrict__ Vt = reinterpret_cast<const T*>(a.V) + lig * VEC;
  const T* __restrict__ wt = reinterpret_cast<const T*>(a.w);
  const bool withv = a.k > 0;
  double q[VEC];
#pragma unroll
  for (int f = 0; f < VEC; ++f) s[f] = q[f] = 0.0;
  double lin = 0.0;
  for (int64_t t = ta; t < tb; ++t) {
    if (t == skip) continue;
    const size_t j = a.col[t];
    const double x = a.unit ? 1.0 : (double)a.val[t];
    if (withv) {
      const vec_t vv = *reinterpret_cast<const vec_t*>(Vt + j * a.vs);
      double vf[VEC];
      fi_get(vv, vf);
#pragma unroll
      for (int f = 0; f < VEC; ++f) {
        const double d = vf[f] * x;
        s[f] += d;
        q[f] += d * d;
      }
    }
    if (a.k1 && lig == 0) lin += (double)wt[j * a.ws] * x;
  }
  double part = 0.0;
#pragma unroll
  for (int f = 0; f < VEC; ++f) part += s[f] * s[f] - q[f];
  for (int off = a.lpr >> 1; off > 0; off >>= 1) part += __shfl_xor(part, off);  // commutative steps: the same bits in every lane
  return w0term + lin + 0.5 * part;
}

template <typename T>
__global__ __launch_bounds__(FI_THREADS) void fold_rows_k(FoldRowsArgs a) {
  constexpr int VEC = StateVec<T>::N;
  const int lpr = a.lpr;
  const int rpw = FI_THREADS / lpr;
  const int gid = threadIdx.x / lpr, lig = threadIdx.x % lpr;
  const int64_t i = (int64_t)blockIdx.x * rpw + gid;
  const bool live = i < a.count;   // every lane stays for the butterfly
  int64_t ta = 0, tb = 0, skip = -1;
  if (live) {
    const int64_t r = a.rows[a.i0 + i];
    ta = a.row_ptr[r];
    tb = a.row_ptr[r + 1];
    skip = ta + a.pos[r];
  }
  double s[VEC];
  const double b = fold_row_sums<T>(a, ta, tb, skip, lig, a.k0 ? a.scal[SC_W0] : 0.0, s);
  if (!live) return;
  const double xu = a.unit ? 1.0 : (double)a.val[skip];
  double* z = a.Z + (size_t)i * a.D;
  if (lig == 0) {
    a.B[i] = b;
    z[0] = a.k1 ? xu : 0.0;
  }
#pragma unroll
  for (int f = 0; f < VEC; ++f) {
    const int ff = lig * VEC + f;
    if (ff < a.k) z[1 + ff] = xu * s[f];
  }
}

// The pair pass: two neighbouring lane groups (2 lpr <= 64 lanes, one wave) take the rows 2t and 2t + 1 of the pair at a sorted position; each
// forms its row's b (without w0: it cancels) and z slice exactly as fold_rows_k does -- a row without a fold entry skips nothing and has z = 0
// by SELECTION, so a sum that is not finite cannot enter through 0 * inf -- and the group of row 2t fetches its partner's values across the
// wave and stores B_t = b_2t - b_2t+1, Z_t = z_2t - z_2t+1.
template <typename T>
__global__ __launch_bounds__(FI_THREADS) void fold_pairs_k(FoldRowsArgs a) {
  constexpr int VEC = StateVec<T>::N;
  const int lpr = a.lpr;
  const int ppw = FI_THREADS / (2 * lpr);
  const int gid = threadIdx.x / lpr, lig = threadIdx.x % lpr;
  const int64_t i = (int64_t)blockIdx.x * ppw + (gid >> 1);
  const bool live = i < a.count;   // both groups of a pair alike; every lane stays for the butterfly and the exchange
  int64_t ta = 0, tb = 0, skip = -1;
  bool has = false;
  if (live) {
    const int64_t r = 2 * a.rows[a.i0 + i] + (gid & 1);
    ta = a.row_ptr[r];
    tb = a.row_ptr[r + 1];
    has = a.row_key[r] != a.n_ids;
    if (has) skip = ta + a.pos[r];
  }
  double s[VEC];
  const double b = fold_row_sums<T>(a, ta, tb, skip, lig, 0.0, s);
  double xu = 0.0;
  if (has) xu = a.unit ? 1.0 : (double)a.val[skip];
  const double z0 = (has && a.k1) ? xu : 0.0;
  double zf[VEC];
#pragma unroll
  for (int f = 0; f < VEC; ++f) zf[f] = has ? xu * s[f] : 0.0;
  const double pb = __shfl_xor(b, lpr), pz0 = __shfl_xor(z0, lpr);
  double pz[VEC];
#pragma unroll
  for (int f = 0; f < VEC; ++f) pz[f] = __shfl_xor(zf[f], lpr);
  if (!live || (gid & 1)) return;
  double* z = a.Z + (size_t)i * a.D;
  if (lig == 0) {
    a.B[i] = b - pb;
    z[0] = z0 - pz0;
  }
#pragma unroll
  for (int f = 0; f < VEC; ++f) {
    const int ff = lig * VEC + f;
    if (ff < a.k) z[1 + ff] = zf[f] - pz[f];
  }
}

// ------------------------------------------------------------------------------------------------------------ Gram and right-hand side

__device__ __forceinline__ int fi_tri(int i, int j, int D) { return i * D - (i * (i - 1)) / 2 + (j - i); }  // packed upper triangle, i <= j

struct FoldGramArgs {
  const double* B;           // slab arrays, indexed by the slab's sorted position
  const double* Z;
  const int64_t* rows;       // sorted (group, row) order, whole call
  int64_t i0;                // the slab's first sorted position
  const float* y;            // NULL: every label is +1
  const uint32_t* chunk_grp; // [chunks] group (slab-local) of every chunk
  const int64_t* chunk_a;    // [chunks] first row (slab-local sorted position) ...
  const int64_t* chunk_b;    // ... and the end
  const double* theta;       // [slab groups][D]
  int D, DP, logistic, dot;
  double* P;                 // [chunks][D (D + 1) / 2 + D]
};

__global__ __launch_bounds__(FI_THREADS) void fold_gram_k(FoldGramArgs a) {
  __shared__ double zt[FI_RT * FI_DPMAX];
  __shared__ double cs[FI_RT], ds[FI_RT];
  __shared__ double th[FI_DPMAX];
  const int tid = threadIdx.x;
  const int D = a.D, DP = a.DP, NB = DP / 4;
  const int ntri = D * (D + 1) / 2;
  const int c = blockIdx.x;
  const int64_t ra = a.chunk_a[c], rb = a.chunk_b[c];
  const uint32_t g = a.chunk_grp[c];
  // thread -> its 4 x 4 block (bi <= bj) of the upper triangle
  int bi = -1, bj = -1;
  {
    int t = tid;
    for (int i = 0; i < NB; ++i) {
      const int w = NB - i;
      if (t < w) { bi = i; bj = i + t; break; }
      t -= w;
    }
  }
  const int ri = tid - FI_RHS_T0;   // the right-hand side's component of this thread, if in [0, D)
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  double racc = 0.0;
  if (tid < DP) th[tid] = (a.dot && tid < D) ? a.theta[(size_t)g * D + tid] : 0.0;

  for (int64_t r0 = ra; r0 < rb; r0 += FI_RT) {
    const int cnt = rb - r0 < FI_RT ? (int)(rb - r0) : FI_RT;
    for (int idx = tid; idx < FI_RT * DP; idx += FI_THREADS) {
      const int rr = idx / DP, cc = idx - rr * DP;
      zt[idx] = (rr < cnt && cc < D) ? a.Z[(size_t)(r0 + rr) * D + cc] : 0.0;
    }
    __syncthreads();
    if (tid < FI_RT) {
      double cr = 0.0, dr = 0.0;
      if (tid < cnt) {
        double yh = a.B[r0 + tid];
        if (a.dot) {
          double dp = 0.0;
          for (int i = 0; i < D; ++i) dp = fma(zt[tid * DP + i], th[i], dp);
          yh += dp;
        }
        const double yr = a.y ? (double)a.y[a.rows[a.i0 + r0 + tid]] : 1.0;   // (no labels: every label is +1, the pair call)
        if (a.logistic) {
          const double m = yr * yh;
          const double sg = 1.0 / (1.0 + exp(-m));   // sigma
          const double ng = 1.0 / (1.0 + exp(m));    // 1 - sigma, without the cancellation
          cr = sg * ng;
          dr = yr * ng;
        } else {
          cr = 1.0;
          dr = yr - yh;
        }
      }
      cs[tid] = cr;
      ds[tid] = dr;
    }
    __syncthreads();
    if (bi >= 0) {
      for (int rr = 0; rr < FI_RT; ++rr) {   // rows past cnt hold zeros
        const double* zr = zt + rr * DP;
        const double cr = cs[rr];
        double zi[4], zj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { zi[u] = cr * zr[4 * bi + u]; zj[u] = zr[4 * bj + u]; }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = fma(zi[i], zj[j], acc[i][j]);
      }
    } else if (ri >= 0 && ri < D) {
      for (int rr = 0; rr < FI_RT; ++rr) racc = fma(ds[rr], zt[rr * DP + ri], racc);
    }
    __syncthreads();
  }
  double* P = a.P + (size_t)c * (ntri + D);
  if (bi >= 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int gi = 4 * bi + i, gj = 4 * bj + j;
        if (gi <= gj && gj < D) P[fi_tri(gi, gj, D)] = acc[i][j];
      }
  } else if (ri >= 0 && ri < D) {
    P[ntri + ri] = racc;
  }
}

// ------------------------------------------------------------------------------------------------------------ solve

struct FoldSolveArgs {
  const double* P;
  const int64_t* cptr;   // [slab groups + 1] chunks of every group
  double* theta;         // [slab groups][D]
  int* status;           // [slab groups]
  int D, k1;
  double lw, lv;
};

__global__ __launch_bounds__(FI_THREADS) void fold_solve_k(FoldSolveArgs a) {
  __shared__ double A[FI_DMAX * FI_DMAX];
  __shared__ double diag[FI_DMAX], xv[FI_DMAX];
  const int tid = threadIdx.x;
  const int D = a.D;
  const int ntri = D * (D + 1) / 2;
  const int g = blockIdx.x;
  const int64_t c0 = a.cptr[g], c1 = a.cptr[g + 1];
  const size_t pstride = (size_t)ntri + D;
  for (int idx = tid; idx < D * D; idx += FI_THREADS) {
    const int i = idx / D, j = idx - i * D;
    if (i > j) continue;
    const int e = fi_tri(i, j, D);
    double s = 0.0;
    for (int64_t c = c0; c < c1; ++c) s += a.P[(size_t)c * pstride + e];   // ascending chunk order
    if (i == j) s += i == 0 ? a.lw : a.lv;
    if (!a.k1 && i == 0) s = j == 0 ? 1.0 : 0.0;   // w_u is not a variable
    A[i * D + j] = s;
    A[j * D + i] = s;
  }
  double rhs = 0.0, th = 0.0;
  if (tid < D) {
    for (int64_t c = c0; c < c1; ++c) rhs += a.P[(size_t)c * pstride + ntri + tid];
    th = a.theta[(size_t)g * D + tid];
    rhs -= (tid == 0 ? a.lw : a.lv) * th;
    if (!a.k1 && tid == 0) rhs = 0.0;
  }
  __syncthreads();
  // right-looking Cholesky on the lower triangle; the diagonal of L goes to diag[]
  bool bad = false;
  for (int j = 0; j < D; ++j) {
    const double piv = A[j * D + j];
    if (!(piv > 0.0) || !isfinite(piv)) { bad = true; break; }   // uniform: every thread reads the same word
    const double l = sqrt(piv);
    if (tid == 0) diag[j] = l;
    for (int i = j + 1 + tid; i < D; i += FI_THREADS) A[i * D + j] = A[i * D + j] / l;
    __syncthreads();
    const int m = D - 1 - j;
    for (int idx = tid; idx < m * m; idx += FI_THREADS) {
      const int i = j + 1 + idx / m, c = j + 1 + idx % m;
      if (c <= i) A[i * D + c] -= A[i * D + j] * A[c * D + j];
    }
    __syncthreads();
  }
  if (bad) {
    if (tid < D) a.theta[(size_t)g * D + tid] = __longlong_as_double(0x7ff8000000000000LL);
    if (tid == 0) a.status[g] = 1;
    return;
  }
  // L y = rhs, then L' x = y: thread i carries component i
  for (int j = 0; j < D; ++j) {
    if (tid == j) xv[j] = rhs / diag[j];
    __syncthreads();
    if (tid > j && tid < D) rhs -= A[tid * D + j] * xv[j];
  }
  __syncthreads();
  if (tid < D) rhs = xv[tid];
  __syncthreads();
  for (int j = D - 1; j >= 0; --j) {
    if (tid == j) xv[j] = rhs / diag[j];
    __syncthreads();
    if (tid < j) rhs -= A[j * D + tid] * xv[j];
  }
  __syncthreads();
  if (tid < D) a.theta[(size_t)g * D + tid] = th + xv[tid];
}

}  // namespace

// arguments checked by fmx_fold_in / fmx_fold_in_pairs; ids are distinct and < p, n_ids >= 1.  Host results in the order of `ids`: theta [n_ids][1 + k],
// rows, status.  pairs: m is a pair matrix (an even row count) and the UNITS that are selected, sorted, counted and summed over are its pairs
// (DESIGN.md section 19): the logistic loop with every label +1 on B_t, Z_t; otherwise the units are m's rows.
int foldin_run(fmx_engine* e, const fmx_matrix* m, const uint32_t* ids, int64_t n_ids, double lw, double lv, int n_newton, bool pairs,
               std::vector<double>* theta_out, std::vector<int64_t>* rows_out, std::vector<int32_t>* status_out) {
  const int k = e->k, D = 1 + k, DP = (D + 3) / 4 * 4;
  const int ntri = D * (D + 1) / 2;
  const bool logistic = pairs || e->hyper.task == FMX_TASK_CLASSIFICATION;
  const int steps = logistic ? n_newton : 1;
  const int64_t n = m->n;                   // rows
  const int64_t nu = pairs ? n / 2 : n;     // units
  const char* unit = pairs ? "pairs" : "rows";
  hipStream_t st = e->stream;

  // ascending ids: group g is the g-th smallest id, whatever order the caller listed them in
  std::vector<uint32_t> order((size_t)n_ids);
  for (int64_t i = 0; i < n_ids; ++i) order[(size_t)i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ids[x] < ids[y]; });
  std::vector<uint32_t> sorted((size_t)n_ids);
  for (int64_t g = 0; g < n_ids; ++g) sorted[(size_t)g] = ids[order[(size_t)g]];
  const size_t words = ((size_t)m->p + 31) / 32;
  std::vector<uint32_t> bits(words, 0u);
  for (uint32_t c : sorted) bits[c >> 5] |= 1u << (c & 31);

  DevBuf d_bits, d_sorted, d_key, d_pkey, d_key_s, d_pos, d_rows, d_rows_s, d_flag, d_off, d_tmp;
  FMX_TRY(dev_buf(&d_bits, words * sizeof(uint32_t)));
  FMX_TRY(dev_buf(&d_sorted, (size_t)n_ids * sizeof(uint32_t)));
  FMX_TRY(dev_buf(&d_flag, sizeof(int)));
  FMX_TRY(dev_buf(&d_off, (size_t)(n_ids + 1) * sizeof(int64_t)));
  FMX_HIP(hipMemcpy(d_bits.get(), bits.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
  FMX_HIP(hipMemcpy(d_sorted.get(), sorted.data(), (size_t)n_ids * sizeof(uint32_t), hipMemcpyHostToDevice));
  FMX_HIP(hipMemset(d_flag.get(), 0, sizeof(int)));
  std::vector<int64_t> off((size_t)n_ids + 1, 0);
  if (n > 0) {
    FMX_TRY(dev_buf(&d_key, (size_t)n * sizeof(uint32_t)));
    FMX_TRY(dev_buf(&d_key_s, (size_t)nu * sizeof(uint32_t)));
    FMX_TRY(dev_buf(&d_pos, (size_t)n * sizeof(uint32_t)));
    FMX_TRY(dev_buf(&d_rows, (size_t)n * sizeof(int64_t)));
    FMX_TRY(dev_buf(&d_rows_s, (size_t)nu * sizeof(int64_t)));
    const int64_t grid = (n + FI_THREADS - 1) / FI_THREADS;
    FMX_CHECK(grid < (1LL << 31), FMX_ERR_INVALID, "fold-in: too many rows (%lld)", (long long)n);
    hipLaunchKernelGGL(fold_find_k, dim3((unsigned)grid), dim3(FI_THREADS), 0, st, m->row_ptr, m->col, m->y, n, (const uint32_t*)d_bits.get(),
                       (const uint32_t*)d_sorted.get(), (int)n_ids, (logistic && !pairs) ? 1 : 0, (uint32_t*)d_key.get(), (uint32_t*)d_pos.get(), (int64_t*)d_rows.get(),
                       (int*)d_flag.get());
    FMX_HIP(hipGetLastError());
    const uint32_t* unit_key = (const uint32_t*)d_key.get();
    if (pairs) {
      // the pairs' keys from the rows'; the pair indices 0 .. nu - 1 to sort along are the first nu entries of the identity fold_find_k wrote
      FMX_TRY(dev_buf(&d_pkey, (size_t)nu * sizeof(uint32_t)));
      hipLaunchKernelGGL(fold_pair_key_k, dim3((unsigned)((nu + FI_THREADS - 1) / FI_THREADS)), dim3(FI_THREADS), 0, st, (const uint32_t*)d_key.get(), nu, (int)n_ids,
                         (uint32_t*)d_pkey.get(), (int*)d_flag.get());
      FMX_HIP(hipGetLastError());
      unit_key = (const uint32_t*)d_pkey.get();
    }
    int flag = 0;
    FMX_HIP(hipMemcpyAsync(&flag, d_flag.get(), sizeof(int), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    FMX_CHECK(!(flag & FI_FLAG_TWO), FMX_ERR_INVALID, "fold-in: a row stores more than one entry of the fold features");
    FMX_CHECK(!(flag & FI_FLAG_LABEL), FMX_ERR_INVALID, "fold-in: CLASSIFICATION labels must be +1 or -1");
    FMX_CHECK(!(flag & FI_FLAG_MIXED), FMX_ERR_INVALID, "fold-in: the two rows of a pair store different fold features");
    const int bits = key_bits((uint64_t)n_ids);
    size_t tb = 0;   // (the two-phase form on a buffer of its own: released below, before the slab loop)
    FMX_TRY(sort_pairs(nullptr, tb, unit_key, (uint32_t*)d_key_s.get(), (const int64_t*)d_rows.get(), (int64_t*)d_rows_s.get(), nu, bits, st));
    FMX_TRY(dev_buf(&d_tmp, tb));
    FMX_TRY(sort_pairs(d_tmp.get(), tb, unit_key, (uint32_t*)d_key_s.get(), (const int64_t*)d_rows.get(), (int64_t*)d_rows_s.get(), nu, bits, st));   // stable: rows (pairs) ascending inside a group
    FMX_TRY(group_offsets((const uint32_t*)d_key_s.get(), nu, n_ids, (int64_t*)d_off.get(), st));   // off[n_ids] = the participating rows (pairs)
    FMX_HIP(hipMemcpyAsync(off.data(), d_off.get(), off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    if (!pairs) d_key.reset();   // (the pair pass asks the rows' keys which of a pair's rows hold the fold entry)
    d_pkey.reset(); d_rows.reset(); d_tmp.reset(); d_key_s.reset();
  }

  for (int64_t g = 0; g < n_ids; ++g)
    FMX_CHECK(off[(size_t)g + 1] - off[(size_t)g] <= FI_GROUP_ROWS_MAX, FMX_ERR_INVALID, "fold-in: feature %u is stored in %lld %s; one fold feature may hold at most %lld",
              sorted[(size_t)g], (long long)(off[(size_t)g + 1] - off[(size_t)g]), unit, (long long)FI_GROUP_ROWS_MAX);
  int64_t slab_rows = g_slab_rows_once.exchange(0), slab_groups = g_slab_groups_once.exchange(0);
  if (slab_rows <= 0) slab_rows = FI_SLAB_ROWS;
  if (slab_groups <= 0) slab_groups = FI_SLAB_GROUPS;
  std::vector<double> theta_s((size_t)n_ids * D, 0.0);   // in group (sorted id) order
  std::vector<int32_t> status_s((size_t)n_ids, 0);
  DevBuf d_B, d_Z, d_P, d_cg, d_ca, d_cb, d_cptr, d_theta, d_status;
  size_t capB = 0, capP = 0, capC = 0, capG = 0;
  for (int64_t g0 = 0; g0 < n_ids;) {
    // the slab: groups [g0, g1) of at most FI_SLAB_ROWS rows together (a larger group is a slab of its own) and FI_SLAB_GROUPS groups
    int64_t g1 = g0 + 1;
    while (g1 < n_ids && g1 - g0 < slab_groups && off[(size_t)g1 + 1] - off[(size_t)g0] <= slab_rows) ++g1;
    const int64_t ng = g1 - g0, i0 = off[(size_t)g0], cnt = off[(size_t)g1] - i0;
    std::vector<uint32_t> cg;
    std::vector<int64_t> ca, cb, cptr((size_t)ng + 1, 0);
    for (int64_t g = g0; g < g1; ++g) {
      for (int64_t a = off[(size_t)g]; a < off[(size_t)g + 1]; a += FI_CHUNK) {
        cg.push_back((uint32_t)(g - g0));
        ca.push_back(a - i0);
        cb.push_back(std::min(a + FI_CHUNK, off[(size_t)g + 1]) - i0);
      }
      cptr[(size_t)(g - g0) + 1] = (int64_t)cg.size();
    }
    const size_t nc = cg.size();
    FMX_CHECK(nc < (1ull << 31), FMX_ERR_INVALID, "fold-in: too many row chunks");
    if ((size_t)cnt > capB) {
      FMX_TRY(dev_buf(&d_B, (size_t)cnt * sizeof(double)));
      FMX_TRY(dev_buf(&d_Z, (size_t)cnt * D * sizeof(double)));
      capB = (size_t)cnt;
    }
    if (nc > capC) {
      FMX_TRY(dev_buf(&d_cg, nc * sizeof(uint32_t)));
      FMX_TRY(dev_buf(&d_ca, nc * sizeof(int64_t)));
      FMX_TRY(dev_buf(&d_cb, nc * sizeof(int64_t)));
      capC = nc;
    }
    if (nc > capP) {
      FMX_TRY(dev_buf(&d_P, nc * (size_t)(ntri + D) * sizeof(double)));
      capP = nc;
    }
    if ((size_t)ng > capG) {
      FMX_TRY(dev_buf(&d_cptr, ((size_t)ng + 1) * sizeof(int64_t)));
      FMX_TRY(dev_buf(&d_theta, (size_t)ng * D * sizeof(double)));
      FMX_TRY(dev_buf(&d_status, (size_t)ng * sizeof(int)));
      capG = (size_t)ng;
    }
    if (nc) {
      FMX_HIP(hipMemcpy(d_cg.get(), cg.data(), nc * sizeof(uint32_t), hipMemcpyHostToDevice));   // (plain copies: an early return may drop the vectors before the stream is done)
      FMX_HIP(hipMemcpy(d_ca.get(), ca.data(), nc * sizeof(int64_t), hipMemcpyHostToDevice));
      FMX_HIP(hipMemcpy(d_cb.get(), cb.data(), nc * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    FMX_HIP(hipMemcpy(d_cptr.get(), cptr.data(), cptr.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    FMX_HIP(hipMemsetAsync(d_theta.get(), 0, (size_t)ng * D * sizeof(double), st));
    FMX_HIP(hipMemsetAsync(d_status.get(), 0, (size_t)ng * sizeof(int), st));

    if (cnt > 0) {
      FoldRowsArgs ra{};
      ra.row_ptr = m->row_ptr; ra.col = m->col; ra.val = m->val;
      ra.rows = (const int64_t*)d_rows_s.get(); ra.pos = (const uint32_t*)d_pos.get();
      ra.i0 = i0; ra.count = cnt;
      ra.scal = e->scal;
      ra.row_key = (const uint32_t*)d_key.get(); ra.n_ids = (uint32_t)n_ids;
      ra.k = k; ra.D = D; ra.k0 = e->hyper.k0; ra.k1 = e->hyper.k1; ra.unit = m->unit_values;
      ra.B = (double*)d_B.get(); ra.Z = (double*)d_Z.get();
      const bool wide = wide_state(e);
      if (wide) { ra.V = e->dV; ra.w = e->dw; ra.vs = e->kp64; ra.ws = 1; ra.lpr = e->kp64 / 2; }
      else { ra.V = e->V; ra.w = mb_wbase(e); ra.vs = e->vstride32; ra.ws = mb_wstride(e); ra.lpr = e->kp32 / 4; }
      FMX_CHECK(ra.lpr >= 1 && ra.lpr <= 64 && (ra.lpr & (ra.lpr - 1)) == 0, FMX_ERR_INVALID, "unsupported padded factor count");
      FMX_CHECK(!pairs || 2 * ra.lpr <= 64, FMX_ERR_INVALID, "unsupported padded factor count");   // a pair's two lane groups share a wave
      const int rpw = FI_THREADS / (pairs ? 2 * ra.lpr : ra.lpr);
      const int64_t grid = (cnt + rpw - 1) / rpw;
      FMX_CHECK(grid < (1LL << 31), FMX_ERR_INVALID, "fold-in: grid too large (%lld)", (long long)grid);
      if (pairs) {
        if (wide) hipLaunchKernelGGL(fold_pairs_k<double>, dim3((unsigned)grid), dim3(FI_THREADS), 0, st, ra);
        else hipLaunchKernelGGL(fold_pairs_k<float>, dim3((unsigned)grid), dim3(FI_THREADS), 0, st, ra);
      } else {
        if (wide) hipLaunchKernelGGL(fold_rows_k<double>, dim3((unsigned)grid), dim3(FI_THREADS), 0, st, ra);
        else hipLaunchKernelGGL(fold_rows_k<float>, dim3((unsigned)grid), dim3(FI_THREADS), 0, st, ra);
      }
      FMX_HIP(hipGetLastError());
    }
    for (int s = 0; s < steps; ++s) {
      if (nc) {
        FoldGramArgs ga{};
        ga.B = (const double*)d_B.get(); ga.Z = (const double*)d_Z.get();
        ga.rows = (const int64_t*)d_rows_s.get(); ga.i0 = i0; ga.y = pairs ? nullptr : m->y;
        ga.chunk_grp = (const uint32_t*)d_cg.get(); ga.chunk_a = (const int64_t*)d_ca.get(); ga.chunk_b = (const int64_t*)d_cb.get();
        ga.theta = (const double*)d_theta.get();
        ga.D = D; ga.DP = DP; ga.logistic = logistic ? 1 : 0; ga.dot = s > 0 ? 1 : 0;
        ga.P = (double*)d_P.get();
        hipLaunchKernelGGL(fold_gram_k, dim3((unsigned)nc), dim3(FI_THREADS), 0, st, ga);
        FMX_HIP(hipGetLastError());
      }
      FoldSolveArgs sa{};
      sa.P = (const double*)d_P.get(); sa.cptr = (const int64_t*)d_cptr.get();
      sa.theta = (double*)d_theta.get(); sa.status = (int*)d_status.get();
      sa.D = D; sa.k1 = e->hyper.k1; sa.lw = lw; sa.lv = lv;
      hipLaunchKernelGGL(fold_solve_k, dim3((unsigned)ng), dim3(FI_THREADS), 0, st, sa);
      FMX_HIP(hipGetLastError());
    }
    FMX_HIP(hipMemcpyAsync(theta_s.data() + (size_t)g0 * D, d_theta.get(), (size_t)ng * D * sizeof(double), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipMemcpyAsync(status_s.data() + (size_t)g0, d_status.get(), (size_t)ng * sizeof(int), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    g0 = g1;
  }

  theta_out->assign((size_t)n_ids * D, 0.0);
  rows_out->assign((size_t)n_ids, 0);
  status_out->assign((size_t)n_ids, 0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t g = 0; g < n_ids; ++g) {
    const size_t i = order[(size_t)g];
    (*rows_out)[i] = off[(size_t)g + 1] - off[(size_t)g];
    (*status_out)[i] = status_s[(size_t)g];
    for (int f = 0; f < D; ++f) (*theta_out)[i * D + f] = status_s[(size_t)g] ? nan : theta_s[(size_t)g * D + f];
  }
  return FMX_OK;
}

void debug_foldin_slab(int64_t rows, int64_t groups) {
  g_slab_rows_once.store(rows > 0 ? rows : 0);
  g_slab_groups_once.store(groups > 0 ? groups : 0);
}

}  // namespace fmx
