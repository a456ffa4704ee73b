// Diversified re-ranking (fmx_diversify): greedy maximal marginal relevance over the pools fmx_topk / fmx_topk_lists write; DESIGN.md section 20.
//
// A context row's pool is P slots (item index, score).  The call picks top_k of them, one per step: the slot with the largest
//   margin(u) = lambda * rel(u) - (1 - lambda) * pen(u),   pen(u) = the largest cosine of item u's projection with a slot picked before,
// under the total order of every ranking path (rank_before; ties by the lower item, then the lower slot).  include/fmx.h holds the contract to
// the bit, tests/diversify_model.py restates it in numpy.  Per call:
//   1. projection   s of the items once (topk_project_rows, with_w0 = false: fmx_project's values);
//   2. selection    one workgroup per context row, rows in chunks of at most 2^15.  Thread tid owns slots tid, tid + 256, ... (at most four) and
//                   keeps their relevance, inverse norm, running penalty and a live bit in registers.
//        LDS form     the pool's s rows are gathered once into a padded LDS tile (row_bytes / 16 lanes per row, 16 bytes each, four loads in
//                     flight per lane, as lists_fused_k gathers) and every chain reads LDS;
//        global form  a pool whose tile exceeds the budget leaves the rows where they are: every thread re-reads its own rows per step (they
//                     are L2-resident after the norms).
//      Per step: every thread forms the margins of its live slots and keeps its best; a __shfl_xor reduction under the order gives four wave
//      winners, which go through LDS so that every thread knows the selected slot; its row is copied to a small LDS buffer; every thread runs
//      the chain of each live row against it and updates the penalty.  Two barriers per step.
// Every value is a function of the row's own pool and the items: no atomics, nothing summed across threads (maxima and the order only), so the
// forms, the chunking and the calls agree in every bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "fm_rank.h"

namespace fmx {
namespace {

constexpr int DV_THREADS = 256;
constexpr int DV_WAVES = DV_THREADS / 64;
constexpr int DV_SLOTS = 4;                     // slots per thread: pools of at most DV_THREADS * DV_SLOTS
constexpr int DV_POOL = DV_THREADS * DV_SLOTS;  // 1024
constexpr int DV_TILE_BYTES = 56 << 10;         // the gather tile: with the static arrays a workgroup stays under 64 KiB, two or more per CU
constexpr int64_t DV_CHUNK = 1 << 15;           // context rows per launch
constexpr int64_t DV_PIECE = 1 << 22;           // slots per staged piece of the host form
constexpr unsigned long long DV_NONE = ~0ull;   // the key of "no slot left": after every real key

std::atomic<int> g_lds_rows{0};   // test hook (sticky): the longest pool the LDS form takes (< 0: none)
std::atomic<int64_t> g_chunk{0};  //                     and the context chunk

struct DivArgs {
  const void* is;        // items: s [ni][ks]
  int64_t ni;
  const int64_t* index;  // [nc][P]
  const double* score;   // [nc][P]
  int P, K, ks, relevance;
  double lambda, mu;
  int64_t* oi;           // [nc][K]
  double* os;            // [nc][K]
  double* om;            // [nc][K] or null
};

// fma(x[ks-1], y[ks-1], ... fma(x[0], y[0], 0)): one accumulator in T, f ascending over the zero-padded factors (ks is a multiple of four
// vectors) -- the chain of tk_pair_score without the bases
template <typename T>
__device__ __forceinline__ T dv_chain(const typename StateVec<T>::vec* __restrict__ x, const typename StateVec<T>::vec* __restrict__ y, int nv) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VN = StateVec<T>::N;
  T acc = (T)0;
  for (int b = 0; b < nv; b += 4) {
    const vec_t x0 = x[b], x1 = x[b + 1], x2 = x[b + 2], x3 = x[b + 3];
    const vec_t y0 = y[b], y1 = y[b + 1], y2 = y[b + 2], y3 = y[b + 3];
    const T *p0 = reinterpret_cast<const T*>(&x0), *p1 = reinterpret_cast<const T*>(&x1), *p2 = reinterpret_cast<const T*>(&x2),
            *p3 = reinterpret_cast<const T*>(&x3);
    const T *q0 = reinterpret_cast<const T*>(&y0), *q1 = reinterpret_cast<const T*>(&y1), *q2 = reinterpret_cast<const T*>(&y2),
            *q3 = reinterpret_cast<const T*>(&y3);
#pragma unroll
    for (int u = 0; u < VN; ++u) acc = fma(p0[u], q0[u], acc);
#pragma unroll
    for (int u = 0; u < VN; ++u) acc = fma(p1[u], q1[u], acc);
#pragma unroll
    for (int u = 0; u < VN; ++u) acc = fma(p2[u], q2[u], acc);
#pragma unroll
    for (int u = 0; u < VN; ++u) acc = fma(p3[u], q3[u], acc);
  }
  return acc;
}

template <typename T, bool LDS>
__global__ __launch_bounds__(DV_THREADS) void diversify_k(DivArgs a) {
  using vec_t = typename StateVec<T>::vec;
  extern __shared__ uint4 tile[];  // LDS form: P rows of ks * sizeof(T) + 16 bytes (the pad keeps the threads' 16-byte row reads on different banks)
  __shared__ uint4 sel[TK_KS_BYTES / 16];  // the selected row
  __shared__ int32_t sit[DV_POOL];         // the item of every slot, -1: empty
  __shared__ double wm[DV_WAVES];          // the wave winners: margin
  __shared__ unsigned long long wk[DV_WAVES];  //              item << 10 | slot
  __shared__ double whi[DV_WAVES], wlo[DV_WAVES];
  __shared__ double sinv;                  // the selected slot's inverse norm

  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  const int P = a.P, K = a.K, ks = a.ks;
  const int rb16 = ks * (int)sizeof(T) / 16;  // 16-byte pieces (= vectors) of a row
  const int stride16 = rb16 + 1;
  const int64_t* __restrict__ idx = a.index + c * P;
  const double* __restrict__ sc = a.score + c * P;
  const uint4* __restrict__ is16 = reinterpret_cast<const uint4*>(a.is);

  // 1, 5: the slots of this thread; an index outside [0, ni) is an empty slot and no row is read for it
  int item[DV_SLOTS];
  double rel[DV_SLOTS], inv[DV_SLOTS], pen[DV_SLOTS];
  unsigned live = 0;
  double hi = -__builtin_inf(), lo = __builtin_inf();
#pragma unroll
  for (int j = 0; j < DV_SLOTS; ++j) {
    const int slot = tid + j * DV_THREADS;
    item[j] = -1; rel[j] = 0.0; inv[j] = 0.0; pen[j] = 0.0;
    if (slot < P) {
      const int64_t ix = idx[slot];
      if (ix >= 0 && ix < a.ni) {
        item[j] = (int)ix;
        live |= 1u << j;
        const double s = sc[slot];
        rel[j] = s;
        hi = s > hi ? s : hi;
        lo = s < lo ? s : lo;
      }
      sit[slot] = item[j];
    }
  }
  if (a.relevance == FMX_DIV_REL_MINMAX) {
    for (int d = 32; d >= 1; d >>= 1) {
      const double oh = __shfl_xor(hi, d), ol = __shfl_xor(lo, d);
      hi = oh > hi ? oh : hi;
      lo = ol < lo ? ol : lo;
    }
    if ((tid & 63) == 0) { whi[tid >> 6] = hi; wlo[tid >> 6] = lo; }
    __syncthreads();
    hi = whi[0]; lo = wlo[0];
#pragma unroll
    for (int w = 1; w < DV_WAVES; ++w) {
      hi = whi[w] > hi ? whi[w] : hi;
      lo = wlo[w] < lo ? wlo[w] : lo;
    }
    hi = hi == 0.0 ? 0.0 : hi;  // a zero bound is +0 whichever zero the reduction met first
    lo = lo == 0.0 ? 0.0 : lo;
    const bool ok = hi - hi == 0.0 && lo - lo == 0.0 && hi > lo;  // both finite
    const double range = hi - lo;
#pragma unroll
    for (int j = 0; j < DV_SLOTS; ++j) {
      const double s = rel[j];
      rel[j] = ok ? (s - lo) / range : (s != s ? s : 0.0);
    }
  }
  __syncthreads();  // sit

  // the gather (LDS form): rb16 consecutive lanes per row, four loads in flight per lane; an empty slot's row is left unwritten and never read
  if (LDS && rb16 > 0) {
    const int pieces = P * rb16;
    for (int p0 = tid; p0 < pieces; p0 += 4 * DV_THREADS) {
      const int p1 = p0 + DV_THREADS < pieces ? p0 + DV_THREADS : p0, p2 = p0 + 2 * DV_THREADS < pieces ? p0 + 2 * DV_THREADS : p0,
                p3 = p0 + 3 * DV_THREADS < pieces ? p0 + 3 * DV_THREADS : p0;
      const int r0 = p0 / rb16, r1 = p1 / rb16, r2 = p2 / rb16, r3 = p3 / rb16;
      const int q0 = p0 - r0 * rb16, q1 = p1 - r1 * rb16, q2 = p2 - r2 * rb16, q3 = p3 - r3 * rb16;
      const int i0 = sit[r0], i1 = sit[r1], i2 = sit[r2], i3 = sit[r3];
      uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0, v2 = v0, v3 = v0;
      if (i0 >= 0) v0 = is16[(int64_t)i0 * rb16 + q0];
      if (i1 >= 0) v1 = is16[(int64_t)i1 * rb16 + q1];
      if (i2 >= 0) v2 = is16[(int64_t)i2 * rb16 + q2];
      if (i3 >= 0) v3 = is16[(int64_t)i3 * rb16 + q3];
      tile[r0 * stride16 + q0] = v0;
      if (p1 != p0) tile[r1 * stride16 + q1] = v1;
      if (p2 != p0) tile[r2 * stride16 + q2] = v2;
      if (p3 != p0) tile[r3 * stride16 + q3] = v3;
    }
    __syncthreads();
  }

  // 3: the norms, one chain per slot
#pragma unroll
  for (int j = 0; j < DV_SLOTS; ++j) {
    if (live & (1u << j)) {
      const vec_t* row = LDS ? reinterpret_cast<const vec_t*>(tile + (tid + j * DV_THREADS) * stride16)
                             : reinterpret_cast<const vec_t*>(is16 + (int64_t)item[j] * rb16);
      const double nrm = (double)dv_chain<T>(row, row, rb16);
      inv[j] = (nrm - nrm == 0.0 && nrm > 0.0) ? 1.0 / sqrt(nrm) : 0.0;
    }
  }

  // 7: the steps
  const double cnan = __builtin_nan("");
  int t = 0;
  for (; t < K; ++t) {
    double bm = cnan;
    unsigned long long bk = DV_NONE;
#pragma unroll
    for (int j = 0; j < DV_SLOTS; ++j) {
      if (live & (1u << j)) {
        const double x = a.lambda * rel[j], y = a.mu * pen[j];
        double m = x - y;
        m = m != m ? cnan : m;  // one NaN for every NaN margin
        const unsigned long long k = ((unsigned long long)(unsigned)item[j] << 10) | (unsigned)(tid + j * DV_THREADS);
        if (rank_before(m, k, bm, bk)) { bm = m; bk = k; }
      }
    }
    for (int d = 32; d >= 1; d >>= 1) {
      const double om = __shfl_xor(bm, d);
      const unsigned long long ok = __shfl_xor(bk, d);
      if (rank_before(om, ok, bm, bk)) { bm = om; bk = ok; }
    }
    if ((tid & 63) == 0) { wm[tid >> 6] = bm; wk[tid >> 6] = bk; }
    __syncthreads();
    bm = wm[0]; bk = wk[0];
#pragma unroll
    for (int w = 1; w < DV_WAVES; ++w) {
      const double om = wm[w];
      const unsigned long long ok = wk[w];
      if (rank_before(om, ok, bm, bk)) { bm = om; bk = ok; }
    }
    if (bk == DV_NONE) break;  // no slot left (the same for every thread)
    const int v = (int)(bk & 1023), iv = (int)(bk >> 10);
    if (tid == 0) {  // 8: the item, the given score's bits, the margin of this step
      a.oi[c * K + t] = iv;
      reinterpret_cast<long long*>(a.os)[c * K + t] = reinterpret_cast<const long long*>(sc)[v];
      if (a.om) a.om[c * K + t] = bm;
    }
    if (t + 1 == K) { ++t; break; }
    if (tid == (v & (DV_THREADS - 1))) {
      const int vj = v / DV_THREADS;
      double x = 0.0;
#pragma unroll
      for (int j = 0; j < DV_SLOTS; ++j) x = j == vj ? inv[j] : x;
      sinv = x;
      live &= ~(1u << vj);
    }
    if (tid < rb16) sel[tid] = LDS ? tile[(size_t)v * stride16 + tid] : is16[(int64_t)iv * rb16 + tid];
    __syncthreads();
    const double vinv = sinv;
#pragma unroll
    for (int j = 0; j < DV_SLOTS; ++j) {
      if (live & (1u << j)) {
        double sim = 0.0;
        if (inv[j] != 0.0 && vinv != 0.0) {
          const vec_t* row = LDS ? reinterpret_cast<const vec_t*>(tile + (tid + j * DV_THREADS) * stride16)
                                 : reinterpret_cast<const vec_t*>(is16 + (int64_t)item[j] * rb16);
          const double d = (double)dv_chain<T>(row, reinterpret_cast<const vec_t*>(sel), rb16);
          sim = (d * inv[j]) * vinv;
        }
        pen[j] = (t == 0 || sim > pen[j]) ? sim : pen[j];
      }
    }
  }
  // the slots beyond the number selected (t of them were)
  for (int s = t + tid; s < K; s += DV_THREADS) {
    a.oi[c * K + s] = -1;
    a.os[c * K + s] = cnan;
    if (a.om) a.om[c * K + s] = cnan;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side

template <typename T>
int diversify_run_t(fmx_engine* e, const fmx_matrix* I, int64_t n, int P, const int64_t* index, const double* score, int K, double lambda, int relevance,
                    int64_t* oi, double* os, double* om, bool host) {
  const hipStream_t st = e->stream;
  const int kp = wide_state(e) ? e->kp64 : e->kp32;
  const int ks = state_factors<T>(e);
  FMX_CHECK(ks * (int)sizeof(T) <= TK_KS_BYTES, FMX_ERR_INVALID, "diversification holds at most %d factors", TK_KS_BYTES / (int)sizeof(T));
  const int hook_rows = g_lds_rows.load();
  const int64_t hook_chunk = g_chunk.load();
  const int64_t chunk_max = hook_chunk > 0 ? std::min(hook_chunk, DV_CHUNK) : DV_CHUNK;
  const int64_t ni = I->n;
  const size_t tile_bytes = (size_t)P * (ks * sizeof(T) + 16);
  const bool lds = tile_bytes <= (size_t)DV_TILE_BYTES && (hook_rows == 0 || P <= hook_rows);

  Scratch S(st);
  double *q = nullptr, *ib = nullptr;
  T* is = nullptr;
  FMX_TRY(S.get(&q, (size_t)std::min<int64_t>(ni, 1 << 16) * kp));
  FMX_TRY(S.get(&is, (size_t)ni * ks));
  FMX_TRY(S.get(&ib, (size_t)ni));
  if (ni > 0) FMX_TRY(topk_project_rows(e, I, 0, ni, false, q, ks, ib, is));  // the items, once per call

  DivArgs a{};
  a.is = is; a.ni = ni; a.P = P; a.K = K; a.ks = ks; a.relevance = relevance; a.lambda = lambda; a.mu = 1.0 - lambda;
  // rows [r0, r0 + cnt) of device arrays, in chunks
  auto launch = [&](const int64_t* d_index, const double* d_score, int64_t* d_oi, double* d_os, double* d_om, int64_t cnt) -> int {
    for (int64_t r = 0; r < cnt; r += chunk_max) {
      const int64_t nc = std::min(chunk_max, cnt - r);
      DivArgs b = a;
      b.index = d_index + r * P; b.score = d_score + r * P;
      b.oi = d_oi + r * K; b.os = d_os + r * K; b.om = d_om ? d_om + r * K : nullptr;
      if (lds) hipLaunchKernelGGL((diversify_k<T, true>), dim3((unsigned)nc), dim3(DV_THREADS), tile_bytes, st, b);
      else hipLaunchKernelGGL((diversify_k<T, false>), dim3((unsigned)nc), dim3(DV_THREADS), 0, st, b);
      FMX_HIP(hipGetLastError());
    }
    return FMX_OK;
  };

  if (!host) {
    FMX_TRY(launch(index, score, oi, os, om, n));
    FMX_HIP(hipStreamSynchronize(st));
    return FMX_OK;
  }
  // the host form stages index / score / outputs in pieces of at most 2^22 slots
  const int64_t rows = std::min(std::max<int64_t>(1, DV_PIECE / P), n);
  int64_t *d_index = nullptr, *d_oi = nullptr;
  double *d_score = nullptr, *d_os = nullptr, *d_om = nullptr;
  FMX_TRY(S.get(&d_index, (size_t)rows * P)); FMX_TRY(S.get(&d_score, (size_t)rows * P));
  FMX_TRY(S.get(&d_oi, (size_t)rows * K)); FMX_TRY(S.get(&d_os, (size_t)rows * K));
  if (om) FMX_TRY(S.get(&d_om, (size_t)rows * K));
  for (int64_t r = 0; r < n; r += rows) {
    const int64_t cnt = std::min(rows, n - r);
    FMX_HIP(hipMemcpyAsync(d_index, index + r * P, (size_t)cnt * P * sizeof(int64_t), hipMemcpyHostToDevice, st));
    FMX_HIP(hipMemcpyAsync(d_score, score + r * P, (size_t)cnt * P * sizeof(double), hipMemcpyHostToDevice, st));
    FMX_TRY(launch(d_index, d_score, d_oi, d_os, d_om, cnt));
    FMX_HIP(hipMemcpyAsync(oi + r * K, d_oi, (size_t)cnt * K * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipMemcpyAsync(os + r * K, d_os, (size_t)cnt * K * sizeof(double), hipMemcpyDeviceToHost, st));
    if (om) FMX_HIP(hipMemcpyAsync(om + r * K, d_om, (size_t)cnt * K * sizeof(double), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
  }
  return FMX_OK;
}

}  // namespace

int diversify_run(fmx_engine* e, const fmx_matrix* I, int64_t n, int P, const int64_t* index, const double* score, int K, double lambda, int relevance,
                  int64_t* oi, double* os, double* om, bool host) {
  if (n <= 0) return FMX_OK;
  return wide_state(e) ? diversify_run_t<double>(e, I, n, P, index, score, K, lambda, relevance, oi, os, om, host)
                       : diversify_run_t<float>(e, I, n, P, index, score, K, lambda, relevance, oi, os, om, host);
}

void debug_diversify_limits(int lds_rows, int64_t chunk) {
  g_lds_rows.store(lds_rows);
  g_chunk.store(chunk > 0 ? chunk : 0);
}

}  // namespace fmx
