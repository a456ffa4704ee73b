// Exact per-entry prediction contributions (fmx_contrib*) and their per-feature summary (fmx_contrib_summary).
//
// For one row with stored entries e (column c(e), value x_e) and factor sums s = sum_e x_e v_c(e), the Shapley value of entry e for the
// raw score, the empty row as baseline, is
//     phi_e = keep_w1 x_e w_c(e) + 1/2 sum_f t_ef (s_f - t_ef),   t_ef = v_c(e),f x_e
// (every pair term x_e x_e' <v_c(e), v_c(e')> is split equally between its two entries), so keep_w0 w0 + sum_e phi_e = y_hat.
//
// fm_contrib_k walks a row twice with the lane-group layout of the forward (fm_rows_forward_k: LPR lanes per row, a 16-byte slice of the
// factor row per lane, the workgroup's entries staged through LDS):
//   walk 1  s_f += t_ef in entry order, fp64 registers -- the forward's own sums, bit for bit;
//   walk 2  per entry the slice's part of sum_f t_ef (s_f - t_ef), a fixed butterfly over the lane group, phi_e into the entry's LDS
//           slot; the chunk's phi then goes out as one coalesced store.
// Walk 2 gathers the V rows walk 1 has just fetched, so it reads them from L2 / MALL.  Every launch is 256-thread workgroups with one
// lane group per row: a row's bits are a function of the row alone (never of the launch's row count, range or chunking).
//
// The summary cuts the matrix into row chunks of at most CB_SUMMARY_ENTRIES entries; per chunk: phi (fm_contrib_k), a stable radix sort of
// (column, phi), a deterministic reduce-by-key, and a plain kernel adding the chunk's partials into the p-long accumulators (keys are
// unique within a chunk: no atomics).  Chunks are added in order, so a matrix and an engine give the same bits every call.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "fm_rank.h"

namespace fmx {
namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_CHUNK = 2048;  // entries staged in LDS at a time (16 KiB); walk 2 overwrites each slot with its entry's phi
constexpr int CB_RU = 4;        // entries whose gathers are in flight together, per lane group
constexpr int64_t CB_SUMMARY_ENTRIES = 1 << 22;  // entries per summary chunk (about 150 MB of scratch)

std::atomic<int64_t> g_summary_chunk_once{0};  // test hook: the next summary's chunk size

__device__ __forceinline__ void cb_get(const float4& v, double* o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
__device__ __forceinline__ void cb_get(const double2& v, double* o) { o[0] = v.x; o[1] = v.y; }

struct ContribArgs {
  const int64_t* row_ptr;
  const uint32_t* col;
  const float* val;
  int64_t r0;        // first row of the launch
  int64_t nrows;
  const void* V;     // feature j's factors at V[j * vs], kp of them (zero-padded)
  const void* w;     // feature j's linear weight at w[j * ws]
  int64_t vs, ws;
  int k1;            // keep_w1
  int unit;          // every value is 1.0f: val is not read
  double* out;       // phi of entry t at out[t - row_ptr[r0]]
};

// (id, x) of `cnt` entries from absolute offset c0 into LDS; all loads before the first store
__device__ __forceinline__ void cb_stage(uint2* stage, const uint32_t* __restrict__ ids, const float* __restrict__ xs, int64_t c0, int cnt, int unit) {
  constexpr int PER = CB_CHUNK / CB_THREADS;
  uint32_t id[PER], xb[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int i = threadIdx.x + u * CB_THREADS;
    const bool in = i < cnt;
    id[u] = in ? ids[c0 + i] : 0u;
    xb[u] = unit ? 0x3f800000u : (in ? __float_as_uint(xs[c0 + i]) : 0u);
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int i = threadIdx.x + u * CB_THREADS;
    if (i < cnt) stage[i] = make_uint2(id[u], xb[u]);
  }
}

template <typename T, int LPR>
__global__ __launch_bounds__(CB_THREADS) void fm_contrib_k(ContribArgs a) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VEC = StateVec<T>::N;
  constexpr int RPW = CB_THREADS / LPR;
  // (id, x) of the staged entries; walk 2 replaces a slot by its entry's phi (8 bytes either way) once the lane group has read it.  A lane
  // group only ever reads and writes its own row's slots, so the chunk's phi leaves as one coalesced store without a second array
  // (32 KiB of LDS would cost a wave per SIMD).
  __shared__ uint2 stage[CB_CHUNK];

  const int tid = threadIdx.x;
  const int gid = tid / LPR;
  const int lig = tid % LPR;
  const int64_t R0 = (int64_t)blockIdx.x * RPW;
  const int64_t R1 = (R0 + RPW < a.nrows) ? R0 + RPW : a.nrows;
  const int64_t lo = a.row_ptr[a.r0 + R0];
  const int64_t hi = a.row_ptr[a.r0 + R1];
  const int64_t obase = a.row_ptr[a.r0];
  const int64_t row = R0 + gid;
  int64_t ta = 0, tb = 0;
  if (row < a.nrows) {
    ta = a.row_ptr[a.r0 + row];
    tb = a.row_ptr[a.r0 + row + 1];
  }
  const T* __restrict__ Vt = reinterpret_cast<const T*>(a.V) + lig * VEC;
  const T* __restrict__ wt = reinterpret_cast<const T*>(a.w ? a.w : a.V);  // always readable
  const bool k1 = a.k1 != 0;
  const bool one = hi - lo <= CB_CHUNK;  // the workgroup's entries fit one stage: walk 2 reuses it

  double s[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) s[i] = 0.0;

  for (int pass = 0; pass < 2; ++pass) {
    for (int64_t c0 = lo; c0 < hi; c0 += CB_CHUNK) {
      const int cnt = (hi - c0 < CB_CHUNK) ? (int)(hi - c0) : CB_CHUNK;
      if (pass == 0 || !one) {  // uniform over the workgroup
        cb_stage(stage, a.col, a.val, c0, cnt, a.unit);
        __syncthreads();
      }
      const int64_t b = ta > c0 ? ta : c0;
      const int64_t e = tb < c0 + cnt ? tb : c0 + cnt;
      for (int64_t t = b; t < e; t += CB_RU) {
        const int o = (int)(t - c0);
        const int last = (int)(e - 1 - c0);
        // straight-line as in the forward: every LDS read, then every gather, then the arithmetic; slots past the row's end repeat
        // entry 0's row with x = +0.0 (computed, never stored)
        uint2 en[CB_RU];
#pragma unroll
        for (int u = 0; u < CB_RU; ++u) en[u] = stage[o + u < last ? o + u : last];
#pragma unroll
        for (int u = 1; u < CB_RU; ++u)
          if (t + u >= e) en[u] = make_uint2(en[0].x, 0u);
        vec_t vv[CB_RU];
        T wv[CB_RU];
#pragma unroll
        for (int u = 0; u < CB_RU; ++u) {
          vv[u] = *reinterpret_cast<const vec_t*>(Vt + (size_t)en[u].x * a.vs);
          if (pass == 1) wv[u] = wt[(size_t)en[u].x * a.ws];
        }
#pragma unroll
        for (int u = 0; u < CB_RU; ++u) {
          const double x = (double)__uint_as_float(en[u].y);
          double vf[VEC];
          cb_get(vv[u], vf);
          if (pass == 0) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) s[i] += vf[i] * x;  // the forward's product and order (fm_rows_forward_k)
          } else {
            double part = 0.0;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
              const double tmp = vf[i] * x;
              part += tmp * (s[i] - tmp);
            }
#pragma unroll
            for (int off = LPR / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);  // commutative steps: every lane holds the same bits
            const double lin = k1 ? (double)wv[u] * x : 0.0;
            if (lig == 0 && t + u < e) reinterpret_cast<double*>(stage)[o + u] = lin + 0.5 * part;
          }
        }
      }
      if (pass == 1) {
        __syncthreads();
        for (int i = tid; i < cnt; i += CB_THREADS) a.out[c0 - obase + i] = reinterpret_cast<const double*>(stage)[i];
      }
      __syncthreads();
    }
  }
}

template <typename T>
int contrib_launch(fmx_engine* e, const ContribArgs& a, int kp) {
  const int lpr = kp / StateVec<T>::N;
  const int rpw = CB_THREADS / lpr;
  const int64_t grid = (a.nrows + rpw - 1) / rpw;
  if (grid == 0) return FMX_OK;
  FMX_CHECK(grid < (1LL << 31), FMX_ERR_INVALID, "contributions: grid too large (%lld)", (long long)grid);
#define FMX_CB_CASE(L) case L: hipLaunchKernelGGL((fm_contrib_k<T, L>), dim3((unsigned)grid), dim3(CB_THREADS), 0, e->stream, a); break;
  switch (lpr) {
    FMX_CB_CASE(1) FMX_CB_CASE(2) FMX_CB_CASE(4) FMX_CB_CASE(8) FMX_CB_CASE(16) FMX_CB_CASE(32) FMX_CB_CASE(64)
    default: FMX_CHECK(false, FMX_ERR_INVALID, "unsupported padded factor count %d", kp);
  }
#undef FMX_CB_CASE
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- summary

struct CbAcc {
  double s, a;
  long long c;
};
struct CbLift {
  __device__ CbAcc operator()(double v) const { return CbAcc{v, fabs(v), 1}; }
};
struct CbPlus {
  __device__ CbAcc operator()(const CbAcc& x, const CbAcc& y) const { return CbAcc{x.s + y.s, x.a + y.a, x.c + y.c}; }
};

// the chunk's per-feature partials into the accumulators, in the chunk's order; keys are unique inside a chunk
__global__ __launch_bounds__(CB_THREADS) void contrib_accum_k(const uint32_t* __restrict__ keys, const CbAcc* __restrict__ agg, const int64_t* __restrict__ n_unique,
                                                             double* __restrict__ sum, double* __restrict__ abs_sum, int64_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x;
  if (i >= *n_unique) return;
  const uint32_t j = keys[i];
  const CbAcc v = agg[i];
  sum[j] += v.s;
  abs_sum[j] += v.a;
  count[j] += v.c;
}

}  // namespace

int contrib_run(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, double* d_out) {
  if (r1 <= r0) return FMX_OK;
  ContribArgs a{};
  a.row_ptr = m->row_ptr; a.col = m->col; a.val = m->val;
  a.r0 = r0; a.nrows = r1 - r0;
  a.k1 = e->hyper.k1;
  a.unit = m->unit_values;
  a.out = d_out;
  if (wide_state(e)) {
    a.V = e->dV; a.w = e->dw; a.vs = e->kp64; a.ws = 1;
    return contrib_launch<double>(e, a, e->kp64);
  }
  a.V = e->V; a.w = mb_wbase(e); a.vs = e->vstride32; a.ws = mb_wstride(e);
  return contrib_launch<float>(e, a, e->kp32);
}

int contrib_summary_run(fmx_engine* e, const fmx_matrix* m, double* sum, double* abs_sum, int64_t* count) {
  const size_t p = m->p;
  int64_t cap = g_summary_chunk_once.exchange(0);
  if (cap <= 0) cap = CB_SUMMARY_ENTRIES;
  // row chunks of at most `cap` entries (a longer row is a chunk of its own), cut on the host's copy of row_ptr
  std::vector<int64_t> rp((size_t)m->n + 1);
  FMX_HIP(hipMemcpy(rp.data(), m->row_ptr, rp.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<int64_t> cuts{0};
  int64_t most = 0;
  while (cuts.back() < m->n) {
    const int64_t c = cuts.back();
    int64_t r = std::upper_bound(rp.begin() + c + 1, rp.end(), rp[(size_t)c] + cap) - rp.begin() - 1;
    if (r <= c) r = c + 1;
    most = std::max(most, rp[(size_t)r] - rp[(size_t)c]);
    cuts.push_back(r);
  }
  int end_bit = 0;
  while (end_bit < 32 && (p - 1) >> end_bit) ++end_bit;
  if (end_bit == 0) end_bit = 1;

  DevBuf acc, phi, phi_s, key_s, uniq, agg, nu, tmp;
  FMX_TRY(dev_buf(&acc, p * (2 * sizeof(double) + sizeof(int64_t))));
  double* d_sum = (double*)acc.get();
  double* d_abs = d_sum + p;
  int64_t* d_cnt = (int64_t*)(d_abs + p);
  FMX_HIP(hipMemsetAsync(d_sum, 0, p * (2 * sizeof(double) + sizeof(int64_t)), e->stream));
  const size_t nmax = (size_t)std::max<int64_t>(most, 1);
  FMX_TRY(dev_buf(&phi, nmax * sizeof(double)));
  FMX_TRY(dev_buf(&phi_s, nmax * sizeof(double)));
  FMX_TRY(dev_buf(&key_s, nmax * sizeof(uint32_t)));
  FMX_TRY(dev_buf(&uniq, nmax * sizeof(uint32_t)));
  FMX_TRY(dev_buf(&agg, nmax * sizeof(CbAcc)));
  FMX_TRY(dev_buf(&nu, sizeof(int64_t)));
  size_t tmp_cap = 0;
  for (size_t c = 0; c + 1 < cuts.size(); ++c) {
    const int64_t base = rp[(size_t)cuts[c]];
    const size_t ne = (size_t)(rp[(size_t)cuts[c + 1]] - base);
    if (ne == 0) continue;
    FMX_TRY(contrib_run(e, m, cuts[c], cuts[c + 1], (double*)phi.get()));
    const uint32_t* keys = m->col + base;
    double* ph = (double*)phi.get();
    double* ph_s = (double*)phi_s.get();
    uint32_t* ks = (uint32_t*)key_s.get();
    auto lifted = rocprim::make_transform_iterator(ph_s, CbLift());
    size_t t1 = 0, t2 = 0;
    FMX_HIP(rocprim::radix_sort_pairs(nullptr, t1, keys, ks, ph, ph_s, ne, 0, end_bit, e->stream));
    FMX_HIP(rocprim::deterministic_reduce_by_key(nullptr, t2, ks, lifted, ne, (uint32_t*)uniq.get(), (CbAcc*)agg.get(), (int64_t*)nu.get(), CbPlus(),
                                                 rocprim::equal_to<uint32_t>(), e->stream));
    const size_t need = std::max(t1, t2);
    if (need > tmp_cap) {
      FMX_HIP(hipStreamSynchronize(e->stream));  // an earlier chunk's kernels may still use the old scratch
      FMX_TRY(dev_buf(&tmp, need));
      tmp_cap = need;
    }
    FMX_HIP(rocprim::radix_sort_pairs(tmp.get(), t1, keys, ks, ph, ph_s, ne, 0, end_bit, e->stream));  // LSD: stable, entry order inside a column
    FMX_HIP(rocprim::deterministic_reduce_by_key(tmp.get(), t2, ks, lifted, ne, (uint32_t*)uniq.get(), (CbAcc*)agg.get(), (int64_t*)nu.get(), CbPlus(),
                                                 rocprim::equal_to<uint32_t>(), e->stream));
    const size_t grid = (std::min(ne, p) + CB_THREADS - 1) / CB_THREADS;
    hipLaunchKernelGGL(contrib_accum_k, dim3((unsigned)grid), dim3(CB_THREADS), 0, e->stream, (const uint32_t*)uniq.get(), (const CbAcc*)agg.get(),
                       (const int64_t*)nu.get(), d_sum, d_abs, d_cnt);
    FMX_HIP(hipGetLastError());
  }
  FMX_HIP(hipStreamSynchronize(e->stream));
  std::vector<double> hs(p), ha(p);
  std::vector<int64_t> hc(p);
  FMX_HIP(hipMemcpy(hs.data(), d_sum, p * sizeof(double), hipMemcpyDeviceToHost));
  FMX_HIP(hipMemcpy(ha.data(), d_abs, p * sizeof(double), hipMemcpyDeviceToHost));
  FMX_HIP(hipMemcpy(hc.data(), d_cnt, p * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::copy(hs.begin(), hs.end(), sum);  // the caller's arrays are written only once everything has succeeded
  std::copy(ha.begin(), ha.end(), abs_sum);
  if (count) std::copy(hc.begin(), hc.end(), count);
  return FMX_OK;
}

void debug_contrib_summary_chunk(int64_t entries) { g_summary_chunk_once.store(entries > 0 ? entries : 0); }

}  // namespace fmx
