// Top-K items per context row under the FM score of the concatenated row c (+) i (fmx_topk).
//
// With s_c = sum_{j in c} x_j v_j (the factor sums the forward forms) the degree-2 FM of c (+) i is exactly
//     y(c (+) i) = y(c) + (y(i) - w0) + <s_c, s_i>
// so ranking every item for every context is two projections (the forward's own row walk, fm_rows_forward_k, with its fp64
// factor sums written out) and a dense [contexts x k] . [k x items] product fused with a per-context selection:
//   1. projection   base (f64) and s (the state type, zero-padded to KS factors) of every item row, then of each chunk of contexts;
//   2. score+select a grid of (context tile x item slice) workgroups.  A workgroup keeps its tile's s in LDS (read as broadcasts),
//                   every thread scores one item of the slice at a time against every context of the tile (a fixed-order fma chain
//                   over f = 0..KS-1), and each context keeps a running threshold -- its K-th best entry so far -- and an LDS buffer of
//                   the candidates that beat it.  A full buffer is sorted together with the current top K (bitonic, the whole
//                   workgroup) and cut back to K, which raises the threshold.  The exclusion list is searched only for candidates that
//                   beat the threshold;
//   3. merge        per context, the slices' lists through the same buffer, then the link on the K survivors.
// The selection state (TkSel, tk_*), the merge kernel and the buffer sizes live in fm_rank.h: fm_neighbors.hip runs the same selection.
// The order is strict and total (a higher score first, on equal scores the lower item index, NaN below every number), so the top-K
// set is unique: neither the tiling, the slice count, the chunking nor the order of the LDS appends can change a result, and a pair's
// score is the same arithmetic wherever it is formed.
#include <algorithm>
#include <cmath>
#include <memory>

#include "fm_rank.h"

namespace fmx {
namespace {

constexpr int64_t TK_PROJ_ROWS = 1 << 16;  // rows per projection slab (bounds the fp64 factor-sum scratch)
constexpr int64_t TK_PARTIAL_MAX = 1 << 24;  // entries of the per-slice lists of one context chunk (12 bytes each)

// fp64 factor sums [n][kp] -> s [n][ks] in the state type: factors 0..k-1, zeros above
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void topk_pack_k(const double* __restrict__ q, int64_t n, int kp, int k, int ks, T* __restrict__ s) {
  const int64_t t = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (t >= n * ks) return;
  const int64_t r = t / ks;
  const int f = (int)(t % ks);
  s[t] = f < k ? (T)q[r * kp + f] : (T)0;
}

// one workgroup per row of the chunk: copy its exclusion ids into xs (same offsets, relative to base) sorted in segments of TK_SEG
__global__ __launch_bounds__(TK_THREADS) void topk_sort_excl_k(const int64_t* __restrict__ rp, const uint32_t* __restrict__ col, int64_t base,
                                                             uint32_t* __restrict__ xs) {
  __shared__ uint32_t buf[TK_SEG];
  const int64_t a = rp[blockIdx.x], b = rp[blockIdx.x + 1];
  for (int64_t s0 = a; s0 < b; s0 += TK_SEG) {
    const int n = (int)(b - s0 < TK_SEG ? b - s0 : TK_SEG);
    int m = 1;
    while (m < n) m <<= 1;
    for (int t = threadIdx.x; t < m; t += TK_THREADS) buf[t] = t < n ? col[s0 + t] : 0xFFFFFFFFu;
    __syncthreads();
    for (int size = 2; size <= m; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = threadIdx.x; t < m / 2; t += TK_THREADS) {
          const int x = 2 * t - (t & (stride - 1)), y = x + stride;
          const uint32_t u = buf[x], v = buf[y];
          if (((x & size) == 0) == (u > v)) { buf[x] = v; buf[y] = u; }
        }
        __syncthreads();
      }
    }
    for (int t = threadIdx.x; t < n; t += TK_THREADS) xs[s0 - base + t] = buf[t];
    __syncthreads();
  }
}

struct TopkArgs {
  const void* cs;         // contexts of the chunk: s [nc][ks]
  const double* cb;       //                        base [nc] (w0 included)
  const void* is;         // items: s [ni][ks]
  const double* ib;       //        base [ni] (no w0)
  int64_t nc, ni;
  int ks, K;
  int64_t slice;          // items per slice (a multiple of TK_THREADS)
  int S;                  // slices
  const int64_t* xrp;     // exclusion row offsets of the chunk's contexts [nc + 1] (absolute), or null
  int64_t xbase;          // xrp[0]: xs[e - xbase] holds entry e
  const uint32_t* xs;     // the chunk's exclusion ids, sorted by segment
  double* ps;             // per-slice lists [nc][S][K]
  int32_t* pi;
};

template <typename T, int CT, int L>
__global__ __launch_bounds__(TK_THREADS) void topk_score_k(TopkArgs a) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VN = StateVec<T>::N;
  constexpr int FB = 4 * VN;  // factors per block: four 16-byte loads of an item row in flight
  constexpr int KSM = TK_KS_BYTES / sizeof(T);
  __shared__ TkSel<CT, L> q;
  __shared__ T sc[CT][KSM];
  __shared__ double bc[CT];
  __shared__ int64_t xa[CT], xb[CT];

  const int K = a.K, ks = a.ks;
  const int64_t c0 = (int64_t)blockIdx.x * CT;
  const int nv = (int)(a.nc - c0 < CT ? a.nc - c0 : CT);  // contexts of this tile
  const int64_t j0 = (int64_t)blockIdx.y * a.slice;
  const int64_t j1 = j0 + a.slice < a.ni ? j0 + a.slice : a.ni;
  const T* __restrict__ cs = reinterpret_cast<const T*>(a.cs);
  const T* __restrict__ is = reinterpret_cast<const T*>(a.is);

  tk_init<CT, L>(q);
  for (int t = threadIdx.x; t < CT * ks; t += TK_THREADS) {
    const int c = t / ks, f = t % ks;
    sc[c][f] = c < nv ? cs[(c0 + c) * ks + f] : (T)0;
  }
  if (threadIdx.x < CT) {
    const int c = threadIdx.x;
    bc[c] = c < nv ? a.cb[c0 + c] : 0.0;
    xa[c] = (a.xrp && c < nv) ? a.xrp[c0 + c] - a.xbase : 0;
    xb[c] = (a.xrp && c < nv) ? a.xrp[c0 + c + 1] - a.xbase : 0;
  }
  __syncthreads();

  double ts[CT];
  int32_t ti[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) { ts[c] = __builtin_nan(""); ti[c] = TK_NONE; }

  for (int64_t jb = j0; jb < j1; jb += TK_THREADS) {
    const int64_t j = jb + threadIdx.x;
    if (j < j1) {
      T acc[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = (T)0;
      const vec_t* row = reinterpret_cast<const vec_t*>(is + j * ks);
      for (int f0 = 0; f0 < ks; f0 += FB) {
        vec_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = row[f0 / VN + u];
        const T* si = reinterpret_cast<const T*>(v);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
#pragma unroll
          for (int f = 0; f < FB; ++f) acc[c] = fma(sc[c][f0 + f], si[f], acc[c]);  // f ascending: one chain per pair
        }
      }
      const double bi = a.ib[j];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (c < nv) {
          const double s = (bc[c] + bi) + (double)acc[c];
          if (rank_before(s, (int32_t)j, ts[c], ti[c]) && !(xa[c] < xb[c] && tk_excluded(a.xs, xa[c], xb[c], (uint32_t)j)))
            tk_offer<CT, L>(q, K, c, s, (int32_t)j);
        }
      }
    }
    tk_round<CT, L>(q, K);
#pragma unroll
    for (int c = 0; c < CT; ++c) { ts[c] = q.s[c][K - 1]; ti[c] = q.i[c][K - 1]; }
  }
  tk_flush<CT, L>(q, K);
  for (int t = threadIdx.x; t < nv * K; t += TK_THREADS) {
    const int c = t / K, r = t % K;
    const size_t o = ((size_t)(c0 + c) * a.S + blockIdx.y) * K + r;
    a.ps[o] = q.s[c][r];
    a.pi[o] = q.i[c][r];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side

// base and s of rows [r0, r1) of m through the forward's row walk: base = y_hat (with w0 only if with_w0), s = the fp64 factor sums in T
template <typename T>
int topk_project(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, bool with_w0, double* q, int ks, double* base, T* s) {
  const bool wide = wide_state(e);
  const int kp = wide ? e->kp64 : e->kp32;
  RowsArgs a{};
  a.row_ptr = m->row_ptr; a.col = m->col; a.val = m->val; a.y = nullptr;
  if (wide) { a.V = e->dV; a.w = e->dw; a.vs = e->kp64; a.ws = 1; }
  else { a.V = e->V; a.w = mb_wbase(e); a.vs = e->vstride32; a.ws = mb_wstride(e); }
  a.scal = e->scal;
  a.link = FMX_LINK_NONE;
  a.unit = m->unit_values;
  a.sort_rows = rows_ragged(m);
  a.flat = rows_flat(m); a.nmat = m->n;
  a.fixed_schedule = 1;
  for (int64_t off = r0; off < r1; off += TK_PROJ_ROWS) {
    const int64_t n = r1 - off < TK_PROJ_ROWS ? r1 - off : TK_PROJ_ROWS;
    a.r0 = off; a.nrows = n;
    a.yhat = base + (off - r0);
    a.qout = q;
    const Hyper keep = e->hyper;
    if (!with_w0) e->hyper.k0 = 0;  // the kernels take the Hyper by value at launch
    const int st = launch_rows_forward(e, a, false, wide);
    e->hyper = keep;
    FMX_TRY(st);
    const int64_t cnt = n * ks;
    if (cnt > 0) {
      hipLaunchKernelGGL((topk_pack_k<T>), dim3((unsigned)((cnt + TK_THREADS - 1) / TK_THREADS)), dim3(TK_THREADS), 0, e->stream, q, n, kp, e->k, ks,
                         s + (off - r0) * ks);
      FMX_HIP(hipGetLastError());
    }
  }
  return FMX_OK;
}

template <typename T, int CT, int L>
int topk_launch(fmx_engine* e, const TopkArgs& a, int link, int64_t* oi, double* os) {
  dim3 g((unsigned)((a.nc + CT - 1) / CT), (unsigned)a.S);
  hipLaunchKernelGGL((topk_score_k<T, CT, L>), g, dim3(TK_THREADS), 0, e->stream, a);
  FMX_HIP(hipGetLastError());
  hipLaunchKernelGGL((topk_merge_k<L>), dim3((unsigned)a.nc), dim3(TK_THREADS), 0, e->stream, a.ps, a.pi, a.S, a.K, e->hyper, link,
                     (const double*)e->probit, oi, os);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

template <typename T>
int topk_dispatch(fmx_engine* e, const TopkArgs& a, int link, int64_t* oi, double* os) {
  switch (topk_slots(a.K)) {
    case 512: return topk_launch<T, 8, 512>(e, a, link, oi, os);
    case 1024: return topk_launch<T, 4, 1024>(e, a, link, oi, os);
    default: return topk_launch<T, 2, 2048>(e, a, link, oi, os);
  }
}

template <typename T>
int topk_run_t(fmx_engine* e, const fmx_matrix* C, int64_t r0, int64_t r1, const fmx_matrix* I, const fmx_matrix* X, int K, int link, int64_t* oi,
               double* os) {
  const int kp = wide_state(e) ? e->kp64 : e->kp32;
  const int ks = state_factors<T>(e);
  FMX_CHECK(ks * (int)sizeof(T) <= TK_KS_BYTES, FMX_ERR_INVALID, "top-K scoring holds at most %d factors", TK_KS_BYTES / (int)sizeof(T));
  const int64_t ni = I->n;
  const int L = topk_slots(K), CT = topk_tile(L);

  // slices (rank_slices), and the chunk of contexts whose per-slice lists fit TK_PARTIAL_MAX
  int64_t chunk = std::min<int64_t>(r1 - r0, 1 << 15);
  int64_t S, slice;
  rank_slices(ni, (chunk + CT - 1) / CT, device_cus(e->cfg.device), TK_THREADS, &slice, &S);
  chunk = std::max<int64_t>(CT, std::min<int64_t>(chunk, TK_PARTIAL_MAX / (S * K) / CT * CT));

  Scratch scratch(e->stream);
  Projections<T> pr;
  FMX_TRY(pr.reserve(scratch, ni, chunk, kp, ks));
  FMX_TRY(topk_project<T>(e, I, 0, ni, false, pr.q, ks, pr.ib, pr.is));  // the items, once per call
  double* ps = nullptr;
  int32_t* pi = nullptr;
  FMX_TRY(scratch.get(&ps, (size_t)chunk * S * K));
  FMX_TRY(scratch.get(&pi, (size_t)chunk * S * K));
  DevBuf xs;  // grows with the chunks' exclusion lists
  size_t xs_cap = 0;
  for (int64_t c = r0; c < r1; c += chunk) {
    const int64_t nc = std::min(chunk, r1 - c);
    FMX_TRY(topk_project<T>(e, C, c, c + nc, true, pr.q, ks, pr.cb, pr.cs));
    TopkArgs a{};
    a.cs = pr.cs; a.cb = pr.cb; a.is = pr.is; a.ib = pr.ib;
    a.nc = nc; a.ni = ni; a.ks = ks; a.K = K; a.slice = slice; a.S = (int)S;
    a.ps = ps; a.pi = pi;
    if (X) {
      int64_t xr[2];
      FMX_HIP(hipMemcpyAsync(&xr[0], X->row_ptr + c, sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
      FMX_HIP(hipMemcpyAsync(&xr[1], X->row_ptr + c + nc, sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
      FMX_HIP(hipStreamSynchronize(e->stream));
      const size_t nx = (size_t)(xr[1] - xr[0]);
      if (nx > 0) {
        if (nx > xs_cap) {
          FMX_HIP(hipStreamSynchronize(e->stream));  // the previous chunk's kernels may still read the old list
          FMX_TRY(dev_buf(&xs, nx * sizeof(uint32_t)));
          xs_cap = nx;
        }
        hipLaunchKernelGGL(topk_sort_excl_k, dim3((unsigned)nc), dim3(TK_THREADS), 0, e->stream, X->row_ptr + c, X->col, xr[0], (uint32_t*)xs.get());
        FMX_HIP(hipGetLastError());
        a.xrp = X->row_ptr + c; a.xbase = xr[0]; a.xs = (const uint32_t*)xs.get();
      }
    }
    FMX_TRY(topk_dispatch<T>(e, a, link, oi + (c - r0) * K, os + (c - r0) * K));
  }
  FMX_HIP(hipStreamSynchronize(e->stream));  // the exclusion list is freed on return
  return FMX_OK;
}

}  // namespace

int topk_project_rows(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, bool with_w0, double* q, int ks, double* base, void* s) {
  return wide_state(e) ? topk_project<double>(e, m, r0, r1, with_w0, q, ks, base, (double*)s) : topk_project<float>(e, m, r0, r1, with_w0, q, ks, base, (float*)s);
}

int topk_sort_excl(hipStream_t st, const int64_t* rp, int64_t nrows, const uint32_t* col, int64_t base, uint32_t* xs) {
  if (nrows <= 0) return FMX_OK;
  hipLaunchKernelGGL(topk_sort_excl_k, dim3((unsigned)nrows), dim3(TK_THREADS), 0, st, rp, col, base, xs);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

int topk_run(fmx_engine* e, const fmx_matrix* C, int64_t r0, int64_t r1, const fmx_matrix* I, const fmx_matrix* X, int K, int link, int64_t* d_index,
             double* d_score) {
  if (r1 <= r0) return FMX_OK;
  if (link == FMX_LINK_PROBIT) FMX_TRY(ensure_probit(e));
  if (I->n == 0) {  // nothing to rank: every slot is padding
    std::vector<int64_t> ni((size_t)(r1 - r0) * K, -1);
    std::vector<double> ns((size_t)(r1 - r0) * K, std::nan(""));
    FMX_HIP(hipMemcpy(d_index, ni.data(), ni.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    FMX_HIP(hipMemcpy(d_score, ns.data(), ns.size() * sizeof(double), hipMemcpyHostToDevice));
    return FMX_OK;
  }
  return wide_state(e) ? topk_run_t<double>(e, C, r0, r1, I, X, K, link, d_index, d_score)
                       : topk_run_t<float>(e, C, r0, r1, I, X, K, link, d_index, d_score);
}

}  // namespace fmx
