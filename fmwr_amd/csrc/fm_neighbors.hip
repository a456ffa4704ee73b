// The K most similar item rows per query row by the cosine (or the dot product) of their factor projections (fmx_neighbors).
//
// With s_r = sum_{j in r} x_j v_j (fmx_project's values, with_w0 = 0) the similarity of query q and item i is
//     d(q, i) = the fma chain of fmx_topk's score without the bases,   cos(q, i) = (d(q, i) * inv(q)) * inv(i),   inv(r) = 1 / sqrt(d(r, r))
// -- fmx_diversify's steps 2-4 (fm_diversify.hip), on every (query, item) pair instead of inside one pool.  include/fmx.h holds the contract to
// the bit, tests/neighbors_model.py restates it in numpy.  Per call:
//   1. projection   s of the items once, of each chunk of queries (topk_project_rows, with_w0 = false); the bases it writes are not read;
//   2. norms        one thread per row: the chain d(r, r) in the state type, then inv in fp64 (FMX_SIM_COSINE only);
//   3. score+select a grid of (query tile x item slice) workgroups with the structure of topk_score_k: the tile's s and inv in LDS (read as
//                   broadcasts), every thread scores one item of the slice at a time against every query of the tile, and each query keeps a
//                   running threshold and an LDS buffer of the candidates that beat it (TkSel, fm_rank.h);
//   4. merge        topk_merge_k (fm_rank.h) with no link.
// The order is fmx_topk's, strict and total, so the top-K set is unique: neither the tiling, the slice count, the chunking nor the order of the
// LDS appends can change a result, and a pair's score is the same arithmetic wherever it is formed.  The dot product stays on the VALU: the
// contract is the fma chain.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "fm_rank.h"

namespace fmx {
namespace {

constexpr int64_t NB_PARTIAL_MAX = 1 << 24;  // entries of the per-slice lists of one query chunk (12 bytes each)
constexpr int64_t NB_SLICES_MAX = 65535;     // the grid's y extent

std::atomic<int64_t> g_slice{0};  // test hook (sticky): items per slice
std::atomic<int64_t> g_chunk{0};  //                     and query rows per chunk

// inv[r] = 1 / sqrt(d(r, r)) if the chain d(r, r) is finite and > 0, else 0 (fmx_diversify's step 3)
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void nb_norm_k(const T* __restrict__ s, int64_t n, int ks, double* __restrict__ inv) {
  const int64_t r = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (r >= n) return;
  using vec_t = typename StateVec<T>::vec;
  constexpr int VN = StateVec<T>::N;
  const vec_t* __restrict__ row = reinterpret_cast<const vec_t*>(s + r * ks);  // ks is whole blocks of four 16-byte vectors
  T acc = (T)0;
  for (int b = 0; b < ks / VN; ++b) {
    const vec_t v = row[b];
    const T* x = reinterpret_cast<const T*>(&v);
#pragma unroll
    for (int u = 0; u < VN; ++u) acc = fma(x[u], x[u], acc);  // f ascending
  }
  const double nrm = (double)acc;
  inv[r] = (nrm - nrm == 0.0 && nrm > 0.0) ? 1.0 / sqrt(nrm) : 0.0;
}

struct NbArgs {
  const void* qs;      // queries of the chunk: s [nq][ks]
  const double* qinv;  //                       inverse norms [nq] (cosine only)
  const void* is;      // items: s [ni][ks]
  const double* iinv;  //        inverse norms [ni] (cosine only)
  int64_t nq, ni;
  int64_t r0;          // the absolute row of the chunk's first query (skip_self)
  int ks, K, cosine, skip;
  int64_t slice;       // items per slice (a multiple of TK_THREADS)
  int S;               // slices
  double* ps;          // per-slice lists [nq][S][K]
  int32_t* pi;
};

template <typename T, int CT, int L>
__global__ __launch_bounds__(TK_THREADS) void nb_score_k(NbArgs a) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VN = StateVec<T>::N;
  constexpr int FB = 4 * VN;  // factors per block: four 16-byte loads of an item row in flight
  constexpr int KSM = TK_KS_BYTES / sizeof(T);
  __shared__ TkSel<CT, L> q;
  __shared__ T sq[CT][KSM];
  __shared__ double vq[CT];

  const int K = a.K, ks = a.ks;
  const bool cosine = a.cosine != 0;
  const int64_t q0 = (int64_t)blockIdx.x * CT;
  const int nv = (int)(a.nq - q0 < CT ? a.nq - q0 : CT);  // queries of this tile
  const int64_t j0 = (int64_t)blockIdx.y * a.slice;
  const int64_t j1 = j0 + a.slice < a.ni ? j0 + a.slice : a.ni;
  const int64_t self0 = a.skip ? a.r0 + q0 : -(int64_t)CT - 1;  // query c's own item row is self0 + c (never an item when not skipping)
  const T* __restrict__ qs = reinterpret_cast<const T*>(a.qs);
  const T* __restrict__ is = reinterpret_cast<const T*>(a.is);

  tk_init<CT, L>(q);
  for (int t = threadIdx.x; t < CT * ks; t += TK_THREADS) {
    const int c = t / ks, f = t % ks;
    sq[c][f] = c < nv ? qs[(q0 + c) * ks + f] : (T)0;
  }
  if (threadIdx.x < CT) {
    const int c = threadIdx.x;
    vq[c] = (cosine && c < nv) ? a.qinv[q0 + c] : 0.0;
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
          for (int f = 0; f < FB; ++f) acc[c] = fma(sq[c][f0 + f], si[f], acc[c]);  // f ascending: one chain per pair
        }
      }
      const double vi = cosine ? a.iinv[j] : 0.0;
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (c < nv) {
          const double d = (double)acc[c];
          const double vc = vq[c];
          const double s = !cosine ? d : (vc == 0.0 || vi == 0.0) ? 0.0 : (d * vc) * vi;  // the query's inverse norm first
          if (rank_before(s, (int32_t)j, ts[c], ti[c]) && j != self0 + c) tk_offer<CT, L>(q, K, c, s, (int32_t)j);
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
    const size_t o = ((size_t)(q0 + c) * a.S + blockIdx.y) * K + r;
    a.ps[o] = q.s[c][r];
    a.pi[o] = q.i[c][r];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side

template <typename T, int CT, int L>
int nb_launch(fmx_engine* e, const NbArgs& a, int64_t* oi, double* os) {
  dim3 g((unsigned)((a.nq + CT - 1) / CT), (unsigned)a.S);
  hipLaunchKernelGGL((nb_score_k<T, CT, L>), g, dim3(TK_THREADS), 0, e->stream, a);
  FMX_HIP(hipGetLastError());
  hipLaunchKernelGGL((topk_merge_k<L>), dim3((unsigned)a.nq), dim3(TK_THREADS), 0, e->stream, a.ps, a.pi, a.S, a.K, e->hyper, (int)FMX_LINK_NONE,
                     (const double*)nullptr, oi, os);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

template <typename T>
int nb_dispatch(fmx_engine* e, const NbArgs& a, int64_t* oi, double* os) {
  switch (topk_slots(a.K)) {
    case 512: return nb_launch<T, 8, 512>(e, a, oi, os);
    case 1024: return nb_launch<T, 4, 1024>(e, a, oi, os);
    default: return nb_launch<T, 2, 2048>(e, a, oi, os);
  }
}

template <typename T>
int nb_norms(fmx_engine* e, const T* s, int64_t n, int ks, double* inv) {
  if (n <= 0) return FMX_OK;
  hipLaunchKernelGGL((nb_norm_k<T>), dim3(blocks(n, TK_THREADS)), dim3(TK_THREADS), 0, e->stream, s, n, ks, inv);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

template <typename T>
int neighbors_run_t(fmx_engine* e, const fmx_matrix* Q, int64_t r0, int64_t r1, const fmx_matrix* I, int K, int metric, bool skip, int64_t* oi, double* os) {
  const int kp = wide_state(e) ? e->kp64 : e->kp32;
  const int ks = state_factors<T>(e);
  FMX_CHECK(ks * (int)sizeof(T) <= TK_KS_BYTES, FMX_ERR_INVALID, "top-K scoring holds at most %d factors", TK_KS_BYTES / (int)sizeof(T));
  const int64_t ni = I->n;
  const int L = topk_slots(K), CT = topk_tile(L);
  const bool cosine = metric == FMX_SIM_COSINE;
  const int64_t hook_slice = g_slice.load(), hook_chunk = g_chunk.load();

  // slices (rank_slices, or the hook's), and the chunk of queries whose per-slice lists fit NB_PARTIAL_MAX
  int64_t chunk = std::min<int64_t>(r1 - r0, 1 << 15);
  int64_t S, slice;
  rank_slices(ni, (chunk + CT - 1) / CT, device_cus(e->cfg.device), TK_THREADS, &slice, &S);
  if (hook_slice > 0) {
    const int64_t least = ((ni + NB_SLICES_MAX - 1) / NB_SLICES_MAX + TK_THREADS - 1) / TK_THREADS * TK_THREADS;
    slice = std::max((hook_slice + TK_THREADS - 1) / TK_THREADS * TK_THREADS, least);
    S = std::max<int64_t>(1, (ni + slice - 1) / slice);
  }
  chunk = std::max<int64_t>(CT, std::min<int64_t>(chunk, NB_PARTIAL_MAX / (S * K) / CT * CT));
  if (hook_chunk > 0) chunk = std::min(chunk, hook_chunk);

  Scratch scratch(e->stream);
  Projections<T> pr;
  FMX_TRY(pr.reserve(scratch, ni, chunk, kp, ks));
  FMX_TRY(topk_project_rows(e, I, 0, ni, false, pr.q, ks, pr.ib, pr.is));  // the items, once per call
  double *iinv = nullptr, *qinv = nullptr;
  if (cosine) {
    FMX_TRY(scratch.get(&iinv, (size_t)ni));
    FMX_TRY(scratch.get(&qinv, (size_t)chunk));
    FMX_TRY(nb_norms<T>(e, pr.is, ni, ks, iinv));
  }
  double* ps = nullptr;
  int32_t* pi = nullptr;
  FMX_TRY(scratch.get(&ps, (size_t)chunk * S * K));
  FMX_TRY(scratch.get(&pi, (size_t)chunk * S * K));
  for (int64_t c = r0; c < r1; c += chunk) {
    const int64_t nq = std::min(chunk, r1 - c);
    FMX_TRY(topk_project_rows(e, Q, c, c + nq, false, pr.q, ks, pr.cb, pr.cs));
    if (cosine) FMX_TRY(nb_norms<T>(e, pr.cs, nq, ks, qinv));
    NbArgs a{};
    a.qs = pr.cs; a.qinv = qinv; a.is = pr.is; a.iinv = iinv;
    a.nq = nq; a.ni = ni; a.r0 = c; a.ks = ks; a.K = K; a.cosine = cosine ? 1 : 0; a.skip = skip ? 1 : 0;
    a.slice = slice; a.S = (int)S;
    a.ps = ps; a.pi = pi;
    FMX_TRY(nb_dispatch<T>(e, a, oi + (c - r0) * K, os + (c - r0) * K));
  }
  FMX_HIP(hipStreamSynchronize(e->stream));
  return FMX_OK;
}

}  // namespace

int neighbors_run(fmx_engine* e, const fmx_matrix* Q, int64_t r0, int64_t r1, const fmx_matrix* I, int K, int metric, bool skip_self, int64_t* d_index,
                  double* d_score) {
  if (r1 <= r0) return FMX_OK;
  if (I->n == 0) {  // nothing to rank: every slot is padding
    std::vector<int64_t> ni((size_t)(r1 - r0) * K, -1);
    std::vector<double> ns((size_t)(r1 - r0) * K, std::nan(""));
    FMX_HIP(hipMemcpy(d_index, ni.data(), ni.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    FMX_HIP(hipMemcpy(d_score, ns.data(), ns.size() * sizeof(double), hipMemcpyHostToDevice));
    return FMX_OK;
  }
  return wide_state(e) ? neighbors_run_t<double>(e, Q, r0, r1, I, K, metric, skip_self, d_index, d_score)
                       : neighbors_run_t<float>(e, Q, r0, r1, I, K, metric, skip_self, d_index, d_score);
}

void debug_neighbors_limits(int64_t slice_items, int64_t chunk_rows) {
  g_slice.store(slice_items > 0 ? slice_items : 0);
  g_chunk.store(chunk_rows > 0 ? chunk_rows : 0);
}

}  // namespace fmx
