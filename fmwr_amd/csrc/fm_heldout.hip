// Ranks of held-out items under fmx_topk's order, and the full-ranking metrics built on them (fmx_heldout_*).
//
// rank(c, h) = |{j eligible for c : j before h}| under fmx_topk's total order (a higher score first, equal scores by the lower item index,
// NaN below every number), eligible = not in c's exclusion list.  Per context chunk:
//   1. projection  base and s of the items once per call, of the chunk's contexts per chunk (topk_project_rows: the top-K's own);
//   2. positives   every held-out entry becomes the key (context << 32 | item); a radix sort, a flag + scan keep each (context, item) once;
//                  each distinct positive is scored with top-K's arithmetic (tk_pair_score), checked against the exclusion list, and a
//                  stable segmented radix sort on a monotone 64-bit key of its score orders each context's positives under the total order
//                  (the input is item-ascending, so equal scores keep the lower item first);
//   3. count       a grid of (context tile x item slice) workgroups.  A tile's s and a window of up to W of each context's sorted positives sit
//                  in LDS; every thread scores one item at a time against the tile (the fma chain of topk_score_k) and, only if the item comes
//                  before the window's last positive and is not excluded, binary-searches the window for the first positive it precedes and
//                  counts that bin (bin 0 in a register).  Bins are integers added to global memory: any order gives the same sums.  A window's
//                  bin 0 already holds every item before its first positive, so the windows of a context are independent;
//   4. finish      per context, the prefix sums of its windows' bins are the ranks of its sorted positives; the fp64 metrics follow from
//                  them in a fixed order, and the ranks are scattered back to the held-out entries (duplicates included).
// An item j = h scores the same bits as h did in step 2 and carries the same index, so it never comes before h.  Nothing is ordered by
// atomics and nothing in floating point is summed by them: the same inputs give the same bits whatever the chunking, slicing or window.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "fm_rank.h"

namespace fmx {
namespace {

constexpr int HO_THREADS = 256;
constexpr int HO_CT = 8;                       // contexts per tile
constexpr int HO_W = 256;                      // sorted positives per context and window in LDS
constexpr int64_t HO_CHUNK = 1 << 15;          // contexts per chunk
constexpr int64_t HO_CHUNK_ENTRIES = 1 << 22;  // held-out entries per chunk (a context with more is a chunk of its own)
constexpr int32_t HO_NONE = 0x7FFFFFFF;

std::atomic<int> g_window_once{0};     // test hook: the next call's window
std::atomic<int64_t> g_chunk_once{0};  //            and context chunk

// entry e of the chunk's held-out entries: key (row - first row) << 32 | item, value e
__global__ void ho_keys_k(const int64_t* __restrict__ rp, int64_t nc, const uint32_t* __restrict__ col, int64_t nh, uint64_t* __restrict__ keys,
                          uint32_t* __restrict__ vals) {
  const int64_t e = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (e >= nh) return;
  const int64_t at = rp[0] + e;
  int64_t lo = 0, hi = nc;  // the row holding the entry: the last r with rp[r] <= at
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rp[mid] <= at) lo = mid; else hi = mid;
  }
  keys[e] = ((uint64_t)lo << 32) | col[at];
  vals[e] = (uint32_t)e;
}

// the score of every distinct positive (top-K's arithmetic), its order key, and the check that it is not excluded: bad = the lowest
// offending context (the same one whatever the order)
template <typename T>
__global__ void ho_score_k(const uint64_t* __restrict__ dkey, int64_t nd, const T* __restrict__ cs, const double* __restrict__ cb, const T* __restrict__ is,
                           const double* __restrict__ ib, int ks, const int64_t* __restrict__ xrp, int64_t xbase, const uint32_t* __restrict__ xs,
                           int64_t cfirst, double* __restrict__ dsc, uint64_t* __restrict__ skey, uint32_t* __restrict__ sval,
                           unsigned long long* __restrict__ bad) {
  const int64_t d = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (d >= nd) return;
  const int64_t c = (int64_t)(dkey[d] >> 32);
  const uint32_t j = (uint32_t)dkey[d];
  const double s = tk_pair_score<T>(cs + c * ks, is + (int64_t)j * ks, ks, cb[c], ib[j]);
  dsc[d] = s;
  skey[d] = rank_order_key(s);
  sval[d] = (uint32_t)d;
  if (xrp) {
    const int64_t a = xrp[c] - xbase, b = xrp[c + 1] - xbase;
    if (a < b && tk_excluded(xs, a, b, j)) atomicMin(bad, (unsigned long long)(cfirst + c));
  }
}

// sorted position t holds distinct positive tord[t]: its score and item in sorted order, and the way back
__global__ void ho_place_k(const uint32_t* __restrict__ tord, int64_t nd, const uint64_t* __restrict__ dkey, const double* __restrict__ dsc,
                           double* __restrict__ ps, int32_t* __restrict__ pi, uint32_t* __restrict__ d2t) {
  const int64_t t = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (t >= nd) return;
  const uint32_t d = tord[t];
  ps[t] = dsc[d];
  pi[t] = (int32_t)(uint32_t)dkey[d];
  d2t[d] = (uint32_t)t;
}

struct CountArgs {
  const void* cs;          // contexts of the chunk: s [nc][ks]
  const double* cb;        //                        base [nc] (w0 included)
  const void* is;          // items: s [ni][ks]
  const double* ib;        //        base [ni] (no w0)
  int64_t nc, ni;
  int ks, W;
  int64_t slice;           // items per slice (a multiple of HO_THREADS)
  const int64_t* xrp;      // exclusion row offsets of the chunk's contexts [nc + 1] (absolute), or null
  int64_t xbase;           // xrp[0]: xs[e - xbase] holds entry e
  const uint32_t* xs;      // the chunk's exclusion ids, sorted by segment
  const int64_t* doff;     // [nc + 1]: context c's sorted distinct positives are [doff[c], doff[c + 1])
  const double* ps;        // their scores
  const int32_t* pi;       //       items
  uint32_t* bins;          // [nd]: bin t counts the eligible items whose first following positive is t (within its window)
};

template <typename T>
__global__ __launch_bounds__(HO_THREADS) void heldout_count_k(CountArgs a) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VN = StateVec<T>::N;
  constexpr int FB = 4 * VN;  // factors per block: four 16-byte loads of an item row in flight
  constexpr int KSM = TK_KS_BYTES / sizeof(T);
  __shared__ T sc[HO_CT][KSM];
  __shared__ double ws[HO_CT][HO_W];
  __shared__ int32_t wi[HO_CT][HO_W];
  __shared__ uint32_t wb[HO_CT][HO_W];
  __shared__ double sv[HO_CT][HO_THREADS];    // a thread's scores of the contexts whose window it may fall into
  __shared__ uint32_t b0[HO_CT][HO_THREADS];  // a thread's own bin-0 counts (no atomics in the item loop)
  __shared__ double bc[HO_CT], ls[HO_CT];
  __shared__ int32_t li[HO_CT];
  __shared__ int64_t xa[HO_CT], xb[HO_CT], da[HO_CT], db[HO_CT];
  __shared__ int wn[HO_CT];

  const int ks = a.ks, W = a.W;
  const int tid = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * HO_CT;
  const int nv = (int)(a.nc - c0 < HO_CT ? a.nc - c0 : HO_CT);
  const int64_t j0 = (int64_t)blockIdx.y * a.slice;
  const int64_t j1 = j0 + a.slice < a.ni ? j0 + a.slice : a.ni;
  const T* __restrict__ cs = reinterpret_cast<const T*>(a.cs);
  const T* __restrict__ is = reinterpret_cast<const T*>(a.is);

  for (int t = tid; t < HO_CT * ks; t += HO_THREADS) {
    const int c = t / ks, f = t % ks;
    sc[c][f] = c < nv ? cs[(c0 + c) * ks + f] : (T)0;
  }
  if (tid < HO_CT) {
    const int c = tid;
    bc[c] = c < nv ? a.cb[c0 + c] : 0.0;
    xa[c] = (a.xrp && c < nv) ? a.xrp[c0 + c] - a.xbase : 0;
    xb[c] = (a.xrp && c < nv) ? a.xrp[c0 + c + 1] - a.xbase : 0;
    da[c] = c < nv ? a.doff[c0 + c] : 0;
    db[c] = c < nv ? a.doff[c0 + c + 1] : 0;
  }
  __syncthreads();
  int64_t most = 0;
  for (int c = 0; c < HO_CT; ++c) most = db[c] - da[c] > most ? db[c] - da[c] : most;
  const int64_t rounds = (most + W - 1) / W;  // 0 for a tile without held-out items

  for (int64_t r = 0; r < rounds; ++r) {
    const int64_t w0 = r * W;
    for (int t = tid; t < HO_CT * HO_W; t += HO_THREADS) {
      const int c = t / HO_W, u = t % HO_W;
      const int64_t p = da[c] + w0 + u;
      const bool in = u < W && p < db[c];
      ws[c][u] = in ? a.ps[p] : __builtin_nan("");
      wi[c][u] = in ? a.pi[p] : HO_NONE;
      wb[c][u] = 0;
    }
    for (int c = 0; c < HO_CT; ++c) b0[c][tid] = 0;
    if (tid < HO_CT) {
      const int64_t left = db[tid] - da[tid] - w0;
      wn[tid] = (int)(left <= 0 ? 0 : left < W ? left : W);
    }
    __syncthreads();
    if (tid < HO_CT && wn[tid] > 0) { ls[tid] = ws[tid][wn[tid] - 1]; li[tid] = wi[tid][wn[tid] - 1]; }
    __syncthreads();

    for (int64_t jb = j0; jb < j1; jb += HO_THREADS) {
      const int64_t j = jb + tid;
      if (j >= j1) break;
      T acc[HO_CT];
#pragma unroll
      for (int c = 0; c < HO_CT; ++c) acc[c] = (T)0;
      const vec_t* row = reinterpret_cast<const vec_t*>(is + j * ks);
      for (int f0 = 0; f0 < ks; f0 += FB) {
        vec_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = row[f0 / VN + u];
        const T* si = reinterpret_cast<const T*>(v);
#pragma unroll
        for (int c = 0; c < HO_CT; ++c) {
#pragma unroll
          for (int f = 0; f < FB; ++f) acc[c] = fma(sc[c][f0 + f], si[f], acc[c]);  // f ascending: topk_score_k's chain
        }
      }
      const double bi = a.ib[j];
      uint32_t mask = 0;  // contexts whose window's last positive the item comes before; every other context is done with it (the usual case)
#pragma unroll
      for (int c = 0; c < HO_CT; ++c) {
        if (wn[c] == 0) continue;
        const double s = (bc[c] + bi) + (double)acc[c];
        if (rank_before(s, (int32_t)j, ls[c], li[c])) { mask |= 1u << c; sv[c][tid] = s; }
      }
      while (mask) {
        const int c = __builtin_ctz(mask);
        mask &= mask - 1;
        if (xa[c] < xb[c] && tk_excluded(a.xs, xa[c], xb[c], (uint32_t)j)) continue;
        const double s = sv[c][tid];
        int lo = 0, hi = wn[c] - 1;  // the first positive the item comes before (the last one qualifies)
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (rank_before(s, (int32_t)j, ws[c][mid], wi[c][mid])) hi = mid; else lo = mid + 1;
        }
        if (lo == 0) ++b0[c][tid];
        else atomicAdd(&wb[c][lo], 1u);
      }
    }
    for (int c = 0; c < HO_CT; ++c)
      if (b0[c][tid]) atomicAdd(&wb[c][0], b0[c][tid]);
    __syncthreads();
    for (int t = tid; t < HO_CT * HO_W; t += HO_THREADS) {
      const int c = t / HO_W, u = t % HO_W;
      if (u < wn[c] && wb[c][u]) atomicAdd(&a.bins[da[c] + w0 + u], wb[c][u]);
    }
    __syncthreads();  // the next window overwrites the LDS
  }
}

struct Ks { int32_t k[32]; };

// one thread per context of the chunk: ranks = the prefix sums of its windows' bins; then its metrics row (NaN without held-out items)
__global__ void ho_finish_k(const int64_t* __restrict__ doff, int64_t nc, const uint32_t* __restrict__ bins, int W, int64_t* __restrict__ trank,
                            double* __restrict__ pc, Ks ks, int n_ks, int64_t n_items, const int64_t* __restrict__ xrp, int64_t xbase,
                            const uint32_t* __restrict__ xs) {
  const int64_t c = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (c >= nc) return;
  const int64_t a = doff[c], b = doff[c + 1], m = b - a;
  int64_t acc = 0;
  for (int64_t t = a; t < b; ++t) {
    if ((t - a) % W == 0) acc = 0;
    acc += bins[t];
    trank[t] = acc;
  }
  if (!pc) return;
  const int cols = 4 * n_ks + 2;
  double* __restrict__ row = pc + c * cols;
  if (m == 0) {
    for (int q = 0; q < cols; ++q) row[q] = __builtin_nan("");
    return;
  }
  int64_t nx = 0;  // distinct excluded items: an id counts where it first occurs (earlier in its sorted segment, or in an earlier segment)
  if (xrp) {
    const int64_t xa = xrp[c] - xbase, xb = xrp[c + 1] - xbase;
    for (int64_t e = xa; e < xb; ++e) {
      const int64_t s0 = xa + (e - xa) / TK_SEG * TK_SEG;
      const bool seen = (e > s0 && xs[e - 1] == xs[e]) || (s0 > xa && tk_excluded(xs, xa, s0, xs[e]));
      nx += seen ? 0 : 1;
    }
  }
  for (int q = 0; q < n_ks; ++q) {
    const int64_t K = ks.k[q];
    int64_t hits = 0;
    double dcg = 0.0, idcg = 0.0;
    for (int64_t t = a; t < b && trank[t] < K; ++t) {  // ranks ascend with t
      ++hits;
      dcg += 1.0 / log2((double)trank[t] + 2.0);
    }
    const int64_t lim = K < m ? K : m;
    for (int64_t t = 0; t < lim; ++t) idcg += 1.0 / log2((double)t + 2.0);
    row[4 * q + 0] = (double)hits / (double)K;
    row[4 * q + 1] = (double)hits / (double)m;
    row[4 * q + 2] = dcg / idcg;
    row[4 * q + 3] = hits > 0 ? 1.0 : 0.0;
  }
  row[4 * n_ks] = 1.0 / (1.0 + (double)trank[a]);
  const int64_t N = n_items - nx - m;
  if (N <= 0) {
    row[4 * n_ks + 1] = __builtin_nan("");
  } else {
    double s = 0.0;
    for (int64_t t = a; t < b; ++t) s += (double)(N - (trank[t] - (t - a))) / (double)N;
    row[4 * n_ks + 1] = s / (double)m;
  }
}

// held-out entry e: the rank (and score) of its distinct positive
__global__ void ho_scatter_k(const uint32_t* __restrict__ e2d, const uint32_t* __restrict__ d2t, int64_t nh, const int64_t* __restrict__ trank,
                             const double* __restrict__ ps, int64_t* __restrict__ out_rank, double* __restrict__ out_score) {
  const int64_t e = (int64_t)blockIdx.x * HO_THREADS + threadIdx.x;
  if (e >= nh) return;
  const uint32_t t = d2t[e2d[e]];
  out_rank[e] = trank[t];
  if (out_score) out_score[e] = ps[t];
}

// one workgroup per metric: thread i sums contexts i, i + 256, ... in order (NaN rows left out), then a fixed tree over the threads
__global__ __launch_bounds__(HO_THREADS) void ho_mean_k(const double* __restrict__ pc, int64_t n, int cols, double* __restrict__ mean,
                                                        int64_t* __restrict__ cnt) {
  __shared__ double ss[HO_THREADS];
  __shared__ int64_t kk[HO_THREADS];
  const int q = blockIdx.x;
  double s = 0.0;
  int64_t k = 0;
  for (int64_t i = threadIdx.x; i < n; i += HO_THREADS) {
    const double v = pc[i * cols + q];
    if (v == v) { s += v; ++k; }
  }
  ss[threadIdx.x] = s;
  kk[threadIdx.x] = k;
  __syncthreads();
  for (int h = HO_THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) { ss[threadIdx.x] += ss[threadIdx.x + h]; kk[threadIdx.x] += kk[threadIdx.x + h]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mean[q] = kk[0] ? ss[0] / (double)kk[0] : __builtin_nan("");
    cnt[q] = kk[0];
  }
}

template <typename T>
int heldout_run_t(fmx_engine* e, const fmx_matrix* C, int64_t r0, int64_t r1, const fmx_matrix* I, const fmx_matrix* H, const fmx_matrix* X,
                  int64_t* d_rank, double* d_score, const int32_t* h_ks, int n_ks, double* pc) {
  const hipStream_t st = e->stream;
  const int kp = wide_state(e) ? e->kp64 : e->kp32;
  const int ks = state_factors<T>(e);
  FMX_CHECK(ks * (int)sizeof(T) <= TK_KS_BYTES, FMX_ERR_INVALID, "held-out ranking holds at most %d factors", TK_KS_BYTES / (int)sizeof(T));
  const int hook_w = g_window_once.exchange(0);
  const int64_t hook_chunk = g_chunk_once.exchange(0);
  const int W = hook_w > 0 ? std::min(hook_w, HO_W) : HO_W;
  const int64_t chunk_max = hook_chunk > 0 ? std::min(hook_chunk, HO_CHUNK) : HO_CHUNK;
  const int64_t n = r1 - r0, ni = I->n;
  Ks ks_arg{};
  for (int q = 0; q < n_ks; ++q) ks_arg.k[q] = h_ks[q];

  // the row offsets of heldout and exclude on the host: the chunks, and the scratch they need
  std::vector<int64_t> hrp((size_t)n + 1), xrp;
  FMX_HIP(hipMemcpyAsync(hrp.data(), H->row_ptr + r0, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (X) {
    xrp.resize((size_t)n + 1);
    FMX_HIP(hipMemcpyAsync(xrp.data(), X->row_ptr + r0, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  }
  FMX_HIP(hipStreamSynchronize(st));
  const std::vector<int64_t> cut = rank_chunks(hrp, n, chunk_max, HO_CHUNK_ENTRIES);
  int64_t max_nh = 0, max_nx = 0, max_nc = 0;
  for (size_t ci = 0; ci + 1 < cut.size(); ++ci) {
    const int64_t a = cut[ci], b = cut[ci + 1];
    max_nh = std::max(max_nh, hrp[b] - hrp[a]);
    if (X) max_nx = std::max(max_nx, xrp[b] - xrp[a]);
    max_nc = std::max(max_nc, b - a);
  }
  FMX_CHECK(max_nh < (1LL << 32), FMX_ERR_INVALID, "a context holds %lld held-out entries: at most 2^32 - 1", (long long)max_nh);

  Scratch S(st);
  Projections<T> pr;
  FMX_TRY(pr.reserve(S, ni, max_nc, kp, ks));
  if (ni > 0 && max_nh > 0) FMX_TRY(topk_project_rows(e, I, 0, ni, false, pr.q, ks, pr.ib, pr.is));  // the items, once per call

  // per-chunk scratch, sized for the largest chunk
  const size_t NH = (size_t)max_nh;
  DistinctPairs dp;
  FMX_TRY(dp.reserve(S, st, NH, max_nc));
  uint32_t *d2t, *bins, *xs;
  double *dsc, *ps;
  int32_t* pi;
  int64_t *trank, *all_rank = nullptr;
  double* all_score = nullptr;
  unsigned long long* bad;
  FMX_TRY(S.get(&d2t, NH)); FMX_TRY(S.get(&bins, NH)); FMX_TRY(S.get(&xs, (size_t)max_nx));
  FMX_TRY(S.get(&dsc, NH)); FMX_TRY(S.get(&ps, NH)); FMX_TRY(S.get(&pi, NH));
  FMX_TRY(S.get(&trank, NH)); FMX_TRY(S.get(&bad, 1));
  const int64_t total = hrp[n] - hrp[0];
  if (d_rank) {  // the outputs are written only once every chunk has passed the exclusion check
    FMX_TRY(S.get(&all_rank, (size_t)total));
    if (d_score) FMX_TRY(S.get(&all_score, (size_t)total));
  }

  const int cus = device_cus(e->cfg.device);
  for (size_t ci = 0; ci + 1 < cut.size(); ++ci) {
    const int64_t c = r0 + cut[ci], nc = cut[ci + 1] - cut[ci];
    const int64_t h0 = hrp[cut[ci]], nh = hrp[cut[ci + 1]] - h0;
    const int64_t* cx = X ? X->row_ptr + c : nullptr;
    int64_t x0 = 0;
    if (X) {
      x0 = xrp[cut[ci]];
      FMX_TRY(topk_sort_excl(st, cx, nc, X->col, x0, xs));
    }
    int64_t nd = 0;
    if (nh > 0) {
      FMX_TRY(topk_project_rows(e, C, c, c + nc, true, pr.q, ks, pr.cb, pr.cs));
      hipLaunchKernelGGL(ho_keys_k, dim3(blocks(nh, HO_THREADS)), dim3(HO_THREADS), 0, st, H->row_ptr + c, nc, H->col, nh, dp.k_in, dp.v_in);
    }
    FMX_TRY(dp.distinct(nh, nc, &nd));  // a chunk without entries still gets its offsets: ho_finish_k reads them
    if (nd > 0) {
      // scores, order keys (into k_in, free again), the exclusion check; then each context's positives under the total order
      FMX_HIP(hipMemsetAsync(bad, 0xFF, sizeof(unsigned long long), st));
      hipLaunchKernelGGL((ho_score_k<T>), dim3(blocks(nd, HO_THREADS)), dim3(HO_THREADS), 0, st, dp.dkey, nd, pr.cs, pr.cb, pr.is, pr.ib, ks, cx, x0,
                         (const uint32_t*)xs, c, dsc, dp.k_in, dp.v_in, bad);
      unsigned long long h_bad = 0;
      FMX_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, st));
      FMX_HIP(hipStreamSynchronize(st));
      FMX_CHECK(h_bad == ~0ull, FMX_ERR_INVALID, "context %llu holds an item both in heldout and in exclude", h_bad);
      FMX_TRY(dp.order(nd, nc));
      hipLaunchKernelGGL(ho_place_k, dim3(blocks(nd, HO_THREADS)), dim3(HO_THREADS), 0, st, dp.v_out, nd, dp.dkey, dsc, ps, pi, d2t);

      // the count pass over (context tile x item slice) workgroups
      const int64_t tiles = (nc + HO_CT - 1) / HO_CT;
      int64_t nsl, slice;
      rank_slices(ni, tiles, cus, HO_THREADS, &slice, &nsl);
      FMX_HIP(hipMemsetAsync(bins, 0, (size_t)nd * sizeof(uint32_t), st));
      CountArgs a{};
      a.cs = pr.cs; a.cb = pr.cb; a.is = pr.is; a.ib = pr.ib; a.nc = nc; a.ni = ni; a.ks = ks; a.W = W; a.slice = slice;
      if (X) { a.xrp = cx; a.xbase = x0; a.xs = xs; }
      a.doff = dp.doff; a.ps = ps; a.pi = pi; a.bins = bins;
      hipLaunchKernelGGL((heldout_count_k<T>), dim3((unsigned)tiles, (unsigned)nsl), dim3(HO_THREADS), 0, st, a);
      FMX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ho_finish_k, dim3(blocks(nc, HO_THREADS)), dim3(HO_THREADS), 0, st, dp.doff, nc, bins, W, trank, pc ? pc + (c - r0) * (4 * n_ks + 2) : nullptr,
                       ks_arg, n_ks, ni, cx, x0, (const uint32_t*)xs);
    if (all_rank && nh > 0)
      hipLaunchKernelGGL(ho_scatter_k, dim3(blocks(nh, HO_THREADS)), dim3(HO_THREADS), 0, st, dp.e2d, d2t, nh, trank, ps, all_rank + (h0 - hrp[0]),
                         all_score ? all_score + (h0 - hrp[0]) : nullptr);
    FMX_HIP(hipGetLastError());
  }
  if (d_rank && total > 0) {
    FMX_HIP(hipMemcpyAsync(d_rank, all_rank, (size_t)total * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    if (d_score) FMX_HIP(hipMemcpyAsync(d_score, all_score, (size_t)total * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  FMX_HIP(hipStreamSynchronize(st));
  return FMX_OK;
}

}  // namespace

int heldout_run(fmx_engine* e, const fmx_matrix* C, int64_t r0, int64_t r1, const fmx_matrix* I, const fmx_matrix* H, const fmx_matrix* X, int64_t* d_rank,
                double* d_score, const int32_t* ks, int n_ks, double* pc) {
  if (r1 <= r0) return FMX_OK;
  return wide_state(e) ? heldout_run_t<double>(e, C, r0, r1, I, H, X, d_rank, d_score, ks, n_ks, pc)
                       : heldout_run_t<float>(e, C, r0, r1, I, H, X, d_rank, d_score, ks, n_ks, pc);
}

int heldout_means(fmx_engine* e, const double* pc, int64_t n, int cols, double* out, int64_t* counted) {
  Scratch S(e->stream);
  double* mean = nullptr;
  int64_t* cnt = nullptr;
  FMX_TRY(S.get(&mean, (size_t)cols)); FMX_TRY(S.get(&cnt, (size_t)cols));
  hipLaunchKernelGGL(ho_mean_k, dim3((unsigned)cols), dim3(HO_THREADS), 0, e->stream, pc, n, cols, mean, cnt);
  FMX_HIP(hipGetLastError());
  std::vector<int64_t> h_cnt((size_t)cols);
  FMX_HIP(hipMemcpyAsync(out, mean, (size_t)cols * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  FMX_HIP(hipMemcpyAsync(h_cnt.data(), cnt, (size_t)cols * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
  FMX_HIP(hipStreamSynchronize(e->stream));
  if (counted) { counted[0] = h_cnt[0]; counted[1] = h_cnt[(size_t)cols - 1]; }
  return FMX_OK;
}

void debug_heldout_limits(int window, int64_t chunk) {
  g_window_once.store(window > 0 ? window : 0);
  g_chunk_once.store(chunk > 0 ? chunk : 0);
}

}  // namespace fmx
