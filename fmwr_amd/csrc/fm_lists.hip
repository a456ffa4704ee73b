// Re-ranking of candidate lists (fmx_rank_lists, fmx_topk_lists) and the projections behind the score (fmx_project); DESIGN.md section 17.
//
// lists' row c names L_c, the candidates of context c.  score(c, j) is fmx_topk's raw score of the pair, bit for bit (the projections of
// topk_project_rows, one fma chain in the state type over f = 0 .. ks - 1, then (base_c + base_j) + (double)dot), and
// pos(c, j) = |{j' in distinct(L_c) : j' before j}| under fmx_topk's total order (a higher score first, equal scores by the lower item index,
// NaN below every number).  Per chunk of contexts:
//   1. projection   base and s of the items once per call, of the chunk's contexts per chunk (topk_project_rows: the top-K's own);
//   2. fused path   a context whose list fits the LDS budget is one workgroup: s_c and the list in LDS; the candidates' s rows are gathered
//                   cooperatively (row_bytes / 16 lanes per row, 16 bytes each, four rows in flight per lane group) into a padded LDS tile; one
//                   thread per candidate runs the single fma chain out of LDS; (score, item, entry) are sorted in LDS (bitonic, under the total
//                   order), a flag + scan over equal items gives the distinct positions, and every entry's result is written where it stood;
//      general path the entries of every longer list become keys (context << 32 | item); a radix sort, a flag + scan keep each (context, item)
//                   once; each distinct candidate is scored (tk_pair_score), a stable segmented radix sort on a monotone 64-bit key of the
//                   score orders each context's candidates (the input is item-ascending, so equal scores keep the lower item first), and
//                   score and position go back to the entries;
//   3. fmx_topk_lists is the same pass with another last step: the distinct candidate with pos < K writes slot pos of its context; the other
//      slots were filled with -1 / NaN before.
// The order is strict and total on distinct items, so a list's positions do not depend on the sorting algorithm: the two paths give the same
// bits.  Nothing is ordered by atomics and no floating-point value is summed by them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "fm_rank.h"

namespace fmx {
namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_LDS_ENTRIES = 1024;           // the longest list the fused path takes (entries, duplicates included)
constexpr int LS_TILE_BYTES = 36 << 10;        // the gather tile of a workgroup: tile rows x (row bytes + 16)
constexpr int64_t LS_CHUNK = 1 << 15;          // contexts per chunk
constexpr int64_t LS_CHUNK_ENTRIES = 1 << 22;  // list entries per chunk (a context with more is a chunk of its own)
constexpr int64_t LS_PROJ_ROWS = 1 << 16;      // rows per slab of fmx_project
constexpr int32_t LS_NONE = 0x7FFFFFFF;        // padding entry (score NaN): below every item, NaN-scored ones included

std::atomic<int> g_lds_entries{0};  // test hook (sticky): the fused path's budget
std::atomic<int64_t> g_chunk{0};    //                     and the context chunk

// ---------------------------------------------------------------------------------------------------------------- fused path

struct FusedArgs {
  const void* cs;        // contexts of the chunk: s [nc][ks]
  const double* cb;      //                        base [nc] (w0 included)
  const void* is;        // items: s [ni][ks]
  const double* ib;      //        base [ni] (no w0)
  const int64_t* rp;     // the chunk's rows of lists: [nc + 1] absolute entry offsets
  const uint32_t* col;   // lists' column ids
  int64_t out0;          // entry out0 is index 0 of out_score / out_pos
  int ks, budget, tr;    // factors (padded); lists of at most `budget` entries are taken; rows per gather tile
  int K, link;
  double* out_score;     // ranking: per entry (out_pos may be null)
  int64_t* out_pos;
  int64_t* oi;           // top-K: [nc][K], pre-filled with -1 / NaN
  double* os;
  Hyper h;
  const double* pn_y;
};

template <typename T>
__global__ __launch_bounds__(LS_THREADS) void lists_fused_k(FusedArgs a) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VN = StateVec<T>::N;
  constexpr int KSM = TK_KS_BYTES / sizeof(T);
  extern __shared__ uint4 tile[];  // tr rows of ks * sizeof(T) + 16 bytes: the pad keeps the threads' 16-byte row reads on different banks
  __shared__ T sc[KSM];
  __shared__ double ss[LS_LDS_ENTRIES];
  __shared__ int32_t si[LS_LDS_ENTRIES];
  __shared__ int32_t se[LS_LDS_ENTRIES];
  __shared__ int part[2][LS_THREADS];

  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  const int64_t e0 = a.rp[c], len = a.rp[c + 1] - e0;
  if (len <= 0 || len > a.budget) return;  // an empty list; a long one is the general path's
  const int n = (int)len, ks = a.ks;
  int m = 1;
  while (m < n) m <<= 1;

  const T* __restrict__ cs = reinterpret_cast<const T*>(a.cs) + c * ks;
  for (int f = tid; f < ks; f += LS_THREADS) sc[f] = cs[f];
  for (int t = tid; t < m; t += LS_THREADS) {
    si[t] = t < n ? (int32_t)a.col[e0 + t] : LS_NONE;
    se[t] = t;
    if (t >= n) ss[t] = __builtin_nan("");
  }
  __syncthreads();

  const double bc = a.cb[c];
  const int rb16 = ks * (int)sizeof(T) / 16;  // 16-byte pieces of a row
  const int stride16 = rb16 + 1;
  const uint4* __restrict__ is16 = reinterpret_cast<const uint4*>(a.is);
  for (int t0 = 0; t0 < n; t0 += a.tr) {
    const int rows = n - t0 < a.tr ? n - t0 : a.tr;
    const int pieces = rows * rb16;
    for (int p0 = tid; p0 < pieces; p0 += 4 * LS_THREADS) {
      // four loads in flight per lane; the lanes p .. p + rb16 - 1 cover one row (a piece past the end re-reads piece p0 and is dropped)
      const int p1 = p0 + LS_THREADS < pieces ? p0 + LS_THREADS : p0, p2 = p0 + 2 * LS_THREADS < pieces ? p0 + 2 * LS_THREADS : p0,
                p3 = p0 + 3 * LS_THREADS < pieces ? p0 + 3 * LS_THREADS : p0;
      const int r0 = p0 / rb16, r1 = p1 / rb16, r2 = p2 / rb16, r3 = p3 / rb16;
      const int q0 = p0 - r0 * rb16, q1 = p1 - r1 * rb16, q2 = p2 - r2 * rb16, q3 = p3 - r3 * rb16;
      const uint4 v0 = is16[(int64_t)si[t0 + r0] * rb16 + q0];
      const uint4 v1 = is16[(int64_t)si[t0 + r1] * rb16 + q1];
      const uint4 v2 = is16[(int64_t)si[t0 + r2] * rb16 + q2];
      const uint4 v3 = is16[(int64_t)si[t0 + r3] * rb16 + q3];
      tile[r0 * stride16 + q0] = v0;
      if (p1 != p0) tile[r1 * stride16 + q1] = v1;
      if (p2 != p0) tile[r2 * stride16 + q2] = v2;
      if (p3 != p0) tile[r3 * stride16 + q3] = v3;
    }
    __syncthreads();
    if (tid < rows) {
      const vec_t* row = reinterpret_cast<const vec_t*>(tile + (size_t)tid * stride16);
      T acc = (T)0;
      for (int f0 = 0; f0 < ks; f0 += VN) {
        const vec_t x = row[f0 / VN];
        const T* xs = reinterpret_cast<const T*>(&x);
#pragma unroll
        for (int u = 0; u < VN; ++u) acc = fma(sc[f0 + u], xs[u], acc);  // f ascending, one accumulator: the chain of tk_pair_score
      }
      ss[t0 + tid] = (bc + a.ib[si[t0 + tid]]) + (double)acc;
    }
    __syncthreads();  // the next tile overwrites the LDS
  }

  // bitonic sort of the m slots under the total order (duplicates of an item are equal: they end up side by side)
  for (int size = 2; size <= m; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < m / 2; t += LS_THREADS) {
        const int x = 2 * t - (t & (stride - 1)), y = x + stride;
        const double sx = ss[x], sy = ss[y];
        const int32_t ix = si[x], iy = si[y];
        const bool swap = (x & size) == 0 ? rank_before(sy, iy, sx, ix) : rank_before(sx, ix, sy, iy);
        if (swap) {
          const int32_t ex = se[x];
          ss[x] = sy; ss[y] = sx; si[x] = iy; si[y] = ix; se[x] = se[y]; se[y] = ex;
        }
      }
      __syncthreads();
    }
  }

  // positions: the heads (first of each run of one item) counted up to every slot; thread t owns slots [t E, t E + E)
  const int E = (m + LS_THREADS - 1) / LS_THREADS;
  const int b0 = tid * E;
  int heads = 0;
  for (int t = b0; t < b0 + E && t < n; ++t) heads += (t == 0 || si[t] != si[t - 1]) ? 1 : 0;
  part[0][tid] = heads;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < LS_THREADS; d <<= 1) {
    part[cur ^ 1][tid] = part[cur][tid] + (tid >= d ? part[cur][tid - d] : 0);
    cur ^= 1;
    __syncthreads();
  }
  int pos = part[cur][tid] - heads - 1;  // of the last distinct candidate before this thread's slots
  for (int t = b0; t < b0 + E && t < n; ++t) {
    const bool head = t == 0 || si[t] != si[t - 1];
    pos += head ? 1 : 0;
    if (a.oi) {
      if (head && pos < a.K) {
        a.oi[c * a.K + pos] = si[t];
        a.os[c * a.K + pos] = rank_link(a.h, ss[t], a.link, a.pn_y);
      }
    } else {
      const int64_t o = e0 - a.out0 + se[t];
      a.out_score[o] = rank_link(a.h, ss[t], a.link, a.pn_y);
      if (a.out_pos) a.out_pos[o] = pos;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- general path

// entry g of the chunk's long lists (long list q = context lc[q] holds entries [loff[q], loff[q + 1])): key context << 32 | item, value g,
// and where the entry stands among the chunk's entries
__global__ void ls_keys_k(const int64_t* __restrict__ rp, const uint32_t* __restrict__ lc, const int64_t* __restrict__ loff, int64_t nlong,
                          const uint32_t* __restrict__ col, int64_t nl, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                          uint32_t* __restrict__ gat) {
  const int64_t g = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
  if (g >= nl) return;
  int64_t lo = 0, hi = nlong;  // the last q with loff[q] <= g
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (loff[mid] <= g) lo = mid; else hi = mid;
  }
  const uint32_t c = lc[lo];
  const int64_t at = rp[c] + (g - loff[lo]);
  keys[g] = ((uint64_t)c << 32) | col[at];
  vals[g] = (uint32_t)g;
  gat[g] = (uint32_t)(at - rp[0]);
}

// the score of every distinct candidate (top-K's arithmetic) and its order key
template <typename T>
__global__ void ls_score_k(const uint64_t* __restrict__ dkey, int64_t nd, const T* __restrict__ cs, const double* __restrict__ cb, const T* __restrict__ is,
                           const double* __restrict__ ib, int ks, double* __restrict__ dsc, uint64_t* __restrict__ skey, uint32_t* __restrict__ sval) {
  const int64_t d = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
  if (d >= nd) return;
  const int64_t c = (int64_t)(dkey[d] >> 32);
  const uint32_t j = (uint32_t)dkey[d];
  const double s = tk_pair_score<T>(cs + c * ks, is + (int64_t)j * ks, ks, cb[c], ib[j]);
  dsc[d] = s;
  skey[d] = rank_order_key(s);
  sval[d] = (uint32_t)d;
}

// sorted slot t holds distinct candidate tord[t]: its position in its context's list
__global__ void ls_place_k(const uint32_t* __restrict__ tord, int64_t nd, const uint64_t* __restrict__ dkey, const int64_t* __restrict__ doff,
                           uint32_t* __restrict__ dpos) {
  const int64_t t = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
  if (t >= nd) return;
  const uint32_t d = tord[t];
  dpos[d] = (uint32_t)(t - doff[dkey[d] >> 32]);
}

// entry g: the score and the position of its distinct candidate, written where the entry stands
__global__ void ls_scatter_k(const uint32_t* __restrict__ e2d, const uint32_t* __restrict__ gat, int64_t nl, const double* __restrict__ dsc,
                             const uint32_t* __restrict__ dpos, Hyper h, int link, const double* __restrict__ pn_y, double* __restrict__ out_score,
                             int64_t* __restrict__ out_pos) {
  const int64_t g = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
  if (g >= nl) return;
  const uint32_t d = e2d[g];
  out_score[gat[g]] = rank_link(h, dsc[d], link, pn_y);
  if (out_pos) out_pos[gat[g]] = dpos[d];
}

// distinct candidate d with pos < K: slot pos of its context
__global__ void ls_topk_scatter_k(const uint64_t* __restrict__ dkey, int64_t nd, const double* __restrict__ dsc, const uint32_t* __restrict__ dpos, int K,
                                  Hyper h, int link, const double* __restrict__ pn_y, int64_t* __restrict__ oi, double* __restrict__ os) {
  const int64_t d = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
  if (d >= nd || dpos[d] >= (uint32_t)K) return;
  const int64_t o = (int64_t)(dkey[d] >> 32) * K + dpos[d];
  oi[o] = (int64_t)(uint32_t)dkey[d];
  os[o] = rank_link(h, dsc[d], link, pn_y);
}

__global__ void ls_fill_k(int64_t n, int64_t* __restrict__ oi, double* __restrict__ os) {
  const int64_t t = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
  if (t < n) { oi[t] = -1; os[t] = __builtin_nan(""); }
}

// s [n][ks] in the state type -> f64 [n][k]: the widening is exact, the zero padding is dropped
template <typename T>
__global__ void ls_widen_k(const T* __restrict__ s, int64_t n, int ks, int k, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * LS_THREADS + threadIdx.x;
  if (t >= n * k) return;
  out[t] = (double)s[t / k * ks + t % k];
}

// ---------------------------------------------------------------------------------------------------------------- host side

template <typename T>
int lists_run_t(fmx_engine* e, const fmx_matrix* C, int64_t r0, int64_t r1, const fmx_matrix* I, const fmx_matrix* Lm, int link, int K, double* d_score,
                int64_t* d_pos, int64_t* d_index, double* d_tscore) {
  const hipStream_t st = e->stream;
  const int kp = wide_state(e) ? e->kp64 : e->kp32;
  const int ks = state_factors<T>(e);
  FMX_CHECK(ks * (int)sizeof(T) <= TK_KS_BYTES, FMX_ERR_INVALID, "list ranking holds at most %d factors", TK_KS_BYTES / (int)sizeof(T));
  const int hook_lds = g_lds_entries.load();
  const int64_t hook_chunk = g_chunk.load();
  const int budget = hook_lds > 0 ? std::min(hook_lds, LS_LDS_ENTRIES) : LS_LDS_ENTRIES;
  const int64_t chunk_max = hook_chunk > 0 ? std::min(hook_chunk, LS_CHUNK) : LS_CHUNK;
  const int64_t n = r1 - r0, ni = I->n;
  const bool topk = d_index != nullptr;
  const double* pn_y = (const double*)e->probit;

  // the row offsets of lists on the host: the chunks, which lists are long, and the scratch the general path needs
  std::vector<int64_t> hrp((size_t)n + 1);
  FMX_HIP(hipMemcpyAsync(hrp.data(), Lm->row_ptr + r0, (n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  const std::vector<int64_t> cut = rank_chunks(hrp, n, chunk_max, LS_CHUNK_ENTRIES);
  int64_t max_nl = 0, max_long = 0, max_nc = 0, max_nh = 0;
  for (size_t ci = 0; ci + 1 < cut.size(); ++ci) {
    const int64_t a = cut[ci], b = cut[ci + 1];
    int64_t nl = 0, nlong = 0;
    for (int64_t c = a; c < b; ++c) {
      const int64_t len = hrp[c + 1] - hrp[c];
      if (len > budget) { nl += len; ++nlong; }
    }
    max_nl = std::max(max_nl, nl);
    max_long = std::max(max_long, nlong);
    max_nc = std::max(max_nc, b - a);
    max_nh = std::max(max_nh, hrp[b] - hrp[a]);
  }
  FMX_CHECK(max_nh < (1LL << 32), FMX_ERR_INVALID, "a context's list holds %lld entries: at most 2^32 - 1", (long long)max_nh);
  const int64_t total = hrp[n] - hrp[0];

  if (topk) {
    hipLaunchKernelGGL(ls_fill_k, dim3(blocks(n * K, LS_THREADS)), dim3(LS_THREADS), 0, st, n * K, d_index, d_tscore);
    FMX_HIP(hipGetLastError());
  }
  if (total == 0) {
    FMX_HIP(hipStreamSynchronize(st));
    return FMX_OK;
  }

  Scratch S(st);
  Projections<T> pr;
  FMX_TRY(pr.reserve(S, ni, max_nc, kp, ks));
  FMX_TRY(topk_project_rows(e, I, 0, ni, false, pr.q, ks, pr.ib, pr.is));  // the items, once per call

  // the general path's scratch, sized for the chunk with the most entries in long lists
  const size_t NL = (size_t)max_nl;
  DistinctPairs dp;
  uint32_t *dpos = nullptr, *gat = nullptr, *lc = nullptr;
  double* dsc = nullptr;
  int64_t* loff = nullptr;
  if (max_nl > 0) {
    FMX_TRY(dp.reserve(S, st, NL, max_nc));
    FMX_TRY(S.get(&dpos, NL)); FMX_TRY(S.get(&gat, NL)); FMX_TRY(S.get(&dsc, NL));
    FMX_TRY(S.get(&lc, (size_t)max_long)); FMX_TRY(S.get(&loff, (size_t)max_long + 1));
  }

  const int row_bytes = ks * (int)sizeof(T) + 16;
  int tr = LS_THREADS;
  while (tr > 32 && tr * row_bytes > LS_TILE_BYTES) tr >>= 1;

  std::vector<uint32_t> h_lc;
  std::vector<int64_t> h_loff;
  for (size_t ci = 0; ci + 1 < cut.size(); ++ci) {
    const int64_t c = r0 + cut[ci], nc = cut[ci + 1] - cut[ci];
    const int64_t h0 = hrp[cut[ci]], nh = hrp[cut[ci + 1]] - h0;
    if (nh == 0) continue;
    h_lc.clear();
    h_loff.assign(1, 0);
    int64_t nshort = 0;
    for (int64_t r = 0; r < nc; ++r) {
      const int64_t len = hrp[cut[ci] + r + 1] - hrp[cut[ci] + r];
      if (len > budget) { h_lc.push_back((uint32_t)r); h_loff.push_back(h_loff.back() + len); }
      else if (len > 0) ++nshort;
    }
    const int64_t nlong = (int64_t)h_lc.size(), nl = h_loff.back();
    FMX_TRY(topk_project_rows(e, C, c, c + nc, true, pr.q, ks, pr.cb, pr.cs));
    double* o_score = topk ? nullptr : d_score + (h0 - hrp[0]);
    int64_t* o_pos = (topk || !d_pos) ? nullptr : d_pos + (h0 - hrp[0]);
    int64_t* o_index = topk ? d_index + (c - r0) * K : nullptr;
    double* o_tscore = topk ? d_tscore + (c - r0) * K : nullptr;

    if (nshort > 0) {
      FusedArgs a{};
      a.cs = pr.cs; a.cb = pr.cb; a.is = pr.is; a.ib = pr.ib; a.rp = Lm->row_ptr + c; a.col = Lm->col; a.out0 = h0;
      a.ks = ks; a.budget = budget; a.tr = tr; a.K = K; a.link = link;
      a.out_score = o_score; a.out_pos = o_pos; a.oi = o_index; a.os = o_tscore; a.h = e->hyper; a.pn_y = pn_y;
      hipLaunchKernelGGL((lists_fused_k<T>), dim3((unsigned)nc), dim3(LS_THREADS), (size_t)tr * row_bytes, st, a);
      FMX_HIP(hipGetLastError());
    }
    if (nl > 0) {
      FMX_HIP(hipMemcpyAsync(lc, h_lc.data(), (size_t)nlong * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      FMX_HIP(hipMemcpyAsync(loff, h_loff.data(), (size_t)(nlong + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(ls_keys_k, dim3(blocks(nl, LS_THREADS)), dim3(LS_THREADS), 0, st, Lm->row_ptr + c, (const uint32_t*)lc, (const int64_t*)loff, nlong, Lm->col, nl,
                         dp.k_in, dp.v_in, gat);
      int64_t nd = 0;
      FMX_TRY(dp.distinct(nl, nc, &nd));  // (its read-back waits for the copies of the host lists above, too)
      // scores and order keys (into k_in, free again); then each context's candidates under the total order
      hipLaunchKernelGGL((ls_score_k<T>), dim3(blocks(nd, LS_THREADS)), dim3(LS_THREADS), 0, st, dp.dkey, nd, pr.cs, pr.cb, pr.is, pr.ib, ks, dsc, dp.k_in,
                         dp.v_in);
      FMX_TRY(dp.order(nd, nc));
      hipLaunchKernelGGL(ls_place_k, dim3(blocks(nd, LS_THREADS)), dim3(LS_THREADS), 0, st, dp.v_out, nd, dp.dkey, dp.doff, dpos);
      if (topk)
        hipLaunchKernelGGL(ls_topk_scatter_k, dim3(blocks(nd, LS_THREADS)), dim3(LS_THREADS), 0, st, dp.dkey, nd, dsc, dpos, K, e->hyper, link, pn_y, o_index, o_tscore);
      else
        hipLaunchKernelGGL(ls_scatter_k, dim3(blocks(nl, LS_THREADS)), dim3(LS_THREADS), 0, st, dp.e2d, gat, nl, dsc, dpos, e->hyper, link, pn_y, o_score, o_pos);
      FMX_HIP(hipGetLastError());
    }
  }
  FMX_HIP(hipStreamSynchronize(st));
  return FMX_OK;
}

template <typename T>
int project_run_t(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, bool with_w0, double* d_base, double* d_s) {
  const hipStream_t st = e->stream;
  const int kp = wide_state(e) ? e->kp64 : e->kp32;
  const int ks = state_factors<T>(e), k = e->k;
  const int64_t slab = std::min<int64_t>(r1 - r0, LS_PROJ_ROWS);
  Scratch S(st);
  double* q = nullptr;
  T* s = nullptr;
  FMX_TRY(S.get(&q, (size_t)slab * kp));
  FMX_TRY(S.get(&s, (size_t)slab * ks));
  for (int64_t r = r0; r < r1; r += slab) {
    const int64_t n = std::min(slab, r1 - r);
    FMX_TRY(topk_project_rows(e, m, r, r + n, with_w0, q, ks, d_base + (r - r0), s));
    if (k > 0) {
      hipLaunchKernelGGL((ls_widen_k<T>), dim3(blocks(n * k, LS_THREADS)), dim3(LS_THREADS), 0, st, (const T*)s, n, ks, k, d_s + (r - r0) * k);
      FMX_HIP(hipGetLastError());
    }
  }
  FMX_HIP(hipStreamSynchronize(st));
  return FMX_OK;
}

}  // namespace

int lists_run(fmx_engine* e, const fmx_matrix* C, int64_t r0, int64_t r1, const fmx_matrix* I, const fmx_matrix* Lm, int link, int K, double* d_score,
              int64_t* d_pos, int64_t* d_index, double* d_tscore) {
  if (r1 <= r0) return FMX_OK;
  if (link == FMX_LINK_PROBIT) FMX_TRY(ensure_probit(e));
  return wide_state(e) ? lists_run_t<double>(e, C, r0, r1, I, Lm, link, K, d_score, d_pos, d_index, d_tscore)
                       : lists_run_t<float>(e, C, r0, r1, I, Lm, link, K, d_score, d_pos, d_index, d_tscore);
}

int project_run(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, bool with_w0, double* d_base, double* d_s) {
  if (r1 <= r0) return FMX_OK;
  return wide_state(e) ? project_run_t<double>(e, m, r0, r1, with_w0, d_base, d_s) : project_run_t<float>(e, m, r0, r1, with_w0, d_base, d_s);
}

void debug_lists_limits(int lds_entries, int64_t chunk) {
  g_lds_entries.store(lds_entries > 0 ? lds_entries : 0);
  g_chunk.store(chunk > 0 ? chunk : 0);
}

}  // namespace fmx
