// A clustered (inverted-file) item index and the approximate top-K over its probed lists (fmx_index_build, fmx_index_from_assign, fmx_topk_index;
// DESIGN.md section 29).  include/fmx.h holds the contract to the bit, tests/index_model.py restates it in numpy.
//
// The index is plain data: n_lists centroids of k + 1 doubles, the list of every item, and the lists as CSR (items ascending inside a list).  The
// augmented vector of item i is a_i = (s_i widened to double, base_i), fmx_project(with_w0 = 0)'s values: the item side of fmx_topk's score is the
// inner product of (s_c, 1) with a_i.
//
//   build    a deterministic k-means over the a_i.  Seeds: the finite items in the order of (pair_hash(seed, 0, i, 5), i) -- a compaction of the
//            finite ids and one stable 64-bit radix sort.  Assign: a grid over item tiles, one item per thread; the centroids are staged in LDS
//            in slices of lists and read as broadcasts; a thread holds IX_FB components of its row and IX_LG carried accumulators at a time, so
//            every (item, list) distance is ONE fp64 chain with f ascending whatever k is, and the running (best, list) is carried across
//            slices.  Update: a stable sort of (list, item), the list offsets by binary search (group_offsets), and one workgroup per list that
//            sums component by component in THE ORDER OF fm_columns.hip's sums -- chunks of 1 024 positions of the list, lane l of a wave adds
//            positions l, l + 64, ... from +0.0, an xor butterfly (strides 32 .. 1), the chunk sums added ascending from +0.0 -- over the finite
//            members (a non-finite member adds nothing).  No floating-point atomics anywhere.
//   search   the items are projected once per call (fmx_topk's projection) and gathered into list order; per chunk of contexts
//            coarse   g(c, l) = mu_l[k] + the fp64 chain of (double) s_c . mu_l over the non-empty lists; the first n_probe of them under
//                     rank_before by fm_rank.h's LDS selection (TkSel) with K = n_probe -- a segmented radix sort of rank_order_key where
//                     n_probe is beyond the selection's 1 024 slots, and no kernel at all where every non-empty list is probed;
//            fine     two forms, the same bits.  A pair's score is fmx_topk's chain and sum bit for bit, the selection is keyed by the
//                     ORIGINAL item id, and the exclusion list is searched for candidates that beat the threshold only.
//                       context  one workgroup per context walks its probed lists (the list-ordered rows are contiguous), TkSel<1, L>, and
//                                writes the K survivors under the link.  Good for few contexts.
//                       list     the (context, probe slot) pairs sorted by list; a workgroup takes one list and up to CT of the pairs that
//                                probe it -- topk_score_k's tile loop with the contexts gathered through the pairs -- and topk_merge_k merges
//                                a context's P lists.  A list is read once per tile instead of once per context.
//                     The rule: the context form -- the list form lost at every measured point (profiles/index.txt) and runs only
//                     where the test hook asks for it.
// The order is fmx_topk's, strict and total: the result is a function of the probe set alone, and the probe set of (g, l) alone.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <memory>
#include <vector>

#include "fm_prims.h"
#include "fm_rank.h"

namespace fmx {
namespace {

constexpr int IX_FB = 8;                        // components of an item's row a thread holds at a time (assign)
constexpr int IX_LG = 8;                        // lists per group of carried accumulators (assign)
constexpr int IX_ASSIGN_LDS = 48 * 1024;        // bytes of staged centroids per slice
constexpr int IX_CHUNK = 1024;                  // positions per chunk of a list's sums
constexpr int IX_SELECT_MAX = 1024;             // the most probes the LDS selection holds (top_k's limit: L <= 2048)
constexpr int64_t IX_COARSE_MAX = 1 << 24;      // (context, list) keys of one chunk of the sorted coarse form
constexpr int64_t IX_PARTIAL_MAX = 1 << 24;     // entries of the per-pair lists of one chunk of the list form (12 bytes each)
constexpr uint64_t IX_SEED_STREAM = 5;          // pair_hash's stream of the seed order

std::atomic<int> g_form{0};          // test hook (sticky): 0 the rule, 1 the context form, 2 the list form
std::atomic<int64_t> g_chunk{0};     //                     context rows per chunk
std::atomic<int> g_slice{0};         //                     lists per LDS slice of the assign kernel

// ---------------------------------------------------------------------------------------------------------------- build kernels

// a[i] = (s_i, base_i); fin[i] = 1 if all k + 1 components are finite
__global__ __launch_bounds__(TK_THREADS) void ix_aug_k(const double* __restrict__ s, const double* __restrict__ base, int64_t n, int k, double* __restrict__ aug,
                                                     uint32_t* __restrict__ fin) {
  const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (i >= n) return;
  const int D = k + 1;
  bool ok = true;
  for (int f = 0; f < D; ++f) {
    const double x = f < k ? s[i * k + f] : base[i];
    aug[i * D + f] = x;
    ok = ok && (x - x == 0.0);
  }
  fin[i] = ok ? 1u : 0u;
}

// the finite items, compacted in ascending order, with their hash keys
__global__ __launch_bounds__(TK_THREADS) void ix_seed_keys_k(const uint32_t* __restrict__ fin, const uint32_t* __restrict__ pos, int64_t n, uint64_t seed,
                                                           uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (i >= n || !fin[i]) return;
  key[pos[i]] = pair_hash(seed, 0, (uint64_t)i, IX_SEED_STREAM);
  val[pos[i]] = (uint32_t)i;
}

// centroid l = a bit copy of a of the l-th item of the seed order
__global__ __launch_bounds__(TK_THREADS) void ix_seed_copy_k(const double* __restrict__ aug, const uint32_t* __restrict__ order, int n_lists, int D,
                                                           double* __restrict__ cen) {
  const int64_t t = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (t >= (int64_t)n_lists * D) return;
  cen[t] = aug[(int64_t)order[t / D] * D + t % D];
}

// one item per thread against every centroid, staged in LDS `slice` lists at a time: mu is [slice rounded up to IX_LG][D rounded up to IX_FB],
// zero-padded (a padded component adds fma(0, 0, acc) = acc; a padded list is never compared)
__global__ __launch_bounds__(TK_THREADS) void ix_assign_k(const double* __restrict__ aug, const uint32_t* __restrict__ fin, int64_t n, int D,
                                                        const double* __restrict__ cen, int n_lists, int slice, uint32_t* __restrict__ assign) {
  extern __shared__ double mu[];
  const int DP = (D + IX_FB - 1) / IX_FB * IX_FB;
  const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  const bool live = i < n;
  const double* __restrict__ row = aug + (live ? i : 0) * D;
  double best = __builtin_inf();
  uint32_t bl = 0;
  for (int l0 = 0; l0 < n_lists; l0 += slice) {
    const int nl = n_lists - l0 < slice ? n_lists - l0 : slice;
    const int nlp = (nl + IX_LG - 1) / IX_LG * IX_LG;
    __syncthreads();  // the previous slice has been read
    for (int t = threadIdx.x; t < nlp * DP; t += TK_THREADS) {
      const int l = t / DP, f = t % DP;
      mu[t] = (l < nl && f < D) ? cen[(int64_t)(l0 + l) * D + f] : 0.0;
    }
    __syncthreads();
    if (live) {
      for (int g = 0; g < nlp; g += IX_LG) {
        double acc[IX_LG];
#pragma unroll
        for (int q = 0; q < IX_LG; ++q) acc[q] = 0.0;
        for (int f0 = 0; f0 < DP; f0 += IX_FB) {
          double x[IX_FB];
#pragma unroll
          for (int u = 0; u < IX_FB; ++u) x[u] = f0 + u < D ? row[f0 + u] : 0.0;
#pragma unroll
          for (int q = 0; q < IX_LG; ++q) {
            const double* __restrict__ m = mu + (g + q) * DP + f0;
#pragma unroll
            for (int u = 0; u < IX_FB; ++u) {
              const double t = x[u] - m[u];
              acc[q] = fma(t, t, acc[q]);  // f ascending: one chain per (item, list)
            }
          }
        }
#pragma unroll
        for (int q = 0; q < IX_LG; ++q)
          if (g + q < nl && acc[q] < best) { best = acc[q]; bl = (uint32_t)(l0 + g + q); }  // lists ascending: the first strictly lower one
      }
    }
  }
  if (live) assign[i] = fin[i] ? bl : 0u;
}

__global__ __launch_bounds__(TK_THREADS) void ix_iota_k(int64_t n, uint32_t* __restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}

// one workgroup per list: mu_l[f] = sum / cnt over the list's finite members, the sum in the stated order; a list without one keeps its bits
__global__ __launch_bounds__(TK_THREADS) void ix_update_k(const double* __restrict__ aug, const uint32_t* __restrict__ fin, int D, const int64_t* __restrict__ lp,
                                                        const int32_t* __restrict__ li, double* __restrict__ cen) {
  __shared__ double part[TK_THREADS / 64];
  __shared__ unsigned long long cnt_s;
  const int l = blockIdx.x;
  const int64_t a = lp[l], b = lp[l + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) cnt_s = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (int64_t q = a + threadIdx.x; q < b; q += TK_THREADS) mine += fin[li[q]];
  if (mine) atomicAdd(&cnt_s, mine);  // an integer count: its order is irrelevant
  __syncthreads();
  const unsigned long long cnt = cnt_s;
  if (cnt == 0) return;
  constexpr int64_t ROUND = (int64_t)(TK_THREADS / 64) * IX_CHUNK;  // one chunk per wave
  for (int f = 0; f < D; ++f) {
    double run = 0.0;
    for (int64_t c0 = a; c0 < b; c0 += ROUND) {
      const int64_t ca = c0 + (int64_t)wave * IX_CHUNK;
      const int64_t cb = ca + IX_CHUNK < b ? ca + IX_CHUNK : b;
      double s = 0.0;
      for (int64_t q = ca + lane; q < cb; q += 64) {
        const int64_t j = li[q];
        if (fin[j]) s = __dadd_rn(s, aug[j * D + f]);
      }
#pragma unroll
      for (int st = 32; st > 0; st >>= 1) s = __dadd_rn(s, __shfl_xor(s, st, 64));
      if (lane == 0) part[wave] = s;
      __syncthreads();
      if (threadIdx.x == 0)
        for (int w = 0; w < TK_THREADS / 64; ++w)
          if (c0 + (int64_t)w * IX_CHUNK < b) run = __dadd_rn(run, part[w]);  // chunk sums ascending
      __syncthreads();
    }
    if (threadIdx.x == 0) cen[(int64_t)l * D + f] = run / (double)cnt;
  }
}

// ---------------------------------------------------------------------------------------------------------------- search kernels

// rows of the list order: row q of the output is row li[q] of the input (16-byte pieces)
__global__ __launch_bounds__(TK_THREADS) void ix_gather_k(const float4* __restrict__ is, const double* __restrict__ ib, const int32_t* __restrict__ li, int64_t n,
                                                        int vecs, float4* __restrict__ os, double* __restrict__ ob) {
  const int per = vecs > 0 ? vecs : 1;  // (no factors: the bases alone)
  const int64_t t = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (t >= n * per) return;
  const int64_t q = t / per;
  const int v = (int)(t % per);
  const int64_t j = li[q];
  if (v < vecs) os[q * vecs + v] = is[j * vecs + v];
  if (v == 0) ob[q] = ib[j];
}

// the ids of the non-empty lists, ascending: ne[0 .. non_empty)
__global__ __launch_bounds__(TK_THREADS) void ix_nonempty_k(const int64_t* __restrict__ lp, int n_lists, const uint32_t* __restrict__ pos, int32_t* __restrict__ ne) {
  const int l = blockIdx.x * TK_THREADS + threadIdx.x;
  if (l < n_lists && lp[l + 1] > lp[l]) ne[pos[l]] = l;
}
__global__ __launch_bounds__(TK_THREADS) void ix_nonempty_flag_k(const int64_t* __restrict__ lp, int n_lists, uint32_t* __restrict__ flag) {
  const int l = blockIdx.x * TK_THREADS + threadIdx.x;
  if (l < n_lists) flag[l] = lp[l + 1] > lp[l] ? 1u : 0u;
}

__global__ __launch_bounds__(TK_THREADS) void ix_fill_i64_k(int64_t n, int64_t v, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (i < n) out[i] = v;
}

struct CoarseArgs {
  const void* cs;        // contexts of the chunk: s [nc][ks]
  int64_t nc;
  int ks, k;
  const double* cen;     // [n_lists][k + 1]
  const int64_t* lp;     // [n_lists + 1]
  int n_lists;
  int P;                 // probes per context: min(n_probe, non_empty)
  int32_t* probe;        // [nc][P]
  int64_t* scanned;      // [nc] or null
};

// g(c, l) of one context and one list: mu_l[k] + the fp64 chain over f = 0 .. k-1
template <typename T>
__device__ __forceinline__ double ix_coarse_score(const T* __restrict__ sc, const double* __restrict__ m, int k) {
  double acc = 0.0;
  for (int f = 0; f < k; ++f) acc = fma((double)sc[f], m[f], acc);
  return m[k] + acc;
}

// a tile of CT contexts, threads over the lists: each context's first P non-empty lists under rank_before on (g, l)
template <typename T, int CT, int L>
__global__ __launch_bounds__(TK_THREADS) void ix_coarse_k(CoarseArgs a) {
  constexpr int KSM = TK_KS_BYTES / sizeof(T);
  __shared__ TkSel<CT, L> q;
  __shared__ T sc[CT][KSM];  // widened where it is read: the same values as a widened copy

  const int P = a.P, ks = a.ks, k = a.k;
  const int64_t c0 = (int64_t)blockIdx.x * CT;
  const int nv = (int)(a.nc - c0 < CT ? a.nc - c0 : CT);
  const T* __restrict__ cs = reinterpret_cast<const T*>(a.cs);

  tk_init<CT, L>(q);
  for (int t = threadIdx.x; t < CT * ks; t += TK_THREADS) {
    const int c = t / ks, f = t % ks;
    sc[c][f] = c < nv ? cs[(c0 + c) * ks + f] : (T)0;
  }
  __syncthreads();

  double ts[CT];
  int32_t ti[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) { ts[c] = __builtin_nan(""); ti[c] = TK_NONE; }

  for (int l0 = 0; l0 < a.n_lists; l0 += TK_THREADS) {
    const int l = l0 + threadIdx.x;
    if (l < a.n_lists && a.lp[l + 1] > a.lp[l]) {
      const double* __restrict__ m = a.cen + (int64_t)l * (k + 1);
      double acc[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = 0.0;
      for (int f = 0; f < k; ++f) {
        const double mf = m[f];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = fma((double)sc[c][f], mf, acc[c]);  // f ascending: one chain per (context, list)
      }
      const double mk = m[k];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (c < nv) {
          const double g = mk + acc[c];
          if (rank_before(g, (int32_t)l, ts[c], ti[c])) tk_offer<CT, L>(q, P, c, g, (int32_t)l);
        }
      }
    }
    tk_round<CT, L>(q, P);
#pragma unroll
    for (int c = 0; c < CT; ++c) { ts[c] = q.s[c][P - 1]; ti[c] = q.i[c][P - 1]; }
  }
  tk_flush<CT, L>(q, P);
  for (int t = threadIdx.x; t < nv * P; t += TK_THREADS) {
    const int c = t / P, r = t % P;
    const int32_t l = q.i[c][r];
    a.probe[(c0 + c) * P + r] = l == TK_NONE ? -1 : l;
  }
  if (a.scanned && threadIdx.x < nv) {
    const int c = threadIdx.x;
    int64_t sum = 0;
    for (int r = 0; r < P; ++r) {
      const int32_t l = q.i[c][r];
      if (l != TK_NONE) sum += a.lp[l + 1] - a.lp[l];
    }
    a.scanned[c0 + c] = sum;
  }
}

// the sorted coarse form: key[c][j] = rank_order_key(g(c, ne[j])), val = ne[j]; segment c is sorted ascending (stable: equal g keep the lower list)
template <typename T>
__global__ __launch_bounds__(TK_THREADS) void ix_coarse_keys_k(const T* __restrict__ cs, int64_t nc, int ks, int k, const double* __restrict__ cen,
                                                             const int32_t* __restrict__ ne, int64_t n_ne, uint64_t* __restrict__ key, uint32_t* __restrict__ val,
                                                             int64_t* __restrict__ off) {
  const int64_t t = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (t <= nc) off[t] = t * n_ne;
  if (t >= nc * n_ne) return;
  const int64_t c = t / n_ne;
  const int32_t l = ne[t % n_ne];
  key[t] = rank_order_key(ix_coarse_score<T>(cs + c * ks, cen + (int64_t)l * (k + 1), k));
  val[t] = (uint32_t)l;
}
__global__ __launch_bounds__(TK_THREADS) void ix_coarse_take_k(const uint32_t* __restrict__ val, int64_t nc, int64_t n_ne, int P, const int64_t* __restrict__ lp,
                                                             int32_t* __restrict__ probe, int64_t* __restrict__ scanned) {
  const int64_t c = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (c >= nc) return;
  int64_t sum = 0;
  for (int r = 0; r < P; ++r) {
    const int32_t l = (int32_t)val[c * n_ne + r];
    probe[c * P + r] = l;
    sum += lp[l + 1] - lp[l];
  }
  if (scanned) scanned[c] = sum;
}

struct FineArgs {
  const void* cs;        // contexts of the chunk: s [nc][ks]
  const double* cb;      //                        base [nc] (w0 included)
  const void* ls;        // items in list order: s [ni][ks]
  const double* lb;      //                      base [ni] (no w0)
  const int32_t* li;     // position -> item
  const int64_t* lp;     // list -> positions
  const int32_t* probe;  // [nc][P], or one row for every context (pstride 0)
  int64_t pstride;
  int P;
  int ks, K;
  const int64_t* xrp;    // exclusion row offsets of the chunk's contexts [nc + 1] (absolute), or null
  int64_t xbase;
  const uint32_t* xs;
  Hyper h;
  int link;
  const double* pn_y;
  int64_t* oi;           // [nc][K]
  double* os;
};

// the context form: one workgroup per context over its probed lists
template <typename T, int L>
__global__ __launch_bounds__(TK_THREADS) void ix_fine_ctx_k(FineArgs a) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VN = StateVec<T>::N;
  constexpr int FB = 4 * VN;
  constexpr int KSM = TK_KS_BYTES / sizeof(T);
  __shared__ TkSel<1, L> q;
  __shared__ T sc[KSM];

  const int K = a.K, ks = a.ks;
  const int64_t c = blockIdx.x;
  const T* __restrict__ cs = reinterpret_cast<const T*>(a.cs);
  const T* __restrict__ ls = reinterpret_cast<const T*>(a.ls);
  tk_init<1, L>(q);
  for (int f = threadIdx.x; f < ks; f += TK_THREADS) sc[f] = cs[c * ks + f];
  const double bc = a.cb[c];
  const int64_t xa = a.xrp ? a.xrp[c] - a.xbase : 0, xb = a.xrp ? a.xrp[c + 1] - a.xbase : 0;
  const int32_t* __restrict__ probe = a.probe + c * a.pstride;
  __syncthreads();

  double ts = __builtin_nan("");
  int32_t ti = TK_NONE;
  for (int p = 0; p < a.P; ++p) {
    const int32_t l = probe[p];
    if (l < 0) continue;  // uniform
    const int64_t q0 = a.lp[l], q1 = a.lp[l + 1];
    for (int64_t qb = q0; qb < q1; qb += TK_THREADS) {
      const int64_t pos = qb + threadIdx.x;
      if (pos < q1) {
        T acc = (T)0;
        const vec_t* row = reinterpret_cast<const vec_t*>(ls + pos * ks);
        for (int f0 = 0; f0 < ks; f0 += FB) {
          vec_t v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = row[f0 / VN + u];
          const T* si = reinterpret_cast<const T*>(v);
#pragma unroll
          for (int f = 0; f < FB; ++f) acc = fma(sc[f0 + f], si[f], acc);  // fmx_topk's chain
        }
        const double s = (bc + a.lb[pos]) + (double)acc;
        const int32_t j = a.li[pos];
        if (rank_before(s, j, ts, ti) && !(xa < xb && tk_excluded(a.xs, xa, xb, (uint32_t)j))) tk_offer<1, L>(q, K, 0, s, j);
      }
      tk_round<1, L>(q, K);
      ts = q.s[0][K - 1]; ti = q.i[0][K - 1];
    }
  }
  tk_flush<1, L>(q, K);
  for (int r = threadIdx.x; r < K; r += TK_THREADS) {
    const int32_t j = q.i[0][r];
    const size_t o = (size_t)c * K + r;
    a.oi[o] = j == TK_NONE ? -1 : (int64_t)j;
    a.os[o] = j == TK_NONE ? __builtin_nan("") : rank_link(a.h, q.s[0][r], a.link, a.pn_y);
  }
}

// The list form.  The chunk's (context, probe slot) pairs e = c * P + p are sorted by their list; a workgroup (a "tile") takes one list and up
// to CT of the pairs that probe it: topk_score_k's tile loop with the tile's contexts gathered through the pairs and the slice being the list,
// so a list is read once per tile instead of once per context.  The tile's lists go to ps / pi [nc][P][K], row e: topk_merge_k with S = P
// merges them.
struct ListArgs {
  const void* cs;
  const double* cb;
  const void* ls;
  const double* lb;
  const int32_t* li;
  const int64_t* lp;
  int n_lists, P, ks, K;
  const uint32_t* pair;  // the pairs in list order
  const int64_t* poff;   // [n_lists + 1] list l's pairs are pair[poff[l] .. poff[l + 1])
  const int64_t* toff;   // [n_lists + 1] list l's tiles are toff[l] .. toff[l + 1]; toff[n_lists] = the tiles in all
  const int64_t* xrp;
  int64_t xbase;
  const uint32_t* xs;
  double* ps;
  int32_t* pi;
};

__global__ __launch_bounds__(TK_THREADS) void ix_pair_keys_k(const int32_t* __restrict__ probe, int64_t pstride, int P, int64_t n, uint32_t* __restrict__ key,
                                                           uint32_t* __restrict__ val) {
  const int64_t e = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (e >= n) return;
  key[e] = (uint32_t)probe[(e / P) * pstride + e % P];
  val[e] = (uint32_t)e;
}

// tcnt[l] = the tiles of list l (l < n_lists), 0 for the entry behind them: their exclusive sum is toff
__global__ __launch_bounds__(TK_THREADS) void ix_tile_counts_k(const int64_t* __restrict__ poff, int n_lists, int CT, int64_t* __restrict__ tcnt) {
  const int l = blockIdx.x * TK_THREADS + threadIdx.x;
  if (l > n_lists) return;
  tcnt[l] = l < n_lists ? (poff[l + 1] - poff[l] + CT - 1) / CT : 0;
}

template <typename T, int CT, int L>
__global__ __launch_bounds__(TK_THREADS) void ix_fine_list_k(ListArgs a) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VN = StateVec<T>::N;
  constexpr int FB = 4 * VN;
  constexpr int KSM = TK_KS_BYTES / sizeof(T);
  __shared__ TkSel<CT, L> q;
  __shared__ T sc[CT][KSM];
  __shared__ double bc[CT];
  __shared__ int64_t xa[CT], xb[CT];
  __shared__ uint32_t pe[CT];

  const int64_t w = blockIdx.x;
  if (w >= a.toff[a.n_lists]) return;  // the grid is an upper bound of the tiles (uniform)
  int lo = 0, hi = a.n_lists;          // the list of tile w: the last l with toff[l] <= w (a list without tiles shares its offset with the next one)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.toff[mid] <= w) lo = mid; else hi = mid;
  }
  const int l = lo;
  const int64_t e0 = a.poff[l] + (w - a.toff[l]) * CT;
  const int nv = (int)(a.poff[l + 1] - e0 < CT ? a.poff[l + 1] - e0 : CT);  // pairs of this tile
  const int K = a.K, ks = a.ks;
  const T* __restrict__ cs = reinterpret_cast<const T*>(a.cs);
  const T* __restrict__ ls = reinterpret_cast<const T*>(a.ls);

  tk_init<CT, L>(q);
  if (threadIdx.x < CT) {
    const int c = threadIdx.x;
    const uint32_t e = c < nv ? a.pair[e0 + c] : 0u;
    const int64_t ctx = e / (uint32_t)a.P;
    pe[c] = e;
    bc[c] = c < nv ? a.cb[ctx] : 0.0;
    xa[c] = (a.xrp && c < nv) ? a.xrp[ctx] - a.xbase : 0;
    xb[c] = (a.xrp && c < nv) ? a.xrp[ctx + 1] - a.xbase : 0;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < CT * ks; t += TK_THREADS) {
    const int c = t / ks, f = t % ks;
    sc[c][f] = c < nv ? cs[(int64_t)(pe[c] / (uint32_t)a.P) * ks + f] : (T)0;
  }
  __syncthreads();

  double ts[CT];
  int32_t ti[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) { ts[c] = __builtin_nan(""); ti[c] = TK_NONE; }

  const int64_t q0 = a.lp[l], q1 = a.lp[l + 1];
  for (int64_t qb = q0; qb < q1; qb += TK_THREADS) {
    const int64_t pos = qb + threadIdx.x;
    if (pos < q1) {
      T acc[CT];
#pragma unroll
      for (int c = 0; c < CT; ++c) acc[c] = (T)0;
      const vec_t* row = reinterpret_cast<const vec_t*>(ls + pos * ks);
      for (int f0 = 0; f0 < ks; f0 += FB) {
        vec_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = row[f0 / VN + u];
        const T* si = reinterpret_cast<const T*>(v);
#pragma unroll
        for (int c = 0; c < CT; ++c) {
#pragma unroll
          for (int f = 0; f < FB; ++f) acc[c] = fma(sc[c][f0 + f], si[f], acc[c]);  // fmx_topk's chain
        }
      }
      const double bi = a.lb[pos];
      const int32_t j = a.li[pos];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        if (c < nv) {
          const double s = (bc[c] + bi) + (double)acc[c];
          if (rank_before(s, j, ts[c], ti[c]) && !(xa[c] < xb[c] && tk_excluded(a.xs, xa[c], xb[c], (uint32_t)j))) tk_offer<CT, L>(q, K, c, s, j);
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
    const size_t o = (size_t)pe[c] * K + r;
    a.ps[o] = q.s[c][r];
    a.pi[o] = q.i[c][r];
  }
}

// ---------------------------------------------------------------------------------------------------------------- host side

struct IndexFree { void operator()(fmx_item_index* ix) const { index_free(ix); } };
using IndexPtr = std::unique_ptr<fmx_item_index, IndexFree>;

int index_alloc(int device, int64_t n, int n_lists, int k, IndexPtr* out) {
  IndexPtr ix(new fmx_item_index());
  ix->device = device; ix->n_items = n; ix->n_lists = n_lists; ix->k = k;
  FMX_HIP(hipMalloc((void**)&ix->centroid, (size_t)n_lists * (k + 1) * sizeof(double)));
  FMX_HIP(hipMalloc((void**)&ix->assign, (size_t)std::max<int64_t>(n, 1) * sizeof(uint32_t)));
  FMX_HIP(hipMalloc((void**)&ix->list_ptr, (size_t)(n_lists + 1) * sizeof(int64_t)));
  FMX_HIP(hipMalloc((void**)&ix->list_item, (size_t)std::max<int64_t>(n, 1) * sizeof(int32_t)));
  *out = std::move(ix);
  return FMX_OK;
}

// the lists of ix->assign: a stable sort of (list, item) and the offsets; kin / kout / vin are scratch of n_items words each
int index_lists(fmx_item_index* ix, Scratch& S, uint32_t* kin, uint32_t* kout, uint32_t* vin, bool host_copy) {
  const hipStream_t st = S.st;
  const int64_t n = ix->n_items;
  if (n > 0) {
    FMX_HIP(hipMemcpyAsync(kin, ix->assign, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(ix_iota_k, dim3(blocks(n, TK_THREADS)), dim3(TK_THREADS), 0, st, n, vin);
    FMX_HIP(hipGetLastError());
    FMX_TRY(sort_pairs(S, kin, kout, vin, (uint32_t*)ix->list_item, n, key_bits((uint64_t)ix->n_lists - 1)));  // item ids below 2^31: the same bits as int32
  }
  FMX_TRY(group_offsets(kout, n, ix->n_lists, ix->list_ptr, st));
  if (host_copy) {
    ix->h_list_ptr.resize((size_t)ix->n_lists + 1);
    FMX_HIP(hipMemcpyAsync(ix->h_list_ptr.data(), ix->list_ptr, ix->h_list_ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    ix->non_empty = 0;
    for (int l = 0; l < ix->n_lists; ++l) ix->non_empty += ix->h_list_ptr[(size_t)l + 1] > ix->h_list_ptr[(size_t)l];
  }
  return FMX_OK;
}

int assign_launch(const fmx_item_index* ix, hipStream_t st, const double* aug, const uint32_t* fin) {
  const int D = ix->k + 1, DP = (D + IX_FB - 1) / IX_FB * IX_FB;
  const int fit = std::max(IX_LG, IX_ASSIGN_LDS / (DP * (int)sizeof(double)) / IX_LG * IX_LG);  // whole accumulator groups
  int slice = g_slice.load();
  slice = slice > 0 ? std::min(slice, fit) : fit;
  slice = std::min(slice, ix->n_lists);
  const size_t lds = (size_t)((slice + IX_LG - 1) / IX_LG * IX_LG) * DP * sizeof(double);
  if (ix->n_items == 0) return FMX_OK;
  hipLaunchKernelGGL(ix_assign_k, dim3(blocks(ix->n_items, TK_THREADS)), dim3(TK_THREADS), lds, st, aug, fin, ix->n_items, D, (const double*)ix->centroid,
                     ix->n_lists, slice, ix->assign);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

template <typename T, int L>
int fine_ctx_launch(fmx_engine* e, const FineArgs& a, int64_t nc) {
  hipLaunchKernelGGL((ix_fine_ctx_k<T, L>), dim3((unsigned)nc), dim3(TK_THREADS), 0, e->stream, a);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

template <typename T>
int fine_ctx(fmx_engine* e, const FineArgs& a, int64_t nc) {
  switch (topk_slots(a.K)) {
    case 512: return fine_ctx_launch<T, 512>(e, a, nc);
    case 1024: return fine_ctx_launch<T, 1024>(e, a, nc);
    default: return fine_ctx_launch<T, 2048>(e, a, nc);
  }
}

// the list form of one chunk: `tiles` is an upper bound of the tile count (the kernel reads the true one)
template <typename T, int CT, int L>
int fine_list_launch(fmx_engine* e, const ListArgs& a, int64_t nc, int64_t tiles, int link, int64_t* oi, double* os) {
  hipLaunchKernelGGL((ix_fine_list_k<T, CT, L>), dim3((unsigned)tiles), dim3(TK_THREADS), 0, e->stream, a);
  FMX_HIP(hipGetLastError());
  hipLaunchKernelGGL((topk_merge_k<L>), dim3((unsigned)nc), dim3(TK_THREADS), 0, e->stream, (const double*)a.ps, (const int32_t*)a.pi, a.P, a.K, e->hyper, link,
                     (const double*)e->probit, oi, os);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

template <typename T>
int fine_list(fmx_engine* e, const ListArgs& a, int64_t nc, int64_t tiles, int link, int64_t* oi, double* os) {
  switch (topk_slots(a.K)) {
    case 512: return fine_list_launch<T, 8, 512>(e, a, nc, tiles, link, oi, os);
    case 1024: return fine_list_launch<T, 4, 1024>(e, a, nc, tiles, link, oi, os);
    default: return fine_list_launch<T, 2, 2048>(e, a, nc, tiles, link, oi, os);
  }
}

template <typename T, int CT, int L>
int coarse_launch(fmx_engine* e, const CoarseArgs& a) {
  hipLaunchKernelGGL((ix_coarse_k<T, CT, L>), dim3((unsigned)((a.nc + CT - 1) / CT)), dim3(TK_THREADS), 0, e->stream, a);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

template <typename T>
int coarse_select(fmx_engine* e, const CoarseArgs& a) {
  switch (topk_slots(a.P)) {
    case 512: return coarse_launch<T, 8, 512>(e, a);
    case 1024: return coarse_launch<T, 4, 1024>(e, a);
    default: return coarse_launch<T, 2, 2048>(e, a);
  }
}

template <typename T>
int topk_index_run_t(fmx_engine* e, const fmx_item_index* ix, const fmx_matrix* C, int64_t r0, int64_t r1, const fmx_matrix* I, const fmx_matrix* X, int K,
                     int n_probe, int link, int64_t* oi, double* os, int64_t* oscan) {
  const hipStream_t st = e->stream;
  const int kp = wide_state(e) ? e->kp64 : e->kp32;
  const int ks = state_factors<T>(e), k = e->k;
  FMX_CHECK(ks * (int)sizeof(T) <= TK_KS_BYTES, FMX_ERR_INVALID, "top-K scoring holds at most %d factors", TK_KS_BYTES / (int)sizeof(T));
  const int64_t ni = I->n, n_ne = ix->non_empty;
  const int P = (int)std::min<int64_t>(n_probe, n_ne);
  const bool all = P == n_ne;                        // every non-empty list: the probe set needs no scores
  const bool sorted = !all && P > IX_SELECT_MAX;     // beyond the LDS selection: the segmented sort

  int64_t chunk = std::min<int64_t>(r1 - r0, 1 << 15);
  if (sorted) chunk = std::max<int64_t>(1, std::min(chunk, IX_COARSE_MAX / n_ne));
  const int64_t hook_chunk = g_chunk.load();
  if (hook_chunk > 0) chunk = std::min(chunk, hook_chunk);
  // The form.  THE RULE (profiles/index.txt): the context form.  The first rule -- the list form when a chunk has at least
  // CT pairs per non-empty list on average -- was measured and lost at every point (the list form is 1.6 to 12 times slower at 100 000 contexts,
  // 1.1 to 1.4 times at 1 and 64), so the list form runs only where the hook asks for it.  It keeps a list of K entries per (context, probe
  // slot) pair: its chunk holds at most IX_PARTIAL_MAX of them
  const int CT = topk_tile(topk_slots(K));
  const bool by_list = g_form.load() == 2;
  if (by_list) chunk = std::max<int64_t>(1, std::min(chunk, IX_PARTIAL_MAX / ((int64_t)P * K)));

  Scratch scratch(st);
  Projections<T> pr;
  FMX_TRY(pr.reserve(scratch, ni, chunk, kp, ks));
  FMX_TRY(topk_project_rows(e, I, 0, ni, false, pr.q, ks, pr.ib, pr.is));  // the items, once per call: the engine's current parameters
  T* ls = nullptr;
  double* lb = nullptr;
  FMX_TRY(scratch.get(&ls, (size_t)ni * ks));
  FMX_TRY(scratch.get(&lb, (size_t)ni));
  const int vecs = ks * (int)sizeof(T) / 16;
  hipLaunchKernelGGL(ix_gather_k, dim3(blocks(ni * std::max(vecs, 1), TK_THREADS)), dim3(TK_THREADS), 0, st, (const float4*)pr.is, (const double*)pr.ib,
                     (const int32_t*)ix->list_item, ni, vecs, (float4*)ls, lb);
  FMX_HIP(hipGetLastError());

  int32_t *probe = nullptr, *ne = nullptr;
  FMX_TRY(scratch.get(&probe, all ? (size_t)P : (size_t)chunk * P));
  uint64_t *key_in = nullptr, *key_out = nullptr;
  uint32_t *val_in = nullptr, *val_out = nullptr;
  int64_t* off = nullptr;
  if (all || sorted) {
    uint32_t *flag = nullptr, *pos = nullptr;
    FMX_TRY(scratch.get(&flag, (size_t)ix->n_lists)); FMX_TRY(scratch.get(&pos, (size_t)ix->n_lists));
    hipLaunchKernelGGL(ix_nonempty_flag_k, dim3(blocks(ix->n_lists, TK_THREADS)), dim3(TK_THREADS), 0, st, (const int64_t*)ix->list_ptr, ix->n_lists, flag);
    FMX_HIP(hipGetLastError());
    FMX_TRY(exclusive_sum(scratch, (const uint32_t*)flag, pos, (int64_t)ix->n_lists));
    if (sorted) FMX_TRY(scratch.get(&ne, (size_t)n_ne));
    hipLaunchKernelGGL(ix_nonempty_k, dim3(blocks(ix->n_lists, TK_THREADS)), dim3(TK_THREADS), 0, st, (const int64_t*)ix->list_ptr, ix->n_lists,
                       (const uint32_t*)pos, all ? probe : ne);
    FMX_HIP(hipGetLastError());
  }
  if (sorted) {
    const size_t cnt = (size_t)chunk * n_ne;
    FMX_TRY(scratch.get(&key_in, cnt)); FMX_TRY(scratch.get(&key_out, cnt));
    FMX_TRY(scratch.get(&val_in, cnt)); FMX_TRY(scratch.get(&val_out, cnt));
    FMX_TRY(scratch.get(&off, (size_t)chunk + 1));
  }

  uint32_t *pk_in = nullptr, *pk_out = nullptr, *pv_in = nullptr, *pv_out = nullptr;
  int64_t *poff = nullptr, *tcnt = nullptr, *toff = nullptr;
  double* ps = nullptr;
  int32_t* pi = nullptr;
  if (by_list) {
    const size_t pairs = (size_t)chunk * P;
    FMX_TRY(scratch.get(&pk_in, pairs)); FMX_TRY(scratch.get(&pk_out, pairs)); FMX_TRY(scratch.get(&pv_in, pairs)); FMX_TRY(scratch.get(&pv_out, pairs));
    FMX_TRY(scratch.get(&poff, (size_t)ix->n_lists + 1)); FMX_TRY(scratch.get(&tcnt, (size_t)ix->n_lists + 1)); FMX_TRY(scratch.get(&toff, (size_t)ix->n_lists + 1));
    FMX_TRY(scratch.get(&ps, pairs * K)); FMX_TRY(scratch.get(&pi, pairs * K));
  }

  DevBuf xs;  // grows with the chunks' exclusion lists
  size_t xs_cap = 0;
  for (int64_t c = r0; c < r1; c += chunk) {
    const int64_t nc = std::min(chunk, r1 - c);
    FMX_TRY(topk_project_rows(e, C, c, c + nc, true, pr.q, ks, pr.cb, pr.cs));
    int64_t* scan = oscan ? oscan + (c - r0) : nullptr;
    if (all) {
      if (scan) {
        hipLaunchKernelGGL(ix_fill_i64_k, dim3(blocks(nc, TK_THREADS)), dim3(TK_THREADS), 0, st, nc, ni, scan);
        FMX_HIP(hipGetLastError());
      }
    } else if (sorted) {
      const int64_t cnt = nc * n_ne;
      hipLaunchKernelGGL((ix_coarse_keys_k<T>), dim3(blocks(std::max(cnt, nc + 1), TK_THREADS)), dim3(TK_THREADS), 0, st, (const T*)pr.cs, nc, ks, k,
                         (const double*)ix->centroid, (const int32_t*)ne, n_ne, key_in, val_in, off);
      FMX_HIP(hipGetLastError());
      FMX_TRY(scratch.with_temp([&](void* t, size_t& b) { return seg_sort_pairs(t, b, key_in, key_out, val_in, val_out, cnt, nc, off, st); }));
      hipLaunchKernelGGL(ix_coarse_take_k, dim3(blocks(nc, TK_THREADS)), dim3(TK_THREADS), 0, st, (const uint32_t*)val_out, nc, n_ne, P,
                         (const int64_t*)ix->list_ptr, probe, scan);
      FMX_HIP(hipGetLastError());
    } else {
      CoarseArgs ca{};
      ca.cs = pr.cs; ca.nc = nc; ca.ks = ks; ca.k = k; ca.cen = ix->centroid; ca.lp = ix->list_ptr; ca.n_lists = ix->n_lists; ca.P = P;
      ca.probe = probe; ca.scanned = scan;
      FMX_TRY(coarse_select<T>(e, ca));
    }
    FineArgs a{};
    a.cs = pr.cs; a.cb = pr.cb; a.ls = ls; a.lb = lb; a.li = ix->list_item; a.lp = ix->list_ptr;
    a.probe = probe; a.pstride = all ? 0 : P; a.P = P; a.ks = ks; a.K = K;
    a.h = e->hyper; a.link = link; a.pn_y = (const double*)e->probit;
    a.oi = oi + (c - r0) * K; a.os = os + (c - r0) * K;
    if (X) {
      int64_t xr[2];
      FMX_HIP(hipMemcpyAsync(&xr[0], X->row_ptr + c, sizeof(int64_t), hipMemcpyDeviceToHost, st));
      FMX_HIP(hipMemcpyAsync(&xr[1], X->row_ptr + c + nc, sizeof(int64_t), hipMemcpyDeviceToHost, st));
      FMX_HIP(hipStreamSynchronize(st));
      const size_t nx = (size_t)(xr[1] - xr[0]);
      if (nx > 0) {
        if (nx > xs_cap) {  // (the stream is drained: the previous chunk's kernels no longer read the old list)
          FMX_TRY(dev_buf(&xs, nx * sizeof(uint32_t)));
          xs_cap = nx;
        }
        FMX_TRY(topk_sort_excl(st, X->row_ptr + c, nc, X->col, xr[0], (uint32_t*)xs.get()));
        a.xrp = X->row_ptr + c; a.xbase = xr[0]; a.xs = (const uint32_t*)xs.get();
      }
    }
    if (!by_list) {
      FMX_TRY(fine_ctx<T>(e, a, nc));
      continue;
    }
    const int64_t pairs = nc * P;
    hipLaunchKernelGGL(ix_pair_keys_k, dim3(blocks(pairs, TK_THREADS)), dim3(TK_THREADS), 0, st, (const int32_t*)probe, a.pstride, P, pairs, pk_in, pv_in);
    FMX_HIP(hipGetLastError());
    FMX_TRY(sort_pairs(scratch, pk_in, pk_out, pv_in, pv_out, pairs, key_bits((uint64_t)ix->n_lists - 1)));
    FMX_TRY(group_offsets(pk_out, pairs, ix->n_lists, poff, st));
    hipLaunchKernelGGL(ix_tile_counts_k, dim3(blocks(ix->n_lists + 1, TK_THREADS)), dim3(TK_THREADS), 0, st, (const int64_t*)poff, ix->n_lists, CT, tcnt);
    FMX_HIP(hipGetLastError());
    FMX_TRY(exclusive_sum(scratch, (const int64_t*)tcnt, toff, (int64_t)ix->n_lists + 1));
    ListArgs la{};
    la.cs = a.cs; la.cb = a.cb; la.ls = a.ls; la.lb = a.lb; la.li = a.li; la.lp = a.lp;
    la.n_lists = ix->n_lists; la.P = P; la.ks = ks; la.K = K;
    la.pair = pv_out; la.poff = poff; la.toff = toff;
    la.xrp = a.xrp; la.xbase = a.xbase; la.xs = a.xs;
    la.ps = ps; la.pi = pi;
    // every list with pairs has at most one tile that is not full: pairs / CT + min(non-empty lists, pairs) bounds the tiles
    FMX_TRY(fine_list<T>(e, la, nc, pairs / CT + std::min<int64_t>(n_ne, pairs), link, a.oi, a.os));
  }
  FMX_HIP(hipStreamSynchronize(st));  // the exclusion list is freed on return
  return FMX_OK;
}

}  // namespace

int index_build_run(fmx_engine* e, const fmx_matrix* items, int n_lists, int n_iter, uint64_t seed, fmx_item_index** out) {
  const hipStream_t st = e->stream;
  const int64_t n = items->n;
  const int k = e->k, D = k + 1;
  Scratch S(st);
  double *base = nullptr, *s = nullptr, *aug = nullptr;
  uint32_t *fin = nullptr, *pos = nullptr, *kin = nullptr, *kout = nullptr, *vin = nullptr, *order = nullptr;
  uint64_t *hk = nullptr, *hko = nullptr;
  FMX_TRY(S.get(&base, (size_t)n)); FMX_TRY(S.get(&s, (size_t)n * k)); FMX_TRY(S.get(&aug, (size_t)n * D));
  FMX_TRY(S.get(&fin, (size_t)n)); FMX_TRY(S.get(&pos, (size_t)n));
  FMX_TRY(S.get(&kin, (size_t)n)); FMX_TRY(S.get(&kout, (size_t)n)); FMX_TRY(S.get(&vin, (size_t)n)); FMX_TRY(S.get(&order, (size_t)n));
  FMX_TRY(S.get(&hk, (size_t)n)); FMX_TRY(S.get(&hko, (size_t)n));
  FMX_TRY(project_run(e, items, 0, n, false, base, s));
  hipLaunchKernelGGL(ix_aug_k, dim3(blocks(n, TK_THREADS)), dim3(TK_THREADS), 0, st, (const double*)s, (const double*)base, n, k, aug, fin);
  FMX_HIP(hipGetLastError());
  FMX_TRY(exclusive_sum(S, (const uint32_t*)fin, pos, n));
  uint32_t last[2] = {0, 0};
  FMX_HIP(hipMemcpyAsync(&last[0], pos + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipMemcpyAsync(&last[1], fin + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  const int64_t nf = (int64_t)last[0] + last[1];
  FMX_CHECK(n_lists <= nf, FMX_ERR_INVALID, "n_lists must be at most the number of finite items (%lld of %lld; got %d)", (long long)nf, (long long)n, n_lists);

  IndexPtr ix;
  FMX_TRY(index_alloc(e->cfg.device, n, n_lists, k, &ix));
  // 1. seeds
  hipLaunchKernelGGL(ix_seed_keys_k, dim3(blocks(n, TK_THREADS)), dim3(TK_THREADS), 0, st, (const uint32_t*)fin, (const uint32_t*)pos, n, seed, hk, vin);
  FMX_HIP(hipGetLastError());
  FMX_TRY(sort_pairs(S, hk, hko, vin, order, nf, 64));
  hipLaunchKernelGGL(ix_seed_copy_k, dim3(blocks((int64_t)n_lists * D, TK_THREADS)), dim3(TK_THREADS), 0, st, (const double*)aug, (const uint32_t*)order, n_lists, D,
                     ix->centroid);
  FMX_HIP(hipGetLastError());
  // 2.-4. n_iter times (assign, update), then the final assign
  for (int it = 0; it < n_iter; ++it) {
    FMX_TRY(assign_launch(ix.get(), st, aug, fin));
    FMX_TRY(index_lists(ix.get(), S, kin, kout, vin, false));
    hipLaunchKernelGGL(ix_update_k, dim3((unsigned)n_lists), dim3(TK_THREADS), 0, st, (const double*)aug, (const uint32_t*)fin, D, (const int64_t*)ix->list_ptr,
                       (const int32_t*)ix->list_item, ix->centroid);
    FMX_HIP(hipGetLastError());
  }
  FMX_TRY(assign_launch(ix.get(), st, aug, fin));
  FMX_TRY(index_lists(ix.get(), S, kin, kout, vin, true));
  *out = ix.release();
  return FMX_OK;
}

int index_from_assign_run(fmx_engine* e, int64_t n, int n_lists, const uint32_t* assign, const double* centroid, fmx_item_index** out) {
  const hipStream_t st = e->stream;
  Scratch S(st);
  uint32_t *kin = nullptr, *kout = nullptr, *vin = nullptr;
  FMX_TRY(S.get(&kin, (size_t)n)); FMX_TRY(S.get(&kout, (size_t)n)); FMX_TRY(S.get(&vin, (size_t)n));
  IndexPtr ix;
  FMX_TRY(index_alloc(e->cfg.device, n, n_lists, e->k, &ix));
  if (n > 0) FMX_HIP(hipMemcpy(ix->assign, assign, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
  FMX_HIP(hipMemcpy(ix->centroid, centroid, (size_t)n_lists * (e->k + 1) * sizeof(double), hipMemcpyHostToDevice));
  FMX_TRY(index_lists(ix.get(), S, kin, kout, vin, true));
  *out = ix.release();
  return FMX_OK;
}

int index_export_run(const fmx_item_index* ix, double* centroid, uint32_t* assign, int64_t* list_ptr, int32_t* list_item) {
  if (centroid) FMX_HIP(hipMemcpy(centroid, ix->centroid, (size_t)ix->n_lists * (ix->k + 1) * sizeof(double), hipMemcpyDeviceToHost));
  if (assign && ix->n_items > 0) FMX_HIP(hipMemcpy(assign, ix->assign, (size_t)ix->n_items * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (list_ptr) std::copy(ix->h_list_ptr.begin(), ix->h_list_ptr.end(), list_ptr);
  if (list_item && ix->n_items > 0) FMX_HIP(hipMemcpy(list_item, ix->list_item, (size_t)ix->n_items * sizeof(int32_t), hipMemcpyDeviceToHost));
  return FMX_OK;
}

void index_free(fmx_item_index* ix) {
  if (!ix) return;
  (void)hipFree(ix->centroid); (void)hipFree(ix->assign); (void)hipFree(ix->list_ptr); (void)hipFree(ix->list_item);
  delete ix;
}

int topk_index_run(fmx_engine* e, const fmx_item_index* ix, const fmx_matrix* C, int64_t r0, int64_t r1, const fmx_matrix* I, const fmx_matrix* X, int K,
                   int n_probe, int link, int64_t* d_index, double* d_score, int64_t* d_scanned) {
  if (r1 <= r0) return FMX_OK;
  if (link == FMX_LINK_PROBIT) FMX_TRY(ensure_probit(e));
  if (ix->non_empty == 0) {  // nothing to rank: every slot is padding
    std::vector<int64_t> ni((size_t)(r1 - r0) * K, -1), nz((size_t)(r1 - r0), 0);
    std::vector<double> ns((size_t)(r1 - r0) * K, std::nan(""));
    FMX_HIP(hipMemcpy(d_index, ni.data(), ni.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    FMX_HIP(hipMemcpy(d_score, ns.data(), ns.size() * sizeof(double), hipMemcpyHostToDevice));
    if (d_scanned) FMX_HIP(hipMemcpy(d_scanned, nz.data(), nz.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    return FMX_OK;
  }
  return wide_state(e) ? topk_index_run_t<double>(e, ix, C, r0, r1, I, X, K, n_probe, link, d_index, d_score, d_scanned)
                       : topk_index_run_t<float>(e, ix, C, r0, r1, I, X, K, n_probe, link, d_index, d_score, d_scanned);
}

int debug_index_limits(int fine_form, int64_t chunk_rows, int assign_slice_lists) {
  FMX_CHECK(fine_form >= 0 && fine_form <= 2, FMX_ERR_INVALID, "fine_form must be 0 (the rule), 1 (context) or 2 (list) (got %d)", fine_form);
  g_form.store(fine_form);
  g_chunk.store(chunk_rows > 0 ? chunk_rows : 0);
  g_slice.store(assign_slice_lists > 0 ? assign_slice_lists : 0);
  return FMX_OK;
}

}  // namespace fmx
