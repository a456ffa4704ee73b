// Negative sampling for FMX_TASK_RANKING (fmx_matrix_pairs): the pair matrix of sampled preference pairs.
//
//   1. positives   every entry of the positives matrix becomes the key (context << 32 | item); one radix sort orders them by context, then
//                  item, and a flag + scan + compaction keeps each (context, item) once.  A context's positives are then one sorted run
//                  P_c of the unique keys, found by a binary search per context;
//   2. negatives   pair t (= distinct positive u = t / n_neg, draw t % n_neg) draws r = mulhi(h, items - |P_c|) from a counter-based hash
//                  h of (seed, epoch, t): exactly uniform over the non-positives of c, no rejection.  The r-th non-positive is r + L, L the
//                  number of positives with P[idx] - idx <= r (P[idx] - idx non-positives lie below P[idx]): a binary search;
//   2b. hard       fmx_matrix_pairs_hard only: candidate q of pair t is the same draw on hash stream 0 (q = 0: the
//                  negative of step 2) or q + 1; the candidate first in fmx_topk's order under the engine's score (its projections and
//                  tk_pair_score, bit for bit) replaces the negative.  Steps 1, 3 and 4 are shared;
//   3. shuffle     a stable radix sort of the pair indices on a second 64-bit hash of (seed, epoch, t): equal keys keep index order;
//   4. rows        row lengths, an inclusive scan into row_ptr, then lane groups copy the context's and the item's entries (coalesced
//                  within a row), labels 1.  The flags (rows_sorted, unit_values, fixed_row_len, fields) are then computed from the
//                  rows themselves (check_rows_sorted), so they hold exactly where the concatenated rows satisfy them.
// Every stage is a sort, a scan or a per-element kernel with fixed outputs: no ordering by atomics, the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <vector>

#include "fm_prims.h"

namespace fmx {
namespace {

constexpr int PT = 256;
constexpr int GATHER_LANES = 16;  // lanes copying one output row

__global__ void pos_keys_k(const int64_t* __restrict__ rp, int64_t n, const uint32_t* __restrict__ col, int64_t nnz, uint64_t* __restrict__ keys) {
  const int64_t e = (int64_t)blockIdx.x * PT + threadIdx.x;
  if (e >= nnz) return;
  int64_t lo = 0, hi = n;  // the row holding entry e: the last r with rp[r] <= e
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rp[mid] <= e) lo = mid; else hi = mid;
  }
  keys[e] = ((uint64_t)lo << 32) | col[e];
}

__global__ void uniq_flags_k(const uint64_t* __restrict__ k, int64_t nnz, uint64_t* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * PT + threadIdx.x;
  if (e < nnz) flag[e] = (e == 0 || k[e] != k[e - 1]) ? 1ull : 0ull;
}

__global__ void uniq_compact_k(const uint64_t* __restrict__ k, const uint64_t* __restrict__ flag, const uint64_t* __restrict__ pos, int64_t nnz,
                               uint64_t* __restrict__ u) {
  const int64_t e = (int64_t)blockIdx.x * PT + threadIdx.x;
  if (e < nnz && flag[e]) u[pos[e]] = k[e];
}

// off[c] = first unique key of context c (c = 0 .. n_ctx: off[n_ctx] = n_uniq); bad = the lowest context whose positives cover every item
__global__ void ctx_offsets_k(const uint64_t* __restrict__ u, int64_t n_uniq, int64_t n_ctx, uint64_t n_items, int64_t* __restrict__ off,
                              unsigned long long* __restrict__ bad) {
  const int64_t c = (int64_t)blockIdx.x * PT + threadIdx.x;
  if (c > n_ctx) return;
  const uint64_t key = (uint64_t)c << 32;
  int64_t lo = 0, hi = n_uniq;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (u[mid] < key) lo = mid + 1; else hi = mid;
  }
  off[c] = lo;
  if (c < n_ctx) {  // the count of context c from the next context's offset, searched again here (no cross-thread read)
    const uint64_t key2 = (uint64_t)(c + 1) << 32;
    int64_t lo2 = lo, hi2 = n_uniq;
    while (lo2 < hi2) {
      const int64_t mid = (lo2 + hi2) >> 1;
      if (u[mid] < key2) lo2 = mid + 1; else hi2 = mid;
    }
    if ((uint64_t)(lo2 - lo) >= n_items) atomicMin(bad, (unsigned long long)c);  // the minimum: the same context whatever the order
  }
}

// The draw of pair t on hash stream `stream` from the avail = items - m non-positives of a context whose m sorted positives are u[b, b + m):
// r = mulhi(h, avail) (draw_r), then the r-th non-positive r + L with L = #{idx : P[idx] - idx <= r} (draw_rank: the binary search on the
// caller's lo = 0, hi = m).  draw_k and the hard pass (draw_one) share both pieces, so candidate 0 is draw_k's negative by construction; draw_k
// spells out draw_one's three lines, which keeps its ISA exactly the sampler's of before the hard pass existed (profiles/isa_check.py).
__device__ __forceinline__ uint64_t draw_r(uint64_t seed, uint64_t epoch, uint64_t t, uint64_t stream, uint64_t avail) {
  return __umul64hi(pair_hash(seed, epoch, t, stream), avail);
}
__device__ __forceinline__ void draw_rank(const uint64_t* __restrict__ u, int64_t b, uint64_t r, int64_t& lo, int64_t& hi) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((uint64_t)(uint32_t)u[b + mid] - (uint64_t)mid <= r) lo = mid + 1; else hi = mid;
  }
}
__device__ __forceinline__ uint32_t draw_one(const uint64_t* __restrict__ u, int64_t b, int64_t m, uint64_t avail, uint64_t seed, uint64_t epoch,
                                             uint64_t t, uint64_t stream) {
  const uint64_t r = draw_r(seed, epoch, t, stream, avail);
  int64_t lo = 0, hi = m;
  draw_rank(u, b, r, lo, hi);
  return (uint32_t)(r + (uint64_t)lo);
}

__global__ void draw_k(const uint64_t* __restrict__ u, const int64_t* __restrict__ off, int64_t n_pairs, int n_neg, uint64_t n_items, uint64_t seed,
                       uint64_t epoch, uint32_t* __restrict__ pc, uint32_t* __restrict__ pi, uint32_t* __restrict__ pj, uint64_t* __restrict__ skey,
                       uint32_t* __restrict__ sidx) {
  const int64_t t = (int64_t)blockIdx.x * PT + threadIdx.x;
  if (t >= n_pairs) return;
  const uint64_t key = u[t / n_neg];
  const uint32_t c = (uint32_t)(key >> 32), i = (uint32_t)key;
  const int64_t b = off[c], m = off[c + 1] - b;
  const uint64_t avail = n_items - (uint64_t)m;  // >= 1: checked before the launch
  const uint64_t r = draw_r(seed, epoch, (uint64_t)t, 0, avail);
  int64_t lo = 0, hi = m;
  draw_rank(u, b, r, lo, hi);
  pc[t] = c; pi[t] = i; pj[t] = (uint32_t)(r + (uint64_t)lo);
  skey[t] = pair_hash(seed, epoch, (uint64_t)t, 1);
  sidx[t] = (uint32_t)t;
}

// tk_pair_score's arithmetic -- one fma chain in T over f = 0 .. ks - 1, then (bc + bi) + (double)acc -- with both rows read in 16-byte
// pieces, four of each in flight per block of FB factors, as topk_score_k reads an item row (ks is a multiple of FB; rows are 64-byte aligned)
template <typename T>
__device__ __forceinline__ double hn_pair_score(const T* __restrict__ sc, const T* __restrict__ si, int ks, double bc, double bi) {
  using vec_t = typename StateVec<T>::vec;
  constexpr int VN = StateVec<T>::N, FB = 4 * VN;
  const vec_t* __restrict__ rc = reinterpret_cast<const vec_t*>(sc);
  const vec_t* __restrict__ ri = reinterpret_cast<const vec_t*>(si);
  T acc = (T)0;
  for (int f0 = 0; f0 < ks; f0 += FB) {
    vec_t a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { a[u] = rc[f0 / VN + u]; b[u] = ri[f0 / VN + u]; }
    const T* x = reinterpret_cast<const T*>(a);
    const T* y = reinterpret_cast<const T*>(b);
#pragma unroll
    for (int f = 0; f < FB; ++f) acc = fma(x[f], y[f], acc);  // f ascending: the chain of tk_pair_score
  }
  return (bc + bi) + (double)acc;
}

// Hard negatives of pairs [t0, t1) (pre-shuffle order: the pairs of the projected contexts [c0, c0 + chunk)).  A lane group of G lanes (n_cand
// rounded up to a power of two; G divides the wave) per pair: lane q < n_cand draws candidate q (stream 0 for q = 0 -- draw_k's negative --,
// stream q + 1 above) and scores it with fmx_topk's arithmetic; the group's first candidate under the total order replaces pj[t].  The order is
// total, so the butterfly's association cannot change the winner; the padding lanes (NaN, index ~0) come after every candidate.
template <typename T>
__global__ __launch_bounds__(PT) void hard_choose_k(const uint64_t* __restrict__ u, const int64_t* __restrict__ off, int64_t t0, int64_t t1, int64_t c0,
                                                    int n_neg, int n_cand, int G, uint64_t n_items, uint64_t seed, uint64_t epoch,
                                                    const T* __restrict__ cs, const double* __restrict__ cb, const T* __restrict__ is,
                                                    const double* __restrict__ ib, int ks, uint32_t* __restrict__ pj) {
  const int64_t g = (int64_t)blockIdx.x * PT + threadIdx.x;
  const int64_t t = t0 + g / G;
  const int q = (int)(threadIdx.x & (G - 1));
  double s = __builtin_nan("");
  uint32_t j = 0xFFFFFFFFu;
  if (t < t1 && q < n_cand) {
    const uint64_t key = u[t / n_neg];
    const uint32_t c = (uint32_t)(key >> 32);
    const int64_t b = off[c], m = off[c + 1] - b;
    j = draw_one(u, b, m, n_items - (uint64_t)m, seed, epoch, (uint64_t)t, q == 0 ? 0 : (uint64_t)q + 1);
    const int64_t lc = (int64_t)c - c0;
    s = hn_pair_score<T>(cs + lc * ks, is + (int64_t)j * ks, ks, cb[lc], ib[j]);
  }
  for (int o = G >> 1; o > 0; o >>= 1) {  // every lane of the group takes part: no early exit above
    const double so = __shfl_xor(s, o, G);
    const uint32_t jo = (uint32_t)__shfl_xor((int)j, o, G);
    if (rank_before(so, jo, s, j)) { s = so; j = jo; }
  }
  if (t < t1 && q == 0) pj[t] = j;
}

// output pair s takes sampled pair order[s]: its (c, i, j) in output order and the lengths of rows 2s, 2s + 1
__global__ void row_lengths_k(const uint32_t* __restrict__ order, int64_t n_pairs, const uint32_t* __restrict__ pc, const uint32_t* __restrict__ pi,
                              const uint32_t* __restrict__ pj, const int64_t* __restrict__ crp, const int64_t* __restrict__ irp, uint32_t* __restrict__ oc,
                              uint32_t* __restrict__ oi, uint32_t* __restrict__ oj, int64_t* __restrict__ len) {
  const int64_t s = (int64_t)blockIdx.x * PT + threadIdx.x;
  if (s >= n_pairs) return;
  const uint32_t t = order[s];
  const uint32_t c = pc[t], i = pi[t], j = pj[t];
  oc[s] = c; oi[s] = i; oj[s] = j;
  const int64_t lc = crp[c + 1] - crp[c];
  len[2 * s] = lc + (irp[i + 1] - irp[i]);
  len[2 * s + 1] = lc + (irp[j + 1] - irp[j]);
}

__global__ __launch_bounds__(PT) void gather_rows_k(int64_t n_rows, const int64_t* __restrict__ orp, const uint32_t* __restrict__ oc,
                                                    const uint32_t* __restrict__ oi, const uint32_t* __restrict__ oj, const int64_t* __restrict__ crp,
                                                    const uint32_t* __restrict__ ccol, const float* __restrict__ cval, const int64_t* __restrict__ irp,
                                                    const uint32_t* __restrict__ icol, const float* __restrict__ ival, uint32_t* __restrict__ col,
                                                    float* __restrict__ val, float* __restrict__ y) {
  const int64_t r = ((int64_t)blockIdx.x * PT + threadIdx.x) / GATHER_LANES;
  const int lane = threadIdx.x % GATHER_LANES;
  if (r >= n_rows) return;
  const int64_t s = r >> 1;
  const uint32_t c = oc[s], it = (r & 1) ? oj[s] : oi[s];
  const int64_t dst = orp[r];
  const int64_t c0 = crp[c], lc = crp[c + 1] - c0;
  const int64_t i0 = irp[it], li = irp[it + 1] - i0;
  for (int64_t x = lane; x < lc; x += GATHER_LANES) { col[dst + x] = ccol[c0 + x]; val[dst + x] = cval[c0 + x]; }
  for (int64_t x = lane; x < li; x += GATHER_LANES) { col[dst + lc + x] = icol[i0 + x]; val[dst + lc + x] = ival[i0 + x]; }
  if (lane == 0) y[r] = 1.0f;
}

constexpr int64_t HN_CHUNK = 1 << 16;   // contexts projected per chunk of the hard pass
std::atomic<int64_t> g_hard_chunk_once{0};  // test hook: the next hard pass's chunk

// The hard pass, between the draws and the shuffle: the items' projection once, then per chunk of contexts that holds pairs, the chunk's
// projection (fmx_topk's own, topk_project_rows) and one choice launch over the chunk's contiguous pairs [off[c0] n_neg, off[c1] n_neg).
// Scratch: the two projections (and the projection's fp64 staging); nothing is kept per candidate.
template <typename T>
int hard_pass(fmx_engine* e, Scratch& S, const fmx_matrix* C, const fmx_matrix* I, const uint64_t* u, const int64_t* off, int64_t n_ctx, int n_neg,
              int n_cand, uint64_t seed, uint64_t epoch, uint32_t* pj) {
  const hipStream_t st = e->stream;
  const int kp = wide_state(e) ? e->kp64 : e->kp32;
  const int ks = state_factors<T>(e);
  const int64_t ni = I->n;
  const int64_t hook = g_hard_chunk_once.exchange(0);
  const int64_t chunk = std::max<int64_t>(1, std::min(n_ctx, hook > 0 ? std::min(hook, HN_CHUNK) : HN_CHUNK));
  std::vector<int64_t> h_off((size_t)n_ctx + 1);
  FMX_HIP(hipMemcpy(h_off.data(), off, (size_t)(n_ctx + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  FMX_HIP(hipDeviceSynchronize());  // the draws (null stream) have landed before the engine's stream overwrites their negatives
  Projections<T> pr;
  FMX_TRY(pr.reserve(S, ni, chunk, kp, ks));
  FMX_TRY(topk_project_rows(e, I, 0, ni, false, pr.q, ks, pr.ib, pr.is));
  int G = 1;
  while (G < n_cand) G <<= 1;
  for (int64_t c0 = 0; c0 < n_ctx; c0 += chunk) {
    const int64_t c1 = std::min(n_ctx, c0 + chunk);
    const int64_t t0 = h_off[(size_t)c0] * n_neg, t1 = h_off[(size_t)c1] * n_neg;
    if (t1 == t0) continue;
    FMX_TRY(topk_project_rows(e, C, c0, c1, true, pr.q, ks, pr.cb, pr.cs));
    hipLaunchKernelGGL((hard_choose_k<T>), dim3(blocks((t1 - t0) * G, PT)), dim3(PT), 0, st, u, off, t0, t1, c0, n_neg, n_cand, G, (uint64_t)ni, seed,
                       epoch, pr.cs, pr.cb, pr.is, pr.ib, ks, pj);
    FMX_HIP(hipGetLastError());
  }
  FMX_HIP(hipStreamSynchronize(st));  // the shuffle (null stream) reads the chosen negatives
  return FMX_OK;
}

}  // namespace

void debug_pairs_hard_chunk(int64_t contexts) { g_hard_chunk_once.store(contexts > 0 ? contexts : 0); }

int pairs_build(const fmx_matrix* C, const fmx_matrix* I, const fmx_matrix* X, int n_neg, uint64_t seed, int64_t epoch, fmx_matrix** out, fmx_engine* e,
                int n_cand) {
  const hipStream_t st = nullptr;
  Scratch S;  // drains the whole device before freeing: the null stream and the engine's are both in use
  const int64_t nnz = X->nnz, n_ctx = X->n, n_items = I->n;
  // 1. the distinct positives, sorted by (context, item)
  uint64_t *k_in = nullptr, *k_out = nullptr, *flag = nullptr, *pos = nullptr, *u = nullptr;
  FMX_TRY(S.get(&k_in, nnz)); FMX_TRY(S.get(&k_out, nnz)); FMX_TRY(S.get(&flag, nnz)); FMX_TRY(S.get(&pos, nnz + 1));
  int64_t n_uniq = 0;
  if (nnz > 0) {
    hipLaunchKernelGGL(pos_keys_k, dim3(blocks(nnz, PT)), dim3(PT), 0, st, X->row_ptr, n_ctx, X->col, nnz, k_in);
    FMX_TRY(sort_keys(S, k_in, k_out, nnz, ctx_key_bits(n_ctx)));
    hipLaunchKernelGGL(uniq_flags_k, dim3(blocks(nnz, PT)), dim3(PT), 0, st, k_out, nnz, flag);
    FMX_TRY(exclusive_sum(S, flag, pos, nnz));
    uint64_t h[2] = {0, 0};
    FMX_HIP(hipMemcpyAsync(&h[0], pos + (nnz - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipMemcpyAsync(&h[1], flag + (nnz - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    n_uniq = (int64_t)(h[0] + h[1]);
  }
  FMX_TRY(S.get(&u, n_uniq));
  if (n_uniq > 0) hipLaunchKernelGGL(uniq_compact_k, dim3(blocks(nnz, PT)), dim3(PT), 0, st, k_out, flag, pos, nnz, u);
  int64_t* off = nullptr;
  unsigned long long* bad = nullptr;
  FMX_TRY(S.get(&off, n_ctx + 1)); FMX_TRY(S.get(&bad, 1));
  FMX_HIP(hipMemsetAsync(bad, 0xFF, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(ctx_offsets_k, dim3(blocks(n_ctx + 1, PT)), dim3(PT), 0, st, u, n_uniq, n_ctx, (uint64_t)n_items, off, bad);
  unsigned long long h_bad = 0;
  FMX_HIP(hipMemcpyAsync(&h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  FMX_CHECK(h_bad == ~0ull, FMX_ERR_INVALID, "context %llu has every one of the %lld items as a positive: there is no negative to draw", h_bad, (long long)n_items);
  const int64_t n_pairs = n_uniq * (int64_t)n_neg;
  FMX_CHECK(n_pairs < (1LL << 32) - 1, FMX_ERR_INVALID, "%lld pairs: at most 2^32 - 2 per call (sample a slice of the contexts at a time)", (long long)n_pairs);

  // 2. negatives, 3. shuffle
  uint32_t *pc, *pi, *pj, *sidx, *order, *oc, *oi, *oj;
  uint64_t *skey, *skey_s;
  FMX_TRY(S.get(&pc, n_pairs)); FMX_TRY(S.get(&pi, n_pairs)); FMX_TRY(S.get(&pj, n_pairs)); FMX_TRY(S.get(&sidx, n_pairs)); FMX_TRY(S.get(&order, n_pairs));
  FMX_TRY(S.get(&oc, n_pairs)); FMX_TRY(S.get(&oi, n_pairs)); FMX_TRY(S.get(&oj, n_pairs));
  FMX_TRY(S.get(&skey, n_pairs)); FMX_TRY(S.get(&skey_s, n_pairs));
  int64_t *lens = nullptr, *len = nullptr;  // row lengths; len = row_ptr of the output (len[0] = 0, then their inclusive scan)
  FMX_TRY(S.get(&lens, 2 * n_pairs)); FMX_TRY(S.get(&len, 2 * n_pairs + 1));
  int64_t total = 0;
  if (n_pairs > 0) {
    hipLaunchKernelGGL(draw_k, dim3(blocks(n_pairs, PT)), dim3(PT), 0, st, u, off, n_pairs, n_neg, (uint64_t)n_items, seed, (uint64_t)epoch, pc, pi, pj, skey, sidx);
    if (e) {  // 2b. hard negatives: each pj[t] becomes the best of its n_cand candidates
      FMX_HIP(hipGetLastError());
      FMX_TRY(wide_state(e) ? hard_pass<double>(e, S, C, I, u, off, n_ctx, n_neg, n_cand, seed, (uint64_t)epoch, pj)
                            : hard_pass<float>(e, S, C, I, u, off, n_ctx, n_neg, n_cand, seed, (uint64_t)epoch, pj));
    }
    FMX_TRY(sort_pairs(S, skey, skey_s, sidx, order, n_pairs, 64));  // stable: equal keys keep index order
    // 4. row lengths -> row_ptr
    FMX_HIP(hipMemsetAsync(len, 0, sizeof(int64_t), st));
    hipLaunchKernelGGL(row_lengths_k, dim3(blocks(n_pairs, PT)), dim3(PT), 0, st, order, n_pairs, pc, pi, pj, C->row_ptr, I->row_ptr, oc, oi, oj, lens);
    FMX_TRY(inclusive_sum(S, lens, len + 1, 2 * n_pairs));
    FMX_HIP(hipMemcpyAsync(&total, len + 2 * n_pairs, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
  }
  fmx_matrix* m = nullptr;
  FMX_TRY(alloc_matrix(C->device, 2 * n_pairs, C->p, total, true, &m));
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> keep(m, free_matrix);
  if (n_pairs > 0) {
    FMX_HIP(hipMemcpyAsync(m->row_ptr, len, (size_t)(2 * n_pairs + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    const int64_t threads = 2 * n_pairs * GATHER_LANES;
    hipLaunchKernelGGL(gather_rows_k, dim3(blocks(threads, PT)), dim3(PT), 0, st, 2 * n_pairs, len, oc, oi, oj, C->row_ptr, C->col, C->val, I->row_ptr, I->col,
                       I->val, m->col, m->val, m->y);
  } else {
    FMX_HIP(hipMemsetAsync(m->row_ptr, 0, sizeof(int64_t), st));
  }
  FMX_HIP(hipGetLastError());
  FMX_HIP(hipStreamSynchronize(st));
  FMX_TRY(check_rows_sorted(m));  // the flags, from the rows as they are
  *out = keep.release();
  return FMX_OK;
}

}  // namespace fmx
