// Negative sampling for FMX_TASK_RANKING (fmx_matrix_pairs): the pair matrix of sampled preference pairs.
//
//   1. positives   every entry of the positives matrix becomes the key (context << 32 | item); one radix sort orders them by context, then
//                  item, and a flag + scan + compaction keeps each (context, item) once.  A context's positives are then one sorted run
//                  P_c of the unique keys, found by a binary search per context;
//   2. negatives   pair t (= distinct positive u = t / n_neg, draw t % n_neg) draws r = mulhi(h, items - |P_c|) from a counter-based hash
//                  h of (seed, epoch, t): exactly uniform over the non-positives of c, no rejection.  The r-th non-positive is r + L, L the
//                  number of positives with P[idx] - idx <= r (P[idx] - idx non-positives lie below P[idx]): a binary search;
//   3. shuffle     a stable radix sort of the pair indices on a second 64-bit hash of (seed, epoch, t): equal keys keep index order;
//   4. rows        row lengths, an inclusive scan into row_ptr, then lane groups copy the context's and the item's entries (coalesced
//                  within a row), labels 1.  The flags (rows_sorted, unit_values, fixed_row_len, fields) are then computed from the
//                  rows themselves (check_rows_sorted), so they hold exactly where the concatenated rows satisfy them.
// Every stage is a sort, a scan or a per-element kernel with fixed outputs: no ordering by atomics, the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "fmx_internal.h"

namespace fmx {
namespace {

constexpr int PT = 256;
constexpr int GATHER_LANES = 16;  // lanes copying one output row

// splitmix64's finaliser, chained over the words of the counter
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
__device__ __forceinline__ uint64_t pair_hash(uint64_t seed, uint64_t epoch, uint64_t t, uint64_t stream) {
  uint64_t h = mix64(seed + 0x9E3779B97F4A7C15ull);
  h = mix64(h ^ (epoch * 0xD6E8FEB86659FD93ull + stream));
  return mix64(h ^ (t + 0x632BE59BD9B4E019ull));
}

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

__global__ void draw_k(const uint64_t* __restrict__ u, const int64_t* __restrict__ off, int64_t n_pairs, int n_neg, uint64_t n_items, uint64_t seed,
                       uint64_t epoch, uint32_t* __restrict__ pc, uint32_t* __restrict__ pi, uint32_t* __restrict__ pj, uint64_t* __restrict__ skey,
                       uint32_t* __restrict__ sidx) {
  const int64_t t = (int64_t)blockIdx.x * PT + threadIdx.x;
  if (t >= n_pairs) return;
  const uint64_t key = u[t / n_neg];
  const uint32_t c = (uint32_t)(key >> 32), i = (uint32_t)key;
  const int64_t b = off[c], m = off[c + 1] - b;
  const uint64_t avail = n_items - (uint64_t)m;  // >= 1: checked before the launch
  const uint64_t r = __umul64hi(pair_hash(seed, epoch, (uint64_t)t, 0), avail);
  int64_t lo = 0, hi = m;  // L = #{idx : P[idx] - idx <= r}
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((uint64_t)(uint32_t)u[b + mid] - (uint64_t)mid <= r) lo = mid + 1; else hi = mid;
  }
  pc[t] = c; pi[t] = i; pj[t] = (uint32_t)(r + (uint64_t)lo);
  skey[t] = pair_hash(seed, epoch, (uint64_t)t, 1);
  sidx[t] = (uint32_t)t;
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

struct Scratch {  // device allocations of one call, freed on every exit
  std::vector<void*> p;
  template <typename T>
  int get(T** out, size_t count) {
    void* q = nullptr;
    FMX_HIP(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    p.push_back(q);
    *out = (T*)q;
    return FMX_OK;
  }
  ~Scratch() {
    (void)hipDeviceSynchronize();
    for (void* q : p) (void)hipFree(q);
  }
};

inline unsigned blocks(int64_t n) { return (unsigned)((n + PT - 1) / PT); }

}  // namespace

int pairs_build(const fmx_matrix* C, const fmx_matrix* I, const fmx_matrix* X, int n_neg, uint64_t seed, int64_t epoch, fmx_matrix** out) {
  const hipStream_t st = nullptr;
  Scratch S;
  const int64_t nnz = X->nnz, n_ctx = X->n, n_items = I->n;
  // 1. the distinct positives, sorted by (context, item)
  uint64_t *k_in = nullptr, *k_out = nullptr, *flag = nullptr, *pos = nullptr, *u = nullptr;
  FMX_TRY(S.get(&k_in, nnz)); FMX_TRY(S.get(&k_out, nnz)); FMX_TRY(S.get(&flag, nnz)); FMX_TRY(S.get(&pos, nnz + 1));
  int end_bit = 33;
  while (end_bit < 64 && (1ll << (end_bit - 32)) < n_ctx) ++end_bit;
  size_t tb = 0, tmax = 0;
  void* temp = nullptr;
  FMX_HIP(rocprim::radix_sort_keys(nullptr, tb, k_in, k_out, (size_t)nnz, 0, end_bit, st)); tmax = tb > tmax ? tb : tmax;
  FMX_HIP(rocprim::exclusive_scan(nullptr, tb, flag, pos, (uint64_t)0, (size_t)nnz, rocprim::plus<uint64_t>(), st)); tmax = tb > tmax ? tb : tmax;
  uint8_t* temp_b = nullptr;
  FMX_TRY(S.get(&temp_b, tmax + 16));
  temp = temp_b;
  int64_t n_uniq = 0;
  if (nnz > 0) {
    hipLaunchKernelGGL(pos_keys_k, dim3(blocks(nnz)), dim3(PT), 0, st, X->row_ptr, n_ctx, X->col, nnz, k_in);
    tb = tmax;
    FMX_HIP(rocprim::radix_sort_keys(temp, tb, k_in, k_out, (size_t)nnz, 0, end_bit, st));
    hipLaunchKernelGGL(uniq_flags_k, dim3(blocks(nnz)), dim3(PT), 0, st, k_out, nnz, flag);
    tb = tmax;
    FMX_HIP(rocprim::exclusive_scan(temp, tb, flag, pos, (uint64_t)0, (size_t)nnz, rocprim::plus<uint64_t>(), st));
    uint64_t h[2] = {0, 0};
    FMX_HIP(hipMemcpyAsync(&h[0], pos + (nnz - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipMemcpyAsync(&h[1], flag + (nnz - 1), sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    n_uniq = (int64_t)(h[0] + h[1]);
  }
  FMX_TRY(S.get(&u, n_uniq));
  if (n_uniq > 0) hipLaunchKernelGGL(uniq_compact_k, dim3(blocks(nnz)), dim3(PT), 0, st, k_out, flag, pos, nnz, u);
  int64_t* off = nullptr;
  unsigned long long* bad = nullptr;
  FMX_TRY(S.get(&off, n_ctx + 1)); FMX_TRY(S.get(&bad, 1));
  FMX_HIP(hipMemsetAsync(bad, 0xFF, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(ctx_offsets_k, dim3(blocks(n_ctx + 1)), dim3(PT), 0, st, u, n_uniq, n_ctx, (uint64_t)n_items, off, bad);
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
    hipLaunchKernelGGL(draw_k, dim3(blocks(n_pairs)), dim3(PT), 0, st, u, off, n_pairs, n_neg, (uint64_t)n_items, seed, (uint64_t)epoch, pc, pi, pj, skey, sidx);
    size_t tb2 = 0, tb3 = 0;
    FMX_HIP(rocprim::radix_sort_pairs(nullptr, tb2, skey, skey_s, sidx, order, (size_t)n_pairs, 0, 64, st));
    FMX_HIP(rocprim::inclusive_scan(nullptr, tb3, lens, len + 1, (size_t)(2 * n_pairs), rocprim::plus<int64_t>(), st));
    uint8_t* temp2 = nullptr;
    FMX_TRY(S.get(&temp2, (tb2 > tb3 ? tb2 : tb3) + 16));
    FMX_HIP(rocprim::radix_sort_pairs(temp2, tb2, skey, skey_s, sidx, order, (size_t)n_pairs, 0, 64, st));  // stable: equal keys keep index order
    // 4. row lengths -> row_ptr
    FMX_HIP(hipMemsetAsync(len, 0, sizeof(int64_t), st));
    hipLaunchKernelGGL(row_lengths_k, dim3(blocks(n_pairs)), dim3(PT), 0, st, order, n_pairs, pc, pi, pj, C->row_ptr, I->row_ptr, oc, oi, oj, lens);
    FMX_HIP(rocprim::inclusive_scan(temp2, tb3, lens, len + 1, (size_t)(2 * n_pairs), rocprim::plus<int64_t>(), st));
    FMX_HIP(hipMemcpyAsync(&total, len + 2 * n_pairs, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
  }
  fmx_matrix* m = nullptr;
  FMX_TRY(alloc_matrix_public(C->device, 2 * n_pairs, C->p, total, true, &m));
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> keep(m, free_matrix);
  if (n_pairs > 0) {
    FMX_HIP(hipMemcpyAsync(m->row_ptr, len, (size_t)(2 * n_pairs + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    const int64_t threads = 2 * n_pairs * GATHER_LANES;
    hipLaunchKernelGGL(gather_rows_k, dim3(blocks(threads)), dim3(PT), 0, st, 2 * n_pairs, len, oc, oi, oj, C->row_ptr, C->col, C->val, I->row_ptr, I->col,
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
