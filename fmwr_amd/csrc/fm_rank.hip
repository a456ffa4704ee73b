// The distinct-pairs pipeline of fm_heldout.hip and fm_lists.hip (DistinctPairs in fm_rank.h; DESIGN.md sections 12, 15 and 17).
//
// A chunk's entries arrive as keys (context << 32 | item) with their entry numbers as values:
//   distinct   a radix sort by key, a head flag per run of equal keys, an inclusive scan of the flags: sorted entry i belongs to distinct pair
//              pos[i] - 1.  The distinct keys are written out ascending, every entry learns its pair, the count is read back (the one host
//              synchronisation), and each context's run of pairs is found by binary search;
//   order      once the caller has scored the pairs: a stable segmented radix sort on the monotone key of the score, one segment per context.
// The sorts and the scan are fm_prims.hip's.  Sorts, a scan and per-element kernels with fixed outputs: nothing is ordered by atomics, the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fm_prims.h"

namespace fmx {
namespace {

constexpr int RK_THREADS = 256;

__global__ void rank_heads_k(const uint64_t* __restrict__ k, int64_t n, uint32_t* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x;
  if (e < n) flag[e] = (e == 0 || k[e] != k[e - 1]) ? 1u : 0u;
}

// sorted entry i is distinct pair pos[i] - 1: entry -> distinct pair, and the distinct keys
__global__ void rank_distinct_k(const uint64_t* __restrict__ k, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ pos, int64_t n,
                                uint64_t* __restrict__ dkey, uint32_t* __restrict__ e2d) {
  const int64_t e = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x;
  if (e >= n) return;
  const uint32_t d = pos[e] - 1;
  e2d[vals[e]] = d;
  if (e == 0 || k[e] != k[e - 1]) dkey[d] = k[e];
}

// off[c] = the first distinct pair of context c, c = 0 .. nc (off[nc] = nd)
__global__ void rank_offsets_k(const uint64_t* __restrict__ dkey, int64_t nd, int64_t nc, int64_t* __restrict__ off) {
  const int64_t c = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x;
  if (c > nc) return;
  const uint64_t key = (uint64_t)c << 32;
  int64_t lo = 0, hi = nd;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (dkey[mid] < key) lo = mid + 1; else hi = mid;
  }
  off[c] = lo;
}

}  // namespace

int DistinctPairs::reserve(Scratch& S, hipStream_t st, size_t max_entries, int64_t max_nc) {
  st_ = st;
  const size_t N = max_entries;
  FMX_TRY(S.get(&k_in, N)); FMX_TRY(S.get(&k_out, N)); FMX_TRY(S.get(&dkey, N));
  FMX_TRY(S.get(&v_in, N)); FMX_TRY(S.get(&v_out, N)); FMX_TRY(S.get(&flag_, N)); FMX_TRY(S.get(&pos_, N));
  FMX_TRY(S.get(&e2d, N)); FMX_TRY(S.get(&doff, (size_t)max_nc + 1));
  end_bit_ = ctx_key_bits(max_nc);
  size_t tb = 0;  // the temporary storage of the three sorts and scans, once per call for the largest chunk
  FMX_TRY(sort_pairs(nullptr, tb, k_in, k_out, v_in, v_out, (int64_t)N, end_bit_, st_)); tmax_ = tb;
  FMX_TRY(inclusive_sum(nullptr, tb, flag_, pos_, (int64_t)N, st_)); tmax_ = std::max(tmax_, tb);
  FMX_TRY(seg_sort_pairs(nullptr, tb, k_in, k_out, v_in, v_out, (int64_t)N, max_nc, doff, st_)); tmax_ = std::max(tmax_, tb);
  return S.temp(tmax_, &temp_);
}

int DistinctPairs::distinct(int64_t n, int64_t nc, int64_t* nd) {
  *nd = 0;
  if (n > 0) {
    size_t tb = tmax_;
    FMX_TRY(sort_pairs(temp_, tb, k_in, k_out, v_in, v_out, n, end_bit_, st_));
    hipLaunchKernelGGL(rank_heads_k, dim3(blocks(n, RK_THREADS)), dim3(RK_THREADS), 0, st_, k_out, n, flag_);
    tb = tmax_;
    FMX_TRY(inclusive_sum(temp_, tb, flag_, pos_, n, st_));
    hipLaunchKernelGGL(rank_distinct_k, dim3(blocks(n, RK_THREADS)), dim3(RK_THREADS), 0, st_, k_out, v_out, pos_, n, dkey, e2d);
    uint32_t h_nd = 0;
    FMX_HIP(hipMemcpyAsync(&h_nd, pos_ + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st_));
    FMX_HIP(hipStreamSynchronize(st_));
    *nd = h_nd;
  }
  hipLaunchKernelGGL(rank_offsets_k, dim3(blocks(nc + 1, RK_THREADS)), dim3(RK_THREADS), 0, st_, dkey, *nd, nc, doff);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

int DistinctPairs::order(int64_t nd, int64_t nc) {
  size_t tb = tmax_;
  return seg_sort_pairs(temp_, tb, k_in, k_out, v_in, v_out, nd, nc, doff, st_);
}

}  // namespace fmx
