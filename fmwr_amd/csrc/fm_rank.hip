// The distinct-pairs pipeline of fm_heldout.hip and fm_lists.hip (DistinctPairs in fm_rank.h; DESIGN.md sections 12, 15 and 17).
//
// A chunk's entries arrive as keys (context << 32 | item) with their entry numbers as values:
//   distinct   a radix sort by key, a head flag per run of equal keys, an inclusive scan of the flags: sorted entry i belongs to distinct pair
//              pos[i] - 1.  The distinct keys are written out ascending, every entry learns its pair, the count is read back (the one host
//              synchronisation), and each context's run of pairs is found by binary search;
//   order      once the caller has scored the pairs: a stable segmented radix sort on the monotone key of the score, one segment per context.
// Sorts, a scan and per-element kernels with fixed outputs: nothing is ordered by atomics, the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "fm_rank.h"

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
  end_bit_ = 33;  // the key's bits in use: 32 of the item, and the context's
  while (end_bit_ < 64 && (1LL << (end_bit_ - 32)) < max_nc) ++end_bit_;
  size_t tb = 0;
  tmax_ = 0;
  if (N > 0) {  // the temporary storage of the three rocprim calls, once per call for the largest chunk
    FMX_HIP(rocprim::radix_sort_pairs(nullptr, tb, k_in, k_out, v_in, v_out, N, 0, end_bit_, st_)); tmax_ = std::max(tmax_, tb);
    FMX_HIP(rocprim::inclusive_scan(nullptr, tb, flag_, pos_, N, rocprim::plus<uint32_t>(), st_)); tmax_ = std::max(tmax_, tb);
    FMX_HIP(rocprim::segmented_radix_sort_pairs(nullptr, tb, k_in, k_out, v_in, v_out, (unsigned)N, (unsigned)max_nc, doff, doff + 1, 0, 64, st_));
    tmax_ = std::max(tmax_, tb);
  }
  FMX_TRY(S.get(&temp_, tmax_ + 16));
  return FMX_OK;
}

int DistinctPairs::distinct(int64_t n, int64_t nc, int64_t* nd) {
  *nd = 0;
  if (n > 0) {
    size_t tb = tmax_;
    FMX_HIP(rocprim::radix_sort_pairs(temp_, tb, k_in, k_out, v_in, v_out, (size_t)n, 0, end_bit_, st_));
    hipLaunchKernelGGL(rank_heads_k, dim3(blocks(n, RK_THREADS)), dim3(RK_THREADS), 0, st_, k_out, n, flag_);
    tb = tmax_;
    FMX_HIP(rocprim::inclusive_scan(temp_, tb, flag_, pos_, (size_t)n, rocprim::plus<uint32_t>(), st_));
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
  FMX_HIP(rocprim::segmented_radix_sort_pairs(temp_, tb, k_in, k_out, v_in, v_out, (unsigned)nd, (unsigned)nc, doff, doff + 1, 0, 64, st_));
  return FMX_OK;
}

}  // namespace fmx
