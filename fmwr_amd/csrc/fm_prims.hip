// The query side's sorts and scans (fm_prims.h): the one query-side file that includes rocprim.  Every function hands rocprim the iterator
// types, the operator and the default configuration of the call it replaced in fm_rank.hip, fm_pairs.hip, fm_foldin.hip, fm_select.hip or
// fm_metrics.hip, so the device code is the code those files held, once (profiles/prims_refactor.txt).  Add an instantiation when a pipeline
// needs one, not before: each costs seconds of build time and hundreds of kilobytes.
#include <hip/hip_runtime.h>

#include <cstring>  // (rocprim's headers call memset)

#include <rocprim/rocprim.hpp>

#include "fm_prims.h"

namespace fmx {

// n <= 0: nothing to do (a size query answers 0); otherwise the rocprim call, in either of its phases
#define FMX_PRIM(n, call)                                  \
  do {                                                     \
    if ((n) <= 0) { if (!temp) bytes = 0; return FMX_OK; } \
    FMX_HIP(call);                                         \
    return FMX_OK;                                         \
  } while (0)

int sort_pairs(void* temp, size_t& bytes, uint64_t* k_in, uint64_t* k_out, uint32_t* v_in, uint32_t* v_out, int64_t n, int bits, hipStream_t st) {
  FMX_PRIM(n, rocprim::radix_sort_pairs(temp, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, bits, st));
}
int sort_pairs(void* temp, size_t& bytes, uint32_t* k_in, uint32_t* k_out, uint32_t* v_in, uint32_t* v_out, int64_t n, int bits, hipStream_t st) {
  FMX_PRIM(n, rocprim::radix_sort_pairs(temp, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, bits, st));
}
int sort_pairs(void* temp, size_t& bytes, const uint32_t* k_in, uint32_t* k_out, const int64_t* v_in, int64_t* v_out, int64_t n, int bits, hipStream_t st) {
  FMX_PRIM(n, rocprim::radix_sort_pairs(temp, bytes, k_in, k_out, v_in, v_out, (size_t)n, 0, bits, st));
}
int sort_keys(void* temp, size_t& bytes, uint64_t* k_in, uint64_t* k_out, int64_t n, int bits, hipStream_t st) {
  FMX_PRIM(n, rocprim::radix_sort_keys(temp, bytes, k_in, k_out, (size_t)n, 0, bits, st));
}
int seg_sort_pairs(void* temp, size_t& bytes, uint64_t* k_in, uint64_t* k_out, uint32_t* v_in, uint32_t* v_out, int64_t n, int64_t segments, int64_t* off,
                   hipStream_t st) {
  FMX_PRIM(n, rocprim::segmented_radix_sort_pairs(temp, bytes, k_in, k_out, v_in, v_out, (unsigned)n, (unsigned)segments, off, off + 1, 0, 64, st));
}
int exclusive_sum(void* temp, size_t& bytes, const uint32_t* in, uint32_t* out, int64_t n, hipStream_t st) {
  FMX_PRIM(n, rocprim::exclusive_scan(temp, bytes, in, out, (uint32_t)0, (size_t)n, rocprim::plus<uint32_t>(), st));
}
int exclusive_sum(void* temp, size_t& bytes, const int64_t* in, int64_t* out, int64_t n, hipStream_t st) {
  FMX_PRIM(n, rocprim::exclusive_scan(temp, bytes, in, out, (int64_t)0, (size_t)n, rocprim::plus<int64_t>(), st));
}
int exclusive_sum(void* temp, size_t& bytes, uint64_t* in, uint64_t* out, int64_t n, hipStream_t st) {
  FMX_PRIM(n, rocprim::exclusive_scan(temp, bytes, in, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), st));
}
int inclusive_sum(void* temp, size_t& bytes, uint32_t* in, uint32_t* out, int64_t n, hipStream_t st) {
  FMX_PRIM(n, rocprim::inclusive_scan(temp, bytes, in, out, (size_t)n, rocprim::plus<uint32_t>(), st));
}
int inclusive_sum(void* temp, size_t& bytes, int64_t* in, int64_t* out, int64_t n, hipStream_t st) {
  FMX_PRIM(n, rocprim::inclusive_scan(temp, bytes, in, out, (size_t)n, rocprim::plus<int64_t>(), st));
}
int inclusive_max(void* temp, size_t& bytes, const uint32_t* in, uint32_t* out, int64_t n, hipStream_t st) {
  FMX_PRIM(n, rocprim::inclusive_scan(temp, bytes, in, out, (size_t)n, rocprim::maximum<uint32_t>(), st));
}
#undef FMX_PRIM

namespace {
constexpr int PR_THREADS = 256;
__global__ __launch_bounds__(PR_THREADS) void group_offsets_k(const uint32_t* __restrict__ key, int64_t n, int64_t G, int64_t* __restrict__ off) {
  const int64_t g = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
  if (g > G) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)key[mid] < g) lo = mid + 1; else hi = mid;
  }
  off[g] = lo;
}
}  // namespace

int group_offsets(const uint32_t* keys, int64_t n, int64_t G, int64_t* off, hipStream_t st) {
  hipLaunchKernelGGL(group_offsets_k, dim3(blocks(G + 1, PR_THREADS)), dim3(PR_THREADS), 0, st, keys, n, G, off);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

}  // namespace fmx
