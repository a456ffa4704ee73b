// Column selection on the device: fmx_matrix_column_stats*, fmx_column_map_select*, fmx_column_map_hash*,
// fmx_matrix_remap_columns*.  One matrix derived from another along the columns, as fm_select.hip derives one along the rows.  The counts, the
// maps and the remapped matrix are integers and copied bits; every floating-point sum has one stated order.  tests/columns_model.py restates
// every output bit for bit.
//
//   stats    unit    a one-hot source whose rows ascend strictly (unit_values and rows_sorted: no column twice in a row): 64-bit integer atomics
//                    per entry, sum = sum_sq = (double) entries.  No sort.
//            sorted  everything else: a stable radix sort of (column, entry index) -- rows ascend inside a column's run and same-row duplicates
//                    are adjacent --, the run offsets by binary search (group_offsets), the heads of equal-row runs (and those of positive rows) counted by
//                    ONE 64-bit scan of the packed head flags: no atomics, so a column that every row holds costs what any other does.
//                    THE ORDER OF THE SUMS: a column's run is cut into chunks of COL_CHUNK = 1 024 positions; one wave sums a chunk: lane l adds
//                    the terms at positions l, l + 64, ... in that order from +0.0, the lanes meet in an xor butterfly (strides 32, 16, ..., 1:
//                    every lane holds the same bits); one thread per column adds its chunk sums ascending from +0.0.  A function of the column's
//                    own entry list alone.  On one-hot data every partial sum is a small integer: the same bits as the unit form.
//   select   a survivor flag per column, for the cap one 64-bit radix sort of (~count, id) and a kernel that clears the flags behind the cap, one
//            exclusive scan, one kernel for the map and one for the segments' new ranges.
//   hash     one kernel.
//   remap    the range check of the map (the lowest offending column comes back with the entry total in ONE read) and the new id of every entry.
//            KEEP   flags, one 64-bit scan, a row-pointer kernel and a scatter: split_entries_run's shape.
//            SUM / FIRST  a row's entries sorted by (new id << 32 | position in the row), dropped entries with an all-ones key last; the heads of
//                   equal-id runs; a head reduces its run in source order and writes it into a staging row at the SOURCE row's offset; then the
//                   head counts are scanned and the staging rows compacted.  Two forms write the same staging bits:
//                     group  rows of at most group_entries entries: a lane group of 16, 32 or 64 lanes, a bitonic network over __shfl_xor, the
//                            heads by comparing neighbours, the head lane walks its run through shuffles.  No barrier, no LDS.
//                     long   the other rows, gathered into a compact key array: seg_sort_pairs with the rows as segments, head flags, a scan,
//                            one thread per head.
//            The output goes through check_rows_sorted; no flag is copied from the source.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <vector>

#include "fm_prims.h"

namespace fmx {
namespace {

constexpr int CT = 256;
constexpr uint32_t COL_DROP = 0xFFFFFFFFu;
constexpr int COL_CHUNK = 1024;                  // positions per chunk of a column's sums
constexpr int COL_GROUP_MAX = 64;                // longest row of the lane-group form
constexpr int64_t COL_LAUNCH_ENTRIES = 1LL << 28;
constexpr int64_t COL_LAUNCH_ROWS = 1LL << 22;
constexpr int64_t COL_MAX_ITEMS = 0x7FFFFFFFLL;

std::atomic<int> g_group_entries{0};
std::atomic<int64_t> g_chunk_entries{0}, g_launch_rows{0};

struct ColLimits {
  int group_entries;       // rows of at most this many source entries take the lane-group form (< 0: none does, and stats never takes the unit form)
  int64_t chunk_entries;   // entries (sorted positions, output entries) per launch of a per-entry kernel
  int64_t launch_rows;     // rows, columns or chunks per launch of the other kernels
};
ColLimits col_limits() {
  ColLimits l;
  l.group_entries = g_group_entries.load();
  l.chunk_entries = g_chunk_entries.load();
  l.launch_rows = g_launch_rows.load();
  if (l.group_entries == 0 || l.group_entries > COL_GROUP_MAX) l.group_entries = COL_GROUP_MAX;
  if (l.chunk_entries <= 0) l.chunk_entries = COL_LAUNCH_ENTRIES;
  if (l.launch_rows <= 0) l.launch_rows = COL_LAUNCH_ROWS;
  return l;
}

// f(a, b) for the cuts [a, b) of [0, total) of at most `cut` items
template <typename F>
int in_cuts(int64_t total, int64_t cut, F f) {
  for (int64_t a = 0; a < total; a += cut) FMX_TRY(f(a, std::min(total, a + cut)));
  return FMX_OK;
}

// the row holding entry e: the last r in [0, n) with rp[r] <= e; with rows of L > 0 entries each, a division
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ rp, int64_t n, int64_t e, int L = 0) {
  if (L > 0) return e / L;
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rp[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(CT) void col_iota_k(int64_t N, uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (i < N) idx[i] = (uint32_t)i;
}

// ---------------------------------------------------------------------------------------------------------------------------- stats

// unit form: entries [e0, e1); count[3 c + {0, 1, 2}]
__global__ __launch_bounds__(CT) void cst_unit_k(const int64_t* __restrict__ rp, int64_t n, int L, const uint32_t* __restrict__ col, const float* __restrict__ y,
                                                int64_t e0, int64_t e1, unsigned long long* __restrict__ count) {
  const int64_t e = e0 + (int64_t)blockIdx.x * CT + threadIdx.x;
  if (e >= e1) return;
  const size_t c = col[e];
  atomicAdd(&count[3 * c], 1ull);
  atomicAdd(&count[3 * c + 1], 1ull);
  if (y && y[row_of(rp, n, e, L)] > 0.0f) atomicAdd(&count[3 * c + 2], 1ull);
}

__global__ __launch_bounds__(CT) void cst_unit_values_k(int64_t p, const int64_t* __restrict__ count, double* __restrict__ value) {
  const int64_t c = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (c >= p) return;
  const double s = (double)count[3 * c];
  value[2 * c] = s; value[2 * c + 1] = s;
}

// sorted form, positions [q0, q1) of the (column, entry) order: the head of an equal-row run as 1 in the low half of hf[q], a head whose row is
// positive as 1 in the high half too (one 64-bit scan counts both: a call holds fewer than 2^31 entries, so the low half never carries)
__global__ __launch_bounds__(CT) void cst_heads_k(const int64_t* __restrict__ rp, int64_t n, int L, const float* __restrict__ y, const uint32_t* __restrict__ cs,
                                                 const uint32_t* __restrict__ es, int64_t q0, int64_t q1, uint64_t* __restrict__ hf) {
  const int64_t q = q0 + (int64_t)blockIdx.x * CT + threadIdx.x;
  if (q >= q1) return;
  const uint32_t c = cs[q];
  const int64_t r = row_of(rp, n, (int64_t)es[q], L);
  uint64_t f = 0;
  if (!(q > 0 && cs[q - 1] == c && row_of(rp, n, (int64_t)es[q - 1], L) == r)) f = 1ull | ((y && y[r] > 0.0f) ? (1ull << 32) : 0ull);
  hf[q] = f;
}

// columns [0, p]: the counts of a column from its run [off[c], off[c + 1]) and the scanned head flags, and its chunks (nch[p] = 0: the scan ends
// in the total)
__global__ __launch_bounds__(CT) void cst_lens_k(int64_t p, const int64_t* __restrict__ off, const uint64_t* __restrict__ hs, int64_t* __restrict__ count,
                                                int64_t* __restrict__ nch) {
  const int64_t c = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (c > p) return;
  int64_t len = 0;
  if (c < p) {
    const int64_t a = off[c], b = off[c + 1];
    len = b - a;
    const uint64_t d = hs[b] - hs[a];   // both halves ascend along the scan: no borrow
    count[3 * c] = len; count[3 * c + 1] = (int64_t)(d & 0xFFFFFFFFull); count[3 * c + 2] = (int64_t)(d >> 32);
  }
  if (nch) nch[c] = (len + COL_CHUNK - 1) / COL_CHUNK;
}

// one wave per chunk w of [w0, w1): part[2 w + {0, 1}]
__global__ __launch_bounds__(CT) void cst_chunks_k(int64_t p, const int64_t* __restrict__ off, const int64_t* __restrict__ coff, const uint32_t* __restrict__ es,
                                                  const float* __restrict__ val, int64_t w0, int64_t w1, double* __restrict__ part) {
  const int64_t w = w0 + ((int64_t)blockIdx.x * CT + threadIdx.x) / 64;
  const int lane = threadIdx.x & 63;
  double s = 0.0, s2 = 0.0;
  if (w < w1) {
    int64_t lo = 0, hi = p;   // the column of chunk w: the last c with coff[c] <= w (a column without entries shares its offset with the next one)
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (coff[mid] <= w) lo = mid; else hi = mid;
    }
    const int64_t a = off[lo] + (w - coff[lo]) * COL_CHUNK;
    const int64_t b = a + COL_CHUNK < off[lo + 1] ? a + COL_CHUNK : off[lo + 1];
    for (int64_t q = a + lane; q < b; q += 64) {
      const double x = (double)val[es[q]];
      s = __dadd_rn(s, x);
      s2 = __dadd_rn(s2, __dmul_rn(x, x));
    }
  }
#pragma unroll
  for (int st = 32; st > 0; st >>= 1) {
    s = __dadd_rn(s, __shfl_xor(s, st, 64));
    s2 = __dadd_rn(s2, __shfl_xor(s2, st, 64));
  }
  if (w < w1 && lane == 0) { part[2 * w] = s; part[2 * w + 1] = s2; }
}

__global__ __launch_bounds__(CT) void cst_sums_k(int64_t p, const int64_t* __restrict__ coff, const double* __restrict__ part, double* __restrict__ value) {
  const int64_t c = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (c >= p) return;
  double s = 0.0, s2 = 0.0;
  for (int64_t w = coff[c]; w < coff[c + 1]; ++w) { s = __dadd_rn(s, part[2 * w]); s2 = __dadd_rn(s2, part[2 * w + 1]); }
  value[2 * c] = s; value[2 * c + 1] = s2;
}

// d_count i64[p][3], d_value f64[p][2] or null
int stats_run(const fmx_matrix* m, int64_t* d_count, double* d_value) {
  const hipStream_t st = nullptr;
  const ColLimits lim = col_limits();
  const int64_t p = m->p, n = m->n, nnz = m->nnz;
  if (p == 0) return FMX_OK;
  const float* y = m->has_labels ? m->y : nullptr;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(d_count);
  FMX_HIP(hipMemsetAsync(d_count, 0, (size_t)p * 3 * sizeof(int64_t), st));
  Scratch S;
  if (m->unit_values && m->rows_sorted && lim.group_entries >= 0) {
    FMX_TRY(in_cuts(nnz, lim.chunk_entries, [&](int64_t a, int64_t b) {
      hipLaunchKernelGGL(cst_unit_k, dim3(blocks(b - a, CT)), dim3(CT), 0, st, m->row_ptr, n, m->fixed_row_len, m->col, y, a, b, cnt);
      FMX_HIP(hipGetLastError());
      return FMX_OK;
    }));
    if (d_value) {
      hipLaunchKernelGGL(cst_unit_values_k, dim3(blocks(p, CT)), dim3(CT), 0, st, p, (const int64_t*)d_count, d_value);
      FMX_HIP(hipGetLastError());
    }
    FMX_HIP(hipStreamSynchronize(st));
    return FMX_OK;
  }
  uint32_t *cs = nullptr, *ei = nullptr, *es = nullptr;
  int64_t *off = nullptr, *nch = nullptr, *coff = nullptr;
  FMX_TRY(S.get(&cs, (size_t)nnz)); FMX_TRY(S.get(&ei, (size_t)nnz)); FMX_TRY(S.get(&es, (size_t)nnz));
  FMX_TRY(S.get(&off, (size_t)p + 1));
  if (nnz > 0) {
    hipLaunchKernelGGL(col_iota_k, dim3(blocks(nnz, CT)), dim3(CT), 0, st, nnz, ei);
    FMX_HIP(hipGetLastError());
    FMX_TRY(sort_pairs(S, const_cast<uint32_t*>(m->col), cs, ei, es, nnz, key_bits((uint64_t)p - 1)));   // stable: entry indices ascend in a run
  }
  FMX_TRY(group_offsets(cs, nnz, p, off, st));
  uint64_t *hf = nullptr, *hs = nullptr;
  FMX_TRY(S.get(&hf, (size_t)nnz + 1)); FMX_TRY(S.get(&hs, (size_t)nnz + 1));
  FMX_HIP(hipMemsetAsync(hf + nnz, 0, sizeof(uint64_t), st));
  FMX_TRY(in_cuts(nnz, lim.chunk_entries, [&](int64_t a, int64_t b) {
    hipLaunchKernelGGL(cst_heads_k, dim3(blocks(b - a, CT)), dim3(CT), 0, st, m->row_ptr, n, m->fixed_row_len, y, (const uint32_t*)cs, (const uint32_t*)es, a, b, hf);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }));
  FMX_TRY(exclusive_sum(S, hf, hs, nnz + 1));
  if (d_value) { FMX_TRY(S.get(&nch, (size_t)p + 1)); FMX_TRY(S.get(&coff, (size_t)p + 1)); }
  hipLaunchKernelGGL(cst_lens_k, dim3(blocks(p + 1, CT)), dim3(CT), 0, st, p, (const int64_t*)off, (const uint64_t*)hs, d_count, nch);
  FMX_HIP(hipGetLastError());
  if (d_value) {
    FMX_TRY(exclusive_sum(S, (const int64_t*)nch, coff, p + 1));
    int64_t chunks = 0;
    FMX_HIP(hipMemcpyAsync(&chunks, coff + p, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    double* part = nullptr;
    FMX_TRY(S.get(&part, (size_t)chunks * 2));
    FMX_TRY(in_cuts(chunks, lim.launch_rows, [&](int64_t a, int64_t b) {
      hipLaunchKernelGGL(cst_chunks_k, dim3(blocks((b - a) * 64, CT)), dim3(CT), 0, st, p, (const int64_t*)off, (const int64_t*)coff, (const uint32_t*)es,
                         (const float*)m->val, a, b, part);
      FMX_HIP(hipGetLastError());
      return FMX_OK;
    }));
    hipLaunchKernelGGL(cst_sums_k, dim3(blocks(p, CT)), dim3(CT), 0, st, p, (const int64_t*)coff, (const double*)part, d_value);
    FMX_HIP(hipGetLastError());
  }
  FMX_HIP(hipStreamSynchronize(st));
  return FMX_OK;
}

// --------------------------------------------------------------------------------------------------------------------------- select

struct RuleDev {
  int by_rows, bucket;
  int64_t min_count, max_count, max_features;
  uint32_t keep_prefix;
  int64_t nseg;
};

// columns [0, p]: the survivor flag (flag[p] = 0) and, for the cap, the key (~count, id) of a candidate -- all ones for every other column
__global__ __launch_bounds__(CT) void csel_flags_k(int64_t p, const int64_t* __restrict__ count, RuleDev ru, int64_t* __restrict__ flag, uint64_t* __restrict__ key) {
  const int64_t j = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (j > p) return;
  int64_t f = 0;
  uint64_t k = ~0ull;
  if (j < p) {
    const int64_t c = count[3 * j + (ru.by_rows ? 1 : 0)];
    if (j < (int64_t)ru.keep_prefix) f = 1;
    else if (c >= ru.min_count && (ru.max_count == 0 || c <= ru.max_count)) {
      f = 1;
      const uint64_t cc = c < 0 ? 0ull : (c > 0xFFFFFFFFLL ? 0xFFFFFFFFull : (uint64_t)c);
      k = ((uint64_t)(~(uint32_t)cc) << 32) | (uint64_t)j;
    }
  }
  flag[j] = f;
  if (key && j < p) key[j] = k;
}

// sorted positions [max_features, p): a candidate behind the cap does not survive
__global__ __launch_bounds__(CT) void csel_cap_k(int64_t p, int64_t cap, const uint64_t* __restrict__ ks, int64_t* __restrict__ flag) {
  const int64_t q = cap + (int64_t)blockIdx.x * CT + threadIdx.x;
  if (q >= p) return;
  const uint64_t k = ks[q];
  if (k != ~0ull) flag[(uint32_t)k] = 0;
}

// the segment of column j: the last s in [0, nseg) with base[s] <= j
__device__ __forceinline__ int64_t seg_of(const uint32_t* __restrict__ base, int64_t nseg, uint32_t j) {
  int64_t lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (base[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(CT) void csel_map_k(int64_t p, const int64_t* __restrict__ flag, const int64_t* __restrict__ pos, const uint32_t* __restrict__ base,
                                                RuleDev ru, uint32_t* __restrict__ map) {
  const int64_t j = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (j >= p) return;
  const int64_t s = seg_of(base, ru.nseg, (uint32_t)j);
  uint32_t v = COL_DROP;
  if (flag[j]) v = (uint32_t)(pos[j] + (ru.bucket ? s : 0));
  else if (ru.bucket) v = (uint32_t)(pos[base[s + 1]] + s);
  map[j] = v;
}

__global__ __launch_bounds__(CT) void csel_segs_k(const int64_t* __restrict__ pos, const uint32_t* __restrict__ base, RuleDev ru, uint32_t* __restrict__ nsb) {
  const int64_t s = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (s <= ru.nseg) nsb[s] = (uint32_t)(pos[base[s]] + (ru.bucket ? s : 0));
}

// every refusal of a rule; host only.  base: the segments' bases (the rule's, or {0, p})
int check_select(int64_t p, const void* count, const fmx_column_rule* ru, const void* map, const uint32_t* new_p, std::vector<uint32_t>* base) {
  FMX_CHECK(ru != nullptr, FMX_ERR_INVALID, "rule is NULL");
  FMX_CHECK(ru->struct_size == sizeof(fmx_column_rule), FMX_ERR_INVALID, "rule.struct_size does not match this library");
  FMX_CHECK(ru->by == FMX_COLUMNS_BY_ROWS || ru->by == FMX_COLUMNS_BY_ENTRIES, FMX_ERR_INVALID, "unknown rule.by %d", (int)ru->by);
  FMX_CHECK(ru->rare == FMX_RARE_DROP || ru->rare == FMX_RARE_BUCKET, FMX_ERR_INVALID, "unknown rule.rare %d", (int)ru->rare);
  FMX_CHECK(ru->min_count >= 0 && ru->max_count >= 0 && ru->max_features >= 0, FMX_ERR_INVALID, "min_count, max_count and max_features must not be negative");
  FMX_CHECK(ru->reserved == 0, FMX_ERR_INVALID, "rule.reserved must be 0");
  FMX_CHECK((int64_t)ru->keep_prefix <= p, FMX_ERR_INVALID, "keep_prefix %u is above the feature count %lld", ru->keep_prefix, (long long)p);
  FMX_CHECK(ru->n_segments >= 0 && (ru->n_segments == 0 || ru->segment_base != nullptr), FMX_ERR_INVALID, "n_segments is negative or segment_base is NULL");
  FMX_CHECK(p + std::max<int64_t>(ru->n_segments, 1) <= 0xFFFFFFFELL, FMX_ERR_INVALID, "the features and the segments' buckets do not fit 32-bit ids");
  FMX_CHECK((count != nullptr && map != nullptr) || p == 0, FMX_ERR_INVALID, "the count table or the map is NULL");
  FMX_CHECK(new_p != nullptr, FMX_ERR_INVALID, "new_p is NULL");
  if (ru->n_segments == 0) { base->assign({0u, (uint32_t)p}); return FMX_OK; }
  const uint32_t* b = ru->segment_base;
  FMX_CHECK(b[0] == 0 && (int64_t)b[ru->n_segments] == p, FMX_ERR_INVALID, "segment_base must start at 0 and end at the feature count");
  for (int32_t s = 0; s < ru->n_segments; ++s) FMX_CHECK(b[s] <= b[s + 1], FMX_ERR_INVALID, "segment_base descends at segment %d", (int)s);
  base->assign(b, b + ru->n_segments + 1);
  return FMX_OK;
}

int select_run(int64_t p, const int64_t* d_count, const fmx_column_rule& r, const std::vector<uint32_t>& base, uint32_t* d_map, std::vector<uint32_t>* nsb) {
  const hipStream_t st = nullptr;
  const RuleDev ru{r.by == FMX_COLUMNS_BY_ROWS, r.rare == FMX_RARE_BUCKET, r.min_count, r.max_count, r.max_features, r.keep_prefix, (int64_t)base.size() - 1};
  Scratch S;
  int64_t *flag = nullptr, *pos = nullptr;
  uint32_t *dbase = nullptr, *dnsb = nullptr;
  uint64_t *key = nullptr, *ks = nullptr;
  FMX_TRY(S.get(&flag, (size_t)p + 1)); FMX_TRY(S.get(&pos, (size_t)p + 1));
  FMX_TRY(S.get(&dbase, base.size())); FMX_TRY(S.get(&dnsb, base.size()));
  FMX_HIP(hipMemcpyAsync(dbase, base.data(), base.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  const bool cap = ru.max_features > 0 && ru.max_features < p;
  if (cap) { FMX_TRY(S.get(&key, (size_t)p)); FMX_TRY(S.get(&ks, (size_t)p)); }
  hipLaunchKernelGGL(csel_flags_k, dim3(blocks(p + 1, CT)), dim3(CT), 0, st, p, d_count, ru, flag, key);
  FMX_HIP(hipGetLastError());
  if (cap) {
    FMX_TRY(sort_keys(S, key, ks, p, 64));
    hipLaunchKernelGGL(csel_cap_k, dim3(blocks(p - ru.max_features, CT)), dim3(CT), 0, st, p, ru.max_features, (const uint64_t*)ks, flag);
    FMX_HIP(hipGetLastError());
  }
  FMX_TRY(exclusive_sum(S, (const int64_t*)flag, pos, p + 1));
  if (p > 0) {
    hipLaunchKernelGGL(csel_map_k, dim3(blocks(p, CT)), dim3(CT), 0, st, p, (const int64_t*)flag, (const int64_t*)pos, (const uint32_t*)dbase, ru, d_map);
    FMX_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(csel_segs_k, dim3(blocks(ru.nseg + 1, CT)), dim3(CT), 0, st, (const int64_t*)pos, (const uint32_t*)dbase, ru, dnsb);
  FMX_HIP(hipGetLastError());
  nsb->resize(base.size());
  FMX_HIP(hipMemcpyAsync(nsb->data(), dnsb, base.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  return FMX_OK;
}

// ----------------------------------------------------------------------------------------------------------------------------- hash

__global__ __launch_bounds__(CT) void chash_k(int64_t p, uint32_t n_buckets, uint64_t seed, uint64_t salt, uint32_t keep_prefix, uint32_t* __restrict__ map) {
  const int64_t j = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (j >= p) return;
  map[j] = j < (int64_t)keep_prefix ? (uint32_t)j : keep_prefix + (uint32_t)__umul64hi(pair_hash(seed, salt, (uint64_t)j, 4), (uint64_t)n_buckets);
}

int check_hash(int64_t p, uint32_t n_buckets, uint32_t keep_prefix, const void* map, const uint32_t* new_p) {
  FMX_CHECK(n_buckets >= 1, FMX_ERR_INVALID, "n_buckets must be at least 1");
  FMX_CHECK((int64_t)keep_prefix <= p, FMX_ERR_INVALID, "keep_prefix %u is above the feature count %lld", keep_prefix, (long long)p);
  FMX_CHECK((uint64_t)keep_prefix + n_buckets <= 0xFFFFFFFEull, FMX_ERR_INVALID, "keep_prefix + n_buckets does not fit a 32-bit id");
  FMX_CHECK(map != nullptr || p == 0, FMX_ERR_INVALID, "the map is NULL");
  FMX_CHECK(new_p != nullptr, FMX_ERR_INVALID, "new_p is NULL");
  return FMX_OK;
}

int hash_run(int64_t p, uint32_t n_buckets, uint64_t seed, uint64_t salt, uint32_t keep_prefix, uint32_t* d_map) {
  if (p > 0) {
    hipLaunchKernelGGL(chash_k, dim3(blocks(p, CT)), dim3(CT), 0, nullptr, p, n_buckets, seed, salt, keep_prefix, d_map);
    FMX_HIP(hipGetLastError());
    FMX_HIP(hipStreamSynchronize(nullptr));
  }
  return FMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------- remap

// the lowest column whose map value is neither below new_p nor COL_DROP into *bad
__global__ __launch_bounds__(CT) void crm_check_k(int64_t p, const uint32_t* __restrict__ map, uint32_t new_p, unsigned long long* __restrict__ bad) {
  const int64_t j = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (j >= p) return;
  const uint32_t v = map[j];
  if (v != COL_DROP && v >= new_p) atomicMin(bad, (unsigned long long)j);   // the minimum: the same column whatever the order
}

// entries [e0, e1): the new id of every entry and, for KEEP, the kept flag
__global__ __launch_bounds__(CT) void crm_ids_k(const uint32_t* __restrict__ col, const uint32_t* __restrict__ map, int64_t e0, int64_t e1, uint32_t* __restrict__ nid,
                                               int64_t* __restrict__ flag) {
  const int64_t e = e0 + (int64_t)blockIdx.x * CT + threadIdx.x;
  if (e >= e1) return;
  const uint32_t v = map[col[e]];
  nid[e] = v;
  if (flag) flag[e] = v != COL_DROP ? 1 : 0;
}

__global__ __launch_bounds__(CT) void crm_keep_ptrs_k(const int64_t* __restrict__ rp, int64_t n, const int64_t* __restrict__ kpos, int64_t* __restrict__ orp) {
  const int64_t r = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (r <= n) orp[r] = kpos[rp[r]];
}

__global__ __launch_bounds__(CT) void crm_keep_scatter_k(int64_t e0, int64_t e1, const uint32_t* __restrict__ nid, const int64_t* __restrict__ kpos,
                                                        const uint32_t* __restrict__ val, uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval) {
  const int64_t e = e0 + (int64_t)blockIdx.x * CT + threadIdx.x;
  if (e >= e1) return;
  const uint32_t v = nid[e];
  if (v == COL_DROP) return;
  const int64_t k = kpos[e];
  ocol[k] = v; oval[k] = val[e];
}

// the merged value of a run: SUM rounds the fp64 sum once to fp32, FIRST keeps the first entry's bits
__device__ __forceinline__ uint32_t crm_value(int first, uint32_t first_bits, double acc) { return first ? first_bits : __float_as_uint((float)acc); }

// group form: G lanes per row of [r0, r1); rows longer than glim are left to the long form.  Writes the merged row into the staging arrays at the
// source row's offset and its length into cnt[r].  No lane leaves before the last shuffle.
template <int G>
__global__ __launch_bounds__(CT) void crm_group_k(const int64_t* __restrict__ rp, int64_t r0, int64_t r1, int glim, const uint32_t* __restrict__ nid,
                                                 const uint32_t* __restrict__ val, int first, uint32_t* __restrict__ scol, uint32_t* __restrict__ sval,
                                                 int64_t* __restrict__ cnt) {
  const int64_t r = r0 + ((int64_t)blockIdx.x * CT + threadIdx.x) / G;
  const int lane = threadIdx.x & (G - 1);
  int64_t a = 0;
  int len = 0;
  bool active = false;
  if (r < r1) {
    a = rp[r];
    const int64_t l = rp[r + 1] - a;
    active = l <= (int64_t)glim;
    len = active ? (int)l : 0;
  }
  uint64_t key = ~0ull;
  if (lane < len) {
    const uint32_t v = nid[a + lane];
    if (v != COL_DROP) key = ((uint64_t)v << 32) | (uint64_t)lane;
  }
#pragma unroll
  for (int size = 2; size <= G; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const uint64_t other = __shfl_xor(key, stride, G);
      const bool take_min = ((lane & size) == 0) == ((lane & stride) == 0);
      const uint64_t lo = key < other ? key : other, hi = key < other ? other : key;
      key = take_min ? lo : hi;
    }
  }
  const uint64_t prev = __shfl_up(key, 1, G);
  const uint32_t id = (uint32_t)(key >> 32);
  const bool valid = key != ~0ull;
  const bool head = valid && (lane == 0 || (uint32_t)(prev >> 32) != id);
  const uint64_t ballot = __ballot(head);
  const int shift = (threadIdx.x & 63) & ~(G - 1);
  const uint64_t mine = G == 64 ? ballot : ((ballot >> shift) & ((1ull << (G & 63)) - 1ull));
  const int rank = __popcll(mine & ((1ull << lane) - 1ull));
  uint32_t first_bits = 0;
  double acc = 0.0;
  if (head) {
    first_bits = val[a + (uint32_t)key];
    acc = (double)__uint_as_float(first_bits);
  }
  bool running = head;
  for (int d = 1; d < G; ++d) {
    const uint64_t k = __shfl_down(key, d, G);
    running = running && lane + d < G && k != ~0ull && (uint32_t)(k >> 32) == id;
    if (running && !first) acc = __dadd_rn(acc, (double)__uint_as_float(val[a + (uint32_t)k]));
    if (!__any(running)) break;
  }
  if (head) { scol[a + rank] = id; sval[a + rank] = crm_value(first, first_bits, acc); }
  if (active && lane == 0) cnt[r] = (int64_t)__popcll(mine);
}

// long form.  rows [0, n]: is the row long, and its entries if so ([n]: 0, the scans end in the totals)
__global__ __launch_bounds__(CT) void crm_long_flags_k(const int64_t* __restrict__ rp, int64_t n, int glim, int64_t* __restrict__ lflag, int64_t* __restrict__ llen) {
  const int64_t r = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (r > n) return;
  int64_t l = 0, f = 0;
  if (r < n) { l = rp[r + 1] - rp[r]; f = l > (int64_t)glim; }
  lflag[r] = f; llen[r] = f ? l : 0;
}

// the list of the long rows and their offsets in the compact key array (loff[NL] = the total)
__global__ __launch_bounds__(CT) void crm_long_list_k(int64_t n, const int64_t* __restrict__ lflag, const int64_t* __restrict__ lidx, const int64_t* __restrict__ lbase,
                                                     int64_t* __restrict__ lrow, int64_t* __restrict__ loff) {
  const int64_t r = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (r > n) return;
  if (r == n) { loff[lidx[n]] = lbase[n]; return; }
  if (lflag[r]) { lrow[lidx[r]] = r; loff[lidx[r]] = lbase[r]; }
}

// positions [q0, q1) of the compact array: key = new id << 32 | position in the row (a dropped entry: all ones), value = the long row's index
__global__ __launch_bounds__(CT) void crm_long_keys_k(const int64_t* __restrict__ rp, const int64_t* __restrict__ lrow, const int64_t* __restrict__ loff, int64_t NL,
                                                     const uint32_t* __restrict__ nid, int64_t q0, int64_t q1, uint64_t* __restrict__ key, uint32_t* __restrict__ seg) {
  const int64_t q = q0 + (int64_t)blockIdx.x * CT + threadIdx.x;
  if (q >= q1) return;
  const int64_t i = row_of(loff, NL, q);   // (an empty long row shares its offset with the next one: the last one with loff <= q holds q)
  const int64_t pos = q - loff[i];
  const uint32_t v = nid[rp[lrow[i]] + pos];
  key[q] = v == COL_DROP ? ~0ull : (((uint64_t)v << 32) | (uint64_t)pos);
  seg[q] = (uint32_t)i;
}

// sorted positions [q0, q1): the heads of the equal-id runs
__global__ __launch_bounds__(CT) void crm_long_heads_k(const int64_t* __restrict__ loff, const uint64_t* __restrict__ ks, const uint32_t* __restrict__ seg, int64_t q0,
                                                      int64_t q1, int64_t* __restrict__ hflag) {
  const int64_t q = q0 + (int64_t)blockIdx.x * CT + threadIdx.x;
  if (q >= q1) return;
  const uint64_t k = ks[q];
  hflag[q] = (k != ~0ull && (q == loff[seg[q]] || (uint32_t)(ks[q - 1] >> 32) != (uint32_t)(k >> 32))) ? 1 : 0;
}

// one thread per head of [q0, q1): walks its run in source order
__global__ __launch_bounds__(CT) void crm_long_walk_k(const int64_t* __restrict__ rp, const int64_t* __restrict__ lrow, const int64_t* __restrict__ loff,
                                                     const uint64_t* __restrict__ ks, const uint32_t* __restrict__ seg, const int64_t* __restrict__ hflag,
                                                     const int64_t* __restrict__ hpos, int64_t q0, int64_t q1, const uint32_t* __restrict__ val, int first,
                                                     uint32_t* __restrict__ scol, uint32_t* __restrict__ sval) {
  const int64_t q = q0 + (int64_t)blockIdx.x * CT + threadIdx.x;
  if (q >= q1 || !hflag[q]) return;
  const int64_t i = seg[q];
  const int64_t a = rp[lrow[i]], end = loff[i + 1];
  const uint64_t k = ks[q];
  const uint32_t id = (uint32_t)(k >> 32);
  const uint32_t first_bits = val[a + (uint32_t)k];
  double acc = (double)__uint_as_float(first_bits);
  if (!first)
    for (int64_t t = q + 1; t < end; ++t) {
      const uint64_t kt = ks[t];
      if (kt == ~0ull || (uint32_t)(kt >> 32) != id) break;
      acc = __dadd_rn(acc, (double)__uint_as_float(val[a + (uint32_t)kt]));
    }
  const int64_t slot = a + (hpos[q] - hpos[loff[i]]);
  scol[slot] = id; sval[slot] = crm_value(first, first_bits, acc);
}

__global__ __launch_bounds__(CT) void crm_long_counts_k(int64_t NL, const int64_t* __restrict__ lrow, const int64_t* __restrict__ loff, const int64_t* __restrict__ hpos,
                                                       int64_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * CT + threadIdx.x;
  if (i < NL) cnt[lrow[i]] = hpos[loff[i + 1]] - hpos[loff[i]];
}

// staging row -> output row: G lanes (a power of two, at most 64) per row of [r0, r1), take_group_k's shape
__global__ __launch_bounds__(CT) void crm_compact_k(const int64_t* __restrict__ rp, const int64_t* __restrict__ orp, int64_t r0, int64_t r1, int G,
                                                   const uint32_t* __restrict__ scol, const uint32_t* __restrict__ sval, uint32_t* __restrict__ ocol,
                                                   uint32_t* __restrict__ oval) {
  const int64_t r = r0 + ((int64_t)blockIdx.x * CT + threadIdx.x) / G;
  const int lane = threadIdx.x & (G - 1);
  if (r >= r1) return;
  const int64_t d0 = orp[r], len = orp[r + 1] - d0, s0 = rp[r];   // len <= the source row's entries
  for (int64_t x = lane; x < len; x += G) { ocol[d0 + x] = scol[s0 + x]; oval[d0 + x] = sval[s0 + x]; }
}

int remap_run(const fmx_matrix* m, const uint32_t* d_map, uint32_t new_p, int combine, fmx_matrix** out) {
  const hipStream_t st = nullptr;
  const ColLimits lim = col_limits();
  const int64_t n = m->n, nnz = m->nnz;
  const uint32_t* val = reinterpret_cast<const uint32_t*>(m->val);
  Scratch S;
  uint32_t* nid = nullptr;
  int64_t *flag = nullptr, *tot = nullptr;   // tot: the scanned offsets; the slot behind their total holds the lowest column with a bad map value (all ones: none)
  FMX_TRY(S.get(&nid, (size_t)nnz));
  const bool keep = combine == FMX_COMBINE_KEEP;
  const int64_t items = keep ? nnz : n;
  FMX_TRY(S.get(&flag, (size_t)items + 1)); FMX_TRY(S.get(&tot, (size_t)items + 2));
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(tot + items + 1);
  FMX_HIP(hipMemsetAsync(bad, 0xFF, sizeof(int64_t), st));
  FMX_HIP(hipMemsetAsync(flag + items, 0, sizeof(int64_t), st));   // the scan ends in the total
  if (m->p > 0) {
    hipLaunchKernelGGL(crm_check_k, dim3(blocks(m->p, CT)), dim3(CT), 0, st, (int64_t)m->p, d_map, new_p, bad);
    FMX_HIP(hipGetLastError());
  }
  FMX_TRY(in_cuts(nnz, lim.chunk_entries, [&](int64_t a, int64_t b) {
    hipLaunchKernelGGL(crm_ids_k, dim3(blocks(b - a, CT)), dim3(CT), 0, st, (const uint32_t*)m->col, d_map, a, b, nid, keep ? flag : nullptr);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }));
  uint32_t *scol = nullptr, *sval = nullptr;
  if (!keep) {
    const int first = combine == FMX_COMBINE_FIRST ? 1 : 0;
    FMX_TRY(S.get(&scol, (size_t)nnz)); FMX_TRY(S.get(&sval, (size_t)nnz));
    FMX_HIP(hipMemsetAsync(flag, 0, ((size_t)n + 1) * sizeof(int64_t), st));
    int glim = lim.group_entries;   // < 0: no row takes the group form
    if (glim >= 0) {
      const int widest = std::min(glim, m->max_row_len);
      glim = std::min(glim, widest <= 16 ? 16 : widest <= 32 ? 32 : 64);   // never more entries than lanes
      FMX_TRY(in_cuts(n, lim.launch_rows, [&](int64_t a, int64_t b) {
        if (widest <= 16) hipLaunchKernelGGL((crm_group_k<16>), dim3(blocks((b - a) * 16, CT)), dim3(CT), 0, st, m->row_ptr, a, b, glim, (const uint32_t*)nid, val, first, scol, sval, flag);
        else if (widest <= 32) hipLaunchKernelGGL((crm_group_k<32>), dim3(blocks((b - a) * 32, CT)), dim3(CT), 0, st, m->row_ptr, a, b, glim, (const uint32_t*)nid, val, first, scol, sval, flag);
        else hipLaunchKernelGGL((crm_group_k<64>), dim3(blocks((b - a) * 64, CT)), dim3(CT), 0, st, m->row_ptr, a, b, glim, (const uint32_t*)nid, val, first, scol, sval, flag);
        FMX_HIP(hipGetLastError());
        return FMX_OK;
      }));
    }
    if (glim < 0 || m->max_row_len > glim) {
      int64_t *lflag = nullptr, *llen = nullptr, *lidx = nullptr, *lbase = nullptr;
      FMX_TRY(S.get(&lflag, (size_t)n + 1)); FMX_TRY(S.get(&llen, (size_t)n + 1)); FMX_TRY(S.get(&lidx, (size_t)n + 1)); FMX_TRY(S.get(&lbase, (size_t)n + 1));
      hipLaunchKernelGGL(crm_long_flags_k, dim3(blocks(n + 1, CT)), dim3(CT), 0, st, m->row_ptr, n, glim, lflag, llen);
      FMX_HIP(hipGetLastError());
      FMX_TRY(exclusive_sum(S, (const int64_t*)lflag, lidx, n + 1));
      FMX_TRY(exclusive_sum(S, (const int64_t*)llen, lbase, n + 1));
      int64_t NL = 0, LT = 0;
      FMX_HIP(hipMemcpyAsync(&NL, lidx + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
      FMX_HIP(hipMemcpyAsync(&LT, lbase + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
      FMX_HIP(hipStreamSynchronize(st));
      if (NL > 0) {
        int64_t *lrow = nullptr, *loff = nullptr, *hflag = nullptr, *hpos = nullptr;
        uint64_t *key = nullptr, *ks = nullptr;
        uint32_t *seg = nullptr, *segs = nullptr;
        FMX_TRY(S.get(&lrow, (size_t)NL)); FMX_TRY(S.get(&loff, (size_t)NL + 1));
        FMX_TRY(S.get(&key, (size_t)LT)); FMX_TRY(S.get(&ks, (size_t)LT)); FMX_TRY(S.get(&seg, (size_t)LT)); FMX_TRY(S.get(&segs, (size_t)LT));
        FMX_TRY(S.get(&hflag, (size_t)LT + 1)); FMX_TRY(S.get(&hpos, (size_t)LT + 1));
        hipLaunchKernelGGL(crm_long_list_k, dim3(blocks(n + 1, CT)), dim3(CT), 0, st, n, (const int64_t*)lflag, (const int64_t*)lidx, (const int64_t*)lbase, lrow, loff);
        FMX_HIP(hipGetLastError());
        FMX_TRY(in_cuts(LT, lim.chunk_entries, [&](int64_t a, int64_t b) {
          hipLaunchKernelGGL(crm_long_keys_k, dim3(blocks(b - a, CT)), dim3(CT), 0, st, m->row_ptr, (const int64_t*)lrow, (const int64_t*)loff, NL, (const uint32_t*)nid, a, b,
                             key, seg);
          FMX_HIP(hipGetLastError());
          return FMX_OK;
        }));
        if (LT > 0) FMX_TRY(S.with_temp([&](void* t, size_t& bytes) { return seg_sort_pairs(t, bytes, key, ks, seg, segs, LT, NL, loff, st); }));
        FMX_HIP(hipMemsetAsync(hflag + LT, 0, sizeof(int64_t), st));
        FMX_TRY(in_cuts(LT, lim.chunk_entries, [&](int64_t a, int64_t b) {
          hipLaunchKernelGGL(crm_long_heads_k, dim3(blocks(b - a, CT)), dim3(CT), 0, st, (const int64_t*)loff, (const uint64_t*)ks, (const uint32_t*)segs, a, b, hflag);
          FMX_HIP(hipGetLastError());
          return FMX_OK;
        }));
        FMX_TRY(exclusive_sum(S, (const int64_t*)hflag, hpos, LT + 1));
        FMX_TRY(in_cuts(LT, lim.chunk_entries, [&](int64_t a, int64_t b) {
          hipLaunchKernelGGL(crm_long_walk_k, dim3(blocks(b - a, CT)), dim3(CT), 0, st, m->row_ptr, (const int64_t*)lrow, (const int64_t*)loff, (const uint64_t*)ks,
                             (const uint32_t*)segs, (const int64_t*)hflag, (const int64_t*)hpos, a, b, val, first, scol, sval);
          FMX_HIP(hipGetLastError());
          return FMX_OK;
        }));
        hipLaunchKernelGGL(crm_long_counts_k, dim3(blocks(NL, CT)), dim3(CT), 0, st, NL, (const int64_t*)lrow, (const int64_t*)loff, (const int64_t*)hpos, flag);
        FMX_HIP(hipGetLastError());
      }
    }
  }
  FMX_TRY(exclusive_sum(S, (const int64_t*)flag, tot, items + 1));
  int64_t back[2] = {0, 0};
  FMX_HIP(hipMemcpyAsync(back, tot + items, sizeof(back), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  FMX_CHECK(back[1] == -1, FMX_ERR_INVALID, "map[%lld] is neither below new_p (%u) nor 0xFFFFFFFF", (long long)back[1], new_p);
  const int64_t total = back[0];
  fmx_matrix* o = nullptr;
  FMX_TRY(alloc_matrix(m->device, n, new_p, total, m->has_labels != 0, &o));
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> hold(o, free_matrix);
  uint32_t *ocol = o->col, *oval = reinterpret_cast<uint32_t*>(o->val);
  if (keep) {
    hipLaunchKernelGGL(crm_keep_ptrs_k, dim3(blocks(n + 1, CT)), dim3(CT), 0, st, m->row_ptr, n, (const int64_t*)tot, o->row_ptr);
    FMX_HIP(hipGetLastError());
    FMX_TRY(in_cuts(nnz, lim.chunk_entries, [&](int64_t a, int64_t b) {
      hipLaunchKernelGGL(crm_keep_scatter_k, dim3(blocks(b - a, CT)), dim3(CT), 0, st, a, b, (const uint32_t*)nid, (const int64_t*)tot, val, ocol, oval);
      FMX_HIP(hipGetLastError());
      return FMX_OK;
    }));
  } else {
    FMX_HIP(hipMemcpyAsync(o->row_ptr, tot, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    int G = 2;
    while (G < 64 && (int64_t)G * n < total) G <<= 1;   // the mean output row, rounded up to a power of two
    FMX_TRY(in_cuts(total > 0 ? n : 0, lim.launch_rows, [&](int64_t a, int64_t b) {
      hipLaunchKernelGGL(crm_compact_k, dim3(blocks((b - a) * G, CT)), dim3(CT), 0, st, m->row_ptr, (const int64_t*)tot, a, b, G, (const uint32_t*)scol, (const uint32_t*)sval,
                         ocol, oval);
      FMX_HIP(hipGetLastError());
      return FMX_OK;
    }));
  }
  if (m->has_labels && n > 0) FMX_HIP(hipMemcpyAsync(o->y, m->y, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
  FMX_HIP(hipStreamSynchronize(st));
  FMX_TRY(check_rows_sorted(o));
  *out = hold.release();
  return FMX_OK;
}

int check_remap(const fmx_matrix* m, const void* map, uint32_t new_p, int32_t combine, fmx_matrix** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(map != nullptr || m->p == 0, FMX_ERR_INVALID, "the map is NULL");
  FMX_CHECK(new_p != COL_DROP, FMX_ERR_INVALID, "new_p must be below 0xFFFFFFFF");
  FMX_CHECK(combine == FMX_COMBINE_KEEP || combine == FMX_COMBINE_SUM || combine == FMX_COMBINE_FIRST, FMX_ERR_INVALID, "unknown combine %d", (int)combine);
  FMX_CHECK(m->n <= COL_MAX_ITEMS && m->nnz <= COL_MAX_ITEMS, FMX_ERR_INVALID, "at most 2^31 - 1 rows and stored entries per call");
  return FMX_OK;
}

template <typename T>
int col_upload(DevBuf* b, const T* host, int64_t count) {
  FMX_TRY(dev_buf(b, (size_t)count * sizeof(T)));
  if (count > 0) FMX_HIP(hipMemcpy(b->get(), host, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
  return FMX_OK;
}

}  // namespace

void debug_columns_limits(int group_entries, int64_t chunk_entries, int64_t rows_per_launch) {
  g_group_entries.store(group_entries);
  g_chunk_entries.store(chunk_entries > 0 ? chunk_entries : 0);
  g_launch_rows.store(rows_per_launch > 0 ? rows_per_launch : 0);
}

}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_matrix_column_stats_device(const fmx_matrix* m, void* dev_count_i64, void* dev_value_f64) {
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(dev_count_i64 != nullptr || m->p == 0, FMX_ERR_INVALID, "the count table is NULL");
  FMX_CHECK(m->n <= COL_MAX_ITEMS && m->nnz <= COL_MAX_ITEMS, FMX_ERR_INVALID, "at most 2^31 - 1 rows and stored entries per call");
  FMX_TRY(use_device(m->device));
  return stats_run(m, (int64_t*)dev_count_i64, (double*)dev_value_f64);
}

int fmx_matrix_column_stats(const fmx_matrix* m, int64_t* count, double* value) {
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(count != nullptr || m->p == 0, FMX_ERR_INVALID, "the count table is NULL");
  FMX_CHECK(m->n <= COL_MAX_ITEMS && m->nnz <= COL_MAX_ITEMS, FMX_ERR_INVALID, "at most 2^31 - 1 rows and stored entries per call");
  FMX_TRY(use_device(m->device));
  if (m->p == 0) return FMX_OK;
  DevBuf dc, dv;
  FMX_TRY(dev_buf(&dc, (size_t)m->p * 3 * sizeof(int64_t)));
  if (value) FMX_TRY(dev_buf(&dv, (size_t)m->p * 2 * sizeof(double)));
  FMX_TRY(stats_run(m, (int64_t*)dc.get(), (double*)dv.get()));
  FMX_HIP(hipMemcpy(count, dc.get(), (size_t)m->p * 3 * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (value) FMX_HIP(hipMemcpy(value, dv.get(), (size_t)m->p * 2 * sizeof(double), hipMemcpyDeviceToHost));
  return FMX_OK;
}

int fmx_column_map_select_device(int device, uint32_t p, const void* dev_count_i64, const fmx_column_rule* rule, void* dev_map_u32, uint32_t* new_p,
                                 uint32_t* new_segment_base) {
  std::vector<uint32_t> base, nsb;
  FMX_TRY(check_select(p, dev_count_i64, rule, dev_map_u32, new_p, &base));
  FMX_TRY(use_device(device));
  FMX_TRY(select_run(p, (const int64_t*)dev_count_i64, *rule, base, (uint32_t*)dev_map_u32, &nsb));
  *new_p = nsb.back();
  if (new_segment_base) std::memcpy(new_segment_base, nsb.data(), nsb.size() * sizeof(uint32_t));
  return FMX_OK;
}

int fmx_column_map_select(int device, uint32_t p, const int64_t* count, const fmx_column_rule* rule, uint32_t* map, uint32_t* new_p, uint32_t* new_segment_base) {
  std::vector<uint32_t> base, nsb;
  FMX_TRY(check_select(p, count, rule, map, new_p, &base));
  FMX_TRY(use_device(device));
  DevBuf dc, dm;
  FMX_TRY(col_upload(&dc, count, (int64_t)p * 3));
  FMX_TRY(dev_buf(&dm, (size_t)p * sizeof(uint32_t)));
  FMX_TRY(select_run(p, (const int64_t*)dc.get(), *rule, base, (uint32_t*)dm.get(), &nsb));
  if (p > 0) FMX_HIP(hipMemcpy(map, dm.get(), (size_t)p * sizeof(uint32_t), hipMemcpyDeviceToHost));
  *new_p = nsb.back();
  if (new_segment_base) std::memcpy(new_segment_base, nsb.data(), nsb.size() * sizeof(uint32_t));
  return FMX_OK;
}

int fmx_column_map_hash_device(int device, uint32_t p, uint32_t n_buckets, uint64_t seed, uint64_t salt, uint32_t keep_prefix, void* dev_map_u32, uint32_t* new_p) {
  FMX_TRY(check_hash(p, n_buckets, keep_prefix, dev_map_u32, new_p));
  FMX_TRY(use_device(device));
  FMX_TRY(hash_run(p, n_buckets, seed, salt, keep_prefix, (uint32_t*)dev_map_u32));
  *new_p = keep_prefix + n_buckets;
  return FMX_OK;
}

int fmx_column_map_hash(int device, uint32_t p, uint32_t n_buckets, uint64_t seed, uint64_t salt, uint32_t keep_prefix, uint32_t* map, uint32_t* new_p) {
  FMX_TRY(check_hash(p, n_buckets, keep_prefix, map, new_p));
  FMX_TRY(use_device(device));
  DevBuf dm;
  FMX_TRY(dev_buf(&dm, (size_t)p * sizeof(uint32_t)));
  FMX_TRY(hash_run(p, n_buckets, seed, salt, keep_prefix, (uint32_t*)dm.get()));
  if (p > 0) FMX_HIP(hipMemcpy(map, dm.get(), (size_t)p * sizeof(uint32_t), hipMemcpyDeviceToHost));
  *new_p = keep_prefix + n_buckets;
  return FMX_OK;
}

int fmx_matrix_remap_columns_device(const fmx_matrix* m, const void* dev_map_u32, uint32_t new_p, int32_t combine, fmx_matrix** out) {
  FMX_TRY(check_remap(m, dev_map_u32, new_p, combine, out));
  FMX_TRY(use_device(m->device));
  return remap_run(m, (const uint32_t*)dev_map_u32, new_p, combine, out);
}

int fmx_matrix_remap_columns(const fmx_matrix* m, const uint32_t* map, uint32_t new_p, int32_t combine, fmx_matrix** out) {
  FMX_TRY(check_remap(m, map, new_p, combine, out));
  for (uint32_t j = 0; j < m->p; ++j)
    FMX_CHECK(map[j] == COL_DROP || map[j] < new_p, FMX_ERR_INVALID, "map[%u] = %u is neither below new_p (%u) nor 0xFFFFFFFF", j, map[j], new_p);
  FMX_TRY(use_device(m->device));
  DevBuf dm;
  FMX_TRY(col_upload(&dm, map, (int64_t)m->p));
  return remap_run(m, (const uint32_t*)dm.get(), new_p, combine, out);
}

int fmx_debug_columns_limits(int32_t group_entries, int64_t chunk_entries, int64_t rows_per_launch) {
  debug_columns_limits(group_entries, chunk_entries, rows_per_launch);
  return FMX_OK;
}

int fmx_debug_matrix_flags(const fmx_matrix* m, int32_t* out) {
  FMX_CHECK(m != nullptr && out != nullptr, FMX_ERR_INVALID, "NULL argument");
  out[0] = m->rows_sorted; out[1] = m->unit_values; out[2] = m->fixed_row_len; out[3] = m->max_row_len;
  out[4] = m->field_base.empty() ? 0 : (int32_t)m->field_base.size() - 1;
  return FMX_OK;
}

int fmx_debug_matrix_layout(const fmx_matrix* m, int32_t* dense_prefix, int32_t* n_fields, uint32_t* base) {
  FMX_CHECK(m != nullptr && dense_prefix != nullptr && n_fields != nullptr && base != nullptr, FMX_ERR_INVALID, "NULL argument");
  const size_t C = m->field_base.empty() ? 0 : m->field_base.size() - 1;
  FMX_CHECK(C <= (size_t)FMX_MAX_FIELDS, FMX_ERR_INVALID, "a layout of %zu fields", C);
  *dense_prefix = m->dense_prefix;
  *n_fields = (int32_t)C;
  for (size_t c = 0; c < (size_t)FMX_MAX_FIELDS + 1; ++c) base[c] = (C && c <= C) ? m->field_base[c] : 0u;
  return FMX_OK;
}

}  // extern "C"
