// Value binning on the device: fmx_matrix_column_quantiles, fmx_matrix_bin_columns.  Dense columns become one-hot buckets:
// the fit finds equal-mass edges of chosen columns, the apply replaces those columns' entries by (bucket id, 1.0f).  All of it is integer work on
// the values' bits -- a value is only ever compared, through the 32-bit order key vkey(x) -- so tests/bins_model.py restates every output bit for bit.
//
//   vkey     the float's bits with -0 taken as +0; a set sign bit gives the complement, otherwise the bits with the top bit set; every NaN gives
//            0xFFFFFFFF, above +inf's 0xFF800000.  Ascending in vkey = ascending in x, NaN last (rank_order_key's idea on fp32).
//   slots    one table u32[p] for both calls, made by one kernel from the ascending column list: a chosen column holds 0x80000000 | its slot,
//            every other column the number of chosen columns below it.
//   fit      the chosen columns' entries are counted and then appended (one integer atomic per wave: the order of the appends does not matter,
//            the sort's key is the whole record) as keys slot << 32 | vkey; sort_keys over 32 + key_bits(n_cols - 1) bits; a thread per slot finds
//            the slot's run and its first NaN by binary search; one workgroup per slot reads the candidates L[floor(b cnt / n_bins)], flags those
//            above the candidate before them (candidate 0 is L[0]: the flagged ones are the distinct candidates > L[0]) and compacts them by a
//            workgroup scan.  Everything comes back in ONE read.
//   apply    one pass over the entries, a lane moves four (16 bytes of columns, 16 of values): the slot table gives the shift of an unchanged
//            column, or the slot; the bucket is #{edges <= x} by a branch-free binary search over the slot's run of the packed table of edge
//            KEYS (vkey(e) <= vkey(x) is e <= x for the non-NaN edges; a NaN's key lies above every edge, so its count is n_edges, and the NaN
//            id is one more).  Two forms with the same bits: the packed table staged in LDS, or read from global memory.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <vector>

#include "fm_prims.h"
#include "fmx_test_hooks.h"

namespace fmx {
namespace {

constexpr int BT = 256;
constexpr uint32_t BIN_SLOT = 0x80000000u;        // slot table: the column is binned, the low bits are its slot
constexpr uint32_t BIN_ONE = 0x3F800000u;         // 1.0f
constexpr uint32_t BIN_NAN_KEY = 0xFFFFFFFFu;
constexpr int BIN_MAX_BINS = 65536;
constexpr int64_t BIN_MAX_EDGES = 65535;          // edges of one column
constexpr int BIN_LDS_EDGES = 12288;              // 48 KiB of edge keys: three workgroups of the apply stay resident on a CU's 160 KiB
constexpr int64_t BIN_LAUNCH_ENTRIES = 1LL << 28;
constexpr int64_t BIN_MAX_ITEMS = 0x7FFFFFFFLL;
constexpr int BIN_GROUP_PIECES = 16;              // 16-byte pieces per lane of an apply workgroup: the staging of the table is paid once per 16 Ki entries

std::atomic<int> g_lds_edges{0};
std::atomic<int64_t> g_chunk_entries{0};

struct BinLimits {
  int lds_edges;           // the packed table goes through LDS when it holds at most this many edges (< 0: never)
  int64_t chunk_entries;   // entries per launch of a per-entry kernel, a multiple of 4
};
BinLimits bin_limits() {
  BinLimits l{g_lds_edges.load(), g_chunk_entries.load()};
  if (l.lds_edges == 0 || l.lds_edges > BIN_LDS_EDGES) l.lds_edges = BIN_LDS_EDGES;
  if (l.chunk_entries <= 0) l.chunk_entries = BIN_LAUNCH_ENTRIES;
  l.chunk_entries = std::max<int64_t>(4, l.chunk_entries & ~3LL);
  return l;
}

__host__ __device__ __forceinline__ uint32_t vkey_bits(uint32_t b) {
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return BIN_NAN_KEY;
  if (b == 0x80000000u) b = 0;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the bits of the (non-NaN) value behind a key
__device__ __forceinline__ uint32_t vkey_value(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }

// columns [0, p): slot[c] = BIN_SLOT | s where cols[s] == c, otherwise #{s : cols[s] < c}
__global__ __launch_bounds__(BT) void bin_slots_k(int64_t p, const uint32_t* __restrict__ cols, int n_cols, uint32_t* __restrict__ slot) {
  const int64_t c = (int64_t)blockIdx.x * BT + threadIdx.x;
  if (c >= p) return;
  int lo = 0, hi = n_cols;   // the first s with cols[s] >= c
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)cols[mid] < c) lo = mid + 1; else hi = mid;
  }
  slot[c] = (lo < n_cols && (int64_t)cols[lo] == c) ? (BIN_SLOT | (uint32_t)lo) : (uint32_t)lo;
}

// ------------------------------------------------------------------------------------------------------------------------------ fit

// entries [e0, e1): the chosen ones are counted (key == null) or appended to key[] behind *cursor; one atomic per wave that holds any
__global__ __launch_bounds__(BT) void bin_gather_k(const uint32_t* __restrict__ col, const uint32_t* __restrict__ val, const uint32_t* __restrict__ slot, int64_t e0,
                                                  int64_t e1, unsigned long long* __restrict__ cursor, uint64_t* __restrict__ key) {
  const int64_t e = e0 + (int64_t)blockIdx.x * BT + threadIdx.x;
  uint32_t s = 0;
  if (e < e1) s = slot[col[e]];
  const bool take = (s & BIN_SLOT) != 0;
  const uint64_t ballot = __ballot(take);   // (uniform: no lane has left)
  if (ballot == 0) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((unsigned long long)ballot) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(ballot));
  base = __shfl(base, leader, 64);
  if (take && key) {
    const uint32_t x = val ? val[e] : BIN_ONE;
    key[base + (unsigned long long)__popcll(ballot & ((1ull << lane) - 1ull))] = ((uint64_t)(s & ~BIN_SLOT) << 32) | (uint64_t)vkey_bits(x);
  }
}

// slots [0, n_cols]: bnd[2 s] = the first sorted position whose key is >= s << 32, bnd[2 s + 1] = the first that is >= s << 32 | NaN key
__global__ __launch_bounds__(BT) void bin_bounds_k(const uint64_t* __restrict__ ks, int64_t total, int n_cols, int64_t* __restrict__ bnd) {
  const int64_t t = (int64_t)blockIdx.x * BT + threadIdx.x;
  if (t >= 2 * ((int64_t)n_cols + 1)) return;
  const uint64_t want = ((uint64_t)(t >> 1) << 32) | ((t & 1) ? (uint64_t)BIN_NAN_KEY : 0ull);
  int64_t lo = 0, hi = total;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ks[mid] < want) lo = mid + 1; else hi = mid;
  }
  bnd[t] = lo;
}

// one workgroup per slot s.  cnt = the slot's non-NaN entries L = ks[a .. a + cnt); candidate b = L[floor(b cnt / n_bins)], candidate 0 = L[0]; an edge is
// a candidate above the one before it.  edges[s][..] is cleared beforehand (the padding is +0.0)
__global__ __launch_bounds__(BT) void bin_edges_k(const uint64_t* __restrict__ ks, const int64_t* __restrict__ bnd, int n_bins, uint32_t* __restrict__ edges,
                                                 int32_t* __restrict__ n_edges, int64_t* __restrict__ count, uint32_t* __restrict__ range) {
  __shared__ int wsum[BT / 64];
  __shared__ int base_s;
  const int s = blockIdx.x;
  const int64_t a = bnd[2 * s], cnt = bnd[2 * s + 1] - a, nan = bnd[2 * s + 2] - bnd[2 * s + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) base_s = 0;
  __syncthreads();
  if (cnt > 0) {
    uint32_t* out = edges + (size_t)s * (size_t)(n_bins - 1);
    for (int b0 = 1; b0 < n_bins; b0 += BT) {   // (uniform trip count: the barriers below are reached by every thread)
      const int b = b0 + threadIdx.x;
      bool flag = false;
      uint32_t k = 0;
      if (b < n_bins) {
        k = (uint32_t)ks[a + (int64_t)(((uint64_t)b * (uint64_t)cnt) / (uint64_t)n_bins)];
        const uint32_t before = (uint32_t)ks[a + (int64_t)(((uint64_t)(b - 1) * (uint64_t)cnt) / (uint64_t)n_bins)];
        flag = k > before;
      }
      const uint64_t ballot = __ballot(flag);
      if (lane == 0) wsum[wave] = __popcll(ballot);
      __syncthreads();
      int pos = base_s + __popcll(ballot & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
      for (int w = 0; w < BT / 64; ++w) {
        if (w < wave) pos += wsum[w];
        all += wsum[w];
      }
      if (flag) out[pos] = vkey_value(k);
      __syncthreads();   // every thread has read base_s and wsum
      if (threadIdx.x == 0) base_s += all;
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    n_edges[s] = base_s;
    count[2 * s] = cnt; count[2 * s + 1] = nan;
    range[2 * s] = cnt > 0 ? vkey_value((uint32_t)ks[a]) : 0u;
    range[2 * s + 1] = cnt > 0 ? vkey_value((uint32_t)ks[a + cnt - 1]) : 0u;
  }
}

// the column list of both calls: what can be said without the matrix, then the matrix and the range (cols ascends: the last id is the highest)
int check_cols(const fmx_matrix* m, const uint32_t* cols, int32_t n_cols) {
  FMX_CHECK(n_cols >= 0, FMX_ERR_INVALID, "n_cols must not be negative");
  FMX_CHECK(cols != nullptr, FMX_ERR_INVALID, "cols is NULL");
  for (int32_t s = 1; s < n_cols; ++s)
    FMX_CHECK(cols[s - 1] < cols[s], FMX_ERR_INVALID, "cols must ascend strictly (cols[%d] = %u follows %u)", (int)s, cols[s], cols[s - 1]);
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(n_cols == 0 || cols[n_cols - 1] < m->p, FMX_ERR_INVALID, "cols[%d] = %u is not below the feature count %u", (int)n_cols - 1,
            n_cols ? cols[n_cols - 1] : 0u, m->p);
  return FMX_OK;
}

int slots_run(const fmx_matrix* m, const uint32_t* cols, int n_cols, Scratch& S, uint32_t** slot) {
  uint32_t* dcols = nullptr;
  FMX_TRY(S.get(&dcols, (size_t)n_cols)); FMX_TRY(S.get(slot, (size_t)m->p));
  if (n_cols > 0) FMX_HIP(hipMemcpyAsync(dcols, cols, (size_t)n_cols * sizeof(uint32_t), hipMemcpyHostToDevice, S.st));
  if (m->p > 0) {
    hipLaunchKernelGGL(bin_slots_k, dim3(blocks(m->p, BT)), dim3(BT), 0, S.st, (int64_t)m->p, (const uint32_t*)dcols, n_cols, *slot);
    FMX_HIP(hipGetLastError());
  }
  return FMX_OK;
}

int quantiles_run(const fmx_matrix* m, const uint32_t* cols, int n_cols, int n_bins, float* edges, int32_t* n_edges, int64_t* count, float* range) {
  const BinLimits lim = bin_limits();
  const int64_t nnz = m->nnz;
  const uint32_t* val = m->unit_values ? nullptr : reinterpret_cast<const uint32_t*>(m->val);
  Scratch S;
  const hipStream_t st = S.st;
  uint32_t* slot = nullptr;
  FMX_TRY(slots_run(m, cols, n_cols, S, &slot));
  unsigned long long* cursor = nullptr;   // [0] the count pass, [1] the append pass
  FMX_TRY(S.get(&cursor, 2));
  FMX_HIP(hipMemsetAsync(cursor, 0, 2 * sizeof(unsigned long long), st));
  for (int64_t a = 0; a < nnz; a += lim.chunk_entries) {
    const int64_t b = std::min(nnz, a + lim.chunk_entries);
    hipLaunchKernelGGL(bin_gather_k, dim3(blocks(b - a, BT)), dim3(BT), 0, st, (const uint32_t*)m->col, val, (const uint32_t*)slot, a, b, cursor, (uint64_t*)nullptr);
    FMX_HIP(hipGetLastError());
  }
  unsigned long long total_u = 0;
  FMX_HIP(hipMemcpyAsync(&total_u, cursor, sizeof(total_u), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  const int64_t total = (int64_t)total_u;
  uint64_t *key = nullptr, *ks = nullptr;
  FMX_TRY(S.get(&key, (size_t)total)); FMX_TRY(S.get(&ks, (size_t)total));
  if (total > 0) {
    for (int64_t a = 0; a < nnz; a += lim.chunk_entries) {
      const int64_t b = std::min(nnz, a + lim.chunk_entries);
      hipLaunchKernelGGL(bin_gather_k, dim3(blocks(b - a, BT)), dim3(BT), 0, st, (const uint32_t*)m->col, val, (const uint32_t*)slot, a, b, cursor + 1, key);
      FMX_HIP(hipGetLastError());
    }
    FMX_TRY(sort_keys(S, key, ks, total, 32 + key_bits((uint64_t)n_cols - 1)));
  }
  // the one block that is read back: count i64[n_cols][2] | n_edges i32[n_cols] | range u32[n_cols][2] | edges u32[n_cols][n_bins - 1]
  const size_t ne_words = (size_t)n_cols * (size_t)(n_bins - 1);
  const size_t words = (size_t)n_cols * 7 + ne_words;
  uint32_t* back = nullptr;
  int64_t* bnd = nullptr;
  FMX_TRY(S.get(&back, words + 2)); FMX_TRY(S.get(&bnd, 2 * ((size_t)n_cols + 1)));
  int64_t* d_count = reinterpret_cast<int64_t*>(back);
  int32_t* d_ne = reinterpret_cast<int32_t*>(back + (size_t)n_cols * 4);
  uint32_t* d_range = back + (size_t)n_cols * 5;
  uint32_t* d_edges = back + (size_t)n_cols * 7;
  if (ne_words > 0) FMX_HIP(hipMemsetAsync(d_edges, 0, ne_words * sizeof(uint32_t), st));
  hipLaunchKernelGGL(bin_bounds_k, dim3(blocks(2 * ((int64_t)n_cols + 1), BT)), dim3(BT), 0, st, (const uint64_t*)ks, total, n_cols, bnd);
  FMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(bin_edges_k, dim3((unsigned)n_cols), dim3(BT), 0, st, (const uint64_t*)ks, (const int64_t*)bnd, n_bins, d_edges, d_ne, d_count, d_range);
  FMX_HIP(hipGetLastError());
  std::vector<uint32_t> host(words);
  FMX_HIP(hipMemcpyAsync(host.data(), back, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  std::memcpy(count, host.data(), (size_t)n_cols * 2 * sizeof(int64_t));
  std::memcpy(n_edges, host.data() + (size_t)n_cols * 4, (size_t)n_cols * sizeof(int32_t));
  std::memcpy(range, host.data() + (size_t)n_cols * 5, (size_t)n_cols * 2 * sizeof(float));
  if (ne_words > 0) std::memcpy(edges, host.data() + (size_t)n_cols * 7, ne_words * sizeof(float));
  return FMX_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------- apply

// what the apply kernel reads beside the entries: slot u32[p]; shift u32[n_cols + 1]: the ids that the binned columns below slot r add (an unchanged
// column c with r binned columns below it becomes c + shift[r], the binned column of slot s starts at cols[s] + shift[s]); eoff u32[n_cols + 2]: slot
// s's run of the packed table ekey u32[total edges] (the last offset twice: an unchanged column above every binned one reads eoff[n_cols + 1])
struct BinTab {
  const uint32_t* slot;
  const uint32_t* shift;
  const uint32_t* eoff;
  const uint32_t* ekey;
  int n_edges;   // of all slots
};

// (c, x bits) -> the output entry.  E: the packed table, in LDS or in global memory
__device__ __forceinline__ void bin_entry(const BinTab& t, const uint32_t* __restrict__ E, uint32_t c, uint32_t x, uint32_t* oc, uint32_t* ov) {
  const uint32_t s = t.slot[c];
  const bool binned = (s & BIN_SLOT) != 0;
  const uint32_t r = s & ~BIN_SLOT;
  const uint32_t e0 = t.eoff[r];
  const uint32_t e1 = t.eoff[r + 1];
  uint32_t len = binned ? e1 - e0 : 0u;
  const uint32_t kx = vkey_bits(x);
  uint32_t lo = 0;   // #{edges of the slot <= x}: every step keeps the answer inside [lo, lo + len]
  while (len > 0) {
    const uint32_t half = len >> 1;
    const bool le = E[e0 + lo + half] <= kx;
    lo = le ? lo + half + 1 : lo;
    len = le ? len - half - 1 : half;
  }
  *oc = c + t.shift[r] + lo + (binned && kx == BIN_NAN_KEY ? 1u : 0u);
  *ov = binned ? BIN_ONE : x;
}

// entries [e0, e1), e0 a multiple of 4: a workgroup owns BT * BIN_GROUP_PIECES consecutive 16-byte pieces, lane l the pieces l, l + BT, ...
template <bool LDS>
__global__ __launch_bounds__(BT) void bin_apply_k(const BinTab t, const uint32_t* __restrict__ col, const uint32_t* __restrict__ val, int64_t e0, int64_t e1,
                                                 uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval) {
  extern __shared__ uint32_t lds_e[];
  if (LDS) {
    for (int i = threadIdx.x; i < t.n_edges; i += BT) lds_e[i] = t.ekey[i];
    __syncthreads();
  }
  const uint32_t* E = LDS ? lds_e : t.ekey;
  const int64_t q0 = (e0 >> 2) + (int64_t)blockIdx.x * (BT * BIN_GROUP_PIECES);
#pragma unroll 1
  for (int i = 0; i < BIN_GROUP_PIECES; ++i) {
    const int64_t o = (q0 + (int64_t)i * BT + threadIdx.x) << 2;
    if (o >= e1) break;
    if (o + 4 <= e1) {
      const uint4 c = *reinterpret_cast<const uint4*>(col + o);
      const uint4 x = val ? *reinterpret_cast<const uint4*>(val + o) : make_uint4(BIN_ONE, BIN_ONE, BIN_ONE, BIN_ONE);
      uint4 oc, ov;
      bin_entry(t, E, c.x, x.x, &oc.x, &ov.x);
      bin_entry(t, E, c.y, x.y, &oc.y, &ov.y);
      bin_entry(t, E, c.z, x.z, &oc.z, &ov.z);
      bin_entry(t, E, c.w, x.w, &oc.w, &ov.w);
      *reinterpret_cast<uint4*>(ocol + o) = oc;
      *reinterpret_cast<uint4*>(oval + o) = ov;
    } else {
      for (int64_t e = o; e < e1; ++e) bin_entry(t, E, col[e], val ? val[e] : BIN_ONE, ocol + e, oval + e);
    }
  }
}

// every refusal of fmx_matrix_bin_columns; host only.  base: new_base[p + 1], filled only where nothing is refused
int check_spec(const fmx_matrix* m, const fmx_bin_spec* sp, const uint32_t* new_base, fmx_matrix** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(sp != nullptr, FMX_ERR_INVALID, "spec is NULL");
  FMX_CHECK(new_base != nullptr, FMX_ERR_INVALID, "new_base is NULL");
  FMX_CHECK(sp->struct_size == sizeof(fmx_bin_spec), FMX_ERR_INVALID, "spec.struct_size does not match this library");
  FMX_CHECK(sp->reserved == 0, FMX_ERR_INVALID, "spec.reserved must be 0");
  FMX_CHECK(sp->n_cols >= 0, FMX_ERR_INVALID, "n_cols must not be negative");
  FMX_CHECK(sp->edge_offset != nullptr, FMX_ERR_INVALID, "spec.edge_offset is NULL");
  FMX_CHECK(sp->edge_offset[0] == 0, FMX_ERR_INVALID, "spec.edge_offset must start at 0");
  for (int32_t s = 0; s < sp->n_cols; ++s) {   // the edges: nothing here needs the matrix
    const int64_t a = sp->edge_offset[s], b = sp->edge_offset[s + 1];
    FMX_CHECK(b >= a, FMX_ERR_INVALID, "spec.edge_offset descends at column slot %d", (int)s);
    FMX_CHECK(b - a <= BIN_MAX_EDGES, FMX_ERR_INVALID, "column slot %d has %lld edges: at most %lld", (int)s, (long long)(b - a), (long long)BIN_MAX_EDGES);
    FMX_CHECK(b == a || sp->edges != nullptr, FMX_ERR_INVALID, "spec.edges is NULL");
    for (int64_t i = a; i < b; ++i) {
      FMX_CHECK(sp->edges[i] == sp->edges[i], FMX_ERR_INVALID, "edge %lld of column slot %d is NaN", (long long)(i - a), (int)s);
      FMX_CHECK(i == a || sp->edges[i - 1] < sp->edges[i], FMX_ERR_INVALID, "the edges of column slot %d do not ascend strictly at edge %lld", (int)s, (long long)(i - a));
    }
  }
  FMX_TRY(check_cols(m, sp->cols, sp->n_cols));
  // every binned column adds its edges + 1 ids to the p there were: at most 2^31 columns of at most 2^16 each, no overflow in 64 bits
  const uint64_t width = (uint64_t)m->p + (uint64_t)sp->edge_offset[sp->n_cols] + (uint64_t)sp->n_cols;
  FMX_CHECK(width <= 0xFFFFFFFEull, FMX_ERR_INVALID, "the widths of the columns sum to %llu: above 2^32 - 2", (unsigned long long)width);
  return FMX_OK;
}

int apply_run(const fmx_matrix* m, const fmx_bin_spec* sp, fmx_matrix** out) {
  const BinLimits lim = bin_limits();
  const int n_cols = sp->n_cols;
  const int64_t n = m->n, nnz = m->nnz, n_edges = sp->edge_offset[n_cols];
  std::vector<uint32_t> tab(2 * (size_t)n_cols + 3 + (size_t)n_edges);   // shift[n_cols + 1] | eoff[n_cols + 2] | ekey
  uint32_t *shift = tab.data(), *eoff = shift + n_cols + 1, *ekey = eoff + n_cols + 2;
  shift[0] = 0;
  for (int s = 0; s < n_cols; ++s) {
    eoff[s] = (uint32_t)sp->edge_offset[s];
    shift[s + 1] = shift[s] + (uint32_t)(sp->edge_offset[s + 1] - sp->edge_offset[s]) + 1u;
  }
  eoff[n_cols] = eoff[n_cols + 1] = (uint32_t)n_edges;
  for (int64_t i = 0; i < n_edges; ++i) {
    uint32_t b;
    std::memcpy(&b, sp->edges + i, sizeof(b));
    ekey[i] = vkey_bits(b);
  }
  fmx_matrix* o = nullptr;
  FMX_TRY(alloc_matrix(m->device, n, m->p + shift[n_cols], nnz, m->has_labels != 0, &o));
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> hold(o, free_matrix);
  {
    Scratch S;
    const hipStream_t st = S.st;
    uint32_t *slot = nullptr, *dtab = nullptr;
    FMX_TRY(slots_run(m, sp->cols, n_cols, S, &slot));
    FMX_TRY(S.get(&dtab, tab.size()));
    FMX_HIP(hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    const BinTab t{slot, dtab, dtab + n_cols + 1, dtab + 2 * (size_t)n_cols + 3, (int)n_edges};
    const bool lds = lim.lds_edges > 0 && n_edges <= (int64_t)lim.lds_edges;
    const uint32_t* val = m->unit_values ? nullptr : reinterpret_cast<const uint32_t*>(m->val);
    uint32_t *ocol = o->col, *oval = reinterpret_cast<uint32_t*>(o->val);
    for (int64_t a = 0; a < nnz; a += lim.chunk_entries) {
      const int64_t b = std::min(nnz, a + lim.chunk_entries);
      const unsigned grid = blocks(((b + 3) >> 2) - (a >> 2), BT * BIN_GROUP_PIECES);
      if (lds) hipLaunchKernelGGL(bin_apply_k<true>, dim3(grid), dim3(BT), (size_t)n_edges * sizeof(uint32_t), st, t, (const uint32_t*)m->col, val, a, b, ocol, oval);
      else hipLaunchKernelGGL(bin_apply_k<false>, dim3(grid), dim3(BT), 0, st, t, (const uint32_t*)m->col, val, a, b, ocol, oval);
      FMX_HIP(hipGetLastError());
    }
    FMX_HIP(hipMemcpyAsync(o->row_ptr, m->row_ptr, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    if (m->has_labels && n > 0) FMX_HIP(hipMemcpyAsync(o->y, m->y, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    FMX_HIP(hipStreamSynchronize(st));   // (the host tables are read by the copies above)
  }
  FMX_TRY(check_rows_sorted(o));
  *out = hold.release();
  return FMX_OK;
}

}  // namespace
}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_debug_bins_limits(int32_t lds_edges, int64_t chunk_entries) {
  g_lds_edges.store(lds_edges);
  g_chunk_entries.store(chunk_entries > 0 ? chunk_entries : 0);
  return FMX_OK;
}

int fmx_matrix_column_quantiles(const fmx_matrix* m, const uint32_t* cols, int32_t n_cols, int32_t n_bins, float* edges, int32_t* n_edges, int64_t* count,
                                float* range) {
  FMX_CHECK(n_bins >= 1 && n_bins <= BIN_MAX_BINS, FMX_ERR_INVALID, "n_bins must be in 1..%d (got %d)", BIN_MAX_BINS, (int)n_bins);
  FMX_CHECK(cols != nullptr && n_edges != nullptr && count != nullptr && range != nullptr && (edges != nullptr || n_bins == 1), FMX_ERR_INVALID,
            "cols, edges, n_edges, count or range is NULL");
  FMX_TRY(check_cols(m, cols, n_cols));
  FMX_CHECK(m->nnz <= BIN_MAX_ITEMS, FMX_ERR_INVALID, "at most 2^31 - 1 stored entries per call");
  if (n_cols == 0) return FMX_OK;
  FMX_TRY(use_device(m->device));
  return quantiles_run(m, cols, n_cols, n_bins, edges, n_edges, count, range);
}

int fmx_matrix_bin_columns(const fmx_matrix* m, const fmx_bin_spec* spec, uint32_t* new_base, fmx_matrix** out) {
  FMX_TRY(check_spec(m, spec, new_base, out));
  FMX_TRY(use_device(m->device));
  FMX_TRY(apply_run(m, spec, out));
  uint32_t at = 0;
  int32_t s = 0;
  for (uint32_t c = 0; c < m->p; ++c) {
    new_base[c] = at;
    if (s < spec->n_cols && spec->cols[s] == c) {
      at += (uint32_t)(spec->edge_offset[s + 1] - spec->edge_offset[s]) + 2u;
      ++s;
    } else {
      at += 1u;
    }
  }
  new_base[m->p] = at;
  return FMX_OK;
}

}  // extern "C"
