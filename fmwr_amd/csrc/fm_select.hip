// Row selection on the device: fmx_matrix_take*, fmx_split_assign*, fmx_matrix_select*, fmx_matrix_split_entries,
// fmx_row_permutation*.  Everything is integer work -- hash keys, ranks inside segments, prefix sums, copies -- so tests/split_model.py
// reproduces every output bit for bit.
//
//   keys     H(seed, salt, t, stream): the pair sampler's pair_hash (fm_rank.h).
//            stream 0 rows, 1 groups, 2 entries ((row << 32) | column), 3 the epoch permutation (salt = epoch).
//   ranking  (seg_rank) items 0 .. N-1, each in a segment, ordered inside the segment by (key, item) or, for the TAIL order, by the item descending:
//            a stable 64-bit radix sort of the item ids by key, then a stable one by segment id; heads and tails of the segment runs, two max-scans
//            (the tails on the reversed array) give every sorted position its run [a, b]; rank = pos - a (TAIL: b - pos), size = b - a + 1.  One
//            kernel turns (rank, size) into the part and stores it at the item.  No array of the size of the segment COUNT exists, and nothing is
//            ordered by atomics.
//   take     the gather of fm_join.hip (gather_rows: the length pass with the range check, the scan, the allocation and the entry copy in its fixed,
//            group or flat form are described there, once) on a table of ONE block: the source, the row list, base 0.
//   select   a flag per row, an exclusive scan, the compaction into an ascending row list, then take.
//   entries  seg_rank with the entries as items and the rows as segments, one scan of the kept flags, two compactions.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "fm_prims.h"

namespace fmx {
namespace {

constexpr int ST = 256;
constexpr uint32_t SEL_NONE = 0xFFFFFFFFu;
constexpr int64_t SEL_MAX_ITEMS = 0x7FFFFFFFLL; // items of one ranking: positions are 32-bit

// ------------------------------------------------------------------------------------------------------------------------- ranking

struct PartRule {
  int n_folds;           // > 0: folds; 0: hold-out
  int64_t hold_count;
  double hold_fraction;
  int64_t min_keep;
};

// the part of the item of rank rho in a segment of s items (s >= 1)
__device__ __forceinline__ uint32_t part_of(const PartRule& ru, uint64_t rho, uint64_t s) {
  if (ru.n_folds > 0) return (uint32_t)(rho * (uint64_t)ru.n_folds / s);   // rho < 2^32, n_folds <= 2^16
  const int64_t c = ru.hold_count > 0 ? ru.hold_count : (int64_t)floor(__dmul_rn(ru.hold_fraction, (double)s));
  int64_t room = (int64_t)s - ru.min_keep;
  if (room < 0) room = 0;
  const int64_t q = c < room ? c : room;
  return (int64_t)rho < q ? 1u : 0u;
}

__global__ __launch_bounds__(ST) void sel_keys_k(int64_t N, uint64_t seed, uint64_t salt, uint64_t stream, uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (i < N) key[i] = pair_hash(seed, salt, (uint64_t)i, stream);
}

__global__ __launch_bounds__(ST) void sel_iota_k(int64_t N, uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (i < N) idx[i] = (uint32_t)i;
}

// the segment id of the item at every position, an id out of range as nseg (the bucket after the last segment)
__global__ __launch_bounds__(ST) void sel_seg_keys_k(int64_t N, const uint32_t* __restrict__ seg, const uint32_t* __restrict__ idx, uint64_t nseg,
                                                    uint32_t* __restrict__ gk) {
  const int64_t pos = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (pos >= N) return;
  const uint32_t g = seg[idx[pos]];
  gk[pos] = (uint64_t)g < nseg ? g : (uint32_t)nseg;   // nseg <= 2^31 - 1
}

// a run's head holds its own position, its tail its own position in the reversed array; every other slot 0
__global__ __launch_bounds__(ST) void sel_runs_k(int64_t N, const uint32_t* __restrict__ gs, uint32_t* __restrict__ head, uint32_t* __restrict__ tailr) {
  const int64_t pos = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (pos >= N) return;
  const uint32_t g = gs[pos];
  head[pos] = (pos > 0 && gs[pos - 1] != g) ? (uint32_t)pos : 0u;
  const int64_t q = N - 1 - pos;
  tailr[q] = (pos + 1 < N && gs[pos + 1] != g) ? (uint32_t)q : 0u;
}

__global__ __launch_bounds__(ST) void sel_part_k(int64_t N, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ gs, uint64_t nseg,
                                                const uint32_t* __restrict__ start, const uint32_t* __restrict__ rend, int keyed, PartRule ru,
                                                uint32_t* __restrict__ part) {
  const int64_t pos = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (pos >= N) return;
  const int64_t i = idx ? (int64_t)idx[pos] : pos;
  int64_t a = 0, b = N - 1;
  if (gs) {
    if ((uint64_t)gs[pos] >= nseg) { part[i] = SEL_NONE; return; }
    a = (int64_t)start[pos];
    b = N - 1 - (int64_t)rend[N - 1 - pos];
  }
  const uint64_t s = (uint64_t)(b - a + 1);
  const uint64_t rho = (uint64_t)(keyed ? pos - a : b - pos);
  part[i] = part_of(ru, rho, s);
}

// The part of every item: d_seg u32[N] the item's segment (null: one segment), d_key u64[N] its key (null: the TAIL order; overwritten otherwise).
// presorted: the segment ids ascend with the item and are all in range (the entries of a CSR), so the TAIL order needs no sort at all.
int seg_rank(Scratch& S, hipStream_t st, int64_t N, const uint32_t* d_seg, uint64_t nseg, bool presorted, uint64_t* d_key, const PartRule& ru,
             uint32_t* d_part) {
  if (N <= 0) return FMX_OK;
  const unsigned nb = blocks(N, ST);
  const uint32_t* idx = nullptr;
  uint32_t* idx_in = nullptr;
  if (d_key) {
    uint64_t* key_out = nullptr;
    uint32_t* idx_a = nullptr;
    FMX_TRY(S.get(&key_out, (size_t)N)); FMX_TRY(S.get(&idx_in, (size_t)N)); FMX_TRY(S.get(&idx_a, (size_t)N));
    hipLaunchKernelGGL(sel_iota_k, dim3(nb), dim3(ST), 0, st, N, idx_in);
    FMX_HIP(hipGetLastError());
    FMX_TRY(sort_pairs(S, d_key, key_out, idx_in, idx_a, N, 64));   // stable: equal keys keep their order
    idx = idx_a;
  }
  const uint32_t* gs = nullptr;
  uint32_t *start = nullptr, *rend = nullptr;
  if (d_seg) {
    if (!d_key && presorted) {
      gs = d_seg;
    } else {
      uint32_t *gk = nullptr, *gso = nullptr, *idx_b = nullptr;
      FMX_TRY(S.get(&gk, (size_t)N)); FMX_TRY(S.get(&gso, (size_t)N)); FMX_TRY(S.get(&idx_b, (size_t)N));
      if (!idx) {
        FMX_TRY(S.get(&idx_in, (size_t)N));
        hipLaunchKernelGGL(sel_iota_k, dim3(nb), dim3(ST), 0, st, N, idx_in);
        FMX_HIP(hipGetLastError());
        idx = idx_in;
      }
      hipLaunchKernelGGL(sel_seg_keys_k, dim3(nb), dim3(ST), 0, st, N, d_seg, idx, nseg, gk);
      FMX_HIP(hipGetLastError());
      FMX_TRY(sort_pairs(S, gk, gso, const_cast<uint32_t*>(idx), idx_b, N, key_bits(nseg)));
      gs = gso; idx = idx_b;
    }
    uint32_t *head = nullptr, *tailr = nullptr;
    FMX_TRY(S.get(&head, (size_t)N)); FMX_TRY(S.get(&tailr, (size_t)N));
    FMX_TRY(S.get(&start, (size_t)N)); FMX_TRY(S.get(&rend, (size_t)N));
    hipLaunchKernelGGL(sel_runs_k, dim3(nb), dim3(ST), 0, st, N, gs, head, tailr);
    FMX_HIP(hipGetLastError());
    FMX_TRY(inclusive_max(S, (const uint32_t*)head, start, N));
    FMX_TRY(inclusive_max(S, (const uint32_t*)tailr, rend, N));
  }
  hipLaunchKernelGGL(sel_part_k, dim3(nb), dim3(ST), 0, st, N, idx, gs, nseg, (const uint32_t*)start, (const uint32_t*)rend, d_key ? 1 : 0, ru, d_part);
  FMX_HIP(hipGetLastError());
  return FMX_OK;
}

__global__ __launch_bounds__(ST) void sel_group_part_k(int64_t n, const uint32_t* __restrict__ grp, int64_t G, const uint32_t* __restrict__ gpart,
                                                      uint32_t* __restrict__ part) {
  const int64_t r = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (r >= n) return;
  const uint32_t g = grp[r];
  part[r] = (int64_t)g < G ? gpart[g] : SEL_NONE;
}

// ---------------------------------------------------------------------------------------------------------------------------- take

// rows d_rows[0 .. n_take) (device i64) of m as a new matrix: the gather of one block
int take_rows(const fmx_matrix* m, const int64_t* d_rows, int64_t n_take, fmx_matrix** out) {
  GatherTab tab{};
  tab.nb = 1;
  GatherBlk& k = tab.b[0];
  k.rp = m->row_ptr; k.col = m->col; k.val = reinterpret_cast<const uint32_t*>(m->val);
  k.rows = d_rows; k.n = m->n; k.base = 0; k.L = m->fixed_row_len; k.unit = m->unit_values ? 1 : 0;
  fmx_matrix* o = nullptr;
  uint64_t bad = 0;
  int64_t longest = 0;   // (at most max_row_len: the core's other refusal cannot arise)
  FMX_TRY(gather_rows(m->device, tab, take_limits(), m->max_row_len, n_take, m->p, m->has_labels ? m->y : nullptr, d_rows, &o, &bad, &longest));
  FMX_CHECK(bad == GATHER_NO_BAD_KEY, FMX_ERR_INVALID, "rows[%lld] is outside 0..%lld", (long long)(bad / FMX_JOIN_MAX_BLOCKS), (long long)m->n - 1);
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> keep(o, free_matrix);
  if (!m->field_base.empty() && n_take > 0) {   // a field layout holds for every multiset of the source's rows
    o->rows_sorted = m->rows_sorted; o->unit_values = m->unit_values; o->max_row_len = m->max_row_len;
    o->fixed_row_len = m->fixed_row_len; o->dense_prefix = m->dense_prefix; o->field_base = m->field_base;
  } else {
    FMX_TRY(check_rows_sorted(o));
  }
  *out = keep.release();
  return FMX_OK;
}

// -------------------------------------------------------------------------------------------------------------------------- select

__global__ __launch_bounds__(ST) void select_flags_k(int64_t n, const uint32_t* __restrict__ part, uint32_t which, int complement, int64_t* __restrict__ flag) {
  const int64_t r = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (r > n) return;
  int64_t f = 0;
  if (r < n) {
    const uint32_t p = part[r];
    f = complement ? (p != which && p != SEL_NONE) : (p == which);
  }
  flag[r] = f;   // flag[n] = 0: the scan ends in the count
}

__global__ __launch_bounds__(ST) void select_rows_k(int64_t n, const int64_t* __restrict__ flag, const int64_t* __restrict__ pos, int64_t* __restrict__ rows) {
  const int64_t r = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (r < n && flag[r]) rows[pos[r]] = r;
}

// the ascending list of the selected rows into a buffer of its own (*d_rows, hipMalloc), their number into *count
int select_list(const fmx_matrix* m, const uint32_t* d_part, uint32_t which, int complement, DevBuf* rows, int64_t* count) {
  const hipStream_t st = nullptr;
  const int64_t n = m->n;
  Scratch S;
  int64_t *flag = nullptr, *pos = nullptr;
  FMX_TRY(S.get(&flag, (size_t)n + 1)); FMX_TRY(S.get(&pos, (size_t)n + 1));
  hipLaunchKernelGGL(select_flags_k, dim3(blocks(n + 1, ST)), dim3(ST), 0, st, n, d_part, which, complement, flag);
  FMX_HIP(hipGetLastError());
  FMX_TRY(exclusive_sum(S, (const int64_t*)flag, pos, n + 1));
  FMX_HIP(hipMemcpyAsync(count, pos + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  FMX_TRY(dev_buf(rows, (size_t)*count * sizeof(int64_t)));
  if (*count > 0) {
    hipLaunchKernelGGL(select_rows_k, dim3(blocks(n, ST)), dim3(ST), 0, st, n, (const int64_t*)flag, (const int64_t*)pos, (int64_t*)rows->get());
    FMX_HIP(hipGetLastError());
  }
  return FMX_OK;   // (S drains the device before its buffers go)
}

// ------------------------------------------------------------------------------------------------------------------------- entries

// the row of every entry and its key (null: the TAIL order needs none)
__global__ __launch_bounds__(ST) void entry_keys_k(const int64_t* __restrict__ rp, int64_t n, const uint32_t* __restrict__ col, int64_t nnz, uint64_t seed, uint64_t salt,
                                                  uint32_t* __restrict__ seg, uint64_t* __restrict__ key) {
  const int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (e >= nnz) return;
  int64_t lo = 0, hi = n;   // the row holding entry e: the last r with rp[r] <= e
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rp[mid] <= e) lo = mid; else hi = mid;
  }
  seg[e] = (uint32_t)lo;
  if (key) key[e] = pair_hash(seed, salt, ((uint64_t)lo << 32) | col[e], 2);
}

__global__ __launch_bounds__(ST) void entry_flags_k(int64_t nnz, const uint32_t* __restrict__ held, int64_t* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (e <= nnz) flag[e] = (e < nnz && !held[e]) ? 1 : 0;
}

// kpos[e] = kept entries before e: the two outputs' row offsets from the source's
__global__ __launch_bounds__(ST) void entry_ptrs_k(const int64_t* __restrict__ rp, int64_t n, const int64_t* __restrict__ kpos, int64_t* __restrict__ krp,
                                                  int64_t* __restrict__ hrp) {
  const int64_t r = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (r > n) return;
  const int64_t b = rp[r], k = kpos[b];
  krp[r] = k; hrp[r] = b - k;
}

__global__ __launch_bounds__(ST) void entry_scatter_k(int64_t nnz, const uint32_t* __restrict__ held, const int64_t* __restrict__ kpos, const uint32_t* __restrict__ col,
                                                     const uint32_t* __restrict__ val, uint32_t* __restrict__ kcol, uint32_t* __restrict__ kval,
                                                     uint32_t* __restrict__ hcol, uint32_t* __restrict__ hval) {
  const int64_t e = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (e >= nnz) return;
  const int64_t k = kpos[e];
  if (held[e]) { hcol[e - k] = col[e]; hval[e - k] = val[e]; }
  else { kcol[k] = col[e]; kval[k] = val[e]; }
}

int split_entries_run(const fmx_matrix* m, int order, const PartRule& ru, uint64_t seed, uint64_t salt, fmx_matrix** out_kept, fmx_matrix** out_held) {
  const hipStream_t st = nullptr;
  const int64_t n = m->n, nnz = m->nnz;
  Scratch S;
  uint32_t *seg = nullptr, *held = nullptr;
  uint64_t* key = nullptr;
  int64_t *flag = nullptr, *kpos = nullptr;
  FMX_TRY(S.get(&seg, (size_t)nnz)); FMX_TRY(S.get(&held, (size_t)nnz));
  if (order == FMX_SPLIT_ORDER_HASH) FMX_TRY(S.get(&key, (size_t)nnz));
  FMX_TRY(S.get(&flag, (size_t)nnz + 1)); FMX_TRY(S.get(&kpos, (size_t)nnz + 1));
  if (nnz > 0) {
    hipLaunchKernelGGL(entry_keys_k, dim3(blocks(nnz, ST)), dim3(ST), 0, st, m->row_ptr, n, m->col, nnz, seed, salt, seg, order == FMX_SPLIT_ORDER_HASH ? key : nullptr);
    FMX_HIP(hipGetLastError());
    FMX_TRY(seg_rank(S, st, nnz, seg, (uint64_t)n, true, order == FMX_SPLIT_ORDER_HASH ? key : nullptr, ru, held));
  }
  hipLaunchKernelGGL(entry_flags_k, dim3(blocks(nnz + 1, ST)), dim3(ST), 0, st, nnz, (const uint32_t*)held, flag);
  FMX_HIP(hipGetLastError());
  FMX_TRY(exclusive_sum(S, (const int64_t*)flag, kpos, nnz + 1));
  int64_t n_kept = 0;
  FMX_HIP(hipMemcpyAsync(&n_kept, kpos + nnz, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  fmx_matrix *k = nullptr, *h = nullptr;
  FMX_TRY(alloc_matrix(m->device, n, m->p, n_kept, m->has_labels != 0, &k));
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> keep_k(k, free_matrix);
  FMX_TRY(alloc_matrix(m->device, n, m->p, nnz - n_kept, m->has_labels != 0, &h));
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> keep_h(h, free_matrix);
  hipLaunchKernelGGL(entry_ptrs_k, dim3(blocks(n + 1, ST)), dim3(ST), 0, st, m->row_ptr, n, (const int64_t*)kpos, k->row_ptr, h->row_ptr);
  FMX_HIP(hipGetLastError());
  if (nnz > 0) {
    hipLaunchKernelGGL(entry_scatter_k, dim3(blocks(nnz, ST)), dim3(ST), 0, st, nnz, (const uint32_t*)held, (const int64_t*)kpos, m->col,
                       reinterpret_cast<const uint32_t*>(m->val), k->col, reinterpret_cast<uint32_t*>(k->val), h->col, reinterpret_cast<uint32_t*>(h->val));
    FMX_HIP(hipGetLastError());
  }
  if (m->has_labels && n > 0) {
    FMX_HIP(hipMemcpyAsync(k->y, m->y, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    FMX_HIP(hipMemcpyAsync(h->y, m->y, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
  }
  FMX_HIP(hipStreamSynchronize(st));
  FMX_TRY(check_rows_sorted(k));
  FMX_TRY(check_rows_sorted(h));
  *out_kept = keep_k.release();
  *out_held = keep_h.release();
  return FMX_OK;
}

// --------------------------------------------------------------------------------------------------------------------- permutation

__global__ __launch_bounds__(ST) void widen_k(int64_t n, const uint32_t* __restrict__ in, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * ST + threadIdx.x;
  if (i < n) out[i] = (int64_t)in[i];
}

int permutation_run(int64_t n, uint64_t seed, uint64_t epoch, int64_t* d_out) {
  if (n <= 0) return FMX_OK;
  const hipStream_t st = nullptr;
  Scratch S;
  uint64_t *key = nullptr, *key_out = nullptr;
  uint32_t *idx = nullptr, *idx_out = nullptr;
  FMX_TRY(S.get(&key, (size_t)n)); FMX_TRY(S.get(&key_out, (size_t)n)); FMX_TRY(S.get(&idx, (size_t)n)); FMX_TRY(S.get(&idx_out, (size_t)n));
  hipLaunchKernelGGL(sel_keys_k, dim3(blocks(n, ST)), dim3(ST), 0, st, n, seed, epoch, (uint64_t)3, key);
  hipLaunchKernelGGL(sel_iota_k, dim3(blocks(n, ST)), dim3(ST), 0, st, n, idx);
  FMX_HIP(hipGetLastError());
  FMX_TRY(sort_pairs(S, key, key_out, idx, idx_out, n, 64));
  hipLaunchKernelGGL(widen_k, dim3(blocks(n, ST)), dim3(ST), 0, st, n, (const uint32_t*)idx_out, d_out);
  FMX_HIP(hipGetLastError());
  FMX_HIP(hipStreamSynchronize(st));
  return FMX_OK;
}

// -------------------------------------------------------------------------------------------------------------------------- assign

// every refusal of a split rule; host only
int check_rule(int32_t order, int32_t n_folds, int64_t hold_count, double hold_fraction, int64_t min_keep) {
  FMX_CHECK(order == FMX_SPLIT_ORDER_HASH || order == FMX_SPLIT_ORDER_TAIL, FMX_ERR_INVALID, "unknown order %d", (int)order);
  FMX_CHECK(n_folds == 0 || (n_folds >= 2 && n_folds <= 65536), FMX_ERR_INVALID, "n_folds must be 0 (hold-out) or in 2..65536 (got %d)", (int)n_folds);
  FMX_CHECK(hold_count >= 0, FMX_ERR_INVALID, "hold_count must not be negative");
  FMX_CHECK(min_keep >= 0, FMX_ERR_INVALID, "min_keep must not be negative");
  FMX_CHECK(hold_fraction >= 0.0 && hold_fraction <= 1.0, FMX_ERR_INVALID, "hold_fraction must be in [0, 1]");   // (false for NaN)
  return FMX_OK;
}

int check_assign(int64_t n, bool groups, int64_t n_groups, const fmx_split_spec* spec, const void* out) {
  FMX_CHECK(spec != nullptr, FMX_ERR_INVALID, "spec is NULL");
  FMX_CHECK(spec->struct_size == sizeof(fmx_split_spec), FMX_ERR_INVALID, "spec.struct_size does not match this library");
  FMX_CHECK(spec->scope >= FMX_SPLIT_ROWS && spec->scope <= FMX_SPLIT_GROUPS, FMX_ERR_INVALID, "unknown scope %d", (int)spec->scope);
  FMX_TRY(check_rule(spec->order, spec->n_folds, spec->hold_count, spec->hold_fraction, spec->min_keep));
  FMX_CHECK(n >= 0 && n <= SEL_MAX_ITEMS, FMX_ERR_INVALID, "n must be in 0..2^31 - 1");
  FMX_CHECK(groups || spec->scope == FMX_SPLIT_ROWS, FMX_ERR_INVALID, "this scope needs the group of every row");
  FMX_CHECK(!groups || (n_groups >= 1 && n_groups <= SEL_MAX_ITEMS), FMX_ERR_INVALID, "n_groups must be in 1..2^31 - 1");
  FMX_CHECK(out != nullptr || n == 0, FMX_ERR_INVALID, "the output is NULL");
  return FMX_OK;
}

int assign_run(int64_t n, const uint32_t* d_group, int64_t G, const fmx_split_spec& sp, uint32_t* d_part) {
  if (n <= 0) return FMX_OK;
  const hipStream_t st = nullptr;
  Scratch S;
  const PartRule ru{sp.n_folds, sp.hold_count, sp.hold_fraction, sp.min_keep};
  const bool hash = sp.order == FMX_SPLIT_ORDER_HASH;
  if (sp.scope == FMX_SPLIT_GROUPS) {
    uint32_t* gpart = nullptr;
    uint64_t* key = nullptr;
    FMX_TRY(S.get(&gpart, (size_t)G));
    if (hash) {
      FMX_TRY(S.get(&key, (size_t)G));
      hipLaunchKernelGGL(sel_keys_k, dim3(blocks(G, ST)), dim3(ST), 0, st, G, sp.seed, sp.salt, (uint64_t)1, key);
      FMX_HIP(hipGetLastError());
    }
    FMX_TRY(seg_rank(S, st, G, nullptr, 1, false, key, ru, gpart));
    hipLaunchKernelGGL(sel_group_part_k, dim3(blocks(n, ST)), dim3(ST), 0, st, n, d_group, G, (const uint32_t*)gpart, d_part);
    FMX_HIP(hipGetLastError());
  } else {
    uint64_t* key = nullptr;
    if (hash) {
      FMX_TRY(S.get(&key, (size_t)n));
      hipLaunchKernelGGL(sel_keys_k, dim3(blocks(n, ST)), dim3(ST), 0, st, n, sp.seed, sp.salt, (uint64_t)0, key);
      FMX_HIP(hipGetLastError());
    }
    FMX_TRY(seg_rank(S, st, n, sp.scope == FMX_SPLIT_WITHIN_GROUPS ? d_group : nullptr, (uint64_t)G, false, key, ru, d_part));
  }
  FMX_HIP(hipStreamSynchronize(st));
  return FMX_OK;
}

}  // namespace

}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_free_device(void* dev_ptr) {
  if (dev_ptr) FMX_HIP(hipFree(dev_ptr));
  return FMX_OK;
}

int fmx_matrix_take_device(const fmx_matrix* m, const void* dev_rows_i64, int64_t n_take, fmx_matrix** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(n_take >= 0 && (dev_rows_i64 != nullptr || n_take == 0), FMX_ERR_INVALID, "n_take is negative or the row list is NULL");
  FMX_TRY(use_device(m->device));
  return take_rows(m, (const int64_t*)dev_rows_i64, n_take, out);
}

int fmx_matrix_take(const fmx_matrix* m, const int64_t* rows, int64_t n_take, fmx_matrix** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(n_take >= 0 && (rows != nullptr || n_take == 0), FMX_ERR_INVALID, "n_take is negative or the row list is NULL");
  for (int64_t t = 0; t < n_take; ++t)
    FMX_CHECK(rows[t] >= 0 && rows[t] < m->n, FMX_ERR_INVALID, "rows[%lld] = %lld is outside 0..%lld", (long long)t, (long long)rows[t], (long long)m->n - 1);
  FMX_TRY(use_device(m->device));
  DevBuf d;
  FMX_TRY(upload(&d, rows, n_take));
  return take_rows(m, (const int64_t*)d.get(), n_take, out);
}

int fmx_split_assign_device(int device, int64_t n, const void* dev_group_u32, int64_t n_groups, const fmx_split_spec* spec, void* dev_part_u32) {
  FMX_TRY(check_assign(n, dev_group_u32 != nullptr, n_groups, spec, dev_part_u32));
  FMX_TRY(use_device(device));
  return assign_run(n, (const uint32_t*)dev_group_u32, dev_group_u32 ? n_groups : 1, *spec, (uint32_t*)dev_part_u32);
}

int fmx_split_assign(int device, int64_t n, const uint32_t* group_of_row, int64_t n_groups, const fmx_split_spec* spec, uint32_t* out_part) {
  FMX_TRY(check_assign(n, group_of_row != nullptr, n_groups, spec, out_part));
  if (group_of_row)
    for (int64_t r = 0; r < n; ++r)
      FMX_CHECK((int64_t)group_of_row[r] < n_groups, FMX_ERR_INVALID, "group_of_row[%lld] = %u is outside 0..%lld", (long long)r, group_of_row[r], (long long)n_groups - 1);
  FMX_TRY(use_device(device));
  if (n == 0) return FMX_OK;
  DevBuf dg, dp;
  if (group_of_row) FMX_TRY(upload(&dg, group_of_row, n));
  FMX_TRY(dev_buf(&dp, (size_t)n * sizeof(uint32_t)));
  FMX_TRY(assign_run(n, (const uint32_t*)dg.get(), group_of_row ? n_groups : 1, *spec, (uint32_t*)dp.get()));
  FMX_HIP(hipMemcpy(out_part, dp.get(), (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return FMX_OK;
}

int fmx_matrix_select_device(const fmx_matrix* m, const void* dev_part_u32, uint32_t which, int32_t complement, fmx_matrix** out, void** dev_rows_i64) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (dev_rows_i64) *dev_rows_i64 = nullptr;
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(dev_part_u32 != nullptr || m->n == 0, FMX_ERR_INVALID, "the part array is NULL");
  FMX_TRY(use_device(m->device));
  DevBuf rows;
  int64_t count = 0;
  FMX_TRY(select_list(m, (const uint32_t*)dev_part_u32, which, complement ? 1 : 0, &rows, &count));
  FMX_TRY(take_rows(m, (const int64_t*)rows.get(), count, out));
  if (dev_rows_i64) *dev_rows_i64 = rows.release();
  return FMX_OK;
}

int fmx_matrix_select(const fmx_matrix* m, const uint32_t* part_of_row, uint32_t which, int32_t complement, fmx_matrix** out, int64_t* out_rows) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(part_of_row != nullptr || m->n == 0, FMX_ERR_INVALID, "the part array is NULL");
  FMX_TRY(use_device(m->device));
  DevBuf part, rows;
  FMX_TRY(upload(&part, part_of_row, m->n));
  int64_t count = 0;
  FMX_TRY(select_list(m, (const uint32_t*)part.get(), which, complement ? 1 : 0, &rows, &count));
  FMX_TRY(take_rows(m, (const int64_t*)rows.get(), count, out));
  if (out_rows && count > 0) {
    const hipError_t err = hipMemcpy(out_rows, rows.get(), (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost);
    if (err != hipSuccess) {
      free_matrix(*out);
      *out = nullptr;
      set_error("fmx_matrix_select: the copy of the row list failed: %s", hipGetErrorString(err));
      return FMX_ERR_HIP;
    }
  }
  return FMX_OK;
}

int fmx_matrix_split_entries(const fmx_matrix* m, int32_t order, int64_t hold_count, double hold_fraction, int64_t min_keep, uint64_t seed, uint64_t salt,
                             fmx_matrix** out_kept, fmx_matrix** out_held) {
  FMX_CHECK(out_kept != nullptr && out_held != nullptr, FMX_ERR_INVALID, "an output is NULL");
  *out_kept = nullptr; *out_held = nullptr;
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_TRY(check_rule(order, 0, hold_count, hold_fraction, min_keep));
  FMX_CHECK(m->n <= SEL_MAX_ITEMS && m->nnz <= SEL_MAX_ITEMS, FMX_ERR_INVALID, "at most 2^31 - 1 rows and stored entries per call");
  FMX_TRY(use_device(m->device));
  const PartRule ru{0, hold_count, hold_fraction, min_keep};
  return split_entries_run(m, order, ru, seed, salt, out_kept, out_held);
}

int fmx_row_permutation_device(int device, int64_t n, uint64_t seed, uint64_t epoch, void* dev_rows_i64) {
  FMX_CHECK(n >= 0 && n <= SEL_MAX_ITEMS, FMX_ERR_INVALID, "n must be in 0..2^31 - 1");
  FMX_CHECK(dev_rows_i64 != nullptr || n == 0, FMX_ERR_INVALID, "the output is NULL");
  FMX_TRY(use_device(device));
  return permutation_run(n, seed, epoch, (int64_t*)dev_rows_i64);
}

int fmx_row_permutation(int device, int64_t n, uint64_t seed, uint64_t epoch, int64_t* out_rows) {
  FMX_CHECK(n >= 0 && n <= SEL_MAX_ITEMS, FMX_ERR_INVALID, "n must be in 0..2^31 - 1");
  FMX_CHECK(out_rows != nullptr || n == 0, FMX_ERR_INVALID, "the output is NULL");
  FMX_TRY(use_device(device));
  if (n == 0) return FMX_OK;
  DevBuf d;
  FMX_TRY(dev_buf(&d, (size_t)n * sizeof(int64_t)));
  FMX_TRY(permutation_run(n, seed, epoch, (int64_t*)d.get()));
  FMX_HIP(hipMemcpy(out_rows, d.get(), (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
  return FMX_OK;
}

}  // extern "C"
