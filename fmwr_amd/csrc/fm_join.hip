// The row gather behind fmx_matrix_take*, fmx_matrix_select* and fmx_matrix_join* (gather_rows), and matrix composition on the
// device: fmx_matrix_join*, fmx_matrix_stack.  Everything is integer work and copied bits, so tests/join_model.py and tests/split_model.py reproduce
// every output bit for bit.
//
//   gather   row t of the output holds, block after block, the entries of row rows_b[t] of block b with col_base_b added to the column ids; an
//            INDICATOR block (no source matrix) contributes the one entry (col_base_b + rows_b[t], 1.0f).  A length pass with the range check (the
//            lowest t * 16 + b by atomicMin: the same answer whatever the order), an exclusive 64-bit scan whose total, the bad key and the longest
//            output row come back in ONE read, the allocation, then the entry copy in one of three forms that write the same bits:
//              fixed   every block has a fixed row length (an indicator: 1): the output position gives (t, j) by a division and the block by a
//                      prefix table, a lane moves four entries (16 bytes of columns, 16 of values); the reads are 16 bytes wide where every
//                      block's length is a multiple of four
//              group   output rows of at most GATHER_GROUP_MAX entries: a lane group per output row walks the blocks, sized by the mean output row
//              flat    longer rows: the output stream is cut into 16-byte pieces, a lane finds the row of its piece by binary search in the scanned
//                      offsets and walks on across blocks and rows
//            A unit-valued block's values are filled, not read.  The labels are copied by a kernel of their own.
//   join     the block table of the caller's blocks, the gather, the refusal's message and the flags of a join (join_layout, or the detector).
//   take     (fm_select.hip: take_rows) the gather of ONE block with base 0 and a row list, under take's own message and flags rule.  The kernels
//            that walk the table are compiled a second time with the block count fixed at one (NB = 1): the block loops fold and the record is read
//            through scalar loads.
//   stack    the parts' rows one after the other: device-to-device copies, and one kernel that adds each part's entry offset to its row pointers.
// The block table (at most 16 records) goes to the kernels by value; none of them uses scratch, LDS or a floating-point atomic.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <vector>

#include "fm_prims.h"
#include "fmx_test_hooks.h"

namespace fmx {
namespace {

constexpr int JT = 256;
constexpr int GATHER_GROUP_MAX = 512;              // longest output row of the group form
constexpr int64_t GATHER_LAUNCH_ROWS = 1LL << 22;  // output rows (flat form: 16-byte pieces) per launch
constexpr int64_t GATHER_MAX_ROW = 0x7FFFFFFFLL;   // entries of one output row
constexpr uint32_t ONE_BITS = 0x3F800000u;         // 1.0f
constexpr int STACK_MAX_PARTS = 1024;

// the sticky values of the two test hooks, as they were handed over: 0 the default, negative never
struct GatherHook {
  std::atomic<int> fixed{0}, group{0};
  std::atomic<int64_t> rows{0};
  void set(int fixed_entries, int group_entries, int64_t rows_per_launch) {
    fixed.store(fixed_entries);
    group.store(group_entries);
    rows.store(rows_per_launch > 0 ? rows_per_launch : 0);
  }
  GatherLimits limits() const {
    GatherLimits l{fixed.load(), group.load(), rows.load()};
    if (l.fixed_max == 0) l.fixed_max = 0x7FFFFFFF;
    if (l.group_max == 0 || l.group_max > GATHER_GROUP_MAX) l.group_max = GATHER_GROUP_MAX;
    if (l.launch_rows <= 0) l.launch_rows = GATHER_LAUNCH_ROWS;
    return l;
  }
};
GatherHook g_join_hook, g_take_hook;

// NB, the template parameter of the kernels that walk the table: 0 the table's own block count, 1 one block.  Every kernel reads the count as
// (NB ? NB : tab.nb) and a block as tab.b[NB == 1 ? 0 : b], in place: through a helper function, however it is inlined, the compiler arranges the
// NB = 0 kernels differently (profiles/gather_refactor.txt holds them to the instructions they had before there was an NB)
// len[t] of output row t (a block whose id is out of range counts 0 and sends t * 16 + b to flags[0] by atomicMin), len[n_out] = 0 so that the
// scan ends in the total.  want_max: the longest joined row goes to flags[1] -- a wave's maximum first, over shuffles, then one atomicMax per wave
// that still has something to add (the plain read only spares atomics: a stale value is a smaller one); the host asks for it only where its own
// bound, the sum of the sources' longest rows, does not settle the form
template <int NB>
__global__ __launch_bounds__(JT) void gather_len_k(const GatherTab tab, int64_t n_out, int want_max, int64_t* __restrict__ len, unsigned long long* __restrict__ flags) {
  const int64_t t = (int64_t)blockIdx.x * JT + threadIdx.x;
  int64_t l = 0;
  if (t < n_out) {
    for (int b = 0; b < (NB ? NB : tab.nb); ++b) {
      const GatherBlk& k = tab.b[NB == 1 ? 0 : b];
      const int64_t r = k.rows ? k.rows[t] : t;
      if (r < 0 || r >= k.n) atomicMin(flags, (unsigned long long)t * FMX_JOIN_MAX_BLOCKS + (unsigned long long)b);
      else l += !k.rp ? 1 : k.L > 0 ? k.L : k.rp[r + 1] - k.rp[r];   // (a source of fixed row length: rp[r + 1] - rp[r] is L)
    }
  }
  if (want_max) {   // (uniform: every lane of the wave takes part in the shuffles)
    int64_t w = l;
    for (int s = 32; s >= 1; s >>= 1) {
      const int64_t o = __shfl_xor(w, s);
      w = o > w ? o : w;
    }
    if ((threadIdx.x & 63) == 0 && (unsigned long long)w > flags[1]) atomicMax(flags + 1, (unsigned long long)w);
  }
  if (t <= n_out) len[t] = l;
}

__global__ __launch_bounds__(JT) void gather_labels_k(const int64_t* __restrict__ rows, int64_t t0, int64_t t1, const uint32_t* __restrict__ y,
                                                   uint32_t* __restrict__ oy) {
  const int64_t t = t0 + (int64_t)blockIdx.x * JT + threadIdx.x;
  if (t < t1) oy[t] = y[rows ? rows[t] : t];
}

// fixed form: output rows [t0, t1) of L = tab.Ltot entries each.  Thread q of the launch owns the 16-byte piece [4 Q, 4 Q + 4) of the output stream,
// Q = (t0 L) / 4 + q, clipped to the launch's entries [t0 L, t1 L): a piece that straddles two launches is shared between them entry by entry.
template <int NB, bool V4>
__global__ __launch_bounds__(JT) void gather_fixed_k(const GatherTab tab, int64_t t0, int64_t t1, uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval) {
  const int L = tab.Ltot;
  const int64_t e0 = t0 * L, e1 = t1 * L;
  const int64_t o = ((e0 >> 2) + (int64_t)blockIdx.x * JT + threadIdx.x) << 2;
  if (o >= e1) return;
  int64_t t = o / L;
  int j = (int)(o - t * L);
  int b = 0;
  while (b + 1 < (NB ? NB : tab.nb) && j >= tab.b[b + 1].pre) ++b;
  if (V4) {   // every block's length is a multiple of 4 (no indicator): a piece lies inside one block, all of it 16-byte aligned, e0 and e1 multiples of 4
    const GatherBlk& k = tab.b[NB == 1 ? 0 : b];
    const int64_t src = (k.rows ? k.rows[t] : t) * k.L + (j - k.pre);
    uint4 c = *reinterpret_cast<const uint4*>(k.col + src);
    c.x += k.base; c.y += k.base; c.z += k.base; c.w += k.base;
    *reinterpret_cast<uint4*>(ocol + o) = c;
    *reinterpret_cast<uint4*>(oval + o) = k.unit ? make_uint4(ONE_BITS, ONE_BITS, ONE_BITS, ONE_BITS) : *reinterpret_cast<const uint4*>(k.val + src);
    return;
  }
  uint32_t c[4] = {0, 0, 0, 0}, v[4] = {ONE_BITS, ONE_BITS, ONE_BITS, ONE_BITS};
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int64_t e = o + x;
    if (e >= e0 && e < e1) {
      const GatherBlk& k = tab.b[NB == 1 ? 0 : b];
      const int64_t r = k.rows ? k.rows[t] : t;
      if (k.rp) {
        const int64_t src = r * k.L + (j - k.pre);
        c[x] = k.col[src] + k.base;
        if (!k.unit) v[x] = k.val[src];
      } else {
        c[x] = (uint32_t)r + k.base;
      }
    }
    if (++j == L) { j = 0; b = 0; ++t; }
    else if (b + 1 < (NB ? NB : tab.nb) && j >= tab.b[b + 1].pre) ++b;   // every block holds at least one entry: one step at most
  }
  if (o >= e0 && o + 4 <= e1) {
    *reinterpret_cast<uint4*>(ocol + o) = make_uint4(c[0], c[1], c[2], c[3]);
    *reinterpret_cast<uint4*>(oval + o) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x)
      if (o + x >= e0 && o + x < e1) { ocol[o + x] = c[x]; oval[o + x] = v[x]; }
  }
}

// group form: G lanes (a power of two, at most 64) per output row of [t0, t1) walk the blocks
template <int NB>
__global__ __launch_bounds__(JT) void gather_group_k(const GatherTab tab, const int64_t* __restrict__ off, int64_t t0, int64_t t1, int G,
                                                  uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval) {
  const int64_t t = t0 + ((int64_t)blockIdx.x * JT + threadIdx.x) / G;
  const int lane = threadIdx.x & (G - 1);
  if (t >= t1) return;
  int64_t d = off[t];
  for (int b = 0; b < (NB ? NB : tab.nb); ++b) {
    const GatherBlk& k = tab.b[NB == 1 ? 0 : b];
    const int64_t r = k.rows ? k.rows[t] : t;
    if (!k.rp) {
      if (lane == 0) { ocol[d] = (uint32_t)r + k.base; oval[d] = ONE_BITS; }
      ++d;
      continue;
    }
    const int64_t s0 = k.rp[r], len = k.rp[r + 1] - s0;
    for (int64_t x = lane; x < len; x += G) {
      ocol[d + x] = k.col[s0 + x] + k.base;
      oval[d + x] = k.unit ? ONE_BITS : k.val[s0 + x];
    }
    d += len;
  }
}

// flat form: the 16-byte pieces [q0, q1) of the output stream of all n_out rows; a lane finds the row of its piece's first entry by binary search in
// the scanned offsets (the last t with off[t] <= e: the row that holds e, since an empty row shares its offset with the row after it) and walks on
// across blocks and rows
template <int NB>
__global__ __launch_bounds__(JT) void gather_flat_k(const GatherTab tab, const int64_t* __restrict__ off, int64_t n_out, int64_t q0, int64_t q1, int64_t total,
                                                 uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval) {
  const int64_t q = q0 + (int64_t)blockIdx.x * JT + threadIdx.x;
  if (q >= q1) return;
  const int64_t o = q << 2;
  const int cnt = (int)(total - o < 4 ? total - o : 4);   // q1 <= ceil(total / 4): cnt >= 1
  int64_t lo = 0, hi = n_out - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= o) lo = mid; else hi = mid - 1;
  }
  int64_t t = lo;
  int b = -1;
  int64_t d0 = off[t], d1 = d0;   // the output positions [d0, d1) of block b of row t; s0: its first source entry, or the indicator's id
  int64_t s0 = 0;
  uint32_t c[4] = {0, 0, 0, 0}, v[4] = {ONE_BITS, ONE_BITS, ONE_BITS, ONE_BITS};
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    if (x < cnt) {
      const int64_t e = o + x;
      while (e >= d1) {   // e < total = off[n_out]: t stays below n_out
        if (++b == (NB ? NB : tab.nb)) { b = 0; ++t; }
        const GatherBlk& k = tab.b[NB == 1 ? 0 : b];
        const int64_t r = k.rows ? k.rows[t] : t;
        d0 = d1;
        if (k.rp) { s0 = k.rp[r]; d1 = d0 + (k.rp[r + 1] - s0); }
        else { s0 = r; d1 = d0 + 1; }
      }
      const GatherBlk& k = tab.b[NB == 1 ? 0 : b];
      if (k.rp) {
        c[x] = k.col[s0 + (e - d0)] + k.base;
        if (!k.unit) v[x] = k.val[s0 + (e - d0)];
      } else {
        c[x] = (uint32_t)s0 + k.base;
      }
    }
  }
  if (cnt == 4) {
    *reinterpret_cast<uint4*>(ocol + o) = make_uint4(c[0], c[1], c[2], c[3]);
    *reinterpret_cast<uint4*>(oval + o) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x)
      if (x < cnt) { ocol[o + x] = c[x]; oval[o + x] = v[x]; }
  }
}

// the flags of a join that qualifies (include/fmx.h): every block an indicator or a field layout, the shifted ranges ascending without overlap, a
// dense prefix in block 0 alone and only under col_base 0.  False: the output goes through the detector
bool join_layout(const fmx_join_block* blk, int nb, uint32_t out_p, fmx_matrix* o) {
  std::vector<uint32_t> base;
  uint64_t end = 0;
  int dense = 0, len = 0, sorted = 1, unit = 1;
  for (int b = 0; b < nb; ++b) {
    const fmx_matrix* m = blk[b].m;
    const uint64_t lo = blk[b].col_base, hi = lo + (m ? (uint64_t)m->p : (uint64_t)blk[b].n_ids);
    if (lo < end || hi <= lo) return false;
    end = hi;
    if (!m) {
      base.push_back((uint32_t)lo);
      len += 1;
      continue;
    }
    if (m->field_base.empty() || m->fixed_row_len <= 0 || (int)m->field_base.size() != m->fixed_row_len - m->dense_prefix + 1) return false;
    if (m->dense_prefix > 0 && (b != 0 || lo != 0)) return false;
    if (b == 0) dense = m->dense_prefix;
    for (size_t c = 0; c + 1 < m->field_base.size(); ++c) base.push_back((uint32_t)(lo + m->field_base[c]));
    len += m->fixed_row_len;
    sorted = sorted && m->rows_sorted;
    unit = unit && m->unit_values;
  }
  if (base.empty() || (int)base.size() > FMX_MAX_FIELDS || len > 64) return false;
  base[0] = (uint32_t)dense;   // the first field's range opens at the dense prefix, as fmx_matrix_set_fields wants it
  base.push_back(out_p);
  for (size_t c = 0; c + 1 < base.size(); ++c)
    if (base[c] >= base[c + 1]) return false;
  o->rows_sorted = sorted; o->unit_values = unit; o->max_row_len = len; o->fixed_row_len = len; o->dense_prefix = dense;
  o->field_base = base;
  return true;
}

// the checks of both entry points that need no device
int join_check(const fmx_join_block* blk, int32_t nb, int64_t n_out, int32_t labels_from) {
  FMX_CHECK(blk != nullptr, FMX_ERR_INVALID, "blocks is NULL");
  FMX_CHECK(nb >= 1 && nb <= FMX_JOIN_MAX_BLOCKS, FMX_ERR_INVALID, "n_blocks must be in 1..%d (got %d)", FMX_JOIN_MAX_BLOCKS, (int)nb);
  FMX_CHECK(n_out >= 0, FMX_ERR_INVALID, "n_out must not be negative");
  for (int b = 0; b < nb; ++b) {
    if (blk[b].m) {
      FMX_CHECK(blk[b].rows != nullptr || blk[b].m->n == n_out, FMX_ERR_INVALID, "block %d has no row list and its source holds %lld rows, not n_out = %lld", b,
                (long long)blk[b].m->n, (long long)n_out);
    } else {
      FMX_CHECK(blk[b].n_ids >= 0, FMX_ERR_INVALID, "block %d: n_ids must not be negative", b);
      FMX_CHECK(blk[b].rows != nullptr || n_out == 0, FMX_ERR_INVALID, "block %d is an indicator block and has no id list", b);
    }
  }
  FMX_CHECK(labels_from >= -1 && labels_from < nb, FMX_ERR_INVALID, "labels_from must be -1 or a block index below %d (got %d)", (int)nb, (int)labels_from);
  if (labels_from >= 0)
    FMX_CHECK(blk[labels_from].m != nullptr && blk[labels_from].m->has_labels, FMX_ERR_INVALID, "labels_from names block %d, which %s", (int)labels_from,
              blk[labels_from].m ? "has no labels" : "is an indicator block");
  return FMX_OK;
}

// the checks that come before any launch (they read nothing but the host records either)
int join_check_ranges(int device, const fmx_join_block* blk, int nb, uint32_t out_p) {
  for (int b = 0; b < nb; ++b)
    FMX_CHECK(!blk[b].m || blk[b].m->device == device, FMX_ERR_INVALID, "block %d's source is on device %d, not %d", b, blk[b].m ? blk[b].m->device : -1, device);
  for (int b = 0; b < nb; ++b) {
    const uint64_t width = blk[b].m ? (uint64_t)blk[b].m->p : (uint64_t)blk[b].n_ids;
    FMX_CHECK((uint64_t)blk[b].col_base + width <= (uint64_t)out_p, FMX_ERR_INVALID, "block %d: col_base %u + %llu columns exceed out_p = %u", b, blk[b].col_base,
              (unsigned long long)width, out_p);
  }
  return FMX_OK;
}

// The gather (fmx_internal.h: gather_rows) with the kernels of block count NB.  The table's pre and Ltot are filled here
template <int NB>
int gather_run(int device, GatherTab tab, const GatherLimits& lim, int64_t bound, int64_t n_out, uint32_t out_p, const float* y_src, const int64_t* y_rows,
               fmx_matrix** out, uint64_t* bad_key, int64_t* longest_row) {
  const hipStream_t st = nullptr;
  bool all_fixed = true, v4 = true;
  int64_t ltot = 0;
  for (int b = 0; b < tab.nb; ++b) {
    GatherBlk& k = tab.b[b];
    k.pre = (int)std::min<int64_t>(ltot, 0x7FFFFFFF);
    if (k.L <= 0) all_fixed = false;
    if (k.L & 3) v4 = false;
    ltot += k.L > 0 ? k.L : 0;
  }
  tab.Ltot = (int)std::min<int64_t>(ltot, 0x7FFFFFFF);
  Scratch S;
  int64_t *len = nullptr, *off = nullptr;   // off[n_out + 1]: the lowest bad t * 16 + b (all ones: none), off[n_out + 2]: the longest output row, beside the total
  FMX_TRY(S.get(&len, (size_t)n_out + 1)); FMX_TRY(S.get(&off, (size_t)n_out + 3));
  FMX_HIP(hipMemsetAsync(off + n_out + 1, 0xFF, sizeof(int64_t), st));
  // the longest output row is at most the caller's bound: where that keeps every row in the group form, nothing is measured (nor cleared, nor read)
  const int want_max = ((lim.group_max > 0 && bound > lim.group_max) || bound > GATHER_MAX_ROW) ? 1 : 0;
  if (want_max) FMX_HIP(hipMemsetAsync(off + n_out + 2, 0, sizeof(int64_t), st));
  hipLaunchKernelGGL(gather_len_k<NB>, dim3(blocks(n_out + 1, JT)), dim3(JT), 0, st, tab, n_out, want_max, len, reinterpret_cast<unsigned long long*>(off + n_out + 1));
  FMX_HIP(hipGetLastError());
  FMX_TRY(exclusive_sum(S, (const int64_t*)len, off, n_out + 1));
  int64_t back[3] = {0, 0, 0};
  FMX_HIP(hipMemcpyAsync(back, off + n_out, sizeof(back), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  const int64_t total = back[0], longest = want_max ? back[2] : bound;
  *bad_key = (uint64_t)back[1];
  *longest_row = longest;
  if (back[1] != -1 || longest > GATHER_MAX_ROW) return FMX_OK;   // the caller's refusal, in its own words
  fmx_matrix* o = nullptr;
  FMX_TRY(alloc_matrix(device, n_out, out_p, total, y_src != nullptr, &o));
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> keep(o, free_matrix);
  FMX_HIP(hipMemcpyAsync(o->row_ptr, off, (size_t)(n_out + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  uint32_t *ocol = o->col, *oval = reinterpret_cast<uint32_t*>(o->val);
  const int L = tab.Ltot;
  const int form = (all_fixed && lim.fixed_max > 0 && ltot <= lim.fixed_max) ? 0 : (lim.group_max > 0 && longest <= lim.group_max) ? 1 : 2;
  if (form == 2 && total > 0) {
    const int64_t pieces = (total + 3) >> 2;
    for (int64_t q0 = 0; q0 < pieces; q0 += lim.launch_rows) {
      const int64_t q1 = std::min(pieces, q0 + lim.launch_rows);
      hipLaunchKernelGGL(gather_flat_k<NB>, dim3(blocks(q1 - q0, JT)), dim3(JT), 0, st, tab, (const int64_t*)off, n_out, q0, q1, total, ocol, oval);
      FMX_HIP(hipGetLastError());
    }
  }
  int G = 2;
  if (form == 1 && n_out > 0)
    while (G < 64 && (int64_t)G * n_out < total) G <<= 1;   // the mean output row length, rounded up to a power of two
  for (int64_t t0 = 0; t0 < n_out; t0 += lim.launch_rows) {
    const int64_t t1 = std::min(n_out, t0 + lim.launch_rows);
    if (form == 0 && total > 0) {
      const int64_t pieces = ((t1 * L + 3) >> 2) - ((t0 * L) >> 2);
      if (v4) hipLaunchKernelGGL((gather_fixed_k<NB, true>), dim3(blocks(pieces, JT)), dim3(JT), 0, st, tab, t0, t1, ocol, oval);
      else hipLaunchKernelGGL((gather_fixed_k<NB, false>), dim3(blocks(pieces, JT)), dim3(JT), 0, st, tab, t0, t1, ocol, oval);
      FMX_HIP(hipGetLastError());
    } else if (form == 1 && total > 0) {
      hipLaunchKernelGGL(gather_group_k<NB>, dim3(blocks((t1 - t0) * G, JT)), dim3(JT), 0, st, tab, (const int64_t*)off, t0, t1, G, ocol, oval);
      FMX_HIP(hipGetLastError());
    }
    if (y_src) {
      hipLaunchKernelGGL(gather_labels_k, dim3(blocks(t1 - t0, JT)), dim3(JT), 0, st, y_rows, t0, t1, reinterpret_cast<const uint32_t*>(y_src),
                         reinterpret_cast<uint32_t*>(o->y));
      FMX_HIP(hipGetLastError());
    }
  }
  FMX_HIP(hipStreamSynchronize(st));
  *out = keep.release();
  return FMX_OK;
}

// d_rows[b]: the device row list of block b, or null
int join_run(int device, const fmx_join_block* blk, int nb, const int64_t* const* d_rows, int64_t n_out, uint32_t out_p, int labels_from, fmx_matrix** out) {
  GatherTab tab{};
  tab.nb = nb;
  int64_t bound = 0;   // the longest joined row is at most the sum of the sources' longest rows
  for (int b = 0; b < nb; ++b) {
    const fmx_matrix* m = blk[b].m;
    GatherBlk& k = tab.b[b];
    k.rp = m ? m->row_ptr : nullptr;
    k.col = m ? m->col : nullptr;
    k.val = m ? reinterpret_cast<const uint32_t*>(m->val) : nullptr;
    k.rows = d_rows[b];
    k.n = m ? m->n : blk[b].n_ids;
    k.base = blk[b].col_base;
    k.L = m ? m->fixed_row_len : 1;
    k.unit = m ? (m->unit_values ? 1 : 0) : 1;
    bound += m ? m->max_row_len : 1;
  }
  fmx_matrix* o = nullptr;
  uint64_t bad = 0;
  int64_t longest = 0;
  FMX_TRY(gather_rows(device, tab, g_join_hook.limits(), bound, n_out, out_p, labels_from >= 0 ? blk[labels_from].m->y : nullptr,
                      labels_from >= 0 ? d_rows[labels_from] : nullptr, &o, &bad, &longest));
  if (bad != GATHER_NO_BAD_KEY) {
    const int b = (int)(bad % FMX_JOIN_MAX_BLOCKS);
    FMX_CHECK(false, FMX_ERR_INVALID, "rows[%lld] of block %d is outside 0..%lld", (long long)(bad / FMX_JOIN_MAX_BLOCKS), b, (long long)tab.b[b].n - 1);
  }
  FMX_CHECK(o != nullptr, FMX_ERR_INVALID, "a joined row would hold %lld entries: at most 2^31 - 1", (long long)longest);
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> keep(o, free_matrix);
  if (!(n_out > 0 && join_layout(blk, nb, out_p, o))) FMX_TRY(check_rows_sorted(o));
  *out = keep.release();
  return FMX_OK;
}

// out_rp[row0[k] + r] = rp_k[r] + e0[k] for every row r of part k, out_rp[n] = the total; the part of an output row by binary search in row0
__global__ __launch_bounds__(JT) void stack_ptrs_k(int n_parts, const int64_t* const* __restrict__ part_rp, const int64_t* __restrict__ row0,
                                                  const int64_t* __restrict__ e0, int64_t n, int64_t* __restrict__ out_rp) {
  const int64_t r = (int64_t)blockIdx.x * JT + threadIdx.x;
  if (r > n) return;
  if (r == n) { out_rp[n] = e0[n_parts]; return; }
  int lo = 0, hi = n_parts - 1;   // the last part k with row0[k] <= r: the one that holds r (an empty part shares its first row with the part after it)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (row0[mid] <= r) lo = mid; else hi = mid - 1;
  }
  out_rp[r] = part_rp[lo][r - row0[lo]] + e0[lo];
}

int stack_run(const fmx_matrix* const* parts, int n_parts, bool labels, fmx_matrix** out) {
  const hipStream_t st = nullptr;
  std::vector<int64_t> tabs(2 * ((size_t)n_parts + 1), 0);   // row0[n_parts + 1] | e0[n_parts + 1]
  int64_t *row0 = tabs.data(), *e0 = tabs.data() + n_parts + 1;
  std::vector<const int64_t*> rps((size_t)n_parts);
  for (int k = 0; k < n_parts; ++k) {
    row0[k + 1] = row0[k] + parts[k]->n;
    e0[k + 1] = e0[k] + parts[k]->nnz;
    rps[(size_t)k] = parts[k]->row_ptr;
  }
  const int64_t n = row0[n_parts], total = e0[n_parts];
  const fmx_matrix* first = parts[0];
  fmx_matrix* o = nullptr;
  FMX_TRY(alloc_matrix(first->device, n, first->p, total, labels, &o));
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> keep(o, free_matrix);
  Scratch S;
  int64_t* d_tabs = nullptr;
  const int64_t** d_rps = nullptr;
  FMX_TRY(S.get(&d_tabs, tabs.size())); FMX_TRY(S.get(&d_rps, rps.size()));
  FMX_HIP(hipMemcpyAsync(d_tabs, tabs.data(), tabs.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
  FMX_HIP(hipMemcpyAsync(d_rps, rps.data(), rps.size() * sizeof(const int64_t*), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(stack_ptrs_k, dim3(blocks(n + 1, JT)), dim3(JT), 0, st, n_parts, (const int64_t* const*)d_rps, (const int64_t*)d_tabs,
                     (const int64_t*)(d_tabs + n_parts + 1), n, o->row_ptr);
  FMX_HIP(hipGetLastError());
  bool same = !first->field_base.empty();
  int sorted = 1, unit = 1, longest = 0;
  for (int k = 0; k < n_parts; ++k) {
    const fmx_matrix* m = parts[k];
    if (m->nnz > 0) {
      FMX_HIP(hipMemcpyAsync(o->col + e0[k], m->col, (size_t)m->nnz * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      FMX_HIP(hipMemcpyAsync(o->val + e0[k], m->val, (size_t)m->nnz * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (labels && m->n > 0) FMX_HIP(hipMemcpyAsync(o->y + row0[k], m->y, (size_t)m->n * sizeof(float), hipMemcpyDeviceToDevice, st));
    same = same && m->field_base == first->field_base && m->dense_prefix == first->dense_prefix && m->fixed_row_len == first->fixed_row_len;
    sorted = sorted && m->rows_sorted;
    unit = unit && m->unit_values;
    longest = std::max(longest, m->max_row_len);
  }
  FMX_HIP(hipStreamSynchronize(st));   // (the host tables are read by the copies above)
  if (same && n > 0) {   // rows that all satisfy one field layout satisfy it together
    o->rows_sorted = sorted; o->unit_values = unit; o->max_row_len = longest;
    o->fixed_row_len = first->fixed_row_len; o->dense_prefix = first->dense_prefix; o->field_base = first->field_base;
  } else {
    FMX_TRY(check_rows_sorted(o));
  }
  *out = keep.release();
  return FMX_OK;
}

}  // namespace

GatherLimits take_limits() { return g_take_hook.limits(); }

int gather_rows(int device, const GatherTab& tab, const GatherLimits& lim, int64_t bound_longest, int64_t n_out, uint32_t out_p, const float* y_src,
                const int64_t* y_rows, fmx_matrix** out, uint64_t* bad_key, int64_t* longest) {
  *out = nullptr;
  return tab.nb == 1 ? gather_run<1>(device, tab, lim, bound_longest, n_out, out_p, y_src, y_rows, out, bad_key, longest)
                     : gather_run<0>(device, tab, lim, bound_longest, n_out, out_p, y_src, y_rows, out, bad_key, longest);
}

}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_debug_join_limits(int32_t fixed_entries, int32_t group_entries, int64_t rows_per_launch) {
  g_join_hook.set(fixed_entries, group_entries, rows_per_launch);
  return FMX_OK;
}

int fmx_debug_take_limits(int32_t fixed_entries, int32_t group_entries, int64_t rows_per_launch) {
  g_take_hook.set(fixed_entries, group_entries, rows_per_launch);
  return FMX_OK;
}

int fmx_matrix_join_device(int device, const fmx_join_block* blocks, int32_t n_blocks, int64_t n_out, uint32_t out_p, int32_t labels_from, fmx_matrix** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_TRY(join_check(blocks, n_blocks, n_out, labels_from));
  FMX_TRY(join_check_ranges(device, blocks, n_blocks, out_p));
  FMX_TRY(use_device(device));
  const int64_t* d_rows[FMX_JOIN_MAX_BLOCKS] = {};
  for (int b = 0; b < n_blocks; ++b) d_rows[b] = (const int64_t*)blocks[b].rows;
  return join_run(device, blocks, n_blocks, d_rows, n_out, out_p, labels_from, out);
}

int fmx_matrix_join(int device, const fmx_join_block* blocks, int32_t n_blocks, int64_t n_out, uint32_t out_p, int32_t labels_from, fmx_matrix** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_TRY(join_check(blocks, n_blocks, n_out, labels_from));
  FMX_TRY(join_check_ranges(device, blocks, n_blocks, out_p));
  FMX_TRY(use_device(device));
  DevBuf bufs[FMX_JOIN_MAX_BLOCKS];
  const int64_t* d_rows[FMX_JOIN_MAX_BLOCKS] = {};
  for (int b = 0; b < n_blocks; ++b) {
    if (!blocks[b].rows) continue;
    FMX_TRY(upload(&bufs[b], (const int64_t*)blocks[b].rows, n_out));
    d_rows[b] = (const int64_t*)bufs[b].get();
  }
  return join_run(device, blocks, n_blocks, d_rows, n_out, out_p, labels_from, out);
}

int fmx_matrix_stack(const fmx_matrix* const* parts, int32_t n_parts, fmx_matrix** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(parts != nullptr, FMX_ERR_INVALID, "parts is NULL");
  FMX_CHECK(n_parts >= 1 && n_parts <= STACK_MAX_PARTS, FMX_ERR_INVALID, "n_parts must be in 1..%d (got %d)", STACK_MAX_PARTS, (int)n_parts);
  int labelled = 0;
  for (int k = 0; k < n_parts; ++k) {
    FMX_CHECK(parts[k] != nullptr, FMX_ERR_INVALID, "part %d is NULL", k);
    FMX_CHECK(parts[k]->p == parts[0]->p, FMX_ERR_INVALID, "part %d has %u features, part 0 has %u", k, parts[k]->p, parts[0]->p);
    FMX_CHECK(parts[k]->device == parts[0]->device, FMX_ERR_INVALID, "part %d is on device %d, part 0 on device %d", k, parts[k]->device, parts[0]->device);
    labelled += parts[k]->has_labels ? 1 : 0;
  }
  FMX_CHECK(labelled == 0 || labelled == n_parts, FMX_ERR_INVALID, "%d of the %d parts have labels: all of them or none", labelled, (int)n_parts);
  FMX_TRY(use_device(parts[0]->device));
  return stack_run(parts, n_parts, labelled > 0, out);
}

}  // extern "C"
