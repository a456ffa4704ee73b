// Target and count encoding on the device: fmx_target_stats*, fmx_target_table_*, fmx_matrix_encode_targets*.  The fit counts, per
// (slot, part) CELL, the rows that store an encoded column, the positive ones among them and -- FMX_TARGET_LABEL -- the sum of their labels in the order of
// fmx_matrix_column_stats; the apply turns the ids of the encoded segments into MEAN and COUNT columns and leaves a row's own part out.  Integers, copied
// bits and floating-point chains in one stated order: tests/target_model.py restates every output bit for bit.
//
//   table    two device arrays of RECORDS, one record per slot.
//              cnt  i64[W][RC]: {N, A, (rows, positive rows) of part 0, 1, ...}; N and A are the sums over the parts.  RC = 4, 8 or 16 words for up to
//                   1, 3 or 7 parts -- a power of two, so a record never straddles a 128-byte line: what an entry of the apply needs, the totals and its
//                   own part's cell, is ONE line for n_parts <= 7 -- and a multiple of 16 words above that (the totals' line and the part's line).
//              sum  f64[W][RS] (FMX_TARGET_LABEL): {T, the sum of part 0, 1, ...}, T the chain over the parts; RS = 2, 4, 8, 16 words for up to 1, 3, 7, 15
//                   parts, a multiple of 16 above.  A LABEL entry reads one line of either array.
//   terms    one device block (TermTab) every kernel stages in LDS: per term the column range [lo, hi), the first slot, the first output column and the
//            kinds.  term_of is a branch-free binary search over lo (the terms' segments ascend strictly, so their ranges ascend and do not overlap).
//   fit      unit    a one-hot source with strictly ascending rows under FMX_TARGET_POSITIVE: 64-bit integer atomics per entry straight into the cells.
//            sorted  everything else: the entries inside an encoded segment of a row with a valid part are compacted (flags, one 64-bit scan, a scatter),
//                    sorted by (slot * n_parts + part, entry index) -- a stable radix sort: rows ascend inside a cell's run and same-row duplicates are
//                    adjacent --, the heads of equal-row runs (and those of positive rows) counted by ONE scan of the packed flags, as cst_heads_k does.
//                    LABEL: the heads' rows are scattered to a list by their scanned rank; a wave sums a chunk of 1 024 rows of a cell (lane strides of 64
//                    from +0.0, xor butterfly 32 .. 1), one thread per cell adds its chunk sums ascending.  No atomics.
//            Both end in tt_totals_k: N, A and T of every slot.
//   apply    length  a lane group per row ORs the bits of the terms the row holds (enc_len_k); fm_prims' 64-bit scan; the total comes back in one read.
//            fill    three forms that write the same bits:
//              single  a source of fixed row length whose layout puts exactly one entry of every encoded segment at a fixed position: no length pass,
//                      arithmetic row pointers, a thread per 16-byte piece of the output stream, as cross_single_k (enc_single_k)
//              group   rows of at most group_entries (<= 64) entries, a lane per entry: per term the lanes of the term's entries gather their records, the
//                      integer sums meet in an xor butterfly and the LABEL chain walks the set bits of the ballot in source order (enc_rows_k)
//              long    longer rows: the same kernel with a whole wave per row, walking the row in chunks of 64 entries per term
// No floating-point atomic, no scratch.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "fm_prims.h"
#include "fmx_test_hooks.h"

struct fmx_target_table {
  int device = 0;
  uint32_t p = 0;
  int n_parts = 1, target = 0;
  std::vector<uint32_t> segment_base, term_segment;
  std::vector<uint32_t> term_base;   // [n_terms + 1]
  int64_t W = 0;
  int RC = 4, RS = 0;                // words of a record of cnt / sum
  int64_t* cnt = nullptr;
  double* sum = nullptr;
};

namespace fmx {
namespace {

constexpr int TT = 256;
constexpr int TG_MAX_SEGMENTS = 4096;
constexpr int TG_MAX_TERMS = 64;
constexpr int TG_MAX_PARTS = 64;
constexpr int TG_CHUNK = 1024;                    // rows of a cell per chunk of its sum
constexpr int TG_GROUP_MAX = 64;                  // longest row of the group form: a lane per entry
constexpr int64_t TG_LAUNCH_ENTRIES = 1LL << 28;
constexpr int64_t TG_LAUNCH_ROWS = 1LL << 22;
constexpr int64_t TG_MAX_ITEMS = 0x7FFFFFFFLL;
constexpr uint64_t TG_MAX_WIDTH = 0xFFFFFFFEull;
constexpr uint32_t TG_NONE = 0xFFFFFFFFu;
constexpr uint32_t TG_ONE = 0x3F800000u;          // 1.0f
constexpr uint32_t TG_NAN32 = 0x7FC00000u;
constexpr unsigned long long TG_NAN64 = 0x7FF8000000000000ull;

std::atomic<int> g_single{0}, g_group{0};
std::atomic<int64_t> g_chunk{0}, g_rows{0};

struct TgLimits {
  bool single;          // the apply may take the single form
  int group_max;        // rows of at most this many entries take the group form (< 0: none does, and the fit never takes the unit form)
  int64_t chunk_entries, launch_rows;
};
TgLimits tg_limits() {
  TgLimits l{g_single.load() >= 0, g_group.load(), g_chunk.load(), g_rows.load()};
  if (l.group_max == 0 || l.group_max > TG_GROUP_MAX) l.group_max = TG_GROUP_MAX;
  if (l.group_max < 0) l.group_max = -1;
  if (l.chunk_entries <= 0) l.chunk_entries = TG_LAUNCH_ENTRIES;
  if (l.launch_rows <= 0) l.launch_rows = TG_LAUNCH_ROWS;
  return l;
}

// f(a, b) for the cuts [a, b) of [0, total) of at most `cut` items
template <typename F>
int in_cuts(int64_t total, int64_t cut, F f) {
  for (int64_t a = 0; a < total; a += cut) FMX_TRY(f(a, std::min(total, a + cut)));
  return FMX_OK;
}

// the terms as the kernels read them.  lo: in the single form of the apply the POSITION of the term's entry inside a source row goes to pos
struct TermTab {
  uint32_t lo[TG_MAX_TERMS], hi[TG_MAX_TERMS];   // the term's columns
  uint32_t tb[TG_MAX_TERMS];                     // its first slot
  uint32_t ob[TG_MAX_TERMS];                     // its first output column (enc_base[t])
  uint32_t kind[TG_MAX_TERMS];
  uint32_t pos[TG_MAX_TERMS];
  uint32_t om[2 * TG_MAX_TERMS];                 // the single form: new entry j of an output row is term om[j] & 0xFF, its second column if om[j] >> 8
};
constexpr int TERMTAB_WORDS = sizeof(TermTab) / sizeof(uint32_t);

struct TabD {   // the table as the kernels see it
  int64_t* cnt;
  double* sum;   // null: FMX_TARGET_POSITIVE
  int RC, RS, P;
};

__device__ __forceinline__ void tt_stage(const TermTab* __restrict__ src, TermTab* lds) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d = reinterpret_cast<uint32_t*>(lds);
  for (int i = threadIdx.x; i < TERMTAB_WORDS; i += TT) d[i] = s[i];
  __syncthreads();
}

// the term whose columns hold c, or -1: the last t with lo[t] <= c, if c < hi[t] (an empty term shares its lo with the next one and is never the answer)
__device__ __forceinline__ int term_of(const TermTab& T, int n_terms, uint32_t c) {
  uint32_t a = 0, len = (uint32_t)n_terms;   // a ends as #{t : lo[t] <= c}
  while (len > 0) {
    const uint32_t half = len >> 1;
    const bool le = T.lo[a + half] <= c;
    a = le ? a + half + 1 : a;
    len = le ? len - half - 1 : half;
  }
  if (a == 0) return -1;
  return c < T.hi[a - 1] ? (int)a - 1 : -1;
}

// the row holding entry e: the last r in [0, n) with rp[r] <= e; with rows of L > 0 entries each, a division
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ rp, int64_t n, int64_t e, int L) {
  if (L > 0) return e / L;
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (rp[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ double canon64(double x) { return x != x ? __longlong_as_double((long long)TG_NAN64) : x; }

// ------------------------------------------------------------------------------------------------------------------------------- fit

struct FitArgs {
  const int64_t* rp;
  int64_t n;
  int L;
  const uint32_t* col;
  const float* y;
  const uint32_t* part;   // null: every row is part 0
  const TermTab* tt;
  int n_terms, P;
};

// the cell of entry e, or TG_NONE: outside every encoded segment, or a row without a valid part
__device__ __forceinline__ uint32_t cell_of(const FitArgs& a, const TermTab& T, int64_t e, int64_t* row) {
  const uint32_t c = a.col[e];
  const int t = term_of(T, a.n_terms, c);
  if (t < 0) return TG_NONE;
  const int64_t r = row_of(a.rp, a.n, e, a.L);
  const uint32_t f = a.part ? a.part[r] : 0u;
  if (f >= (uint32_t)a.P) return TG_NONE;
  *row = r;
  return (T.tb[t] + (c - T.lo[t])) * (uint32_t)a.P + f;   // < W * n_parts <= 2^31 - 1
}

// unit form, entries [e0, e1): a one-hot source with strictly ascending rows holds no column twice in a row, so every entry is a row of its cell
__global__ __launch_bounds__(TT) void tfit_unit_k(const FitArgs a, int64_t e0, int64_t e1, TabD tab) {
  __shared__ TermTab T;
  tt_stage(a.tt, &T);
  const int64_t e = e0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (e >= e1) return;
  int64_t r = 0;
  const uint32_t k = cell_of(a, T, e, &r);
  if (k == TG_NONE) return;
  const size_t slot = k / (uint32_t)a.P, f = k % (uint32_t)a.P;
  unsigned long long* rec = reinterpret_cast<unsigned long long*>(tab.cnt) + slot * (size_t)tab.RC + 2 + 2 * f;
  atomicAdd(rec, 1ull);
  if (a.y[r] > 0.0f) atomicAdd(rec + 1, 1ull);
}

// sorted form, entries [e0, e1): the cell of every entry and whether it takes part (flag[nnz] = 0: the scan ends in the total)
__global__ __launch_bounds__(TT) void tfit_keys_k(const FitArgs a, int64_t e0, int64_t e1, uint32_t* __restrict__ key, int64_t* __restrict__ flag) {
  __shared__ TermTab T;
  tt_stage(a.tt, &T);
  const int64_t e = e0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (e >= e1) return;
  int64_t r = 0;
  const uint32_t k = cell_of(a, T, e, &r);
  key[e] = k;
  flag[e] = k != TG_NONE ? 1 : 0;
}

__global__ __launch_bounds__(TT) void tfit_compact_k(int64_t e0, int64_t e1, const uint32_t* __restrict__ key, const int64_t* __restrict__ pos, uint32_t* __restrict__ kc,
                                                    uint32_t* __restrict__ ec) {
  const int64_t e = e0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (e >= e1) return;
  const uint32_t k = key[e];
  if (k == TG_NONE) return;
  const int64_t q = pos[e];
  kc[q] = k; ec[q] = (uint32_t)e;
}

// positions [q0, q1) of the (cell, entry) order: the head of an equal-row run as 1 in the low half of hf[q], a head whose row is positive as 1 in the high
// half too (one 64-bit scan counts both: a call holds fewer than 2^31 entries, so the low half never carries)
__global__ __launch_bounds__(TT) void tfit_heads_k(const FitArgs a, const uint32_t* __restrict__ ks, const uint32_t* __restrict__ es, int64_t q0, int64_t q1,
                                                  uint64_t* __restrict__ hf) {
  const int64_t q = q0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (q >= q1) return;
  const uint32_t k = ks[q];
  const int64_t r = row_of(a.rp, a.n, (int64_t)es[q], a.L);
  uint64_t f = 0;
  if (!(q > 0 && ks[q - 1] == k && row_of(a.rp, a.n, (int64_t)es[q - 1], a.L) == r)) f = 1ull | (a.y[r] > 0.0f ? (1ull << 32) : 0ull);
  hf[q] = f;
}

// LABEL: the row of every head at its scanned rank -- the cells' row lists, one behind the other, rows ascending inside a cell
__global__ __launch_bounds__(TT) void tfit_rows_k(const FitArgs a, const uint32_t* __restrict__ es, const uint64_t* __restrict__ hf, const uint64_t* __restrict__ hs,
                                                 int64_t q0, int64_t q1, uint32_t* __restrict__ hrow) {
  const int64_t q = q0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (q >= q1 || !(hf[q] & 1ull)) return;
  hrow[hs[q] & 0xFFFFFFFFull] = (uint32_t)row_of(a.rp, a.n, (int64_t)es[q], a.L);
}

// cells [k0, k1) of [0, cells]: the counts of a cell from its run [off[k], off[k + 1]) and the scanned head flags, and its chunks (nch[cells] = 0)
__global__ __launch_bounds__(TT) void tfit_cells_k(int64_t cells, int64_t k0, int64_t k1, const int64_t* __restrict__ off, const uint64_t* __restrict__ hs, TabD tab,
                                                  int64_t* __restrict__ nch) {
  const int64_t k = k0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (k >= k1) return;
  int64_t rows = 0;
  if (k < cells) {
    const uint64_t d = hs[off[k + 1]] - hs[off[k]];   // both halves ascend along the scan: no borrow
    rows = (int64_t)(d & 0xFFFFFFFFull);
    const size_t slot = (size_t)(k / tab.P), f = (size_t)(k % tab.P);
    int64_t* rec = tab.cnt + slot * (size_t)tab.RC + 2 + 2 * f;
    rec[0] = rows; rec[1] = (int64_t)(d >> 32);
  }
  if (nch) nch[k] = (rows + TG_CHUNK - 1) / TG_CHUNK;
}

// one wave per chunk w of [w0, w1): psum[w]
__global__ __launch_bounds__(TT) void tfit_chunks_k(int64_t cells, const int64_t* __restrict__ off, const uint64_t* __restrict__ hs, const int64_t* __restrict__ coff,
                                                   const uint32_t* __restrict__ hrow, const float* __restrict__ y, int64_t w0, int64_t w1, double* __restrict__ psum) {
  const int64_t w = w0 + ((int64_t)blockIdx.x * TT + threadIdx.x) / 64;
  const int lane = threadIdx.x & 63;
  double s = 0.0;
  if (w < w1) {
    int64_t lo = 0, hi = cells;   // the cell of chunk w: the last k with coff[k] <= w (a cell without rows shares its offset with the next one)
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (coff[mid] <= w) lo = mid; else hi = mid;
    }
    const int64_t h0 = (int64_t)(hs[off[lo]] & 0xFFFFFFFFull), h1 = (int64_t)(hs[off[lo + 1]] & 0xFFFFFFFFull);
    const int64_t a = h0 + (w - coff[lo]) * TG_CHUNK;
    const int64_t b = a + TG_CHUNK < h1 ? a + TG_CHUNK : h1;
    for (int64_t q = a + lane; q < b; q += 64) s = __dadd_rn(s, (double)y[hrow[q]]);
  }
#pragma unroll
  for (int st = 32; st > 0; st >>= 1) s = __dadd_rn(s, __shfl_xor(s, st, 64));
  if (w < w1 && lane == 0) psum[w] = s;
}

__global__ __launch_bounds__(TT) void tfit_sums_k(int64_t k0, int64_t k1, const int64_t* __restrict__ coff, const double* __restrict__ psum, TabD tab) {
  const int64_t k = k0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (k >= k1) return;
  double s = 0.0;
  for (int64_t w = coff[k]; w < coff[k + 1]; ++w) s = __dadd_rn(s, psum[w]);
  tab.sum[(size_t)(k / tab.P) * (size_t)tab.RS + 1 + (size_t)(k % tab.P)] = canon64(s);
}

// slots [s0, s1): N, A and T from the cells
__global__ __launch_bounds__(TT) void tt_totals_k(int64_t s0, int64_t s1, TabD tab) {
  const int64_t s = s0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (s >= s1) return;
  int64_t* rec = tab.cnt + (size_t)s * (size_t)tab.RC;
  uint64_t N = 0, A = 0;   // (wraps like the model's int64 on counts no fit can give)
  for (int g = 0; g < tab.P; ++g) { N += (uint64_t)rec[2 + 2 * g]; A += (uint64_t)rec[3 + 2 * g]; }
  rec[0] = (int64_t)N; rec[1] = (int64_t)A;
  if (tab.sum) {
    double* sr = tab.sum + (size_t)s * (size_t)tab.RS;
    double t = 0.0;
    for (int g = 0; g < tab.P; ++g) t = __dadd_rn(t, sr[1 + g]);
    sr[0] = canon64(t);
  }
}

// cells [k0, k1): record <-> the exchange layout count[cell][2], sum[cell]
__global__ __launch_bounds__(TT) void tt_unpack_k(int64_t k0, int64_t k1, TabD tab, int64_t* __restrict__ count, double* __restrict__ sum) {
  const int64_t k = k0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (k >= k1) return;
  const size_t slot = (size_t)(k / tab.P), f = (size_t)(k % tab.P);
  if (count) { count[2 * k] = tab.cnt[slot * (size_t)tab.RC + 2 + 2 * f]; count[2 * k + 1] = tab.cnt[slot * (size_t)tab.RC + 3 + 2 * f]; }
  if (sum) sum[k] = tab.sum[slot * (size_t)tab.RS + 1 + f];
}

__global__ __launch_bounds__(TT) void tt_pack_k(int64_t k0, int64_t k1, TabD tab, const int64_t* __restrict__ count, const double* __restrict__ sum) {
  const int64_t k = k0 + (int64_t)blockIdx.x * TT + threadIdx.x;
  if (k >= k1) return;
  const size_t slot = (size_t)(k / tab.P), f = (size_t)(k % tab.P);
  tab.cnt[slot * (size_t)tab.RC + 2 + 2 * f] = count[2 * k]; tab.cnt[slot * (size_t)tab.RC + 3 + 2 * f] = count[2 * k + 1];
  if (sum) tab.sum[slot * (size_t)tab.RS + 1 + f] = sum[k];
}

// ----------------------------------------------------------------------------------------------------------------------------- apply

struct EncArgs {
  const int64_t* rp;
  const uint32_t* col;
  const uint32_t* val;    // null: every value is 1.0f
  const uint32_t* part;   // null: every row is encoded with the totals
  const TermTab* tt;
  const int64_t* cnt;
  const double* sum;      // null: FMX_TARGET_POSITIVE
  int RC, RS, P, n_terms, keep;
  double pm, strength;    // pm = prior * strength, rounded on the host
  uint32_t prior_bits;    // (float) prior
  uint64_t mean_mask, count_mask;   // the terms with a MEAN / a COUNT column
};

// what one entry adds: dn to n, da to the integer a, x to the LABEL chain.  f: the row's part, TG_NONE for the totals
__device__ __forceinline__ void enc_entry(const EncArgs& a, size_t slot, uint32_t f, uint64_t* dn, uint64_t* da, double* x) {
  const int64_t* rec = a.cnt + slot * (size_t)a.RC;
  const longlong2 tot = *reinterpret_cast<const longlong2*>(rec);   // (records start on 16 bytes: RC is even)
  uint64_t n = (uint64_t)tot.x, p = (uint64_t)tot.y;
  if (f != TG_NONE) {
    const longlong2 own = *reinterpret_cast<const longlong2*>(rec + 2 + 2 * (size_t)f);
    n -= (uint64_t)own.x; p -= (uint64_t)own.y;
  }
  *dn = n; *da = p;
  if (a.sum) {
    const double* sr = a.sum + slot * (size_t)a.RS;
    const double t = sr[0];
    *x = f != TG_NONE ? __dsub_rn(t, sr[1 + (size_t)f]) : t;
  }
}

__device__ __forceinline__ void enc_values(const EncArgs& a, uint64_t un, uint64_t ua, double chain, uint32_t* mean, uint32_t* count) {
  const long long n = (long long)un;
  const double av = a.sum ? chain : __ll2double_rn((long long)ua);
  const double den = __dadd_rn(__ll2double_rn(n), a.strength);
  const float m = den == 0.0 ? __uint_as_float(a.prior_bits) : __double2float_rn(__ddiv_rn(__dadd_rn(av, a.pm), den));
  *mean = m != m ? TG_NAN32 : __float_as_uint(m);
  *count = __float_as_uint(__ll2float_rn(n));
}

// the valid part of row r, or TG_NONE
__device__ __forceinline__ uint32_t enc_part(const EncArgs& a, int64_t r) {
  if (!a.part) return TG_NONE;
  const uint32_t f = a.part[r];
  return f < (uint32_t)a.P ? f : TG_NONE;
}

// rows [r0, r1), G lanes each: len[r] = the entries of output row r
__global__ __launch_bounds__(TT) void enc_len_k(const EncArgs a, int64_t r0, int64_t r1, int G, int64_t* __restrict__ len) {
  __shared__ TermTab T;
  tt_stage(a.tt, &T);
  const int64_t r = r0 + ((int64_t)blockIdx.x * TT + threadIdx.x) / G;
  const int lane = threadIdx.x & (G - 1);
  const bool live = r < r1;
  const int64_t s0 = live ? a.rp[r] : 0;
  const int64_t n = live ? a.rp[r + 1] - s0 : 0;
  uint64_t held = 0;
  for (int64_t x = lane; x < n; x += G) {
    const int t = term_of(T, a.n_terms, a.col[s0 + x]);
    if (t >= 0) held |= 1ull << t;
  }
  for (int s = G >> 1; s >= 1; s >>= 1) held |= __shfl_xor(held, s, G);   // (every lane of the wave is here)
  if (live && lane == 0) len[r] = (a.keep ? n : 0) + __popcll(held & a.mean_mask) + __popcll(held & a.count_mask);
}

// out_rp[t] = t * Lo for t = 0 .. n
__global__ __launch_bounds__(TT) void enc_ptrs_k(int64_t n, int64_t Lo, int64_t* __restrict__ out_rp) {
  const int64_t t = (int64_t)blockIdx.x * TT + threadIdx.x;
  if (t <= n) out_rp[t] = t * Lo;
}

// single form: output rows [t0, t1) of Lo = keep L + NE entries, NE the new columns.  Thread q owns the 16-byte piece [4 Q, 4 Q + 4) of the output stream,
// Q = (t0 Lo) / 4 + q, clipped to the launch's entries (as cross_single_k, fm_cross.hip)
__global__ __launch_bounds__(TT) void enc_single_k(const EncArgs a, int L, int NE, int64_t t0, int64_t t1, uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval) {
  __shared__ TermTab T;
  tt_stage(a.tt, &T);
  const int kL = a.keep ? L : 0;
  const int Lo = kL + NE;
  const int64_t e0 = t0 * Lo, e1 = t1 * Lo;
  const int64_t o = ((e0 >> 2) + (int64_t)blockIdx.x * TT + threadIdx.x) << 2;
  if (o >= e1) return;
  int64_t t = o / Lo;
  int j = (int)(o - t * Lo);
  uint32_t c[4] = {0, 0, 0, 0}, v[4] = {TG_ONE, TG_ONE, TG_ONE, TG_ONE};
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int64_t e = o + x;
    if (e >= e0 && e < e1) {
      const int64_t s0 = t * L;
      if (j < kL) {
        c[x] = a.col[s0 + j];
        if (a.val) v[x] = a.val[s0 + j];
      } else {
        const uint32_t w = T.om[j - kL];
        const int tm = (int)(w & 0xFFu), second = (int)(w >> 8);
        const uint32_t id = a.col[s0 + T.pos[tm]];
        uint64_t dn = 0, da = 0;
        double xs = 0.0;
        if (id >= T.lo[tm] && id < T.hi[tm]) enc_entry(a, (size_t)T.tb[tm] + (id - T.lo[tm]), enc_part(a, t), &dn, &da, &xs);   // (the layout promises it)
        uint32_t mean, count;
        enc_values(a, dn, da, __dadd_rn(0.0, xs), &mean, &count);
        c[x] = T.ob[tm] + (uint32_t)second;
        v[x] = (T.kind[tm] & FMX_ENCODE_MEAN) && !second ? mean : count;
      }
    }
    if (++j == Lo) { j = 0; ++t; }
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

// group and long form: rows [r0, r1) of more than min_len and at most max_len entries, G lanes each (the group form: max_len <= G, one chunk; the long
// form: G = 64, a wave walks the row in chunks of 64 entries, once per term)
__global__ __launch_bounds__(TT) void enc_rows_k(const EncArgs a, const int64_t* __restrict__ off, int64_t r0, int64_t r1, int G, int64_t min_len, int64_t max_len,
                                                uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval) {
  __shared__ TermTab T;
  tt_stage(a.tt, &T);
  const int64_t r = r0 + ((int64_t)blockIdx.x * TT + threadIdx.x) / G;
  const int lane = threadIdx.x & (G - 1);
  const int gsh = (threadIdx.x & 63) & ~(G - 1);
  const uint64_t gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
  const bool live = r < r1;
  const int64_t s0 = live ? a.rp[r] : 0;
  int64_t n = live ? a.rp[r + 1] - s0 : 0;
  if (n <= min_len || n > max_len) n = 0;   // (the whole lane group: the other form's row, or a row that emits nothing)
  int64_t d = n > 0 ? off[r] : 0;
  if (a.keep) {
    for (int64_t x = lane; x < n; x += G) { ocol[d + x] = a.col[s0 + x]; oval[d + x] = a.val ? a.val[s0 + x] : TG_ONE; }
    d += n;
  }
  const uint32_t f = n > 0 ? enc_part(a, r) : TG_NONE;
  uint32_t c0 = 0;   // the first chunk's entry and its term: a short row is searched once
  int t0 = -1;
  if (lane < n) { c0 = a.col[s0 + lane]; t0 = term_of(T, a.n_terms, c0); }
  for (int t = 0; t < a.n_terms; ++t) {   // (uniform)
    uint64_t un = 0, ua = 0;
    double chain = 0.0;
    bool any = false;
    for (int64_t x0 = 0; x0 < n; x0 += G) {   // (uniform over the lane group: the shuffles below stay inside it)
      const int64_t x = x0 + lane;
      uint32_t c = c0;
      int tm = t0;
      if (x0 > 0) {
        tm = -1;
        if (x < n) { c = a.col[s0 + x]; tm = term_of(T, a.n_terms, c); }
      }
      const bool mine = tm == t;
      uint64_t dn = 0, da = 0;
      double xs = 0.0;
      if (mine) enc_entry(a, (size_t)T.tb[t] + (c - T.lo[t]), f, &dn, &da, &xs);
      uint64_t m = (__ballot(mine) >> gsh) & gmask;
      if (m == 0) continue;
      any = true;
      for (int s = G >> 1; s >= 1; s >>= 1) { dn += __shfl_xor(dn, s, G); da += __shfl_xor(da, s, G); }
      un += dn; ua += da;
      if (a.sum)
        while (m) {   // the chain takes the entries in source order
          const int src = __ffsll((unsigned long long)m) - 1;
          chain = __dadd_rn(chain, __shfl(xs, gsh + src, 64));
          m &= m - 1;
        }
    }
    if (!any) continue;
    const uint32_t kind = T.kind[t];
    if (lane == 0) {
      uint32_t mean, count;
      enc_values(a, un, ua, chain, &mean, &count);
      int at = 0;
      if (kind & FMX_ENCODE_MEAN) { ocol[d] = T.ob[t]; oval[d] = mean; at = 1; }
      if (kind & FMX_ENCODE_COUNT) { ocol[d + at] = T.ob[t] + (uint32_t)at; oval[d + at] = count; }
    }
    d += __popc(kind);
  }
}

// ------------------------------------------------------------------------------------------------------------------------------ host

void free_table(fmx_target_table* t) {
  if (!t) return;
  if (t->cnt) (void)hipFree(t->cnt);
  if (t->sum) (void)hipFree(t->sum);
  delete t;
}
using TableHold = std::unique_ptr<fmx_target_table, void (*)(fmx_target_table*)>;

// the words of a record of `need` words: the next power of two up to 16, a multiple of 16 above -- a record never straddles a 128-byte line it need not
int record_words(int need, int least) {
  int w = least;
  while (w < need && w < 16) w <<= 1;
  return w >= need ? w : (need + 15) / 16 * 16;
}

// every refusal of a layout that can be seen without the matrix; host only
int layout_check(const fmx_target_spec* sp, std::vector<uint32_t>* term_base) {
  FMX_CHECK(sp != nullptr, FMX_ERR_INVALID, "spec is NULL");
  FMX_CHECK(sp->struct_size == sizeof(fmx_target_spec), FMX_ERR_INVALID, "spec.struct_size does not match this library");
  FMX_CHECK(sp->reserved == 0, FMX_ERR_INVALID, "spec.reserved must be 0");
  FMX_CHECK(sp->n_segments >= 1 && sp->n_segments <= TG_MAX_SEGMENTS, FMX_ERR_INVALID, "n_segments must be in 1..%d (got %d)", TG_MAX_SEGMENTS, (int)sp->n_segments);
  FMX_CHECK(sp->n_terms >= 1 && sp->n_terms <= TG_MAX_TERMS, FMX_ERR_INVALID, "n_terms must be in 1..%d (got %d)", TG_MAX_TERMS, (int)sp->n_terms);
  FMX_CHECK(sp->n_parts >= 1 && sp->n_parts <= TG_MAX_PARTS, FMX_ERR_INVALID, "n_parts must be in 1..%d (got %d)", TG_MAX_PARTS, (int)sp->n_parts);
  FMX_CHECK(sp->target == FMX_TARGET_POSITIVE || sp->target == FMX_TARGET_LABEL, FMX_ERR_INVALID, "unknown target %d", (int)sp->target);
  FMX_CHECK(sp->segment_base != nullptr, FMX_ERR_INVALID, "spec.segment_base is NULL");
  FMX_CHECK(sp->term_segment != nullptr, FMX_ERR_INVALID, "spec.term_segment is NULL");
  const uint32_t* base = sp->segment_base;
  FMX_CHECK(base[0] == 0, FMX_ERR_INVALID, "spec.segment_base must start at 0");
  for (int32_t s = 0; s < sp->n_segments; ++s)
    FMX_CHECK(base[s] <= base[s + 1], FMX_ERR_INVALID, "spec.segment_base descends at segment %d", (int)s);
  term_base->assign((size_t)sp->n_terms + 1, 0u);
  uint64_t W = 0;
  for (int32_t t = 0; t < sp->n_terms; ++t) {
    const uint32_t s = sp->term_segment[t];
    FMX_CHECK(s < (uint32_t)sp->n_segments, FMX_ERR_INVALID, "term %d names segment %u: there are %d segments", (int)t, s, (int)sp->n_segments);
    FMX_CHECK(t == 0 || sp->term_segment[t - 1] < s, FMX_ERR_INVALID, "spec.term_segment does not ascend strictly at term %d", (int)t);
    W += (uint64_t)(base[s + 1] - base[s]);
    FMX_CHECK(W * (uint64_t)sp->n_parts <= (uint64_t)TG_MAX_ITEMS, FMX_ERR_INVALID, "the encoded segments hold %llu columns: with %d parts above 2^31 - 1 cells",
              (unsigned long long)W, (int)sp->n_parts);
    (*term_base)[(size_t)t + 1] = (uint32_t)W;
  }
  return FMX_OK;
}

int stats_check(const fmx_matrix* m, const fmx_target_spec* sp, fmx_target_table** out, std::vector<uint32_t>* term_base) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_TRY(layout_check(sp, term_base));
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(sp->segment_base[sp->n_segments] == m->p, FMX_ERR_INVALID, "spec.segment_base ends at %u, not at the feature count %u", sp->segment_base[sp->n_segments], m->p);
  FMX_CHECK(m->has_labels != 0, FMX_ERR_INVALID, "the matrix has no labels: a target encoding needs them");
  FMX_CHECK(m->n <= TG_MAX_ITEMS && m->nnz <= TG_MAX_ITEMS, FMX_ERR_INVALID, "at most 2^31 - 1 rows and stored entries per call");
  return FMX_OK;
}

// an empty table (every cell 0) of the layout on the current device
int table_alloc(int device, const fmx_target_spec* sp, const std::vector<uint32_t>& term_base, TableHold* hold) {
  fmx_target_table* t = new fmx_target_table();
  hold->reset(t);
  t->device = device;
  t->p = sp->segment_base[sp->n_segments];
  t->n_parts = sp->n_parts;
  t->target = sp->target;
  t->segment_base.assign(sp->segment_base, sp->segment_base + sp->n_segments + 1);
  t->term_segment.assign(sp->term_segment, sp->term_segment + sp->n_terms);
  t->term_base = term_base;
  t->W = term_base.back();
  t->RC = record_words(2 + 2 * sp->n_parts, 4);
  t->RS = sp->target == FMX_TARGET_LABEL ? record_words(1 + sp->n_parts, 2) : 0;
  const size_t cb = (size_t)std::max<int64_t>(t->W, 1) * (size_t)t->RC * sizeof(int64_t);
  FMX_HIP(hipMalloc(&t->cnt, cb));
  FMX_HIP(hipMemsetAsync(t->cnt, 0, cb, nullptr));
  if (t->RS) {
    const size_t sb = (size_t)std::max<int64_t>(t->W, 1) * (size_t)t->RS * sizeof(double);
    FMX_HIP(hipMalloc(&t->sum, sb));
    FMX_HIP(hipMemsetAsync(t->sum, 0, sb, nullptr));
  }
  return FMX_OK;
}

TabD tab_of(const fmx_target_table* t) { return TabD{t->cnt, t->sum, t->RC, t->RS, t->n_parts}; }

void terms_of(const fmx_target_table* t, TermTab* tt) {
  std::memset(tt, 0, sizeof(*tt));
  for (size_t k = 0; k < t->term_segment.size(); ++k) {
    tt->lo[k] = t->segment_base[t->term_segment[k]];
    tt->hi[k] = t->segment_base[t->term_segment[k] + 1];
    tt->tb[k] = t->term_base[k];
  }
}

int totals_run(const fmx_target_table* t, const TgLimits& lim, hipStream_t st) {
  return in_cuts(t->W, lim.launch_rows, [&](int64_t a, int64_t b) {
    hipLaunchKernelGGL(tt_totals_k, dim3(blocks(b - a, TT)), dim3(TT), 0, st, a, b, tab_of(t));
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  });
}

int stats_run(const fmx_matrix* m, const uint32_t* d_part, fmx_target_table* t) {
  const TgLimits lim = tg_limits();
  const int64_t n = m->n, nnz = m->nnz, cells = t->W * t->n_parts;
  const int n_terms = (int)t->term_segment.size();
  const bool label = t->target == FMX_TARGET_LABEL;
  Scratch S;
  const hipStream_t st = S.st;
  if (cells == 0 || nnz == 0) { FMX_HIP(hipStreamSynchronize(st)); return FMX_OK; }
  TermTab tt;
  terms_of(t, &tt);
  TermTab* dtt = nullptr;
  FMX_TRY(S.get(&dtt, 1));
  FMX_HIP(hipMemcpyAsync(dtt, &tt, sizeof(tt), hipMemcpyHostToDevice, st));
  const FitArgs a{m->row_ptr, n, m->fixed_row_len, m->col, m->y, d_part, dtt, n_terms, t->n_parts};
  const TabD tab = tab_of(t);
  if (m->unit_values && m->rows_sorted && !label && lim.group_max >= 0) {
    FMX_TRY(in_cuts(nnz, lim.chunk_entries, [&](int64_t e0, int64_t e1) {
      hipLaunchKernelGGL(tfit_unit_k, dim3(blocks(e1 - e0, TT)), dim3(TT), 0, st, a, e0, e1, tab);
      FMX_HIP(hipGetLastError());
      return FMX_OK;
    }));
    FMX_TRY(totals_run(t, lim, st));
    FMX_HIP(hipStreamSynchronize(st));   // (the host table is read by the copy above)
    return FMX_OK;
  }
  uint32_t* key = nullptr;
  int64_t *flag = nullptr, *pos = nullptr;
  FMX_TRY(S.get(&key, (size_t)nnz)); FMX_TRY(S.get(&flag, (size_t)nnz + 1)); FMX_TRY(S.get(&pos, (size_t)nnz + 1));
  FMX_HIP(hipMemsetAsync(flag + nnz, 0, sizeof(int64_t), st));
  FMX_TRY(in_cuts(nnz, lim.chunk_entries, [&](int64_t e0, int64_t e1) {
    hipLaunchKernelGGL(tfit_keys_k, dim3(blocks(e1 - e0, TT)), dim3(TT), 0, st, a, e0, e1, key, flag);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }));
  FMX_TRY(exclusive_sum(S, (const int64_t*)flag, pos, nnz + 1));
  int64_t M = 0;   // the entries that take part
  FMX_HIP(hipMemcpyAsync(&M, pos + nnz, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  FMX_HIP(hipStreamSynchronize(st));
  if (M == 0) return FMX_OK;
  uint32_t *kc = nullptr, *ec = nullptr, *ks = nullptr, *es = nullptr;
  FMX_TRY(S.get(&kc, (size_t)M)); FMX_TRY(S.get(&ec, (size_t)M)); FMX_TRY(S.get(&ks, (size_t)M)); FMX_TRY(S.get(&es, (size_t)M));
  FMX_TRY(in_cuts(nnz, lim.chunk_entries, [&](int64_t e0, int64_t e1) {
    hipLaunchKernelGGL(tfit_compact_k, dim3(blocks(e1 - e0, TT)), dim3(TT), 0, st, e0, e1, (const uint32_t*)key, (const int64_t*)pos, kc, ec);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }));
  FMX_TRY(sort_pairs(S, kc, ks, ec, es, M, key_bits((uint64_t)cells - 1)));   // stable: entry indices ascend in a run
  int64_t* off = nullptr;
  FMX_TRY(S.get(&off, (size_t)cells + 1));
  FMX_TRY(group_offsets(ks, M, cells, off, st));
  uint64_t *hf = nullptr, *hs = nullptr;
  FMX_TRY(S.get(&hf, (size_t)M + 1)); FMX_TRY(S.get(&hs, (size_t)M + 1));
  FMX_HIP(hipMemsetAsync(hf + M, 0, sizeof(uint64_t), st));
  FMX_TRY(in_cuts(M, lim.chunk_entries, [&](int64_t q0, int64_t q1) {
    hipLaunchKernelGGL(tfit_heads_k, dim3(blocks(q1 - q0, TT)), dim3(TT), 0, st, a, (const uint32_t*)ks, (const uint32_t*)es, q0, q1, hf);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }));
  FMX_TRY(exclusive_sum(S, hf, hs, M + 1));
  int64_t *nch = nullptr, *coff = nullptr;
  if (label) { FMX_TRY(S.get(&nch, (size_t)cells + 1)); FMX_TRY(S.get(&coff, (size_t)cells + 1)); }
  FMX_TRY(in_cuts(cells + 1, lim.launch_rows, [&](int64_t k0, int64_t k1) {
    hipLaunchKernelGGL(tfit_cells_k, dim3(blocks(k1 - k0, TT)), dim3(TT), 0, st, cells, k0, k1, (const int64_t*)off, (const uint64_t*)hs, tab, nch);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }));
  if (label) {
    uint32_t* hrow = nullptr;
    FMX_TRY(S.get(&hrow, (size_t)M));
    FMX_TRY(in_cuts(M, lim.chunk_entries, [&](int64_t q0, int64_t q1) {
      hipLaunchKernelGGL(tfit_rows_k, dim3(blocks(q1 - q0, TT)), dim3(TT), 0, st, a, (const uint32_t*)es, (const uint64_t*)hf, (const uint64_t*)hs, q0, q1, hrow);
      FMX_HIP(hipGetLastError());
      return FMX_OK;
    }));
    FMX_TRY(exclusive_sum(S, (const int64_t*)nch, coff, cells + 1));
    int64_t chunks = 0;
    FMX_HIP(hipMemcpyAsync(&chunks, coff + cells, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    double* psum = nullptr;
    FMX_TRY(S.get(&psum, (size_t)chunks));
    FMX_TRY(in_cuts(chunks, lim.launch_rows, [&](int64_t w0, int64_t w1) {
      hipLaunchKernelGGL(tfit_chunks_k, dim3(blocks((w1 - w0) * 64, TT)), dim3(TT), 0, st, cells, (const int64_t*)off, (const uint64_t*)hs, (const int64_t*)coff,
                         (const uint32_t*)hrow, (const float*)m->y, w0, w1, psum);
      FMX_HIP(hipGetLastError());
      return FMX_OK;
    }));
    FMX_TRY(in_cuts(cells, lim.launch_rows, [&](int64_t k0, int64_t k1) {
      hipLaunchKernelGGL(tfit_sums_k, dim3(blocks(k1 - k0, TT)), dim3(TT), 0, st, k0, k1, (const int64_t*)coff, (const double*)psum, tab);
      FMX_HIP(hipGetLastError());
      return FMX_OK;
    }));
  }
  FMX_TRY(totals_run(t, lim, st));
  FMX_HIP(hipStreamSynchronize(st));
  return FMX_OK;
}

int stats_entry(const fmx_matrix* m, const uint32_t* host_part, const void* dev_part, const fmx_target_spec* sp, fmx_target_table** out) {
  std::vector<uint32_t> term_base;
  FMX_TRY(stats_check(m, sp, out, &term_base));
  FMX_TRY(use_device(m->device));
  DevBuf dp;
  if (host_part) { FMX_TRY(upload(&dp, host_part, m->n)); dev_part = dp.get(); }
  TableHold hold(nullptr, free_table);
  FMX_TRY(table_alloc(m->device, sp, term_base, &hold));
  FMX_TRY(stats_run(m, (const uint32_t*)dev_part, hold.get()));
  *out = hold.release();
  return FMX_OK;
}

// every refusal of the apply; host only.  eb: enc_base as it will be handed back
int enc_check(const fmx_matrix* m, const fmx_target_table* t, const fmx_encode_spec* sp, const uint32_t* enc_base, fmx_matrix** out, std::vector<uint32_t>* eb) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(sp != nullptr, FMX_ERR_INVALID, "spec is NULL");
  FMX_CHECK(enc_base != nullptr, FMX_ERR_INVALID, "enc_base is NULL");
  FMX_CHECK(sp->struct_size == sizeof(fmx_encode_spec), FMX_ERR_INVALID, "spec.struct_size does not match this library");
  FMX_CHECK(sp->reserved == 0, FMX_ERR_INVALID, "spec.reserved must be 0");
  FMX_CHECK(sp->keep_source == 0 || sp->keep_source == 1, FMX_ERR_INVALID, "keep_source must be 0 or 1 (got %d)", (int)sp->keep_source);
  FMX_CHECK(sp->kinds != nullptr, FMX_ERR_INVALID, "spec.kinds is NULL");
  FMX_CHECK(std::isfinite(sp->strength) && sp->strength >= 0.0, FMX_ERR_INVALID, "strength must be finite and not negative");
  FMX_CHECK(std::isfinite(sp->prior), FMX_ERR_INVALID, "prior must be finite");
  FMX_CHECK(t != nullptr, FMX_ERR_INVALID, "the table is NULL");
  const size_t n_terms = t->term_segment.size();
  uint64_t sum = sp->keep_source ? (uint64_t)t->p : 0ull;
  eb->assign(n_terms + 1, 0u);
  (*eb)[0] = (uint32_t)sum;
  for (size_t k = 0; k < n_terms; ++k) {
    const uint32_t kind = sp->kinds[k];
    FMX_CHECK(kind != 0 && (kind & ~(FMX_ENCODE_MEAN | FMX_ENCODE_COUNT)) == 0, FMX_ERR_INVALID, "kinds[%zu] = %u: FMX_ENCODE_MEAN, FMX_ENCODE_COUNT or both", k, kind);
    sum += (uint64_t)__builtin_popcount(kind);
    FMX_CHECK(sum <= TG_MAX_WIDTH, FMX_ERR_INVALID, "the widths sum to %llu: above 2^32 - 2", (unsigned long long)sum);
    (*eb)[k + 1] = (uint32_t)sum;
  }
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(m->p == t->p, FMX_ERR_INVALID, "the matrix has %u features, the table was made for %u", m->p, t->p);
  FMX_CHECK(m->device == t->device, FMX_ERR_INVALID, "the matrix is on device %d, the table on device %d", m->device, t->device);
  FMX_CHECK(m->n <= TG_MAX_ITEMS && m->nnz <= TG_MAX_ITEMS, FMX_ERR_INVALID, "at most 2^31 - 1 rows and stored entries per call");
  return FMX_OK;
}

// The single form applies where the source's layout (fixed row length L, dense prefix D, field bases) gives every encoded segment to exactly one position
// of the row (single_positions, fm_cross.hip): the segment IS the range of position j.  pos: per term its position
bool single_positions(const fmx_matrix* m, const fmx_target_table* t, uint32_t* pos) {
  const int L = m->fixed_row_len, D = m->dense_prefix;
  if (L <= 0 || m->n <= 0 || m->field_base.empty() || D < 0 || (int)m->field_base.size() != L - D + 1) return false;
  std::vector<uint64_t> lo((size_t)L + 1);
  for (int j = 0; j < L; ++j) lo[(size_t)j] = j < D ? (uint64_t)j : (uint64_t)m->field_base[(size_t)(j - D)];
  if (D < L) lo[(size_t)D] = (uint64_t)D;   // the first field's range opens at the dense prefix
  lo[(size_t)L] = m->p;
  for (int j = 0; j < L; ++j)
    if (lo[(size_t)j] >= lo[(size_t)j + 1]) return false;
  for (size_t k = 0; k < t->term_segment.size(); ++k) {
    const uint64_t a = t->segment_base[t->term_segment[k]], b = t->segment_base[t->term_segment[k] + 1];
    const auto it = std::lower_bound(lo.begin(), lo.end() - 1, a);
    if (it == lo.end() - 1 || *it != a || *(it + 1) != b) return false;
    pos[k] = (uint32_t)(it - lo.begin());
  }
  return true;
}

int enc_run(const fmx_matrix* m, const fmx_target_table* t, const uint32_t* d_part, const fmx_encode_spec* sp, const std::vector<uint32_t>& eb, fmx_matrix** out) {
  const TgLimits lim = tg_limits();
  const int n_terms = (int)t->term_segment.size(), keep = sp->keep_source ? 1 : 0;
  const int64_t n = m->n;
  const uint32_t out_p = eb[(size_t)n_terms];
  TermTab tt;
  terms_of(t, &tt);
  uint64_t mean_mask = 0, count_mask = 0;
  int NE = 0;
  for (int k = 0; k < n_terms; ++k) {
    tt.ob[k] = eb[(size_t)k];
    tt.kind[k] = sp->kinds[k];
    if (sp->kinds[k] & FMX_ENCODE_MEAN) mean_mask |= 1ull << k;
    if (sp->kinds[k] & FMX_ENCODE_COUNT) count_mask |= 1ull << k;
    for (int j = 0; j < __builtin_popcount(sp->kinds[k]); ++j) tt.om[NE++] = (uint32_t)k | ((uint32_t)j << 8);
  }
  const bool single = lim.single && single_positions(m, t, tt.pos);
  Scratch S;
  const hipStream_t st = S.st;
  TermTab* dtt = nullptr;
  FMX_TRY(S.get(&dtt, 1));
  FMX_HIP(hipMemcpyAsync(dtt, &tt, sizeof(tt), hipMemcpyHostToDevice, st));
  const float prior_f = (float)sp->prior;
  uint32_t prior_bits;
  std::memcpy(&prior_bits, &prior_f, sizeof(prior_bits));
  const EncArgs a{m->row_ptr, m->col, m->unit_values ? nullptr : reinterpret_cast<const uint32_t*>(m->val), d_part, dtt, t->cnt, t->sum, t->RC, t->RS, t->n_parts,
                  n_terms, keep, sp->prior * sp->strength, sp->strength, prior_bits, mean_mask, count_mask};
  fmx_matrix* o = nullptr;
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> hold(nullptr, free_matrix);
  if (single) {
    const int L = m->fixed_row_len;
    const int64_t Lo = (int64_t)keep * L + NE, total = n * Lo;
    FMX_CHECK(total <= TG_MAX_ITEMS, FMX_ERR_INVALID, "the output would hold %lld entries: at most 2^31 - 1", (long long)total);
    FMX_TRY(alloc_matrix(m->device, n, out_p, total, m->has_labels != 0, &o));
    hold.reset(o);
    hipLaunchKernelGGL(enc_ptrs_k, dim3(blocks(n + 1, TT)), dim3(TT), 0, st, n, Lo, o->row_ptr);
    FMX_HIP(hipGetLastError());
    for (int64_t t0 = 0; t0 < n; t0 += lim.launch_rows) {
      const int64_t t1 = std::min(n, t0 + lim.launch_rows);
      const int64_t pieces = ((t1 * Lo + 3) >> 2) - ((t0 * Lo) >> 2);
      hipLaunchKernelGGL(enc_single_k, dim3(blocks(pieces, TT)), dim3(TT), 0, st, a, L, NE, t0, t1, o->col, reinterpret_cast<uint32_t*>(o->val));
      FMX_HIP(hipGetLastError());
    }
  } else {
    // a lane group covers the longest row of the group form; the length pass and the long form walk longer rows in chunks
    const int reach = lim.group_max > 0 ? (int)std::min<int64_t>(lim.group_max, std::max(1, m->max_row_len)) : TG_GROUP_MAX;
    const int G = reach <= 16 ? 16 : reach <= 32 ? 32 : 64;
    int64_t *len = nullptr, *off = nullptr;   // off[n]: the total
    FMX_TRY(S.get(&len, (size_t)n + 1)); FMX_TRY(S.get(&off, (size_t)n + 1));
    FMX_HIP(hipMemsetAsync(len + n, 0, sizeof(int64_t), st));
    for (int64_t r0 = 0; r0 < n; r0 += lim.launch_rows) {
      const int64_t r1 = std::min(n, r0 + lim.launch_rows);
      hipLaunchKernelGGL(enc_len_k, dim3(blocks((r1 - r0) * G, TT)), dim3(TT), 0, st, a, r0, r1, G, len);
      FMX_HIP(hipGetLastError());
    }
    FMX_TRY(exclusive_sum(S, (const int64_t*)len, off, n + 1));
    int64_t total = 0;
    FMX_HIP(hipMemcpyAsync(&total, off + n, sizeof(total), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    FMX_CHECK(total <= TG_MAX_ITEMS, FMX_ERR_INVALID, "the output would hold %lld entries: at most 2^31 - 1", (long long)total);
    FMX_TRY(alloc_matrix(m->device, n, out_p, total, m->has_labels != 0, &o));
    hold.reset(o);
    FMX_HIP(hipMemcpyAsync(o->row_ptr, off, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    uint32_t *ocol = o->col, *oval = reinterpret_cast<uint32_t*>(o->val);
    const int64_t gmax = lim.group_max > 0 ? lim.group_max : 0;   // rows of at most gmax entries: the group form
    const bool any_long = m->max_row_len > gmax;
    for (int64_t r0 = 0; r0 < n && total > 0; r0 += lim.launch_rows) {
      const int64_t r1 = std::min(n, r0 + lim.launch_rows);
      if (gmax > 0) {
        hipLaunchKernelGGL(enc_rows_k, dim3(blocks((r1 - r0) * G, TT)), dim3(TT), 0, st, a, (const int64_t*)off, r0, r1, G, (int64_t)0, gmax, ocol, oval);
        FMX_HIP(hipGetLastError());
      }
      if (any_long) {
        hipLaunchKernelGGL(enc_rows_k, dim3(blocks((r1 - r0) * 64, TT)), dim3(TT), 0, st, a, (const int64_t*)off, r0, r1, 64, gmax, (int64_t)TG_MAX_ITEMS, ocol, oval);
        FMX_HIP(hipGetLastError());
      }
    }
  }
  if (m->has_labels && n > 0) FMX_HIP(hipMemcpyAsync(o->y, m->y, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
  FMX_HIP(hipStreamSynchronize(st));   // (the host table is read by the copy above)
  FMX_TRY(check_rows_sorted(o));
  *out = hold.release();
  return FMX_OK;
}

int enc_entry_point(const fmx_matrix* m, const fmx_target_table* t, const uint32_t* host_part, const void* dev_part, const fmx_encode_spec* sp, uint32_t* enc_base,
                    fmx_matrix** out) {
  std::vector<uint32_t> eb;
  FMX_TRY(enc_check(m, t, sp, enc_base, out, &eb));
  FMX_TRY(use_device(m->device));
  DevBuf dp;
  if (host_part) { FMX_TRY(upload(&dp, host_part, m->n)); dev_part = dp.get(); }
  FMX_TRY(enc_run(m, t, (const uint32_t*)dev_part, sp, eb, out));
  std::memcpy(enc_base, eb.data(), eb.size() * sizeof(uint32_t));
  return FMX_OK;
}

}  // namespace
}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_debug_target_limits(int32_t single, int32_t group_entries, int64_t chunk_entries, int64_t rows_per_launch) {
  g_single.store(single);
  g_group.store(group_entries);
  g_chunk.store(chunk_entries > 0 ? chunk_entries : 0);
  g_rows.store(rows_per_launch > 0 ? rows_per_launch : 0);
  return FMX_OK;
}

int fmx_target_stats(const fmx_matrix* m, const uint32_t* part, const fmx_target_spec* spec, fmx_target_table** out) {
  return stats_entry(m, part, nullptr, spec, out);
}

int fmx_target_stats_device(const fmx_matrix* m, const void* dev_part_u32, const fmx_target_spec* spec, fmx_target_table** out) {
  return stats_entry(m, nullptr, dev_part_u32, spec, out);
}

int fmx_target_table_from_arrays(int device, const fmx_target_spec* layout, const int64_t* count, const double* sum, fmx_target_table** out) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  std::vector<uint32_t> term_base;
  FMX_TRY(layout_check(layout, &term_base));
  const int64_t cells = (int64_t)term_base.back() * layout->n_parts;
  FMX_CHECK(count != nullptr || cells == 0, FMX_ERR_INVALID, "count is NULL");
  const bool label = layout->target == FMX_TARGET_LABEL;
  FMX_CHECK(!label || sum != nullptr || cells == 0, FMX_ERR_INVALID, "sum is NULL: a FMX_TARGET_LABEL table needs the sums");
  FMX_TRY(use_device(device));
  TableHold hold(nullptr, free_table);
  FMX_TRY(table_alloc(device, layout, term_base, &hold));
  const TgLimits lim = tg_limits();
  DevBuf dc, ds;
  FMX_TRY(upload(&dc, count, cells * 2));
  if (label) FMX_TRY(upload(&ds, sum, cells));
  FMX_TRY(in_cuts(cells, lim.launch_rows, [&](int64_t a, int64_t b) {
    hipLaunchKernelGGL(tt_pack_k, dim3(blocks(b - a, TT)), dim3(TT), 0, nullptr, a, b, tab_of(hold.get()), (const int64_t*)dc.get(), label ? (const double*)ds.get() : nullptr);
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }));
  FMX_TRY(totals_run(hold.get(), lim, nullptr));
  FMX_HIP(hipStreamSynchronize(nullptr));
  *out = hold.release();
  return FMX_OK;
}

int fmx_target_table_info(const fmx_target_table* t, int64_t* info) {
  FMX_CHECK(t != nullptr && info != nullptr, FMX_ERR_INVALID, "NULL argument");
  info[0] = t->device; info[1] = t->p; info[2] = (int64_t)t->segment_base.size() - 1; info[3] = (int64_t)t->term_segment.size();
  info[4] = t->n_parts; info[5] = t->target; info[6] = t->W;
  info[7] = std::max<int64_t>(t->W, 1) * ((int64_t)t->RC * (int64_t)sizeof(int64_t) + (int64_t)t->RS * (int64_t)sizeof(double));
  return FMX_OK;
}

int fmx_target_table_export(const fmx_target_table* t, uint32_t* segment_base, uint32_t* term_segment, int64_t* count, double* sum) {
  FMX_CHECK(t != nullptr, FMX_ERR_INVALID, "the table is NULL");
  if (segment_base) std::memcpy(segment_base, t->segment_base.data(), t->segment_base.size() * sizeof(uint32_t));
  if (term_segment) std::memcpy(term_segment, t->term_segment.data(), t->term_segment.size() * sizeof(uint32_t));
  const int64_t cells = t->W * t->n_parts;
  if (t->target != FMX_TARGET_LABEL) sum = nullptr;
  if ((!count && !sum) || cells == 0) return FMX_OK;
  FMX_TRY(use_device(t->device));
  const TgLimits lim = tg_limits();
  DevBuf dc, ds;
  if (count) FMX_TRY(dev_buf(&dc, (size_t)cells * 2 * sizeof(int64_t)));
  if (sum) FMX_TRY(dev_buf(&ds, (size_t)cells * sizeof(double)));
  FMX_TRY(in_cuts(cells, lim.launch_rows, [&](int64_t a, int64_t b) {
    hipLaunchKernelGGL(tt_unpack_k, dim3(blocks(b - a, TT)), dim3(TT), 0, nullptr, a, b, tab_of(t), (int64_t*)dc.get(), (double*)ds.get());
    FMX_HIP(hipGetLastError());
    return FMX_OK;
  }));
  if (count) FMX_HIP(hipMemcpy(count, dc.get(), (size_t)cells * 2 * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (sum) FMX_HIP(hipMemcpy(sum, ds.get(), (size_t)cells * sizeof(double), hipMemcpyDeviceToHost));
  return FMX_OK;
}

int fmx_target_table_free(fmx_target_table* t) {
  if (!t) return FMX_OK;
  FMX_TRY(use_device(t->device));
  free_table(t);
  return FMX_OK;
}

int fmx_matrix_encode_targets(const fmx_matrix* m, const fmx_target_table* table, const uint32_t* part, const fmx_encode_spec* spec, uint32_t* enc_base, fmx_matrix** out) {
  return enc_entry_point(m, table, part, nullptr, spec, enc_base, out);
}

int fmx_matrix_encode_targets_device(const fmx_matrix* m, const fmx_target_table* table, const void* dev_part_u32, const fmx_encode_spec* spec, uint32_t* enc_base,
                                     fmx_matrix** out) {
  return enc_entry_point(m, table, nullptr, dev_part_u32, spec, enc_base, out);
}

}  // extern "C"
