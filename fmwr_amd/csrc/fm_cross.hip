// Feature crosses on the device: fmx_matrix_cross.  The column space is cut into segments; a term (a, b) gives every pair of a
// row's entries of segment a and of segment b an id of its own -- exact, u * width(b) + v, or hashed into n_buckets -- and the product of the two
// values, rounded once.  Ids are integer work and the product is the IEEE binary32 product, so tests/cross_model.py restates every output bit for bit.
//
//   tables   one device block u32[n_segments + 1 | 8 n_terms]: the segment bases and a record per term (CrossTermD).  Every kernel stages what it
//            needs of it in LDS once per workgroup.
//   seg_of   the segment of a column id: the last s with base[s] <= c, by a branch-free binary search over the staged bases.  The length pass and
//            every fill form call this one function.
//   value    (float)((double)x * (double)y): the product of two binary32 values is exact in binary64, so the one conversion is the one rounding,
//            subnormals kept whatever the file's fp32 flags say; a NaN result becomes 0x7FC00000.
//   length   a lane group per row (cross_len_k): per term the counts of E_a and E_b by ballots over the row's chunks, the row's entries saturating at
//            2^31 (the lowest such row goes to a flag by atomicMin); fm_prims' 64-bit scan; total and flag come back in ONE read.
//   fill     three forms that write the same bits:
//              single  a source of fixed row length whose layout puts exactly one entry of every named segment at a fixed position, no self-cross:
//                      every term is one entry per row, the row pointers are arithmetic, there is no length pass; the term table holds positions;
//                      a lane writes 16 bytes of ids and 16 of values (cross_single_k)
//              group   rows of at most group_entries (<= 64) entries: a lane per entry, the positions of E_a and E_b are the set bits of two ballots,
//                      lanes enumerate the pair index q -> (i, j) with group-uniform divisors and fetch the two entries over shuffles (cross_group_k)
//              long    longer rows: a workgroup per row; E_a and E_b go through LDS in tiles of CROSS_TILE entries made by a block scan that resumes
//                      where the last tile ended, and a pair's output position is computed from its two ranks (cross_long_k)
// No floating-point atomic, no scratch; the only atomics are the integer atomicMin of the refusal.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <vector>

#include "fm_prims.h"
#include "fmx_test_hooks.h"

namespace fmx {
namespace {

constexpr int XT = 256;
constexpr int CROSS_MAX_SEGMENTS = 4096;
constexpr int CROSS_MAX_TERMS = 64;
constexpr int CROSS_GROUP_MAX = 64;                // longest row of the group form: a lane per entry
constexpr int CROSS_TILE = 1024;                   // entries of one LDS tile of the long form (4 tiles of 4 KiB)
constexpr int64_t CROSS_LAUNCH_ROWS = 1LL << 22;
constexpr int64_t CROSS_MAX_ITEMS = 0x7FFFFFFFLL;  // entries of one output row, and of the output
constexpr uint64_t CROSS_MAX_WIDTH = 0xFFFFFFFEull;
constexpr uint32_t CROSS_ONE = 0x3F800000u;        // 1.0f
constexpr uint32_t CROSS_NAN = 0x7FC00000u;
constexpr uint32_t CROSS_NO_SEG = 0xFFFFFFFFu;
constexpr uint32_t CROSS_STREAM0 = 128;            // pair_hash's stream of term t is 128 + t
constexpr int CROSS_TERM_WORDS = 8;

std::atomic<int> g_single{0}, g_group{0};
std::atomic<int64_t> g_rows{0};

struct CrossLimits {
  bool single;          // the single form may be taken
  int group_max;        // rows of at most this many entries take the group form (< 0: none does)
  int64_t launch_rows;
};
CrossLimits cross_limits() {
  CrossLimits l{g_single.load() >= 0, g_group.load(), g_rows.load()};
  if (l.group_max == 0 || l.group_max > CROSS_GROUP_MAX) l.group_max = CROSS_GROUP_MAX;
  if (l.group_max < 0) l.group_max = -1;
  if (l.launch_rows <= 0) l.launch_rows = CROSS_LAUNCH_ROWS;
  return l;
}

// a term as the kernels read it.  a, b: the two segments -- in the single form the two POSITIONS inside a source row (never equal there)
struct CrossTermD {
  uint32_t a, b;
  uint32_t base_a, base_b;   // the first column of either segment
  uint32_t width_b;
  uint32_t n_buckets;        // 0: exact
  uint32_t out_base;         // cross_base[t]
  uint32_t stream;
};
static_assert(sizeof(CrossTermD) == CROSS_TERM_WORDS * sizeof(uint32_t), "a term record is eight words");

struct CrossArgs {
  const int64_t* rp;
  const uint32_t* col;
  const uint32_t* val;   // null: every value is 1.0f
  const uint32_t* tab;   // seg u32[n_seg + 1] | CrossTermD[n_terms]
  int n_seg, n_terms, keep;
  uint64_t seed, salt;
};

// lds: (with_seg: the bases, then) the term records; ends in a barrier
__device__ __forceinline__ void cross_stage(const CrossArgs& a, uint32_t* lds, bool with_seg) {
  const int skip = a.n_seg + 1;
  const int words = (with_seg ? skip : 0) + CROSS_TERM_WORDS * a.n_terms;
  const uint32_t* src = with_seg ? a.tab : a.tab + skip;
  for (int i = threadIdx.x; i < words; i += XT) lds[i] = src[i];
  __syncthreads();
}

// the last s in [0, n_seg) with S[s] <= c (S[0] = 0 and c < S[n_seg]; an empty segment shares its base with the one after it and is never the answer)
__device__ __forceinline__ uint32_t seg_of(const uint32_t* S, int n_seg, uint32_t c) {
  uint32_t lo = 0, len = (uint32_t)n_seg;   // lo ends as #{s < n_seg : S[s] <= c}
  while (len > 0) {
    const uint32_t half = len >> 1;
    const bool le = S[lo + half] <= c;
    lo = le ? lo + half + 1 : lo;
    len = le ? len - half - 1 : half;
  }
  return lo - 1;
}

__device__ __forceinline__ uint32_t cross_value(uint32_t xa, uint32_t xb) {
  const float f = (float)((double)__uint_as_float(xa) * (double)__uint_as_float(xb));
  return f != f ? CROSS_NAN : __float_as_uint(f);
}

__device__ __forceinline__ uint32_t cross_id(const CrossTermD& t, uint32_t ca, uint32_t cb, uint64_t seed, uint64_t salt) {
  uint32_t u = ca - t.base_a, v = cb - t.base_b;
  if (t.a == t.b && u > v) { const uint32_t w = u; u = v; v = w; }
  if (t.n_buckets) return t.out_base + (uint32_t)__umul64hi(pair_hash(seed, salt, ((uint64_t)u << 32) | (uint64_t)v, (uint64_t)t.stream), (uint64_t)t.n_buckets);
  return t.out_base + u * t.width_b + v;
}

// the position of the k-th (from 0) set bit of m; k < popcount(m)
__device__ __forceinline__ int nth_bit(uint64_t m, int k) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const int c = __popcll(m & ((1ull << w) - 1ull));
    const bool up = k >= c;
    k = up ? k - c : k;
    m = up ? m >> w : m;
    pos = up ? pos + w : pos;
  }
  return pos;
}

// ---------------------------------------------------------------------------------------------------------------------------- length

// rows [r0, r1), G lanes each: len[r] = the entries of output row r, 0 for a row of more than 2^31 - 1 (whose index goes to *flag by atomicMin)
__global__ __launch_bounds__(XT) void cross_len_k(const CrossArgs a, int64_t r0, int64_t r1, int G, int64_t* __restrict__ len, unsigned long long* __restrict__ flag) {
  extern __shared__ uint32_t lds[];
  cross_stage(a, lds, true);
  const uint32_t* S = lds;
  const CrossTermD* T = reinterpret_cast<const CrossTermD*>(lds + a.n_seg + 1);
  const int64_t r = r0 + ((int64_t)blockIdx.x * XT + threadIdx.x) / G;
  const int lane = threadIdx.x & (G - 1);
  const int gsh = (threadIdx.x & 63) & ~(G - 1);
  const uint64_t gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
  const bool live = r < r1;
  const int64_t s0 = live ? a.rp[r] : 0;
  const int64_t n = live ? a.rp[r + 1] - s0 : 0;
  uint32_t sg0 = CROSS_NO_SEG;   // the segment of the first chunk's entry: a short row is searched once
  if (lane < n) sg0 = seg_of(S, a.n_seg, a.col[s0 + lane]);
  uint64_t l = a.keep ? (uint64_t)n : 0ull;
  for (int t = 0; t < a.n_terms; ++t) {   // (uniform)
    const uint32_t sa = T[t].a, sb = T[t].b;
    uint64_t na = 0, nb = 0;
    for (int64_t x0 = 0; x0 < n; x0 += G) {   // (uniform over the lane group: a ballot's bits of other groups are masked out)
      const int64_t x = x0 + lane;
      uint32_t sg = sg0;
      if (x0 > 0) sg = x < n ? seg_of(S, a.n_seg, a.col[s0 + x]) : CROSS_NO_SEG;
      na += (uint64_t)__popcll((__ballot(sg == sa) >> gsh) & gmask);
      nb += (uint64_t)__popcll((__ballot(sg == sb) >> gsh) & gmask);
    }
    l += sa == sb ? (na * (na - 1ull)) >> 1 : na * nb;   // (na, nb < 2^31: no overflow; na = 0 gives 0)
    if (l > (uint64_t)CROSS_MAX_ITEMS) l = (uint64_t)CROSS_MAX_ITEMS + 1ull;
  }
  if (live && lane == 0) {
    const bool bad = l > (uint64_t)CROSS_MAX_ITEMS;
    if (bad) atomicMin(flag, (unsigned long long)r);
    len[r] = bad ? 0 : (int64_t)l;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------ fill

// out_rp[t] = t * Lo for t = 0 .. n
__global__ __launch_bounds__(XT) void cross_ptrs_k(int64_t n, int64_t Lo, int64_t* __restrict__ out_rp) {
  const int64_t t = (int64_t)blockIdx.x * XT + threadIdx.x;
  if (t <= n) out_rp[t] = t * Lo;
}

// single form: output rows [t0, t1) of Lo = keep L + n_terms entries.  Thread q owns the 16-byte piece [4 Q, 4 Q + 4) of the output stream, Q = (t0 Lo) / 4 + q,
// clipped to the launch's entries: a piece that straddles two launches is shared between them entry by entry (as gather_fixed_k, fm_join.hip)
__global__ __launch_bounds__(XT) void cross_single_k(const CrossArgs a, int L, int64_t t0, int64_t t1, uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval) {
  extern __shared__ uint32_t lds[];
  cross_stage(a, lds, false);
  const CrossTermD* T = reinterpret_cast<const CrossTermD*>(lds);
  const int kL = a.keep ? L : 0;
  const int Lo = kL + a.n_terms;
  const int64_t e0 = t0 * Lo, e1 = t1 * Lo;
  const int64_t o = ((e0 >> 2) + (int64_t)blockIdx.x * XT + threadIdx.x) << 2;
  if (o >= e1) return;
  int64_t t = o / Lo;
  int j = (int)(o - t * Lo);
  uint32_t c[4] = {0, 0, 0, 0}, v[4] = {CROSS_ONE, CROSS_ONE, CROSS_ONE, CROSS_ONE};
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int64_t e = o + x;
    if (e >= e0 && e < e1) {
      const int64_t s0 = t * L;
      if (j < kL) {
        c[x] = a.col[s0 + j];
        if (a.val) v[x] = a.val[s0 + j];
      } else {
        const CrossTermD tm = T[j - kL];
        c[x] = cross_id(tm, a.col[s0 + tm.a], a.col[s0 + tm.b], a.seed, a.salt);
        if (a.val) v[x] = cross_value(a.val[s0 + tm.a], a.val[s0 + tm.b]);
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

// group form: rows [r0, r1) of at most group_max (<= G <= 64) entries, a lane per entry; longer rows are left to the long form
__global__ __launch_bounds__(XT) void cross_group_k(const CrossArgs a, const int64_t* __restrict__ off, int64_t r0, int64_t r1, int G, int group_max,
                                                   uint32_t* __restrict__ ocol, uint32_t* __restrict__ oval) {
  extern __shared__ uint32_t lds[];
  cross_stage(a, lds, true);
  const uint32_t* S = lds;
  const CrossTermD* T = reinterpret_cast<const CrossTermD*>(lds + a.n_seg + 1);
  const int64_t r = r0 + ((int64_t)blockIdx.x * XT + threadIdx.x) / G;
  const int lane = threadIdx.x & (G - 1);
  const int gsh = (threadIdx.x & 63) & ~(G - 1);
  const uint64_t gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
  const bool live = r < r1;
  const int64_t s0 = live ? a.rp[r] : 0;
  int64_t n = live ? a.rp[r + 1] - s0 : 0;
  if (n > group_max) n = 0;
  uint32_t c = 0, x = CROSS_ONE, sg = CROSS_NO_SEG;
  if (lane < n) {
    c = a.col[s0 + lane];
    if (a.val) x = a.val[s0 + lane];
    sg = seg_of(S, a.n_seg, c);
  }
  int64_t d = n > 0 ? off[r] : 0;
  if (a.keep) {
    if (lane < n) { ocol[d + lane] = c; oval[d + lane] = x; }
    d += n;
  }
  for (int t = 0; t < a.n_terms; ++t) {   // (uniform: every lane of the wave takes part in the ballots)
    const CrossTermD tm = T[t];
    const bool self = tm.a == tm.b;
    const uint64_t mA = (__ballot(sg == tm.a) >> gsh) & gmask;
    const uint64_t mB = self ? mA : (__ballot(sg == tm.b) >> gsh) & gmask;
    const int na = __popcll(mA), nb = __popcll(mB);
    const int cnt = self ? (na * (na - 1)) >> 1 : na * nb;
    for (int q0 = 0; q0 < cnt; q0 += G) {   // (uniform over the lane group: the shuffles below read lanes of the group itself)
      const int q = q0 + lane;
      const bool mine = q < cnt;
      const int qq = mine ? q : 0;
      int i, j;
      if (self) {   // pairs i < j of E_a, i-major: row i of the triangle holds na - 1 - i of them
        int rem = qq;
        i = 0;
        while (rem >= na - 1 - i) { rem -= na - 1 - i; ++i; }
        j = i + 1 + rem;
      } else {
        i = qq / nb;
        j = qq - i * nb;
      }
      const int la = gsh + nth_bit(mA, i), lb = gsh + nth_bit(mB, j);
      const uint32_t ca = __shfl(c, la, 64), cb = __shfl(c, lb, 64);
      const uint32_t xa = __shfl(x, la, 64), xb = __shfl(x, lb, 64);
      if (mine) {
        ocol[d + q] = cross_id(tm, ca, cb, a.seed, a.salt);
        oval[d + q] = a.val ? cross_value(xa, xb) : CROSS_ONE;
      }
    }
    d += cnt;
  }
}

// long form, one workgroup per row.  lds behind the tables: four tiles u32[CROSS_TILE] (A's columns, A's values, B's columns, B's values), wsum[4], next[1]
struct CrossRow {
  const uint32_t* S;
  int n_seg;
  const uint32_t* col;
  const uint32_t* val;
  int64_t s0, n;
  int* wsum;     // [16]: four wave sums, [4] the cursor behind a tile's last entry, [5..8] the second count's wave sums
};

// how many entries of the row lie in segments sa and sb (block-wide; the answer in every thread)
__device__ __forceinline__ void long_count(const CrossRow& w, uint32_t sa, uint32_t sb, int* na, int* nb) {
  int ca = 0, cb = 0;
  for (int64_t x = threadIdx.x; x < w.n; x += XT) {
    const uint32_t sg = seg_of(w.S, w.n_seg, w.col[w.s0 + x]);
    ca += sg == sa ? 1 : 0;
    cb += sg == sb ? 1 : 0;
  }
  for (int s = 32; s >= 1; s >>= 1) { ca += __shfl_xor(ca, s); cb += __shfl_xor(cb, s); }
  int* both = w.wsum;
  if ((threadIdx.x & 63) == 0) { both[threadIdx.x >> 6] = ca; both[5 + (threadIdx.x >> 6)] = cb; }
  __syncthreads();
  *na = both[0] + both[1] + both[2] + both[3];
  *nb = both[5] + both[6] + both[7] + both[8];
  __syncthreads();
}

// the next `want` entries of segment sg from row position cur on into (tc, tv); returns the position behind the last one taken (block-wide; the row
// holds at least `want` more such entries)
__device__ __forceinline__ int64_t long_fill(const CrossRow& w, uint32_t sg, int64_t cur, int want, uint32_t* tc, uint32_t* tv) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int got = 0;
  while (got < want && cur < w.n) {   // (uniform: got and cur are the same in every thread)
    const int64_t x = cur + threadIdx.x;
    uint32_t c = 0;
    bool flag = false;
    if (x < w.n) {
      c = w.col[w.s0 + x];
      flag = seg_of(w.S, w.n_seg, c) == sg;
    }
    const uint64_t ballot = __ballot(flag);
    if (lane == 0) w.wsum[wave] = __popcll(ballot);
    __syncthreads();
    int slot = got + __popcll(ballot & ((1ull << lane) - 1ull)), all = 0;
#pragma unroll
    for (int k = 0; k < XT / 64; ++k) {
      if (k < wave) slot += w.wsum[k];
      all += w.wsum[k];
    }
    if (flag && slot < want) {
      tc[slot] = c;
      tv[slot] = w.val ? w.val[w.s0 + x] : CROSS_ONE;
      if (slot == want - 1) w.wsum[4] = (int)(x - cur) + 1;
    }
    __syncthreads();
    if (got + all >= want) { cur += w.wsum[4]; got = want; }
    else { cur += XT; got += all; }
  }
  __syncthreads();   // the tile is written (and wsum[4] read) before anyone goes on
  return cur;
}

__global__ __launch_bounds__(XT) void cross_long_k(const CrossArgs a, const int64_t* __restrict__ off, int64_t r0, int group_max, uint32_t* __restrict__ ocol,
                                                  uint32_t* __restrict__ oval) {
  extern __shared__ uint32_t lds[];
  const int64_t r = r0 + blockIdx.x;
  const int64_t s0 = a.rp[r], n = a.rp[r + 1] - s0;
  if (n <= group_max) return;   // (the whole workgroup: the group form's row)
  cross_stage(a, lds, true);
  const CrossTermD* T = reinterpret_cast<const CrossTermD*>(lds + a.n_seg + 1);
  uint32_t* tiles = lds + a.n_seg + 1 + CROSS_TERM_WORDS * a.n_terms;
  uint32_t *Ac = tiles, *Av = tiles + CROSS_TILE, *Bc0 = tiles + 2 * CROSS_TILE, *Bv0 = tiles + 3 * CROSS_TILE;
  CrossRow w{lds, a.n_seg, a.col, a.val, s0, n, reinterpret_cast<int*>(tiles + 4 * CROSS_TILE)};
  int64_t d = off[r];
  if (a.keep) {
    for (int64_t x = threadIdx.x; x < n; x += XT) {
      ocol[d + x] = a.col[s0 + x];
      oval[d + x] = a.val ? a.val[s0 + x] : CROSS_ONE;
    }
    d += n;
  }
  for (int t = 0; t < a.n_terms; ++t) {
    const CrossTermD tm = T[t];
    const bool self = tm.a == tm.b;
    int na = 0, nb = 0;   // (a row's entries of one segment: below 2^31, the length pass has held the row's pairs to that)
    long_count(w, tm.a, tm.b, &na, &nb);
    const int64_t cnt = self ? ((int64_t)na * (na - 1)) >> 1 : (int64_t)na * nb;
    if (cnt == 0) continue;
    int64_t curA = 0;
    for (int ia0 = 0; ia0 < na; ia0 += CROSS_TILE) {
      const int ca = std::min(CROSS_TILE, na - ia0);
      curA = long_fill(w, tm.a, curA, ca, Ac, Av);
      int64_t curB = 0;
      for (int jb0 = self ? ia0 : 0; jb0 < nb; jb0 += CROSS_TILE) {   // (a self-cross starts at the diagonal tile: the tiles before it hold no i < j)
        const int cb = std::min(CROSS_TILE, nb - jb0);
        const uint32_t *Bc = Bc0, *Bv = Bv0;
        if (self && jb0 == ia0) { Bc = Ac; Bv = Av; curB = curA; }               // the diagonal tile is A's own
        else if (!(nb <= CROSS_TILE && ia0 > 0)) curB = long_fill(w, tm.b, curB, cb, Bc0, Bv0);   // (a single B tile is made once)
        for (int p = threadIdx.x; p < ca * cb; p += XT) {
          const int i = p / cb, j = p - i * cb;
          const int64_t ra = ia0 + i, rb = jb0 + j;
          if (self && ra >= rb) continue;
          const int64_t idx = self ? ((ra * (2 * (int64_t)na - ra - 1)) >> 1) + (rb - ra - 1) : ra * nb + rb;
          ocol[d + idx] = cross_id(tm, Ac[i], Bc[j], a.seed, a.salt);
          oval[d + idx] = a.val ? cross_value(Av[i], Bv[j]) : CROSS_ONE;
        }
        __syncthreads();   // the tiles are read before the next fill
      }
    }
    d += cnt;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------ host

// every refusal of fmx_matrix_cross; host only.  cb: cross_base as it will be handed back, n_terms + 1 values
int cross_check(const fmx_matrix* m, const fmx_cross_spec* sp, const uint32_t* cross_base, fmx_matrix** out, std::vector<uint32_t>* cb) {
  FMX_CHECK(out != nullptr, FMX_ERR_INVALID, "out is NULL");
  *out = nullptr;
  FMX_CHECK(sp != nullptr, FMX_ERR_INVALID, "spec is NULL");
  FMX_CHECK(cross_base != nullptr, FMX_ERR_INVALID, "cross_base is NULL");
  FMX_CHECK(sp->struct_size == sizeof(fmx_cross_spec), FMX_ERR_INVALID, "spec.struct_size does not match this library");
  FMX_CHECK(sp->reserved == 0, FMX_ERR_INVALID, "spec.reserved must be 0");
  FMX_CHECK(sp->n_segments >= 1 && sp->n_segments <= CROSS_MAX_SEGMENTS, FMX_ERR_INVALID, "n_segments must be in 1..%d (got %d)", CROSS_MAX_SEGMENTS, (int)sp->n_segments);
  FMX_CHECK(sp->n_terms >= 1 && sp->n_terms <= CROSS_MAX_TERMS, FMX_ERR_INVALID, "n_terms must be in 1..%d (got %d)", CROSS_MAX_TERMS, (int)sp->n_terms);
  FMX_CHECK(sp->keep_source == 0 || sp->keep_source == 1, FMX_ERR_INVALID, "keep_source must be 0 or 1 (got %d)", (int)sp->keep_source);
  FMX_CHECK(sp->segment_base != nullptr, FMX_ERR_INVALID, "spec.segment_base is NULL");
  FMX_CHECK(sp->terms != nullptr, FMX_ERR_INVALID, "spec.terms is NULL");
  const uint32_t* base = sp->segment_base;
  FMX_CHECK(base[0] == 0, FMX_ERR_INVALID, "spec.segment_base must start at 0");
  for (int32_t s = 0; s < sp->n_segments; ++s)
    FMX_CHECK(base[s] <= base[s + 1], FMX_ERR_INVALID, "spec.segment_base descends at segment %d", (int)s);
  uint64_t sum = 0;   // of the terms' widths; each term adds at most 2^64 - 1 and the sum is cut off as soon as it is too large
  std::vector<uint64_t> width((size_t)sp->n_terms);
  for (int32_t t = 0; t < sp->n_terms; ++t) {
    const fmx_cross_term& k = sp->terms[t];
    FMX_CHECK(k.reserved == 0, FMX_ERR_INVALID, "term %d: reserved must be 0", (int)t);
    FMX_CHECK(k.seg_a <= k.seg_b, FMX_ERR_INVALID, "term %d: seg_a = %u is above seg_b = %u", (int)t, k.seg_a, k.seg_b);
    FMX_CHECK(k.seg_b < (uint32_t)sp->n_segments, FMX_ERR_INVALID, "term %d names segment %u: there are %d segments", (int)t, k.seg_b, (int)sp->n_segments);
    width[(size_t)t] = k.n_buckets ? (uint64_t)k.n_buckets : (uint64_t)(base[k.seg_a + 1] - base[k.seg_a]) * (uint64_t)(base[k.seg_b + 1] - base[k.seg_b]);
    sum = (sum > CROSS_MAX_WIDTH || width[(size_t)t] > CROSS_MAX_WIDTH) ? CROSS_MAX_WIDTH + 1 : sum + width[(size_t)t];
  }
  FMX_CHECK(sum <= CROSS_MAX_WIDTH, FMX_ERR_INVALID, "the widths of the terms sum above 2^32 - 2");
  FMX_CHECK(m != nullptr, FMX_ERR_INVALID, "NULL matrix");
  FMX_CHECK(base[sp->n_segments] == m->p, FMX_ERR_INVALID, "spec.segment_base ends at %u, not at the feature count %u", base[sp->n_segments], m->p);
  sum += sp->keep_source ? (uint64_t)m->p : 0ull;
  FMX_CHECK(sum <= CROSS_MAX_WIDTH, FMX_ERR_INVALID, "the widths sum to %llu: above 2^32 - 2", (unsigned long long)sum);
  cb->assign((size_t)sp->n_terms + 1, 0u);
  (*cb)[0] = sp->keep_source ? m->p : 0u;
  for (int32_t t = 0; t < sp->n_terms; ++t) (*cb)[(size_t)t + 1] = (*cb)[(size_t)t] + (uint32_t)width[(size_t)t];
  return FMX_OK;
}

// The single form applies where the source's layout (fixed row length L, dense prefix D, field bases) gives every segment a term names to exactly one
// position of the row: the segment IS the range of position j -- [j, j + 1) for j < D, [field_base[j - D], field_base[j - D + 1]) behind it.  The
// positions' ranges tile [0, p), so a segment that equals one of them holds that position's entry of every row and no other.  pos: per term (pa, pb)
bool single_positions(const fmx_matrix* m, const fmx_cross_spec* sp, std::vector<uint32_t>* pos) {
  const int L = m->fixed_row_len, D = m->dense_prefix;
  if (L <= 0 || m->n <= 0 || m->field_base.empty() || D < 0 || (int)m->field_base.size() != L - D + 1) return false;
  std::vector<uint64_t> lo((size_t)L + 1);
  for (int j = 0; j < L; ++j) lo[(size_t)j] = j < D ? (uint64_t)j : (uint64_t)m->field_base[(size_t)(j - D)];
  if (D < L) lo[(size_t)D] = (uint64_t)D;   // the first field's range opens at the dense prefix
  lo[(size_t)L] = m->p;
  for (int j = 0; j < L; ++j)
    if (lo[(size_t)j] >= lo[(size_t)j + 1]) return false;
  pos->clear();
  for (int32_t t = 0; t < sp->n_terms; ++t) {
    const uint32_t seg[2] = {sp->terms[t].seg_a, sp->terms[t].seg_b};
    if (seg[0] == seg[1]) return false;   // a self-cross of a one-entry segment emits nothing: the rows are not n_terms longer
    for (int k = 0; k < 2; ++k) {
      const uint64_t a = sp->segment_base[seg[k]], b = sp->segment_base[seg[k] + 1];
      const auto it = std::lower_bound(lo.begin(), lo.end() - 1, a);
      if (it == lo.end() - 1 || *it != a || *(it + 1) != b) return false;
      pos->push_back((uint32_t)(it - lo.begin()));
    }
  }
  return true;
}

int cross_run(const fmx_matrix* m, const fmx_cross_spec* sp, const std::vector<uint32_t>& cb, fmx_matrix** out) {
  const CrossLimits lim = cross_limits();
  const int n_seg = sp->n_segments, n_terms = sp->n_terms, keep = sp->keep_source ? 1 : 0;
  const int64_t n = m->n;
  const uint32_t out_p = cb[(size_t)n_terms];
  std::vector<uint32_t> pos;
  const bool single = lim.single && single_positions(m, sp, &pos);
  std::vector<uint32_t> tab((size_t)n_seg + 1 + (size_t)CROSS_TERM_WORDS * (size_t)n_terms);
  std::memcpy(tab.data(), sp->segment_base, ((size_t)n_seg + 1) * sizeof(uint32_t));
  for (int t = 0; t < n_terms; ++t) {
    const fmx_cross_term& k = sp->terms[t];
    const uint32_t* base = sp->segment_base;
    CrossTermD d{k.seg_a, k.seg_b, base[k.seg_a], base[k.seg_b], base[k.seg_b + 1] - base[k.seg_b], k.n_buckets, cb[(size_t)t], CROSS_STREAM0 + (uint32_t)t};
    if (single) { d.a = pos[2 * (size_t)t]; d.b = pos[2 * (size_t)t + 1]; }
    std::memcpy(tab.data() + n_seg + 1 + (size_t)CROSS_TERM_WORDS * (size_t)t, &d, sizeof(d));
  }
  Scratch S;
  const hipStream_t st = S.st;
  uint32_t* dtab = nullptr;
  FMX_TRY(S.get(&dtab, tab.size()));
  FMX_HIP(hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  const CrossArgs a{m->row_ptr, m->col, m->unit_values ? nullptr : reinterpret_cast<const uint32_t*>(m->val), dtab, n_seg, n_terms, keep, sp->seed, sp->salt};
  const size_t lds_terms = (size_t)CROSS_TERM_WORDS * (size_t)n_terms * sizeof(uint32_t);
  const size_t lds_tab = ((size_t)n_seg + 1) * sizeof(uint32_t) + lds_terms;
  const size_t lds_long = lds_tab + (4 * (size_t)CROSS_TILE + 16) * sizeof(uint32_t);
  fmx_matrix* o = nullptr;
  std::unique_ptr<fmx_matrix, void (*)(fmx_matrix*)> hold(nullptr, free_matrix);
  if (single) {
    const int L = m->fixed_row_len;
    const int64_t Lo = (int64_t)keep * L + n_terms, total = n * Lo;
    FMX_CHECK(total <= CROSS_MAX_ITEMS, FMX_ERR_INVALID, "the output would hold %lld entries: at most 2^31 - 1", (long long)total);
    FMX_TRY(alloc_matrix(m->device, n, out_p, total, m->has_labels != 0, &o));
    hold.reset(o);
    hipLaunchKernelGGL(cross_ptrs_k, dim3(blocks(n + 1, XT)), dim3(XT), 0, st, n, Lo, o->row_ptr);
    FMX_HIP(hipGetLastError());
    for (int64_t t0 = 0; t0 < n; t0 += lim.launch_rows) {
      const int64_t t1 = std::min(n, t0 + lim.launch_rows);
      const int64_t pieces = ((t1 * Lo + 3) >> 2) - ((t0 * Lo) >> 2);
      hipLaunchKernelGGL(cross_single_k, dim3(blocks(pieces, XT)), dim3(XT), lds_terms, st, a, L, t0, t1, o->col, reinterpret_cast<uint32_t*>(o->val));
      FMX_HIP(hipGetLastError());
    }
  } else {
    // a lane group covers the longest row of the group form; the length pass walks longer rows in chunks of it
    const int reach = lim.group_max > 0 ? (int)std::min<int64_t>(lim.group_max, std::max(1, m->max_row_len)) : CROSS_GROUP_MAX;
    const int G = reach <= 16 ? 16 : reach <= 32 ? 32 : 64;
    int64_t *len = nullptr, *off = nullptr;   // off[n]: the total, off[n + 1]: the lowest row of more than 2^31 - 1 entries (all ones: none)
    FMX_TRY(S.get(&len, (size_t)n + 1)); FMX_TRY(S.get(&off, (size_t)n + 2));
    FMX_HIP(hipMemsetAsync(len + n, 0, sizeof(int64_t), st));
    FMX_HIP(hipMemsetAsync(off + n + 1, 0xFF, sizeof(int64_t), st));
    for (int64_t r0 = 0; r0 < n; r0 += lim.launch_rows) {
      const int64_t r1 = std::min(n, r0 + lim.launch_rows);
      hipLaunchKernelGGL(cross_len_k, dim3(blocks((r1 - r0) * G, XT)), dim3(XT), lds_tab, st, a, r0, r1, G, len, reinterpret_cast<unsigned long long*>(off + n + 1));
      FMX_HIP(hipGetLastError());
    }
    FMX_TRY(exclusive_sum(S, (const int64_t*)len, off, n + 1));
    int64_t back[2] = {0, 0};
    FMX_HIP(hipMemcpyAsync(back, off + n, sizeof(back), hipMemcpyDeviceToHost, st));
    FMX_HIP(hipStreamSynchronize(st));
    FMX_CHECK(back[1] == -1, FMX_ERR_INVALID, "row %lld would hold more than 2^31 - 1 entries", (long long)back[1]);
    FMX_CHECK(back[0] <= CROSS_MAX_ITEMS, FMX_ERR_INVALID, "the output would hold %lld entries: at most 2^31 - 1", (long long)back[0]);
    FMX_TRY(alloc_matrix(m->device, n, out_p, back[0], m->has_labels != 0, &o));
    hold.reset(o);
    FMX_HIP(hipMemcpyAsync(o->row_ptr, off, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    uint32_t *ocol = o->col, *oval = reinterpret_cast<uint32_t*>(o->val);
    const bool any_long = lim.group_max < 0 || m->max_row_len > lim.group_max;
    for (int64_t r0 = 0; r0 < n && back[0] > 0; r0 += lim.launch_rows) {
      const int64_t r1 = std::min(n, r0 + lim.launch_rows);
      if (lim.group_max > 0) {
        hipLaunchKernelGGL(cross_group_k, dim3(blocks((r1 - r0) * G, XT)), dim3(XT), lds_tab, st, a, (const int64_t*)off, r0, r1, G, lim.group_max, ocol, oval);
        FMX_HIP(hipGetLastError());
      }
      if (any_long) {
        hipLaunchKernelGGL(cross_long_k, dim3((unsigned)(r1 - r0)), dim3(XT), lds_long, st, a, (const int64_t*)off, r0, lim.group_max, ocol, oval);
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

}  // namespace
}  // namespace fmx

using namespace fmx;

extern "C" {

int fmx_debug_cross_limits(int32_t single, int32_t group_entries, int64_t rows_per_launch) {
  g_single.store(single);
  g_group.store(group_entries);
  g_rows.store(rows_per_launch > 0 ? rows_per_launch : 0);
  return FMX_OK;
}

int fmx_matrix_cross(const fmx_matrix* m, const fmx_cross_spec* spec, uint32_t* cross_base, fmx_matrix** out) {
  std::vector<uint32_t> cb;
  FMX_TRY(cross_check(m, spec, cross_base, out, &cb));
  FMX_TRY(use_device(m->device));
  FMX_TRY(cross_run(m, spec, cb, out));
  std::memcpy(cross_base, cb.data(), cb.size() * sizeof(uint32_t));
  return FMX_OK;
}

}  // extern "C"
