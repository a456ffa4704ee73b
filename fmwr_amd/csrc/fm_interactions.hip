// Exact pairwise interaction values (fmx_interactions*) and their per-group summary (fmx_interactions_summary).
//
// For one row with stored entries e_0 .. e_{m-1} (column c(e), value x_e) the pair term of entries a < b is
//     I(a, b) = sum_f t_a[f] t_b[f],   t_e[f] = (double) v_c(e),f * (double) x_e   (fm_contrib_k's tmp)
// formed as ONE fp64 chain: the accumulator starts at +0.0, f ascends over the engine's k factors, every product is rounded, then every sum
// (__dmul_rn / __dadd_rn: never an fma, whatever the build's contraction setting).  Only the k stored factors run through the chain, never
// the tables' zero padding (for finite x the padding could not change a bit -- a sum of exact zeros added to the accumulator -- but a NaN or
// an infinite x would turn it into NaN, so it stays out).  A NaN value leaves as the canonical quiet NaN.
//
// The order of a row's pairs ("strongest first"): the larger |I| first (-0 = +0), equal magnitudes by the lower a, then the lower b, NaN after
// every number in (a, b) order.  It is strict and total, so the top_m pairs of a row are unique, and both forms below, which evaluate the same
// chain per pair, give the same bits:
//   wave form       rows of at most E_w entries (32: configs[1]'s rows hold 30): one wave per row, four rows per workgroup.  The row's t goes
//                   into a padded LDS tile, one slice of 16 factors at a time (32 or 64 for rows of at most 16 or 8 entries); every lane
//                   owns up to 8 pairs of the triangle and carries their accumulators across the slices; top_m rounds of argmax under the
//                   order, by __shfl_xor butterflies of (key, position).  A wave orders its own LDS traffic; the kernel has no barrier.
//   workgroup form  longer rows, one workgroup per row: entries in tiles of E_t (32), the tile pairs (A <= B) in order, a thread owns up to 4 of
//                   a tile pair's E_t^2 values.  The running best top_m sits in LDS; a tile pair none of whose values beats the current
//                   last place is skipped, every other one is merged by top_m rounds of argmax over (old best, the tile pair's values).
// A row's result depends on the row and the parameters alone.  Nothing is ordered or summed by atomics.
//
// The summary gives each workgroup a contiguous run of rows (the cut is a function of the row count alone) and a triangular G x G table of
// (sum, abs_sum, count) in LDS.  Rows are taken in ascending order, a row's entries in tiles of 256; per tile pair the tiles are sorted stably
// by group (a rank count in LDS), so that the entries of one group are a run, and every cell {g, h} is owned by ONE thread, which adds the
// pairs of run g x run h sequentially into it.  On one-hot field data every run has length 1 and every cell gets one add per row.  The
// workgroups' tables go to global memory and a second kernel adds them per cell in ascending workgroup order.
#include <algorithm>
#include <atomic>
#include <vector>

#include "fm_rank.h"

namespace fmx {
namespace {

constexpr int IX_THREADS = 256;
constexpr int IX_WAVES = IX_THREADS / 64;
constexpr int IX_EW = 32;            // most entries of a wave-form row: 32 * 31 / 2 = 496 pairs <= 64 lanes * IX_PPL
constexpr int IX_PPL = 8;            // pairs per lane (wave form)
constexpr int IX_ET = 32;            // most entries of a tile (workgroup form): 32 * 32 values = 256 threads * IX_PPT
constexpr int IX_PPT = 4;            // values per thread and tile pair (workgroup form)
constexpr int IX_KS = 16;            // factors staged at a time
constexpr int IX_LD = IX_KS + 1;     // an odd row pitch in doubles: lanes reading one factor of different entries hit different banks
constexpr int IX_MAX_M = 64;         // top_m limit
constexpr int SM_TS = 256;           // entries per tile of the summary
constexpr int SM_TILE = 1024;        // doubles of t the summary stages per tile pair (8 KiB); larger tile pairs read V from L2
constexpr int SM_MAX_G = 64;         // group limit
constexpr int64_t SM_WGS = 1024;     // workgroups of the default row cut
constexpr int64_t SM_MAX_WGS = 65536;

std::atomic<int> g_ew_once{0}, g_et_once{0};
std::atomic<int64_t> g_rows_once{0};

__device__ __forceinline__ double ix_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double ix_add(double a, double b) { return __dadd_rn(a, b); }
// orders a wave's own LDS writes before its later LDS reads (other lanes' data): a wave's LDS instructions are served in order
__device__ __forceinline__ void ix_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double ix_canon(double v) { return v != v ? __longlong_as_double(0x7ff8000000000000LL) : v; }
// descending in this key = the order on values: 0 no candidate, 1 NaN, then the bits of |I| (monotone for non-negative doubles)
__device__ __forceinline__ unsigned long long ix_key(double v) {
  return v != v ? 1ull : (unsigned long long)__double_as_longlong(fabs(v)) + 2ull;
}
__device__ __forceinline__ bool ix_before(unsigned long long ka, unsigned long long pa, unsigned long long kb, unsigned long long pb) {
  return ka > kb || (ka == kb && pa < pb);
}

struct IxArgs {
  const int64_t* row_ptr;
  const uint32_t* col;
  const float* val;
  int64_t r0;        // first row of the launch
  int64_t nrows;
  const void* V;     // feature j's factors at V[j * vs]
  int64_t vs;
  int k;             // factors (not padded)
  int unit;          // every value is 1.0f: val is not read
  int top_m;
  int ew, et;        // a row of at most ew entries takes the wave form; tile size of the workgroup form
  int64_t* oa;       // [nrows][top_m]
  int64_t* ob;
  double* ov;
};

// (six waves per SIMD: the gathers and the LDS chain live on latency hiding; 80 VGPRs hold the 8 accumulators, keys and positions without scratch)
template <typename T>
__global__ __launch_bounds__(IX_THREADS, 6) void fm_interactions_wave_k(IxArgs a) {
  __shared__ double tile[IX_WAVES][IX_EW * IX_LD];
  __shared__ uint2 ent[IX_WAVES][IX_EW];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * IX_WAVES + wv;
  int m = -1;
  int64_t ta = 0;
  if (row < a.nrows) {
    ta = a.row_ptr[a.r0 + row];
    const int64_t len = a.row_ptr[a.r0 + row + 1] - ta;
    if (len <= a.ew) m = (int)len;   // a.ew <= IX_EW
  }
  if (m < 0) return;                 // not this form's row, or past the range (uniform over the wave; the kernel has no workgroup barrier)
  const int npairs = m * (m - 1) / 2;
  if (lane < m) ent[wv][lane] = make_uint2(a.col[ta + lane], a.unit ? 0x3f800000u : __float_as_uint(a.val[ta + lane]));

  // pair q of the triangle, by its higher entry: q = b (b - 1) / 2 + a
  int pa[IX_PPL], pb[IX_PPL];
  double acc[IX_PPL];
#pragma unroll
  for (int j = 0; j < IX_PPL; ++j) {
    const int q = lane + 64 * j;
    pa[j] = pb[j] = 0;                    // an idle slot: never read, never stored to the output
    if (64 * j < npairs) {                // uniform: a short row decodes only the slots it uses
      int b = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)q)) * 0.5f);
      while (b * (b - 1) / 2 > q) --b;
      while ((b + 1) * b / 2 <= q) ++b;
      if (q < npairs) { pb[j] = b; pa[j] = q - b * (b - 1) / 2; }
    }
    acc[j] = 0.0;
  }

  const T* __restrict__ Vt = reinterpret_cast<const T*>(a.V);
  // The wave works on its own part of the LDS alone, so it orders its LDS traffic with wave-level fences and never waits for the workgroup's
  // other rows.  A short row stages more factors at a time (the tile holds 544 doubles: 32 x 17, 16 x 33 or 8 x 65, the pitch odd each time):
  // fewer dependent gather rounds, and the chain's order is the same
  const int ks = m <= 8 ? 4 * IX_KS : m <= 16 ? 2 * IX_KS : IX_KS;
  const int ld = ks + 1;
  double* tw = tile[wv];
  for (int f0 = 0; f0 < a.k && npairs > 0; f0 += ks) {
    const int kn = a.k - f0 < ks ? a.k - f0 : ks;
    ix_wave_sync();   // ent is visible; the previous slice has been read
    for (int i = lane; i < m * ks; i += 64) {
      const int en = i / ks, f = i % ks;
      if (f < kn) {
        const uint2 u = ent[wv][en];
        tw[en * ld + f] = ix_mul((double)Vt[(size_t)u.x * a.vs + f0 + f], (double)__uint_as_float(u.y));
      }
    }
    ix_wave_sync();
#pragma unroll
    for (int j = 0; j < IX_PPL; ++j) {
      if (lane + 64 * j < npairs) {
        const double* ra = tw + pa[j] * ld;
        const double* rb = tw + pb[j] * ld;
        double s = acc[j];
        for (int f = 0; f < kn; ++f) s = ix_add(s, ix_mul(ra[f], rb[f]));
        acc[j] = s;
      }
    }
  }
  unsigned long long ck[IX_PPL];
  unsigned cp[IX_PPL];
#pragma unroll
  for (int j = 0; j < IX_PPL; ++j) {
    ck[j] = lane + 64 * j < npairs ? ix_key(acc[j]) : 0ull;
    cp[j] = (unsigned)(pa[j] * 64 + pb[j]);
  }
  unsigned taken = 0;
  const int live = a.top_m < npairs ? a.top_m : npairs;   // every round up to here has a winner; the slots after it are empty
  for (int t = 0; t < live; ++t) {
    unsigned long long bk = 0ull;
    unsigned bp = 0xffffffffu;
    double bv = 0.0;
    int bj = -1;
#pragma unroll
    for (int j = 0; j < IX_PPL; ++j) {
      if (ck[j] != 0ull && !((taken >> j) & 1u) && ix_before(ck[j], cp[j], bk, bp)) { bk = ck[j]; bp = cp[j]; bv = acc[j]; bj = j; }
    }
    unsigned long long wk = bk;
    unsigned wp = bp;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {   // commutative steps of a strict order: every lane ends with the same winner
      const unsigned long long ok = __shfl_xor(wk, off);
      const unsigned op = __shfl_xor(wp, off);
      if (ix_before(ok, op, wk, wp)) { wk = ok; wp = op; }
    }
    const size_t o = (size_t)row * a.top_m + t;
    if (bj >= 0 && bp == wp) {   // positions are unique: one lane owns the winner
      taken |= 1u << bj;
      a.oa[o] = (int64_t)(wp >> 6);
      a.ob[o] = (int64_t)(wp & 63u);
      a.ov[o] = ix_canon(bv);
    }
  }
  if (live + lane < a.top_m) {   // top_m <= 64: one lane per empty slot
    const size_t o = (size_t)row * a.top_m + live + lane;
    a.oa[o] = -1; a.ob[o] = -1; a.ov[o] = ix_canon(__longlong_as_double(-1LL));
  }
}

template <typename T>
__global__ __launch_bounds__(IX_THREADS) void fm_interactions_wg_k(IxArgs a) {
  __shared__ double tA[IX_ET * IX_LD], tB[IX_ET * IX_LD];
  __shared__ uint2 eA[IX_ET], eB[IX_ET];
  __shared__ unsigned long long bestk[2][IX_MAX_M], bestp[2][IX_MAX_M];
  __shared__ double bestv[2][IX_MAX_M];
  __shared__ unsigned long long wvk[2][IX_WAVES], wvp[2][IX_WAVES];
  __shared__ double wvv[2][IX_WAVES];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t row = blockIdx.x;
  const int64_t ta = a.row_ptr[a.r0 + row];
  const int64_t m = a.row_ptr[a.r0 + row + 1] - ta;
  if (m <= a.ew) return;   // the wave form's row (uniform over the workgroup)
  const int et = a.et, M = a.top_m;
  const T* __restrict__ Vt = reinterpret_cast<const T*>(a.V);
  int cur = 0;
  if (tid < IX_MAX_M) { bestk[0][tid] = 0ull; bestp[0][tid] = ~0ull; bestv[0][tid] = 0.0; }

  const int64_t ntiles = (m + et - 1) / et;
  for (int64_t A = 0; A < ntiles; ++A) {
    const int cntA = (int)(m - A * et < et ? m - A * et : et);
    for (int64_t B = A; B < ntiles; ++B) {
      const int cntB = (int)(m - B * et < et ? m - B * et : et);
      const bool diag = A == B;
      __syncthreads();   // the previous tile pair's LDS traffic is over (and the best list is initialised)
      if (tid < cntA) {
        const int64_t i = ta + A * et + tid;
        eA[tid] = make_uint2(a.col[i], a.unit ? 0x3f800000u : __float_as_uint(a.val[i]));
      } else if (!diag && tid >= 64 && tid - 64 < cntB) {
        const int64_t i = ta + B * et + (tid - 64);
        eB[tid - 64] = make_uint2(a.col[i], a.unit ? 0x3f800000u : __float_as_uint(a.val[i]));
      }
      int ia[IX_PPT], ib[IX_PPT];
      bool ok[IX_PPT];
      double acc[IX_PPT];
#pragma unroll
      for (int j = 0; j < IX_PPT; ++j) {
        const int q = tid + IX_THREADS * j;
        ia[j] = q / et;
        ib[j] = q % et;
        ok[j] = ia[j] < cntA && ib[j] < cntB && (!diag || ia[j] < ib[j]);
        if (!ok[j]) ia[j] = ib[j] = 0;
        acc[j] = 0.0;
      }
      const double* tb = diag ? tA : tB;
      for (int f0 = 0; f0 < a.k; f0 += IX_KS) {
        const int kn = a.k - f0 < IX_KS ? a.k - f0 : IX_KS;
        __syncthreads();
        const int slots = cntA + (diag ? 0 : cntB);
        for (int i = tid; i < slots * IX_KS; i += IX_THREADS) {
          const int en = i / IX_KS, f = i % IX_KS;
          if (f < kn) {
            const uint2 u = en < cntA ? eA[en] : eB[en - cntA];
            const double t = ix_mul((double)Vt[(size_t)u.x * a.vs + f0 + f], (double)__uint_as_float(u.y));
            if (en < cntA) tA[en * IX_LD + f] = t;
            else tB[(en - cntA) * IX_LD + f] = t;
          }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < IX_PPT; ++j) {
          if (ok[j]) {
            const double* ra = &tA[ia[j] * IX_LD];
            const double* rb = &tb[ib[j] * IX_LD];
            double s = acc[j];
            for (int f = 0; f < kn; ++f) s = ix_add(s, ix_mul(ra[f], rb[f]));
            acc[j] = s;
          }
        }
      }

      // candidates of this tile pair that come before the current last place (all of them while the list is not full)
      const unsigned long long lk = bestk[cur][M - 1], lp = bestp[cur][M - 1];
      unsigned long long ck[IX_PPT + 1], cp[IX_PPT + 1];
      bool any = false;
#pragma unroll
      for (int j = 0; j < IX_PPT; ++j) {
        ck[j] = ok[j] ? ix_key(acc[j]) : 0ull;
        cp[j] = ((unsigned long long)(A * et + ia[j]) << 32) | (unsigned long long)(B * et + ib[j]);
        if (ck[j] != 0ull && !ix_before(ck[j], cp[j], lk, lp)) ck[j] = 0ull;
        any = any || ck[j] != 0ull;
      }
      if (!__syncthreads_or(any ? 1 : 0)) continue;   // uniform

      // merge: thread t < M also holds the old list's entry t; M rounds of argmax rebuild the list in the other buffer
      double ov = 0.0;
      ck[IX_PPT] = 0ull; cp[IX_PPT] = ~0ull;
      if (tid < M) { ck[IX_PPT] = bestk[cur][tid]; cp[IX_PPT] = bestp[cur][tid]; ov = bestv[cur][tid]; }
      unsigned taken = 0;
      for (int t = 0; t < M; ++t) {
        const int par = t & 1;
        unsigned long long bk = 0ull, bp = ~0ull;
        double bv = 0.0;
        int bj = -1;
#pragma unroll
        for (int j = 0; j <= IX_PPT; ++j) {
          if (ck[j] != 0ull && !((taken >> j) & 1u) && ix_before(ck[j], cp[j], bk, bp)) {
            bk = ck[j]; bp = cp[j]; bj = j;
            bv = j < IX_PPT ? acc[j < IX_PPT ? j : 0] : ov;
          }
        }
        unsigned long long wk = bk, wp = bp;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const unsigned long long k2 = __shfl_xor(wk, off);
          const unsigned long long p2 = __shfl_xor(wp, off);
          if (ix_before(k2, p2, wk, wp)) { wk = k2; wp = p2; }
        }
        if (lane == 0) { wvk[par][wv] = wk; wvp[par][wv] = wp; }
        if (wk != 0ull && bj >= 0 && bp == wp) wvv[par][wv] = bv;
        __syncthreads();   // one barrier per round: round t + 2 reuses this buffer only after every thread has passed round t + 1's barrier
        unsigned long long gk = wvk[par][0], gp = wvp[par][0];
        int gw = 0;
#pragma unroll
        for (int w = 1; w < IX_WAVES; ++w) {
          if (ix_before(wvk[par][w], wvp[par][w], gk, gp)) { gk = wvk[par][w]; gp = wvp[par][w]; gw = w; }
        }
        if (gk != 0ull && bj >= 0 && bp == gp) taken |= 1u << bj;
        if (tid == 0) {
          bestk[cur ^ 1][t] = gk;
          bestp[cur ^ 1][t] = gk != 0ull ? gp : ~0ull;
          bestv[cur ^ 1][t] = gk != 0ull ? wvv[par][gw] : 0.0;
        }
      }
      cur ^= 1;
    }
  }
  __syncthreads();
  if (tid < M) {
    const size_t o = (size_t)row * M + tid;
    const unsigned long long k = bestk[cur][tid], p = bestp[cur][tid];
    a.oa[o] = k != 0ull ? (int64_t)(p >> 32) : -1;
    a.ob[o] = k != 0ull ? (int64_t)(p & 0xffffffffull) : -1;
    a.ov[o] = k != 0ull ? ix_canon(bestv[cur][tid]) : ix_canon(__longlong_as_double(-1LL));
  }
}

// ---------------------------------------------------------------------------------------------------------------- summary

struct SumArgs {
  const int64_t* row_ptr;
  const uint32_t* col;
  const float* val;
  int64_t n;
  const void* V;
  int64_t vs;
  int k;
  int unit;
  const uint32_t* grp;   // group of feature j; null: j itself
  int G;
  int64_t rows_per_wg;
  double* part;          // [workgroups][2][cells]: sum, abs_sum
  int64_t* pcnt;         // [workgroups][cells]
};

__host__ __device__ inline int sm_cells(int G) { return G * (G + 1) / 2; }
__device__ __forceinline__ int sm_cell(int G, int g, int h) { return g * G - g * (g - 1) / 2 + (h - g); }   // g <= h
inline size_t sm_lds_bytes(int G) {
  return (size_t)sm_cells(G) * 24 + SM_TILE * sizeof(double) + 2 * SM_TS * 2 * sizeof(uint32_t) + 2 * SM_MAX_G * 2 * sizeof(int) + 2 * SM_TS;
}

template <typename T>
__global__ __launch_bounds__(IX_THREADS) void fm_interactions_summary_k(SumArgs a) {
  extern __shared__ double sm_lds[];
  const int G = a.G, cells = sm_cells(G);
  double* s_sum = sm_lds;
  double* s_abs = s_sum + cells;
  long long* s_cnt = reinterpret_cast<long long*>(s_abs + cells);
  double* tile = reinterpret_cast<double*>(s_cnt + cells);
  uint32_t* ecol = reinterpret_cast<uint32_t*>(tile + SM_TILE);   // [2][SM_TS], sorted by group
  uint32_t* exb = ecol + 2 * SM_TS;                               // [2][SM_TS]
  int* rbeg = reinterpret_cast<int*>(exb + 2 * SM_TS);            // [2][SM_MAX_G]: the run of group g in tile w is [rbeg, rend)
  int* rend = rbeg + 2 * SM_MAX_G;
  unsigned char* rawg = reinterpret_cast<unsigned char*>(rend + 2 * SM_MAX_G);   // [2][SM_TS], entry order

  const int tid = threadIdx.x;
  const T* __restrict__ Vt = reinterpret_cast<const T*>(a.V);
  for (int i = tid; i < cells; i += IX_THREADS) { s_sum[i] = 0.0; s_abs[i] = 0.0; s_cnt[i] = 0; }
  const int ld = a.k | 1;   // odd pitch of a staged t row

  const int64_t R0 = (int64_t)blockIdx.x * a.rows_per_wg;
  const int64_t R1 = R0 + a.rows_per_wg < a.n ? R0 + a.rows_per_wg : a.n;
  for (int64_t row = R0; row < R1; ++row) {
    const int64_t ta = a.row_ptr[row];
    const int64_t m = a.row_ptr[row + 1] - ta;
    if (m < 2) continue;
    const int64_t ntiles = (m + SM_TS - 1) / SM_TS;
    for (int64_t A = 0; A < ntiles; ++A) {
      for (int64_t B = A; B < ntiles; ++B) {
        const bool diag = A == B;
        const int cnt[2] = {(int)(m - A * SM_TS < SM_TS ? m - A * SM_TS : SM_TS), diag ? 0 : (int)(m - B * SM_TS < SM_TS ? m - B * SM_TS : SM_TS)};
        __syncthreads();   // the previous tile pair is done with the staging (and the tables are initialised)
        uint32_t c[2] = {0, 0}, xb[2] = {0, 0};
        int g[2] = {0, 0};
#pragma unroll
        for (int w = 0; w < 2; ++w) {
          if (tid < cnt[w]) {
            const int64_t i = ta + (w ? B : A) * SM_TS + tid;
            c[w] = a.col[i];
            xb[w] = a.unit ? 0x3f800000u : __float_as_uint(a.val[i]);
            g[w] = (int)(a.grp ? a.grp[c[w]] : c[w]);
            rawg[w * SM_TS + tid] = (unsigned char)g[w];
          }
        }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 2; ++w) {   // stable rank of the entry among its tile's groups; the group's run (thread g)
          int rank = 0, lo = 0, eq = 0;
          for (int j = 0; j < cnt[w]; ++j) {
            const int gj = rawg[w * SM_TS + j];
            rank += (gj < g[w] || (gj == g[w] && j < tid)) ? 1 : 0;
            lo += gj < tid ? 1 : 0;
            eq += gj == tid ? 1 : 0;
          }
          if (tid < cnt[w]) { ecol[w * SM_TS + rank] = c[w]; exb[w * SM_TS + rank] = xb[w]; }
          if (tid < G) { rbeg[w * SM_MAX_G + tid] = lo; rend[w * SM_MAX_G + tid] = lo + eq; }
        }
        __syncthreads();
        const int slots = cnt[0] + cnt[1];
        const bool staged = a.k > 0 && slots * ld <= SM_TILE;   // uniform
        if (staged) {
          for (int i = tid; i < slots * a.k; i += IX_THREADS) {
            const int en = i / a.k, f = i % a.k;
            const int w = en < cnt[0] ? 0 : 1, s = w ? en - cnt[0] : en;
            tile[en * ld + f] = ix_mul((double)Vt[(size_t)ecol[w * SM_TS + s] * a.vs + f], (double)__uint_as_float(exb[w * SM_TS + s]));
          }
          __syncthreads();
        }
        // I of sorted entry ea of tile 0 with sorted entry eb of tile wb
        auto pair_value = [&](int ea, int wb, int eb) -> double {
          double s = 0.0;
          if (staged) {
            const double* ra = tile + ea * ld;
            const double* rb = tile + (wb ? cnt[0] + eb : eb) * ld;
            for (int f = 0; f < a.k; ++f) s = ix_add(s, ix_mul(ra[f], rb[f]));
          } else {
            const T* va = Vt + (size_t)ecol[ea] * a.vs;
            const T* vb = Vt + (size_t)ecol[wb * SM_TS + eb] * a.vs;
            const double xa = (double)__uint_as_float(exb[ea]), xq = (double)__uint_as_float(exb[wb * SM_TS + eb]);
            for (int f = 0; f < a.k; ++f) s = ix_add(s, ix_mul(ix_mul((double)va[f], xa), ix_mul((double)vb[f], xq)));
          }
          return s;
        };
        for (int q = tid; q < G * G; q += IX_THREADS) {   // one thread per cell {g <= h}: no two threads add into one cell
          const int cg = q / G, ch = q % G;
          if (cg > ch) continue;
          const int wb = diag ? 0 : 1;
          const int ag0 = rbeg[cg], ag1 = rend[cg], bh0 = rbeg[wb * SM_MAX_G + ch], bh1 = rend[wb * SM_MAX_G + ch];
          const int ah0 = rbeg[ch], ah1 = rend[ch], bg0 = rbeg[wb * SM_MAX_G + cg], bg1 = rend[wb * SM_MAX_G + cg];
          const bool first = ag1 > ag0 && bh1 > bh0 && (cg != ch || !diag || ag1 - ag0 > 1);
          const bool second = !diag && cg != ch && ah1 > ah0 && bg1 > bg0;
          if (!first && !second) continue;
          const int cell = sm_cell(G, cg, ch);
          double s = s_sum[cell], ab = s_abs[cell];
          long long n = s_cnt[cell];
          if (first) {
            for (int ea = ag0; ea < ag1; ++ea) {
              for (int eb = (diag && cg == ch) ? ea + 1 : bh0; eb < bh1; ++eb) {
                const double v = pair_value(ea, wb, eb);
                s = ix_add(s, v); ab = ix_add(ab, fabs(v)); ++n;
              }
            }
          }
          if (second) {   // tile A's run of h with tile B's run of g: the same unordered cell
            for (int ea = ah0; ea < ah1; ++ea) {
              for (int eb = bg0; eb < bg1; ++eb) {
                const double v = pair_value(ea, wb, eb);
                s = ix_add(s, v); ab = ix_add(ab, fabs(v)); ++n;
              }
            }
          }
          s_sum[cell] = s; s_abs[cell] = ab; s_cnt[cell] = n;
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < cells; i += IX_THREADS) {
    a.part[((size_t)blockIdx.x * 2 + 0) * cells + i] = s_sum[i];
    a.part[((size_t)blockIdx.x * 2 + 1) * cells + i] = s_abs[i];
    a.pcnt[(size_t)blockIdx.x * cells + i] = s_cnt[i];
  }
}

// the workgroups' tables, added per cell in ascending workgroup order, into the symmetric G x G tables
__global__ __launch_bounds__(IX_THREADS) void fm_interactions_summary_add_k(const double* __restrict__ part, const int64_t* __restrict__ pcnt, int64_t wgs, int G,
                                                                           double* __restrict__ sum, double* __restrict__ abs_sum, int64_t* __restrict__ count) {
  const int q = blockIdx.x * IX_THREADS + threadIdx.x;
  if (q >= G * G) return;
  const int g = q / G, h = q % G;
  if (g > h) return;
  const int cells = sm_cells(G), cell = sm_cell(G, g, h);
  double s = 0.0, ab = 0.0;
  int64_t n = 0;
  for (int64_t w = 0; w < wgs; ++w) {
    s = ix_add(s, part[((size_t)w * 2 + 0) * cells + cell]);
    ab = ix_add(ab, part[((size_t)w * 2 + 1) * cells + cell]);
    n += pcnt[(size_t)w * cells + cell];
  }
  sum[g * G + h] = s; sum[h * G + g] = s;
  abs_sum[g * G + h] = ab; abs_sum[h * G + g] = ab;
  count[g * G + h] = n; count[h * G + g] = n;
}

void ix_tables(const fmx_engine* e, const void** V, int64_t* vs) {
  if (wide_state(e)) { *V = e->dV; *vs = e->kp64; }
  else { *V = e->V; *vs = e->vstride32; }
}

}  // namespace

InterLimits interactions_take_limits() {
  InterLimits l;
  l.wave_entries = g_ew_once.exchange(0);
  l.tile_entries = g_et_once.exchange(0);
  l.summary_rows = g_rows_once.exchange(0);
  if (l.wave_entries <= 0 || l.wave_entries > IX_EW) l.wave_entries = IX_EW;
  if (l.tile_entries < 2 || l.tile_entries > IX_ET) l.tile_entries = IX_ET;
  if (l.summary_rows < 0) l.summary_rows = 0;
  return l;
}

void debug_interactions_limits(int wave_entries, int tile_entries, int64_t summary_rows) {
  g_ew_once.store(wave_entries > 0 ? wave_entries : 0);
  g_et_once.store(tile_entries > 0 ? tile_entries : 0);
  g_rows_once.store(summary_rows > 0 ? summary_rows : 0);
}

int interactions_run(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, int top_m, const InterLimits& lim, int64_t* d_a, int64_t* d_b, double* d_v) {
  if (r1 <= r0) return FMX_OK;
  IxArgs a{};
  a.row_ptr = m->row_ptr; a.col = m->col; a.val = m->val;
  a.r0 = r0; a.nrows = r1 - r0;
  ix_tables(e, &a.V, &a.vs);
  a.k = e->k;
  a.unit = m->unit_values;
  a.top_m = top_m;
  a.ew = lim.wave_entries; a.et = lim.tile_entries;
  a.oa = d_a; a.ob = d_b; a.ov = d_v;
  FMX_CHECK(a.nrows < (1LL << 31), FMX_ERR_INVALID, "interactions: at most 2^31 - 1 rows per call (got %lld)", (long long)a.nrows);
  const bool wide = wide_state(e);
  const unsigned wgrid = (unsigned)((a.nrows + IX_WAVES - 1) / IX_WAVES);
  if (wide) hipLaunchKernelGGL(fm_interactions_wave_k<double>, dim3(wgrid), dim3(IX_THREADS), 0, e->stream, a);
  else hipLaunchKernelGGL(fm_interactions_wave_k<float>, dim3(wgrid), dim3(IX_THREADS), 0, e->stream, a);
  FMX_HIP(hipGetLastError());
  if (m->max_row_len > a.ew || m->max_row_len <= 0) {   // some row may be longer than the wave form takes: those rows' workgroups do the work
    if (wide) hipLaunchKernelGGL(fm_interactions_wg_k<double>, dim3((unsigned)a.nrows), dim3(IX_THREADS), 0, e->stream, a);
    else hipLaunchKernelGGL(fm_interactions_wg_k<float>, dim3((unsigned)a.nrows), dim3(IX_THREADS), 0, e->stream, a);
    FMX_HIP(hipGetLastError());
  }
  return FMX_OK;
}

int interactions_summary_run(fmx_engine* e, const fmx_matrix* m, const uint32_t* groups, int G, const InterLimits& lim, double* sum, double* abs_sum, int64_t* count) {
  if (m->n == 0) return FMX_OK;
  int64_t rows = lim.summary_rows > 0 ? lim.summary_rows : (m->n + SM_WGS - 1) / SM_WGS;   // the row cut: a function of the row count alone
  if ((m->n + rows - 1) / rows > SM_MAX_WGS) rows = (m->n + SM_MAX_WGS - 1) / SM_MAX_WGS;
  const int64_t wgs = (m->n + rows - 1) / rows;
  const size_t cells = (size_t)sm_cells(G), gg = (size_t)G * G;
  DevBuf dgrp, part, pcnt, out;
  if (groups) {
    FMX_TRY(dev_buf(&dgrp, (size_t)m->p * sizeof(uint32_t)));
    FMX_HIP(hipMemcpy(dgrp.get(), groups, (size_t)m->p * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  FMX_TRY(dev_buf(&part, (size_t)wgs * 2 * cells * sizeof(double)));
  FMX_TRY(dev_buf(&pcnt, (size_t)wgs * cells * sizeof(int64_t)));
  FMX_TRY(dev_buf(&out, gg * (2 * sizeof(double) + sizeof(int64_t))));
  double* d_sum = (double*)out.get();
  double* d_abs = d_sum + gg;
  int64_t* d_cnt = (int64_t*)(d_abs + gg);
  SumArgs a{};
  a.row_ptr = m->row_ptr; a.col = m->col; a.val = m->val;
  a.n = m->n;
  ix_tables(e, &a.V, &a.vs);
  a.k = e->k;
  a.unit = m->unit_values;
  a.grp = (const uint32_t*)dgrp.get();
  a.G = G;
  a.rows_per_wg = rows;
  a.part = (double*)part.get();
  a.pcnt = (int64_t*)pcnt.get();
  const size_t lds = sm_lds_bytes(G);   // at most 63 744 bytes (G = 64)
  if (wide_state(e)) hipLaunchKernelGGL(fm_interactions_summary_k<double>, dim3((unsigned)wgs), dim3(IX_THREADS), lds, e->stream, a);
  else hipLaunchKernelGGL(fm_interactions_summary_k<float>, dim3((unsigned)wgs), dim3(IX_THREADS), lds, e->stream, a);
  FMX_HIP(hipGetLastError());
  hipLaunchKernelGGL(fm_interactions_summary_add_k, dim3((unsigned)((gg + IX_THREADS - 1) / IX_THREADS)), dim3(IX_THREADS), 0, e->stream, (const double*)a.part,
                     (const int64_t*)a.pcnt, wgs, G, d_sum, d_abs, d_cnt);
  FMX_HIP(hipGetLastError());
  FMX_HIP(hipStreamSynchronize(e->stream));
  std::vector<double> hs(gg), ha(gg);
  std::vector<int64_t> hc(gg);
  FMX_HIP(hipMemcpy(hs.data(), d_sum, gg * sizeof(double), hipMemcpyDeviceToHost));
  FMX_HIP(hipMemcpy(ha.data(), d_abs, gg * sizeof(double), hipMemcpyDeviceToHost));
  FMX_HIP(hipMemcpy(hc.data(), d_cnt, gg * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::copy(hs.begin(), hs.end(), sum);   // the caller's arrays are written only once everything has succeeded
  std::copy(ha.begin(), ha.end(), abs_sum);
  if (count) std::copy(hc.begin(), hc.end(), count);
  return FMX_OK;
}

}  // namespace fmx
