// What the ranking entry points share ("shared ranking code"): fm_topk.hip, fm_heldout.hip, fm_lists.hip and
// fm_pairs.hip agree bit for bit on a pair's score and on the order of two pairs because they take both from here; fm_neighbors.hip takes the
// order and fm_topk.hip's LDS selection; fm_contrib.hip and fm_foldin.hip take the vector trait and the device buffers.  The tile dot loops of topk_score_k and heldout_count_k are NOT here: moved
// into a shared function they compile to other code (DESIGN.md section 12 has the figures), so they stay written out where they run.
#pragma once
#include <algorithm>
#include <memory>
#include <vector>

#include "fmx_internal.h"
#include "fm_probit.h"

namespace fmx {

// ---------------------------------------------------------------------------------------------------------------- device side

// the state type's 16-byte vector
template <typename T> struct StateVec;
template <> struct StateVec<float> { using vec = float4; static constexpr int N = 4; };
template <> struct StateVec<double> { using vec = double2; static constexpr int N = 2; };

// the total order of every ranking path: does (sa, ia) come before (sb, ib)?  A higher score first, equal scores by the lower index, NaN
// below every number
template <typename I>
__device__ __forceinline__ bool rank_before(double sa, I ia, double sb, I ib) {
  const bool an = sa != sa, bn = sb != sb;
  if (an != bn) return bn;
  if (!an && sa != sb) return sa > sb;
  return ia < ib;
}

// ascending in this key = the total order on scores (ties of the key are equal scores; -0 and +0 are one score, NaN last)
__device__ __forceinline__ uint64_t rank_order_key(double s) {
  if (s != s) return ~0ull;
  s = (s == 0.0) ? 0.0 : s;
  const uint64_t u = (uint64_t)__double_as_longlong(s);
  const uint64_t asc = (u >> 63) ? ~u : (u | 0x8000000000000000ull);  // ascending in s
  return ~asc;
}

// The counter-based hash of the pair sampler (fm_pairs.hip) and the row selection (fm_select.hip): splitmix64's finaliser, chained over the
// words of the counter.  tests/split_model.py restates it; the bits are pinned there and by the sampler's tests.
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
__device__ __forceinline__ uint64_t pair_hash(uint64_t seed, uint64_t epoch, uint64_t t, uint64_t stream) {
  uint64_t h = mix64(seed + 0x9E3779B97F4A7C15ull);
  h = mix64(h ^ (epoch * 0xD6E8FEB86659FD93ull + stream));
  return mix64(h ^ (t + 0x632BE59BD9B4E019ull));
}

// the output transform of fmx_predict (link_apply in fm_batch_kernels.hip), on the raw score of a selected pair
__device__ __forceinline__ double rank_link(const Hyper& h, double y, int link, const double* __restrict__ pn_y) {
  if (link == FMX_LINK_LOGISTIC) return 1.0 / (1.0 + exp(-y));
  if (link == FMX_LINK_PROBIT) return fast_pnorm(pn_y, y);
  if (link == FMX_LINK_CLAMP) {
    if (y < h.min_t) return h.min_t;
    if (y > h.max_t) return h.max_t;
  }
  return y;
}

constexpr int TK_SEG = 2048;       // exclusion lists are sorted (and searched) in segments of this many ids
constexpr int TK_KS_BYTES = 1024;  // a context's s in LDS: at most 256 floats / 128 doubles
// is item j in the context's exclusion list x[a, b), sorted within each segment of TK_SEG ids?
static __device__ bool tk_excluded(const uint32_t* __restrict__ x, int64_t a, int64_t b, uint32_t j) {
  for (int64_t s0 = a; s0 < b; s0 += TK_SEG) {
    const int64_t end = b < s0 + TK_SEG ? b : s0 + TK_SEG;
    int64_t lo = s0, hi = end;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (x[mid] < j) lo = mid + 1; else hi = mid;
    }
    if (lo < end && x[lo] == j) return true;
  }
  return false;
}
// the score of one (context, item) pair exactly as topk_score_k forms it: an fma chain in the state type T over f = 0 .. ks-1 (the
// zero-padded factors included), then (base_c + base_i) + (double)dot
template <typename T>
__device__ __forceinline__ double tk_pair_score(const T* __restrict__ sc, const T* __restrict__ si, int ks, double bc, double bi) {
  T acc = (T)0;
  for (int f = 0; f < ks; ++f) acc = fma(sc[f], si[f], acc);
  return (bc + bi) + (double)acc;
}

// The selection of fm_topk.hip and fm_neighbors.hip (DESIGN.md sections 12 and 21): a workgroup's running top K per context row in LDS, and the merge
// of the per-slice lists.  In an unnamed namespace, as in fm_topk.hip before the move: every file that uses them compiles its own copy under the
// same symbol names, which is what profiles/isa_check.py compares.
namespace {

constexpr int TK_THREADS = 256;
constexpr int32_t TK_NONE = 0x7FFFFFFF;    // padding entry (score NaN): below every item, NaN-scored ones included

// Selection state of CT contexts in LDS: slots [0, K) the current top K in order, [K, K + cnt) candidates, the rest padding.
// Invariant between flushes: cnt <= L - K - TK_THREADS, so one round of the workgroup (at most one candidate per thread and
// context) always fits.  L >= K + TK_THREADS.
template <int CT, int L>
struct TkSel {
  double s[CT][L];
  int32_t i[CT][L];
  int cnt[CT];
};

template <int CT, int L>
__device__ void tk_init(TkSel<CT, L>& q) {
  for (int t = threadIdx.x; t < CT * L; t += TK_THREADS) { q.s[t / L][t % L] = __builtin_nan(""); q.i[t / L][t % L] = TK_NONE; }
  if (threadIdx.x < CT) q.cnt[threadIdx.x] = 0;
}

// bitonic sort of every context's L slots, best first; then slots [K, L) back to padding.  Ends with a barrier.
template <int CT, int L>
__device__ void tk_flush(TkSel<CT, L>& q, int K) {
  __syncthreads();
  for (int size = 2; size <= L; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < CT * (L / 2); t += TK_THREADS) {
        const int c = t / (L / 2), pr = t % (L / 2);
        const int a = 2 * pr - (pr & (stride - 1));  // the pair (a, a + stride), a with bit `stride` clear
        const int b = a + stride;
        const double sa = q.s[c][a], sb = q.s[c][b];
        const int32_t ia = q.i[c][a], ib = q.i[c][b];
        const bool swap = (a & size) == 0 ? rank_before(sb, ib, sa, ia) : rank_before(sa, ia, sb, ib);
        if (swap) { q.s[c][a] = sb; q.s[c][b] = sa; q.i[c][a] = ib; q.i[c][b] = ia; }
      }
      __syncthreads();
    }
  }
  for (int t = threadIdx.x; t < CT * (L - K); t += TK_THREADS) {
    const int c = t / (L - K), r = K + t % (L - K);
    q.s[c][r] = __builtin_nan(""); q.i[c][r] = TK_NONE;
  }
  if (threadIdx.x < CT) q.cnt[threadIdx.x] = 0;
  __syncthreads();
}

// one round done (every thread has offered its candidates): flush if a buffer could overflow in the next round
template <int CT, int L>
__device__ void tk_round(TkSel<CT, L>& q, int K) {
  __syncthreads();
  bool full = false;
#pragma unroll
  for (int c = 0; c < CT; ++c) full |= q.cnt[c] > L - K - TK_THREADS;
  __syncthreads();                  // every thread has read the counts before the next round appends
  if (full) tk_flush<CT, L>(q, K);  // uniform: every thread read the same counts
}

template <int CT, int L>
__device__ __forceinline__ void tk_offer(TkSel<CT, L>& q, int K, int c, double s, int32_t j) {
  const int pos = atomicAdd(&q.cnt[c], 1);  // order of the appends is irrelevant: the flush sorts under the total order
  q.s[c][K + pos] = s;
  q.i[c][K + pos] = j;
}

// one workgroup per context: the S per-slice lists through the same selection, then the link; item index -1 / NaN for padding
template <int L>
__global__ __launch_bounds__(TK_THREADS) void topk_merge_k(const double* __restrict__ ps, const int32_t* __restrict__ pi, int S, int K, Hyper h, int link,
                                                         const double* __restrict__ pn_y, int64_t* __restrict__ oi, double* __restrict__ os) {
  __shared__ TkSel<1, L> q;
  tk_init<1, L>(q);
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * S * K;
  const int64_t total = (int64_t)S * K;
  double ts = __builtin_nan("");
  int32_t ti = TK_NONE;
  for (int64_t e0 = 0; e0 < total; e0 += TK_THREADS) {
    const int64_t e = e0 + threadIdx.x;
    if (e < total) {
      const double s = ps[base + e];
      const int32_t j = pi[base + e];
      if (j != TK_NONE && rank_before(s, j, ts, ti)) tk_offer<1, L>(q, K, 0, s, j);
    }
    tk_round<1, L>(q, K);
    ts = q.s[0][K - 1]; ti = q.i[0][K - 1];
  }
  tk_flush<1, L>(q, K);
  for (int r = threadIdx.x; r < K; r += TK_THREADS) {
    const int32_t j = q.i[0][r];
    const size_t o = (size_t)blockIdx.x * K + r;
    oi[o] = j == TK_NONE ? -1 : (int64_t)j;
    os[o] = j == TK_NONE ? __builtin_nan("") : rank_link(h, q.s[0][r], link, pn_y);
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------- host side

// fm_topk.hip: base and s of rows [r0, r1) of m through the forward's row walk (fixed schedule): base = y_hat (w0 only if with_w0), s = the
// fp64 factor sums in the state type (float for fp32 tables, double for fp64), zero-padded to ks; q is scratch of min(r1 - r0, 2^16) x kp doubles
int topk_project_rows(fmx_engine* e, const fmx_matrix* m, int64_t r0, int64_t r1, bool with_w0, double* q, int ks, double* base, void* s);
// the exclusion ids of rows [0, nrows) of rp / col (absolute offsets rp[r]) into xs[rp[r] - base ...], sorted within segments of TK_SEG
int topk_sort_excl(hipStream_t st, const int64_t* rp, int64_t nrows, const uint32_t* col, int64_t base, uint32_t* xs);

// the factors of a projected row: k padded with zeros to whole blocks of four 16-byte loads
template <typename T>
int state_factors(const fmx_engine* e) {
  constexpr int FB = 4 * StateVec<T>::N;
  return (e->k + FB - 1) / FB * FB;
}

inline unsigned blocks(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

inline int device_cus(int device) {
  hipDeviceProp_t pr{};
  return (hipGetDeviceProperties(&pr, device) == hipSuccess && pr.multiProcessorCount > 0) ? pr.multiProcessorCount : 256;
}

// the item slices of a (context tile x item slice) grid: enough workgroups for the device (two resident per CU, four rounds of them), slices
// of at least 1 024 items and a multiple of the workgroup
inline void rank_slices(int64_t ni, int64_t tiles, int cus, int threads, int64_t* slice, int64_t* S) {
  int64_t n = std::max<int64_t>(1, std::min<int64_t>((8LL * cus + tiles - 1) / tiles, ni / 1024));
  int64_t sl = ((ni + n - 1) / n + threads - 1) / threads * threads;
  if (sl == 0) sl = threads;
  *slice = sl;
  *S = std::max<int64_t>(1, (ni + sl - 1) / sl);
}

// the buffer of L slots per context and the tile height that keeps a workgroup's selection state at 48 KiB
inline int topk_slots(int K) { return K + TK_THREADS <= 512 ? 512 : K + TK_THREADS <= 1024 ? 1024 : 2048; }
inline int topk_tile(int L) { return L == 512 ? 8 : L == 1024 ? 4 : 2; }

// one device buffer, freed when it goes out of scope or is replaced (the caller drains the stream that may still use it first)
struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
using DevBuf = std::unique_ptr<void, DevFree>;
inline int dev_buf(DevBuf* b, size_t bytes) {
  void* p = nullptr;
  FMX_HIP(hipMalloc(&p, bytes ? bytes : 1));
  b->reset(p);
  return FMX_OK;
}

// device allocations of one call, freed on every exit after the stream drains (default-constructed: after the whole device drains)
struct Scratch {
  hipStream_t st = nullptr;
  bool device = true;
  std::vector<void*> p;
  Scratch() {}
  explicit Scratch(hipStream_t s) : st(s), device(false) {}
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  template <typename T>
  int get(T** out, size_t count) {
    void* q = nullptr;
    FMX_HIP(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    p.push_back(q);
    *out = (T*)q;
    return FMX_OK;
  }
  // The temporary storage of the call's sorts and scans (fm_prims.h): ONE block that only grows.  A larger request takes a new block; the old
  // one stays on the list until the destructor, so a kernel in flight keeps its storage.  Calls on the one stream take turns on the block.
  int temp(size_t bytes, void** out) {
    if (bytes > tmp_bytes) { FMX_TRY(get(&tmp, bytes)); tmp_bytes = bytes; }
    *out = tmp;
    return FMX_OK;
  }
  // f(temp, bytes) in the two-phase form: once for the size, once to run on the block
  template <typename F>
  int with_temp(F f) {
    size_t bytes = 0;
    void* t = nullptr;
    FMX_TRY(f(nullptr, bytes)); FMX_TRY(temp(bytes, &t));
    return f(t, bytes);
  }
  ~Scratch() {
    if (device) (void)hipDeviceSynchronize(); else (void)hipStreamSynchronize(st);
    for (void* q : p) (void)hipFree(q);
  }

 private:
  uint8_t* tmp = nullptr;
  size_t tmp_bytes = 0;
};

// the projections of one call (topk_project_rows): the items' s and base, one chunk of contexts', and the fp64 staging q
template <typename T>
struct Projections {
  double *q = nullptr, *ib = nullptr, *cb = nullptr;
  T *is = nullptr, *cs = nullptr;
  int reserve(Scratch& S, int64_t ni, int64_t max_nc, int kp, int ks) {
    FMX_TRY(S.get(&q, (size_t)std::min<int64_t>(std::max(ni, max_nc), 1 << 16) * kp));
    FMX_TRY(S.get(&is, (size_t)ni * ks)); FMX_TRY(S.get(&ib, (size_t)ni));
    FMX_TRY(S.get(&cs, (size_t)max_nc * ks)); FMX_TRY(S.get(&cb, (size_t)max_nc));
    return FMX_OK;
  }
};

// chunks of at most chunk_max rows, halved until a chunk's entries fit max_entries (a row with more is a chunk of its own): chunk c covers
// rows [cut[c], cut[c + 1]) of the n rows whose entry offsets are hrp[0 .. n]
inline std::vector<int64_t> rank_chunks(const std::vector<int64_t>& hrp, int64_t n, int64_t chunk_max, int64_t max_entries) {
  std::vector<int64_t> cut{0};
  while (cut.back() < n) {
    const int64_t a = cut.back();
    int64_t b = std::min(n, a + chunk_max);
    while (b > a + 1 && hrp[b] - hrp[a] > max_entries) b = a + std::max<int64_t>(1, (b - a) / 2);
    cut.push_back(b);
  }
  return cut;
}

// fm_rank.hip: the distinct (context, item) pairs of a chunk's entries and each context's pairs in the total order, for fm_heldout.hip and
// fm_lists.hip.  The caller fills k_in / v_in and launches what differs (keys, scores, place, scatter) between the steps; the scratch is taken
// once per call for the largest chunk.
struct DistinctPairs {
  uint64_t *k_in = nullptr, *k_out = nullptr;  // sort keys in / out
  uint32_t *v_in = nullptr, *v_out = nullptr;  // sort values in / out
  uint64_t* dkey = nullptr;                    // [nd] the distinct keys (context << 32 | item), ascending
  uint32_t* e2d = nullptr;                     // [n] entry -> distinct pair
  int64_t* doff = nullptr;                     // [nc + 1] context c's distinct pairs are [doff[c], doff[c + 1])
  // scratch for chunks of up to max_entries entries of up to max_nc contexts, on stream st
  int reserve(Scratch& S, hipStream_t st, size_t max_entries, int64_t max_nc);
  // k_in[e] = context << 32 | item, v_in[e] = e for the chunk's n entries: dkey, e2d, doff and *nd (one read-back; none for n = 0, which
  // still writes doff)
  int distinct(int64_t n, int64_t nc, int64_t* nd);
  // k_in[d] = rank_order_key(score of distinct pair d), v_in[d] = d: v_out[t] = the pair at sorted slot t, each context's pairs in the total
  // order (stable: the input is item-ascending, so equal scores keep the lower item first)
  int order(int64_t nd, int64_t nc);

 private:
  hipStream_t st_ = nullptr;
  uint32_t *flag_ = nullptr, *pos_ = nullptr;
  void* temp_ = nullptr;
  size_t tmax_ = 0;
  int end_bit_ = 33;
};

}  // namespace fmx
