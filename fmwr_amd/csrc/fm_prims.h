// The sorts and scans of the query side ("shared ranking code"): fm_prims.hip is the one query-side file that includes
// rocprim, so its kernels are compiled once.  fm_rank.hip, fm_pairs.hip, fm_foldin.hip, fm_select.hip and fm_metrics.hip take them from here,
// and so does the next pipeline.  Every sort is a stable LSD radix sort over the low `bits` bits of the key.
//
// Two forms, one name.  The two-phase form mirrors rocprim's: temp == nullptr stores the size of the temporary storage in `bytes`, otherwise
// the call runs on stream st.  The convenience form takes the call's Scratch in place of (temp, bytes) and no stream: it sizes, draws the
// storage from the Scratch's one grow-only block and runs on the Scratch's stream.  n <= 0 is FMX_OK and launches nothing.
#pragma once
#include "fm_rank.h"

namespace fmx {

int sort_pairs(void* temp, size_t& bytes, uint64_t* k_in, uint64_t* k_out, uint32_t* v_in, uint32_t* v_out, int64_t n, int bits, hipStream_t st);
int sort_pairs(void* temp, size_t& bytes, uint32_t* k_in, uint32_t* k_out, uint32_t* v_in, uint32_t* v_out, int64_t n, int bits, hipStream_t st);
int sort_pairs(void* temp, size_t& bytes, const uint32_t* k_in, uint32_t* k_out, const int64_t* v_in, int64_t* v_out, int64_t n, int bits, hipStream_t st);
int sort_keys(void* temp, size_t& bytes, uint64_t* k_in, uint64_t* k_out, int64_t n, int bits, hipStream_t st);
// segment s is [off[s], off[s + 1]) of the n pairs; all 64 bits of the key
int seg_sort_pairs(void* temp, size_t& bytes, uint64_t* k_in, uint64_t* k_out, uint32_t* v_in, uint32_t* v_out, int64_t n, int64_t segments, int64_t* off,
                   hipStream_t st);
int exclusive_sum(void* temp, size_t& bytes, const uint32_t* in, uint32_t* out, int64_t n, hipStream_t st);
int exclusive_sum(void* temp, size_t& bytes, const int64_t* in, int64_t* out, int64_t n, hipStream_t st);
int exclusive_sum(void* temp, size_t& bytes, uint64_t* in, uint64_t* out, int64_t n, hipStream_t st);
int inclusive_sum(void* temp, size_t& bytes, uint32_t* in, uint32_t* out, int64_t n, hipStream_t st);
int inclusive_sum(void* temp, size_t& bytes, int64_t* in, int64_t* out, int64_t n, hipStream_t st);
int inclusive_max(void* temp, size_t& bytes, const uint32_t* in, uint32_t* out, int64_t n, hipStream_t st);

template <typename... A> int sort_pairs(Scratch& S, A... a) { return S.with_temp([&](void* t, size_t& b) { return sort_pairs(t, b, a..., S.st); }); }
template <typename... A> int sort_keys(Scratch& S, A... a) { return S.with_temp([&](void* t, size_t& b) { return sort_keys(t, b, a..., S.st); }); }
template <typename... A> int exclusive_sum(Scratch& S, A... a) { return S.with_temp([&](void* t, size_t& b) { return exclusive_sum(t, b, a..., S.st); }); }
template <typename... A> int inclusive_sum(Scratch& S, A... a) { return S.with_temp([&](void* t, size_t& b) { return inclusive_sum(t, b, a..., S.st); }); }
template <typename... A> int inclusive_max(Scratch& S, A... a) { return S.with_temp([&](void* t, size_t& b) { return inclusive_max(t, b, a..., S.st); }); }

// off[g] = the first position of the n ascending keys whose key is >= g, for g = 0 .. G
int group_offsets(const uint32_t* keys, int64_t n, int64_t G, int64_t* off, hipStream_t st);

// a host array on the device for the length of a call
template <typename T>
int upload(DevBuf* b, const T* host, int64_t count) {
  FMX_TRY(dev_buf(b, (size_t)count * sizeof(T)));
  if (count > 0) FMX_HIP(hipMemcpy(b->get(), host, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
  return FMX_OK;
}

// the bits of the keys 0 .. top, at least 1
inline int key_bits(uint64_t top) { return top == 0 ? 1 : 64 - __builtin_clzll((unsigned long long)top); }
// the bits in use of a (context << 32 | item) key for n_ctx contexts: 32 of the item, and the context's
inline int ctx_key_bits(int64_t n_ctx) { return std::min(64, 32 + key_bits(n_ctx > 1 ? (uint64_t)n_ctx - 1 : 0)); }

}  // namespace fmx
