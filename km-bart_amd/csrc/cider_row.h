// The row rule of the CIDEr reward (csrc/cider_reward.hip): which tokens of an id row are scored, how an n-gram becomes a 64-bit
// key and how a key is looked up in a sorted table.  src/rewards.py holds the same three rules on the host (reward_tokens,
// the key packing of build_cider_tables, its unsigned order).  DESIGN.md section 6r.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cider_reward.h"

namespace {

constexpr int kCiderWave = 64;

// The n tokens from tok[j] as one key: the first token in the highest of the n used 16-bit slots.  Tokens are < 65536 (the
// row load drops any other), so orders do not collide inside a key; every order has a key space of its own.
__device__ __forceinline__ uint64_t cider_key_pack(const int* tok, int j, int n) {
  uint64_t key = 0;
  for (int k = 0; k < n; ++k) key = (key << 16) | (uint64_t)(uint32_t)tok[j + k];
  return key;
}

// Index of `key` in keys[0 .. n) (ascending UNSIGNED, distinct), -1 when absent.  A lower-bound search: ceil(log2(n + 1))
// dependent loads and one more for the equality; nothing is read outside [0, n).
__device__ __forceinline__ int64_t cider_search(const uint64_t* __restrict__ keys, int64_t n, uint64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < n && keys[lo] == key) ? lo : -1;
}

// The token rule.  Of the row's L columns idr[0 .. L): column 0 (the decoder start token) is skipped, the row stops in front
// of the first `eos` behind it, every `pad` and `bos` is dropped, and so is a token outside [0, 65536) (never from generate();
// it has no key).  The kept tokens go to tok[] (LDS, KMB_CIDER_MAX_T ints) in order; returns their number.  Every thread of
// the workgroup calls this (barriers) with L <= THREADS: column `tid` is thread tid's.  scratch: 2 * THREADS / 64 LDS ints.
template <int THREADS>
__device__ __forceinline__ int cider_row_load(const int64_t* __restrict__ idr, int L, int pad, int bos, int eos, int* tok,
                                              int* scratch, int tid) {
  constexpr int WAVES = THREADS / kCiderWave;
  const int lane = tid & (kCiderWave - 1), wave = tid / kCiderWave;
  const int64_t v = tid < L ? idr[tid] : (int64_t)-1;
  const bool is_eos = tid >= 1 && tid < L && v == (int64_t)eos;
  const unsigned long long eos_mask = __ballot(is_eos);
  if (lane == 0) scratch[wave] = eos_mask ? wave * kCiderWave + (__ffsll((long long)eos_mask) - 1) : L;
  __syncthreads();
  int end = L;
  for (int w = 0; w < WAVES; ++w) end = min(end, scratch[w]);
  const bool keep = tid >= 1 && tid < end && v != (int64_t)pad && v != (int64_t)bos && v >= 0 && v < 65536;
  const unsigned long long keep_mask = __ballot(keep);
  if (lane == 0) scratch[WAVES + wave] = __popcll(keep_mask);
  __syncthreads();
  int before = 0, total = 0;
  for (int w = 0; w < WAVES; ++w) {
    const int c = scratch[WAVES + w];
    before += w < wave ? c : 0;
    total += c;
  }
  if (keep) tok[before + __popcll(keep_mask & ((1ull << lane) - 1ull))] = (int)v;
  __syncthreads();
  return total;
}

}  // namespace
