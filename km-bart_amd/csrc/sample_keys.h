// Rank keys of the sampling kernels (sample.hip, beam_sample.hip): order-preserving fp32 keys, the 48-bit (value, index) rank key,
// fixed-point softmax masses, and the workgroup scan of the radix selects.  1024-lane workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace {
// unsigned order of the key = order of the value (NaN is mapped to -inf and -0 to +0 before); key 0 marks a slot past V
__device__ __forceinline__ uint32_t order_key(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// rank key: larger = earlier in (value descending, index ascending)
__device__ __forceinline__ uint64_t rank_key(uint32_t k, int i) { return ((uint64_t)k << 16) | (uint32_t)(0xffff - i); }

// exp(x - max); 1 at the maximum itself, so a row whose maximum is +-inf still has finite masses
__device__ __forceinline__ float rel_exp(uint32_t k, float mx) {
  const float x = key_value(k);
  return x == mx ? 1.f : expf(x - mx);
}
__device__ __forceinline__ unsigned long long mass_fixed(uint32_t k, float mx) {
  return (unsigned long long)(rel_exp(k, mx) * 0x1p40f);
}

// exclusive prefix over the workgroup in thread order, and the totals
template <class Smem>
__device__ __forceinline__ void block_exscan(Smem& sh, uint32_t& c, unsigned long long& m, uint32_t& ctot, unsigned long long& mtot) {
  constexpr int kWaves = 16;   // 1024-lane workgroups
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t ci = c;
  unsigned long long mi = m;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t cu = __shfl_up(ci, o, 64);
    const unsigned long long mu = __shfl_up(mi, o, 64);
    if (lane >= o) { ci += cu; mi += mu; }
  }
  if (lane == 63) { sh.wc[w] = ci; sh.wm[w] = mi; }
  __syncthreads();
  // the 16 wave totals: exclusive prefix by the first 16 lanes (slot kWaves = grand total); a thread then reads two
  // values instead of holding all 16 pairs in registers next to the row
  if (threadIdx.x < kWaves) {
    const uint32_t c0 = sh.wc[lane];
    const unsigned long long m0 = sh.wm[lane];
    uint32_t cx = c0;
    unsigned long long mx = m0;
#pragma unroll
    for (int o = 1; o < kWaves; o <<= 1) {
      const uint32_t cu = __shfl_up(cx, o, 64);
      const unsigned long long mu = __shfl_up(mx, o, 64);
      if (lane >= o) { cx += cu; mx += mu; }
    }
    sh.wc_ex[lane] = cx - c0; sh.wm_ex[lane] = mx - m0;
    if (lane == kWaves - 1) { sh.wc_ex[kWaves] = cx; sh.wm_ex[kWaves] = mx; }
  }
  __syncthreads();
  const uint32_t cb = sh.wc_ex[w], ct = sh.wc_ex[kWaves];
  const unsigned long long mb = sh.wm_ex[w], mt = sh.wm_ex[kWaves];
  c = cb + ci - c; m = mb + mi - m; ctot = ct; mtot = mt;
}
}  // namespace
