// The streaming log-sum-exp of an fp32 logits row by one 256-thread workgroup: shared by loss.hip's ce_kernel and beam_step.hip's
// logsoftmax_topk_kernel (the forms for rows too long to hold in registers).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  if (mn == -INFINITY) { m = mn; s = 0.f; return; }
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

// block-wide (max, sumexp) of row[0:V]; result broadcast to all threads
__device__ __forceinline__ void row_lse(const float* __restrict__ row, int V, float* sh, float& m_out, float& s_out) {
  const int tid = threadIdx.x;
  float m = -INFINITY, s = 0.f;
  const int V4 = V & ~3;
  for (int i = tid * 4; i < V4; i += 1024) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(row + i);
    const float mx = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    if (mx > m) { s *= __expf(m - mx); m = mx; }
    if (m != -INFINITY) s += __expf(x[0] - m) + __expf(x[1] - m) + __expf(x[2] - m) + __expf(x[3] - m);
  }
  for (int i = V4 + tid; i < V; i += 256) {
    const float x = row[i];
    if (x > m) { s *= __expf(m - x); m = x; }
    if (m != -INFINITY) s += __expf(x - m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    online_merge(m, s, m2, s2);
  }
  const int wave = tid >> 6;
  if ((tid & 63) == 0) { sh[wave * 2] = m; sh[wave * 2 + 1] = s; }
  __syncthreads();
  m = sh[0]; s = sh[1];
#pragma unroll
  for (int w = 1; w < 4; ++w) online_merge(m, s, sh[w * 2], sh[w * 2 + 1]);
  __syncthreads();
  m_out = m; s_out = s;
}

}  // namespace
