// Greedy tail of generate(num_beams=1, do_sample=False): transformers 3.0.2 _generate_no_beam_search as the reference runs it
// by default (vcg_generate.py --num_beams 1; the training callback's generate(), vcg_train.py:183-194), per row in one launch:
// EOS ban -> argmax -> log-probability of the chosen token -> finished-row bookkeeping [-> the next step's embedding].
// The log-probability sums are those of the reference's sample_sentence (src/model/utils.py:34-56).
//
// One workgroup of 1024 lanes per row, one streaming pass: every lane keeps a running (maximum, lowest index of that maximum,
// sum of exp(x - maximum)) over the columns it reads, the lanes are combined by a butterfly inside the wave and the waves
// through LDS, always by the rule (greater value, else equal value and smaller index).  The row is never held: any V >= 1.
// The order of every sum is fixed by the layout, no floating-point atomics: the same inputs give the same bits.
// DESIGN.md section 6g.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "embed_row.h"
#include "greedy.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;           // 16-byte loads a lane has in flight
constexpr int kNone = 0x7fffffff;

struct GreedyArgs {
  const float* logits; int ld, V, ban_token;
  int64_t* unfinished; int64_t pad_token, eos_token;
  int64_t* next_tokens; int64_t* ids; int t, ld_ids;
  int32_t* flag; float* logprob_sum; float* logprob_out;
  KmbEmbedNext en;
};

// running maximum m, the lowest index i that holds it (kNone: no finite entry yet), s = sum of exp(x - m) over the entries seen
struct Run { float m; int i; float s; };

__device__ __forceinline__ float clean(float x, int i, int ban) { return (x != x || i == ban) ? -INFINITY : x; }

// a lane meets its columns in ascending order, so a strictly greater value keeps the lowest index of a tie
__device__ __forceinline__ void take1(Run& a, float x, int i) {
  if (x > a.m) {
    a.s = a.s * __expf(a.m - x) + 1.f;   // m = -inf: s is 0 and stays 0
    a.m = x; a.i = i;
  } else if (a.m > -INFINITY) {
    a.s += __expf(x - a.m);
  }
}
__device__ __forceinline__ void take4(Run& a, const f32x4& v, int i0, int ban) {
  const float x0 = clean(v[0], i0, ban), x1 = clean(v[1], i0 + 1, ban), x2 = clean(v[2], i0 + 2, ban), x3 = clean(v[3], i0 + 3, ban);
  const float cm = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
  if (cm > a.m) {
    a.s *= __expf(a.m - cm);
    a.m = cm;
    a.i = i0 + (x0 == cm ? 0 : x1 == cm ? 1 : x2 == cm ? 2 : 3);
  }
  if (a.m > -INFINITY) a.s += (__expf(x0 - a.m) + __expf(x1 - a.m)) + (__expf(x2 - a.m) + __expf(x3 - a.m));
}
// symmetric in its arguments down to the bits (a + b == b + a): every lane of a butterfly ends with the same triple
__device__ __forceinline__ Run combine(const Run& a, const Run& b) {
  Run r;
  r.m = fmaxf(a.m, b.m);
  r.s = r.m > -INFINITY ? a.s * __expf(a.m - r.m) + b.s * __expf(b.m - r.m) : 0.f;
  r.i = (b.m > a.m || (b.m == a.m && b.i < a.i)) ? b.i : a.i;
  return r;
}
__device__ __forceinline__ Run shfl_xor(const Run& a, int o) {
  return Run{__shfl_xor(a.m, o, 64), __shfl_xor(a.i, o, 64), __shfl_xor(a.s, o, 64)};
}

template <int NCH>
__global__ __launch_bounds__(kThreads) void greedy_step_kernel(GreedyArgs a) {
  __shared__ float wm[kWaves], ws[kWaves];
  __shared__ int wi[kWaves];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* row = a.logits + (size_t)r * a.ld;
  Run run{-INFINITY, kNone, 0.f};
  if (((uintptr_t)row & 15) == 0) {
    // chunk c = columns 4c .. 4c + 3, lane tid reads chunks tid, tid + 1024, ...; the V % 4 last columns one lane each
    const int nvec = a.V >> 2;
    const f32x4* rv = reinterpret_cast<const f32x4*>(row);
    for (int c0 = tid; c0 < nvec; c0 += kThreads * kUnroll) {
      f32x4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = rv[min(c0 + u * kThreads, nvec - 1)];   // clamped: never past column V - 1
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * kThreads;
        if (c < nvec) take4(run, v[u], c * 4, a.ban_token);
      }
    }
    const int i = nvec * 4 + tid;
    if (i < a.V) take1(run, clean(row[i], i, a.ban_token), i);
  } else {
    // a row that does not start on 16 bytes (ld % 4 != 0): one column per load
    for (int i0 = tid; i0 < a.V; i0 += kThreads * kUnroll) {
      float v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = row[min(i0 + u * kThreads, a.V - 1)];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int i = i0 + u * kThreads;
        if (i < a.V) take1(run, clean(v[u], i, a.ban_token), i);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) run = combine(run, shfl_xor(run, o));
  if (lane == 0) { wm[w] = run.m; wi[w] = run.i; ws[w] = run.s; }
  __syncthreads();
  if (w != 0) return;
  run = lane < kWaves ? Run{wm[lane], wi[lane], ws[lane]} : Run{-INFINITY, kNone, 0.f};
#pragma unroll
  for (int o = kWaves / 2; o > 0; o >>= 1) run = combine(run, shfl_xor(run, o));
  int tok32 = 0;
  if (lane == 0) {
    // the chosen value is the maximum: x[token] - logsumexp(x) = -log(sum of exp(x - maximum))
    const bool any = run.i != kNone;
    float lp = any ? -logf(run.s) : -INFINITY;
    int64_t tok = any ? run.i : 0;
    bool live = true;
    if (a.unfinished) {
      int64_t u = a.unfinished[r];
      live = u != 0;
      if (!live) tok = a.pad_token;
      u = (live && tok != a.eos_token) ? 1 : 0;
      a.unfinished[r] = u;
      if (u && a.flag) atomicOr(a.flag, 1);
    } else if (a.flag) {
      atomicOr(a.flag, 1);
    }
    if (!live) lp = 0.f;
    a.next_tokens[r] = tok;
    if (a.ids) a.ids[(size_t)r * a.ld_ids + a.t] = tok;
    if (a.logprob_sum && live) a.logprob_sum[r] += lp;
    if (a.logprob_out) a.logprob_out[r] = lp;
    tok32 = (int)tok;
  }
  // the next decode step's input row, by this wave (beam_fold.h's beam_embed_next for a single row)
  if (a.en.E == nullptr) return;
  int tok = __shfl(tok32, 0, 64);
  tok = tok < 0 ? 0 : (tok >= a.en.V ? a.en.V - 1 : tok);   // never read outside the table
  embed_ln_row<NCH>(a.en.E + (size_t)tok * a.en.D, a.en.prow, a.en.scale, a.en.gamma, a.en.beta, nullptr, a.en.y, nullptr, nullptr, r,
                    a.en.D, a.en.eps, KmbDrop{0u, 0u, 1.f}, lane);
}

}  // namespace

hipError_t kmb_greedy_step_launch(const float* logits, int ld, int V, int R, int ban_token, int64_t* unfinished, int64_t pad_token,
                                  int64_t eos_token, int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag,
                                  float* logprob_sum, float* logprob_out, hipStream_t stream, const KmbEmbedNext* embed) {
  if (R <= 0) return hipSuccess;
  GreedyArgs a{logits, ld, V, ban_token, unfinished, pad_token, eos_token, next_tokens, ids, t, ld_ids, flag, logprob_sum, logprob_out,
               KmbEmbedNext{}};
  if (embed != nullptr && embed->E != nullptr) {
    if ((embed->D & 7) || embed->D < 8 || embed->D > 1024) return hipErrorNotSupported;
    a.en = *embed;
  }
  // the chunk count of kmb_embed_ln_fwd_launch for this width: the rows must come out with the same bits
  if (a.en.E != nullptr && a.en.D > 512)
    hipLaunchKernelGGL(greedy_step_kernel<2>, dim3(R), dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(greedy_step_kernel<1>, dim3(R), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}
