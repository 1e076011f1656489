// Training and scoring losses over the tied vocabulary (reference src/model/model.py:397-403: CrossEntropyLoss(), mean over
// labels != -100): cross-entropy on fp32 and on bf16 logits, one workgroup per row (register-resident where the row fits; the
// 256-thread form reads its 197 KB row twice, the second pass from L2 / Infinity Cache), the row-sized pieces of the tied-head
// cross-entropy whose vocabulary-sized part runs in the head GEMM's epilogue, and the finish kernels of kmb_score.
// Generation's log_softmax + top-k and beam steps are in beam_step.hip.
#include "common.h"
#include "kernels.h"
#include "row_lse.h"

namespace {

// one workgroup of 1024 threads, eight independent loads in flight per thread (a 256-thread loop of dependent loads took
// 54 us for the 32768 labels of the benchmark batch)
// A label is VALID when 0 <= label < V; -100 is ignored (CrossEntropyLoss(ignore_index=-100), reference
// src/model/model.py:400-402); any other value is an input error the reference's loss raises on: such rows are treated as
// ignored by every cross-entropy kernel here, are NOT counted, and set bit 1 (value 2) of `status` (may be null) so that the
// host's input check reports them.
__global__ __launch_bounds__(1024) void count_valid_kernel(const int64_t* __restrict__ labels, int n, int V,
                                                           int32_t* __restrict__ count, int32_t* __restrict__ status) {
  __shared__ int sh[16];
  int c = 0, bad = 0;
  int i = threadIdx.x;
  for (; i + 7 * 1024 < n; i += 8 * 1024) {
    int64_t v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = labels[i + k * 1024];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const bool ok = v[k] >= 0 && v[k] < V;
      c += ok ? 1 : 0;
      bad |= (!ok && v[k] != -100) ? 1 : 0;
    }
  }
  for (; i < n; i += 1024) {
    const int64_t v = labels[i];
    const bool ok = v >= 0 && v < V;
    c += ok ? 1 : 0;
    bad |= (!ok && v != -100) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  if (bad && status != nullptr) atomicOr(status, 2);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sh[k];
    count[0] = t;
  }
}

// The denominator word of loss_reduction "sum": 1 with at least one valid label, 0 without (the kernels' n > 0 guards stay as they are)
__global__ void count_flag_kernel(const int32_t* __restrict__ count, int32_t* __restrict__ flag) {
  if (threadIdx.x == 0 && blockIdx.x == 0) flag[0] = count[0] > 0 ? 1 : 0;
}

// LS (label smoothing, eps > 0): the target is (1 - eps) onehot + eps / V over the V real columns, so
//   loss_r = lse - (1 - eps) v_label - eps mean_{j < V} v_j,   gradient row = (p - (1 - eps) onehot - eps / V) * scale / n, rounded once;
// pad columns and ignored rows stay exactly zero.  LS = false is the code it was (eps is not read).
// W (per-row loss weights): loss_r and the gradient row are multiplied by weights[r] -- ONE multiply of the row's
// loss and of the row's factor gs, so that a weight of 1.0f changes no bit; the weight is read only in rows with a valid label (an ignored
// row's weight may hold anything, NaN included) and is block-uniform like the label.  W = false is the code it was (weights is not read).
// `count` is the denominator word: the number of valid labels ("mean"), or kmb_count_flag_launch's 0 / 1 word ("sum").
template <bool LS, bool W>
__global__ __launch_bounds__(256) void ce_kernel(const float* __restrict__ logits, int ldv, int V,
                                                 const int64_t* __restrict__ labels, const int32_t* __restrict__ count,
                                                 float grad_scale, float* __restrict__ loss_rows,
                                                 bf16_t* __restrict__ dlogits, float eps,
                                                 const float* __restrict__ weights) {
  __shared__ float sh[8];
  __shared__ float shz[LS ? 4 : 1];
  const int r = blockIdx.x, tid = threadIdx.x;
  const float* row = logits + (size_t)r * ldv;
  const int64_t label = labels[r];
  const bool valid = label >= 0 && label < V;   // ignored: -100; out of range: flagged by count_valid
  float w = 1.f;
  if (W && valid) w = weights[r];   // issued in front of the row's loads, consumed behind them
  float m = 0.f, s = 1.f;
  if (valid) row_lse(row, V, sh, m, s);  // block-uniform branch
  const float lse = m + __logf(s);
  float zmean = 0.f;
  if (LS && valid) {   // block-uniform: the row's mean logit (a third read of the row, from L2 like the second)
    float z = 0.f;
    for (int i = tid; i < V; i += 256) z += row[i];
    z = wave_sum(z);
    if ((tid & 63) == 0) shz[tid >> 6] = z;
    __syncthreads();
    zmean = ((shz[0] + shz[1]) + (shz[2] + shz[3])) / (float)V;
  }
  if (LS) {
    if (tid == 0) {
      const float l = valid ? (lse - (1.f - eps) * row[label] - eps * zmean) : 0.f;
      loss_rows[r] = (W && valid) ? w * l : l;
    }
  } else {
    if (tid == 0) {
      const float l = valid ? (lse - row[label]) : 0.f;
      loss_rows[r] = (W && valid) ? w * l : l;
    }
  }
  if (dlogits == nullptr) return;
  const float uni = LS ? eps / (float)V : 0.f, hot = LS ? 1.f - eps : 1.f;
  bf16_t* drow = dlogits + (size_t)r * ldv;
  const int n = count[0];
  float gs = (valid && n > 0) ? grad_scale / (float)n : 0.f;
  if (W && valid) gs *= w;
  for (int i = tid * 8; i < ldv; i += 2048) {
    float o[8];
    if (valid) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = i + e;
        float p = 0.f;
        if (c < V) {
          p = __expf(row[c] - lse);
          if (LS) p -= uni;
          if (c == (int)label) p -= hot;
        }
        o[e] = p * gs;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = 0.f;
    }
    *reinterpret_cast<u32x4*>(drow + i) = pack8(o);
  }
}

// Register-resident form for rows of up to NV * 4096 columns: 1024 threads hold the whole fp32 row (NV float4 each),
// so the logits are read from memory once (max, sum-exp and the gradient all come from registers).
template <int NV, bool LS, bool W>
__global__ __launch_bounds__(1024) void ce_kernel_reg(const float* __restrict__ logits, int ldv, int V,
                                                      const int64_t* __restrict__ labels,
                                                      const int32_t* __restrict__ count, float grad_scale,
                                                      float* __restrict__ loss_rows, bf16_t* __restrict__ dlogits, float eps,
                                                      const float* __restrict__ weights) {
  __shared__ float sh[LS ? 48 : 32];
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* row = logits + (size_t)r * ldv;
  const int64_t label = labels[r];
  const bool valid = label >= 0 && label < V;  // block-uniform (ignored: -100; out of range: flagged by count_valid)
  typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
  if (!valid) {
    if (tid == 0) loss_rows[r] = 0.f;
    if (dlogits != nullptr) {
      const u32x2 zero = {0u, 0u};
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int i = (tid + 1024 * j) * 4;
        if (i < ldv) *reinterpret_cast<u32x2*>(dlogits + (size_t)r * ldv + i) = zero;
      }
    }
    return;
  }
  float w = 1.f;
  if (W) w = weights[r];   // valid rows only; block-uniform, issued with the label in front of the row's loads and consumed behind them
  f32x4 x[NV];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = (tid + 1024 * j) * 4;
    if (i < ldv) {
      x[j] = *reinterpret_cast<const f32x4*>(row + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i + e >= V) x[j][e] = -INFINITY;
        m = fmaxf(m, x[j][e]);
      }
    } else {
      x[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    }
  }
  m = wave_max(m);
  if (lane == 0) sh[wave] = m;
  __syncthreads();
  m = sh[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) m = fmaxf(m, sh[w]);
  float s = 0.f;
  if (m != -INFINITY) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += __expf(x[j][e] - m);
  }
  s = wave_sum(s);
  if (lane == 0) sh[16 + wave] = s;
  if (LS) {   // the row's mean logit over the V real columns, from the registers
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((tid + 1024 * j) * 4 + e < V) z += x[j][e];
    z = wave_sum(z);
    if (lane == 0) sh[32 + wave] = z;
  }
  __syncthreads();
  s = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) s += sh[16 + w];
  const float lse = m + __logf(s);
  float uni = 0.f, hot = 1.f;
  if (LS) {
    float z = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) z += sh[32 + w];
    uni = eps / (float)V; hot = 1.f - eps;
    if (tid == 0) {
      const float l = lse - hot * row[label] - eps * (z / (float)V);
      loss_rows[r] = W ? w * l : l;
    }
  } else {
    if (tid == 0) {
      const float l = lse - row[label];
      loss_rows[r] = W ? w * l : l;
    }
  }
  if (dlogits == nullptr) return;
  const int n = count[0];
  float gs = n > 0 ? grad_scale / (float)n : 0.f;
  if (W) gs *= w;
  bf16_t* drow = dlogits + (size_t)r * ldv;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = (tid + 1024 * j) * 4;
    if (i < ldv) {
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float p = __expf(x[j][e] - lse);  // exp(-inf) = 0 in the pad columns
        if (LS && i + e < V) p -= uni;    // (the pad columns stay exactly zero)
        if (i + e == (int)label) p -= hot;
        o[e] = p * gs;
      }
      const u32x2 pk = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
      *reinterpret_cast<u32x2*>(drow + i) = pk;
    }
  }
}

// SUM (loss_reduction "sum"): the rows' sum itself -- exactly 0 without a valid label, every row being 0 then; count is not read
template <bool SUM>
__global__ __launch_bounds__(1024) void loss_finish_kernel(const float* __restrict__ loss_rows, int rows,
                                                           const int32_t* __restrict__ count, float* __restrict__ loss) {
  __shared__ float sh[16];
  float a = 0.f;
  int i = threadIdx.x;
  for (; i + 7 * 1024 < rows; i += 8 * 1024) {   // eight independent loads in flight per thread
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = loss_rows[i + k * 1024];
    a += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  }
  for (; i < rows; i += 1024) a += loss_rows[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sh[k];
    if (SUM) {
      loss[0] = t;
    } else {
      const int n = count[0];
      // torch CrossEntropyLoss(mean) over zero valid targets is NaN
      loss[0] = n > 0 ? t / (float)n : __uint_as_float(0x7fc00000u);
    }
  }
}

// The training head keeps its logits in bf16 (the reference's AMP path holds them in fp16, src/training.py:118-134 with
// autocast; CE itself runs in fp32 on the up-cast values, as here): 1024 threads hold the row as NV8 chunks of 8 bf16
// (read once, 16-byte loads), max / sum-exp / loss in fp32 registers, and the gradient (softmax - onehot) * scale / count
// is written back IN PLACE over the logits (dlogits == logits is allowed: every element is read before the first
// store of its thread, and a thread only rewrites what it read).  Halves the head GEMM's store and the CE's read
// against fp32 logits: 3.3 GB -> 1.65 GB each per step at the benchmark batch.
template <int NV8, bool LS, bool W>
__global__ __launch_bounds__(1024) void ce_kernel_reg_bf16(const bf16_t* logits, int ldv, int V,
                                                           const int64_t* __restrict__ labels,
                                                           const int32_t* __restrict__ count, float grad_scale,
                                                           float* __restrict__ loss_rows, bf16_t* dlogits, float eps,
                                                           const float* __restrict__ weights) {
  __shared__ float sh[LS ? 56 : 33];
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bf16_t* row = logits + (size_t)r * ldv;
  const int64_t label = labels[r];
  const bool valid = label >= 0 && label < V;  // block-uniform (ignored: -100; out of range: flagged by count_valid)
  if (!valid) {
    if (tid == 0) loss_rows[r] = 0.f;
    if (dlogits != nullptr) {
      const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < NV8; ++j) {
        const int i = (tid + 1024 * j) * 8;
        if (i < ldv) *reinterpret_cast<u32x4*>(dlogits + (size_t)r * ldv + i) = zero;
      }
    }
    return;
  }
  float w = 1.f;
  if (W) w = weights[r];   // valid rows only; block-uniform, issued with the label in front of the row's loads and consumed behind them
  float x[NV8][8];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV8; ++j) {
    const int i = (tid + 1024 * j) * 8;
    if (i < ldv) {
      unpack8(*reinterpret_cast<const u32x4*>(row + i), x[j]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (i + e >= V) x[j][e] = -INFINITY;
        m = fmaxf(m, x[j][e]);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[j][e] = -INFINITY;
    }
  }
  m = wave_max(m);
  if (lane == 0) sh[wave] = m;
  __syncthreads();
  m = sh[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) m = fmaxf(m, sh[w]);
  float s = 0.f;
  if (m != -INFINITY) {
#pragma unroll
    for (int j = 0; j < NV8; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s += __expf(x[j][e] - m);
        // the label's logit comes from the registers of the one thread that holds it (the row may be overwritten below)
        if ((tid + 1024 * j) * 8 + e == (int)label) sh[32] = x[j][e];
      }
  }
  s = wave_sum(s);
  if (lane == 0) sh[16 + wave] = s;
  if (LS) {   // the row's mean logit over the V real columns, from the registers
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < NV8; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if ((tid + 1024 * j) * 8 + e < V) z += x[j][e];
    z = wave_sum(z);
    if (lane == 0) sh[40 + wave] = z;
  }
  __syncthreads();
  s = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) s += sh[16 + w];
  const float lse = m + __logf(s);
  float uni = 0.f, hot = 1.f;
  if (LS) {
    float z = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) z += sh[40 + w];
    uni = eps / (float)V; hot = 1.f - eps;
    if (tid == 0) {
      const float l = lse - hot * sh[32] - eps * (z / (float)V);
      loss_rows[r] = W ? w * l : l;
    }
  } else {
    if (tid == 0) {
      const float l = lse - sh[32];
      loss_rows[r] = W ? w * l : l;
    }
  }
  if (dlogits == nullptr) return;
  const int n = count[0];
  float gs = n > 0 ? grad_scale / (float)n : 0.f;
  if (W) gs *= w;
  bf16_t* drow = dlogits + (size_t)r * ldv;
#pragma unroll
  for (int j = 0; j < NV8; ++j) {
    const int i = (tid + 1024 * j) * 8;
    if (i < ldv) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float p = __expf(x[j][e] - lse);  // exp(-inf) = 0 in the pad columns
        if (LS && i + e < V) p -= uni;    // (the pad columns stay exactly zero)
        if (i + e == (int)label) p -= hot;
        o[e] = p * gs;
      }
      *reinterpret_cast<u32x4*>(drow + i) = pack8(o);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Tied-head cross-entropy WITHOUT a pass over the logits (round 3).  Reference src/model/model.py:397-402:
//   loss = mean over valid rows of  lse(v_r) - v_r[label_r],   v_r = h_r E^T + b.
// The head GEMM (KmbGemm act 5) stores  P[r][j] = exp(v_rj - c_r)  in bf16 with c_r = the label's logit, so that
// P[r][label] = 1 exactly; a logit more than 80 above the label's (a row whose loss exceeds 80 nats) saturates at 2^115
// instead of overflowing (the epilogue clamps the exponent), ignored rows store zeros (their shift is +1e30); the GEMM
// leaves the fp32 row sums S_r = sum_j P[r][j] (per 64-column block) and d_r = v_r[label] - c_r.  Then
//   loss_r = log S_r - d_r,      softmax_rj = P[r][j] / S_r,
//   dlogits_rj = g (P[r][j] / S_r - [j == label_r]),          g = lm_factor / (number of valid rows)
// is never materialised: the row finish replaces the label's entry by P'[r][label_r] = P[r][label_r] - S_r (one bf16
// element per row: the difference rounded once, the relative error the two-kernel path's bf16 gradient row has there), and
// with a_r = g / S_r
//   dH_r  = a_r * sum_j P'[r][j] E_j            (the data-gradient GEMM runs on P', its slab finish applies a_r)
//   dE    = P'^T (a . H)                        (the weight-gradient GEMM runs on P' and the row-scaled copy a . H)
// so the 2 x 3.3 GB read-modify-write of ce_kernel_reg_bf16 (1.76 ms of a b = 1024 step) disappears; P is stored at
// 8 significant bits relative to the probability itself (the two-kernel path rounds the LOGIT to 8 bits: 3-6 % on p).
// (A first version kept P intact and corrected both products afterwards -- S_r E[label_r] in the finish and an atomic
// scatter of S_r (a . H)_r into dE: 115 us of fp32 atomics per b = 1024 step for the same precision.)

// c_r = h_r . E[label_r] + bias[label_r]; ignored / out-of-range rows get c_r = +1e30, so that their stored row is
// exp(v - 1e30) = 0 and their sum 0 whatever the logits are (nothing downstream has to rely on a zero factor); one wave per row
__global__ __launch_bounds__(256) void ce_label_logit_kernel(const bf16_t* __restrict__ H, int ldh, const bf16_t* __restrict__ E,
                                                             int lde, const float* __restrict__ bias,
                                                             const int64_t* __restrict__ labels, int rows, int d, int V,
                                                             float* __restrict__ shift) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const long long lab = labels[r];
  if (lab < 0 || lab >= V) {
    if (lane == 0) shift[r] = 1e30f;
    return;
  }
  const bf16_t* h = H + (size_t)r * ldh;
  const bf16_t* e = E + (size_t)lab * lde;
  float acc = 0.f;
  for (int i = lane * 8; i < d; i += 512) {
    float a[8], b[8];
    unpack8(*reinterpret_cast<const u32x4*>(h + i), a);
    unpack8(*reinterpret_cast<const u32x4*>(e + i), b);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = fmaf(a[k], b[k], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) shift[r] = acc + bias[lab];
}

// bias_pad[0, V) = bias, bias_pad[V, Vpad) = -1e30 (exp -> 0: the padded vocabulary columns contribute nothing)
__global__ __launch_bounds__(256) void ce_pad_bias_kernel(const float* __restrict__ bias, int V, int Vpad, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < Vpad) out[i] = i < V ? bias[i] : -1e30f;
}

// per row: S_r, loss_r, a_r, the row-scaled copy a . H (bf16), and the label's entry of the stored matrix turned into
// P[r, label_r] - S_r (so that a_r P'[r, :] IS the softmax gradient row and both gradient GEMMs need no correction term;
// the entry is exp(pick_r) ~ 1 against S_r >= 1: one bf16 rounding of the difference, the same relative error the bf16
// gradient row of the two-kernel path carries at the label); one wave per row
// W: weights[r] (read in valid rows only) multiplies loss_r and a_r once; S_r and the label's entry of P' are weight-free
template <bool W>
__global__ __launch_bounds__(256) void ce_rows_finish_kernel(const float* __restrict__ row_sums, int ld_sums, int nparts,
                                                             const float* __restrict__ pick, const int64_t* __restrict__ labels,
                                                             const int32_t* __restrict__ count, float lm_factor, int rows, int d, int V,
                                                             const bf16_t* __restrict__ H, int ldh, float* __restrict__ loss_rows,
                                                             float* __restrict__ srow, float* __restrict__ alpha,
                                                             bf16_t* __restrict__ ah, bf16_t* __restrict__ P, int ldp,
                                                             const float* __restrict__ weights) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const long long lab = labels[r];
  const bool valid = lab != -100 && lab >= 0 && lab < V;
  float w = 1.f;
  if (W && valid) w = weights[r];
  float s = 0.f;
  for (int i = lane; i < nparts; i += 64) s += row_sums[(size_t)r * ld_sums + i];
  s = wave_sum(s);
  const int n = count[0];
  float a = (valid && n > 0 && s > 0.f) ? lm_factor / ((float)n * s) : 0.f;
  if (W && valid) a *= w;
  if (lane == 0) {
    const float pk = pick != nullptr ? pick[r] : 0.f;   // v_r[label] - c_r: 0 up to summation order when c_r is the label's logit
    const float l = valid ? __logf(s) - pk : 0.f;
    loss_rows[r] = (W && valid) ? w * l : l;
    srow[r] = valid ? s : 0.f;
    alpha[r] = a;
    if (valid && P != nullptr) P[(size_t)r * ldp + lab] = f2bf(__expf(pk) - s);
  }
  if (ah != nullptr) {
    for (int i = lane * 8; i < d; i += 512) {
      float x[8];
      unpack8(*reinterpret_cast<const u32x4*>(H + (size_t)r * ldh + i), x);
#pragma unroll
      for (int k = 0; k < 8; ++k) x[k] *= a;
      *reinterpret_cast<u32x4*>(ah + (size_t)r * d + i) = pack8(x);
    }
  }
}

// dH_r = a_r * sum_s slab[s][r]  (the label's correction is inside the matrix the GEMM multiplied);  8 columns per thread
__global__ __launch_bounds__(256) void ce_dgrad_finish_kernel(const float* __restrict__ slab, int nslabs, size_t stride,
                                                              const float* __restrict__ alpha, bf16_t* __restrict__ out, int rows, int d) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;   // chunk of 8 columns
  const int per_row = d >> 3;
  const int r = (int)(idx / per_row);
  if (r >= rows) return;
  const int c = (int)(idx - (size_t)r * per_row) * 8;
  const float a = alpha[r];
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (a != 0.f) {
    const float* src = slab + (size_t)r * d + c;
    f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 4);
    add_slabs2<4>(lo, hi, src, stride, nslabs);
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] *= a;
  }
  *reinterpret_cast<u32x4*>(out + (size_t)r * d + c) = pack8(v);
}

// ------------------------------------------------------------------------------------------------------------------
// Label smoothing as rank-one terms (kmb_set_label_smoothing).  The target row is (1 - eps) onehot + eps / V over
// the V real columns.  With the tied head v_r = h_r E^T + b every smoothing term is rank one:
//   wsum = sum_{j < V} E_j,  bsum = sum_{j < V} b_j,     zbar_r = mean_{j < V} v_rj = (h_r . wsum + bsum) / V       (no sum over the row)
//   loss_r = log S_r - pick_r + eps (c_r - zbar_r)       (c_r: the row shift = the label's logit, S_r: the act 5 epilogue's row sum)
//   dlogits_rj = g (softmax_rj - (1 - eps) [j == label_r] - eps / V),   g = lm_factor / n
// The label's entry of the stored matrix becomes P'[r][label_r] = bf16(exp(pick_r) - (1 - eps) S_r) -- a_r P' then carries the softmax and
// the onehot part -- and the uniform part never touches the matrix: with beta_r = eps g / V on valid rows (0 elsewhere)
//   dH_r -= beta_r wsum      (the data-gradient finish, before its one bf16 rounding)
//   dE_j -= u for j < V,     u = sum_r beta_r h_r      (the weight-gradient launch's bias operand, or its slab reduction's row vector)
// Both d-wide sums are deterministic: a fixed grid leaves per-workgroup partial rows, kmb_reduce_parts_launch sums them in slot order.

// wsum | bsum: workgroup w sums rows [w * rpw, (w + 1) * rpw) of E and of the bias.  A row is d / 8 16-byte chunks; the 256 threads are
// CW = min(d / 8, 256) column lanes x 256 / CW row lanes (d = 768: 96 x 2), four rows in flight per thread; the row lanes meet in LDS.
constexpr int VS_MAX_SLOTS = 512;
__global__ __launch_bounds__(256) void ce_vocab_sum_kernel(const bf16_t* __restrict__ E, int lde, const float* __restrict__ bias, int V, int d,
                                                           int rpw, int ldp, float* __restrict__ partials) {
  extern __shared__ float vs_red[];   // [256 / CW][8 * CW]
  const int nch = d >> 3, cw = nch < 256 ? nch : 256, rl = 256 / cw;
  const int tid = threadIdx.x, cl = tid % cw, rlane = tid / cw;
  const int r0 = blockIdx.x * rpw, r1 = (r0 + rpw) < V ? (r0 + rpw) : V;
  float* out = partials + (size_t)blockIdx.x * ldp;
  for (int c0 = 0; c0 < nch; c0 += cw) {   // one trip unless d > 2048
    const int ch = c0 + cl;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (rlane < rl && ch < nch) {
      const bf16_t* col = E + (size_t)ch * 8;
      int r = r0 + rlane;
      for (; r + 3 * rl < r1; r += 4 * rl) {
        u32x4 q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = *reinterpret_cast<const u32x4*>(col + (size_t)(r + k * rl) * lde);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float x[8];
          unpack8(q[k], x);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += x[e];
        }
      }
      for (; r < r1; r += rl) {
        float x[8];
        unpack8(*reinterpret_cast<const u32x4*>(col + (size_t)r * lde), x);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] += x[e];
      }
    }
    __syncthreads();   // (the previous trip's readers are done)
    if (rlane < rl) {
#pragma unroll
      for (int e = 0; e < 8; ++e) vs_red[(size_t)rlane * 8 * cw + cl * 8 + e] = acc[e];
    }
    __syncthreads();
    for (int i = tid; i < 8 * cw; i += 256) {
      const int col = c0 * 8 + i;
      if (col < d) {
        float t = 0.f;
        for (int k = 0; k < rl; ++k) t += vs_red[(size_t)k * 8 * cw + i];
        out[col] = t;
      }
    }
  }
  // the bias of the same rows: wave 0, lane-strided, butterfly
  if (tid < 64) {
    float b = 0.f;
    for (int r = r0 + tid; r < r1; r += 64) b += bias[r];
    b = wave_sum(b);
    if (tid == 0) out[d] = b;
  }
}

// ce_rows_finish_kernel with smoothing.  One wave per row, four rows per trip, a fixed grid (kmb_ce_rows_slots) walking the rows with its
// stride; each wave keeps sum -beta_r h_r of its rows in its own LDS row, the four meet at the end: u_part[workgroup][d].
// W: as in ce_rows_finish_kernel, and beta_r carries the weight too (so u = sum_r beta_r h_r does)
template <bool W>
__global__ __launch_bounds__(256) void ce_rows_finish_ls_kernel(const float* __restrict__ row_sums, int ld_sums, int nparts,
                                                                const float* __restrict__ pick, const float* __restrict__ shift,
                                                                const int64_t* __restrict__ labels, const int32_t* __restrict__ count,
                                                                float lm_factor, float eps, int rows, int d, int V,
                                                                const bf16_t* __restrict__ H, int ldh, const float* __restrict__ wsum,
                                                                float* __restrict__ loss_rows, float* __restrict__ srow,
                                                                float* __restrict__ alpha, float* __restrict__ beta, bf16_t* __restrict__ ah,
                                                                bf16_t* __restrict__ P, int ldp, float* __restrict__ u_part,
                                                                const float* __restrict__ weights) {
  extern __shared__ float ls_acc[];   // [4][d]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* acc = ls_acc + (size_t)wave * d;
  if (u_part != nullptr)
    for (int i = lane; i < d; i += 64) acc[i] = 0.f;
  __syncthreads();   // (below, element lane * 8 + k + 512 t of the wave's row belongs to that one lane in every trip)
  const int n = count[0];
  const float bsum = wsum[d], invV = 1.f / (float)V;
  for (int r = blockIdx.x * 4 + wave; r < rows; r += gridDim.x * 4) {
    const long long lab = labels[r];
    const bool valid = lab != -100 && lab >= 0 && lab < V;
    float w = 1.f;
    if (W && valid) w = weights[r];
    float s = 0.f;
    for (int i = lane; i < nparts; i += 64) s += row_sums[(size_t)r * ld_sums + i];
    s = wave_sum(s);
    float a = (valid && n > 0 && s > 0.f) ? lm_factor / ((float)n * s) : 0.f;
    float b = (valid && n > 0) ? eps * lm_factor / ((float)n * (float)V) : 0.f;
    if (W && valid) { a *= w; b *= w; }
    float dot = 0.f;
    for (int i = lane * 8; i < d; i += 512) {
      float x[8];
      unpack8(*reinterpret_cast<const u32x4*>(H + (size_t)r * ldh + i), x);
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(wsum + i), w1 = *reinterpret_cast<const f32x4*>(wsum + i + 4);
      const float w[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
#pragma unroll
      for (int k = 0; k < 8; ++k) dot = fmaf(x[k], w[k], dot);
      if (u_part != nullptr && b != 0.f) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[i + k] -= b * x[k];
      }
      if (ah != nullptr) {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] *= a;
        *reinterpret_cast<u32x4*>(ah + (size_t)r * d + i) = pack8(x);
      }
    }
    dot = wave_sum(dot);
    if (lane == 0) {
      const float pk = pick != nullptr ? pick[r] : 0.f;
      const float zbar = (dot + bsum) * invV;
      const float l = valid ? __logf(s) - pk + eps * (shift[r] - zbar) : 0.f;
      loss_rows[r] = (W && valid) ? w * l : l;
      srow[r] = valid ? s : 0.f;
      alpha[r] = a;
      beta[r] = b;
      if (valid && P != nullptr) P[(size_t)r * ldp + lab] = f2bf(__expf(pk) - (1.f - eps) * s);
    }
  }
  if (u_part == nullptr) return;
  __syncthreads();
  for (int i = threadIdx.x; i < d; i += 256)
    u_part[(size_t)blockIdx.x * d + i] = ((ls_acc[i] + ls_acc[d + i]) + ls_acc[2 * d + i]) + ls_acc[3 * d + i];
}

// ce_dgrad_finish_kernel with the vector term: dH_r = a_r * sum_s slab[s][r] - beta_r * wsum, one rounding
__global__ __launch_bounds__(256) void ce_dgrad_finish_ls_kernel(const float* __restrict__ slab, int nslabs, size_t stride,
                                                                 const float* __restrict__ alpha, const float* __restrict__ beta,
                                                                 const float* __restrict__ wsum, bf16_t* __restrict__ out, int rows, int d) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;   // chunk of 8 columns
  const int per_row = d >> 3;
  const int r = (int)(idx / per_row);
  if (r >= rows) return;
  const int c = (int)(idx - (size_t)r * per_row) * 8;
  const float a = alpha[r], b = beta[r];
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (a != 0.f) {
    const float* src = slab + (size_t)r * d + c;
    f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 4);
    add_slabs2<4>(lo, hi, src, stride, nslabs);
    v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] *= a;
  }
  if (b != 0.f) {
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(wsum + c), w1 = *reinterpret_cast<const f32x4*>(wsum + c + 4);
    const float w[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] -= b * w[k];
  }
  *reinterpret_cast<u32x4*>(out + (size_t)r * d + c) = pack8(v);
}


// ------------------------------------------------------------------------------------------------------------------
// Scoring a given target sequence (kmb_score; reference scripts/filter_reason.py:24-52: log_softmax over the [B, T, V] logits,
// the label's entry token by token, the mean over labels >= 0 per sample).  The head GEMM's scoring class (gemm_lean.hip
// LN_SCORE) leaves per row and 64-column block (maximum, sum of exp(v - maximum)); this is the row finish:
//   logp_r = v_r[label_r] - lse_r,   lse_r = M + log sum_b s_b exp(m_b - M),  M = max_b m_b
// with the label's logit from ce_label_logit_kernel.  Rows whose label is -100 or out of range get 0.  One wave per row; the
// blocks are walked lane-strided and folded by a butterfly: a fixed order, no atomics.
__global__ __launch_bounds__(256) void score_rows_finish_kernel(const float* __restrict__ stats, int nblk, const float* __restrict__ label_logit,
                                                                const int64_t* __restrict__ labels, int rows, int V, float* __restrict__ logp) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const long long lab = labels[r];
  if (lab < 0 || lab >= V) {
    if (lane == 0) logp[r] = 0.f;
    return;
  }
  const kmb_f32x2* st = reinterpret_cast<const kmb_f32x2*>(stats) + (size_t)r * nblk;
  float m = -INFINITY;
  for (int i = lane; i < nblk; i += 64) m = fmaxf(m, st[i][0]);
  m = wave_max(m);
  float s = 0.f;
  for (int i = lane; i < nblk; i += 64) {
    const kmb_f32x2 b = st[i];
    s += b[1] * expf(b[0] - m);
  }
  s = wave_sum(s);
  if (lane == 0) logp[r] = label_logit[r] - (m + logf(s));
}

// Per batch item: nll[b] = sum over its T rows, in row order, of -logp of the rows with a valid label, count[b] = their number.
// src_is_nll: src holds the rows' losses (loss_rows of ce_kernel_reg / ce_kernel_reg_bf16, the fallback head paths) instead of
// log-probabilities; either way logp_out (may alias src) receives the log-probabilities, 0 in ignored rows.  One thread per item.
__global__ __launch_bounds__(256) void score_segments_kernel(const float* src, int src_is_nll, const int64_t* __restrict__ labels, int B, int T,
                                                             int V, float* logp_out, float* __restrict__ nll, int32_t* __restrict__ count) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float a = 0.f;
  int n = 0;
  for (int t = 0; t < T; ++t) {
    const size_t r = (size_t)b * T + t;
    const long long lab = labels[r];
    const bool valid = lab >= 0 && lab < V;
    const float x = src[r];
    const float lp = valid ? (src_is_nll ? -x : x) : 0.f;
    logp_out[r] = lp;
    if (valid) { a -= lp; ++n; }
  }
  nll[b] = a;
  count[b] = n;
}

}  // namespace

hipError_t kmb_ce_label_logit_launch(const bf16_t* H, int ldh, const bf16_t* E, int lde, const float* bias, const int64_t* labels,
                                     int rows, int d, int V, float* shift, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if ((d & 7) || (ldh & 7) || (lde & 7)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ce_label_logit_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, H, ldh, E, lde, bias, labels, rows, d, V, shift);
  return hipGetLastError();
}
hipError_t kmb_ce_pad_bias_launch(const float* bias, int V, int Vpad, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(ce_pad_bias_kernel, dim3((Vpad + 255) / 256), dim3(256), 0, stream, bias, V, Vpad, out);
  return hipGetLastError();
}
hipError_t kmb_ce_rows_finish_launch(const float* row_sums, int ld_sums, int nparts, const float* pick, const int64_t* labels,
                                     const int32_t* count, float lm_factor, int rows, int d, int V, const bf16_t* H, int ldh,
                                     float* loss_rows, float* srow, float* alpha, bf16_t* ah, bf16_t* P, int ldp, hipStream_t stream,
                                     const float* weights) {
  if (rows <= 0) return hipSuccess;
  if ((d & 7) || (ldh & 7)) return hipErrorInvalidValue;
  if (weights != nullptr)
    hipLaunchKernelGGL(ce_rows_finish_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, stream, row_sums, ld_sums, nparts, pick, labels, count,
                       lm_factor, rows, d, V, H, ldh, loss_rows, srow, alpha, ah, P, ldp, weights);
  else
    hipLaunchKernelGGL(ce_rows_finish_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, stream, row_sums, ld_sums, nparts, pick, labels, count,
                       lm_factor, rows, d, V, H, ldh, loss_rows, srow, alpha, ah, P, ldp, nullptr);
  return hipGetLastError();
}
hipError_t kmb_ce_dgrad_finish_launch(const float* slab, int nslabs, size_t stride, const float* alpha, bf16_t* out, int rows, int d,
                                      hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if ((d & 7) || (stride & 3)) return hipErrorInvalidValue;
  const size_t chunks = (size_t)rows * (d >> 3);
  hipLaunchKernelGGL(ce_dgrad_finish_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, slab, nslabs, stride, alpha,
                     out, rows, d);
  return hipGetLastError();
}

int kmb_ce_vocab_sum_ld(int d) { return d + 8; }
int kmb_ce_vocab_sum_slots(int V, int d) {
  // >= 32 rows per row lane and workgroup (eight trips of four rows in flight), at most VS_MAX_SLOTS workgroups: 50320 x 768 -> 512 slots of 99 rows
  const int nch = d >> 3, cw = nch < 256 ? nch : 256, rl = cw > 0 ? 256 / cw : 1;
  int slots = (V + 32 * rl - 1) / (32 * rl);
  if (slots > VS_MAX_SLOTS) slots = VS_MAX_SLOTS;
  return slots < 1 ? 1 : slots;
}
hipError_t kmb_ce_vocab_sum_launch(const bf16_t* E, int lde, const float* bias, int V, int d, float* partials, float* wsum, hipStream_t stream) {
  if (V <= 0 || d <= 0 || (d & 7) || (lde & 7) || lde < d || ((uintptr_t)E & 15) || ((uintptr_t)wsum & 15)) return hipErrorInvalidValue;
  const int slots = kmb_ce_vocab_sum_slots(V, d), ld = kmb_ce_vocab_sum_ld(d);
  const int rpw = (V + slots - 1) / slots;
  const int nch = d >> 3, cw = nch < 256 ? nch : 256, rl = 256 / cw;
  hipLaunchKernelGGL(ce_vocab_sum_kernel, dim3(slots), dim3(256), (size_t)rl * 8 * cw * sizeof(float), stream, E, lde, bias, V, d, rpw, ld, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return kmb_reduce_parts_launch(partials, slots, ld, wsum, d + 1, stream);
}
int kmb_ce_rows_slots(int rows) {
  const int wgs = (rows + 3) / 4;
  return wgs < 1024 ? (wgs < 1 ? 1 : wgs) : 1024;   // 1024 workgroups: eight rows per wave at the benchmark batch, 3 MB of partial rows at d = 768
}
hipError_t kmb_ce_rows_finish_ls_launch(const float* row_sums, int ld_sums, int nparts, const float* pick, const float* shift,
                                        const int64_t* labels, const int32_t* count, float lm_factor, float eps, int rows, int d, int V,
                                        const bf16_t* H, int ldh, const float* wsum, float* loss_rows, float* srow, float* alpha, float* beta,
                                        bf16_t* ah, bf16_t* P, int ldp, float* u_partials, float* neg_u, hipStream_t stream,
                                        const float* weights) {
  if (rows <= 0) return hipSuccess;
  if (d <= 0 || (d & 7) || (ldh & 7) || d > 4096 || ((uintptr_t)wsum & 15) || (u_partials == nullptr) != (neg_u == nullptr)) return hipErrorInvalidValue;
  const int slots = kmb_ce_rows_slots(rows);
  if (weights != nullptr)
    hipLaunchKernelGGL(ce_rows_finish_ls_kernel<true>, dim3(slots), dim3(256), (size_t)4 * d * sizeof(float), stream, row_sums, ld_sums, nparts, pick,
                       shift, labels, count, lm_factor, eps, rows, d, V, H, ldh, wsum, loss_rows, srow, alpha, beta, ah, P, ldp, u_partials, weights);
  else
    hipLaunchKernelGGL(ce_rows_finish_ls_kernel<false>, dim3(slots), dim3(256), (size_t)4 * d * sizeof(float), stream, row_sums, ld_sums, nparts, pick,
                       shift, labels, count, lm_factor, eps, rows, d, V, H, ldh, wsum, loss_rows, srow, alpha, beta, ah, P, ldp, u_partials, nullptr);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || neg_u == nullptr) return e;
  return kmb_reduce_parts_launch(u_partials, slots, d, neg_u, d, stream);
}
hipError_t kmb_ce_dgrad_finish_ls_launch(const float* slab, int nslabs, size_t stride, const float* alpha, const float* beta,
                                         const float* wsum, bf16_t* out, int rows, int d, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if ((d & 7) || (stride & 3) || ((uintptr_t)wsum & 15)) return hipErrorInvalidValue;
  const size_t chunks = (size_t)rows * (d >> 3);
  hipLaunchKernelGGL(ce_dgrad_finish_ls_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, stream, slab, nslabs, stride, alpha,
                     beta, wsum, out, rows, d);
  return hipGetLastError();
}

hipError_t kmb_score_rows_finish_launch(const float* stats, int nblk, const float* label_logit, const int64_t* labels, int rows, int V,
                                        float* logp, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (nblk <= 0 || ((uintptr_t)stats & 7)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(score_rows_finish_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, stats, nblk, label_logit, labels, rows, V, logp);
  return hipGetLastError();
}
hipError_t kmb_score_segments_launch(const float* src, int src_is_nll, const int64_t* labels, int B, int T, int V, float* logp_out,
                                     float* nll, int32_t* count, hipStream_t stream) {
  if (B <= 0 || T <= 0) return hipSuccess;
  hipLaunchKernelGGL(score_segments_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, src, src_is_nll, labels, B, T, V, logp_out, nll, count);
  return hipGetLastError();
}

hipError_t kmb_count_valid_launch(const int64_t* labels, int n, int V, int32_t* count, int32_t* status, hipStream_t stream) {
  hipLaunchKernelGGL(count_valid_kernel, dim3(1), dim3(1024), 0, stream, labels, n, V, count, status);
  return hipGetLastError();
}

hipError_t kmb_count_flag_launch(const int32_t* count, int32_t* flag, hipStream_t stream) {
  hipLaunchKernelGGL(count_flag_kernel, dim3(1), dim3(64), 0, stream, count, flag);
  return hipGetLastError();
}

namespace {
// one launch line per row kernel: the weighted instance with weights, the instance there always was without
template <bool LS, bool W>
void ce_f32_pick(const float* logits, int ldv, int V, const int64_t* labels, int rows, const int32_t* count, float grad_scale,
                 float* loss_rows, bf16_t* dlogits, hipStream_t stream, float eps, const float* weights) {
  if (ldv <= 13 * 4096)
    hipLaunchKernelGGL((ce_kernel_reg<13, LS, W>), dim3(rows), dim3(1024), 0, stream, logits, ldv, V, labels, count, grad_scale, loss_rows, dlogits, eps, weights);
  else
    hipLaunchKernelGGL((ce_kernel<LS, W>), dim3(rows), dim3(256), 0, stream, logits, ldv, V, labels, count, grad_scale, loss_rows, dlogits, eps, weights);
}
template <bool LS, bool W>
void ce_bf16_pick(const bf16_t* logits, int ldv, int V, const int64_t* labels, int rows, const int32_t* count, float grad_scale,
                  float* loss_rows, bf16_t* dlogits, hipStream_t stream, float eps, const float* weights) {
  if (ldv <= 7 * 8192)
    hipLaunchKernelGGL((ce_kernel_reg_bf16<7, LS, W>), dim3(rows), dim3(1024), 0, stream, logits, ldv, V, labels, count, grad_scale, loss_rows, dlogits, eps, weights);
  else
    hipLaunchKernelGGL((ce_kernel_reg_bf16<8, LS, W>), dim3(rows), dim3(1024), 0, stream, logits, ldv, V, labels, count, grad_scale, loss_rows, dlogits, eps, weights);
}
}  // namespace

hipError_t kmb_ce_launch(const float* logits, int ldv, int V, const int64_t* labels, int rows, const int32_t* count,
                         float grad_scale, float* loss_rows, bf16_t* dlogits, hipStream_t stream, float eps, const float* weights) {
  if (rows <= 0) return hipSuccess;
  if ((ldv & 7) || ((uintptr_t)logits & 15) || !(eps >= 0.f && eps < 1.f)) return hipErrorInvalidValue;
  if (weights != nullptr) {
    if (eps > 0.f) ce_f32_pick<true, true>(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, stream, eps, weights);
    else ce_f32_pick<false, true>(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, stream, 0.f, weights);
  } else if (eps > 0.f) {
    ce_f32_pick<true, false>(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, stream, eps, nullptr);
  } else {
    ce_f32_pick<false, false>(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, stream, 0.f, nullptr);
  }
  return hipGetLastError();
}

hipError_t kmb_ce_bf16_launch(const bf16_t* logits, int ldv, int V, const int64_t* labels, int rows, const int32_t* count,
                              float grad_scale, float* loss_rows, bf16_t* dlogits, hipStream_t stream, float eps, const float* weights) {
  if (rows <= 0) return hipSuccess;
  if ((ldv & 7) || ((uintptr_t)logits & 15) || ldv > 8 * 8192 || !(eps >= 0.f && eps < 1.f)) return hipErrorInvalidValue;
  if (weights != nullptr) {
    if (eps > 0.f) ce_bf16_pick<true, true>(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, stream, eps, weights);
    else ce_bf16_pick<false, true>(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, stream, 0.f, weights);
  } else if (eps > 0.f) {
    ce_bf16_pick<true, false>(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, stream, eps, nullptr);
  } else {
    ce_bf16_pick<false, false>(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, stream, 0.f, nullptr);
  }
  return hipGetLastError();
}

hipError_t kmb_loss_finish_launch(const float* loss_rows, int rows, const int32_t* count, float* loss,
                                  hipStream_t stream, bool sum) {
  if (sum) hipLaunchKernelGGL(loss_finish_kernel<true>, dim3(1), dim3(1024), 0, stream, loss_rows, rows, count, loss);
  else hipLaunchKernelGGL(loss_finish_kernel<false>, dim3(1), dim3(1024), 0, stream, loss_rows, rows, count, loss);
  return hipGetLastError();
}
