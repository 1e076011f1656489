// C-ABI wrappers around single kernels (unit tests, profiling).  See include/kmbart.h.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <string>

#include "kernels.h"
#include "sample.h"
#include "beam_sample.h"
#include "greedy.h"
#include "beam_process.h"
#include "logits_process.h"
#include "cider_reward.h"

extern "C" const char* kmb_last_error(void);
int kmb_set_error(const char* msg);  // engine.cpp

namespace {
int hipfail(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  char buf[512];
  snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  return kmb_set_error(buf);
}
}  // namespace

// (shader clock ticks, 100 MHz real-time ticks) per XCD: the quotient of two stamps' differences is the clock the chip held in
// between (MI355X_MICROARCH.md "DVFS give-back" item 6).  One wave per workgroup, the grid round-robins over the eight XCDs.
__global__ void clock_stamp_kernel(long long* out) {
  if (threadIdx.x == 0) {
    const unsigned xcc = __builtin_amdgcn_s_getreg(0xF814) & 7u;   // HW_REG_XCC_ID
    const long long c = (long long)__builtin_amdgcn_s_memtime(), r = (long long)__builtin_amdgcn_s_memrealtime();
    out[2 * xcc] = c; out[2 * xcc + 1] = r;   // any workgroup of the XCD may win: the pairs are microseconds apart at most
  }
}

extern "C" {

int kmb_clock_stamp(int64_t* out16, void* stream) {
  if (!out16) return kmb_set_error("kmb_clock_stamp: out16 (device, 16 x int64) is required");
  hipLaunchKernelGGL(clock_stamp_kernel, dim3(64), dim3(64), 0, (hipStream_t)stream, (long long*)out16);
  return hipfail(hipGetLastError(), "clock_stamp");
}

// n per-sample region-feature tensors (device pointers in a HOST array; rows[i] rows of feat_dim contiguous floats each, rows[i] may be 0)
// -> packed_out [sum rows, feat_dim] in list order: the batch layout kmb_batch.image_features wants, in ceil(n / 128) launches
int kmb_pack_features(const float* const* rows_dev_ptrs, const int32_t* rows, int32_t n, int32_t feat_dim, float* packed_out, void* stream) {
  if (n < 0 || feat_dim <= 0 || (n > 0 && (!rows_dev_ptrs || !rows || !packed_out))) return kmb_set_error("kmb_pack_features: bad arguments");
  int32_t off = 0;
  for (int32_t i0 = 0; i0 < n; i0 += KMB_PACK_MAX) {
    KmbPackList l;
    l.n = 0;
    for (int32_t i = i0; i < n && i < i0 + KMB_PACK_MAX; ++i) {
      if (rows[i] < 0 || (rows[i] > 0 && !rows_dev_ptrs[i])) return kmb_set_error("kmb_pack_features: null tensor with rows > 0, or a negative row count");
      l.src[l.n] = rows_dev_ptrs[i]; l.rows[l.n] = rows[i]; l.off[l.n] = off; ++l.n;
      off += rows[i];
    }
    const int e = hipfail(kmb_pack_features_launch(l, feat_dim, packed_out, (hipStream_t)stream), "pack_features");
    if (e) return e;
  }
  return 0;
}

int kmb_op_gemm(const KmbGemm* p, void* stream) {
  const char* why = kmb_gemm_check(*p);
  if (why) return kmb_set_error(why);
  return hipfail(kmb_gemm_launch(*p, (hipStream_t)stream), "gemm");
}
int kmb_op_gemm_group(const KmbGemm* probs, int32_t n, void* stream) {
  if (!probs) return kmb_set_error("kmb_op_gemm_group: null problem list");
  const char* why = kmb_gemm_group_check(probs, n);
  if (why) return kmb_set_error(why);
  return hipfail(kmb_gemm_group_launch(probs, n, (hipStream_t)stream), "gemm_group");
}
int kmb_op_gemm_allrows(const KmbGemm* p, void* stream) {
  const char* why = kmb_gemm_check(*p);
  if (!why) why = kmb_gemm_allrows_check(*p);
  if (why) return kmb_set_error(why);
  return hipfail(kmb_gemm_allrows_launch(*p, nullptr, (hipStream_t)stream), "gemm_allrows");
}
int64_t kmb_op_gemm_allrows_stats_floats(int N) { return (int64_t)kmb_gemm_allrows_stats_floats(N); }
int kmb_op_gemm_allrows_stats(const KmbGemm* p, float* stats, void* stream) {
  const char* why = kmb_gemm_check(*p);
  if (!why) why = kmb_gemm_allrows_check(*p);
  if (why) return kmb_set_error(why);
  if (!stats) return kmb_set_error("kmb_op_gemm_allrows_stats: stats is required");
  return hipfail(kmb_gemm_allrows_launch(*p, stats, (hipStream_t)stream), "gemm_allrows_stats");
}
// the scoring class of the vocabulary projection (gemm_lean.hip LN_SCORE) and its finish (loss.hip), without a model
int64_t kmb_op_gemm_score_stats_floats(int M, int N) { return M > 0 && N > 0 ? (int64_t)M * (N / 64) * 2 : 0; }
int kmb_op_gemm_score(const KmbGemm* p, float* stats, void* stream) {
  if (!p) return kmb_set_error("kmb_op_gemm_score: null problem");
  const char* why = kmb_gemm_score_check(*p, stats);
  if (why) return kmb_set_error(why);
  return hipfail(kmb_gemm_score_launch(*p, stats, (hipStream_t)stream), "gemm_score");
}
int kmb_op_score_rows_finish(const float* stats, int blocks, const float* label_logit, const int64_t* labels, int B, int T, int V,
                             float* token_logprob, float* sample_nll, int32_t* sample_count, void* stream) {
  if (!stats || !label_logit || !labels || !token_logprob || !sample_nll || !sample_count || blocks <= 0 || B <= 0 || T <= 0 || V <= 0)
    return kmb_set_error("kmb_op_score_rows_finish: bad arguments");
  int e = hipfail(kmb_score_rows_finish_launch(stats, blocks, label_logit, labels, B * T, V, token_logprob, (hipStream_t)stream), "score_rows_finish");
  if (e) return e;
  return hipfail(kmb_score_segments_launch(token_logprob, 0, labels, B, T, V, token_logprob, sample_nll, sample_count, (hipStream_t)stream),
                 "score_segments");
}
int kmb_beam_step_stats(const float* logits, int ld, int V, int B, int num_beams, const float* add, int force_token, int ban_token,
                        int k, int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx,
                        const float* stats, int stats_blocks, void* stream) {
  if (!logits || !out || !stats) return kmb_set_error("kmb_beam_step_stats: missing tensor");
  if (!next_scores || !next_tokens || !next_beam_idx) return kmb_set_error("kmb_beam_step_stats: missing output");
  const KmbBeamStep p{logits, ld, V, B, num_beams, add, force_token, ban_token, k, out, eos_token, next_scores, next_tokens, next_beam_idx};
  const hipError_t e = kmb_beam_step_stats_launch(p, stats, stats_blocks, (hipStream_t)stream);
  if (e == hipErrorNotSupported)
    return kmb_set_error("kmb_beam_step_stats: unsupported shape (B * num_beams <= 320, k <= 16, num_beams <= 16, V %% 4 == 0, "
                         "stats_blocks == ceil(V / 256))");
  return hipfail(e, "beam_step_stats");
}
int kmb_op_attn_fwd(const KmbAttn* p, void* stream) {
  const char* why = kmb_attn_check(*p, 0);
  if (why) return kmb_set_error(why);
  return hipfail(kmb_attn_fwd_launch(*p, (hipStream_t)stream), "attn_fwd");
}
int kmb_op_attn_bwd(const KmbAttn* p, void* stream) {
  const char* why = kmb_attn_check(*p, 1);
  if (why) return kmb_set_error(why);
  return hipfail(kmb_attn_bwd_launch(*p, (hipStream_t)stream), "attn_bwd");
}
int kmb_op_attn_decode(const KmbAttnDecode* p, void* stream) {
  if (!p) return kmb_set_error("kmb_op_attn_decode: null problem");
  const char* why = kmb_attn_decode_check(*p);
  if (why) return kmb_set_error(why);
  return hipfail(kmb_attn_decode_launch(*p, (hipStream_t)stream), "attn_decode");
}
int kmb_op_decode_block(const KmbDecodeBlock* p, void* stream) {
  const char* why = kmb_decode_block_check(*p);
  if (why) return kmb_set_error(why);
  return hipfail(kmb_decode_block_launch(*p, (hipStream_t)stream), "decode_block");
}
int kmb_op_decode_pack(const kmb_bf16* W, int ld, int N, int K, kmb_bf16* packed, void* stream) {
  return hipfail(kmb_decode_pack_launch(&W, &ld, &N, &K, &packed, 1, (hipStream_t)stream), "decode_pack");
}
int kmb_op_decode_pack_fp8(const kmb_bf16* W, int ld, int N, int K, uint8_t* codes, int8_t* exps, void* stream) {
  if (!W || !codes || !exps) return kmb_set_error("kmb_op_decode_pack_fp8: missing tensor");
  return hipfail(kmb_decode_pack_fp8_launch(&W, &ld, &N, &K, &codes, &exps, 1, (hipStream_t)stream), "decode_pack_fp8");
}
int kmb_abi_sizeof_decode_block(void) { return (int)sizeof(KmbDecodeBlock); }
int kmb_op_ln_fwd(const kmb_bf16* z, const float* gamma, const float* beta, kmb_bf16* y, float* mean, float* rstd,
                  int M, int D, float eps, void* stream) {
  return hipfail(kmb_ln_fwd_launch(z, gamma, beta, y, mean, rstd, M, D, eps, (hipStream_t)stream), "ln_fwd");
}
int64_t kmb_op_ln_bwd_scratch(int M, int D) { return (int64_t)kmb_ln_bwd_parts(M) * 3 * D; }
int kmb_op_ln_bwd(const kmb_bf16* dy, const kmb_bf16* z, const float* mean, const float* rstd, const float* gamma,
                  kmb_bf16* dz, kmb_bf16* out2, const KmbDrop* dy_drop, const KmbDrop* out2_drop, float* dgamma,
                  float* dbeta, float* scratch, int M, int D, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const KmbDrop none{0u, 0u, 1.f};
  int rc = hipfail(kmb_ln_bwd_launch(dy, z, mean, rstd, gamma, dz, out2, dy_drop ? *dy_drop : none,
                                     out2_drop ? *out2_drop : none, scratch, M, D, s), "ln_bwd");
  if (rc) return rc;
  const int np = kmb_ln_bwd_parts(M);
  rc = hipfail(kmb_reduce_parts_launch(scratch, np, 3 * D, dgamma, D, s), "ln_bwd reduce");
  if (rc) return rc;
  return hipfail(kmb_reduce_parts_launch(scratch + D, np, 3 * D, dbeta, D, s), "ln_bwd reduce");
}
// the same kernel reduced as the engine reduces it (engine_train.cpp ln_backward with a bias slot): ONE kmb_reduce_parts2_launch sends
// columns [0, 2 D) of the partial rows to dgamma | dbeta (adjacent, as in the arena) and the third partial, the column sums of the
// sub-layer gradient, to dsub
int kmb_op_ln_bwd_sub(const kmb_bf16* dy, const kmb_bf16* z, const float* mean, const float* rstd, const float* gamma,
                      kmb_bf16* dz, kmb_bf16* out2, const KmbDrop* dy_drop, const KmbDrop* out2_drop, float* dgamma,
                      float* dbeta, float* dsub, float* scratch, int M, int D, void* stream) {
  if (!dy || !z || !mean || !rstd || !gamma || !dz || !dgamma || !dbeta || !dsub || !scratch || M <= 0 || D <= 0)
    return kmb_set_error("kmb_op_ln_bwd_sub: dy, z, mean, rstd, gamma, dz, dgamma, dbeta, dsub and scratch are required, M and D positive");
  if ((D & 7) || D > 2048) return kmb_set_error("kmb_op_ln_bwd_sub: D must be a multiple of 8 and at most 2048");
  if (dbeta != dgamma + D) return kmb_set_error("kmb_op_ln_bwd_sub: dbeta must be dgamma + D (one 2 D-wide output, as in the gradient arena)");
  if ((((uintptr_t)dy | (uintptr_t)z | (uintptr_t)dz | (uintptr_t)out2) & 7) ||
      (((uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)gamma | (uintptr_t)dgamma | (uintptr_t)dsub | (uintptr_t)scratch) & 3))
    return kmb_set_error("kmb_op_ln_bwd_sub: dy, z, dz and out2 must be 8-byte aligned, the float pointers 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const KmbDrop none{0u, 0u, 1.f};
  const int rc = hipfail(kmb_ln_bwd_launch(dy, z, mean, rstd, gamma, dz, out2, dy_drop ? *dy_drop : none,
                                           out2_drop ? *out2_drop : none, scratch, M, D, s), "ln_bwd");
  if (rc) return rc;
  return hipfail(kmb_reduce_parts2_launch(scratch, kmb_ln_bwd_parts(M), 3 * D, dgamma, 2 * D, dsub, D, s), "ln_bwd reduce2");
}
// the decode step's residual projection behind a split-K GEMM: slabs summed in slice order, + bias + residual, bf16, LayerNorm
int kmb_op_ln_fwd_slabs(const float* slabs, int nslabs, int64_t stride, const float* bias, const kmb_bf16* residual, int ld_res,
                        const float* gamma, const float* beta, kmb_bf16* y, int M, int D, float eps, void* stream) {
  if (!slabs || !residual || !gamma || !beta || !y || nslabs < 1 || stride < 0 || M <= 0 || D <= 0 || ld_res < D)
    return kmb_set_error("kmb_op_ln_fwd_slabs: slabs, residual (the kernel always reads it), gamma, beta and y are required, "
                         "nslabs >= 1, stride >= 0, M and D positive, ld_res >= D");
  if ((D & 7) || D > 1024) return kmb_set_error("kmb_op_ln_fwd_slabs: D must be a multiple of 8 and at most 1024");
  if ((stride & 3) || (ld_res & 7)) return kmb_set_error("kmb_op_ln_fwd_slabs: stride must be a multiple of 4, ld_res of 8");
  if ((((uintptr_t)slabs | (uintptr_t)residual | (uintptr_t)y) & 15) || (((uintptr_t)bias | (uintptr_t)gamma | (uintptr_t)beta) & 3))
    return kmb_set_error("kmb_op_ln_fwd_slabs: slabs, residual and y must be 16-byte aligned, bias, gamma and beta 4-byte aligned");
  return hipfail(kmb_ln_fwd_slabs_launch(slabs, nslabs, (size_t)stride, bias, residual, ld_res, gamma, beta, y, M, D, eps,
                                         (hipStream_t)stream), "ln_fwd_slabs");
}
// out[i] = beta * out[i] + sum over s < nslabs of slabs[s * stride + i], in slice order (a split weight gradient)
int kmb_op_reduce_slabs(const float* slabs, int nslabs, int64_t stride, float* out, int64_t n, float beta, void* stream) {
  if (!slabs || !out || nslabs < 1 || stride < 0 || n <= 0) return kmb_set_error("kmb_op_reduce_slabs: bad arguments");
  if ((n & 3) || (stride & 3) || (((uintptr_t)slabs | (uintptr_t)out) & 15))
    return kmb_set_error("kmb_op_reduce_slabs: n and stride must be multiples of 4, the pointers 16-byte aligned");
  return hipfail(kmb_reduce_slabs_launch(slabs, nslabs, (size_t)stride, out, (size_t)n, beta, (hipStream_t)stream), "reduce_slabs");
}
// the same sum stored as bf16 (a split data gradient)
int kmb_op_reduce_slabs_bf16(const float* slabs, int nslabs, int64_t stride, kmb_bf16* out, int64_t n, void* stream) {
  if (!slabs || !out || nslabs < 1 || stride < 0 || n <= 0) return kmb_set_error("kmb_op_reduce_slabs_bf16: bad arguments");
  if ((n & 7) || (stride & 3) || (((uintptr_t)slabs | (uintptr_t)out) & 15))
    return kmb_set_error("kmb_op_reduce_slabs_bf16: n must be a multiple of 8, stride of 4, the pointers 16-byte aligned");
  return hipfail(kmb_reduce_slabs_bf16_launch(slabs, nslabs, (size_t)stride, out, (size_t)n, (hipStream_t)stream), "reduce_slabs_bf16");
}
// ... with a linear layer's epilogue: out = bf16(drop((sum + bias) * (column < col_scale_n ? col_scale : 1)) + residual)
int kmb_op_reduce_slabs_epi(const float* slabs, int nslabs, int64_t stride, const float* bias, float col_scale, int col_scale_n,
                            const KmbDrop* drop, const kmb_bf16* residual, int ld_res, kmb_bf16* out, int ld_out, int M, int N,
                            void* stream) {
  if (!slabs || !out || nslabs < 1 || stride < 0 || M <= 0 || N <= 0 || ld_out < N || (residual && ld_res < N))
    return kmb_set_error("kmb_op_reduce_slabs_epi: slabs and out are required, nslabs >= 1, stride >= 0, M and N positive, ld_out and ld_res >= N");
  if ((N & 7) || (stride & 3) || (ld_out & 7) || (residual && (ld_res & 7)))
    return kmb_set_error("kmb_op_reduce_slabs_epi: N, ld_out and ld_res must be multiples of 8, stride of 4");
  if ((((uintptr_t)slabs | (uintptr_t)out | (uintptr_t)residual) & 15) || ((uintptr_t)bias & 3))
    return kmb_set_error("kmb_op_reduce_slabs_epi: slabs, out and residual must be 16-byte aligned, bias 4-byte aligned");
  const KmbDrop dr = drop ? *drop : KmbDrop{0u, 0u, 1.f};
  if (dr.thr16 > 65535u) return kmb_set_error("kmb_op_reduce_slabs_epi: thr16 must be at most 65535");
  return hipfail(kmb_reduce_slabs_epi_launch(slabs, nslabs, (size_t)stride, bias, col_scale, col_scale_n, dr, residual, ld_res, out,
                                             ld_out, M, N, (hipStream_t)stream), "reduce_slabs_epi");
}
int64_t kmb_op_colsum_scratch(int M, int N) { return (int64_t)kmb_colsum_parts(M) * N; }
int kmb_op_colsum(const kmb_bf16* X, int ld, int M, int N, float* out, float* scratch, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = hipfail(kmb_colsum_launch(X, ld, M, N, scratch, s), "colsum");
  if (rc) return rc;
  return hipfail(kmb_reduce_parts_launch(scratch, kmb_colsum_parts(M), N, out, N, s), "colsum reduce");
}
int kmb_op_img_rowmap(const int64_t* ids, const int32_t* feat_off, int B, int S, int64_t img_feat_id, int64_t cls_id,
                      int32_t* img_src, int32_t* status, void* stream) {
  return hipfail(kmb_img_rowmap_launch(ids, feat_off, B, S, img_feat_id, cls_id, img_src, status, (hipStream_t)stream), "img_rowmap");
}
int kmb_op_cast_pad(const float* x, int N, int Fin, kmb_bf16* y, int Fpad, void* stream) {
  return hipfail(kmb_cast_pad_launch(x, N, Fin, y, Fpad, (hipStream_t)stream), "cast_pad");
}
int kmb_op_embed_ln_fwd(const int64_t* ids, const int32_t* img_src, const float* E, const float* img_emb,
                        const float* P, int pos_base, int S, float scale, const float* gamma, const float* beta,
                        kmb_bf16* z, kmb_bf16* y, float* mean, float* rstd, int M, int D, float eps,
                        const KmbDrop* drop, void* stream) {
  const KmbDrop none{0u, 0u, 1.f};
  return hipfail(kmb_embed_ln_fwd_launch(ids, img_src, E, img_emb, P, pos_base, S, scale, gamma, beta, z, y, mean,
                                         rstd, M, D, eps, drop ? *drop : none, (hipStream_t)stream), "embed_ln_fwd");
}
int kmb_op_embed_bwd(const kmb_bf16* dz, const int64_t* ids, const int32_t* img_src, float scale, float* dE,
                     kmb_bf16* dimg, int64_t pad_id, int M, int D, void* stream) {
  return hipfail(kmb_embed_bwd_launch(dz, ids, img_src, scale, dE, dimg, pad_id, M, D, (hipStream_t)stream), "embed_bwd");
}
int kmb_op_pos_bwd(const kmb_bf16* dz, int B, int S, int D, float* dP, int pos_base, int P_rows, void* stream) {
  return hipfail(kmb_pos_bwd_launch(dz, B, S, D, dP, pos_base, P_rows, (hipStream_t)stream), "pos_bwd");
}
int kmb_op_ce(const float* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale,
              float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = hipfail(kmb_count_valid_launch(labels, rows, V, count, nullptr, s), "count_valid");
  if (rc) return rc;
  rc = hipfail(kmb_ce_launch(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, s), "ce");
  if (rc) return rc;
  return hipfail(kmb_loss_finish_launch(loss_rows, rows, count, loss, s), "loss_finish");
}
// the training head's bf16 form (ce_kernel_reg_bf16): dlogits may be null or equal to logits; status (optional) as kmb_op_count_valid
int kmb_op_ce_bf16(const kmb_bf16* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float* loss_rows,
                   kmb_bf16* dlogits, int32_t* count, float* loss, int32_t* status, void* stream) {
  if (!logits || !labels || !loss_rows || !count || !loss || rows <= 0 || V <= 0 || ldv < V)
    return kmb_set_error("kmb_op_ce_bf16: bad arguments");
  if ((ldv & 7) || ldv > 65536) return kmb_set_error("kmb_op_ce_bf16: ldv must be a multiple of 8 and at most 65536");
  hipStream_t s = (hipStream_t)stream;
  int rc = hipfail(kmb_count_valid_launch(labels, rows, V, count, status, s), "count_valid");
  if (rc) return rc;
  rc = hipfail(kmb_ce_bf16_launch(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, s), "ce_bf16");
  if (rc) return rc;
  return hipfail(kmb_loss_finish_launch(loss_rows, rows, count, loss, s), "loss_finish");
}
int kmb_op_count_valid(const int64_t* labels, int n, int V, int32_t* count, int32_t* status, void* stream) {
  if (!labels || !count || n < 0) return kmb_set_error("kmb_op_count_valid: bad arguments");
  return hipfail(kmb_count_valid_launch(labels, n, V, count, status, (hipStream_t)stream), "count_valid");
}
int kmb_op_loss_finish(const float* loss_rows, int rows, const int32_t* count, float* loss, void* stream) {
  if (!loss_rows || !count || !loss || rows <= 0) return kmb_set_error("kmb_op_loss_finish: bad arguments");
  return hipfail(kmb_loss_finish_launch(loss_rows, rows, count, loss, (hipStream_t)stream), "loss_finish");
}
int kmb_op_ce_label_logit(const kmb_bf16* H, int ldh, const kmb_bf16* E, int lde, const float* bias, const int64_t* labels, int rows,
                          int d, int V, int Vpad, float* shift, float* bias_pad, void* stream) {
  if (!H || !E || !bias || !labels || !shift || !bias_pad || rows <= 0 || d <= 0 || V <= 0 || Vpad < V || ldh < d || lde < d)
    return kmb_set_error("kmb_op_ce_label_logit: bad arguments");
  if ((d & 7) || (ldh & 7) || (lde & 7)) return kmb_set_error("kmb_op_ce_label_logit: d, ldh and lde must be multiples of 8");
  const int rc = hipfail(kmb_ce_label_logit_launch(H, ldh, E, lde, bias, labels, rows, d, V, shift, (hipStream_t)stream), "ce_label_logit");
  if (rc) return rc;
  return hipfail(kmb_ce_pad_bias_launch(bias, V, Vpad, bias_pad, (hipStream_t)stream), "ce_pad_bias");
}
int kmb_op_ce_rows_finish(const float* row_sums, int ld_sums, int nparts, const float* pick, const int64_t* labels, const int32_t* count,
                          float lm_factor, int rows, int d, int V, const kmb_bf16* H, int ldh, float* loss_rows, float* srow,
                          float* alpha, kmb_bf16* ah, kmb_bf16* P, int ldp, void* stream) {
  if (!row_sums || !labels || !count || !loss_rows || !srow || !alpha || rows <= 0 || nparts <= 0 || ld_sums < nparts || V <= 0 ||
      (ah && !H) || (P && ldp < V))
    return kmb_set_error("kmb_op_ce_rows_finish: bad arguments");
  if (ah && (d <= 0 || (d & 7) || (ldh & 7) || ldh < d)) return kmb_set_error("kmb_op_ce_rows_finish: d and ldh must be multiples of 8, ldh >= d");
  return hipfail(kmb_ce_rows_finish_launch(row_sums, ld_sums, nparts, pick, labels, count, lm_factor, rows, ah ? d : 0, V, H, ldh, loss_rows,
                                           srow, alpha, ah, P, ldp, (hipStream_t)stream), "ce_rows_finish");
}
int kmb_op_ce_dgrad_finish(const float* slab, int nslabs, int64_t stride, const float* alpha, kmb_bf16* out, int rows, int d, void* stream) {
  if (!slab || !alpha || !out || rows <= 0 || nslabs < 1 || d <= 0 || stride < 0) return kmb_set_error("kmb_op_ce_dgrad_finish: bad arguments");
  if ((d & 7) || (stride & 3)) return kmb_set_error("kmb_op_ce_dgrad_finish: d must be a multiple of 8, stride of 4");
  return hipfail(kmb_ce_dgrad_finish_launch(slab, nslabs, (size_t)stride, alpha, out, rows, d, (hipStream_t)stream), "ce_dgrad_finish");
}
// ---- label smoothing (kmb_set_label_smoothing), piece by piece
static bool eps_ok(float eps) { return eps >= 0.f && eps < 1.f; }   // (NaN fails both)
int kmb_op_ce_smooth(const float* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float eps,
                     float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss, void* stream) {
  if (!logits || !labels || !loss_rows || !count || !loss || rows <= 0 || V <= 0 || ldv < V) return kmb_set_error("kmb_op_ce_smooth: bad arguments");
  if (!eps_ok(eps)) return kmb_set_error("kmb_op_ce_smooth: eps must be in [0, 1)");
  hipStream_t s = (hipStream_t)stream;
  int rc = hipfail(kmb_count_valid_launch(labels, rows, V, count, nullptr, s), "count_valid");
  if (rc) return rc;
  rc = hipfail(kmb_ce_launch(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, s, eps), "ce_smooth");
  if (rc) return rc;
  return hipfail(kmb_loss_finish_launch(loss_rows, rows, count, loss, s), "loss_finish");
}
int kmb_op_ce_bf16_smooth(const kmb_bf16* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float eps,
                          float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss, int32_t* status, void* stream) {
  if (!logits || !labels || !loss_rows || !count || !loss || rows <= 0 || V <= 0 || ldv < V)
    return kmb_set_error("kmb_op_ce_bf16_smooth: bad arguments");
  if ((ldv & 7) || ldv > 65536) return kmb_set_error("kmb_op_ce_bf16_smooth: ldv must be a multiple of 8 and at most 65536");
  if (!eps_ok(eps)) return kmb_set_error("kmb_op_ce_bf16_smooth: eps must be in [0, 1)");
  hipStream_t s = (hipStream_t)stream;
  int rc = hipfail(kmb_count_valid_launch(labels, rows, V, count, status, s), "count_valid");
  if (rc) return rc;
  rc = hipfail(kmb_ce_bf16_launch(logits, ldv, V, labels, rows, count, grad_scale, loss_rows, dlogits, s, eps), "ce_bf16_smooth");
  if (rc) return rc;
  return hipfail(kmb_loss_finish_launch(loss_rows, rows, count, loss, s), "loss_finish");
}
int64_t kmb_op_ce_vocab_sum_scratch(int V, int d) {
  if (V <= 0 || d <= 0) return 0;
  return (int64_t)kmb_ce_vocab_sum_slots(V, d) * kmb_ce_vocab_sum_ld(d);
}
int kmb_op_ce_vocab_sum(const kmb_bf16* E, int lde, const float* bias, int V, int d, float* wsum, float* scratch, void* stream) {
  if (!E || !bias || !wsum || !scratch || V <= 0 || d <= 0 || lde < d) return kmb_set_error("kmb_op_ce_vocab_sum: bad arguments");
  if ((d & 7) || (lde & 7) || ((uintptr_t)E & 15) || ((uintptr_t)wsum & 15))
    return kmb_set_error("kmb_op_ce_vocab_sum: d and lde must be multiples of 8, E and wsum 16-byte aligned");
  return hipfail(kmb_ce_vocab_sum_launch(E, lde, bias, V, d, scratch, wsum, (hipStream_t)stream), "ce_vocab_sum");
}
int64_t kmb_op_ce_rows_finish_smooth_scratch(int rows, int d) {
  if (rows <= 0 || d <= 0) return 0;
  return (int64_t)kmb_ce_rows_slots(rows) * d;
}
int kmb_op_ce_rows_finish_smooth(const float* row_sums, int ld_sums, int nparts, const float* pick, const float* shift, const int64_t* labels,
                                 const int32_t* count, float lm_factor, float eps, int rows, int d, int V, const kmb_bf16* H, int ldh,
                                 const float* wsum, float* loss_rows, float* srow, float* alpha, float* beta, kmb_bf16* ah, kmb_bf16* P,
                                 int ldp, float* neg_u, float* scratch, void* stream) {
  if (!row_sums || !shift || !labels || !count || !H || !wsum || !loss_rows || !srow || !alpha || !beta || rows <= 0 || nparts <= 0 ||
      ld_sums < nparts || V <= 0 || (P && ldp < V) || (neg_u && !scratch))
    return kmb_set_error("kmb_op_ce_rows_finish_smooth: bad arguments");
  if (d <= 0 || (d & 7) || (ldh & 7) || ldh < d || d > 4096 || ((uintptr_t)wsum & 15))
    return kmb_set_error("kmb_op_ce_rows_finish_smooth: d and ldh must be multiples of 8, ldh >= d, d <= 4096, wsum 16-byte aligned");
  if (!eps_ok(eps)) return kmb_set_error("kmb_op_ce_rows_finish_smooth: eps must be in [0, 1)");
  return hipfail(kmb_ce_rows_finish_ls_launch(row_sums, ld_sums, nparts, pick, shift, labels, count, lm_factor, eps, rows, d, V, H, ldh, wsum,
                                              loss_rows, srow, alpha, beta, ah, P, ldp, neg_u ? scratch : nullptr, neg_u, (hipStream_t)stream),
                 "ce_rows_finish_smooth");
}
int kmb_op_ce_dgrad_finish_smooth(const float* slab, int nslabs, int64_t stride, const float* alpha, const float* beta, const float* wsum,
                                  kmb_bf16* out, int rows, int d, void* stream) {
  if (!slab || !alpha || !beta || !wsum || !out || rows <= 0 || nslabs < 1 || d <= 0 || stride < 0)
    return kmb_set_error("kmb_op_ce_dgrad_finish_smooth: bad arguments");
  if ((d & 7) || (stride & 3) || ((uintptr_t)wsum & 15))
    return kmb_set_error("kmb_op_ce_dgrad_finish_smooth: d must be a multiple of 8, stride of 4, wsum 16-byte aligned");
  return hipfail(kmb_ce_dgrad_finish_ls_launch(slab, nslabs, (size_t)stride, alpha, beta, wsum, out, rows, d, (hipStream_t)stream),
                 "ce_dgrad_finish_smooth");
}
// ---- per-row loss weights and the "sum" reduction (kmb_forward_opts.row_weights / loss_reduction), piece by piece
// the denominator word the kernels divide by: count[0] for the mean; for the sum count[1] = count[0] > 0, written here
static int weighted_den(int32_t* count, int reduction, hipStream_t s, const int32_t** den) {
  *den = count;
  if (reduction == 0) return 0;
  *den = count + 1;
  return hipfail(kmb_count_flag_launch(count, count + 1, s), "count_flag");
}
int kmb_op_ce_weighted(const float* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float eps,
                       const float* weights, int reduction, float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss, void* stream) {
  if (!logits || !labels || !loss_rows || !count || !loss || rows <= 0 || V <= 0 || ldv < V) return kmb_set_error("kmb_op_ce_weighted: bad arguments");
  if (!eps_ok(eps)) return kmb_set_error("kmb_op_ce_weighted: eps must be in [0, 1)");
  if (reduction != 0 && reduction != 1) return kmb_set_error("kmb_op_ce_weighted: reduction must be 0 (mean) or 1 (sum)");
  hipStream_t s = (hipStream_t)stream;
  int rc = hipfail(kmb_count_valid_launch(labels, rows, V, count, nullptr, s), "count_valid");
  if (rc) return rc;
  const int32_t* den;
  if ((rc = weighted_den(count, reduction, s, &den))) return rc;
  rc = hipfail(kmb_ce_launch(logits, ldv, V, labels, rows, den, grad_scale, loss_rows, dlogits, s, eps, weights), "ce_weighted");
  if (rc) return rc;
  return hipfail(kmb_loss_finish_launch(loss_rows, rows, count, loss, s, reduction == 1), "loss_finish");
}
int kmb_op_ce_bf16_weighted(const kmb_bf16* logits, int ldv, int V, const int64_t* labels, int rows, float grad_scale, float eps,
                            const float* weights, int reduction, float* loss_rows, kmb_bf16* dlogits, int32_t* count, float* loss,
                            int32_t* status, void* stream) {
  if (!logits || !labels || !loss_rows || !count || !loss || rows <= 0 || V <= 0 || ldv < V)
    return kmb_set_error("kmb_op_ce_bf16_weighted: bad arguments");
  if ((ldv & 7) || ldv > 65536) return kmb_set_error("kmb_op_ce_bf16_weighted: ldv must be a multiple of 8 and at most 65536");
  if (!eps_ok(eps)) return kmb_set_error("kmb_op_ce_bf16_weighted: eps must be in [0, 1)");
  if (reduction != 0 && reduction != 1) return kmb_set_error("kmb_op_ce_bf16_weighted: reduction must be 0 (mean) or 1 (sum)");
  hipStream_t s = (hipStream_t)stream;
  int rc = hipfail(kmb_count_valid_launch(labels, rows, V, count, status, s), "count_valid");
  if (rc) return rc;
  const int32_t* den;
  if ((rc = weighted_den(count, reduction, s, &den))) return rc;
  rc = hipfail(kmb_ce_bf16_launch(logits, ldv, V, labels, rows, den, grad_scale, loss_rows, dlogits, s, eps, weights), "ce_bf16_weighted");
  if (rc) return rc;
  return hipfail(kmb_loss_finish_launch(loss_rows, rows, count, loss, s, reduction == 1), "loss_finish");
}
int kmb_op_ce_rows_finish_weighted(const float* row_sums, int ld_sums, int nparts, const float* pick, const float* shift,
                                   const int64_t* labels, int32_t* count, float lm_factor, float eps, const float* weights, int reduction,
                                   int rows, int d, int V, const kmb_bf16* H, int ldh, const float* wsum, float* loss_rows, float* srow,
                                   float* alpha, float* beta, kmb_bf16* ah, kmb_bf16* P, int ldp, float* neg_u, float* scratch, void* stream) {
  if (!row_sums || !labels || !count || !loss_rows || !srow || !alpha || rows <= 0 || nparts <= 0 || ld_sums < nparts || V <= 0 ||
      (ah && !H) || (P && ldp < V))
    return kmb_set_error("kmb_op_ce_rows_finish_weighted: bad arguments");
  if (!eps_ok(eps)) return kmb_set_error("kmb_op_ce_rows_finish_weighted: eps must be in [0, 1)");
  if (reduction != 0 && reduction != 1) return kmb_set_error("kmb_op_ce_rows_finish_weighted: reduction must be 0 (mean) or 1 (sum)");
  hipStream_t s = (hipStream_t)stream;
  const int32_t* den;
  if (int rc = weighted_den(count, reduction, s, &den)) return rc;
  if (eps > 0.f) {
    if (!shift || !H || !wsum || !beta || (neg_u && !scratch)) return kmb_set_error("kmb_op_ce_rows_finish_weighted: eps > 0 needs shift, H, wsum and beta");
    if (d <= 0 || (d & 7) || (ldh & 7) || ldh < d || d > 4096 || ((uintptr_t)wsum & 15))
      return kmb_set_error("kmb_op_ce_rows_finish_weighted: d and ldh must be multiples of 8, ldh >= d, d <= 4096, wsum 16-byte aligned");
    return hipfail(kmb_ce_rows_finish_ls_launch(row_sums, ld_sums, nparts, pick, shift, labels, den, lm_factor, eps, rows, d, V, H, ldh, wsum,
                                                loss_rows, srow, alpha, beta, ah, P, ldp, neg_u ? scratch : nullptr, neg_u, s, weights),
                   "ce_rows_finish_weighted");
  }
  if (ah && (d <= 0 || (d & 7) || (ldh & 7) || ldh < d)) return kmb_set_error("kmb_op_ce_rows_finish_weighted: d and ldh must be multiples of 8, ldh >= d");
  return hipfail(kmb_ce_rows_finish_launch(row_sums, ld_sums, nparts, pick, labels, den, lm_factor, rows, ah ? d : 0, V, H, ldh, loss_rows,
                                           srow, alpha, ah, P, ldp, s, weights), "ce_rows_finish_weighted");
}
int kmb_op_reduce_slabs_rowvec(const float* slabs, int nslabs, int64_t stride, float* out, int M, int N, float beta, const float* rowvec,
                               void* stream) {
  if (!slabs || !out || !rowvec || nslabs < 1 || stride < 0 || M <= 0 || N <= 0) return kmb_set_error("kmb_op_reduce_slabs_rowvec: bad arguments");
  if ((N & 3) || (stride & 3) || ((uintptr_t)rowvec & 15) || ((uintptr_t)out & 15) || ((uintptr_t)slabs & 15))
    return kmb_set_error("kmb_op_reduce_slabs_rowvec: N and stride must be multiples of 4, the pointers 16-byte aligned");
  return hipfail(kmb_reduce_slabs_rowvec_launch(slabs, nslabs, (size_t)stride, out, (size_t)M * N, beta, rowvec, N, (hipStream_t)stream),
                 "reduce_slabs_rowvec");
}
int kmb_op_kl_div(const float* logits, int ld, int C, const float* target, int ldt, int rows, float grad_scale, float* loss_rows,
                  kmb_bf16* dlogits, int ldd, void* stream) {
  if (!logits || !target || !loss_rows || rows <= 0 || C <= 0 || ld < C || ldt < C || (dlogits && ldd < C))
    return kmb_set_error("kmb_op_kl_div: bad arguments");
  return hipfail(kmb_kl_div_launch(logits, ld, C, target, ldt, rows, grad_scale, loss_rows, dlogits, dlogits ? ldd : C, (hipStream_t)stream),
                 "kl_div");
}
int kmb_op_gather_rows_bf16(const kmb_bf16* src, int src_ld, const int32_t* idx, kmb_bf16* dst, int dst_ld, int rows, int cols,
                            void* stream) {
  if (!src || !idx || !dst || rows <= 0 || cols <= 0 || src_ld < cols || dst_ld < cols) return kmb_set_error("kmb_op_gather_rows_bf16: bad arguments");
  if ((cols & 7) || (src_ld & 7) || (dst_ld & 7)) return kmb_set_error("kmb_op_gather_rows_bf16: cols, src_ld and dst_ld must be multiples of 8");
  return hipfail(kmb_gather_rows_bf16_launch(src, src_ld, idx, dst, dst_ld, rows, cols, (hipStream_t)stream), "gather_rows_bf16");
}
int kmb_op_gather_rows_drop_bf16(const kmb_bf16* src, int src_ld, const int32_t* idx_a, const int32_t* idx_b, kmb_bf16* dst, int dst_ld,
                                 int rows, int cols, const KmbDrop* drop, void* stream) {
  const int halves = idx_b ? 2 : 1;
  if (!src || !dst || rows <= 0 || cols <= 0 || src_ld < cols || dst_ld / halves < cols)
    return kmb_set_error("kmb_op_gather_rows_drop_bf16: bad arguments");
  if ((cols & 7) || (src_ld & 7) || (dst_ld & 7))
    return kmb_set_error("kmb_op_gather_rows_drop_bf16: cols, src_ld and dst_ld must be multiples of 8");
  if (!idx_a && idx_b) return kmb_set_error("kmb_op_gather_rows_drop_bf16: idx_b needs idx_a (identity rows take no second half)");
  if (dst == src && idx_a) return kmb_set_error("kmb_op_gather_rows_drop_bf16: dst may be src with identity rows only (a gather in place would race)");
  const KmbDrop dr = drop ? *drop : KmbDrop{0u, 0u, 1.f};
  if (dr.thr16 > 65535u || (dr.thr16 != 0u && !(dr.scale > 0.f && dr.scale <= 3.4028234e38f)))
    return kmb_set_error("kmb_op_gather_rows_drop_bf16: thr16 must be at most 65535 and the scale finite and positive");
  return hipfail(kmb_gather_rows_drop_bf16_launch(src, src_ld, idx_a, idx_b, dst, dst_ld, rows, cols, dr, (hipStream_t)stream),
                 "gather_rows_drop_bf16");
}
int kmb_op_scatter_add_rows(const kmb_bf16* src, int src_ld, const int32_t* idx, float* acc, int rows, int cols, void* stream) {
  if (!src || !idx || !acc || rows <= 0 || cols <= 0 || src_ld < cols) return kmb_set_error("kmb_op_scatter_add_rows: bad arguments");
  return hipfail(kmb_scatter_add_rows_launch(src, src_ld, idx, acc, rows, cols, (hipStream_t)stream), "scatter_add_rows");
}
int kmb_op_add_f32_into_bf16(kmb_bf16* y, const float* a, int64_t n, void* stream) {
  if (!y || !a || n <= 0) return kmb_set_error("kmb_op_add_f32_into_bf16: bad arguments");
  if (n & 7) return kmb_set_error("kmb_op_add_f32_into_bf16: n must be a multiple of 8");
  return hipfail(kmb_add_f32_into_bf16_launch(y, a, (size_t)n, (hipStream_t)stream), "add_f32_into_bf16");
}
int kmb_op_mean_rows(const float* rows, int n, float factor, float denom, float* out, void* stream) {
  if (!rows || !out || n <= 0) return kmb_set_error("kmb_op_mean_rows: bad arguments");
  return hipfail(kmb_mean_rows_launch(rows, n, factor, denom, out, (hipStream_t)stream), "mean_rows");
}
int kmb_op_adamw(float* p, const float* g, float* m, float* v, kmb_bf16* p_bf16, int64_t n, const KmbAdamW* hp,
                 void* stream) {
  return hipfail(kmb_adamw_launch(p, g, m, v, p_bf16, (size_t)n, *hp, (hipStream_t)stream), "adamw");
}
int kmb_op_grad_sumsq_slots(int64_t n) { return n > 0 ? kmb_grad_sumsq_slots((size_t)n) : 0; }
int kmb_op_grad_sumsq(const float* g, int64_t n, float grad_scale, double* partials, int32_t slot0, void* stream) {
  if (!g || !partials || n <= 0 || slot0 < 0) return kmb_set_error("kmb_op_grad_sumsq: bad arguments");
  if ((uintptr_t)g & 15) return kmb_set_error("kmb_op_grad_sumsq: g must be 16-byte aligned");
  return hipfail(kmb_grad_sumsq_launch(g, (size_t)n, grad_scale, partials + slot0, (hipStream_t)stream), "grad_sumsq");
}
int kmb_op_clip_finish(const double* partials, int32_t nslots, float max_norm, int32_t skip_nonfinite, const KmbAdamW* hp,
                       KmbStepState* state, void* stream) {
  if (!partials || nslots <= 0 || !hp || !state) return kmb_set_error("kmb_op_clip_finish: bad arguments");
  return hipfail(kmb_clip_finish_launch(partials, nslots, max_norm, skip_nonfinite, *hp, state, (hipStream_t)stream), "clip_finish");
}
int kmb_op_adamw_dev(float* p, const float* g, float* m, float* v, kmb_bf16* p_bf16, int64_t n, const KmbAdamW* hp,
                     const KmbStepState* state, void* stream) {
  if (!hp || !state) return kmb_set_error("kmb_op_adamw_dev: hp and state are required");
  return hipfail(kmb_adamw_dev_launch(p, g, m, v, p_bf16, (size_t)n, *hp, state, (hipStream_t)stream), "adamw_dev");
}
int kmb_op_grad_fold(float* dst, const float* src, int64_t n, int add, void* stream) {
  if (!dst || !src || n <= 0) return kmb_set_error("kmb_op_grad_fold: bad arguments");
  if (((uintptr_t)dst | (uintptr_t)src) & 3) return kmb_set_error("kmb_op_grad_fold: dst and src must be 4-byte aligned");
  if (dst < src + n && src < dst + n) return kmb_set_error("kmb_op_grad_fold: dst and src overlap");
  return hipfail(kmb_grad_fold_launch(dst, src, (size_t)n, add, (hipStream_t)stream), "grad_fold");
}
int kmb_op_cast_bf16(const float* x, kmb_bf16* y, int64_t n, void* stream) {
  return hipfail(kmb_cast_f32_bf16_launch(x, y, (size_t)n, (hipStream_t)stream), "cast");
}
int kmb_op_dropout_mask(uint32_t seed, float p, int rows, int cols, uint8_t* keep, void* stream) {
  uint32_t thr = (uint32_t)lrintf(p * 65536.f);
  if (thr > 65535u) thr = 65535u;
  return hipfail(kmb_dropout_mask_launch(seed, thr, rows, cols, keep, (hipStream_t)stream), "dropout_mask");
}
int kmb_gemm_shared_device(int on) {
  kmb_gemm_set_shared_device(on);
  return 0;
}
int kmb_debug_gemm_route(const KmbGemm* p, int forced_variant, int32_t* out, int32_t cap) {
  if (!p || !out || cap < 1 || forced_variant < 0) return -1;
  if (kmb_gemm_check(*p) != nullptr) return -1;
  return kmb_gemm_route(*p, forced_variant, out, cap);
}
int kmb_debug_decode_route(const KmbDecodeBlock* p) {
  if (!p || kmb_decode_block_check(*p) != nullptr) return -1;
  return kmb_decode_block_route(*p);
}
int kmb_debug_attn_route(const KmbAttn* p, int backward) {
  if (!p || kmb_attn_check(*p, backward != 0) != nullptr) return -1;
  return kmb_attn_route(*p, backward != 0);
}
int kmb_beam_merge(const float* val, const int32_t* idx, int B, int num_beams, int k, int V, int32_t* out, void* stream) {
  return hipfail(kmb_beam_merge_launch(val, idx, B, num_beams, k, V, out, -1, nullptr, nullptr, nullptr, (hipStream_t)stream), "beam_merge");
}
int kmb_beam_merge_select(const float* val, const int32_t* idx, int B, int num_beams, int k, int V, int32_t* out,
                          int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, void* stream) {
  if (!next_scores || !next_tokens || !next_beam_idx) return kmb_set_error("kmb_beam_merge_select: missing output");
  return hipfail(kmb_beam_merge_launch(val, idx, B, num_beams, k, V, out, eos_token, next_scores, next_tokens, next_beam_idx,
                                       (hipStream_t)stream), "beam_merge_select");
}
int kmb_beam_step(const float* logits, int ld, int V, int B, int num_beams, const float* add, int force_token, int ban_token,
                  int k, int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx,
                  float* scratch, int64_t scratch_floats, void* stream) {
  if (!logits || !out || !scratch) return kmb_set_error("kmb_beam_step: missing tensor");
  if (!next_scores || !next_tokens || !next_beam_idx) return kmb_set_error("kmb_beam_step: missing output");
  const KmbBeamStep p{logits, ld, V, B, num_beams, add, force_token, ban_token, k, out, eos_token, next_scores, next_tokens, next_beam_idx};
  const hipError_t e = kmb_beam_step_launch(p, scratch, scratch_floats > 0 ? (size_t)scratch_floats : 0, (hipStream_t)stream);
  if (e == hipErrorNotSupported)
    return kmb_set_error("kmb_beam_step: unsupported shape (k <= 16, num_beams <= 16, num_beams * k <= 256, ld %% 4 == 0, "
                         "scratch of kmb_logsoftmax_topk_scratch(B * num_beams) floats): use kmb_logsoftmax_topk_ws + kmb_beam_merge_select");
  return hipfail(e, "beam_step");
}
int kmb_logsoftmax_topk(const float* logits, int ld, int V, int rows, const float* add, int force_token, int ban_token,
                        int k, float* out_val, int32_t* out_idx, void* stream) {
  return hipfail(kmb_logsoftmax_topk_launch(logits, ld, V, rows, add, force_token, ban_token, k, out_val, out_idx, nullptr, 0,
                                            (hipStream_t)stream), "logsoftmax_topk");
}
int kmb_logsoftmax_topk_ws(const float* logits, int ld, int V, int rows, const float* add, int force_token, int ban_token,
                           int k, float* out_val, int32_t* out_idx, float* scratch, int64_t scratch_floats, void* stream) {
  return hipfail(kmb_logsoftmax_topk_launch(logits, ld, V, rows, add, force_token, ban_token, k, out_val, out_idx, scratch,
                                            scratch_floats > 0 ? (size_t)scratch_floats : 0, (hipStream_t)stream), "logsoftmax_topk");
}
int64_t kmb_logsoftmax_topk_scratch(int rows) { return (int64_t)kmb_logsoftmax_topk_scratch_floats(rows); }
int kmb_sample_step(const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p, int ban_token,
                    const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token, int64_t eos_token,
                    int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* info_out, void* stream) {
  if (kmb_sample_validate("kmb_sample_step", logits, ld, V, R, temperature, top_k, top_p, ban_token, noise, ld_noise, unfinished,
                          pad_token, eos_token, next_tokens, ids, t, ld_ids) != 0)
    return -1;
  return hipfail(kmb_sample_step_launch(logits, ld, V, R, temperature, top_k, top_p, ban_token, noise, ld_noise, unfinished,
                                        pad_token, eos_token, next_tokens, ids, t, ld_ids, flag, info_out, (hipStream_t)stream),
                 "sample_step");
}
int kmb_sample_scored_step(const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p, int ban_token,
                           const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token, int64_t eos_token,
                           int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* info_out, float* logprob_sum,
                           float* logprob_out, int ld_logprob, void* stream) {
  if (kmb_sample_validate("kmb_sample_scored_step", logits, ld, V, R, temperature, top_k, top_p, ban_token, noise, ld_noise,
                          unfinished, pad_token, eos_token, next_tokens, ids, t, ld_ids, logprob_out != nullptr, ld_logprob) != 0)
    return -1;
  return hipfail(kmb_sample_scored_step_launch(logits, ld, V, R, temperature, top_k, top_p, ban_token, noise, ld_noise, unfinished,
                                               pad_token, eos_token, next_tokens, ids, t, ld_ids, flag, info_out, logprob_sum,
                                               logprob_out, ld_logprob, (hipStream_t)stream),
                 "sample_scored_step");
}

int kmb_greedy_step(const float* logits, int ld, int V, int R, int ban_token, int64_t* unfinished, int64_t pad_token, int64_t eos_token,
                    int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* logprob_sum, float* logprob_out,
                    void* stream) {
  if (kmb_greedy_validate("kmb_greedy_step", logits, ld, V, R, ban_token, unfinished, pad_token, eos_token, next_tokens, ids, t,
                          ld_ids) != 0)
    return -1;
  return hipfail(kmb_greedy_step_launch(logits, ld, V, R, ban_token, unfinished, pad_token, eos_token, next_tokens, ids, t, ld_ids, flag,
                                        logprob_sum, logprob_out, (hipStream_t)stream),
                 "greedy_step");
}

int kmb_logits_process(float* logits, int ld, int V, int R, const int64_t* ids, int ld_ids, int t, float repetition_penalty,
                       int no_repeat_ngram_size, const int32_t* bad_tokens, const int32_t* bad_offsets, int n_bad, void* stream) {
  if (kmb_logits_process_validate("kmb_logits_process", logits, ld, V, R, ids, ld_ids, t, repetition_penalty, no_repeat_ngram_size,
                                  bad_tokens, bad_offsets, n_bad) != 0)
    return -1;
  return hipfail(kmb_logits_process_launch(logits, ld, V, R, ids, ld_ids, t, repetition_penalty, no_repeat_ngram_size, bad_tokens,
                                           bad_offsets, n_bad, (hipStream_t)stream),
                 "logits_process");
}

int kmb_cider_reward(const int64_t* ids, int ld, int B, int L, int pad_token, int bos_token, int eos_token, const int32_t* item_of_row,
                     int n_items, const int64_t* df_keys, const float* df_idf, const int64_t* df_offsets, float idf_miss,
                     const int32_t* item_ref_offsets, int n_refs, const int32_t* ref_len, const float* ref_norm,
                     const int32_t* ref_ng_offsets, const int64_t* ref_keys, const float* ref_w, int64_t n_ref_entries, int variant,
                     float sigma, float* out, void* stream) {
  if (!df_offsets) return kmb_set_error("kmb_cider_reward: df_offsets (host, 5 x int64) is required");
  KmbCiderTables t{n_items, (const uint64_t*)df_keys, df_idf, {df_offsets[0], df_offsets[1], df_offsets[2], df_offsets[3], df_offsets[4]},
                   idf_miss, item_ref_offsets, n_refs, ref_len, ref_norm, ref_ng_offsets, (const uint64_t*)ref_keys, ref_w, n_ref_entries};
  if (kmb_cider_reward_validate("kmb_cider_reward", ids, ld, B, L, item_of_row, t, variant, sigma, out) != 0) return -1;
  return hipfail(kmb_cider_reward_launch(ids, ld, B, L, pad_token, bos_token, eos_token, item_of_row, t, variant, sigma, out,
                                         (hipStream_t)stream),
                 "cider_reward");
}

int64_t kmb_beam_step_processed_scratch(int rows, int t, int n_bad) {
  return (int64_t)kmb_beam_step_processed_scratch_floats(rows, t, n_bad);
}
int kmb_beam_step_processed(const float* logits, int ld, int V, int B, int num_beams, const float* add, int force_token, int ban_token,
                            int k, int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx,
                            float* scratch, int64_t scratch_floats, const int64_t* ids_in, int64_t* ids_out, int ld_ids, int t,
                            float repetition_penalty, int no_repeat_ngram_size, const int32_t* bad_tokens, const int32_t* bad_offsets,
                            int n_bad, void* stream) {
  const KmbBeamProcess pr{ids_in, ids_out, ld_ids, t, repetition_penalty, no_repeat_ngram_size, bad_tokens, bad_offsets, n_bad};
  const KmbBeamStep p{logits, ld, V, B, num_beams, add, force_token, ban_token, k, out, eos_token, next_scores, next_tokens, next_beam_idx};
  if (kmb_beam_step_processed_validate("kmb_beam_step_processed", p, scratch, scratch_floats, pr) != 0) return -1;
  return hipfail(kmb_beam_step_processed_launch(p, scratch, (size_t)scratch_floats, pr, (hipStream_t)stream), "beam_step_processed");
}

int64_t kmb_beam_sample_scratch(int rows) { return (int64_t)kmb_beam_sample_scratch_floats(rows); }
int kmb_beam_sample_step(const float* logits, int ld, int V, int B, int num_beams, const float* add, float temperature, int top_k,
                         float top_p, int ban_token, const float* noise, int ld_noise, int k, int32_t* out, int eos_token,
                         float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, float* scratch, int64_t scratch_floats,
                         void* stream) {
  if (kmb_beam_sample_validate("kmb_beam_sample_step", logits, ld, V, B, num_beams, temperature, top_k, top_p, ban_token, noise,
                               ld_noise, k, out, eos_token, next_scores, next_tokens, next_beam_idx, scratch, scratch_floats) != 0)
    return -1;
  return hipfail(kmb_beam_sample_step_launch(logits, ld, V, B, num_beams, add, temperature, top_k, top_p, ban_token, noise, ld_noise,
                                             k, out, eos_token, next_scores, next_tokens, next_beam_idx, scratch, (size_t)scratch_floats,
                                             (hipStream_t)stream),
                 "beam_sample_step");
}

}  // extern "C"

// The argument checks of kmb_beam_step_processed and kmb_gen_beam_step_processed (`who` names the caller in the message): the
// processors' as kmb_logits_process_validate, the beam step's shape limits, and what the kernels index with.
int kmb_beam_step_processed_validate(const char* who, const KmbBeamStep& p, const float* scratch, int64_t scratch_floats,
                                     const KmbBeamProcess& pr) {
  char buf[256];
  auto bad = [&](const char* what) {
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return kmb_set_error(buf);
  };
  if (!p.logits || !p.out || !p.next_scores || !p.next_tokens || !p.next_beam_idx || !scratch || !pr.ids_in || !pr.ids_out)
    return bad("logits, out, next_scores, next_tokens, next_beam_idx, scratch, ids_in and ids_out are required");
  if (pr.ids_in == pr.ids_out) return bad("ids_in and ids_out must be two buffers");
  if (p.nb < 1 || p.nb > 16 || p.k < 1 || p.k > 16 || p.nb * p.k > 256)
    return bad("need 1 <= k <= 16, 1 <= num_beams <= 16 and num_beams * k <= 256");
  if (p.V < 1 || p.V > KMB_BEAM_EDIT_MAX_V || p.B < 0 || p.ld < p.V || (p.ld & 3) || p.ld > 4 * 4 * 13 * 256 || ((uintptr_t)p.logits & 15) ||
      (int64_t)p.B * p.nb > 65535)
    return bad("need 1 <= V <= 65536, B >= 0, B * num_beams <= 65535, V <= ld <= 53248, ld % 4 == 0 and 16-byte aligned logits");
  if (p.B > 0 && kmb_logits_process_validate(who, p.logits, p.ld, p.V, p.B * p.nb, pr.ids_in, pr.ld_ids, pr.t, pr.repetition_penalty,
                                             pr.no_repeat_ngram_size, pr.bad_tokens, pr.bad_offsets, pr.n_bad) != 0)
    return -1;
  if (pr.ld_ids <= pr.t) return bad("need ld_ids > t (column t is written)");
  if (p.force_token < -1 || p.force_token >= p.V) return bad("force_token must be -1 or a token id < V");
  if (p.ban_token < -1 || p.ban_token >= p.V) return bad("ban_token must be -1 or a token id < V");
  if (p.eos < -1 || p.eos >= p.V) return bad("eos_token must be -1 or a token id < V");
  if (scratch_floats < 0 || (size_t)scratch_floats < kmb_beam_step_processed_scratch_floats(p.B * p.nb, pr.t, pr.n_bad))
    return bad("scratch needs kmb_beam_step_processed_scratch(B * num_beams, t, n_bad) floats");
  return 0;
}

// The argument checks of kmb_beam_sample_step and kmb_gen_beam_sample_step (`who` names the caller in the message).
int kmb_beam_sample_validate(const char* who, const float* logits, int ld, int V, int B, int num_beams, float temperature, int top_k,
                             float top_p, int ban_token, const float* noise, int ld_noise, int k, const int32_t* out, int eos_token,
                             const float* next_scores, const int64_t* next_tokens, const int32_t* next_beam_idx, const float* scratch,
                             int64_t scratch_floats) {
  char buf[256];
  auto bad = [&](const char* what) {
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return kmb_set_error(buf);
  };
  if (!logits || !noise || !out || !next_scores || !next_tokens || !next_beam_idx || !scratch)
    return bad("logits, noise, out, next_scores, next_tokens, next_beam_idx and scratch are required");
  if (num_beams < 1 || k != 2 * num_beams || k > KMB_BEAM_SAMPLE_MAX_K) return bad("need k == 2 * num_beams <= 16");
  if (V < 1 || V > KMB_BEAM_SAMPLE_MAX_V || B < 0 || ld < V || ld_noise < num_beams * V)
    return bad("need 1 <= V <= 65536, B >= 0, ld >= V, ld_noise >= num_beams * V");
  if (scratch_floats < 0 || (size_t)scratch_floats < kmb_beam_sample_scratch_floats(B * num_beams))
    return bad("scratch needs kmb_beam_sample_scratch(B * num_beams) floats");
  if (!(temperature > 0.f) || std::isinf(temperature)) return bad("temperature must be finite and > 0");
  if (top_k < 0) return bad("top_k must be >= 0");
  if (!(top_p > 0.f && top_p <= 1.f)) return bad("top_p must lie in (0, 1]");
  if (ban_token < -1 || ban_token >= V) return bad("ban_token must be -1 or a token id < V");
  if (eos_token < -1 || eos_token >= V) return bad("eos_token must be -1 or a token id < V");
  return 0;
}

// The argument checks of kmb_sample_step, kmb_sample_scored_step and kmb_gen_sample_step (`who` names the caller in the message).
int kmb_sample_validate(const char* who, const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p,
                        int ban_token, const float* noise, int ld_noise, const int64_t* unfinished, int64_t pad_token,
                        int64_t eos_token, const int64_t* next_tokens, const int64_t* ids, int t, int ld_ids, bool has_logprob_out,
                        int ld_logprob) {
  char buf[256];
  auto bad = [&](const char* what) {
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return kmb_set_error(buf);
  };
  if (!logits || !noise || !next_tokens) return bad("logits, noise and next_tokens are required");
  if (V < 1 || V > KMB_SAMPLE_MAX_V || R < 0 || ld < V || ld_noise < V)
    return bad("need 1 <= V <= 65536, R >= 0, ld >= V, ld_noise >= V");
  if (!(temperature > 0.f) || std::isinf(temperature)) return bad("temperature must be finite and > 0");
  if (top_k < 0) return bad("top_k must be >= 0");
  if (!(top_p >= 0.f && top_p <= 1.f)) return bad("top_p must lie in [0, 1]");
  if (ban_token < -1 || ban_token >= V) return bad("ban_token must be -1 or a token id < V");
  if (unfinished && (pad_token < 0 || pad_token >= V || eos_token < -1 || eos_token >= V))
    return bad("pad_token must be a token id, eos_token -1 or a token id");
  if (ids && (t < 0 || t >= ld_ids)) return bad("need 0 <= t < ld_ids");
  if (has_logprob_out && ld_logprob < 1) return bad("need ld_logprob >= 1 with logprob_out");
  return 0;
}

// The argument checks of kmb_greedy_step and kmb_gen_greedy_step (`who` names the caller in the message).
int kmb_greedy_validate(const char* who, const float* logits, int ld, int V, int R, int ban_token, const int64_t* unfinished,
                        int64_t pad_token, int64_t eos_token, const int64_t* next_tokens, const int64_t* ids, int t, int ld_ids) {
  char buf[256];
  auto bad = [&](const char* what) {
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return kmb_set_error(buf);
  };
  if (!logits || !next_tokens) return bad("logits and next_tokens are required");
  if (V < 1 || R < 1 || ld < V) return bad("need V >= 1, R >= 1, ld >= V");
  if (ban_token < -1 || ban_token >= V) return bad("ban_token must be -1 or a token id < V");
  if (eos_token < -1 || eos_token >= V) return bad("eos_token must be -1 or a token id < V");
  if (unfinished && (pad_token < 0 || pad_token >= V)) return bad("pad_token must be a token id < V");
  if (ids && (t < 0 || t >= ld_ids)) return bad("need 0 <= t < ld_ids");
  return 0;
}

// The argument checks of kmb_logits_process and kmb_gen_logits_process (`who` names the caller in the message).
int kmb_logits_process_validate(const char* who, const float* logits, int ld, int V, int R, const int64_t* ids, int ld_ids, int t,
                                float repetition_penalty, int no_repeat_ngram_size, const int32_t* bad_tokens,
                                const int32_t* bad_offsets, int n_bad) {
  char buf[256];
  auto bad = [&](const char* what) {
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return kmb_set_error(buf);
  };
  if (!logits || !ids) return bad("logits and ids are required");
  if (V < 1 || R < 1 || ld < V) return bad("need V >= 1, R >= 1, ld >= V");
  if (t < 1 || t > KMB_PROCESS_MAX_T || ld_ids < t) return bad("need 1 <= t <= 1024 and ld_ids >= t");
  if (!(repetition_penalty >= 1.f) || std::isinf(repetition_penalty)) return bad("repetition_penalty must be finite and >= 1");
  if (no_repeat_ngram_size < 0) return bad("no_repeat_ngram_size must be >= 0");
  if (n_bad < 0 || n_bad > KMB_PROCESS_MAX_BAD) return bad("need 0 <= n_bad <= 4096");
  if (n_bad > 0 && (!bad_tokens || !bad_offsets)) return bad("bad_tokens and bad_offsets (n_bad + 1 of them) are required with n_bad > 0");
  return 0;
}

// The argument checks of kmb_cider_reward (`who` names the caller in the message).
int kmb_cider_reward_validate(const char* who, const int64_t* ids, int ld, int B, int L, const int32_t* item_of_row,
                              const KmbCiderTables& t, int variant, float sigma, const float* out) {
  char buf[256];
  auto bad = [&](const char* what) {
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return kmb_set_error(buf);
  };
  if (!ids || !item_of_row || !out) return bad("ids, item_of_row and out are required");
  if (!t.df_keys || !t.df_idf || !t.item_ref_offsets || !t.ref_len || !t.ref_norm || !t.ref_ng_offsets || !t.ref_keys || !t.ref_w)
    return bad("every table pointer is required (an empty table still has an allocation behind it)");
  if (B < 0) return bad("need B >= 0");
  if (L < 1 || L > KMB_CIDER_MAX_T || ld < L) return bad("need 1 <= L <= 256 (KMB_CIDER_MAX_T) and ld >= L");
  if (variant != KMB_CIDER_VARIANT_D && variant != KMB_CIDER_VARIANT_PLAIN) return bad("variant must be 0 (CIDEr-D) or 1 (plain CIDEr)");
  if (!(sigma > 0.f) || std::isinf(sigma)) return bad("sigma must be finite and > 0");
  if (t.n_items < 0 || t.n_refs < 0 || t.n_ref_entries < 0) return bad("need n_items >= 0, n_refs >= 0, n_ref_entries >= 0");
  if (t.df_offsets[0] != 0) return bad("df_offsets must start at 0");
  for (int n = 0; n < KMB_CIDER_ORDERS; ++n)
    if (t.df_offsets[n + 1] < t.df_offsets[n]) return bad("df_offsets must ascend");
  return 0;
}
