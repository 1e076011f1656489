// Launchers of the sampling tail of generate(do_sample=True, num_beams=1) (csrc/sample.hip; C-ABI kmb_sample_step,
// kmb_sample_scored_step, kmb_gen_sample_step).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

// Largest vocabulary one workgroup holds in registers (1024 lanes x 64 values; token ids fit 16 bits).
#define KMB_SAMPLE_MAX_V 65536

// One workgroup per row r < R of logits [R, ld] (fp32): EOS ban, temperature, top-k, top-p, exponential-race draw on
// noise [R, ld_noise], finished-row bookkeeping.  Arguments as kmb_sample_step (include/kmbart.h), already validated;
// hipErrorNotSupported for V > KMB_SAMPLE_MAX_V.
hipError_t kmb_sample_step_launch(const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p,
                                  int ban_token, const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token,
                                  int64_t eos_token, int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag,
                                  float* info_out, hipStream_t stream);

// The argument checks of kmb_sample_step, kmb_sample_scored_step and kmb_gen_sample_step (`who` names the caller in the message;
// capi_ops.cpp).  has_logprob_out: the scored forms pass logprob_out != NULL, and ld_logprob must then be >= 1.
int kmb_sample_validate(const char* who, const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p,
                        int ban_token, const float* noise, int ld_noise, const int64_t* unfinished, int64_t pad_token,
                        int64_t eos_token, const int64_t* next_tokens, const int64_t* ids, int t, int ld_ids, bool has_logprob_out = false,
                        int ld_logprob = 1);

// The scored form, same launch count and the same tokens: also the chosen token's log-probability under the distribution it was drawn
// from (after the ban, the temperature, top-k and top-p) -- logprob_sum[r] += lp for the rows unfinished on entry, logprob_out[r *
// ld_logprob] = lp (0 for a finished row), either may be NULL.  embed (optional; D % 8 == 0, D <= 1024): the same launch embeds the
// chosen tokens for the next decode step, row r of embed->y (kmb_embed_ln_fwd_launch's work on next_tokens, bit-identical rows);
// hipErrorNotSupported for another D.
hipError_t kmb_sample_scored_step_launch(const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p,
                                         int ban_token, const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token,
                                         int64_t eos_token, int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag,
                                         float* info_out, float* logprob_sum, float* logprob_out, int ld_logprob, hipStream_t stream,
                                         const KmbEmbedNext* embed = nullptr);
