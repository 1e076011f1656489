// Launcher of the greedy tail of generate(num_beams=1, do_sample=False) (csrc/greedy.hip; C-ABI kmb_greedy_step, kmb_gen_greedy_step).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

// The argument checks of kmb_greedy_step and kmb_gen_greedy_step (`who` names the caller in the message; capi_ops.cpp).
int kmb_greedy_validate(const char* who, const float* logits, int ld, int V, int R, int ban_token, const int64_t* unfinished,
                        int64_t pad_token, int64_t eos_token, const int64_t* next_tokens, const int64_t* ids, int t, int ld_ids);

// One workgroup per row r < R of logits [R, ld] (fp32): EOS ban, argmax (lowest index on ties), the chosen token's
// log-probability, finished-row bookkeeping.  Arguments as kmb_greedy_step (include/kmbart.h), already validated.
// embed (optional; D % 8 == 0, D <= 1024): the same launch embeds the chosen tokens for the next decode step, row r of
// embed->y (kmb_embed_ln_fwd_launch's work on next_tokens, bit-identical rows); hipErrorNotSupported for another D.
hipError_t kmb_greedy_step_launch(const float* logits, int ld, int V, int R, int ban_token, int64_t* unfinished, int64_t pad_token,
                                  int64_t eos_token, int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag,
                                  float* logprob_sum, float* logprob_out, hipStream_t stream, const KmbEmbedNext* embed = nullptr);
