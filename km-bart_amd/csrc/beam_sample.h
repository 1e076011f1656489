// Launcher of the beam-sampling step of generate(do_sample=True, num_beams > 1) (csrc/beam_sample.hip; C-ABI kmb_beam_sample_step,
// kmb_gen_beam_sample_step).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

// Largest number of draws per batch item (k = 2 * num_beams) and vocabulary (token ids fit the 16-bit index of the rank key).
#define KMB_BEAM_SAMPLE_MAX_K 16
#define KMB_BEAM_SAMPLE_MAX_V 65536
// Scratch floats per beam row: its at most 16 draws (race key, score, flat index).
#define KMB_BEAM_SAMPLE_ROW_FLOATS 48

size_t kmb_beam_sample_scratch_floats(int rows);
// The C-ABI's argument checks (capi_ops.cpp): 0, or non-zero with kmb_last_error set to "<who>: <what is wrong>".
int kmb_beam_sample_validate(const char* who, const float* logits, int ld, int V, int B, int num_beams, float temperature, int top_k,
                             float top_p, int ban_token, const float* noise, int ld_noise, int k, const int32_t* out, int eos_token,
                             const float* next_scores, const int64_t* next_tokens, const int32_t* next_beam_idx, const float* scratch,
                             int64_t scratch_floats);

// Two launches.  One workgroup per row of logits [B * num_beams, ld] (fp32, V real columns): log-softmax, EOS ban, + add[row],
// / temperature, top-k / top-p, and the row's at most k draws of the exponential race on noise [B, ld_noise] (column
// beam * V + token) into scratch (kmb_beam_sample_scratch_floats(B * nb) floats).  Then one workgroup per batch item: its k
// draws, sorted by score, and the next beams.  Arguments as kmb_beam_sample_step (include/kmbart.h), already validated;
// hist / embed as kmb_beam_step_launch.  hipErrorNotSupported: k != 2 * num_beams, k > KMB_BEAM_SAMPLE_MAX_K or
// V > KMB_BEAM_SAMPLE_MAX_V.
hipError_t kmb_beam_sample_step_launch(const float* logits, int ld, int V, int B, int nb, const float* add, float temperature,
                                       int top_k, float top_p, int ban_token, const float* noise, int ld_noise, int k, int32_t* out,
                                       int eos, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, float* scratch,
                                       size_t scratch_floats, hipStream_t stream, const KmbHistGather* hist = nullptr,
                                       const KmbEmbedNext* embed = nullptr);
