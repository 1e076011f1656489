// Launcher of the sampling tail of generate(do_sample=True, num_beams=1) (csrc/sample.hip; C-ABI kmb_sample_step).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// Largest vocabulary one workgroup holds in registers (1024 lanes x 64 values; token ids fit 16 bits).
#define KMB_SAMPLE_MAX_V 65536

// One workgroup per row r < R of logits [R, ld] (fp32): EOS ban, temperature, top-k, top-p, exponential-race draw on
// noise [R, ld_noise], finished-row bookkeeping.  Arguments as kmb_sample_step (include/kmbart.h), already validated;
// hipErrorNotSupported for V > KMB_SAMPLE_MAX_V.
hipError_t kmb_sample_step_launch(const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p,
                                  int ban_token, const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token,
                                  int64_t eos_token, int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag,
                                  float* info_out, hipStream_t stream);
