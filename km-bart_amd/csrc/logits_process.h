// Launcher of generate()'s score processors on the device (csrc/logits_process.hip; C-ABI kmb_logits_process,
// kmb_gen_logits_process): repetition penalty, no-repeat n-grams and bad words on one decode step's logits, in place.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int KMB_PROCESS_MAX_T = 1024;     // tokens of a row the kernel holds in LDS
constexpr int KMB_PROCESS_MAX_BAD = 4096;   // bad-word sequences of a table

// The argument checks of kmb_logits_process and kmb_gen_logits_process (`who` names the caller in the message; capi_ops.cpp).
int kmb_logits_process_validate(const char* who, const float* logits, int ld, int V, int R, const int64_t* ids, int ld_ids, int t,
                                float repetition_penalty, int no_repeat_ngram_size, const int32_t* bad_tokens,
                                const int32_t* bad_offsets, int n_bad);

// One workgroup per row r < R of logits [R, ld] (fp32), edited in place from the row's tokens ids[r * ld_ids + 0 .. t).
// Arguments as kmb_logits_process (include/kmbart.h), already validated.
hipError_t kmb_logits_process_launch(float* logits, int ld, int V, int R, const int64_t* ids, int ld_ids, int t,
                                     float repetition_penalty, int no_repeat_ngram_size, const int32_t* bad_tokens,
                                     const int32_t* bad_offsets, int n_bad, hipStream_t stream);
