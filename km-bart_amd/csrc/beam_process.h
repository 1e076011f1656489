// The beam step with generate()'s score processors on the device (C-ABI kmb_beam_step_processed, kmb_gen_beam_step_processed;
// DESIGN.md section 6n): csrc/beam_process.hip writes every beam row's edit set, csrc/beam_step.hip's EDIT forms of the beam step's two
// launches consume it.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"
#include "logits_process.h"

constexpr int KMB_BEAM_EDIT_MAX_V = 65536;   // the edit launch resolves "a ban wins over a penalty" in an LDS bitmap over the vocabulary

// The processors' arguments of a step: the rows' tokens ids_in [rows, ld_ids] int64, columns [0, t); ids_out [rows, ld_ids] receives
// the next beams' histories, columns [0, t].  repetition_penalty / no_repeat_ngram_size / bad words as kmb_logits_process.
struct KmbBeamProcess {
  const int64_t* ids_in; int64_t* ids_out; int ld_ids, t;
  float repetition_penalty; int no_repeat_ngram_size;
  const int32_t* bad_tokens; const int32_t* bad_offsets; int n_bad;
};

// What the combine / merge launch needs of it: the edit lists (ew words per row), the penalty, the two id buffers.
struct KmbBeamEdit {
  const int32_t* edit; int ew, t;
  float p, inv_p; int penalise;
  const int64_t* ids_in; int64_t* ids_out; int ld_ids;
};

// A row's edit list, int32 words, a token or -1 in every slot: [0, t) the penalised tokens that no ban hits (slot j: the token at
// position j when that is its first occurrence), [t, 2 t) the tokens the n-grams ban (slot j: the window at j), [2 t, 2 t + n_bad)
// the tokens the bad words ban.  The min_length ban_token stays the part kernel's own `ban`; a penalised ban_token is dropped here.
inline int kmb_beam_edit_words(int t, int n_bad) { return 2 * (t > 0 ? t : 0) + (n_bad > 0 ? n_bad : 0); }

// One workgroup per row r < rows: edit[r * kmb_beam_edit_words(t, n_bad) ...] from ids_in.  Arguments already validated.
hipError_t kmb_beam_edit_launch(const KmbBeamProcess& pr, int V, int rows, int ban_token, int32_t* edit, hipStream_t stream);

size_t kmb_beam_step_processed_scratch_floats(int rows, int t, int n_bad);
// kmb_beam_step_launch's arguments and contract (hist / embed: the decode loop's folded reorder and embedding) plus the processors.
// hipErrorNotSupported: a shape outside kmb_beam_step's limits, V > 65536, or too little scratch.
hipError_t kmb_beam_step_processed_launch(const KmbBeamStep& p, float* scratch, size_t scratch_floats, const KmbBeamProcess& pr,
                                          hipStream_t stream);

// The argument checks of kmb_beam_step_processed and kmb_gen_beam_step_processed (`who` names the caller in the message; capi_ops.cpp).
int kmb_beam_step_processed_validate(const char* who, const KmbBeamStep& p, const float* scratch, int64_t scratch_floats,
                                     const KmbBeamProcess& pr);
