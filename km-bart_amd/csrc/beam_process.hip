// The edit sets of a beam step with generate()'s score processors: for every beam row, which tokens the
// repetition penalty scales and which the no-repeat n-grams, the bad words and min_length ban -- the row rule of logits_process.hip
// (process_row.h), written out as a list instead of applied, because beam search edits log-probabilities: the beam step's part
// kernel (beam_step.hip) drops the listed tokens from its selection and the combine launch brings the penalised ones back with their
// scaled score.
//
// One workgroup of 256 lanes per row, the row's t tokens in LDS.  Bans first, into the list and into an LDS bitmap over the
// vocabulary (V <= 65536; LDS atomics); behind a barrier the penalised tokens, without those the bitmap holds: a ban wins over a
// penalty.  Every slot of the list is written, -1 where it names nothing: the list has one writer per word and no counters, plain
// stores to global memory.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "beam_process.h"
#include "process_row.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBitWords = KMB_BEAM_EDIT_MAX_V / 32;

struct EditArgs {
  const int64_t* ids; int ld_ids, t, V, R;
  int penalise, n, ban;
  const int32_t* bad_tokens; const int32_t* bad_offsets; int n_bad;
  int32_t* edit; int ew;
};

__global__ __launch_bounds__(kThreads) void beam_edit_kernel(EditArgs a) {
  __shared__ int tok[KMB_PROCESS_MAX_T];
  __shared__ int kept;
  __shared__ uint32_t banned[kBitWords];
  const int r = blockIdx.x, tid = threadIdx.x;
  int32_t* out = a.edit + (size_t)r * a.ew;
  for (int i = tid; i < kBitWords; i += kThreads) banned[i] = 0u;
  const int t = process_row_load<kThreads>(a.ids + (size_t)r * a.ld_ids, a.t, a.V, tok, &kept, tid);
  __syncthreads();   // the bitmap is clear (process_row_load has a barrier of its own; this one does not rely on it)

  if (tid == 0 && a.ban >= 0) atomicOr(&banned[a.ban >> 5], 1u << (a.ban & 31));
  const int n = a.n;
  for (int j = tid; j < a.t; j += kThreads) {
    int x = -1;
    if (n > 0 && j + n <= t && process_row_ngram(tok, t, n, j)) x = tok[j + n - 1];
    out[a.t + j] = x;
    if (x >= 0) atomicOr(&banned[x >> 5], 1u << (x & 31));
  }
  for (int s = tid; s < a.n_bad; s += kThreads) {
    const int x = process_row_bad_word(tok, t, a.V, a.R, a.bad_tokens, a.bad_offsets, s);
    out[2 * a.t + s] = x;
    if (x >= 0) atomicOr(&banned[x >> 5], 1u << (x & 31));
  }
  __syncthreads();

  for (int j = tid; j < a.t; j += kThreads) {
    int x = -1;
    if (a.penalise && j < t) {
      const int c = tok[j];
      if (!((banned[c >> 5] >> (c & 31)) & 1u) && process_row_first(tok, j)) x = c;
    }
    out[j] = x;
  }
}

}  // namespace

hipError_t kmb_beam_edit_launch(const KmbBeamProcess& pr, int V, int rows, int ban_token, int32_t* edit, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (pr.t < 1 || pr.t > KMB_PROCESS_MAX_T || V < 1 || V > KMB_BEAM_EDIT_MAX_V || ban_token >= V) return hipErrorInvalidValue;
  EditArgs a{pr.ids_in, pr.ld_ids, pr.t, V, rows, pr.repetition_penalty != 1.0f ? 1 : 0, pr.no_repeat_ngram_size, ban_token,
             pr.bad_tokens, pr.bad_offsets, pr.n_bad, edit, kmb_beam_edit_words(pr.t, pr.n_bad)};
  hipLaunchKernelGGL(beam_edit_kernel, dim3(rows), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}
