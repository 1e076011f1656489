// generate()'s score processors on one decode step's logits, in place: transformers 3.0.2 postprocess_next_token_scores as
// the one-beam loops apply it (model.py _postprocess_next_token_scores, in its order) -- repetition penalty, then the bans of
// no_repeat_ngram_size and bad_words_ids.  The min_length EOS ban stays the ban_token of the greedy / sampling step behind it.
//
// One workgroup of 256 lanes per row.  The row's t tokens go into LDS as int32 (t <= 1024); a token outside [0, V) is dropped
// from the row as if it had never been generated.  The edit touches at most t words for the penalty, t for the n-gram bans
// and n_bad for the bad words: nothing streams over [R, V].
//   A  penalty p != 1: every DISTINCT token of the row once -- position j acts only when no i < j holds the same token, so a
//      word has one writer: v < 0 ? v * p : v * (1 / p), the reciprocal taken once in fp32 (what torch's device kernel computes
//      for tensor / python_scalar).
//   -- barrier: a token can be penalised and banned --
//   B  bans, -inf: idempotent stores, any order.  n-grams (n > 0, t + 1 >= n): every j <= t - n whose n - 1 tokens equal the
//      row's last n - 1 bans the token behind them.  Bad word s with head s[:-1]: s[-1] is banned when the head is empty, or
//      len(head) <= R (the reference's length test against the number of ROWS) and len(head) <= t and the row ends with it.
// No atomics, plain stores.  Columns >= V and every word not named above keep their bits.  DESIGN.md section 6m.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "logits_process.h"
#include "process_row.h"

namespace {

constexpr int kThreads = 256;

struct ProcessArgs {
  float* logits; int ld, V, R;
  const int64_t* ids; int ld_ids, t;
  float p, inv_p; int penalise, n;
  const int32_t* bad_tokens; const int32_t* bad_offsets; int n_bad;
};

__global__ __launch_bounds__(kThreads) void logits_process_kernel(ProcessArgs a) {
  __shared__ int tok[KMB_PROCESS_MAX_T];
  __shared__ int kept;
  const int r = blockIdx.x, tid = threadIdx.x;
  float* row = a.logits + (size_t)r * a.ld;
  const int t = process_row_load<kThreads>(a.ids + (size_t)r * a.ld_ids, a.t, a.V, tok, &kept, tid);

  if (a.penalise) {
    for (int j = tid; j < t; j += kThreads) {
      if (process_row_first(tok, j)) {
        const int x = tok[j];
        const float v = row[x];
        row[x] = v < 0.f ? v * a.p : v * a.inv_p;
      }
    }
  }
  __syncthreads();

  const int n = a.n;
  if (n > 0 && t + 1 >= n) {
    for (int j = tid; j + n <= t; j += kThreads)
      if (process_row_ngram(tok, t, n, j)) row[tok[j + n - 1]] = -INFINITY;
  }
  for (int s = tid; s < a.n_bad; s += kThreads) {
    const int last = process_row_bad_word(tok, t, a.V, a.R, a.bad_tokens, a.bad_offsets, s);
    if (last >= 0) row[last] = -INFINITY;
  }
}

}  // namespace

hipError_t kmb_logits_process_launch(float* logits, int ld, int V, int R, const int64_t* ids, int ld_ids, int t,
                                     float repetition_penalty, int no_repeat_ngram_size, const int32_t* bad_tokens,
                                     const int32_t* bad_offsets, int n_bad, hipStream_t stream) {
  if (R <= 0) return hipSuccess;
  if (t < 1 || t > KMB_PROCESS_MAX_T) return hipErrorInvalidValue;
  ProcessArgs a{logits, ld, V, R, ids, ld_ids, t, repetition_penalty, 1.0f / repetition_penalty, repetition_penalty != 1.0f ? 1 : 0,
                no_repeat_ngram_size, bad_tokens, bad_offsets, n_bad};
  hipLaunchKernelGGL(logits_process_kernel, dim3(R), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}
