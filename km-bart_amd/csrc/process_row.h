// The row rule of generate()'s score processors, shared by logits_process.hip (one beam: the logits are edited in place) and
// beam_process.hip (beams: the row's edit set is written out for the beam step): a row's tokens in LDS as int32, which of them
// are penalised (the first occurrence of each), which tokens the no-repeat n-grams ban (window compare) and which the bad
// words ban (tail compare).  transformers 3.0.2 postprocess_next_token_scores; DESIGN.md sections 6m and 6n.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "logits_process.h"

namespace {

// The row's t tokens idr[0 .. t) into tok[] (LDS, KMB_PROCESS_MAX_T ints); a token outside [0, V) is dropped from the row as if
// it had never been generated (one lane closes the gaps, in order).  Returns the number of tokens kept.  Every thread of the
// workgroup calls this (barriers); tok[] is complete on return.  kept: one LDS int.
template <int THREADS>
__device__ __forceinline__ int process_row_load(const int64_t* __restrict__ idr, int t_in, int V, int* tok, int* kept, int tid) {
  int outside = 0;
  for (int j = tid; j < t_in; j += THREADS) {
    const int64_t v = idr[j];
    const bool in = v >= 0 && v < (int64_t)V;
    tok[j] = in ? (int)v : -1;
    outside |= in ? 0 : 1;
  }
  int t = t_in;
  if (__syncthreads_or(outside)) {
    // tokens outside the vocabulary (never from generate()): one lane closes the gaps, in order
    if (tid == 0) {
      int w = 0;
      for (int j = 0; j < t_in; ++j) {
        const int x = tok[j];
        if (x >= 0) tok[w++] = x;
      }
      *kept = w;
    }
    __syncthreads();
    t = *kept;
  }
  return t;
}

// position j holds the first occurrence of its token: the penalty acts once per distinct token
__device__ __forceinline__ bool process_row_first(const int* tok, int j) {
  const int x = tok[j];
  for (int i = 0; i < j; ++i)
    if (tok[i] == x) return false;
  return true;
}

// no_repeat_ngram_size n > 0, j + n <= t: the n - 1 tokens from j equal the row's last n - 1 -- tok[j + n - 1] is banned
__device__ __forceinline__ bool process_row_ngram(const int* tok, int t, int n, int j) {
  const int tail = t + 1 - n;          // the row's last n - 1 tokens start here
  for (int k = 0; k < n - 1; ++k)
    if (tok[j + k] != tok[tail + k]) return false;
  return true;
}

// Bad word s with head s[:-1]: s[-1] is banned when the head is empty, or len(head) <= R (the reference's length test against
// the number of ROWS) and len(head) <= t and the row ends with it.  Returns the banned token, -1 for none.
__device__ __forceinline__ int process_row_bad_word(const int* tok, int t, int V, int R, const int32_t* __restrict__ bad_tokens,
                                                    const int32_t* __restrict__ bad_offsets, int s) {
  const int b = bad_offsets[s], e = bad_offsets[s + 1];
  if (b < 0 || e <= b) return -1;      // an empty sequence: the packer refuses it
  const int last = bad_tokens[e - 1], h = e - b - 1;
  if (last < 0 || last >= V) return -1;
  if (h == 0) return last;
  if (h > R || h > t) return -1;
  for (int k = 0; k < h; ++k)
    if (tok[t - h + k] != bad_tokens[b + k]) return -1;
  return last;
}

}  // namespace
