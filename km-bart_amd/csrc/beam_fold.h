// The work a beam step folds into the launch that has just chosen the next beams (the decode loop's reorder and embedding):
// shared by beam_step.hip's beam steps and beam_sample.hip's beam sampling step.  snext: LDS, the item's nb chosen beam rows in
// [0, 16), their tokens in [16, 32), written by lane 0 of wave 0.
#pragma once
#include "common.h"
#include "kernels.h"
#include "embed_row.h"

namespace {
// The beam reorder of the self-attention caches' history index (optim.hip gather_hist_kernel: dst[r][t] = src[next_beam_idx[r]][t], t < nt)
// for the item's nb rows, by the wave that has just chosen them: the decode loop's reorder launch folded into its beam step (round 6).
__device__ __forceinline__ void beam_hist_gather(const KmbHistGather& hg, const int32_t* snext, int b, int nb, int lane) {
  if (hg.dst == nullptr) return;
  __builtin_amdgcn_wave_barrier();   // snext was written by lane 0 of this wave
  for (int e = lane; e < nb * hg.nt; e += 64) {
    const int i = e / hg.nt, t = e - i * hg.nt;
    hg.dst[(size_t)(b * nb + i) * hg.ld + t] = hg.src[(size_t)snext[i] * hg.ld + t];
  }
}

// ... and the next decode step's input rows: embedding of the chosen tokens + position + LayerNorm (embed.hip's embed_ln_fwd_kernel, the
// same row code: embed_row.h), one wave per beam row; all the workgroup's threads call this (it has a barrier)
__device__ __forceinline__ void beam_embed_next(const KmbEmbedNext& en, const int32_t* snext, int b, int nb, int wave, int lane) {
  if (en.E == nullptr) return;
  __syncthreads();   // snext[16 ..] was written by wave 0
  if (wave < nb) {
    const int row = b * nb + wave;
    int tok = snext[16 + wave];
    tok = tok < 0 ? 0 : (tok >= en.V ? en.V - 1 : tok);   // (a real column unless V < k; never read outside the table)
    embed_ln_row<2>(en.E + (size_t)tok * en.D, en.prow, en.scale, en.gamma, en.beta, nullptr, en.y, nullptr, nullptr, row,
                    en.D, en.eps, KmbDrop{0u, 0u, 1.f}, lane);
  }
}
}  // namespace
