// CIDEr / CIDEr-D over token ids (Vedantam et al. 2015; the -D form with the clipped numerator and the Gaussian length penalty):
// one score per row of a [B, L] id matrix against reference tables in device memory, ONE launch, no host synchronisation.
//
//   g_x,n(w) = count_x(w) * idf_n(w);  s_n(h, r) = sum_{w in h} num(g_h(w), g_r(w)) / (||g_h,n|| ||g_r,n||), 0 when a norm is 0,
//   num = min(g_h, g_r) * g_r (D) or g_h * g_r (plain);  pen = exp(-(L_h - L_r)^2 / (2 sigma^2)) (D) or 1 (plain);
//   score = (10 / m) sum_r pen * 1/4 sum_n s_n over the m references of the row's item, 0 when m = 0.
//
// One workgroup of 256 lanes per row, lane j owns hypothesis position j (L <= KMB_CIDER_MAX_T = 256).
//   A  the token rule (cider_row.h) leaves the row's T scored tokens in LDS.
//   B  per order n: the T - n + 1 keys go to LDS; a compare sweep over them gives position j its n-gram's multiplicity and
//      whether j is the n-gram's first occurrence (no sort); first occurrences look the idf up by binary search in the order's
//      df slice (idf_miss when absent) and keep g_h = count * idf in LDS, every other position keeps 0.  The four ||g_h,n||^2
//      are reduced over the workgroup: a shuffle tree inside a wave, the four waves' partials added in one fixed order.
//   C  the references of the item are dealt to the four WAVES (reference k to wave k % 4), so a reference costs no barrier: a
//      lane walks its four positions, looks each non-zero g_h's key up in the reference's (reference, order) slice and adds
//      the numerator to the order's accumulator; a shuffle tree per order, then s_n, the penalty, and the wave's running sum.
//   D  the four waves' sums (each reference entered as pen * 0.25 * sum_n s_n), added in one fixed order, times 10 / m.
// fp32 throughout, no atomics, every sum in a fixed order: the same input gives the same bits.  The kernel computes no
// logarithm (the tables hold idf and count * idf) and one expf per reference.  An item index outside [0, N), an item without
// references and an empty hypothesis score 0 and read no table.  DESIGN.md section 6r.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "cider_reward.h"
#include "cider_row.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kCiderWave;
constexpr int kPerLane = KMB_CIDER_MAX_T / kCiderWave;   // hypothesis positions of a lane in phase C
static_assert(KMB_CIDER_MAX_T <= kThreads, "one lane per column");

struct CiderArgs {
  const int64_t* ids; int ld, L; int pad, bos, eos;
  const int32_t* item_of_row;
  KmbCiderTables t;
  int plain; float neg_inv_2s2;
  float* out;
};

// sum over the 64 lanes of a wave, the same tree on every launch; every lane gets the result
__device__ __forceinline__ float wave_sum(float v) {
  for (int d = kCiderWave / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, kCiderWave);
  return v;
}

__global__ __launch_bounds__(kThreads) void cider_reward_kernel(CiderArgs a) {
  __shared__ int tok[KMB_CIDER_MAX_T];
  __shared__ uint64_t keys[KMB_CIDER_ORDERS][KMB_CIDER_MAX_T];
  __shared__ float gh[KMB_CIDER_ORDERS][KMB_CIDER_MAX_T];
  __shared__ int scratch[2 * kWaves];
  __shared__ float part[kWaves][KMB_CIDER_ORDERS];
  __shared__ float wave_total[kWaves];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & (kCiderWave - 1), wave = tid / kCiderWave;
  const KmbCiderTables& t = a.t;

  // every test below is uniform over the workgroup: all of its lanes leave together, in front of the barriers
  const int item = a.item_of_row[row];
  int r0 = 0, m = 0;
  if (item >= 0 && item < t.n_items) {
    r0 = t.item_ref_offsets[item];
    m = t.item_ref_offsets[item + 1] - r0;
  }
  if (m <= 0 || r0 < 0 || (int64_t)r0 + m > (int64_t)t.n_refs) {
    if (tid == 0) a.out[row] = 0.f;
    return;
  }
  const int T = cider_row_load<kThreads>(a.ids + (size_t)row * a.ld, a.L, a.pad, a.bos, a.eos, tok, scratch, tid);
  if (T == 0) {
    if (tid == 0) a.out[row] = 0.f;
    return;
  }

  // B: keys, multiplicities, first occurrences, g_h and its norms
  for (int n = 1; n <= KMB_CIDER_ORDERS; ++n) keys[n - 1][tid] = tid + n <= T ? cider_key_pack(tok, tid, n) : 0;
  __syncthreads();
  float sq[KMB_CIDER_ORDERS];
  for (int n = 1; n <= KMB_CIDER_ORDERS; ++n) {
    const int M = T - n + 1;       // n-grams of this order (<= 0: none)
    float g = 0.f;
    if (tid < M) {
      const uint64_t key = keys[n - 1][tid];
      int count = 0;
      bool first = true;
      for (int i = 0; i < M; ++i) {
        const bool eq = keys[n - 1][i] == key;
        count += eq ? 1 : 0;
        first = first && !(eq && i < tid);
      }
      if (first) {
        const int64_t lo = t.df_offsets[n - 1];
        const int64_t at = cider_search(t.df_keys + lo, t.df_offsets[n] - lo, key);
        g = (float)count * (at >= 0 ? t.df_idf[lo + at] : t.idf_miss);
      }
    }
    gh[n - 1][tid] = g;
    sq[n - 1] = wave_sum(g * g);
  }
  if (lane == 0)
    for (int n = 0; n < KMB_CIDER_ORDERS; ++n) part[wave][n] = sq[n];
  __syncthreads();
  float norm_h[KMB_CIDER_ORDERS];
  for (int n = 0; n < KMB_CIDER_ORDERS; ++n) norm_h[n] = sqrtf((part[0][n] + part[1][n]) + (part[2][n] + part[3][n]));

  // C: reference k of the item belongs to wave k % kWaves
  float mine = 0.f;
  for (int k = wave; k < m; k += kWaves) {
    const int r = r0 + k;
    float acc[KMB_CIDER_ORDERS];
    for (int n = 0; n < KMB_CIDER_ORDERS; ++n) {
      acc[n] = 0.f;
      const float nr = t.ref_norm[(size_t)r * KMB_CIDER_ORDERS + n];
      if (!(norm_h[n] > 0.f) || !(nr > 0.f)) continue;          // uniform over the wave
      const int lo = t.ref_ng_offsets[(size_t)r * KMB_CIDER_ORDERS + n];
      const int cnt = t.ref_ng_offsets[(size_t)r * KMB_CIDER_ORDERS + n + 1] - lo;
      if (lo < 0 || cnt <= 0 || (int64_t)lo + cnt > t.n_ref_entries) continue;
      float s = 0.f;
      for (int q = 0; q < kPerLane; ++q) {
        const int j = lane + q * kCiderWave;
        const float g = gh[n][j];
        if (g > 0.f) {
          const int64_t at = cider_search(t.ref_keys + lo, cnt, keys[n][j]);
          if (at >= 0) {
            const float gr = t.ref_w[lo + at];
            s += a.plain ? g * gr : fminf(g, gr) * gr;
          }
        }
      }
      acc[n] = wave_sum(s) / (norm_h[n] * nr);
    }
    float pen = 1.f;
    if (!a.plain) {
      const int d = T - t.ref_len[r];
      pen = expf((float)(d * d) * a.neg_inv_2s2);
    }
    mine += pen * (0.25f * ((acc[0] + acc[1]) + (acc[2] + acc[3])));
  }
  if (lane == 0) wave_total[wave] = mine;
  __syncthreads();
  if (tid == 0) a.out[row] = ((wave_total[0] + wave_total[1]) + (wave_total[2] + wave_total[3])) * (10.f / (float)m);
}

}  // namespace

hipError_t kmb_cider_reward_launch(const int64_t* ids, int ld, int B, int L, int pad_token, int bos_token, int eos_token,
                                   const int32_t* item_of_row, const KmbCiderTables& t, int variant, float sigma, float* out,
                                   hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  CiderArgs a{ids, ld, L, pad_token, bos_token, eos_token, item_of_row, t, variant == KMB_CIDER_VARIANT_PLAIN ? 1 : 0,
              (float)(-1.0 / (2.0 * (double)sigma * (double)sigma)), out};
  hipLaunchKernelGGL(cider_reward_kernel, dim3(B), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}
