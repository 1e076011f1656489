// Sampling tail of generate(do_sample=True, num_beams=1): transformers 3.0.2 _generate_no_beam_search as reached from the
// reference's nucleus-sampling mode (src/generation.py:22-32, vcg_generate.py:97-106), per row in one launch:
// EOS ban -> / temperature -> top-k -> top-p -> softmax -> exponential-race draw -> finished-row bookkeeping
// [-> the chosen token's log-probability under the filtered distribution -> the next step's embedding] (the scored form).
//
// One workgroup of 1024 lanes per row; the row stays in registers (NPER values per lane, token i = j * 1024 + lane).
// Both thresholds come from a radix select over a 48-bit rank key (order-preserving value key << 16 | 0xffff - index:
// descending key = the order of a stable descending sort), four 12-bit digits, histograms in LDS with integer atomics
// only: a count histogram finds the k-th token of top-k, a mass histogram (fixed point, 2^-40 units) the cut of top-p.
// Nothing depends on the order in which lanes arrive, so the same inputs give the same token bits.  DESIGN.md section 6d.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "embed_row.h"
#include "sample.h"
#include "sample_keys.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kDigit = 12;
constexpr int kBins = 1 << kDigit;
constexpr int kBinsPerThread = kBins / kThreads;
constexpr int kNone = 0x7fffffff;

struct SampleArgs {
  const float* logits; int ld, V;
  float temperature; int top_k; float top_p; int ban_token;
  const float* noise; int ld_noise;
  int64_t* unfinished; int64_t pad_token, eos_token;
  int64_t* next_tokens; int64_t* ids; int t, ld_ids;
  int32_t* flag; float* info_out;
  float* logprob_sum; float* logprob_out; int ld_logprob;   // the scored form only
  KmbEmbedNext en;
};

struct Smem {
  uint32_t cnt[kBins];
  unsigned long long mass[kBins];
  uint32_t wc[kWaves], wc_ex[kWaves + 1];
  unsigned long long wm[kWaves], wm_ex[kWaves + 1];
  float wmax[kWaves], wf[kWaves];
  int wi[kWaves];
  uint32_t sel_bin, sel_cnt, sel_key;
  int sel_idx;
  unsigned long long sel_above;
  float wsum[kWaves];     // the scored form: a wave's kept mass and the key of its best token
  uint32_t wkey[kWaves];
};

// A new name for the lane index in every phase: nothing derived from it (a token index, a 64-bit address offset) is
// computed once and kept live in registers for a later phase -- hipcc would otherwise hold one such value per token
// across the whole kernel and spill.
template <int NPER>
__device__ __forceinline__ void fence_keys(uint32_t (&key)[NPER]) {
#pragma unroll
  for (int j = 0; j < NPER; ++j) asm volatile("" : "+v"(key[j]));
}
__device__ __forceinline__ int fresh_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

// Digit PASS (0..3, 12 bits each, most significant first) of the rank key of token i with value key k, and whether the
// token's rank key begins with `prefix` (the 12 * PASS bits chosen before).  Spelled per pass on 32-bit halves: a 64-bit
// key per register value would be loop-invariant and kept live across the passes.
template <int PASS>
__device__ __forceinline__ bool digit_of(uint32_t k, int i, uint64_t prefix, int& bin) {
  const uint32_t inv = (uint32_t)(0xffff - i);
  if (PASS == 0) { bin = (int)(k >> 20); return true; }
  if (PASS == 1) { bin = (int)((k >> 8) & 0xfffu); return (k >> 20) == (uint32_t)prefix; }
  if (PASS == 2) { bin = (int)(((k & 0xffu) << 4) | (inv >> 12)); return (k >> 8) == (uint32_t)prefix; }
  bin = (int)(inv & 0xfffu);
  return k == (uint32_t)(prefix >> 4) && (inv >> 12) == (uint32_t)(prefix & 0xfu);
}

// One pass of the radix select over the tokens with key != 0 (see select_rank).  Returns true when the search
// has ended: `prefix` then holds the selected token's full rank key.
template <int NPER, bool kMass, int PASS>
__device__ __forceinline__ bool select_pass(Smem& sh, uint32_t (&key)[NPER], float mx,
                                            unsigned long long& want, float top_p, uint64_t& prefix) {
  const int tid = fresh_tid();
  fence_keys(key);
  for (int b = tid; b < kBins; b += kThreads) {
    sh.cnt[b] = 0;
    if (kMass) sh.mass[b] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    int bin;
    // key 0 (no token) lands in bin 0 of pass 0, which the scan skips, and never matches a chosen prefix: real keys are
    // >= order_key(-inf) = 0x007fffff
    if (digit_of<PASS>(key[j], j * kThreads + tid, prefix, bin)) {
      atomicAdd(&sh.cnt[bin], 1u);
      if (kMass) atomicAdd(&sh.mass[bin], mass_fixed(key[j], mx));
    }
  }
  __syncthreads();
  // thread t reads bins kBins-1 - 4t .. kBins-4 - 4t: thread order is descending rank order
  uint32_t c[kBinsPerThread], cs = 0, ctot;
  unsigned long long m[kBinsPerThread], ms = 0, mtot;
#pragma unroll
  for (int q = 0; q < kBinsPerThread; ++q) {
    const int b = kBins - 1 - (tid * kBinsPerThread + q);
    c[q] = (PASS == 0 && b == 0) ? 0u : sh.cnt[b];
    m[q] = (!kMass || (PASS == 0 && b == 0)) ? 0ull : sh.mass[b];
    cs += c[q]; ms += m[q];
  }
  block_exscan(sh, cs, ms, ctot, mtot);
  if (kMass && PASS == 0) want = (unsigned long long)floor((double)top_p * (double)mtot);
#pragma unroll
  for (int q = 0; q < kBinsPerThread; ++q) {
    // exactly one bin of the pass holds the selected token
    const bool hit = kMass ? (c[q] != 0 && ms <= want && (ms + m[q] > want || cs + c[q] == ctot))
                           : (c[q] != 0 && cs < want && want <= cs + c[q]);
    if (hit) {
      sh.sel_bin = (uint32_t)(kBins - 1 - (tid * kBinsPerThread + q));
      sh.sel_cnt = c[q];
      sh.sel_above = kMass ? ms : cs;
    }
    cs += c[q]; ms += m[q];
  }
  __syncthreads();
  prefix = (prefix << kDigit) | sh.sel_bin;
  want -= sh.sel_above;
  if (PASS == 3) return true;
  if (sh.sel_cnt != 1) return false;
  // the bin holds the selected token alone: its key ends the search
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const int i = j * kThreads + tid;
    int bin;
    if (digit_of<PASS + 1 < 4 ? PASS + 1 : 3>(key[j], i, prefix, bin)) { sh.sel_key = key[j]; sh.sel_idx = i; }
  }
  __syncthreads();
  prefix = rank_key(sh.sel_key, sh.sel_idx);
  return true;
}

// Radix select over the rank keys of the tokens with key != 0; returns the rank key of the selected token.
// kMass = false: the want-th token (1-based).  kMass = true: the last token whose exclusive mass (sum of mass_fixed over
// the tokens ranked before it) is <= floor(top_p * total mass).
template <int NPER, bool kMass>
__device__ __forceinline__ uint64_t select_rank(Smem& sh, uint32_t (&key)[NPER], float mx,
                                                unsigned long long want, float top_p) {
  uint64_t prefix = 0;
  if (select_pass<NPER, kMass, 0>(sh, key, mx, want, top_p, prefix)) return prefix;
  if (select_pass<NPER, kMass, 1>(sh, key, mx, want, top_p, prefix)) return prefix;
  if (select_pass<NPER, kMass, 2>(sh, key, mx, want, top_p, prefix)) return prefix;
  select_pass<NPER, kMass, 3>(sh, key, mx, want, top_p, prefix);
  return prefix;
}

// kScored: also lp = log(m_tok / sum of m_i over the kept tokens), m = rel_exp, the masses the draw itself uses -- summed in the
// draw loop, which already visits every kept token once, per lane in ascending j, by a butterfly inside the wave (a + b == b + a: every
// lane holds the same bits) and over the waves in wave order: a fixed order, no floating-point atomics.  The row maximum is always kept
// and has mass 1, so the sum is >= 1 and lp <= 0; log(m_tok) is taken as x_tok - max (0 at the maximum itself, infinite or not).
// Then wave 0 embeds the chosen token for the next decode step (a.en.E != nullptr; NCH as kmb_embed_ln_fwd_launch picks it).
template <int NPER, bool kScored, int NCH>
__global__ __launch_bounds__(kThreads) void sample_step_kernel(SampleArgs a) {
  __shared__ Smem sh;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* row = a.logits + (size_t)r * a.ld;
  uint32_t key[NPER];
  {
    float x[NPER];
#pragma unroll
    for (int j = 0; j < NPER; ++j) x[j] = row[min(j * kThreads + tid, a.V - 1)];   // every load in flight at once
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPER; ++j) {
      const int i = j * kThreads + tid;
      float v = x[j];
      if (i == a.ban_token || v != v) v = -INFINITY;
      if (a.temperature != 1.f) v = v / a.temperature;   // correctly rounded divide (hipcc's default for fp32 '/')
      v += 0.f;
      key[j] = i < a.V ? order_key(v) : 0u;
      if (i < a.V) mx = fmaxf(mx, v);
    }
    mx = wave_max(mx);
    if (lane == 0) sh.wmax[w] = mx;
  }
  __syncthreads();
  float mx = sh.wmax[0];
#pragma unroll
  for (int v = 1; v < kWaves; ++v) mx = fmaxf(mx, sh.wmax[v]);

  // top-k (model.py _top_k_top_p_filtering): remove x < the k-th largest value -- ties with it stay
  const int k = a.top_k < a.V ? a.top_k : a.V;
  if (k > 0 && k < a.V) {
    const uint32_t t_k = (uint32_t)(select_rank<NPER, false>(sh, key, mx, (unsigned long long)k, 0.f) >> 16);
#pragma unroll
    for (int j = 0; j < NPER; ++j) key[j] = key[j] < t_k ? 0u : key[j];   // removed tokens leave the row
  }
  // top-p over the survivors: keep a token iff the mass ranked before it is <= top_p (the first token always)
  uint64_t cut = rank_key(1u, 0xffff);   // below every real token, above key 0
  if (a.top_p < 1.f) cut = select_rank<NPER, true>(sh, key, mx, 0ull, a.top_p);

  // draw: argmax over the kept tokens of p / q, p = softmax over them; q is read at kept tokens only
  const float* q = a.noise + (size_t)r * a.ld_noise;
  const uint32_t cut_key = (uint32_t)(cut >> 16), cut_inv = (uint32_t)(cut & 0xffffu);
  uint32_t n = 0, kmin = 0xffffffffu, bestk = 0;
  float best = -INFINITY, msum = 0.f;
  int besti = kNone;
  const int lt = fresh_tid();
  fence_keys(key);
#pragma unroll
  for (int j = 0; j < NPER; ++j) {
    const int i = j * kThreads + lt;
    if (key[j] > cut_key || (key[j] == cut_key && (uint32_t)(0xffff - i) >= cut_inv)) {
      ++n;
      kmin = min(kmin, key[j]);
      const float m = rel_exp(key[j], mx);
      float v = m / q[i];
      if (v != v) v = -INFINITY;
      if (kScored) {
        msum += m;
        if (v > best || besti == kNone) bestk = key[j];
      }
      if (v > best || besti == kNone) { best = v; besti = i; }   // i ascends with j: the lowest index wins a tie
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n += __shfl_xor(n, o, 64);
    kmin = min(kmin, __shfl_xor(kmin, o, 64));
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(besti, o, 64);
    const bool take = oi != kNone && (besti == kNone || ob > best || (ob == best && oi < besti));
    if (kScored) {
      msum += __shfl_xor(msum, o, 64);
      const uint32_t ok = __shfl_xor(bestk, o, 64);
      if (take) bestk = ok;
    }
    if (take) { best = ob; besti = oi; }
  }
  if (lane == 0) {
    sh.wc[w] = n; sh.wm[w] = kmin; sh.wf[w] = best; sh.wi[w] = besti;
    if (kScored) { sh.wsum[w] = msum; sh.wkey[w] = bestk; }
  }
  __syncthreads();
  if (kScored ? w != 0 : tid != 0) return;
  int tok32 = 0;
  if (lane == 0) {
    for (int v = 1; v < kWaves; ++v) {
      n += sh.wc[v];
      kmin = min(kmin, (uint32_t)sh.wm[v]);
      const float ob = sh.wf[v];
      const int oi = sh.wi[v];
      const bool take = oi != kNone && (besti == kNone || ob > best || (ob == best && oi < besti));
      if (kScored) {
        msum += sh.wsum[v];
        if (take) bestk = sh.wkey[v];
      }
      if (take) { best = ob; besti = oi; }
    }
    int64_t tok = besti;   // the top token is always kept: a real column
    bool live = true;
    if (a.unfinished) {
      int64_t u = a.unfinished[r];
      live = u != 0;
      if (!u) tok = a.pad_token;
      u = (u && tok != a.eos_token) ? 1 : 0;
      a.unfinished[r] = u;
      if (u && a.flag) atomicOr(a.flag, 1);
    } else if (a.flag) {
      atomicOr(a.flag, 1);
    }
    a.next_tokens[r] = tok;
    if (a.ids) a.ids[(size_t)r * a.ld_ids + a.t] = tok;
    if (a.info_out) { a.info_out[2 * r] = (float)n; a.info_out[2 * r + 1] = key_value(kmin); }
    if (kScored) {
      const float x = key_value(bestk);
      const float lp = live ? (x == mx ? 0.f : x - mx) - logf(msum) : 0.f;
      if (a.logprob_sum && live) a.logprob_sum[r] += lp;
      if (a.logprob_out) a.logprob_out[(size_t)r * a.ld_logprob] = lp;
    }
    tok32 = (int)tok;
  }
  if (!kScored) return;
  // the next decode step's input row, by this wave (greedy.hip's tail)
  if (a.en.E == nullptr) return;
  int etok = __shfl(tok32, 0, 64);
  etok = etok < 0 ? 0 : (etok >= a.en.V ? a.en.V - 1 : etok);   // never read outside the table
  embed_ln_row<NCH>(a.en.E + (size_t)etok * a.en.D, a.en.prow, a.en.scale, a.en.gamma, a.en.beta, nullptr, a.en.y, nullptr, nullptr, r,
                    a.en.D, a.en.eps, KmbDrop{0u, 0u, 1.f}, lane);
}

template <bool kScored, int NCH>
void launch_for(int V, int R, const SampleArgs& a, hipStream_t stream) {
  if (V <= 16 * kThreads)
    hipLaunchKernelGGL((sample_step_kernel<16, kScored, NCH>), dim3(R), dim3(kThreads), 0, stream, a);
  else if (V <= 52 * kThreads)   // vcg_base: 50 320
    hipLaunchKernelGGL((sample_step_kernel<52, kScored, NCH>), dim3(R), dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((sample_step_kernel<64, kScored, NCH>), dim3(R), dim3(kThreads), 0, stream, a);
}

}  // namespace

hipError_t kmb_sample_step_launch(const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p,
                                  int ban_token, const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token,
                                  int64_t eos_token, int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag,
                                  float* info_out, hipStream_t stream) {
  if (V > KMB_SAMPLE_MAX_V) return hipErrorNotSupported;
  if (R <= 0) return hipSuccess;
  const SampleArgs a{logits, ld, V, temperature, top_k, top_p, ban_token, noise, ld_noise, unfinished, pad_token, eos_token,
                     next_tokens, ids, t, ld_ids, flag, info_out, nullptr, nullptr, 0, KmbEmbedNext{}};
  launch_for<false, 1>(V, R, a, stream);
  return hipGetLastError();
}

hipError_t kmb_sample_scored_step_launch(const float* logits, int ld, int V, int R, float temperature, int top_k, float top_p,
                                         int ban_token, const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token,
                                         int64_t eos_token, int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag,
                                         float* info_out, float* logprob_sum, float* logprob_out, int ld_logprob, hipStream_t stream,
                                         const KmbEmbedNext* embed) {
  if (V > KMB_SAMPLE_MAX_V) return hipErrorNotSupported;
  if (R <= 0) return hipSuccess;
  SampleArgs a{logits, ld, V, temperature, top_k, top_p, ban_token, noise, ld_noise, unfinished, pad_token, eos_token,
               next_tokens, ids, t, ld_ids, flag, info_out, logprob_sum, logprob_out, ld_logprob, KmbEmbedNext{}};
  if (embed != nullptr && embed->E != nullptr) {
    if ((embed->D & 7) || embed->D < 8 || embed->D > 1024) return hipErrorNotSupported;
    a.en = *embed;
  }
  // the chunk count of kmb_embed_ln_fwd_launch for this width: the rows must come out with the same bits
  if (a.en.E != nullptr && a.en.D > 512)
    launch_for<true, 2>(V, R, a, stream);
  else
    launch_for<true, 1>(V, R, a, stream);
  return hipGetLastError();
}
