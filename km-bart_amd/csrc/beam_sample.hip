// Beam-sampling step of generate(do_sample=True, num_beams > 1): transformers 3.0.2 _generate_beam_search, sampling branch, as
// reached from the reference's generation CLI with --num_beams and --do_sample (src/generation.py:22-32).  Per batch item, one
// step: per beam row log_softmax -> EOS ban -> + beam score -> / temperature -> top-k -> top-p (min_tokens_to_keep = 2);
// torch.multinomial's 2 * num_beams draws without replacement over the item's num_beams * V filtered scores (the exponential
// race: the k largest s - log q, q the caller's Exp(1) noise); the draws sorted by score; the next beams (the first num_beams
// non-EOS draws); optionally the history-index reorder and the next step's embedding (beam_fold.h).  DESIGN.md section 6e.
//
// Two launches: one workgroup of 1024 lanes per beam row finds the row's at most k draws (scratch), then one small workgroup per
// batch item merges them.  No row is held in registers: a phase that needs the row streams it and recomputes the scores.
// Thresholds come from radix selects over the 48-bit rank key (sample_keys.h) with LDS histograms and integer atomics only; with
// top-k the candidates are collected into an LDS list in one pass and top-k, top-p and the draw run on that list.  Nothing
// depends on the order in which lanes arrive: identical inputs, identical bits.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "kernels.h"
#include "beam_fold.h"
#include "beam_sample.h"
#include "sample_keys.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kDigit = 12;
constexpr int kBins = 1 << kDigit;
constexpr int kBinsPerThread = kBins / kThreads;
constexpr int kList = 1024;     // live tokens kept in LDS after top-k
constexpr int kUnroll = 8;      // loads in flight per lane while streaming a row
constexpr int kMaxK = KMB_BEAM_SAMPLE_MAX_K;
constexpr int kMaxNb = KMB_BEAM_SAMPLE_MAX_K / 2;
constexpr int kRowFloats = KMB_BEAM_SAMPLE_ROW_FLOATS;   // one row's candidates in the scratch

struct Smem {
  uint32_t cnt[kBins];
  unsigned long long mass[kBins];
  uint32_t lkey[kList];
  uint16_t lidx[kList];
  uint32_t wc[kWaves], wc_ex[kWaves + 1];
  unsigned long long wm[kWaves], wm_ex[kWaves + 1];
  float wf[kWaves], wg[kWaves], wh[kWaves];
  uint32_t sel_bin, sel_cnt, n_list;
  unsigned long long sel_above_c, sel_above_m, sel_key;
  // the row's draws: score, race key, beam * V + token
  float cs[kMaxK], cz[kMaxK];
  int cf[kMaxK];
  uint32_t cn[1];
};

struct Args {
  const float* logits; int ld, V, nb; const float* add;
  float temperature; int top_k; float top_p; int ban;
  const float* noise; int ld_noise; int k;
  int32_t* out; int eos; float* next_scores; int64_t* next_tokens; int32_t* next_beam_idx;
};

// s = (log_softmax(x) with s[ban] = -inf + beam score) / T, the order of the host loop; NaN reads as -inf, -0 as +0
struct RowScore {
  float M, L, a, T;
  int ban;
  __device__ __forceinline__ float operator()(float x, int i) const {
    float v = (x - M) - L;
    if (i == ban) v = -INFINITY;
    v = v + a;
    if (T != 1.f) v = v / T;   // correctly rounded divide (hipcc's default for fp32 '/')
    if (v != v) v = -INFINITY;
    return v + 0.f;
  }
};

// f(x_i, i) for the tokens i < V of this lane: i = lane index + 1024 * j, kUnroll loads in flight
template <class F>
__device__ __forceinline__ void stream_row(const float* __restrict__ x, int V, F&& f) {
  for (int base = threadIdx.x; base < V; base += kThreads * kUnroll) {
    float v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int i = base + u * kThreads;
      v[u] = x[i < V ? i : V - 1];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int i = base + u * kThreads;
      if (i < V) f(v[u], i);
    }
  }
}

// (max, sum of exp(x - max)) pairs; symmetric in its arguments, so a butterfly leaves every lane the same bits
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const bool mine = m >= om;
  const float hi = mine ? m : om, lo = mine ? om : m;
  const float shi = (m == om) ? s : (mine ? s : os), slo = (m == om) ? os : (mine ? os : s);
  m = hi;
  s = lo == -INFINITY ? (m == om ? s + os : shi) : shi + slo * expf(lo - hi);
}

// Radix select over the rank keys of the tokens src visits (src(g) calls g(value key, index) for this lane's live tokens).
// In rank order (value descending, index ascending) token p is "in" iff p < P0 or, with use_mass, the softmax mass ranked before
// it (fixed point, relative to mx >= every value) is <= floor(top_p * total mass).  The in tokens form a prefix; returns the rank
// key of its last token (0: src visits nothing).  Up to four passes of 12 bits; a bin holding one token ends the search early.
template <class Src>
__device__ uint64_t select_rank(Smem& sh, Src&& src, float mx, int P0, bool use_mass, float top_p) {
  const int tid = threadIdx.x;
  uint64_t prefix = 0;
  unsigned long long c_above = 0, m_above = 0, W = 0;
  for (int pass = 0; pass < 4; ++pass) {
    for (int b = tid; b < kBins; b += kThreads) {
      sh.cnt[b] = 0;
      if (use_mass) sh.mass[b] = 0;
    }
    __syncthreads();
    const int sh_hi = 48 - kDigit * pass, sh_lo = sh_hi - kDigit;
    src([&](uint32_t key, int i) {
      const uint64_t rk = rank_key(key, i);
      if ((rk >> sh_hi) == prefix) {
        const int bin = (int)((rk >> sh_lo) & (kBins - 1));
        atomicAdd(&sh.cnt[bin], 1u);
        if (use_mass) atomicAdd(&sh.mass[bin], mass_fixed(key, mx));
      }
    });
    __syncthreads();
    // thread t reads bins kBins-1 - 4t .. kBins-4 - 4t: thread order is descending rank order
    uint32_t c[kBinsPerThread], cs = 0, ctot;
    unsigned long long m[kBinsPerThread], ms = 0, mtot;
#pragma unroll
    for (int q = 0; q < kBinsPerThread; ++q) {
      const int b = kBins - 1 - (tid * kBinsPerThread + q);
      c[q] = sh.cnt[b];
      m[q] = use_mass ? sh.mass[b] : 0ull;
      cs += c[q]; ms += m[q];
    }
    block_exscan(sh, cs, ms, ctot, mtot);
    if (ctot == 0) return 0;   // (pass 0 only: later passes hold the selected bin's tokens)
    if (pass == 0 && use_mass) W = (unsigned long long)floor((double)top_p * (double)mtot);
#pragma unroll
    for (int q = 0; q < kBinsPerThread; ++q) {
      // the bin's first token sits at c_above + cs with that much mass before it, the next bin's first at + c[q]
      const unsigned long long p0 = c_above + cs, e0 = m_above + ms, p1 = p0 + c[q], e1 = e0 + m[q];
      const bool in0 = p0 < (unsigned long long)P0 || (use_mass && e0 <= W);
      const bool in1 = p1 < (unsigned long long)P0 || (use_mass && e1 <= W);
      if (c[q] != 0 && in0 && (!in1 || cs + c[q] == ctot)) {   // exactly one bin of the pass
        sh.sel_bin = (uint32_t)(kBins - 1 - (tid * kBinsPerThread + q));
        sh.sel_cnt = c[q];
        sh.sel_above_c = cs;
        sh.sel_above_m = ms;
      }
      cs += c[q]; ms += m[q];
    }
    __syncthreads();
    prefix = (prefix << kDigit) | sh.sel_bin;
    c_above += sh.sel_above_c;
    m_above += sh.sel_above_m;
    const uint32_t n = sh.sel_cnt;
    __syncthreads();
    if (pass == 3) return prefix;
    if (n == 1) {   // the bin holds the token alone: one more visit finds its full key
      src([&](uint32_t key, int i) {
        const uint64_t rk = rank_key(key, i);
        if ((rk >> sh_lo) == prefix) sh.sel_key = rk;
      });
      __syncthreads();
      const uint64_t rk = sh.sel_key;
      __syncthreads();
      return rk;
    }
  }
  return prefix;
}

// Stage 1, one workgroup per beam row r = b * nb + j: the row's at most k draws (race key, score, j * V + token) into
// scratch[r * kRowFloats ..]: keys at [0, 16), scores at [16, 32), flat indices (int bits, -1: none) at [32, 48).
__global__ __launch_bounds__(kThreads) void beam_sample_row_kernel(const Args a, float* __restrict__ scratch) {
  __shared__ Smem sh;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, nb = a.nb, b = r / nb, j = r - b * nb;
  const float* x = a.logits + (size_t)r * a.ld;
  const float* qn = a.noise + (size_t)b * a.ld_noise + (size_t)j * V;
  // log-sum-exp over the row (the banned token included: the ban follows the normalisation); m2: the largest unbanned logit
  float m = -INFINITY, s = 0.f, m2 = -INFINITY;
  stream_row(x, V, [&](float v, int i) {
    if (v != v) return;
    if (i != a.ban) m2 = fmaxf(m2, v);
    if (v == -INFINITY) return;
    if (v > m) { s = s * expf(m - v) + 1.f; m = v; }
    else s += expf(v - m);
  });
  const float lane_max = m2;   // this lane's largest unbanned logit: the bound of the top-k candidates below
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    lse_merge(m, s, om, os);
    m2 = fmaxf(m2, __shfl_xor(m2, o, 64));
  }
  if (lane == 0) { sh.wf[w] = m; sh.wg[w] = s; sh.wh[w] = m2; }
  __syncthreads();
  m = sh.wf[0]; s = sh.wg[0]; m2 = sh.wh[0];
  for (int v = 1; v < kWaves; ++v) {
    lse_merge(m, s, sh.wf[v], sh.wg[v]);
    m2 = fmaxf(m2, sh.wh[v]);
  }
  const RowScore sf{m, logf(s), a.add != nullptr ? a.add[r] : 0.f, a.temperature, a.ban};
  const float smax = sf(m2, V);   // >= every score of the row (monotone in the logit; token V is never the banned one)
  auto all_src = [&](auto&& g) { stream_row(x, V, [&](float v, int i) { g(order_key(sf(v, i)), i); }); };

  // top-k (min_tokens_to_keep = 2): remove s < the k-th largest score -- ties with it stay
  const int keff = a.top_k > 0 ? min(max(a.top_k, 2), V) : V;
  uint32_t tk = 0;   // live: key >= tk (every real key is >= order_key(-inf) > 0)
  // Candidates first: the lanes' maxima are scores of distinct tokens, so at least keff tokens score >= the keff-th largest of
  // them (c0) and the keff best are among {s >= c0}, usually a few times keff tokens: one pass collects them into LDS and the
  // select runs there.  Without top-k, or when they do not fit, the selects stream the row.
  uint32_t c0 = 0;
  if (keff < V && keff <= kThreads) {
    sh.lkey[tid] = order_key(sf(lane_max, V));
    sh.lidx[tid] = (uint16_t)tid;
    __syncthreads();
    auto lanes_src = [&](auto&& g) { g(sh.lkey[tid], tid); };
    c0 = (uint32_t)(select_rank(sh, lanes_src, 0.f, keff, false, 0.f) >> 16);
  } else if (keff >= V && V <= kList) {
    c0 = 1;   // every token
  }
  bool listed = false;
  uint32_t nl = 0;
  if (c0 != 0) {
    if (tid == 0) sh.n_list = 0;
    __syncthreads();
    all_src([&](uint32_t key, int i) {
      if (key >= c0) {
        const uint32_t slot = atomicAdd(&sh.n_list, 1u);
        if (slot < (uint32_t)kList) { sh.lkey[slot] = key; sh.lidx[slot] = (uint16_t)i; }
      }
    });
    __syncthreads();
    nl = sh.n_list;
    listed = nl <= (uint32_t)kList;
  }
  auto list_src = [&](auto&& g) {
    for (int e = tid; e < (int)nl; e += kThreads) g(sh.lkey[e], (int)sh.lidx[e]);
  };
  if (keff < V) tk = (uint32_t)((listed ? select_rank(sh, list_src, 0.f, keff, false, 0.f)
                                        : select_rank(sh, all_src, 0.f, keff, false, 0.f)) >> 16);
  auto live_src = [&](auto&& g) {
    if (listed) {
      list_src([&](uint32_t key, int i) { if (key >= tk) g(key, i); });
    } else {
      all_src([&](uint32_t key, int i) { if (key >= tk) g(key, i); });
    }
  };
  // top-p over the live tokens: keep the first three by rank and every token whose mass ranked before it is <= top_p
  // (transformers' rm[..., :2] = 0 followed by the shift right)
  uint64_t cut = 0;   // kept: rank key >= cut
  if (a.top_p < 1.f) cut = select_rank(sh, live_src, smax, 3, true, a.top_p);
  // the draw: the k largest s - log q over the kept tokens (noise read there only), ties to the lower index
  auto race = [&](uint32_t key, int i) {
    float z = key_value(key) - logf(qn[i]);
    if (z != z) z = -INFINITY;
    return z + 0.f;
  };
  auto draw_src = [&](auto&& g) {
    live_src([&](uint32_t key, int i) { if (rank_key(key, i) >= cut) g(order_key(race(key, i)), i); });
  };
  const uint64_t thr = select_rank(sh, draw_src, 0.f, a.k, false, 0.f);
  if (tid == 0) sh.cn[0] = 0;
  __syncthreads();
  live_src([&](uint32_t key, int i) {
    if (rank_key(key, i) < cut) return;
    const float z = race(key, i);
    if (rank_key(order_key(z), i) >= thr) {   // at most k tokens (rank keys are unique)
      const uint32_t slot = atomicAdd(&sh.cn[0], 1u);
      if (slot < (uint32_t)kMaxK) { sh.cs[slot] = key_value(key); sh.cz[slot] = z; sh.cf[slot] = j * V + i; }
    }
  });
  __syncthreads();
  if (tid < kMaxK) {   // (slot order follows the atomics; the merge orders by (key, flat index))
    const bool in = tid < (int)min(sh.cn[0], (uint32_t)kMaxK);
    float* o = scratch + (size_t)r * kRowFloats;
    o[tid] = in ? sh.cz[tid] : -INFINITY;
    o[kMaxK + tid] = in ? sh.cs[tid] : -INFINITY;
    o[2 * kMaxK + tid] = __int_as_float(in ? sh.cf[tid] : -1);
  }
}

// Stage 2, one workgroup of 64 * nb lanes per batch item: the item's k draws from its rows' candidates, sorted by score, the next
// beams, and the folded reorder / embedding.
__global__ __launch_bounds__(64 * kMaxNb) void beam_sample_merge_kernel(const Args a, const float* __restrict__ scratch,
                                                                         const KmbHistGather hg, const KmbEmbedNext en) {
  __shared__ float cand[kMaxNb * kRowFloats];
  __shared__ float dz[kMaxK], ds[kMaxK];
  __shared__ int dq[kMaxK], df[kMaxK];
  __shared__ int32_t snext[32];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = a.V, nb = a.nb;
  for (int e = tid; e < nb * kRowFloats; e += blockDim.x) cand[e] = scratch[(size_t)b * nb * kRowFloats + e];
  __syncthreads();
  if (w == 0) {
    // torch.multinomial's draw order: the item's k largest race keys, ties to the lower flat index.  Lane l holds candidates l and
    // l + 64 (row e / 16, slot e % 16) as 64-bit keys (race key order | ~flat index; 0: none); a draw is one wave maximum.
    unsigned long long key[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int e = lane + 64 * q, at = (e / kMaxK) * kRowFloats + (e % kMaxK);
      const int f = e < nb * kMaxK ? __float_as_int(cand[at + 2 * kMaxK]) : -1;
      key[q] = f >= 0 ? ((unsigned long long)order_key(cand[at]) << 32) | (0xffffffffu - (uint32_t)f) : 0ull;
    }
    for (int d = 0; d < a.k; ++d) {
      unsigned long long best = key[0] > key[1] ? key[0] : key[1];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ob = __shfl_xor(best, o, 64);
        best = ob > best ? ob : best;
      }
      if (best == 0ull) {   // fewer kept tokens than draws (degenerate rows): defined, never a real continuation
        if (lane == 0) { ds[d] = -INFINITY; df[d] = 0; }
        continue;
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        if (key[q] == best) {   // unique: the flat index is part of the key
          const int e = lane + 64 * q;
          ds[d] = cand[(e / kMaxK) * kRowFloats + kMaxK + (e % kMaxK)];
          df[d] = (int)(0xffffffffu - (uint32_t)best);
          key[q] = 0ull;
        }
      }
    }
  }
  __syncthreads();
  // sorted by score, descending; ties keep the draw order: draw d goes to its rank
  if (tid < a.k) {
    const float sv = ds[tid];
    int rank = 0;
    for (int e = 0; e < a.k; ++e) rank += (ds[e] > sv || (ds[e] == sv && e < tid)) ? 1 : 0;
    dz[rank] = sv;
    dq[rank] = df[tid];
  }
  __syncthreads();
  if (tid == 0) {
    // candidates for the host's bookkeeping, and the next beams: in order, the first nb draws whose token is not EOS
    int n_sel = 0;
    for (int d = 0; d < a.k; ++d) {
      const float sv = dz[d];
      const int f = dq[d], beam = f / V, tok = f - beam * V;
      a.out[((size_t)b * a.k + d) * 2] = __float_as_int(sv);
      a.out[((size_t)b * a.k + d) * 2 + 1] = f;
      if (n_sel < nb && tok != a.eos) {
        snext[n_sel] = b * nb + beam; snext[16 + n_sel] = tok;
        const size_t o = (size_t)b * nb + n_sel++;
        a.next_scores[o] = sv; a.next_tokens[o] = tok; a.next_beam_idx[o] = b * nb + beam;
      }
    }
    for (; n_sel < nb; ++n_sel) {   // cannot happen with k = 2 * nb (at most one EOS draw per beam); keep the rows defined
      snext[n_sel] = b * nb; snext[16 + n_sel] = a.eos >= 0 ? a.eos : 0;
      const size_t o = (size_t)b * nb + n_sel;
      a.next_scores[o] = -1e9f; a.next_tokens[o] = a.eos >= 0 ? a.eos : 0; a.next_beam_idx[o] = b * nb;
    }
  }
  if (w == 0) beam_hist_gather(hg, snext, b, nb, lane);
  beam_embed_next(en, snext, b, nb, w, lane);
}

}  // namespace

size_t kmb_beam_sample_scratch_floats(int rows) { return (size_t)(rows > 0 ? rows : 0) * kRowFloats; }

hipError_t kmb_beam_sample_step_launch(const float* logits, int ld, int V, int B, int nb, const float* add, float temperature,
                                       int top_k, float top_p, int ban_token, const float* noise, int ld_noise, int k, int32_t* out,
                                       int eos, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, float* scratch,
                                       size_t scratch_floats, hipStream_t stream, const KmbHistGather* hist, const KmbEmbedNext* embed) {
  if (nb < 1 || k != 2 * nb || k > KMB_BEAM_SAMPLE_MAX_K || V < 1 || V > KMB_BEAM_SAMPLE_MAX_V) return hipErrorNotSupported;
  if (B <= 0) return hipSuccess;
  if (!logits || !noise || !out || !next_scores || !next_tokens || !next_beam_idx) return hipErrorInvalidValue;
  if (!scratch || scratch_floats < kmb_beam_sample_scratch_floats(B * nb)) return hipErrorInvalidValue;
  const KmbHistGather hg = hist != nullptr ? *hist : KmbHistGather{nullptr, nullptr, 0, 0};
  const KmbEmbedNext en = embed != nullptr ? *embed : KmbEmbedNext{};
  if (en.E != nullptr && ((en.D & 7) || en.D > 1024 || en.D <= 512)) return hipErrorInvalidValue;   // embed_ln_row<2>
  const Args a{logits, ld, V, nb, add, temperature, top_k, top_p, ban_token, noise, ld_noise, k, out, eos, next_scores,
               next_tokens, next_beam_idx};
  hipLaunchKernelGGL(beam_sample_row_kernel, dim3(B * nb), dim3(kThreads), 0, stream, a, scratch);
  hipLaunchKernelGGL(beam_sample_merge_kernel, dim3(B), dim3(64 * nb), 0, stream, a, (const float*)scratch, hg, en);
  return hipGetLastError();
}
