// Generation's selection kernels on fp32 logits: per row log_softmax + top-k (one workgroup per row, or the row split into parts
// and combined), the beam merge per batch item, and the fused beam steps of the decode loop -- plain, with generate()'s score
// processors, and from the all-rows vocabulary projection's block statistics.  Candidates are ordered by
// (value desc, index asc) everywhere.
#include "common.h"
#include "kernels.h"
#include "row_lse.h"
#include "beam_fold.h"
#include "beam_process.h"

namespace {

// Candidates are 64-bit keys: (order-preserving bits of the value) << 32 | (0x7fffffff - index), so "larger key" IS
// (value desc, index asc) and every comparison is one branch-free unsigned compare.  (The first version compared
// value and index with short-circuit logic: the compiler turned each element of a rescan into branches, 5.5 us
// per round.)  Key 0 = no element.
__device__ __forceinline__ unsigned long long topk_key(float v, int i) {
  const uint32_t b = __float_as_uint(v);
  const uint32_t ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)ord << 32) | (uint32_t)(0x7fffffff - i);
}
__device__ __forceinline__ float topk_key_value(unsigned long long key) {
  const uint32_t ord = (uint32_t)(key >> 32);
  return __uint_as_float((ord & 0x80000000u) ? (ord & 0x7fffffffu) : ~ord);
}
__device__ __forceinline__ int topk_key_index(unsigned long long key) { return 0x7fffffff - (int)(uint32_t)key; }
// the winner of a selection round as it is written out: no element left (key 0) reads -inf at index 0x7fffffff
__device__ __forceinline__ float topk_winner_value(unsigned long long wk) { return wk != 0ull ? topk_key_value(wk) : -INFINITY; }
__device__ __forceinline__ int topk_winner_index(unsigned long long wk) { return wk != 0ull ? topk_key_index(wk) : 0x7fffffff; }

// Per row: logp = log_softmax(row) (or the forced-token distribution), then the k best of logp + add[row] in
// (value desc, index asc) order.  Thread t owns elements t, t+256, ...; it keeps its own best in registers, a round
// is one block-wide arg-max over those 256 candidates, and only the winner's wave rescans the winner's ~V/256
// elements (64 lanes wide, from L2) for its next candidate -- the row is swept 3 times in total instead of k+2.
__global__ __launch_bounds__(256) void logsoftmax_topk_kernel(const float* __restrict__ logits, int ldv, int V,
                                                              const float* __restrict__ add, int force_token,
                                                              int ban, int k, float* __restrict__ out_val,
                                                              int32_t* __restrict__ out_idx) {
  __shared__ float sh[8];
  __shared__ float shv[4];
  __shared__ int shi[4];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const float* row = logits + (size_t)r * ldv;
  const float a = add != nullptr ? add[r] : 0.f;
  if (force_token >= 0) {
    // every other logit is -inf: log_softmax is 0 at the forced token, -inf elsewhere (ties in index order)
    for (int j = tid; j < k; j += 256) {
      out_val[(size_t)r * k + j] = j == 0 ? a : -INFINITY;
      out_idx[(size_t)r * k + j] = j == 0 ? force_token : (j - 1 < force_token ? j - 1 : j);
    }
    return;
  }
  float m, s;
  row_lse(row, V, sh, m, s);
  const float lse = m + __logf(s);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  // `ban`: that token scores -inf AFTER the normalisation (the log-sum-exp above includes it)
  for (int i = tid; i < V; i += 256) {
    const float x = i == ban ? -INFINITY : row[i];
    if (x > bv || bi == 0x7fffffff) { bv = x; bi = i; }
  }
  for (int j = 0; j < k; ++j) {
    float wv = bv;
    int wi = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v2 = __shfl_xor(wv, o, 64);
      const int i2 = __shfl_xor(wi, o, 64);
      if (v2 > wv || (v2 == wv && i2 < wi)) { wv = v2; wi = i2; }
    }
    if (lane == 0) { shv[tid >> 6] = wv; shi[tid >> 6] = wi; }
    __syncthreads();
    wv = shv[0]; wi = shi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (shv[w] > wv || (shv[w] == wv && shi[w] < wi)) { wv = shv[w]; wi = shi[w]; }
    __syncthreads();
    if (tid == 0) {
      out_val[(size_t)r * k + j] = (wv - lse) + a;
      out_idx[(size_t)r * k + j] = wi;
    }
    if (wi == 0x7fffffff) continue;  // fewer than k elements in the row
    const int owner = wi & 255;
    if ((tid >> 6) == (owner >> 6)) {  // wave-uniform: the owner's wave finds the owner's next candidate
      float nv = -INFINITY;
      int ni = 0x7fffffff;
      for (int i = owner + 256 * lane; i < V; i += 256 * 64) {
        const float x = i == ban ? -INFINITY : row[i];
        const bool after = (x < wv) || (x == wv && i > wi);
        if (after && (x > nv || ni == 0x7fffffff || (x == nv && i < ni))) { nv = x; ni = i; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(nv, o, 64);
        const int i2 = __shfl_xor(ni, o, 64);
        if (i2 != 0x7fffffff && (ni == 0x7fffffff || v2 > nv || (v2 == nv && i2 < ni))) { nv = v2; ni = i2; }
      }
      if (tid == owner) { bv = nv; bi = ni; }
    }
  }
}

// Register-resident form (rows of up to NV * 4096 columns): 1024 threads hold the fp32 row, so the logits are read
// from memory ONCE -- max, sum-exp, every thread's candidate and the owner's rescans all come from registers (the
// 256-thread form above sweeps the row three times and rescans from L2; 102 us -> per decode step at 320 rows).
// Thread t owns the float4 chunks t, t + 1024, ...; same (value desc, index asc) order.
template <int NV>
__global__ __launch_bounds__(1024) void logsoftmax_topk_reg_kernel(const float* __restrict__ logits, int ldv, int V,
                                                                   const float* __restrict__ add, int force_token,
                                                                   int ban, int k, float* __restrict__ out_val,
                                                                   int32_t* __restrict__ out_idx) {
  __shared__ float sh[32];
  __shared__ float shv[16];
  __shared__ int shi[16];
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* row = logits + (size_t)r * ldv;
  const float a = add != nullptr ? add[r] : 0.f;
  if (force_token >= 0) {
    for (int j = tid; j < k; j += 1024) {
      out_val[(size_t)r * k + j] = j == 0 ? a : -INFINITY;
      out_idx[(size_t)r * k + j] = j == 0 ? force_token : (j - 1 < force_token ? j - 1 : j);
    }
    return;
  }
  f32x4 x[NV];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = (tid + 1024 * j) * 4;
    if (i < ldv) {
      x[j] = *reinterpret_cast<const f32x4*>(row + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (i + e >= V) x[j][e] = -INFINITY;
        m = fmaxf(m, x[j][e]);
      }
    } else {
      x[j] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    }
  }
  m = wave_max(m);
  if (lane == 0) sh[wave] = m;
  __syncthreads();
  m = sh[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) m = fmaxf(m, sh[w]);
  float s = 0.f;
  if (m != -INFINITY) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) s += __expf(x[j][e] - m);
  }
  s = wave_sum(s);
  if (lane == 0) sh[16 + wave] = s;
  __syncthreads();
  s = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) s += sh[16 + w];
  const float lse = m + __logf(s);
  if (ban >= 0) {   // banned token: -inf after the normalisation
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((tid + 1024 * j) * 4 + e == ban) x[j][e] = -INFINITY;
  }
  unsigned long long best = 0ull;
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = (tid + 1024 * j) * 4 + e;
      const unsigned long long key = i < V ? topk_key(x[j][e], i) : 0ull;
      best = key > best ? key : best;
    }
  __shared__ unsigned long long shk[16];
  for (int jr = 0; jr < k; ++jr) {
    unsigned long long wk = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t lo = __shfl_xor((uint32_t)wk, o, 64);
      const uint32_t hi = __shfl_xor((uint32_t)(wk >> 32), o, 64);
      const unsigned long long k2 = ((unsigned long long)hi << 32) | lo;
      wk = k2 > wk ? k2 : wk;
    }
    if (lane == 0) shk[wave] = wk;
    __syncthreads();
    wk = shk[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) {
      const unsigned long long k2 = shk[w];
      wk = k2 > wk ? k2 : wk;
    }
    __syncthreads();
    const int wi = topk_winner_index(wk);
    if (tid == 0) {
      out_val[(size_t)r * k + jr] = (topk_winner_value(wk) - lse) + a;
      out_idx[(size_t)r * k + jr] = wi;
    }
    if (wk == 0ull) continue;  // fewer than k elements in the row
    const int owner = (wi >> 2) & 1023;
    if (wave == (owner >> 6)) {   // wave-uniform: the owner's next candidate, out of its registers
      unsigned long long nk = 0ull;
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = (tid + 1024 * j) * 4 + e;
          unsigned long long key = i < V ? topk_key(x[j][e], i) : 0ull;
          key = key < wk ? key : 0ull;
          nk = key > nk ? key : nk;
        }
      if (tid == owner) best = nk;
    }
  }
}

// ---- two-launch form for decode-sized problems (a few hundred rows x 50k columns) ----
// One workgroup per row leaves the launch as long as the slowest CU: 320 rows on 256 CUs = 64 CUs with two 200 KB rows
// to pull in (41 us before the first candidate is out), and every one of the k selection rounds is a workgroup-wide
// arg-max plus a rescan of the winner's 52 registers (5.5 us per round: 90 us at k = 10).  Here a row is split into
// TOPK_PARTS parts, one 256-thread workgroup each (1280 workgroups: every CU streams): a part computes its own
// (max, sum-exp) and its own k best -- per wave, with no workgroup barrier in the rounds: every thread keeps its best
// TWO keys, so popping a winner is a register move and the 52-element rescan only runs for a thread that wins a second
// time -- and a second, tiny launch combines the parts of a row: log-sum-exp from the (max, sum) pairs, k best of the
// TOPK_PARTS * k candidates.  Same (value desc, index asc) order, same outputs.
constexpr int TOPK_PARTS = 4, TOPK_KMAX = 16, TOPK_PW = 2 + 2 * TOPK_KMAX;   // words per (row, part) record
constexpr int TOPK_PART_NV = 13;   // float4 chunks per thread of the part kernel: a part holds up to 13 * 256 chunks

// Wave-wide maximum, result in every lane.  DPP moves instead of the shuffle tree (twelve dependent ds_bpermute per call of the
// 64-bit form through the LDS crossbar: 2.3 us per selection round with five waves per SIMD): rotations by 1, 2, 4, 8 inside each
// row of 16 lanes leave the row maximum in every lane of the row (max is idempotent), row_bcast:15 folds row 0 into 1 and 2 into 3,
// row_bcast:31 folds lane 31 into rows 2 and 3; lane 63 then holds the wave maximum.  One step for 64-bit keys, one for floats.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_max_step(unsigned long long v) {
  const int lo = __builtin_amdgcn_update_dpp((int)(uint32_t)v, (int)(uint32_t)v, CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(uint32_t)(v >> 32), (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xf, false);
  const unsigned long long v2 = ((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo;   // lanes outside ROW_MASK: v itself
  return v2 > v ? v2 : v;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max_step(float v) {
  const float o = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
  return fmaxf(v, o);
}
template <typename T>
__device__ __forceinline__ T dpp_max_to_lane63(T v) {
  v = dpp_max_step<0x121, 0xf>(v);   // row_ror:1
  v = dpp_max_step<0x122, 0xf>(v);   // row_ror:2
  v = dpp_max_step<0x124, 0xf>(v);   // row_ror:4
  v = dpp_max_step<0x128, 0xf>(v);   // row_ror:8
  v = dpp_max_step<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v = dpp_max_step<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
  v = dpp_max_to_lane63(v);
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, 63);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ float wave_max_f32_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dpp_max_to_lane63(v)), 63));
}

// Selection inside a wave (64 lanes x 4 NV values, k best as 64-bit keys into cand[0 .. TOPK_KMAX), 0 = none), round 4:
// the kernel is bound by its vector-ALU work (5 waves per SIMD x ~2500 instructions; the first form built a 64-bit key
// per element and kept every thread's best two keys: 14 instructions per element, 220 registers, three rounds of
// workgroups per launch), so the keys are not built at all for elements that cannot win:
//   1. every lane's two largest VALUES (three instructions per element),
//   2. at most k rounds of a wave-wide maximum over the lanes' current best, the winners popping to their second value,
//      until k values have been counted: the last maximum T is a LOWER bound of the wave's k-th largest value (a lane
//      holding three or more of the k best has contributed only two, the count was filled by smaller ones),
//   3. one pass over the elements: the few with value >= T (k, plus ties and the third-bests of step 2) get their key
//      and a slot of cand[] (ballot + prefix count).  The caller's merge of the waves orders by key as before.
// Fewer than k finite values in the wave, or more than TOPK_KMAX elements >= T (rows of equal logits): the exact, slow
// form below -- k rounds of "largest key below the previous winner" over all elements.  Same keys, same order of the
// final result either way.
template <int NV>
__device__ __forceinline__ void wave_topk(const f32x4 (&x)[NV], int idx0, int chunks_left, int V, int ban, int k, int lane,
                                          unsigned long long* cand, unsigned long long skip = 0ull) {
  // skip: bit 4 j + e set -- element (j, e) is an edited token of a processed beam step, invalid like `ban` (and -inf in x)
  // idx0: index of x[0][0] of this thread; element (j, e) has index idx0 + 1024 j + e; valid iff j * 256 < chunks_left
  // (chunks_left = chunks_per_part - tid), index < V and != ban.  Invalid elements hold -inf (the caller masked them).
  float v1 = -INFINITY, v2 = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float t = fminf(v1, x[j][e]);
      v1 = fmaxf(v1, x[j][e]);
      v2 = fmaxf(v2, t);
    }
  int cnt = 0;
  float T = -INFINITY;
  bool exact = false;
  for (int jr = 0; jr < k && cnt < k; ++jr) {
    const float wm = wave_max_f32_dpp(v1);
    if (wm == -INFINITY) { exact = true; break; }
    const bool mine = v1 == wm;
    cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(mine));
    T = wm;
    if (mine) { v1 = v2; v2 = -INFINITY; }
  }
  if (cnt < k) exact = true;
  int n = 0;
  if (!exact) {
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool hit = x[j][e] >= T;   // T > -inf: invalid elements never hit
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
        if (bal != 0ull) {
          const int slot = n + __builtin_popcountll(bal & below);
          if (hit && slot < TOPK_KMAX) cand[slot] = topk_key(x[j][e], idx0 + 1024 * j + e);
          n += __builtin_popcountll(bal);
        }
      }
    if (n > TOPK_KMAX) exact = true;
  }
  if (!exact) {
    if (lane >= n && lane < TOPK_KMAX) cand[lane] = 0ull;
    return;
  }
  unsigned long long last = ~0ull;
  for (int jr = 0; jr < TOPK_KMAX; ++jr) {
    unsigned long long best = 0ull;
    if (jr < k && last != 0ull) {
#pragma unroll
      for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = idx0 + 1024 * j + e;
          unsigned long long key = (j * 256 < chunks_left && i < V && i != ban && !((skip >> (4 * j + e)) & 1ull)) ? topk_key(x[j][e], i) : 0ull;
          key = key < last ? key : 0ull;
          best = key > best ? key : best;
        }
      best = wave_max_u64(best);
      last = best;
    }
    if (lane == 0) cand[jr] = best;
  }
}

#ifndef KMB_TOPK_OCC
#define KMB_TOPK_OCC 4   // workgroups per CU the register budget is cut for (128 registers: no spills; 2, 4 and 5 measure alike)
#endif
// EDIT (a processed beam step): edit[r * ew + 0 .. ew) names the row's edited tokens (penalised or banned; -1: an
// empty slot).  They leave the selection like `ban`, after the normalisation: an LDS bitmap over the part's own columns, one nibble
// per float4 chunk.  The part's (max, sum-exp) describe the raw row.
template <int NV, bool EDIT = false>   // float4 chunks per thread: chunks per part <= NV * 256
__global__ __launch_bounds__(256, KMB_TOPK_OCC) void topk_part_kernel(const float* __restrict__ logits, int ldv, int V, int ban, int k,
                                                                      int chunks_per_part, float* __restrict__ part,
                                                                      const int32_t* __restrict__ edit, int ew) {
  __shared__ float sh[8];
  __shared__ unsigned long long cand[4][TOPK_KMAX];
  __shared__ uint32_t ebits[EDIT ? NV * 256 * 4 / 32 : 1];
  const int p = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (EDIT) {
    for (int i = tid; i < NV * 256 * 4 / 32; i += 256) ebits[i] = 0u;
    __syncthreads();
  }
  const float* row = logits + (size_t)r * ldv;
  f32x4 x[NV];
  float m = -INFINITY;
  // every load first, from a clamped address and with no branch around it: a load inside `if (in range) { load; mask; }` is
  // followed by its own s_waitcnt vmcnt(0), i.e. NV dependent memory round trips per thread (rounds 2-3 shipped that)
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = tid + 256 * j;
    const int i = (p * chunks_per_part + c) * 4;
    x[j] = *reinterpret_cast<const f32x4*>(row + ((c < chunks_per_part && i < ldv) ? i : 0));
  }
  if (EDIT) {   // behind the row's loads, which the first use below waits for anyway
    const int32_t* er = edit + (size_t)r * ew;
    const int col0 = p * chunks_per_part * 4, ncol = chunks_per_part * 4;
    for (int i = tid; i < ew; i += 256) {
      const int c = er[i] - col0;   // an empty slot is -1: below the part
      if (c >= 0 && c < ncol) atomicOr(&ebits[c >> 5], 1u << (c & 31));
    }
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = tid + 256 * j;
    const int i = (p * chunks_per_part + c) * 4;
    const bool in = c < chunks_per_part && i < ldv;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!in || i + e >= V) x[j][e] = -INFINITY;
      m = fmaxf(m, x[j][e]);
    }
  }
  m = wave_max(m);
  if (lane == 0) sh[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
  float sum = 0.f;
  if (m != -INFINITY) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) sum += __expf(x[j][e] - m);
  }
  sum = wave_sum(sum);
  if (lane == 0) sh[4 + wave] = sum;
  // the banned token is excluded AFTER the normalisation above
  const int idx0 = (p * chunks_per_part + tid) * 4;
  if (ban >= 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (idx0 + 1024 * j + e == ban) x[j][e] = -INFINITY;
  }
  unsigned long long skip = 0ull;
  if (EDIT) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = tid + 256 * j;   // chunk c of the part: columns 4 c .. 4 c + 3, one nibble of word c / 8
      const uint32_t nib = (ebits[c >> 3] >> ((c & 7) * 4)) & 0xfu;
      skip |= (unsigned long long)nib << (4 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((nib >> e) & 1u) x[j][e] = -INFINITY;
    }
  }
  wave_topk<NV>(x, idx0, chunks_per_part - tid, V, ban, k, lane, cand[wave], skip);
  __syncthreads();
  if (wave == 0) {
    float* out = part + ((size_t)r * TOPK_PARTS + p) * TOPK_PW;
    if (lane == 0) { out[0] = m; out[1] = (sh[4] + sh[5]) + (sh[6] + sh[7]); }
    unsigned long long key = cand[lane >> 4][lane & 15];   // 4 x TOPK_KMAX = 64
    for (int jr = 0; jr < k; ++jr) {
      const unsigned long long wk = wave_max_u64(key);
      if (lane == 0) {
        out[2 + 2 * jr] = topk_winner_value(wk);
        reinterpret_cast<int32_t*>(out)[3 + 2 * jr] = topk_winner_index(wk);
      }
      if (key == wk) key = 0ull;
    }
  }
}

// log-sum-exp of a row from the (max, sum-exp) pairs of its TOPK_PARTS part records
__device__ __forceinline__ float parts_lse(const float* __restrict__ rec) {
  float M = -INFINITY;
#pragma unroll
  for (int q = 0; q < TOPK_PARTS; ++q) M = fmaxf(M, rec[q * TOPK_PW]);
  float S = 0.f;
#pragma unroll
  for (int q = 0; q < TOPK_PARTS; ++q) {
    const float mq = rec[q * TOPK_PW];
    if (mq != -INFINITY) S += rec[q * TOPK_PW + 1] * __expf(mq - M);
  }
  return M + __logf(S);
}

// one wave per row: combine the parts (val_row / idx_row: the row's k outputs, global memory or LDS)
__device__ __forceinline__ void topk_combine_row(const float* __restrict__ part, int r, const float* __restrict__ add, int force_token,
                                                 int k, float* val_row, int32_t* idx_row, int lane) {
  const float a = add != nullptr ? add[r] : 0.f;
  if (force_token >= 0) {   // every other logit is -inf: log_softmax is 0 at the forced token (ties in index order)
    for (int j = lane; j < k; j += 64) {
      val_row[j] = j == 0 ? a : -INFINITY;
      idx_row[j] = j == 0 ? force_token : (j - 1 < force_token ? j - 1 : j);
    }
    return;
  }
  const float* rec = part + (size_t)r * TOPK_PARTS * TOPK_PW;
  const float lse = parts_lse(rec);
  unsigned long long key = 0ull;
  if (lane < TOPK_PARTS * k) {
    const float* c = rec + (lane / k) * TOPK_PW + 2 + 2 * (lane % k);
    const int i = reinterpret_cast<const int32_t*>(c)[1];
    if (i != 0x7fffffff) key = topk_key(c[0], i);
  }
  for (int jr = 0; jr < k; ++jr) {
    const unsigned long long wk = wave_max_u64(key);
    if (lane == 0) {
      val_row[jr] = (topk_winner_value(wk) - lse) + a;
      idx_row[jr] = topk_winner_index(wk);
    }
    if (key == wk) key = 0ull;
  }
}
__global__ __launch_bounds__(256) void topk_combine_kernel(const float* __restrict__ part, int rows, const float* __restrict__ add,
                                                           int force_token, int k, float* __restrict__ out_val,
                                                           int32_t* __restrict__ out_idx) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  topk_combine_row(part, r, add, force_token, k, out_val + (size_t)r * k, out_idx + (size_t)r * k, lane);
}

// Beam search, per batch item: the best `k` of the nb * k candidates its beams produced (val / idx from
// logsoftmax_topk_kernel, rows b*nb .. b*nb + nb - 1), ordered by (value desc, candidate position asc) -- what
// torch.topk over the [nb * V] scores of mixins.py's beam step returns, restricted to each beam's own top k (enough:
// the best k overall contain at most k from any beam).  Output, packed for ONE device-to-host copy:
// out[(b*k + j)*2] = score bits (fp32), out[(b*k + j)*2 + 1] = beam * V + token.
//
// next_scores != null: the same launch also picks the beams of the next step, so that the decode loop needs no host
// round trip: in candidate order, the first nb candidates whose token is not EOS (transformers 3.0.2
// _generate_beam_search: an EOS candidate either closes a hypothesis or is skipped, it never continues a beam) ->
// next_scores / next_tokens / next_beam_idx [b*nb + i] (beam index = row of the KV cache to continue from).  What the
// host does with the finished hypotheses and with `done` batch items does not feed back into the other rows.
// (val / idx: the nb * k candidates of batch item b -- global memory or LDS; one wave)
__device__ __forceinline__ void beam_merge_item(const float* val, const int32_t* idx, int b, int lane, int nb, int k, int V,
                                                int32_t* __restrict__ out, int eos, float* __restrict__ next_scores,
                                                int64_t* __restrict__ next_tokens, int32_t* __restrict__ next_beam_idx,
                                                int32_t* snext = nullptr) {
  // (snext != nullptr: the nb chosen beam rows also into that LDS array [0, 16) and their tokens into [16, 32), for the history gather
  //  and the next step's embedding that follow in the same launch)
  // one wave per batch item; lane l holds candidates l, l + 64, l + 128, l + 192 (n <= 256) as 64-bit keys
  // (value bits in order | ~position): a selection round is one DPP wave maximum (round 4; the first form ran a shuffle
  // tree over (value, position) pairs, a workgroup barrier and a global load of the winner's token per round: 1 us each)
  const int n = nb * k;
  unsigned long long key[4];
  int tokv[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = lane + 64 * q;
    const bool in = i < n;
    const float v = val[in ? i : 0];
    tokv[q] = idx[in ? i : 0];
    key[q] = in ? topk_key(v, i) : 0ull;     // topk_key: larger value first, then smaller position; never 0 for a real entry
  }
  int n_sel = 0;
  for (int j = 0; j < k; ++j) {
    unsigned long long best = key[0] > key[1] ? key[0] : key[1];
    const unsigned long long b23 = key[2] > key[3] ? key[2] : key[3];
    best = best > b23 ? best : b23;
    const unsigned long long wk = wave_max_u64(best);   // k <= n: there is always a candidate left
    const int bi = topk_key_index(wk);
    const int q = bi >> 6;
    int tok = 0;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      if (qq == q && lane == (bi & 63)) { tok = tokv[qq]; key[qq] = 0ull; }
    }
    tok = __shfl(tok, bi & 63, 64);   // the owner's token to every lane
    if (lane == 0) {
      const float bv = topk_key_value(wk);
      const int beam = bi / k;
      out[((size_t)b * k + j) * 2] = __float_as_int(bv);
      out[((size_t)b * k + j) * 2 + 1] = beam * V + tok;
      if (next_scores != nullptr && n_sel < nb && tok != eos) {
        if (snext != nullptr) { snext[n_sel] = b * nb + beam; snext[16 + n_sel] = tok; }
        const size_t o = (size_t)b * nb + n_sel++;
        next_scores[o] = bv; next_tokens[o] = tok; next_beam_idx[o] = b * nb + beam;
      }
    }
  }
  if (lane == 0 && next_scores != nullptr) {
    for (; n_sel < nb; ++n_sel) {   // cannot happen with k >= 2 * nb (at most one EOS candidate per beam); keep the rows defined
      if (snext != nullptr) { snext[n_sel] = b * nb; snext[16 + n_sel] = eos >= 0 ? eos : 0; }
      const size_t o = (size_t)b * nb + n_sel;
      next_scores[o] = -1e9f; next_tokens[o] = eos >= 0 ? eos : 0; next_beam_idx[o] = b * nb;
    }
  }
}
__global__ __launch_bounds__(64) void beam_merge_kernel(const float* __restrict__ val, const int32_t* __restrict__ idx,
                                                        int nb, int k, int V, int32_t* __restrict__ out, int eos,
                                                        float* __restrict__ next_scores, int64_t* __restrict__ next_tokens,
                                                        int32_t* __restrict__ next_beam_idx) {
  const int b = blockIdx.x, n = nb * k;
  beam_merge_item(val + (size_t)b * n, idx + (size_t)b * n, b, threadIdx.x, nb, k, V, out, eos, next_scores, next_tokens, next_beam_idx);
}

// ---- the fused beam steps: one workgroup per batch item ----
// Wave w < nb leaves the k candidates of beam row b * nb + w in LDS (sval / sidx [w * k ...]; each kernel declares the arrays itself:
// one struct for the three moved their LDS offsets), and all of them end alike: wave 0 merges the item's candidates and gathers the
// history index for the beams it chose (snext: beam_fold.h), then one wave per chosen beam embeds its token for the next decode step.
// `between` runs in every thread after wave 0's work.
template <typename Between>
__device__ __forceinline__ void beam_step_finish(const float* sval, const int32_t* sidx, int32_t* snext, int b, int wave, int lane, int nb, int k,
                                                 int V, int32_t* __restrict__ out, int eos, float* __restrict__ next_scores,
                                                 int64_t* __restrict__ next_tokens, int32_t* __restrict__ next_beam_idx,
                                                 const KmbHistGather& hg, const KmbEmbedNext& en, Between between) {
  __syncthreads();
  if (wave == 0) {
    beam_merge_item(sval, sidx, b, lane, nb, k, V, out, eos, next_scores, next_tokens, next_beam_idx, snext);
    beam_hist_gather(hg, snext, b, nb, lane);
  }
  between();
  beam_embed_next(en, snext, b, nb, wave, lane);
}

// topk_combine_kernel + beam_merge_kernel in one launch (the decode loop), same arithmetic and order.
__global__ __launch_bounds__(1024) void beam_combine_merge_kernel(const float* __restrict__ part, const float* __restrict__ add,
                                                                  int force_token, int nb, int k, int V, int32_t* __restrict__ out,
                                                                  int eos, float* __restrict__ next_scores,
                                                                  int64_t* __restrict__ next_tokens, int32_t* __restrict__ next_beam_idx,
                                                                  const KmbHistGather hg, const KmbEmbedNext en) {
  __shared__ float sval[256];
  __shared__ int32_t sidx[256];
  __shared__ int32_t snext[32];
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave < nb) topk_combine_row(part, b * nb + wave, add, force_token, k, sval + wave * k, sidx + wave * k, lane);
  beam_step_finish(sval, sidx, snext, b, wave, lane, nb, k, V, out, eos, next_scores, next_tokens, next_beam_idx, hg, en, [] {});
}

// ---- the beam step with generate()'s score processors ----
// The row's tokens split in two: the edited ones (beam_process.hip's list: penalised-and-not-banned, banned) and all others.
// topk_part_kernel<13, true> left the best UNEDITED tokens of every part and the raw row's (max, sum-exp); here the penalised tokens join
// them: logits[r][x] gathered, (v - lse) scaled by the penalty.  Candidates are ordered by their final score (value desc, token asc),
// what torch.topk over the edited log-probabilities orders by -- the penalty does not keep the order of the logits.
// One wave per row; up to KMB_PROCESS_MAX_T = 1024 penalised tokens, 16 per lane, every gather issued before the first use.
__device__ __forceinline__ void topk_combine_row_edit(const float* __restrict__ part, int r, const float* __restrict__ add, int force_token,
                                                      int k, float* val_row, int32_t* idx_row, int lane, const float* __restrict__ logits,
                                                      int ldv, const KmbBeamEdit& ed) {
  if (force_token >= 0) {   // log_softmax is exactly 0 at the forced token: the penalty leaves it, and no ban hits it (the caller's routing)
    topk_combine_row(part, r, add, force_token, k, val_row, idx_row, lane);
    return;
  }
  constexpr int NQ = KMB_PROCESS_MAX_T / 64;
  const float a = add != nullptr ? add[r] : 0.f;
  const float* rec = part + (size_t)r * TOPK_PARTS * TOPK_PW;
  const int32_t* er = ed.edit + (size_t)r * ed.ew;   // slots [0, t): the penalised tokens, -1 for none
  const float* row = logits + (size_t)r * ldv;
  int xs[NQ];
  float vs[NQ];
  if (ed.penalise) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int j = lane + 64 * q;
      const int x = er[j < ed.t ? j : 0];
      xs[q] = j < ed.t ? x : -1;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) vs[q] = row[xs[q] >= 0 ? xs[q] : 0];
  } else {
#pragma unroll
    for (int q = 0; q < NQ; ++q) { xs[q] = -1; vs[q] = 0.f; }
  }
  const float lse = parts_lse(rec);
  unsigned long long key = 0ull, pk[NQ];
  if (lane < TOPK_PARTS * k) {
    const float* c = rec + (lane / k) * TOPK_PW + 2 + 2 * (lane % k);
    const int i = reinterpret_cast<const int32_t*>(c)[1];
    if (i != 0x7fffffff) key = topk_key((c[0] - lse) + a, i);
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const float s = vs[q] - lse;
    pk[q] = xs[q] >= 0 ? topk_key((s < 0.f ? s * ed.p : s * ed.inv_p) + a, xs[q]) : 0ull;
  }
  for (int jr = 0; jr < k; ++jr) {
    unsigned long long best = key;
#pragma unroll
    for (int q = 0; q < NQ; ++q) best = pk[q] > best ? pk[q] : best;
    const unsigned long long wk = wave_max_u64(best);
    if (lane == 0) {
      val_row[jr] = topk_winner_value(wk);
      idx_row[jr] = topk_winner_index(wk);
    }
    if (key == wk) key = 0ull;   // (a token is in one list only, once: the keys are distinct)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (pk[q] == wk) pk[q] = 0ull;
  }
}
// beam_combine_merge_kernel on the processed rows; the workgroup also moves the item's token histories on for the next step's edit:
// ids_out[i][0 .. t) = ids_in[next_beam_idx[i]][0 .. t), ids_out[i][t] = next_tokens[i].
__global__ __launch_bounds__(1024) void beam_combine_merge_edit_kernel(const float* __restrict__ part, const float* __restrict__ add,
                                                                       int force_token, int nb, int k, int V, int32_t* __restrict__ out,
                                                                       int eos, float* __restrict__ next_scores,
                                                                       int64_t* __restrict__ next_tokens, int32_t* __restrict__ next_beam_idx,
                                                                       const KmbHistGather hg, const KmbEmbedNext en,
                                                                       const float* __restrict__ logits, int ldv, const KmbBeamEdit ed) {
  __shared__ float sval[256];
  __shared__ int32_t sidx[256];
  __shared__ int32_t snext[32];
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave < nb) topk_combine_row_edit(part, b * nb + wave, add, force_token, k, sval + wave * k, sidx + wave * k, lane, logits, ldv, ed);
  beam_step_finish(sval, sidx, snext, b, wave, lane, nb, k, V, out, eos, next_scores, next_tokens, next_beam_idx, hg, en, [&] {
    __syncthreads();   // snext was written by wave 0
    const int w = ed.t + 1;
    for (int e = threadIdx.x; e < nb * w; e += 64 * nb) {
      const int i = e / w, j = e - i * w;
      ed.ids_out[(size_t)(b * nb + i) * ed.ld_ids + j] = j < ed.t ? ed.ids_in[(size_t)snext[i] * ed.ld_ids + j] : (int64_t)snext[16 + i];
    }
  });
}

// ---- the beam step behind the all-rows vocabulary projection's STATS epilogue (round 6) ----
// gemm.hip's gemm_kernel_allrows<true> leaves, per row and 256-column block, the block's maximum logit and its sum of exp(v - maximum):
// stats[(row * nblk + blk) * 2], [... + 1].  With them ONE launch does what topk_part_kernel +
// beam_combine_merge_kernel did, without streaming the 64 MB of logits again (topk_part: 22.9 us of a 553 us decode step):
//   * log-sum-exp of the row from the nblk pairs;
//   * T = the (k + 1 if a token is banned)-th largest block maximum: at least k admissible logits are >= T, so the k best are among
//     the elements >= T, and those sit in the blocks whose maximum is >= T -- typically k or k + 1 blocks of 1 KB, read HS_BATCH at a time;
//   * the k best of those candidates by (value desc, index asc) key, as everywhere else; then the item's merge (beam_merge_item).
// More than HS_CAND elements >= T (rows of equal logits): k rounds of "largest key below the previous winner" over the selected blocks.
// Same selection as the two-launch path; the scores differ from it in the last bits only through the log-sum-exp's grouping
// (197 blocks of 256 columns instead of 4 parts).
constexpr int HS_ROWS = 320, HS_COLS = 256, HS_CAND = 128, HS_BLK_MAX = 256, HS_BATCH = 12;   // HS_BATCH: blocks read at a time (k = 10: 10 or 11 blocks)

__device__ __forceinline__ void beam_stats_row(const float* __restrict__ logits, int ldv, int V, const float* __restrict__ stats, int nblk,
                                               int r, const float* __restrict__ add, int force_token, int ban, int k, float* val_row,
                                               int32_t* idx_row, unsigned long long* cand, uint16_t* sel, int lane) {
  const float a = add != nullptr ? add[r] : 0.f;
  if (force_token >= 0) {   // (topk_combine_row)
    for (int j = lane; j < k; j += 64) {
      val_row[j] = j == 0 ? a : -INFINITY;
      idx_row[j] = j == 0 ? force_token : (j - 1 < force_token ? j - 1 : j);
    }
    return;
  }
  float mq[4], sq[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int blk = lane + 64 * q;
    const bool in = blk < nblk;
    const float2 ms = reinterpret_cast<const float2*>(stats)[(size_t)r * nblk + (in ? blk : 0)];
    mq[q] = in ? ms.x : -INFINITY;
    sq[q] = in ? ms.y : 0.f;
  }
  const float M = wave_max_f32_dpp(fmaxf(fmaxf(mq[0], mq[1]), fmaxf(mq[2], mq[3])));
  float S = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (mq[q] != -INFINITY) S += sq[q] * __expf(mq[q] - M);
  S = wave_sum(S);
  const float lse = M + __logf(S);
  // T: the keff-th largest block maximum (a lane's four, sorted, pop one per round: equal maxima are counted one per lane and round)
  const int keff = k + (ban >= 0 ? 1 : 0);
  float h0 = mq[0], h1 = mq[1], h2 = mq[2], h3 = mq[3];
  {
    float t;
#define KMB_CSWAP(x, y) t = fminf(x, y); x = fmaxf(x, y); y = t;
    KMB_CSWAP(h0, h1) KMB_CSWAP(h2, h3) KMB_CSWAP(h0, h2) KMB_CSWAP(h1, h3) KMB_CSWAP(h1, h2)
#undef KMB_CSWAP
  }
  float T = -INFINITY;
  int cnt = 0;
  for (int jr = 0; jr < keff && cnt < keff; ++jr) {
    const float wm = wave_max_f32_dpp(h0);
    if (wm == -INFINITY) break;
    const bool mine = h0 == wm;
    cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(mine));
    T = wm;
    if (mine) { h0 = h1; h1 = h2; h2 = h3; h3 = -INFINITY; }
  }
  if (cnt < keff) T = -INFINITY;   // fewer blocks than keff: every block is read, every admissible element is a candidate
  const unsigned long long below = (1ull << lane) - 1ull;
  int n_sel = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool pick = lane + 64 * q < nblk && mq[q] >= T;
    const unsigned long long bal = __builtin_amdgcn_ballot_w64(pick);
    if (pick) sel[n_sel + __builtin_popcountll(bal & below)] = (uint16_t)(lane + 64 * q);
    n_sel += __builtin_popcountll(bal);
  }
  __builtin_amdgcn_wave_barrier();
  const float* row = logits + (size_t)r * ldv;
  int n = 0;
  for (int base = 0; base < n_sel; base += HS_BATCH) {
    f32x4 x[HS_BATCH];
    int c0[HS_BATCH];
#pragma unroll
    for (int u = 0; u < HS_BATCH; ++u) {   // every load first, clamped
      const int blk = sel[base + u < n_sel ? base + u : base];
      c0[u] = blk * HS_COLS + lane * 4;
      const bool in = base + u < n_sel && c0[u] < V;     // V % 4 == 0, ldv >= V: a group of four is inside or outside
      x[u] = *reinterpret_cast<const f32x4*>(row + (in ? c0[u] : 0));
      if (!in) c0[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < HS_BATCH; ++u) {
      if (base + u < n_sel) {   // wave-uniform (no `break`: the loop must unroll, x[] lives in registers)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool hit = c0[u] >= 0 && !(x[u][e] < T) && c0[u] + e != ban;   // (!(x < T): a NaN is a candidate, as in the two-launch path)
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(hit);
        if (bal != 0ull) {
          const int slot = n + __builtin_popcountll(bal & below);
          if (hit && slot < HS_CAND) cand[slot] = topk_key(x[u][e], c0[u] + e);
          n += __builtin_popcountll(bal);
        }
      }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  if (n >= k && n <= HS_CAND) {
    unsigned long long k0 = lane < n ? cand[lane] : 0ull;
    unsigned long long k1 = lane + 64 < n ? cand[lane + 64] : 0ull;
    for (int jr = 0; jr < k; ++jr) {
      const unsigned long long wk = wave_max_u64(k0 > k1 ? k0 : k1);
      if (lane == 0) {
        val_row[jr] = (topk_winner_value(wk) - lse) + a;
        idx_row[jr] = topk_winner_index(wk);
      }
      if (k0 == wk) k0 = 0ull;
      if (k1 == wk) k1 = 0ull;
    }
    return;
  }
  // The exact, slow form (keys are unique: the index is part of the key).  Also the way out when the fast form found FEWER than k
  // candidates, which takes NaNs in the row (block maxima skip them, `mq >= T` skips their blocks): then every block is read and every
  // admissible element is a candidate, so that -- as in the two-launch path -- the k indices handed on are always real columns.
  const bool all = n < k;
  if (all) T = -INFINITY;
  const int nb_read = all ? nblk : n_sel;
  unsigned long long last = ~0ull;
  for (int jr = 0; jr < k; ++jr) {
    unsigned long long best = 0ull;
    if (last != 0ull) {
      for (int b = 0; b < nb_read; ++b) {
        const int c = (all ? b : (int)sel[b]) * HS_COLS + lane * 4;
        if (c >= V) continue;
        const f32x4 x = *reinterpret_cast<const f32x4*>(row + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          unsigned long long key = (!(x[e] < T) && c + e != ban) ? topk_key(x[e], c + e) : 0ull;
          key = key < last ? key : 0ull;
          best = key > best ? key : best;
        }
      }
      best = wave_max_u64(best);
      last = best;
    }
    if (lane == 0) {
      val_row[jr] = (topk_winner_value(best) - lse) + a;
      idx_row[jr] = topk_winner_index(best);
    }
  }
}

__global__ __launch_bounds__(1024) void beam_stats_merge_kernel(const float* __restrict__ logits, int ldv, const float* __restrict__ stats,
                                                                int nblk, const float* __restrict__ add, int force_token, int ban, int nb,
                                                                int k, int V, int32_t* __restrict__ out, int eos,
                                                                float* __restrict__ next_scores, int64_t* __restrict__ next_tokens,
                                                                int32_t* __restrict__ next_beam_idx, const KmbHistGather hg,
                                                                const KmbEmbedNext en) {
  __shared__ float sval[256];
  __shared__ int32_t sidx[256];
  __shared__ int32_t snext[32];
  __shared__ unsigned long long cand[16][HS_CAND];
  __shared__ uint16_t sel[16][HS_BLK_MAX + 8];
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave < nb)
    beam_stats_row(logits, ldv, V, stats, nblk, b * nb + wave, add, force_token, ban, k, sval + wave * k, sidx + wave * k, cand[wave],
                   sel[wave], lane);
  beam_step_finish(sval, sidx, snext, b, wave, lane, nb, k, V, out, eos, next_scores, next_tokens, next_beam_idx, hg, en, [] {});
}

// ---- launchers ----

// the split form: whole float4 chunks of an aligned row, a part within the part kernel's registers, the rows within the launch grid
int topk_part_chunks(int ldv) { return (ldv / 4 + TOPK_PARTS - 1) / TOPK_PARTS; }
bool topk_parts_ok(const float* logits, int ldv, int rows, int k) {
  return k >= 1 && k <= TOPK_KMAX && (ldv & 3) == 0 && ((uintptr_t)logits & 15) == 0 && topk_part_chunks(ldv) <= TOPK_PART_NV * 256 &&
         rows <= 65535;
}
template <bool EDIT>
void topk_part_launch(const float* logits, int ldv, int V, int rows, int ban_token, int k, float* part, const int32_t* edit, int ew,
                      hipStream_t stream) {
  hipLaunchKernelGGL((topk_part_kernel<TOPK_PART_NV, EDIT>), dim3(TOPK_PARTS, rows), dim3(256), 0, stream, logits, ldv, V, ban_token, k,
                     topk_part_chunks(ldv), part, edit, ew);
}

// What the three beam-step launchers check alike, after their own shape conditions (`own_ok`), and the optional work they fold in:
// hist / embed need the next beams.  hipErrorNotSupported: the shape is for another path; hipErrorInvalidValue: a missing output.
hipError_t beam_step_args(const KmbBeamStep& p, bool own_ok, KmbHistGather& hg, KmbEmbedNext& en) {
  if (!(own_ok && p.k >= 1 && p.k <= TOPK_KMAX && p.nb >= 1 && p.nb <= 16 && p.nb * p.k <= 256 && (p.ld & 3) == 0 &&
        ((uintptr_t)p.logits & 15) == 0))
    return hipErrorNotSupported;
  if (p.next_scores != nullptr && (!p.next_tokens || !p.next_beam_idx)) return hipErrorInvalidValue;
  hg = p.hist != nullptr && p.next_scores != nullptr ? *p.hist : KmbHistGather{nullptr, nullptr, 0, 0};
  en = p.embed != nullptr && p.next_scores != nullptr ? *p.embed : KmbEmbedNext{};
  if (en.E != nullptr && ((en.D & 7) || en.D > 1024 || en.D <= 512)) return hipErrorInvalidValue;   // embed_ln_row<2>
  return hipSuccess;
}

}  // namespace

size_t kmb_logsoftmax_topk_scratch_floats(int rows) { return (size_t)(rows > 0 ? rows : 0) * TOPK_PARTS * TOPK_PW; }

hipError_t kmb_logsoftmax_topk_launch(const float* logits, int ldv, int V, int rows, const float* add,
                                      int force_token, int ban_token, int k, float* out_val, int32_t* out_idx,
                                      float* scratch, size_t scratch_floats, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  if (scratch != nullptr && scratch_floats >= kmb_logsoftmax_topk_scratch_floats(rows) && topk_parts_ok(logits, ldv, rows, k)) {
    if (force_token < 0) topk_part_launch<false>(logits, ldv, V, rows, ban_token, k, scratch, nullptr, 0, stream);
    hipLaunchKernelGGL(topk_combine_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, scratch, rows, add, force_token, k, out_val, out_idx);
    return hipGetLastError();
  }
  if (ldv <= 13 * 4096 && (ldv & 3) == 0 && ((uintptr_t)logits & 15) == 0)
    hipLaunchKernelGGL((logsoftmax_topk_reg_kernel<13>), dim3(rows), dim3(1024), 0, stream, logits, ldv, V, add, force_token, ban_token, k, out_val, out_idx);
  else
    hipLaunchKernelGGL(logsoftmax_topk_kernel, dim3(rows), dim3(256), 0, stream, logits, ldv, V, add, force_token, ban_token, k, out_val, out_idx);
  return hipGetLastError();
}

// log-softmax top-k of every beam row + the per-item merge + the next step's beams: topk_part (unless the token is forced) and ONE
// launch for the rest.  hipErrorNotSupported: the shape needs the separate launches (kmb_logsoftmax_topk_launch + kmb_beam_merge_launch).
hipError_t kmb_beam_step_launch(const KmbBeamStep& p, float* scratch, size_t scratch_floats, hipStream_t stream) {
  if (p.B <= 0) return hipSuccess;
  const int rows = p.B * p.nb;
  KmbHistGather hg;
  KmbEmbedNext en;
  const hipError_t e = beam_step_args(p, scratch != nullptr && scratch_floats >= kmb_logsoftmax_topk_scratch_floats(rows) &&
                                             topk_parts_ok(p.logits, p.ld, rows, p.k), hg, en);
  if (e != hipSuccess) return e;
  if (p.force_token < 0) topk_part_launch<false>(p.logits, p.ld, p.V, rows, p.ban_token, p.k, scratch, nullptr, 0, stream);
  hipLaunchKernelGGL(beam_combine_merge_kernel, dim3(p.B), dim3(64 * p.nb), 0, stream, scratch, p.add, p.force_token, p.nb, p.k, p.V, p.out,
                     p.eos, p.next_scores, p.next_tokens, p.next_beam_idx, hg, en);
  return hipGetLastError();
}

// kmb_beam_step_launch with generate()'s score processors: the rows' edit sets (beam_process.hip, one launch), the part
// kernel without the edited tokens, and the combine / merge launch that brings the penalised ones back and moves the token histories
// on.  A forced step launches the last of the three only.  scratch: kmb_beam_step_processed_scratch_floats(rows, t, n_bad) words.
size_t kmb_beam_step_processed_scratch_floats(int rows, int t, int n_bad) {
  const size_t r = rows > 0 ? rows : 0;
  return kmb_logsoftmax_topk_scratch_floats(rows) + r * kmb_beam_edit_words(t, n_bad);
}
hipError_t kmb_beam_step_processed_launch(const KmbBeamStep& p, float* scratch, size_t scratch_floats, const KmbBeamProcess& pr,
                                          hipStream_t stream) {
  if (p.B <= 0) return hipSuccess;
  const int rows = p.B * p.nb;
  KmbHistGather hg;
  KmbEmbedNext en;
  const hipError_t e = beam_step_args(p, scratch != nullptr && scratch_floats >= kmb_beam_step_processed_scratch_floats(rows, pr.t, pr.n_bad) &&
                                             topk_parts_ok(p.logits, p.ld, rows, p.k) && p.V <= KMB_BEAM_EDIT_MAX_V && pr.t >= 1 &&
                                             pr.t <= KMB_PROCESS_MAX_T, hg, en);
  if (e != hipSuccess) return e;
  if (!p.next_scores || !pr.ids_in || !pr.ids_out) return hipErrorInvalidValue;
  const int ew = kmb_beam_edit_words(pr.t, pr.n_bad);
  int32_t* edit = reinterpret_cast<int32_t*>(scratch + kmb_logsoftmax_topk_scratch_floats(rows));
  const KmbBeamEdit ed{edit, ew, pr.t, pr.repetition_penalty, 1.0f / pr.repetition_penalty, pr.repetition_penalty != 1.0f ? 1 : 0,
                       pr.ids_in, pr.ids_out, pr.ld_ids};
  if (p.force_token < 0) {
    const hipError_t ee = kmb_beam_edit_launch(pr, p.V, rows, p.ban_token, edit, stream);
    if (ee != hipSuccess) return ee;
    topk_part_launch<true>(p.logits, p.ld, p.V, rows, p.ban_token, p.k, scratch, edit, ew, stream);
  }
  hipLaunchKernelGGL(beam_combine_merge_edit_kernel, dim3(p.B), dim3(64 * p.nb), 0, stream, scratch, p.add, p.force_token, p.nb, p.k, p.V,
                     p.out, p.eos, p.next_scores, p.next_tokens, p.next_beam_idx, hg, en, p.logits, p.ld, ed);
  return hipGetLastError();
}

// The same step from the all-rows projection's per-block statistics (gemm.hip kmb_gemm_allrows_launch with stats): one launch.
// hipErrorNotSupported: the shape needs kmb_beam_step_launch.
hipError_t kmb_beam_step_stats_launch(const KmbBeamStep& p, const float* stats, int nblk, hipStream_t stream) {
  if (p.B <= 0) return hipSuccess;
  KmbHistGather hg;
  KmbEmbedNext en;
  const hipError_t e = beam_step_args(p, stats != nullptr && nblk >= 1 && nblk <= HS_BLK_MAX && nblk == (p.V + HS_COLS - 1) / HS_COLS &&
                                             p.B * p.nb <= HS_ROWS && (p.V & 3) == 0 && p.ld >= p.V, hg, en);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(beam_stats_merge_kernel, dim3(p.B), dim3(64 * p.nb), 0, stream, p.logits, p.ld, stats, nblk, p.add, p.force_token,
                     p.ban_token, p.nb, p.k, p.V, p.out, p.eos, p.next_scores, p.next_tokens, p.next_beam_idx, hg, en);
  return hipGetLastError();
}

hipError_t kmb_beam_merge_launch(const float* val, const int32_t* idx, int B, int nb, int k, int V, int32_t* out, int eos,
                                 float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  if (nb * k > 256 || k <= 0) return hipErrorInvalidValue;
  if (next_scores != nullptr && (!next_tokens || !next_beam_idx)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(64), 0, stream, val, idx, nb, k, V, out, eos, next_scores, next_tokens,
                     next_beam_idx);
  return hipGetLastError();
}
