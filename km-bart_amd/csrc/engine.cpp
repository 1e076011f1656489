// Host-side driver of the KM-BART hot path: owns the parameter census, lays activations out in the
// caller's workspace and enqueues the HIP kernels of one training step / decode step on a stream.
// No device allocation, no synchronisation: the Python host (torch) owns memory and streams.
//
// Reference call path being replaced:
//   src/training.py:118-143 -> src/model/model.py:325-405 -> src/model/modules.py:104-165
//   + transformers 3.0.2 EncoderLayer / BartDecoder / AdamW.
#include <cstdarg>

#include "engine_internal.h"

namespace kmbi __attribute__((visibility("hidden"))) {

thread_local std::string g_err;
int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}
__thread bool g_f32 = false;
__thread float* g_small_slab = nullptr;
__thread size_t g_small_floats = 0;

size_t add_param(kmb_handle* h, const std::string& name, int rows, int cols) {
  h->arena = align_up(h->arena, 64);
  const size_t off = h->arena;
  h->params.push_back({name, off, rows, cols});
  h->arena += (size_t)rows * cols;
  return off;
}

void add_attn(kmb_handle* h, const std::string& p, const std::string& ln, AttnP& a) {
  const int d = h->d;
  a.qkv_w = add_param(h, p + "q_proj.weight", d, d);
  add_param(h, p + "k_proj.weight", d, d);
  add_param(h, p + "v_proj.weight", d, d);
  a.qkv_b = add_param(h, p + "q_proj.bias", 1, d);
  add_param(h, p + "k_proj.bias", 1, d);
  add_param(h, p + "v_proj.bias", 1, d);
  a.o_w = add_param(h, p + "out_proj.weight", d, d);
  a.o_b = add_param(h, p + "out_proj.bias", 1, d);
  a.ln_g = add_param(h, ln + ".weight", 1, d);
  a.ln_b = add_param(h, ln + ".bias", 1, d);
}

// cross-attention block of a decoder layer: query projection, output projection, LayerNorm (k | v: see kmb_handle::xkv_w)
void add_cross_attn(kmb_handle* h, const std::string& p, const std::string& ln, AttnP& a) {
  const int d = h->d;
  a.qkv_w = add_param(h, p + "q_proj.weight", d, d);
  a.qkv_b = add_param(h, p + "q_proj.bias", 1, d);
  a.o_w = add_param(h, p + "out_proj.weight", d, d);
  a.o_b = add_param(h, p + "out_proj.bias", 1, d);
  a.ln_g = add_param(h, ln + ".weight", 1, d);
  a.ln_b = add_param(h, ln + ".bias", 1, d);
}

void add_ffn(kmb_handle* h, const std::string& p, int F, LayerP& L) {
  const int d = h->d;
  L.fc1_w = add_param(h, p + "fc1.weight", F, d);
  L.fc1_b = add_param(h, p + "fc1.bias", 1, F);
  L.fc2_w = add_param(h, p + "fc2.weight", d, F);
  L.fc2_b = add_param(h, p + "fc2.bias", 1, d);
  L.ln_g = add_param(h, p + "final_layer_norm.weight", 1, d);
  L.ln_b = add_param(h, p + "final_layer_norm.bias", 1, d);
}

// ---- optional per-launch timing of the GEMM kernels with HIP events (bench.py roofline leg) ----
struct GemmProfiler {
  bool on = false;
  std::vector<hipEvent_t> ev;        // pairs
  // pair: the event pair that brackets the launch; share: this record's part of that launch's time (1 for a launch of its own; a
  // grouped weight-gradient launch has one record per problem, time split by FLOPs, `launch` 1 on the first of them only)
  struct Rec { int variant; double flops; int M, N, K, split, act, res; size_t pair = 0; float share = 1.f; int launch = 1; int group_n = 1; };
  std::vector<Rec> recs;
  size_t used = 0;
} g_prof;

int prof_begin(hipStream_t s) {   // the first event of the next pair, recorded on s (the pool grows as needed)
  if (g_prof.used + 2 > g_prof.ev.size()) {
    const size_t old = g_prof.ev.size();
    g_prof.ev.resize(old + 512);
    for (size_t i = old; i < g_prof.ev.size(); ++i) HIPCHK(hipEventCreate(&g_prof.ev[i]));
  }
  HIPCHK(hipEventRecord(g_prof.ev[g_prof.used], s));
  return 0;
}

KmbGemm gemm0() { KmbGemm g; memset(&g, 0, sizeof(g)); g.col_scale = 1.f; g.drop_scale = 1.f; return g; }

int run_gemm(const KmbGemm& g, hipStream_t s) {
  if (g_f32) {
    const char* why32 = kmb_f32_gemm_check(g);
    if (why32) return fail("fp32 validation GEMM: %s", why32);
    HIPCHK(kmb_f32_gemm_launch(g, s));
    return 0;
  }
  const char* why = kmb_gemm_check(g);
  if (why) return fail("%s (M=%d N=%d K=%d lda=%d ldb=%d akc=%d bkc=%d)", why, g.M, g.N, g.K, g.lda, g.ldb, g.a_kc, g.b_kc);
  // Small-batch regime (the reference's default per-GPU batch is 64: M = 2048-4096 rows): a forward / data-gradient
  // GEMM with N = 768 has 96-192 output tiles for 256 CUs and a serial K loop of up to 48 steps.  Split K over
  // workgroups and let one pass sum the slabs and apply the linear layer's epilogue (bias, q-scale, dropout, residual).
  // 2048x768x3072: 51 -> ~20 us stand-alone; inside a step the idle CUs were already running the side stream's weight
  // gradients, so the whole step gains 2 % at b = 64 (8.06 -> 7.87 ms).  Large batches never take this path.
  static const bool small_ok = !(getenv("KMB_SMALL_SPLIT") && getenv("KMB_SMALL_SPLIT")[0] == '0');
  if (small_ok && g_small_slab != nullptr && g.a_kc == 1 && g.split_k <= 1 && g.act == 0 && !g.preact && !g.colsum && !g.aux &&
      !g.out_f32 && g.out_bf16 && g.beta == 0.f && (g.N & 7) == 0 && (g.K % 64) == 0 && g.M > 512) {
    const int tiles = ((g.M + 127) / 128) * ((g.N + 127) / 128);
    const int nt = g.K / 64;
    static const int small_fill = KMB_DIAG_ENV("KMB_SMALL_FILL") ? atoi(KMB_DIAG_ENV("KMB_SMALL_FILL")) : 512;   // A/B knob
    int S = tiles > 0 ? small_fill / tiles : 1;
    // Round 6: only for <= 48 tiles (M <= 1024 rows of N = 768: b <= 16 encoder rows, b <= 32 decoder rows).  Above that the four-stage 128 x 128
    // kernel (variant 5) -- whose K loop lost its drained prefetch and its accumulator shuffles this round -- runs a lone workgroup's whole K loop
    // faster than five slices + the reduction pass: same box, alternating processes, two rounds (KMB_SMALL_SPLIT=1 | 0): b = 48 6.35-6.37 -> 6.18-6.24 ms,
    // b = 64 6.83-6.91 -> 6.57-6.74, b = 96 8.44-8.52 -> 8.13-8.15; b = 32 and 128 equal; b = 16 4.80-4.86 with the split, 5.05-5.11 without.
    if (tiles > 48) S = 1;
    if (S > 8) S = 8;
    if (S > nt / 4) S = nt / 4;
    while (S > 1 && (size_t)S * g.M * g.N > g_small_floats) --S;
    if (S >= 3) {   // two slices do not pay for the extra pass (b = 128: 10.98 vs 10.92 ms); 96-tile shapes get five
      KmbGemm q = g;
      q.split_k = S; q.slab = g_small_slab; q.out_bf16 = nullptr; q.bias = nullptr; q.residual = nullptr;
      q.drop_thr16 = 0u; q.col_scale = 1.f; q.col_scale_n = 0;
      KCHK(run_gemm(q, s));
      const KmbDrop dr{g.drop_thr16, g.drop_seed, g.drop_scale};
      HIPCHK(kmb_reduce_slabs_epi_launch(g_small_slab, S, (size_t)g.M * g.N, g.bias, g.col_scale, g.col_scale_n, dr, g.residual,
                                         g.ld_res, g.out_bf16, g.ld_out_bf16, g.M, g.N, s));
      return 0;
    }
  }
  if (g_prof.on) {
    KCHK(prof_begin(s));
    HIPCHK(kmb_gemm_launch(g, s));
    HIPCHK(hipEventRecord(g_prof.ev[g_prof.used + 1], s));
    g_prof.recs.push_back({g.a_kc * 2 + g.b_kc, 2.0 * g.M * g.N * (double)g.K, g.M, g.N, g.K, g.split_k, g.act, g.residual != nullptr ? 1 : 0,
                           g_prof.used / 2, 1.f, 1, 1});
    g_prof.used += 2;
    return 0;
  }
  HIPCHK(kmb_gemm_launch(g, s));
  return 0;
}

// Y[M,N] = X[M,K] W[N,K]^T + b
KmbGemm lin_fwd(const bf16_t* x, int ldx, const bf16_t* w, const float* b, int M, int N, int K) {
  KmbGemm g = gemm0();
  g.A = x; g.lda = ldx; g.a_kc = 1; g.B = w; g.ldb = K; g.b_kc = 1; g.M = M; g.N = N; g.K = K; g.bias = b;
  return g;
}
// dX[M,K] = dY[M,N] W[N,K]
KmbGemm lin_dgrad(const bf16_t* dy, int lddy, const bf16_t* w, int M, int N, int K) {
  KmbGemm g = gemm0();
  g.A = dy; g.lda = lddy; g.a_kc = 1; g.B = w; g.ldb = K; g.b_kc = 0; g.M = M; g.N = K; g.K = N;
  return g;
}
// dW[N,K] = dY[M,N]^T X[M,K]   (fp32, written straight into the gradient arena)
KmbGemm lin_wgrad(const bf16_t* dy, int lddy, const bf16_t* x, int ldx, float* dW, int M, int N, int K, float beta) {
  KmbGemm g = gemm0();
  g.A = dy; g.lda = lddy; g.a_kc = 0; g.B = x; g.ldb = ldx; g.b_kc = 0; g.M = N; g.N = K; g.K = M;
  g.out_f32 = dW; g.ld_out_f32 = K; g.beta = beta;
  return g;
}

// Weight-gradient GEMMs have few output tiles (768x768 -> 36) and a very long reduction (all tokens):
// split K over workgroups so that the grid fills the chip; partial slabs are summed by one pass.
// `slab` / `slab_floats`: the partial-sum buffer of the STREAM the launch goes to.  The side stream's weight gradients use
// h->tl.slab; the pre-training heads (head_run, caller's stream, concurrent with the tied matrix's gradient on the side
// stream) have their own h->tl.head_slab -- two streams never share one.
int run_wgrad(kmb_handle* h, KmbGemm g, hipStream_t s, float* slab, size_t slab_floats) {
  const int tiles = ((g.M + 127) / 128) * ((g.N + 127) / 128);
  const int nt = (g.K + 63) / 64;
  // Slices fill `fill` workgroup slots: 512 (two 128x128 workgroups per CU) when the reduction is long.  With a short
  // reduction (small batches: <= 8192 encoder tokens; the rule goes by the batch, not by the GEMM: a per-GEMM rule measured
  // worse at b = 128) the slab traffic of many slices -- S x the gradient written, then read --
  // costs more than the fuller grid buys, and the caller's stream keeps the other CUs busy anyway: whole step, same box
  // (tools/step_ab_seq.sh): b = 64 7.52 ms with 256 against 7.78 with 512 (384: 7.67, 192: 7.60), b = 128 10.51 with 384
  // against 10.80 (256: 10.95), b = 32 5.99 with 256 against 6.17, b = 256 16.7 with 512 against 18.3 with 256.
  static const int fill_env = KMB_DIAG_ENV("KMB_WGRAD_FILL") ? atoi(KMB_DIAG_ENV("KMB_WGRAD_FILL")) : 0;   // A/B knob
  const int mmax = h->Me > h->Md ? h->Me : h->Md;   // tokens of the longer side: how busy the caller's stream keeps the chip
  // Round 6: 768 slots from 16384 tokens on (was 512).  With the transposing reads as inline asm in every split-K kernel (no drained prefetch) a
  // slice is cheaper than it was when 512 was measured: same box, alternating processes (KMB_WGRAD_FILL, diagnostic library, two rounds each):
  // b = 256 14.17-14.20 ms with 768 against 14.30-14.38 with 512 (1024: 14.28-14.30, 1536: 15.2), b = 512 24.20-24.34 against 24.46-24.59,
  // b = 1024 44.49-44.57 against 44.61-45.01; b = 128 (8192 tokens: stays at 384) 9.40-9.44 with 768 against 9.17-9.26.
  const int fill = fill_env > 0 ? fill_env : mmax <= 4096 ? 256 : mmax <= 8192 ? 384 : 768;
  int S = fill / tiles;   // floor: a partial last round costs more than it fills
                         // (tools/wgrad_split_sweep.py: 36 tiles S14 59 us vs S11 70 us, 72 tiles S7 97 vs S6 104)
  if (S > 16) S = 16;
  // 128-160 tiles and a very long reduction (3072x768 over 32768 tokens): 256x256 tiles with a slice count that fills
  // the chip once beat the 128x128 kernel at S = 3 by 10-12 % (tools/wgrad_split_sweep.py); with these slices the
  // launcher's timing picks the 256x256 kernel.  (Slice counts rounded to the 8 XCDs -- 3 -> 4, 7 -> 8, 14 -> 16, one slice
  // per XCD under the slice-major enumeration -- measured 18 % slower on the weight gradients: 780 -> 638 TFLOP/s.)
  // (wider ranges gain what the longer slab reduction costs -- unless the reduction is very long: 2304x768 over 65536
  // tokens, 108 tiles: 9 slices of the 256x256 kernel 251 us against 4 of the 128x128 kernel 294)
  static const int slots256 = KMB_DIAG_ENV("KMB_WG256_SLOTS") ? atoi(KMB_DIAG_ENV("KMB_WG256_SLOTS")) : 256;   // A/B knob: workgroup slots the 256 x 256 slices fill
  if (tiles >= 96 && tiles <= 160) {
    const int tiles256 = ((g.M + 255) / 256) * ((g.N + 255) / 256);
    const int s256 = slots256 / tiles256;
    if (s256 > S && ((tiles >= 128 && nt >= 512) || nt / s256 >= 100)) S = s256;
  }
  // More 256x256 tiles than CUs and a poorly filled last round (the tied 50320x768 matrix: 591 tiles = 2.31 rounds, 77 %
  // of three): two or three K slices make the rounds come out even (x 3 = 6.93 of 7).  3137 -> 2480 + 155 us of slab
  // reduction at 32768 tokens (tools/wgrad_split_sweep.py's sibling measurement).
  if (S <= 1 && nt >= 256) {
    const int tiles256 = ((g.M + 255) / 256) * ((g.N + 255) / 256);
    if (tiles256 > 256) {
      auto eff = [&](int k) { const double r = (double)tiles256 * k / 256.0; return r / std::ceil(r); };
      int best = 1;
      for (int k = 2; k <= 3; ++k)
        if (eff(k) > eff(best) + 0.02) best = k;
      if (eff(best) >= eff(1) + 0.10) S = best;
    }
  }
  // 64 .. 128 tiles of 256x256 and no slice from the rules above (the batched cross-attention k | v weights: 9216 x 768 =
  // 108 tiles): two or more slices so that the 256x256 kernel covers the chip once
  if (S <= 1 && nt >= 128) {
    const int tiles256 = ((g.M + 255) / 256) * ((g.N + 255) / 256);
    if (tiles256 >= 64 && tiles256 <= 128) S = slots256 / tiles256;
  }
  if (S > nt / 2) S = nt / 2;
  while (S > 1 && (size_t)S * g.M * g.N > slab_floats) --S;
  if (S <= 1 || slab == nullptr || g.ld_out_f32 != g.N || ((size_t)g.M * g.N & 3)) return run_gemm(g, s);
  float* out = g.out_f32;
  const float beta = g.beta;
  // a bias on a weight gradient is a row vector added to every row of dW (the tied matrix's -u under label smoothing, engine_train.cpp
  // head_fused_ce): the un-split launch above adds it in its epilogue, a split one where the slabs are summed
  const float* rowvec = g.bias;
  g.split_k = S; g.slab = slab; g.out_f32 = nullptr; g.beta = 0.f; g.bias = nullptr;
  KCHK(run_gemm(g, s));
  // KMB_SKIP_SLAB_REDUCE=1 (diagnostic build, TIMING ONLY -- the gradients are never written): what the 63 reduction launches of a
  // step cost where they run (b = 256: 0.62 of 15.85 ms, b = 512: 0.6 of 27.0, b = 1024: 0.6 of 49.7, b = 64: nothing).  Folding the
  // reduction into the GEMM -- the slices of a tile meet at a counter and the last one sums the slabs, write-through stores and
  // L2-bypassing loads so that it is correct across XCDs -- was built in round 5, bit-identical, and SLOWER (3072 x 768 x 8192 in
  // 7 slices: 80 -> 139 us; the step +2.5 % at b = 64, +5 % at 256, +4 % at 1024): slabs written through to memory and read back
  // past the L2 cost several times what the pass over L2- / Infinity-Cache-resident slabs costs (profiles/r05_grouped_weight_gradients.md)
  static const bool skip_reduce = KMB_DIAG_ENV("KMB_SKIP_SLAB_REDUCE") != nullptr;
  if (skip_reduce) return 0;
  if (rowvec) HIPCHK(kmb_reduce_slabs_rowvec_launch(slab, S, (size_t)g.M * g.N, out, (size_t)g.M * g.N, beta, rowvec, g.N, s));
  else HIPCHK(kmb_reduce_slabs_launch(slab, S, (size_t)g.M * g.N, out, (size_t)g.M * g.N, beta, s));
  return 0;
}

int ensure_side(kmb_handle* h) {
  if (!h->side_on || h->side != nullptr) return 0;
  const char* env = getenv("KMB_NO_SIDE_STREAM");
  if (env && env[0] == '1') { h->side_on = false; return 0; }
  {
    // The side stream carries the weight gradients, which nothing in backward waits for; the caller's stream carries the
    // critical path (data gradients, LayerNorm / attention backward, reducers).  KMB_SIDE_PRIORITY = low | high | default
    // picks the side stream's queue priority (experiment knob; default: the device's default priority).
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    const char* pr = KMB_DIAG_ENV("KMB_SIDE_PRIORITY");
    if (pr && (pr[0] == 'l' || pr[0] == 'h'))
      HIPCHK(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, pr[0] == 'l' ? least : greatest));
    else
      HIPCHK(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
  }
  h->ring.resize(1024);   // more than one backward pass records (~90): an event is never re-recorded while an earlier wait on it may be pending
  for (auto& e : h->ring) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  h->layer_done.resize(h->cfg.encoder_layers + h->cfg.decoder_layers + 2);
  for (auto& e : h->layer_done) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&h->head_wgrad_done, hipEventDisableTiming));
  return 0;
}

// Orders stream `to` behind everything enqueued on stream `from` so far: an event recorded on `from`, waited for on `to`.  The handle form
// takes the event from the ring (ensure_side), which is long enough that no event is re-recorded while a wait on it may be pending.
int order_behind(hipEvent_t e, hipStream_t from, hipStream_t to) {
  HIPCHK(hipEventRecord(e, from));
  HIPCHK(hipStreamWaitEvent(to, e, 0));
  return 0;
}
int order_behind(kmb_handle* h, hipStream_t from, hipStream_t to) { return order_behind(h->next_event(), from, to); }

// Weight gradients are off the critical path (nothing in backward reads them): enqueue them on the side stream
// behind an event that marks "everything the main stream has produced so far".  Two different GEMMs in flight are
// out of phase, so one's output-store burst overlaps the other's matrix work and partial waves get filled.
// Grouped weight gradients (csrc/gemm.hip, gemm_group_wgrad_kernel).  With few tokens a weight gradient has 36-144 output
// tiles and a short reduction: alone it needs a 3- to 7-fold split-K plus a slab reduction to cover the chip -- 63 + 91
// launches a step on the side stream, each GEMM behind an event pair.  A layer's four to six weight gradients together are
// 432-504 tiles: ONE launch, whole reductions, no slabs (16 launches a step).  wgrad_side() parks eligible problems in
// h->wg_pending while h->wg_group is set (kmb_backward: token count under the rule there); wgrad_flush() sends them out
// behind a marker of the caller's stream -- at the end of every layer, before that layer's completion events are recorded
// on the side stream.  The operands are per-layer buffers that stay valid until then (the layer_done rule).
// Measured (same box, alternating processes, profiles/r05_grouped_weight_gradients.md): the step gets faster for up to 48
// samples (b = 8: 5.89 -> 5.69 ms, 16: 5.54 -> 5.26, 32: 5.77 -> 5.59, 48: 6.66 -> 6.56) and slower from 64 on (7.25 -> 7.31,
// b = 128: 9.82 -> 10.10): the side stream's busy time falls from 3.1 to 1.8 ms at b = 64, but a launch that occupies every
// workgroup slot of the chip for 85-160 us holds up the caller's stream more than seven-fold split-K launches of 252
// workgroups did -- and without ANY weight gradient that step still takes 6.33 ms (diagnostic KMB_SKIP_WGRAD), without the
// optimizer 6.44: at that size the step is the caller's stream plus the 0.78 ms of AdamW traffic.
int wgrad_flush(kmb_handle* h, hipStream_t sA) {
  if (h->wg_pending.empty()) return 0;
  std::vector<KmbGemm> ps;
  ps.swap(h->wg_pending);
  const bool on_side = h->side_on && h->side != nullptr;
  hipStream_t s = on_side ? h->side : sA;
  if (on_side) KCHK(order_behind(h, sA, h->side));
  if (ps.size() == 1) return run_wgrad(h, ps[0], s, h->tl.slab, h->tl.slab_floats);   // nothing to group with
  if (g_prof.on) KCHK(prof_begin(s));
  HIPCHK(kmb_gemm_group_launch(ps.data(), (int)ps.size(), s));
  if (g_prof.on) {
    HIPCHK(hipEventRecord(g_prof.ev[g_prof.used + 1], s));
    double total = 0.0;
    for (const KmbGemm& g : ps) total += 2.0 * g.M * g.N * (double)g.K;
    for (size_t i = 0; i < ps.size(); ++i) {
      const KmbGemm& g = ps[i];
      const double fl = 2.0 * g.M * g.N * (double)g.K;
      g_prof.recs.push_back({0, fl, g.M, g.N, g.K, 0, 0, 0, g_prof.used / 2, (float)(fl / total), i == 0 ? 1 : 0, (int)ps.size()});
    }
    g_prof.used += 2;
  }
  return 0;
}

int wgrad_side(kmb_handle* h, const KmbGemm& g, hipStream_t sA) {
  if (h->wg_group && !g_f32 && kmb_gemm_group_check(&g, 1) == nullptr) {
    h->wg_pending.push_back(g);
    if ((int)h->wg_pending.size() == KMB_GEMM_GROUP_MAX) return wgrad_flush(h, sA);
    return 0;
  }
  KCHK(wgrad_flush(h, sA));   // (keeps the side stream's order: an ineligible problem goes out behind the parked ones)
  // KMB_SKIP_WGRAD=1 (diagnostic build, TIMING ONLY -- the gradients are wrong): no weight-gradient GEMM, no event.  What
  // the step costs without them bounds what any regrouping of the side stream's work can buy (tools/step_ab.sh)
  static const bool skip = KMB_DIAG_ENV("KMB_SKIP_WGRAD") != nullptr;
  if (skip) return 0;
  if (!h->side_on || h->side == nullptr) return run_wgrad(h, g, sA, h->tl.slab, h->tl.slab_floats);
  KCHK(order_behind(h, sA, h->side));
  KCHK(run_wgrad(h, g, h->side, h->tl.slab, h->tl.slab_floats));
  // KMB_SIDE_SERIALIZE=1 (diagnostic): the caller's stream waits for every weight gradient -- the side stream's
  // launches stay where they are, nothing overlaps (run-to-run reproducibility)
  static const bool serialize = KMB_DIAG_ENV("KMB_SIDE_SERIALIZE") != nullptr;
  if (serialize) KCHK(order_behind(h, h->side, sA));
  return 0;
}

// The reducers that fold partial sums into parameter gradients (LayerNorm gamma / beta, biases) produce nothing backward
// waits for: like the weight-gradient GEMMs they go to the side stream, behind an event that marks the producer of the
// partials on the caller's stream.  They are tiny (4-10 us alone) but sat on the critical path between two data-gradient
// GEMMs, where -- sharing the GPU with a weight-gradient GEMM of the side stream -- each took ~57 us (62 per step:
// rocprofv3 kernel stats of the overlapped step, profiles/r02_kernel_stats_b1024.md).  `parts` must not be rewritten
// before the side stream has read it: the per-site, per-layer-parity buffers of BwdBufs.
// Measured (whole step, same box, alternating processes, tools/step_ab_seq.sh): b = 1024 52.9 / 53.1 ms against 53.5 / 53.9
// with the reducers on the caller's stream; b = 256 16.50 / 16.55 against 16.21 / 16.39 -- the other way round (short
// backward: the extra events cost more than the reducers) -- so only long batches take this path.
hipStream_t reducer_stream(kmb_handle* h, hipStream_t sA) {
  static const char* env = KMB_DIAG_ENV("KMB_REDUCERS_ON_MAIN");   // "1": never on the side stream, "0": always (A/B knob)
  const bool want = env ? env[0] == '0' : (h->Me > h->Md ? h->Me : h->Md) >= 16384;
  if (!want || !h->side_on || h->side == nullptr) return sA;
  return order_behind(h, sA, h->side) == 0 ? h->side : sA;
}

// ---- launches that follow the precision mode (bf16 product kernels / fp32 validation kernels)
int attn_forward(kmb_handle* h, const AttnIO& io, int B, int H, bf16_t* o, float* lse, KmbDrop adr, hipStream_t s) {
  KmbAttn a; memset(&a, 0, sizeof(a));
  if (g_f32 && adr.thr16) return fail("fp32 validation mode runs without dropout");
  if (adr.thr16) { a.drop_thr16 = adr.thr16; a.drop_seed = adr.seed; a.drop_scale = adr.scale; }
  a.Q = io.q; a.K = io.k; a.V = io.v; a.ldq = io.ldq; a.ldk = io.ldkv; a.ldv = io.ldkv;
  a.B = B; a.H = H; a.Tq = io.Tq; a.Tk = io.Tk; a.key_mask = io.mask; a.causal = io.causal;
  a.O = o; a.ldo = h->d; a.lse = lse;
  if (g_f32) { HIPCHK(kmb_f32_attn_fwd_launch(a, s)); return 0; }
  const char* why = kmb_attn_check(a, 0);
  if (why) return fail("%s", why);
  HIPCHK(kmb_attn_fwd_launch(a, s));
  return 0;
}

int ln_forward(const bf16_t* z, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd, int M, int D,
               float eps, hipStream_t s) {
  if (g_f32) HIPCHK(kmb_f32_ln_fwd_launch((const float*)z, gamma, beta, (float*)y, mean, rstd, M, D, eps, s));
  else HIPCHK(kmb_ln_fwd_launch(z, gamma, beta, y, mean, rstd, M, D, eps, s));
  return 0;
}

int embed_ln_forward(const int64_t* ids, const int32_t* img_src, const float* E, const float* img_emb, const float* P,
                     int pos_base, int S, float scale, const float* gamma, const float* beta, bf16_t* z, bf16_t* y,
                     float* mean, float* rstd, int M, int D, float eps, KmbDrop drop, hipStream_t s) {
  if (g_f32) {
    if (drop.thr16) return fail("fp32 validation mode runs without dropout");
    HIPCHK(kmb_f32_embed_ln_fwd_launch(ids, img_src, E, img_emb, P, pos_base, S, scale, gamma, beta, (float*)z, (float*)y,
                                       mean, rstd, M, D, eps, s));
  } else {
    HIPCHK(kmb_embed_ln_fwd_launch(ids, img_src, E, img_emb, P, pos_base, S, scale, gamma, beta, z, y, mean, rstd, M, D,
                                   eps, drop, s));
  }
  return 0;
}

int attn_backward(kmb_handle* h, const AttnIO& io, int B, int H, bf16_t* o, float* lse, const bf16_t* dO, bf16_t* dq,
                  int lddq, bf16_t* dk, bf16_t* dv, int lddkv, float* cs_q, float* cs_k, float* cs_v, int ld_cs,
                  KmbDrop adr, hipStream_t s) {
  KmbAttn a; memset(&a, 0, sizeof(a));
  if (adr.thr16) { a.drop_thr16 = adr.thr16; a.drop_seed = adr.seed; a.drop_scale = adr.scale; }   // the forward's mask
  a.Q = io.q; a.K = io.k; a.V = io.v; a.ldq = io.ldq; a.ldk = io.ldkv; a.ldv = io.ldkv;
  a.B = B; a.H = H; a.Tq = io.Tq; a.Tk = io.Tk; a.key_mask = io.mask; a.causal = io.causal;
  a.O = o; a.ldo = h->d; a.lse = lse; a.dO = dO; a.lddo = h->d;
  a.dQ = dq; a.lddq = lddq; a.dK = dk; a.dV = dv; a.lddk = lddkv; a.lddv = lddkv; a.dq_scale = 0.125f;
  a.dq_colsum = cs_q; a.dk_colsum = cs_k; a.dv_colsum = cs_v; a.ld_colsum = ld_cs;
  const char* why = kmb_attn_check(a, 1);
  if (why) return fail("%s", why);
  HIPCHK(kmb_attn_bwd_launch(a, s));
  return 0;
}

// diagnostic: KMB_BWD_TRACE=1 checksums intermediate buffers of backward on their own stream (no synchronisation); the
// table is printed by kmb_debug_trace_dump.  Finds the first buffer that differs between two passes.
struct TraceRec { const char* name; int layer; };
std::vector<TraceRec> g_trace;
unsigned long long* g_trace_dev = nullptr;
bool g_trace_on = false;
int g_trace_layer = -1;
int trace(const char* name, const void* p, size_t bytes, hipStream_t s) {
  if (!g_trace_on) return 0;
  static const char* only = KMB_DIAG_ENV("KMB_BWD_TRACE_ONLY");   // substring filter: fewer probes disturb the timing less
  if (only && !strstr(name, only)) return 0;
  if (!g_trace_dev) HIPCHK(hipMalloc(&g_trace_dev, 4096 * sizeof(unsigned long long)));
  if (g_trace.size() >= 4096) return 0;
  HIPCHK(kmb_hash_words_launch(p, bytes, g_trace_dev + g_trace.size(), s));
  g_trace.push_back({name, g_trace_layer});
  return 0;
}

int check_bound(const kmb_handle* h) {
  if (!h->P || !h->G || !h->PB) return fail("arenas are not bound (kmb_bind_arenas)");
  if (!h->ws) return fail("workspace is not bound (kmb_bind_workspace)");
  return 0;
}

}  // namespace kmbi
using namespace kmbi;

// =============================================================================================
int kmb_set_error(const char* msg) { g_err = msg ? msg : ""; return 1; }

extern "C" {

const char* kmb_last_error(void) { return g_err.c_str(); }
int kmb_version(void) { return 1; }

int kmb_create(const kmb_config* cfg, kmb_handle** out) {
  if (!cfg || !out) return fail("kmb_create: null argument");
  if (cfg->d_model != cfg->encoder_attention_heads * 64 || cfg->d_model != cfg->decoder_attention_heads * 64)
    return fail("kmb_create: head_dim must be 64 (d_model=%d heads=%d/%d)", cfg->d_model, cfg->encoder_attention_heads,
                cfg->decoder_attention_heads);
  if (cfg->d_model > 2048) return fail("kmb_create: d_model > 2048 is not supported");
  if ((cfg->encoder_ffn_dim & 63) || (cfg->decoder_ffn_dim & 63)) return fail("kmb_create: ffn dims must be multiples of 64");
  if (cfg->attention_dropout != 0.f || cfg->activation_dropout != 0.f)
    return fail("kmb_create: attention_dropout / activation_dropout != 0 are not implemented (vcg_base uses 0.0)");
  kmb_handle* h = new kmb_handle();
  h->cfg = *cfg;
  if (h->cfg.layer_norm_eps <= 0.f) h->cfg.layer_norm_eps = 1e-5f;
  h->d = cfg->d_model; h->He = cfg->encoder_attention_heads; h->Hd = cfg->decoder_attention_heads;
  h->Fe = cfg->encoder_ffn_dim; h->Fd = cfg->decoder_ffn_dim; h->V = cfg->vocab_size;
  h->Vpad = (int)align_up((size_t)cfg->vocab_size, 128);
  h->Fin = cfg->image_feature_size; h->Fpad = (int)align_up((size_t)cfg->image_feature_size, 64);   // K of the image projection: a multiple of the GEMMs' K step
  h->Prows = cfg->max_position_embeddings + cfg->extra_pos_embeddings;
  const int d = h->d;
  h->img_w = add_param(h, "model.encoder.embed_images.linear.weight", d, h->Fin);
  h->img_b = add_param(h, "model.encoder.embed_images.linear.bias", 1, d);
  h->enc_pos = add_param(h, "model.encoder.embed_positions.weight", h->Prows, d);
  h->enc_lne_g = add_param(h, "model.encoder.layernorm_embedding.weight", 1, d);
  h->enc_lne_b = add_param(h, "model.encoder.layernorm_embedding.bias", 1, d);
  std::vector<size_t> marks;  // bucket boundaries in arena order
  h->attn_used[0].assign(cfg->encoder_layers, KmbDrop{0u, 0u, 1.f});
  h->attn_used[1].assign(cfg->decoder_layers, KmbDrop{0u, 0u, 1.f});
  h->attn_used[2].assign(cfg->decoder_layers, KmbDrop{0u, 0u, 1.f});
  h->act_used[0].assign(cfg->encoder_layers, KmbDrop{0u, 0u, 1.f});
  h->act_used[1].assign(cfg->decoder_layers, KmbDrop{0u, 0u, 1.f});
  h->enc.resize(cfg->encoder_layers);
  for (int l = 0; l < cfg->encoder_layers; ++l) {
    marks.push_back(align_up(h->arena, 64));
    const std::string p = "model.encoder.layers." + std::to_string(l) + ".";
    add_attn(h, p + "self_attn.", p + "self_attn_layer_norm", h->enc[l].sa);
    add_ffn(h, p, h->Fe, h->enc[l]);
  }
  marks.push_back(align_up(h->arena, 64));
  h->dec_pos = add_param(h, "model.decoder.embed_positions.weight", h->Prows, d);
  h->dec_lne_g = add_param(h, "model.decoder.layernorm_embedding.weight", 1, d);
  h->dec_lne_b = add_param(h, "model.decoder.layernorm_embedding.bias", 1, d);
  h->dec.resize(cfg->decoder_layers);
  // every layer's cross-attention k | v weights, then their biases: part of the decoder-embedding segment of the arena
  // (its gradients are complete when the batched weight gradient behind the last decoder layer's backward has run)
  h->xkv_w = align_up(h->arena, 64);
  for (int l = 0; l < cfg->decoder_layers; ++l) {
    const std::string p = "model.decoder.layers." + std::to_string(l) + ".encoder_attn.";
    h->dec[l].ca_kv_w = add_param(h, p + "k_proj.weight", d, d);
    add_param(h, p + "v_proj.weight", d, d);
  }
  h->xkv_b = align_up(h->arena, 64);
  for (int l = 0; l < cfg->decoder_layers; ++l) {
    const std::string p = "model.decoder.layers." + std::to_string(l) + ".encoder_attn.";
    h->dec[l].ca_kv_b = add_param(h, p + "k_proj.bias", 1, d);
    add_param(h, p + "v_proj.bias", 1, d);
  }
  for (int l = 0; l < cfg->decoder_layers; ++l) {
    marks.push_back(align_up(h->arena, 64));
    const std::string p = "model.decoder.layers." + std::to_string(l) + ".";
    add_attn(h, p + "self_attn.", p + "self_attn_layer_norm", h->dec[l].sa);
    add_cross_attn(h, p + "encoder_attn.", p + "encoder_attn_layer_norm", h->dec[l].ca);
    add_ffn(h, p, h->Fd, h->dec[l]);
  }
  marks.push_back(align_up(h->arena, 64));
  {  // BartClassificationHead: dense -> tanh -> out_proj
    const char* names[3] = {"mrm_head", "attribute_head", "relation_head"};
    const int C[3] = {cfg->num_labels, cfg->num_attributes, cfg->num_relations};
    h->heads_begin = align_up(h->arena, 64);
    for (int k = 0; k < 3; ++k) {
      if (C[k] <= 0) continue;
      HeadP& H = h->head[k];
      H.on = true; H.C = C[k]; H.d_in = (k == 2) ? 2 * d : d;
      const std::string n = names[k];
      H.dw = add_param(h, n + ".dense.weight", d, H.d_in);
      H.db = add_param(h, n + ".dense.bias", 1, d);
      H.ow = add_param(h, n + ".out_proj.weight", H.C, d);
      H.ob = add_param(h, n + ".out_proj.bias", 1, H.C);
    }
    h->heads_end = align_up(h->arena, 64);
  }
  h->shared = add_param(h, "model.shared.weight", h->V, d);
  h->arena = align_up(h->arena, 64);
  // arena segments: [0,m0) enc embed+img | enc layers | dec embed | dec layers | shared
  // completion order in backward: dec layers (last..first), dec embed, enc layers (last..first), enc embed, shared
  const int Le = cfg->encoder_layers, Ld = cfg->decoder_layers;
  auto seg = [&](size_t a, size_t b) { h->buckets.push_back({a, b - a}); };
  for (int l = Ld - 1; l >= 0; --l) seg(marks[Le + 1 + l], marks[Le + 2 + l]);
  // (the decoder-layer-0 segment ends where the heads begin; the heads' gradients are complete after forward and
  //  ride in the last bucket together with the tied matrix)
  seg(marks[Le], marks[Le + 1]);
  for (int l = Le - 1; l >= 0; --l) seg(marks[l], marks[l + 1]);
  seg(0, marks[0]);
  seg(h->heads_begin, h->arena);  // heads (if any) + tied matrix
  h->events.resize(h->buckets.size());
  for (auto& e : h->events) {
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      // no device (CPU build container): events are created lazily in kmb_backward instead
      e = nullptr;
      (void)hipGetLastError();
    }
  }
  const char* ch = KMB_DIAG_ENV("KMB_LM_CHUNK");
  if (ch && atoi(ch) > 0) h->lm_chunk = atoi(ch);
  *out = h;
  return 0;
}

void kmb_destroy(kmb_handle* h) {
  if (!h) return;
  for (auto e : h->events) if (e) (void)hipEventDestroy(e);
  for (auto e : h->ring) if (e) (void)hipEventDestroy(e);
  for (auto e : h->layer_done) if (e) (void)hipEventDestroy(e);
  if (h->head_wgrad_done) (void)hipEventDestroy(h->head_wgrad_done);
  if (h->side) (void)hipStreamDestroy(h->side);
  (void)kmb_comm_destroy(h);
  delete h;
}

int kmb_param_count(const kmb_handle* h) { return (int)h->params.size(); }
int kmb_param_info(const kmb_handle* h, int idx, const char** name, int64_t* offset, int32_t* rows, int32_t* cols) {
  if (idx < 0 || idx >= (int)h->params.size()) return fail("kmb_param_info: index %d out of range", idx);
  const ParamInfo& p = h->params[idx];
  if (name) *name = p.name.c_str();
  if (offset) *offset = (int64_t)p.off;
  if (rows) *rows = p.rows;
  if (cols) *cols = p.cols;
  return 0;
}
int64_t kmb_arena_elems(const kmb_handle* h) { return (int64_t)h->arena; }
int64_t kmb_bf16_arena_elems(const kmb_handle* h) {
  // mirror + zero rows padding the tied matrix to Vpad + padded image weight [d, Fpad]
  return (int64_t)(h->shared + (size_t)h->Vpad * h->d + (size_t)h->d * h->Fpad + 64);
}
int kmb_logits_ld(const kmb_handle* h) { return h->Vpad; }

int kmb_bind_arenas(kmb_handle* h, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                    kmb_bf16* params_bf16, float* final_logits_bias) {
  if (!params || !params_bf16 || !final_logits_bias) return fail("kmb_bind_arenas: params, bf16 mirror and final_logits_bias are required");
  if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)params_bf16) & 255)
    return fail("kmb_bind_arenas: arenas must be 256-byte aligned");
  h->P = params; h->G = grads; h->M1 = exp_avg; h->M2 = exp_avg_sq; h->PB = params_bf16; h->flb = final_logits_bias;
  h->imgw_pad = h->PB + align_up(h->shared + (size_t)h->Vpad * h->d, 64);
  h->mirror_version++;
  return 0;
}

int kmb_bind_workspace(kmb_handle* h, void* ws, int64_t bytes) {
  if (((uintptr_t)ws) & 255) return fail("kmb_bind_workspace: workspace must be 256-byte aligned");
  h->ws = (char*)ws; h->ws_bytes = (size_t)bytes; h->have_fwd = false; h->have_hdec = false; h->gen.active = false; h->gen.packed_at = nullptr;
  return 0;
}

// ---- gradient accumulation (include/kmbart.h; the folds are kmb_backward's, engine_train.cpp)
int kmb_bind_grad_stage(kmb_handle* h, float* stage, int64_t floats) {
  if (!h) return fail("kmb_bind_grad_stage: null handle");
  if (h->accum) return fail("kmb_bind_grad_stage: switch accumulation off before binding another stage");
  if (!stage) { h->GS = nullptr; h->stage_floats = 0; return 0; }
  if (floats < 0 || (size_t)floats < h->arena) return fail("kmb_bind_grad_stage: the stage holds %lld floats, the arena %zu", (long long)floats, h->arena);
  if ((uintptr_t)stage & 255) return fail("kmb_bind_grad_stage: the stage must be 256-byte aligned");
  if (h->ws && (char*)stage < h->ws + h->ws_bytes && (char*)(stage + floats) > h->ws) return fail("kmb_bind_grad_stage: the stage lies inside the workspace");
  if (h->G && stage < h->G + h->arena && stage + floats > h->G) return fail("kmb_bind_grad_stage: the stage overlaps the gradient arena");
  h->GS = stage; h->stage_floats = (size_t)floats;
  return 0;
}

int kmb_set_grad_accumulation(kmb_handle* h, int on) {
  if (!h) return fail("kmb_set_grad_accumulation: null handle");
  if (h->have_fwd) return fail("kmb_set_grad_accumulation: a need_grad forward is waiting for its backward (its gradients are already written)");
  if (on && !h->GS) return fail("kmb_set_grad_accumulation: no stage is bound (kmb_bind_grad_stage)");
  if (on && !h->accum) h->grad_fresh = true;
  h->accum = on != 0;
  return 0;
}

int kmb_zero_grad(kmb_handle* h) {
  if (!h) return fail("kmb_zero_grad: null handle");
  h->grad_fresh = true;
  return 0;
}

int kmb_set_seed(kmb_handle* h, uint64_t seed) { h->seed = seed; h->step = 0; return 0; }

int kmb_set_attention_dropout(kmb_handle* h, float p) {
  if (!h) return fail("kmb_set_attention_dropout: null handle");
  if (!(p >= 0.f && p < 1.f)) return fail("kmb_set_attention_dropout: the probability must be in [0, 1), got %g", (double)p);   // (NaN fails both)
  h->attn_p = p;
  return 0;
}

int kmb_attention_dropout_site(kmb_handle* h, int kind, int layer, uint32_t* thr16, uint32_t* seed) {
  if (!h || !thr16 || !seed) return fail("kmb_attention_dropout_site: null argument");
  if (kind < 0 || kind > 2) return fail("kmb_attention_dropout_site: kind must be 0 (encoder self), 1 (decoder self) or 2 (decoder cross)");
  if (layer < 0 || layer >= (int)h->attn_used[kind].size()) return fail("kmb_attention_dropout_site: no layer %d", layer);
  const KmbDrop& dr = h->attn_used[kind][layer];
  *thr16 = dr.thr16; *seed = dr.thr16 ? dr.seed : 0u;
  return 0;
}

int kmb_set_activation_dropout(kmb_handle* h, float p) {
  if (!h) return fail("kmb_set_activation_dropout: null handle");
  if (!(p >= 0.f && p < 1.f)) return fail("kmb_set_activation_dropout: the probability must be in [0, 1), got %g", (double)p);   // (NaN fails both)
  h->act_p = p;
  return 0;
}

int kmb_activation_dropout_site(kmb_handle* h, int kind, int layer, uint32_t* thr16, uint32_t* seed) {
  if (!h || !thr16 || !seed) return fail("kmb_activation_dropout_site: null argument");
  if (kind < 0 || kind > 1) return fail("kmb_activation_dropout_site: kind must be 0 (encoder FFN) or 1 (decoder FFN)");
  if (layer < 0 || layer >= (int)h->act_used[kind].size()) return fail("kmb_activation_dropout_site: no layer %d", layer);
  const KmbDrop& dr = h->act_used[kind][layer];
  *thr16 = dr.thr16; *seed = dr.thr16 ? dr.seed : 0u;
  return 0;
}

int kmb_set_classif_dropout(kmb_handle* h, float p) {
  if (!h) return fail("kmb_set_classif_dropout: null handle");
  if (!(p >= 0.f && p < 1.f)) return fail("kmb_set_classif_dropout: the probability must be in [0, 1), got %g", (double)p);   // (NaN fails both)
  h->cls_p = p;
  return 0;
}

int kmb_set_label_smoothing(kmb_handle* h, float eps) {
  if (!h) return fail("kmb_set_label_smoothing: null handle");
  if (!(eps >= 0.f && eps < 1.f)) return fail("kmb_set_label_smoothing: eps must be in [0, 1), got %g", (double)eps);   // (NaN fails both)
  h->label_smoothing = eps;
  return 0;
}

int kmb_last_head_form(const kmb_handle* h) { return h ? h->last_head_form : -1; }

int kmb_classif_dropout_site(kmb_handle* h, int head, int which, uint32_t* thr16, uint32_t* seed) {
  if (!h || !thr16 || !seed) return fail("kmb_classif_dropout_site: null argument");
  if (head < 0 || head > 2) return fail("kmb_classif_dropout_site: head must be 0 (masked-region), 1 (attribute) or 2 (relation)");
  if (which < 0 || which > 1) return fail("kmb_classif_dropout_site: which must be 0 (the head's input) or 1 (its hidden activations)");
  const KmbDrop& dr = h->cls_used[head][which];
  *thr16 = dr.thr16; *seed = dr.thr16 ? dr.seed : 0u;
  return 0;
}

int kmb_abi_sizeof_attn(void) { return (int)sizeof(KmbAttn); }
int kmb_abi_sizeof_forward_opts(void) { return (int)sizeof(kmb_forward_opts); }

int kmb_sync_params(kmb_handle* h, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!h->P || !h->PB) return fail("kmb_sync_params: arenas are not bound");
  HIPCHK(kmb_cast_f32_bf16_launch(h->P, h->PB, h->arena, s));
  h->mirror_version++;
  // zero rows [V, Vpad) of the tied matrix mirror; padded image weight [d, Fpad]
  HIPCHK(hipMemsetAsync(h->PB + h->shared + (size_t)h->V * h->d, 0, (size_t)(h->Vpad - h->V) * h->d * sizeof(bf16_t), s));
  HIPCHK(kmb_cast_rows_launch(h->pf(h->img_w), h->Fin, h->imgw_pad, h->Fpad, h->d, h->Fin, s));
  return 0;
}

int kmb_bucket_count(const kmb_handle* h) { return (int)h->buckets.size(); }
int kmb_bucket_range(const kmb_handle* h, int i, int64_t* offset, int64_t* count) {
  if (i < 0 || i >= (int)h->buckets.size()) return fail("kmb_bucket_range: index out of range");
  *offset = (int64_t)h->buckets[i].off; *count = (int64_t)h->buckets[i].count;
  return 0;
}
int kmb_stream_wait_bucket(kmb_handle* h, int i, void* stream) {
  if (i < 0 || i >= (int)h->events.size() || !h->events[i]) return fail("kmb_stream_wait_bucket: no event %d", i);
  HIPCHK(hipStreamWaitEvent((hipStream_t)stream, h->events[i], 0));
  return 0;
}

static int read_status(kmb_handle* h, const char* who, int32_t* status_host, hipStream_t s, bool wait) {
  if (!h->status) return fail("%s: no forward has run", who);
  HIPCHK(hipMemcpyAsync(status_host, h->status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (wait) HIPCHK(hipStreamSynchronize(s));
  return 0;
}
int kmb_read_status(kmb_handle* h, int32_t* status_host, void* stream) { return read_status(h, "kmb_read_status", status_host, (hipStream_t)stream, true); }
int kmb_read_status_async(kmb_handle* h, int32_t* status_host, void* stream) { return read_status(h, "kmb_read_status_async", status_host, (hipStream_t)stream, false); }

int kmb_set_precision(kmb_handle* h, int fp32) {
  h->fp32 = fp32 != 0; h->have_fwd = false; h->have_hdec = false; h->gen.active = false;
  return 0;
}
int kmb_act_bytes(const kmb_handle* h) { return h->fp32 ? 4 : 2; }

int kmb_reserve_head_rows(kmb_handle* h, int n) {
  if (n < 0) return fail("kmb_reserve_head_rows: negative row count");
  h->head_rows_cap = n;
  return 0;
}

// diagnostic: start (on = 1) / stop recording buffer checksums in backward; dump prints "index layer name checksum"
int kmb_debug_trace(int on) {
  g_trace_on = on != 0;
  if (on) g_trace.clear();
  return 0;
}
int kmb_debug_trace_dump(const char* path) {
  HIPCHK(hipDeviceSynchronize());
  std::vector<unsigned long long> hst(g_trace.size());
  if (!hst.empty()) HIPCHK(hipMemcpy(hst.data(), g_trace_dev, hst.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  FILE* f = fopen(path, "w");
  if (!f) return fail("kmb_debug_trace_dump: cannot open %s", path);
  for (size_t i = 0; i < hst.size(); ++i) fprintf(f, "%zu %d %s %016llx\n", i, g_trace[i].layer, g_trace[i].name, hst[i]);
  fclose(f);
  return 0;
}

// 0: weight-gradient GEMMs stay on the caller's stream (serial backward; used while timing single kernels)
int kmb_set_side_stream(kmb_handle* h, int enable) {
  h->side_on = enable != 0;
  return 0;
}

int kmb_profile_gemm(int enable) {
  g_prof.on = enable != 0;
  if (enable) { g_prof.used = 0; g_prof.recs.clear(); }
  return 0;
}

// variant index = a_kc*2 + b_kc (3: forward, 2: dgrad, 0: wgrad).  Synchronises the events.
int kmb_profile_read(int variant, int64_t* launches, double* total_ms, double* total_flops) {
  int64_t n = 0; double ms = 0, fl = 0;
  for (size_t i = 0; i < g_prof.recs.size(); ++i) {
    if (g_prof.recs[i].variant != variant) continue;
    float t = 0.f;
    const size_t pr = g_prof.recs[i].pair;
    HIPCHK(hipEventSynchronize(g_prof.ev[2 * pr + 1]));
    HIPCHK(hipEventElapsedTime(&t, g_prof.ev[2 * pr], g_prof.ev[2 * pr + 1]));
    ms += t * g_prof.recs[i].share; fl += g_prof.recs[i].flops; n += g_prof.recs[i].launch;
  }
  *launches = n; *total_ms = ms; *total_flops = fl;
  return 0;
}

// one line per GEMM problem of the profiled calls: variant M N K split act microseconds residual group -- `group` = n for a
// problem that went out as one of the n of a grouped weight-gradient launch (its microseconds are its FLOP share of that
// launch), 1 for a launch of its own
int kmb_profile_dump(const char* path) {
  FILE* f = fopen(path, "w");
  if (!f) return fail("kmb_profile_dump: cannot open %s", path);
  for (size_t i = 0; i < g_prof.recs.size(); ++i) {
    float t = 0.f;
    const auto& r = g_prof.recs[i];
    HIPCHK(hipEventSynchronize(g_prof.ev[2 * r.pair + 1]));
    HIPCHK(hipEventElapsedTime(&t, g_prof.ev[2 * r.pair], g_prof.ev[2 * r.pair + 1]));
    fprintf(f, "%d %d %d %d %d %d %.3f %d %d\n", r.variant, r.M, r.N, r.K, r.split, r.act, t * r.share * 1e3, r.res, r.group_n);   // res: the epilogue reads a residual operand
  }
  fclose(f);
  return 0;
}

}  // extern "C"
