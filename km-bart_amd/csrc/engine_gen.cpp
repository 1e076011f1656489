// Generation: the decode workspace, kmb_gen_begin (encoder + cross-attention keys | values + weight packing), the decode step and the
// step entry points that choose the next tokens.
#include "engine_internal.h"
#include "beam_process.h"
#include "beam_sample.h"
#include "greedy.h"
#include "logits_process.h"
#include "sample.h"

using namespace kmbi;

namespace {

constexpr int GEN_MAX_SPLIT = 12;

// the fused decode blocks need d_model = 768 (one 768-deep weight block per attention projection, 64-wide heads) and an
// FFN width of 768 .. 3072 in steps of 768
bool gen_fused_eligible(const kmb_handle* h) {
  return h->d == 768 && h->Hd * 64 == h->d && (h->Fd % 768) == 0 && h->Fd <= 3072 && (h->Fd % 64) == 0;
}

size_t layout_gen(const kmb_handle* h, char* base, size_t cap, int B, int S, int nb, int Tmax, int Ntot, GenLayout* out) {
  const int d = h->d, Fe = h->Fe, Fd = h->Fd, Ld = h->cfg.decoder_layers;
  const size_t Me = (size_t)B * S, R = (size_t)B * nb;
  Bump bp(base, cap);
  GenLayout g;
  g.status = bp.take<int32_t>(4);
  g.xf = bp.act((size_t)(Ntot > 0 ? Ntot : 1) * h->Fpad);
  g.img_emb = bp.take<float>((size_t)(Ntot > 0 ? Ntot : 1) * d);
  g.img_src = bp.take<int32_t>(Me);
  g.xe[0] = bp.act(Me * d); g.xe[1] = bp.act(Me * d);
  EncAct& a = g.ea;
  a.qkv = bp.act(Me * 3 * d); a.o = bp.act(Me * d); a.z1 = bp.act(Me * d);
  a.y1 = bp.act(Me * d); a.u = bp.act(Me * Fe); a.hh = bp.act(Me * Fe);
  a.z2 = bp.act(Me * d); a.lse = bp.take<float>((size_t)B * h->He * S);
  a.m1 = bp.take<float>(Me); a.r1 = bp.take<float>(Me); a.m2 = bp.take<float>(Me); a.r2 = bp.take<float>(Me);
  g.ckv.resize(Ld);
  g.kc.resize(Ld); g.vc.resize(Ld);
  bf16_t* ckv_all = bp.act(Me * (size_t)Ld * 2 * d);   // [Me, Ld * 2d]: layer l's cross-attention k | v are columns [l * 2d, (l + 1) * 2d)
  for (int l = 0; l < Ld; ++l) {
    g.ckv[l] = ckv_all + (size_t)l * 2 * d;
    g.kc[l] = bp.act(R * Tmax * d); g.vc[l] = bp.act(R * Tmax * d);
  }
  g.kv_row = bp.take<int32_t>(2 * R);   // two copies: a reorder of independent rows (num_beams == 1) gathers it into the other one
  g.x0 = bp.act(R * d); g.x1 = bp.act(R * d); g.qkv = bp.act(R * 3 * d);
  g.o = bp.act(R * d); g.z = bp.act(R * d); g.y = bp.act(R * d); g.cq = bp.act(R * d);
  g.u = bp.act(R * Fd); g.hh = bp.act(R * Fd);
  g.mean = bp.take<float>(R); g.rstd = bp.take<float>(R);
  g.slab = bp.take<float>((size_t)GEN_MAX_SPLIT * R * d);
  if (gen_fused_eligible(h)) {
    const size_t dd = (size_t)d * d, fd = (size_t)Fd * d;
    const size_t sizes[6] = {3 * dd, dd, dd, dd, fd, fd};
    const size_t rows[6] = {3 * (size_t)d, (size_t)d, (size_t)d, (size_t)d, (size_t)Fd, (size_t)d};
    const bool f8 = h->gen.w_format == KMB_WFMT_FP8_E4M3;   // one byte per element and one exponent per weight row
    for (int l = 0; l < Ld; ++l)
      for (int i = 0; i < 6; ++i) {
        if (f8) {
          g.wp.push_back(reinterpret_cast<bf16_t*>(bp.take<uint8_t>(sizes[i])));
          g.wexp.push_back(bp.take<int8_t>(rows[i]));
        } else {
          g.wp.push_back(bp.act(sizes[i]));
        }
      }
  }
  g.hist[0] = bp.take<int32_t>(R * Tmax); g.hist[1] = bp.take<int32_t>(R * Tmax);
  g.head_stats = bp.take<float>(kmb_gemm_allrows_stats_floats(h->V));
  if (out) *out = g;
  return bp.used();
}

}  // namespace

extern "C" {

int64_t kmb_gen_workspace_bytes(const kmb_handle* h, int B, int S, int num_beams, int max_length, int n_features) {
  return (int64_t)layout_gen(h, nullptr, 0, B, S, num_beams, max_length, n_features, nullptr);
}

// FP8 decoder weights exist only in the fused decode blocks: why a generation of `rows` rows cannot run on them (NULL: it can).  There
// is no bf16 fall-back -- it would return other tokens.
static const char* fp8_refusal(const kmb_handle* h, long long rows) {
  if (!gen_fused_eligible(h))
    return "the fused decode blocks do not take this configuration (d_model 768, 64-wide heads, decoder FFN 768 .. 3072 in steps of 768)";
  if (h->fp32) return "the fp32 validation mode has no generation and no reduced-precision weights";
  const char* fused_env = getenv("KMB_GEN_FUSED");
  if (fused_env && fused_env[0] == '0') return "KMB_GEN_FUSED=0 selects the launch-per-operation path, which reads bf16 weights";
  if (rows > 1024) return "more than 1024 rows (batch x beams) take the GEMM path, which reads bf16 weights";
  return nullptr;
}

int kmb_gen_set_weight_format(kmb_handle* h, int format) {
  if (!h) return fail("kmb_gen_set_weight_format: null handle");
  if (format != KMB_WFMT_BF16 && format != KMB_WFMT_FP8_E4M3)
    return fail("kmb_gen_set_weight_format: unknown weight format %d (0 = bf16, 1 = FP8 e4m3)", format);
  if (format == KMB_WFMT_FP8_E4M3 && !gen_fused_eligible(h))
    return fail("kmb_gen_set_weight_format: FP8 decoder weights need the fused decode blocks: %s", fp8_refusal(h, 0));
  h->gen.w_format = format;
  h->gen.active = false;   // the active generation's copies are in the other format and the workspace is sized anew
  return 0;
}

int kmb_gen_begin(kmb_handle* h, const kmb_batch* batch, int num_beams, int max_length, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KCHK(check_bound(h));
  if (!batch || !batch->input_ids || !batch->feat_offsets) return fail("kmb_gen_begin: input_ids and feat_offsets are required");
  if (num_beams < 1 || max_length < 2) return fail("kmb_gen_begin: bad num_beams / max_length");
  if (max_length > h->cfg.max_position_embeddings) return fail("kmb_gen_begin: max_length exceeds max_position_embeddings");
  const kmb_batch& bt = *batch;
  const int d = h->d, B = bt.B, S = bt.S, Me = B * S;
  const bool f8 = h->gen.w_format == KMB_WFMT_FP8_E4M3;
  if (f8) {   // before anything is queued
    if (const char* why = fp8_refusal(h, (long long)B * num_beams)) {
      h->gen.active = false;
      return fail("kmb_gen_begin: FP8 decoder weights: %s", why);
    }
  }
  GenLayout g;
  const size_t need = layout_gen(h, h->ws, h->ws_bytes, B, S, num_beams, max_length, bt.n_features, &g);
  if (need > h->ws_bytes) return fail("kmb_gen_begin: workspace too small (%zu > %zu bytes)", need, h->ws_bytes);
  if (h->fp32) return fail("kmb_gen_begin: generation is not available in the fp32 validation mode");
  h->have_fwd = false; h->have_hdec = false;   // the training layout's buffers are overwritten from here on
  const int Le = h->cfg.encoder_layers, Ld = h->cfg.decoder_layers;
  h->status = g.status;
  HIPCHK(hipMemsetAsync(h->status, 0, 16, s));
  KCHK(encoder_forward(h, g.encoder(), bt, false, s));   // (over the layer-shared generation buffers)
  auto& G = h->gen;
  G.active = true; G.B = B; G.S = S; G.nb = num_beams; G.R = B * num_beams; G.Tmax = max_length; G.bt = bt;
  G.L = std::move(g);
  G.kv_row = G.L.kv_row; G.hcur = 0; G.x0_step = -1;
  G.last_x = nullptr; G.last_z = nullptr; G.last_g = nullptr; G.last_b = nullptr;
  G.head_stats_blocks = 0; G.head_stats_for = nullptr;
  const bf16_t* enc = G.L.xe[Le & 1];
  // cross-attention K|V of every decoder layer, computed once per batch item (not per beam), all layers in ONE GEMM
  if (Ld > 0) {
    KmbGemm gm = lin_fwd(enc, d, h->wb(h->xkv_w), h->pf(h->xkv_b), Me, Ld * 2 * d, d);
    gm.out_bf16 = G.L.ckv[0]; gm.ld_out_bf16 = Ld * 2 * d;
    KCHK(run_gemm(gm, s));
  }
  // (skipped when the copies of the last kmb_gen_begin are still there: same place in the workspace, the bf16 mirror unchanged since,
  //  no training forward in between -- that one re-uses the workspace and clears packed_at)
  if (!G.L.wp.empty() && !(G.packed_at == G.L.wp[0] && G.packed_version == h->mirror_version && G.packed_format == G.w_format)) {   // fragment-order copies of the decoder weights for the fused decode blocks, one launch per 48
    std::vector<const bf16_t*> src; std::vector<bf16_t*> dst; std::vector<int> ld, nn, kk;
    for (int l = 0; l < Ld; ++l) {
      const LayerP& L = h->dec[l];
      const size_t offs[6] = {L.sa.qkv_w, L.sa.o_w, L.ca.qkv_w, L.ca.o_w, L.fc1_w, L.fc2_w};
      const int N6[6] = {3 * d, d, d, d, h->Fd, d}, K6[6] = {d, d, d, d, d, h->Fd};
      for (int i = 0; i < 6; ++i) {
        src.push_back(h->wb(offs[i])); dst.push_back(G.L.wp[(size_t)l * 6 + i]); ld.push_back(K6[i]); nn.push_back(N6[i]); kk.push_back(K6[i]);
      }
    }
    for (size_t i0 = 0; i0 < src.size(); i0 += 48) {
      const int n = (int)std::min<size_t>(48, src.size() - i0);
      if (f8)   // (the same slots hold codes, and the exponents go beside them)
        HIPCHK(kmb_decode_pack_fp8_launch(src.data() + i0, ld.data() + i0, nn.data() + i0, kk.data() + i0,
                                          reinterpret_cast<uint8_t* const*>(dst.data() + i0), G.L.wexp.data() + i0, n, s));
      else
        HIPCHK(kmb_decode_pack_launch(src.data() + i0, ld.data() + i0, nn.data() + i0, kk.data() + i0, dst.data() + i0, n, s));
    }
    G.packed_at = G.L.wp[0]; G.packed_version = h->mirror_version; G.packed_format = G.w_format;
  }
  // beam row -> batch item, written on the device: a host table needed a copy and a stream synchronisation here, and the
  // host then sat out the encoder (1.1 ms at batch 64) instead of queueing the first decode steps behind it
  HIPCHK(kmb_iota_div_launch(G.kv_row, G.R, num_beams, s));
  return 0;
}

int kmb_gen_encoder_states(kmb_handle* h, kmb_bf16* enc_out, void* stream) {
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_encoder_states: call kmb_gen_begin first");
  if (!enc_out) return fail("kmb_gen_encoder_states: enc_out is required");
  const bf16_t* enc = G.L.xe[h->cfg.encoder_layers & 1];
  HIPCHK(hipMemcpyAsync(enc_out, enc, (size_t)G.B * G.S * h->d * sizeof(bf16_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int kmb_gen_step(kmb_handle* h, const int64_t* tokens, int step, float* logits_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_step: call kmb_gen_begin first");
  if (step < 0 || step >= G.Tmax) return fail("kmb_gen_step: step %d outside the cache (Tmax=%d)", step, G.Tmax);
  const int d = h->d, R = G.R, F = h->Fd;
  const float eps = h->cfg.layer_norm_eps;
  const float scale = h->cfg.scale_embedding ? sqrtf((float)d) : 1.f;
  const KmbDrop nodrop{0u, 0u, 1.f};
  // BartDecoder with use_cache: only the last token, learned position (len-1) + 2.  tokens = NULL: the caller asks for the rows the
  // preceding kmb_gen_beam_step(reorder_step = step - 1) embedded from the tokens it chose (same row code) -- requested, never
  // inferred from an address: a caller may have edited that buffer since, or the allocator handed it to another tensor
  if (!tokens) {
    if (G.x0_step != step)
      return fail("kmb_gen_step: tokens = NULL but no kmb_gen_beam_step embedded the tokens of step %d (pending: %d)", step, G.x0_step);
  } else {
    HIPCHK(kmb_embed_ln_fwd_launch(tokens, nullptr, h->pf(h->shared), nullptr, h->pf(h->dec_pos),
                                   h->cfg.extra_pos_embeddings + step, 1, scale, h->pf(h->dec_lne_g),
                                   h->pf(h->dec_lne_b), nullptr, G.L.x0, nullptr, nullptr, R, d, eps, nodrop, s));
  }
  G.x0_step = -1;
  bf16_t* x = G.L.x0; bf16_t* xn = G.L.x1;
  // residual projection + LayerNorm (BartDecoderLayer: x = LN(residual + dropout(proj(x)))).  With R = batch x beams rows
  // the projection has 18 output tiles of 128 x 128 and a serial K loop: split K over workgroups and let ONE kernel sum
  // the slabs, add bias and residual and normalise (no GEMM epilogue, no separate LayerNorm launch).
  auto proj_ln = [&](const bf16_t* in, int K, size_t w_off, size_t b_off, const bf16_t* res, size_t g_off, size_t be_off,
                     bf16_t* out) -> int {
    const int nt = K / 64;
    static const int s_small = KMB_DIAG_ENV("KMB_GEN_SPLIT_SMALL") ? atoi(KMB_DIAG_ENV("KMB_GEN_SPLIT_SMALL")) : 3;   // tuning knobs
    static const int s_large = KMB_DIAG_ENV("KMB_GEN_SPLIT_LARGE") ? atoi(KMB_DIAG_ENV("KMB_GEN_SPLIT_LARGE")) : 6;
    int S = K >= 2048 ? s_large : s_small;
    if (S > nt / 2) S = nt / 2;
    if (S > GEN_MAX_SPLIT) S = GEN_MAX_SPLIT;
    if (S > 1 && (K % 64) == 0 && (d & 7) == 0 && d <= 1024) {
      KmbGemm g = lin_fwd(in, K, h->wb(w_off), nullptr, R, d, K);
      g.split_k = S; g.slab = G.L.slab; g.out_bf16 = nullptr; g.out_f32 = nullptr;
      KCHK(run_gemm(g, s));
      HIPCHK(kmb_ln_fwd_slabs_launch(G.L.slab, S, (size_t)R * d, h->pf(b_off), res, d, h->pf(g_off), h->pf(be_off), out, R, d,
                                     eps, s));
      return 0;
    }
    KmbGemm g = lin_fwd(in, K, h->wb(w_off), h->pf(b_off), R, d, K);
    g.residual = res; g.ld_res = d; g.out_bf16 = G.L.z; g.ld_out_bf16 = d;
    KCHK(run_gemm(g, s));
    HIPCHK(kmb_ln_fwd_launch(G.L.z, h->pf(g_off), h->pf(be_off), out, G.L.mean, G.L.rstd, R, d, eps, s));
    return 0;
  };
  // Fused form (csrc/decode.hip): six launches per layer, the LayerNorms folded into the consumers, weights read from
  // the fragment-order copies made by kmb_gen_begin.  Configurations gen_fused_eligible() rejects, and KMB_GEN_FUSED=0,
  // take the launch-per-operation path below.
  const char* fused_env = getenv("KMB_GEN_FUSED");   // read per call: tests compare the two paths in one process
  // the blocks work on 16-row tiles that each stream the layer's weights through L2: their time grows with the rows, while
  // the 128-row GEMM tiles of the launch-per-operation path amortise the weights (even at 1280 rows, faster below)
  const bool fused = !(fused_env && fused_env[0] == '0') && !G.L.wp.empty() && R <= 1024;
  const bool f8 = G.w_format == KMB_WFMT_FP8_E4M3;
  if (f8 && !fused) {   // (kmb_gen_begin has checked; the environment may have changed since)
    const char* why = fp8_refusal(h, R);
    return fail("kmb_gen_step: FP8 decoder weights: %s", why ? why : "the fused decode blocks are not available");
  }
  if (fused) {
    const bf16_t* zin = G.L.x0;                       // layer input: normalised rows (layer 0) or pre-LayerNorm sums
    const float *lg = nullptr, *lb = nullptr;       // ... and the LayerNorm that turns them into the layer input
    // wi: the block's weight among the layer's six packed copies (FP8: its row exponents go with it)
    auto block = [&](KmbDecodeBlock& b, size_t wi) -> int {
      b.W = G.L.wp[wi];
      if (f8) { b.w_format = KMB_WFMT_FP8_E4M3; b.w_exp = G.L.wexp[wi]; }
      const char* why = kmb_decode_block_check(b);
      if (why) return fail("kmb_gen_step: %s", why);
      HIPCHK(kmb_decode_block_launch(b, s));
      return 0;
    };
    for (int l = 0; l < h->cfg.decoder_layers; ++l) {
      const LayerP& L = h->dec[l];
      KmbDecodeBlock b;
      memset(&b, 0, sizeof(b));
      b.kind = 1; b.in = zin; b.ld_in = d; b.gamma = lg; b.beta = lb; b.eps = eps; b.ln_out = lg ? G.L.x1 : nullptr;
      b.bias = h->pf(L.sa.qkv_b); b.R = R; b.K = d; b.N = 3 * d; b.out = G.L.o; b.ld_out = d;
      b.H = h->Hd; b.q_scale = 0.125f; b.Kc = G.L.kc[l]; b.Vc = G.L.vc[l]; b.Tmax = G.Tmax; b.ldc = d; b.Tk = step + 1;
      b.hist = G.L.hist[G.hcur];
      KCHK(block(b, (size_t)l * 6 + 0));
      const bf16_t* xres = lg ? G.L.x1 : zin;
      memset(&b, 0, sizeof(b));
      b.kind = 0; b.in = G.L.o; b.ld_in = d; b.bias = h->pf(L.sa.o_b); b.R = R; b.K = d; b.N = d;
      b.residual = xres; b.ld_res = d; b.out = G.L.z; b.ld_out = d;
      KCHK(block(b, (size_t)l * 6 + 1));
      memset(&b, 0, sizeof(b));
      b.kind = 2; b.in = G.L.z; b.ld_in = d; b.gamma = h->pf(L.sa.ln_g); b.beta = h->pf(L.sa.ln_b); b.eps = eps; b.ln_out = G.L.y;
      b.bias = h->pf(L.ca.qkv_b); b.R = R; b.K = d; b.N = d; b.out = G.L.o; b.ld_out = d;
      b.H = h->Hd; b.q_scale = 0.125f; b.Kc = G.L.ckv[l]; b.Vc = G.L.ckv[l] + d; b.Tmax = G.S; b.ldc = h->cfg.decoder_layers * 2 * d; b.Tk = G.S;
      b.kv_row = G.kv_row; b.key_mask = G.bt.attention_mask; b.mask_ld = G.S; b.kv_group = G.nb;   // kv_row[i] = i / nb
      KCHK(block(b, (size_t)l * 6 + 2));
      memset(&b, 0, sizeof(b));
      b.kind = 0; b.in = G.L.o; b.ld_in = d; b.bias = h->pf(L.ca.o_b); b.R = R; b.K = d; b.N = d;
      b.residual = G.L.y; b.ld_res = d; b.out = G.L.z; b.ld_out = d;
      KCHK(block(b, (size_t)l * 6 + 3));
      memset(&b, 0, sizeof(b));
      b.kind = 0; b.in = G.L.z; b.ld_in = d; b.gamma = h->pf(L.ca.ln_g); b.beta = h->pf(L.ca.ln_b); b.eps = eps; b.ln_out = G.L.y;
      b.bias = h->pf(L.fc1_b); b.R = R; b.K = d; b.N = F; b.act = 1; b.out = G.L.hh; b.ld_out = F;
      KCHK(block(b, (size_t)l * 6 + 4));
      memset(&b, 0, sizeof(b));
      b.kind = 0; b.in = G.L.hh; b.ld_in = F; b.bias = h->pf(L.fc2_b); b.R = R; b.K = F; b.N = d;
      b.residual = G.L.y; b.ld_res = d; b.out = G.L.z; b.ld_out = d;
      KCHK(block(b, (size_t)l * 6 + 5));
      zin = G.L.z; lg = h->pf(L.ln_g); lb = h->pf(L.ln_b);
    }
    G.last_x = nullptr; G.last_z = G.L.z; G.last_g = lg; G.last_b = lb;
    if (lg && logits_out) {   // the last LayerNorm feeds only the vocabulary projection
      HIPCHK(kmb_ln_fwd_launch(G.L.z, lg, lb, G.L.x1, G.L.mean, G.L.rstd, R, d, eps, s));
      x = G.L.x1;
      G.last_x = x; G.last_z = nullptr;
    }
    if (!lg) { G.last_x = G.L.x0; G.last_z = nullptr; }   // a decoder without layers: the embedding output
  }
  for (int l = 0; !fused && l < h->cfg.decoder_layers; ++l) {
    const LayerP& L = h->dec[l];
    KmbGemm g = lin_fwd(x, d, h->wb(L.sa.qkv_w), h->pf(L.sa.qkv_b), R, 3 * d, d);
    g.col_scale = 0.125f; g.col_scale_n = d; g.out_bf16 = G.L.qkv; g.ld_out_bf16 = 3 * d;
    KCHK(run_gemm(g, s));
    KmbAttnDecode a; memset(&a, 0, sizeof(a));
    a.Q = G.L.qkv; a.ldq = 3 * d; a.Kc = G.L.kc[l]; a.Vc = G.L.vc[l]; a.Tmax = G.Tmax; a.ldc = d;
    a.R = R; a.H = h->Hd; a.Tk = step + 1; a.O = G.L.o; a.ldo = d;
    // this step's key / value: attended to from the projection output and appended to the cache by the same launch
    a.new_k = G.L.qkv + d; a.new_v = G.L.qkv + 2 * d; a.ld_new = 3 * d; a.Kw = G.L.kc[l]; a.Vw = G.L.vc[l];
    a.hist = G.L.hist[G.hcur];
    if (const char* why = kmb_attn_decode_check(a)) return fail("kmb_gen_step: %s", why);
    HIPCHK(kmb_attn_decode_launch(a, s));
    KCHK(proj_ln(G.L.o, d, L.sa.o_w, L.sa.o_b, x, L.sa.ln_g, L.sa.ln_b, G.L.y));
    // cross attention over the cached encoder K|V of the row's batch item
    g = lin_fwd(G.L.y, d, h->wb(L.ca.qkv_w), h->pf(L.ca.qkv_b), R, d, d);
    g.col_scale = 0.125f; g.col_scale_n = d; g.out_bf16 = G.L.cq; g.ld_out_bf16 = d;
    KCHK(run_gemm(g, s));
    memset(&a, 0, sizeof(a));
    a.Q = G.L.cq; a.ldq = d; a.Kc = G.L.ckv[l]; a.Vc = G.L.ckv[l] + d; a.Tmax = G.S; a.ldc = h->cfg.decoder_layers * 2 * d; a.kv_row = G.kv_row;
    a.key_mask = G.bt.attention_mask; a.mask_ld = G.S; a.mask_row = G.kv_row;
    a.R = R; a.H = h->Hd; a.Tk = G.S; a.O = G.L.o; a.ldo = d;
    if (const char* why = kmb_attn_decode_check(a)) return fail("kmb_gen_step: %s", why);
    HIPCHK(kmb_attn_decode_launch(a, s));
    KCHK(proj_ln(G.L.o, d, L.ca.o_w, L.ca.o_b, G.L.y, L.ca.ln_g, L.ca.ln_b, G.L.y));   // in place: a lane rewrites only the chunks it read
    // FFN
    g = lin_fwd(G.L.y, d, h->wb(L.fc1_w), h->pf(L.fc1_b), R, F, d);
    g.act = 1; g.out_bf16 = G.L.hh; g.ld_out_bf16 = F;
    KCHK(run_gemm(g, s));
    KCHK(proj_ln(G.L.hh, F, L.fc2_w, L.fc2_b, G.L.y, L.ln_g, L.ln_b, xn));
    bf16_t* t = x; x = xn; xn = t;
  }
  if (!fused) { G.last_x = x; G.last_z = nullptr; }
  G.head_stats_blocks = 0; G.head_stats_for = nullptr;
  if (logits_out) {
    KmbGemm g = lin_fwd(x, d, h->wb(h->shared), h->flb, R, h->V, d);
    g.out_f32 = logits_out; g.ld_out_f32 = h->Vpad;
    // KMB_GEN_HEAD_STATS=0: the projection without its statistics epilogue, the beam step in two launches over the logits (read per call:
    // tests compare the two in one process)
    const char* hs_env = getenv("KMB_GEN_HEAD_STATS");
    const bool want_stats = !(hs_env && hs_env[0] == '0');
    KCHK(run_vocab_gemm(g, s, want_stats ? G.L.head_stats : nullptr, want_stats ? &G.head_stats_blocks : nullptr));
    if (G.head_stats_blocks > 0) G.head_stats_for = logits_out;
  }
  return 0;
}

// The generation state after a beam reorder whose history gather is queued: the other history copy is current, and with independent
// rows (num_beams == 1: the cached forward of src/model/model.py:384-397 with caller-expanded rows) the row -> cross-attention item
// table follows into its other copy, as _reorder_cache (mixins.py:419-434) permutes the encoder side.  (With num_beams > 1 a beam
// search only permutes rows inside a batch item and the table is unchanged.)
static int gen_reordered(kmb_handle* h, const int32_t* beam_idx, hipStream_t s) {
  auto& G = h->gen;
  G.hcur ^= 1;
  if (G.nb == 1) {
    int32_t* other = G.kv_row == G.L.kv_row ? G.L.kv_row + G.R : G.L.kv_row;
    HIPCHK(kmb_gather_i32_launch(G.kv_row, beam_idx, other, G.R, s));
    G.kv_row = other;
  }
  return 0;
}

// The next-step embedding plan of the four step entry points: the launch that chooses the tokens of a decode step also embeds them for
// decode step `step` (kmb_gen_step's embedding arguments, rows into x0), and kmb_gen_step(tokens = NULL) of that step then uses them.
// step < 0: no step follows.  The step must lie inside the cache and d_model be a multiple of 8, at most 1024.  Where x0 still holds the
// final decoder states kmb_gen_last_hidden returns (the launch-per-operation path swaps x0 / x1 once per layer, so an even number of
// layers ends there) the two families differ:
//   beam (kmb_gen_beam_step, kmb_gen_beam_sample_step): no folding then -- the next kmb_gen_step embeds -- and only for d_model > 512;
//   one beam (kmb_gen_greedy_step, kmb_gen_sample_step): one wave embeds one row, so any width folds, and the rows go to x1, which is
//   free once the step's layers are queued -- the two buffers change names and last_x keeps pointing at the states.
// Taking a plan clears x0_step (nothing is pending while the launch may fail); gen_embed_done records the step after the launch.
struct GenEmbedPlan {
  bool on = false; int step = -1; KmbEmbedNext en{};
  const KmbEmbedNext* arg() const { return on ? &en : nullptr; }
};
static GenEmbedPlan gen_embed_plan(kmb_handle* h, int step, bool beam_family) {
  auto& G = h->gen;
  const int d = h->d;
  GenEmbedPlan p;
  p.on = step >= 0 && step < G.Tmax && (d & 7) == 0 && d <= 1024 && (!beam_family || (d > 512 && G.last_x != G.L.x0));
  G.x0_step = -1;
  if (!p.on) return p;
  if (G.last_x == G.L.x0) std::swap(G.L.x0, G.L.x1);   // (one-beam family only: the beam family is not eligible here)
  p.step = step;
  p.en.E = h->pf(h->shared); p.en.prow = h->pf(h->dec_pos) + (size_t)(h->cfg.extra_pos_embeddings + step) * d;
  p.en.gamma = h->pf(h->dec_lne_g); p.en.beta = h->pf(h->dec_lne_b); p.en.y = G.L.x0;
  p.en.scale = h->cfg.scale_embedding ? sqrtf((float)d) : 1.f; p.en.D = d; p.en.eps = h->cfg.layer_norm_eps; p.en.V = h->V;
  return p;
}
static void gen_embed_done(kmb_handle* h, const GenEmbedPlan& p) {
  if (p.on) h->gen.x0_step = p.step;
}

// What a beam step also folds into its launch: the history-index reorder of kmb_gen_reorder(next_beam_idx, reorder_step), when reorder_step >= 0.
// A reorder means another decode step follows, at position reorder_step + 1, on the tokens chosen here.
static KmbHistGather gen_fold_hist(const kmb_handle* h, int reorder_step) {
  const auto& G = h->gen;
  return KmbHistGather{G.L.hist[G.hcur], G.L.hist[G.hcur ^ 1], G.Tmax, reorder_step + 1};
}

// The beam step of the decode loop on the logits of the last kmb_gen_step (mixins.py:386-417 via transformers 3.0.2
// _generate_beam_search: log_softmax + beam score, the 2 * num_beams best per batch item, the next step's beams): kmb_beam_step's
// arguments and outputs.  When that step's vocabulary projection left its per-block statistics (all-rows kernel, 257 .. 320 beam rows),
// ONE launch selects from them; otherwise kmb_beam_step's two launches over the logits.
// reorder_step >= 0: also kmb_gen_reorder(next_beam_idx, reorder_step) (_reorder_cache, mixins.py:419-434), by the launch that has just
// chosen the beams, no launch of its own.
int kmb_gen_beam_step(kmb_handle* h, const float* logits, int ld, int num_beams, const float* add, int force_token, int ban_token, int k,
                      int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, float* scratch,
                      int64_t scratch_floats, int reorder_step, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_beam_step: call kmb_gen_begin first");
  if (!logits || !out || !next_scores || !next_tokens || !next_beam_idx) return fail("kmb_gen_beam_step: missing tensor");
  if (num_beams != G.nb) return fail("kmb_gen_beam_step: num_beams %d, kmb_gen_begin had %d", num_beams, G.nb);
  if (reorder_step >= G.Tmax) return fail("kmb_gen_beam_step: reorder_step %d outside the cache (Tmax=%d)", reorder_step, G.Tmax);
  const bool fold = reorder_step >= 0;
  const KmbHistGather hg = gen_fold_hist(h, reorder_step);
  const GenEmbedPlan ep = gen_embed_plan(h, fold ? reorder_step + 1 : -1, true);
  const KmbBeamStep p{logits, ld, h->V, G.B, num_beams, add, force_token, ban_token, k, out, eos_token, next_scores, next_tokens,
                      next_beam_idx, fold ? &hg : nullptr, ep.arg()};
  hipError_t e = hipErrorNotSupported;
  if (force_token < 0 && G.head_stats_blocks > 0 && G.head_stats_for == logits)
    e = kmb_beam_step_stats_launch(p, G.L.head_stats, G.head_stats_blocks, s);
  if (e == hipErrorNotSupported) e = kmb_beam_step_launch(p, scratch, scratch_floats > 0 ? (size_t)scratch_floats : 0, s);
  if (e == hipErrorNotSupported) return fail("kmb_gen_beam_step: unsupported shape (k <= 16, num_beams <= 16, num_beams * k <= 256)");
  HIPCHK(e);
  gen_embed_done(h, ep);
  return fold ? gen_reordered(h, next_beam_idx, (hipStream_t)stream) : 0;
}

// The beam step of the decode loop with generate()'s score processors (kmb_beam_step_processed on the logits of the last kmb_gen_step),
// with kmb_gen_beam_step's reorder / embedding contract.  The logits are not edited -- the head statistics stay what they are -- but an
// edit can invalidate the block maxima the statistics path takes its threshold from: this step never selects from them.
int kmb_gen_beam_step_processed(kmb_handle* h, const float* logits, int ld, int num_beams, const float* add, int force_token, int ban_token,
                                int k, int32_t* out, int eos_token, float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx,
                                float* scratch, int64_t scratch_floats, const int64_t* ids_in, int64_t* ids_out, int ld_ids, int t,
                                float repetition_penalty, int no_repeat_ngram_size, const int32_t* bad_tokens, const int32_t* bad_offsets,
                                int n_bad, int reorder_step, void* stream) {
  if (!h) return fail("kmb_gen_beam_step_processed: call kmb_gen_begin first");
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_beam_step_processed: call kmb_gen_begin first");
  if (num_beams != G.nb) return fail("kmb_gen_beam_step_processed: num_beams %d, kmb_gen_begin had %d", num_beams, G.nb);
  if (reorder_step >= G.Tmax) return fail("kmb_gen_beam_step_processed: reorder_step %d outside the cache (Tmax=%d)", reorder_step, G.Tmax);
  // the stateless form's argument checks, before anything is launched or the generation state changes
  const KmbBeamProcess pr{ids_in, ids_out, ld_ids, t, repetition_penalty, no_repeat_ngram_size, bad_tokens, bad_offsets, n_bad};
  KmbBeamStep p{logits, ld, h->V, G.B, num_beams, add, force_token, ban_token, k, out, eos_token, next_scores, next_tokens, next_beam_idx};
  if (kmb_beam_step_processed_validate("kmb_gen_beam_step_processed", p, scratch, scratch_floats, pr) != 0) return -1;
  const bool fold = reorder_step >= 0;
  const KmbHistGather hg = gen_fold_hist(h, reorder_step);
  const GenEmbedPlan ep = gen_embed_plan(h, fold ? reorder_step + 1 : -1, true);
  p.hist = fold ? &hg : nullptr;
  p.embed = ep.arg();
  HIPCHK(kmb_beam_step_processed_launch(p, scratch, (size_t)scratch_floats, pr, (hipStream_t)stream));
  gen_embed_done(h, ep);
  return fold ? gen_reordered(h, next_beam_idx, (hipStream_t)stream) : 0;
}

// The beam-sampling step of the decode loop (kmb_beam_sample_step on the logits of the last kmb_gen_step), with kmb_gen_beam_step's
// reorder / embedding contract.  The sampling filter needs every logit of the row: the projection's statistics are not used.
int kmb_gen_beam_sample_step(kmb_handle* h, const float* logits, int ld, int num_beams, const float* add, float temperature, int top_k,
                             float top_p, int ban_token, const float* noise, int ld_noise, int k, int32_t* out, int eos_token,
                             float* next_scores, int64_t* next_tokens, int32_t* next_beam_idx, float* scratch, int64_t scratch_floats,
                             int reorder_step, void* stream) {
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_beam_sample_step: call kmb_gen_begin first");
  if (num_beams != G.nb) return fail("kmb_gen_beam_sample_step: num_beams %d, kmb_gen_begin had %d", num_beams, G.nb);
  if (reorder_step >= G.Tmax) return fail("kmb_gen_beam_sample_step: reorder_step %d outside the cache (Tmax=%d)", reorder_step, G.Tmax);
  // the stateless form's argument checks, before anything is launched or the generation state changes
  if (kmb_beam_sample_validate("kmb_gen_beam_sample_step", logits, ld, h->V, G.B, num_beams, temperature, top_k, top_p, ban_token,
                               noise, ld_noise, k, out, eos_token, next_scores, next_tokens, next_beam_idx, scratch, scratch_floats) != 0)
    return -1;
  const bool fold = reorder_step >= 0;
  const KmbHistGather hg = gen_fold_hist(h, reorder_step);
  const GenEmbedPlan ep = gen_embed_plan(h, fold ? reorder_step + 1 : -1, true);
  HIPCHK(kmb_beam_sample_step_launch(logits, ld, h->V, G.B, num_beams, add, temperature, top_k, top_p, ban_token, noise, ld_noise, k,
                                     out, eos_token, next_scores, next_tokens, next_beam_idx, scratch, (size_t)scratch_floats,
                                     (hipStream_t)stream, fold ? &hg : nullptr, ep.arg()));
  gen_embed_done(h, ep);
  return fold ? gen_reordered(h, next_beam_idx, (hipStream_t)stream) : 0;
}

// The greedy step of the decode loop (kmb_greedy_step on the logits of the last kmb_gen_step).  embed_step >= 0: another decode step
// follows at that position on the tokens chosen here, and the same launch embeds them (gen_embed_plan, one-beam family; with
// kmb_embed_ln_fwd_launch's chunk count for the width).
int kmb_gen_greedy_step(kmb_handle* h, const float* logits, int ld, int ban_token, int64_t* unfinished, int64_t pad_token,
                        int64_t eos_token, int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* logprob_sum,
                        float* logprob_out, int embed_step, void* stream) {
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_greedy_step: call kmb_gen_begin first");
  if (G.nb != 1) return fail("kmb_gen_greedy_step: needs num_beams == 1, kmb_gen_begin had %d", G.nb);
  if (embed_step < -1) return fail("kmb_gen_greedy_step: embed_step must be -1 or a decode step");
  // the stateless form's argument checks, before anything is launched or the generation state changes
  if (kmb_greedy_validate("kmb_gen_greedy_step", logits, ld, h->V, G.R, ban_token, unfinished, pad_token, eos_token, next_tokens, ids, t,
                          ld_ids) != 0)
    return -1;
  const GenEmbedPlan ep = gen_embed_plan(h, embed_step, false);
  HIPCHK(kmb_greedy_step_launch(logits, ld, h->V, G.R, ban_token, unfinished, pad_token, eos_token, next_tokens, ids, t, ld_ids, flag,
                                logprob_sum, logprob_out, (hipStream_t)stream, ep.arg()));
  gen_embed_done(h, ep);
  return 0;
}

// The sampling step of the decode loop (kmb_sample_scored_step on the logits of the last kmb_gen_step), with kmb_gen_greedy_step's
// embed_step contract: the launch that draws the tokens embeds them for the next decode step.
int kmb_gen_sample_step(kmb_handle* h, const float* logits, int ld, float temperature, int top_k, float top_p, int ban_token,
                        const float* noise, int ld_noise, int64_t* unfinished, int64_t pad_token, int64_t eos_token,
                        int64_t* next_tokens, int64_t* ids, int t, int ld_ids, int32_t* flag, float* info_out, float* logprob_sum,
                        float* logprob_out, int ld_logprob, int embed_step, void* stream) {
  if (!h) return fail("kmb_gen_sample_step: call kmb_gen_begin first");
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_sample_step: call kmb_gen_begin first");
  if (G.nb != 1) return fail("kmb_gen_sample_step: needs num_beams == 1, kmb_gen_begin had %d", G.nb);
  if (embed_step < -1) return fail("kmb_gen_sample_step: embed_step must be -1 or a decode step");
  // the stateless form's argument checks, before anything is launched or the generation state changes
  if (kmb_sample_validate("kmb_gen_sample_step", logits, ld, h->V, G.R, temperature, top_k, top_p, ban_token, noise, ld_noise,
                          unfinished, pad_token, eos_token, next_tokens, ids, t, ld_ids, logprob_out != nullptr, ld_logprob) != 0)
    return -1;
  const GenEmbedPlan ep = gen_embed_plan(h, embed_step, false);
  HIPCHK(kmb_sample_scored_step_launch(logits, ld, h->V, G.R, temperature, top_k, top_p, ban_token, noise, ld_noise, unfinished,
                                       pad_token, eos_token, next_tokens, ids, t, ld_ids, flag, info_out, logprob_sum, logprob_out,
                                       ld_logprob, (hipStream_t)stream, ep.arg()));
  gen_embed_done(h, ep);
  return 0;
}

// The score processors of the decode loop (kmb_logits_process on the logits of the last kmb_gen_step, in place).  The statistics the
// step's vocabulary projection left describe the logits as it wrote them: edited logits have none.
int kmb_gen_logits_process(kmb_handle* h, float* logits, int ld, const int64_t* ids, int ld_ids, int t, float repetition_penalty,
                           int no_repeat_ngram_size, const int32_t* bad_tokens, const int32_t* bad_offsets, int n_bad, void* stream) {
  if (!h) return fail("kmb_gen_logits_process: call kmb_gen_begin first");
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_logits_process: call kmb_gen_begin first");
  if (G.nb != 1) return fail("kmb_gen_logits_process: needs num_beams == 1, kmb_gen_begin had %d", G.nb);
  if (kmb_logits_process_validate("kmb_gen_logits_process", logits, ld, h->V, G.R, ids, ld_ids, t, repetition_penalty,
                                  no_repeat_ngram_size, bad_tokens, bad_offsets, n_bad) != 0)
    return -1;
  if (G.head_stats_for == logits) { G.head_stats_blocks = 0; G.head_stats_for = nullptr; }
  HIPCHK(kmb_logits_process_launch(logits, ld, h->V, G.R, ids, ld_ids, t, repetition_penalty, no_repeat_ngram_size, bad_tokens,
                                   bad_offsets, n_bad, (hipStream_t)stream));
  return 0;
}

int kmb_gen_last_hidden(kmb_handle* h, kmb_bf16* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_last_hidden: call kmb_gen_begin first");
  if (!out) return fail("kmb_gen_last_hidden: out is required");
  if (G.last_x) {
    HIPCHK(hipMemcpyAsync(out, G.last_x, (size_t)G.R * h->d * sizeof(bf16_t), hipMemcpyDeviceToDevice, s));
  } else if (G.last_z && G.last_g) {
    HIPCHK(kmb_ln_fwd_launch(G.last_z, G.last_g, G.last_b, out, G.L.mean, G.L.rstd, G.R, h->d, h->cfg.layer_norm_eps, s));
  } else {
    return fail("kmb_gen_last_hidden: no kmb_gen_step has run since kmb_gen_begin");
  }
  return 0;
}

int kmb_gen_embedded_step(const kmb_handle* h) {
  return h && h->gen.active ? h->gen.x0_step : -1;
}

int kmb_gen_stats_blocks(const kmb_handle* h, const float* logits) {
  return h && h->gen.active && logits && h->gen.head_stats_for == logits ? h->gen.head_stats_blocks : 0;
}

int kmb_gen_reorder(kmb_handle* h, const int32_t* beam_idx, int step, void* stream) {   // permutes the history index, not the caches
  hipStream_t s = (hipStream_t)stream;
  auto& G = h->gen;
  if (!G.active) return fail("kmb_gen_reorder: call kmb_gen_begin first");
  HIPCHK(kmb_gather_hist_launch(G.L.hist[G.hcur], beam_idx, G.L.hist[G.hcur ^ 1], G.R, G.Tmax, step + 1, s));
  return gen_reordered(h, beam_idx, s);
}

}  // extern "C"
