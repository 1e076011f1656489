// The training step: workspace layout, forward (encoder, decoder, LM head, pre-training heads), backward (with gradient
// accumulation's per-bucket folds), kmb_score and the readers of the last forward's activations.
#include "engine_internal.h"

namespace kmbi __attribute__((visibility("hidden"))) {

int bias_grad(kmb_handle* h, const bf16_t* dy, int ld, int M, int N, float* out, hipStream_t s) {
  HIPCHK(kmb_colsum_launch(dy, ld, M, N, h->tl.parts, s));
  HIPCHK(kmb_reduce_parts_launch(h->tl.parts, kmb_colsum_parts(M), N, out, N, s));
  return 0;
}

constexpr size_t NO_BIAS = (size_t)-1;
// bias_off: gradient slot of the bias of the linear that produced the (dropped) sub-layer output, or NO_BIAS
// site_parts: this site's own partials buffer (the reducer then runs on the side stream), or nullptr: the shared scratch,
// reducer on the caller's stream
int ln_backward(kmb_handle* h, const bf16_t* dy, const bf16_t* z, const float* mean, const float* rstd, size_t g_off,
                size_t b_off, bf16_t* dz, bf16_t* out2, KmbDrop dy_drop, KmbDrop out2_drop, int M, hipStream_t s,
                size_t bias_off = NO_BIAS, float* site_parts = nullptr) {
  const int d = h->d;
  if (b_off != g_off + (size_t)d) return fail("LayerNorm weight/bias are not adjacent in the arena");
  float* parts = site_parts ? site_parts : h->tl.parts;
  HIPCHK(kmb_ln_bwd_launch(dy, z, mean, rstd, h->pf(g_off), dz, out2, dy_drop, out2_drop, parts, M, d, s));
  const int np = kmb_ln_bwd_parts(M);
  hipStream_t rs = site_parts ? reducer_stream(h, s) : s;
  // partials are [np][3][d]: dgamma | dbeta (adjacent in the arena too: one reduce) | column sums of the sub-layer gradient
  if (bias_off != NO_BIAS) HIPCHK(kmb_reduce_parts2_launch(parts, np, 3 * d, h->gf(g_off), 2 * d, h->gf(bias_off), d, rs));
  else HIPCHK(kmb_reduce_parts_launch(parts, np, 3 * d, h->gf(g_off), 2 * d, rs));
  return 0;
}

// scratch for partial reductions: LayerNorm [<=1024][3][d], attention bias partials [B][3d],
// GEMM column sums [ceil(M/128)][F], colsum kernel [<=64][maxN]
size_t parts_floats(const kmb_handle* h, int Mmax, int B) {
  const size_t d = h->d;
  size_t maxN = 3 * d;
  if ((size_t)h->Fe > maxN) maxN = h->Fe;
  if ((size_t)h->Fd > maxN) maxN = h->Fd;
  size_t need = (size_t)kmb_ln_bwd_parts(Mmax) * 3 * d;
  const size_t attn = (size_t)B * 3 * d;
  const size_t gsum = ((size_t)Mmax + 63) / 64 * maxN;
  const size_t csum = (size_t)64 * maxN;
  if (attn > need) need = attn;
  if (gsum > need) need = gsum;
  if (csum > need) need = csum;
  return need + 1024;
}

// ------------------------------------------------------------------ workspace layout (training)
// With base == nullptr this only measures.  Bd: the decoder's batch, B inputs x targets per input -- the decoder's row count Md = Bd * T is
// independent of the encoder's Me = B * S (the log-sum-exps of both decoder attentions have Bd * Hd * T entries either way: cross-attention
// runs B items of Tq = (Bd / B) * T).
size_t layout_train(const kmb_handle* h, char* base, size_t cap, int B, int Bd, int S, int T, int Ntot, TrainLayout* out) {
  const int d = h->d, Fe = h->Fe, Fd = h->Fd;
  const size_t Me = (size_t)B * S, Md = (size_t)Bd * T;
  const size_t Mmax = Me > Md ? Me : Md;
  const int Le = h->cfg.encoder_layers, Ld = h->cfg.decoder_layers;
  Bump bp(base, cap);
  TrainLayout L;
  L.status = bp.take<int32_t>(4);
  L.count = bp.take<int32_t>(4);
  L.loss_dev = bp.take<float>(4);
  L.xf = bp.act((size_t)(Ntot > 0 ? Ntot : 1) * h->Fpad);
  L.img_emb = bp.take<float>((size_t)(Ntot > 0 ? Ntot : 1) * d);
  L.dimg = bp.act((size_t)(Ntot > 0 ? Ntot : 1) * d);
  L.img_src = bp.take<int32_t>(Me);
  L.ze0 = bp.act(Me * d);
  L.me0 = bp.take<float>(Me); L.re0 = bp.take<float>(Me);
  L.zd0 = bp.act(Md * d);
  L.md0 = bp.take<float>(Md); L.rd0 = bp.take<float>(Md);
  L.xe.resize(Le + 1); L.xd.resize(Ld + 1);
  for (int l = 0; l <= Le; ++l) L.xe[l] = bp.act(Me * d);
  for (int l = 0; l <= Ld; ++l) L.xd[l] = bp.act(Md * d);
  L.ea.resize(Le);
  for (int l = 0; l < Le; ++l) {
    EncAct& a = L.ea[l];
    a.qkv = bp.act(Me * 3 * d); a.o = bp.act(Me * d); a.z1 = bp.act(Me * d);
    a.y1 = bp.act(Me * d); a.u = bp.act(Me * Fe); a.hh = bp.act(Me * Fe);
    a.z2 = bp.act(Me * d);
    a.lse = bp.take<float>((size_t)B * h->He * S);
    a.m1 = bp.take<float>(Me); a.r1 = bp.take<float>(Me); a.m2 = bp.take<float>(Me); a.r2 = bp.take<float>(Me);
  }
  L.da.resize(Ld);
  L.ckv_all = bp.act(Me * (size_t)Ld * 2 * d);    // [Me, Ld * 2d]: layer l's k | v are columns [l * 2d, (l + 1) * 2d)
  L.dckv_all = bp.act(Me * (size_t)Ld * 2 * d);
  for (int l = 0; l < Ld; ++l) {
    DecAct& a = L.da[l];
    a.qkv = bp.act(Md * 3 * d); a.o1 = bp.act(Md * d); a.z1 = bp.act(Md * d);
    a.y1 = bp.act(Md * d); a.cq = bp.act(Md * d); a.ckv = EP(L.ckv_all, (size_t)l * 2 * d);
    a.o2 = bp.act(Md * d); a.z2 = bp.act(Md * d); a.y2 = bp.act(Md * d);
    a.u = bp.act(Md * Fd); a.hh = bp.act(Md * Fd); a.z3 = bp.act(Md * d);
    a.lse1 = bp.take<float>((size_t)Bd * h->Hd * T); a.lse2 = bp.take<float>((size_t)Bd * h->Hd * T);
    a.m1 = bp.take<float>(Md); a.r1 = bp.take<float>(Md); a.m2 = bp.take<float>(Md); a.r2 = bp.take<float>(Md);
    a.m3 = bp.take<float>(Md); a.r3 = bp.take<float>(Md);
  }
  // bf16 product path: the training logits live in dlogits_c (bf16, turned into their own gradient in place by the CE
  // kernel); logits_c only holds the split-K slabs of the head's data gradient (<= 8 x Md x d floats).  The fp32
  // validation mode keeps fp32 logits here, in row chunks of lm_chunk.
  const size_t CH = Md < (size_t)h->lm_chunk ? Md : (size_t)h->lm_chunk;
  L.logits_c_floats = (g_f32 || h->Vpad > 65536 || force_fp32_head()) ? std::max(CH * h->Vpad, (size_t)8 * Md * d) : (size_t)8 * Md * d;
  L.logits_c = bp.take<float>(L.logits_c_floats);
  L.dlogits_c = bp.act(Md * h->Vpad);   // all rows: the head's dgrad / wgrad run once, un-chunked
  // split-K partial slabs of the weight-gradient GEMMs: 14 slices of a 768x768 matrix ... 3 of the tied V x d matrix
  // (the latter only when the batch is long enough for run_wgrad to split it: >= 256 K steps = 16384 decoder tokens)
  L.slab_floats = std::max((size_t)20 << 20, Md >= 16384 ? (size_t)3 * h->V * d : (size_t)0);
  L.slab = bp.take<float>(L.slab_floats);
  // slabs of the small-batch split-K forward / dgrad GEMMs (run_gemm) on the caller's stream; only small batches use them
  L.small_floats = Mmax <= 8192 ? (size_t)8 * Mmax * d : 1024;
  L.small_slab = bp.take<float>(L.small_floats);
  L.loss_rows = bp.take<float>(Md);
  L.ce_shift = bp.take<float>(Md); L.ce_pick = bp.take<float>(Md);
  L.ce_srow = bp.take<float>(Md); L.ce_alpha = bp.take<float>(Md);
  L.ce_bias = bp.take<float>(h->Vpad);
  L.ce_ah = bp.act(Md * d);
  L.dhdec = bp.act(Md * d);
  L.dyA = bp.act(Mmax * d); L.dyB = bp.act(Mmax * d);
  L.dz = bp.act(Mmax * d);
  const int Fmax = Fe > Fd ? Fe : Fd;
  for (BwdBufs& bb : L.bb) {
    for (int site = 0; site < 3; ++site) {
      bb.dz[site] = bp.act(Mmax * d);
      bb.dsub[site] = bp.act(Mmax * d);
    }
    bb.du = bp.act(Mmax * Fmax);
    bb.dqkv = bp.act(Mmax * 3 * d);
    bb.dcq = bp.act(Md * d);
    for (int site = 0; site < 6; ++site) bb.parts[site] = bp.take<float>(parts_floats(h, (int)Mmax, Bd));
  }
  L.dob = bp.act(Mmax * d); L.denc = bp.act(Me * d);
  L.parts = bp.take<float>(parts_floats(h, (int)Mmax, Bd));
  L.losses5 = bp.take<float>(8);
  // pre-training head scratch (only when heads exist and rows were reserved)
  if ((h->head[0].on || h->head[1].on || h->head[2].on) && h->head_rows_cap > 0) {
    const size_t n = (size_t)h->head_rows_cap;
    size_t Cpad = 8;
    for (int k = 0; k < 3; ++k)
      if (h->head[k].on && align_up((size_t)h->head[k].C, 8) > Cpad) Cpad = align_up((size_t)h->head[k].C, 8);
    L.hx = bp.act(n * 2 * d); L.hy = bp.act(n * d); L.hdy = bp.act(n * d);
    L.hdx = bp.act(n * 2 * d); L.hdlg = bp.act(n * Cpad); L.hlg = bp.take<float>(n * Cpad);
    L.hloss = bp.take<float>(n); L.dhead = bp.take<float>(Md * d);
    // run_wgrad picks S <= 512 / tiles128 slices: S x M x N stays under 512 x 128 x 128 floats (+ edge-tile slack)
    L.head_slab_floats = (size_t)9 << 20;
    L.head_slab = bp.take<float>(L.head_slab_floats);
    L.hyd = bp.act(n * d);   // (carved last: every other buffer stays where it was)
  }
  {   // label smoothing in the fused head (behind everything else, for the same reason): wsum | bsum, -u, beta, and the partial slots of whichever
      // of the two deterministic sums is running (the vocabulary sum's are consumed before the row finish writes its own)
    const size_t vs = (size_t)kmb_ce_vocab_sum_slots(h->V, d) * kmb_ce_vocab_sum_ld(d), us = (size_t)kmb_ce_rows_slots((int)Md) * d;
    L.ls_wsum = bp.take<float>(kmb_ce_vocab_sum_ld(d)); L.ls_negu = bp.take<float>(d); L.ls_beta = bp.take<float>(Md);
    L.ls_parts = bp.take<float>(vs > us ? vs : us);
  }
  if (out) *out = std::move(L);
  return bp.used();
}

// KMB_PRINT_LAYOUT (diagnostic build): the addresses of backward's buffers in the bound workspace (overlap check)
void print_layout(const kmb_handle* h, const TrainLayout& L) {
  const int d = h->d, Me = h->Me, Md = h->Md;
  auto pr = [&](const char* n, const void* p, size_t bytes) { fprintf(stderr, "LAYOUT %s %p %zu\n", n, p, bytes); };
  const size_t Mm = (size_t)(Me > Md ? Me : Md);
  pr("slab", L.slab, L.slab_floats * 4); pr("dhdec", L.dhdec, (size_t)Md * d * 2); pr("dyA", L.dyA, Mm * d * 2);
  pr("dyB", L.dyB, Mm * d * 2); pr("dz", L.dz, Mm * d * 2); pr("dob", L.dob, Mm * d * 2); pr("denc", L.denc, (size_t)Me * d * 2);
  pr("parts", L.parts, 0); pr("logits_c", L.logits_c, 0); pr("dlogits_c", L.dlogits_c, (size_t)Md * h->Vpad * 2);
  for (const BwdBufs& bb : L.bb) {
    for (int st = 0; st < 3; ++st) { pr("bb.dz", bb.dz[st], Mm * d * 2); pr("bb.dsub", bb.dsub[st], Mm * d * 2); }
    pr("bb.du", bb.du, Mm * (size_t)(h->Fe > h->Fd ? h->Fe : h->Fd) * 2); pr("bb.dqkv", bb.dqkv, Mm * 3 * d * 2);
    pr("bb.dcq", bb.dcq, (size_t)Md * d * 2);
  }
  pr("ws_begin", h->ws, h->ws_bytes);
}

// ------------------------------------------------------------------ shared sub-graphs
// post-LN FFN block forward: z = x + drop(fc2(adrop(gelu(fc1(x))))) ; out = LN(z).  adr (activation dropout): hh = m * GeLU(a) and
// u = m * GeLU'(a) come out of the fc1 launch, m = keep ? scale : 0 -- everything behind it, backward included, runs unchanged
int ffn_forward(kmb_handle* h, const LayerP& L, int F, const bf16_t* x, bf16_t* u, bf16_t* hh, bf16_t* z, float* mean,
                float* rstd, bf16_t* out, int M, KmbDrop dr, KmbDrop adr, hipStream_t s) {
  const int d = h->d;
  KmbGemm g = lin_fwd(x, d, h->wb(L.fc1_w), h->pf(L.fc1_b), M, F, d);
  g.act = 1; g.preact = u; g.ld_preact = F; g.out_bf16 = hh; g.ld_out_bf16 = F;
  if (adr.thr16) { g.drop_thr16 = adr.thr16; g.drop_seed = adr.seed; g.drop_scale = adr.scale; }
  KCHK(run_gemm(g, s));
  g = lin_fwd(hh, F, h->wb(L.fc2_w), h->pf(L.fc2_b), M, d, F);
  g.drop_thr16 = dr.thr16; g.drop_seed = dr.seed; g.drop_scale = dr.scale;
  g.residual = x; g.ld_res = d; g.out_bf16 = z; g.ld_out_bf16 = d;
  KCHK(run_gemm(g, s));
  KCHK(ln_forward(z, h->pf(L.ln_g), h->pf(L.ln_b), out, mean, rstd, M, d, h->cfg.layer_norm_eps, s));
  return 0;
}

// backward of the FFN block.  dy: grad wrt LN output.  Result: grad wrt block input x in dx_out.
int ffn_backward(kmb_handle* h, const LayerP& L, int F, const bf16_t* x, const bf16_t* u, const bf16_t* hh,
                 const bf16_t* z, const float* mean, const float* rstd, const bf16_t* dy, bf16_t* dx_out, int M,
                 KmbDrop dr, BwdBufs& bb, hipStream_t s) {
  const int d = h->d;
  bf16_t* dz = bb.dz[0];
  bf16_t* dsub = dr.thr16 ? bb.dsub[0] : dz;
  KCHK(ln_backward(h, dy, z, mean, rstd, L.ln_g, L.ln_b, dz, dr.thr16 ? dsub : nullptr, KmbDrop{0u, 0u, 1.f}, dr, M, s,
                   L.fc2_b, bb.parts[0]));
  KCHK(trace("ffn.dz", dz, (size_t)M * d * 2, s));
  KCHK(wgrad_side(h, lin_wgrad(dsub, d, hh, F, h->gf(L.fc2_w), M, d, F, 0.f), s));
  KmbGemm g = lin_dgrad(dsub, d, h->wb(L.fc2_w), M, d, F);
  g.act = 2; g.aux = u; g.ld_aux = F; g.out_bf16 = bb.du; g.ld_out_bf16 = F;
  g.colsum = bb.parts[1];  // per-64-row-block column sums of du = partials of the fc1 bias gradient
  KCHK(run_gemm(g, s));
  HIPCHK(kmb_reduce_parts_launch(bb.parts[1], (M + 63) / 64, F, h->gf(L.fc1_b), F, reducer_stream(h, s)));
  KCHK(wgrad_side(h, lin_wgrad(bb.du, F, x, d, h->gf(L.fc1_w), M, F, d, 0.f), s));
  KCHK(trace("ffn.du", bb.du, (size_t)M * F * 2, s));
  g = lin_dgrad(bb.du, F, h->wb(L.fc1_w), M, F, d);
  g.residual = dz; g.ld_res = d; g.out_bf16 = dx_out; g.ld_out_bf16 = d;
  KCHK(run_gemm(g, s));
  KCHK(trace("ffn.dx", dx_out, (size_t)M * d * 2, s));
  return 0;
}

// self-attention block forward: z = x + drop(out_proj(attn(qkv(x)))) ; out = LN(z)
int self_attn_forward(kmb_handle* h, const AttnP& A, int H, const bf16_t* x, bf16_t* qkv, bf16_t* o, float* lse,
                      bf16_t* z, float* mean, float* rstd, bf16_t* out, int B, int T, const int64_t* mask, int causal,
                      KmbDrop dr, KmbDrop adr, hipStream_t s) {
  const int d = h->d, M = B * T;
  KmbGemm g = lin_fwd(x, d, h->wb(A.qkv_w), h->pf(A.qkv_b), M, 3 * d, d);
  g.col_scale = 0.125f; g.col_scale_n = d; g.out_bf16 = qkv; g.ld_out_bf16 = 3 * d;
  KCHK(run_gemm(g, s));
  AttnIO io{qkv, 3 * d, EP(qkv, d), EP(qkv, 2 * d), 3 * d, T, T, mask, causal};
  KCHK(attn_forward(h, io, B, H, o, lse, adr, s));
  g = lin_fwd(o, d, h->wb(A.o_w), h->pf(A.o_b), M, d, d);
  g.drop_thr16 = dr.thr16; g.drop_seed = dr.seed; g.drop_scale = dr.scale;
  g.residual = x; g.ld_res = d; g.out_bf16 = z; g.ld_out_bf16 = d;
  KCHK(run_gemm(g, s));
  KCHK(ln_forward(z, h->pf(A.ln_g), h->pf(A.ln_b), out, mean, rstd, M, d, h->cfg.layer_norm_eps, s));
  return 0;
}

int self_attn_backward(kmb_handle* h, const AttnP& A, int H, const bf16_t* x, bf16_t* qkv, bf16_t* o, float* lse,
                       const bf16_t* z, const float* mean, const float* rstd, const bf16_t* dy, bf16_t* dx_out, int B,
                       int T, const int64_t* mask, int causal, KmbDrop dr, KmbDrop adr, BwdBufs& bb, hipStream_t s) {
  const int d = h->d, M = B * T;
  bf16_t* dz = bb.dz[1];
  bf16_t* dsub = dr.thr16 ? bb.dsub[1] : dz;
  KCHK(ln_backward(h, dy, z, mean, rstd, A.ln_g, A.ln_b, dz, dr.thr16 ? dsub : nullptr, KmbDrop{0u, 0u, 1.f}, dr, M, s,
                   A.o_b, bb.parts[2]));
  KCHK(trace("sa.dz", dz, (size_t)M * d * 2, s));
  KCHK(wgrad_side(h, lin_wgrad(dsub, d, o, d, h->gf(A.o_w), M, d, d, 0.f), s));
  KmbGemm g = lin_dgrad(dsub, d, h->wb(A.o_w), M, d, d);
  g.out_bf16 = h->tl.dob; g.ld_out_bf16 = d;
  KCHK(run_gemm(g, s));
  KCHK(trace("sa.dob", h->tl.dob, (size_t)M * d * 2, s));
  KCHK(trace("sa.o(saved)", o, (size_t)M * d * 2, s));
  KCHK(trace("sa.qkv(saved)", qkv, (size_t)M * 3 * d * 2, s));
  AttnIO io{qkv, 3 * d, qkv + d, qkv + 2 * d, 3 * d, T, T, mask, causal};
  KCHK(attn_backward(h, io, B, H, o, lse, h->tl.dob, bb.dqkv, 3 * d, bb.dqkv + d, bb.dqkv + 2 * d, 3 * d, bb.parts[3],
                     bb.parts[3] + d, bb.parts[3] + 2 * d, 3 * d, adr, s));
  HIPCHK(kmb_reduce_parts_launch(bb.parts[3], B, 3 * d, h->gf(A.qkv_b), 3 * d, reducer_stream(h, s)));
  KCHK(trace("sa.dqkv", bb.dqkv, (size_t)M * 3 * d * 2, s));
  KCHK(wgrad_side(h, lin_wgrad(bb.dqkv, 3 * d, x, d, h->gf(A.qkv_w), M, 3 * d, d, 0.f), s));
  g = lin_dgrad(bb.dqkv, 3 * d, h->wb(A.qkv_w), M, 3 * d, d);
  g.residual = dz; g.ld_res = d; g.out_bf16 = dx_out; g.ld_out_bf16 = d;
  KCHK(run_gemm(g, s));
  KCHK(trace("sa.dx", dx_out, (size_t)M * d * 2, s));
  return 0;
}


// One BartClassificationHead (dropout -> dense -> tanh -> dropout -> out_proj) on gathered decoder rows, its loss and, with need_grad, all of
// its gradients: parameter gradients go to the arena, the gradient wrt the decoder states is scatter-added (fp32) into h->tl.dhead.
// Reference src/model/model.py:133-158, :248-289.
// classif_dropout (train, kmb_set_classif_dropout): with m_in [n, d_in] and m_h [n, d] holding keep * scale or 0, logits = out_proj(m_h . t),
// t = tanh(dense(m_in . x)).  hx holds m_in . x (the gather applies the mask; one launch for the relation head's two halves), hy the unmasked t,
// hyd = m_h . t.  Backward: d_out_w = dlogits^T hyd; d_pre = m_h . (dlogits W_o) . (1 - t^2) -- the act 4 epilogue multiplies by 1 - hy^2 and
// then applies the hidden site's mask; d_dense_w = d_pre^T hx; d_x = m_in . (d_pre W_d) -- the input site's mask in that GEMM's epilogue.
// Without it (both thresholds zero) the launches are exactly the ones of a build that never had the setting.
int head_run(kmb_handle* h, int k, const bf16_t* hdec, int n, const int32_t* rows_a, const int32_t* rows_b,
             const float* soft_targets, const int64_t* labels, float factor, bool train, bool need_grad, float* loss_out,
             hipStream_t s) {
  const HeadP& H = h->head[k];
  const int d = h->d, din = H.d_in, C = H.C;
  const int Cpad = (int)align_up((size_t)C, 8);
  if (n <= 0) {  // the reference skips the term; its parameters get no gradient this step
    HIPCHK(hipMemsetAsync(loss_out, 0, sizeof(float), s));
    if (need_grad) HIPCHK(hipMemsetAsync(h->gf(H.dw), 0, (H.ob + (size_t)C - H.dw) * sizeof(float), s));
    return 0;
  }
  if (n > h->head_rows_cap || h->tl.hx == nullptr) return fail("head rows %d exceed the reserved %d (kmb_reserve_head_rows)", n, h->head_rows_cap);
  const KmbDrop din_dr = h->cls_drop_site(k, 0, train), dh_dr = h->cls_drop_site(k, 1, train);
  // gather: [n, d] (or [n, 2d] = object | subject for the relation head)
  if (din_dr.thr16) {
    HIPCHK(kmb_gather_rows_drop_bf16_launch(hdec, d, rows_a, rows_b, h->tl.hx, din, n, d, din_dr, s));
  } else {
    HIPCHK(kmb_gather_rows_bf16_launch(hdec, d, rows_a, h->tl.hx, din, n, d, s));
    if (rows_b) HIPCHK(kmb_gather_rows_bf16_launch(hdec, d, rows_b, h->tl.hx + d, din, n, d, s));
  }
  KmbGemm g = lin_fwd(h->tl.hx, din, h->wb(H.dw), h->pf(H.db), n, d, din);
  g.act = 3; g.out_bf16 = h->tl.hy; g.ld_out_bf16 = d;
  KCHK(run_gemm(g, s));
  const bf16_t* hyo = h->tl.hy;   // what out_proj reads
  if (dh_dr.thr16) {
    HIPCHK(kmb_gather_rows_drop_bf16_launch(h->tl.hy, d, nullptr, nullptr, h->tl.hyd, d, n, d, dh_dr, s));
    hyo = h->tl.hyd;
  }
  g = lin_fwd(hyo, d, h->wb(H.ow), h->pf(H.ob), n, C, d);
  g.out_f32 = h->tl.hlg; g.ld_out_f32 = Cpad;
  KCHK(run_gemm(g, s));
  if (soft_targets) {  // F.kl_div(log_softmax(pred), target, reduction='batchmean') * factor
    HIPCHK(kmb_kl_div_launch(h->tl.hlg, Cpad, C, soft_targets, C, n, factor, h->tl.hloss, need_grad ? h->tl.hdlg : nullptr, Cpad, s));
    HIPCHK(kmb_mean_rows_launch(h->tl.hloss, n, factor, (float)n, loss_out, s));
  } else {             // CrossEntropyLoss()(pred, labels) * factor
    HIPCHK(kmb_count_valid_launch(labels, n, C, h->tl.count + 1, h->tl.status, s));
    HIPCHK(kmb_ce_launch(h->tl.hlg, Cpad, C, labels, n, h->tl.count + 1, factor, h->tl.hloss, need_grad ? h->tl.hdlg : nullptr, s));
    HIPCHK(kmb_mean_rows_launch(h->tl.hloss, n, factor, (float)n, loss_out, s));
  }
  if (!need_grad) return 0;
  // out_proj
  KCHK(bias_grad(h, h->tl.hdlg, Cpad, n, C, h->gf(H.ob), s));
  KCHK(run_wgrad(h, lin_wgrad(h->tl.hdlg, Cpad, hyo, d, h->gf(H.ow), n, C, d, 0.f), s, h->tl.head_slab, h->tl.head_slab_floats));
  g = lin_dgrad(h->tl.hdlg, Cpad, h->wb(H.ow), n, Cpad, d);   // reduction over the padded class dim (pad columns are zero)
  g.N = d; g.K = Cpad; g.act = 4; g.aux = h->tl.hy; g.ld_aux = d; g.out_bf16 = h->tl.hdy; g.ld_out_bf16 = d;
  if (dh_dr.thr16) { g.drop_thr16 = dh_dr.thr16; g.drop_seed = dh_dr.seed; g.drop_scale = dh_dr.scale; }   // behind the 1 - aux^2 multiply
  KCHK(run_gemm(g, s));
  // dense
  KCHK(bias_grad(h, h->tl.hdy, d, n, d, h->gf(H.db), s));
  KCHK(run_wgrad(h, lin_wgrad(h->tl.hdy, d, h->tl.hx, din, h->gf(H.dw), n, d, din, 0.f), s, h->tl.head_slab, h->tl.head_slab_floats));
  g = lin_dgrad(h->tl.hdy, d, h->wb(H.dw), n, d, din);
  g.out_bf16 = h->tl.hdx; g.ld_out_bf16 = din;
  if (din_dr.thr16) { g.drop_thr16 = din_dr.thr16; g.drop_seed = din_dr.seed; g.drop_scale = din_dr.scale; }
  KCHK(run_gemm(g, s));
  HIPCHK(kmb_scatter_add_rows_launch(h->tl.hdx, din, rows_a, h->tl.dhead, n, d, s));
  if (rows_b) HIPCHK(kmb_scatter_add_rows_launch(h->tl.hdx + d, din, rows_b, h->tl.dhead, n, d, s));
  return 0;
}

int encoder_forward(kmb_handle* h, const EncoderBufs& eb, const kmb_batch& bt, bool train, hipStream_t s) {
  const int d = h->d, B = bt.B, S = bt.S, Me = B * S;
  const float eps = h->cfg.layer_norm_eps;
  const float scale = h->cfg.scale_embedding ? sqrtf((float)d) : 1.f;
  if (bt.n_features > 0 && g_f32) {   // the raw fp32 features against the fp32 master weight [d, Fin]
    KmbGemm g = lin_fwd(reinterpret_cast<const bf16_t*>(bt.image_features), h->Fin, h->wb(h->img_w), h->pf(h->img_b),
                        bt.n_features, d, h->Fin);
    g.out_f32 = eb.img_emb; g.ld_out_f32 = d;
    KCHK(run_gemm(g, s));
  } else if (bt.n_features > 0) {
    HIPCHK(kmb_cast_pad_launch(bt.image_features, bt.n_features, h->Fin, eb.xf, h->Fpad, s));
    KmbGemm g = lin_fwd(eb.xf, h->Fpad, h->imgw_pad, h->pf(h->img_b), bt.n_features, d, h->Fpad);
    g.out_f32 = eb.img_emb; g.ld_out_f32 = d;
    KCHK(run_gemm(g, s));
  }
  HIPCHK(kmb_img_rowmap_launch(bt.input_ids, bt.feat_offsets, B, S, h->cfg.img_feat_id, h->cfg.cls_token_id,
                               eb.img_src, eb.status, s));
  KCHK(embed_ln_forward(bt.input_ids, eb.img_src, h->pf(h->shared), eb.img_emb, h->pf(h->enc_pos),
                        h->cfg.extra_pos_embeddings, S, scale, h->pf(h->enc_lne_g), h->pf(h->enc_lne_b),
                        eb.ze0, eb.x(0), eb.me0, eb.re0, Me, d, eps, h->drop_site(1, train), s));
  for (int l = 0; l < h->cfg.encoder_layers; ++l) {
    const LayerP& L = h->enc[l];
    const EncAct& a = eb.act(l);
    KCHK(self_attn_forward(h, L.sa, h->He, eb.x(l), a.qkv, a.o, a.lse, a.z1, a.m1, a.r1, a.y1, B, S,
                           bt.attention_mask, 0, h->drop_site(10 + 2 * l, train), h->attn_drop_site(0, l, train), s));
    KCHK(ffn_forward(h, L, h->Fe, a.y1, a.u, a.hh, a.z2, a.m2, a.r2, eb.x(l + 1), Me, h->drop_site(11 + 2 * l, train),
                     h->act_drop_site(0, l, train), s));
  }
  return 0;
}

// the tied LM head on rows [0, Md) of hdec: fp32 logits [Md, Vpad] (src/model/model.py:397)
// The vocabulary projection with fp32 logits.  A decode step's rows (batch x beams = 257 .. 320: the benchmarked 64 x 5): one
// workgroup per 256 vocabulary columns holds ALL rows, so every row of the tied matrix crosses a CU's memory pipe once
// (gemm.hip "All rows" kernel: 58 -> 47 us at 320 rows, tools/allrows_time.py; at <= 192 rows the 128x128 tiles already read
// the matrix once or twice and are faster: 31 against 39 us).  Bit-identical either way; KMB_GEMM_ALLROWS=0: always the tuner's pick.
// stats / stats_blocks (a generation step): the all-rows kernel also leaves every row's per-block (maximum, sum-exp) pairs there and
// *stats_blocks = their number, for the beam step that follows (beam_step.hip beam_stats_merge_kernel); 0 when another kernel ran.
int run_vocab_gemm(const KmbGemm& g, hipStream_t s, float* stats, int* stats_blocks) {
  static const bool allrows_ok = !(KMB_DIAG_ENV("KMB_GEMM_ALLROWS") && KMB_DIAG_ENV("KMB_GEMM_ALLROWS")[0] == '0');
  if (stats_blocks) *stats_blocks = 0;
  if (allrows_ok && !g_f32 && g.M > 256 && g.M <= 320 && kmb_gemm_allrows_check(g) == nullptr) {
    HIPCHK(kmb_gemm_allrows_launch(g, stats_blocks ? stats : nullptr, s));
    if (stats_blocks && stats) *stats_blocks = kmb_gemm_allrows_blocks(g.N);
    return 0;
  }
  return run_gemm(g, s);
}

static int head_logits(kmb_handle* h, const bf16_t* hdec, int Md, float* logits_out, hipStream_t s) {
  const int d = h->d;
  const int CH = Md < h->lm_chunk ? Md : h->lm_chunk;
  for (int r0 = 0; r0 < Md; r0 += CH) {
    const int rows = (Md - r0) < CH ? (Md - r0) : CH;
    KmbGemm g = lin_fwd(EP(hdec, (size_t)r0 * d), d, h->wb(h->shared), h->flb, rows, h->V, d);
    g.out_f32 = logits_out + (size_t)r0 * h->Vpad; g.ld_out_f32 = h->Vpad;
    KCHK(run_vocab_gemm(g, s));
  }
  return 0;
}

// ---------------------------------------------------------------------------------- the tied LM head + cross-entropy
// Split count of the head's data gradient dH[Md, d] = dlogits[Md, Vpad] E (1: no split).  [Md, d] has few 256x256 tiles (192 at
// Md = 16384: three quarters of the CUs) and the reduction runs over the whole vocabulary (788 K steps): split it so that the grid is
// a whole number of rounds; a small pass sums the slabs.  The slabs live in the fp32 logits buffer, which is free once the CE ran.
// (Md * d a multiple of 8: the slab passes' vector width -- the fused branch's Md % 256 == 0 implies it.)
static int head_dgrad_split(const kmb_handle* h, int Md) {
  const int d = h->d;
  const int tiles256 = ((Md + 255) / 256) * ((d + 255) / 256);
  static const int rounds = KMB_DIAG_ENV("KMB_HEAD_DGRAD_ROUNDS") ? atoi(KMB_DIAG_ENV("KMB_HEAD_DGRAD_ROUNDS")) : 3;   // tuning knob
  int S = tiles256 > 0 ? (256 * rounds) / tiles256 : 1;
  if (S > 8) S = 8;
  while (S > 1 && (size_t)S * Md * d > h->tl.logits_c_floats) --S;
  return (S > 1 && ((size_t)Md * d & 7) == 0 && h->Vpad / 64 >= 2 * S) ? S : 1;
}

// dE[V, d] = dlogits^T rows_operand (overwrites: the embedding scatter-adds of backward come on top), on the side stream: it overlaps
// the start of backward, whose embedding scatter-adds wait for head_wgrad_done
// rowvec (label smoothing, the fused head's -u): added to every one of the V rows where the gradient is written (run_wgrad)
static int head_wgrad_on_side(kmb_handle* h, const bf16_t* dlogits, const bf16_t* rows_operand, hipStream_t s, const float* rowvec = nullptr) {
  KCHK(ensure_side(h));
  KmbGemm gw = lin_wgrad(dlogits, h->Vpad, rows_operand, h->d, h->gf(h->shared), h->Md, h->V, h->d, 0.f);
  gw.bias = rowvec;
  KCHK(wgrad_side(h, gw, s));
  if (h->side_on && h->side) {
    HIPCHK(hipEventRecord(h->head_wgrad_done, h->side));
    h->head_wgrad_pending = true;
  }
  return 0;
}

// What the fused cross-entropy and kmb_score's store-free head start from: the label's logit of each of the Md rows as the row shift,
// the bias padded to Vpad with -1e30, and the projection of `rows` rows onto the padded vocabulary (*g, not launched)
static int head_padded_setup(kmb_handle* h, const bf16_t* hdec, const int64_t* labels, int Md, int rows, KmbGemm* g, hipStream_t s) {
  const int d = h->d;
  HIPCHK(kmb_ce_label_logit_launch(hdec, d, h->wb(h->shared), d, h->flb, labels, Md, d, h->V, h->tl.ce_shift, s));
  HIPCHK(kmb_ce_pad_bias_launch(h->flb, h->V, h->Vpad, h->tl.ce_bias, s));
  *g = lin_fwd(hdec, d, h->wb(h->shared), h->tl.ce_bias, rows, h->Vpad, d);
  return 0;
}

// Cross-entropy without a pass over the logits (loss.hip "Tied-head cross-entropy WITHOUT a pass over the logits"):
// the head GEMM stores exp(logit - label's logit) and per-row sums, the data- and weight-gradient GEMMs run on that
// matrix with per-row factors applied outside.
// What kmb_forward_opts adds to the LM criterion: the per-row weights (null: none) and the denominator word every
// head form divides by -- the number of valid labels ("mean"), or the 0 / 1 word of kmb_count_flag_launch ("sum").
struct LmLoss {
  const float* weights;
  const int32_t* den;
  bool sum;
};

static int head_fused_ce(kmb_handle* h, const bf16_t* hdec, const int64_t* labels, float lmf, bool need_grad, const LmLoss& lw, hipStream_t s) {
  const int d = h->d, Md = h->Md, nparts = h->Vpad / 64;
  const TrainLayout& L = h->tl;
  KmbGemm g;
  KCHK(head_padded_setup(h, hdec, labels, Md, Md, &g, s));
  g.act = 5; g.out_bf16 = L.dlogits_c; g.ld_out_bf16 = h->Vpad;
  g.row_shift = L.ce_shift; g.row_sums = L.logits_c; g.row_sums_ld = nparts; g.pick_col = nullptr; g.pick_out = nullptr;   // the shift is the label's logit itself: v[label] - shift = 0 up to summation order
  KCHK(run_gemm(g, s));
  // Label smoothing (loss.hip "Label smoothing as rank-one terms"): one read of the tied matrix for wsum | bsum, then the row finish, the
  // data-gradient finish and the weight gradient each take one more operand.  eps == 0: the launches below are the ones there always were.
  const float eps = h->label_smoothing;
  if (eps > 0.f) {
    HIPCHK(kmb_ce_vocab_sum_launch(h->wb(h->shared), d, h->flb, h->V, d, L.ls_parts, L.ls_wsum, s));
    HIPCHK(kmb_ce_rows_finish_ls_launch(L.logits_c, nparts, nparts, nullptr, L.ce_shift, labels, lw.den, lmf, eps, Md, d, h->V, hdec, d, L.ls_wsum,
                                        L.loss_rows, L.ce_srow, L.ce_alpha, L.ls_beta, need_grad ? L.ce_ah : nullptr,
                                        need_grad ? L.dlogits_c : nullptr, h->Vpad, need_grad ? L.ls_parts : nullptr,
                                        need_grad ? L.ls_negu : nullptr, s, lw.weights));
  } else {
    HIPCHK(kmb_ce_rows_finish_launch(L.logits_c, nparts, nparts, nullptr, labels, lw.den, lmf, Md, d, h->V, hdec, d, L.loss_rows, L.ce_srow,
                                     L.ce_alpha, need_grad ? L.ce_ah : nullptr, need_grad ? L.dlogits_c : nullptr, h->Vpad, s, lw.weights));
  }
  if (!need_grad) return 0;
  // dH_r = a_r sum_j P'_rj E_j: the GEMM on P' into fp32 slabs (the row sums in that buffer were consumed by the launch above), then the finish
  KmbGemm gd = lin_dgrad(L.dlogits_c, h->Vpad, h->wb(h->shared), Md, h->Vpad, d);
  const int S = head_dgrad_split(h, Md);
  if (S > 1) { gd.split_k = S; gd.slab = L.logits_c; }
  else { gd.out_f32 = L.logits_c; gd.ld_out_f32 = d; }
  KCHK(run_gemm(gd, s));
  if (eps > 0.f) {
    HIPCHK(kmb_ce_dgrad_finish_ls_launch(L.logits_c, S, (size_t)Md * d, L.ce_alpha, L.ls_beta, L.ls_wsum, L.dhdec, Md, d, s));
    return head_wgrad_on_side(h, L.dlogits_c, L.ce_ah, s, L.ls_negu);   // dE[j] = (P'^T (a . H))[j] - u for j < V
  }
  HIPCHK(kmb_ce_dgrad_finish_launch(L.logits_c, S, (size_t)Md * d, L.ce_alpha, L.dhdec, Md, d, s));
  return head_wgrad_on_side(h, L.dlogits_c, L.ce_ah, s);   // dE = P'^T (a . H)
}

// Two-kernel bf16 head (product path without whole tiles, KMB_FUSED_CE=0): ONE GEMM writes bf16 logits into dlogits_c and the CE kernel
// turns them into the gradient in place.  (Taken only without logits_out, so with labels.)
static int head_bf16(kmb_handle* h, const bf16_t* hdec, const int64_t* labels, float lmf, bool need_grad, const LmLoss& lw, hipStream_t s) {
  const TrainLayout& L = h->tl;
  KmbGemm g = lin_fwd(hdec, h->d, h->wb(h->shared), h->flb, h->Md, h->V, h->d);
  g.out_bf16 = L.dlogits_c; g.ld_out_bf16 = h->Vpad;
  KCHK(run_gemm(g, s));
  HIPCHK(kmb_ce_bf16_launch(L.dlogits_c, h->Vpad, h->V, labels, h->Md, lw.den, lmf, L.loss_rows, need_grad ? L.dlogits_c : nullptr, s,
                            h->label_smoothing, lw.weights));
  return 0;
}

// fp32 head (logits requested by the caller / fp32 validation mode / very wide vocabularies / KMB_FP32_HEAD=1) in row chunks of lm_chunk
// (8192) rows that bound the fp32 buffer: one launch at the benchmark batch.  Smaller chunks (KMB_LM_CHUNK) keep the fp32 logits on-die but
// quantise the tile count worse: 512-row chunks measured 0.8 % slower end to end.
static int head_fp32(kmb_handle* h, const bf16_t* hdec, const int64_t* labels, float lmf, bool need_grad, float* logits_out, const LmLoss& lw,
                     hipStream_t s) {
  const int d = h->d, Md = h->Md;
  const TrainLayout& L = h->tl;
  const int CH = Md < h->lm_chunk ? Md : h->lm_chunk;
  for (int r0 = 0; r0 < Md; r0 += CH) {
    const int rows = (Md - r0) < CH ? (Md - r0) : CH;
    KmbGemm g = lin_fwd(EP(hdec, (size_t)r0 * d), d, h->wb(h->shared), h->flb, rows, h->V, d);
    float* lg = logits_out ? logits_out + (size_t)r0 * h->Vpad : L.logits_c;
    if (!logits_out && (size_t)rows * h->Vpad > L.logits_c_floats) return fail("forward: the fp32 logits chunk does not fit the workspace's logits buffer");
    g.out_f32 = lg; g.ld_out_f32 = h->Vpad;
    KCHK(run_gemm(g, s));
    if (!labels) continue;
    HIPCHK(kmb_ce_launch(lg, h->Vpad, h->V, labels + r0, rows, lw.den, lmf, L.loss_rows + r0,
                         need_grad ? L.dlogits_c + (size_t)r0 * h->Vpad : nullptr, s, h->label_smoothing, lw.weights ? lw.weights + r0 : nullptr));
  }
  return 0;
}

// the gradients of the two heads that leave dlogits in dlogits_c: dH = dlogits E (reduction over the padded vocabulary; pad columns /
// rows are zero), then the tied matrix's
static int head_grads_from_dlogits(kmb_handle* h, const bf16_t* hdec, hipStream_t s) {
  const int d = h->d, Md = h->Md;
  const TrainLayout& L = h->tl;
  KmbGemm gd = lin_dgrad(L.dlogits_c, h->Vpad, h->wb(h->shared), Md, h->Vpad, d);
  const int S = head_dgrad_split(h, Md);
  if (S > 1) {
    gd.split_k = S; gd.slab = L.logits_c;
    KCHK(run_gemm(gd, s));
    HIPCHK(kmb_reduce_slabs_bf16_launch(L.logits_c, S, (size_t)Md * d, L.dhdec, (size_t)Md * d, s));
  } else {
    gd.out_bf16 = L.dhdec; gd.ld_out_bf16 = d;
    KCHK(run_gemm(gd, s));
  }
  return head_wgrad_on_side(h, L.dlogits_c, hdec, s);
}

static int lm_head(kmb_handle* h, const bf16_t* hdec, const int64_t* labels, float lmf, bool need_grad, float* loss_out, float* logits_out,
                   const float* row_weights, bool sum, hipStream_t s) {
  const int d = h->d, Md = h->Md;
  // KMB_FP32_HEAD=1 forces the fp32 head (chunked fp32 logits + ce_kernel_reg) in the product mode as well: the bf16 head
  // rounds logits of magnitude 10-20 to 8 significant bits before the softmax (the reference's AMP path holds fp16
  // logits, its CPU path fp32); measured effect on the vcg_base loss 5e-5 relative either way.
  const bool bf16_head = !g_f32 && !logits_out && h->Vpad <= 65536 && !force_fp32_head();
  // The fused cross-entropy needs whole 256-row / 256-column tiles (Md % 256 == 0; the vocabulary is padded to Vpad with a -1e30 bias);
  // other shapes and KMB_FUSED_CE=0 take the two-kernel path.
  const char* fce = getenv("KMB_FUSED_CE");     // read per call: tests flip it inside one process
  const bool fused_ce_env = !(fce && fce[0] == '0');
  const int nparts = h->Vpad / 64;
  const bool fused_ce = bf16_head && labels && fused_ce_env && (Md % 256) == 0 && (h->Vpad % 256) == 0 && (d % 64) == 0 &&
                        d >= 128 && (long)(Md / 256) * (h->Vpad / 256) >= 128 && (size_t)Md * nparts <= h->tl.logits_c_floats;
  if (labels) h->last_head_form = fused_ce ? 2 : bf16_head ? 1 : 0;
  // "sum": the third word of the count block holds the 0 / 1 denominator; "mean" without weights: the arguments there always were
  LmLoss lw{row_weights, h->tl.count, sum};
  if (labels && sum) {
    HIPCHK(kmb_count_flag_launch(h->tl.count, h->tl.count + 2, s));
    lw.den = h->tl.count + 2;
  }
  if (fused_ce) KCHK(head_fused_ce(h, hdec, labels, lmf, need_grad, lw, s));
  else if (bf16_head) KCHK(head_bf16(h, hdec, labels, lmf, need_grad, lw, s));
  else KCHK(head_fp32(h, hdec, labels, lmf, need_grad, logits_out, lw, s));
  if (labels && need_grad && !fused_ce) KCHK(head_grads_from_dlogits(h, hdec, s));
  if (labels) {
    HIPCHK(kmb_loss_finish_launch(h->tl.loss_rows, Md, h->tl.count, h->tl.loss_dev, s, sum));
    if (loss_out) HIPCHK(hipMemcpyAsync(loss_out, h->tl.loss_dev, sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

}  // namespace kmbi
using namespace kmbi;

extern "C" {

int64_t kmb_workspace_bytes(const kmb_handle* h, int B, int S, int T, int n_features) {
  PrecisionScope scope(h);
  return (int64_t)layout_train(h, nullptr, 0, B, B, S, T, n_features, nullptr);
}

int64_t kmb_workspace_bytes_grouped(const kmb_handle* h, int B, int S, int T, int n_features, int targets_per_input) {
  PrecisionScope scope(h);
  const int G = targets_per_input > 1 ? targets_per_input : 1;
  return (int64_t)layout_train(h, nullptr, 0, B, B * G, S, T, n_features, nullptr);
}

// --------------------------------------------------------------------------------- forward
static int forward_impl(kmb_handle* h, const kmb_batch* batch, const kmb_pretrain* extra, const kmb_forward_opts* opts,
                        int train, int need_grad, float* loss_out, float* logits_out, kmb_bf16* enc_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KCHK(check_bound(h));
  PrecisionScope scope(h);
  if (h->fp32 && (train || need_grad || extra))
    return fail("kmb_forward: the fp32 validation mode (kmb_set_precision) is an eval-mode forward only");
  const bf16_t* enc_in = opts ? opts->encoder_states : nullptr;
  // need_grad with given encoder states: backward stops at them (kmb_encoder_states_grad hands out dL/d states, the encoder's
  // parameter gradients are zero) -- src/model/model.py:76-83 run with a tensor that requires grad
  if (!batch || !batch->input_ids || !batch->decoder_input_ids || !batch->feat_offsets)
    return fail("kmb_forward: input_ids, decoder_input_ids and feat_offsets are required");
  const kmb_batch& bt = *batch;
  if (bt.B <= 0 || bt.S <= 0 || bt.T <= 0) return fail("kmb_forward: empty batch");
  if (bt.S > h->cfg.max_position_embeddings || bt.T > h->cfg.max_position_embeddings)
    return fail("kmb_forward: sequence longer than max_position_embeddings");
  if (need_grad && !bt.labels && !extra) return fail("kmb_forward: need_grad requires labels");
  if (need_grad && (!h->G)) return fail("kmb_forward: gradient arena is not bound");
  const float* row_weights = opts ? opts->row_weights : nullptr;
  const int loss_reduction = opts ? opts->loss_reduction : 0;
  if (row_weights && !bt.labels) return fail("kmb_forward: row_weights weigh the rows' cross-entropy and need labels");
  if (loss_reduction != 0 && loss_reduction != 1) return fail("kmb_forward: loss_reduction must be 0 (mean) or 1 (sum), got %d", loss_reduction);
  if (row_weights && opts->skip_head) return fail("kmb_forward: row_weights with skip_head: there is no loss to weigh");
  // several targets per input: the decoder tensors hold bt.B * G rows of T tokens, row i belongs to input i / G
  const int tpi = opts ? opts->targets_per_input : 0;
  if (tpi < 0) return fail("kmb_forward: targets_per_input must not be negative, got %d", tpi);
  const int G = tpi > 1 ? tpi : 1;
  if (G > 1 && extra) return fail("kmb_forward_pretrain: targets_per_input > 1 is not supported by the pre-training forward");
  if (G > 1 && (long long)G * bt.T > 384)
    return fail("kmb_forward: targets_per_input * T = %lld > 384: the cross-attention backward takes at most 384 query rows per input", (long long)G * bt.T);
  if (G > 1 && (long long)bt.B * G > 0x7fffffff / (bt.T > bt.S ? bt.T : bt.S)) return fail("kmb_forward: B * targets_per_input * T does not fit in 31 bits");
  {
    TrainLayout tl;
    const size_t need = layout_train(h, h->ws, h->ws_bytes, bt.B, bt.B * G, bt.S, bt.T, bt.n_features, &tl);
    if (need > h->ws_bytes) return fail("kmb_forward: workspace too small (%zu > %zu bytes)", need, h->ws_bytes);
    h->tl = std::move(tl);
    h->status = h->tl.status;
  }
  if (!h->fp32 && h->tl.small_floats > 1024) { g_small_slab = h->tl.small_slab; g_small_floats = h->tl.small_floats; }
  h->gen.active = false; h->gen.packed_at = nullptr;   // the activations of this forward overwrite the generation workspace
  const int d = h->d, B = bt.B, S = bt.S, T = bt.T, Bd = B * G, Me = B * S, Md = Bd * T;
  h->bt = bt; h->Me = Me; h->Md = Md; h->Ntot = bt.n_features; h->tpi = G;
  h->fwd_train = train != 0; h->have_fwd = false; h->have_hdec = false; h->have_bwd = false;
  h->enc_given = enc_in != nullptr;
  if (train) {
    h->step += 1;
    for (auto& v : h->attn_used) std::fill(v.begin(), v.end(), KmbDrop{0u, 0u, 1.f});   // what THIS training forward uses is recorded as it goes
    for (auto& v : h->act_used) std::fill(v.begin(), v.end(), KmbDrop{0u, 0u, 1.f});
    for (auto& hd : h->cls_used) for (KmbDrop& u : hd) u = KmbDrop{0u, 0u, 1.f};
  }
  const bool tr = train != 0;
  const float eps = h->cfg.layer_norm_eps;
  const float scale = h->cfg.scale_embedding ? sqrtf((float)d) : 1.f;
  HIPCHK(hipMemsetAsync(h->tl.status, 0, 16, s));

  // encoder once, unless the caller already holds its output (src/model/model.py:76-83)
  if (enc_in) HIPCHK(hipMemcpyAsync(h->tl.xe[h->cfg.encoder_layers], enc_in, (size_t)Me * d * esz(), hipMemcpyDeviceToDevice, s));
  else KCHK(encoder_forward(h, h->tl.encoder(), bt, tr, s));
  const bf16_t* enc = h->tl.xe[h->cfg.encoder_layers];
  if (enc_out) HIPCHK(hipMemcpyAsync(enc_out, enc, (size_t)Me * d * esz(), hipMemcpyDeviceToDevice, s));

  // ---- decoder (teacher forced): HF3.0.2 BartDecoder.forward via src/model/model.py:87-97
  KCHK(embed_ln_forward(bt.decoder_input_ids, nullptr, h->pf(h->shared), nullptr, h->pf(h->dec_pos),
                        h->cfg.extra_pos_embeddings, T, scale, h->pf(h->dec_lne_g), h->pf(h->dec_lne_b),
                        h->tl.zd0, h->tl.xd[0], h->tl.md0, h->tl.rd0, Md, d, eps, h->drop_site(2, tr), s));
  const int Ldec = h->cfg.decoder_layers;
  const int ldkv = Ldec * 2 * d;   // row stride of the batched cross-attention k | v buffers
  if (Ldec > 0) {   // every decoder layer's cross-attention keys | values in ONE GEMM (same input: the encoder output)
    KmbGemm g = lin_fwd(enc, d, h->wb(h->xkv_w), h->pf(h->xkv_b), Me, ldkv, d);
    g.out_bf16 = h->tl.ckv_all; g.ld_out_bf16 = ldkv;
    KCHK(run_gemm(g, s));
  }
  for (int l = 0; l < h->cfg.decoder_layers; ++l) {
    const LayerP& L = h->dec[l];
    DecAct& a = h->tl.da[l];
    KCHK(self_attn_forward(h, L.sa, h->Hd, h->tl.xd[l], a.qkv, a.o1, a.lse1, a.z1, a.m1, a.r1, a.y1, Bd, T,
                           bt.decoder_attention_mask, 1, h->drop_site(100 + 3 * l, tr), h->attn_drop_site(1, l, tr), s));
    // cross attention: q from decoder states (scaled), k|v from the encoder output
    KmbGemm g = lin_fwd(a.y1, d, h->wb(L.ca.qkv_w), h->pf(L.ca.qkv_b), Md, d, d);
    g.col_scale = 0.125f; g.col_scale_n = d; g.out_bf16 = a.cq; g.ld_out_bf16 = d;
    KCHK(run_gemm(g, s));
    // (an input's G targets are G * T contiguous query rows, cross-attention is not causal: ONE item of Tq = G * T per input)
    AttnIO io{a.cq, d, a.ckv, EP(a.ckv, d), ldkv, G * T, S, bt.attention_mask, 0};
    KCHK(attn_forward(h, io, B, h->Hd, a.o2, a.lse2, h->attn_drop_site(2, l, tr), s));
    const KmbDrop dr = h->drop_site(101 + 3 * l, tr);
    g = lin_fwd(a.o2, d, h->wb(L.ca.o_w), h->pf(L.ca.o_b), Md, d, d);
    g.drop_thr16 = dr.thr16; g.drop_seed = dr.seed; g.drop_scale = dr.scale;
    g.residual = a.y1; g.ld_res = d; g.out_bf16 = a.z2; g.ld_out_bf16 = d;
    KCHK(run_gemm(g, s));
    KCHK(ln_forward(a.z2, h->pf(L.ca.ln_g), h->pf(L.ca.ln_b), a.y2, a.m2, a.r2, Md, d, eps, s));
    KCHK(ffn_forward(h, L, h->Fd, a.y2, a.u, a.hh, a.z3, a.m3, a.r3, h->tl.xd[l + 1], Md, h->drop_site(102 + 3 * l, tr),
                     h->act_drop_site(1, l, tr), s));
  }
  const bf16_t* hdec = h->tl.xd[h->cfg.decoder_layers];
  h->have_hdec = true;
  if (opts && opts->decoder_states_out)   // MultiModalBartModel.forward returns the decoder states (src/model/model.py:100-103)
    HIPCHK(hipMemcpyAsync(opts->decoder_states_out, hdec, (size_t)Md * d * esz(), hipMemcpyDeviceToDevice, s));
  if (opts && opts->skip_head) return 0;

  // ---- tied LM head + CE (src/model/model.py:397-403)
  if (bt.labels) HIPCHK(kmb_count_valid_launch(bt.labels, Md, h->V, h->tl.count, h->tl.status, s));
  if (bt.labels || logits_out) KCHK(lm_head(h, hdec, bt.labels, extra ? extra->lm_factor : 1.f, need_grad != 0, loss_out, logits_out,
                                           row_weights, loss_reduction == 1, s));
  if (extra && need_grad && !bt.labels) {
    // no LM term (src/model/model.py:293-302 allows labels=None beside head labels): the decoder-state gradient and the
    // tied matrix's gradient start from zero; the heads add into the former, backward's embedding scatter-adds into the latter
    HIPCHK(hipMemsetAsync(h->tl.dhdec, 0, (size_t)Md * d * sizeof(bf16_t), s));
    HIPCHK(hipMemsetAsync(h->gf(h->shared), 0, (size_t)h->V * d * sizeof(float), s));
    h->head_wgrad_pending = false;
  }
  if (extra) {
    // ---- pre-training heads on the decoder states (src/model/model.py:248-289) and the weighted total (:304-307)
    const bool any = (extra->n_mrm > 0 && h->head[0].on) || (extra->n_attr > 0 && h->head[1].on) ||
                     (extra->n_rel > 0 && h->head[2].on);
    if (need_grad && any) HIPCHK(hipMemsetAsync(h->tl.dhead, 0, (size_t)Md * d * sizeof(float), s));
    HIPCHK(hipMemsetAsync(h->tl.losses5, 0, 8 * sizeof(float), s));
    if (bt.labels) HIPCHK(kmb_mean_rows_launch(h->tl.loss_dev, 1, extra->lm_factor, 1.f, h->tl.losses5 + 1, s));
    if (h->head[0].on)
      KCHK(head_run(h, 0, hdec, extra->n_mrm, extra->mrm_rows, nullptr, extra->mrm_targets, nullptr, extra->mrm_factor,
                    tr, need_grad != 0, h->tl.losses5 + 2, s));
    if (h->head[1].on)
      KCHK(head_run(h, 1, hdec, extra->n_attr, extra->attr_rows, nullptr, nullptr, extra->attr_labels,
                    extra->attr_factor, tr, need_grad != 0, h->tl.losses5 + 3, s));
    if (h->head[2].on)
      KCHK(head_run(h, 2, hdec, extra->n_rel, extra->rel_obj_rows, extra->rel_subj_rows, nullptr, extra->rel_labels,
                    extra->rel_factor, tr, need_grad != 0, h->tl.losses5 + 4, s));
    if (need_grad && any) HIPCHK(kmb_add_f32_into_bf16_launch(h->tl.dhdec, h->tl.dhead, (size_t)Md * d, s));
    HIPCHK(kmb_mean_rows_launch(h->tl.losses5 + 1, 4, 1.f, 1.f, h->tl.losses5, s));
    if (extra->losses_out)
      HIPCHK(hipMemcpyAsync(extra->losses_out, h->tl.losses5, 5 * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  h->have_fwd = need_grad != 0;
  return 0;
}

int kmb_forward(kmb_handle* h, const kmb_batch* batch, int train, int need_grad, float* loss_out, float* logits_out,
                kmb_bf16* enc_out, void* stream) {
  return forward_impl(h, batch, nullptr, nullptr, train, need_grad, loss_out, logits_out, enc_out, stream);
}

int kmb_forward_ex(kmb_handle* h, const kmb_batch* batch, const kmb_forward_opts* opts, int train, int need_grad,
                   float* loss_out, float* logits_out, kmb_bf16* enc_out, void* stream) {
  return forward_impl(h, batch, nullptr, opts, train, need_grad, loss_out, logits_out, enc_out, stream);
}

// Scores of a given target sequence (reference scripts/filter_reason.py:24-52: forward without labels, log_softmax over the [B, T, V]
// logits, the label's entry per token, the mean per sample): an eval-mode forward up to the decoder states, then a head that leaves
// no V-sized matrix.  Store-free path (1): the label's logit from 2 d values per row (ce_label_logit_kernel), ONE GEMM over the rows
// rounded up to whole 256-row tiles whose epilogue keeps per row and 64-column block (maximum, sum-exp) only (gemm_lean.hip LN_SCORE;
// the statistics live where the training head keeps its bf16 matrix), the row finish, the per-sample sums.  The tail rows [Md, Mpad) are
// whatever the workspace holds behind the decoder states: they are multiplied like ignored rows, their statistics land in rows of their own
// and nothing reads them.  Fallback (0; fewer than 256 rows, a vocabulary / width the persistent layout does not take, the fp32 validation
// mode, KMB_SCORE_FALLBACK=1): fp32 logits in row chunks that fit the existing logits scratch + ce_kernel_reg, whose loss_rows are the
// per-row values, then the same per-sample reduction.
int kmb_score(kmb_handle* h, const kmb_batch* batch, float* token_logprob, float* sample_nll, int32_t* sample_count, int32_t* path_out,
              void* stream) {
  if (!h) return fail("kmb_score: null handle");
  if (!batch || !batch->labels) return fail("kmb_score: labels are required (the sequence to score)");
  if (!token_logprob || !sample_nll || !sample_count) return fail("kmb_score: token_logprob, sample_nll and sample_count are required");
  kmb_forward_opts o{};
  o.skip_head = 1;
  KCHK(forward_impl(h, batch, nullptr, &o, 0, 0, nullptr, nullptr, nullptr, stream));
  hipStream_t s = (hipStream_t)stream;
  PrecisionScope scope(h);
  if (!h->fp32 && h->tl.small_floats > 1024) { g_small_slab = h->tl.small_slab; g_small_floats = h->tl.small_floats; }
  const kmb_batch& bt = *batch;
  const int d = h->d, B = bt.B, T = bt.T, Md = B * T;
  const bf16_t* hdec = h->tl.xd[h->cfg.decoder_layers];
  const bf16_t* Eb = h->wb(h->shared);
  HIPCHK(kmb_count_valid_launch(bt.labels, Md, h->V, h->tl.count, h->tl.status, s));
  const char* fb = getenv("KMB_SCORE_FALLBACK");   // read per call: tests flip it inside one process
  const bool forced = fb && fb[0] == '1';
  const int Mpad = (Md + 255) & ~255, nparts = h->Vpad / 64;
  const size_t head_bytes = (size_t)Md * h->Vpad * esz();   // the training head's matrix (dlogits_c): idle in an eval forward
  const bool in_ws = (const char*)hdec + (size_t)Mpad * d * sizeof(bf16_t) <= h->ws + h->ws_bytes;
  const bool store_free = !g_f32 && !forced && Md >= 256 && (h->Vpad % 256) == 0 && (d % 64) == 0 && d >= 320 &&
                          (long)(Mpad / 256) * (h->Vpad / 256) >= 128 && in_ws && (size_t)Mpad * nparts * 2 * sizeof(float) <= head_bytes;
  if (path_out) *path_out = store_free ? 1 : 0;
  if (store_free) {
    float* stats = reinterpret_cast<float*>(h->tl.dlogits_c);
    KmbGemm g;
    KCHK(head_padded_setup(h, hdec, bt.labels, Md, Mpad, &g, s));
    if (const char* why = kmb_gemm_score_check(g, stats)) return fail("kmb_score: %s", why);
    HIPCHK(kmb_gemm_score_launch(g, stats, s));
    HIPCHK(kmb_score_rows_finish_launch(stats, nparts, h->tl.ce_shift, bt.labels, Md, h->V, token_logprob, s));
    HIPCHK(kmb_score_segments_launch(token_logprob, 0, bt.labels, B, T, h->V, token_logprob, sample_nll, sample_count, s));
    return 0;
  }
  // fallback: the larger of the two head scratch buffers holds the fp32 logits of a row chunk
  float* buf = h->tl.logits_c;
  size_t cap = h->tl.logits_c_floats;
  if (head_bytes / sizeof(float) > cap) { buf = reinterpret_cast<float*>(h->tl.dlogits_c); cap = head_bytes / sizeof(float); }
  const size_t fit = cap / (size_t)h->Vpad;
  if (fit >= 1) {
    int CH = Md < h->lm_chunk ? Md : h->lm_chunk;
    if ((size_t)CH > fit) CH = (int)fit;
    for (int r0 = 0; r0 < Md; r0 += CH) {
      const int rows = (Md - r0) < CH ? (Md - r0) : CH;
      KmbGemm g = lin_fwd(EP(hdec, (size_t)r0 * d), d, Eb, h->flb, rows, h->V, d);
      g.out_f32 = buf; g.ld_out_f32 = h->Vpad;
      KCHK(run_vocab_gemm(g, s));
      HIPCHK(kmb_ce_launch(buf, h->Vpad, h->V, bt.labels + r0, rows, h->tl.count, 1.f, h->tl.loss_rows + r0, nullptr, s));
    }
  } else {   // (a single decoder row of a wide vocabulary: the bf16 head's matrix is all there is room for)
    if (g_f32) return fail("kmb_score: the logits scratch does not hold one fp32 row");
    KmbGemm g = lin_fwd(hdec, d, Eb, h->flb, Md, h->V, d);
    g.out_bf16 = h->tl.dlogits_c; g.ld_out_bf16 = h->Vpad;
    KCHK(run_gemm(g, s));
    HIPCHK(kmb_ce_bf16_launch(h->tl.dlogits_c, h->Vpad, h->V, bt.labels, Md, h->tl.count, 1.f, h->tl.loss_rows, nullptr, s));
  }
  HIPCHK(kmb_score_segments_launch(h->tl.loss_rows, 1, bt.labels, B, T, h->V, token_logprob, sample_nll, sample_count, s));
  return 0;
}

int kmb_hidden_state(kmb_handle* h, int which, int index, kmb_bf16* out, void* stream) {
  if (!h->have_hdec) return fail("kmb_hidden_state: no forward whose activations are still in the workspace");
  if (h->fp32) return fail("kmb_hidden_state: not available in the fp32 validation mode");
  const auto& xs = which == 0 ? h->tl.xe : h->tl.xd;
  if ((which != 0 && which != 1) || index < 0 || index >= (int)xs.size() || !xs[index]) return fail("kmb_hidden_state: index out of range");
  const size_t rows = which == 0 ? (size_t)h->Me : (size_t)h->Md;
  HIPCHK(hipMemcpyAsync(out, xs[index], rows * h->d * sizeof(bf16_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

// dL / d(encoder states) of the last kmb_backward as bf16 [B * S, d_model]: the sum of every decoder layer's cross-attention key /
// value data gradients, i.e. what the encoder's backward starts from (and all there is when the forward was given its states)
int kmb_encoder_states_grad(kmb_handle* h, kmb_bf16* out, void* stream) {
  if (!h || !out) return fail("kmb_encoder_states_grad: handle and out are required");
  if (!h->have_bwd) return fail("kmb_encoder_states_grad: run kmb_backward first");
  HIPCHK(hipMemcpyAsync(out, h->tl.denc, (size_t)h->Me * h->d * sizeof(bf16_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

int kmb_attention_probs(kmb_handle* h, int which, int layer, float* out, void* stream) {
  if (!h->have_hdec) return fail("kmb_attention_probs: no forward whose activations are still in the workspace");
  if (h->fp32) return fail("kmb_attention_probs: not available in the fp32 validation mode");
  if (h->tpi > 1) return fail("kmb_attention_probs: not available after a forward with targets_per_input > 1");
  const int d = h->d, B = h->bt.B;
  if (which == 0) {
    if (layer < 0 || layer >= (int)h->tl.ea.size()) return fail("kmb_attention_probs: layer out of range");
    const EncAct& a = h->tl.ea[layer];
    HIPCHK(kmb_attn_probs_launch(a.qkv, 3 * d, EP(a.qkv, d), 3 * d, a.lse, h->bt.attention_mask, 0, B, h->He, h->bt.S, h->bt.S, out,
                                 (hipStream_t)stream));
  } else if (which == 1) {
    if (layer < 0 || layer >= (int)h->tl.da.size()) return fail("kmb_attention_probs: layer out of range");
    const DecAct& a = h->tl.da[layer];
    HIPCHK(kmb_attn_probs_launch(a.qkv, 3 * d, EP(a.qkv, d), 3 * d, a.lse1, h->bt.decoder_attention_mask, 1, B, h->Hd, h->bt.T, h->bt.T,
                                 out, (hipStream_t)stream));
  } else {
    return fail("kmb_attention_probs: which must be 0 (encoder) or 1 (decoder)");
  }
  return 0;
}

// logits of the LAST forward's decoder states (outputs[1] of a training forward, src/model/model.py:397-405) without
// re-running the model: one head GEMM on the states still in the workspace
int kmb_last_logits(kmb_handle* h, float* logits_out, void* stream) {
  KCHK(check_bound(h));
  if (!h->have_hdec || h->Md <= 0) return fail("kmb_last_logits: no forward whose decoder states are still in the workspace");
  if (!logits_out) return fail("kmb_last_logits: logits_out is required");
  PrecisionScope scope(h);
  return head_logits(h, h->tl.xd[h->cfg.decoder_layers], h->Md, logits_out, (hipStream_t)stream);
}

int kmb_forward_pretrain(kmb_handle* h, const kmb_batch* batch, const kmb_pretrain* extra, int train, int need_grad,
                         float* logits_out, kmb_bf16* enc_out, void* stream) {
  if (!extra) return fail("kmb_forward_pretrain: extra is required");
  if ((extra->n_mrm > 0 && !h->head[0].on) || (extra->n_attr > 0 && !h->head[1].on) || (extra->n_rel > 0 && !h->head[2].on))
    return fail("kmb_forward_pretrain: rows given for a head this model was built without (num_labels / num_attributes / num_relations)");
  return forward_impl(h, batch, extra, nullptr, train, need_grad, nullptr, logits_out, enc_out, stream);
}

int kmb_forward_pretrain_ex(kmb_handle* h, const kmb_batch* batch, const kmb_pretrain* extra, const kmb_forward_opts* opts,
                            int train, int need_grad, float* logits_out, kmb_bf16* enc_out, void* stream) {
  if (!extra) return fail("kmb_forward_pretrain_ex: extra is required");
  if (opts && opts->skip_head) return fail("kmb_forward_pretrain_ex: skip_head does not apply to the pre-training forward");
  if ((extra->n_mrm > 0 && !h->head[0].on) || (extra->n_attr > 0 && !h->head[1].on) || (extra->n_rel > 0 && !h->head[2].on))
    return fail("kmb_forward_pretrain_ex: rows given for a head this model was built without (num_labels / num_attributes / num_relations)");
  return forward_impl(h, batch, extra, opts, train, need_grad, nullptr, logits_out, enc_out, stream);
}

// --------------------------------------------------------------------------------- backward
static int backward_impl(kmb_handle* h, float loss_scale, const float* loss_scale_dev, void* stream);
int kmb_backward(kmb_handle* h, float loss_scale, void* stream) { return backward_impl(h, loss_scale, nullptr, stream); }
int kmb_backward_dev(kmb_handle* h, const float* loss_scale_dev, void* stream) {
  if (!loss_scale_dev) return fail("kmb_backward_dev: loss_scale_dev is required");
  return backward_impl(h, 1.f, loss_scale_dev, stream);
}

static int backward_impl(kmb_handle* h, float loss_scale, const float* loss_scale_dev, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  KCHK(check_bound(h));
  PrecisionScope scope(h);
  if (h->tl.small_floats > 1024) { g_small_slab = h->tl.small_slab; g_small_floats = h->tl.small_floats; }
  if (!h->have_fwd) return fail("kmb_backward: no forward with need_grad=1 to differentiate");
  h->have_fwd = false;
  h->have_bwd = true;
  // grouped weight gradients (wgrad_flush) for short token reductions; KMB_WGRAD_GROUP=0: every weight gradient its own
  // (split-K) launch, as for long ones
  struct GroupScope {
    kmb_handle* h;
    ~GroupScope() { h->wg_group = false; h->wg_pending.clear(); }
  } group_scope{h};
  {
    static const bool group_ok = !(getenv("KMB_WGRAD_GROUP") && getenv("KMB_WGRAD_GROUP")[0] == '0');
    static const int group_tokens = KMB_DIAG_ENV("KMB_WGRAD_GROUP_TOKENS") ? atoi(KMB_DIAG_ENV("KMB_WGRAD_GROUP_TOKENS")) : 3072;   // <= 48 samples x 64 tokens
    h->wg_group = group_ok && !h->fp32 && (h->Me > h->Md ? h->Me : h->Md) <= group_tokens;
    h->wg_pending.clear();
  }
  const kmb_batch& bt = h->bt;
  const int d = h->d, B = bt.B, S = bt.S, T = bt.T, G = h->tpi, Bd = B * G, Me = h->Me, Md = h->Md;
  const bool tr = h->fwd_train;
  const float scale = h->cfg.scale_embedding ? sqrtf((float)d) : 1.f;
  const int Le = h->cfg.encoder_layers, Ld = h->cfg.decoder_layers;
  for (auto& e : h->events)
    if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  KCHK(ensure_side(h));
  const bool side = h->side_on && h->side != nullptr;
  if (KMB_DIAG_ENV("KMB_PRINT_LAYOUT")) print_layout(h, h->tl);
  int ev = 0;
  // layer c may only start once the side stream has finished layer c-2 (it still reads that layer's gradient buffers)
  auto layer_begin = [&](int c) -> int {
    if (side && c >= 2) HIPCHK(hipStreamWaitEvent(s, h->layer_done[c - 2], 0));
    return 0;
  };
  // the bucket of layer c is complete when BOTH streams are past this point: record its event on the side stream
  // behind a marker of the main stream, so the main stream never waits here
  // (c < 0: a bucket that is no layer's -- the decoder embedding's)
  // Gradient accumulation: this backward's writers fill the stage (kmb_handle::gf); a bucket's fold into G goes out on the stream that
  // records the bucket's event, right in front of it and behind both streams' writers, exactly as the event is.  The event then
  // means "the ACCUMULATED gradient of this bucket is complete".  The first backward after kmb_zero_grad overwrites G without reading it.
  // The next micro-step's writers are ordered behind these folds: every backward ends with the caller's stream behind the side stream,
  // and the side stream's work always starts behind a marker of the caller's stream (wgrad_side, wgrad_flush, reducer_stream).
  const bool accum = h->accum, fold_add = accum && !h->grad_fresh;
  if (accum) h->grad_fresh = false;
  auto fold_bucket = [&](int bucket, hipStream_t fs) -> int {
    if (!accum) return 0;
    const Bucket& bk = h->buckets[bucket];
    HIPCHK(kmb_grad_fold_launch(h->G + bk.off, h->GS + bk.off, bk.count, fold_add ? 1 : 0, fs));
    return 0;
  };
  auto layer_end = [&](int c, int bucket) -> int {
    KCHK(wgrad_flush(h, s));   // the layer's parked weight gradients go out as one launch (grouped path)
    if (!side) { KCHK(fold_bucket(bucket, s)); HIPCHK(hipEventRecord(h->events[bucket], s)); return 0; }
    KCHK(order_behind(h, s, h->side));
    if (accum && c >= 0) HIPCHK(hipEventRecord(h->layer_done[c], h->side));   // (the fold reads none of the layer's gradient buffers)
    KCHK(fold_bucket(bucket, h->side));
    HIPCHK(hipEventRecord(h->events[bucket], h->side));
    if (!accum && c >= 0) HIPCHK(hipEventRecord(h->layer_done[c], h->side));
    return 0;
  };
  const bool scaled = loss_scale != 1.f || loss_scale_dev != nullptr;
  if (scaled) {
    HIPCHK(kmb_scale_bf16_launch(h->tl.dhdec, (size_t)Md * d, loss_scale, loss_scale_dev, s));
    if (h->head_wgrad_pending) {
      // the tied matrix's head gradient is being written on the side stream: scale it there, behind the GEMM, and move
      // the completion event behind the scaling (the main stream keeps running ahead).  The device scalar was written
      // by the caller on the MAIN stream (autograd's grad_out, GradScaler's scale): the side stream must not read it
      // before the main stream got that far -- it was last ordered behind main in the middle of forward.
      if (loss_scale_dev) KCHK(order_behind(h, s, h->side));
      HIPCHK(kmb_scale_f32_launch(h->gf(h->shared), (size_t)h->V * d, loss_scale, loss_scale_dev, h->side));
      HIPCHK(hipEventRecord(h->head_wgrad_done, h->side));
    } else {
      HIPCHK(kmb_scale_f32_launch(h->gf(h->shared), (size_t)h->V * d, loss_scale, loss_scale_dev, s));
    }
    // the pre-training heads' parameter gradients were written by forward (head_run) at scale 1
    if (h->heads_end > h->heads_begin)
      HIPCHK(kmb_scale_f32_launch(h->gf(h->heads_begin), h->heads_end - h->heads_begin, loss_scale, loss_scale_dev, s));
  }
  const bf16_t* enc = h->tl.xe[Le];
  const bf16_t* dy = h->tl.dhdec;
  bf16_t* pp[2] = {h->tl.dyA, h->tl.dyB};
  int cur = 0, c = 0;
  bool denc_init = false;
  // ---- decoder layers
  for (int l = Ld - 1; l >= 0; --l, ++c) {
    const LayerP& L = h->dec[l];
    DecAct& a = h->tl.da[l];
    BwdBufs& bb = h->tl.bb[c & 1];
    KCHK(layer_begin(c));
    g_trace_layer = 100 + l;
    bf16_t* t0 = pp[cur]; bf16_t* t1 = pp[cur ^ 1];
    KCHK(ffn_backward(h, L, h->Fd, a.y2, a.u, a.hh, a.z3, a.m3, a.r3, dy, t0, Md, h->drop_site(102 + 3 * l, tr), bb, s));
    {  // cross-attention block: y2 = LN(z2), z2 = y1 + drop(out_proj(attn(cq, ckv)))
      const KmbDrop dr = h->drop_site(101 + 3 * l, tr);
      bf16_t* dz = bb.dz[2];
      bf16_t* dsub = dr.thr16 ? bb.dsub[2] : dz;
      KCHK(ln_backward(h, t0, a.z2, a.m2, a.r2, L.ca.ln_g, L.ca.ln_b, dz, dr.thr16 ? dsub : nullptr,
                       KmbDrop{0u, 0u, 1.f}, dr, Md, s, L.ca.o_b, bb.parts[4]));
      KCHK(trace("ca.dz", dz, (size_t)Md * d * 2, s));
      KCHK(wgrad_side(h, lin_wgrad(dsub, d, a.o2, d, h->gf(L.ca.o_w), Md, d, d, 0.f), s));
      KmbGemm g = lin_dgrad(dsub, d, h->wb(L.ca.o_w), Md, d, d);
      g.out_bf16 = h->tl.dob; g.ld_out_bf16 = d;
      KCHK(run_gemm(g, s));
      const int ldkv = Ld * 2 * d;
      bf16_t* dkv = h->tl.dckv_all + (size_t)l * 2 * d;   // this layer's columns of the batched k | v gradient
      AttnIO io{a.cq, d, a.ckv, a.ckv + d, ldkv, G * T, S, bt.attention_mask, 0};   // dK | dV: summed over the input's G targets in the kernel
      KCHK(attn_backward(h, io, B, h->Hd, a.o2, a.lse2, h->tl.dob, bb.dcq, d, dkv, dkv + d, ldkv, bb.parts[5],
                         bb.parts[5] + d, bb.parts[5] + 2 * d, 3 * d, h->attn_drop_used(2, l, tr), s));
      // bias gradients from the attention kernel's per-batch-item column sums [B][q | k | v]: q's bias lives in the layer,
      // the k | v biases of all layers together (kmb_handle::xkv_b)
      HIPCHK(kmb_reduce_parts2_launch(bb.parts[5], B, 3 * d, h->gf(L.ca.qkv_b), d, h->gf(L.ca_kv_b), 2 * d, reducer_stream(h, s)));
      KCHK(trace("ca.dob", h->tl.dob, (size_t)Md * d * 2, s));
      KCHK(trace("ca.dcq", bb.dcq, (size_t)Md * d * 2, s));
      KCHK(wgrad_side(h, lin_wgrad(bb.dcq, d, a.y1, d, h->gf(L.ca.qkv_w), Md, d, d, 0.f), s));
      g = lin_dgrad(bb.dcq, d, h->wb(L.ca.qkv_w), Md, d, d);
      g.residual = dz; g.ld_res = d; g.out_bf16 = t1; g.ld_out_bf16 = d;
      KCHK(run_gemm(g, s));
      KCHK(trace("ca.t1", t1, (size_t)Md * d * 2, s));
    }
    KCHK(self_attn_backward(h, L.sa, h->Hd, h->tl.xd[l], a.qkv, a.o1, a.lse1, a.z1, a.m1, a.r1, t1, t0, Bd, T,
                            bt.decoder_attention_mask, 1, h->drop_site(100 + 3 * l, tr), h->attn_drop_used(1, l, tr), bb, s));
    dy = t0;  // t0 now holds d(loss)/d(xd[l]); keep it as the input of the next iteration
    cur ^= 1;  // next iteration writes its first result into the other buffer
    KCHK(layer_end(c, ev++));
  }
  // ---- cross-attention keys | values of ALL decoder layers: one data gradient (the encoder output's gradient, reduction
  // over Ld * 2d) and one weight gradient
  if (Ld > 0) {
    const int ldkv = Ld * 2 * d;
    KCHK(trace("ca.dckv_all", h->tl.dckv_all, (size_t)Me * ldkv * 2, s));
    KCHK(wgrad_side(h, lin_wgrad(h->tl.dckv_all, ldkv, enc, d, h->gf(h->xkv_w), Me, ldkv, d, 0.f), s));
    KmbGemm g = lin_dgrad(h->tl.dckv_all, ldkv, h->wb(h->xkv_w), Me, ldkv, d);
    g.out_bf16 = h->tl.denc; g.ld_out_bf16 = d;
    KCHK(run_gemm(g, s));
    KCHK(trace("ca.denc", h->tl.denc, (size_t)Me * d * 2, s));
    denc_init = true;
  }
  // ---- decoder embedding: xd[0] = drop(LN(zd0))  (main stream only)
  KCHK(ln_backward(h, dy, h->tl.zd0, h->tl.md0, h->tl.rd0, h->dec_lne_g, h->dec_lne_b, h->tl.dz, nullptr, h->drop_site(2, tr),
                   KmbDrop{0u, 0u, 1.f}, Md, s));
  if (h->head_wgrad_pending) {
    HIPCHK(hipStreamWaitEvent(s, h->head_wgrad_done, 0));
    h->head_wgrad_pending = false;
  }
  HIPCHK(kmb_embed_bwd_launch(h->tl.dz, bt.decoder_input_ids, nullptr, scale, h->gf(h->shared), nullptr,
                              h->cfg.pad_token_id, Md, d, s));
  HIPCHK(kmb_pos_bwd_launch(h->tl.dz, Bd, T, d, h->gf(h->dec_pos), h->cfg.extra_pos_embeddings, h->Prows, s));
  // this bucket also holds the cross-attention k | v weights and biases of every decoder layer, whose gradients come from
  // the side stream (the batched weight gradient above, the per-layer bias reducers): complete when BOTH streams are here
  KCHK(layer_end(-1, ev++));
  // ---- encoder layers
  if (!denc_init) HIPCHK(hipMemsetAsync(h->tl.denc, 0, (size_t)Me * d * sizeof(bf16_t), s));
  if (h->enc_given) {
    // The forward started from the caller's encoder states: the gradient stops at them (h->tl.denc, kmb_encoder_states_grad).
    // The encoder's parameters took no part: their buckets are zero, complete here (the tied matrix keeps the decoder side's
    // contributions: the head's weight gradient and the decoder embedding's scatter-add above).
    for (int l = Le - 1; l >= 0; --l, ++ev) {
      HIPCHK(hipMemsetAsync(h->gf(h->buckets[ev].off), 0, h->buckets[ev].count * sizeof(float), s));
      KCHK(fold_bucket(ev, s));
      HIPCHK(hipEventRecord(h->events[ev], s));
    }
    HIPCHK(hipMemsetAsync(h->gf(h->buckets[ev].off), 0, h->buckets[ev].count * sizeof(float), s));
    if (side) KCHK(order_behind(h, h->side, s));
    KCHK(fold_bucket(ev, s));
    HIPCHK(hipEventRecord(h->events[ev++], s));
    KCHK(fold_bucket(ev, s));
    HIPCHK(hipEventRecord(h->events[ev++], s));
    return 0;
  }
  dy = h->tl.denc;
  cur = 0;
  for (int l = Le - 1; l >= 0; --l, ++c) {
    const LayerP& L = h->enc[l];
    EncAct& a = h->tl.ea[l];
    BwdBufs& bb = h->tl.bb[c & 1];
    KCHK(layer_begin(c));
    g_trace_layer = l;
    bf16_t* t0 = pp[cur]; bf16_t* t1 = pp[cur ^ 1];
    KCHK(ffn_backward(h, L, h->Fe, a.y1, a.u, a.hh, a.z2, a.m2, a.r2, dy, t0, Me, h->drop_site(11 + 2 * l, tr), bb, s));
    KCHK(self_attn_backward(h, L.sa, h->He, h->tl.xe[l], a.qkv, a.o, a.lse, a.z1, a.m1, a.r1, t0, t1, B, S,
                            bt.attention_mask, 0, h->drop_site(10 + 2 * l, tr), h->attn_drop_used(0, l, tr), bb, s));
    dy = t1;  // t0 / t1 keep their roles: the next ffn_backward reads t1 and writes t0
    KCHK(layer_end(c, ev++));
  }
  // ---- encoder embedding (+ image projection, src/model/modules.py:24-41)
  KCHK(ln_backward(h, dy, h->tl.ze0, h->tl.me0, h->tl.re0, h->enc_lne_g, h->enc_lne_b, h->tl.dz, nullptr, h->drop_site(1, tr),
                   KmbDrop{0u, 0u, 1.f}, Me, s));
  HIPCHK(kmb_embed_bwd_launch(h->tl.dz, bt.input_ids, h->tl.img_src, scale, h->gf(h->shared), h->tl.dimg, h->cfg.pad_token_id,
                              Me, d, s));
  HIPCHK(kmb_pos_bwd_launch(h->tl.dz, B, S, d, h->gf(h->enc_pos), h->cfg.extra_pos_embeddings, h->Prows, s));
  if (h->Ntot > 0) {
    KCHK(bias_grad(h, h->tl.dimg, d, h->Ntot, d, h->gf(h->img_b), s));
    KCHK(wgrad_side(h, lin_wgrad(h->tl.dimg, d, h->tl.xf, h->Fpad, h->gf(h->img_w), h->Ntot, d, h->Fin, 0.f), s));  // shares the slab
  } else {
    HIPCHK(hipMemsetAsync(h->gf(h->img_w), 0, ((size_t)d * h->Fin) * sizeof(float), s));
    HIPCHK(hipMemsetAsync(h->gf(h->img_b), 0, (size_t)d * sizeof(float), s));
  }
  KCHK(wgrad_flush(h, s));
  if (side) KCHK(order_behind(h, h->side, s));  // everything the optimizer reads must be ordered behind the side stream's last weight gradient
  KCHK(fold_bucket(ev, s));
  HIPCHK(hipEventRecord(h->events[ev++], s));
  KCHK(fold_bucket(ev, s));
  HIPCHK(hipEventRecord(h->events[ev++], s));  // tied matrix: complete once the encoder-side scatter-add is in
  return 0;
}

}  // extern "C"
